"""scoreSplitWide's tile loop (rasr_amd/csrc/gmm_kernels_split.hip): diagonal-maximum at D = 39, pooled covariance,
against oracle.OracleFloat with the float contract of tests/test_gpu_parity.py (1e-4 relative; a different best
density only where the oracle's score of the returned density is within the same tolerance).

The shapes are the ways the loop can go wrong: whole mixtures of equal length, a partial last frame tile, one-tile
mixtures (an emit after every step), chunks shorter than the prefetch depth of 3 tiles and of exactly 3, 4, 6 and 7
tiles (the remainders of the loop's unroll by 6), mixtures without densities, and scores only.

The chunking is read from RASR_GMM_TARGET_BLOCKS once per process, so the GPU side of every case runs in two child
processes: the default (small models: one mixture per chunk, the prologue then straight into the tail) and 4 target
blocks (chunks of many mixtures).  No scorer option selects the 128-frame scoreSplit at these K steps (the choice
between the two is a build switch), so the oracle comparison stands alone.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import rasr_amd as ra

from test_gpu_parity import _check_float

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 39
# densities per mixture: 1, 1, 2, 10, 1, 3, 4, 6, 7, ... tiles of 16
RAGGED = [1, 16, 17, 160, 3, 48, 64, 96, 112, 5, 100, 2, 33, 80, 16, 1, 1, 20, 49, 128,
          7, 150, 15, 31, 65, 97, 113, 9, 48, 64, 96, 112, 1, 17, 160, 3, 40, 8, 24, 1]


def _with_empty():
    """Mixtures without densities at a chunk's start, between two mixtures (twice in a row) and at the end."""
    rng = np.random.Generator(np.random.PCG64(17))
    groups = [0, 20, 0, 0, 33, 16, 0, 1, 48, 0]
    n = sum(groups)
    means = rng.standard_normal((n, D), dtype=np.float32)
    var = (0.5 + np.abs(rng.standard_normal((1, D), dtype=np.float32))).astype(np.float32)
    offs = np.cumsum([0] + groups).astype(np.uint32)
    logw = np.concatenate([np.full(g, -np.log(max(g, 1))) for g in groups])
    return ra.MixtureSet(means, var, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32), offs,
                         np.arange(n, dtype=np.uint32), logw)


def _models():
    m = {"uniform": ra.synthetic_mixture_set(24, 160, D, seed=31, weights="random"),
         "ragged": ra.synthetic_mixture_set(len(RAGGED), RAGGED, D, seed=32, weights="random"),
         "empty": _with_empty()}
    for tiles in (1, 2, 3, 4, 6, 7):  # one mixture per chunk by default: chunks of exactly that many tiles
        m[f"tiles{tiles}"] = ra.synthetic_mixture_set(8, 16 * tiles - 3, D, seed=40 + tiles, weights="random")
    return m


# case -> (model, frames, with best densities)
CASES = {"uniform-512": ("uniform", 512, True), "uniform-300": ("uniform", 300, True),
         "ragged": ("ragged", 200, True), "ragged-scores": ("ragged", 200, False), "empty": ("empty", 70, True)}
CASES.update({f"tiles{t}": (f"tiles{t}", 64, True) for t in (1, 2, 3, 4, 6, 7)})
ENVS = {"default": None, "few-chunks": "4"}


def _frames(case):
    return ra.synthetic_frames(CASES[case][1], D, seed=13)


def _run_cases(out):
    """Child process: every case through the wide kernel."""
    models, res = _models(), {}
    for case, (model, _, best) in CASES.items():
        frames = _frames(case)
        sc = ra.Scorer(models[model], "diagonal-maximum", max_frames=len(frames))
        assert sc.main_kernel() == "scoreSplitWide"
        s, b = sc.score_host(frames, want_best=best)
        res[case + ".s"] = s
        if best:
            res[case + ".b"] = b
    np.savez(out, **res)


@pytest.fixture(scope="module")
def gpu_results(gpu, tmp_path_factory):
    res = {}
    for name, blocks in ENVS.items():
        out = str(tmp_path_factory.mktemp("wide") / f"{name}.npz")
        env = dict(os.environ)
        env.pop("RASR_GMM_TARGET_BLOCKS", None)
        if blocks:
            env["RASR_GMM_TARGET_BLOCKS"] = blocks
        code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; "
                f"import test_split_wide_step as t; t._run_cases({out!r})")
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        res[name] = dict(np.load(out))
    return res


@pytest.fixture(scope="module")
def references():
    models, ref = _models(), {}
    for case, (model, _, _) in CASES.items():
        ref[case] = (models[model], _frames(case)) + tuple(oracle.OracleFloat(models[model]).score(_frames(case), n_threads=8))
    return ref


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("case", list(CASES))
def test_wide_against_oracle(gpu_results, references, env, case):
    ms, frames, ref_s, ref_b = references[case]
    s, b = gpu_results[env][case + ".s"], gpu_results[env].get(case + ".b")
    err = np.abs(s.astype(np.float64) - ref_s) / np.maximum(1.0, np.abs(ref_s.astype(np.float64)))
    print(f"{env} {case}: max rel err {np.nanmax(err):.3e}, best densities differing "
          f"{0 if b is None else int((b != ref_b).sum())}")
    empty = np.diff(ms.mixture_offsets.astype(np.int64)) == 0
    assert np.array_equal(s[empty], ref_s[empty])  # no density: 0.5 * FLT_MAX, density 0xffffffff
    if b is not None:
        assert np.array_equal(b[empty], ref_b[empty])
    for e in np.flatnonzero(~empty):  # _check_float takes rows of one mixture offset
        _check_float(s[e:e + 1], None if b is None else b[e:e + 1], ref_s[e:e + 1], ref_b[e:e + 1], ms, frames, None,
                     mixture_offset=int(e))

