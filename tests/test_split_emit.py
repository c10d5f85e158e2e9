"""The per-mixture emit of the float split-f16 kernels (scoreSplitWide, scoreSplit, scoreSplit32): the key-only
cross-lane reduce, the select-free finalize with its one rare branch, and scoreSplitWide's four-frames-per-lane
stores, against oracle.OracleFloat under the float rule of tests/test_gpu_parity.py (scores within 1e-4 relative, a
different best density only on a near tie of the two densities' float64 scores)."""
import numpy as np
import pytest

import oracle
import rasr_amd as ra

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4  # tests/test_gpu_parity.py


def _assert_close(gpu, ref):
    """|gpu - ref| <= REL_TOL * max(1, |ref|); bit-equal values (the FLT_MAX-class scores of mixtures without a finite
    candidate, infinities) have no error."""
    g, r = gpu.astype(np.float64), ref.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(g - r) / np.maximum(1.0, np.abs(r))
    err[gpu.view(np.uint32) == ref.view(np.uint32)] = 0.0
    assert gpu.shape == ref.shape and not np.isnan(err).any() and err.max(initial=0.0) <= REL_TOL, \
        f"max rel err {err.max(initial=0.0)}, {int(np.isnan(err).sum())} undefined"


def _f64_density_score(ms, e, j, x):
    i = int(ms.mixture_offsets[e]) + int(j)
    d = int(ms.mixture_densities[i])
    var = ms.variances[int(ms.density_covariance[d])].astype(np.float64)
    m = ms.means[int(ms.density_mean[d])].astype(np.float64)
    ln = len(var) * np.log(2 * np.pi) + np.log(var).sum()
    return 0.5 * (-2 * ms.mixture_log_weights[i] + ln + (((m - x) ** 2) / var).sum())


def _check_float(gpu_s, gpu_b, ref_s, ref_b, ms, frames):
    _assert_close(gpu_s, ref_s)
    assert gpu_b.shape == ref_b.shape
    for e, t in np.argwhere(gpu_b != ref_b):
        n = int(ms.mixture_offsets[e + 1] - ms.mixture_offsets[e])
        assert gpu_b[e, t] < n and ref_b[e, t] < n, f"mixture {e} frame {t}: {gpu_b[e, t]} vs {ref_b[e, t]}"
        x = frames[t].astype(np.float64)
        a, b = _f64_density_score(ms, e, gpu_b[e, t], x), _f64_density_score(ms, e, ref_b[e, t], x)
        assert abs(a - b) <= REL_TOL * max(1.0, abs(b)), f"mixture {e} frame {t}: {gpu_b[e, t]} vs {ref_b[e, t]}"


COUNTS = [0, 1, 16, 17, 0, 160, 0, 0, 16, 17, 1, 0]  # every kind also first and last of a chunk


@pytest.fixture(scope="module")
def pooled39():
    ms = ra.synthetic_mixture_set(len(COUNTS), COUNTS, 39, seed=61, weights="random")
    frames = ra.synthetic_frames(300, 39, seed=62)
    ref_s, ref_b = oracle.OracleFloat(ms).score(frames, n_threads=8)
    return ms, frames, ref_s, ref_b


@pytest.mark.parametrize("n", [1, 17, 255, 256, 257, 300])
def test_smallest_shapes(gpu, pooled39, n):
    """A partial last wave and a partial four-frame store group at the frame bound; empty, one-tile and many-tile
    mixtures."""
    ms, frames, ref_s, ref_b = pooled39
    s, b = ra.Scorer(ms, "diagonal-maximum", max_frames=n).score_host(frames[:n])
    assert s.shape == (len(COUNTS), n)
    _check_float(s, b, ref_s[:, :n], ref_b[:, :n], ms, frames)
    empty = [i for i, c in enumerate(COUNTS) if c == 0]
    assert (b[empty] == 0xFFFFFFFF).all() and np.array_equal(s[empty], ref_s[empty, :n])


@pytest.mark.parametrize("d", [39, 80])
def test_exact_ties_across_lane_groups(gpu, d):
    """Copies of one density in rows 4 g + r of different lane groups g (same slot r: equal keys) and in a later
    tile: the lowest density index wins, whichever groups hold the copies.  D = 39: scoreSplitWide and scoreSplit32,
    D = 80: scoreSplit."""
    n = 40
    rng = np.random.Generator(np.random.PCG64(63))
    means = rng.standard_normal((n, d), dtype=np.float32)
    # rows 4 g + r of 16-row tiles: groups {1, 2}; groups {1, 2, 3} and tile 1; tile 1 groups {0, 2, 3}; all groups
    # and tile 2
    copies = {6: [6, 10], 5: [5, 9, 13, 21], 18: [18, 26, 30], 3: [3, 7, 11, 15, 35]}
    for first, rows in copies.items():
        means[rows] = means[first]
    var = (0.5 + np.abs(rng.standard_normal((1, d), dtype=np.float32))).astype(np.float32)
    ms = ra.MixtureSet(means, var, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32), np.array([0, n], np.uint32),
                       np.arange(n, dtype=np.uint32), np.full(n, -np.log(n)))
    centres = np.array(list(copies))[rng.integers(0, len(copies), 257)]
    frames = (means[centres] + 0.05 * rng.standard_normal((257, d), dtype=np.float32)).astype(np.float32)
    ref_s, ref_b = oracle.OracleFloat(ms).score(frames)
    lowest = np.full(n, -1)
    for first, rows in copies.items():
        lowest[rows] = first
    dup = lowest[ref_b[0]] >= 0  # the oracle's winner is a duplicated density (any of its copies)
    assert dup.mean() > 0.9
    for kopts in ({}, {"split_tile16": True}, {"split_tile32": True}) if d == 39 else ({},):
        s, b = ra.Scorer(ms, "diagonal-maximum", max_frames=257, **kopts).score_host(frames)
        _check_float(s, b, ref_s, ref_b, ms, frames)  # every frame: the near-tie rule
        assert np.array_equal(b[0, dup], lowest[ref_b[0, dup]]), kopts


@pytest.mark.parametrize("kind", ["diagonal-maximum", "batch-diagonal-maximum-float"])
def test_non_finite_frames(gpu, kind):
    """NaN, infinite and 1e12 frames: no finite candidate, and batch-float's overflowed total.  On a NaN frame the
    batch-float reference propagates the NaN into its score, where the scorer reports a mixture without a finite
    candidate: there the scorer's own rule is asserted, FLT_MAX bit for bit for every mixture."""
    ms = ra.synthetic_mixture_set(len(COUNTS), COUNTS, 39, seed=61, weights="random")
    frames = ra.synthetic_frames(70, 39, seed=64)
    nan_frames = [3, 8]
    frames[3] = np.nan
    frames[8, 5] = np.nan
    frames[17] = np.inf
    frames[18, ::2] = -np.inf
    frames[33] = 1e12
    frames[34] *= 1e12
    frames[65] = 3e19  # ||x'||^2 overflows f32
    if kind == "diagonal-maximum":
        ref_s, ref_b = oracle.OracleFloat(ms).score(frames)
        s, b = ra.Scorer(ms, kind, max_frames=70).score_host(frames)
        _check_float(s, b, ref_s, ref_b, ms, frames)
    else:
        ref_s = oracle.batch_float_score(ms, frames)
        s, _ = ra.Scorer(ms, kind, max_frames=70).score_host(frames)
        rest = np.setdiff1d(np.arange(70), nan_frames)
        _assert_close(np.ascontiguousarray(s[:, rest]), np.ascontiguousarray(ref_s[:, rest]))
        flt_max = np.float32(3.40282347e+38).view(np.uint32)
        assert (s[:, nan_frames].view(np.uint32) == flt_max).all(), s[:, nan_frames]


@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_batch_float(gpu, pooled39, scale):
    ms, frames, _, _ = pooled39
    ref = oracle.batch_float_score(ms, frames[:257], n_threads=8)
    s, _ = ra.Scorer(ms, "batch-diagonal-maximum-float", max_frames=257, score_scale=scale).score_host(frames[:257])
    _assert_close(s, (np.float32(scale) * ref).astype(np.float32))


@pytest.mark.parametrize("dim,tying", [(45, "pooled"), (80, "pooled"), (16, "mixture-specific")])
def test_other_emits(gpu, dim, tying):
    """D = 45: scoreSplit32; D = 80: scoreSplit; mixture-specific covariances at D = 16: the covariance-free layout."""
    ms = ra.synthetic_mixture_set(len(COUNTS), COUNTS, dim, seed=65, weights="random", tying=tying)
    frames = ra.synthetic_frames(257, dim, seed=66)
    ref_s, ref_b = oracle.OracleFloat(ms).score(frames, n_threads=8)
    s, b = ra.Scorer(ms, "diagonal-maximum", max_frames=257).score_host(frames)
    _check_float(s, b, ref_s, ref_b, ms, frames)
