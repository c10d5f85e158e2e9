"""What the estimator, the affine and the MLLR accumulators share (rasr_amd/csrc/gmm_pairaccum.hh): one small pair list
with one pair of every kind that is skipped, fed to all three handles, and the rule that a host call waits for the
device call before it on the same handle.  Every table must equal the numpy restatements (tests/affine_restatement.py,
tests/mllr_restatement.py, numpy_order of tests/test_estimator_accumulate.py) BIT FOR BIT.

The topology validation that the three creates share is tests/cpp/pair_topology_test.cc, run here without a GPU.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import affine_restatement as ar
import mllr_restatement as mr
import rasr_amd as ra
from test_estimator_accumulate import assert_bit_equal, numpy_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES, N_KEYS, NAN_FRAME = 8, 2, 7
HANDLES = ["estimator", "affine", "mllr-1-leaf", "mllr-3-leaves"]


def test_pair_topology_cpp_program(built):
    """tests/cpp/pair_topology_test.cc: the topology unit alone as a stand-alone program (built by make)."""
    r = subprocess.run([os.path.join(ROOT, "build", "tests", "pair_topology_test")], capture_output=True, text=True)
    assert r.returncode == 0 and "pair_topology_test: ok" in r.stdout, r.stdout + r.stderr


@functools.lru_cache(maxsize=None)
def case():
    """6 mixtures x 3 densities, D = 3, 8 frames, 40 pairs.  Frame 7 is NaN and named only by pairs that every handle
    skips: mixture out of range, density out of range, density 0xffffffff.  One pair names frame 8 (out of range), one
    names key 2 of 2 on a good frame: the keyed handles skip it, the estimator, which takes no keys, counts it."""
    ms = ra.synthetic_mixture_set(6, 3, 3, seed=11, n_covariances=3)
    frames = ra.synthetic_frames(N_FRAMES, 3, seed=12)
    frames[NAN_FRAME] = np.nan
    rng = np.random.default_rng(13)
    n = 40
    pf = rng.integers(0, NAN_FRAME, size=n).astype(np.uint32)
    pm = rng.integers(0, 6, size=n).astype(np.uint32)
    pd = rng.integers(0, 3, size=n).astype(np.uint32)
    pk = rng.integers(0, N_KEYS, size=n).astype(np.uint32)
    pw = rng.uniform(0.25, 2.0, size=n)
    pf[3] = N_FRAMES                          # frame out of range
    pf[9], pm[9] = NAN_FRAME, 6               # mixture out of range
    pf[17], pd[17] = NAN_FRAME, 3             # density out of range
    pf[26], pd[26] = NAN_FRAME, 0xFFFFFFFF    # no best density
    pk[33] = N_KEYS                           # key out of range
    c = dict(ms=ms, frames=frames, pf=pf, pm=pm, pd=pd, pk=pk, pw=pw)
    # the expected tables and skipped counts after one call and after two
    c["estimator"] = [numpy_order(ms, frames, pf, pm, pd, pw)]
    c["estimator"].append(numpy_order(ms, frames, pf, pm, pd, pw, tables=c["estimator"][0][0]))
    c["affine"] = [ar.accumulate(ms, frames, pf, pm, pd, pw, pk, n_keys=N_KEYS)]
    c["affine"].append(ar.accumulate(ms, frames, pf, pm, pd, pw, pk, n_keys=N_KEYS, tables=c["affine"][0][0]))
    for name, n_leaves in (("mllr-1-leaf", 1), ("mllr-3-leaves", 3)):
        leaf = (np.arange(6) % n_leaves).astype(np.uint32)
        c[name] = [mr.accumulate(ms, leaf, n_leaves, frames, pf, pm, pd, pw, pk, n_keys=N_KEYS)]
        c[name].append(mr.accumulate(ms, leaf, n_leaves, frames, pf, pm, pd, pw, pk, n_keys=N_KEYS, tables=c[name][0][0]))
    assert [c[h][0][1] for h in HANDLES] == [4, 5, 5, 5] and [c[h][1][1] for h in HANDLES] == [4, 5, 5, 5]
    return c


def create(handle):
    ms = case()["ms"]
    if handle == "estimator":
        return ra.Estimator(ms, max_pairs=64)
    if handle == "affine":
        return ra.AffineTransformAccumulator(ms, N_KEYS, max_pairs=64)
    n_leaves = 1 if handle == "mllr-1-leaf" else 3
    return ra.MllrAccumulator(ms, (np.arange(6) % n_leaves).astype(np.uint32), n_leaves, N_KEYS, max_pairs=64,
                              kinds=("full", "shift"))


def device_call(gpu, handle, acc, stream=None):
    """The case's list in one device call on `stream`; returns the tensors, which the call may still read."""
    import torch
    c = case()

    def ints(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(gpu)
    t = [torch.from_numpy(c["frames"]).to(gpu), ints(c["pf"]), ints(c["pm"]), ints(c["pd"]),
         torch.from_numpy(c["pw"]).to(gpu), ints(c["pk"])]
    torch.cuda.synchronize()
    if handle == "estimator":
        acc.accumulate_device(*t[:5], stream=stream)
    else:
        acc.accumulate_device(*t, stream=stream)
    return t


def host_call(handle, acc):
    c = case()
    if handle == "estimator":
        acc.accumulate_host(c["frames"], c["pf"], c["pm"], c["pd"], c["pw"])
    elif handle == "affine":
        acc.accumulate(c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], c["pk"])
    else:
        acc.accumulate_host(c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], c["pk"])


def same_bits(got, want, what):
    g, w = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    assert g.shape == w.shape, what
    assert np.isfinite(g).all(), f"{what}: not finite"
    diff = g.view(np.uint64) != np.ascontiguousarray(w).view(np.uint64)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ"


def assert_handle(handle, acc, want):
    """Every table of the handle is finite and equals the restatement's bit for bit."""
    ms = case()["ms"]
    if handle == "estimator":
        got = acc.get()
        assert all(np.isfinite(v).all() for v in got.values())
        assert_bit_equal(got, want)
    elif handle == "affine":
        for key in range(N_KEYS):
            got, ref = acc.tables(key), ar.finalize(want[key], ms)
            assert set(got) == {"beta", "k", "G", "mean", "cov"}
            for name in got:
                same_bits(got[name], ref[name], f"key {key} {name}")
    else:
        for key in range(N_KEYS):
            for leaf in range(acc.n_leaves):
                got = acc.tables(key, leaf)
                assert set(got) == {"Z", "G", "count_full", "count_shift", "beta", "shift"}
                for name in got:
                    same_bits(got[name], want[key][leaf][name], f"key {key} leaf {leaf} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("handle", HANDLES)
def test_skipped_pairs_and_tables(gpu, handle):
    want, skipped = case()[handle][0]
    acc = create(handle)
    held = device_call(gpu, handle, acc)
    assert acc.skipped == skipped
    assert_handle(handle, acc, want)
    del held


@pytest.mark.gpu
def test_one_leaf_mllr_skips_what_affine_skips(gpu):
    counts = []
    for handle in ("affine", "mllr-1-leaf"):
        acc = create(handle)
        held = device_call(gpu, handle, acc)
        counts.append(acc.skipped)
        del held
    assert counts[0] == counts[1] == 5


@pytest.mark.gpu
@pytest.mark.parametrize("handle", HANDLES)
def test_host_call_waits_for_device_call(gpu, handle):
    """A device call on a stream of its own, the host call straight after it: the host call must not overwrite what the
    device call still reads, and the tables are those of the two calls in sequence."""
    import torch
    want, skipped = case()[handle][1]
    acc = create(handle)
    held = device_call(gpu, handle, acc, stream=torch.cuda.Stream(device=gpu))
    host_call(handle, acc)
    assert acc.skipped == 2 * skipped
    assert_handle(handle, acc, want)
    del held
