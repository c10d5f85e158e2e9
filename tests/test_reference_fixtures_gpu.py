"""The GPU scorers against replies of the REFERENCE's own scorers (tests/golden/ref, made by
scripts/make_ref_golden.py from oracle/_ref/ref_scorers; nothing here reads a reference tree or the executable).

Float types: the project's 1e-4 relative contract with its near-tie rule (_check_float) on every frame whose
values are finite, on any host CPU.  On the two frames holding an inf / a nan the float contract's "non-finite
values exactly" (DESIGN.md section 3): nan where the reference has nan, the same signed infinity where it has
one, and its finite sentinels (0.5 FLT_MAX, FLT_MAX, the backoff score) within the same 1e-4.  These tests found
diagonal-sum returning nan for the frame holding +inf, where the reference returns +inf; the diagonal-sum kernels
were mended (kSplitInfFrame, gmm_kernels_split.hip).
GMM_FLAG_REFERENCE_ORDER and the integer types: bit for bit, which binds only where the host's rsqrtss gives the fixture's 1/sqrt(var) table (the rule of
tests/test_golden.py; tests/golden/ref/cpu_<vendor>/ holds the set made on the GPU host's CPU)."""
import os

import numpy as np
import pytest

import rasr_amd as ra
from oracle import ref_cases as rc
from test_gpu_parity import _assert_close, _check_float
from test_reference_pin import HERE, REF_GOLDEN, load_fixture, same_rsqrt_or_skip

pytestmark = pytest.mark.gpu

_id = lambda p: os.path.relpath(p, os.path.join(HERE, "golden", "ref"))  # noqa: E731

# main_kernel() where a fixture is meant to reach a particular kernel (the rules of
# test_gpu_parity.test_float_kernel_selection and test_covariances.test_float_tying_dimension_boundaries):
# (fixture, type) -> (scorer options, kernel)
KERNELS = {
    ("d39_pooled_random_float", "diagonal-maximum"): [({}, "scoreSplitWide")],  # one covariance, D <= 40
    ("d39_pooled_random_float", "batch-diagonal-maximum-float"): [({}, "scoreSplitWide")],
    ("d45_pooled_random", "diagonal-maximum"): [({}, "scoreSplit32"), (dict(split_tile16=True), "scoreSplit")],
    ("d45_pooled_random", "diagonal-sum"): [({}, "scoreSplit32Sum")],
    ("d39_mixture_specific_random", "diagonal-maximum"): [({}, "scoreSplit")],  # covariance-free layout, 8 K steps
    ("d39_mixture_specific_random", "diagonal-sum"): [({}, "scoreSplitSum")],
    ("d16_none_uniform", "diagonal-maximum"): [({}, "scoreSplitWide")],  # covariance-free layout, D <= 20
}


def _options(kind, mws, gs):
    kw = dict(mixture_weight_scale=mws, gaussian_scale=gs)
    if kind.startswith("preselection"):
        kw.update(clusters=rc.PRESEL["clusters"], select_clusters=rc.PRESEL["select"],
                  clustering_iterations=rc.PRESEL["iterations"], backoff_score=rc.PRESEL["backoff"])
    return kw


@pytest.mark.parametrize("path", REF_GOLDEN, ids=_id)
def test_float_types_against_reference(gpu, path):
    ms, _, frames, replies, _ = load_fixture(path)
    name = os.path.splitext(os.path.basename(path))[0]
    finite = np.isfinite(frames).all(1)
    assert finite.sum() == len(frames) - 2
    done = 0
    for (kind, mws, gs), r in replies.items():
        if kind not in rc.FLOAT_KINDS:
            continue
        for extra, kernel in KERNELS.get((name, kind), [({}, None)]):
            sc = ra.Scorer(ms, kind, max_frames=len(frames), **_options(kind, mws, gs), **extra)
            if kernel is not None:
                assert sc.main_kernel() == kernel, (name, kind, extra)
            s, b = sc.score_host(frames)
            ref_b = r.get("best")
            if ref_b is None:
                b = None
            print(f"{name} {kind} {extra}: non-finite frames gpu {s[0, ~finite]} reference {r['scores'][0, ~finite]}")
            _check_float(s[:, finite], None if b is None else b[:, finite], r["scores"][:, finite],
                         None if b is None else ref_b[:, finite], ms, frames[finite], None, mws=mws, gs=gs)
            rs, gs_ = r["scores"][:, ~finite], s[:, ~finite]
            assert np.array_equal(np.isnan(gs_), np.isnan(rs)), (name, kind)
            assert np.array_equal(np.isposinf(gs_), np.isposinf(rs)), (name, kind)
            assert np.array_equal(np.isneginf(gs_), np.isneginf(rs)), (name, kind)
            if np.isfinite(rs).any():
                _assert_close(gs_[np.isfinite(rs)], rs[np.isfinite(rs)])
            if b is not None:  # no best density where the reference has none
                assert np.array_equal(b[:, ~finite] == 0xFFFFFFFF, ref_b[:, ~finite] == 0xFFFFFFFF), (name, kind)
            done += 1
    if not done:
        assert not any(k[0] in rc.FLOAT_KINDS for k in replies)


@pytest.mark.parametrize("path", REF_GOLDEN, ids=_id)
def test_reference_order_bit_exact(gpu, path):
    ms, _, frames, replies, z = load_fixture(path)
    todo = [(k, r) for k, r in replies.items() if k[0] == "diagonal-maximum"]
    if todo:
        same_rsqrt_or_skip(ms, z)
    for (kind, mws, gs), r in todo:
        s, b = ra.Scorer(ms, kind, max_frames=len(frames), reference_order=True, mixture_weight_scale=mws,
                         gaussian_scale=gs).score_host(frames)
        assert rc.bits_equal(s, r["scores"]), (kind, mws, gs)
        assert np.array_equal(b, r["best"])


@pytest.mark.parametrize("path", REF_GOLDEN, ids=_id)
def test_integer_types_bit_exact(gpu, path):
    ms, frames, _, replies, z = load_fixture(path)
    todo = [(k, r) for k, r in replies.items() if k[0] in rc.INT_KINDS]
    if todo:
        same_rsqrt_or_skip(ms, z)
    for (kind, mws, gs), r in todo:
        s, b = ra.Scorer(ms, kind, max_frames=len(frames), **_options(kind, mws, gs)).score_host(frames)
        assert rc.bits_equal(s, r["scores"]), kind
        if "best" in r:
            assert np.array_equal(b, r["best"]), kind
