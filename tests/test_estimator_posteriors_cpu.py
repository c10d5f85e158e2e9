"""The Baum-Welch surface without a GPU: the four calls (gmm_density_posteriors_pairs_device / _host,
gmm_estimator_accumulate_posteriors_device / _host) are declared, exported and bound, the default weight threshold
is Core::Type<f32>::epsilon, and the numpy restatements the GPU tests compare the device with
(tests/posteriors_restatement.py) are self-consistent on a tiny model."""
import ctypes
import os
import re

import numpy as np

import posteriors_restatement as pr
import rasr_amd as ra
from rasr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"rasr_gmm.h": ["gmm_density_posteriors_pairs_device", "gmm_density_posteriors_pairs_host"],
         "rasr_gmm_estimator.h": ["gmm_estimator_accumulate_posteriors_device",
                                  "gmm_estimator_accumulate_posteriors_host"]}


def test_symbols_declared_exported_and_bound(built):
    lib = ctypes.CDLL(_capi.LIB_PATH)
    bound = {p[0]: p for p in _capi.PROTOTYPES}
    for header, names in CALLS.items():
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for n in names:
            assert re.search(r"^int\s+" + n + r"\s*\(", src, re.M), (header, n)
            assert hasattr(lib, n), n
            assert n in bound and bound[n][1] is ctypes.c_int, n
    # the argument counts of the declarations
    assert len(bound["gmm_density_posteriors_pairs_device"][2]) == 11
    assert len(bound["gmm_density_posteriors_pairs_host"][2]) == 10
    assert len(bound["gmm_estimator_accumulate_posteriors_device"][2]) == 11
    assert len(bound["gmm_estimator_accumulate_posteriors_host"][2]) == 10
    assert bound["gmm_estimator_accumulate_posteriors_device"][2][9] is ctypes.c_double
    for cls, names in ((ra.Scorer, ["density_posteriors_device", "density_posteriors"]),
                       (ra.Estimator, ["accumulate_posteriors_device", "accumulate_posteriors_host"])):
        for n in names:
            assert callable(getattr(cls, n)), n


def test_null_handles_are_refused(built):
    lib = ra.load_library()
    assert lib.gmm_density_posteriors_pairs_device(None, None, 0, 0, None, None, 0, None, 0, None, None) == -1
    assert lib.gmm_density_posteriors_pairs_host(None, None, 0, 0, None, None, 0, None, 0, None) == -1
    assert lib.gmm_estimator_accumulate_posteriors_device(None, None, None, 0, 0, None, None, None, 0, 0.0, None) == -1
    assert lib.gmm_estimator_accumulate_posteriors_host(None, None, None, 0, 0, None, None, None, 0, 0.0) == -1
    assert b"null" in lib.gmm_last_error()


def test_default_weight_threshold():
    assert ra.DEFAULT_WEIGHT_THRESHOLD == float(np.finfo(np.float32).eps)
    header = open(os.path.join(ROOT, "include", "rasr_gmm_estimator.h")).read()
    m = re.search(r"#define\s+GMM_ESTIMATOR_DEFAULT_WEIGHT_THRESHOLD\s+(\S+)", header)
    assert m and float(m.group(1)) == ra.DEFAULT_WEIGHT_THRESHOLD


def _tiny():
    counts = np.array([3, 1, 0, 7, 2])
    ms = ra.synthetic_mixture_set(5, counts, 13, seed=3, n_covariances=2, weights="random")
    frames = ra.synthetic_frames(6, 13, seed=4)
    pf = np.repeat(np.arange(6, dtype=np.uint32), 5)
    pm = np.tile(np.arange(5, dtype=np.uint32), 6)
    return ms, frames, pf, pm


def test_restated_rows_sum_to_one_small_scores(built):
    """Rows sum to 1 within n 2^-22.  That bound knows nothing of the size of the scores, and the f32 rounding of the
    log denominator alone moves every posterior of a row by up to ulp32(logDen) / 2 relative: it can hold only while
    ulp32(logDen) stays near 2^-22.  So it is asserted on a model of dimension 2, whose scores stay below 16 (the 13-
    dimensional model below has logDen of 17 .. 47 and its rows are off by up to 3.8 n 2^-22; they are held to
    the bound that follows the scores, row_sum_bound)."""
    counts = np.array([3, 1, 0, 7, 2])
    ms = ra.synthetic_mixture_set(5, counts, 2, seed=3, n_covariances=2, weights="random")
    frames = ra.synthetic_frames(40, 2, seed=4)
    pf = np.repeat(np.arange(40, dtype=np.uint32), 5)
    pm = np.tile(np.arange(5, dtype=np.uint32), 40)
    post, logden, _ = pr.posteriors(pr.SumModel(ms), frames, pf, pm, 7)
    assert np.nanmax(np.where(np.isfinite(logden), np.abs(logden), 0)) < 16
    n = counts[pm]
    dev = np.abs(post.astype(np.float64).sum(axis=1) - 1.0)
    assert (dev[n > 0] <= n[n > 0] * 2.0 ** -22).all(), (dev[n > 0] / (n[n > 0] * 2.0 ** -22)).max()
    assert not post[n == 0].any()


def test_restated_posteriors(built):
    ms, frames, pf, pm = _tiny()
    model = pr.SumModel(ms)
    post, logden, scores = pr.posteriors(model, frames, pf, pm, 8)
    n = np.diff(ms.mixture_offsets.astype(np.int64))[pm]
    for i in range(len(pf)):
        assert (post[i, n[i]:] == 0).all()
        if n[i] == 0:
            assert logden[i] == np.inf and not post[i].any()
            continue
        # rows sum to 1 as far as the scores' size lets them (the restatement's expf / logf: half an ulp each)
        assert abs(post[i].astype(np.float64).sum() - 1.0) <= pr.row_sum_bound(logden[i], scores[i], post[i], 0.5)
        assert (post[i, :n[i]] > 0).all() and np.argmax(post[i]) == np.argmin(scores[i])
        if n[i] == 1:
            assert post[i, 0] == 1.0 and logden[i] == scores[i][0]
    # the log denominator is the diagonal-sum score of the oracle
    ref = model.oracle.score(frames)[0][pm, pf]
    ok = n > 0
    assert np.allclose(logden[ok], ref[ok], rtol=1e-6, atol=0)
    # out-of-range pairs
    p2, l2, _ = pr.posteriors(model, frames, [6, 0], [0, 5], 8)
    assert not p2.any() and (l2 == np.inf).all()
    # the bounds are positive where there is a posterior, and the floor elsewhere
    b_log, b_post = pr.posterior_bounds(logden, scores, post)
    assert (b_log[ok] > 0).all() and (b_post >= 2.0 ** -126).all()


def test_widen_is_exact():
    a = np.array([0.0, 1.0, -2.5, 2.0 ** -126, 2.0 ** -149, -3 * 2.0 ** -149, 1e-38, 3.4e38], np.float32)
    a.view(np.uint32)[4] = 1  # the smallest subnormal whatever the process's flush mode made of the literal
    a.view(np.uint32)[5] = 0x80000003
    got = pr.widen(a)
    assert got[4] == 2.0 ** -149 and got[5] == -3 * 2.0 ** -149 and got[3] == 2.0 ** -126
    assert got[1] == 1.0 and got[2] == -2.5 and got[0] == 0.0


def test_restated_expansion_and_threshold(built):
    ms, frames, pf, pm = _tiny()
    model = pr.SumModel(ms)
    post, _, _ = pr.posteriors(model, frames, pf, pm, 7)
    pw = np.random.default_rng(5).uniform(0.0, 2.0, size=len(pf))
    pw[:3] = [0.0, 1e-9, 1e6]
    fr, en, we, skipped, total = pr.expand(ms, 6, pf, pm, pw, post, ra.DEFAULT_WEIGHT_THRESHOLD)
    assert skipped == 6  # the empty mixture 2, once per frame
    assert total == 6 * 13 and 0 < len(we) < total
    assert (we > ra.DEFAULT_WEIGHT_THRESHOLD).all()
    # (pair, density) order: entries ascend within a pair, pairs ascend
    off = ms.mixture_offsets.astype(np.int64)
    mix_of = np.searchsorted(off, en, side="right") - 1
    pair_of = fr * 5 + mix_of
    assert (np.diff(pair_of) >= 0).all() and (np.diff(en)[np.diff(pair_of) == 0] > 0).all()
    # everything dropped is at or under the threshold; a higher threshold drops more, never adds
    all_w = pr.expand(ms, 6, pf, pm, pw, post, -np.inf)[2]
    assert len(all_w) == total and (np.sort(all_w)[:total - len(we)] <= ra.DEFAULT_WEIGHT_THRESHOLD).all()
    quarter = pr.expand(ms, 6, pf, pm, pw, post, 0.25)[2]
    assert len(quarter) < len(we) and (quarter > 0.25).all() and int((all_w > 0.25).sum()) == len(quarter)
    # strict: a threshold equal to an occurring weight excludes it
    t = float(np.sort(we)[len(we) // 2])
    strict = pr.expand(ms, 6, pf, pm, pw, post, t)[2]
    assert t not in strict and len(strict) == int((all_w > t).sum()) < int((all_w >= t).sum())
    # NaN weights never pass
    pn = pw.copy()
    pn[10] = np.nan
    assert not np.isnan(pr.expand(ms, 6, pf, pm, pn, post, -np.inf)[2]).any()
    # the tables: weights add up, the chunked rule equals the sequential one below a piece
    tab = pr.accumulate(ms, frames, fr, en, we)
    seq = pr.accumulate(ms, frames, fr, en, we, chunk=None)
    pr.assert_bit_equal(tab, seq)
    assert tab["entry_weights"].sum() == np.float64(sum(tab["entry_weights"]))
    assert np.isclose(tab["entry_weights"].sum(), we.sum(), rtol=1e-12)
    assert np.isclose(tab["covariance_weights"].sum(), we.sum(), rtol=1e-12)
    assert pr.expected_file(ms, tab)[:6] == b"MIXSET"
