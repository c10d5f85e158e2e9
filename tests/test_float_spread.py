"""The float 1e-4 contract on models of growing spread, per kernel family, against the oracle.

Every float kernel evaluates ||x'||^2 + ||m'||^2 - 2 x'.m' about one centre in f32; the oracle forms (mu - x) isv
before squaring.  The ladder (tests/float_spread_models.py: means ~ N(0, s^2), variances ~ U[0.01, 0.1], s = 1, 2, 3,
5, 8; frames at 0.05 sigma of a density -- the 16 of largest rho among them --, about the centre, and at c + 2 (mu - c)
of the farthest densities) leaves the regime in which that cancellation is harmless.  At every rung and family:

* with accept_spread_bound (the matrix-core kernel whatever the model): the measured error, with and without best
  densities, is at most the bound predicted from the model alone (gmm_float_spread_bound) -- the test that fails if
  the prediction is optimistic.  A best density other than the oracle's is accepted where the two densities' float64
  scores agree within max(1e-4, 2 predicted) relative (each candidate is off by at most `predicted`, so a swap needs
  them within twice that), and for at most 1 % of the (frame, mixture) cells: the float64 scores alone put 10-14 of
  20480 cells that close on these models.  Each case prints its measured error and its ratio to the statistic, the
  numbers behind kappa in DESIGN.md section 3;
* with default flags: where the prediction is within 1e-4, the same kernel within 1e-4 (tests/test_gpu_parity.py's
  _check_float, again at most 1 % near ties); where it is not, diagonal-maximum and batch-diagonal-maximum-float run
  scoreDirect, bit-exact, and diagonal-sum and preselection-batch-float are refused with GMM_ERR_UNSUPPORTED and a
  message that carries the predicted bound.

The paths that use the reference's arithmetic whatever the model (GMM_FLAG_REFERENCE_ORDER, gmm_best_density_pairs,
the density posteriors) get one case each at s = 8, asserting what they promise everywhere."""
import functools

import numpy as np
import pytest

import oracle
import rasr_amd as ra
from rasr_amd import _capi

import float_spread_models as fm
from test_gpu_parity import REL_TOL, _f64_density_score

pytestmark = pytest.mark.gpu

PRESEL = {"clusters": 64, "select_clusters": 8}
FAMILIES = {
    # id: (scorer type, dimension, covariances, layout options, kernel, covariance-free layout)
    "splitwide": ("diagonal-maximum", 39, 1, {}, "scoreSplitWide", False),
    "split32": ("diagonal-maximum", 45, 1, {}, "scoreSplit32", False),
    "split16": ("diagonal-maximum", 45, 1, {"split_tile16": True}, "scoreSplit", False),
    "f32": ("diagonal-maximum", 39, 1, {"native_f32": True}, "scoreF32", False),
    "covfree-d39": ("diagonal-maximum", 39, 3, {}, "scoreSplit", True),
    "covfree-d16": ("diagonal-maximum", 16, 3, {}, "scoreSplitWide", True),
    "f32-cov3": ("diagonal-maximum", 45, 3, {}, "scoreF32", False),
    "batch": ("batch-diagonal-maximum-float", 39, 1, {}, "scoreSplitWide", False),
    "sum32": ("diagonal-sum", 39, 1, {}, "scoreSplit32Sum", False),
    "sum16": ("diagonal-sum", 39, 1, {"split_tile16": True}, "scoreSplitSum", False),
    "presel": ("preselection-batch-float", 39, 1, {}, "scoreSplit", False),
}
ASSIGNING = ("diagonal-maximum", "diagonal-sum")
EXACT_ROUTE = ("diagonal-maximum", "batch-diagonal-maximum-float")


@functools.lru_cache(maxsize=None)
def _reference(kind, s, d, c):
    """(scores, best densities or None) of the oracle, computed once per model and type; not to be written to."""
    ms, frames = fm.spread_model(s, d, c), fm.ladder_frames(s, d, c)
    if kind == "diagonal-maximum":
        return oracle.OracleFloat(ms).score(frames, n_threads=8)
    if kind == "diagonal-sum":
        return oracle.OracleFloatSum(ms).score(frames, n_threads=8)
    if kind == "batch-diagonal-maximum-float":
        return oracle.batch_float_score(ms, frames, n_threads=8), None
    ref = oracle.OraclePresel(ms, "float", clusters=PRESEL["clusters"], select=PRESEL["select_clusters"])
    return ref.score(frames, n_threads=8), None


def _rel_err(got, ref):
    ref = ref.astype(np.float64)
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def _near_ties(ms, frames, got_b, ref_b, tol):
    """Cells whose best density differs from the oracle's: every one a near tie of the float64 scores (within tol
    relative, the rule of test_gpu_parity._check_float), and at most 1 % of the table."""
    mism = np.argwhere(got_b != ref_b)
    for e, t in mism:
        x = frames[t].astype(np.float64)
        a = _f64_density_score(ms, e, got_b[e, t], x)
        b = _f64_density_score(ms, e, ref_b[e, t], x)
        assert abs(a - b) <= tol * max(1.0, abs(b)), f"mixture {e} frame {t}: {got_b[e, t]} vs {ref_b[e, t]}"
    assert len(mism) <= 0.01 * got_b.size, f"{len(mism)} of {got_b.size} cells differ from the oracle's best density"
    return len(mism)


def _score(sc, kind, frames):
    """The handle's scores with and, for the assigning types, without best densities."""
    s, b = sc.score_host(frames)
    if kind not in ASSIGNING:
        return [s], None
    return [s, sc.score_host(frames, want_best=False)[0]], b


@pytest.mark.parametrize("s", fm.SPREADS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_spread_ladder(gpu, family, s):
    kind, d, c, opts, kernel, cov_free = FAMILIES[family]
    ms, frames = fm.spread_model(s, d, c), fm.ladder_frames(s, d, c)
    ref_s, ref_b = _reference(kind, s, d, c)
    kw = dict(opts, max_frames=len(frames), **(PRESEL if kind.startswith("preselection") else {}))
    stat, predicted = ra.float_spread_bound(ms, kind, **opts)
    assert abs(stat - fm.spread_statistic(ms, kind, covariance_free=cov_free)[0]) <= 1e-9 * stat

    # the matrix-core kernel whatever the model: within the predicted bound
    sc = ra.Scorer(ms, kind, accept_spread_bound=True, **kw)
    assert sc.main_kernel() == kernel
    assert sc.spread_bound() == (stat, predicted)
    scores, best = _score(sc, kind, frames)
    err = max(_rel_err(g, ref_s) for g in scores)
    print(f"{family} s={s}: max rel err {err:.3g}, statistic {stat:.3g}, ratio {err / stat:.2f}, predicted {predicted:.3g}")
    assert err <= predicted, f"measured {err:.3g} above the predicted bound {predicted:.3g} (statistic {stat:.3g})"
    if best is not None:
        _near_ties(ms, frames, best, ref_b, max(REL_TOL, 2 * predicted))
    sc.close()

    # default flags: the contract as stated, by the fast kernel, the exact route or a refusal
    if predicted <= _capi.FLOAT_CONTRACT:
        sc = ra.Scorer(ms, kind, **kw)
        assert sc.main_kernel() == kernel
        scores, best = _score(sc, kind, frames)
        assert max(_rel_err(g, ref_s) for g in scores) <= REL_TOL
        if best is not None:
            _near_ties(ms, frames, best, ref_b, REL_TOL)
    elif kind in EXACT_ROUTE:
        sc = ra.Scorer(ms, kind, **kw)
        assert sc.main_kernel() == "scoreDirect"
        assert sc.spread_bound() == (stat, predicted)
        scores, best = _score(sc, kind, frames)
        for g in scores:
            assert np.array_equal(g.view(np.uint32), ref_s.view(np.uint32))
        if best is not None:
            assert np.array_equal(best, ref_b)
    else:
        with pytest.raises(ra.GmmError) as refusal:
            ra.Scorer(ms, kind, **kw)
        assert refusal.value.code == _capi.GMM_ERR_UNSUPPORTED
        assert "%.3g" % predicted in str(refusal.value) and "GMM_FLAG_ACCEPT_SPREAD_BOUND" in str(refusal.value)


# ---- the paths that use the reference's arithmetic whatever the model, at the widest rung ----

def test_reference_order_at_s8(gpu):
    """GMM_FLAG_REFERENCE_ORDER (scoreDirect), which a model predicted above the contract is routed to: bit-exact."""
    for kind, c in (("diagonal-maximum", 1), ("diagonal-maximum", 3), ("batch-diagonal-maximum-float", 1)):
        ms, frames = fm.spread_model(8, 39, c), fm.ladder_frames(8, 39, c)
        ref_s, ref_b = _reference(kind, 8, 39, c)
        sc = ra.Scorer(ms, kind, max_frames=len(frames), reference_order=True)
        assert sc.main_kernel() == "scoreDirect" and sc.spread_bound() == (0.0, 0.0)
        scores, best = _score(sc, kind, frames)
        for g in scores:
            assert np.array_equal(g.view(np.uint32), ref_s.view(np.uint32))
        if best is not None:
            assert np.array_equal(best, ref_b)


def test_best_density_pairs_at_s8(gpu):
    """gmm_best_density_pairs of a routed diagonal-maximum handle: the restatement's own arithmetic and order, so
    the oracle's best densities; of a diagonal-sum handle on its matrix-core kernel: its f32 density scores, the
    oracle's best densities but for near ties (tests/test_best_pairs.py)."""
    ms, frames = fm.spread_model(8, 39), fm.ladder_frames(8, 39)
    pf, pm = np.meshgrid(np.arange(len(frames), dtype=np.uint32), np.arange(ms.n_mixtures, dtype=np.uint32), indexing="ij")
    pf, pm = pf.ravel(), pm.ravel()
    for kind, kw in (("diagonal-maximum", {}), ("diagonal-sum", {"accept_spread_bound": True})):
        sc = ra.Scorer(ms, kind, max_frames=len(frames), **kw)
        out = np.empty((ms.n_mixtures, len(frames)), np.float32)
        cid = sc.score_host_ring(frames, 0, len(frames), out, lazy_best=True)
        got = sc.best_pairs(cid, pf, pm).reshape(len(frames), ms.n_mixtures).T
        if kind == "diagonal-maximum":
            assert sc.main_kernel() == "scoreDirect" and np.array_equal(got, _reference(kind, 8, 39, 1)[1])
        else:
            _near_ties(ms, frames, got, _reference(kind, 8, 39, 1)[1], REL_TOL)


def test_density_posteriors_at_s8(gpu):
    """gmm_density_posteriors_pairs_* (the reference's scalar order) on the widest model: within the bounds of
    tests/test_estimator_posteriors.py, for frames near a far density, about the centre and beyond the model."""
    import posteriors_restatement as pr
    from test_estimator_posteriors import check_posteriors, device_posteriors
    ms = fm.spread_model(8, 39)
    frames = fm.ladder_frames(8, 39)[[0, 1, 2, 3, 9, 10, 100, 101, 240, 241, 254, 255]]
    sc = ra.Scorer(ms, "diagonal-sum", max_frames=len(frames), accept_spread_bound=True)
    pf, pm = np.meshgrid(np.arange(len(frames), dtype=np.uint32), np.arange(ms.n_mixtures, dtype=np.uint32), indexing="ij")
    pf, pm = pf.ravel(), pm.ravel()
    K = sc.max_entries()
    post, logden = device_posteriors(gpu, sc, frames, pf, pm, K)
    check_posteriors(ms, pr.SumModel(ms), frames, pf, pm, post, logden, K, "s = 8")


def test_offset_model_is_within_the_contract(gpu):
    """test_gpu_parity._offset_model, the widest model of the float tests before this ladder, stays on the
    matrix-core kernels: its predicted bound is within the contract on every layout those tests run."""
    from test_gpu_parity import _offset_model
    for ms, opts in ((_offset_model(80, "ragged", 39), {}), (_offset_model(80, "ragged", 45), {}),
                     (_offset_model(80, "ragged", 45), {"split_tile16": True}), (_offset_model(40, 12, 39, c=3), {}),
                     (_offset_model(40, 12, 39, c=3), {"native_f32": True})):
        sc = ra.Scorer(ms, "diagonal-maximum", max_frames=8, **opts)
        assert sc.spread_bound()[1] <= _capi.FLOAT_CONTRACT and sc.main_kernel() != "scoreDirect"
