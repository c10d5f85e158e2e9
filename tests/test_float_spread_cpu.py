"""The spread statistic behind the float contract's condition (gmm_float_spread_bound), without
a GPU:

* the library's statistic against the numpy float64 restatement (tests/float_spread_models.py) within 1e-9 relative,
  for every layout, the scales and a mixture shard;
* monotone in the spread s of the ladder, and predicted = kappa x statistic with the kappa DESIGN.md records;
* the models the suite pins kernel names on stay within the contract, so none of them is routed: the benchmark's, and
  every model of test_float_kernel_selection, tests/test_k_step_ladder.py and tests/test_large_mixtures.py."""
import numpy as np
import pytest

import rasr_amd as ra
from rasr_amd import _capi

import float_spread_models as fm

KAPPA = 3.65  # 1.5 x the largest measured ratio (2.42), rounded up
LAYOUTS = [
    # scorer type, dimension, covariances, layout options, covariance-free layout
    ("diagonal-maximum", 39, 1, {}, False),
    ("diagonal-maximum", 45, 1, {"split_tile16": True}, False),
    ("diagonal-maximum", 39, 1, {"native_f32": True}, False),
    ("diagonal-maximum", 39, 3, {}, True),
    ("diagonal-maximum", 16, 3, {}, True),
    ("diagonal-maximum", 39, 3, {"native_f32": True}, False),
    ("diagonal-maximum", 45, 3, {}, False),  # 6 D + 4 > 256: the f32 kernel
    ("batch-diagonal-maximum-float", 39, 1, {}, False),
    ("diagonal-sum", 39, 1, {}, False),
    ("diagonal-sum", 16, 3, {}, True),
    ("preselection-batch-float", 39, 1, {}, False),
]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: "%s-D%d-C%d-%s" % (v[0], v[1], v[2], "-".join(v[3]) or "default"))
def test_statistic_against_restatement(built, layout):
    kind, d, c, opts, cov_free = layout
    last = 0.0
    for s in fm.SPREADS:
        ms = fm.spread_model(s, d, c)
        stat, predicted = ra.float_spread_bound(ms, kind, **opts)
        want, _ = fm.spread_statistic(ms, kind, covariance_free=cov_free)
        assert abs(stat - want) <= 1e-9 * want, (s, stat, want)
        assert abs(predicted - KAPPA * stat) <= 1e-12 * predicted
        assert stat > last, f"statistic not monotone in the spread: {stat} at s = {s} after {last}"
        last = stat


def test_statistic_scales_and_shard(built):
    """The Gaussian scale is in isv and the log norm, the mixture-weight scale in the row constant (batch-float takes
    neither); a mixture shard's statistic is over its own entries."""
    ms = fm.spread_model(2, 39)
    for kind in ("diagonal-maximum", "diagonal-sum", "batch-diagonal-maximum-float"):
        stat, _ = ra.float_spread_bound(ms, kind, mixture_weight_scale=0.7, gaussian_scale=1.3)
        scales = (0.7, 1.3) if kind != "batch-diagonal-maximum-float" else (1.0, 1.0)
        want, _ = fm.spread_statistic(ms, kind, *scales)
        assert abs(stat - want) <= 1e-9 * want
    whole, entry = fm.spread_statistic(ms)
    owner = int(np.searchsorted(ms.mixture_offsets, entry, side="right")) - 1
    for rng in ((0, owner), (owner, owner + 1), (owner + 1, ms.n_mixtures)):
        if rng[0] == rng[1]:
            continue
        stat, _ = ra.float_spread_bound(ms, mixture_range=rng)
        want, _ = fm.spread_statistic(ms, mixture_range=rng)
        assert abs(stat - want) <= 1e-9 * want
        assert (stat == ra.float_spread_bound(ms)[0]) == (rng[0] == owner) and stat <= whole * (1 + 1e-9)


def test_quantized_types_have_no_bound(built):
    with pytest.raises(ra.GmmError) as err:
        ra.float_spread_bound(fm.spread_model(1, 39), "SIMD-diagonal-maximum")
    assert err.value.code == _capi.GMM_ERR_UNSUPPORTED


def test_where_the_guard_engages_on_the_ladder(built):
    """One covariance at D = 39 / 45: s = 1 is within the contract, s >= 2 is not (measured on an MI355X: 1.03e-4 on
    scoreSplitWide at s = 2)."""
    for d in (39, 45):
        assert ra.float_spread_bound(fm.spread_model(1, d))[1] <= _capi.FLOAT_CONTRACT
        for s in fm.SPREADS[1:]:
            assert ra.float_spread_bound(fm.spread_model(s, d))[1] > _capi.FLOAT_CONTRACT


def _within(ms, kind, **opts):
    _, predicted = ra.float_spread_bound(ms, kind, **opts)
    assert predicted <= _capi.FLOAT_CONTRACT, f"{kind} {opts}: predicted {predicted:.3g}"
    return predicted


def test_pinned_models_stay_within_the_contract(built):
    """No model whose kernel name a test asserts comes near the threshold -- but for the offset, narrow models
    (test_gpu_parity._offset_model and test_large_mixtures' accuracy worst case), which were built to be the widest the
    float kernels hold 1e-4 on and are predicted at 4.4e-5 to 9.2e-5."""
    import test_gpu_parity as gp
    import test_k_step_ladder as kl
    import test_large_mixtures as lm
    worst = 0.0
    # test_float_kernel_selection
    for (m, k, d, c), opts in (((10, 4, 39, 1), {}), ((10, 4, 45, 1), {}), ((10, 4, 9, 1), {}),
                               ((10, 4, 45, 1), {"split_tile16": True}), ((10, 4, 39, 1), {"split_tile32": True}),
                               ((4, 600, 45, 1), {}), ((10, 4, 60, 1), {"split_tile32": True}), ((10, 4, 39, 3), {}),
                               ((10, 4, 16, 3), {}), ((10, 4, 45, 3), {}), ((10, 4, 39, 1), {"native_f32": True}),
                               ((10, 4, 90, 1), {})):
        worst = max(worst, _within(gp._model(m, k, d, c, "random"), "diagonal-maximum", **opts))
    worst = max(worst, _within(gp._model(10, 4, 39, 1, "random"), "batch-diagonal-maximum-float"))
    # tests/test_k_step_ladder.py: every rung of the expanded-form kernels, both count vectors, every type of the rung
    for family, _, _, d, opts in kl.LADDER:
        if family.startswith("direct"):
            continue
        for name in kl.COUNTS:
            ms, _ = kl._inputs(d, name, kl._model_opts(opts))
            for kind in kl.FAMILIES[family][1]:
                worst = max(worst, _within(ms, kind, **kl._scorer_opts(opts)))
    # tests/test_large_mixtures.py: key widths and fallbacks, diagonal-sum
    for case in lm._float_cases():
        d, c, opts, k, _ = case.values[0]
        worst = max(worst, _within(lm.large_model(k, d, c), "diagonal-maximum", **opts))
    for k, opts in ((513, {}), (1024, {}), (512, {}), (512, {"split_tile16": True})):
        worst = max(worst, _within(lm.large_model(k, 39), "diagonal-sum", **opts))
    assert worst <= 2e-6, worst
    # the offset, narrow models
    for d, c, opts, _, _ in lm.ACCURACY_CASES:
        for k in (160, 512, 1024):
            _within(gp._offset_model(5, lm.counts_for(k), d, c=c), "diagonal-maximum", **opts)
    for ms, opts in ((gp._offset_model(80, "ragged", 39), {}), (gp._offset_model(80, "ragged", 45), {}),
                     (gp._offset_model(40, 12, 39, c=3), {}), (gp._offset_model(40, 12, 39, c=3), {"native_f32": True})):
        for extra in ({}, {"split_tile16": True}, {"split_tile32": True}, {"native_f32": True}):
            _within(ms, "diagonal-maximum", **dict(opts, **extra))
    _within(gp._offset_model(80, "ragged", 39), "batch-diagonal-maximum-float")


def test_benchmark_model_stays_within_the_contract(built):
    """bench.py's default model (5000 mixtures x 160 densities, D = 39, seed 2024) on the float types: the flagship
    keeps its kernel."""
    ms = ra.synthetic_mixture_set(5000, 160, 39, seed=2024)
    for kind in ("diagonal-maximum", "batch-diagonal-maximum-float"):
        assert _within(ms, kind) <= 2e-6
