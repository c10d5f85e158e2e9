"""gmm_estimator_estimate_ebw (include/rasr_gmm_estimator.h "The EBW estimate") against the restatement in
tests/ebw_restatement.py, on the tiny ragged topology of tests/test_ebw_file_cpu.py, pooled and one covariance per
density, for global-rwth and local-rwth.

Both sides run the same IEEE f64 sequence in the header's fixed order, so the f64 iteration constants are asked to be
bit-equal; the narrowed f32 means and variances are asked to be equal; the f64 log weights pass through the C library's
log / exp / log1p on both sides (math.* here) and are allowed one f32 ulp, the tolerance of
tests/cpp/affine_estimate_test.cc.
"""
import numpy as np
import pytest

import ebw_restatement as er
import rasr_amd as ra
from rasr_amd import _capi

D, COUNTS = 5, [1, 3, 2, 1]
TYPES = ["global-rwth", "local-rwth"]


def previous(tying, zero_weight=False):
    ms = ra.synthetic_mixture_set(len(COUNTS), COUNTS, D, seed=5, tying=tying, weights="random")
    if zero_weight:  # a previous mixture weight of 0: exp(-inf)
        lw = ms.mixture_log_weights.copy()
        lw[2] = -np.inf
        ms = ra.MixtureSet(means=ms.means, variances=ms.variances, density_mean=ms.density_mean,
                           density_covariance=ms.density_covariance, mixture_offsets=ms.mixture_offsets,
                           mixture_densities=ms.mixture_densities, mixture_log_weights=lw)
    return ms


def statistics(ms, seed, den_scale=0.5):
    """Tables as an accumulation would leave them: per density a weight, sums near weight * mean, squared sums near
    weight * (variance + mean^2); the denominator a scaled, perturbed copy."""
    rng = np.random.default_rng(seed)
    tabs = []
    for scale in (1.0, den_scale):
        t = er.zero_tables(ms)
        w = rng.uniform(20, 60, ms.n_entries) * scale
        t["entry_weights"][:] = w
        for e, d in enumerate(ms.mixture_densities):
            m, c = ms.density_mean[d], ms.density_covariance[d]
            mu = ms.means[m].astype(np.float64) + rng.normal(0, 0.05, D)
            t["mean_sums"][m] += w[e] * mu
            t["mean_weights"][m] += w[e]
            t["covariance_sums"][c] += w[e] * (ms.variances[c].astype(np.float64) * rng.uniform(0.9, 1.1, D) + mu * mu)
            t["covariance_weights"][c] += w[e]
        tabs.append(t)
    return tabs


def check(prev, num, den, **config):
    data = er.write_file(prev, num, den, 0.0)
    want, want_ic = er.estimate(prev, num, den, **config)
    got_ic = ra.ebw_iteration_constants(data, prev, **config)
    assert np.array_equal(got_ic.view(np.uint64), want_ic.view(np.uint64)), (got_ic, want_ic)
    got = ra.estimate_ebw(data, prev, **config)
    for key in ("density_mean", "density_covariance", "mixture_offsets", "mixture_densities"):
        assert np.array_equal(getattr(got, key), want[key]), key
    assert np.array_equal(got.means.view(np.uint32), want["means"].view(np.uint32))
    assert np.array_equal(got.variances.view(np.uint32), want["variances"].view(np.uint32))
    lw, ref = got.mixture_log_weights, want["mixture_log_weights"]
    assert (np.abs(lw - ref) <= 2.0 ** -23 * np.abs(ref)).all()
    return got, got_ic


@pytest.mark.parametrize("tying", ["pooled", "none"])
@pytest.mark.parametrize("kind", TYPES)
def test_against_restatement(tying, kind):
    prev = previous(tying)
    num, den = statistics(prev, 1)
    got, ic = check(prev, num, den, iteration_constants_type=kind)
    assert (ic >= 1).all() and not np.array_equal(got.means, prev.means)
    # other parameters move the constants
    _, ic2 = check(prev, num, den, iteration_constants_type=kind, step_size=3.0, beta=0.5, sigma_minimum=0.01)
    assert not np.array_equal(ic, ic2)


@pytest.mark.parametrize("tying", ["pooled", "none"])
@pytest.mark.parametrize("kind", TYPES)
def test_cases(tying, kind):
    prev = previous(tying)
    # a mixture with one density is mixture 0 and 3 of the topology throughout
    # minimum variance applied
    num, den = statistics(prev, 2)
    got, _ = check(prev, num, den, iteration_constants_type=kind, minimum_variance=5.0)
    assert (got.variances == np.float32(5.0)).any()
    # a previous mixture weight of 0
    zero = previous(tying, zero_weight=True)
    got, _ = check(zero, num, den, iteration_constants_type=kind)
    assert got.mixture_log_weights[2] < -1e300
    # a weight driven negative inside the Cambridge iteration: a negative numerator weight on the density with the
    # largest denominator / previous weight ratio, whose k is 0, so that its weight becomes the numerator weight
    neg = {k: v.copy() for k, v in num.items()}
    neg["entry_weights"][1] = -5.0
    heavy = {k: v.copy() for k, v in den.items()}
    heavy["entry_weights"][1] = 1e4
    got, _ = check(prev, neg, heavy, iteration_constants_type=kind, minimum_observation_weight=0.0)
    assert got.mixture_log_weights[1] < -1e300
    # removal: a density under the minimum observation weight leaves the model
    low = {k: v.copy() for k, v in num.items()}
    low["entry_weights"][3] = 1.0
    got, ic = check(prev, low, den, iteration_constants_type=kind)
    assert got.n_entries == sum(COUNTS) - 1 and len(ic) == sum(COUNTS) - 1


@pytest.mark.parametrize("kind", TYPES)
def test_mean_kept_where_weight_is_not_positive(kind):
    """dtWeight + ic <= 0: the density keeps its previous mean.  The constants outgrow any denominator weight of a
    density whose previous mixture weight is positive (D_k holds -dtWeight / previous weight), so the branch is reached
    only through a previous weight of 0, which leaves the density the minimum constant: entry 2 of the topology, with
    a denominator 10 heavier than its numerator, gets ic = 1 and dtWeight + ic = -9."""
    prev = previous("pooled", zero_weight=True)
    num, den = statistics(prev, 3)
    den["mean_weights"][2] = num["mean_weights"][2] + 10.0
    _, ic = er.estimate(prev, num, den, iteration_constants_type=kind)
    dt = num["mean_weights"][2] - den["mean_weights"][2]
    assert ic[2] == 1.0 and dt + ic[2] <= 0
    got, got_ic = check(prev, num, den, iteration_constants_type=kind)
    assert np.array_equal(got.means[2], prev.means[2]) and got_ic[2] == 1.0
    assert not np.array_equal(got.means[1], prev.means[1])
    # with one covariance per density that density's covariance has no positive weight left: a status (the reference's
    # verify(weight > 0)), not an abort
    alone = previous("none", zero_weight=True)
    num, den = statistics(alone, 3)
    den["mean_weights"][2] = num["mean_weights"][2] + 10.0
    with pytest.raises(ra.GmmError) as err:
        ra.estimate_ebw(er.write_file(alone, num, den, 0.0), alone, iteration_constants_type=kind)
    assert err.value.code == _capi.GMM_ERR_INVALID_ARGUMENT


def test_refusals():
    prev = previous("pooled")
    num, den = statistics(prev, 1)
    data = er.write_file(prev, num, den, 0.0)

    def code(fn):
        with pytest.raises(ra.GmmError) as err:
            fn()
        return err.value.code
    assert code(lambda: ra.estimate_ebw(data, prev, iteration_constants_type="cambridge")) == _capi.GMM_ERR_UNSUPPORTED
    assert code(lambda: ra.estimate_ebw(data[:-1], prev)) == _capi.GMM_ERR_INVALID_ARGUMENT
    other = ra.synthetic_mixture_set(4, [1, 2, 3, 1], D, seed=5, tying="pooled")
    assert code(lambda: ra.estimate_ebw(data, other)) == _capi.GMM_ERR_INVALID_ARGUMENT
    assert code(lambda: ra.estimate_ebw(data, previous("none"))) == _capi.GMM_ERR_INVALID_ARGUMENT
    # a density held by two mixture entries, in a topology that passes the checks against its own previous set
    shared = ra.MixtureSet(means=prev.means[:6], variances=prev.variances, density_mean=np.arange(6, dtype=np.uint32),
                           density_covariance=np.zeros(6, dtype=np.uint32), mixture_offsets=prev.mixture_offsets,
                           mixture_densities=np.array([0, 1, 2, 3, 4, 1, 5], dtype=np.uint32),
                           mixture_log_weights=prev.mixture_log_weights)
    s_num, s_den = statistics(shared, 4)
    assert code(lambda: ra.estimate_ebw(er.write_file(shared, s_num, s_den, 0.0), shared)) == _capi.GMM_ERR_UNSUPPORTED
    # statistics from which no positive variance comes out (the constants keep finite ones positive): a status, not
    # an abort
    bad = {k: v.copy() for k, v in num.items()}
    bad["covariance_sums"][:] = np.nan
    assert code(lambda: ra.estimate_ebw(er.write_file(prev, bad, den, 0.0), prev)) == _capi.GMM_ERR_INVALID_ARGUMENT
