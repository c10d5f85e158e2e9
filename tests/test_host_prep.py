"""Host-side model preparation of the product (rasr_amd/csrc/gmm_prepare.cc, via the C-ABI
gmm_prepare_quantized_host, no GPU needed) against the oracle's restatement: the quantization
scale, scaled inverse deviations, log normalisation, prepared means and constant weights must be
bit-identical (they decide every quantized score)."""
import numpy as np
import pytest

import oracle
import rasr_amd as ra

MODELS = [
    dict(n_mixtures=100, densities_per_mixture=10, dimension=39, seed=1),
    dict(n_mixtures=60, densities_per_mixture=17, dimension=45, seed=2, weights="random"),
    dict(n_mixtures=40, densities_per_mixture=9, dimension=39, seed=3, n_covariances=4, weights="random"),
    dict(n_mixtures=10, densities_per_mixture=5, dimension=80, seed=4),
    dict(n_mixtures=30, densities_per_mixture=3, dimension=1, seed=5),
]


@pytest.mark.parametrize("kw", MODELS)
def test_simd_prepare_bit_exact(built, kw):
    ms = ra.synthetic_mixture_set(**kw)
    o = oracle.OracleSimd(ms)
    p = ra.prepare_quantized_host(ms, "SIMD-diagonal-maximum")
    assert p["scaling"] == o.scaling
    assert np.array_equal(p["isv"], o.isv)
    assert np.array_equal(p["log_norm"], o.log_norm)
    assert np.array_equal(p["prepared_mean"], o.prepared_mean)
    assert np.array_equal(p["constant_weight"], o.constant_weight)


@pytest.mark.parametrize("kw", [m for m in MODELS if m.get("n_covariances", 1) == 1])
def test_batch_int_prepare_bit_exact(built, kw):
    ms = ra.synthetic_mixture_set(**kw)
    scale_, var, const = oracle.batch_int_prepare(ms)
    p = ra.prepare_quantized_host(ms, "batch-diagonal-maximum-int")
    assert np.array_equal(p["isv"][0], var)
    assert np.array_equal(p["constant_weight"], const)
    assert np.float32(2.0 * np.float64(np.float32(p["scaling"]) * np.float32(p["scaling"]))) == np.float32(scale_)


def test_prepare_rejects_bad_models(built):
    ms = ra.synthetic_mixture_set(5, 3, 8, seed=9)
    ms.variances[0, 3] = 0.0  # require(checkDiagonal) -- CovarianceFeatureScorerElement.cc:26
    with pytest.raises(ra.GmmError, match="covariance diagonal"):
        ra.prepare_quantized_host(ms)
    ms2 = ra.synthetic_mixture_set(5, 3, 8, seed=9, n_covariances=2)
    with pytest.raises(ra.GmmError, match="pooled"):
        ra.prepare_quantized_host(ms2, "batch-diagonal-maximum-int")
    ms3 = ra.synthetic_mixture_set(5, 3, 8, seed=9)
    ms3.mixture_densities[2] = 1000
    with pytest.raises(ra.GmmError, match="out of range"):
        ra.prepare_quantized_host(ms3)


def _regroup(ms, k):
    """The same densities, weights and tables with every mixture cut into mixtures of at most k entries: the rows of
    the device tiles, their biases and bounds stay what they were, only the entry counts change."""
    off = ms.mixture_offsets.astype(np.int64)
    cuts = [0]
    for m in range(ms.n_mixtures):
        cuts += list(range(int(off[m]) + k, int(off[m + 1]), k)) + [int(off[m + 1])]
    return ra.MixtureSet(ms.means, ms.variances, ms.density_mean, ms.density_covariance, cuts, ms.mixture_densities,
                         ms.mixture_log_weights)


@pytest.mark.parametrize("kind", ["SIMD-diagonal-maximum", "batch-diagonal-maximum-int"])
def test_prepare_refuses_by_density_index_bits(built, kind):
    """The packed (score, density) key leaves the score 31 - idxBits bits, idxBits = bits(largest mixture): a model of
    tightly clustered means (a large quantization scale, hence large constant weights) passes with mixtures of 256
    entries (idxBits 8, limit 2^23 - 2) and is refused with 1024 (idxBits 10, limit 2^21 - 2).  The models of
    tests/test_large_mixtures.py pass at idxBits 10 and 11 (its test_quantized_idx_bits prepares them)."""
    base = ra.synthetic_mixture_set(3, [1024, 5, 700], 39, seed=3, weights="random")
    ms = ra.MixtureSet(base.means * np.float32(0.1), base.variances, base.density_mean, base.density_covariance,
                       base.mixture_offsets, base.mixture_densities, base.mixture_log_weights)
    with pytest.raises(ra.GmmError, match=r"model outside the packed \(score, density\) int32 range; use fewer densities "
                                          r"per mixture") as err:
        ra.prepare_quantized_host(ms, kind)
    assert err.value.code == ra._capi.GMM_ERR_INVALID_ARGUMENT
    small = _regroup(ms, 256)
    assert small.n_entries == ms.n_entries and int(np.diff(small.mixture_offsets.astype(np.int64)).max()) == 256
    p = ra.prepare_quantized_host(small, kind)  # the same rows at idxBits 8
    # the unscaled model at 1024 entries: the count alone does not refuse
    q = ra.prepare_quantized_host(base, kind)
    assert p["scaling"] > 5 * q["scaling"]


def test_prepare_refuses_mixtures_too_large(built):
    """Several covariances leave the frame's sum of squares (<= D 128^2) as headroom in every key: at D = 128 that
    is 2^21, all a key of idxBits 10 (a mixture of 513 .. 1024 entries) has.  The same densities in mixtures of at
    most 256 are accepted."""
    ms = ra.synthetic_mixture_set(2, [513, 3], 128, seed=4, n_covariances=2, weights="random")
    with pytest.raises(ra.GmmError, match=r"mixtures too large for the packed \(score, density\) int32 encoding") as err:
        ra.prepare_quantized_host(ms)
    assert err.value.code == ra._capi.GMM_ERR_INVALID_ARGUMENT
    ra.prepare_quantized_host(_regroup(ms, 256))
    # one covariance needs no headroom: the same count is no refusal there
    ra.prepare_quantized_host(ra.synthetic_mixture_set(2, [513, 3], 128, seed=4, weights="random"))


def test_multiply_and_quantize_matches_context(built):
    # quantized frame of the reference Context (SimdFeatureScorer.cc:22-35) == oracle, here via host prep tables
    ms = ra.synthetic_mixture_set(20, 4, 39, seed=6, n_covariances=3)
    o = oracle.OracleSimd(ms)
    p = ra.prepare_quantized_host(ms)
    x = ra.synthetic_frames(5, 39, seed=1)
    for f in x:
        q = o.quantize_frame(f)
        for c in range(3):
            want = oracle.quantize_array(f * p["isv"][c])
            assert np.array_equal(q[c, :39], want)
            assert not q[c, 39:].any()
