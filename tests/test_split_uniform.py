"""scoreSplitWide's uniform form (chunks whose mixtures all have the same, compiled, tile count: the loop body is whole
mixtures with the mixture bounds at compile-time places) against the generic form of the same kernel, bit for bit, and
against oracle.OracleFloat under the float rule of tests/test_gpu_parity.py (scores within 1e-4 relative, a different
best density only on a near tie of the two densities' float64 scores).

Pooled float diagonal-maximum at D = 39 (4 K steps), with and without best densities.  The compiled tile counts are
8 and 10 (gmm_kernels.hh SplitWideUniformT); a loop body is lcm(6, T) steps = 3 mixtures at both, and it runs while a
further mixture follows it, so chunks of 2 and 3 mixtures run no body, 4 run one body and the rest in the generic
steps, 7 run two.  gmm_scorer_set_chunk_target puts that many mixtures into a chunk: a target of 8 workgroup rows cuts
8 c mixtures into 8 chunks of c."""
import numpy as np
import pytest

import oracle
import rasr_amd as ra

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4  # tests/test_gpu_parity.py
D = 39
FRAMES = [1, 255, 256, 257, 512]
WIDE_FRAMES = 256  # frames of a scoreSplitWide workgroup: the frame tiles of a call
# (densities per mixture, mixtures per chunk): 8 and 10 tiles; 150 densities leave padding rows in the tenth tile
MODELS = [(160, 2), (160, 3), (160, 4), (160, 7), (128, 2), (128, 3), (128, 4), (128, 7), (150, 4)]


def _assert_close(gpu, ref):
    g, r = gpu.astype(np.float64), ref.astype(np.float64)
    err = np.abs(g - r) / np.maximum(1.0, np.abs(r))
    assert gpu.shape == ref.shape and not np.isnan(err).any() and err.max(initial=0.0) <= REL_TOL, \
        f"max rel err {err.max(initial=0.0)}"


def _f64_density_score(ms, e, j, x):
    i = int(ms.mixture_offsets[e]) + int(j)
    d = int(ms.mixture_densities[i])
    var = ms.variances[int(ms.density_covariance[d])].astype(np.float64)
    m = ms.means[int(ms.density_mean[d])].astype(np.float64)
    ln = len(var) * np.log(2 * np.pi) + np.log(var).sum()
    return 0.5 * (-2 * ms.mixture_log_weights[i] + ln + (((m - x) ** 2) / var).sum())


def _check_best(gpu_b, ref_b, ms, frames):
    assert gpu_b.shape == ref_b.shape
    for e, t in np.argwhere(gpu_b != ref_b):
        n = int(ms.mixture_offsets[e + 1] - ms.mixture_offsets[e])
        assert gpu_b[e, t] < n and ref_b[e, t] < n, f"mixture {e} frame {t}: {gpu_b[e, t]} vs {ref_b[e, t]}"
        x = frames[t].astype(np.float64)
        a, b = _f64_density_score(ms, e, gpu_b[e, t], x), _f64_density_score(ms, e, ref_b[e, t], x)
        assert abs(a - b) <= REL_TOL * max(1.0, abs(b)), f"mixture {e} frame {t}: {gpu_b[e, t]} vs {ref_b[e, t]}"


def _scorers(ms):
    """The model on the default scorer and on the one that keeps the generic form."""
    pair = (ra.Scorer(ms, "diagonal-maximum", max_frames=max(FRAMES)),
            ra.Scorer(ms, "diagonal-maximum", max_frames=max(FRAMES), split_wide_generic=True))
    assert all(sc.main_kernel() == "scoreSplitWide" and sc.k_steps() == 4 for sc in pair)
    return pair


def _set_chunks(scorers, n_chunks, n):
    """n_chunks chunks for a call of n frames, whatever its frame tiles."""
    for sc in scorers:
        sc.set_chunk_target(n_chunks * ((n + WIDE_FRAMES - 1) // WIDE_FRAMES))


_frames = ra.synthetic_frames(max(FRAMES), D, seed=72)
_cache = {}


def _case(key, counts):
    """(model, scorers, oracle scores, oracle best densities) of a model, built once."""
    if key not in _cache:
        ms = ra.synthetic_mixture_set(len(counts), counts, D, seed=71, weights="random")
        ref_s, ref_b = oracle.OracleFloat(ms).score(_frames, n_threads=8)
        _cache[key] = (ms, _scorers(ms), ref_s, ref_b)
    return _cache[key]


def _compare(ms, scorers, ref_s, ref_b, n, want_best):
    """Both scorers on the first n frames: bit-equal to each other, the float rule against the oracle."""
    uni, gen = scorers
    s, b = uni.score_host(_frames[:n], want_best=want_best)
    gs, gb = gen.score_host(_frames[:n], want_best=want_best)
    assert np.array_equal(s.view(np.int32), gs.view(np.int32))
    _assert_close(s, ref_s[:, :n])
    if want_best:
        assert np.array_equal(b, gb)
        _check_best(b, ref_b[:, :n], ms, _frames)


@pytest.mark.parametrize("want_best", [True, False], ids=["best", "scores"])
@pytest.mark.parametrize("n", FRAMES)
@pytest.mark.parametrize("densities,per_chunk", MODELS)
def test_uniform_chunks(gpu, densities, per_chunk, n, want_best):
    ms, scorers, ref_s, ref_b = _case((densities, per_chunk), [densities] * (8 * per_chunk))
    _set_chunks(scorers, 8, n)
    assert scorers[0].chunk_forms(n) == (8, 0) and scorers[1].chunk_forms(n) == (0, 8)
    _compare(ms, scorers, ref_s, ref_b, n, want_best)


# 16 mixtures of 10 tiles, 10 ragged ones of 80 tiles in all, 16 of 10 tiles: 8 chunks of 50 tiles or a little more,
# the first three uniform, the fourth not
MIXED = [160] * 16 + [16, 300, 33, 160, 1, 250, 100, 48, 129, 176] + [160] * 16


@pytest.mark.parametrize("want_best", [True, False], ids=["best", "scores"])
@pytest.mark.parametrize("n", [255, 512])
def test_uniform_and_ragged_chunks(gpu, n, want_best):
    """Both forms in one call, each over its own chunks: a launch per form."""
    ms, scorers, ref_s, ref_b = _case("mixed", MIXED)
    _set_chunks(scorers, 8, n)
    u, g = scorers[0].chunk_forms(n)
    assert u >= 3 and g >= 1
    assert scorers[1].chunk_forms(n) == (0, u + g)
    _compare(ms, scorers, ref_s, ref_b, n, want_best)
    launches, generic_launches = _launches(scorers[0], n), _launches(scorers[1], n)
    assert launches == generic_launches + 1


def _launches(sc, n):
    import ctypes
    k, name = ctypes.c_uint32(), ctypes.c_char_p()
    assert sc._lib.gmm_scorer_launch_info(sc.handle, n, ctypes.byref(k), ctypes.byref(name)) == 0
    assert name.value == b"scoreSplitWide"
    return k.value


@pytest.mark.parametrize("want_best", [True, False], ids=["best", "scores"])
@pytest.mark.parametrize("n", [257])
def test_tile_count_without_a_uniform_form(gpu, n, want_best):
    """6 tiles per mixture: no form is compiled for it, every chunk runs the generic one."""
    ms, scorers, ref_s, ref_b = _case("six", [96] * 32)
    _set_chunks(scorers, 8, n)
    assert scorers[0].chunk_forms(n) == (0, 8)
    _compare(ms, scorers, ref_s, ref_b, n, want_best)


def test_default_chunks_of_a_uniform_model(gpu):
    """The chunk table a call builds by itself: every chunk of a uniform model is uniform, one scorer launch."""
    ms, scorers, ref_s, ref_b = _case((160, 4), [160] * 32)
    _set_chunks(scorers, 0, 1)
    u, g = scorers[0].chunk_forms(300)
    assert u > 0 and g == 0
    _compare(ms, scorers, ref_s, ref_b, 300, True)
    assert _launches(scorers[0], 300) == _launches(scorers[1], 300)
