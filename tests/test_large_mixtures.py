"""Large mixtures: 128 .. 1025 densities in one mixture, where code paths change shape with the largest mixture.

Before this module no GPU parity test compared a score of a mixture of more than 160 densities (5000 x 160, 24 x 160, the
(70, 150) pairs case; the 600-density model of test_float_kernel_selection checks a kernel name only).  What changes
with the mixture size:

* split-f16 float kernels: the low keyBits mantissa bits of a row value hold (tile, slot); gmm_prepare.cc gives
  16-row tiles 6 bits up to 256 densities, 7 up to 512, 8 up to 1024, and 32-row tiles 6 / 7 / 8 bits up to
  128 / 256 / 512; past 512 a 32-row model moves to 16 rows, past 1024 the float types fall to scoreF32 and
  diagonal-sum is refused.  The reported score is the midpoint of the masked bits, v 2^e - offsetK0: its error is
  relative to the SHIFTED value, not to the score;
* quantized kernels: idxBits = bits(maxEntries) of the packed (score, density) int32 key, 9 and 10 here;
* per-pair kernels (best densities, posteriors): one wave per pair, 64 densities a pass, rows of maxEntries.

Models: counts [K, 1, K - 1, 17, K], frames on the means of densities (37 t) mod K_m of mixtures 0, 2, 4 in turn (plus
small noise), so that winners land in every tile and every row position, the last real row and the row next to the
pad tile included; the CPU oracle alone establishes that before any GPU result is looked at (_assert_coverage).

Tolerances: the float contract of tests/test_gpu_parity.py (REL_TOL = 1e-4 of max(1, |ref|), another best density only
for a tie within it); SIMD / batch-int bit-exact; posteriors and accumulation as tests/test_estimator_posteriors.py.

Measured on an MI355X, max |gpu - f64| / max(1, |f64|) on the offset, narrow-Gaussian models (test_accuracy_worst_case,
with best densities; scores-only calls carry no tag and lose nothing):

    kernel (tile rows)              D, covariances   6 bits (K = 160)   7 bits            8 bits
    scoreSplitWide (16)             39, 1            2.98e-5            1.81e-5 (K 512)   2.20e-5 (K 1024)
    scoreSplit32 (32)               39, 1            --                 3.22e-5 (K 160)   2.06e-5 (K 512)
    scoreSplit32 (32)               45, 1            --                 2.43e-5 (K 160)   2.58e-5 (K 512)
    scoreSplit (16)                 45, 1            2.21e-5            2.27e-5 (K 512)   2.70e-5 (K 1024)
    scoreSplit, covariance-free (16) 39, 3           1.17e-5            1.59e-5 (K 512)   2.19e-5 (K 1024)

The same calls without best densities: 1.3e-5 .. 2.9e-5, so on these models and frames (on a density, or far from all)
the f16 split and the f32 sums set the error and the key width adds at most 6e-6.  The contract holds with a factor of
three to spare at every width; no kernel choice was changed.

scoreSplitWide's chunk capacity (gmm_score.cc, "a mixture has more tiles than a scoreSplitWide chunk can address"): a
chunk is closed once it holds min(perChunk, kSplitWideChunkTiles / 2) tiles, so the refusal needs ONE mixture of more
than kSplitWideChunkTiles / 2 = 419 422 tiles (6.7 million densities).  The split layout exists only up to 1024
densities (64 tiles, 66 with the pair padding) per mixture, so no model reaches the refusal, whatever the memory: there
is no case for it.

diagonal-sum takes at most 1024 densities per mixture (test_diagonal_sum_refuses_1025), so its per-pair cases run on
the K = 1024 model, the largest a diagonal-sum handle exists for; SIMD and diagonal-maximum pairs run at K = 1025.
"""
import numpy as np
import pytest

import oracle
import posteriors_restatement as pr
import rasr_amd as ra
import test_best_pairs as bp
import test_diagonal_sum as ds
import test_estimator_posteriors as ep
import test_gpu_parity as gp
from rasr_amd import _capi

pytestmark = pytest.mark.gpu

N_FRAMES = 257  # crosses scoreSplitWide's 256-frame workgroup and the 128-frame waves


def counts_for(k):
    return [k, 1, k - 1, 17, k]


def large_model(k, d, c=1, seed=5):
    """Counts [K, 1, K - 1, 17, K], random weights in a narrow band (w ~ U[0.5, 1.5] normalised: -2 log w within 2.2
    in a mixture, far below the distance between two means), so that a frame on a mean is won by that density."""
    base = ra.synthetic_mixture_set(5, counts_for(k), d, seed=seed + k, n_covariances=c)
    rng = np.random.Generator(np.random.PCG64(seed + 1000 + k))
    logw = np.concatenate([np.log(w / w.sum()) for w in (rng.uniform(0.5, 1.5, n) for n in counts_for(k))])
    return ra.MixtureSet(base.means, base.variances, base.density_mean, base.density_covariance, base.mixture_offsets,
                         base.mixture_densities, logw)


def _targets(k):
    """(mixture, density) of frame t: mixtures 0, 2, 4 in turn, density (37 t) mod K_m; the last frames on the last
    real rows (K - 1: row (K - 1) % 16 of the last tile, the row next to the pad rows / the pad tile)."""
    cnt = counts_for(k)
    tg = [((0, 2, 4)[t % 3], (37 * t) % cnt[(0, 2, 4)[t % 3]]) for t in range(N_FRAMES)]
    tg[-3:] = [(0, k - 1), (2, k - 2), (4, k - 1)]
    return tg


def target_frames(ms, k, seed=9, noise=0.02):
    rng = np.random.Generator(np.random.PCG64(seed))
    frames = np.empty((N_FRAMES, ms.dimension), np.float32)
    for t, (m, j) in enumerate(_targets(k)):
        dns = int(ms.mixture_densities[int(ms.mixture_offsets[m]) + j])
        sd = np.sqrt(ms.variances[int(ms.density_covariance[dns])])
        frames[t] = ms.means[int(ms.density_mean[dns])] + noise * sd * rng.standard_normal(ms.dimension)
    return frames


def _assert_coverage(ref_b, k):
    """On the oracle's best densities alone: the K-sized mixtures' winners cover every 16-row tile 0 .. ceil(K/16)-1
    and all 16 row positions; the last real density of mixtures 0 and 4 wins its frame."""
    win = np.concatenate([ref_b[0], ref_b[4]]).astype(np.int64)
    assert win.max() < k
    assert set(win // 16) == set(range((k + 15) // 16)), "a tile without a winner"
    if k >= 16:
        assert set(win % 16) == set(range(16)), "a row position without a winner"
    assert ref_b[0, N_FRAMES - 3] == k - 1 and ref_b[4, N_FRAMES - 1] == k - 1


def _bits_for(n):
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def key_bits(k, rows):
    """gmm_prepare.cc: key width of the split-f16 kernels for mixtures of at most k densities."""
    return _bits_for((k + 31) // 32) + 4 if rows == 32 else _bits_for((((k + 15) // 16) + 1) & ~1) + 2


_MODELS = {}


def _case(k, d, c):
    """(model, frames, OracleFloat scores and best densities), computed once per (K, D, C)."""
    key = (k, d, c)
    if key not in _MODELS:
        ms = large_model(k, d, c)
        frames = target_frames(ms, k)
        ref_s, ref_b = oracle.OracleFloat(ms).score(frames, n_threads=8)
        _assert_coverage(ref_b, k)
        _MODELS[key] = (ms, frames, ref_s, ref_b)
    return _MODELS[key]


# ---------------------------------------------------------------------------------------------------------------
# 1. key widths and fallbacks of the float types
# ---------------------------------------------------------------------------------------------------------------

def _float_cases():
    out = []
    for k in (256, 257, 512, 513, 1008, 1024):  # 1008: 63 tiles, the pad tile is tile 63
        out.append((39, 1, {}, k, "scoreSplitWide"))
    out.append((39, 1, {}, 1025, "scoreF32"))
    for k in (257, 513, 1024):
        # 16-row tiles asked for: at D = 39 (4 K steps) that is scoreSplitWide again, the pair kernel scoreSplit takes
        # 16-row models of more K steps (D = 45: 5), so both dimensions run
        out.append((39, 1, {"split_tile16": True}, k, "scoreSplitWide"))
        out.append((45, 1, {"split_tile16": True}, k, "scoreSplit"))
    for k in (128, 129, 256, 257, 512):
        out.append((45, 1, {}, k, "scoreSplit32"))
    out.append((45, 1, {}, 513, "scoreSplit"))
    for k in (513, 1024):
        out.append((39, 3, {}, k, "scoreSplit"))  # covariance-free layout, keyBitsCov
    out.append((39, 3, {}, 1025, "scoreF32"))
    out.append((16, 3, {}, 1024, "scoreSplitWide"))
    return [pytest.param(c, id="D%d-C%d-%s-K%d" % (c[0], c[1], "split16" if c[2] else "default", c[3])) for c in out]


@pytest.mark.parametrize("case", _float_cases())
def test_float_key_widths_and_fallbacks(gpu, case):
    d, c, opts, k, kernel = case
    ms, frames, ref_s, ref_b = _case(k, d, c)
    sc = ra.Scorer(ms, "diagonal-maximum", max_frames=N_FRAMES, **opts)
    assert sc.main_kernel() == kernel
    s, b = sc.score_host(frames)
    err = gp._assert_close(s, ref_s).max()
    gp._check_float(s, b, ref_s, ref_b, ms, frames, None)
    s0, none = sc.score_host(frames, want_best=False)
    assert none is None
    err0 = gp._assert_close(s0, ref_s).max()
    print(f"D={d} C={c} K={k} {kernel}: max rel err {err:.3g} with best densities, {err0:.3g} scores only, "
          f"{int((b != ref_b).sum())} best densities differ (ties within the contract)")
    if c == 1:
        bf = ra.Scorer(ms, "batch-diagonal-maximum-float", max_frames=N_FRAMES, **opts)
        assert bf.main_kernel() == kernel
        ref = oracle.batch_float_score(ms, frames, n_threads=8)
        gp._assert_close(bf.score_host(frames)[0], ref)
        gp._assert_close(bf.score_host(frames, want_best=False)[0], ref)


# ---------------------------------------------------------------------------------------------------------------
# 2. diagonal-sum
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,opts,kernel", [(513, {}, "scoreSplitSum"), (1024, {}, "scoreSplitSum"),
                                           (512, {}, "scoreSplit32Sum"), (512, {"split_tile16": True}, "scoreSplitSum")])
def test_diagonal_sum_large(gpu, k, opts, kernel):
    ms, frames, _, _ = _case(k, 39, 1)
    ref_s, ref_b = oracle.OracleFloatSum(ms).score(frames, n_threads=8)
    sc = ra.Scorer(ms, "diagonal-sum", max_frames=N_FRAMES, **opts)
    assert sc.main_kernel() == kernel
    s, b = sc.score_host(frames)
    ds._check(ms, frames, s, b, ref_s, ref_b)
    assert ds._close(s, ds._f64_sum(ms, frames)) <= gp.REL_TOL
    s0, _ = sc.score_host(frames, want_best=False)
    assert ds._close(s0, ref_s.astype(np.float64)) <= gp.REL_TOL


def test_diagonal_sum_refuses_1025(gpu):
    """No split layout past 1024 densities per mixture: the refusal (and its code) of a model without one, as
    test_diagonal_sum_needs_split_kernel has it for 3 covariances at D = 45."""
    no_layout = ra.synthetic_mixture_set(10, 4, 45, seed=1, n_covariances=3)
    want = ep.code(lambda: ra.Scorer(no_layout, "diagonal-sum"))
    assert want == _capi.GMM_ERR_INVALID_ARGUMENT
    ms = large_model(1025, 39)
    with pytest.raises(ra.GmmError, match="diagonal-sum") as err:
        ra.Scorer(ms, "diagonal-sum", max_frames=N_FRAMES)
    assert err.value.code == want
    assert ra.Scorer(large_model(1024, 39), "diagonal-sum", max_frames=N_FRAMES).main_kernel() == "scoreSplitSum"


# ---------------------------------------------------------------------------------------------------------------
# 3. the accuracy worst case: offset, narrow Gaussians, where offsetK0 makes the shifted value several times the score
# ---------------------------------------------------------------------------------------------------------------

def _f64_maximum(ms, frames):
    """min_d 0.5 (-2 log c_d + logNorm + chi2_d) in float64, [mixtures, frames]."""
    out = np.empty((ms.n_mixtures, len(frames)))
    fr = frames.astype(np.float64)
    for e in range(ms.n_mixtures):
        b, en = int(ms.mixture_offsets[e]), int(ms.mixture_offsets[e + 1])
        idx = ms.mixture_densities[b:en]
        mean = ms.means[ms.density_mean[idx]].astype(np.float64)
        var = ms.variances[ms.density_covariance[idx]].astype(np.float64)
        ln = var.shape[1] * np.log(2 * np.pi) + np.log(var).sum(axis=1)
        chi = np.stack([(((mean - x) ** 2) / var).sum(axis=1) for x in fr])  # F x K
        out[e] = (0.5 * (-2 * ms.mixture_log_weights[b:en][None] + ln[None] + chi)).min(axis=1)
    return out


_WORST = {}


def _worst_case(k, d, c):
    key = (k, d, c)
    if key not in _WORST:
        ms = gp._offset_model(5, counts_for(k), d, c=c)
        frames = gp._frames_near(ms, N_FRAMES, seed=43 + c)
        _WORST[key] = (ms, frames, _f64_maximum(ms, frames))
    return _WORST[key]


ACCURACY_CASES = [
    # D, covariances, options, kernel at K = 160 / 512 / 1024, tile rows at each
    (39, 1, {}, ("scoreSplitWide", "scoreSplitWide", "scoreSplitWide"), (16, 16, 16)),
    (39, 1, {"split_tile32": True}, ("scoreSplit32", "scoreSplit32", "scoreSplitWide"), (32, 32, 16)),
    (45, 1, {}, ("scoreSplit32", "scoreSplit32", "scoreSplit"), (32, 32, 16)),
    (45, 1, {"split_tile16": True}, ("scoreSplit", "scoreSplit", "scoreSplit"), (16, 16, 16)),
    (39, 3, {}, ("scoreSplit", "scoreSplit", "scoreSplit"), (16, 16, 16)),
]


@pytest.mark.parametrize("ki", [0, 1, 2], ids=["K160", "K512", "K1024"])
@pytest.mark.parametrize("case", ACCURACY_CASES, ids=lambda c: "D%d-C%d-%s" % (c[0], c[1], "-".join(c[2]) or "default"))
def test_accuracy_worst_case(gpu, case, ki):
    """The 1e-4 contract against the float64 score at key widths 6, 7 and 8 (K = 160: the coverage before this module;
    K = 512 and 1024 are new).  The figures printed here are the table of the module's docstring and of DESIGN.md."""
    d, c, opts, kernels, rows = case
    k = (160, 512, 1024)[ki]
    ms, frames, f64 = _worst_case(k, d, c)
    sc = ra.Scorer(ms, "diagonal-maximum", max_frames=N_FRAMES, **opts)
    assert sc.main_kernel() == kernels[ki]
    s, b = sc.score_host(frames)
    s0, _ = sc.score_host(frames, want_best=False)
    err = np.abs(s.astype(np.float64) - f64) / np.maximum(1.0, np.abs(f64))
    err0 = np.abs(s0.astype(np.float64) - f64) / np.maximum(1.0, np.abs(f64))
    print(f"ACCURACY D={d} C={c} K={k} {kernels[ki]} rows={rows[ki]} key bits={key_bits(k, rows[ki])}: "
          f"max rel err {err.max():.3g} with best densities, {err0.max():.3g} scores only")
    assert err.max() <= gp.REL_TOL
    assert err0.max() <= gp.REL_TOL
    ref_s, ref_b = oracle.OracleFloat(ms).score(frames, n_threads=8)
    gp._check_float(s, b, ref_s, ref_b, ms, frames, None)


# ---------------------------------------------------------------------------------------------------------------
# 4. SIMD / batch-int: idxBits 9 and 10
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [257, 1024])
def test_quantized_idx_bits(gpu, k):
    ms, frames, _, _ = _case(k, 39, 1)
    assert _bits_for(k) == (9 if k == 257 else 10)
    ra.prepare_quantized_host(ms, "SIMD-diagonal-maximum")  # accepted on the key layout (test_host_prep.py pins the refusals)
    ra.prepare_quantized_host(ms, "batch-diagonal-maximum-int")
    ref_s, ref_b, _ = oracle.OracleSimd(ms).score(frames, n_threads=8)
    _assert_coverage(ref_b.astype(np.int64), k)
    sc = ra.Scorer(ms, "SIMD-diagonal-maximum", max_frames=N_FRAMES)
    s, b = sc.score_host(frames)
    gp._assert_bit_exact(s, ref_s)
    assert np.array_equal(b, ref_b)
    gp._assert_bit_exact(sc.score_host(frames, want_best=False)[0], ref_s)
    # the same handle's key layout serving the scores-only call
    nt = ra.Scorer(ms, "SIMD-diagonal-maximum", max_frames=N_FRAMES, no_score_only_twin=True)
    gp._assert_bit_exact(nt.score_host(frames, want_best=False)[0], ref_s)
    ref = oracle.batch_int_score(ms, frames, n_threads=8)
    for opts in ({}, {"full_keys": True}):
        bi = ra.Scorer(ms, "batch-diagonal-maximum-int", max_frames=N_FRAMES, **opts)
        gp._assert_bit_exact(bi.score_host(frames)[0], ref)
        gp._assert_bit_exact(bi.score_host(frames, want_best=False)[0], ref)


# ---------------------------------------------------------------------------------------------------------------
# 5. per-pair kernels
# ---------------------------------------------------------------------------------------------------------------

def _passes(ref_b, pm, pf, k):
    """The 64-density passes the pairs' winners lie in, by mixture."""
    return {m: set((ref_b[pm, pf][pm == m].astype(np.int64) // 64).tolist()) for m in range(5)}


@pytest.mark.parametrize("kind", ["SIMD-diagonal-maximum", "diagonal-maximum", "diagonal-sum"])
def test_pairs_large(gpu, kind):
    k = 1024 if kind == "diagonal-sum" else 1025  # diagonal-sum: the largest mixture the type takes
    ms, frames, ref_s, ref_b = _case(k, 39, 1)
    if kind == "SIMD-diagonal-maximum":
        ref_b = oracle.OracleSimd(ms).score(frames, n_threads=8)[1]
    elif kind == "diagonal-sum":
        ref_b = oracle.OracleFloatSum(ms).score(frames, n_threads=8)[1]
    pf, pm = bp._all_pairs(N_FRAMES, 5)
    last = (k - 1) // 64
    p = _passes(ref_b, pm, pf, k)
    assert {0, last // 2, last} <= p[0] and last in p[4] and p[1] == {0}  # first, middle, last pass; mixture 1
    sc = ra.Scorer(ms, kind, max_frames=N_FRAMES)
    got, _ = bp._host_pairs(sc, frames, pf, pm)
    assert np.array_equal(got, ref_b[pm, pf])


@pytest.fixture(scope="module")
def sum_case(gpu):
    ms, frames, _, _ = _case(1024, 39, 1)
    sc = ra.Scorer(ms, "diagonal-sum", max_frames=N_FRAMES)
    # frames on densities of the first, a middle and the last pass of mixtures 0, 2, 4 (the last three are the last
    # real rows), every mixture for some of them, a bad pair
    tf = np.array([0, 12, 27, 13, 254, 255, 256], np.uint32)
    pf = np.concatenate([tf, tf, [0, 3, 256, 1, N_FRAMES]]).astype(np.uint32)
    pm = np.concatenate([np.array(_targets(1024))[tf, 0], [4, 2, 0, 4, 2, 0, 0], [1, 3, 1, 3, 0]]).astype(np.uint32)
    return ms, frames, sc, pf, pm


def test_posteriors_large(gpu, sum_case):
    ms, frames, sc, pf, pm = sum_case
    assert sc.max_entries() == 1024
    post, logden = ep.device_posteriors(gpu, sc, frames, pf, pm)
    assert post.shape == (len(pf), 1024)
    ref_post, _ = ep.check_posteriors(ms, pr.SumModel(ms), frames, pf, pm, post, logden, 1024, "K = 1024")
    on_target = ref_post[:7].argmax(axis=1)
    assert {0, 15} <= set((on_target // 64).tolist()) and len(set((on_target // 64).tolist())) >= 3
    hp, hl = sc.density_posteriors(frames, pf, pm, 1024 + 5)  # padding columns past rowStride = maxEntries
    assert np.array_equal(hp[:, :1024].view(np.uint32), post.view(np.uint32)) and not hp[:, 1024:].any()
    assert np.array_equal(hl.view(np.uint32), logden.view(np.uint32))


def test_accumulate_posteriors_large(gpu, sum_case):
    ms, frames, sc, pf, pm = sum_case
    pw = np.random.default_rng(3).uniform(0.5, 2.0, size=len(pf))
    # a threshold low enough that densities of several passes of one pair stay in
    thr = 1e-30
    ref, skipped, live, total, _ = ep.expected(gpu, sc, ms, frames, pf, pm, pw, threshold=thr)
    assert skipped == 1 and total == int(np.array(counts_for(1024))[pm[:-1]].sum()) and len(pf) < live < total
    e = ra.Estimator(ms, max_pairs=len(pf) * 1024)
    assert ep.accumulate_posteriors(gpu, e, frames, pf, pm, pw, sc, threshold=thr) == 1
    pr.assert_bit_equal(e.get(), ref)
    small = ra.Estimator(ms, max_pairs=len(pf) * 1024 - 1)
    assert ep.code(lambda: ep.accumulate_posteriors(gpu, small, frames, pf, pm, pw, sc)) == _capi.GMM_ERR_CAPACITY
