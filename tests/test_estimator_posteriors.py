"""Baum-Welch accumulation on the device: gmm_density_posteriors_pairs_* (rasr_amd/csrc/gmm_kernels_posterior.hip) and
gmm_estimator_accumulate_posteriors_* (include/rasr_gmm_estimator.h).

A. The posteriors against the numpy restatement (tests/posteriors_restatement.py: oracle.float_distance /
   oracle.gauss_log_norm for the density scores, f32 operations in the reference's order for the rest).  The device and
   the host library may differ by about an ulp per expf / logf; the order being the same, that gives
       |logDen - ref| <= 2 ulp32(|ref|)
       |post - ref|   <= (2 ulp32(|logDen_ref|) + ulp32(|logDen_ref - s_j|) + 2^-20) post_ref + 2^-126
   Measured on an MI355X (the maxima each case prints): logDen equal to the restatement's in every pair of every
   case (0 ulp32), posteriors at most 0.024 of their bound, |row sum - 1| at most 3.99e-6 (0.44 of row_sum_bound,
   which follows the size of the scores: the rounding of logDen alone moves a row by ulp32(logDen) / 2).
   The second shape (10 mixtures of 70-150 densities, D = 45) runs with one covariance, as it does for this scorer
   type in tests/test_best_pairs.py: a diagonal-sum scorer of several covariances takes D <= 42.  The fourth shape
   puts the several covariances and the 64- / 128-entry lane blocks together at D = 39.
B. The accumulation, bit for bit, against the restatement fed with THE DEVICE'S OWN posteriors of the same inputs:
   expanded in (pair, density) order, w * (f64) post <= threshold dropped, the sequential f64 rule in pieces of 512.
"""
import numpy as np
import pytest

import posteriors_restatement as pr
import rasr_amd as ra
from rasr_amd import _capi

pytestmark = pytest.mark.gpu

THR = ra.DEFAULT_WEIGHT_THRESHOLD


# ---------------------------------------------------------------------------------------------------------------
# device calls
# ---------------------------------------------------------------------------------------------------------------

def _ints(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(gpu)


def _frames(gpu, frames, stride=None):
    import torch
    D = frames.shape[1]
    x = torch.zeros((frames.shape[0], stride or D), dtype=torch.float32, device=gpu)
    x[:, :D] = torch.from_numpy(np.ascontiguousarray(frames)).to(gpu)
    return x


def device_posteriors(gpu, sc, frames, pf, pm, row_stride=None, stride=None):
    import torch
    post, logden = sc.density_posteriors_device(_frames(gpu, frames, stride), _ints(gpu, pf), _ints(gpu, pm), row_stride)
    torch.cuda.synchronize()
    return post.cpu().numpy(), logden.cpu().numpy()


def accumulate_posteriors(gpu, e, frames, pf, pm, pw=None, scorer=None, threshold=None, stride=None):
    import torch
    x, tf, tm = _frames(gpu, frames, stride), _ints(gpu, pf), _ints(gpu, pm)
    tw = None if pw is None else torch.from_numpy(np.ascontiguousarray(pw, dtype=np.float64)).to(gpu)
    torch.cuda.synchronize()
    e.accumulate_posteriors_device(x, tf, tm, tw, scorer=scorer, weight_threshold=threshold)
    return e.skipped  # waits for the call: the tensors may go


def accumulate_viterbi(gpu, e, frames, pf, pm, pd, pw=None):
    import torch
    x, tf, tm, td = _frames(gpu, frames), _ints(gpu, pf), _ints(gpu, pm), _ints(gpu, pd)
    tw = None if pw is None else torch.from_numpy(np.ascontiguousarray(pw, dtype=np.float64)).to(gpu)
    torch.cuda.synchronize()
    e.accumulate_device(x, tf, tm, td, tw)
    return e.skipped


def _counts(m, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=m)


def _all_pairs(nf, nm):
    f, m = np.meshgrid(np.arange(nf, dtype=np.uint32), np.arange(nm, dtype=np.uint32), indexing="ij")
    return f.ravel(), m.ravel()


def _k_max(ms):
    return int(np.diff(ms.mixture_offsets.astype(np.int64)).max())


def code(fn):
    with pytest.raises(ra.GmmError) as err:
        fn()
    return err.value.code


# ---------------------------------------------------------------------------------------------------------------
# A. posteriors
# ---------------------------------------------------------------------------------------------------------------

def check_posteriors(ms, model, frames, pf, pm, got_post, got_logden, row_stride, label):
    ref_post, ref_logden, scores = pr.posteriors(model, frames, pf, pm, row_stride)
    b_log, b_post = pr.posterior_bounds(ref_logden, scores, ref_post)
    n = np.array([len(s) for s in scores])
    ok = n > 0
    # bad pairs and empty mixtures: zero rows and +inf
    assert (got_logden[~ok] == np.inf).all() and not got_post[~ok].any()
    d_log = np.abs(got_logden[ok].astype(np.float64) - ref_logden[ok].astype(np.float64))
    d_post = np.abs(got_post.astype(np.float64) - ref_post.astype(np.float64))
    sums = np.abs(got_post.astype(np.float64).sum(axis=1) - 1.0)
    s_bound = np.array([pr.row_sum_bound(ref_logden[i], scores[i], ref_post[i], 4) if n[i] else 1.0
                        for i in range(len(pf))])
    print(f"{label}: max |logDen - ref| = {(d_log / pr.ulp32(ref_logden[ok])).max():.2f} ulp32 "
          f"({(d_log / b_log[ok]).max():.3f} of the bound), max |post - ref| = {(d_post / b_post).max():.3f} of the bound, "
          f"max |row sum - 1| = {sums[ok].max():.3e} ({(sums[ok] / s_bound[ok]).max():.3f} of the bound)")
    assert (d_log <= b_log[ok]).all()
    assert (d_post <= b_post).all()
    assert (sums[ok] <= s_bound[ok]).all()
    # padding columns are 0
    for i in range(len(pf)):
        assert not got_post[i, n[i]:].any()
    # the log denominator is the diagonal-sum score
    ref_score = model.oracle.score(frames)[0]
    inr = ok & (np.asarray(pf) < frames.shape[0])
    want = ref_score[np.asarray(pm)[inr], np.asarray(pf)[inr]]
    assert np.allclose(got_logden[inr], want, rtol=1e-6, atol=0)
    return ref_post, ref_logden


POSTERIOR_CASES = [
    # mixtures, (low, high) densities per mixture, D, covariances, frames
    (30, (1, 40), 39, 1, 33),     # the common shape
    (10, (70, 150), 45, 1, 9),    # crosses the 64- and 128-entry lane blocks
    (16, (0, 5), 13, 1, 20),      # empty mixtures, D % 4 != 0
    (10, (70, 150), 39, 2, 6),    # the lane blocks with several covariances
]


@pytest.mark.parametrize("case", POSTERIOR_CASES)
def test_posteriors_against_restatement(gpu, case):
    m, (lo, hi), d, c, f = case
    ms = ra.synthetic_mixture_set(m, _counts(m, lo, hi, m + d), d, seed=76 + m, n_covariances=c, weights="random")
    frames = ra.synthetic_frames(f, d, seed=77)
    sc = ra.Scorer(ms, "diagonal-sum", max_frames=f)
    pf, pm = _all_pairs(f, m)
    # pairs out of range among them
    pf = np.concatenate([pf, [f, 0, 1 << 30, 0xFFFFFFFF]]).astype(np.uint32)
    pm = np.concatenate([pm, [0, m, 1, 0xFFFFFFFF]]).astype(np.uint32)
    K = _k_max(ms) + 3  # padding columns
    assert sc.max_entries() == K - 3
    post, logden = device_posteriors(gpu, sc, frames, pf, pm, K, stride=d + 5)
    check_posteriors(ms, pr.SumModel(ms), frames, pf, pm, post, logden, K, f"case {case}")
    if lo == 0:
        assert (np.diff(ms.mixture_offsets) == 0).any()
    # the host call and a second device call: the same bits
    hp, hl = sc.density_posteriors(frames, pf, pm, K)
    assert np.array_equal(hp.view(np.uint32), post.view(np.uint32)) and np.array_equal(hl.view(np.uint32), logden.view(np.uint32))
    p2, l2 = device_posteriors(gpu, sc, frames, pf, pm, K)
    assert np.array_equal(p2.view(np.uint32), post.view(np.uint32)) and np.array_equal(l2.view(np.uint32), logden.view(np.uint32))


def test_posteriors_scales(gpu):
    """The handle's mixture-weight and Gaussian scales are in the posteriors; its score_scale is not."""
    ms = ra.synthetic_mixture_set(20, _counts(20, 2, 30, 5), 39, seed=78, weights="random")
    frames = ra.synthetic_frames(15, 39, seed=79)
    sc = ra.Scorer(ms, "diagonal-sum", max_frames=15, mixture_weight_scale=3.0, gaussian_scale=0.25, score_scale=2.0)
    pf, pm = _all_pairs(15, 20)
    K = _k_max(ms)
    post, logden = device_posteriors(gpu, sc, frames, pf, pm)
    assert post.shape == (300, K)
    ref_post, _ = check_posteriors(ms, pr.SumModel(ms, 3.0, 0.25), frames, pf, pm, post, logden, K, "scales")
    plain = pr.posteriors(pr.SumModel(ms), frames, pf, pm, K)[0]
    assert np.abs(plain - ref_post).max() > 1e-3  # the scales matter


def test_posteriors_underflow(gpu):
    """A frame on one density's mean, the others far away: every other posterior underflows, that one is 1."""
    base = ra.synthetic_mixture_set(4, 6, 39, seed=80, weights="random")
    ms = ra.MixtureSet(means=base.means * np.float32(10), variances=base.variances, density_mean=base.density_mean,
                       density_covariance=base.density_covariance, mixture_offsets=base.mixture_offsets,
                       mixture_densities=base.mixture_densities, mixture_log_weights=base.mixture_log_weights)
    entry = [2, 6, 17, 23]  # one entry of each mixture
    frames = ms.means[ms.density_mean[ms.mixture_densities[entry]]].copy()
    sc = ra.Scorer(ms, "diagonal-sum", max_frames=4)
    pf, pm = np.arange(4, dtype=np.uint32), np.arange(4, dtype=np.uint32)
    post, logden = device_posteriors(gpu, sc, frames, pf, pm)
    check_posteriors(ms, pr.SumModel(ms), frames, pf, pm, post, logden, 6, "underflow")
    for i, e in enumerate(entry):
        j = e - 6 * i
        assert post[i, j] == 1.0
        assert (np.delete(post[i], j) < 2.0 ** -126).all()


def test_posterior_errors(gpu):
    ms = ra.synthetic_mixture_set(8, _counts(8, 1, 9, 2), 39, seed=81)
    frames = ra.synthetic_frames(6, 39, seed=82)
    pf, pm = _all_pairs(6, 8)
    for kind in ["SIMD-diagonal-maximum", "diagonal-maximum", "batch-diagonal-maximum-int"]:
        sc = ra.Scorer(ms, kind, max_frames=8)
        assert code(lambda: device_posteriors(gpu, sc, frames, pf, pm, 16)) == _capi.GMM_ERR_UNSUPPORTED
        assert code(lambda: sc.density_posteriors(frames, pf, pm, 16)) == _capi.GMM_ERR_UNSUPPORTED
    sc = ra.Scorer(ms, "diagonal-sum", max_frames=8)
    K = _k_max(ms)
    assert code(lambda: device_posteriors(gpu, sc, frames, pf, pm, K - 1)) == _capi.GMM_ERR_CAPACITY
    assert code(lambda: sc.density_posteriors(frames, pf, pm, K - 1)) == _capi.GMM_ERR_CAPACITY
    assert code(lambda: sc.density_posteriors(frames[:, :38], pf, pm, K)) == _capi.GMM_ERR_INVALID_ARGUMENT
    empty = sc.density_posteriors(frames, [], [], K)
    assert empty[0].shape == (0, K) and empty[1].shape == (0,)


# ---------------------------------------------------------------------------------------------------------------
# B. accumulation
# ---------------------------------------------------------------------------------------------------------------

def expected(gpu, sc, top, frames, pf, pm, pw, threshold=THR, tables=None, chunk=pr.CHUNK):
    """(tables, skipped, live contributions, contributions, their f64 weights before the threshold) of one call, from
    the device's own posteriors."""
    post, _ = device_posteriors(gpu, sc, frames, pf, pm)
    fr, en, we, skipped, total = pr.expand(top, frames.shape[0], pf, pm, pw, post, threshold)
    all_w = pr.expand(top, frames.shape[0], pf, pm, pw, post, -np.inf)[2]
    return pr.accumulate(top, frames, fr, en, we, tables, chunk), skipped, len(we), total, all_w


def random_pairs(top, n_frames, n, seed):
    rng = np.random.default_rng(seed)
    counts = np.diff(top.mixture_offsets.astype(np.int64))
    pm = rng.choice(np.nonzero(counts > 0)[0], size=n).astype(np.uint32)
    pf = rng.integers(0, n_frames, size=n).astype(np.uint32)
    return pf, pm


@pytest.fixture(scope="module")
def case1(gpu):
    """12 mixtures of 0..9 densities (mixture 4 empty), D = 39, 3 covariances, 50 frames, 200 pairs; weights with 0,
    1e-9, 1 and 1e6 among them."""
    counts = np.array([3, 9, 1, 5, 0, 7, 2, 9, 4, 6, 8, 1])
    top = ra.synthetic_mixture_set(12, counts, 39, seed=11, n_covariances=3, weights="random")
    frames = ra.synthetic_frames(50, 39, seed=12)
    pf, pm = random_pairs(top, 50, 200, 13)
    pw = np.random.default_rng(14).uniform(0.0, 2.0, size=200)
    pw[[3, 77, 150]] = 0.0
    pw[[5, 90]] = 1e-9
    pw[[8, 120]] = 1.0
    pw[[11, 160]] = 1e6
    sc = ra.Scorer(top, "diagonal-sum", max_frames=50)
    ref, skipped, live, total, all_w = expected(gpu, sc, top, frames, pf, pm, pw)
    assert skipped == 0 and 0 < live < total
    return dict(top=top, frames=frames, pf=pf, pm=pm, pw=pw, sc=sc, ref=ref, live=live, total=total, all_w=all_w, K=9)


def test_case1_default_threshold_and_file(gpu, case1):
    c = case1
    e = ra.Estimator(c["top"], max_pairs=200 * c["K"])
    assert accumulate_posteriors(gpu, e, c["frames"], c["pf"], c["pm"], c["pw"], c["sc"], stride=48) == 0
    got = e.get()
    pr.assert_bit_equal(got, c["ref"])
    assert np.isclose(got["entry_weights"].sum(), c["all_w"][c["all_w"] > THR].sum(), rtol=1e-12)
    # unweighted: every pair hands out about one unit
    ref1, _, _, _, _ = expected(gpu, c["sc"], c["top"], c["frames"], c["pf"], c["pm"], None)
    e.reset()
    accumulate_posteriors(gpu, e, c["frames"], c["pf"], c["pm"], None, c["sc"])
    pr.assert_bit_equal(e.get(), ref1)
    assert abs(e.get()["entry_weights"].sum() - 200) < 1e-3
    # the file (its estimate: test_shared_mean_topology; a file with an empty mixture, as this one, has none)
    assert e.to_bytes() == pr.expected_file(c["top"], ref1)


def test_shared_mean_topology(gpu):
    """Densities 1 and 2 of mixture 1 share mean 0: its contributions arrive in density order within a pair."""
    rng = np.random.default_rng(21)
    D = 11
    top = ra.MixtureSet(means=rng.standard_normal((4, D)).astype(np.float32),
                        variances=(0.5 + rng.random((2, D))).astype(np.float32),
                        density_mean=[2, 0, 0, 1, 3], density_covariance=[1, 0, 0, 1, 0],
                        mixture_offsets=[0, 2, 4, 5], mixture_densities=[3, 1, 2, 3, 0],
                        mixture_log_weights=np.log([0.5, 0.5, 0.5, 0.5, 1.0]))
    frames = ra.synthetic_frames(30, D, seed=22)
    pf, pm = random_pairs(top, 30, 150, 23)
    pw = np.random.default_rng(24).uniform(0.0, 2.0, size=150)
    sc = ra.Scorer(top, "diagonal-sum", max_frames=30)
    ref, skipped, live, total, _ = expected(gpu, sc, top, frames, pf, pm, pw)
    assert skipped == 0 and total == 150 + int((pm < 2).sum())
    e = ra.Estimator(top, max_pairs=300)
    assert accumulate_posteriors(gpu, e, frames, pf, pm, pw, sc) == 0
    got = e.get()
    pr.assert_bit_equal(got, ref)
    assert got["mean_weights"][0] == pytest.approx(got["entry_weights"][1] + got["entry_weights"][2], rel=1e-12)
    want = pr.expected_file(top, ref)
    assert e.to_bytes() == want
    # and it reads back: the estimate of the handle is the estimate of the restatement's file
    ms = e.estimate(minimum_observation_weight=0.0)
    ref_ms = ra.estimate_mixture_set(want, minimum_observation_weight=0.0)
    assert np.array_equal(ms.means.view(np.uint32), ref_ms.means.view(np.uint32))
    assert np.array_equal(ms.variances.view(np.uint32), ref_ms.variances.view(np.uint32))
    assert np.array_equal(ms.mixture_densities, ref_ms.mixture_densities)


@pytest.mark.parametrize("D", [39, 80])
def test_piece_rule(gpu, D):
    """One covariance, one mixture of three densities, 700 pairs on frames between the means: all three posteriors
    pass, so every mean gets 700 > 512 contributions and the covariance 2100."""
    top = ra.synthetic_mixture_set(1, 3, D, seed=31)
    rng = np.random.default_rng(32 + D)
    a = 1.0 / 3 + rng.uniform(-0.02, 0.02, size=(300, 3))
    frames = ((a / a.sum(axis=1, keepdims=True)) @ top.means.astype(np.float64)
              + 0.05 * rng.standard_normal((300, D))).astype(np.float32)
    pf = rng.integers(0, 300, size=700).astype(np.uint32)
    pm = np.zeros(700, np.uint32)
    pw = rng.uniform(0.5, 2.0, size=700)
    sc = ra.Scorer(top, "diagonal-sum", max_frames=300)
    ref, skipped, live, total, all_w = expected(gpu, sc, top, frames, pf, pm, pw)
    assert skipped == 0 and live == total == 2100 and (all_w > THR).all()
    seq = expected(gpu, sc, top, frames, pf, pm, pw, chunk=None)[0]
    for k in ["mean_sums", "covariance_sums"]:
        assert (ref[k] != seq[k]).any(), k  # a kernel that summed sequentially would not pass below
    e = ra.Estimator(top, max_pairs=2100)
    assert accumulate_posteriors(gpu, e, frames, pf, pm, pw, sc) == 0
    pr.assert_bit_equal(e.get(), ref)


def test_thresholds(gpu, case1):
    c = case1
    top, frames, pf, pm, pw, sc = (c[k] for k in ["top", "frames", "pf", "pm", "pw", "sc"])
    e = ra.Estimator(top, max_pairs=1800)
    # 0.25
    ref, _, live, _, _ = expected(gpu, sc, top, frames, pf, pm, pw, 0.25)
    assert 0 < live < c["live"]
    assert accumulate_posteriors(gpu, e, frames, pf, pm, pw, sc, threshold=0.25) == 0
    pr.assert_bit_equal(e.get(), ref)
    # exactly one occurring finalWeight: the compare is strict, that contribution stays out
    t = float(np.sort(c["all_w"][c["all_w"] > THR])[c["live"] // 2])
    ref_t, _, live_t, _, _ = expected(gpu, sc, top, frames, pf, pm, pw, t)
    assert live_t == int((c["all_w"] > t).sum()) < int((c["all_w"] >= t).sum())
    e.reset()
    accumulate_posteriors(gpu, e, frames, pf, pm, pw, sc, threshold=t)
    pr.assert_bit_equal(e.get(), ref_t)
    below = expected(gpu, sc, top, frames, pf, pm, pw, np.nextafter(t, 0.0))[0]
    assert (below["entry_weights"] != ref_t["entry_weights"]).any()  # a >= compare would have given this
    # a NaN weight passes no threshold, and is no skip
    pn = pw.copy()
    pn[20] = np.nan
    ref_n = expected(gpu, sc, top, frames, pf, pm, pn, -1.0)[0]
    e.reset()
    assert accumulate_posteriors(gpu, e, frames, pf, pm, pn, sc, threshold=-1.0) == 0
    pr.assert_bit_equal(e.get(), ref_n)
    assert not np.isnan(e.get()["entry_weights"]).any()


def test_mixed_calls_and_reset(gpu, case1):
    c = case1
    top, frames, pf, pm, pw, sc = (c[k] for k in ["top", "frames", "pf", "pm", "pw", "sc"])
    e = ra.Estimator(top, max_pairs=1800)
    h = 100
    t1 = expected(gpu, sc, top, frames, pf[:h], pm[:h], pw[:h])[0]
    t2 = expected(gpu, sc, top, frames, pf[h:], pm[h:], pw[h:], tables=t1)[0]
    accumulate_posteriors(gpu, e, frames, pf[:h], pm[:h], pw[:h], sc)
    accumulate_posteriors(gpu, e, frames, pf[h:], pm[h:], pw[h:], sc)
    pr.assert_bit_equal(e.get(), t2)
    # then a Viterbi call with given densities on the same handle
    counts = np.diff(top.mixture_offsets.astype(np.int64))
    pd = (np.random.default_rng(15).integers(0, 1 << 30, size=200) % counts[pm]).astype(np.uint32)
    entry = top.mixture_offsets.astype(np.int64)[pm] + pd
    t3 = pr.accumulate(top, frames, pf.astype(np.int64), entry, pw, t2)
    assert accumulate_viterbi(gpu, e, frames, pf, pm, pd, pw) == 0
    pr.assert_bit_equal(e.get(), t3)
    e.reset()
    pr.assert_bit_equal(e.get(), pr.zero_tables(top))
    assert e.skipped == 0
    accumulate_posteriors(gpu, e, frames, pf, pm, pw, sc)
    pr.assert_bit_equal(e.get(), c["ref"])


def test_no_scorer_single_density(gpu, case1):
    c = case1
    single = ra.synthetic_mixture_set(6, 1, 39, seed=6)
    f1, m1 = c["pf"][:64], (c["pm"][:64] % 6).astype(np.uint32)
    w1 = np.random.default_rng(16).uniform(0.0, 2.0, size=64)
    w1[:6] = [0.0, THR, np.nextafter(THR, 1.0), 1e-9, 1.0, 1e6]
    keep = w1 > THR
    assert keep.sum() == 61 and keep[2] and not keep[1]
    e = ra.Estimator(single, max_pairs=64)  # K_max is 1 without a scorer
    assert accumulate_posteriors(gpu, e, c["frames"], f1, m1, w1) == 0
    v = ra.Estimator(single, max_pairs=64)
    accumulate_viterbi(gpu, v, c["frames"], f1[keep], m1[keep], np.zeros(61, np.uint32), w1[keep])
    pr.assert_bit_equal(e.get(), v.get())
    entry = single.mixture_offsets.astype(np.int64)[m1[keep]]
    pr.assert_bit_equal(e.get(), pr.accumulate(single, c["frames"], f1[keep].astype(np.int64), entry, w1[keep]))
    # bad pairs are counted, weights under the threshold are not
    assert accumulate_posteriors(gpu, e, c["frames"], [50, 1, 2], [0, 6, 3], [1.0, 1.0, 0.0]) == 2


def test_host_call(gpu, case1):
    c = case1
    top, frames, pw, sc = c["top"], c["frames"], c["pw"], c["sc"]
    # bad pairs and pairs on the empty mixture 4 among the good ones
    pf = np.concatenate([[50, 3], c["pf"], [7, 1 << 30]]).astype(np.uint32)
    pm = np.concatenate([[0, 4], c["pm"], [12, 2]]).astype(np.uint32)
    pw = np.concatenate([[1.0, 1.0], pw, [1.0, 1.0]])
    e = ra.Estimator(top, max_pairs=204 * 9)
    padded = np.zeros((50, 44), np.float32)
    padded[:, :39] = frames
    e.accumulate_posteriors_host(padded, pf, pm, pw, scorer=sc)
    d = ra.Estimator(top, max_pairs=204 * 9)
    assert accumulate_posteriors(gpu, d, frames, pf, pm, pw, sc) == 4
    assert e.skipped == 4
    pr.assert_bit_equal(e.get(), d.get())
    pr.assert_bit_equal(d.get(), c["ref"])  # the four change nothing
    assert e.to_bytes() == d.to_bytes()


def test_errors_change_nothing(gpu, case1):
    c = case1
    top, frames, pf, pm, pw, sc = (c[k] for k in ["top", "frames", "pf", "pm", "pw", "sc"])
    e = ra.Estimator(top, max_pairs=204 * 9)
    sf = np.concatenate([[3, 50, 2], pf, [8]]).astype(np.uint32)
    sm = np.concatenate([[4, 1, 12], pm, [4]]).astype(np.uint32)
    sw = np.concatenate([[1.0, 1.0, 1.0], pw, [1.0]])
    assert accumulate_posteriors(gpu, e, frames, sf, sm, sw, sc) == 4  # once per pair, not per density
    pr.assert_bit_equal(e.get(), c["ref"])
    before = e.get()
    for kind in ["SIMD-diagonal-maximum", "diagonal-maximum"]:
        other = ra.Scorer(top, kind, max_frames=50)
        assert code(lambda: accumulate_posteriors(gpu, e, frames, pf, pm, pw, other)) == _capi.GMM_ERR_UNSUPPORTED
        assert code(lambda: e.accumulate_posteriors_host(frames, pf, pm, pw, scorer=other)) == _capi.GMM_ERR_UNSUPPORTED
    small = ra.Estimator(top, max_pairs=200 * 9 - 1)  # n_pairs * K_max > max_pairs
    assert code(lambda: accumulate_posteriors(gpu, small, frames, pf, pm, pw, sc)) == _capi.GMM_ERR_CAPACITY
    assert code(lambda: small.accumulate_posteriors_host(frames, pf, pm, pw, scorer=sc)) == _capi.GMM_ERR_CAPACITY
    pr.assert_bit_equal(small.get(), pr.zero_tables(top))
    wrong = ra.Scorer(ra.synthetic_mixture_set(12, 3, 39, seed=5), "diagonal-sum", max_frames=50)
    assert code(lambda: accumulate_posteriors(gpu, e, frames, pf, pm, pw, wrong)) == _capi.GMM_ERR_INVALID_ARGUMENT
    shard = ra.Scorer(top, "diagonal-sum", max_frames=50, mixture_range=(2, 8))
    assert code(lambda: accumulate_posteriors(gpu, e, frames, pf, pm, pw, shard)) == _capi.GMM_ERR_UNSUPPORTED
    assert code(lambda: accumulate_posteriors(gpu, e, frames, pf, pm, pw)) == _capi.GMM_ERR_INVALID_ARGUMENT  # cc:398
    pr.assert_bit_equal(e.get(), before)
    assert e.skipped == 4
