"""Joint numerator / denominator accumulation for discriminative training on the device:
gmm_estimator_accumulate_discriminative_* (rasr_amd/csrc/gmm_kernels_accum.hip with two sides, include/rasr_gmm_estimator.h
"Discriminative training"), against the plain-numpy restatement of the contract in tests/ebw_restatement.py.

Everything is compared bit for bit: both sides run the same IEEE f64 operations in the same order.  The only
inequality is the distance of the joint-piece sum from the sequential sum beyond GMM_ESTIMATOR_CHUNK contributions,
bounded as for the maximum-likelihood calls by 2 n 2^-53 sum|term| (n rounded adds, each regrouping moving the sum by
at most an ulp of a partial sum).
"""
import numpy as np
import pytest

import ebw_restatement as er
import rasr_amd as ra
from rasr_amd import _capi

pytestmark = pytest.mark.gpu

NAN = np.nan
COUNTS = [1, 4, 2, 3, 1, 2]  # the ragged model of 6 mixtures
KEYS = ("mean_sums", "mean_weights", "covariance_sums", "covariance_weights", "entry_weights")


def _ints(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(gpu)


def _f64(gpu, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(gpu)


def _frames(gpu, frames, stride=None):
    import torch
    D = frames.shape[1]
    x = torch.zeros((frames.shape[0], stride or D), dtype=torch.float32, device=gpu)
    x[:, :D] = torch.from_numpy(np.ascontiguousarray(frames)).to(gpu)
    return x


def disc(gpu, e, frames, pf, pm, pd, wn, wd, scorer=None, stride=None):
    import torch
    args = (_frames(gpu, frames, stride), _ints(gpu, pf), _ints(gpu, pm), None if pd is None else _ints(gpu, pd),
            _f64(gpu, wn), _f64(gpu, wd))
    torch.cuda.synchronize()
    e.accumulate_discriminative_device(*args, scorer=scorer)
    return e.skipped  # waits for the call: the tensors may go


def disc_posteriors(gpu, e, frames, pf, pm, wn, wd, scorer=None, threshold=None):
    import torch
    args = (_frames(gpu, frames), _ints(gpu, pf), _ints(gpu, pm), _f64(gpu, wn), _f64(gpu, wd))
    torch.cuda.synchronize()
    e.accumulate_discriminative_posteriors_device(*args, scorer=scorer, weight_threshold=threshold)
    return e.skipped


def ml(gpu, e, frames, pf, pm, pd, pw):
    import torch
    args = (_frames(gpu, frames), _ints(gpu, pf), _ints(gpu, pm), _ints(gpu, pd), _f64(gpu, pw))
    torch.cuda.synchronize()
    e.accumulate_device(*args)
    return e.skipped


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint64), np.asarray(b[k], dtype=np.float64).view(np.uint64)) for k in KEYS)


def code(fn):
    with pytest.raises(ra.GmmError) as err:
        fn()
    return err.value.code


def entries_of(ms, pm, pd):
    return ms.mixture_offsets.astype(np.int64)[pm] + pd


def viterbi_case(ms, n, n_frames, seed, absent=True):
    """n good pairs with a density each and two weight lists; with `absent`, NaN on one or both sides here and there."""
    rng = np.random.default_rng(seed)
    counts = np.diff(ms.mixture_offsets.astype(np.int64))
    pf = rng.integers(0, n_frames, n).astype(np.uint32)
    pm = rng.integers(0, len(counts), n).astype(np.uint32)
    pd = (rng.integers(0, 1 << 20, n) % counts[pm]).astype(np.uint32)
    wn, wd = rng.uniform(-1, 2, n), rng.uniform(0, 3, n)
    if absent:
        wn[rng.random(n) < 0.25] = NAN
        wd[rng.random(n) < 0.25] = NAN
        wn[7], wd[7] = NAN, NAN  # on neither side
        wn[8] = 0.0              # a zero weight is live
    return pf, pm, pd, wn, wd


# ---------------------------------------------------------------------------------------------------------------
# equality with the sequential restatement and with two maximum-likelihood handles
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,n_cov", [(1, 1), (39, 1), (64, 1), (65, 1), (130, 1), (39, 3)])
def test_equals_sequential_and_two_ml_handles(gpu, dim, n_cov):
    ms = ra.synthetic_mixture_set(6, COUNTS, dim, seed=3 + dim, n_covariances=n_cov)
    F, n = 40, 300
    frames = ra.synthetic_frames(F, dim, seed=11)
    e = ra.Estimator(ms, 512)
    e_num, e_den = ra.Estimator(ms, 512), ra.Estimator(ms, 512)
    num, den = er.zero_tables(ms), er.zero_tables(ms)
    prev = (er.zero_tables(ms), er.zero_tables(ms))
    skipped = 0
    for call in range(2):  # the second call starts from the first one's tables
        pf, pm, pd, wn, wd = viterbi_case(ms, n, F, 100 * dim + call)
        # bad pairs: frame, mixture, density out of range -- counted once each
        pf[20], pm[21], pd[22] = F, 6, 4
        skipped += 3
        assert disc(gpu, e, frames, pf, pm, pd, wn, wd, stride=dim + 3) == skipped
        g = np.ones(n, dtype=bool)
        g[20:23] = False
        ent, fr, a, b = entries_of(ms, pm[g], pd[g]), pf[g], wn[g], wd[g]
        num, den = er.sequential(ms, frames, ent, fr, a, num), er.sequential(ms, frames, ent, fr, b, den)
        prev = er.joint(ms, frames, ent, fr, a, b, *prev)
        for eh, w in ((e_num, wn), (e_den, wd)):
            keep = ~np.isnan(w)
            ml(gpu, eh, frames, pf[keep], pm[keep], pd[keep], w[keep])
    got_num, got_den = e.get(), e.get_denominator()
    assert same(got_num, num) and same(got_den, den)          # the reference's sequential loop, per side
    assert same(got_num, prev[0]) and same(got_den, prev[1])  # at most 512 per accumulator: the joint rule is that loop
    assert same(got_num, e_num.get()) and same(got_den, e_den.get())
    assert got_den["covariance_weights"].sum() > 0 and not same(got_num, got_den)
    # the host form: the same bits
    h = ra.Estimator(ms, 512)
    for call in range(2):
        pf, pm, pd, wn, wd = viterbi_case(ms, n, F, 100 * dim + call)
        pf[20], pm[21], pd[22] = F, 6, 4
        h.accumulate_discriminative_host(frames, pf, pm, pd, wn, wd)
    assert same(h.get(), got_num) and same(h.get_denominator(), got_den) and h.skipped == skipped


def test_sidedness(gpu):
    ms = ra.synthetic_mixture_set(6, COUNTS, 39, seed=4)
    F, n = 40, 300
    frames = ra.synthetic_frames(F, 39, seed=12)
    pf, pm, pd, wn, wd = viterbi_case(ms, n, F, 5, absent=False)
    e, ref = ra.Estimator(ms, 512), ra.Estimator(ms, 512)
    # something in both table sets first
    disc(gpu, e, frames, pf, pm, pd, wd, wn)
    ml(gpu, ref, frames, pf, pm, pd, wd)
    n0, d0 = e.get(), e.get_denominator()
    # no denominator weights: the denominator tables stay, the numerator is the maximum-likelihood call
    disc(gpu, e, frames, pf, pm, pd, wn, None)
    ml(gpu, ref, frames, pf, pm, pd, wn)
    n1 = e.get()
    assert same(e.get_denominator(), d0) and same(n1, ref.get()) and not same(n1, n0)
    # the mirror: the denominator after (wn, then wd) equals a maximum-likelihood handle fed the same two lists
    ref_d = ra.Estimator(ms, 512)
    ml(gpu, ref_d, frames, pf, pm, pd, wn)
    ml(gpu, ref_d, frames, pf, pm, pd, wd)
    disc(gpu, e, frames, pf, pm, pd, None, wd)
    assert same(e.get(), n1) and same(e.get_denominator(), ref_d.get())
    # one pair, weight on one side only
    d1 = e.get_denominator()
    one = (pf[:1], pm[:1], pd[:1])
    disc(gpu, e, frames, *one, np.array([0.5]), np.array([NAN]))
    n2 = e.get()
    assert same(e.get_denominator(), d1) and not same(n2, n1)
    disc(gpu, e, frames, *one, np.array([NAN]), np.array([0.5]))
    assert same(e.get(), n2) and not same(e.get_denominator(), d1)
    assert e.skipped == 0


# ---------------------------------------------------------------------------------------------------------------
# pieces: more than GMM_ESTIMATOR_CHUNK joint contributions on the pooled covariance
# ---------------------------------------------------------------------------------------------------------------

def piece_case(n):
    ms = ra.synthetic_mixture_set(6, COUNTS, 39, seed=6)  # one covariance: every pair lands on it
    F = 64
    frames = ra.synthetic_frames(F, 39, seed=13)
    pf, pm, pd, wn, wd = viterbi_case(ms, n, F, 1000 + n, absent=False)
    i = np.arange(n)
    wd[i % 3 == 0] = NAN                      # every third pair numerator-only
    wn[(i % 3 != 0) & (i % 5 == 0)] = NAN     # every fifth denominator-only
    return ms, frames, pf, pm, pd, wn, wd


@pytest.mark.parametrize("n", [511, 512, 513, 1025, 1600])
def test_pieces(gpu, n):
    ms, frames, pf, pm, pd, wn, wd = piece_case(n)
    assert _capi.GMM_ESTIMATOR_CHUNK == er.CHUNK == 512
    ent = entries_of(ms, pm, pd)
    z = er.zero_tables(ms)
    jn, jd = er.joint(ms, frames, ent, pf, wn, wd, z, z)
    if n > 513:
        # the test shows something only if the pieces cut from the joint list are not the pieces a side would cut
        # from its own list (at 513 the second joint piece holds one contribution, and 0 + x is x)
        own_n = er.joint(ms, frames, ent, pf, wn, None, z, z)[0]
        own_d = er.joint(ms, frames, ent, pf, None, wd, z, z)[1]
        assert not same(jn, own_n) and not same(jd, own_d)
    e = ra.Estimator(ms, 1600)
    assert disc(gpu, e, frames, pf, pm, pd, wn, wd) == 0
    got_n, got_d = e.get(), e.get_denominator()
    assert same(got_n, jn) and same(got_d, jd)
    for got, w in ((got_n, wn), (got_d, wd)):
        seq = er.sequential(ms, frames, ent, pf, w, z)
        if n <= 512:
            assert same(got, seq)
        cnt, mag = er.abs_term_sums(ms, frames, ent, pf, w)
        live = int((~np.isnan(w)).sum())
        assert cnt["cov"][0] == live
        worst = 0.0
        for key, c in (("mean_sums", cnt["mean"][:, None]), ("covariance_sums", cnt["cov"][:, None])):
            bound = 2.0 * c * 2.0 ** -53 * mag[key]
            diff = np.abs(got[key] - seq[key])
            assert (diff <= bound).all()
            worst = max(worst, float((diff / np.maximum(bound, 1e-300)).max()))
        wbound = 2.0 * live * 2.0 ** -53 * np.abs(w[~np.isnan(w)]).sum()
        assert abs(got["covariance_weights"][0] - seq["covariance_weights"][0]) <= wbound
        print(f"n = {n}: max |joint - sequential| = {worst:.3f} of the bound")


# ---------------------------------------------------------------------------------------------------------------
# one kernel family, two meanings of a weight: the maximum-likelihood call's and the joint call's
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 65])  # 65: a second lane block
def test_nan_weight_keeps_its_two_meanings(gpu, dim):
    """A NaN weight is a value to the maximum-likelihood call (it poisons its destinations) and "not live" to the joint
    call (nothing is added).  513 pairs on one mean, so two pieces and a combine; the NaN pair sits in the second."""
    ms = ra.synthetic_mixture_set(6, COUNTS, dim, seed=40 + dim)  # one covariance: every pair lands on it
    F = 32
    frames = ra.synthetic_frames(F, dim, seed=17)
    rng = np.random.default_rng(41 + dim)
    # entry 0 (mixture 0, density 0) takes 513 pairs; six pairs of other entries in between
    others = {3: (1, 2), 100: (2, 0), 300: (3, 1), 400: (1, 0), 515: (5, 1), 517: (4, 0)}
    n = 513 + len(others)
    pm, pd = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for at, (m, d) in others.items():
        pm[at], pd[at] = m, d
    pf = rng.integers(0, F, n).astype(np.uint32)
    w = rng.uniform(0.5, 2, n)
    ent = entries_of(ms, pm, pd)
    mean_of = ms.density_mean[ms.mixture_densities[ent]].astype(np.int64)
    heavy = np.flatnonzero(ent == 0)
    assert len(heavy) == 513 and (mean_of[ent != 0] != mean_of[0]).all() and ms.n_covariances == 1
    bad = heavy[-1]  # the 513th pair of its mean and of its entry, and in the second piece of the covariance
    assert bad >= 512
    w[bad] = NAN
    z = er.zero_tables(ms)

    e = ra.Estimator(ms, n)
    assert ml(gpu, e, frames, pf, pm, pd, w) == 0
    got = e.get()
    seq = er.sequential(ms, frames, ent, pf, w, z)  # the live rows: right wherever the NaN pair does not land
    hit = {"mean_sums": mean_of[0], "mean_weights": mean_of[0], "covariance_sums": 0, "covariance_weights": 0,
           "entry_weights": 0}
    for key in KEYS:
        poisoned = np.zeros(len(got[key]), dtype=bool)
        poisoned[hit[key]] = True
        assert np.isnan(got[key][poisoned]).all(), key
        assert np.array_equal(got[key][~poisoned].view(np.uint64), seq[key][~poisoned].view(np.uint64)), key

    j = ra.Estimator(ms, n)
    assert disc(gpu, j, frames, pf, pm, pd, w, None) == 0
    keep = np.arange(n) != bad
    want = er.joint(ms, frames, ent[keep], pf[keep], w[keep], None, z, z)[0]
    got = j.get()
    assert same(got, want) and not any(np.isnan(got[k]).any() for k in KEYS)
    assert same(j.get_denominator(), z)


@pytest.mark.parametrize("n", [513, 1600])
def test_one_sided_joint_call_is_a_maximum_likelihood_call(gpu, n):
    """With one side and no absent pair the joint piece cut is the side's own cut: bit-equal beyond 512 too."""
    ms = ra.synthetic_mixture_set(6, COUNTS, 39, seed=6)
    F = 64
    frames = ra.synthetic_frames(F, 39, seed=13)
    pf, pm, pd, w, _ = viterbi_case(ms, n, F, 2000 + n, absent=False)
    ref = ra.Estimator(ms, n)
    assert ml(gpu, ref, frames, pf, pm, pd, w) == 0
    want = ref.get()
    assert want["covariance_weights"][0] != 0
    z = er.zero_tables(ms)
    num = ra.Estimator(ms, n)
    assert disc(gpu, num, frames, pf, pm, pd, w, None) == 0
    assert same(num.get(), want) and same(num.get_denominator(), z)
    den = ra.Estimator(ms, n)
    assert disc(gpu, den, frames, pf, pm, pd, None, w) == 0
    assert same(den.get_denominator(), want) and same(den.get(), z)


# ---------------------------------------------------------------------------------------------------------------
# posterior mode
# ---------------------------------------------------------------------------------------------------------------

def test_posterior_mode(gpu):
    counts = [7, 1, 3, 5, 2, 4]  # K_max = 7
    ms = ra.synthetic_mixture_set(6, counts, 39, seed=8, weights="random")
    F, thr = 20, 0.2  # 120 pairs: at most 440 slots, so at most 512 on the pooled covariance
    frames = ra.synthetic_frames(F, 39, seed=14)
    sc = ra.Scorer(ms, "diagonal-sum", max_frames=F)
    f, m = np.meshgrid(np.arange(F, dtype=np.uint32), np.arange(6, dtype=np.uint32), indexing="ij")
    pf = np.concatenate([f.ravel(), [F, 0, 0xFFFFFFFF]]).astype(np.uint32)  # three bad pairs
    pm = np.concatenate([m.ravel(), [0, 6, 0xFFFFFFFF]]).astype(np.uint32)
    n = len(pf)
    rng = np.random.default_rng(15)
    wn, wd = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    wn[5], wd[6] = NAN, 0.0
    post = sc.density_posteriors(frames, pf, pm, 7)[0]
    ent, fr, a, b, bad = er.posterior_rows(ms, pf, pm, F, post, wn, wd, thr)
    la, lb = ~np.isnan(a), ~np.isnan(b)
    # slots live on the numerator only, on the denominator only, on both and on neither
    assert min((la & ~lb).sum(), (~la & lb).sum(), (la & lb).sum(), (~la & ~lb).sum()) >= 5
    assert bad == 3
    z = er.zero_tables(ms)
    jn, jd = er.joint(ms, frames, ent, fr, a, b, z, z)
    e = ra.Estimator(ms, n * 7)
    assert disc_posteriors(gpu, e, frames, pf, pm, wn, wd, scorer=sc, threshold=thr) == 3  # a bad pair counts once
    assert same(e.get(), jn) and same(e.get_denominator(), jd)
    # each side is what the maximum-likelihood posterior call makes of its weights (at most 512 per accumulator here)
    assert same(jn, er.sequential(ms, frames, ent, fr, a, z)) and same(jd, er.sequential(ms, frames, ent, fr, b, z))
    for side, w in ((e.get(), wn), (e.get_denominator(), wd)):
        r = ra.Estimator(ms, n * 7)
        import torch
        r.accumulate_posteriors_device(_frames(gpu, frames), _ints(gpu, pf), _ints(gpu, pm), _f64(gpu, np.nan_to_num(w)),
                                       scorer=sc, weight_threshold=thr)
        torch.cuda.synchronize()
        assert same(side, r.get())
    # one side alone, and the host form
    e1 = ra.Estimator(ms, n * 7)
    disc_posteriors(gpu, e1, frames, pf, pm, None, wd, scorer=sc, threshold=thr)
    assert same(e1.get(), z) and same(e1.get_denominator(), jd)
    h = ra.Estimator(ms, n * 7)
    h.accumulate_discriminative_posteriors_host(frames, pf, pm, wn, wd, scorer=sc, weight_threshold=thr)
    assert same(h.get(), jn) and same(h.get_denominator(), jd) and h.skipped == 3


def test_infinite_row_stays_on_its_side(gpu):
    """A frame row holding inf, live on one side only: the other side adds nothing, not 0 * inf."""
    ms = ra.synthetic_mixture_set(4, 1, 5, seed=9)  # one density per mixture: no scorer, posterior 1
    frames = ra.synthetic_frames(6, 5, seed=16)
    frames[2, 3] = np.inf
    pf = np.array([0, 2, 1, 2], dtype=np.uint32)
    pm = np.array([0, 1, 1, 3], dtype=np.uint32)
    wn = np.array([0.5, 0.75, 0.25, 0.01])
    wd = np.array([0.5, 0.01, 0.25, 0.75])  # 0.01 is under the threshold
    e = ra.Estimator(ms, 16)
    assert disc_posteriors(gpu, e, frames, pf, pm, wn, wd, threshold=0.1) == 0
    ent, fr, a, b, _ = er.posterior_rows(ms, pf, pm, 6, np.ones((4, 1), np.float32), wn, wd, 0.1)
    z = er.zero_tables(ms)
    jn, jd = er.joint(ms, frames, ent, fr, a, b, z, z)
    got_n, got_d = e.get(), e.get_denominator()
    assert same(got_n, jn) and same(got_d, jd)
    assert np.isinf(got_n["mean_sums"][1, 3]) and np.isfinite(got_d["mean_sums"][1]).all()
    assert np.isinf(got_d["mean_sums"][3, 3]) and np.isfinite(got_n["mean_sums"][3]).all()
    # the Viterbi form, the absent side marked by NaN
    v = ra.Estimator(ms, 16)
    disc(gpu, v, frames, pf, pm, None, np.where(np.isnan(a), NAN, wn), np.where(np.isnan(b), NAN, wd))
    assert same(v.get(), jn) and same(v.get_denominator(), jd)


# ---------------------------------------------------------------------------------------------------------------
# mixed use, refusals, determinism, files
# ---------------------------------------------------------------------------------------------------------------

def test_mixed_use_and_reset(gpu):
    ms = ra.synthetic_mixture_set(6, COUNTS, 39, seed=4)
    F, n = 40, 200
    frames = ra.synthetic_frames(F, 39, seed=12)
    pf, pm, pd, wn, wd = viterbi_case(ms, n, F, 21)
    ent = entries_of(ms, pm, pd)
    e = ra.Estimator(ms, 512)
    z = er.zero_tables(ms)
    assert same(e.get_denominator(), z)  # before any discriminative call
    ml(gpu, e, frames, pf, pm, pd, np.nan_to_num(wn))
    num = er.sequential(ms, frames, ent, pf, np.nan_to_num(wn), z)
    disc(gpu, e, frames, pf, pm, pd, wn, wd)
    num, den = er.sequential(ms, frames, ent, pf, wn, num), er.sequential(ms, frames, ent, pf, wd, z)
    ml(gpu, e, frames, pf, pm, pd, np.nan_to_num(wd))  # a maximum-likelihood call adds to the numerator tables
    num = er.sequential(ms, frames, ent, pf, np.nan_to_num(wd), num)
    e.accumulate_objective(1.5)
    e.accumulate_objective(-0.25)
    assert same(e.get(), num) and same(e.get_denominator(), den) and e.objective == 1.25
    e.reset()
    assert same(e.get(), z) and same(e.get_denominator(), z) and e.objective == 0.0 and e.skipped == 0
    disc(gpu, e, frames, pf, pm, pd, wn, wd)
    assert same(e.get(), er.sequential(ms, frames, ent, pf, wn, z)) and same(e.get_denominator(), den)


def test_refusals_change_nothing(gpu):
    ms = ra.synthetic_mixture_set(6, COUNTS, 39, seed=4, weights="random")
    F, n = 40, 100
    frames = ra.synthetic_frames(F, 39, seed=12)
    pf, pm, pd, wn, wd = viterbi_case(ms, n, F, 22)
    pf[3] = F  # one skipped pair
    e = ra.Estimator(ms, 100)
    assert disc(gpu, e, frames, pf, pm, pd, wn, wd) == 1
    before = (e.get(), e.get_denominator())
    big = [np.concatenate([a, a[:1]]) for a in (pf, pm, pd, wn, wd)]
    assert code(lambda: disc(gpu, e, frames, *big)) == _capi.GMM_ERR_CAPACITY
    assert code(lambda: disc(gpu, e, frames, pf, pm, pd, None, None)) == _capi.GMM_ERR_INVALID_ARGUMENT
    assert code(lambda: e.accumulate_discriminative_host(frames, pf, pm, pd, None, None)) == _capi.GMM_ERR_INVALID_ARGUMENT
    sum_scorer = ra.Scorer(ms, "diagonal-sum", max_frames=F)
    max_scorer = ra.Scorer(ms, "SIMD-diagonal-maximum", max_frames=F)
    k = 25  # 25 * K_max = 100 slots fit, 26 do not
    assert code(lambda: disc_posteriors(gpu, e, frames, pf[:k + 1], pm[:k + 1], wn[:k + 1], wd[:k + 1],
                                        scorer=sum_scorer)) == _capi.GMM_ERR_CAPACITY
    assert code(lambda: disc_posteriors(gpu, e, frames, pf[:k], pm[:k], wn[:k], wd[:k],
                                        scorer=max_scorer)) == _capi.GMM_ERR_UNSUPPORTED
    assert code(lambda: disc_posteriors(gpu, e, frames, pf[:k], pm[:k], None, None,
                                        scorer=sum_scorer)) == _capi.GMM_ERR_INVALID_ARGUMENT
    assert code(lambda: e.accumulate_discriminative_posteriors_host(frames, pf[:k], pm[:k], None, None,
                                                                    scorer=sum_scorer)) == _capi.GMM_ERR_INVALID_ARGUMENT
    assert same(e.get(), before[0]) and same(e.get_denominator(), before[1]) and e.skipped == 1
    # a refused first call on a fresh handle leaves it a maximum-likelihood handle
    fresh = ra.Estimator(ms, 100)
    assert code(lambda: disc(gpu, fresh, frames, pf, pm, pd, None, None)) == _capi.GMM_ERR_INVALID_ARGUMENT
    assert same(fresh.get_denominator(), er.zero_tables(ms)) and fresh.skipped == 0
    # the posterior call that fits goes through
    assert disc_posteriors(gpu, e, frames, pf[:k], pm[:k], wn[:k], wd[:k], scorer=sum_scorer) == 2


def test_determinism_and_file_bytes(gpu):
    ms, frames, pf, pm, pd, wn, wd = piece_case(1600)
    files = []
    for _ in range(2):
        e = ra.Estimator(ms, 1600)
        disc(gpu, e, frames, pf, pm, pd, wn, wd)
        e.accumulate_objective(-3.75)
        files.append(e.to_bytes_discriminative())
    assert files[0] == files[1]
    z = er.zero_tables(ms)
    jn, jd = er.joint(ms, frames, entries_of(ms, pm, pd), pf, wn, wd, z, z)
    assert files[0] == er.write_file(ms, jn, jd, -3.75)
    # the maximum-likelihood bytes of the same handle hold the numerator only and are not this file
    assert e.to_bytes() != files[0] and ra.combine_estimators([e.to_bytes()]) == e.to_bytes()


def test_shards_written_and_combined(gpu, tmp_path):
    """Accumulate two shards, write both files, combine them: the file of the tables added in file order."""
    ms = ra.synthetic_mixture_set(6, COUNTS, 39, seed=4, n_covariances=3)
    F = 40
    frames = ra.synthetic_frames(F, 39, seed=12)
    z = er.zero_tables(ms)
    parts, paths = [], []
    for shard in range(2):
        pf, pm, pd, wn, wd = viterbi_case(ms, 300, F, 30 + shard)
        e = ra.Estimator(ms, 512)
        disc(gpu, e, frames, pf, pm, pd, wn, wd)
        e.accumulate_objective(0.1 * (shard + 1))
        paths.append(tmp_path / f"shard{shard}.mix")
        e.write_discriminative(paths[-1])
        ent = entries_of(ms, pm, pd)
        parts.append((er.sequential(ms, frames, ent, pf, wn, z), er.sequential(ms, frames, ent, pf, wd, z)))
        assert paths[-1].read_bytes() == er.write_file(ms, *parts[-1], 0.1 * (shard + 1))
    got = ra.combine_discriminative_estimators([p.read_bytes() for p in paths])
    num = {k: parts[0][0][k] + parts[1][0][k] for k in KEYS}
    den = {k: parts[0][1][k] + parts[1][1][k] for k in KEYS}
    assert got == er.write_file(ms, num, den, 0.1 + 0.2)


@pytest.mark.parametrize("kind", ["global-rwth", "local-rwth"])
def test_end_to_end_estimate(gpu, tmp_path, kind):
    """Accumulate two shards, write them, combine, estimate: the model is the restatement's estimate of the restated
    tables.  The handle form on one handle that saw both shards: the same from its own tables."""
    prev = ra.synthetic_mixture_set(6, COUNTS, 39, seed=4, weights="random")  # pooled: the file's numbering is its own
    F = 40
    frames = ra.synthetic_frames(F, 39, seed=12)
    z = er.zero_tables(prev)
    parts, files = [], []
    both = ra.Estimator(prev, 512)
    seq_num, seq_den = z, z
    for shard in range(2):
        pf, pm, pd, wn, wd = viterbi_case(prev, 300, F, 30 + shard)
        e = ra.Estimator(prev, 512)
        disc(gpu, e, frames, pf, pm, pd, wn, wd)
        disc(gpu, both, frames, pf, pm, pd, wn, wd)
        path = tmp_path / f"shard{shard}.mix"
        e.write_discriminative(path)
        files.append(path.read_bytes())
        ent = entries_of(prev, pm, pd)
        parts.append((er.sequential(prev, frames, ent, pf, wn, z), er.sequential(prev, frames, ent, pf, wd, z)))
        seq_num, seq_den = er.sequential(prev, frames, ent, pf, wn, seq_num), er.sequential(prev, frames, ent, pf, wd, seq_den)
    num = {k: parts[0][0][k] + parts[1][0][k] for k in KEYS}
    den = {k: parts[0][1][k] + parts[1][1][k] for k in KEYS}

    def compare(got, tables):
        want, want_ic = er.estimate(prev, *tables, iteration_constants_type=kind)
        assert len(want_ic) < prev.n_entries  # densities under the minimum observation weight left the model
        for key in ("density_mean", "density_covariance", "mixture_offsets", "mixture_densities"):
            assert np.array_equal(getattr(got, key), want[key]), key
        assert np.array_equal(got.means.view(np.uint32), want["means"].view(np.uint32))
        assert np.array_equal(got.variances.view(np.uint32), want["variances"].view(np.uint32))
        ref = want["mixture_log_weights"]
        assert (np.abs(got.mixture_log_weights - ref) <= 2.0 ** -23 * np.abs(ref)).all()
        return want_ic
    combined = ra.combine_discriminative_estimators(files)
    want_ic = compare(ra.estimate_ebw(combined, prev, iteration_constants_type=kind), (num, den))
    got_ic = ra.ebw_iteration_constants(combined, prev, iteration_constants_type=kind)
    assert np.array_equal(got_ic.view(np.uint64), want_ic.view(np.uint64))
    # the handle form: serializes the device tables, then the same estimate
    assert same(both.get(), seq_num) and same(both.get_denominator(), seq_den)
    compare(both.estimate_ebw(prev, iteration_constants_type=kind), (seq_num, seq_den))
