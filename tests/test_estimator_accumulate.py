"""Device-side maximum-likelihood accumulation (include/rasr_gmm_estimator.h, rasr_amd/csrc/gmm_kernels_accum.hip):
AbstractMixtureSetEstimator::accumulate in Viterbi mode for a list of (frame, mixture[, density][, weight]) pairs.

The numeric contract is restated here in numpy f64 (`numpy_order`): per accumulator the contributions in pair order,
sum = sum + w * x, sum = sum + (w * x) * x, weight = weight + w; more than GMM_ESTIMATOR_CHUNK = 512 contributions of
one call to one accumulator are cut into pieces of 512, piece 0 onto the current value, later pieces from 0 and then
added in piece order.  Every table must equal it BIT FOR BIT.  The other checks: oracle.estimator.accumulate_viterbi
(the purely sequential loop, equal up to 512 contributions), the standard bound between two summation orders beyond,
the written file against oracle.estimator.write_estimator_file with the first-appearance numbering, the scorer's best
densities (OracleSimd / OracleFloat, which tests/test_best_pairs.py pins the pairs kernel to), skips and errors.
"""
import numpy as np
import pytest

import oracle
import rasr_amd as ra
from oracle import estimator as est
from rasr_amd import _capi

pytestmark = pytest.mark.gpu

CHUNK = 512
TABLES = ["mean_sums", "mean_weights", "covariance_sums", "covariance_weights", "entry_weights"]


# ---------------------------------------------------------------------------------------------------------------
# the contract in numpy
# ---------------------------------------------------------------------------------------------------------------

def zero_tables(top):
    D = top.dimension
    return {"mean_sums": np.zeros((top.means.shape[0], D)), "mean_weights": np.zeros(top.means.shape[0]),
            "covariance_sums": np.zeros((top.n_covariances, D)), "covariance_weights": np.zeros(top.n_covariances),
            "entry_weights": np.zeros(top.n_entries)}


def resolve(top, n_frames, pf, pm, pd):
    """Per pair its mixture entry or -1 (skipped): frame, mixture or density out of range."""
    off = top.mixture_offsets.astype(np.int64)
    entry = np.full(len(pf), -1, np.int64)
    for i, (f, m, d) in enumerate(zip(pf.astype(np.int64), pm.astype(np.int64), pd.astype(np.int64))):
        if f < n_frames and m < top.n_mixtures and d < off[m + 1] - off[m]:
            entry[i] = off[m] + d
    return entry


def _ordered(sums, weights, dest, x, w, square, chunk):
    """One table: dest[i] the accumulator of contribution i (pair order), x [n, D] f64 or None, w [n]."""
    for k in np.unique(dest):
        idx = np.nonzero(dest == k)[0]
        parts = []
        for q, start in enumerate(range(0, len(idx), chunk)):
            s = (sums[k].copy() if q == 0 else np.zeros_like(sums[k])) if sums is not None else None
            ww = weights[k] if q == 0 else 0.0
            for i in idx[start:start + chunk]:
                if s is not None:
                    wx = w[i] * x[i]
                    s = s + (wx * x[i] if square else wx)
                ww = ww + w[i]
            parts.append((s, ww))
        s, ww = parts[0]
        for ps, pw in parts[1:]:
            if s is not None:
                s = s + ps
            ww = ww + pw
        if s is not None:
            sums[k] = s
        weights[k] = ww


def numpy_order(top, frames, pf, pm, pd, pw=None, tables=None, chunk=CHUNK):
    """(tables, skipped) after one call on `tables` (zeros if None); chunk=None: the purely sequential sum."""
    t = {k: v.copy() for k, v in (tables or zero_tables(top)).items()}
    entry = resolve(top, frames.shape[0], pf, pm, pd)
    ok = entry >= 0
    e = entry[ok]
    x = frames[pf[ok].astype(np.int64)].astype(np.float64)
    w = np.ones(len(e)) if pw is None else np.asarray(pw, np.float64)[ok]
    dens = top.mixture_densities[e]
    chunk = chunk or max(len(e), 1)
    _ordered(t["mean_sums"], t["mean_weights"], top.density_mean[dens], x, w, False, chunk)
    _ordered(t["covariance_sums"], t["covariance_weights"], top.density_covariance[dens], x, w, True, chunk)
    _ordered(None, t["entry_weights"], e, None, w, False, chunk)
    return t, int((~ok).sum())


def expected_file(top, t):
    """oracle.estimator.write_estimator_file of the tables after MixtureSetEstimatorIndexMap's first-appearance
    renumbering (AbstractMixtureSetEstimator.cc:804-817); also returns the three orders."""
    mean_idx, cov_idx, dens_idx = {}, {}, {}
    for d in top.mixture_densities:
        mean_idx.setdefault(int(top.density_mean[d]), len(mean_idx))
        cov_idx.setdefault(int(top.density_covariance[d]), len(cov_idx))
        dens_idx.setdefault(int(d), len(dens_idx))
    order = [sorted(ix, key=ix.get) for ix in (mean_idx, cov_idx, dens_idx)]
    means = [(t["mean_sums"][m], t["mean_weights"][m]) for m in order[0]]
    covs = [(t["covariance_sums"][c], t["covariance_weights"][c]) for c in order[1]]
    dens = [(mean_idx[int(top.density_mean[d])], cov_idx[int(top.density_covariance[d])]) for d in order[2]]
    off = top.mixture_offsets
    mix = [[(dens_idx[int(top.mixture_densities[e])], t["entry_weights"][e]) for e in range(off[m], off[m + 1])]
           for m in range(top.n_mixtures)]
    return est.write_estimator_file(None, top.dimension, means, covs, dens, mix), order


def assert_bit_equal(got, want):
    for k in TABLES:
        assert got[k].shape == want[k].shape, k
        same = got[k].view(np.uint64) == np.ascontiguousarray(want[k]).view(np.uint64)
        assert same.all(), f"{k}: {int((~same).sum())} of {same.size} elements differ"


# ---------------------------------------------------------------------------------------------------------------
# device calls
# ---------------------------------------------------------------------------------------------------------------

def accumulate_device(gpu, e, frames, pf, pm, pd=None, pw=None, scorer=None, stride=None):
    import torch
    D = frames.shape[1]
    x = torch.zeros((frames.shape[0], stride or D), dtype=torch.float32, device=gpu)
    x[:, :D] = torch.from_numpy(np.ascontiguousarray(frames)).to(gpu)

    def ints(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(gpu)
    tf, tm, td = ints(pf), ints(pm), ints(pd)
    tw = None if pw is None else torch.from_numpy(np.ascontiguousarray(pw, dtype=np.float64)).to(gpu)
    torch.cuda.synchronize()
    e.accumulate_device(x, tf, tm, td, tw, scorer=scorer)
    return e.skipped  # waits for the call: the tensors may go


def random_pairs(top, n_frames, n, seed):
    """n pairs on the non-empty mixtures, frames repeated, a density of the mixture each."""
    rng = np.random.default_rng(seed)
    counts = np.diff(top.mixture_offsets.astype(np.int64))
    pm = rng.choice(np.nonzero(counts > 0)[0], size=n).astype(np.uint32)
    pf = rng.integers(0, n_frames, size=n).astype(np.uint32)
    pd = (rng.integers(0, 1 << 30, size=n) % counts[pm]).astype(np.uint32)
    return pf, pm, pd


@pytest.fixture(scope="module")
def case1():
    """12 mixtures of 0..9 densities (mixture 4 empty), D = 39, 3 covariances, 50 frames, 200 pairs."""
    counts = np.array([3, 9, 1, 5, 0, 7, 2, 9, 4, 6, 8, 1])
    top = ra.synthetic_mixture_set(12, counts, 39, seed=11, n_covariances=3, weights="random")
    frames = ra.synthetic_frames(50, 39, seed=12)
    pf, pm, pd = random_pairs(top, 50, 200, 13)
    assert len(np.unique(pf)) < 200  # frames repeat
    pw = np.random.default_rng(14).uniform(0.0, 2.0, size=200)
    pw[[3, 77, 150]] = 0.0
    ref, _ = numpy_order(top, frames, pf, pm, pd)
    ref_w, _ = numpy_order(top, frames, pf, pm, pd, pw)
    return dict(top=top, frames=frames, pf=pf, pm=pm, pd=pd, pw=pw, ref=ref, ref_w=ref_w)


def test_given_densities(gpu, case1):
    c = case1
    e = ra.Estimator(c["top"], max_pairs=256)
    assert accumulate_device(gpu, e, c["frames"], c["pf"], c["pm"], c["pd"], stride=48) == 0
    got = e.get()
    assert_bit_equal(got, c["ref"])
    # the trainer's sequential loop (oracle): the same sums while no accumulator gets more than 512 contributions
    top = c["top"]
    assignment = top.mixture_densities[top.mixture_offsets[c["pm"]] + c["pd"]]
    means, covs = est.accumulate_viterbi(c["frames"][c["pf"]], assignment, top.means.shape[0], top.n_covariances,
                                         top.density_mean, top.density_covariance)
    for i, (s, w) in enumerate(means):
        assert np.array_equal(got["mean_sums"][i].view(np.uint64), s.view(np.uint64)) and got["mean_weights"][i] == w
    for i, (s, w) in enumerate(covs):
        assert np.array_equal(got["covariance_sums"][i].view(np.uint64), s.view(np.uint64))
        assert got["covariance_weights"][i] == w
    assert got["entry_weights"].sum() == 200 and got["covariance_weights"].sum() == 200


def test_weighted(gpu, case1):
    c = case1
    assert (c["pw"] == 0).sum() == 3 and c["pw"].min() >= 0 and c["pw"].max() < 2
    e = ra.Estimator(c["top"], max_pairs=200)
    assert accumulate_device(gpu, e, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"]) == 0
    assert_bit_equal(e.get(), c["ref_w"])
    assert not np.array_equal(c["ref_w"]["mean_sums"], c["ref"]["mean_sums"])


def _shared_topology(D=11):
    """Densities 1 and 2 on mean 0; density 3 in mixtures 0 and 1; density 4, mean 3 unreferenced; the mixtures'
    order makes the first-appearance numbering differ from the identity in all three maps."""
    rng = np.random.default_rng(21)
    return ra.MixtureSet(means=rng.standard_normal((4, D)).astype(np.float32),
                         variances=(0.5 + rng.random((2, D))).astype(np.float32),
                         density_mean=[2, 0, 0, 1, 3], density_covariance=[1, 0, 0, 1, 0],
                         mixture_offsets=[0, 2, 4, 5], mixture_densities=[3, 1, 2, 3, 0],
                         mixture_log_weights=np.log([0.5, 0.5, 0.5, 0.5, 1.0]))


def test_shared_topology_and_file(gpu):
    top = _shared_topology()
    frames = ra.synthetic_frames(30, top.dimension, seed=22)
    pf, pm, pd = random_pairs(top, 30, 150, 23)
    pw = np.random.default_rng(24).uniform(0.0, 2.0, size=150)
    ref, _ = numpy_order(top, frames, pf, pm, pd, pw)
    e = ra.Estimator(top, max_pairs=150)
    assert accumulate_device(gpu, e, frames, pf, pm, pd, pw) == 0
    got = e.get()
    assert_bit_equal(got, ref)
    # the shared mean holds both densities' frames, the shared density both mixtures'
    assert got["mean_weights"][0] == pytest.approx(got["entry_weights"][1] + got["entry_weights"][2], rel=1e-12)
    assert got["mean_weights"][3] == 0 and not got["mean_sums"][3].any()
    want, order = expected_file(top, ref)
    assert order[0] == [1, 0, 2] and order[1] == [1, 0] and order[2] == [3, 1, 2, 0]  # none is the identity
    data = e.to_bytes()
    assert data == want
    # and it reads back: the library's estimate of it is the restatement's
    ms = ra.estimate_mixture_set(data, minimum_observation_weight=0.0)
    ref_ms = est.estimate(want, minimum_observation_weight=0.0)
    assert np.array_equal(ms.means.view(np.uint32), ref_ms["means"].view(np.uint32))
    assert np.array_equal(ms.mixture_densities, ref_ms["mixture_densities"])


def _piece_case(D):
    """One covariance, one mixture of two densities, 1300 pairs: both means and the covariance get more than 512."""
    top = ra.synthetic_mixture_set(1, 2, D, seed=31)
    frames = ra.synthetic_frames(300, D, seed=32 + D)
    rng = np.random.default_rng(33 + D)
    pf = rng.integers(0, 300, size=1300).astype(np.uint32)
    pm = np.zeros(1300, np.uint32)
    pd = rng.integers(0, 2, size=1300).astype(np.uint32)
    return top, frames, pf, pm, pd


@pytest.mark.parametrize("D", [16, 39, 80])
def test_piece_rule(gpu, D):
    top, frames, pf, pm, pd = _piece_case(D)
    ref, _ = numpy_order(top, frames, pf, pm, pd)
    seq, _ = numpy_order(top, frames, pf, pm, pd, chunk=None)
    # the two orders are different sums: a kernel that summed sequentially would not pass the bit-equal check below
    # (unweighted mean sums are sums of f32 values and exact in f64 in any order; the squares are not)
    assert (ref["covariance_sums"] != seq["covariance_sums"]).any()
    assert min(np.bincount(pd)) > CHUNK
    e = ra.Estimator(top, max_pairs=1300)
    assert accumulate_device(gpu, e, frames, pf, pm, pd) == 0
    got = e.get()
    assert_bit_equal(got, ref)
    # against the purely sequential sum: the standard bound between two summation orders of n terms,
    # |a - b| <= 2 n 2^-53 sum |term| per element
    x = frames[pf].astype(np.float64)
    bound_cov = 2 * 1300 * 2.0 ** -53 * (x * x).sum(axis=0)
    assert (np.abs(got["covariance_sums"][0] - seq["covariance_sums"][0]) <= bound_cov).all()
    for d in range(2):
        n = int((pd == d).sum())
        bound = 2 * n * 2.0 ** -53 * np.abs(x[pd == d]).sum(axis=0)
        assert (np.abs(got["mean_sums"][d] - seq["mean_sums"][d]) <= bound).all()
    assert got["covariance_weights"][0] == 1300 and got["entry_weights"].sum() == 1300
    # weighted, the piece rule shows in the other tables too: mean sums, mean weights and entry weights
    pw = np.random.default_rng(34 + D).uniform(0.0, 2.0, size=1300)
    ref_w, _ = numpy_order(top, frames, pf, pm, pd, pw)
    seq_w, _ = numpy_order(top, frames, pf, pm, pd, pw, chunk=None)
    for k in ["mean_sums", "mean_weights", "covariance_sums", "entry_weights"]:
        assert (ref_w[k] != seq_w[k]).any(), k
    e.reset()
    assert accumulate_device(gpu, e, frames, pf, pm, pd, pw) == 0
    assert_bit_equal(e.get(), ref_w)


def test_two_calls_and_reset(gpu, case1):
    c = case1
    e = ra.Estimator(c["top"], max_pairs=200)
    h = 100
    accumulate_device(gpu, e, c["frames"], c["pf"][:h], c["pm"][:h], c["pd"][:h], c["pw"][:h])
    accumulate_device(gpu, e, c["frames"], c["pf"][h:], c["pm"][h:], c["pd"][h:], c["pw"][h:])
    assert_bit_equal(e.get(), c["ref_w"])  # one in-order pass over all 200
    e.reset()
    assert_bit_equal(e.get(), zero_tables(c["top"]))
    assert e.skipped == 0
    accumulate_device(gpu, e, c["frames"], c["pf"], c["pm"], c["pd"])
    assert_bit_equal(e.get(), c["ref"])


@pytest.mark.parametrize("kind", ["SIMD-diagonal-maximum", "diagonal-maximum"])
def test_with_scorer(gpu, kind):
    counts = np.random.default_rng(41).integers(1, 41, size=20)
    top = ra.synthetic_mixture_set(20, counts, 39, seed=42, weights="random")
    frames = ra.synthetic_frames(40, 39, seed=43)
    pf = np.repeat(np.arange(40, dtype=np.uint32), 3)
    pm = ((3 * pf + np.tile(np.arange(3, dtype=np.uint32), 40)) % 20).astype(np.uint32)  # every mixture 6 times
    orc = oracle.OracleSimd(top) if kind.startswith("SIMD") else oracle.OracleFloat(top)
    best = orc.score(frames)[1]
    ref, skipped = numpy_order(top, frames, pf, pm, best[pm, pf])
    assert skipped == 0
    sc = ra.Scorer(top, kind, max_frames=40)
    e = ra.Estimator(top, max_pairs=120)
    assert accumulate_device(gpu, e, frames, pf, pm, scorer=sc) == 0
    assert_bit_equal(e.get(), ref)
    want, _ = expected_file(top, ref)
    assert e.to_bytes() == want
    for kw in (dict(), dict(minimum_observation_weight=2.0, minimum_variance=0.01)):
        ms, ref_ms = e.estimate(**kw), ra.estimate_mixture_set(want, **kw)
        for f in ["means", "variances", "density_mean", "density_covariance", "mixture_offsets", "mixture_densities",
                  "mixture_log_weights"]:
            a, b = getattr(ms, f), getattr(ref_ms, f)
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f


def test_skips_and_errors(gpu, case1):
    c = case1
    top, frames = c["top"], c["frames"]
    # given densities: an out-of-range frame, mixture and density, a pair on the empty mixture 4 -- spread among
    # the good pairs
    bad = [(50, 0, 0), (1 << 30, 3, 1), (7, 12, 0), (7, 0xFFFFFFFF, 0), (9, 1, 9), (9, 2, 0xFFFFFFFF), (5, 4, 0)]
    pf, pm, pd = list(c["pf"]), list(c["pm"]), list(c["pd"])
    for j, (f, m, d) in enumerate(bad):
        at = 5 + 29 * j
        pf.insert(at, f), pm.insert(at, m), pd.insert(at, d)
    pf, pm, pd = (np.array(a, np.uint32) for a in (pf, pm, pd))
    ref, skipped = numpy_order(top, frames, pf, pm, pd)
    assert skipped == len(bad)
    assert_bit_equal(ref, c["ref"])  # the restatement agrees: the tables of the run without them
    e = ra.Estimator(top, max_pairs=256)
    assert accumulate_device(gpu, e, frames, pf, pm, pd) == len(bad)
    assert_bit_equal(e.get(), c["ref"])
    # with a scorer: the empty mixture has no best density (0xffffffff), frames and mixtures out of range
    sc = ra.Scorer(top, "SIMD-diagonal-maximum", max_frames=50)
    best = oracle.OracleSimd(top).score(frames)[1]
    good = c["pm"] != 4
    gf, gm = c["pf"][good], c["pm"][good]
    ref_s, _ = numpy_order(top, frames, gf, gm, best[gm, gf])
    sf = np.concatenate([[3, 50, 2], gf, [8]]).astype(np.uint32)
    sm = np.concatenate([[4, 1, 12], gm, [4]]).astype(np.uint32)
    e.reset()
    assert accumulate_device(gpu, e, frames, sf, sm, scorer=sc) == 4
    assert_bit_equal(e.get(), ref_s)

    def code(fn):
        with pytest.raises(ra.GmmError) as err:
            fn()
        return err.value.code
    before = e.get()
    assert code(lambda: accumulate_device(gpu, ra.Estimator(top, max_pairs=100), frames, c["pf"], c["pm"], c["pd"])) \
        == _capi.GMM_ERR_CAPACITY
    shard = ra.Scorer(top, "SIMD-diagonal-maximum", max_frames=50, mixture_range=(2, 8))
    assert code(lambda: accumulate_device(gpu, e, frames, gf, gm, scorer=shard)) == _capi.GMM_ERR_UNSUPPORTED
    pooled = ra.synthetic_mixture_set(12, np.diff(top.mixture_offsets.astype(np.int64)), 39, seed=11)  # batch types
    batch = ra.Scorer(pooled, "batch-diagonal-maximum-int", max_frames=50)                            # need one covariance
    assert code(lambda: accumulate_device(gpu, ra.Estimator(pooled, max_pairs=256), frames, gf, gm, scorer=batch)) \
        == _capi.GMM_ERR_UNSUPPORTED
    assert code(lambda: accumulate_device(gpu, e, frames, gf, gm)) == _capi.GMM_ERR_INVALID_ARGUMENT  # verify_ cc:382
    other = ra.Scorer(ra.synthetic_mixture_set(12, 3, 39, seed=5), "SIMD-diagonal-maximum", max_frames=50)
    assert code(lambda: accumulate_device(gpu, e, frames, gf, gm, scorer=other)) == _capi.GMM_ERR_INVALID_ARGUMENT
    assert_bit_equal(e.get(), before)  # a refused call changes nothing
    assert e.skipped == 4
    # one density per mixture: no scorer and no density needed
    single = ra.synthetic_mixture_set(6, 1, 39, seed=6)
    e1 = ra.Estimator(single, max_pairs=64)
    f1, m1 = c["pf"][:64], (c["pm"][:64] % 6).astype(np.uint32)
    assert accumulate_device(gpu, e1, frames, f1, m1) == 0
    assert_bit_equal(e1.get(), numpy_order(single, frames, f1, m1, np.zeros(64, np.uint32))[0])


def test_host_call(gpu, case1):
    c = case1
    e = ra.Estimator(c["top"], max_pairs=200)
    padded = np.zeros((50, 44), np.float32)
    padded[:, :39] = c["frames"]
    e.accumulate_host(padded, c["pf"], c["pm"], c["pd"], c["pw"])
    host = e.get()
    assert_bit_equal(host, c["ref_w"])
    d = ra.Estimator(c["top"], max_pairs=200)
    accumulate_device(gpu, d, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"])
    assert_bit_equal(host, d.get())
    assert e.to_bytes() == d.to_bytes()
    # with a scorer, and skipped pairs counted alike
    sc = ra.Scorer(c["top"], "diagonal-maximum", max_frames=50)
    e.reset(), d.reset()
    e.accumulate_host(c["frames"], c["pf"], c["pm"], scorer=sc)
    accumulate_device(gpu, d, c["frames"], c["pf"], c["pm"], scorer=sc)
    assert_bit_equal(e.get(), d.get())
    assert e.skipped == d.skipped == 0
