"""Device-side accumulation of affine feature transform (CMLLR) statistics per speaker key
(include/rasr_gmm_adaptation.h, rasr_amd/csrc/gmm_kernels_adapt.hip): AffineFeatureTransformAccumulator::accumulate,
finalize and combine for lists of (frame, mixture[, density][, weight][, key]) pairs.

The numeric contract is restated in numpy f64 in tests/affine_restatement.py (per key the pairs in pair order, one
rounding per operation, the division a division, pieces of GMM_AFFINE_CHUNK = 512).  Every table of every key must equal
it BIT FOR BIT; the end-to-end case at the bottom only checks the sign and layout conventions of the whole chain.
"""
import functools

import numpy as np
import pytest

import affine_restatement as ar
import rasr_amd as ra
from rasr_amd import _capi

pytestmark = pytest.mark.gpu

NAMES = ["k", "G", "mean", "cov"]


def model(D, kind):
    """The 20 x 8 model of dimension D: pooled, three covariances, one per mixture, one per density."""
    if kind == "pooled":
        return ra.synthetic_mixture_set(20, 8, D, seed=100 + D)
    if kind == "cov3":
        return ra.synthetic_mixture_set(20, 8, D, seed=100 + D, n_covariances=3)
    return ra.synthetic_mixture_set(20, 8, D, seed=100 + D, tying=kind)


def pairs(ms, n_frames, n, seed):
    rng = np.random.default_rng(seed)
    pf = rng.integers(0, n_frames, size=n).astype(np.uint32)
    pm = rng.integers(0, ms.n_mixtures, size=n).astype(np.uint32)
    pd = (rng.integers(0, 1 << 30, size=n) % np.diff(ms.mixture_offsets.astype(np.int64))[pm]).astype(np.uint32)
    return pf, pm, pd


def run(gpu, acc, frames, pf, pm, pd=None, pw=None, pk=None, scorer=None, stride=None):
    """One device call; returns the skipped count (which waits for the call)."""
    import torch
    D = acc.mixture_set.dimension
    x = torch.full((frames.shape[0], stride or D), 7.5, dtype=torch.float32, device=gpu)  # padding columns: not 0
    x[:, :D] = torch.from_numpy(np.ascontiguousarray(frames[:, :D])).to(gpu)

    def ints(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(gpu)
    tw = None if pw is None else torch.from_numpy(np.ascontiguousarray(pw, dtype=np.float64)).to(gpu)
    torch.cuda.synchronize()
    acc.accumulate_device(x, ints(pf), ints(pm), ints(pd), tw, ints(pk), scorer=scorer)
    return acc.skipped


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_tables(got, want, what=""):
    assert same_bits(np.float64(got["beta"]), np.float64(want["beta"])), f"{what} beta {got['beta']} {want['beta']}"
    for n in NAMES:
        assert got[n].shape == want[n].shape, n
        diff = got[n].view(np.uint64) != np.ascontiguousarray(want[n]).view(np.uint64)
        assert not diff.any(), f"{what} {n}: {int(diff.sum())} of {diff.size} elements differ"


def assert_keys(acc, ref, ms, what=""):
    for key, t in enumerate(ref):
        assert_tables(acc.tables(key), ar.finalize(t, ms), f"{what} key {key}")


@functools.lru_cache(maxsize=None)
def shape_case(D, kind):
    """Three keys interleaved pair by pair (D = 80: two), key 2 of 4 receiving nothing; random f64 weights with a 0 and a
    negative one; 60 frames."""
    ms = model(D, kind)
    frames = ra.synthetic_frames(60, D, seed=200 + D)
    n = 150 if D < 80 else 60
    pf, pm, pd = pairs(ms, 60, n, 300 + D)
    live = np.array([0, 1, 3] if D < 80 else [0, 1], np.uint32)
    pk = live[np.arange(n) % len(live)]
    pw = np.random.default_rng(400 + D).uniform(-0.5, 2.0, size=n)
    pw[5], pw[17] = 0.0, -1.25
    n_keys = 4 if D < 80 else 2
    ref, skipped = ar.accumulate(ms, frames, pf, pm, pd, pw, pk, n_keys=n_keys)
    assert skipped == 0
    return dict(ms=ms, frames=frames, pf=pf, pm=pm, pd=pd, pk=pk, pw=pw, n_keys=n_keys, ref=ref)


@pytest.mark.parametrize("kind", ["pooled", "cov3", "mixture-specific", "none"])
@pytest.mark.parametrize("D", [3, 39, 45, 80])
def test_shapes(gpu, D, kind):
    c = shape_case(D, kind)
    ms = c["ms"]
    assert {"pooled": 1, "cov3": 3, "mixture-specific": 20, "none": 160}[kind] == ms.n_covariances
    acc = ra.AffineTransformAccumulator(ms, c["n_keys"], max_pairs=256)
    assert run(gpu, acc, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], c["pk"], stride=D + 5) == 0
    assert_keys(acc, c["ref"], ms)
    info = acc.info()
    T = (D + 1) * (D + 2) // 2
    small = 1 + (D + 1) + T + D * (D + 1)
    if kind == "pooled":
        # no G table on the device; tables() derives G[i] = cov / v[i], one division
        assert info["pooled"] and info["table_bytes"] == c["n_keys"] * small * 8
        t = acc.tables(0)
        assert same_bits(t["G"], t["cov"][None] / ms.variances[0].astype(np.float64)[:, None, None])
    else:
        assert not info["pooled"] and info["table_bytes"] == c["n_keys"] * (small + D * T) * 8
    if D < 80:  # the key that received nothing stays exactly zero
        t = acc.tables(2)
        assert t["beta"] == 0 and not any(t[n].any() for n in NAMES)
    # reading does not change the handle, and the same call on fresh tables gives the same bits
    assert_keys(acc, c["ref"], ms, "second read")
    acc.reset()
    assert run(gpu, acc, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], c["pk"], stride=D + 5) == 0
    assert_keys(acc, c["ref"], ms, "second run")


@pytest.mark.parametrize("D,n", [(39, 1), (39, 511), (39, 512), (39, 513), (39, 1300), (3, 1300), (45, 1300), (80, 513)])
def test_pair_counts_of_one_key(gpu, D, n):
    """One key receives n pairs (key 1 of 2; key 0 a handful, interleaved): below, at and past the piece size."""
    ms = model(D, "cov3")
    frames = ra.synthetic_frames(60, D, seed=500 + D)
    extra = 7
    pf, pm, pd = pairs(ms, 60, n + extra, 600 + D + n)
    pk = np.ones(n + extra, np.uint32)
    pk[np.linspace(0, n + extra - 1, extra).astype(np.int64)] = 0
    assert int((pk == 1).sum()) == n
    pw = np.random.default_rng(700 + n).uniform(0.0, 2.0, size=n + extra)
    ref, _ = ar.accumulate(ms, frames, pf, pm, pd, pw, pk, n_keys=2)
    if n > ar.CHUNK + 1 and D <= 39:  # the piece rule is visible: the sequential order gives other bits
        seq, _ = ar.accumulate(ms, frames, pf, pm, pd, pw, pk, n_keys=2, chunk=None)
        assert (seq[1]["G"] != ref[1]["G"]).any() and (seq[1]["k"] != ref[1]["k"]).any()
    acc = ra.AffineTransformAccumulator(ms, 2, max_pairs=n + extra)
    assert run(gpu, acc, frames, pf, pm, pd, pw, pk) == 0
    assert_keys(acc, ref, ms)


@functools.lru_cache(maxsize=None)
def case39():
    """D = 39, three covariances, 3 keys, 900 pairs: key 0 gets 600 (two pieces), the others 150 each."""
    ms = model(39, "cov3")
    frames = ra.synthetic_frames(80, 39, seed=801)
    n = 900
    pf, pm, pd = pairs(ms, 80, n, 802)
    pk = np.zeros(n, np.uint32)
    pk[1::6], pk[4::6] = 1, 2
    pw = np.random.default_rng(803).uniform(0.0, 2.0, size=n)
    ref_w, _ = ar.accumulate(ms, frames, pf, pm, pd, pw, pk, n_keys=3)
    ref_1, _ = ar.accumulate(ms, frames, pf, pm, pd, None, pk, n_keys=3)
    return dict(ms=ms, frames=frames, pf=pf, pm=pm, pd=pd, pk=pk, pw=pw, ref_w=ref_w, ref_1=ref_1)


def test_null_weights_are_ones_and_null_keys_are_zero(gpu):
    c = case39()
    ms = c["ms"]
    a = ra.AffineTransformAccumulator(ms, 3, max_pairs=900)
    b = ra.AffineTransformAccumulator(ms, 3, max_pairs=900)
    run(gpu, a, c["frames"], c["pf"], c["pm"], c["pd"], None, c["pk"])
    run(gpu, b, c["frames"], c["pf"], c["pm"], c["pd"], np.ones(900), c["pk"])
    assert_keys(a, c["ref_1"], ms)
    assert_keys(b, c["ref_1"], ms)
    # no keys: everything on key 0
    ref0, _ = ar.accumulate(ms, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], None, n_keys=3)
    a.reset()
    run(gpu, a, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], None)
    assert_keys(a, ref0, ms)
    assert a.tables(0)["beta"] == pytest.approx(c["pw"].sum(), rel=1e-12) and a.tables(1)["beta"] == 0


def test_two_calls_and_reset(gpu):
    c = case39()
    ms = c["ms"]
    h = 774  # key 0 has more than one piece in the first call (516 pairs) and continues from its value in the second
    assert int((c["pk"][:h] == 0).sum()) > ar.CHUNK
    first, _ = ar.accumulate(ms, c["frames"], c["pf"][:h], c["pm"][:h], c["pd"][:h], c["pw"][:h], c["pk"][:h], n_keys=3)
    both, _ = ar.accumulate(ms, c["frames"], c["pf"][h:], c["pm"][h:], c["pd"][h:], c["pw"][h:], c["pk"][h:], n_keys=3,
                            tables=first)
    assert (both[0]["G"] != c["ref_w"][0]["G"]).any()  # not the one-call sum: the pieces fall differently
    acc = ra.AffineTransformAccumulator(ms, 3, max_pairs=900)
    run(gpu, acc, c["frames"], c["pf"][:h], c["pm"][:h], c["pd"][:h], c["pw"][:h], c["pk"][:h])
    assert_keys(acc, first, ms, "first call")
    run(gpu, acc, c["frames"], c["pf"][h:], c["pm"][h:], c["pd"][h:], c["pw"][h:], c["pk"][h:])
    assert_keys(acc, both, ms, "second call")
    acc.reset()
    assert acc.skipped == 0
    for key in range(3):
        t = acc.tables(key)
        assert t["beta"] == 0 and not any(t[n].any() for n in NAMES)
    run(gpu, acc, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], c["pk"])
    assert_keys(acc, c["ref_w"], ms, "after reset")


def test_host_call_equals_device_call(gpu):
    c = case39()
    ms = c["ms"]
    host = ra.AffineTransformAccumulator(ms, 3, max_pairs=900)
    padded = np.full((80, 44), np.nan, np.float32)
    padded[:, :39] = c["frames"]
    host.accumulate(padded, c["pf"], c["pm"], c["pd"], c["pw"], c["pk"])
    assert_keys(host, c["ref_w"], ms, "host")
    dev = ra.AffineTransformAccumulator(ms, 3, max_pairs=900)
    run(gpu, dev, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], c["pk"])
    for key in range(3):
        assert_tables(host.tables(key), dev.tables(key))


def test_add_is_combine(gpu):
    c = case39()
    ms = c["ms"]
    h = 450
    half = [slice(0, h), slice(h, 900)]
    accs, refs = [], []
    for s in half:
        a = ra.AffineTransformAccumulator(ms, 3, max_pairs=900)
        run(gpu, a, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], c["pw"][s], c["pk"][s])
        accs.append(a)
        refs.append(ar.accumulate(ms, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], c["pw"][s], c["pk"][s], n_keys=3)[0])
    for weight in (1.0, 0.5):
        a = accs[0]
        a.reset()
        run(gpu, a, c["frames"], c["pf"][half[0]], c["pm"][half[0]], c["pd"][half[0]], c["pw"][half[0]], c["pk"][half[0]])
        for key in range(3):
            a.add(key, accs[1].tables(key), weight)
            want = ar.combine(refs[0][key], ar.finalize(refs[1][key], ms), weight, 39)
            assert_tables(a.tables(key), ar.finalize(want, ms), f"weight {weight} key {key}")
    # pooled mode: G is not added, it stays cov / v
    pooled = model(39, "pooled")
    p0 = ra.AffineTransformAccumulator(pooled, 1, max_pairs=900)
    p1 = ra.AffineTransformAccumulator(pooled, 1, max_pairs=900)
    r = []
    for a, s in zip((p0, p1), half):
        run(gpu, a, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], c["pw"][s])
        r.append(ar.accumulate(pooled, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], c["pw"][s])[0][0])
    p0.add(0, p1.tables(0), 0.5)
    assert_tables(p0.tables(0), ar.finalize(ar.combine(r[0], ar.finalize(r[1], pooled), 0.5, 39), pooled))


def test_skipped_pairs_and_poisoned_frame(gpu):
    c = case39()
    ms = c["ms"]
    frames = np.concatenate([c["frames"], np.full((1, 39), np.nan, np.float32)])  # frame 80: only skipped pairs name it
    bad = [(81, 0, 0, 0), (1 << 30, 3, 1, 1), (80, 20, 0, 0), (80, 0xFFFFFFFF, 0, 2), (80, 1, 8, 0),
           (80, 2, 0xFFFFFFFF, 1), (80, 5, 0, 3), (80, 5, 0, 0xFFFFFFFF)]
    cols = [list(c[n][:300]) for n in ("pf", "pm", "pd", "pk")]
    pw = list(c["pw"][:300])
    for j, b in enumerate(bad):
        at = 3 + 31 * j
        for col, v in zip(cols, b):
            col.insert(at, v)
        pw.insert(at, 1.0)
    pf, pm, pd, pk = (np.array(a, np.uint32) for a in cols)
    pw = np.array(pw)
    ref, skipped = ar.accumulate(ms, frames, pf, pm, pd, pw, pk, n_keys=3)
    assert skipped == len(bad)
    clean, _ = ar.accumulate(ms, c["frames"], c["pf"][:300], c["pm"][:300], c["pd"][:300], c["pw"][:300], c["pk"][:300], n_keys=3)
    acc = ra.AffineTransformAccumulator(ms, 3, max_pairs=400)
    assert run(gpu, acc, frames, pf, pm, pd, pw, pk) == len(bad)
    assert_keys(acc, clean, ms)
    for key in range(3):
        t = acc.tables(key)
        assert np.isfinite(t["beta"]) and all(np.isfinite(t[n]).all() for n in NAMES)
    assert_keys(acc, ref, ms)


@pytest.mark.parametrize("kind", ["SIMD-diagonal-maximum", "diagonal-maximum"])
def test_density_from_the_scorer(gpu, kind):
    import torch
    counts = np.array([3, 9, 1, 5, 0, 7, 2, 9, 4, 6, 8, 1])  # mixture 4 is empty
    ms = ra.synthetic_mixture_set(12, counts, 39, seed=11, n_covariances=3, weights="random")
    frames = ra.synthetic_frames(41, 39, seed=12)
    frames[40] = np.nan  # named only by the pairs on the empty mixture
    pf = np.repeat(np.arange(40, dtype=np.uint32), 3)
    pm = ((5 * pf + np.tile(np.arange(3, dtype=np.uint32), 40)) % 12).astype(np.uint32)
    pm[pm == 4] = 5
    pf = np.concatenate([pf, [40, 40]]).astype(np.uint32)
    pm = np.concatenate([pm, [4, 4]]).astype(np.uint32)
    pk = (np.arange(len(pf)) % 2).astype(np.uint32)
    sc = ra.Scorer(ms, kind, max_frames=41)
    d_frames = torch.from_numpy(frames).to(gpu)
    best = torch.empty(len(pf), dtype=torch.int32, device=gpu)
    sc.best_pairs_device(d_frames, torch.from_numpy(pf.view(np.int32)).to(gpu), torch.from_numpy(pm.view(np.int32)).to(gpu), best)
    torch.cuda.synchronize()
    best = best.cpu().numpy().view(np.uint32)
    assert (best[-2:] == 0xFFFFFFFF).all() and (best[:-2] < counts[pm[:-2]]).all()
    with_scorer = ra.AffineTransformAccumulator(ms, 2, max_pairs=128)
    assert run(gpu, with_scorer, frames, pf, pm, pk=pk, scorer=sc) == 2
    given = ra.AffineTransformAccumulator(ms, 2, max_pairs=128)
    assert run(gpu, given, frames, pf, pm, best, pk=pk) == 2
    ref, skipped = ar.accumulate(ms, frames, pf, pm, best, None, pk, n_keys=2)
    assert skipped == 2
    for key in range(2):
        assert_tables(with_scorer.tables(key), given.tables(key))
    assert_keys(with_scorer, ref, ms)
    assert all(np.isfinite(with_scorer.tables(0)[n]).all() for n in NAMES)


def test_refusals_leave_the_tables_untouched(gpu):
    c = case39()
    ms = c["ms"]
    acc = ra.AffineTransformAccumulator(ms, 3, max_pairs=300)
    s = slice(0, 300)
    run(gpu, acc, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], c["pw"][s], c["pk"][s])
    before = [acc.tables(key) for key in range(3)]

    def code(fn):
        with pytest.raises(ra.GmmError) as err:
            fn()
        return err.value.code, str(err.value)
    s2 = slice(0, 301)
    assert code(lambda: run(gpu, acc, c["frames"], c["pf"][s2], c["pm"][s2], c["pd"][s2]))[0] == _capi.GMM_ERR_CAPACITY
    other = ra.Scorer(ra.synthetic_mixture_set(20, 8, 40, seed=5), "SIMD-diagonal-maximum", max_frames=80)
    assert code(lambda: run(gpu, acc, c["frames"], c["pf"][s], c["pm"][s], scorer=other))[0] == _capi.GMM_ERR_INVALID_ARGUMENT
    shard = ra.Scorer(ms, "SIMD-diagonal-maximum", max_frames=80, mixture_range=(2, 8))
    assert code(lambda: run(gpu, acc, c["frames"], c["pf"][s], c["pm"][s], scorer=shard))[0] == _capi.GMM_ERR_UNSUPPORTED
    # no density and no scorer on a model with several densities per mixture
    assert code(lambda: run(gpu, acc, c["frames"], c["pf"][s], c["pm"][s]))[0] == _capi.GMM_ERR_INVALID_ARGUMENT
    for key in range(3):
        assert_tables(acc.tables(key), before[key])
    assert acc.skipped == 0
    with pytest.raises(ra.GmmError) as err:
        acc.tables(3)
    assert err.value.code == _capi.GMM_ERR_INVALID_ARGUMENT
    # a handle too large for the device: 2^22 keys x 250 KiB of G tables is a terabyte; the message names the size
    rc, msg = code(lambda: ra.AffineTransformAccumulator(ms, 1 << 22, max_pairs=300))
    assert rc == _capi.GMM_ERR_UNSUPPORTED and "GiB" in msg and "4194304 keys" in msg
    # a dimension past GMM_AFFINE_MAX_DIMENSION
    rc, msg = code(lambda: ra.AffineTransformAccumulator(ra.synthetic_mixture_set(2, 2, 257, seed=1), 1, max_pairs=8))
    assert rc == _capi.GMM_ERR_UNSUPPORTED and "257" in msg
    # one density per mixture: no scorer and no density needed
    single = ra.synthetic_mixture_set(6, 1, 39, seed=6, n_covariances=2)
    a1 = ra.AffineTransformAccumulator(single, 1, max_pairs=64)
    f1, m1 = c["pf"][:64], (c["pm"][:64] % 6).astype(np.uint32)
    assert run(gpu, a1, c["frames"], f1, m1) == 0
    assert_keys(a1, ar.accumulate(single, c["frames"], f1, m1, np.zeros(64, np.uint32))[0], single)


def test_end_to_end_speaker_shift(gpu):
    """Frames drawn from the model, mapped by a known affine map per key; accumulate with the scorer's densities, get,
    estimate (mmiPrime, 5 sweeps), apply: the mean diagonal-maximum score of each key's frames must fall strictly below
    the untransformed one.  A check of the sign and layout conventions only."""
    D, n_per_key = 8, 600
    ms = ra.synthetic_mixture_set(10, 4, D, seed=901, n_covariances=3)
    rng = np.random.default_rng(902)
    dens_cov = ms.density_covariance
    frames, pm, pk = [], [], []
    maps = []
    for key in range(2):
        A = np.eye(D) * (1.3 + 0.4 * key) + 0.1 * rng.standard_normal((D, D))
        b = rng.standard_normal(D) * (1.0 + key)
        maps.append((A, b))
        m = rng.integers(0, 10, size=n_per_key)
        d = ms.mixture_densities[ms.mixture_offsets[m] + rng.integers(0, 4, size=n_per_key)]
        clean = ms.means[ms.density_mean[d]] + rng.standard_normal((n_per_key, D)) * np.sqrt(ms.variances[dens_cov[d]])
        frames.append(clean @ A.T + b)  # what the speaker's channel does to them
        pm.append(m)
        pk.append(np.full(n_per_key, key))
    frames = np.concatenate(frames).astype(np.float32)
    pm, pk = np.concatenate(pm).astype(np.uint32), np.concatenate(pk).astype(np.uint32)
    pf = np.arange(len(frames), dtype=np.uint32)
    sc = ra.Scorer(ms, "diagonal-maximum", max_frames=len(frames))
    acc = ra.AffineTransformAccumulator(ms, 2, max_pairs=len(frames))
    assert run(gpu, acc, frames, pf, pm, pk=pk, scorer=sc) == 0

    def mean_score(x, sel):
        scores = sc.score_host(np.ascontiguousarray(x[sel], dtype=np.float32), want_best=False)
        scores = scores[0] if isinstance(scores, tuple) else scores
        return float(np.mean(scores[pm[sel], np.arange(int(sel.sum()))]))
    for key in range(2):
        sel = pk == key
        t = acc.tables(key)
        assert t["beta"] == n_per_key
        W = ra.estimate_affine_transform(t, "mmiPrime", 5).astype(np.float64)
        assert W.shape == (D, D + 1) and np.isfinite(W).all()
        moved = frames.astype(np.float64) @ W[:, 1:].T + W[:, 0]
        before, after = mean_score(frames, sel), mean_score(moved, sel)
        assert after < before, (key, before, after)
