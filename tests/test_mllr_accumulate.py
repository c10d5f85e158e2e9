"""Device-side accumulation of MLLR mean transform statistics per (speaker key, regression leaf)
(include/rasr_gmm_mllr.h, rasr_amd/csrc/gmm_kernels_mllr.hip): FullAdaptorViterbiEstimator / ShiftAdaptorViterbiEstimator
::accumulate and operator+= for lists of (frame, mixture[, density][, weight][, key]) pairs.

The numeric contract is restated in numpy f64 in tests/mllr_restatement.py (per set the pairs in pair order, one rounding
per operation, the divisions divisions, pieces of GMM_MLLR_CHUNK = 512).  Every table of every (key, leaf) must equal it
BIT FOR BIT.  The end-to-end case at the bottom recovers a known affine map of the means within the bound of
tests/test_mllr_cpu.py and scores the adapted model.
"""
import functools

import numpy as np
import pytest

import mllr_restatement as mr
import rasr_amd as ra
from rasr_amd import _capi

pytestmark = pytest.mark.gpu

KINDS = {"full": ("full",), "shift": ("shift",), "both": ("full", "shift")}
N = mr.NO_ID


def model(D, cov):
    """The 20 x 8 model of dimension D: one covariance, three, one per density."""
    if cov == "pooled":
        return ra.synthetic_mixture_set(20, 8, D, seed=100 + D)
    if cov == "cov3":
        return ra.synthetic_mixture_set(20, 8, D, seed=100 + D, n_covariances=3)
    return ra.synthetic_mixture_set(20, 8, D, seed=100 + D, tying="none")


def leaves(n_mixtures, n_leaves):
    """Mixture m on leaf m mod (n_leaves - 1): the last leaf receives no mixture (one leaf: all on leaf 0)."""
    return (np.arange(n_mixtures) % max(n_leaves - 1, 1)).astype(np.uint32)


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


def assert_tables(got, want, what=""):
    """Every table the handle holds equals the restatement's bit for bit."""
    assert got, what
    for name, g in got.items():
        g, w = np.atleast_1d(np.asarray(g, np.float64)), np.atleast_1d(np.asarray(want[name], np.float64))
        assert g.shape == w.shape, (what, name)
        diff = g.view(np.uint64) != w.view(np.uint64)
        assert not diff.any(), f"{what} {name}: {int(diff.sum())} of {diff.size} elements differ"


def assert_sets(acc, ref, what=""):
    held = {n for k in acc.kinds for n in mr.KIND_NAMES[k]}
    for key, row in enumerate(ref):
        for leaf, want in enumerate(row):
            got = acc.tables(key, leaf)
            assert set(got) == held
            assert_tables(got, want, f"{what} key {key} leaf {leaf}")


def is_zero(t):
    return all(not np.any(v) for v in t.values())


N_LEAVES = {3: 1, 39: 3, 45: 5, 80: 3}


@functools.lru_cache(maxsize=None)
def shape_case(D, cov):
    """Three keys interleaved pair by pair (D = 80: two), key 2 of 4 receiving nothing; random f64 weights with a 0 and a
    negative one; 60 frames; N_LEAVES[D] leaves, the last of which no mixture maps to."""
    ms = model(D, cov)
    frames = ra.synthetic_frames(60, D, seed=200 + D)
    n = 150 if D < 80 else 60
    pf, pm, pd = pairs(ms, 60, n, 300 + D)
    live = np.array([0, 1, 3] if D < 80 else [0, 1], np.uint32)
    pk = live[np.arange(n) % len(live)]
    pw = np.random.default_rng(400 + D).uniform(-0.5, 2.0, size=n)
    pw[5], pw[17] = 0.0, -1.25
    n_keys = 4 if D < 80 else 2
    leaf = leaves(20, N_LEAVES[D])
    ref, skipped = mr.accumulate(ms, leaf, N_LEAVES[D], frames, pf, pm, pd, pw, pk, n_keys=n_keys)
    assert skipped == 0
    return dict(ms=ms, leaf=leaf, frames=frames, pf=pf, pm=pm, pd=pd, pk=pk, pw=pw, n_keys=n_keys, ref=ref)


@pytest.mark.parametrize("kinds", ["full", "shift", "both"])
@pytest.mark.parametrize("cov", ["pooled", "cov3", "none"])
@pytest.mark.parametrize("D", [3, 39, 45, 80])
def test_shapes(gpu, D, cov, kinds):
    c = shape_case(D, cov)
    ms, L = c["ms"], N_LEAVES[D]
    assert {"pooled": 1, "cov3": 3, "none": 160}[cov] == ms.n_covariances
    acc = ra.MllrAccumulator(ms, c["leaf"], L, c["n_keys"], max_pairs=256, kinds=KINDS[kinds])
    assert run(gpu, acc, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], c["pk"], stride=D + 5) == 0
    assert_sets(acc, c["ref"])
    cells = {"full": D * (D + 1) + (D + 1) ** 2 + 1, "shift": 1 + 2 * D}
    info = acc.info()
    assert info["kinds"] == KINDS[kinds] and info["table_bytes"] == c["n_keys"] * L * sum(cells[k] for k in KINDS[kinds]) * 8
    if "full" in KINDS[kinds]:  # the full kind counts pairs, not weights
        for key in range(c["n_keys"]):
            for leaf in range(L):
                assert acc.tables(key, leaf)["count_full"] == int(((c["pk"] == key) & (c["leaf"][c["pm"]] == leaf)).sum())
    if D < 80:  # the key that received nothing stays exactly zero
        assert all(is_zero(acc.tables(2, leaf)) for leaf in range(L))
    if L > 1:  # ... and so does the leaf that no mixture maps to
        assert all(is_zero(acc.tables(key, L - 1)) for key in range(c["n_keys"]))
        assert not is_zero(acc.tables(0, 0))
    # reading does not change the handle, and the same call on fresh tables gives the same bits
    assert_sets(acc, c["ref"], "second read")
    acc.reset()
    assert run(gpu, acc, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], c["pk"], stride=D + 5) == 0
    assert_sets(acc, c["ref"], "second run")


@pytest.mark.parametrize("D,n", [(39, 1), (39, 511), (39, 512), (39, 513), (39, 1300), (3, 1300), (45, 1300), (80, 513)])
def test_pair_counts_of_one_set(gpu, D, n):
    """The set (key 1, leaf 1) receives n pairs; the other sets a handful, interleaved: below, at and past the piece
    size."""
    ms = model(D, "cov3")
    leaf = leaves(20, 3)
    frames = ra.synthetic_frames(60, D, seed=500 + D)
    extra = 9
    pf, pm, pd = pairs(ms, 60, n + extra, 600 + D + n)
    pk = np.ones(n + extra, np.uint32)
    pm[:] = 2 * (pm // 2) + 1  # odd mixtures: leaf 1
    at = np.linspace(0, n + extra - 1, extra).astype(np.int64)
    pk[at[::2]] = 0        # key 0, leaf 1
    pm[at[1::2]] -= 1      # key 1, leaf 0
    assert int(((pk == 1) & (leaf[pm] == 1)).sum()) == n
    pw = np.random.default_rng(700 + n).uniform(0.0, 2.0, size=n + extra)
    ref, _ = mr.accumulate(ms, leaf, 3, frames, pf, pm, pd, pw, pk, n_keys=2)
    if n > mr.CHUNK + 1 and D <= 39:  # the piece rule is visible: the sequential order gives other bits
        seq, _ = mr.accumulate(ms, leaf, 3, frames, pf, pm, pd, pw, pk, n_keys=2, chunk=None)
        assert all(np.any(seq[1][1][name] != ref[1][1][name]) for name in ("Z", "G", "beta", "shift"))
    acc = ra.MllrAccumulator(ms, leaf, 3, 2, max_pairs=n + extra, kinds=KINDS["both"])
    assert run(gpu, acc, frames, pf, pm, pd, pw, pk) == 0
    assert_sets(acc, ref)
    assert acc.tables(1, 1)["count_full"] == n


@functools.lru_cache(maxsize=None)
def case39():
    """D = 39, three covariances, 3 keys x 2 leaves (+ an empty one), 1500 pairs: the set (key 0, leaf 0) gets 600 (two
    pieces)."""
    ms = model(39, "cov3")
    leaf = leaves(20, 3)
    frames = ra.synthetic_frames(80, 39, seed=801)
    n = 1500
    pf, pm, pd = pairs(ms, 80, n, 802)
    rng = np.random.default_rng(804)
    pk = rng.integers(0, 3, size=n).astype(np.uint32)
    first = rng.permutation(n)[:600]
    pk[first] = 0
    pm[first] = 2 * (pm[first] // 2)
    other = np.setdiff1d(np.arange(n), first)
    on00 = other[(pk[other] == 0) & (leaf[pm[other]] == 0)]
    pk[on00] = 1
    assert int(((pk == 0) & (leaf[pm] == 0)).sum()) == 600
    pw = np.random.default_rng(803).uniform(0.0, 2.0, size=n)
    ref_w, _ = mr.accumulate(ms, leaf, 3, frames, pf, pm, pd, pw, pk, n_keys=3)
    return dict(ms=ms, leaf=leaf, frames=frames, pf=pf, pm=pm, pd=pd, pk=pk, pw=pw, ref_w=ref_w, n=n)


def acc39(c, max_pairs=1500, kinds="both", n_keys=3):
    return ra.MllrAccumulator(c["ms"], c["leaf"], 3, n_keys, max_pairs=max_pairs, kinds=KINDS[kinds])


def test_null_weights_are_ones_and_null_keys_are_zero(gpu):
    c = case39()
    s = slice(0, 700)
    ref_1, _ = mr.accumulate(c["ms"], c["leaf"], 3, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], None, c["pk"][s], n_keys=3)
    a, b = acc39(c), acc39(c)
    run(gpu, a, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], None, c["pk"][s])
    run(gpu, b, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], np.ones(700), c["pk"][s])
    assert_sets(a, ref_1)
    assert_sets(b, ref_1)
    # no keys: everything on key 0
    ref0, _ = mr.accumulate(c["ms"], c["leaf"], 3, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], c["pw"][s], None, n_keys=3)
    a.reset()
    run(gpu, a, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], c["pw"][s], None)
    assert_sets(a, ref0)
    t = [a.tables(0, leaf) for leaf in range(2)]
    assert sum(x["count_full"] for x in t) == 700 and is_zero(a.tables(1, 0))
    assert sum(x["count_shift"] for x in t) == pytest.approx(c["pw"][s].sum(), rel=1e-12)


def test_two_calls_and_reset(gpu):
    c = case39()
    ms, leaf, n = c["ms"], c["leaf"], c["n"]
    h = 1400  # (key 0, leaf 0) has more than one piece in the first call and continues from its value in the second
    assert int(((c["pk"][:h] == 0) & (leaf[c["pm"][:h]] == 0)).sum()) > mr.CHUNK
    cut = [slice(0, h), slice(h, n)]
    args = [(c["pf"][s], c["pm"][s], c["pd"][s], c["pw"][s], c["pk"][s]) for s in cut]
    first, _ = mr.accumulate(ms, leaf, 3, c["frames"], *args[0], n_keys=3)
    both, _ = mr.accumulate(ms, leaf, 3, c["frames"], *args[1], n_keys=3, tables=first)
    assert np.any(both[0][0]["G"] != c["ref_w"][0][0]["G"])  # not the one-call sum: the pieces fall differently
    acc = acc39(c)
    run(gpu, acc, c["frames"], *args[0])
    assert_sets(acc, first, "first call")
    run(gpu, acc, c["frames"], *args[1])
    assert_sets(acc, both, "second call")
    acc.reset()
    assert acc.skipped == 0
    assert all(is_zero(acc.tables(key, lf)) for key in range(3) for lf in range(3))
    run(gpu, acc, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], c["pk"])
    assert_sets(acc, c["ref_w"], "after reset")


def test_host_call_equals_device_call(gpu):
    c = case39()
    host = acc39(c)
    padded = np.full((80, 44), np.nan, np.float32)
    padded[:, :39] = c["frames"]
    host.accumulate_host(padded, c["pf"], c["pm"], c["pd"], c["pw"], c["pk"])
    assert_sets(host, c["ref_w"], "host")
    dev = acc39(c)
    run(gpu, dev, c["frames"], c["pf"], c["pm"], c["pd"], c["pw"], c["pk"])
    for key in range(3):
        for leaf in range(3):
            assert_tables(host.tables(key, leaf), dev.tables(key, leaf))


def test_add(gpu):
    c = case39()
    ms, leaf, n = c["ms"], c["leaf"], c["n"]
    half = [slice(0, 750), slice(750, n)]
    args = [(c["pf"][s], c["pm"][s], c["pd"][s], c["pw"][s], c["pk"][s]) for s in half]
    refs = [mr.accumulate(ms, leaf, 3, c["frames"], *a, n_keys=3)[0] for a in args]
    a, b = acc39(c), acc39(c)
    run(gpu, b, c["frames"], *args[1])
    for weight in (1.0, 0.5):
        a.reset()
        run(gpu, a, c["frames"], *args[0])
        for key in range(3):
            for lf in range(3):
                a.add(key, lf, b.tables(key, lf), weight)
                assert_tables(a.tables(key, lf), mr.add(refs[0][key][lf], refs[1][key][lf], weight), f"weight {weight}")
    # the counts are added with no weight
    assert a.tables(0, 0)["count_full"] == refs[0][0][0]["count_full"] + refs[1][0][0]["count_full"]
    # a handle of one kind takes only that kind's tables
    only = acc39(c, kinds="shift")
    t = b.tables(1, 1)
    only.add(1, 1, {n: t[n] for n in mr.KIND_NAMES["shift"]})
    assert_tables(only.tables(1, 1), {n: t[n] for n in mr.KIND_NAMES["shift"]})
    with pytest.raises(ra.GmmError) as err:
        only.add(1, 1, t)
    assert err.value.code == _capi.GMM_ERR_INVALID_ARGUMENT


def test_skipped_pairs_and_poisoned_frame(gpu):
    c = case39()
    ms, leaf = c["ms"], c["leaf"]
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
    ref, skipped = mr.accumulate(ms, leaf, 3, frames, pf, pm, pd, pw, pk, n_keys=3)
    assert skipped == len(bad)
    clean, _ = mr.accumulate(ms, leaf, 3, c["frames"], c["pf"][:300], c["pm"][:300], c["pd"][:300], c["pw"][:300],
                             c["pk"][:300], n_keys=3)
    acc = acc39(c, max_pairs=400)
    assert run(gpu, acc, frames, pf, pm, pd, pw, pk) == len(bad)
    assert_sets(acc, clean)
    assert all(np.all(np.isfinite(v)) for key in range(3) for lf in range(3) for v in acc.tables(key, lf).values())
    assert_sets(acc, ref)


@pytest.mark.parametrize("kind", ["SIMD-diagonal-maximum", "diagonal-maximum"])
def test_density_from_the_scorer(gpu, kind):
    import torch
    counts = np.array([3, 9, 1, 5, 0, 7, 2, 9, 4, 6, 8, 1])  # mixture 4 is empty
    ms = ra.synthetic_mixture_set(12, counts, 39, seed=11, n_covariances=3, weights="random")
    leaf = leaves(12, 3)
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
    with_scorer = ra.MllrAccumulator(ms, leaf, 3, 2, max_pairs=128, kinds=KINDS["both"])
    assert run(gpu, with_scorer, frames, pf, pm, pk=pk, scorer=sc) == 2
    given = ra.MllrAccumulator(ms, leaf, 3, 2, max_pairs=128, kinds=KINDS["both"])
    assert run(gpu, given, frames, pf, pm, best, pk=pk) == 2
    ref, skipped = mr.accumulate(ms, leaf, 3, frames, pf, pm, best, None, pk, n_keys=2)
    assert skipped == 2
    for key in range(2):
        for lf in range(3):
            assert_tables(with_scorer.tables(key, lf), given.tables(key, lf))
    assert_sets(with_scorer, ref)
    assert all(np.all(np.isfinite(v)) for lf in range(3) for v in with_scorer.tables(0, lf).values())


def test_refusals_leave_the_tables_untouched(gpu):
    c = case39()
    ms, leaf = c["ms"], c["leaf"]
    acc = acc39(c, max_pairs=300)
    s = slice(0, 300)
    run(gpu, acc, c["frames"], c["pf"][s], c["pm"][s], c["pd"][s], c["pw"][s], c["pk"][s])
    before = [[acc.tables(key, lf) for lf in range(3)] for key in range(3)]

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
        for lf in range(3):
            assert_tables(acc.tables(key, lf), before[key][lf])
    assert acc.skipped == 0
    for key, lf in ((3, 0), (0, 3)):
        assert code(lambda: acc.tables(key, lf))[0] == _capi.GMM_ERR_INVALID_ARGUMENT
    # a handle too large for the device: 2^22 keys x 3 leaves x 25 KiB is a third of a terabyte; the message names it
    rc, msg = code(lambda: ra.MllrAccumulator(ms, leaf, 3, 1 << 22, max_pairs=300))
    assert rc == _capi.GMM_ERR_UNSUPPORTED and "GiB" in msg and "4194304 keys" in msg
    # a dimension past GMM_MLLR_MAX_DIMENSION
    wide = ra.synthetic_mixture_set(2, 2, 257, seed=1)
    rc, msg = code(lambda: ra.MllrAccumulator(wide, [0, 0], 1, 1, max_pairs=8))
    assert rc == _capi.GMM_ERR_UNSUPPORTED and "257" in msg
    # no keys, no leaves, no kinds, a leaf index past the leaves
    assert code(lambda: ra.MllrAccumulator(ms, leaf, 3, 0, max_pairs=8))[0] == _capi.GMM_ERR_INVALID_ARGUMENT
    assert code(lambda: ra.MllrAccumulator(ms, leaf, 0, 1, max_pairs=8))[0] == _capi.GMM_ERR_INVALID_ARGUMENT
    assert code(lambda: ra.MllrAccumulator(ms, leaf, 3, 1, max_pairs=8, kinds=()))[0] == _capi.GMM_ERR_INVALID_ARGUMENT
    rc, msg = code(lambda: ra.MllrAccumulator(ms, leaf, 1, 1, max_pairs=8))
    assert rc == _capi.GMM_ERR_INVALID_ARGUMENT and "leaf 1" in msg
    # one density per mixture: no scorer and no density needed
    single = ra.synthetic_mixture_set(6, 1, 39, seed=6, n_covariances=2)
    a1 = ra.MllrAccumulator(single, leaves(6, 3), 3, 1, max_pairs=64, kinds=KINDS["both"])
    f1, m1 = c["pf"][:64], (c["pm"][:64] % 6).astype(np.uint32)
    assert run(gpu, a1, c["frames"], f1, m1) == 0
    assert_sets(a1, mr.accumulate(single, leaves(6, 3), 3, c["frames"], f1, m1, np.zeros(64, np.uint32))[0])


def test_end_to_end_known_map(gpu):
    """Per key, frames that are EXACTLY A mu + b of a drawn density's mean (means, A and b on a coarse binary grid, so
    that the f32 frames and the f64 tables are exact): accumulated with the true densities, estimated per leaf and
    applied.  The recovered [b A] meets the bound of tests/test_mllr_cpu.py against the true map, and the mean
    diagonal-maximum score of the frames on the adapted model's scorer lies below the unadapted one."""
    from test_mllr_cpu import C_BOUND, retained_cond
    D, n_per_key, n_keys = 8, 400, 2
    rng = np.random.default_rng(901)
    base = ra.synthetic_mixture_set(10, 8, D, seed=902, n_covariances=3)
    ms = ra.MixtureSet(means=rng.integers(-24, 25, size=(80, D)) / 8.0, variances=base.variances,
                       density_mean=base.density_mean, density_covariance=base.density_covariance,
                       mixture_offsets=base.mixture_offsets, mixture_densities=base.mixture_densities,
                       mixture_log_weights=base.mixture_log_weights)
    leaf = (np.arange(10) // 5).astype(np.uint32)  # two leaves of 40 means each
    tree = {"left": [1, N, N], "right": [2, N, N], "parent": [N, 0, 0], "leaf_number": [N, 0, 1], "root": 0}
    frames, pm, pd, pk, maps = [], [], [], [], []
    for key in range(n_keys):
        A = np.eye(D) * (1.25 + 0.5 * key) + rng.integers(-2, 3, size=(D, D)) / 16.0
        b = rng.integers(-8, 9, size=D) / 8.0 * (1 + key)
        maps.append(np.concatenate([b[:, None], A], axis=1))
        m = rng.integers(0, 10, size=n_per_key)
        d = rng.integers(0, 8, size=n_per_key)
        mu = ms.means[ms.density_mean[ms.mixture_densities[ms.mixture_offsets[m] + d]]].astype(np.float64)
        x = mu @ A.T + b
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)  # exact in f32
        frames.append(x)
        pm.append(m)
        pd.append(d)
        pk.append(np.full(n_per_key, key))
    frames = np.concatenate(frames).astype(np.float32)
    pm, pd, pk = (np.concatenate(a).astype(np.uint32) for a in (pm, pd, pk))
    pf = np.arange(len(frames), dtype=np.uint32)
    acc = ra.MllrAccumulator(ms, leaf, 2, n_keys, max_pairs=len(frames), kinds=KINDS["both"])
    assert run(gpu, acc, frames, pf, pm, pd, None, pk) == 0
    sc = ra.Scorer(ms, "diagonal-maximum", max_frames=n_per_key)

    def mean_score(scorer, sel):
        scores = scorer.score_host(np.ascontiguousarray(frames[sel]), want_best=False)
        scores = scores[0] if isinstance(scores, tuple) else scores
        return float(np.mean(scores[pm[sel], np.arange(int(sel.sum()))]))
    for key in range(n_keys):
        sel = pk == key
        t = acc.leaf_tables(key)
        for lf in range(2):  # at least D + 2 distinct means hit per node
            assert len({(int(a), int(b)) for a, b in zip(pm[sel & (leaf[pm] == lf)], pd[sel & (leaf[pm] == lf)])}) >= D + 2
        est = ra.estimate_mllr(t, leaf, tree, (), min_observation=50.0, kind="full")
        assert list(est["ids"]) == [1, 2] and list(est["matrix_of_mixture"]) == [1] * 5 + [2] * 5
        for lf in range(2):
            cond, kept = retained_cond(t[lf]["G"])
            assert kept == D + 1 and cond <= 1e4
            err = np.abs(est["matrices"][lf] - maps[key]).max()
            bound = C_BOUND * (D + 1) * cond * 2.0 ** -52 * np.abs(maps[key]).max()
            print(f"key {key} leaf {lf}: cond2 {cond:.3g} |W - [b A]| {err:.3g} bound {bound:.3g}")
            assert err <= bound, (key, lf, err, bound)
        adapted = ra.adapt_means(ms, est)
        assert adapted.n_covariances == ms.n_covariances and not np.array_equal(adapted.means, ms.means)
        adapted_sc = ra.Scorer(adapted, "diagonal-maximum", max_frames=n_per_key)
        before, after = mean_score(sc, sel), mean_score(adapted_sc, sel)
        assert after < before, (key, before, after)
        # the shift kind of the same statistics moves the means the right way too
        shifted = ra.adapt_means(ms, ra.estimate_mllr(t, leaf, tree, (), min_observation=50.0, kind="shift"))
        assert mean_score(ra.Scorer(shifted, "diagonal-maximum", max_frames=n_per_key), sel) < before
