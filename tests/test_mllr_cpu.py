"""The MLLR mean transform contract on the CPU (include/rasr_gmm_mllr.h): the numpy restatement
(tests/mllr_restatement.py) against a closed form on exact inputs, the piece rule against the sequential order, the
non-symmetric rounding of G, and gmm_mllr_estimate / gmm_mllr_adapt_means (host only) against the restatement.  No GPU.

The estimate's bound.  W = Z pinv(G) in f64: a backward stable pseudo-inverse and the product of D+1 terms err by the
order of (D+1) * cond2(G) * 2^-52 relative to max|W|, for the library's one-sided Jacobi SVD and for numpy's LAPACK
SVD alike, so |W - W_ref| <= C * (D+1) * cond2(G) * 2^-52 * max|W_ref| with cond2 taken over the retained singular
values.  cond2(G) <= 1e4 is a condition on the inputs, asserted.  C was measured once over every estimated matrix of
this file (the largest ratio: 1.15, at D = 3 with cond2 = 1.4; at most 0.17 at D = 16 and 39) and is fixed at ten times that, 12.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import mllr_restatement as mr
import rasr_amd as ra
from rasr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = mr.NO_ID
C_BOUND = 12.0

# 7 ids, 4 leaves: 0 = (1, 2), 1 = (3, 4), 2 = (5, 6); the leaf ids 3 .. 6 carry the leaf numbers 0 .. 3
TREE7 = {"left": [1, 3, 5, N, N, N, N], "right": [2, 4, 6, N, N, N, N], "parent": [N, 0, 0, 1, 1, 2, 2],
         "leaf_number": [N, N, N, 0, 1, 2, 3], "root": 0}
TREE1 = {"left": [N], "right": [N], "parent": [N], "leaf_number": [0], "root": 0}


def _exact_case():
    """Small-integer features and means, power-of-two variances and weights: every term and every sum is exact."""
    rng = np.random.default_rng(3)
    D, n_dens = 4, 6
    means = rng.integers(-4, 5, size=(n_dens, D)).astype(np.float32)
    variances = (2.0 ** rng.integers(-2, 3, size=(3, D))).astype(np.float32)
    ms = ra.MixtureSet(means=means, variances=variances, density_mean=np.arange(n_dens),
                       density_covariance=np.arange(n_dens) % 3, mixture_offsets=[0, 2, 3, 6],
                       mixture_densities=np.arange(n_dens), mixture_log_weights=np.zeros(n_dens))
    frames = rng.integers(-8, 9, size=(40, D)).astype(np.float32)
    n = 1400
    pf = rng.integers(0, 40, size=n).astype(np.uint32)
    pm = (rng.random(n) < 0.85).astype(np.uint32) * 2  # mixture 2 (leaf 1) gets about 1190 pairs: more than two pieces
    pm[rng.random(n) < 0.05] = 1
    pd = (rng.integers(0, 1 << 20, size=n) % np.diff(ms.mixture_offsets.astype(np.int64))[pm]).astype(np.uint32)
    pk = (rng.random(n) < 0.95).astype(np.uint32)
    pw = (2.0 ** rng.integers(-2, 2, size=n)) * rng.choice([1.0, 1.0, -1.0], size=n)
    return ms, np.array([0, 0, 1]), frames, pf, pm, pd, pk, pw


@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_against_closed_form(weighted):
    ms, leaf, frames, pf, pm, pd, pk, pw = _exact_case()
    if not weighted:
        pw = None
    tables, skipped = mr.accumulate(ms, leaf, 2, frames, pf, pm, pd, pw, pk, n_keys=2)
    assert skipped == 0 and int(((pk == 1) & (pm == 2)).sum()) > 2 * mr.CHUNK
    dens = ms.mixture_densities[ms.mixture_offsets[pm].astype(np.int64) + pd]
    x = frames[pf].astype(np.float64)
    mu = ms.means[ms.density_mean[dens]].astype(np.float64)
    m = np.concatenate([np.ones((len(pf), 1)), mu], axis=1)
    v = ms.variances[ms.density_covariance[dens]].astype(np.float64)
    w = np.ones(len(pf)) if pw is None else pw
    for key in range(2):
        for lf in range(2):
            s = (pk == key) & (leaf[pm] == lf)
            got = tables[key][lf]
            assert np.array_equal(got["Z"], np.einsum("n,ni,nj->ij", w[s], x[s], m[s]))
            assert np.array_equal(got["G"], np.einsum("n,ni,nj->ij", w[s], m[s], m[s]))
            assert got["count_full"] == s.sum() and got["count_shift"] == w[s].sum()
            assert np.array_equal(got["beta"], (w[s, None] / v[s]).sum(axis=0))
            assert np.array_equal(got["shift"], (w[s, None] * (x[s] - mu[s]) / v[s]).sum(axis=0))


@functools.lru_cache(maxsize=None)
def _random_model(D):
    """10 mixtures x 100 densities; the mixtures 2 l and 2 l + 1 on leaf l (5 leaves)."""
    ms = ra.synthetic_mixture_set(10, 100, D, seed=50 + D, n_covariances=3)
    return ms, np.arange(10) // 2


@pytest.mark.parametrize("n", [513, 1300])
def test_piece_rule_against_sequential_order(n):
    ms, _ = _random_model(5)
    leaf = np.zeros(10, np.int64)
    frames = ra.synthetic_frames(n, 5, seed=61)
    rng = np.random.default_rng(62 + n)
    pf = np.arange(n, dtype=np.uint32)
    pm = rng.integers(0, 10, size=n).astype(np.uint32)
    pd = rng.integers(0, 100, size=n).astype(np.uint32)
    pw = rng.uniform(0.0, 2.0, size=n)
    ((pieces,),), _ = mr.accumulate(ms, leaf, 1, frames, pf, pm, pd, pw)
    ((seq,),), _ = mr.accumulate(ms, leaf, 1, frames, pf, pm, pd, pw, chunk=None)
    # 1300 pairs: two different sums, a kernel that summed sequentially would not be bit-equal to the contract.  513
    # pairs: the second piece is one pair, 0 + t = t exactly, so the two orders are the same sum and must agree.
    for name in ("Z", "G", "count_shift", "beta", "shift"):
        assert np.any(pieces[name] != seq[name]) == (n == 1300), name
    assert pieces["count_full"] == seq["count_full"] == n  # a count of pairs: exact either way
    # ... within the standard bound between two summation orders of n terms, 2 n 2^-53 sum |term|
    dens = ms.mixture_densities[ms.mixture_offsets[pm].astype(np.int64) + pd]
    x = frames.astype(np.float64)
    mu32 = ms.means[ms.density_mean[dens]]
    m = np.concatenate([np.ones((n, 1)), mu32.astype(np.float64)], axis=1)
    v = ms.variances[ms.density_covariance[dens]].astype(np.float64)
    c = 2 * n * 2.0 ** -53
    terms = {"Z": np.abs(pw[:, None, None] * x[:, :, None] * m[:, None, :]),
             "G": np.abs(pw[:, None, None] * m[:, :, None] * m[:, None, :]), "count_shift": pw,
             "beta": pw[:, None] / v, "shift": np.abs(pw[:, None] * (frames - mu32).astype(np.float64) / v)}
    for name, t in terms.items():
        assert np.all(np.abs(pieces[name] - seq[name]) <= c * t.sum(axis=0)), name


def test_g_rounds_differently_in_its_two_triangles():
    """(w * m_i) * m_j != (w * m_j) * m_i for some inputs: the contract accumulates all (D+1)^2 cells of G and mirrors
    nothing, so G is symmetric only up to rounding."""
    ms, leaf = _random_model(5)
    frames = ra.synthetic_frames(50, 5, seed=63)
    rng = np.random.default_rng(64)
    pf, pm, pd = (rng.integers(0, hi, size=50).astype(np.uint32) for hi in (50, 10, 100))
    pw = rng.uniform(0.1, 2.0, size=50)
    # one pair shows it already ...
    mu = ms.means[ms.density_mean[ms.mixture_densities[ms.mixture_offsets[pm[0]] + pd[0]]]].astype(np.float64)
    one = (pw[0] * mu)[:, None] * mu[None, :]
    assert np.any(one != one.T)
    # ... and the accumulated table keeps the difference, which a mirrored upper triangle would lose
    tables, _ = mr.accumulate(ms, np.zeros(10, np.int64), 1, frames, pf, pm, pd, pw)
    G = tables[0][0]["G"]
    assert np.any(G != G.T) and np.allclose(G, G.T, rtol=1e-13, atol=0)
    assert np.array_equal(G[0, :], G[:, 0])  # the row and the column of m_0 = 1.0 agree: (w * 1) * m_j, (w * m_j) * 1


LEAF_PAIRS = [300, 40, 250, 260, 120]  # pairs per leaf; leaf 4 lies outside TREE7 (the silence leaf)


@functools.lru_cache(maxsize=None)
def leaf_case(D):
    """Leaf tables of one key from the restatement: LEAF_PAIRS pairs per leaf, frames an affine map of the density's mean
    plus noise."""
    ms, leaf = _random_model(D)
    rng = np.random.default_rng(80 + D)
    pm = np.concatenate([rng.integers(2 * l, 2 * l + 2, size=n) for l, n in enumerate(LEAF_PAIRS)]).astype(np.uint32)
    rng.shuffle(pm)
    n = len(pm)
    pd = rng.integers(0, 100, size=n).astype(np.uint32)
    A = np.eye(D) * 1.2 + 0.1 * rng.standard_normal((D, D))
    mu = ms.means[ms.density_mean[ms.mixture_densities[ms.mixture_offsets[pm].astype(np.int64) + pd]]]
    frames = (mu @ A.T + rng.standard_normal(D) + 0.2 * rng.standard_normal((n, D))).astype(np.float32)
    pw = rng.uniform(0.5, 1.5, size=n)
    tables, skipped = mr.accumulate(ms, leaf, 5, frames, np.arange(n, dtype=np.uint32), pm, pd, pw)
    assert skipped == 0 and [t["count_full"] for t in tables[0]] == LEAF_PAIRS
    return ms, leaf, tables[0]


def retained_cond(G):
    """(cond2 over the singular values pinv keeps, the kept count); the values must lie clear of the 1e-12 threshold."""
    s = np.linalg.svd(G, compute_uv=False)
    assert np.all((s > 1e-6 * s[0]) | (s < 1e-14 * s[0])), s / s[0]
    kept = s[s > 1e-12 * s[0]]
    return kept[0] / kept[-1], len(kept)


def assert_estimate(got, ref, node_tables):
    """ids and the assignment identical; every matrix inside the module docstring's bound (shift: bit-equal)."""
    assert np.array_equal(got["ids"], ref["ids"]) and got["ids"].dtype == np.uint32
    assert np.array_equal(got["matrix_of_mixture"], ref["matrix_of_mixture"])
    assert got["matrices"].shape == ref["matrices"].shape
    worst = 0.0
    for i, w, w_ref in zip(ref["ids"], got["matrices"], ref["matrices"]):
        t = node_tables.get(int(i))
        if ref["kind"] == "shift" or t is None:  # one division per element; the unit matrix
            assert np.array_equal(w.view(np.uint64), w_ref.view(np.uint64)), int(i)
            continue
        cond, _ = retained_cond(t["G"])
        assert cond <= 1e4, cond
        unit = (w.shape[1]) * cond * 2.0 ** -52 * np.abs(w_ref).max()
        ratio = np.abs(w - w_ref).max() / unit
        print(f"D {w.shape[0]} id {int(i)} cond2 {cond:.3g} error / ((D+1) cond2 2^-52 max|W|) = {ratio:.3g}")
        worst = max(worst, ratio)
    assert worst <= C_BOUND, worst


def node_tables_of(ref, leaf_tables, leaf, tree, silence, min_obs, min_sil, kind):
    """The tables every estimated (not unit) matrix of `ref` was made from, by id."""
    names = mr.KIND_NAMES[kind]
    count = names[2] if kind == "full" else names[0]
    node = mr.propagate(leaf_tables, tree, names)
    out = {i: t for i, t in node.items() if t[count] > min_obs}
    for s, m in enumerate(sorted(silence)):
        t = leaf_tables[int(leaf[m])]
        if t[count] > min_sil:
            out[len(tree["left"]) + s] = t
    return {i: t for i, t in out.items() if i in set(int(x) for x in ref["ids"])}


# (min_observation, silence mixtures, min_silence_observation, the ids expected)
TREE7_CASES = {
    "root below threshold": (1e9, [8], 1e9, [0, 7]),
    "one leaf takes its parent": (100.0, [8], 100.0, [1, 3, 5, 6, 7]),
    "both children below, parent above": (270.0, [], 0.0, None),
    "both children below, grandparent above": (520.0, [8], 119.5, [0, 7]),
    "count equal to the threshold": (300.0, [8], 120.0, [1, 2, 7]),
    "two silence mixtures on one leaf": (100.0, [8, 9], 100.0, [1, 3, 5, 6, 7, 8]),
}


@pytest.mark.parametrize("kind", ["full", "shift"])
@pytest.mark.parametrize("case", sorted(TREE7_CASES))
@pytest.mark.parametrize("D", [3, 16, 39])
def test_estimate_against_restatement(built, D, case, kind):
    ms, leaf, tables = leaf_case(D)
    min_obs, silence, min_sil, want_ids = TREE7_CASES[case]
    if kind == "shift":  # the shift kind counts weights: thresholds between the same leaves, on its own counts
        cs = np.array([t["count_shift"] for t in tables])
        min_obs = {1e9: 1e9, 100.0: (cs[1] + cs[4]) / 2, 270.0: (cs[3] + cs[0]) / 2, 520.0: cs[2] + cs[3] + 1.0,
                   300.0: cs[0]}[min_obs]
        min_sil = {1e9: 1e9, 100.0: cs[4] - 1.0, 0.0: 0.0, 119.5: cs[4] - 0.5, 120.0: cs[4]}[min_sil]
    if not silence:  # leaf 4 is then outside everything: its mixtures must not be asked for
        keep = leaf < 4
        leaf = leaf[keep]
    ref = mr.estimate(tables, leaf, TREE7, silence, min_obs, min_sil, kind)
    got = ra.estimate_mllr(tables, leaf, TREE7, silence, min_obs, min_sil, kind)
    if want_ids is not None:
        assert list(ref["ids"]) == want_ids
    else:
        assert list(ref["ids"]) == [1, 2, 3] and list(ref["matrix_of_mixture"][:8]) == [3, 3, 1, 1, 2, 2, 2, 2]
    assert_estimate(got, ref, node_tables_of(ref, tables, leaf, TREE7, silence, min_obs, min_sil, kind))
    if case == "root below threshold":
        unit = mr.unit_matrix(D, kind)
        assert np.array_equal(got["matrices"][0], unit) and np.array_equal(got["matrices"][1], unit)
        assert set(got["matrix_of_mixture"][:8]) == {0} and set(got["matrix_of_mixture"][8:]) == {7}
    if case == "count equal to the threshold":  # neither leaf 0 nor the silence leaf is estimated from its own tables
        assert got["matrix_of_mixture"][0] == 1 and np.array_equal(got["matrices"][2], mr.unit_matrix(D, kind))
    if case == "two silence mixtures on one leaf":  # the later one serves the leaf; both are estimated alike
        assert set(got["matrix_of_mixture"][8:]) == {8}
        assert np.array_equal(got["matrices"][4], got["matrices"][5])


@pytest.mark.parametrize("kind", ["full", "shift"])
@pytest.mark.parametrize("D", [3, 16, 39])
def test_estimate_single_leaf_tree(built, D, kind):
    ms, _, tables = leaf_case(D)
    leaf = np.zeros(10, np.uint32)
    for min_obs in (100.0, 1e9):
        ref = mr.estimate(tables[:1], leaf, TREE1, (), min_obs, 0.0, kind)
        got = ra.estimate_mllr(tables[:1], leaf, TREE1, (), min_obs, 0.0, kind)
        assert list(got["ids"]) == [0] and set(got["matrix_of_mixture"]) == {0}
        assert_estimate(got, ref, {0: tables[0]} if min_obs < 1e9 else {})


def test_estimate_rank_deficient_g(built):
    """Fewer than D+1 affinely independent means: 10 distinct integer means at D = 16, so G (exact) has rank 10 of 17 and
    pinv drops seven singular values, which lie clear of the threshold in both implementations."""
    D = 16
    rng = np.random.default_rng(90)
    means = rng.integers(-3, 4, size=(10, D)).astype(np.float32)
    ms = ra.MixtureSet(means=means, variances=np.ones((1, D), np.float32), density_mean=np.arange(10),
                       density_covariance=np.zeros(10), mixture_offsets=[0, 10], mixture_densities=np.arange(10),
                       mixture_log_weights=np.zeros(10))
    n = 60
    pd = (np.arange(n) % 10).astype(np.uint32)
    frames = (means[pd] @ (np.eye(D) * 1.5 + 0.1 * rng.standard_normal((D, D))).T + 0.5).astype(np.float32)
    tables, _ = mr.accumulate(ms, [0], 1, frames, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32), pd)
    cond, kept = retained_cond(tables[0][0]["G"])
    assert kept == 10 and cond <= 1e4
    ref = mr.estimate(tables[0], [0], TREE1, (), 10.0, 0.0, "full")
    got = ra.estimate_mllr(tables[0], [0], TREE1, (), 10.0, 0.0, "full")
    assert_estimate(got, ref, {0: tables[0][0]})
    assert np.abs(got["matrices"][0]).max() < 1e3  # nothing of the dropped directions' 1 / sigma came through


@pytest.mark.parametrize("kind", ["full", "shift"])
def test_adapt_means_against_restatement(built, kind):
    ms, leaf, tables = leaf_case(16)
    est = ra.estimate_mllr(tables, leaf, TREE7, [8], 100.0, 100.0, kind)
    adapted = ra.adapt_means(ms, est)
    want = mr.adapt_means(ms, est)
    assert adapted.means.dtype == np.float32 and np.array_equal(adapted.means.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(adapted.means, ms.means) and adapted is not ms
    for name in ("variances", "density_mean", "density_covariance", "mixture_offsets", "mixture_densities",
                 "mixture_log_weights"):
        assert np.array_equal(getattr(adapted, name), getattr(ms, name))
    # an unreferenced mean is copied: the model's means plus two that no density names
    extra = ra.MixtureSet(means=np.concatenate([ms.means, np.full((2, 16), 7.25, np.float32)]), variances=ms.variances,
                          density_mean=ms.density_mean, density_covariance=ms.density_covariance,
                          mixture_offsets=ms.mixture_offsets, mixture_densities=ms.mixture_densities,
                          mixture_log_weights=ms.mixture_log_weights)
    out = ra.adapt_means(extra, est).means
    assert np.array_equal(out[:-2], want) and np.all(out[-2:] == 7.25)
    # a mean that two entries name is refused, naming the mean
    dm = ms.density_mean.copy()
    dm[5] = 3
    shared = ra.MixtureSet(means=ms.means, variances=ms.variances, density_mean=dm,
                           density_covariance=ms.density_covariance, mixture_offsets=ms.mixture_offsets,
                           mixture_densities=ms.mixture_densities, mixture_log_weights=ms.mixture_log_weights)
    with pytest.raises(ra.GmmError) as e:
        ra.adapt_means(shared, est)
    assert e.value.code == _capi.GMM_ERR_UNSUPPORTED and "mean 3" in str(e.value)
    # a mixture whose matrix id is not given
    bad = dict(est, matrix_of_mixture=np.where(np.arange(10) == 4, 99, est["matrix_of_mixture"]))
    with pytest.raises(ra.GmmError) as e:
        ra.adapt_means(ms, bad)
    assert e.value.code == _capi.GMM_ERR_INVALID_ARGUMENT and "mixture 4" in str(e.value)


def test_malformed_trees_are_refused(built):
    ms, leaf, tables = leaf_case(3)

    def refused(tree, word, silence=(8,), leaf_of_mixture=leaf):
        with pytest.raises(ra.GmmError) as e:
            ra.estimate_mllr(tables, leaf_of_mixture, tree, silence, 100.0, 100.0, "full")
        assert e.value.code == _capi.GMM_ERR_INVALID_ARGUMENT and word in str(e.value), str(e.value)

    def changed(name, at, value):
        t = {k: (list(v) if k != "root" else v) for k, v in TREE7.items()}
        if name == "root":
            t["root"] = value
        else:
            t[name][at] = value
        return t
    refused(changed("right", 2, 1), "id 1 is reached twice")  # a cycle: id 1 below id 2 as well
    refused(changed("left", 1, 0), "id 0 is reached twice")   # back to the root
    refused(changed("left", 2, 7), "id 2 has a child out of range")
    refused(changed("leaf_number", 5, 5), "leaf id 5")
    refused(changed("parent", 0, 2), "root id 0 has a parent")
    refused(changed("right", 1, N), "id 1 has one child")
    refused(changed("parent", 6, 1), "parent of id 6")
    refused(changed("root", 0, 9), "root id 9")
    refused(TREE7, "mixture 8", silence=())  # leaf 4 is covered by nothing
    refused(TREE7, "silence mixture 10", silence=(10,))
    refused(TREE7, "not ascending", silence=(9, 8))
    refused(TREE7, "mixture 2 maps to leaf 5", leaf_of_mixture=np.where(np.arange(10) == 2, 5, leaf))


def test_mllr_symbols_are_bound(built):
    lib = ra.load_library()
    names = {p[0] for p in _capi.PROTOTYPES}
    for n in ["gmm_mllr_create", "gmm_mllr_destroy", "gmm_mllr_reset", "gmm_mllr_accumulate_device",
              "gmm_mllr_accumulate_host", "gmm_mllr_skipped", "gmm_mllr_info", "gmm_mllr_get", "gmm_mllr_add",
              "gmm_mllr_estimate", "gmm_mllr_adapt_means"]:
        assert n in names and hasattr(lib, n), n
    header = open(os.path.join(ROOT, "include", "rasr_gmm_mllr.h")).read()
    assert "#define GMM_MLLR_CHUNK 512" in header and _capi.GMM_MLLR_CHUNK == mr.CHUNK == 512
    assert "#define GMM_MLLR_MAX_DIMENSION 256" in header
    assert ra.MllrAccumulator is not None and ra.MLLR_KINDS == {"full": 1, "shift": 2}


def test_mllr_estimate_cpp_program(built):
    """tests/cpp/mllr_estimate_test.cc: the estimate unit alone as a stand-alone program (built by make)."""
    r = subprocess.run([os.path.join(ROOT, "build", "tests", "mllr_estimate_test")], capture_output=True, text=True)
    assert r.returncode == 0 and "mllr_estimate_test: ok" in r.stdout, r.stdout + r.stderr
