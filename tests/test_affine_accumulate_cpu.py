"""The affine feature transform contract on the CPU (include/rasr_gmm_adaptation.h): the numpy restatement
(tests/affine_restatement.py) against a closed form on exact inputs, the piece rule against the sequential order, and
gmm_affine_estimate (host only) against the restatement's estimate.  No GPU.

The estimate's bound: under cond2(G[i]) <= 1e4, which the test checks on its inputs first, an f64 solve errs by the
order of (D+1) * cond * 2^-53 < 1e-10 relative, and five sweeps stay below 1e-9: far inside an f32 ulp (6e-8), so the
library's f32 rows may differ from the narrowed restatement only by the narrowing itself,
|W - W_ref| <= ulp32(max|W_ref[i]|) for every element of row i.
"""
import os
import subprocess

import numpy as np
import pytest

import affine_restatement as ar
import rasr_amd as ra
from rasr_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exact_case(n_cov):
    """Small-integer features and means, power-of-two variances and weights: every term and every sum is exact."""
    rng = np.random.default_rng(3)
    D, n_dens = 4, 6
    means = rng.integers(-4, 5, size=(n_dens, D)).astype(np.float32)
    variances = (2.0 ** rng.integers(-2, 3, size=(n_cov, D))).astype(np.float32)
    dcov = np.arange(n_dens) % n_cov
    ms = ra.MixtureSet(means=means, variances=variances, density_mean=np.arange(n_dens), density_covariance=dcov,
                       mixture_offsets=[0, 2, 3, 6], mixture_densities=np.arange(n_dens),
                       mixture_log_weights=np.zeros(n_dens))
    frames = rng.integers(-8, 9, size=(40, D)).astype(np.float32)
    n = 1200  # more than two pieces of one key
    pf = rng.integers(0, 40, size=n).astype(np.uint32)
    pm = rng.integers(0, 3, size=n).astype(np.uint32)
    pd = (rng.integers(0, 1 << 20, size=n) % np.diff(ms.mixture_offsets.astype(np.int64))[pm]).astype(np.uint32)
    pk = (rng.random(n) < 0.9).astype(np.uint32)  # key 1 gets about 1080 pairs, key 0 the rest
    pw = (2.0 ** rng.integers(-2, 2, size=n)) * rng.choice([1.0, 1.0, -1.0], size=n)
    return ms, frames, pf, pm, pd, pk, pw


@pytest.mark.parametrize("n_cov", [1, 3])
@pytest.mark.parametrize("weighted", [False, True])
def test_restatement_against_closed_form(n_cov, weighted):
    ms, frames, pf, pm, pd, pk, pw = _exact_case(n_cov)
    if not weighted:
        pw = None
    tables, skipped = ar.accumulate(ms, frames, pf, pm, pd, pw, pk, n_keys=2)
    assert skipped == 0 and int((pk == 1).sum()) > 2 * ar.CHUNK
    D = ms.dimension
    dens = ms.mixture_densities[ms.mixture_offsets[pm].astype(np.int64) + pd]
    xi = np.concatenate([np.ones((len(pf), 1)), frames[pf].astype(np.float64)], axis=1)
    mu = ms.means[ms.density_mean[dens]].astype(np.float64)
    v = ms.variances[ms.density_covariance[dens]].astype(np.float64)
    w = np.ones(len(pf)) if pw is None else pw
    for key in range(2):
        s = pk == key
        got = ar.finalize(tables[key], ms)
        assert got["beta"] == w[s].sum()
        assert np.array_equal(got["mean"], (xi[s] * w[s, None]).sum(axis=0))
        cov = np.einsum("n,nj,nk->jk", w[s], xi[s], xi[s])
        assert np.array_equal(got["cov"], cov)
        assert np.array_equal(got["k"], np.einsum("n,ni,nj->ij", w[s], mu[s] / v[s], xi[s]))
        if n_cov == 1:  # finalize: G[i] = cov / v[i]
            assert tables[key]["G"] is None
            assert np.array_equal(got["G"], cov[None] / ms.variances[0].astype(np.float64)[:, None, None])
        else:
            assert np.array_equal(got["G"], np.einsum("n,ni,nj,nk->ijk", w[s], 1.0 / v[s], xi[s], xi[s]))
        assert np.array_equal(got["G"], got["G"].transpose(0, 2, 1)) and np.array_equal(got["cov"], got["cov"].T)


def _random_case(D, n_cov, n=400, seed=0):
    ms = ra.synthetic_mixture_set(6, 3, D, seed=50 + seed + D, n_covariances=n_cov)
    frames = ra.synthetic_frames(n, D, seed=60 + seed + D)
    rng = np.random.default_rng(70 + seed + D)
    pf = np.arange(n, dtype=np.uint32)
    pm = rng.integers(0, 6, size=n).astype(np.uint32)
    pd = rng.integers(0, 3, size=n).astype(np.uint32)
    return ms, frames, pf, pm, pd


def test_piece_rule_against_sequential_order():
    ms, frames, pf, pm, pd = _random_case(5, 3, n=1300)
    pw = np.random.default_rng(5).uniform(0.0, 2.0, size=1300)
    (pieces,), _ = ar.accumulate(ms, frames, pf, pm, pd, pw)
    (seq,), _ = ar.accumulate(ms, frames, pf, pm, pd, pw, chunk=None)
    # two different sums: a kernel that summed sequentially would not be bit-equal to the contract
    for name in ("k", "G", "mean", "cov"):
        assert (pieces[name] != seq[name]).any(), name
    # ... within the standard bound between two summation orders of n terms, 2 n 2^-53 sum |term|
    J, K = ar.triangle(5)
    xi = np.concatenate([np.ones((1300, 1)), frames[pf].astype(np.float64)], axis=1)
    dens = ms.mixture_densities[ms.mixture_offsets[pm].astype(np.int64) + pd]
    v = ms.variances[ms.density_covariance[dens]].astype(np.float64)
    mu = ms.means[ms.density_mean[dens]].astype(np.float64)
    c = 2 * 1300 * 2.0 ** -53
    assert (np.abs(pieces["cov"] - seq["cov"]) <= c * (np.abs(xi[:, J] * xi[:, K]) * pw[:, None]).sum(axis=0)).all()
    assert (np.abs(pieces["mean"] - seq["mean"]) <= c * (np.abs(xi) * pw[:, None]).sum(axis=0)).all()
    g_terms = np.abs(xi[:, J] * xi[:, K])[:, None, :] / v[:, :, None] * pw[:, None, None]
    assert (np.abs(pieces["G"] - seq["G"]) <= c * g_terms.sum(axis=0)).all()
    k_terms = np.abs((mu / v)[:, :, None] * xi[:, None, :]) * pw[:, None, None]
    assert (np.abs(pieces["k"] - seq["k"]) <= c * k_terms.sum(axis=0)).all()
    assert abs(pieces["beta"] - seq["beta"]) <= c * pw.sum()


@pytest.fixture(scope="module")
def estimate_tables():
    """Finalized tables of 400 random pairs per (D, covariance count), shared by the estimate tests."""
    out = {}
    for D in (3, 16, 39):
        for n_cov in (1, 3):
            ms, frames, pf, pm, pd = _random_case(D, n_cov)
            (t,), skipped = ar.accumulate(ms, frames, pf, pm, pd)
            assert skipped == 0
            out[D, n_cov] = ar.finalize(t, ms)
    return out


@pytest.mark.parametrize("criterion,iterations", [("naive", 1), ("mmiPrime", 1), ("mmiPrime", 5)])
@pytest.mark.parametrize("n_cov", [1, 3])
@pytest.mark.parametrize("D", [3, 16, 39])
def test_estimate_against_restatement(built, estimate_tables, D, n_cov, criterion, iterations):
    t = estimate_tables[D, n_cov]
    conds = [np.linalg.cond(t["G"][i]) for i in range(D)]
    assert max(conds) <= 1e4, max(conds)  # a condition on the inputs (module docstring)
    ref = ar.estimate(t, criterion, iterations)
    got = ra.estimate_affine_transform(t, criterion, iterations)
    assert got.dtype == np.float32 and got.shape == (D, D + 1)
    bound = ar.ulp32(np.abs(ref).max(axis=1))[:, None]
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), float((err / bound).max())
    if criterion == "mmiPrime" and iterations == 5:  # the sweeps do something
        assert not np.array_equal(got, ra.estimate_affine_transform(t, criterion, 1))


def test_min_observation_weight_returns_initial(built, estimate_tables):
    t = estimate_tables[3, 3]
    init = np.arange(12, dtype=np.float64).reshape(3, 4) / 8
    init[:, 1:] += np.eye(3)  # a regular linear part
    assert t["beta"] == 400
    got = ra.estimate_affine_transform(t, "mmiPrime", 3, min_observation_weight=400.5, initial_transform=init)
    assert np.array_equal(got, init.astype(np.float32))
    ident = ra.estimate_affine_transform(t, "mmiPrime", 3, min_observation_weight=1e9)
    assert np.array_equal(ident, np.concatenate([np.zeros((3, 1)), np.eye(3)], axis=1).astype(np.float32))
    # beta == the threshold is not below it; naive never returns early (cc:204)
    assert not np.array_equal(ra.estimate_affine_transform(t, "mmiPrime", 3, min_observation_weight=400.0,
                                                           initial_transform=init), init.astype(np.float32))
    naive = ra.estimate_affine_transform(t, "naive", 1, min_observation_weight=1e9)
    assert np.array_equal(naive, ra.estimate_affine_transform(t, "naive", 1))


def test_square_initial_transform_gains_offset_column(built, estimate_tables):
    t = estimate_tables[16, 1]
    rng = np.random.default_rng(9)
    square = np.eye(16) + 0.05 * rng.standard_normal((16, 16))
    wide = np.concatenate([np.zeros((16, 1)), square], axis=1)
    a = ra.estimate_affine_transform(t, "mmiPrime", 2, initial_transform=square)
    b = ra.estimate_affine_transform(t, "mmiPrime", 2, initial_transform=wide)
    assert np.array_equal(a, b)
    ref = ar.estimate(t, "mmiPrime", 2, initial=square)
    assert (np.abs(a - ref) <= ar.ulp32(np.abs(ref).max(axis=1))[:, None]).all()
    early = ra.estimate_affine_transform(t, "mmiPrime", 2, min_observation_weight=1e9, initial_transform=square)
    assert np.array_equal(early, wide.astype(np.float32))
    with pytest.raises(ra.GmmError) as e:
        ra.estimate_affine_transform(t, "mmiPrime", 2, initial_transform=np.zeros((16, 15)))
    assert e.value.code == _capi.GMM_ERR_INVALID_ARGUMENT


def test_integer_half_root_choice(built):
    """`1 / 2` in l1 and l2 is an integer division (cc:283-284): the root is chosen by beta * log|.| alone.  Tables with
    a negative definite G (eps1 < 0) and a small beta, where the quadratic term as it seems meant would flip the
    choice: the library follows the reference's text."""
    # D = 1, identity start: cofactors = (0, 1), eps1 = -1, eps2 = 10, roots 0.101 and 9.899; |alpha eps1 + eps2| is
    # larger at the first, 0.5 alpha^2 |eps1| far larger at the second
    D = 1
    t = {"beta": 1.0, "k": np.array([[0.5, -10.0]]), "G": -np.eye(2)[None], "mean": None, "cov": None}
    as_written = ar.estimate(t, "mmiPrime", 1, half=0)
    as_meant = ar.estimate(t, "mmiPrime", 1, half=0.5)
    assert np.isfinite(as_written).all() and np.isfinite(as_meant).all()
    # the precondition: the two readings choose different roots, and not by a rounding
    assert np.abs(as_written - as_meant).max() > 1.0
    got = ra.estimate_affine_transform(t, "mmiPrime", 1)
    assert (np.abs(got - as_written) <= ar.ulp32(np.abs(as_written).max(axis=1))[:, None]).all()
    assert np.abs(got - as_meant).max() > 1.0
    assert D == got.shape[0]


def test_singular_g_and_hlda_are_refused(built, estimate_tables):
    t = dict(estimate_tables[3, 3])
    with pytest.raises(ra.GmmError) as e:
        ra.estimate_affine_transform(t, "hlda", 1)
    assert e.value.code == _capi.GMM_ERR_UNSUPPORTED and "hlda" in str(e.value)
    G = t["G"].copy()
    G[1, 2, :] = G[1, 0, :]  # row 2 = row 0, and symmetric
    G[1, :, 2] = G[1, :, 0]
    G[1, 2, 2] = G[1, 0, 0]
    t["G"] = G
    assert np.linalg.matrix_rank(G[1]) == 3
    for criterion in ("naive", "mmiPrime"):
        with pytest.raises(ra.GmmError) as e:
            ra.estimate_affine_transform(t, criterion, 1)
        assert e.value.code == _capi.GMM_ERR_INVALID_ARGUMENT and "row 1" in str(e.value) and "singular" in str(e.value)
    t["G"] = np.zeros_like(G)
    with pytest.raises(ra.GmmError) as e:
        ra.estimate_affine_transform(t, "naive", 1)
    assert e.value.code == _capi.GMM_ERR_INVALID_ARGUMENT and "row 0" in str(e.value)


def test_affine_symbols_are_bound(built):
    lib = ra.load_library()
    names = {p[0] for p in _capi.PROTOTYPES}
    for n in ["gmm_affine_create", "gmm_affine_destroy", "gmm_affine_reset", "gmm_affine_accumulate_device",
              "gmm_affine_accumulate_host", "gmm_affine_skipped", "gmm_affine_info", "gmm_affine_get", "gmm_affine_add",
              "gmm_affine_estimate"]:
        assert n in names and hasattr(lib, n), n
    header = open(os.path.join(ROOT, "include", "rasr_gmm_adaptation.h")).read()
    assert "#define GMM_AFFINE_CHUNK 512" in header and _capi.GMM_AFFINE_CHUNK == ar.CHUNK == 512
    assert ra.AffineTransformAccumulator is not None and ra.estimate_affine_transform is not None


def test_affine_estimate_cpp_program(built):
    """tests/cpp/affine_estimate_test.cc: the estimate unit alone as a stand-alone program (built by make)."""
    r = subprocess.run([os.path.join(ROOT, "build", "tests", "affine_estimate_test")], capture_output=True, text=True)
    assert r.returncode == 0 and "affine_estimate_test: ok" in r.stdout, r.stdout + r.stderr
