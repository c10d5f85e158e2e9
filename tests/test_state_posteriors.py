"""State posteriors on the device: gmm_state_posteriors_* (rasr_amd/csrc/gmm_kernels_state.hip) against the numpy
restatement (tests/state_posteriors_restatement.py), on crafted score tables unless noted.

minimum_score, minimum_index, n_active and the zero pattern of the posteriors involve no transcendental and are
compared bit for bit; the posteriors and log_z are held to posterior_bound(), whose e_exp / e_log
test_device_function_ulps measures through the call itself and keeps asserting.  Measured on an MI355X (the maxima each
case prints):
    device exp 1.00 ulp from numpy's at most, log1p 0 ulp at integer sums and 1.00 ulp at log1p(exp(-x)); the f64
    posteriors at most 0.10 of their bound, log_z 0.10, the f32 posteriors equal to the narrowed restatement.
"""
import ctypes
import functools

import numpy as np
import pytest

import rasr_amd as ra
import state_posteriors_restatement as sr
from posteriors_restatement import widen
from rasr_amd import _capi

pytestmark = pytest.mark.gpu

MIXTURES = (1, 255, 256, 257, 700)
FRAMES = (1, 63, 64, 65, 300)
SENTINEL = -7.0
INF_PRIORS = (3, 100, 256, 699)  # mixtures taken out by a +inf prior (those below the mixture count)


@functools.lru_cache(maxsize=None)
def _handle(n_mixtures, max_frames=300):
    """A scorer whose only part in the crafted-table tests is its mixture count (and max_frames)."""
    return ra.Scorer(ra.synthetic_mixture_set(n_mixtures, 1, 39, seed=11), "diagonal-maximum", max_frames=max_frames)


@functools.lru_cache(maxsize=None)
def _table(n_mixtures, n_frames=300, seed=0, spread=200.0):
    t = sr.crafted_table(n_mixtures, n_frames, seed=1000 * n_mixtures + seed, spread=spread)
    t.setflags(write=False)
    return t


def _priors(n_mixtures, with_inf=False):
    pri = np.random.default_rng(n_mixtures).random(n_mixtures) * 8.0
    if with_inf:
        pri[[m for m in INF_PRIORS if m < n_mixtures]] = np.inf
    return pri


def device_call(gpu, sc, table, priors=None, scale=1.0, thr=None, score_stride=None, post_stride=None, want=("f32", "f64"),
                in_place=False):
    """One gmm_state_posteriors_device call on table [M, F]: the tables are allocated with the given strides and
    prefilled with SENTINEL.  Returns a dict of numpy arrays, the tables with their padding."""
    import torch
    M, F = table.shape
    ss, ps = score_stride or F, post_stride or F
    d_scores = torch.full((M, ss), SENTINEL, dtype=torch.float32, device=gpu)
    d_scores[:, :F] = torch.from_numpy(np.array(table)).to(gpu)
    d_pri = None if priors is None else torch.from_numpy(np.ascontiguousarray(priors, dtype=np.float64)).to(gpu)
    o32 = o64 = None
    if in_place:
        o32 = d_scores
    elif "f32" in want:
        o32 = torch.full((M, ps), SENTINEL, dtype=torch.float32, device=gpu)
    if "f64" in want:
        o64 = torch.full((M, ss if in_place else ps), SENTINEL, dtype=torch.float64, device=gpu)
    r = sc.state_posteriors_device(d_scores, d_pri, scale, thr, out_f32=o32, out_f64=o64, n_frames=F)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in r.items()}
    out["minimum_index"] = out["minimum_index"].view(np.uint32)
    out["n_active"] = out["n_active"].view(np.uint32)
    out["f32"] = None if o32 is None else o32.cpu().numpy()
    out["f64"] = None if o64 is None else o64.cpu().numpy()
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check(got, table, priors=None, scale=1.0, thr=None, label=""):
    """The device's outputs of one call against the restatement; returns the restatement."""
    ref = sr.restate(table, priors, scale, thr)
    sr.assert_not_hidden(ref)
    M, F = table.shape
    b64, b32, blog = sr.posterior_bound(ref)
    # no transcendental: bit for bit
    assert np.array_equal(bits(got["minimum_score"]), bits(ref["minimum_score"]))
    assert np.array_equal(got["minimum_index"], ref["minimum_index"])
    assert np.array_equal(got["n_active"], ref["n_active"])
    line = [label or f"{M} x {F}"]
    with np.errstate(invalid="ignore"):
        d_log = np.abs(got["log_z"] - ref["log_z"])
        line.append(f"max |log_z - ref| = {np.nanmax(d_log / blog):.4f} of the bound")
        assert (d_log <= blog).all()
        if got["f64"] is not None:
            p = got["f64"][:, :F]
            assert np.array_equal(p == 0.0, ref["posteriors"] == 0.0)
            assert not p[~ref["active"]].any()
            d = np.abs(p - ref["posteriors"])
            line.append(f"max |p64 - ref| = {np.nanmax(d / b64):.4f} of the bound")
            assert (d <= b64).all()
            assert (got["f64"][:, F:] == SENTINEL).all()
        if got["f32"] is not None:
            p = got["f32"][:, :F]
            # the zero pattern, outside the band where the narrowing gives an f32 subnormal (flushed on the host)
            clear = (ref["posteriors"] == 0.0) | (ref["posteriors"] >= 2.0 ** -125) | (ref["posteriors"] < 2.0 ** -151)
            assert np.array_equal(bits(p)[clear] << 1 == 0, (ref["posteriors_f32"] == 0.0)[clear])
            assert not bits(p)[~ref["active"]].any()
            d = np.abs(widen(p).reshape(p.shape) - widen(ref["posteriors_f32"]).reshape(p.shape))
            line.append(f"max |p32 - ref| = {np.nanmax(d / b32):.4f} of the bound")
            assert (d <= b32).all()
    print(", ".join(line))
    return ref


# ---------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_frames", FRAMES)
@pytest.mark.parametrize("n_mixtures", MIXTURES)
def test_shapes(gpu, n_mixtures, n_frames):
    table = _table(n_mixtures)[:, :n_frames]
    pri = _priors(n_mixtures)
    got = device_call(gpu, _handle(n_mixtures), table, pri, score_stride=n_frames + 5, post_stride=n_frames + 11)
    check(got, table, pri)


@pytest.mark.parametrize("n_mixtures", (257, 700))
def test_no_priors_and_per_frame_outputs_only(gpu, n_mixtures):
    table = _table(n_mixtures)[:, :65]
    got = device_call(gpu, _handle(n_mixtures), table, want=())
    check(got, table)


def test_ties_for_the_minimum_lowest_index_wins(gpu):
    table = np.array(_table(700, spread=50.0)[:, :65])
    low = np.float32(1.0)
    table[[600, 256, 255, 300]] = low  # duplicated rows, in two pieces: 255 wins, the others count exp(0) = 1
    got = device_call(gpu, _handle(700), table)
    ref = check(got, table)
    assert (got["minimum_index"] == 255).all() and (ref["log_z_scaled"] > np.log1p(3.0) - 1e-9).all()


@pytest.mark.parametrize("n_mixtures", (257, 700))
def test_infinite_priors(gpu, n_mixtures):
    table = _table(n_mixtures)[:, :65]
    pri = _priors(n_mixtures, with_inf=True)
    got = device_call(gpu, _handle(n_mixtures), table, pri)
    check(got, table, pri)
    out = [m for m in INF_PRIORS if m < n_mixtures]
    assert not got["f64"][out].any() and not got["f32"][out].any()
    assert not np.isin(got["minimum_index"], out).any()


@pytest.mark.parametrize("scale", (0.5, 3.0))
def test_scale(gpu, scale):
    table = _table(257, spread=90.0)[:, :65]
    pri = _priors(257)
    check(device_call(gpu, _handle(257), table, pri, scale=scale), table, pri, scale=scale)


def test_pruning_threshold_at_an_occurring_cell_excludes_it(gpu):
    table = _table(700)[:, :65]
    pri = _priors(700)
    free = sr.restate(table, pri)
    t = 7
    gap = free["s"][:, t] - free["minimum_score"][t]
    m = int(np.nonzero((gap > 0) & (gap + free["minimum_score"][t] == free["s"][:, t]))[0][5])  # an exact cell
    thr = gap[m]
    got = device_call(gpu, _handle(700), table, pri, thr=thr)
    ref = check(got, table, pri, thr=thr)
    assert got["f64"][m, t] == 0.0 and got["f32"][m, t] == 0.0 and not ref["active"][m, t]
    assert 1 <= got["n_active"].min() and got["n_active"][t] < 700


def test_geometry_independence(gpu):
    table = _table(700)
    pri = _priors(700)
    sc = _handle(700)
    whole = device_call(gpu, sc, table, pri, score_stride=300, post_stride=300)
    keys = ("log_z", "minimum_score", "minimum_index", "n_active")
    for t in (0, 63, 64, 299):  # the same frames as 1-frame calls
        one = device_call(gpu, sc, table[:, t:t + 1], pri, score_stride=3, post_stride=2)
        for k in keys:
            assert bits(one[k])[0] == bits(whole[k])[t], (k, t)
        for k in ("f32", "f64"):
            assert np.array_equal(bits(one[k][:, 0]), bits(whole[k][:, t])), (k, t)
    part = device_call(gpu, sc, table[:, 100:165], pri, score_stride=71, post_stride=97)  # a 65-frame call
    for k in keys:
        assert np.array_equal(bits(part[k]), bits(whole[k][100:165])), k
    for k in ("f32", "f64"):
        assert np.array_equal(bits(part[k][:, :65]), bits(whole[k][:, 100:165])), k


def test_in_place(gpu):
    import torch
    table = _table(700)[:, :65]
    pri = _priors(700)
    sc = _handle(700)
    fresh = device_call(gpu, sc, table, pri, score_stride=70, post_stride=70)
    placed = device_call(gpu, sc, table, pri, score_stride=70, in_place=True)
    assert np.array_equal(bits(placed["f32"]), bits(fresh["f32"]))  # the padding too: SENTINEL in both
    assert np.array_equal(bits(placed["f64"]), bits(fresh["f64"]))
    assert np.array_equal(bits(placed["log_z"]), bits(fresh["log_z"]))
    check(placed, table, pri)
    # the alias with another stride is refused, and nothing is written
    d = torch.full((700, 70), SENTINEL, dtype=torch.float32, device=gpu)
    lz = torch.full((65,), SENTINEL, dtype=torch.float64, device=gpu)
    rc = sc._lib.gmm_state_posteriors_device(sc.handle, ctypes.c_void_p(d.data_ptr()), 65, 70, None, 1.0, sr.DBL_MAX,
                                             ctypes.c_void_p(d.data_ptr()), None, 69, ctypes.c_void_p(lz.data_ptr()),
                                             None, None, None, None)
    torch.cuda.synchronize()
    assert rc == _capi.GMM_ERR_INVALID_ARGUMENT
    assert (d == SENTINEL).all().item() and (lz == SENTINEL).all().item()


def test_frame_without_a_finite_score(gpu):
    table = np.array(_table(257)[:, :65])
    table[:, 9] = np.inf
    got = device_call(gpu, _handle(257), table)
    assert got["minimum_index"][9] == sr.NO_INDEX and got["minimum_score"][9] == sr.DBL_MAX
    assert not got["f64"][:, 9].any() and not got["f32"][:, 9].any()
    assert got["log_z"][9] == -sr.DBL_MAX and got["n_active"][9] == 257
    keep = np.arange(65) != 9
    clean = device_call(gpu, _handle(257), np.ascontiguousarray(table[:, keep]))
    for k in ("log_z", "minimum_score", "minimum_index", "n_active"):
        assert np.array_equal(bits(got[k][keep]), bits(clean[k])), k
    for k in ("f32", "f64"):
        assert np.array_equal(bits(got[k][:, keep]), bits(clean[k])), k
    check(clean, np.ascontiguousarray(table[:, keep]))


# ---------------------------------------------------------------------------------------------------------------
# the device library's exp / log1p, measured through the call
# ---------------------------------------------------------------------------------------------------------------

def test_device_function_ulps(gpu):
    """Two mixtures with scores (0, x), no priors, scale 1: s = (0, x), the minimum is 0 at index 0, so
        log_z = log1p(exp(-x))  and  p_1 = exp(a),  a = (-x) - log_z  (one f64 subtraction of values the host has),
    which gives the device's exp at the arguments a directly.  K + 1 mixtures of score 0 give log_z = log1p(K) with
    the sum exact.  For the sums below 1 the argument of log1p is the device's own exp(-x), which the host does not
    see: the distance of log_z to numpy's log1p(exp(-x)) is then at most e_log + e_exp ulps (log1p moves by less than
    an ulp per ulp of its argument), so it is held to that.  sr.E_EXP / sr.E_LOG1P are these maxima plus one ulp for
    numpy's own error."""
    x = np.concatenate([np.linspace(0.0, 320.0, 297), [1e-3, 0.5, 1.0]]).astype(np.float32)
    table = np.stack([np.zeros_like(x), x])
    got = device_call(gpu, _handle(2), table, want=("f64",))
    assert (got["minimum_index"] == 0).all()
    a = (-x.astype(np.float64)) - got["log_z"]
    want = np.exp(a)
    e_exp = np.abs(got["f64"][1] - want) / np.spacing(want)
    want = np.log1p(np.exp(-x.astype(np.float64)))
    e_mix = np.abs(got["log_z"] - want) / np.spacing(want)
    K = 256
    ties = np.zeros((K + 1, K), np.float32)
    for k in range(K):
        ties[k + 1:, k] = 800.0  # frame k: k + 1 cells of score 0, the others far away (exp(-800) = 0)
    got = device_call(gpu, _handle(K + 1), ties, want=())
    want = np.log1p(np.arange(K, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        e_log = np.where(want > 0, np.abs(got["log_z"] - want) / np.spacing(want), got["log_z"] != 0.0)
    print(f"device exp: {e_exp.max():.2f} ulp from numpy's; log1p at 0..{K - 1}: {e_log.max():.2f} ulp; "
          f"log1p(exp(-x)): {e_mix.max():.2f} ulp")
    assert e_exp.max() <= sr.E_EXP - 1
    assert e_log.max() <= sr.E_LOG1P - 1
    assert e_mix.max() <= (sr.E_LOG1P - 1) + (sr.E_EXP - 1)


# ---------------------------------------------------------------------------------------------------------------
# end to end, refusals
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("SIMD-diagonal-maximum", "diagonal-maximum"))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_end_to_end_host_call(gpu, kind, dtype):
    ms = ra.synthetic_mixture_set(20, 6, 39, seed=5)
    frames = ra.synthetic_frames(70, 39, seed=6)
    sc = ra.Scorer(ms, kind, max_frames=128)
    table, _ = sc.score_host(frames, want_best=False)
    pri = _priors(20)
    r = sc.state_posteriors(frames, pri, scale=0.5, dtype=dtype)
    got = {k: r[k] for k in ("log_z", "minimum_score", "minimum_index", "n_active")}
    got["f32"] = r["posteriors"] if dtype == np.float32 else None
    got["f64"] = r["posteriors"] if dtype == np.float64 else None
    check(got, table, pri, scale=0.5, label=f"{kind} {np.dtype(dtype).name}")
    sc.close()


def test_refusals_leave_the_outputs_untouched(gpu):
    import torch
    ms = ra.synthetic_mixture_set(12, 1, 39, seed=11)
    sc = ra.Scorer(ms, "diagonal-maximum", max_frames=64)
    shard = ra.Scorer(ms, "diagonal-maximum", max_frames=64, mixture_range=(0, 6))
    scores = torch.zeros((12, 80), dtype=torch.float32, device=gpu)
    outs = {"f32": torch.full((12, 80), SENTINEL, dtype=torch.float32, device=gpu),
            "f64": torch.full((12, 80), SENTINEL, dtype=torch.float64, device=gpu),
            "lz": torch.full((80,), SENTINEL, dtype=torch.float64, device=gpu),
            "mn": torch.full((80,), SENTINEL, dtype=torch.float64, device=gpu),
            "mi": torch.full((80,), 77, dtype=torch.int32, device=gpu),
            "na": torch.full((80,), 77, dtype=torch.int32, device=gpu)}
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(h, n_frames, stride=80, post_stride=80, scale=1.0, with_outputs=True, table=scores):
        o = [p(outs[k]) if with_outputs else None for k in ("f32", "f64")]
        f = [p(outs[k]) if with_outputs else None for k in ("lz", "mn", "mi", "na")]
        rc = sc._lib.gmm_state_posteriors_device(h, p(table) if table is not None else None, n_frames, stride, None,
                                                 scale, sr.DBL_MAX, o[0], o[1], post_stride, *f, None)
        torch.cuda.synchronize()
        return rc

    assert call(sc.handle, 65) == _capi.GMM_ERR_CAPACITY  # n_frames > max_frames
    assert call(shard.handle, 16) == _capi.GMM_ERR_UNSUPPORTED  # a mixture shard cannot normalise
    assert call(sc.handle, 16, stride=15) == _capi.GMM_ERR_INVALID_ARGUMENT
    assert call(sc.handle, 16, post_stride=15) == _capi.GMM_ERR_INVALID_ARGUMENT
    assert call(sc.handle, 16, scale=float("nan")) == _capi.GMM_ERR_INVALID_ARGUMENT
    assert call(sc.handle, 16, with_outputs=False) == _capi.GMM_ERR_INVALID_ARGUMENT
    assert call(sc.handle, 16, table=None) == _capi.GMM_ERR_INVALID_ARGUMENT
    for k in ("f32", "f64", "lz", "mn"):
        assert (outs[k] == SENTINEL).all().item(), k
    assert (outs["mi"] == 77).all().item() and (outs["na"] == 77).all().item()
    assert call(sc.handle, 16) == _capi.GMM_OK  # and the same call, valid, writes
    assert (outs["na"][:16] == 12).all().item() and (outs["na"][16:] == 77).all().item()
    sc.close()
    shard.close()
