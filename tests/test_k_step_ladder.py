"""Parity at every compiled K-step count of the scoring kernels.

Every scoring kernel is a template over its K-step count; the host picks the instantiation from the dimension D
(gmm_kernels.hh splitKSteps / splitKSteps32 / splitCovKSteps, gmm_prepare.hh f32KStepsInstantiated,
gmm_kernels_direct.hip directBlocks, ceil(D / 64) for the quantized kernels).  Each instantiation is compiled on its
own, with its own software pipeline, so a dimension list such as {16, 39, 45, 80} leaves most of them unrun.  LADDER
names one D for every value of every dispatch list, per kernel family; where the seven limb positions 3D .. 3D+6 of the
split layout (6D .. 6D+3 on the covariance-free layout) cross a K-step boundary at some D of that K-step count, the
rung takes that D.  Where none does the nearest crossing D is another family rung already (16-row pooled: KS 1 has
D <= 8, the crossing D = 9 is the KS 2 rung; 32-row: KS 1 has D <= 3, D = 4 is the KS 2 rung; covariance-free: the only
crossings are D = 5, 21, 37 = the KS 2, 5, 8 rungs).

CPU (no GPU): test_ladder_covers_every_dispatch_list reads the integer_sequence lists from the kernel sources and fails
when a list holds a value without a rung, or a rung's D does not give its K-step count under the restated host
formulas; test_reference_near_ties_below_cap counts, in float64 alone, the (mixture, frame) cells whose two best
densities are within 1e-4 relative -- the only cells where the float contract lets a kernel name another density.

GPU: every rung asserts Scorer.main_kernel() and Scorer.k_steps() (gmm_scorer_k_steps) first, then parity against the
oracle on a 9-mixture model with empty mixtures at both ends (COUNTS["A"]: in the middle too), one-, two- and
three-tile mixtures and a tile with 15 padding rows, at 257 frames (a full 256-frame workgroup and one frame of the next), for two count vectors:

    counts      16-row tiles, padded even (split16, cov16)   32-row tiles (split32)   16-row tiles (f32, i8)
    COUNTS["A"] 14 = 0 2 2 2 0 4 2 2 0  (chunks 2 2 2 4 2 2 0)  7 (chunks of 1, one of 2)   9
    COUNTS["B"] 20 = 0 4 2 4 2 4 2 2 0  (chunks 4 6 6 4 0)      10 (chunks 2 3 3 2 0)       14

(chunks: the tile totals of the mixture chunks gmm_score.cc chunkTableFor cuts at 2 frame tiles; _chunk_tile_totals
restates it and test_count_vectors_differ_mod_4 pins the figures.)  The totals differ mod 4 (14 / 20, 7 / 10, 9 / 14),
and the sum kernels' walk -- first tile, whole groups of four steps, a tail of one or three -- sees a tail of one
(chunks of 2), a tail of three (4) and a group of four with a tail of one (6).  A chunk of 8 tiles needs more than 4
tiles per mixture on average, which mixtures of at most 33 densities cannot give; the larger models of
tests/test_diagonal_sum.py walk those.

Contracts, as everywhere in the suite: float kernels |gpu - ref| <= 1e-4 max(1, |ref|) and a different best density
only under the float64 near-tie rule (test_gpu_parity._check_float), for at most 1 % of a case's cells; scoreDirect,
the pair kernel and the quantized kernels bit for bit; density posteriors as tests/test_estimator_posteriors.py;
empty mixtures 0.5 FLT_MAX (diagonal-maximum), FLT_MAX (batch-float: the reference's untouched minimum) or +inf
(diagonal-sum) and best density 0xFFFFFFFF, bit for bit.

Instantiations no public option reaches (they are compiled, nothing dispatches them):
  * scoreSplit<KS, BEST, PRESEL = false> (the pair kernel) at KS 1..4: gmm_score.cc kernelPlanOf takes scoreSplitWide
    whenever splitWideFrames(KS) != 0, i.e. KS <= 4 (GMM_SPLIT_WIDE is a build-time switch); only preselection-batch-float
    (PRESEL = true) runs scoreSplit at KS 1..4, and it has its own rungs.  scoreSplitWide has no instantiation above 4.
  * the 32-row kernels on the covariance-free layout: gmm_prepare.cc lays several covariances out on 16-row tiles only.
  * scoreI8 with the one-wave workgroup (smallTile 2) and several covariances: gmm_score.cc planFor gives such calls
    smallTile 1; the score-only class layout (scoreI8Cls) exists at one K step only.
"""
import functools
import os
import re

import numpy as np
import pytest

import oracle
import rasr_amd as ra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rasr_amd", "csrc")
REL_TOL = 1e-4
N_FRAMES = 257
NEAR_TIE_CAP = 0.01  # of a case's (mixture, frame) cells
HALF_FLT_MAX = np.float32(0.5) * np.finfo(np.float32).max
NO_DENSITY = 0xFFFFFFFF

COUNTS = {"A": (0, 1, 16, 17, 0, 33, 5, 9, 0), "B": (0, 33, 1, 33, 16, 33, 5, 17, 0)}

DM, BATCH, SUM, PRESEL = "diagonal-maximum", "batch-diagonal-maximum-float", "diagonal-sum", "preselection-batch-float"


# ---- the host's formulas, restated ----

def split_k_steps(d):  # gmm_kernels.hh splitKSteps
    return (3 * d + 4 + 3 + 31) // 32


def split_k_steps32(d):  # splitKSteps32
    return (3 * d + 4 + 3 + 15) // 16


def split_cov_k_steps(d):  # splitCovKSteps
    return (6 * d + 4 + 31) // 32


def _first_at_least(need, steps):
    return next((k for k in sorted(steps) if need <= k), 0)


def f32_k_steps(d, fold, steps):  # gmm_prepare.cc prepareFloat: f32KStepsInstantiated((kUsed + 3) / 4)
    return _first_at_least((d + 1 + (1 if fold else 0) + 3) // 4, steps)


def direct_blocks(d, batch, steps):  # gmm_kernels_direct.hip directBlocks
    return _first_at_least((d + 7) // 8 * 2 if batch else d // 4, steps)


def i8_k_steps(d):
    return (d + 63) // 64


def i8_small_tile(n_frames, multi_cov):  # gmm_score.cc planFor
    if n_frames > 256:
        return 0
    return 2 if n_frames <= 64 and not multi_cov else 1


def _limbs_cross(first, n, width):
    """The n K positions from `first` on lie in two K steps of `width`."""
    return first // width != (first + n - 1) // width


# family: (dispatch list, scorer types of a rung, K steps of D, limb crossing of D or None)
FAMILIES = {
    "split16": ("KSteps16", (DM, BATCH), lambda d, ls: split_k_steps(d), lambda d: _limbs_cross(3 * d, 7, 32)),
    "split16-sum": ("KSteps16", (SUM,), lambda d, ls: split_k_steps(d), lambda d: _limbs_cross(3 * d, 7, 32)),
    "split16-presel": ("KSteps16", (PRESEL,), lambda d, ls: split_k_steps(d), lambda d: _limbs_cross(3 * d, 7, 32)),
    "split32": ("KSteps32", (DM, BATCH), lambda d, ls: split_k_steps32(d), lambda d: _limbs_cross(3 * d, 7, 16)),
    "split32-sum": ("KSteps32", (SUM,), lambda d, ls: split_k_steps32(d), lambda d: _limbs_cross(3 * d, 7, 16)),
    "cov16": ("KSteps16", (DM,), lambda d, ls: split_cov_k_steps(d), lambda d: _limbs_cross(6 * d, 4, 32)),
    "cov16-sum": ("KSteps16", (SUM,), lambda d, ls: split_cov_k_steps(d), lambda d: _limbs_cross(6 * d, 4, 32)),
    "f32": ("f32", (DM, BATCH), lambda d, ls: f32_k_steps(d, False, ls), None),
    "f32-cov": ("f32", (DM,), lambda d, ls: f32_k_steps(d, True, ls), None),
    "direct": ("direct", (DM,), lambda d, ls: direct_blocks(d, False, ls), None),
    "direct-batch": ("direct", (BATCH,), lambda d, ls: direct_blocks(d, True, ls), None),
    "direct-cov": ("direct", (DM,), lambda d, ls: direct_blocks(d, False, ls), None),
}
# the families that run on COUNTS["A"] only (the same kernels' several-covariance template argument)
ONE_COUNT_VECTOR = ("f32-cov", "direct-cov")

T16, T32, NATIVE, REFORD, COV3 = ({"split_tile16": True}, {"split_tile32": True}, {"native_f32": True},
                                  {"reference_order": True}, {"n_covariances": 3})
# (family, expected kernel name, expected k_steps, D, options: Scorer keywords, n_covariances / tying of the model)
LADDER = (
    [("split16", "scoreSplitWide" if ks <= 4 else "scoreSplit", ks, d, T16)
     for ks, d in ((1, 8), (2, 9), (3, 20), (4, 30), (5, 41), (6, 52), (7, 62), (8, 73))]
    + [("split16-sum", "scoreSplitSum", ks, d, T16)
       for ks, d in ((1, 8), (2, 9), (3, 20), (4, 30), (5, 41), (6, 52), (7, 62), (8, 73))]
    + [("split16-presel", "scoreSplit", ks, d, {})
       for ks, d in ((1, 8), (2, 9), (3, 20), (4, 30), (5, 41), (6, 52), (7, 62), (8, 73))]
    + [("split32", "scoreSplit32", ks, d, T32)
       for ks, d in ((1, 3), (2, 4), (3, 9), (4, 14), (5, 20), (6, 25), (7, 30), (8, 36), (9, 41), (10, 46))]
    + [("split32-sum", "scoreSplit32Sum", ks, d, {})
       for ks, d in ((1, 3), (2, 4), (3, 9), (4, 14), (5, 20), (6, 25), (7, 30), (8, 36), (9, 41), (10, 46))]
    + [("cov16", "scoreSplitWide" if ks <= 4 else "scoreSplit", ks, d, opts)
       for ks, d, opts in ((1, 4, COV3), (2, 5, COV3), (3, 15, {"tying": "mixture-specific"}), (4, 20, COV3),
                           (5, 21, COV3), (6, 31, {"tying": "none"}), (7, 36, COV3), (8, 37, COV3))]
    + [("cov16-sum", "scoreSplitSum", ks, d, COV3)
       for ks, d in ((1, 4), (2, 5), (3, 15), (4, 20), (5, 21), (6, 31), (7, 36), (8, 37))]
    + [("f32", "scoreF32", ks, d, NATIVE)
       for ks, d in ((2, 7), (4, 15), (6, 23), (8, 31), (10, 39), (12, 47), (14, 55), (16, 63), (20, 65), (24, 81),
                     (28, 97), (32, 126))]
    + [("f32-cov", "scoreF32", ks, d, {**NATIVE, **COV3})
       for ks, d in ((2, 6), (4, 14), (6, 22), (8, 30), (10, 38), (12, 46), (14, 54), (16, 62), (20, 64), (24, 80),
                     (28, 96), (32, 126))]
    + [(family, "scoreDirect", nb, d, opts)
       for family, opts in (("direct", REFORD), ("direct-batch", REFORD), ("direct-cov", {**REFORD, **COV3}))
       for nb, d in ((2, 7), (4, 13), (6, 22), (8, 29), (10, 37), (12, 45), (16, 53), (24, 75), (32, 101))]
)
# the reference-order row layout also serves the pair and posterior kernels: a density_posteriors call at these nb
POSTERIOR_NB = (6, 8, 16)

SIMD, BINT = "SIMD-diagonal-maximum", "batch-diagonal-maximum-int"
# (scorer type, expected k_steps, expected smallTile, D, frames, model options): the quantized kernels, kSteps 1, 2
# times smallTile 0, 1, 2 (I8Args::smallTile: 2 = one 64-frame wave per workgroup, 1 = 64-frame waves, 0 = 128-frame)
I8_LADDER = (
    [(kind, 1, st, 39, f, {}) for kind in (SIMD, BINT) for f, st in ((64, 2), (65, 1), (257, 0))]
    + [(kind, 2, st, 80, f, {}) for kind in (SIMD, BINT)
       for f, st in ((1, 2), (64, 2), (65, 1), (256, 1), (257, 0), (600, 0))]
    + [(kind, 2, 0, 100, 600, {}) for kind in (SIMD, BINT)]
    + [(SIMD, 2, st, 80, f, COV3) for f, st in ((64, 1), (257, 0))]
)


# ---- CPU: the ladder against the sources ----

def _dispatch_lists():
    """The literal integer_sequence<int, ...> lists of the three kernel sources, by name."""
    def lists(name, pattern):
        with open(os.path.join(CSRC, name)) as f:
            return re.findall(pattern, f.read())

    seq = r"std::integer_sequence<\s*int\s*,\s*((?:\d+\s*,\s*)*\d+)\s*>"
    out = {}
    for alias, body in lists("gmm_kernels_split.hip", r"using\s+(\w+)\s*=\s*" + seq):
        out[alias] = body
    others = {"f32": lists("gmm_kernels_f32.hip", seq), "direct": lists("gmm_kernels_direct.hip", seq)}
    for name, found in others.items():
        assert len(found) == 1, f"{name}: expected one literal dispatch list, found {found}"
        out[name] = found[0]
    return {k: tuple(int(v) for v in body.split(",")) for k, body in out.items()}


def test_ladder_covers_every_dispatch_list():
    lists = _dispatch_lists()
    assert set(lists) == {"KSteps16", "KSteps32", "f32", "direct"}, f"dispatch lists changed: {sorted(lists)}"
    assert {f[0] for f in FAMILIES.values()} == set(lists)
    for family, (list_name, _, k_of, crossing) in FAMILIES.items():
        rungs = [r for r in LADDER if r[0] == family]
        have = sorted(r[2] for r in rungs)
        # every value of the list has a rung, and no rung names a value that is not compiled
        assert have == sorted(lists[list_name]), f"{family}: rungs {have}, {list_name} = {sorted(lists[list_name])}"
        for _, _, ks, d, _ in rungs:
            assert k_of(d, lists[list_name]) == ks, f"{family}: D = {d} gives {k_of(d, lists[list_name])} K steps, not {ks}"
            if crossing is not None:
                # a rung sits on a D whose limbs cross a K-step boundary wherever its K-step count has one
                could = [x for x in range(1, 128) if k_of(x, lists[list_name]) == ks and crossing(x)]
                assert crossing(d) or not could, f"{family} KS {ks}: D = {d} crosses no boundary, D in {could} would"
    # the crossing dimensions of the 16-row pooled layout are all rungs
    assert all(_limbs_cross(3 * d, 7, 32) for d in (9, 20, 30, 41, 52, 62, 73))
    assert {r[3] for r in LADDER if r[0] == "split16"} >= {9, 20, 30, 41, 52, 62, 73}
    # the quantized kernels: kSteps 1, 2 times smallTile 0, 1, 2 (gmm_kernels_i8.hip launchScoreI8)
    for kind, ks, st, d, f, opts in I8_LADDER:
        assert i8_k_steps(d) == ks and i8_small_tile(f, "n_covariances" in opts) == st, (kind, d, f)
    for kind in (SIMD, BINT):
        assert {(r[1], r[2]) for r in I8_LADDER if r[0] == kind and not r[5]} == {(k, s) for k in (1, 2) for s in (0, 1, 2)}
    assert set(POSTERIOR_NB) <= set(lists["direct"])


def _tiles(counts, rows, pad_even):
    t = [(c + rows - 1) // rows for c in counts]
    return [x + (x & 1) for x in t] if pad_even else t


def _chunk_tile_totals(tiles, n_frame_tiles=2, floor=1024):
    """gmm_score.cc chunkTableFor for a small call: the tile totals of its mixture chunks."""
    target = max(1, (max(n_frame_tiles * 256, floor) + n_frame_tiles - 1) // n_frame_tiles)
    if target > 8:
        target = (target + 7) // 8 * 8
    target = min(target, max(1, len(tiles)))
    per_chunk = max(1, (sum(tiles) + target - 1) // target)
    totals, acc = [], 0
    for m, t in enumerate(tiles):
        acc += t
        if acc >= per_chunk and m + 1 < len(tiles):
            totals.append(acc)
            acc = 0
    return totals + [acc]


def test_count_vectors_differ_mod_4():
    a, b = COUNTS["A"], COUNTS["B"]
    assert max(a + b) <= 33  # the key tag stays at 3 or 4 bits
    for rows, pad_even, want in ((16, True, (14, 20)), (32, False, (7, 10)), (16, False, (9, 14))):
        ta, tb = sum(_tiles(a, rows, pad_even)), sum(_tiles(b, rows, pad_even))
        assert (ta, tb) == want and ta % 4 != tb % 4
    assert _chunk_tile_totals(_tiles(a, 16, True)) == [2, 2, 2, 4, 2, 2, 0]
    assert _chunk_tile_totals(_tiles(b, 16, True)) == [4, 6, 6, 4, 0]  # 6: a whole group of four steps, tail of one
    assert _chunk_tile_totals(_tiles(b, 32, False)) == [2, 3, 3, 2, 0]


# ---- the cases' inputs and references, computed once ----

def _model_opts(opts):
    return tuple(sorted((k, v) for k, v in opts.items() if k in ("n_covariances", "tying")))


def _scorer_opts(opts):
    return {k: v for k, v in opts.items() if k not in ("n_covariances", "tying")}


@functools.lru_cache(maxsize=None)
def _inputs(d, counts_name, model_opts, n_frames=N_FRAMES):
    counts = COUNTS[counts_name]
    ms = ra.synthetic_mixture_set(len(counts), list(counts), d, seed=1000 + d, weights="random", **dict(model_opts))
    return ms, ra.synthetic_frames(n_frames, d, seed=2000 + d)


@functools.lru_cache(maxsize=None)
def _reference(kind, d, counts_name, model_opts, n_frames=N_FRAMES):
    """(scores, best densities or None) of the oracle; shared among the rungs on the same inputs, never written to."""
    ms, frames = _inputs(d, counts_name, model_opts, n_frames)
    if kind == DM:
        ref = oracle.OracleFloat(ms).score(frames, n_threads=4)
    elif kind == SUM:
        ref = oracle.OracleFloatSum(ms).score(frames, n_threads=4)
    elif kind == BATCH:
        ref = (oracle.batch_float_score(ms, frames, n_threads=4), None)
    elif kind == SIMD:
        ref = oracle.OracleSimd(ms).score(frames, n_threads=4)[:2]
    else:
        assert kind == BINT
        ref = (oracle.batch_int_score(ms, frames, n_threads=4), None)
    for a in ref:
        if a is not None:
            a.setflags(write=False)
    return ref


def _f64_scores(ms, e, frames):
    """test_gpu_parity._f64_density_score for every entry of mixture e and every frame at once: [frames, entries]."""
    b, en = int(ms.mixture_offsets[e]), int(ms.mixture_offsets[e + 1])
    dns = ms.mixture_densities[b:en]
    var = ms.variances[ms.density_covariance[dns]].astype(np.float64)
    mean = ms.means[ms.density_mean[dns]].astype(np.float64)
    ln = var.shape[1] * np.log(2 * np.pi) + np.log(var).sum(axis=1)
    chi = (((mean[None] - frames.astype(np.float64)[:, None]) ** 2) / var[None]).sum(axis=2)
    return 0.5 * (-2 * ms.mixture_log_weights[b:en][None] + ln[None] + chi)


def _reference_near_ties(ms, frames):
    """Cells whose runner-up density is within REL_TOL relative of the winner, in float64."""
    n = 0
    for e in range(ms.n_mixtures):
        if ms.mixture_offsets[e + 1] - ms.mixture_offsets[e] < 2:
            continue
        s = np.sort(_f64_scores(ms, e, frames), axis=1)
        n += int((s[:, 1] - s[:, 0] <= REL_TOL * np.maximum(1.0, np.abs(s[:, 0]))).sum())
    return n


FLOAT_FAMILIES = [f for f in FAMILIES if not f.startswith("direct") and f != "split16-presel"]


def test_reference_near_ties_below_cap():
    """The seeds (1000 + D for the model, 2000 + D for the frames) leave the float64 reference alone with fewer than
    1 % of a case's 9 x 257 = 2313 cells (23) in a near tie, so the cap on the kernels' near-tie route is theirs to
    meet.  Counted here for every float rung's inputs: 0 to 5 cells per case, but for D = 63 (8 on count vector A,
    6 on B), D = 65 (7, 7) and D = 46 with three covariances (6)."""
    from test_gpu_parity import _f64_density_score
    seen, worst = set(), (0, None)
    for family, _, _, d, opts in LADDER:
        if family not in FLOAT_FAMILIES:
            continue
        for name in COUNTS:
            key = (d, name, _model_opts(opts))
            if key in seen or (name != "A" and family in ONE_COUNT_VECTOR):
                continue
            seen.add(key)
            ms, frames = _inputs(*key)
            n = _reference_near_ties(ms, frames)
            worst = max(worst, (n, key))
            assert n < NEAR_TIE_CAP * ms.n_mixtures * len(frames), f"{key}: {n} near ties in the reference"
    print(f"most reference near ties: {worst[0]} cells at {worst[1]}")
    # the vectorised scores are test_gpu_parity._f64_density_score's
    ms, frames = _inputs(9, "A", ())
    got = _f64_scores(ms, 5, frames[:3])
    for t in range(3):
        for j in (0, 17, 32):
            want = _f64_density_score(ms, 5, j, frames[t].astype(np.float64))
            assert abs(got[t, j] - want) <= 1e-12 * abs(want)


# ---- GPU ----

def _same(a, b):
    assert a.shape == b.shape
    diff = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    assert diff.size == 0, f"{diff.size} differ; first {diff[:5]}: {a.ravel()[diff[:5]]} vs {b.ravel()[diff[:5]]}"


def _empty(ms):
    return np.diff(ms.mixture_offsets.astype(np.int64)) == 0


def _check_empty(kind, ms, s, b, ref_s):
    """Empty mixtures: the type's "no score" value and no density, bit for bit."""
    e = _empty(ms)
    assert e[0] and e[-1]
    _same(np.ascontiguousarray(s[e]), np.ascontiguousarray(ref_s[e]))
    want = {DM: HALF_FLT_MAX, BATCH: np.finfo(np.float32).max, SUM: np.float32(np.inf)}[kind]
    assert (s[e].view(np.uint32) == want.view(np.uint32)).all(), f"empty mixtures score {s[e][:, 0]}, not {want}"
    if b is not None:
        assert (b[e] == NO_DENSITY).all()


def _check_float_case(kind, ms, frames, s, b, ref_s, ref_b):
    """The float contract on the filled mixtures, the empty ones exactly, and the cap on the near-tie route."""
    from test_gpu_parity import _check_float
    _check_empty(kind, ms, s, b, ref_s)
    e = _empty(ms)
    gs, rs = s.copy(), ref_s.copy()
    gs[e] = rs[e] = 0.0  # compared bit for bit above (+inf - +inf is no error)
    err = np.abs(gs.astype(np.float64) - rs.astype(np.float64)) / np.maximum(1.0, np.abs(rs.astype(np.float64)))
    other = 0 if b is None else int((b != ref_b).sum())
    print(f"max rel err {err.max():.3g}, best density differs in {other} of {s.size} cells")
    if b is not None:
        assert other <= NEAR_TIE_CAP * s.size, f"{other} of {s.size} cells name another density than the reference"
    _check_float(gs, b, rs, ref_b, ms, frames, None)


def _rung_id(r):
    return f"{r[0]}-ks{r[2]}-D{r[3]}"


GPU_CASES = [pytest.param(r, name, id=f"{_rung_id(r)}-{name}") for r in LADDER for name in COUNTS
             if name == "A" or r[0] not in ONE_COUNT_VECTOR]


def _open(ms, kind, kernel, ks, opts, n_frames=N_FRAMES, **kw):
    sc = ra.Scorer(ms, kind, max_frames=n_frames, **_scorer_opts(opts), **kw)
    assert sc.main_kernel() == kernel, f"{kind}: {sc.main_kernel()} runs, the rung names {kernel}"
    assert sc.k_steps() == ks, f"{kind}: dispatched on {sc.k_steps()} K steps, the rung names {ks}"
    return sc


def _preselection_case(ms, frames, kernel, ks, opts):
    ref = oracle.OraclePresel(ms, "float", clusters=256, select=32)
    sc = _open(ms, PRESEL, kernel, ks, opts, clusters=256, select_clusters=32)
    s, _ = sc.score_host(frames)
    ref_sel = ref.select(frames)
    assert np.array_equal(sc.cluster_selection(len(frames)), ref_sel)
    ref_s = ref.score(frames, n_threads=4, selection=ref_sel)
    backoff = ref_s == np.float32(40000.0)
    assert backoff[_empty(ms)].all() and np.array_equal(s == np.float32(40000.0), backoff)
    err = np.abs(s.astype(np.float64) - ref_s) / np.maximum(1.0, np.abs(ref_s.astype(np.float64)))
    print(f"max rel err {err.max():.3g}, {int(backoff.sum())} cells at the backoff score")
    assert err.max() <= REL_TOL, f"max rel err {err.max()}"


def _direct_pairs_and_posteriors(sc, ms, frames, ref_b, nb):
    """The pair kernel on the same row layout (nb blocks), and at POSTERIOR_NB the density posteriors."""
    from test_best_pairs import _all_pairs, _host_pairs
    n = 40
    pf, pm = _all_pairs(n, ms.n_mixtures)
    got, _ = _host_pairs(sc, frames[:n], pf, pm)
    assert np.array_equal(got, ref_b[pm, pf])
    assert (got[_empty(ms)[pm]] == NO_DENSITY).all()
    if nb in POSTERIOR_NB and ms.n_covariances == 1:
        import posteriors_restatement as pr
        from test_estimator_posteriors import check_posteriors
        ds = ra.Scorer(ms, SUM, max_frames=n)
        k = ds.max_entries() + 3
        post, logden = ds.density_posteriors(frames[:n], pf, pm, k)
        check_posteriors(ms, pr.SumModel(ms), frames[:n], pf, pm, post, logden, k, f"nb {nb}")


@pytest.mark.gpu
@pytest.mark.parametrize("rung,counts_name", GPU_CASES)
def test_rung(gpu, rung, counts_name):
    family, kernel, ks, d, opts = rung
    ms, frames = _inputs(d, counts_name, _model_opts(opts))
    if family == "split16-presel":
        return _preselection_case(ms, frames, kernel, ks, opts)
    for kind in FAMILIES[family][1]:
        sc = _open(ms, kind, kernel, ks, opts)
        ref_s, ref_b = _reference(kind, d, counts_name, _model_opts(opts))
        s, b = sc.score_host(frames)
        plain, _ = sc.score_host(frames, want_best=False)  # the path without best densities (tests/test_scores_only.py)
        if family.startswith("direct"):
            _same(s, ref_s)
            _same(plain, ref_s)
            _check_empty(kind, ms, s, b if kind == DM else None, ref_s)
            if kind == DM:
                assert np.array_equal(b, ref_b)
            if family == "direct":
                _direct_pairs_and_posteriors(sc, ms, frames, ref_b, ks)
        else:
            _check_float_case(kind, ms, frames, s, b if ref_b is not None else None, ref_s, ref_b)
            _check_float_case(kind, ms, frames, plain, None, ref_s, None)


I8_CASES = [pytest.param(r, name, id=f"{'simd' if r[0] == SIMD else 'bint'}-ks{r[1]}-st{r[2]}-D{r[3]}-F{r[4]}"
                         f"{'-cov' if r[5] else ''}-{name}") for r in I8_LADDER for name in COUNTS]


@pytest.mark.gpu
@pytest.mark.parametrize("rung,counts_name", I8_CASES)
def test_i8_rung(gpu, rung, counts_name):
    kind, ks, _, d, n_frames, opts = rung
    ms, frames = _inputs(d, counts_name, _model_opts(opts), n_frames)
    sc = _open(ms, kind, "scoreI8", ks, opts, n_frames)
    ref_s, ref_b = _reference(kind, d, counts_name, _model_opts(opts), n_frames)
    s, b = sc.score_host(frames)
    _same(s, ref_s)
    plain, _ = sc.score_host(frames, want_best=False)
    _same(plain, ref_s)
    if kind == SIMD:
        assert np.array_equal(b, ref_b)
        assert (b[_empty(ms)] == NO_DENSITY).all()
