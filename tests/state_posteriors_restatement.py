"""numpy restatement of the state posteriors (include/rasr_gmm.h gmm_state_posteriors_*), shared by
tests/test_state_posteriors_cpu.py (its self-consistency, no GPU) and tests/test_state_posteriors.py (the device
against it).

Per frame over the mixtures m, every step one f64 operation (Mm::StatePosteriorFeatureScorer, Viterbi / mixture mode,
StatePosteriorFeatureScorer.cc:81-160, 258-284):
    s_m = prior_m + scale * (f64) score(m);  min: the strict-compare scan from DBL_MAX in ascending m (lowest index on
    ties);  active: all m without pruning, else s_m < (pruning_threshold + min);  d_m = min - s_m;
    sum of exp(d_m) over the active m != minimum_index;  logZ' = log1p(sum);  p_m = exp(d_m - logZ') (0 when pruned);
    log_z = logZ' - min.
The sum's order is the contract's: pieces of CHUNK consecutive mixtures, each added sequentially from 0 in ascending m,
the pieces' sums added sequentially from 0 in piece order.

The tolerance (posterior_bound), with u = 2^-53, e_exp / e_log the ulp bounds of the device's f64 exp / log1p:
    relative error of p_m  <= 2 u [2 e_exp + CHUNK + n_pieces + 2 e_log logZ' + 2 |d_m - logZ'| + 2 e_exp + 2]
    absolute error of log_z <= 2 u [2 e_exp + CHUNK + n_pieces + 2 e_log logZ' + 2 + |log_z|]
(a term of the sum carries e_exp ulps from each side, the device's and numpy's; a piece adds at most CHUNK roundings
and the pieces n_pieces; log1p's e_log ulps of logZ' move the exponent's argument absolutely, as does the rounding
of d_m - logZ' itself; the final exp has e_exp ulps on each side; the rest are the single roundings of d_m and log_z).
The ROCm installation carries no accuracy table of its device library, so E_EXP and E_LOG1P are the largest ulp
distances to numpy measured on an MI355X over arguments of the tests' range (tests/test_state_posteriors.py
test_device_function_ulps, which keeps asserting them) plus one ulp for numpy's own error.  Below 2^-1022 (f64) /
2^-126 (f32) the bound has an absolute floor: the oracle libraries switch the whole test process to flush-to-zero
(tests/conftest.py), so subnormal expectations cannot be trusted; assert_not_hidden() shows the floor hides nothing.
"""
import math

import numpy as np

CHUNK = 256
U = 2.0 ** -53
DBL_MAX = np.finfo(np.float64).max
NO_INDEX = 0xFFFFFFFF
# measured on an MI355X: exp at most 1.00 ulp from numpy's; log1p 0 ulp at the integer sums
# 0..255 and 1.00 ulp at the sums exp(-x) below 1, where the device's own exp may account for one: at most 2; plus 1 for
# numpy's own error each
E_EXP = 2
E_LOG1P = 3
FLOOR64 = 2.0 ** -1022
FLOOR32 = 2.0 ** -126


def scaled_scores(scores, priors, scale):
    """s [M, F] f64: one multiply and one add per cell."""
    scores = np.asarray(scores, dtype=np.float32)
    pri = np.zeros(scores.shape[0]) if priors is None else np.asarray(priors, dtype=np.float64)
    return pri[:, None] + np.float64(scale) * scores.astype(np.float64)


def restate(scores, priors=None, scale=1.0, pruning_threshold=None, chunk=CHUNK):
    """The call's outputs for a [M, F] f32 table, as a dict: s, posteriors (f64 [M, F]), posteriors_f32, log_z,
    log_z_scaled (logZ'), minimum_score, minimum_index (uint32), n_active (uint32), active (bool [M, F]), d.
    chunk=None: the purely sequential sum."""
    s = scaled_scores(scores, priors, scale)
    M, F = s.shape
    thr = DBL_MAX if pruning_threshold is None else np.float64(pruning_threshold)
    mn = np.full(F, DBL_MAX)
    mi = np.full(F, NO_INDEX, np.uint32)
    for m in range(M):
        take = s[m] < mn
        mn = np.where(take, s[m], mn)
        mi = np.where(take, np.uint32(m), mi)
    with np.errstate(over="ignore", invalid="ignore"):
        active = np.ones((M, F), bool) if thr >= DBL_MAX else s < (thr + mn)[None, :]
        d = mn[None, :] - s
        total = np.zeros(F)
        step = chunk or max(M, 1)
        for m0 in range(0, M, step):
            piece = np.zeros(F)
            for m in range(m0, min(m0 + step, M)):
                piece = np.where(active[m] & (mi != m), piece + np.exp(d[m]), piece)
            total = total + piece
        lz = np.log1p(total)
        p = np.where(active, np.exp(d - lz[None, :]), 0.0)
        log_z = lz - mn
    return {"s": s, "posteriors": p, "posteriors_f32": p.astype(np.float32), "log_z": log_z, "log_z_scaled": lz,
            "minimum_score": mn, "minimum_index": mi, "n_active": active.sum(axis=0).astype(np.uint32),
            "active": active, "d": d}


def reference_walk(column, priors=None, scale=1.0, pruning_threshold=None):
    """One frame as the reference's own loops do it, scalar by scalar in list order with math.exp / math.log1p:
    posteriorsAndMixtures(IndicesAndWeights&) (cc:258-284), with pruneScores (cc:104-116) in between when a
    threshold is given.  Returns (p list, None where pruned; logZ; minimum score; minimum index)."""
    n = len(column)
    pri = [0.0] * n if priors is None else [float(w) for w in priors]
    scores = [pri[i] + float(scale) * float(np.float32(column[i])) for i in range(n)]
    min_index, min_score = NO_INDEX, DBL_MAX
    for i in range(n):
        if scores[i] < min_score:
            min_score, min_index = scores[i], i
    kept = list(range(n))
    if pruning_threshold is not None and pruning_threshold < DBL_MAX:
        threshold = pruning_threshold + min_score
        kept = [i for i in range(n) if scores[i] < threshold]
    total = 0.0
    d = {}
    for i in kept:
        d[i] = min_score - scores[i]
        if i != min_index:
            total += math.exp(d[i])
    log_z = math.log1p(total)
    p = [None] * n
    for i in kept:
        p[i] = math.exp(d[i] - log_z)
    return p, log_z - min_score, min_score, min_index


def posterior_bound(ref, e_exp=E_EXP, e_log=E_LOG1P, chunk=CHUNK):
    """(bound on |p - ref| [M, F] for the f64 posteriors, for the f32 posteriors, bound on |log_z - ref| [F]) of a
    restate() result.  The f32 bound adds one f32 ulp of the expectation: the two f64 values, a few f64 ulps apart,
    may narrow to neighbouring f32 values."""
    M = ref["s"].shape[0]
    n_pieces = (M + chunk - 1) // chunk
    lz = ref["log_z_scaled"]
    with np.errstate(invalid="ignore", over="ignore"):
        common = 2 * e_exp + chunk + n_pieces + 2 * e_log * lz
        arg = np.abs(ref["d"] - lz[None, :])
        rel = 2 * U * (common[None, :] + 2 * np.where(np.isfinite(arg), arg, 0.0) + 2 * e_exp + 2)
        b64 = rel * ref["posteriors"] + FLOOR64
        p32 = ref["posteriors_f32"]
        b32 = rel * ref["posteriors"] + np.spacing(np.abs(p32)).astype(np.float64) + FLOOR32
        blog = 2 * U * (common + 2 + np.abs(ref["log_z"]))
    return b64, b32, blog


def assert_not_hidden(ref):
    """The absolute floor hides nothing: at least half of the active cells have a restated posterior above 2^-970."""
    act = ref["active"]
    assert act.any()
    assert (ref["posteriors"][act] > 2.0 ** -970).sum() * 2 >= act.sum()


def crafted_table(n_mixtures, n_frames, seed, spread=200.0, base=40.0):
    """A [M, F] f32 score table: uniform in [base, base + spread), spread a few hundred at most."""
    rng = np.random.default_rng(seed)
    return (base + spread * rng.random((n_mixtures, n_frames))).astype(np.float32)
