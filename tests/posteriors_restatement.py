"""numpy restatements of the Baum-Welch path (include/rasr_gmm.h gmm_density_posteriors_pairs_*,
include/rasr_gmm_estimator.h gmm_estimator_accumulate_posteriors_*), shared by tests/test_estimator_posteriors_cpu.py
(their self-consistency, no GPU) and tests/test_estimator_posteriors.py (the device against them).

Posteriors (GaussDiagonalSumFeatureScorer, GaussDiagonalMaximumFeatureScorer.cc:238-298), every step one f32 operation:
    s_j = 0.5f * ((w_j + logNorm_cov) + distance_j);  best: strict-compare scan from FLT_MAX in entry order;
    sumExp = 0, sumExp + expf(best - s_j) in entry order;  logDen = best - logf(sumExp);  post_j = expf(logDen - s_j).
expf / logf are taken in f64 and rounded to f32 here: within half an ulp of the true value on every CPU, where numpy's
own float32 exp / log are SIMD routines of a few ulps that differ between CPUs.
Accumulation (AbstractMixtureSetEstimator.cc:127-147): the pairs expanded in (pair, density) order, finalWeight =
weight * (f64) posterior, dropped unless finalWeight > threshold; then the sequential f64 rule of
include/rasr_gmm_estimator.h with pieces of GMM_ESTIMATOR_CHUNK = 512.
"""
import numpy as np

import oracle
from oracle import estimator as est

CHUNK = 512
F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
TABLES = ["mean_sums", "mean_weights", "covariance_sums", "covariance_weights", "entry_weights"]


def ulp32(x):
    """The f32 unit in the last place at |x| (f64 array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def expf(x):
    return F32(np.exp(np.float64(x)))


def logf(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return F32(np.log(np.float64(x)))


def widen(a):
    """(f64) of f32 values from their bits: exact also for subnormals in a process whose SSE state flushes them (the
    oracle libraries' -ffast-math startup code sets it, tests/conftest.py)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    bits = a.view(np.uint32)
    sub = ((bits >> 23) & 0xFF) == 0
    mant = (bits & 0x7FFFFF).astype(np.float64)
    small = np.where((bits >> 31) != 0, -1.0, 1.0) * np.ldexp(mant, -149)
    return np.where(sub, small, np.where(sub, 0, a).astype(np.float64))


class SumModel:
    """The diagonal-sum scorer's tables of a mixture set (oracle.OracleFloatSum's prepared model: scaled inverse
    standard deviations [C][D], log normalization factors [C], -2 log weights [entries]) and the f32 density scores."""

    def __init__(self, ms, mixture_weight_scale=1.0, gaussian_scale=1.0):
        self.ms = ms
        self.oracle = oracle.OracleFloatSum(ms, mixture_weight_scale, gaussian_scale)
        m, C, D, E = self.oracle.m, ms.n_covariances, ms.dimension, ms.n_entries
        self.isv = np.ctypeslib.as_array(m.isv, (C, D)).copy()
        self.log_norm = np.ctypeslib.as_array(m.log_norm, (C,)).copy()
        self.w = np.ctypeslib.as_array(m.minus2_log_weight, (max(E, 1),)).copy()[:E]
        if mixture_weight_scale == 1.0 and gaussian_scale == 1.0:
            for c in range(C):
                assert self.log_norm[c] == F32(oracle.gauss_log_norm(ms.variances[c]))

    def scores(self, x, m):
        """s_j of frame x for the entries of mixture m, f32 [n]."""
        ms = self.ms
        b, e = int(ms.mixture_offsets[m]), int(ms.mixture_offsets[m + 1])
        s = np.empty(e - b, np.float32)
        for j in range(e - b):
            dns = int(ms.mixture_densities[b + j])
            cov = int(ms.density_covariance[dns])
            dist = F32(oracle.float_distance(x, ms.means[int(ms.density_mean[dns])], self.isv[cov]))
            s[j] = F32(0.5) * F32(F32(self.w[b + j] + self.log_norm[cov]) + dist)
        return s


def posterior_row(s):
    """(post [n] f32, logDen f32) of the density scores s, in the reference's order."""
    best = F32(FLT_MAX)
    for v in s:
        if best > v:
            best = v
    sum_exp = F32(0)
    with np.errstate(over="ignore", invalid="ignore"):
        for v in s:
            sum_exp = F32(sum_exp + expf(F32(best - v)))
        log_den = F32(best - logf(sum_exp))
        post = np.array([expf(F32(log_den - v)) for v in s], np.float32)
    return post, log_den


def posteriors(model, frames, pf, pm, row_stride):
    """The call's outputs for the pair lists: (posteriors [n_pairs, row_stride] f32, log_denominator [n_pairs] f32, the
    scores s as a list of arrays); a pair out of range or on an empty mixture: zeros, +inf."""
    ms = model.ms
    post = np.zeros((len(pf), row_stride), np.float32)
    logden = np.full(len(pf), np.inf, np.float32)
    scores = []
    for i, (f, m) in enumerate(zip(np.asarray(pf, np.int64), np.asarray(pm, np.int64))):
        s = np.empty(0, np.float32)
        if f < frames.shape[0] and m < ms.n_mixtures:
            s = model.scores(frames[f], m)
        if len(s):
            post[i, :len(s)], logden[i] = posterior_row(s)
        scores.append(s)
    return post, logden, scores


def posterior_bounds(logden_ref, scores, post_ref):
    """The issue's tolerance: (bound on |logDen - ref| [n_pairs], bound on |post - ref| [n_pairs, row_stride]).
    2 ulp32(|logDen|) for the log denominator; for a posterior the log denominator's rounding, the rounding of the
    exponent's argument, four function ulps plus the sum's relative drift (2^-20), all relative to the posterior,
    and a floor at the smallest normal (subnormal handling may differ)."""
    with np.errstate(invalid="ignore"):
        b_log = np.where(np.isfinite(logden_ref), 2 * ulp32(logden_ref), 0.0)
        b_post = np.full(post_ref.shape, 2.0 ** -126)
        for i, s in enumerate(scores):
            if len(s):
                arg = F32(logden_ref[i]) - s
                rel = 2 * ulp32(logden_ref[i]) + ulp32(arg) + 2.0 ** -20
                b_post[i, :len(s)] += rel * post_ref[i, :len(s)].astype(np.float64)
    return b_log, b_post


def row_sum_bound(logden, s, post, function_ulps):
    """Bound on |sum_j post_j - 1| of one row.  With L the exact -log sum exp(-s_j), the exact exp(L - s_j) sum to 1;
    post_j differs from that by the relative errors of: logDen against L (its own rounding, up to ulp32(logDen),
    which covers the rounding of logf's result, and the sum's n + 1 roundings of 2^-24), the rounding of the
    argument logDen - s_j, and `function_ulps` f32 ulps (2^-24 each as a relative error of 2^-23 at most) for the
    expf / logf calls on the way.  The sum of a row therefore moves with the size of the scores: ulp32(logDen) is
    2^-18 at logDen = 40."""
    n = len(s)
    arg = F32(logden) - s
    rel = ulp32(logden) + ulp32(arg) + (n + 1 + 2 * function_ulps) * 2.0 ** -24
    return float((rel * post[:n].astype(np.float64)).sum())


# ---------------------------------------------------------------------------------------------------------------
# accumulation
# ---------------------------------------------------------------------------------------------------------------

def zero_tables(top):
    D = top.dimension
    return {"mean_sums": np.zeros((top.means.shape[0], D)), "mean_weights": np.zeros(top.means.shape[0]),
            "covariance_sums": np.zeros((top.n_covariances, D)), "covariance_weights": np.zeros(top.n_covariances),
            "entry_weights": np.zeros(top.n_entries)}


def expand(top, n_frames, pf, pm, pw, post, threshold):
    """The live contributions of a posterior call in (pair, density) order: (frame [n], entry [n], weight [n] f64,
    skipped pairs, contributions before the threshold).  post [n_pairs, >= K_max] f32: the posteriors to use."""
    off = top.mixture_offsets.astype(np.int64)
    wide = widen(post).reshape(np.shape(post))
    fr, en, we, skipped, total = [], [], [], 0, 0
    for i, (f, m) in enumerate(zip(np.asarray(pf, np.int64), np.asarray(pm, np.int64))):
        if f >= n_frames or m >= top.n_mixtures or off[m + 1] == off[m]:
            skipped += 1
            continue
        w = np.float64(1.0 if pw is None else pw[i])
        for j in range(off[m + 1] - off[m]):
            total += 1
            fw = w * wide[i, j]
            if fw > threshold:  # strict, f64; NaN does not pass
                fr.append(f), en.append(off[m] + j), we.append(fw)
    return np.array(fr, np.int64), np.array(en, np.int64), np.array(we, np.float64), skipped, total


def _ordered(sums, weights, dest, x, w, square, chunk):
    """One table: dest[i] the accumulator of contribution i, x [n, D] f64 or None, w [n]."""
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


def accumulate(top, frames, fr, en, we, tables=None, chunk=CHUNK):
    """The tables after one call whose contributions are (frame, entry, weight) in order; chunk=None: the purely
    sequential sums."""
    t = {k: v.copy() for k, v in (tables or zero_tables(top)).items()}
    x = frames[fr].astype(np.float64).reshape(len(fr), top.dimension)
    dens = top.mixture_densities[en]
    chunk = chunk or max(len(en), 1)
    _ordered(t["mean_sums"], t["mean_weights"], top.density_mean[dens], x, we, False, chunk)
    _ordered(t["covariance_sums"], t["covariance_weights"], top.density_covariance[dens], x, we, True, chunk)
    _ordered(None, t["entry_weights"], en, None, we, False, chunk)
    return t


def expected_file(top, t):
    """oracle.estimator.write_estimator_file of the tables after MixtureSetEstimatorIndexMap's first-appearance
    renumbering (AbstractMixtureSetEstimator.cc:804-817)."""
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
    return est.write_estimator_file(None, top.dimension, means, covs, dens, mix)


def assert_bit_equal(got, want):
    for k in TABLES:
        assert got[k].shape == want[k].shape, k
        same = np.ascontiguousarray(got[k]).view(np.uint64) == np.ascontiguousarray(want[k]).view(np.uint64)
        assert same.all(), f"{k}: {int((~same).sum())} of {same.size} elements differ"
