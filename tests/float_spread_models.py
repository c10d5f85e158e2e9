"""The spread ladder of tests/test_float_spread.py and tests/test_float_spread_cpu.py, and the numpy restatement of
the spread statistic (include/rasr_gmm.h gmm_float_spread_bound).

The float kernels evaluate ||x'||^2 + ||m'||^2 - 2 x'.m' about one centre c (the mean of all means) in f32.  For a
frame near a density far from c in units of its deviations the three terms are of size rho^2 = sum ((mu - c) / sigma)^2
and cancel; the reference squares (mu - x) / sigma and has no such terms.  The ladder widens the means step by step.
"""
import functools

import numpy as np

import oracle
import rasr_amd as ra

SPREADS = (1, 2, 3, 5, 8)
N_FRAMES = 256


@functools.lru_cache(maxsize=None)
def spread_model(s, d, c=1, m=80, seed=41):
    """The shape of test_gpu_parity._offset_model (m ragged mixtures of 1-40 densities, 20 m densities in all, random
    weights) with means ~ N(0, s^2) in every dimension and variances ~ U[0.01, 0.1]: rms |mu - c| / sigma = 4.8 s."""
    counts = ra.ragged_counts(m, m * 20, low=1, high=40, seed=seed)
    base = ra.synthetic_mixture_set(m, counts, d, seed=seed, n_covariances=c, weights="random")
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    var = rng.uniform(0.01, 0.1, (c, d)).astype(np.float32)
    means = (np.float32(s) * rng.standard_normal(base.means.shape)).astype(np.float32)
    return ra.MixtureSet(means, var, base.density_mean, base.density_covariance, base.mixture_offsets,
                         base.mixture_densities, base.mixture_log_weights)


def density_rho2(ms):
    """rho_d^2 = sum ((mu_d - c) / sigma_d)^2 per density, float64."""
    mean = ms.means[ms.density_mean].astype(np.float64)
    var = ms.variances[ms.density_covariance].astype(np.float64)
    return (((mean - ms.means.astype(np.float64).mean(0)) ** 2) / var).sum(1)


@functools.lru_cache(maxsize=None)
def ladder_frames(s, d, c=1, m=80, seed=43, spread=0.05):
    """N_FRAMES frames for spread_model(s, d, c, m):
    * rows 0 .. 239 at mu +- spread * sigma of a density (test_gpu_parity._frames_near): random densities, the 16 of
      largest rho among them -- x' ~ m' with both far from the centre, where the cancellation is worst;
    * every 8th of those rows drawn about the centre instead;
    * rows 240 .. 255 at c + 2 (mu - c) of the 16 densities of largest rho: r >> rho, a large score whose relative
      error should stay small."""
    ms = spread_model(s, d, c, m)
    rng = np.random.Generator(np.random.PCG64(seed + 7 * s + d))
    n_near = N_FRAMES - 16
    far = np.argsort(density_rho2(ms))[::-1][:16]
    dens = rng.integers(0, ms.n_densities, n_near)
    dens[[i for i in range(n_near) if i % 8][:16]] = far
    sd = np.sqrt(ms.variances[ms.density_covariance[dens]])
    frames = np.empty((N_FRAMES, d), np.float64)
    frames[:n_near] = ms.means[ms.density_mean[dens]] + spread * sd * rng.choice([-1.0, 1.0], size=(n_near, d))
    centre = ms.means.astype(np.float64).mean(0)
    frames[:n_near:8] = centre + rng.standard_normal((len(frames[:n_near:8]), d))
    frames[n_near:] = centre + 2.0 * (ms.means[ms.density_mean[far]].astype(np.float64) - centre)
    out = frames.astype(np.float32)
    out.setflags(write=False)
    return out


def spread_statistic(ms, kind="diagonal-maximum", mixture_weight_scale=1.0, gaussian_scale=1.0, covariance_free=False,
                     mixture_range=None):
    """max over the mixture entries e of 2^-23 rho_e^2 / max(1, |c_e / 2|) in float64, from the scorer's own f32 tables:
    isv = 1 / sqrt(var) as the reference computes it (oracle.inverse_sqrt), times sqrt(gaussian scale) for
    diagonal-maximum / diagonal-sum; the centre (f32) = the f64 mean of all means; rho_e^2 over the f32 operands
    m' = (f32) ((mu - c) isv), or with covariance_free (several covariances on the split-f16 kernels) over isv^2
    (mu - c)^2 in f64; c_e = (f32) (-2 log w_e) * mixture-weight scale + logNorm, batch-float (f32) (logNorm - 2 log w_e).
    Returns (statistic, entry that attains it)."""
    scaled = kind in ("diagonal-maximum", "diagonal-sum")
    isv = np.array([[oracle.inverse_sqrt(float(v)) for v in row] for row in ms.variances], np.float32)
    log_norm = np.array([oracle.gauss_log_norm(row) for row in ms.variances]).astype(np.float32)
    if scaled:
        gs = np.float32(np.sqrt(np.float64(np.float32(gaussian_scale))))
        isv = isv * gs
        log_norm = log_norm * (gs * gs)
    acc = np.zeros(ms.dimension, np.float64)
    for row in ms.means.astype(np.float64):  # the library's order: sequential
        acc += row
    centre = (acc / len(ms.means)).astype(np.float32).astype(np.float64)
    b, e = (0, ms.n_mixtures) if mixture_range is None else mixture_range
    lo, hi = int(ms.mixture_offsets[b]), int(ms.mixture_offsets[e])
    dens = ms.mixture_densities[lo:hi]
    cov = ms.density_covariance[dens]
    mu = ms.means[ms.density_mean[dens]].astype(np.float64) - centre
    iv = isv[cov].astype(np.float64)
    if covariance_free:
        rho2 = (iv * iv * mu * mu).sum(1)
    else:
        rho2 = ((mu * iv).astype(np.float32).astype(np.float64) ** 2).sum(1)
    lw = np.asarray(ms.mixture_log_weights[lo:hi], np.float64)
    if scaled:
        const = ((-2 * lw).astype(np.float32) * np.float32(mixture_weight_scale)).astype(np.float64) + log_norm[cov]
    else:
        const = (log_norm[cov].astype(np.float64) - 2 * lw).astype(np.float32).astype(np.float64)
    stat = 2.0 ** -23 * rho2 / np.maximum(1.0, np.abs(0.5 * const))
    i = int(np.argmax(stat))
    return float(stat[i]), lo + i
