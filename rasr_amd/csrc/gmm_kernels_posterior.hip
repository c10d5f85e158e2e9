// gmm_kernels_posterior.hip -- density posteriors of a list of (frame, mixture) pairs (gmm_density_posteriors_pairs_*)
// and their expansion into the Baum-Welch contributions of gmm_estimator_accumulate_posteriors_*.
//
// GaussDiagonalSumFeatureScorer (GaussDiagonalMaximumFeatureScorer.cc:238-298) per pair, n the mixture's entry count:
//   s_j     = 0.5f * ((w_j + logNorm_cov) + distance_j)            calculateScoresAndNumberOfDensities, cc:251-260
//   best    = the strict-compare scan from FLT_MAX in entry order   cc:266-276
//   sumExp  = 0; sumExp = sumExp + expf(best - s_j) in entry order  cc:279-282
//   logDen  = best - logf(sumExp)                                   cc:286
//   post_j  = expf(logDen - s_j)                                    calculateDensityPosteriorProbabilities, cc:296
// The s_j are bestPairs<kPairDiagonalSum>'s values (gmm_kernels_pairs.hip; refDistance is that file's function,
// duplicated here so that neither file's code depends on the other), every f32 operation one explicit _rn
// intrinsic, expf / logf the device library's functions.  One wave per pair: lanes over 64 entries at a time, the
// scan and the sum handed round by v_readlane in entry order (they are wave-uniform), so a row is the same bit
// for bit in every run and for every launch geometry.  The row itself holds the s_j between the passes: lane l
// writes and re-reads only its own elements j = l, l + 64, ...
// A pair whose frame or mixture is out of range, or whose mixture is empty, gets a row of zeros and +inf; its frame
// is never read.
//
// EXPAND (the estimator's call): the tail that writes post_j also writes contribution slot c = pair * rowStride + j:
// finalWeight = pairWeight * (f64) post_j (one f64 multiply), the pair's frame, and the three destination keys of
// gmm_kernels_accum.hip -- the sentinel where j is past the mixture, the pair is bad or finalWeight is not above the
// threshold (a strict f64 compare; NaN does not pass).  The stable sorts of that file then order every destination's
// contributions by slot, which is (pair, density in mixture): the reference's loop order
// (AbstractMixtureSetEstimator.cc:137-145).
#include "gmm_device.hh"

#include <cfloat>

namespace rasr_gmm {
namespace dev {
namespace {

__device__ __forceinline__ uint32_t readLane(uint32_t v, uint32_t j) {
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(j)));
}

// reference-order f32 distance of entry i: gmm_kernels_pairs.hip's refDistance, operation for operation
__device__ __forceinline__ float refDistance(const PairArgs& a, const float* x, uint32_t i, uint32_t cov) {
    const float*   mu  = a.fMean + static_cast<size_t>(i) * a.L;
    const float*   iv  = a.isv + static_cast<size_t>(cov) * a.L;
    const uint32_t nfb = a.D / 4u;
    float          s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (uint32_t b = 0; b < a.nb; ++b) {
        const uint32_t k  = 4u * b;
        const bool     in = b < nfb;
        const float    x0 = in ? x[k] : 0.0f, x1 = in ? x[k + 1] : 0.0f, x2 = in ? x[k + 2] : 0.0f,
                    x3 = in ? x[k + 3] : 0.0f;
        const float d0 = __fmul_rn(__fsub_rn(mu[k], x0), iv[k]);
        const float d1 = __fmul_rn(__fsub_rn(mu[k + 1], x1), iv[k + 1]);
        const float d2 = __fmul_rn(__fsub_rn(mu[k + 2], x2), iv[k + 2]);
        const float d3 = __fmul_rn(__fsub_rn(mu[k + 3], x3), iv[k + 3]);
        s0             = __fadd_rn(s0, __fmul_rn(d0, d0));
        s1             = __fadd_rn(s1, __fmul_rn(d1, d1));
        s2             = __fadd_rn(s2, __fmul_rn(d2, d2));
        s3             = __fadd_rn(s3, __fmul_rn(d3, d3));
    }
    float r = __fadd_rn(__fadd_rn(s0, s1), __fadd_rn(s2, s3));
    for (uint32_t j = 0; j < 3u; ++j) {
        const uint32_t k  = 4u * a.nb + j, dim = 4u * nfb + j;
        const float    xv = dim < a.D ? x[dim] : 0.0f;
        const float    d  = __fmul_rn(__fsub_rn(mu[k], xv), iv[k]);
        r                 = __fadd_rn(r, __fmul_rn(d, d));
    }
    return r;
}

}  // namespace

template <bool EXPAND>
__global__ __launch_bounds__(256) void densityPosteriorsPairs(PosteriorArgs q) {
    const PairArgs& a    = q.pair;
    const uint32_t  lane = threadIdx.x & 63u;
    const uint32_t  p    = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (p >= a.nPairs)
        return;
    const uint32_t f = a.pairFrame[p], m = a.pairMix[p];
    uint32_t       e0 = 0, n = 0;  // n == 0: a bad pair (out of range, or an empty mixture)
    if (f < a.nFrames && m < a.nMixtures) {
        e0 = a.mixOff[m];
        n  = a.mixOff[m + 1] - e0;
    }
    n            = min(n, q.rowStride);  // the callers refuse a smaller row_stride: no store past the row either way
    float* row   = q.posteriors + static_cast<size_t>(p) * q.rowStride;
    float  logDen = __uint_as_float(0x7f800000u);  // +inf
    if (n) {
        const float* x = a.frames + static_cast<size_t>(f) * a.frameStride;
        // the density scores into the row, and the reference's scan over them in entry order
        float best = FLT_MAX;  // Core::Type<Score>::max
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t j = base + lane;
            float          s = 0.0f;
            if (j < n) {
                const uint32_t i = e0 + j, cov = a.entryCov[i];
                const float    r = refDistance(a, x, i, cov);
                s                = __fmul_rn(0.5f, __fadd_rn(__fadd_rn(a.fConst[i], a.fLogNorm[cov]), r));
                row[j]           = s;
            }
            const uint32_t cnt = min(64u, n - base);
            for (uint32_t u = 0; u < cnt; ++u) {
                const float sv = __uint_as_float(readLane(__float_as_uint(s), u));
                if (best > sv)
                    best = sv;
            }
        }
        float sumExp = 0.0f;
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t j = base + lane;
            float          t = 0.0f;
            if (j < n)
                t = expf(__fsub_rn(best, row[j]));
            const uint32_t cnt = min(64u, n - base);
            for (uint32_t u = 0; u < cnt; ++u)
                sumExp = __fadd_rn(sumExp, __uint_as_float(readLane(__float_as_uint(t), u)));
        }
        logDen = __fsub_rn(best, logf(sumExp));
    }
    double w = 1.0;
    if constexpr (EXPAND)
        if (n && q.pairWeight)
            w = q.pairWeight[p];
    for (uint32_t j = lane; j < q.rowStride; j += 64u) {
        float post = 0.0f;
        if (j < n)
            post = expf(__fsub_rn(logDen, row[j]));
        row[j] = post;
        if constexpr (EXPAND) {
            const size_t c  = static_cast<size_t>(p) * q.rowStride + j;
            uint32_t     km = q.nMeans, kc = q.nCovs, ke = q.nEntries, fr = 0;
            double       fw = 0.0;
            if (j < n) {
                fr = f;
                fw = __dmul_rn(w, static_cast<double>(post));  // Mm::Weight finalWeight = weight * dnsWeight
                if (fw > q.threshold && e0 + j < q.nEntries) {
                    ke = e0 + j;
                    km = q.entryMean[ke];
                    kc = q.entryCov[ke];
                }
            }
            q.keyMean[c]       = km;
            q.keyCov[c]        = kc;
            q.keyEntry[c]      = ke;
            q.contribIndex[c]  = static_cast<uint32_t>(c);
            q.contribFrame[c]  = fr;
            q.contribWeight[c] = fw;
        }
    }
    if (lane == 0) {
        if (q.logDen)
            q.logDen[p] = logDen;
        if constexpr (EXPAND)
            if (n == 0)
                atomicAdd(q.skipped, 1ull);
    }
}

__global__ __launch_bounds__(256) void expandSingleDensity(PosteriorArgs q) {
    const PairArgs& a = q.pair;
    const uint32_t  p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.nPairs)
        return;
    const uint32_t f = a.pairFrame[p], m = a.pairMix[p];
    uint32_t       km = q.nMeans, kc = q.nCovs, ke = q.nEntries, fr = 0;
    double         fw = 0.0;
    const bool     ok = f < a.nFrames && m < a.nMixtures;
    if (ok) {
        fr = f;
        fw = __dmul_rn(q.pairWeight ? q.pairWeight[p] : 1.0, 1.0);  // posteriors.push_back(1.0), cc:399-400
        if (fw > q.threshold) {
            ke = a.mixOff[m];
            km = q.entryMean[ke];
            kc = q.entryCov[ke];
        }
    }
    q.keyMean[p]       = km;
    q.keyCov[p]        = kc;
    q.keyEntry[p]      = ke;
    q.contribIndex[p]  = p;
    q.contribFrame[p]  = fr;
    q.contribWeight[p] = fw;
    if (!ok)
        atomicAdd(q.skipped, 1ull);
}

}  // namespace dev

hipError_t launchDensityPosteriors(const PosteriorArgs& a, hipStream_t stream) {
    if (a.pair.nPairs == 0)
        return hipSuccess;
    if (a.pair.kind != kPairDiagonalSum)
        return hipErrorInvalidValue;
    const dim3 grid((a.pair.nPairs + 3u) / 4u);
    if (a.keyMean)
        hipLaunchKernelGGL(dev::densityPosteriorsPairs<true>, grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(dev::densityPosteriorsPairs<false>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchExpandSingleDensity(const PosteriorArgs& a, hipStream_t stream) {
    if (a.pair.nPairs == 0)
        return hipSuccess;
    hipLaunchKernelGGL(dev::expandSingleDensity, dim3((a.pair.nPairs + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rasr_gmm
