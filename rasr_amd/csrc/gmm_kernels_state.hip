// gmm_kernels_state.hip -- state posteriors over a mixture-major score table (gmm_state_posteriors_*).
//
// Mm::StatePosteriorFeatureScorer in Viterbi / mixture mode (StatePosteriorFeatureScorer.cc:81-160, 258-284), per
// frame over the handle's mixtures, every f64 operation one explicit _rn intrinsic:
//   s_m    = prior_m + scale * (f64) score(m)                              workMixtureScores, cc:90
//   min    = the strict-compare scan from DBL_MAX in ascending m            cc:85-94 (minimumScore, minimumIndex)
//   active = every m without pruning, else s_m < pruning_threshold + min    pruneScores, cc:105-116
//   sum    = the sum of exp(min - s_m) over the active m != minimumIndex    workPosteriors, cc:131-138
//   logZ'  = log1p(sum);  p_m = exp((min - s_m) - logZ');  logZ = logZ' - min   cc:139-143
// exp / log1p are the device library's f64 functions.
//
// The table is mixture-major, so a lane takes a frame and a row of 256 frames is one coalesced 1 KiB read.  A workgroup
// of 256 lanes takes 256 frames and one PIECE of kStatePieceMixtures consecutive mixtures; the table is walked three
// times:
//   stateMin    the piece's strict scan in ascending m                    -> partMin, partIdx [piece][frame]
//   stateSum    the frame's minimum from the pieces' (piece order, strict <: the lowest index wins ties), then the
//               piece's terms added sequentially from 0 in ascending m    -> partSum, partCount [piece][frame]
//   stateWrite  minimum and sum from the pieces' (sequentially from 0 in piece order), log1p, the elementwise write;
//               the workgroups of piece 0 also write the per-frame outputs
// The order of every sum is fixed by the mixture index alone, so the result is the same bit for bit for every frame
// count, stride and launch geometry.  stateWrite reads score(m, t) and writes p(m, t) in the same lane, with nothing
// else read from the table: posteriors_f32 may be the score table itself.
// Rows are loaded kRowsInFlight at a time before they are used: the output may alias the input, so the compiler
// cannot move a row's load over the previous row's store by itself.
#include "gmm_device.hh"

#include <cfloat>

namespace rasr_gmm {
namespace dev {
namespace {

constexpr uint32_t kStateFramesPerBlock = 256;
constexpr uint32_t kRowsInFlight        = 8;

// workgroup -> (frame block, piece): frame blocks fastest, so neighbouring workgroups read neighbouring lines
__device__ __forceinline__ bool stateCell(const StateArgs& a, uint32_t& t, uint32_t& m0, uint32_t& m1, uint32_t& piece) {
    const uint32_t nFrameBlocks = (a.nFrames + kStateFramesPerBlock - 1) / kStateFramesPerBlock;
    piece                       = blockIdx.x / nFrameBlocks;
    t                           = (blockIdx.x % nFrameBlocks) * kStateFramesPerBlock + threadIdx.x;
    m0                          = piece * kStatePieceMixtures;
    m1                          = min(m0 + kStatePieceMixtures, a.nMixtures);
    return t < a.nFrames;
}

__device__ __forceinline__ double stateScore(const StateArgs& a, uint32_t m, float score) {
    const double prior = a.priors ? a.priors[m] : 0.0;
    return __dadd_rn(prior, __dmul_rn(a.scale, static_cast<double>(score)));
}

// body(m, s_m) for the mixtures [m0, m1) of frame t in ascending m
template <class Body>
__device__ __forceinline__ void forRows(const StateArgs& a, uint32_t t, uint32_t m0, uint32_t m1, Body body) {
    for (uint32_t m = m0; m < m1; m += kRowsInFlight) {
        float v[kRowsInFlight];
#pragma unroll
        for (uint32_t u = 0; u < kRowsInFlight; ++u)
            v[u] = m + u < m1 ? a.scores[static_cast<size_t>(m + u) * a.scoreStride + t] : 0.0f;
#pragma unroll
        for (uint32_t u = 0; u < kRowsInFlight; ++u)
            if (m + u < m1)
                body(m + u, stateScore(a, m + u, v[u]));
    }
}

// the frame's minimum and its mixture from the pieces', in piece order
__device__ __forceinline__ void frameMinimum(const StateArgs& a, uint32_t t, double& mn, uint32_t& mi) {
    mn = DBL_MAX;
    mi = 0xffffffffu;
    for (uint32_t q = 0; q < a.nPieces; ++q) {
        const size_t at = static_cast<size_t>(q) * a.partStride + t;
        const double v  = a.partMin[at];
        if (v < mn) {
            mn = v;
            mi = a.partIdx[at];
        }
    }
}

struct ActiveTest {
    bool   prune;
    double threshold;  // pruning_threshold + min
    __device__ __forceinline__ ActiveTest(const StateArgs& a, double mn)
        : prune(a.pruningThreshold < DBL_MAX), threshold(__dadd_rn(a.pruningThreshold, mn)) {}
    __device__ __forceinline__ bool operator()(double s) const { return !prune || s < threshold; }
};

}  // namespace

__global__ __launch_bounds__(256) void stateMin(StateArgs a) {
    uint32_t t, m0, m1, piece;
    if (!stateCell(a, t, m0, m1, piece))
        return;
    double   mn = DBL_MAX;
    uint32_t mi = 0xffffffffu;
    forRows(a, t, m0, m1, [&](uint32_t m, double s) {
        if (s < mn) {
            mn = s;
            mi = m;
        }
    });
    const size_t at = static_cast<size_t>(piece) * a.partStride + t;
    a.partMin[at]   = mn;
    a.partIdx[at]   = mi;
}

__global__ __launch_bounds__(256) void stateSum(StateArgs a) {
    uint32_t t, m0, m1, piece;
    if (!stateCell(a, t, m0, m1, piece))
        return;
    double   mn;
    uint32_t mi;
    frameMinimum(a, t, mn, mi);
    const ActiveTest active(a, mn);
    double           sum   = 0.0;
    uint32_t         count = 0;
    forRows(a, t, m0, m1, [&](uint32_t m, double s) {
        if (active(s)) {
            ++count;
            if (m != mi)
                sum = __dadd_rn(sum, exp(__dsub_rn(mn, s)));
        }
    });
    const size_t at = static_cast<size_t>(piece) * a.partStride + t;
    a.partSum[at]   = sum;
    a.partCount[at] = count;
}

__global__ __launch_bounds__(256) void stateWrite(StateArgs a) {
    uint32_t t, m0, m1, piece;
    if (!stateCell(a, t, m0, m1, piece))
        return;
    double   mn;
    uint32_t mi;
    frameMinimum(a, t, mn, mi);
    double   sum   = 0.0;
    uint32_t count = 0;
    for (uint32_t q = 0; q < a.nPieces; ++q) {
        const size_t at = static_cast<size_t>(q) * a.partStride + t;
        sum             = __dadd_rn(sum, a.partSum[at]);
        count += a.partCount[at];
    }
    const double logZ = log1p(sum);
    if (piece == 0) {
        if (a.logZ)
            a.logZ[t] = __dsub_rn(logZ, mn);
        if (a.minScore)
            a.minScore[t] = mn;
        if (a.minIndex)
            a.minIndex[t] = mi;
        if (a.nActive)
            a.nActive[t] = count;
    }
    if (!a.post32 && !a.post64)
        return;
    const ActiveTest active(a, mn);
    forRows(a, t, m0, m1, [&](uint32_t m, double s) {
        const double p  = active(s) ? exp(__dsub_rn(__dsub_rn(mn, s), logZ)) : 0.0;
        const size_t at = static_cast<size_t>(m) * a.postStride + t;
        if (a.post64)
            a.post64[at] = p;
        if (a.post32)
            a.post32[at] = static_cast<float>(p);
    });
}

}  // namespace dev

hipError_t launchStatePosteriors(const StateArgs& a, hipStream_t stream) {
    if (a.nFrames == 0 || a.nMixtures == 0)
        return hipSuccess;
    const uint32_t nFrameBlocks = (a.nFrames + dev::kStateFramesPerBlock - 1) / dev::kStateFramesPerBlock;
    const dim3     grid(nFrameBlocks * a.nPieces), block(dev::kStateFramesPerBlock);
    hipLaunchKernelGGL(dev::stateMin, grid, block, 0, stream, a);
    hipLaunchKernelGGL(dev::stateSum, grid, block, 0, stream, a);
    hipLaunchKernelGGL(dev::stateWrite, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace rasr_gmm
