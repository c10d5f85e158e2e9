// gmm_kernels_accum.hip -- accumulation of aligned (frame, mixture, density) pairs into the f64 statistics of a mixture
// set's means, covariances and mixture entries: the maximum-likelihood calls (gmm_estimator_accumulate_*) and the joint
// numerator / denominator calls of discriminative training (gmm_estimator_accumulate_discriminative_*),
// include/rasr_gmm_estimator.h.
//
// The reference adds one pair at a time (AbstractMixtureEstimator::accumulate -> GaussDensityEstimator::accumulate
// -> VectorAccumulator, plusWeighted / plusSquareWeighted, src/Mm/Utilities.hh:110-146): a scatter-add whose f64
// sums depend on the order of the adds.  Floating-point atomics would make that order the arrival order; this file
// uses the store-and-sum form instead: nothing is scattered, every destination gathers its own contributions in a
// fixed order through an inverted index, and the result is the header's numeric contract bit for bit.
//   1. resolvePairs: a pair -> its mixture entry, mean and covariance (three keys); a pair that is out of range in
//      any way gets the sentinel key (the destination count) and is counted with an integer atomic.  Its frame is
//      never read.  The joint Baum-Welch call has expandPosteriorRows in this place, over posterior rows computed once
//      by gmm_kernels_posterior.hip (the maximum-likelihood one expands in the tail of that kernel).
//   2. three stable radix sorts of (key, pair index) by key (rocPRIM, key bits restricted to the destination
//      range): per destination the list of its pairs, in pair order; the sentinel keys sort behind them.
//   3. accumulateSegments: one wave per (destination, piece of GMM_ESTIMATOR_CHUNK contributions).  A wave is
//      started for every sorted position and goes on only at a piece head, which it recognises by neighbour
//      compares and, inside a run of equal keys, a binary search for the run's start -- no compaction pass, no
//      counters.  Lanes run over the dimensions (d = lane, lane + 64, ...), so a frame row is one coalesced read
//      and any dimension works; the piece's pair indices, frames and weights are fetched 64 at a time, one per
//      lane, and handed out by v_readlane (they are wave-uniform).  What must stay serial is the chain of
//      dependent f64 adds, not the loads: the rows of kRowsAhead pairs are fetched before the adds that need them,
//      so a full piece costs GMM_ESTIMATOR_CHUNK / kRowsAhead memory latencies, not GMM_ESTIMATOR_CHUNK.
//      Piece 0 starts from the table's value and writes it back; a later piece starts from 0 and writes a row of
//      the partial slab (the piece at sorted position i owns slot i / GMM_ESTIMATOR_CHUNK).
//   4. combinePieces: a destination with more than one piece adds its slab rows to the table in piece order.
// The heavy destination is the pooled covariance (every pair of a call): the split rule makes it
// n / GMM_ESTIMATOR_CHUNK waves instead of one.
//
// SIDES.  The kernels are templates over the number of table sets a call adds to, one f64 add chain per lane and side.
//   SIDES = 1, the maximum-likelihood calls: a NULL weight array means every weight is 1, and a NaN weight is added like
//      any other value; resolve keys every in-range pair.
//   SIDES = 2, the discriminative calls: one resolve, one set of sorts and one read of every frame row feed both chains.
//      A side whose weight array is NULL takes no part: its tables are neither read nor written.  A NaN weight marks a
//      contribution that is not live on that side, and the side adds nothing for it -- never 0 * x, which is NaN for an
//      infinite x and turns a -0.0 sum into +0.0; the weights are wave-uniform, so the test is a scalar branch.  A pair
//      or slot live on neither side takes the sentinel keys, as a skipped pair does, so the call's contribution list
//      (which the pieces are cut from) is the slots live on at least one side.  A bad pair is counted once.
// Every f64 operation is one __dmul_rn / __dadd_rn; the unit is built with -ffp-contract=off.  No float atomics.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "gmm_estimator.hh"

namespace rasr_gmm {
namespace dev {

constexpr uint32_t kWave      = 64;
constexpr uint32_t kRowsAhead = 16;  // frame rows in flight ahead of the add chains

__device__ __forceinline__ uint32_t readLane(uint32_t v, uint32_t j) {
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(j)));
}
__device__ __forceinline__ double readLane(double v, uint32_t j) {
    const uint64_t b  = static_cast<uint64_t>(__double_as_longlong(v));
    const uint64_t lo = readLane(static_cast<uint32_t>(b), j), hi = readLane(static_cast<uint32_t>(b >> 32), j);
    return __longlong_as_double(static_cast<long long>((hi << 32) | lo));
}

__device__ __forceinline__ double notLive() {
    return __longlong_as_double(0x7ff8000000000000ll);  // quiet NaN
}

template <int SIDES>
__global__ __launch_bounds__(256) void resolvePairs(ResolveArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.nPairs)
        return;
    const uint32_t f = a.pairFrame[p], m = a.pairMix[p];
    uint32_t       km = a.nMeans, kc = a.nCovs, ke = a.nEntries;  // skipped, or (SIDES 2) live on neither side
    bool           ok = f < a.nFrames && m < a.nMix;
    if (ok) {
        const uint32_t e0 = a.mixOff[m], e1 = a.mixOff[m + 1];
        const uint32_t d  = a.pairDensity ? a.pairDensity[p] : 0u;  // 0xffffffff (no best density) is out of range
        ok                = d < e1 - e0;
        bool live         = ok;
        if (SIDES == 2 && ok) {
            const double w0 = a.weight[0] ? a.weight[0][p] : notLive();
            const double w1 = a.weight[1] ? a.weight[1][p] : notLive();
            live            = w0 == w0 || w1 == w1;
        }
        if (live) {
            ke = e0 + d;
            km = a.entryMean[ke];
            kc = a.entryCov[ke];
        }
    }
    a.keyMean[p]   = km;
    a.keyCov[p]    = kc;
    a.keyEntry[p]  = ke;
    a.pairIndex[p] = p;
    if (!ok)
        atomicAdd(a.skipped, 1ull);
}

// one thread per contribution slot
__global__ __launch_bounds__(256) void expandPosteriorRows(ExpandArgs q) {
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
    if (c >= static_cast<uint64_t>(q.nPairs) * q.rowStride)
        return;
    const uint32_t p = static_cast<uint32_t>(c / q.rowStride), j = static_cast<uint32_t>(c % q.rowStride);
    const uint32_t f = q.pairFrame[p], m = q.pairMix[p];
    uint32_t       e0 = 0, n = 0;  // n == 0: a bad pair (out of range, or an empty mixture)
    if (f < q.nFrames && m < q.nMix) {
        e0 = q.mixOff[m];
        n  = q.mixOff[m + 1] - e0;
    }
    uint32_t km = q.nMeans, kc = q.nCovs, ke = q.nEntries, fr = 0;
    double   fn = notLive(), fd = notLive();
    if (j < n && e0 + j < q.nEntries) {
        fr                = f;
        const double post = static_cast<double>(q.posteriors ? q.posteriors[c] : 1.0f);
        // Mm::Weight finalWeight = weight * dnsPosteriors[index]; live iff finalWeight > weightThreshold_
        if (q.weight[0]) {
            const double fw = __dmul_rn(q.weight[0][p], post);
            if (fw > q.threshold)
                fn = fw;
        }
        if (q.weight[1]) {
            const double fw = __dmul_rn(q.weight[1][p], post);
            if (fw > q.threshold)
                fd = fw;
        }
        if (fn == fn || fd == fd) {
            ke = e0 + j;
            km = q.entryMean[ke];
            kc = q.entryCov[ke];
        }
    }
    q.keyMean[c]      = km;
    q.keyCov[c]       = kc;
    q.keyEntry[c]     = ke;
    q.contribIndex[c] = static_cast<uint32_t>(c);
    q.contribFrame[c] = fr;
    if (q.weight[0])
        q.contribWeight[0][c] = fn;
    if (q.weight[1])
        q.contribWeight[1][c] = fd;
    if (j == 0 && n == 0)
        atomicAdd(q.skipped, 1ull);
}

// first position of the run of key k that position i belongs to (keys ascending, keys[i] == k)
__device__ __forceinline__ uint32_t runStart(const uint32_t* keys, uint32_t i, uint32_t k) {
    uint32_t lo = 0, hi = i;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// one side's adds of one contribution: the sum of the lane's dimension (act) and, in the first lane block, the weight
template <int MODE, int SIDES>
__device__ __forceinline__ void addContribution(double& acc, double& wsum, double w, double xd, bool act, bool lead) {
    if (SIDES == 1 || w == w) {  // wave-uniform: live on this side
        if (act) {
            const double wx = __dmul_rn(w, xd);
            acc = MODE == kAccumSquare ? __dadd_rn(acc, __dmul_rn(wx, xd)) : __dadd_rn(acc, wx);
        }
        if (lead)
            wsum = __dadd_rn(wsum, w);
    }
}

template <int MODE, int SIDES>
__global__ __launch_bounds__(256) void accumulateSegments(AccumArgs a) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t i    = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));  // sorted position
    if (i >= a.nPairs)
        return;
    const uint32_t k = a.keysSorted[i];
    if (k >= a.nDest)  // a skipped pair, or (SIDES 2) a slot live on neither side
        return;
    uint32_t s = i;
    if (i > 0 && a.keysSorted[i - 1] == k)
        s = runStart(a.keysSorted, i, k);
    if ((i - s) % kAccumChunk != 0)  // not the head of a piece
        return;
    const bool first = i == s;
    // the sides that take part (side 1's chain, acc1 / wsum1 / w1j, is dead code for SIDES 1) and the weight of a
    // contribution without one
    const bool     on0 = SIDES == 1 || a.weight[0] != nullptr, on1 = SIDES == 2 && a.weight[1] != nullptr;
    const double   none  = SIDES == 1 ? 1.0 : notLive();
    const uint32_t limit = min(i + kAccumChunk, a.nPairs);
    double         wsum0 = first && on0 ? a.weights[0][k] : 0.0;
    double         wsum1 = first && on1 ? a.weights[1][k] : 0.0;
    for (uint32_t d0 = 0; d0 == 0 || d0 < a.D; d0 += kWave) {
        const uint32_t d    = d0 + lane;
        const bool     act  = MODE != kAccumWeightOnly && d < a.D;
        double         acc0 = 0.0, acc1 = 0.0;
        if (act && first) {
            if (on0)
                acc0 = a.sums[0][static_cast<size_t>(k) * a.D + d];
            if (on1)
                acc1 = a.sums[1][static_cast<size_t>(k) * a.D + d];
        }
        for (uint32_t b = i; b < limit; b += kWave) {
            // this lane's contribution of the block: its pair's frame and weights
            const uint32_t j  = b + lane;
            uint32_t       fj = 0;
            double         w0j = none, w1j = none;
            bool           in = false;
            if (j < limit && a.keysSorted[j] == k) {
                in               = true;
                const uint32_t p = a.indexSorted[j];
                fj               = a.pairFrame[p];
                if (a.weight[0])
                    w0j = a.weight[0][p];
                if (on1)
                    w1j = a.weight[1][p];
            }
            // the run is contiguous: its contributions are the lanes 0 .. n - 1
            const uint32_t n = static_cast<uint32_t>(__popcll(__ballot(in)));
            for (uint32_t c0 = 0; c0 < n; c0 += kRowsAhead) {
                float x[kRowsAhead];
#pragma unroll
                for (uint32_t u = 0; u < kRowsAhead; ++u) {
                    const uint32_t f = readLane(fj, min(c0 + u, n - 1));  // past the end: the last row again, unused
                    x[u]             = act ? a.frames[static_cast<size_t>(f) * a.frameStride + d] : 0.0f;
                }
#pragma unroll
                for (uint32_t u = 0; u < kRowsAhead; ++u) {
                    if (c0 + u < n) {
                        const double w0 = readLane(w0j, c0 + u), w1 = readLane(w1j, c0 + u);
                        const double xd = static_cast<double>(x[u]);
                        addContribution<MODE, SIDES>(acc0, wsum0, w0, xd, act, d0 == 0);
                        if (SIDES == 2)
                            addContribution<MODE, SIDES>(acc1, wsum1, w1, xd, act, d0 == 0);
                    }
                }
            }
            if (n < kWave)
                break;
        }
        if (act) {
            const size_t at = first ? static_cast<size_t>(k) * a.D + d : static_cast<size_t>(i / kAccumChunk) * a.D + d;
            if (on0)
                (first ? a.sums[0] : a.slabSums[0])[at] = acc0;
            if (on1)
                (first ? a.sums[1] : a.slabSums[1])[at] = acc1;
        }
    }
    if (lane == 0) {
        const uint32_t at = first ? k : i / kAccumChunk;
        if (on0)
            (first ? a.weights[0] : a.slabWeights[0])[at] = wsum0;
        if (on1)
            (first ? a.weights[1] : a.slabWeights[1])[at] = wsum1;
    }
}

// one side of combinePieces: the slab rows of the later pieces of destination k, whose first piece starts at i
__device__ __forceinline__ void combineSide(const AccumArgs& a, double* sums, double* weights, const double* slabSums,
                                            const double* slabWeights, uint32_t i, uint32_t k, uint32_t lane) {
    if (a.mode != kAccumWeightOnly)
        for (uint32_t d = lane; d < a.D; d += kWave) {
            double acc = sums[static_cast<size_t>(k) * a.D + d];
            for (uint32_t pos = i + kAccumChunk; pos < a.nPairs && a.keysSorted[pos] == k; pos += kAccumChunk)
                acc = __dadd_rn(acc, slabSums[static_cast<size_t>(pos / kAccumChunk) * a.D + d]);
            sums[static_cast<size_t>(k) * a.D + d] = acc;
        }
    if (lane == 0) {
        double acc = weights[k];
        for (uint32_t pos = i + kAccumChunk; pos < a.nPairs && a.keysSorted[pos] == k; pos += kAccumChunk)
            acc = __dadd_rn(acc, slabWeights[pos / kAccumChunk]);
        weights[k] = acc;
    }
}

template <int SIDES>
__global__ __launch_bounds__(256) void combinePieces(AccumArgs a) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t i    = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (i >= a.nPairs || i + kAccumChunk >= a.nPairs)
        return;
    const uint32_t k = a.keysSorted[i];
    if (k >= a.nDest || (i > 0 && a.keysSorted[i - 1] == k) || a.keysSorted[i + kAccumChunk] != k)
        return;  // not the head of a destination with a second piece
    if (SIDES == 1 || a.weight[0])
        combineSide(a, a.sums[0], a.weights[0], a.slabSums[0], a.slabWeights[0], i, k, lane);
    if (SIDES == 2 && a.weight[1])
        combineSide(a, a.sums[1], a.weights[1], a.slabSums[1], a.slabWeights[1], i, k, lane);
}

template <int SIDES>
int launchAccumulateSegments(const AccumArgs& a, dim3 grid, hipStream_t stream) {
    switch (a.mode) {
        case kAccumSum: hipLaunchKernelGGL((accumulateSegments<kAccumSum, SIDES>), grid, dim3(256), 0, stream, a); break;
        case kAccumSquare:
            hipLaunchKernelGGL((accumulateSegments<kAccumSquare, SIDES>), grid, dim3(256), 0, stream, a);
            break;
        case kAccumWeightOnly:
            hipLaunchKernelGGL((accumulateSegments<kAccumWeightOnly, SIDES>), grid, dim3(256), 0, stream, a);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dev

int launchResolvePairs(const ResolveArgs& a, ihipStream_t* stream) {
    if (a.nPairs == 0)
        return hipSuccess;
    const dim3 grid((a.nPairs + 255u) / 256u);
    if (a.sides == 2)
        hipLaunchKernelGGL(dev::resolvePairs<2>, grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(dev::resolvePairs<1>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

int launchExpandPosteriorRows(const ExpandArgs& a, ihipStream_t* stream) {
    const uint64_t slots = static_cast<uint64_t>(a.nPairs) * a.rowStride;
    if (slots == 0)
        return hipSuccess;
    hipLaunchKernelGGL(dev::expandPosteriorRows, dim3(static_cast<uint32_t>((slots + 255u) / 256u)), dim3(256), 0, stream,
                       a);
    return hipGetLastError();
}

int accumSortTempBytes(uint32_t nPairs, uint32_t endBit, size_t* bytes) {
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, static_cast<const uint32_t*>(nullptr),
                                     static_cast<uint32_t*>(nullptr), static_cast<const uint32_t*>(nullptr),
                                     static_cast<uint32_t*>(nullptr), nPairs, 0u, endBit, hipStream_t(nullptr));
}

int launchAccumSort(void* temp, size_t tempBytes, const uint32_t* keys, const uint32_t* pairIndex, uint32_t* keysSorted,
                    uint32_t* indexSorted, uint32_t nPairs, uint32_t endBit, ihipStream_t* stream) {
    if (nPairs == 0)
        return hipSuccess;
    // the size this call needs (host arithmetic only): the handle's storage was sized for max_pairs at create
    size_t     need = 0;
    hipError_t e    = static_cast<hipError_t>(accumSortTempBytes(nPairs, endBit, &need));
    if (e != hipSuccess)
        return e;
    if (need > tempBytes || (need && !temp))
        return hipErrorOutOfMemory;
    size_t bytes = tempBytes;
    return rocprim::radix_sort_pairs(temp, bytes, keys, keysSorted, pairIndex, indexSorted, nPairs, 0u, endBit, stream);
}

int launchAccumulateSegments(const AccumArgs& a, ihipStream_t* stream) {
    if (a.nPairs == 0)
        return hipSuccess;
    const dim3 grid((a.nPairs + 3u) / 4u);
    return a.sides == 2 ? dev::launchAccumulateSegments<2>(a, grid, stream) : dev::launchAccumulateSegments<1>(a, grid, stream);
}

int launchCombinePieces(const AccumArgs& a, ihipStream_t* stream) {
    if (a.nPairs <= kAccumChunk)  // no destination has a second piece
        return hipSuccess;
    const dim3 grid((a.nPairs - kAccumChunk + 3u) / 4u);
    if (a.sides == 2)
        hipLaunchKernelGGL(dev::combinePieces<2>, grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(dev::combinePieces<1>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rasr_gmm
