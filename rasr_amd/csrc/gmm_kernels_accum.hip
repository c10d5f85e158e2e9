// gmm_kernels_accum.hip -- maximum-likelihood accumulation of aligned (frame, mixture, density) pairs into the f64
// statistics of a mixture set's means, covariances and mixture entries (gmm_estimator_accumulate_*,
// include/rasr_gmm_estimator.h).
//
// The reference adds one pair at a time (AbstractMixtureEstimator::accumulate -> GaussDensityEstimator::accumulate
// -> VectorAccumulator, plusWeighted / plusSquareWeighted, src/Mm/Utilities.hh:110-146): a scatter-add whose f64
// sums depend on the order of the adds.  Floating-point atomics would make that order the arrival order; this file
// uses the store-and-sum form instead: nothing is scattered, every destination gathers its own contributions in a
// fixed order through an inverted index, and the result is the header's numeric contract bit for bit.
//   1. resolvePairs: a pair -> its mixture entry, mean and covariance (three keys); a pair that is out of range in
//      any way gets the sentinel key (the destination count) and is counted with an integer atomic.  Its frame is
//      never read.
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
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "gmm_estimator.hh"

namespace rasr_gmm {
namespace dev {

constexpr uint32_t kWave      = 64;
constexpr uint32_t kRowsAhead = 16;  // frame rows in flight ahead of the add chain

__device__ __forceinline__ uint32_t readLane(uint32_t v, uint32_t j) {
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(j)));
}
__device__ __forceinline__ double readLane(double v, uint32_t j) {
    const uint64_t b  = static_cast<uint64_t>(__double_as_longlong(v));
    const uint64_t lo = readLane(static_cast<uint32_t>(b), j), hi = readLane(static_cast<uint32_t>(b >> 32), j);
    return __longlong_as_double(static_cast<long long>((hi << 32) | lo));
}

__global__ __launch_bounds__(256) void resolvePairs(ResolveArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.nPairs)
        return;
    const uint32_t f = a.pairFrame[p], m = a.pairMix[p];
    uint32_t       km = a.nMeans, kc = a.nCovs, ke = a.nEntries;  // skipped
    bool           ok = f < a.nFrames && m < a.nMix;
    if (ok) {
        const uint32_t e0 = a.mixOff[m], e1 = a.mixOff[m + 1];
        const uint32_t d  = a.pairDensity ? a.pairDensity[p] : 0u;  // 0xffffffff (no best density) is out of range
        ok                = d < e1 - e0;
        if (ok) {
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

template <int MODE>
__global__ __launch_bounds__(256) void accumulateSegments(AccumArgs a) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t i    = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));  // sorted position
    if (i >= a.nPairs)
        return;
    const uint32_t k = a.keysSorted[i];
    if (k >= a.nDest)  // a skipped pair
        return;
    uint32_t s = i;
    if (i > 0 && a.keysSorted[i - 1] == k)
        s = runStart(a.keysSorted, i, k);
    if ((i - s) % kAccumChunk != 0)  // not the head of a piece
        return;
    const bool     first = i == s;
    const uint32_t limit = min(i + kAccumChunk, a.nPairs);
    double         wsum  = first ? a.weights[k] : 0.0;
    for (uint32_t d0 = 0; d0 == 0 || d0 < a.D; d0 += kWave) {
        const uint32_t d   = d0 + lane;
        const bool     act = MODE != kAccumWeightOnly && d < a.D;
        double         acc = 0.0;
        if (act && first)
            acc = a.sums[static_cast<size_t>(k) * a.D + d];
        for (uint32_t b = i; b < limit; b += kWave) {
            // this lane's contribution of the block: its pair's frame and weight
            const uint32_t j  = b + lane;
            uint32_t       fj = 0;
            double         wj = 1.0;
            bool           in = false;
            if (j < limit && a.keysSorted[j] == k) {
                in               = true;
                const uint32_t p = a.indexSorted[j];
                fj               = a.pairFrame[p];
                if (a.pairWeight)
                    wj = a.pairWeight[p];
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
                        const double w = readLane(wj, c0 + u);
                        if (act) {
                            const double xd = static_cast<double>(x[u]);
                            const double wx = __dmul_rn(w, xd);
                            acc = MODE == kAccumSquare ? __dadd_rn(acc, __dmul_rn(wx, xd)) : __dadd_rn(acc, wx);
                        }
                        if (d0 == 0)
                            wsum = __dadd_rn(wsum, w);
                    }
                }
            }
            if (n < kWave)
                break;
        }
        if (act) {
            if (first)
                a.sums[static_cast<size_t>(k) * a.D + d] = acc;
            else
                a.slabSums[static_cast<size_t>(i / kAccumChunk) * a.D + d] = acc;
        }
    }
    if (lane == 0) {
        if (first)
            a.weights[k] = wsum;
        else
            a.slabWeights[i / kAccumChunk] = wsum;
    }
}

__global__ __launch_bounds__(256) void combinePieces(AccumArgs a) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t i    = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (i >= a.nPairs || i + kAccumChunk >= a.nPairs)
        return;
    const uint32_t k = a.keysSorted[i];
    if (k >= a.nDest || (i > 0 && a.keysSorted[i - 1] == k) || a.keysSorted[i + kAccumChunk] != k)
        return;  // not the head of a destination with a second piece
    if (a.mode != kAccumWeightOnly)
        for (uint32_t d = lane; d < a.D; d += kWave) {
            double acc = a.sums[static_cast<size_t>(k) * a.D + d];
            for (uint32_t pos = i + kAccumChunk; pos < a.nPairs && a.keysSorted[pos] == k; pos += kAccumChunk)
                acc = __dadd_rn(acc, a.slabSums[static_cast<size_t>(pos / kAccumChunk) * a.D + d]);
            a.sums[static_cast<size_t>(k) * a.D + d] = acc;
        }
    if (lane == 0) {
        double acc = a.weights[k];
        for (uint32_t pos = i + kAccumChunk; pos < a.nPairs && a.keysSorted[pos] == k; pos += kAccumChunk)
            acc = __dadd_rn(acc, a.slabWeights[pos / kAccumChunk]);
        a.weights[k] = acc;
    }
}

}  // namespace dev

int launchResolvePairs(const ResolveArgs& a, ihipStream_t* stream) {
    if (a.nPairs == 0)
        return hipSuccess;
    hipLaunchKernelGGL(dev::resolvePairs, dim3((a.nPairs + 255u) / 256u), dim3(256), 0, stream, a);
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
    switch (a.mode) {
        case kAccumSum: hipLaunchKernelGGL(dev::accumulateSegments<kAccumSum>, grid, dim3(256), 0, stream, a); break;
        case kAccumSquare: hipLaunchKernelGGL(dev::accumulateSegments<kAccumSquare>, grid, dim3(256), 0, stream, a); break;
        case kAccumWeightOnly:
            hipLaunchKernelGGL(dev::accumulateSegments<kAccumWeightOnly>, grid, dim3(256), 0, stream, a);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

int launchCombinePieces(const AccumArgs& a, ihipStream_t* stream) {
    if (a.nPairs <= kAccumChunk)  // no destination has a second piece
        return hipSuccess;
    hipLaunchKernelGGL(dev::combinePieces, dim3((a.nPairs - kAccumChunk + 3u) / 4u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rasr_gmm
