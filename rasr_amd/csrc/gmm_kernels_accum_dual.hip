// gmm_kernels_accum_dual.hip -- joint numerator / denominator accumulation for discriminative (EBW) training
// (gmm_estimator_accumulate_discriminative_*, include/rasr_gmm_estimator.h).
//
// A lattice gives one (frame, mixture) pair a numerator weight and a denominator weight.  The passes are those of
// gmm_kernels_accum.hip, run ONCE for both sides: the keys of a contribution do not depend on the side, so there is
// one resolve, one set of three stable sorts (that file's launchAccumSort) and one read of every frame row; what is
// doubled is the per-lane accumulator, (accN, accD) with (wsumN, wsumD): two independent f64 add chains per lane
// where the maximum-likelihood kernel has one.
//   1. resolvePairsDual (Viterbi form) / expandDual (Baum-Welch form, over posterior rows computed once by
//      gmm_kernels_posterior.hip): the three keys of every contribution slot, and per side its weight -- NaN where
//      the slot is not live on that side.  A slot live on neither side takes the sentinel keys, as a skipped pair
//      does, so the call's contribution list is the slots live on at least one side.  A bad pair is counted once.
//   2. the three sorts.
//   3. accumulateSegmentsDual: one wave per (destination, piece of GMM_ESTIMATOR_CHUNK joint contributions), lanes
//      over the dimensions, frames and the two weights handed out by v_readlane.  A side adds a contribution iff
//      its weight is not NaN: the weights are wave-uniform, so the predicate is a scalar branch, and a side that
//      skips a slot adds nothing -- never 0 * x, which is NaN for an infinite x and turns a -0.0 sum into +0.0.
//   4. combinePiecesDual: the slab rows of later pieces added in piece order, per side.
// A side whose weight array is NULL takes no part: its tables are neither read nor written.
// Every f64 operation is one __dmul_rn / __dadd_rn; the unit is built with -ffp-contract=off.  No float atomics.
#include <hip/hip_runtime.h>

#include "gmm_estimator.hh"

namespace rasr_gmm {
namespace dev {
namespace {

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

}  // namespace

__global__ __launch_bounds__(256) void resolvePairsDual(DualResolveArgs q) {
    const ResolveArgs& a = q.r;
    const uint32_t     p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.nPairs)
        return;
    const uint32_t f = a.pairFrame[p], m = a.pairMix[p];
    uint32_t       km = a.nMeans, kc = a.nCovs, ke = a.nEntries;  // skipped, or live on neither side
    bool           ok = f < a.nFrames && m < a.nMix;
    if (ok) {
        const uint32_t e0 = a.mixOff[m], e1 = a.mixOff[m + 1];
        const uint32_t d  = a.pairDensity ? a.pairDensity[p] : 0u;  // 0xffffffff (no best density) is out of range
        ok                = d < e1 - e0;
        if (ok) {
            const double wn   = q.weightNum ? q.weightNum[p] : notLive();
            const double wd   = q.weightDen ? q.weightDen[p] : notLive();
            const bool   live = wn == wn || wd == wd;
            if (live) {
                ke = e0 + d;
                km = a.entryMean[ke];
                kc = a.entryCov[ke];
            }
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
__global__ __launch_bounds__(256) void expandDual(DualExpandArgs q) {
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
        if (q.weightNum) {
            const double fw = __dmul_rn(q.weightNum[p], post);
            if (fw > q.threshold)
                fn = fw;
        }
        if (q.weightDen) {
            const double fw = __dmul_rn(q.weightDen[p], post);
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
    if (q.weightNum)
        q.contribWeightNum[c] = fn;
    if (q.weightDen)
        q.contribWeightDen[c] = fd;
    if (j == 0 && n == 0)
        atomicAdd(q.skipped, 1ull);
}

template <int MODE>
__global__ __launch_bounds__(256) void accumulateSegmentsDual(DualAccumArgs a) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t i    = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));  // sorted position
    if (i >= a.nPairs)
        return;
    const uint32_t k = a.keysSorted[i];
    if (k >= a.nDest)  // a skipped pair, or a slot live on neither side
        return;
    uint32_t s = i;
    if (i > 0 && a.keysSorted[i - 1] == k)
        s = runStart(a.keysSorted, i, k);
    if ((i - s) % kAccumChunk != 0)  // not the head of a piece
        return;
    const bool     first = i == s;
    const bool     sideN = a.weight[0] != nullptr, sideD = a.weight[1] != nullptr;
    const uint32_t limit = min(i + kAccumChunk, a.nPairs);
    double         wsumN = first && sideN ? a.weights[0][k] : 0.0;
    double         wsumD = first && sideD ? a.weights[1][k] : 0.0;
    for (uint32_t d0 = 0; d0 == 0 || d0 < a.D; d0 += kWave) {
        const uint32_t d    = d0 + lane;
        const bool     act  = MODE != kAccumWeightOnly && d < a.D;
        double         accN = 0.0, accD = 0.0;
        if (act && first) {
            if (sideN)
                accN = a.sums[0][static_cast<size_t>(k) * a.D + d];
            if (sideD)
                accD = a.sums[1][static_cast<size_t>(k) * a.D + d];
        }
        for (uint32_t b = i; b < limit; b += kWave) {
            // this lane's contribution of the block: its slot's frame and the two weights
            const uint32_t j  = b + lane;
            uint32_t       fj = 0;
            double         wNj = notLive(), wDj = notLive();
            bool           in = false;
            if (j < limit && a.keysSorted[j] == k) {
                in               = true;
                const uint32_t p = a.indexSorted[j];
                fj               = a.pairFrame[p];
                if (sideN)
                    wNj = a.weight[0][p];
                if (sideD)
                    wDj = a.weight[1][p];
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
                        const double wN = readLane(wNj, c0 + u), wD = readLane(wDj, c0 + u);
                        const double xd = static_cast<double>(x[u]);
                        if (wN == wN) {  // wave-uniform: live on the numerator
                            if (act) {
                                const double wx = __dmul_rn(wN, xd);
                                accN = MODE == kAccumSquare ? __dadd_rn(accN, __dmul_rn(wx, xd)) : __dadd_rn(accN, wx);
                            }
                            if (d0 == 0)
                                wsumN = __dadd_rn(wsumN, wN);
                        }
                        if (wD == wD) {  // live on the denominator
                            if (act) {
                                const double wx = __dmul_rn(wD, xd);
                                accD = MODE == kAccumSquare ? __dadd_rn(accD, __dmul_rn(wx, xd)) : __dadd_rn(accD, wx);
                            }
                            if (d0 == 0)
                                wsumD = __dadd_rn(wsumD, wD);
                        }
                    }
                }
            }
            if (n < kWave)
                break;
        }
        if (act) {
            const size_t at = first ? static_cast<size_t>(k) * a.D + d : static_cast<size_t>(i / kAccumChunk) * a.D + d;
            if (sideN)
                (first ? a.sums[0] : a.slabSums[0])[at] = accN;
            if (sideD)
                (first ? a.sums[1] : a.slabSums[1])[at] = accD;
        }
    }
    if (lane == 0) {
        const uint32_t at = first ? k : i / kAccumChunk;
        if (sideN)
            (first ? a.weights[0] : a.slabWeights[0])[at] = wsumN;
        if (sideD)
            (first ? a.weights[1] : a.slabWeights[1])[at] = wsumD;
    }
}

__global__ __launch_bounds__(256) void combinePiecesDual(DualAccumArgs a) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t i    = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (i >= a.nPairs || i + kAccumChunk >= a.nPairs)
        return;
    const uint32_t k = a.keysSorted[i];
    if (k >= a.nDest || (i > 0 && a.keysSorted[i - 1] == k) || a.keysSorted[i + kAccumChunk] != k)
        return;  // not the head of a destination with a second piece
    for (uint32_t side = 0; side < 2; ++side) {
        if (!a.weight[side])
            continue;
        if (a.mode != kAccumWeightOnly)
            for (uint32_t d = lane; d < a.D; d += kWave) {
                double acc = a.sums[side][static_cast<size_t>(k) * a.D + d];
                for (uint32_t pos = i + kAccumChunk; pos < a.nPairs && a.keysSorted[pos] == k; pos += kAccumChunk)
                    acc = __dadd_rn(acc, a.slabSums[side][static_cast<size_t>(pos / kAccumChunk) * a.D + d]);
                a.sums[side][static_cast<size_t>(k) * a.D + d] = acc;
            }
        if (lane == 0) {
            double acc = a.weights[side][k];
            for (uint32_t pos = i + kAccumChunk; pos < a.nPairs && a.keysSorted[pos] == k; pos += kAccumChunk)
                acc = __dadd_rn(acc, a.slabWeights[side][pos / kAccumChunk]);
            a.weights[side][k] = acc;
        }
    }
}

}  // namespace dev

int launchResolvePairsDual(const DualResolveArgs& a, ihipStream_t* stream) {
    if (a.r.nPairs == 0)
        return hipSuccess;
    hipLaunchKernelGGL(dev::resolvePairsDual, dim3((a.r.nPairs + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

int launchExpandDual(const DualExpandArgs& a, ihipStream_t* stream) {
    const uint64_t slots = static_cast<uint64_t>(a.nPairs) * a.rowStride;
    if (slots == 0)
        return hipSuccess;
    hipLaunchKernelGGL(dev::expandDual, dim3(static_cast<uint32_t>((slots + 255u) / 256u)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

int launchAccumulateSegmentsDual(const DualAccumArgs& a, ihipStream_t* stream) {
    if (a.nPairs == 0)
        return hipSuccess;
    const dim3 grid((a.nPairs + 3u) / 4u);
    switch (a.mode) {
        case kAccumSum: hipLaunchKernelGGL(dev::accumulateSegmentsDual<kAccumSum>, grid, dim3(256), 0, stream, a); break;
        case kAccumSquare:
            hipLaunchKernelGGL(dev::accumulateSegmentsDual<kAccumSquare>, grid, dim3(256), 0, stream, a);
            break;
        case kAccumWeightOnly:
            hipLaunchKernelGGL(dev::accumulateSegmentsDual<kAccumWeightOnly>, grid, dim3(256), 0, stream, a);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

int launchCombinePiecesDual(const DualAccumArgs& a, ihipStream_t* stream) {
    if (a.nPairs <= kAccumChunk)  // no destination has a second piece
        return hipSuccess;
    hipLaunchKernelGGL(dev::combinePiecesDual, dim3((a.nPairs - kAccumChunk + 3u) / 4u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rasr_gmm
