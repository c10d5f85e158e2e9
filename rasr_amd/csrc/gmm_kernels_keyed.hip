// gmm_kernels_keyed.hip -- the passes that the keyed accumulations share (gmm_pairaccum.hh): the affine feature
// transform statistics (gmm_kernels_adapt.hip, one table per speaker key) and the MLLR statistics
// (gmm_kernels_mllr.hip, one table per (speaker key, regression leaf)).  Nothing is scattered and no floating-point
// atomic is used: every cell of a table gathers its own contributions in pair order.
//   1. keyedResolve: a pair -> its sort key (key * nLeaves + the leaf of its mixture), mean and covariance; a pair
//      that is out of range in any way gets the sentinel key (the key count) and is counted with an integer atomic.
//      Its frame is never read.
//   2. one stable radix sort of (key, pair index) by key (launchAccumSort of gmm_kernels_accum.hip): per key the
//      list of its pairs, in pair order; the sentinel keys sort behind them.
//   3. indexPieces: the sorted positions' frame, mean, covariance and weight gathered into contiguous arrays, and
//      the first position of every piece of kPieceChunk pairs of a key appended to a list (an integer atomic
//      counter: the list's order is arbitrary and decides nothing, every piece has its own destination).
//   4. the handle's own accumulate kernel: piece 0 of a key starts from the table's value and writes it back; a later
//      piece starts from 0 and writes its row of the slab (the piece at sorted position i owns slot i / kPieceChunk).
//   5. combinePieces: a key with more than one piece adds its slab rows to the table in piece order (_rn adds; the
//      unit is built with -ffp-contract=off like the accumulate kernels' units).
#include <hip/hip_runtime.h>

#include "gmm_pairaccum.hh"

namespace rasr_gmm {
namespace dev {

__global__ __launch_bounds__(256) void keyedResolve(KeyedResolveArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.nPairs)
        return;
    const uint32_t f = a.pairFrame[p], m = a.pairMix[p];
    const uint32_t key = a.pairKey ? a.pairKey[p] : 0u;
    uint32_t       kk = a.nKeys * a.nLeaves, km = 0, kc = 0;  // skipped
    bool           ok = f < a.nFrames && m < a.nMix && key < a.nKeys;
    if (ok) {
        const uint32_t e0 = a.mixOff[m], e1 = a.mixOff[m + 1];
        const uint32_t d  = a.pairDensity ? a.pairDensity[p] : 0u;  // 0xffffffff (no best density) is out of range
        ok                = d < e1 - e0;
        if (ok) {
            kk = key * a.nLeaves + (a.leafOfMixture ? a.leafOfMixture[m] : 0u);
            km = a.entryMean[e0 + d];
            kc = a.entryCov[e0 + d];
        }
    }
    a.key[p]       = kk;
    a.mean[p]      = km;
    a.cov[p]       = kc;
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

__global__ __launch_bounds__(256) void indexPieces(IndexPiecesArgs a) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= a.nPairs)
        return;
    const uint32_t k = a.keysSorted[j];
    if (k >= a.nKeys)  // a skipped pair: none of its data is touched
        return;
    const uint32_t p = a.indexSorted[j];
    a.sFrame[j]      = a.pairFrame[p];
    a.sMean[j]       = a.pairMean[p];
    a.sCov[j]        = a.pairCov[p];
    a.sWeight[j]     = a.pairWeight ? a.pairWeight[p] : 1.0;
    uint32_t s       = j;
    if (j > 0 && a.keysSorted[j - 1] == k)
        s = runStart(a.keysSorted, j, k);
    if ((j - s) % kPieceChunk == 0) {
        const uint32_t slot = atomicAdd(a.nPieces, 1u);
        if (slot < a.maxPieces)
            a.pieces[slot] = j;
    }
}

// grid: x the piece, y the block of cells; table [nKeys][cells], slab [slots][cells]
__global__ __launch_bounds__(256) void combinePieces(const uint32_t* keysSorted, const uint32_t* pieces,
                                                     const uint32_t* nPieces, uint32_t maxPieces, uint32_t nPairs,
                                                     double* table, const double* slab, size_t cells) {
    if (blockIdx.x >= min(*nPieces, maxPieces))
        return;
    const uint32_t i = pieces[blockIdx.x];
    if (i + kPieceChunk >= nPairs)
        return;
    const uint32_t key = keysSorted[i];
    if ((i > 0 && keysSorted[i - 1] == key) || keysSorted[i + kPieceChunk] != key)
        return;  // not the first piece of a key with a second piece
    const size_t c = static_cast<size_t>(blockIdx.y) * kPieceBlock + threadIdx.x;
    if (c >= cells)
        return;
    double acc = table[static_cast<size_t>(key) * cells + c];
    for (uint32_t pos = i + kPieceChunk; pos < nPairs && keysSorted[pos] == key; pos += kPieceChunk)
        acc = __dadd_rn(acc, slab[static_cast<size_t>(pos / kPieceChunk) * cells + c]);
    table[static_cast<size_t>(key) * cells + c] = acc;
}

}  // namespace dev

int launchKeyedResolve(const KeyedResolveArgs& a, ihipStream_t* stream) {
    if (a.nPairs == 0)
        return hipSuccess;
    hipLaunchKernelGGL(dev::keyedResolve, dim3((a.nPairs + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

int launchIndexPieces(const IndexPiecesArgs& a, ihipStream_t* stream) {
    if (a.nPairs == 0)
        return hipSuccess;
    const hipError_t e = hipMemsetAsync(a.nPieces, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::indexPieces, dim3((a.nPairs + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

int launchCombinePieces(const uint32_t* keysSorted, const uint32_t* pieces, const uint32_t* nPieces, uint32_t maxPieces,
                        uint32_t nPairs, double* table, const double* slab, size_t cells, ihipStream_t* stream) {
    if (nPairs <= kPieceChunk)  // no key has a second piece
        return hipSuccess;
    hipLaunchKernelGGL(dev::combinePieces, dim3(maxPieces, static_cast<uint32_t>((cells + kPieceBlock - 1) / kPieceBlock)),
                       dim3(kPieceBlock), 0, stream, keysSorted, pieces, nPieces, maxPieces, nPairs, table, slab, cells);
    return hipGetLastError();
}

}  // namespace rasr_gmm
