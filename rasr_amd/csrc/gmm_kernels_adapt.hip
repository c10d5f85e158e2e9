// gmm_kernels_adapt.hip -- accumulation of aligned (frame, mixture, density, key) pairs into the f64 statistics of
// constrained-MLLR / affine feature transforms, one set of tables per speaker key (gmm_affine_accumulate_*,
// include/rasr_gmm_adaptation.h).
//
// The reference adds one pair at a time into the tables of one key (AffineFeatureTransformAccumulator::accumulate,
// src/Mm/AffineFeatureTransformAccumulator.cc:40-121): per pair D * (D+1)(D+2)/2 f64 divide-multiply-adds for the G
// matrices.  As in gmm_kernels_accum.hip nothing is scattered and no floating-point atomic is used: every cell of a
// table gathers its own contributions in pair order, and the result is the header's numeric contract bit for bit.
//   1. affineResolve: a pair -> its key, mean and covariance; a pair that is out of range in any way gets the
//      sentinel key (the key count) and is counted with an integer atomic.  Its frame is never read.
//   2. one stable radix sort of (key, pair index) by key (launchAccumSort of gmm_kernels_accum.hip): per key the
//      list of its pairs, in pair order; the sentinel keys sort behind them.
//   3. affineIndexPieces: the sorted positions' frame, mean, covariance and weight gathered into contiguous arrays,
//      and the first position of every piece of GMM_AFFINE_CHUNK pairs of a key appended to a list (an integer
//      atomic counter: the list's order is arbitrary and decides nothing, every piece has its own destination).
//   4. affineAccumulateG / affineAccumulateSmall: a workgroup per (piece, block of 256 cells[, group of kAffineRows
//      G matrices]).  A lane owns one cell: for G the cell (j, k) of the upper triangle, with one running sum per
//      matrix i of its group in registers; for the small tables one cell of beta, mean, cov or k.  The piece's pairs
//      are walked serially, kAffineBatch at a time: the workgroup stages the batch's extended features (widened to
//      f64), variances (means) and weights in LDS, then every lane runs its chain of dependent adds over the batch.
//      Per pair a G lane forms p = xi[j] * xi[k] once and divides it by the kAffineRows variances of its group
//      (broadcast LDS reads).  Piece 0 starts from the table's value and writes it back; a later piece starts from 0
//      and writes its row of the slab (the piece at sorted position i owns slot i / GMM_AFFINE_CHUNK).
//   5. affineCombine: a key with more than one piece adds its slab rows to the table in piece order.
// In pooled mode (one covariance) no G work is launched at all.
// Every operation of the contract is an _rn intrinsic and the unit is built with -ffp-contract=off: the correctly
// rounded f64 division expands into fused multiply-adds of its own, the contract's multiplies and adds never fuse.
#include <hip/hip_runtime.h>

#include "gmm_adapt.hh"

namespace rasr_gmm {
namespace dev {

constexpr uint32_t kSmallBatch = 8;  // pairs staged at a time by affineAccumulateSmall (three rows per pair)

__global__ __launch_bounds__(256) void affineResolve(AffineResolveArgs a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.nPairs)
        return;
    const uint32_t f = a.pairFrame[p], m = a.pairMix[p];
    const uint32_t key = a.pairKey ? a.pairKey[p] : 0u;
    uint32_t       kk = a.nKeys, km = 0, kc = 0;  // skipped
    bool           ok = f < a.nFrames && m < a.nMix && key < a.nKeys;
    if (ok) {
        const uint32_t e0 = a.mixOff[m], e1 = a.mixOff[m + 1];
        const uint32_t d  = a.pairDensity ? a.pairDensity[p] : 0u;  // 0xffffffff (no best density) is out of range
        ok                = d < e1 - e0;
        if (ok) {
            kk = key;
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

// pairs of the piece that starts at sorted position i with key k: the positions [i, i + n) hold k, n <= kAffineChunk
__device__ __forceinline__ uint32_t pieceLength(const uint32_t* keys, uint32_t i, uint32_t k, uint32_t nPairs) {
    uint32_t lo = i + 1, hi = min(i + kAffineChunk, nPairs);  // the first position past i whose key is not k
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] == k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - i;
}

__global__ __launch_bounds__(256) void affineIndexPieces(AffineArgs a) {
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
    if ((j - s) % kAffineChunk == 0) {
        const uint32_t slot = atomicAdd(a.nPieces, 1u);
        if (slot < a.maxPieces)
            a.pieces[slot] = j;
    }
}

// cell c of the upper triangle of a (D+1) x (D+1) matrix, rows first: (j, k), j <= k
__device__ __forceinline__ void triangleCell(uint32_t c, uint32_t D, uint32_t& j, uint32_t& k) {
    uint32_t row = 0, len = D + 1;
    while (c >= len) {
        c -= len;
        --len;
        ++row;
    }
    j = row;
    k = row + c;
}

// grid: x the piece, y the block of cells of the triangle, z the group of kAffineRows matrices.
// LDS: xi [kAffineBatch][D+1], v [kAffineBatch][kAffineRows], w [kAffineBatch]
__global__ __launch_bounds__(256) void affineAccumulateG(AffineArgs a) {
    extern __shared__ double lds[];
    if (blockIdx.x >= min(*a.nPieces, a.maxPieces))
        return;
    const uint32_t D = a.D, D1 = D + 1;
    const size_t   T = affineTriangle(D);
    double*        sXi = lds;
    double*        sV  = sXi + kAffineBatch * D1;
    double*        sW  = sV + kAffineBatch * kAffineRows;
    const uint32_t i   = a.pieces[blockIdx.x];
    const uint32_t key = a.keysSorted[i];
    const bool     first = i == 0 || a.keysSorted[i - 1] != key;
    const uint32_t n   = pieceLength(a.keysSorted, i, key, a.nPairs);
    const uint32_t r0  = blockIdx.z * kAffineRows;  // first matrix of the group
    const size_t   c   = static_cast<size_t>(blockIdx.y) * kAffineBlock + threadIdx.x;
    const bool     act = c < T;
    uint32_t       cj = 0, ck = 0;
    if (act)
        triangleCell(static_cast<uint32_t>(c), D, cj, ck);
    double* dst = first ? a.G + (static_cast<size_t>(key) * D) * T : a.slabG + (static_cast<size_t>(i / kAffineChunk) * D) * T;
    double  acc[kAffineRows];
#pragma unroll
    for (uint32_t u = 0; u < kAffineRows; ++u)
        acc[u] = first && act && r0 + u < D ? dst[static_cast<size_t>(r0 + u) * T + c] : 0.0;

    for (uint32_t b0 = 0; b0 < n; b0 += kAffineBatch) {
        const uint32_t nb = min(kAffineBatch, n - b0);
        __syncthreads();  // the previous batch has been read
        for (uint32_t x = threadIdx.x; x < nb * D1; x += kAffineBlock) {
            const uint32_t b = x / D1, j = x - b * D1;
            const uint32_t f = a.sFrame[i + b0 + b];
            sXi[x] = j == 0 ? 1.0 : static_cast<double>(a.frames[static_cast<size_t>(f) * a.frameStride + (j - 1)]);
        }
        for (uint32_t x = threadIdx.x; x < nb * kAffineRows; x += kAffineBlock) {
            const uint32_t b = x / kAffineRows, u = x % kAffineRows;
            const uint32_t cv = a.sCov[i + b0 + b];
            sV[x] = r0 + u < D ? static_cast<double>(a.variances[static_cast<size_t>(cv) * D + r0 + u]) : 1.0;
        }
        if (threadIdx.x < nb)
            sW[threadIdx.x] = a.sWeight[i + b0 + threadIdx.x];
        __syncthreads();
        for (uint32_t b = 0; b < nb; ++b) {
            const double p = __dmul_rn(sXi[b * D1 + cj], sXi[b * D1 + ck]);
            const double w = sW[b];
#pragma unroll
            for (uint32_t u = 0; u < kAffineRows; ++u)
                acc[u] = __dadd_rn(acc[u], __dmul_rn(__ddiv_rn(p, sV[b * kAffineRows + u]), w));
        }
    }
    if (act) {
#pragma unroll
        for (uint32_t u = 0; u < kAffineRows; ++u)
            if (r0 + u < D)
                dst[static_cast<size_t>(r0 + u) * T + c] = acc[u];
    }
}

// grid: x the piece, y the block of cells of the small tables.
// LDS: xi [kSmallBatch][D+1], mu [kSmallBatch][D], v [kSmallBatch][D], w [kSmallBatch]
__global__ __launch_bounds__(256) void affineAccumulateSmall(AffineArgs a) {
    extern __shared__ double lds[];
    if (blockIdx.x >= min(*a.nPieces, a.maxPieces))
        return;
    const uint32_t D = a.D, D1 = D + 1;
    const size_t   T = affineTriangle(D), S = affineSmallCells(D);
    double*        sXi = lds;
    double*        sMu = sXi + kSmallBatch * D1;
    double*        sV  = sMu + kSmallBatch * D;
    double*        sW  = sV + kSmallBatch * D;
    const uint32_t i   = a.pieces[blockIdx.x];
    const uint32_t key = a.keysSorted[i];
    const bool     first = i == 0 || a.keysSorted[i - 1] != key;
    const uint32_t n   = pieceLength(a.keysSorted, i, key, a.nPairs);
    const size_t   c   = static_cast<size_t>(blockIdx.y) * kAffineBlock + threadIdx.x;
    const bool     act = c < S;
    // the cell's term of a pair is (A * B) * w with A = xi[ja] (k cells: mu[ri] / v[ri]) and B = xi[jb]:
    // beta 1 * 1, mean[j] xi[j] * 1, cov[j][k] xi[j] * xi[k], k[i][j] (mu[i] / v[i]) * xi[j] -- a product with the
    // 1.0 of xi[0] is exact, so these are the contract's operations
    uint32_t ja = 0, jb = 0, ri = 0;
    bool     isK = false;
    if (act && c >= 1) {
        if (c < 1 + D1)
            ja = static_cast<uint32_t>(c - 1);
        else if (c < 1 + D1 + T)
            triangleCell(static_cast<uint32_t>(c - 1 - D1), D, ja, jb);
        else {
            const uint32_t r = static_cast<uint32_t>(c - 1 - D1 - T);
            isK = true;
            ri  = r / D1;
            jb  = r - ri * D1;
        }
    }
    double* dst = first ? a.small + static_cast<size_t>(key) * S : a.slabSmall + static_cast<size_t>(i / kAffineChunk) * S;
    double  acc = first && act ? dst[c] : 0.0;

    for (uint32_t b0 = 0; b0 < n; b0 += kSmallBatch) {
        const uint32_t nb = min(kSmallBatch, n - b0);
        __syncthreads();
        for (uint32_t x = threadIdx.x; x < nb * D1; x += kAffineBlock) {
            const uint32_t b = x / D1, j = x - b * D1;
            const uint32_t f = a.sFrame[i + b0 + b];
            sXi[x] = j == 0 ? 1.0 : static_cast<double>(a.frames[static_cast<size_t>(f) * a.frameStride + (j - 1)]);
        }
        for (uint32_t x = threadIdx.x; x < nb * D; x += kAffineBlock) {
            const uint32_t b = x / D, d = x - b * D;
            sMu[x] = static_cast<double>(a.means[static_cast<size_t>(a.sMean[i + b0 + b]) * D + d]);
            sV[x]  = static_cast<double>(a.variances[static_cast<size_t>(a.sCov[i + b0 + b]) * D + d]);
        }
        if (threadIdx.x < nb)
            sW[threadIdx.x] = a.sWeight[i + b0 + threadIdx.x];
        __syncthreads();
        for (uint32_t b = 0; b < nb; ++b) {
            const double A = isK ? __ddiv_rn(sMu[b * D + ri], sV[b * D + ri]) : sXi[b * D1 + ja];
            acc            = __dadd_rn(acc, __dmul_rn(__dmul_rn(A, sXi[b * D1 + jb]), sW[b]));
        }
    }
    if (act)
        dst[c] = acc;
}

// grid: x the piece, y the block of cells; table [nKeys][cells], slab [slots][cells]
__global__ __launch_bounds__(256) void affineCombine(AffineArgs a, double* table, const double* slab, size_t cells) {
    if (blockIdx.x >= min(*a.nPieces, a.maxPieces))
        return;
    const uint32_t i = a.pieces[blockIdx.x];
    if (i + kAffineChunk >= a.nPairs)
        return;
    const uint32_t key = a.keysSorted[i];
    if ((i > 0 && a.keysSorted[i - 1] == key) || a.keysSorted[i + kAffineChunk] != key)
        return;  // not the first piece of a key with a second piece
    const size_t c = static_cast<size_t>(blockIdx.y) * kAffineBlock + threadIdx.x;
    if (c >= cells)
        return;
    double acc = table[static_cast<size_t>(key) * cells + c];
    for (uint32_t pos = i + kAffineChunk; pos < a.nPairs && a.keysSorted[pos] == key; pos += kAffineChunk)
        acc = __dadd_rn(acc, slab[static_cast<size_t>(pos / kAffineChunk) * cells + c]);
    table[static_cast<size_t>(key) * cells + c] = acc;
}

}  // namespace dev

int launchAffineResolve(const AffineResolveArgs& a, ihipStream_t* stream) {
    if (a.nPairs == 0)
        return hipSuccess;
    hipLaunchKernelGGL(dev::affineResolve, dim3((a.nPairs + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

int launchAffineIndexPieces(const AffineArgs& a, ihipStream_t* stream) {
    if (a.nPairs == 0)
        return hipSuccess;
    const hipError_t e = hipMemsetAsync(a.nPieces, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(dev::affineIndexPieces, dim3((a.nPairs + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

int launchAffineAccumulate(const AffineArgs& a, ihipStream_t* stream) {
    if (a.nPairs == 0 || a.maxPieces == 0)
        return hipSuccess;
    const uint32_t D = a.D, D1 = D + 1;
    const size_t   T = affineTriangle(D), S = affineSmallCells(D);
    const size_t   smallLds = (static_cast<size_t>(dev::kSmallBatch) * (D1 + 2 * D + 1)) * sizeof(double);
    hipLaunchKernelGGL(dev::affineAccumulateSmall,
                       dim3(a.maxPieces, static_cast<uint32_t>((S + kAffineBlock - 1) / kAffineBlock)), dim3(kAffineBlock),
                       smallLds, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.G)
        return e;
    const size_t gLds = (static_cast<size_t>(kAffineBatch) * (D1 + kAffineRows + 1)) * sizeof(double);
    hipLaunchKernelGGL(dev::affineAccumulateG,
                       dim3(a.maxPieces, static_cast<uint32_t>((T + kAffineBlock - 1) / kAffineBlock),
                            (D + kAffineRows - 1) / kAffineRows),
                       dim3(kAffineBlock), gLds, stream, a);
    return hipGetLastError();
}

int launchAffineCombine(const AffineArgs& a, ihipStream_t* stream) {
    if (a.nPairs <= kAffineChunk)  // no key has a second piece
        return hipSuccess;
    const size_t S = affineSmallCells(a.D), GT = static_cast<size_t>(a.D) * affineTriangle(a.D);
    hipLaunchKernelGGL(dev::affineCombine, dim3(a.maxPieces, static_cast<uint32_t>((S + kAffineBlock - 1) / kAffineBlock)),
                       dim3(kAffineBlock), 0, stream, a, a.small, a.slabSmall, S);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.G)
        return e;
    hipLaunchKernelGGL(dev::affineCombine, dim3(a.maxPieces, static_cast<uint32_t>((GT + kAffineBlock - 1) / kAffineBlock)),
                       dim3(kAffineBlock), 0, stream, a, a.G, a.slabG, GT);
    return hipGetLastError();
}

}  // namespace rasr_gmm
