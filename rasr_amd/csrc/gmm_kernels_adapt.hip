// gmm_kernels_adapt.hip -- accumulation of aligned (frame, mixture, density, key) pairs into the f64 statistics of
// constrained-MLLR / affine feature transforms, one set of tables per speaker key (gmm_affine_accumulate_*,
// include/rasr_gmm_adaptation.h).
//
// The reference adds one pair at a time into the tables of one key (AffineFeatureTransformAccumulator::accumulate,
// src/Mm/AffineFeatureTransformAccumulator.cc:40-121): per pair D * (D+1)(D+2)/2 f64 divide-multiply-adds for the G
// matrices.  As in gmm_kernels_accum.hip nothing is scattered and no floating-point atomic is used: every cell of a
// table gathers its own contributions in pair order, and the result is the header's numeric contract bit for bit.
//   passes 1-3 and 5: gmm_kernels_keyed.hip (the key of a pair is its speaker key).
//   4. affineAccumulateG / affineAccumulateSmall: a workgroup per (piece, block of 256 cells[, group of kAffineRows
//      G matrices]).  A lane owns one cell: for G the cell (j, k) of the upper triangle, with one running sum per
//      matrix i of its group in registers; for the small tables one cell of beta, mean, cov or k.  The piece's pairs
//      are walked serially, kAffineBatch at a time: the workgroup stages the batch's extended features (widened to
//      f64), variances (means) and weights in LDS, then every lane runs its chain of dependent adds over the batch.
//      Per pair a G lane forms p = xi[j] * xi[k] once and divides it by the kAffineRows variances of its group
//      (broadcast LDS reads).  Piece 0 starts from the table's value and writes it back; a later piece starts from 0
//      and writes its row of the slab (the piece at sorted position i owns slot i / GMM_AFFINE_CHUNK).
// In pooled mode (one covariance) no G work is launched at all.
// Every operation of the contract is an _rn intrinsic and the unit is built with -ffp-contract=off: the correctly
// rounded f64 division expands into fused multiply-adds of its own, the contract's multiplies and adds never fuse.
#include <hip/hip_runtime.h>

#include "gmm_adapt.hh"

namespace rasr_gmm {
namespace dev {

constexpr uint32_t kSmallBatch = 8;  // pairs staged at a time by affineAccumulateSmall (three rows per pair)

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
    double* dst = first ? a.G + (static_cast<size_t>(key) * D) * T : a.slabG + (static_cast<size_t>(i / kPieceChunk) * D) * T;
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
    double* dst = first ? a.small + static_cast<size_t>(key) * S : a.slabSmall + static_cast<size_t>(i / kPieceChunk) * S;
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

}  // namespace dev

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

}  // namespace rasr_gmm
