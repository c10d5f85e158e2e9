// gmm_kernels_mllr.hip -- accumulation of aligned (frame, mixture, density, key) pairs into the f64 statistics of MLLR
// mean transforms, one set of tables per (speaker key, regression leaf) (gmm_mllr_accumulate_*,
// include/rasr_gmm_mllr.h).
//
// The reference adds one pair at a time into the tables of the leaf of the pair's mixture
// (FullAdaptorViterbiEstimator / ShiftAdaptorViterbiEstimator::accumulate, src/Mm/MllrAdaptation.cc:399-416, 599-653,
// 704-714): per pair D(D+1) + (D+1)^2 f64 multiply-multiply-adds for Z and G, and 2 D divisions for the shift kind.
// As in gmm_kernels_adapt.hip nothing is scattered and no floating-point atomic is used: every cell of a set gathers
// its own contributions in pair order, and the result is the header's numeric contract bit for bit.
//   passes 1-3 and 5: gmm_kernels_keyed.hip (the key of a pair is its set, key * nLeaves + the leaf of its mixture).
//   4. mllrAccumulate: a workgroup per (piece, block of 256 cells of the set's one range, MllrLayout).  A lane owns one
//      cell.  The piece's pairs are walked serially, a batch at a time: the workgroup stages per pair the row
//      m | x | (f64)(x -f32 mu) | v (widened to f64) and the weight in LDS, then every lane runs its chain of dependent
//      adds over the batch, two LDS reads per pair: (w * row[a]) * row[b] for a cell of Z (a: x_i, b: m_j) or G (a:
//      m_i, b: m_j), (w * row[a]) / row[b] for a cell of the shift kind (count: 1.0 and 1.0, which is exact; beta: 1.0
//      and v_d; shift: the difference and v_d), 1.0 for the full kind's count.  Piece 0 starts from the table's value
//      and writes it back; a later piece starts from 0 and writes its row of the slab (the piece at sorted position i
//      owns slot i / GMM_MLLR_CHUNK).
// Every operation of the contract is an _rn intrinsic and the unit is built with -ffp-contract=off: the correctly
// rounded f64 division expands into fused multiply-adds of its own, the contract's multiplies and adds never fuse.
#include <hip/hip_runtime.h>

#include "gmm_mllr.hh"

namespace rasr_gmm {
namespace dev {

enum : uint32_t { kCellMul = 0, kCellDiv = 1, kCellOne = 2 };

// grid: x the piece, y the block of cells of the set.  LDS: row [batch][layout.row()], w [batch]
__global__ __launch_bounds__(256) void mllrAccumulate(MllrArgs a, uint32_t batch) {
    extern __shared__ double lds[];
    if (blockIdx.x >= min(*a.nPieces, a.maxPieces))
        return;
    const MllrLayout L = a.layout;
    const uint32_t   D = L.D, D1 = D + 1, R = L.row();
    const size_t     C = L.cells();
    double*          sRow = lds;
    double*          sW   = sRow + static_cast<size_t>(batch) * R;
    const uint32_t   i    = a.pieces[blockIdx.x];
    const uint32_t   set  = a.setsSorted[i];
    const bool       first = i == 0 || a.setsSorted[i - 1] != set;
    const uint32_t   n    = pieceLength(a.setsSorted, i, set, a.nPairs);
    const size_t     c    = static_cast<size_t>(blockIdx.y) * kMllrBlock + threadIdx.x;
    const bool       act  = c < C;
    // the cell's term of a pair: row offsets ia, ib and the class (header comment, pass 4)
    const uint32_t xOff = D1, diffOff = 2 * D + 1, vOff = 3 * D + 1;
    uint32_t       ia = 0, ib = 0, cls = kCellOne;
    if (act && c < L.countFull()) {
        const bool     isG = c >= L.g();
        const uint32_t r   = static_cast<uint32_t>(isG ? c - L.g() : c);
        const uint32_t ri  = r / D1;
        cls                = kCellMul;
        ia                 = isG ? ri : xOff + ri;
        ib                 = r - ri * D1;
    } else if (act && c >= L.countShift()) {
        const uint32_t s = static_cast<uint32_t>(c - L.countShift());
        cls              = kCellDiv;  // s == 0, the count: (w * 1.0) / 1.0
        if (s >= 1 && s <= D)
            ib = vOff + (s - 1);
        else if (s > D) {
            ia = diffOff + (s - 1 - D);
            ib = vOff + (s - 1 - D);
        }
    }
    double* dst = first ? a.tables + static_cast<size_t>(set) * C : a.slab + static_cast<size_t>(i / kPieceChunk) * C;
    double  acc = first && act ? dst[c] : 0.0;

    for (uint32_t b0 = 0; b0 < n; b0 += batch) {
        const uint32_t nb = min(batch, n - b0);
        __syncthreads();  // the previous batch has been read
        for (uint32_t x = threadIdx.x; x < nb * R; x += kMllrBlock) {
            const uint32_t b = x / R, r = x - b * R;
            const uint32_t p = i + b0 + b;
            double         v;
            if (r < D1) {
                v = r == 0 ? 1.0 : static_cast<double>(a.means[static_cast<size_t>(a.sMean[p]) * D + (r - 1)]);
            } else if (r < diffOff) {
                v = static_cast<double>(a.frames[static_cast<size_t>(a.sFrame[p]) * a.frameStride + (r - xOff)]);
            } else if (r < vOff) {
                const uint32_t d = r - diffOff;
                v = static_cast<double>(__fsub_rn(a.frames[static_cast<size_t>(a.sFrame[p]) * a.frameStride + d],
                                                  a.means[static_cast<size_t>(a.sMean[p]) * D + d]));
            } else {
                v = static_cast<double>(a.variances[static_cast<size_t>(a.sCov[p]) * D + (r - vOff)]);
            }
            sRow[x] = v;
        }
        if (threadIdx.x < nb)
            sW[threadIdx.x] = a.sWeight[i + b0 + threadIdx.x];
        __syncthreads();
        for (uint32_t b = 0; b < nb; ++b) {
            const double* row = sRow + b * R;
            const double  wa  = __dmul_rn(sW[b], row[ia]);
            double        t   = 1.0;
            if (cls == kCellMul)
                t = __dmul_rn(wa, row[ib]);
            else if (cls == kCellDiv)
                t = __ddiv_rn(wa, row[ib]);
            acc = __dadd_rn(acc, t);
        }
    }
    if (act)
        dst[c] = acc;
}

}  // namespace dev

int launchMllrAccumulate(const MllrArgs& a, ihipStream_t* stream) {
    if (a.nPairs == 0 || a.maxPieces == 0)
        return hipSuccess;
    const uint32_t batch = mllrBatch(a.layout);
    const size_t   lds   = static_cast<size_t>(batch) * (a.layout.row() + 1) * sizeof(double);
    const size_t   C     = a.layout.cells();
    hipLaunchKernelGGL(dev::mllrAccumulate, dim3(a.maxPieces, static_cast<uint32_t>((C + kMllrBlock - 1) / kMllrBlock)),
                       dim3(kMllrBlock), lds, stream, a, batch);
    return hipGetLastError();
}

}  // namespace rasr_gmm
