// gmm_mllr.hh -- what gmm_mllr.cc (handle, table layout, launch sequence) and gmm_kernels_mllr.hip (pass 4) share
// behind include/rasr_gmm_mllr.h; passes 1-3 and 5 and the piece rule are gmm_pairaccum.hh's.
#pragma once

#include "gmm_pairaccum.hh"

namespace rasr_gmm {

constexpr uint32_t kMllrBlock = 256;  // lanes of a workgroup = cells it owns

// The cells of one (key, leaf) set, one range: full kind Z [D][D+1], G [D+1][D+1], count; then the shift kind's count,
// beta [D], shift [D].  A kind the handle does not hold has no cells.
struct MllrLayout {
    uint32_t D;
    bool     full, shift;
    constexpr size_t zCells() const { return full ? static_cast<size_t>(D) * (D + 1) : 0; }
    constexpr size_t gCells() const { return full ? static_cast<size_t>(D + 1) * (D + 1) : 0; }
    constexpr size_t fullCells() const { return full ? zCells() + gCells() + 1 : 0; }
    constexpr size_t shiftCells() const { return shift ? 1 + 2 * static_cast<size_t>(D) : 0; }
    constexpr size_t cells() const { return fullCells() + shiftCells(); }
    // offsets into the range
    constexpr size_t z() const { return 0; }
    constexpr size_t g() const { return zCells(); }
    constexpr size_t countFull() const { return zCells() + gCells(); }
    constexpr size_t countShift() const { return fullCells(); }
    constexpr size_t beta() const { return fullCells() + 1; }
    constexpr size_t shiftSum() const { return fullCells() + 1 + D; }
    // the staged row of one pair in LDS: m [D+1] (m_0 = 1.0), x [D], and for the shift kind (f64)(x -f32 mu) [D], v [D]
    constexpr uint32_t row() const { return 2 * D + 1 + (shift ? 2 * D : 0); }
};

// pairs staged in LDS at a time: as many as 32 KiB hold, 16 at the most (the batch size decides no bit)
constexpr uint32_t mllrBatch(const MllrLayout& l) {
    const uint32_t fit = (32u * 1024u) / ((l.row() + 1u) * 8u);
    return fit > 16u ? 16u : fit;
}

// pass 4 over the sorted, gathered pairs
struct MllrArgs {
    const uint32_t* setsSorted;  // [nPairs] set, ascending; nSets: skipped pairs (at the end)
    const uint32_t* sFrame;      // [nPairs] the sorted positions' frame, mean, covariance and weight
    const uint32_t* sMean;
    const uint32_t* sCov;
    const double*   sWeight;
    const float*    frames;      // [nFrames][frameStride]
    const float*    means;       // [nMeans][D]
    const float*    variances;   // [nCovs][D]
    const uint32_t* pieces;      // sorted position of every piece's first pair, in any order
    const uint32_t* nPieces;     // [1]
    double*         tables;      // [nSets][layout.cells()]
    double*         slab;        // [pieceSlabSlots][layout.cells()]
    MllrLayout      layout;
    uint32_t        nPairs, nSets, frameStride, maxPieces;
};
int launchMllrAccumulate(const MllrArgs& a, ihipStream_t* stream);  // the pieces' ordered sums

}  // namespace rasr_gmm
