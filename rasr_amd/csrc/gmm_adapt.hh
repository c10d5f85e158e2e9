// gmm_adapt.hh -- what gmm_adapt.cc (handle, table layout, launch sequence) and gmm_kernels_adapt.hip (pass 4) share
// behind include/rasr_gmm_adaptation.h; passes 1-3 and 5 and the piece rule are gmm_pairaccum.hh's.
#pragma once

#include "gmm_pairaccum.hh"

namespace rasr_gmm {

constexpr uint32_t kAffineRows   = 8;    // G matrices (rows i of the transform) a lane keeps running sums of
constexpr uint32_t kAffineBlock  = 256;  // lanes of a workgroup = cells it owns
constexpr uint32_t kAffineBatch  = 16;   // pairs staged in LDS at a time

// cells of one (D+1) x (D+1) upper triangle
constexpr size_t affineTriangle(uint32_t D) {
    return static_cast<size_t>(D + 1) * (D + 2) / 2;
}
// the small tables of one key, one cell each: [0] beta, [1, D+2) mean, then cov's triangle, then k [D][D+1]
constexpr size_t affineSmallCells(uint32_t D) {
    return 1 + (D + 1) + affineTriangle(D) + static_cast<size_t>(D) * (D + 1);
}

// pass 4 over the sorted, gathered pairs.  The struct is the accumulate kernels' argument: its layout decides their
// code, so the members that only the index pass read (now gmm_pairaccum.hh's IndexPiecesArgs) keep their places
struct AffineArgs {
    const uint32_t* keysSorted;   // [nPairs] key, ascending; nKeys: skipped pairs (at the end)
    const uint32_t* indexSorted;  // not read
    const uint32_t* pairFrame;    // not read
    const double*   pairWeight;   // not read
    const uint32_t* pairMean;     // not read
    const uint32_t* pairCov;      // not read
    const float*    frames;       // [nFrames][frameStride]
    const float*    means;        // [nMeans][D]
    const float*    variances;    // [nCovs][D]
    // the sorted positions' data, gathered by pass 3
    uint32_t* sFrame;             // [nPairs]
    uint32_t* sMean;              // [nPairs]
    uint32_t* sCov;               // [nPairs]
    double*   sWeight;            // [nPairs]
    uint32_t* pieces;             // [pieceBound] sorted position of every piece's first pair, in any order
    uint32_t* nPieces;            // [1]
    double*   small;              // [nKeys][affineSmallCells]
    double*   G;                  // [nKeys][D][affineTriangle] or NULL (pooled mode)
    double*   slabSmall;          // [pieceSlabSlots][affineSmallCells]
    double*   slabG;              // [pieceSlabSlots][D][affineTriangle] or NULL
    uint32_t  nPairs, nKeys, D, frameStride, maxPieces;
};
int launchAffineAccumulate(const AffineArgs& a, ihipStream_t* stream);  // the pieces' ordered sums

}  // namespace rasr_gmm
