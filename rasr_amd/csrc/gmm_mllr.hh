// gmm_mllr.hh -- what gmm_mllr.cc (handle, checks, launch sequence) and gmm_kernels_mllr.hip (the device passes) share
// behind include/rasr_gmm_mllr.h.  No HIP types here beyond the stream handle's forward declaration.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/rasr_gmm_mllr.h"
#include "gmm_adapt.hh"

struct ihipStream_t;

namespace rasr_gmm {

constexpr uint32_t kMllrChunk = GMM_MLLR_CHUNK;
constexpr uint32_t kMllrBlock = 256;  // lanes of a workgroup = cells it owns
// pass 3 is gmm_adapt.hh's launchAffineIndexPieces with the sets in the place of the keys: the same piece length
static_assert(kMllrChunk == kAffineChunk, "the affine index pass lists pieces of GMM_AFFINE_CHUNK pairs");

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

// pass 1: every pair resolved to its set key * nLeaves + leafOfMixture[mixture], its mean and its covariance; a skipped
// pair gets the sentinel nKeys * nLeaves (which sorts behind every set) and is counted in *skipped
struct MllrResolveArgs {
    const uint32_t* pairFrame;      // [nPairs]
    const uint32_t* pairMix;        // [nPairs]
    const uint32_t* pairDensity;    // [nPairs] in-mixture index, or NULL: 0
    const uint32_t* pairKey;        // [nPairs] or NULL: 0
    const uint32_t* mixOff;         // [nMix + 1]
    const uint32_t* entryMean;      // [nEntries]
    const uint32_t* entryCov;       // [nEntries]
    const uint32_t* leafOfMixture;  // [nMix]
    uint32_t*       set;            // [nPairs] out
    uint32_t*       mean;           // [nPairs] out
    uint32_t*       cov;            // [nPairs] out
    uint32_t*       pairIndex;      // [nPairs] out: 0, 1, ...
    unsigned long long* skipped;    // += skipped pairs
    uint32_t        nPairs, nFrames, nMix, nKeys, nLeaves;
};
int launchMllrResolve(const MllrResolveArgs& a, ihipStream_t* stream);

// passes 4 and 5 over the sorted, gathered pairs (pass 2 is gmm_estimator.hh's launchAccumSort, pass 3
// launchAffineIndexPieces)
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
    double*         slab;        // [affineSlabSlots][layout.cells()]
    MllrLayout      layout;
    uint32_t        nPairs, nSets, frameStride, maxPieces;
};
int launchMllrAccumulate(const MllrArgs& a, ihipStream_t* stream);  // pass 4: the pieces' ordered sums
int launchMllrCombine(const MllrArgs& a, ihipStream_t* stream);     // pass 5: later pieces added in order

}  // namespace rasr_gmm
