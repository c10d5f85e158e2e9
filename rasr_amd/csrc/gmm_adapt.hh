// gmm_adapt.hh -- what gmm_adapt.cc (handle, checks, launch sequence) and gmm_kernels_adapt.hip (the device passes)
// share behind include/rasr_gmm_adaptation.h.  No HIP types here beyond the stream handle's forward declaration.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/rasr_gmm_adaptation.h"

struct ihipStream_t;

namespace rasr_gmm {

constexpr uint32_t kAffineChunk  = GMM_AFFINE_CHUNK;
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
// slots of the later pieces' slabs of a call of nPairs pairs: the later piece whose first pair sits at sorted
// position i uses slot i / kAffineChunk, which no other later piece shares (gmm_estimator.hh, accumSlabSlots)
constexpr uint32_t affineSlabSlots(uint32_t nPairs) {
    return nPairs / kAffineChunk + 1;
}
// pieces of a call of nPairs pairs over nKeys keys, at most
constexpr uint32_t affineMaxPieces(uint32_t nPairs, uint32_t nKeys) {
    return nPairs / kAffineChunk + (nKeys < nPairs ? nKeys : nPairs);
}

// pass 1: every pair resolved to its key, mean and covariance; a skipped pair gets the sentinel key nKeys (which
// sorts behind every key) and is counted in *skipped
struct AffineResolveArgs {
    const uint32_t* pairFrame;    // [nPairs]
    const uint32_t* pairMix;      // [nPairs]
    const uint32_t* pairDensity;  // [nPairs] in-mixture index, or NULL: 0
    const uint32_t* pairKey;      // [nPairs] or NULL: 0
    const uint32_t* mixOff;       // [nMix + 1]
    const uint32_t* entryMean;    // [nEntries]
    const uint32_t* entryCov;     // [nEntries]
    uint32_t*       key;          // [nPairs] out
    uint32_t*       mean;         // [nPairs] out
    uint32_t*       cov;          // [nPairs] out
    uint32_t*       pairIndex;    // [nPairs] out: 0, 1, ...
    unsigned long long* skipped;  // += skipped pairs
    uint32_t        nPairs, nFrames, nMix, nKeys;
};
int launchAffineResolve(const AffineResolveArgs& a, ihipStream_t* stream);

// passes 3 to 5 over the sorted pairs (pass 2 is gmm_estimator.hh's launchAccumSort)
struct AffineArgs {
    const uint32_t* keysSorted;   // [nPairs] key, ascending; nKeys: skipped pairs (at the end)
    const uint32_t* indexSorted;  // [nPairs] pair of the sorted position, ascending within a key
    const uint32_t* pairFrame;    // [nPairs]
    const double*   pairWeight;   // [nPairs] or NULL: 1
    const uint32_t* pairMean;     // [nPairs] resolved mean
    const uint32_t* pairCov;      // [nPairs] resolved covariance
    const float*    frames;       // [nFrames][frameStride]
    const float*    means;        // [nMeans][D]
    const float*    variances;    // [nCovs][D]
    // the sorted positions' data, gathered by pass 3
    uint32_t* sFrame;             // [nPairs]
    uint32_t* sMean;              // [nPairs]
    uint32_t* sCov;               // [nPairs]
    double*   sWeight;            // [nPairs]
    uint32_t* pieces;             // [affineMaxPieces] sorted position of every piece's first pair, in any order
    uint32_t* nPieces;            // [1] zeroed before pass 3
    double*   small;              // [nKeys][affineSmallCells]
    double*   G;                  // [nKeys][D][affineTriangle] or NULL (pooled mode)
    double*   slabSmall;          // [affineSlabSlots][affineSmallCells]
    double*   slabG;              // [affineSlabSlots][D][affineTriangle] or NULL
    uint32_t  nPairs, nKeys, D, frameStride, maxPieces;
};
int launchAffineIndexPieces(const AffineArgs& a, ihipStream_t* stream);  // pass 3: gather, list the pieces
int launchAffineAccumulate(const AffineArgs& a, ihipStream_t* stream);   // pass 4: the pieces' ordered sums
int launchAffineCombine(const AffineArgs& a, ihipStream_t* stream);      // pass 5: later pieces added in order

}  // namespace rasr_gmm
