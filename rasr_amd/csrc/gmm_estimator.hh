// gmm_estimator.hh -- what gmm_estimator.cc (handle, checks, launch sequence), gmm_kernels_accum.hip (the device
// passes) and host/MixtureSetEstimatorFile.cc (the file format) share behind include/rasr_gmm_estimator.h.
// No HIP types here beyond the stream handle's forward declaration: the file-format unit is plain C++.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rasr_gmm_estimator.h"

struct ihipStream_t;

namespace rasr_gmm {

constexpr uint32_t kAccumChunk = GMM_ESTIMATOR_CHUNK;

// slots of the partial slab of a call of nPairs pairs: a later piece (piece >= 1 of its destination) whose first
// contribution sits at sorted position i uses slot i / kAccumChunk, which no other later piece shares
constexpr uint32_t accumSlabSlots(uint32_t nPairs) {
    return nPairs / kAccumChunk + 1;
}

// The device passes add to one or two table sets ("sides") per call.  sides == 1, the maximum-likelihood calls: a NULL
// weight array means every weight is 1 and a NaN weight is a value like any other.  sides == 2, the discriminative
// calls (numerator, denominator): a side's weight array holds NaN where the contribution is not live on that side, and
// a NULL array is a side that receives nothing from the call -- its tables are neither read nor written.

// pass 1: every pair resolved to its mixture entry, mean and covariance; a pair that is skipped gets the three
// sentinel keys (the destination count, which sorts behind every destination) and is counted in *skipped.  With two
// sides a good pair live on neither gets the sentinel keys too and is not counted
struct ResolveArgs {
    const uint32_t* pairFrame;    // [nPairs]
    const uint32_t* pairMix;      // [nPairs]
    const uint32_t* pairDensity;  // [nPairs] in-mixture index, or NULL: 0 (one density per mixture)
    const double*   weight[2];    // [nPairs] or NULL, read with two sides only
    const uint32_t* mixOff;       // [nMix + 1]
    const uint32_t* entryMean;    // [nEntries]
    const uint32_t* entryCov;     // [nEntries]
    uint32_t*       keyMean;      // [nPairs] out
    uint32_t*       keyCov;       // [nPairs] out
    uint32_t*       keyEntry;     // [nPairs] out
    uint32_t*       pairIndex;    // [nPairs] out: 0, 1, ... (the sorts' values)
    unsigned long long* skipped;  // += skipped pairs
    uint32_t        nPairs, nFrames, nMix, nMeans, nCovs, nEntries, sides;
};
int launchResolvePairs(const ResolveArgs& a, ihipStream_t* stream);

// pass 1 of the joint Baum-Welch call: the posterior rows (gmm_density_posteriors_pairs_device's, computed once)
// expanded into contribution slots c = pair * rowStride + j with one finalWeight per side (NaN where not above the
// threshold); a bad pair is counted once.  (The maximum-likelihood call expands in the tail of the posterior kernel.)
struct ExpandArgs {
    const uint32_t* pairFrame;         // [nPairs]
    const uint32_t* pairMix;           // [nPairs]
    const double*   weight[2];         // [nPairs] or NULL
    const float*    posteriors;        // [nPairs][rowStride], or NULL: one density per mixture, posterior 1
    const uint32_t* mixOff;            // [nMix + 1]
    const uint32_t* entryMean;         // [nEntries]
    const uint32_t* entryCov;          // [nEntries]
    uint32_t*       keyMean;           // [nPairs * rowStride] out
    uint32_t*       keyCov;
    uint32_t*       keyEntry;
    uint32_t*       contribIndex;      // out: 0, 1, ...
    uint32_t*       contribFrame;      // out
    double*         contribWeight[2];  // out (written only for a given side)
    unsigned long long* skipped;       // += bad pairs, once each
    double          threshold;
    uint32_t        nPairs, rowStride, nFrames, nMix, nMeans, nCovs, nEntries;
};
int launchExpandPosteriorRows(const ExpandArgs& a, ihipStream_t* stream);

// pass 2: the stable sort of (destination, pair index) by destination over the key bits [0, endBit)
// (the launch* functions and this one return a hipError_t as int: this header names no HIP type)
int accumSortTempBytes(uint32_t nPairs, uint32_t endBit, size_t* bytes);  // temporary storage of such a sort
int launchAccumSort(void* temp, size_t tempBytes, const uint32_t* keys, const uint32_t* pairIndex, uint32_t* keysSorted,
                    uint32_t* indexSorted, uint32_t nPairs, uint32_t endBit, ihipStream_t* stream);

// passes 3 and 4 over one inverted index, one accumulator per destination and side
enum AccumMode : int { kAccumSum = 0, kAccumSquare = 1, kAccumWeightOnly = 2 };
struct AccumArgs {
    const uint32_t* keysSorted;      // [nPairs] destination, ascending; >= nDest: skipped pairs (at the end)
    const uint32_t* indexSorted;     // [nPairs] pair of the contribution, ascending within a destination
    const uint32_t* pairFrame;       // [nPairs]
    const float*    frames;          // [nFrames][frameStride]
    const double*   weight[2];       // [nPairs] per contribution, or NULL (see "sides" above)
    double*         sums[2];         // [nDest][D] (NULL for kAccumWeightOnly)
    double*         weights[2];      // [nDest]
    double*         slabSums[2];     // [accumSlabSlots][D]
    double*         slabWeights[2];  // [accumSlabSlots]
    uint32_t        nPairs, nDest, D, frameStride, sides;
    int             mode;            // AccumMode
};
int launchAccumulateSegments(const AccumArgs& a, ihipStream_t* stream);
int launchCombinePieces(const AccumArgs& a, ihipStream_t* stream);

// ---- the file format (host/MixtureSetEstimatorFile.cc) ----

// an estimator's topology and host copies of its tables
struct EstimatorTables {
    uint32_t        D, nMeans, nCovs, nDens, nMix;
    const uint32_t* dnsMean;  // [nDens]
    const uint32_t* dnsCov;   // [nDens]
    const uint32_t* mixOff;   // [nMix + 1]
    const uint32_t* mixDens;  // [nEntries]
    const double*   meanSums;
    const double*   meanWeights;
    const double*   covSums;
    const double*   covWeights;
    const double*   entryWeights;
};
// AbstractMixtureSetEstimator::write (cc:416-420, 481-509) with MixtureSetEstimatorIndexMap's numbering (cc:804-817)
std::vector<unsigned char> writeEstimatorFile(const EstimatorTables& t);

// the denominator tables (laid out as the numerator's in EstimatorTables) and the objective function
struct DenominatorTables {
    const double* meanSums;
    const double* meanWeights;
    const double* covSums;
    const double* covWeights;
    const double* entryWeights;
    double        objective;
};
// EbwDiscriminativeMixtureSetEstimator::write: writeEstimatorFile's bytes with every mean and covariance followed by
// its denominator accumulator, every mixture's entries by its denominator weights, the objective function last
std::vector<unsigned char> writeDiscriminativeEstimatorFile(const EstimatorTables& t, const DenominatorTables& den);

}  // namespace rasr_gmm
