// gmm_align.hh -- what gmm_align.cc (the handle behind include/rasr_gmm_align.h) and the two kernel units
// (gmm_kernels_align.hip, gmm_kernels_align_posterior.hip) share: the constants and the argument structs.  Both modes'
// arguments are the batch, the table and the search part below plus what the mode adds.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "host/AlignGraph.hh"

namespace rasr_gmm {

// a segment of at most kAlignWaveStates states is aligned by ONE wave, with no workgroup barrier in the frame step
// (two states per lane at most); a larger one by the whole workgroup of kAlignThreads lanes, which loops over its
// states above kAlignThreads
constexpr uint32_t kAlignThreads    = 256;
constexpr uint32_t kAlignWaveStates = 128;
// LDS of a workgroup: two f32 score rows and two rows of active marks, a byte each (GMM_ALIGN_MAX_STATES)
constexpr uint32_t kAlignLdsBytesPerState = 2 * (sizeof(float) + 1);
static_assert(GMM_ALIGN_MAX_STATES * kAlignLdsBytesPerState <= 60 * 1024, "the rows of the largest segment fit in LDS");
static_assert(GMM_ALIGN_MAX_STATES <= 0x10000 && GMM_ALIGN_MAX_IN_ARCS <= 0xffff,
              "a backpointer packs (ordinal in the incoming list, source state) into 16 + 16 bits");

// the batch (AlignPlan, uploaded by gmm_aligner_set_segments)
struct AlignBatch {
    const AlignSegment* segments;
    const uint32_t*     order;  // workgroup b aligns segment order[b]
    const uint32_t *    inOffset, *inSource, *inArc, *inMixture;
    const float *       inWeight, *finalWeight;
    uint32_t            nSegments;
    uint32_t            rowStates;  // the LDS rows' length: the largest segment's states, rounded up to 64
};

// the score table of a call
struct AlignTable {
    const float* scores;  // [nMixtures][scoreStride]
    uint32_t     scoreStride, nTableFrames;
};

// gmm_align_search as the kernels read it
struct AlignSearch {
    float    minPruning, maxPruning, factor;
    double   minAverage;
    uint32_t untilNoDifference, nBest;
};

// The search part of a call (gmm_aligner_*_search_*): off in the fixed-threshold calls, whose kernels read none of it.
// With it on the kernels ignore the call's `pruning`
struct AlignSearchCall {
    AlignSearch rule;
    float*      outThreshold;   // [nSegments] or NULL
    uint32_t*   outIterations;  // [nSegments] or NULL
    uint32_t    on;
};

// The Viterbi call (gmm_kernels_align.hip)
struct AlignArgs : AlignBatch, AlignTable {
    float           pruning;
    uint32_t*       cells;  // the backpointers: (ordinal << 16) | source state per (frame, state) cell
    uint32_t *      outMixture, *outState, *outArc;  // [table columns] or NULL
    float*          outScore;                        // [nSegments] or NULL
    uint32_t*       outHypotheses;                   // [nSegments] or NULL
    AlignSearchCall search;
};

// the kernel with or without the retry loop and the n-best step, as a.search.on says
hipError_t launchAlign(const AlignArgs& a, hipStream_t stream);

// The Baum-Welch call (gmm_kernels_align_posterior.hip).  LDS of a segment's workgroup: two f64 potential rows, two f32
// score rows and two rows of active marks (GMM_ALIGN_MAX_STATES_POSTERIOR); the rows are rounded up to 64 states
constexpr uint32_t kAlignPosteriorLdsBytesPerState = 2 * (sizeof(double) + sizeof(float) + 1);
static_assert(((GMM_ALIGN_MAX_STATES_POSTERIOR + 63u) & ~63u) * kAlignPosteriorLdsBytesPerState <= 63 * 1024,
              "the rows of the largest segment fit in LDS beside the reductions");
static_assert(GMM_ALIGN_MAX_STATES_POSTERIOR <= GMM_ALIGN_MAX_STATES, "set_segments accepts what the posterior call does");
// the item passes run one wave per frame, kAlignItemWaves of them at most; each has a row of the weight scratch
constexpr uint32_t kAlignItemWaves = 1024;

struct AlignPosteriorArgs : AlignBatch, AlignTable {
    // the batch's tables of this mode
    const uint32_t *arcOffset, *arcTarget, *arcMixture;  // the arcs as given: CSR by global source state
    const float*    arcWeight;
    const uint32_t *groupOffset, *groupMixture, *groupArcOffset, *groupSource, *groupTarget;
    const float*    groupWeight;
    const uint32_t *colSegment, *colFrameOffset;  // the segments by table column, their ordered frames
    // the call
    float    pruning, minPosterior;
    uint32_t maxItems;
    // the scratch: per (frame, state) cell the forward and backward potentials and the active mark; per segment
    // -bw[initial] and whether it has an alignment; per ordered frame the minimum, the inverse sum and the item count
    // (then offset); per item wave a row of rowGroups weights
    double * fwPot, *bwPot;
    uint8_t* mark;
    double*  segTotalInv;
    uint32_t* segHas;
    float *   frameMin, *frameInv;
    uint32_t* frameCount;  // [nFrames + 1]
    float*    waveWeights;
    uint32_t  rowGroups;
    // the outputs
    uint32_t *outItemFrame, *outItemMixture;
    double*   outItemWeight;
    uint32_t *outColumnOffset, *outNItems;
    float*    outScore;
    uint32_t* outHypotheses;
    double*   outLogTotal;
    uint32_t  nFrames;
    AlignSearchCall search;
};

// the sweep with or without the retry loop and the n-best step, as a.search.on says, then the item launches
hipError_t launchAlignPosteriors(const AlignPosteriorArgs& a, hipStream_t stream);

}  // namespace rasr_gmm
