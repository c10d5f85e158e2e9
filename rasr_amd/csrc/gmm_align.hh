// gmm_align.hh -- what gmm_align.cc (the handle behind include/rasr_gmm_align.h) and gmm_kernels_align.hip share.
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

struct AlignArgs {
    // the batch (AlignPlan, uploaded by gmm_aligner_set_segments)
    const AlignSegment* segments;
    const uint32_t*     order;  // workgroup b aligns segment order[b]
    const uint32_t *    inOffset, *inSource, *inArc, *inMixture;
    const float *       inWeight, *finalWeight;
    // the call
    const float* scores;  // [nMixtures][scoreStride]
    uint32_t     scoreStride;
    float        pruning;
    uint32_t*    cells;   // the backpointers: (ordinal << 16) | source state per (frame, state) cell
    uint32_t *   outMixture, *outState, *outArc;  // [table columns] or NULL
    float*       outScore;                        // [nSegments] or NULL
    uint32_t*    outHypotheses;                   // [nSegments] or NULL
    uint32_t     nSegments;
    uint32_t     rowStates;  // the LDS rows' length: the largest segment's states, rounded up to 64
};

hipError_t launchAlign(const AlignArgs& a, hipStream_t stream);

}  // namespace rasr_gmm
