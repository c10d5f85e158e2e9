// AlignGraph.hh -- a batch of alignment automata (gmm_align_graphs) validated and turned into what the alignment kernel
// reads: the segment descriptors and the incoming-arc lists per target state, ordered by (source state, arc position).
// For the Baum-Welch call it also keeps the arcs as given (the backward pass walks a state's outgoing arcs), groups each
// segment's arcs by mixture and lists the segments by table column.
// Plain C++, no HIP (tests/cpp/align_graph_test.cc and tests/cpp/align_posterior_graph_test.cc run it alone).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/rasr_gmm_align.h"

namespace rasr_gmm {

// one segment as the kernel sees it
struct AlignSegment {
    uint32_t stateBegin;  // its first state in the batch's state arrays
    uint32_t nStates;
    uint32_t initial;     // local
    uint32_t frameBegin;  // its first column of the table
    uint32_t nFrames;
    uint32_t pad;
    uint64_t cellBegin;   // its first backpointer cell: cell (t, q) is cellBegin + t * nStates + q
};

struct AlignCapacity {
    uint32_t maxSegments, maxStates, maxArcs;
    uint64_t maxCells;
    uint32_t nMixtures;
};

struct AlignPlan {
    std::vector<AlignSegment> segments;
    std::vector<uint32_t>     order;       // the segments by descending cell count: the workgroups' order
    std::vector<uint32_t>     inOffset;    // [nStates + 1]: the incoming arcs of global state q are inOffset[q] .. [q+1]
    std::vector<uint32_t>     inSource;    // [nArcs] local source state
    std::vector<uint32_t>     inArc;       // [nArcs] the arc's index in the batch's arc arrays
    std::vector<uint32_t>     inMixture;   // [nArcs]
    std::vector<float>        inWeight;    // [nArcs]
    std::vector<float>        finalWeight; // [nStates]
    uint32_t                  nStates = 0, nArcs = 0;
    uint32_t                  maxSegmentStates = 0;  // the largest segment
    uint64_t                  frameEnd = 0;          // the largest frame_begin + n_frames
    uint64_t                  nCells = 0;
    // The Baum-Welch call (gmm_aligner_posteriors_*), built with every plan:
    // the arcs as given, CSR by global source state
    std::vector<uint32_t> arcOffset, arcTarget, arcMixture;
    std::vector<float>    arcWeight;
    // the arcs of every segment grouped by mixture: segment s owns the groups groupOffset[s] .. [s+1], in ascending
    // mixture order; group g is the mixture groupMixture[g] and owns the entries groupArcOffset[g] .. [g+1] of
    // groupSource / groupTarget / groupWeight, which keep the (source state, arc position) order
    std::vector<uint32_t> groupOffset, groupMixture, groupArcOffset, groupSource, groupTarget;
    std::vector<float>    groupWeight;
    uint32_t              maxSegmentGroups = 0;
    // the segments by ascending frame_begin: colSegment[i] is the i-th, its frames are the ordered frames
    // colFrameOffset[i] .. [i+1] (the order of the item list); nFrames in all
    std::vector<uint32_t> colSegment;
    std::vector<uint64_t> colFrameOffset;
    uint64_t              nFrames = 0;
};

// GMM_OK, or the status gmm_aligner_set_segments documents with *message set; out is complete or untouched.
int buildAlignPlan(const gmm_align_graphs& g, const AlignCapacity& cap, AlignPlan& out, std::string* message);

}  // namespace rasr_gmm
