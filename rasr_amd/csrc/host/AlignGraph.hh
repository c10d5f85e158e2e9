// AlignGraph.hh -- a batch of alignment automata (gmm_align_graphs) validated and turned into what the alignment kernel
// reads: the segment descriptors and the incoming-arc lists per target state, ordered by (source state, arc position).
// Plain C++, no HIP (tests/cpp/align_graph_test.cc runs it alone).
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
};

// GMM_OK, or the status gmm_aligner_set_segments documents with *message set; out is complete or untouched.
int buildAlignPlan(const gmm_align_graphs& g, const AlignCapacity& cap, AlignPlan& out, std::string* message);

}  // namespace rasr_gmm
