// align_posterior_graph_test.cc -- host/AlignGraph.cc alone (no GPU, no HIP, no Python): what the plan holds for the
// Baum-Welch call -- the arcs as given, each segment's arcs grouped by mixture in ascending mixture order with the
// (source state, arc position) order kept inside a group, and the segments by table column.
// Also built with -fsanitize=address,undefined and run by `make check-align-posterior-graph`.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../rasr_amd/csrc/host/AlignGraph.hh"

using namespace rasr_gmm;

namespace {

int failures = 0;

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

const float kInf = INFINITY;

// Three segments over a table of 10 mixtures.
//   segment 0: 3 states, columns 6..8.  state 0: -> 1 (mixture 7), -> 0 (2), -> 1 (7: a parallel arc of the SAME mixture),
//              -> 1 (2: a parallel arc of another);  state 1: -> 1 (2), -> 2 (7);  state 2: -> 2 (2).
//              Mixture 2 is used by all three states, mixture 7 by two.
//   segment 1: 2 states, columns 0..1, initial state 1.  1 -> 0 (9), 0 -> 0 (8)
//   segment 2: 1 state without arcs, column 3
struct Batch {
    std::vector<uint32_t> stateOffset{0, 3, 5, 6};
    std::vector<uint32_t> arcOffset{0, 4, 6, 7, 8, 9, 9};
    std::vector<uint32_t> arcTarget{1, 0, 1, 1, 1, 2, 2, 0, 0};
    std::vector<uint32_t> arcMixture{7, 2, 7, 2, 2, 7, 2, 8, 9};
    std::vector<float>    arcWeight{0.5f, 1.f, 1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f, 4.5f};
    std::vector<uint32_t> initial{0, 1, 0};
    std::vector<float>    finalWeight{kInf, kInf, 0.25f, 0.f, kInf, 0.f};
    std::vector<uint32_t> frameBegin{6, 0, 3};
    std::vector<uint32_t> nFrames{3, 2, 1};
    gmm_align_graphs graphs() const {
        gmm_align_graphs g{};
        g.n_segments    = static_cast<uint32_t>(frameBegin.size());
        g.state_offset  = stateOffset.data();
        g.arc_offset    = arcOffset.data();
        g.arc_target    = arcTarget.data();
        g.arc_mixture   = arcMixture.data();
        g.arc_weight    = arcWeight.data();
        g.initial_state = initial.data();
        g.final_weight  = finalWeight.data();
        g.frame_begin   = frameBegin.data();
        g.n_frames      = nFrames.data();
        return g;
    }
};

const AlignCapacity kCap{4, 8, 16, 64, 10};

template <class T>
bool same(const std::vector<T>& a, std::initializer_list<T> b) {
    return a == std::vector<T>(b);
}

void testGroups() {
    const Batch b;
    AlignPlan   p;
    std::string message;
    CHECK(buildAlignPlan(b.graphs(), kCap, p, &message) == GMM_OK);
    // the arcs as given
    CHECK(p.arcOffset == b.arcOffset);
    CHECK(p.arcTarget == b.arcTarget);
    CHECK(p.arcMixture == b.arcMixture);
    CHECK(p.arcWeight == b.arcWeight);
    // segment 0: mixtures 2 and 7; segment 1: 8 and 9 (state 0's arc, then state 1's); segment 2: none
    CHECK(same<uint32_t>(p.groupOffset, {0, 2, 4, 4}));
    CHECK(same<uint32_t>(p.groupMixture, {2, 7, 8, 9}));
    CHECK(same<uint32_t>(p.groupArcOffset, {0, 4, 7, 8, 9}));
    CHECK(p.maxSegmentGroups == 2);
    // mixture 2 of segment 0: the arcs 1, 3 (state 0, in position order), 4 (state 1), 6 (state 2) -- several states
    // share the mixture, the parallel arc 0 -> 1 of mixture 2 stands after 0 -> 0;
    // mixture 7: the arcs 0, 2 (the two parallel arcs of one mixture, in position order), 5
    CHECK(same<uint32_t>(p.groupSource, {0, 0, 1, 2, 0, 0, 1, 0, 1}));
    CHECK(same<uint32_t>(p.groupTarget, {0, 1, 1, 2, 1, 1, 2, 0, 0}));
    CHECK(same<float>(p.groupWeight, {1.f, 2.f, 2.5f, 3.5f, 0.5f, 1.5f, 3.f, 4.f, 4.5f}));
    // by table column: segment 1 (0..1), segment 2 (3), segment 0 (6..8)
    CHECK(same<uint32_t>(p.colSegment, {1, 2, 0}));
    CHECK(same<uint64_t>(p.colFrameOffset, {0, 2, 3, 6}));
    CHECK(p.nFrames == 6);
}

// every arc is in exactly one group, of its own mixture, and the groups of a segment ascend
void testPartition() {
    const Batch b;
    AlignPlan   p;
    CHECK(buildAlignPlan(b.graphs(), kCap, p, nullptr) == GMM_OK);
    CHECK(p.groupSource.size() == b.arcTarget.size());
    for (size_t s = 0; s + 1 < p.groupOffset.size(); ++s)
        for (uint32_t g = p.groupOffset[s]; g < p.groupOffset[s + 1]; ++g) {
            CHECK(g == p.groupOffset[s] || p.groupMixture[g - 1] < p.groupMixture[g]);
            CHECK(p.groupArcOffset[g] < p.groupArcOffset[g + 1]);
            for (uint32_t k = p.groupArcOffset[g] + 1; k < p.groupArcOffset[g + 1]; ++k)
                CHECK(p.groupSource[k - 1] <= p.groupSource[k]);
        }
}

// no segments: refused, and the plan given keeps what it held
void testEmpty() {
    Batch b;
    AlignPlan   p;
    CHECK(buildAlignPlan(b.graphs(), kCap, p, nullptr) == GMM_OK);
    gmm_align_graphs g = b.graphs();
    g.n_segments       = 0;
    std::string message;
    CHECK(buildAlignPlan(g, kCap, p, &message) == GMM_ERR_INVALID_ARGUMENT);
    CHECK(!message.empty());
    CHECK(p.groupMixture.size() == 4 && p.colSegment.size() == 3);
}

// a batch without any arc: every group list is empty but well formed
void testNoArcs() {
    const std::vector<uint32_t> stateOffset{0, 1}, arcOffset{0, 0}, frameBegin{2}, nFrames{1};
    const std::vector<float>    finalWeight{0.f};
    gmm_align_graphs            g{};
    g.n_segments   = 1;
    g.state_offset = stateOffset.data();
    g.arc_offset   = arcOffset.data();
    g.final_weight = finalWeight.data();
    g.frame_begin  = frameBegin.data();
    g.n_frames     = nFrames.data();
    AlignPlan p;
    CHECK(buildAlignPlan(g, kCap, p, nullptr) == GMM_OK);
    CHECK(same<uint32_t>(p.groupOffset, {0, 0}));
    CHECK(same<uint32_t>(p.groupArcOffset, {0}));
    CHECK(p.groupMixture.empty() && p.groupSource.empty() && p.arcTarget.empty());
    CHECK(same<uint32_t>(p.arcOffset, {0, 0}));
    CHECK(p.maxSegmentGroups == 0 && p.nFrames == 1);
}

}  // namespace

int main() {
    testGroups();
    testPartition();
    testEmpty();
    testNoArcs();
    if (failures) {
        std::printf("align_posterior_graph_test: %d check(s) FAILED\n", failures);
        return 1;
    }
    std::printf("align_posterior_graph_test: all checks passed\n");
    return 0;
}
