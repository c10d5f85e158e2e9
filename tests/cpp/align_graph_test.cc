// align_graph_test.cc -- host/AlignGraph.cc alone (no GPU, no HIP, no Python): the validation of a batch of alignment
// automata -- the status and the message of every refusal gmm_aligner_set_segments documents, and that a refusal leaves
// the plan it was given untouched -- and the incoming-arc lists in (source state, arc position) order.
// Also built with -fsanitize=address,undefined and run by `make check-align-graph`.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

// Two segments over a table of 10 mixtures.
//   segment 0: 3 states, columns 4..8.  0 -> 1 twice (parallel arcs, mixtures 7 and 2), 0 -> 0, 1 -> 1, 1 -> 2, 2 -> 1 (a
//              back arc), 2 -> 2
//   segment 1: 2 states, columns 0..2, initial state 1.  1 -> 0, 0 -> 0
struct Batch {
    std::vector<uint32_t> stateOffset{0, 3, 5};
    std::vector<uint32_t> arcOffset{0, 3, 5, 7, 8, 9};
    std::vector<uint32_t> arcTarget{1, 0, 1, 1, 2, 1, 2, 0, 0};
    std::vector<uint32_t> arcMixture{7, 0, 2, 1, 3, 4, 5, 9, 8};
    std::vector<float>    arcWeight{0.5f, 1.f, 1.5f, 2.f, 2.5f, 3.f, 3.5f, 4.f, 4.5f};
    std::vector<uint32_t> initial{0, 1};
    std::vector<float>    finalWeight{kInf, kInf, 0.25f, 0.f, kInf};
    std::vector<uint32_t> frameBegin{4, 0};
    std::vector<uint32_t> nFrames{5, 3};
    bool                  withInitial = true;
    gmm_align_graphs graphs() const {
        gmm_align_graphs g{};
        g.n_segments    = static_cast<uint32_t>(frameBegin.size());
        g.state_offset  = stateOffset.data();
        g.arc_offset    = arcOffset.data();
        g.arc_target    = arcTarget.data();
        g.arc_mixture   = arcMixture.data();
        g.arc_weight    = arcWeight.data();
        g.initial_state = withInitial ? initial.data() : nullptr;
        g.final_weight  = finalWeight.data();
        g.frame_begin   = frameBegin.data();
        g.n_frames      = nFrames.data();
        return g;
    }
};

// exactly what the batch needs: 2 segments, 5 states, 9 arcs, 5 * 3 + 3 * 2 = 21 cells
const AlignCapacity kExact{2, 5, 9, 21, 10};

void expect(const Batch& b, const AlignCapacity& cap, int status, const std::string& text) {
    AlignPlan plan;
    plan.nStates = 77;  // a refusal leaves the plan as it was
    std::string            message = "untouched";
    const gmm_align_graphs g       = b.graphs();
    const int              rc      = buildAlignPlan(g, cap, plan, &message);
    CHECK(rc == status);
    if (message != "aligner segments: " + text) {
        std::printf("FAILED: message '%s', expected 'aligner segments: %s'\n", message.c_str(), text.c_str());
        ++failures;
    }
    CHECK(plan.nStates == 77 && plan.segments.empty() && plan.inOffset.empty());
}

}  // namespace

int main() {
    {  // the plan of the good batch
        const Batch            b;
        AlignPlan              p;
        std::string            message;
        const gmm_align_graphs g = b.graphs();
        CHECK(buildAlignPlan(g, kExact, p, &message) == GMM_OK);
        CHECK(message.empty());
        CHECK(p.nStates == 5 && p.nArcs == 9 && p.nCells == 21 && p.maxSegmentStates == 3 && p.frameEnd == 9);
        CHECK(p.segments.size() == 2);
        CHECK(p.segments[0].stateBegin == 0 && p.segments[0].nStates == 3 && p.segments[0].initial == 0 &&
              p.segments[0].frameBegin == 4 && p.segments[0].nFrames == 5 && p.segments[0].cellBegin == 0);
        CHECK(p.segments[1].stateBegin == 3 && p.segments[1].nStates == 2 && p.segments[1].initial == 1 &&
              p.segments[1].frameBegin == 0 && p.segments[1].nFrames == 3 && p.segments[1].cellBegin == 15);
        CHECK((p.order == std::vector<uint32_t>{0, 1}));
        // incoming lists by (source state, arc position): the parallel arcs 0 -> 1 keep their order (arcs 0 and 2),
        // the back arc 2 -> 1 (arc 5) comes after 1 -> 1 (arc 3)
        CHECK((p.inOffset == std::vector<uint32_t>{0, 1, 5, 7, 9, 9}));
        CHECK((p.inArc == std::vector<uint32_t>{1, 0, 2, 3, 5, 4, 6, 7, 8}));
        CHECK((p.inSource == std::vector<uint32_t>{0, 0, 0, 1, 2, 1, 2, 0, 1}));
        CHECK((p.inMixture == std::vector<uint32_t>{0, 7, 2, 1, 4, 3, 5, 9, 8}));
        CHECK((p.inWeight == std::vector<float>{1.f, 0.5f, 1.5f, 2.f, 3.f, 2.5f, 3.5f, 4.f, 4.5f}));
        CHECK(p.finalWeight == b.finalWeight);
    }
    {  // NULL initial states: local state 0; the longer segment goes first
        Batch b;
        b.withInitial = false;
        b.nFrames     = {1, 3};
        b.frameBegin  = {3, 0};  // adjacent ranges are disjoint
        AlignPlan              p;
        std::string            message;
        const gmm_align_graphs g = b.graphs();
        CHECK(buildAlignPlan(g, kExact, p, &message) == GMM_OK);
        CHECK(p.segments[1].initial == 0 && p.nCells == 9 && p.frameEnd == 4);
        CHECK((p.order == std::vector<uint32_t>{1, 0}));
    }
    // ---- refusals ----
    {
        Batch b;
        b.arcTarget[4] = 3;  // segment 0 has states 0..2
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "segment 0: arc 4 has target 3 of 3 states");
        b              = Batch();
        b.arcTarget[8] = 2;  // a valid GLOBAL index is still outside segment 1
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "segment 1: arc 8 has target 2 of 2 states");
    }
    {
        Batch b;
        b.arcMixture[6] = 10;
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "segment 0: arc 6 has mixture 10 of 10");
    }
    {
        Batch b;
        b.frameBegin = {2, 0};  // columns 2..6 and 0..2
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "the frame ranges of segment 1 and segment 0 overlap");
        b.frameBegin = {0, 0};
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "the frame ranges of segment 0 and segment 1 overlap");
    }
    {
        Batch b;
        b.nFrames[1] = 0;
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "segment 1 has no frames");
    }
    {
        Batch b;
        b.frameBegin[0] = 0xfffffffcu;  // 5 frames from here end at 2^32 + 1
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "segment 0: its frame range ends past 2^32");
    }
    {
        Batch b;
        b.initial[1] = 2;
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "segment 1: initial state 2 of 2");
    }
    {
        Batch b;
        b.stateOffset = {0, 5, 5};
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "segment 1 has no states");
        b.stateOffset = {0, 6, 5};
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "state_offset decreases at segment 1");
        b.stateOffset = {1, 3, 5};
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "state_offset[0] is not 0");
    }
    {
        Batch b;
        b.arcOffset = {0, 3, 2, 7, 8, 9};
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "arc_offset decreases at state 1");
        b.arcOffset[0] = 1;
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "arc_offset[0] is not 0");
    }
    {  // every capacity exceeded by one
        const Batch   b;
        AlignCapacity c = kExact;
        c.maxSegments   = 1;
        expect(b, c, GMM_ERR_CAPACITY, "2 segments exceed max_segments 1");
        c           = kExact;
        c.maxStates = 4;
        expect(b, c, GMM_ERR_CAPACITY, "5 states exceed max_states 4");
        c         = kExact;
        c.maxArcs = 8;
        expect(b, c, GMM_ERR_CAPACITY, "9 arcs exceed max_arcs 8");
        c          = kExact;
        c.maxCells = 20;
        expect(b, c, GMM_ERR_CAPACITY, "21 cells (frames x states) exceed max_cells 20");
    }
    {  // one state above the limit is refused, the limit itself is taken: a chain q -> q + 1
        for (uint32_t n : {uint32_t(GMM_ALIGN_MAX_STATES), uint32_t(GMM_ALIGN_MAX_STATES) + 1}) {
            Batch b;
            b.stateOffset = {0, n};
            b.arcOffset.resize(n + 1);
            for (uint32_t q = 0; q <= n; ++q)
                b.arcOffset[q] = q < n ? q : n - 1;
            b.arcTarget.resize(n - 1);
            for (uint32_t q = 0; q + 1 < n; ++q)
                b.arcTarget[q] = q + 1;
            b.arcMixture.assign(n - 1, 0);
            b.arcWeight.assign(n - 1, 0.f);
            b.initial = {0};
            b.finalWeight.assign(n, 0.f);
            b.frameBegin = {0};
            b.nFrames    = {2};
            const AlignCapacity c{1, n, n, 2ull * n, 10};
            if (n == GMM_ALIGN_MAX_STATES) {
                AlignPlan              p;
                std::string            message;
                const gmm_align_graphs g = b.graphs();
                CHECK(buildAlignPlan(g, c, p, &message) == GMM_OK);
                CHECK(p.maxSegmentStates == n && p.inOffset[n] == n - 1 && p.inOffset[1] == 0 && p.inSource[n - 2] == n - 2);
            } else {
                expect(b, c, GMM_ERR_UNSUPPORTED,
                       "segment 0 has " + std::to_string(n) + " states, more than GMM_ALIGN_MAX_STATES " +
                               std::to_string(GMM_ALIGN_MAX_STATES));
            }
        }
    }
    {  // one arc above the in-degree limit: parallel arcs 0 -> 0
        for (uint32_t k : {uint32_t(GMM_ALIGN_MAX_IN_ARCS), uint32_t(GMM_ALIGN_MAX_IN_ARCS) + 1}) {
            Batch b;
            b.stateOffset = {0, 1};
            b.arcOffset   = {0, k};
            b.arcTarget.assign(k, 0);
            b.arcMixture.assign(k, 1);
            b.arcWeight.assign(k, 0.f);
            b.initial     = {0};
            b.finalWeight = {0.f};
            b.frameBegin  = {0};
            b.nFrames     = {1};
            const AlignCapacity c{1, 1, k, 1, 10};
            if (k == GMM_ALIGN_MAX_IN_ARCS) {
                AlignPlan              p;
                std::string            message;
                const gmm_align_graphs g = b.graphs();
                CHECK(buildAlignPlan(g, c, p, &message) == GMM_OK);
                CHECK(p.inArc[k - 1] == k - 1);
            } else {
                expect(b, c, GMM_ERR_UNSUPPORTED,
                       "state 0 is entered by " + std::to_string(k) + " arcs, more than GMM_ALIGN_MAX_IN_ARCS " +
                               std::to_string(GMM_ALIGN_MAX_IN_ARCS));
            }
        }
    }
    {
        Batch b;
        b.frameBegin.clear();
        expect(b, kExact, GMM_ERR_INVALID_ARGUMENT, "no segments");
    }
    if (failures) {
        std::printf("align_graph_test: %d check(s) failed\n", failures);
        return EXIT_FAILURE;
    }
    std::printf("align_graph_test: ok\n");
    return EXIT_SUCCESS;
}
