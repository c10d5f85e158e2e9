// AlignGraph.cc -- see AlignGraph.hh.
#include "AlignGraph.hh"

#include <algorithm>
#include <numeric>

namespace rasr_gmm {

namespace {

int refuse(int code, std::string* message, const std::string& text) {
    if (message)
        *message = "aligner segments: " + text;
    return code;
}

std::string seg(uint32_t s) {
    return "segment " + std::to_string(s);
}

}  // namespace

int buildAlignPlan(const gmm_align_graphs& g, const AlignCapacity& cap, AlignPlan& out, std::string* message) {
    const uint32_t S = g.n_segments;
    if (S == 0)
        return refuse(GMM_ERR_INVALID_ARGUMENT, message, "no segments");
    if (!g.state_offset || !g.arc_offset || !g.final_weight || !g.frame_begin || !g.n_frames)
        return refuse(GMM_ERR_INVALID_ARGUMENT, message, "null array");
    if (S > cap.maxSegments)
        return refuse(GMM_ERR_CAPACITY, message,
                      std::to_string(S) + " segments exceed max_segments " + std::to_string(cap.maxSegments));
    if (g.state_offset[0] != 0)
        return refuse(GMM_ERR_INVALID_ARGUMENT, message, "state_offset[0] is not 0");
    for (uint32_t s = 0; s < S; ++s) {
        if (g.state_offset[s + 1] < g.state_offset[s])
            return refuse(GMM_ERR_INVALID_ARGUMENT, message, "state_offset decreases at " + seg(s));
        if (g.state_offset[s + 1] == g.state_offset[s])
            return refuse(GMM_ERR_INVALID_ARGUMENT, message, seg(s) + " has no states");
    }
    const uint32_t nStates = g.state_offset[S];
    if (nStates > cap.maxStates)
        return refuse(GMM_ERR_CAPACITY, message,
                      std::to_string(nStates) + " states exceed max_states " + std::to_string(cap.maxStates));
    if (g.arc_offset[0] != 0)
        return refuse(GMM_ERR_INVALID_ARGUMENT, message, "arc_offset[0] is not 0");
    for (uint32_t q = 0; q < nStates; ++q)
        if (g.arc_offset[q + 1] < g.arc_offset[q])
            return refuse(GMM_ERR_INVALID_ARGUMENT, message, "arc_offset decreases at state " + std::to_string(q));
    const uint32_t nArcs = g.arc_offset[nStates];
    if (nArcs > cap.maxArcs)
        return refuse(GMM_ERR_CAPACITY, message,
                      std::to_string(nArcs) + " arcs exceed max_arcs " + std::to_string(cap.maxArcs));
    if (nArcs && (!g.arc_target || !g.arc_mixture || !g.arc_weight))
        return refuse(GMM_ERR_INVALID_ARGUMENT, message, "null array");

    AlignPlan p;
    p.nStates = nStates;
    p.nArcs   = nArcs;
    p.segments.resize(S);
    p.inOffset.assign(static_cast<size_t>(nStates) + 1, 0);
    // the segments, their frame ranges and cells; the arcs' targets and mixtures; the in-degrees into inOffset[q + 1]
    for (uint32_t s = 0; s < S; ++s) {
        AlignSegment& d = p.segments[s];
        d.stateBegin    = g.state_offset[s];
        d.nStates       = g.state_offset[s + 1] - g.state_offset[s];
        d.initial       = g.initial_state ? g.initial_state[s] : 0;
        d.frameBegin    = g.frame_begin[s];
        d.nFrames       = g.n_frames[s];
        d.pad           = 0;
        d.cellBegin     = p.nCells;
        if (d.initial >= d.nStates)
            return refuse(GMM_ERR_INVALID_ARGUMENT, message,
                          seg(s) + ": initial state " + std::to_string(d.initial) + " of " + std::to_string(d.nStates));
        if (d.nFrames == 0)
            return refuse(GMM_ERR_INVALID_ARGUMENT, message, seg(s) + " has no frames");
        const uint64_t end = static_cast<uint64_t>(d.frameBegin) + d.nFrames;
        if (end > 0x100000000ull)
            return refuse(GMM_ERR_INVALID_ARGUMENT, message, seg(s) + ": its frame range ends past 2^32");
        p.frameEnd = std::max(p.frameEnd, end);
        if (d.nStates > GMM_ALIGN_MAX_STATES)
            return refuse(GMM_ERR_UNSUPPORTED, message,
                          seg(s) + " has " + std::to_string(d.nStates) + " states, more than GMM_ALIGN_MAX_STATES " +
                                  std::to_string(GMM_ALIGN_MAX_STATES));
        const uint64_t cells = static_cast<uint64_t>(d.nFrames) * d.nStates;
        if (cells >= 0x100000000ull)
            return refuse(GMM_ERR_UNSUPPORTED, message, seg(s) + " has 2^32 cells (frames x states) or more");
        p.nCells += cells;
        p.maxSegmentStates = std::max(p.maxSegmentStates, d.nStates);
        for (uint32_t a = g.arc_offset[d.stateBegin]; a < g.arc_offset[d.stateBegin + d.nStates]; ++a) {
            if (g.arc_target[a] >= d.nStates)
                return refuse(GMM_ERR_INVALID_ARGUMENT, message,
                              seg(s) + ": arc " + std::to_string(a) + " has target " + std::to_string(g.arc_target[a]) +
                                      " of " + std::to_string(d.nStates) + " states");
            if (g.arc_mixture[a] >= cap.nMixtures)
                return refuse(GMM_ERR_INVALID_ARGUMENT, message,
                              seg(s) + ": arc " + std::to_string(a) + " has mixture " + std::to_string(g.arc_mixture[a]) +
                                      " of " + std::to_string(cap.nMixtures));
            ++p.inOffset[static_cast<size_t>(d.stateBegin) + g.arc_target[a] + 1];
        }
    }
    if (p.nCells > cap.maxCells)
        return refuse(GMM_ERR_CAPACITY, message,
                      std::to_string(p.nCells) + " cells (frames x states) exceed max_cells " + std::to_string(cap.maxCells));
    for (uint32_t q = 0; q < nStates; ++q)
        if (p.inOffset[q + 1] > GMM_ALIGN_MAX_IN_ARCS)
            return refuse(GMM_ERR_UNSUPPORTED, message,
                          "state " + std::to_string(q) + " is entered by " + std::to_string(p.inOffset[q + 1]) +
                                  " arcs, more than GMM_ALIGN_MAX_IN_ARCS " + std::to_string(GMM_ALIGN_MAX_IN_ARCS));
    // frame ranges pairwise disjoint: by ascending begin, each ends before the next begins
    std::vector<uint32_t> byBegin(S);
    std::iota(byBegin.begin(), byBegin.end(), 0u);
    std::sort(byBegin.begin(), byBegin.end(), [&](uint32_t a, uint32_t b) {
        return p.segments[a].frameBegin != p.segments[b].frameBegin ? p.segments[a].frameBegin < p.segments[b].frameBegin
                                                                    : a < b;
    });
    for (uint32_t i = 0; i + 1 < S; ++i) {
        const AlignSegment &a = p.segments[byBegin[i]], &b = p.segments[byBegin[i + 1]];
        if (static_cast<uint64_t>(a.frameBegin) + a.nFrames > b.frameBegin)
            return refuse(GMM_ERR_INVALID_ARGUMENT, message,
                          "the frame ranges of " + seg(byBegin[i]) + " and " + seg(byBegin[i + 1]) + " overlap");
    }
    // the incoming lists: a counting sort by target over the arcs in (source state, arc position) order keeps that order
    for (uint32_t q = 0; q < nStates; ++q)
        p.inOffset[q + 1] += p.inOffset[q];
    p.inSource.resize(nArcs);
    p.inArc.resize(nArcs);
    p.inMixture.resize(nArcs);
    p.inWeight.resize(nArcs);
    std::vector<uint32_t> fill(p.inOffset.begin(), p.inOffset.end() - 1);
    for (uint32_t s = 0; s < S; ++s) {
        const AlignSegment& d = p.segments[s];
        for (uint32_t src = 0; src < d.nStates; ++src)
            for (uint32_t a = g.arc_offset[d.stateBegin + src]; a < g.arc_offset[d.stateBegin + src + 1]; ++a) {
                const uint32_t at = fill[d.stateBegin + g.arc_target[a]]++;
                p.inSource[at]    = src;
                p.inArc[at]       = a;
                p.inMixture[at]   = g.arc_mixture[a];
                p.inWeight[at]    = g.arc_weight[a];
            }
    }
    p.finalWeight.assign(g.final_weight, g.final_weight + nStates);
    // the Baum-Welch call: the arcs as given ...
    p.arcOffset.assign(g.arc_offset, g.arc_offset + nStates + 1);
    if (nArcs) {
        p.arcTarget.assign(g.arc_target, g.arc_target + nArcs);
        p.arcMixture.assign(g.arc_mixture, g.arc_mixture + nArcs);
        p.arcWeight.assign(g.arc_weight, g.arc_weight + nArcs);
    }
    // ... each segment's arcs grouped by mixture: a stable sort of the arcs, which stand in (source state, arc
    // position) order, keeps that order inside a group ...
    p.groupOffset.assign(1, 0u);
    p.groupArcOffset.assign(1, 0u);
    p.groupSource.reserve(nArcs);
    p.groupTarget.reserve(nArcs);
    p.groupWeight.reserve(nArcs);
    std::vector<uint32_t> source, byMixture;
    for (uint32_t s = 0; s < S; ++s) {
        const AlignSegment& d  = p.segments[s];
        const uint32_t      a0 = g.arc_offset[d.stateBegin], a1 = g.arc_offset[d.stateBegin + d.nStates];
        source.resize(a1 - a0);
        for (uint32_t src = 0; src < d.nStates; ++src)
            for (uint32_t a = g.arc_offset[d.stateBegin + src]; a < g.arc_offset[d.stateBegin + src + 1]; ++a)
                source[a - a0] = src;
        byMixture.resize(a1 - a0);
        std::iota(byMixture.begin(), byMixture.end(), a0);
        std::stable_sort(byMixture.begin(), byMixture.end(),
                         [&](uint32_t a, uint32_t b) { return g.arc_mixture[a] < g.arc_mixture[b]; });
        for (size_t i = 0; i < byMixture.size(); ++i) {
            const uint32_t a = byMixture[i];
            if (i == 0 || g.arc_mixture[a] != g.arc_mixture[byMixture[i - 1]]) {
                if (i)
                    p.groupArcOffset.push_back(static_cast<uint32_t>(p.groupSource.size()));
                p.groupMixture.push_back(g.arc_mixture[a]);
            }
            p.groupSource.push_back(source[a - a0]);
            p.groupTarget.push_back(g.arc_target[a]);
            p.groupWeight.push_back(g.arc_weight[a]);
        }
        if (!byMixture.empty())
            p.groupArcOffset.push_back(static_cast<uint32_t>(p.groupSource.size()));
        const uint32_t groups = static_cast<uint32_t>(p.groupMixture.size()) - p.groupOffset.back();
        p.maxSegmentGroups    = std::max(p.maxSegmentGroups, groups);
        p.groupOffset.push_back(static_cast<uint32_t>(p.groupMixture.size()));
    }
    // ... and the segments by table column
    p.colSegment = byBegin;
    p.colFrameOffset.assign(1, 0);
    for (uint32_t i = 0; i < S; ++i)
        p.colFrameOffset.push_back(p.colFrameOffset.back() + p.segments[byBegin[i]].nFrames);
    p.nFrames = p.colFrameOffset.back();
    // the longest segments first: a workgroup's time grows with its frames and with the arcs it scans per frame
    p.order.resize(S);
    std::iota(p.order.begin(), p.order.end(), 0u);
    std::stable_sort(p.order.begin(), p.order.end(), [&](uint32_t a, uint32_t b) {
        return static_cast<uint64_t>(p.segments[a].nFrames) * p.segments[a].nStates >
               static_cast<uint64_t>(p.segments[b].nFrames) * p.segments[b].nStates;
    });
    out = std::move(p);
    return GMM_OK;
}

}  // namespace rasr_gmm
