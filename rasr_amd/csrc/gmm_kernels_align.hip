// gmm_kernels_align.hip -- Viterbi alignment of a batch of segments over a mixture-major score table
// (gmm_aligner_align_*; the contract is include/rasr_gmm_align.h's).
//
// Search::Aligner in Viterbi mode (src/Search/Aligner.cc:135-158, 189-309, 376-436), restated per TARGET state: the
// reference walks the previous frame's hypotheses and pushes each one's arcs; here a lane owns a target state q and pulls
// its incoming arcs, which gmm_aligner_set_segments lists in (source state, arc position) order -- the order in which
// the reference's pushes reach q whenever its hypothesis list is in ascending state order.
//
// One workgroup per segment, a loop over the frames.  Per frame, in LDS: the previous frame's scores and active marks
// (read), this frame's (written), double-buffered, so the frame step has two synchronisations:
//   scan     every lane, for each of its states: the candidates (score(p) + w) + table[m][column] of the incoming arcs
//            from active p, first-initialises / replace iff current >= candidate; score, reached mark and backpointer
//            written; the lane's minimum over its reached states (strict >, from FLT_MAX)
//   minimum  across the lanes (shuffles inside a wave, LDS across the waves)                        -- sync 1
//   prune    threshold = minimum + pruning; a lane clears the marks of its states above it           -- sync 2
// The emission gather table[m][column] is issued for every incoming arc whether or not its source is active: the load
// then does not wait for the LDS read of the mark, and consecutive frames of a lane stay in one cache line.
// A segment of at most kAlignWaveStates states is aligned by wave 0 alone: the two synchronisations are then no
// barriers at all, only the order of one wave's LDS operations.
// After the last frame: the final scan (a lexicographic minimum over (final weight + score, state), which is the
// reference's strict < scan in ascending state order), then the trace-back: lane 0 follows the chain of backpointers,
// one dependent load per frame, and leaves (ordinal, state) of frame t in the frame's cell 0; all lanes then resolve
// these to the arc, its mixture and its target and write the outputs.
// Every floating-point operation is an _rn intrinsic (the unit is also built with -ffp-contract=off).
// The end of the frame step (minimum, threshold) and everything of the search are gmm_align_step.hh's, shared with the
// Baum-Welch sweep; the scan, the prune's keep loop and the final scan (which also sums the hypotheses) are this unit's.
// alignViterbi<true> (gmm_aligner_align_search_*) is the same kernel with the search on: the retry loop of feed(vector)
// around the frame loop, the n-best step in the prune; alignViterbi<false> has none of it, nor its LDS.
#include "gmm_align_step.hh"

namespace rasr_gmm {
namespace dev {
namespace {

constexpr uint32_t kNone = 0xffffffffu;

// the final scan's order: a smaller value first, the lower state among equal values
__device__ __forceinline__ void finalStep(float& v, uint32_t& q, float v2, uint32_t q2) {
    const bool take = v2 < v || (v2 == v && q2 < q);
    v               = take ? v2 : v;
    q               = take ? q2 : q;
}

// kSearch: the pass below runs inside the retry loop of feed(vector), with the n-best step in its prune; without it the
// function is the one pass at a.pruning
template <bool kWave, bool kSearch>
__device__ __forceinline__ void alignSegment(const AlignArgs& a, const uint32_t segment, float* rows, uint8_t* marks,
                                             float* redV, uint32_t* redQ, SearchLds* searchLds) {
    constexpr uint32_t T   = kWave ? 64u : kAlignThreads;
    const AlignSegment sg  = a.segments[segment];
    const uint32_t     tid = threadIdx.x, n = sg.nStates, gb = sg.stateBegin;
    const uint32_t     wave = tid >> 6, lane = tid & 63u;
    uint32_t* const    cells = a.cells + sg.cellBegin;
    float              pruning = a.pruning, previous = FLT_MAX, best;
    uint32_t           iterations = 0, bestState, hypotheses;
    if constexpr (kSearch)
        pruning = a.search.rule.minPruning;

    for (;;) {  // the passes of the search; one without it
        // start: the initial state alone, with score 0
        for (uint32_t q = tid; q < n; q += T) {
            rows[q]  = 0.0f;
            marks[q] = q == sg.initial;
        }
        sync<kWave>();

        hypotheses = 0;
        for (uint32_t t = 0; t < sg.nFrames; ++t) {
            const uint32_t       from = (t & 1u) * a.rowStates, to = ((t & 1u) ^ 1u) * a.rowStates;
            const float* const   prev = rows + from;
            const uint8_t* const prevMark = marks + from;
            float* const         cur = rows + to;
            uint8_t* const       curMark = marks + to;
            const float* const   column = a.scores + sg.frameBegin + t;
            uint32_t* const      back = cells + static_cast<size_t>(t) * n;
            float                mn = FLT_MAX;
            uint32_t             nReached = 0;  // kSearch only
            for (uint32_t q = tid; q < n; q += T) {
                const uint32_t j0 = a.inOffset[gb + q], j1 = a.inOffset[gb + q + 1];
                bool           reached = false;
                float          score = 0.0f;
                uint32_t       bp = 0;
                for (uint32_t j = j0; j < j1; ++j) {
                    const uint32_t p = a.inSource[j];
                    const float    w = a.inWeight[j];
                    const float    e = column[static_cast<size_t>(a.inMixture[j]) * a.scoreStride];
                    if (prevMark[p]) {
                        const float cand = __fadd_rn(__fadd_rn(prev[p], w), e);
                        if (!reached || score >= cand) {
                            score = cand;
                            bp    = ((j - j0) << 16) | p;
                        }
                        reached = true;
                    }
                }
                cur[q]     = score;
                curMark[q] = reached;
                back[q]    = bp;
                if (reached)
                    mn = minStep(mn, score);
                if constexpr (kSearch)
                    nReached += reached;
            }
            const float threshold = pruneThreshold<kWave, kSearch>(mn, nReached, pruning, cur, curMark, n,
                                                                   a.search.rule.nBest, redV, searchLds);
            for (uint32_t q = tid; q < n; q += T)
                if (curMark[q]) {
                    const bool keep = cur[q] <= threshold;
                    curMark[q]      = keep;
                    hypotheses += keep;
                }
            sync<kWave>();
        }

        // the final scan over the active states of the last frame
        const uint32_t last = (sg.nFrames & 1u) * a.rowStates;
        best      = FLT_MAX;
        bestState = kNone;
        for (uint32_t q = tid; q < n; q += T)
            if (marks[last + q]) {
                const float v = __fadd_rn(a.finalWeight[gb + q], rows[last + q]);
                if (v < best) {
                    best      = v;
                    bestState = q;
                }
            }
        for (uint32_t d = 32; d; d >>= 1) {
            const float    v2 = __shfl_xor(best, d);
            const uint32_t q2 = __shfl_xor(bestState, d);
            finalStep(best, bestState, v2, q2);
            hypotheses += __shfl_xor(hypotheses, d);
        }
        if constexpr (!kWave) {
            // redV's last readers are behind the last frame's second barrier; the hypotheses ride on the scan's barrier
            if (lane == 0) {
                redV[wave]          = best;
                redQ[wave]          = bestState;
                redQ[kWaves + wave] = hypotheses;
            }
            __syncthreads();
            best       = FLT_MAX;
            bestState  = kNone;
            hypotheses = 0;
            for (uint32_t w = 0; w < kWaves; ++w) {
                finalStep(best, bestState, redV[w], redQ[w]);
                hypotheses += redQ[kWaves + w];
            }
        }
        // the pass is over: every lane holds its score and hypothesis count, so one wave decides in every lane alike.
        // The next pass overwrites the backpointers
        if constexpr (kSearch) {
            if (!searchPassEnds<kWave, kWave>(a.search, *searchLds, segment, best, hypotheses, sg.nFrames, iterations,
                                              previous, pruning))
                continue;
        }
        break;
    }
    if (tid == 0) {
        if (a.outScore)
            a.outScore[segment] = best;
        if (a.outHypotheses)
            a.outHypotheses[segment] = hypotheses;
    }
    if (!a.outMixture && !a.outState && !a.outArc)
        return;
    if (bestState == kNone) {
        for (uint32_t t = tid; t < sg.nFrames; t += T) {
            const size_t at = static_cast<size_t>(sg.frameBegin) + t;
            if (a.outMixture)
                a.outMixture[at] = kNone;
            if (a.outState)
                a.outState[at] = kNone;
            if (a.outArc)
                a.outArc[at] = kNone;
        }
        return;
    }
    // the trace-back over the other lanes' backpointer stores
    sync<kWave, true>();
    if (tid == 0) {
        uint32_t q = bestState;
        for (uint32_t t = sg.nFrames; t-- > 0;) {
            uint32_t* const back = cells + static_cast<size_t>(t) * n;
            const uint32_t  bp   = back[q];
            back[0]              = (bp & 0xffff0000u) | q;
            q                    = bp & 0xffffu;
        }
    }
    sync<kWave, true>();
    for (uint32_t t = tid; t < sg.nFrames; t += T) {
        const uint32_t rec = cells[static_cast<size_t>(t) * n];
        const uint32_t q = rec & 0xffffu, j = a.inOffset[gb + q] + (rec >> 16);
        const size_t   at = static_cast<size_t>(sg.frameBegin) + t;
        if (a.outMixture)
            a.outMixture[at] = a.inMixture[j];
        if (a.outState)
            a.outState[at] = q;
        if (a.outArc)
            a.outArc[at] = a.inArc[j];
    }
}

}  // namespace

// one workgroup per segment; in a search each with its own number of passes
template <bool kSearch>
__global__ __launch_bounds__(kAlignThreads) void alignViterbi(AlignArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ float    redV[kWaves];
    __shared__ uint32_t redQ[2 * kWaves];
    static_assert(GMM_ALIGN_MAX_STATES * kAlignLdsBytesPerState + sizeof(redV) + sizeof(redQ) + sizeof(SearchLds) +
                                  2 * kLdsAlign <= kLdsBytes,
                  "the rows of the largest segment fit beside all static LDS, the search's included");
    SearchLds* searchLds = nullptr;
    if constexpr (kSearch) {
        __shared__ SearchLds s;
        searchLds = &s;
    }
    float* const   rows  = reinterpret_cast<float*>(lds);
    uint8_t* const marks = lds + 2u * a.rowStates * sizeof(float);
    const uint32_t segment = a.order[blockIdx.x];
    // uniform over the workgroup: either wave 0 alone, with no barrier, or all waves through every barrier
    if (a.segments[segment].nStates <= kAlignWaveStates) {
        if (threadIdx.x < 64)
            alignSegment<true, kSearch>(a, segment, rows, marks, redV, redQ, searchLds);
    } else {
        alignSegment<false, kSearch>(a, segment, rows, marks, redV, redQ, searchLds);
    }
}

}  // namespace dev

hipError_t launchAlign(const AlignArgs& a, hipStream_t stream) {
    if (a.nSegments == 0)
        return hipSuccess;
    const size_t ldsBytes = static_cast<size_t>(a.rowStates) * kAlignLdsBytesPerState;
    const auto   kernel   = a.search.on ? dev::alignViterbi<true> : dev::alignViterbi<false>;
    hipLaunchKernelGGL(kernel, dim3(a.nSegments), dim3(kAlignThreads), ldsBytes, stream, a);
    return hipGetLastError();
}

}  // namespace rasr_gmm
