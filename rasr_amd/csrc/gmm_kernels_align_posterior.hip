// gmm_kernels_align_posterior.hip -- Baum-Welch alignment of a batch of segments over a mixture-major score table:
// per-frame mixture posteriors (gmm_aligner_posteriors_*; the contract is include/rasr_gmm_align.h's).
//
// Search::Aligner in baum-welch mode (src/Search/Aligner.cc:160-187, 206-309, 376-396, 438-452, 696-779), posterior64
// (src/Fsa/Sssp.cc:67-222) and Alignment::combineItems .. filterWeightsGT (src/Speech/Alignment.cc:442-578), restated per
// target state as gmm_kernels_align.hip restates Viterbi mode.  Five launches, no host synchronisation between them:
//   alignPosteriorSweep   one workgroup per segment, the longest first; single-wave form up to kAlignWaveStates states.
//       forward   a loop over the frames, rows double-buffered in LDS.  A lane owns target states; per state it scans the
//                 incoming arcs from the states active after the previous frame, in (source state, arc position) order,
//                 and forms BOTH the f32 collected score of the search and the f64 forward potential of posterior64 (its
//                 batch form: a <= scan for the minimum, then the sum over the other arcs).  The potential of a state
//                 depends on the survivors of the previous frame only, so it needs no pass of its own; the one of a
//                 state pruned afterwards is never read.  Minimum, threshold and marks as in the Viterbi kernel.
//                 Per (frame, state) cell it leaves the active mark and the forward potential in the scratch.
//       end       lane 0 collects final weight + score over the active final states in ascending order.
//       backward  a loop over the frames from the last, a lane owns source states and walks their outgoing arcs in arc
//                 order; the row of the next frame in LDS, the marks from the scratch.  Leaves the backward potential per
//                 cell; lane 0 forms bw[initial].  A state that reaches no final state keeps the zero, DBL_MAX.
//   alignPosteriorItems<false>  one WAVE per frame (of any segment).  A lane owns mixture groups of the frame's segment
//                 and walks each group's arcs, which stand in (source state, arc position) order: the arcs with both ends
//                 active give f32 log posteriors, collected in that order.  Clip, the frame's minimum, exp.  The sum in
//                 ascending mixture order is a chain of f32 additions: every lane runs it over the 64 values of a chunk
//                 passed round with constant-lane shuffles.  Leaves minimum, 1 / sum and the count of kept items per frame.
//   alignPosteriorScan    one workgroup: the exclusive scan of the counts over the frames in column order; the total.
//   alignPosteriorColumns the CSR over the table columns, by a search of the column's segment.
//   alignPosteriorItems<true>   the item pass again with the minimum and 1 / sum known: writes the compact list.
// Every f32 / f64 add, subtract, multiply and divide is an _rn intrinsic (the unit is also built with
// -ffp-contract=off); exp and log1p are the device library's f64 functions.  No atomics.
// The end of the forward frame step (minimum, threshold), the sum of the hypotheses and everything of the search are
// gmm_align_step.hh's, shared with the Viterbi kernel; posterior64's batch collect is written once, batchCollect64.
// alignPosteriorSweep<true> (gmm_aligner_posteriors_search_*) is the sweep with the search on: the retry loop of
// feed(vector) around forward and end, the n-best step in the prune (its digit counters are integer LDS atomics);
// alignPosteriorSweep<false> has none of it, nor its LDS.  The other four launches serve both.
#include "gmm_align_step.hh"

#include <cmath>

namespace rasr_gmm {
namespace dev {
namespace {

// LogSemiring<f32>::collect: FLT_MAX is the zero; min - log1p(exp(min - max)), the transcendentals in f64 on the widened
// difference, their value rounded once to f32
__device__ __forceinline__ float collect32(float a, float b) {
    if (b == FLT_MAX)
        return a;
    if (a == FLT_MAX)
        return b;
    const float mn = b < a ? b : a, mx = a < b ? b : a;
    const float y  = __double2float_rn(log1p(exp(static_cast<double>(__fsub_rn(mn, mx)))));
    return __fsub_rn(mn, y);
}

// posterior64's arc score: potential + f32 weight in f64, an infinity becomes the zero
__device__ __forceinline__ double extend64(double potential, float arcScore) {
    const double s = __dadd_rn(potential, static_cast<double>(arcScore));
    return isinf(s) ? DBL_MAX : s;
}

// posterior64's batch collect, closed: min - log1p(sum), at most the zero (log1p(0) is 0 exactly)
__device__ __forceinline__ double close64(double mn, double sum) {
    const double v = sum == 0.0 ? mn : __dsub_rn(mn, log1p(sum));
    return v < DBL_MAX ? v : DBL_MAX;
}

// posterior64's batch collect over the arcs k0 .. k1 of a state: a <= scan for the minimum of score(k) over the arcs
// with active(k), then the sum of exp(minimum - score(k)) over the other active arcs, closed.  visit(k) runs once per
// active arc, in arc order, beside the scan
struct NoVisit {
    __device__ void operator()(uint32_t) const {}
};
template <class Active, class Score, class Visit = NoVisit>
__device__ __forceinline__ double batchCollect64(uint32_t k0, uint32_t k1, Active active, Score score,
                                                 Visit visit = Visit{}) {
    double   potMin = DBL_MAX;
    uint32_t kMin = k1, nActive = 0;
    for (uint32_t k = k0; k < k1; ++k)
        if (active(k)) {
            visit(k);
            ++nActive;
            const double s = score(k);
            if (s <= potMin) {
                potMin = s;
                kMin   = k;
            }
        }
    double sum = 0.0;
    if (nActive > 1)
        for (uint32_t k = k0; k < k1; ++k)
            if (k != kMin && active(k))
                sum = __dadd_rn(sum, exp(__dsub_rn(potMin, score(k))));
    return close64(potMin, sum);
}

// posterior64's backward step of the (global) source state: its arcs, in arc order, into the states active in the next
// frame, whose marks, potentials and table column are given
__device__ __forceinline__ double backwardState(const AlignPosteriorArgs& a, uint32_t state, const uint8_t* nextMark,
                                                const double* next, const float* column) {
    return batchCollect64(
            a.arcOffset[state], a.arcOffset[state + 1], [&](uint32_t k) { return nextMark[a.arcTarget[k]] != 0; },
            [&](uint32_t k) {
                const float arcScore =
                        __fadd_rn(a.arcWeight[k], column[static_cast<size_t>(a.arcMixture[k]) * a.scoreStride]);
                return extend64(next[a.arcTarget[k]], arcScore);
            });
}

// kSearch: the forward part and the end run inside the retry loop of feed(vector), with the n-best step in the prune; a
// pass overwrites the cells of the one before, and the backward sweep runs once, over the last pass's.  Without it the
// function is the one pass at a.pruning
template <bool kWave, bool kSearch>
__device__ __forceinline__ void sweepSegment(const AlignPosteriorArgs& a, const uint32_t segment, double* rows64,
                                             float* rows32, uint8_t* marks, float* redV, uint32_t* redQ,
                                             SearchLds* searchLds) {
    constexpr uint32_t T   = kWave ? 64u : kAlignThreads;
    const AlignSegment sg  = a.segments[segment];
    const uint32_t     tid = threadIdx.x, n = sg.nStates, gb = sg.stateBegin, R = a.rowStates;
    double* const      fwPot = a.fwPot + sg.cellBegin;
    double* const      bwPot = a.bwPot + sg.cellBegin;
    uint8_t* const     mark  = a.mark + sg.cellBegin;
    const uint32_t     last = (sg.nFrames & 1u) * R;
    float              pruning = a.pruning, previous = FLT_MAX;  // previous: lane 0's
    uint32_t           iterations = 0;
    if constexpr (kSearch)
        pruning = a.search.rule.minPruning;

    for (;;) {  // the passes of the search; one without it
        for (uint32_t q = tid; q < n; q += T) {
            rows32[q] = 0.0f;
            rows64[q] = 0.0;
            marks[q]  = q == sg.initial;
        }
        sync<kWave>();

        // forward
        uint32_t hypotheses = 0;
        for (uint32_t t = 0; t < sg.nFrames; ++t) {
            const uint32_t       from = (t & 1u) * R, to = ((t & 1u) ^ 1u) * R;
            const float* const   prev = rows32 + from;
            const double* const  prevPot = rows64 + from;
            const uint8_t* const prevMark = marks + from;
            float* const         cur = rows32 + to;
            double* const        curPot = rows64 + to;
            uint8_t* const       curMark = marks + to;
            const float* const   column = a.scores + sg.frameBegin + t;
            const size_t         row = static_cast<size_t>(t) * n;
            float                mn = FLT_MAX;
            uint32_t             nReached = 0;  // kSearch only
            for (uint32_t q = tid; q < n; q += T) {
                const uint32_t j0 = a.inOffset[gb + q], j1 = a.inOffset[gb + q + 1];
                bool           reached = false;
                float          score = 0.0f;
                auto           arcScore = [&](uint32_t j) {
                    return __fadd_rn(a.inWeight[j], column[static_cast<size_t>(a.inMixture[j]) * a.scoreStride]);
                };
                const double pot = batchCollect64(
                        j0, j1, [&](uint32_t j) { return prevMark[a.inSource[j]] != 0; },
                        [&](uint32_t j) { return extend64(prevPot[a.inSource[j]], arcScore(j)); },
                        [&](uint32_t j) {
                            const float cand = __fadd_rn(prev[a.inSource[j]], arcScore(j));
                            score            = reached ? collect32(score, cand) : cand;
                            reached          = true;
                        });
                cur[q]           = score;
                curPot[q]        = pot;
                curMark[q]       = reached;
                fwPot[row + q]   = pot;
                if (reached)
                    mn = minStep(mn, score);
                if constexpr (kSearch)
                    nReached += reached;
            }
            const float threshold = pruneThreshold<kWave, kSearch>(mn, nReached, pruning, cur, curMark, n,
                                                                   a.search.rule.nBest, redV, searchLds);
            for (uint32_t q = tid; q < n; q += T) {
                bool keep = false;
                if (curMark[q]) {
                    keep       = cur[q] <= threshold;
                    curMark[q] = keep;
                    hypotheses += keep;
                }
                mark[row + q] = keep;
            }
            sync<kWave>();
        }

        hypotheses = sumHypotheses<kWave>(hypotheses, redQ);

        // end: lane 0's alignmentScore() over the active final states in ascending order; in a search it then decides
        // whether the pass was the last, and only the last one's results are written
        float    result = FLT_MAX;
        uint32_t has = 0;
        if (tid == 0) {
            for (uint32_t q = 0; q < n; ++q)
                if (marks[last + q]) {
                    const float fw = a.finalWeight[gb + q];
                    if (fw != INFINITY) {
                        const float v = __fadd_rn(fw, rows32[last + q]);
                        result        = result == FLT_MAX ? v : collect32(result, v);
                        has           = 1;
                    }
                }
            if (!has)
                result = FLT_MAX;
        }
        if constexpr (kSearch) {
            if (!searchPassEnds<kWave, false>(a.search, *searchLds, segment, result, hypotheses, sg.nFrames, iterations,
                                              previous, pruning))
                continue;
        }
        if (tid == 0) {
            if (a.outScore)
                a.outScore[segment] = result;
            if (a.outHypotheses)
                a.outHypotheses[segment] = hypotheses;
            a.segHas[segment] = has;
            redQ[kWaves]      = has;
        }
        break;
    }
    // redQ[kWaves] and the marks of the scratch are read below by other lanes than wrote them
    sync<kWave, true>();
    if (!redQ[kWaves]) {
        if (tid == 0) {
            a.segTotalInv[segment] = 0.0;
            if (a.outLogTotal)
                a.outLogTotal[segment] = DBL_MAX;
        }
        return;
    }

    // backward: the last frame's potentials are the final weights
    {
        const uint32_t t = sg.nFrames - 1;
        double* const  cur = rows64 + (t & 1u) * R;
        const size_t   row = static_cast<size_t>(t) * n;
        for (uint32_t q = tid; q < n; q += T) {
            const float  fw = a.finalWeight[gb + q];
            const double v  = marks[last + q] && fw != INFINITY ? static_cast<double>(fw) : DBL_MAX;
            cur[q]          = v;
            bwPot[row + q]  = v;
        }
    }
    sync<kWave>();
    for (uint32_t t = sg.nFrames - 1; t-- > 0;) {
        double* const        cur = rows64 + (t & 1u) * R;
        const double* const  next = rows64 + ((t & 1u) ^ 1u) * R;
        const size_t         row = static_cast<size_t>(t) * n;
        const uint8_t* const nextMark = mark + row + n;
        const float* const   column = a.scores + sg.frameBegin + t + 1;
        for (uint32_t p = tid; p < n; p += T) {
            const double v = mark[row + p] ? backwardState(a, gb + p, nextMark, next, column) : DBL_MAX;
            cur[p]         = v;
            bwPot[row + p] = v;
        }
        sync<kWave>();
    }
    // bw[initial]: the backward step of the initial state with frame 0 as the next frame
    if (tid == 0) {
        const double total     = backwardState(a, gb + sg.initial, mark, rows64, a.scores + sg.frameBegin);
        a.segTotalInv[segment] = -total;
        if (a.outLogTotal)
            a.outLogTotal[segment] = total;
    }
}

// the ordered frame r: its segment (the last i with colFrameOffset[i] <= r) and its frame in it
__device__ __forceinline__ uint32_t frameSegment(const AlignPosteriorArgs& a, uint32_t r, uint32_t& t) {
    uint32_t lo = 0, hi = a.nSegments;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.colFrameOffset[mid] <= r)
            lo = mid;
        else
            hi = mid;
    }
    t = r - a.colFrameOffset[lo];
    return a.colSegment[lo];
}

}  // namespace

// one workgroup per segment; in a search each with its own number of forward passes
template <bool kSearch>
__global__ __launch_bounds__(kAlignThreads) void alignPosteriorSweep(AlignPosteriorArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ float    redV[kWaves];
    __shared__ uint32_t redQ[kWaves + 1];
    static_assert(((GMM_ALIGN_MAX_STATES_POSTERIOR + 63u) & ~63u) * kAlignPosteriorLdsBytesPerState + sizeof(redV) +
                                  sizeof(redQ) + sizeof(SearchLds) + 2 * kLdsAlign <= kLdsBytes,
                  "the rows of the largest segment fit beside all static LDS, the search's included");
    SearchLds* searchLds = nullptr;
    if constexpr (kSearch) {
        __shared__ SearchLds s;
        searchLds = &s;
    }
    double* const  rows64 = reinterpret_cast<double*>(lds);
    float* const   rows32 = reinterpret_cast<float*>(lds + 2u * a.rowStates * sizeof(double));
    uint8_t* const marks  = lds + 2u * a.rowStates * (sizeof(double) + sizeof(float));
    const uint32_t segment = a.order[blockIdx.x];
    if (a.segments[segment].nStates <= kAlignWaveStates) {
        if (threadIdx.x < 64)
            sweepSegment<true, kSearch>(a, segment, rows64, rows32, marks, redV, redQ, searchLds);
    } else {
        sweepSegment<false, kSearch>(a, segment, rows64, rows32, marks, redV, redQ, searchLds);
    }
}

// one wave per ordered frame
template <bool kWrite>
__global__ __launch_bounds__(64) void alignPosteriorItems(AlignPosteriorArgs a) {
    const uint32_t lane = threadIdx.x;
    float* const   weights = a.waveWeights + static_cast<size_t>(blockIdx.x) * a.rowGroups;
    for (uint32_t r = blockIdx.x; r < a.nFrames; r += gridDim.x) {
        uint32_t       t;
        const uint32_t segment = frameSegment(a, r, t);
        if (!a.segHas[segment]) {
            if (!kWrite && lane == 0)
                a.frameCount[r] = 0;
            continue;
        }
        const AlignSegment   sg = a.segments[segment];
        const uint32_t       n = sg.nStates;
        const size_t         row = sg.cellBegin + static_cast<size_t>(t) * n;
        const uint8_t* const curMark = a.mark + row;
        const double* const  bw = a.bwPot + row;
        // frame 0's sources: the initial state alone, with potential 0
        const uint8_t* const prevMark = a.mark + (t ? row - n : row);
        const double* const  fw = a.fwPot + (t ? row - n : row);
        const double         totalInv = a.segTotalInv[segment];
        const uint32_t       column = sg.frameBegin + t;
        const uint32_t       g0 = a.groupOffset[segment], nGroups = a.groupOffset[segment + 1] - g0;
        const uint32_t       nChunks = (nGroups + 63u) / 64u;
        float                frameMin = kWrite ? a.frameMin[r] : FLT_MAX;
        const float          frameInv = kWrite ? a.frameInv[r] : 0.0f;
        uint32_t             count = 0;
        const uint32_t       base = kWrite ? a.frameCount[r] : 0;

        // a group's collected log posterior, clipped to [0, FLT_MAX]; false without an arc of the trellis
        auto collectGroup = [&](uint32_t g, float& x) -> bool {
            const float    e = a.scores[static_cast<size_t>(a.groupMixture[g0 + g]) * a.scoreStride + column];
            const uint32_t k0 = a.groupArcOffset[g0 + g], k1 = a.groupArcOffset[g0 + g + 1];
            bool           has = false;
            for (uint32_t k = k0; k < k1; ++k) {
                const uint32_t p = a.groupSource[k], q = a.groupTarget[k];
                const bool     from = t == 0 ? p == sg.initial : prevMark[p] != 0;
                if (from && curMark[q]) {
                    const float  arcScore = __fadd_rn(a.groupWeight[k], e);
                    const double f        = t == 0 ? 0.0 : fw[p];
                    const double sum =
                            __dadd_rn(__dadd_rn(__dadd_rn(f, static_cast<double>(arcScore)), bw[q]), totalInv);
                    const float lp = sum < static_cast<double>(FLT_MAX) ? __double2float_rn(sum) : FLT_MAX;
                    x              = has ? collect32(x, lp) : lp;
                    has            = true;
                }
            }
            if (has)
                x = x < 0.0f ? 0.0f : (x > FLT_MAX ? FLT_MAX : x);
            return has;
        };
        // exp(-(x - minimum)) in std space
        auto expm = [&](float x) -> float {
            const float d = __fsub_rn(x, frameMin);
            return isinf(d) ? 0.0f : __double2float_rn(exp(-static_cast<double>(d)));
        };

        if constexpr (!kWrite) {
            // the collected values, each lane's own entries of the wave's row; the minimum
            for (uint32_t c = 0; c < nChunks; ++c) {
                const uint32_t g = c * 64u + lane;
                float          x = 0.0f;
                const bool     has = g < nGroups && collectGroup(g, x);
                if (g < nGroups)
                    weights[g] = has ? x : NAN;
                if (has)
                    frameMin = minStep(frameMin, x);
            }
            for (uint32_t d = 32; d; d >>= 1)
                frameMin = minStep(frameMin, __shfl_xor(frameMin, d));
            // the sum in ascending mixture order: a chain of f32 additions, run by every lane alike
            float sum = 0.0f;
            for (uint32_t c = 0; c < nChunks; ++c) {
                const uint32_t g = c * 64u + lane;
                const float    x = g < nGroups ? weights[g] : NAN;
                const bool     has = !isnan(x);
                const float    w = has ? expm(x) : 0.0f;
                if (g < nGroups)
                    weights[g] = has ? w : NAN;
                const unsigned long long hasMask = __ballot(has);
#pragma unroll
                for (uint32_t i = 0; i < 64; ++i) {
                    const float wi = __shfl(w, static_cast<int>(i));
                    if ((hasMask >> i) & 1ull)
                        sum = __fadd_rn(sum, wi);
                }
            }
            const float inv = sum != 0.0f ? __fdiv_rn(1.0f, sum) : 1.0f;
            for (uint32_t c = 0; c < nChunks; ++c) {
                const uint32_t g = c * 64u + lane;
                // a group without an arc of the trellis left a NaN, which is above nothing
                const bool keep = g < nGroups && __fmul_rn(weights[g], inv) > a.minPosterior;
                count += __popcll(__ballot(keep));
            }
            if (lane == 0) {
                a.frameMin[r]   = frameMin;
                a.frameInv[r]   = inv;
                a.frameCount[r] = count;
            }
        } else {
            for (uint32_t c = 0; c < nChunks; ++c) {
                const uint32_t g = c * 64u + lane;
                float          x = 0.0f, w = 0.0f;
                bool           keep = false;
                if (g < nGroups && collectGroup(g, x)) {
                    w    = __fmul_rn(expm(x), frameInv);
                    keep = w > a.minPosterior;
                }
                const unsigned long long keepMask = __ballot(keep);
                const uint32_t           at = base + count + __popcll(keepMask & ((1ull << lane) - 1ull));
                if (keep && at < a.maxItems) {
                    a.outItemFrame[at]   = column;
                    a.outItemMixture[at] = a.groupMixture[g0 + g];
                    a.outItemWeight[at]  = static_cast<double>(w);
                }
                count += __popcll(keepMask);
            }
        }
    }
}

// the exclusive scan of frameCount[0 .. nFrames) in place, the total into frameCount[nFrames] and *outNItems
constexpr uint32_t kScanPerLane = 16;
__global__ __launch_bounds__(kAlignThreads) void alignPosteriorScan(AlignPosteriorArgs a) {
    __shared__ uint32_t part[kAlignThreads];
    const uint32_t      tid = threadIdx.x;
    uint32_t            carry = 0;
    for (uint64_t begin = 0; begin < a.nFrames; begin += static_cast<uint64_t>(kAlignThreads) * kScanPerLane) {
        const uint64_t first = begin + static_cast<uint64_t>(tid) * kScanPerLane;
        uint32_t       v[kScanPerLane], mine = 0;
        for (uint32_t i = 0; i < kScanPerLane; ++i) {
            v[i] = first + i < a.nFrames ? a.frameCount[first + i] : 0;
            mine += v[i];
        }
        part[tid] = mine;
        __syncthreads();
        for (uint32_t d = 1; d < kAlignThreads; d <<= 1) {
            const uint32_t other = tid >= d ? part[tid - d] : 0;
            __syncthreads();
            part[tid] += other;
            __syncthreads();
        }
        uint32_t run = carry + part[tid] - mine;
        for (uint32_t i = 0; i < kScanPerLane; ++i)
            if (first + i < a.nFrames) {
                a.frameCount[first + i] = run;
                run += v[i];
            }
        carry += part[kAlignThreads - 1];
        __syncthreads();
    }
    if (tid == 0) {
        a.frameCount[a.nFrames] = carry;
        if (a.outNItems)
            *a.outNItems = carry;
    }
}

// out_column_offset[c], c in 0 .. nTableFrames: the items before table column c
__global__ __launch_bounds__(kAlignThreads) void alignPosteriorColumns(AlignPosteriorArgs a) {
    const uint64_t c = static_cast<uint64_t>(blockIdx.x) * kAlignThreads + threadIdx.x;
    if (c > a.nTableFrames)
        return;
    // the last segment, by column, that begins at or before c
    uint32_t lo = 0, hi = a.nSegments;  // the answer is in [lo, hi) if any begins at or before c
    if (a.segments[a.colSegment[0]].frameBegin > c) {
        a.outColumnOffset[c] = 0;
        return;
    }
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.segments[a.colSegment[mid]].frameBegin <= c)
            lo = mid;
        else
            hi = mid;
    }
    const AlignSegment sg = a.segments[a.colSegment[lo]];
    const uint64_t     in = c - sg.frameBegin;
    a.outColumnOffset[c] = in < sg.nFrames ? a.frameCount[a.colFrameOffset[lo] + in] : a.frameCount[a.colFrameOffset[lo + 1]];
}

}  // namespace dev

hipError_t launchAlignPosteriors(const AlignPosteriorArgs& a, hipStream_t stream) {
    if (a.nSegments == 0)
        return hipSuccess;
    const size_t ldsBytes = static_cast<size_t>(a.rowStates) * kAlignPosteriorLdsBytesPerState;
    const auto   sweep    = a.search.on ? dev::alignPosteriorSweep<true> : dev::alignPosteriorSweep<false>;
    hipLaunchKernelGGL(sweep, dim3(a.nSegments), dim3(kAlignThreads), ldsBytes, stream, a);
    const uint32_t itemWaves = a.nFrames < kAlignItemWaves ? a.nFrames : kAlignItemWaves;
    hipLaunchKernelGGL(dev::alignPosteriorItems<false>, dim3(itemWaves), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(dev::alignPosteriorScan, dim3(1), dim3(kAlignThreads), 0, stream, a);
    if (a.outColumnOffset) {
        const uint32_t blocks = static_cast<uint32_t>((static_cast<uint64_t>(a.nTableFrames) + kAlignThreads) / kAlignThreads);
        hipLaunchKernelGGL(dev::alignPosteriorColumns, dim3(blocks), dim3(kAlignThreads), 0, stream, a);
    }
    if (a.outItemFrame)
        hipLaunchKernelGGL(dev::alignPosteriorItems<true>, dim3(itemWaves), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rasr_gmm
