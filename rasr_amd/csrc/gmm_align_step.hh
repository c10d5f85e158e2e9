// gmm_align_step.hh -- the device code that the Viterbi kernel (gmm_kernels_align.hip) and the Baum-Welch sweep
// (gmm_kernels_align_posterior.hip) share, with and without the search; included by the two kernel units only.
//   the step    sync, minStep, kWaves; pruneThreshold, the end of a frame step behind a mode's candidate loop: the
//               frame's minimum over the wave and the workgroup, the threshold, the n-best step; sumHypotheses
//   the search  the stop rule of Search::Aligner::feed(vector) (src/Search/Aligner.cc:594-621), the n-best step of prune
//               (src/Search/Aligner.cc:254-276) and searchPassEnds, the end of a pass; the contract is
//               include/rasr_gmm_align.h's ("THE SEARCH").  The fixed-threshold instantiations use nothing of it and
//               have no SearchLds.
//
// The n-best step is a k-th-smallest selection over the reached states' scores of the frame's row in LDS, k = n_best:
//   select   a radix select on the order-preserving u32 image of the scores, most significant digit first, 4 bits a
//            pass: the lanes count their states that still match the digits found so far into 16 integer LDS counters
//            (integer atomics: their result does not depend on the arrival order), then every lane reads the 16
//            counters and finds the digit that holds the k-th.  Eight passes, each with its own counters, so they are
//            cleared once and a pass costs one synchronisation.
//   ties     if more states hold the k-th score than may stay, the lowest state indices stay: a prefix count in state
//            order, ballots and popcounts inside a wave, the waves' counts per round of kAlignThreads states through LDS.
//   demote   every state behind the first k gets the score threshold + 1.
// A lane reads and writes the scores of its own states only (q = tid, tid + T, ...), as the frame step does.
#pragma once

#include <cfloat>

#include "gmm_align.hh"

namespace rasr_gmm {
namespace dev {

constexpr uint32_t kWaves       = kAlignThreads / 64;
constexpr uint32_t kNBestPasses = 8, kNBestBins = 16;
constexpr uint32_t kNBestRounds = GMM_ALIGN_MAX_STATES / kAlignThreads;  // the rounds of kAlignThreads states of a row
static_assert(GMM_ALIGN_MAX_STATES % kAlignThreads == 0 && GMM_ALIGN_MAX_STATES_POSTERIOR <= GMM_ALIGN_MAX_STATES,
              "kNBestRounds covers the rows of both modes");

// the static LDS of a search instantiation beside the rows and its own redV / redQ: together they have to fit what
// include/rasr_gmm_align.h leaves free for the reductions in both modes (1 KiB in Baum-Welch mode)
struct SearchLds {
    uint32_t count[kNBestPasses][kNBestBins];  // the digit counters of the radix select
    uint32_t equal[kNBestRounds][kWaves];      // per round and wave: the states that hold the k-th score
    uint32_t reached[kWaves];                  // the frame's reached states per wave
    uint32_t stop;                             // lane 0's verdict on the pass
};
// each kernel asserts on ALL its static LDS (this and its own reduction arrays) beside the largest rows; the dynamic
// rows start 16-byte aligned behind it
constexpr uint32_t kLdsBytes = 64 * 1024, kLdsAlign = 16;

// between two phases.  A single-wave segment needs no barrier: one wave's LDS operations complete in order, so the fence
// only keeps the compiler from moving them (kGlobal: the phases hand over global memory as well)
template <bool kWave, bool kGlobal = false>
__device__ __forceinline__ void sync() {
    if constexpr (kWave) {
        if constexpr (kGlobal)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        else
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

// minimumScore's step: result > score ? score : result (a NaN never enters)
__device__ __forceinline__ float minStep(float result, float score) {
    return result > score ? score : result;
}

// Core::isAlmostEqual(f32, f32) (src/Core/Utility.hh:316-321), left to right
__device__ __forceinline__ bool almostEqual(float a, float b) {
    const float d = fabsf(__fsub_rn(a, b));
    const float e = __fmul_rn(__fadd_rn(__fadd_rn(fabsf(a), fabsf(b)), FLT_MIN), FLT_EPSILON);
    return d < e;
}

// After a pass at `pruning` that gave (score, hypotheses), the `iterations`-th of the segment: true if it was the last.
// Otherwise `pruning` becomes the next threshold.  `previous` starts as FLT_MAX.
__device__ __forceinline__ bool searchStops(const AlignSearch& s, float score, uint32_t hypotheses, uint32_t nFrames,
                                            uint32_t iterations, float& previous, float& pruning) {
    if (s.factor <= 1.0f)
        return true;
    const bool ok = score != FLT_MAX &&
                    __ddiv_rn(static_cast<double>(hypotheses), static_cast<double>(nFrames)) >= s.minAverage;
    if (ok && (!s.untilNoDifference || (iterations > 1 && almostEqual(score, previous))))
        return true;
    previous         = score;
    const float next = __fmul_rn(pruning, s.factor);
    if (!(next <= s.maxPruning))
        return true;  // the schedule is exhausted: the outputs are this pass's
    pruning = next;
    return false;
}

// the order-preserving u32 image of a score: a < b as floats iff key(a) < key(b), -0 and +0 share one key
__device__ __forceinline__ uint32_t orderKey(float x) {
    uint32_t u = __float_as_uint(x);
    u          = u == 0x80000000u ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The n-best step of one frame; called by all T lanes with nBest below the number of reached states (marks != 0) of the
// row.  The scores and marks of the row are complete and each lane has written its own; `demoted` is threshold + 1.
template <bool kWave>
__device__ __forceinline__ void nBestStep(float* cur, const uint8_t* curMark, uint32_t n, uint32_t nBest, float demoted,
                                          SearchLds& s) {
    constexpr uint32_t T   = kWave ? 64u : kAlignThreads;
    const uint32_t     tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t* const    count = &s.count[0][0];
    for (uint32_t i = tid; i < kNBestPasses * kNBestBins; i += T)
        count[i] = 0;
    sync<kWave>();

    // select: after pass p the first 4 (p + 1) bits of the k-th smallest key; k counts inside the keys that share them
    uint32_t prefix = 0, k = nBest, equalCount = 0;
    for (uint32_t pass = 0; pass < kNBestPasses; ++pass) {
        const uint32_t shift = 28u - 4u * pass;
        const uint32_t above = pass ? 0xffffffffu << (shift + 4u) : 0u;  // the digits found so far
        for (uint32_t q = tid; q < n; q += T)
            if (curMark[q]) {
                const uint32_t key = orderKey(cur[q]);
                if ((key & above) == prefix)
                    atomicAdd(&s.count[pass][(key >> shift) & (kNBestBins - 1u)], 1u);
            }
        sync<kWave>();
        uint32_t before = 0, digit = kNBestBins - 1u, below = 0, at = 0;
        bool     found = false;
        for (uint32_t d = 0; d < kNBestBins; ++d) {
            const uint32_t c = s.count[pass][d];
            if (!found && before + c >= k) {
                found = true;
                digit = d;
                below = before;
                at    = c;
            }
            before += c;
        }
        // (found always: the keys that share the prefix are at least k)
        k -= found ? below : 0u;
        prefix |= digit << shift;
        equalCount = at;
    }
    // prefix: the k-th smallest key; of the equalCount states that hold it the first k stay, 1 <= k <= equalCount
    if (equalCount <= k) {
        for (uint32_t q = tid; q < n; q += T)
            if (curMark[q] && orderKey(cur[q]) > prefix)
                cur[q] = demoted;
        return;
    }
    // ties at the cut: the rank of a state among the holders of the k-th key, in state order
    const uint32_t rounds = (n + T - 1u) / T;  // at most kNBestRounds
    if constexpr (!kWave) {
        for (uint32_t r = 0, q = tid; r < rounds; ++r, q += T) {
            const bool               eq = q < n && curMark[q] && orderKey(cur[q]) == prefix;
            const unsigned long long mask = __ballot(eq);
            if (lane == 0)
                s.equal[r][wave] = static_cast<uint32_t>(__popcll(mask));
        }
        __syncthreads();
    }
    uint32_t running = 0;
    for (uint32_t r = 0, q = tid; r < rounds; ++r, q += T) {
        const bool               mine = q < n && curMark[q];
        const uint32_t           key  = mine ? orderKey(cur[q]) : 0u;
        const bool               eq   = mine && key == prefix;
        const unsigned long long mask = __ballot(eq);
        uint32_t                 rank = running + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
        if constexpr (kWave) {
            running += static_cast<uint32_t>(__popcll(mask));
        } else {
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint32_t c = s.equal[r][w];
                rank += w < wave ? c : 0u;
                running += c;
            }
        }
        if (mine && (key > prefix || (eq && rank >= k)))
            cur[q] = demoted;
    }
}

// The end of a frame step, behind the candidate loop of the mode: every lane has written the scores `cur` and reached
// marks `curMark` of its states and brings their minimum `mn` (minStep from FLT_MAX) and, in a search, their number.
// Reduces both across the lanes (shuffles inside a wave, redV and the search's LDS across the waves, one barrier), forms
// threshold = minimum + pruning and, in a search that reached more than n_best states, runs the n-best step.  Returns
// the threshold; the caller's keep loop clears the marks above it.
template <bool kWave, bool kSearch>
__device__ __forceinline__ float pruneThreshold(float mn, uint32_t nReached, float pruning, float* cur,
                                                const uint8_t* curMark, uint32_t n, uint32_t nBest, float* redV,
                                                SearchLds* s) {
    for (uint32_t d = 32; d; d >>= 1) {
        mn = minStep(mn, __shfl_xor(mn, d));
        if constexpr (kSearch)
            nReached += __shfl_xor(nReached, d);
    }
    if constexpr (!kWave) {
        const uint32_t wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63u) == 0) {
            redV[wave] = mn;
            if constexpr (kSearch)
                s->reached[wave] = nReached;
        }
        __syncthreads();
        mn = FLT_MAX;
        for (uint32_t w = 0; w < kWaves; ++w)
            mn = minStep(mn, redV[w]);
        if constexpr (kSearch) {
            nReached = 0;
            for (uint32_t w = 0; w < kWaves; ++w)
                nReached += s->reached[w];
        }
    }
    const float threshold = __fadd_rn(mn, pruning);
    if constexpr (kSearch) {
        // uniform over the workgroup: every lane holds the same count
        if (nBest < nReached)
            nBestStep<kWave>(cur, curMark, n, nBest, __fadd_rn(threshold, 1.0f), *s);
    }
    return threshold;
}

// the lanes' counts of kept hypotheses, summed over the wave and, through red[kWaves] and one barrier, the workgroup
// (the sweep's; the Viterbi kernel's sum rides on the barrier of its final scan)
template <bool kWave>
__device__ __forceinline__ uint32_t sumHypotheses(uint32_t hypotheses, uint32_t* red) {
    for (uint32_t d = 32; d; d >>= 1)
        hypotheses += __shfl_xor(hypotheses, d);
    if constexpr (!kWave) {
        if ((threadIdx.x & 63u) == 0)
            red[threadIdx.x >> 6] = hypotheses;
        __syncthreads();
        hypotheses = 0;
        for (uint32_t w = 0; w < kWaves; ++w)
            hypotheses += red[w];
    }
    return hypotheses;
}

// The end of a search pass at `pruning`, called by all lanes.  kEveryLane (one wave whose lanes all hold the pass's score
// and hypotheses): every lane decides alike (searchStops), without LDS.  Otherwise (score, hypotheses) are lane 0's: it
// decides (`previous` is its own) and hands the verdict over in LDS; the other lanes' next threshold is the same one f32
// product of values every lane holds.  After the last pass lane 0 writes the segment's threshold and iterations.
// Returns whether the pass was the last.
template <bool kWave, bool kEveryLane>
__device__ __forceinline__ bool searchPassEnds(const AlignSearchCall& sc, SearchLds& s, uint32_t segment, float score,
                                               uint32_t hypotheses, uint32_t nFrames, uint32_t& iterations,
                                               float& previous, float& pruning) {
    static_assert(kWave || !kEveryLane, "only a single wave decides in every lane");
    const float at = pruning;
    ++iterations;
    bool stop;
    if constexpr (kEveryLane) {
        stop = searchStops(sc.rule, score, hypotheses, nFrames, iterations, previous, pruning);
    } else {
        if (threadIdx.x == 0)
            s.stop = searchStops(sc.rule, score, hypotheses, nFrames, iterations, previous, pruning);
        sync<kWave>();
        stop = s.stop != 0;
        if (!stop && threadIdx.x != 0)
            pruning = __fmul_rn(pruning, sc.rule.factor);
    }
    if (stop && threadIdx.x == 0) {
        if (sc.outThreshold)
            sc.outThreshold[segment] = at;
        if (sc.outIterations)
            sc.outIterations[segment] = iterations;
    }
    return stop;
}

}  // namespace dev
}  // namespace rasr_gmm
