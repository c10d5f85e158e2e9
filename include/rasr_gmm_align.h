/*
 * rasr_gmm_align.h -- Viterbi time alignment of a batch of segments over a score table ON THE DEVICE (C-ABI).
 *
 * gmm_score_device fills a mixture-major score table; the estimator, EBW, CMLLR and MLLR handles take (frame, mixture)
 * pairs as device pointers.  This handle is the step between them: for every segment of a batch it aligns the segment's
 * automaton against the segment's columns of the table and writes one mixture index per column, which goes straight
 * into gmm_estimator_accumulate_device and its siblings (pair_frame = 0, 1, 2, ..., pair_mixture = out_mixture).
 * Replaces Search::Aligner in Viterbi mode with acoustic pruning:
 *   Aligner::SearchSpace::addStartupHypothesis                    src/Search/Aligner.cc:189-204
 *   Aligner::SearchSpace::expand                                  src/Search/Aligner.cc:206-243
 *   Aligner::SearchSpace::activateOrUpdateStateHypothesisViterbi  src/Search/Aligner.cc:135-158
 *   Aligner::SearchSpace::minimumScore, prune (threshold only)    src/Search/Aligner.cc:245-309
 *   Aligner::feed(Scorer)                                         src/Search/Aligner.cc:585-592
 *   Aligner::SearchSpace::finalStatePotential                     src/Search/Aligner.cc:376-396
 *   Aligner::SearchSpace::getAlignmentFsaViterbi                  src/Search/Aligner.cc:398-436
 * Baum-Welch mode (the per-frame mixture posteriors) is gmm_aligner_posteriors_*, described further down; the
 * threshold-increase loop of feed(vector) and n-best pruning are the gmm_aligner_*_search_* calls at the end.
 * Not covered: per-frame local scores, building
 * the automata from a lexicon or from allophone states, word lattices, a RASR-side adapter.
 *
 * THE MODEL.  A segment has an automaton: states, arcs (target, emission label = a mixture index, f32 weight), an
 * initial state, and a f32 final weight per state (+inf: not final).  An arc consumes one frame; n frames give a path
 * of exactly n arcs from the initial state to a final state.  All scores are costs (-log): smaller is better.
 *
 * THE NUMERIC CONTRACT: every operation is one IEEE f32 rounding, nothing is contracted into an fma, and the result is
 * the same bit for bit for every batch composition, launch geometry and run.  "Active" is a property of a state of its
 * own, never a sentinel score: +inf, FLT_MAX and NaN are legal scores and get what the comparisons below give.
 *   start      before frame 0 only the initial state is active, with score 0.0f.
 *   expand     frame t, state q: the candidates of q are its incoming arcs a = (p -> q, mixture m, weight w) from states
 *              p active after frame t-1, in the order (p ascending, position of a among p's arcs ascending); each is
 *                  cand = (score(p) + w) + table[m][frame_begin + t]         added left to right
 *              The first candidate initialises q's score; a later one replaces it iff current >= cand (a later equal
 *              candidate wins).  q is reached iff it has a candidate.
 *   prune      min = FLT_MAX; for every reached q: if (min > score(q)) min = score(q);
 *              threshold = min + pruning_threshold;  q is active after frame t iff it is reached and
 *              score(q) <= threshold.  FLT_MAX or +inf as pruning_threshold keep everything, by this arithmetic.
 *              The segment's hypothesis count adds the number of active states of every frame.
 *   end        after the last frame: best = FLT_MAX; for the active q in ascending order: v = final_weight(q) + score(q);
 *              if (v < best) { best = v; end state = q }  (the first of equals wins).  best is the segment's score;
 *              if no v is below FLT_MAX the segment has no alignment.  Otherwise the path is traced back from the end
 *              state along the winning candidates.
 * Scores: the per-state scores, the pruning decisions and the final score equal the reference's on every automaton:
 * they are minima of the same f32 values (NaN aside, whose fate depends on the order of the candidates).
 * Paths: the reference walks its hypothesis LIST of the previous frame, and each state's arcs, in order; the list is in
 * first-activation order.  Wherever that list is in ascending state order in every frame the candidates of a state
 * arrive in exactly the order above, and the path (and every NaN) equals the reference's.  That holds for INTERVAL
 * GRAPHS: every state's arcs are listed by ascending target, its targets cover a contiguous interval [lo_p, hi_p], and
 * lo and hi do not decrease with p -- every left-to-right loop / forward / skip HMM is one (DESIGN.md section 16 has
 * the induction).  On other automata exact ties are broken by the order stated here; the path found is still one of
 * the optimal paths.  tests/aligner_restatement.py restates both orders.
 *
 * Errors as in rasr_gmm.h: a negative status, the message via gmm_last_error().
 */
#ifndef RASR_GMM_ALIGN_H
#define RASR_GMM_ALIGN_H

#include <stdint.h>

#include "rasr_gmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The most states one segment may have.  A workgroup keeps two f32 score rows and two rows of active marks (a byte per
 * state) in LDS, double-buffered over the frames: 10 bytes per state out of the 64 KiB a workgroup takes without asking
 * for more, 4 KiB of which stay free for the reductions.  (64 KiB - 4 KiB) / 10 = 6144. */
#define GMM_ALIGN_MAX_STATES 6144

/* The most states of a segment in a Baum-Welch (posteriors) call.  Its workgroup keeps two f64 potential rows beside the
 * two f32 score rows and the two rows of marks: 26 bytes per state, in rows rounded up to 64 states, out of the same
 * 64 KiB, 1 KiB of which stays free for the reductions.  (64 KiB - 1 KiB) / 26 = 2481, in whole rows of 64: 2432. */
#define GMM_ALIGN_MAX_STATES_POSTERIOR 2432

/* The most arcs that may enter one state: a backpointer keeps the arc's ordinal in the state's incoming list in 16
 * bits. */
#define GMM_ALIGN_MAX_IN_ARCS 65535

/* The value of every per-frame output of a segment without an alignment (the accumulate calls skip and count it). */
#define GMM_ALIGN_NONE 0xffffffffu

typedef struct gmm_aligner gmm_aligner;

/* A batch of segments, HOST arrays; the automata are concatenated.  n_states = state_offset[n_segments], n_arcs =
 * arc_offset[n_states]. */
typedef struct gmm_align_graphs {
    uint32_t        n_segments;
    const uint32_t* state_offset;  /* [n_segments + 1] from 0: segment s owns the states state_offset[s] .. [s+1]   */
    const uint32_t* arc_offset;    /* [n_states + 1] from 0: CSR by (global) source state                            */
    const uint32_t* arc_target;    /* [n_arcs] the target, a state index LOCAL to the arc's segment                  */
    const uint32_t* arc_mixture;   /* [n_arcs] the emission label: a row of the score table                          */
    const float*    arc_weight;    /* [n_arcs]                                                                       */
    const uint32_t* initial_state; /* [n_segments] local index, or NULL: local state 0 everywhere                    */
    const float*    final_weight;  /* [n_states]; +inf: not a final state                                            */
    const uint32_t* frame_begin;   /* [n_segments] the segment's first column of the score table                     */
    const uint32_t* n_frames;      /* [n_segments] its number of columns, >= 1                                       */
} gmm_align_graphs;

/* All device memory of the handle, for batches of up to max_segments segments, max_states states and max_arcs arcs in
 * all, over a table of n_mixtures rows; max_cells bounds the sum over the segments of n_frames * n_states of one batch
 * (the backpointer scratch, 4 bytes a cell).  Later calls allocate nothing.  GMM_ERR_INVALID_ARGUMENT for a zero
 * capacity or n_mixtures == 0. */
int gmm_aligner_create(uint32_t max_segments, uint32_t max_states, uint32_t max_arcs, uint64_t max_cells,
                       uint32_t n_mixtures, int device, gmm_aligner** out);
/* Waits for the last call on the handle. */
int gmm_aligner_destroy(gmm_aligner* aligner);

/* Sets the batch the following align calls work on; synchronous (it waits for the last align call first).  Everything
 * is validated before anything changes, so a refused call leaves the previously set segments in place:
 *   GMM_ERR_INVALID_ARGUMENT  a NULL array; offsets that do not start at 0 or decrease; a segment without states; an
 *                             initial state or a target outside the segment; a mixture >= n_mixtures; n_frames == 0;
 *                             frame ranges that overlap (the outputs are indexed by table column) or end past 2^32
 *   GMM_ERR_CAPACITY          more segments, states, arcs or cells than the handle was created for
 *   GMM_ERR_UNSUPPORTED       a segment of more than GMM_ALIGN_MAX_STATES states, a state entered by more than
 *                             GMM_ALIGN_MAX_IN_ARCS arcs, a segment of 2^32 cells or more
 * It builds and uploads the incoming-arc lists per target state, ordered by (source state, arc position). */
int gmm_aligner_set_segments(gmm_aligner* aligner, const gmm_align_graphs* graphs);

/* Aligns every segment of the batch.  All pointers are DEVICE pointers; the call is enqueued on `stream` (a hipStream_t;
 * NULL = default stream), synchronizes nothing and allocates nothing.
 *   scores             [n_mixtures][score_stride] f32, as gmm_score_device writes it; n_table_frames columns are valid
 *   pruning_threshold  the reference's acousticPruningThreshold_
 *   out_mixture, out_state, out_arc   [n_table_frames] u32 each, any may be NULL: for column frame_begin[s] + t the arc
 *                      taken on frame t of segment s -- its mixture, its target state (local) and its index in the
 *                      batch's arc arrays.  Columns of no segment are never written; every column of a segment without
 *                      an alignment holds GMM_ALIGN_NONE
 *   out_score          [n_segments] f32 or NULL: alignmentScore(), FLT_MAX without an alignment
 *   out_hypotheses     [n_segments] u32 or NULL: the sum over the frames of the active states (the statistic behind
 *                      min-average-number-of-state-hypotheses)
 * Errors, each before anything is written: GMM_ERR_INVALID_ARGUMENT for NULL scores, score_stride < n_table_frames, a
 * segment that ends past n_table_frames, every output NULL, or no segments set.
 * The call uses the handle's scratch: calls on one handle are made on one stream, or ordered by the caller. */
int gmm_aligner_align_device(gmm_aligner* aligner, const float* scores, uint32_t n_table_frames, uint32_t score_stride,
                             float pruning_threshold, uint32_t* out_mixture, uint32_t* out_state, uint32_t* out_arc,
                             float* out_score, uint32_t* out_hypotheses, void* stream);

/* The same call from a HOST table into HOST outputs: copies the table in, aligns, copies the outputs out; synchronous.
 * Columns of no segment keep what the host arrays held. */
int gmm_aligner_align_host(gmm_aligner* aligner, const float* scores, uint32_t n_table_frames, uint32_t score_stride,
                           float pruning_threshold, uint32_t* out_mixture, uint32_t* out_state, uint32_t* out_arc,
                           float* out_score, uint32_t* out_hypotheses);

/*
 * BAUM-WELCH MODE: per-frame mixture posteriors of the batch set by gmm_aligner_set_segments.  Replaces Search::Aligner
 * in baum-welch mode with acoustic pruning, up to the normalised alignment items:
 *   Aligner::SearchSpace::activateOrUpdateStateHypothesisBaumWelch, expand, prune   src/Search/Aligner.cc:160-187, 206-309
 *   Aligner::SearchSpace::finalStatePotential, getAlignmentFsaBaumWelch             src/Search/Aligner.cc:376-396, 438-452
 *   Aligner::getAlignment, getAlignmentPosteriorFsa                                 src/Search/Aligner.cc:696-779
 *   Fsa::posterior64                                                                src/Fsa/Sssp.cc:67-222
 *   LogSemiring::collect                                                            src/Fsa/tRealSemiring.cc:130-146
 *   Alignment::combineItems .. filterWeightsGT                                      src/Speech/Alignment.cc:442-578
 * Not covered: use-partial-sums, a positive min-weight (the arc-level prunePosterior), gamma scaling, the
 * state-posteriors statistics channel, a RASR-side adapter.
 *
 * THE NUMERIC CONTRACT of this mode.  Every f32 or f64 add, subtract, multiply and divide is one correctly rounded
 * operation, nothing is contracted; every exp and log1p is evaluated in f64 on the exactly widened argument and, in an
 * f32 step, its value is rounded once to f32.  The result is the same bit for bit for every batch composition, launch
 * geometry and run (no floating-point atomics).  Defined for finite table entries, arc weights and final weights (+inf
 * as a final weight: not final); for other inputs the result is unspecified, the call stays in bounds and terminates.
 *   collect(a, b)  f32: b == FLT_MAX -> a; a == FLT_MAX -> b; else with lo = min(a, b), hi = max(a, b):
 *                  lo - f32(log1p(exp(f64(lo - hi))))          (FLT_MAX is the log semiring's zero)
 *   1 search   f32.  Start as in Viterbi mode.  Frame t, state q: over the incoming arcs (p -> q, m, w) from the states p
 *              active after frame t-1, in (p ascending, arc position ascending) order:
 *                  arcScore = w + table[m][frame_begin + t];   cand = score(p) + arcScore
 *              the first candidate initialises score(q), a later one gives score(q) = collect(score(q), cand).
 *              prune: exactly Viterbi mode's, on these scores; so is the hypothesis count.
 *              end: result = FLT_MAX; for the active q with a final weight below +inf, ascending: v = final_weight(q) +
 *              score(q); result = (result == FLT_MAX) ? v : collect(result, v).  The segment HAS AN ALIGNMENT iff there is
 *              such a q; otherwise it has no items, out_score = FLT_MAX and out_log_total = DBL_MAX.
 *   2 trellis  nodes: the initial state before frame 0 and every (t, q) with q active after frame t; arcs: (t-1, p) ->
 *              (t, q) for every arc p -> q with both ends nodes, with the f32 weight arcScore.
 *   3 potentials, f64, zero = DBL_MAX.  extend(x, s) = x + f64(s), an infinity replaced by DBL_MAX.  The batch form over
 *              values v_1 .. v_k in a stated order: min = DBL_MAX, and for i = 1 .. k: if (v_i <= min) min = v_i, i* = i;
 *              sum = 0, and for i != i*, in order: sum += exp(min - v_i);  potential = min - log1p(sum), DBL_MAX if that
 *              is not below DBL_MAX.
 *              fw(initial) = 0;  fw(t, q): over the trellis arcs into (t, q) in (p, arc position) order, v = extend(fw(t-1,
 *              p), arcScore).   bw(T-1, q) = f64(final_weight(q)) if that is below +inf, else DBL_MAX;  bw(t, p), and
 *              bw(initial): over the trellis arcs out of the node in arc order, v = extend(bw(t+1, q), arcScore).
 *              out_log_total = bw(initial).  A node that reaches no final state keeps DBL_MAX.
 *              An arc's log posterior: x = ((fw(source) + f64(arcScore)) + bw(target)) + (-bw(initial)), left to right in
 *              f64; lp = f32(x) if x < FLT_MAX, else FLT_MAX.
 *   4 items    per (column, mixture) that has a trellis arc: the lp of its arcs collected, in (source state, arc position)
 *              order, the first initialising; clipped to [0, FLT_MAX].  Per column: min = FLT_MAX, lowered by every item
 *              below it; w = lp - min; w = f32(exp(f64(-w))), 0 for an infinite w; sum = 0.0f + the w in ascending
 *              mixture order; inv = 1.0f / sum, or 1 if the sum is 0; weight = w * inv.  An item is kept iff
 *              weight > min_posterior; nothing is renormalised after that.
 * Against the reference this fixes two orders that its std::sort leaves open (the order in which equal (time, emission)
 * items are collected, and the one in which a frame's weights are summed) and evaluates the f32 steps' exp and log1p
 * through f64; DESIGN.md section 17 bounds both.  tests/aligner_posterior_restatement.py restates this contract.
 */

/* The Baum-Welch call.  All pointers are DEVICE pointers; enqueued on `stream`, no synchronisation.  The FIRST posterior
 * call on a handle allocates the posterior scratch, sized from the capacities given at creation (per cell two f64
 * potentials and a mark; per frame 12 bytes, max_cells of them; min(n_mixtures, max_arcs) f32 for each of 1024 waves;
 * the arcs as given and grouped by mixture), and uploads the batch's tables for this mode; later calls allocate nothing,
 * and a later gmm_aligner_set_segments uploads them itself.  (set_segments builds them on the host with every batch.)
 *   scores, n_table_frames, score_stride, pruning_threshold, stream     as for gmm_aligner_align_device
 *   min_posterior      keep an item iff weight > min_posterior; 0 is the reference's filterWeightsGT(0.0)
 *   max_items          the capacity of the three item arrays
 *   out_item_frame, out_item_mixture [max_items] u32, out_item_weight [max_items] f64 (each holds a f32 value exactly):
 *                      the compact list of the kept items, ordered by (table column, mixture) ascending; all three or
 *                      none.  As they stand they are pair_frame, pair_mixture and pair_weight of
 *                      gmm_estimator_accumulate_posteriors_device and its siblings
 *   out_column_offset  [n_table_frames + 1] u32 or NULL: CSR into the list by table column; columns of no segment and of
 *                      a segment without an alignment are empty
 *   out_n_items        one u32 or NULL: the number of items the call produces.  Above max_items nothing past max_items is
 *                      written, the list is invalid, the count is still exact
 *   out_score          [n_segments] f32 or NULL: the Baum-Welch alignmentScore(), FLT_MAX without an alignment
 *   out_hypotheses     [n_segments] u32 or NULL: as in the Viterbi call
 *   out_log_total      [n_segments] f64 or NULL: bw(initial), DBL_MAX without an alignment
 * Errors, each before anything is written: GMM_ERR_INVALID_ARGUMENT as for the align call, and for some but not all of
 * the item arrays, or item arrays with max_items == 0; GMM_ERR_UNSUPPORTED for a segment of more than
 * GMM_ALIGN_MAX_STATES_POSTERIOR states. */
int gmm_aligner_posteriors_device(gmm_aligner* aligner, const float* scores, uint32_t n_table_frames,
                                  uint32_t score_stride, float pruning_threshold, float min_posterior, uint32_t max_items,
                                  uint32_t* out_item_frame, uint32_t* out_item_mixture, double* out_item_weight,
                                  uint32_t* out_column_offset, uint32_t* out_n_items, float* out_score,
                                  uint32_t* out_hypotheses, double* out_log_total, void* stream);

/* The same call from a HOST table into HOST outputs; synchronous.  GMM_ERR_CAPACITY if the call produces more than
 * max_items items: *out_n_items and the per-segment outputs are then still written, the item arrays and
 * out_column_offset are not. */
int gmm_aligner_posteriors_host(gmm_aligner* aligner, const float* scores, uint32_t n_table_frames, uint32_t score_stride,
                                float pruning_threshold, float min_posterior, uint32_t max_items, uint32_t* out_item_frame,
                                uint32_t* out_item_mixture, double* out_item_weight, uint32_t* out_column_offset,
                                uint32_t* out_n_items, float* out_score, uint32_t* out_hypotheses, double* out_log_total);

/*
 * THE SEARCH: the pruning-threshold search of Search::Aligner::feed(vector) and the n-best pruning of prune, in both
 * modes, inside the one call:
 *   Aligner::feed(const std::vector<Scorer>&)                     src/Search/Aligner.cc:594-621
 *   Aligner::SearchSpace::prune (n-best)                          src/Search/Aligner.cc:254-276
 *   Core::isAlmostEqual(f32, f32)                                 src/Core/Utility.hh:316-321
 * THE NUMERIC CONTRACT: f32, every operation one rounding, the result the same bit for bit for every batch composition,
 * launch geometry and run (the only atomics are integer counts).  Per segment, independently of the others:
 *   schedule   t = min_pruning; the next t = t * increment_factor, one f32 multiply.  A pass runs while t <= max_pruning.
 *   a pass     the fixed-threshold contract above from `start` to `end` (in Baum-Welch mode: step 1, the f32 search) with
 *              pruning_threshold = t and the n-best step below in `prune`.  It gives score (the value of out_score) and
 *              hypotheses, counted from 0 in every pass.
 *   after it   1  if increment_factor <= 1: stop.
 *              2  ok = (score != FLT_MAX) && ((double)hypotheses / (double)n_frames >= min_average_hypotheses)
 *              3  if ok and !until_no_score_difference: stop.
 *              4  if ok, this is not the first pass, and almost_equal(score, previous): stop.
 *              5  otherwise previous = score (it starts as FLT_MAX) and the next threshold follows.
 *              almost_equal(a, b) = fabsf(a - b) < ((fabsf(a) + fabsf(b)) + FLT_MIN) * FLT_EPSILON, left to right.
 *   outputs    those of the last pass run, also when the schedule is exhausted: a segment that never reached a final
 *              state then has GMM_ALIGN_NONE columns, FLT_MAX and no items.  out_threshold is that pass's t,
 *              out_iterations the number of passes.  In Baum-Welch mode steps 2 to 4 are those of the last pass.
 *   n-best     in `prune`, with R the number of reached states of the frame.  min and threshold = min + t are formed
 *              first, over all reached states.  If n_best < R: with the reached states ordered by (score ascending,
 *              state index ascending; -0 equals +0), every state behind the first n_best gets score = threshold + 1.0f
 *              (one f32 add), which stays its score if it survives.  Then, as before, a state is active iff
 *              score <= threshold: the demoted states go while threshold + 1 > threshold in f32 (always below 2^24);
 *              where the sum rounds back to threshold (always from 2^25 on, and between 2^24 and 2^25 for every second
 *              value, a tie rounding to even) they stay with the new score, as in the reference.  The reference's std::nth_element leaves open which of
 *              several equal scores at the cut survive; the state order closes that, and the result is the reference's
 *              wherever the n_best-th and the next score differ.  With NaN scores the step is unspecified; the call
 *              stays in bounds and terminates.
 * tests/aligner_search_restatement.py restates this contract.
 */

/* The most thresholds a schedule may have.  From FLT_MIN to FLT_MAX with a factor of 2 there are 254, so no configuration
 * with a factor of 2 or more is refused; a finite max_pruning and this cap bound the running time of every kernel (a
 * factor of 1 + 2^-23 would otherwise run up to 2^31 passes). */
#define GMM_ALIGN_MAX_ITERATIONS 256

typedef struct gmm_align_search {
    float    min_pruning;               /* min-acoustic-pruning,  default 50           */
    float    max_pruning;               /* max-acoustic-pruning,  default FLT_MAX      */
    float    increment_factor;          /* acoustic-pruning-increment-factor, default 2 */
    double   min_average_hypotheses;    /* min-average-number-of-states, default 0     */
    int      until_no_score_difference; /* increase-pruning-until-no-score-difference, default 1 */
    uint32_t n_best;                    /* n-best-pruning, default 0x7fffffff          */
} gmm_align_search;

/* The reference's defaults, as listed. */
void gmm_default_align_search(gmm_align_search* search);

/* gmm_aligner_align_device / _host with the search in place of pruning_threshold, and two more per-segment outputs,
 * either of which may be NULL (they do not count as "an output requested"):
 *   out_threshold   [n_segments] f32: the threshold of the last pass
 *   out_iterations  [n_segments] u32: the number of passes
 * The device call still synchronizes nothing and allocates nothing.  Beyond the errors of the sibling call,
 * GMM_ERR_INVALID_ARGUMENT before anything is written for: a NULL search; a NaN in any field; min_pruning < FLT_MIN;
 * max_pruning not finite; min_pruning > max_pruning; increment_factor <= 1 with min_pruning != max_pruning (the
 * reference's criticalError); n_best == 0; a schedule of more than GMM_ALIGN_MAX_ITERATIONS thresholds. */
int gmm_aligner_align_search_device(gmm_aligner* aligner, const float* scores, uint32_t n_table_frames,
                                    uint32_t score_stride, const gmm_align_search* search, uint32_t* out_mixture,
                                    uint32_t* out_state, uint32_t* out_arc, float* out_score, uint32_t* out_hypotheses,
                                    float* out_threshold, uint32_t* out_iterations, void* stream);
int gmm_aligner_align_search_host(gmm_aligner* aligner, const float* scores, uint32_t n_table_frames,
                                  uint32_t score_stride, const gmm_align_search* search, uint32_t* out_mixture,
                                  uint32_t* out_state, uint32_t* out_arc, float* out_score, uint32_t* out_hypotheses,
                                  float* out_threshold, uint32_t* out_iterations);

/* gmm_aligner_posteriors_device / _host likewise; the first-use allocation of the Baum-Welch mode is the same one. */
int gmm_aligner_posteriors_search_device(gmm_aligner* aligner, const float* scores, uint32_t n_table_frames,
                                         uint32_t score_stride, const gmm_align_search* search, float min_posterior,
                                         uint32_t max_items, uint32_t* out_item_frame, uint32_t* out_item_mixture,
                                         double* out_item_weight, uint32_t* out_column_offset, uint32_t* out_n_items,
                                         float* out_score, uint32_t* out_hypotheses, double* out_log_total,
                                         float* out_threshold, uint32_t* out_iterations, void* stream);
int gmm_aligner_posteriors_search_host(gmm_aligner* aligner, const float* scores, uint32_t n_table_frames,
                                       uint32_t score_stride, const gmm_align_search* search, float min_posterior,
                                       uint32_t max_items, uint32_t* out_item_frame, uint32_t* out_item_mixture,
                                       double* out_item_weight, uint32_t* out_column_offset, uint32_t* out_n_items,
                                       float* out_score, uint32_t* out_hypotheses, double* out_log_total,
                                       float* out_threshold, uint32_t* out_iterations);

#ifdef __cplusplus
}
#endif

#endif /* RASR_GMM_ALIGN_H */
