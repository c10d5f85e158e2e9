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
 * Not covered: Baum-Welch mode (the arc posteriors), n-best pruning, the threshold-increase loop of
 * feed(vector) -- out_score and out_hypotheses are what a caller needs to run it --, per-frame local scores, building
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

#ifdef __cplusplus
}
#endif

#endif /* RASR_GMM_ALIGN_H */
