/*
 * rasr_gmm_mllr.h -- MLLR mean transforms of speaker adaptation (C-ABI): accumulation per (speaker key, regression
 * leaf) ON THE DEVICE, the estimation of one matrix per regression class over a binary tree on the host, and the
 * adapted means, which go straight back into gmm_scorer_create as a new mixture set.
 *
 * Aligned (frame, mixture) pairs, a density per pair and a weight -- what rasr_gmm.h and rasr_gmm_estimator.h already
 * produce on the device -- are accumulated into the f64 statistics of Mm::FullAdaptorViterbiEstimator and
 * Mm::ShiftAdaptorViterbiEstimator, one set of tables per (key, leaf), n_keys * n_leaves sets side by side.  Replaces
 *   FullAdaptorViterbiEstimator::accumulate (weighted)    src/Mm/MllrAdaptation.cc:599-653, 704-714
 *   ShiftAdaptorViterbiEstimator::accumulate (weighted)   src/Mm/MllrAdaptation.cc:399-416
 *   AccumulatorBase::operator+=                           src/Mm/MllrAdaptation.cc:274-277
 *   AdaptorEstimator::propagate                           src/Mm/MllrAdaptation.hh:223-242
 *   estimateWMatrices, adaptor()                          src/Mm/MllrAdaptation.cc:358-379, 444-531, 671-827
 *   FullAdaptor / ShiftAdaptor::adaptMixtureSet           src/Mm/MllrAdaptation.cc:146-170, 59-79
 * Not covered: BandMllrAdaptation, SemiTiedAdaptation, the binary estimator and adaptor files (read / write),
 * ShiftAdaptor's pre-adaptor form, building the tree from a CART, a RASR-side adapter.
 *
 * THE TABLES of one (key, leaf), D the dimension of the mixture set:
 *   full kind (GMM_MLLR_FULL)     Z [D][D+1]     sum of w * x m^T
 *                                 G [D+1][D+1]   sum of w * m m^T, the FULL matrix: its two triangles round differently
 *                                 count          the number of pairs (count_++: not the weight)
 *   shift kind (GMM_MLLR_SHIFT)   count          the summed weight
 *                                 beta  [D]      sum of w / v
 *                                 shift [D]      sum of w * (x - mu) / v
 * with x the feature, m = (1, mu_0, ..., mu_{D-1}) the extended mean and v the diagonal covariance of the pair's
 * density.
 *
 * THE NUMERIC CONTRACT: deterministic order, no floating-point atomics -- rasr_gmm_adaptation.h's, per (key, leaf).
 * With x_i = (f64) of the f32 feature, m_j = (f64) of the f32 mean (m_0 = 1.0), v_d = (f64) of the f32 variance, w the
 * pair's f64 weight, every operation rounded once in IEEE f64 and nothing fused, a pair updates, in the reference's
 * operand order,
 *     Z[i][j]  = Z[i][j]  + ((w * x_i) * m_j)                       cc:615-619
 *     G[i][j]  = G[i][j]  + ((w * m_i) * m_j)                       cc:648-652   all (D+1)^2 cells, no mirroring
 *     count    = count + 1.0                                        full kind: per pair
 *     count    = count + w                                          shift kind, cc:410
 *     beta[d]  = beta[d]  + (w / v_d)                               cc:412
 *     shift[d] = shift[d] + ((w * (f64)(x_d -f32 mu_d)) / v_d)      cc:413-414
 * The shift difference is the f32 subtraction of the two f32 values, widened afterwards.  The divisions are
 * divisions: never a multiplication by a stored reciprocal.  NULL weights are the weighted form with w = 1.0: for the
 * full kind that equals the reference's unweighted text exactly; for the shift kind the unweighted text divides in f32
 * (cc:393-395, 438-439), which is NOT what a NULL weight computes here -- the weighted form is the contract.
 * The set (key, leaf of the pair's mixture) receives its non-skipped pairs in pair order.  With more than
 * GMM_MLLR_CHUNK pairs of one (key, leaf) in a call, they are cut into consecutive pieces of GMM_MLLR_CHUNK; piece 0
 * is accumulated onto the current value, every later piece from 0, and the later pieces' results are then added in
 * piece order.  The result depends neither on the launch geometry nor on the run; tests/mllr_restatement.py restates
 * it in numpy.
 * The reference binary is built with -ffast-math: as in rasr_gmm_adaptation.h the reference's text in the STATED order
 * is the contract, not the bits of one build of it.
 *
 * Errors as in rasr_gmm.h: a negative status, the message via gmm_last_error().
 */
#ifndef RASR_GMM_MLLR_H
#define RASR_GMM_MLLR_H

#include <stdint.h>

#include "rasr_gmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs per piece of one (key, leaf) in one call; part of the numeric contract above. */
#define GMM_MLLR_CHUNK 512

/* The largest dimension a handle takes (the kernel stages a batch of pairs in LDS). */
#define GMM_MLLR_MAX_DIMENSION 256

/* The kinds of statistics: a bit mask for gmm_mllr_create, one of them for gmm_mllr_estimate / gmm_mllr_adapt_means. */
#define GMM_MLLR_FULL 1
#define GMM_MLLR_SHIFT 2

/* "None" in the tree arrays of gmm_mllr_estimate (Core::BinaryTree::invalidId). */
#define GMM_MLLR_NO_ID 0xffffffffu

typedef struct gmm_mllr_accumulator gmm_mllr_accumulator;

/* n_keys * n_leaves sets of zeroed f64 tables of the kinds in `kinds` on `device` for the model `set` (its dimension,
 * means, variances and the density -> mean / covariance and mixture tables are copied), and the scratch of a call of up
 * to max_pairs pairs.  leaf_of_mixture[n_mixtures] is the reference's leafIndex_: the regression leaf of every
 * mixture; n_leaves may exceed the number of leaves of any tree (the reference appends a silence leaf outside the
 * tree, src/Am/AdaptationTree.cc:94-98).  The size -- the tables, the later pieces' slabs of a max_pairs call and the
 * pair scratch -- is computed before anything is allocated: a handle past three quarters of the device's free memory is
 * GMM_ERR_UNSUPPORTED, and the message names the size.  GMM_ERR_UNSUPPORTED also for D > GMM_MLLR_MAX_DIMENSION;
 * GMM_ERR_INVALID_ARGUMENT for n_keys == 0, n_leaves == 0, kinds == 0 (or bits beyond the two kinds), D == 0, a leaf
 * index >= n_leaves or model indices out of range. */
int gmm_mllr_create(const gmm_mixture_set* set, const uint32_t* leaf_of_mixture, uint32_t n_leaves, uint32_t n_keys,
                    int kinds, uint32_t max_pairs, int device, gmm_mllr_accumulator** out);
int gmm_mllr_destroy(gmm_mllr_accumulator* acc);

/* Zeroes all tables and the skipped count. */
int gmm_mllr_reset(gmm_mllr_accumulator* acc);

/* accumulate(feature, density, mixture, mixtureSet, weight) for a list of pairs: pair i adds frame pair_frame[i] (row at
 * frames + pair_frame[i] * frame_stride floats) with weight pair_weight[i] (f64; NULL: weight 1.0) and one density of
 * mixture pair_mixture[i] to the tables of (pair_key[i] (NULL: key 0), leaf_of_mixture[pair_mixture[i]]).
 * The arguments, the density resolution, the skipping rules and the errors are exactly those of
 * gmm_affine_accumulate_device (rasr_gmm_adaptation.h):
 *   pair_density != NULL            the in-mixture index pair_density[i]; `scorer` is ignored;
 *   else scorer != NULL             the scorer's best density of the pair (gmm_best_density_pairs_device's kernel, on
 *                                   the same stream);
 *   else                            every mixture must hold exactly one density: GMM_ERR_INVALID_ARGUMENT otherwise.
 * A pair is skipped and counted (gmm_mllr_skipped), and its frame is never read, when its frame, mixture, density or
 * key is out of range or the scorer answers 0xffffffff.
 * All pointers are DEVICE pointers; the call is enqueued on `stream` (a hipStream_t; NULL = default stream), does not
 * synchronize the host and allocates nothing.
 * Errors: GMM_ERR_CAPACITY for n_pairs > max_pairs; GMM_ERR_UNSUPPORTED for a scorer on another device, on a mixture
 * shard, density-sharded, or of a type without the pairs kernel; GMM_ERR_INVALID_ARGUMENT for a scorer whose
 * dimension, mixture count or entry count differs from the set's.  A refused call changes nothing.
 * The call uses the handle's scratch: calls on one handle are made from one thread and on one stream, or ordered by
 * the caller. */
int gmm_mllr_accumulate_device(gmm_mllr_accumulator* acc, gmm_scorer* scorer, const float* frames, uint32_t n_frames,
                               uint32_t frame_stride, const uint32_t* pair_frame, const uint32_t* pair_mixture,
                               const uint32_t* pair_density, const double* pair_weight, const uint32_t* pair_key,
                               uint32_t n_pairs, void* stream);

/* The same call with HOST arrays: copies them in and is synchronous. */
int gmm_mllr_accumulate_host(gmm_mllr_accumulator* acc, gmm_scorer* scorer, const float* frames, uint32_t n_frames,
                             uint32_t frame_stride, const uint32_t* pair_frame, const uint32_t* pair_mixture,
                             const uint32_t* pair_density, const double* pair_weight, const uint32_t* pair_key,
                             uint32_t n_pairs);

/* Pairs skipped since creation or the last reset.  Waits for the last accumulate call. */
int gmm_mllr_skipped(gmm_mllr_accumulator* acc, uint64_t* skipped);

/* Device bytes of the handle: *table_bytes the sets' accumulators, *scratch_bytes the later pieces' slabs and the pair
 * scratch of a max_pairs call; *kinds the mask given at creation.  Any pointer may be NULL. */
int gmm_mllr_info(const gmm_mllr_accumulator* acc, uint64_t* table_bytes, uint64_t* scratch_bytes, int* kinds);

/* Waits for the last call and copies the tables of one (key, leaf) to the host: Z [D][D+1], G [D+1][D+1], count_full
 * [1] (full kind); count_shift [1], beta [D], shift [D] (shift kind).  Any pointer may be NULL; a non-NULL pointer to
 * a table of a kind the handle does not hold is GMM_ERR_INVALID_ARGUMENT.  Reading does not change the handle, which
 * can go on accumulating. */
int gmm_mllr_get(gmm_mllr_accumulator* acc, uint32_t key, uint32_t leaf, double* Z, double* G, double* count_full,
                 double* count_shift, double* beta, double* shift);

/* operator+= (cc:274-277) from raw host tables in gmm_mllr_get's layout, scaled: every element of Z, G, beta and shift
 * becomes dst = dst + src * weight, one multiply and one add, each rounded; the counts are added with no weight,
 * dst = dst + src.  A NULL pointer leaves its table as it is; a table of a kind the handle does not hold is
 * GMM_ERR_INVALID_ARGUMENT.  Frame-sharded ranks exchange their tables this way, with no collective. */
int gmm_mllr_add(gmm_mllr_accumulator* acc, uint32_t key, uint32_t leaf, const double* Z, const double* G,
                 const double* count_full, const double* count_shift, const double* beta, const double* shift,
                 double weight);

/* estimateWMatrices and adaptor() (cc:358-379, 444-531, 671-827) for ONE key, host only: no device, no handle, plain
 * C++ with no LAPACK.  kind is GMM_MLLR_FULL or GMM_MLLR_SHIFT.
 * The leaf tables, as gmm_mllr_get returns them for leaf 0 .. n_leaves-1: full kind Z [n_leaves][D][D+1], G
 * [n_leaves][D+1][D+1], count [n_leaves] (count_full; beta and shift are not read); shift kind count [n_leaves]
 * (count_shift), beta [n_leaves][D], shift [n_leaves][D] (Z and G are not read).
 * The binary tree over node ids 0 .. n_tree_ids-1: left[], right[], parent[] with GMM_MLLR_NO_ID for none, root the
 * root's id; an id with neither child is a leaf and leaf_number[id] is its leaf (read for leaf ids only).  Ids that
 * the root does not reach are ignored.
 *   propagate      post-order from the root: node = left; node += right, elementwise f64 adds over the tables and
 *                  the counts.
 *   a node         is estimated iff its count > min_observation (strict): full kind W = Z * pinv(G), [D][D+1],
 *                  column 0 the offset; shift kind shift[d] / beta[d], [1][D].
 *   a tree leaf    (ascending id) climbs to its first ancestor that passes; if the root does not pass, the unit
 *                  matrix (adaptationUnitMatrix: zero offset, identity; shift kind: zeros) at the root's id serves
 *                  all tree leaves.
 *   silence        the mixtures silence_mixtures[0 .. n_silence), ascending, take the ids n_tree_ids, n_tree_ids + 1,
 *                  ...: each is estimated from the tables of its own leaf alone iff that leaf's count >
 *                  min_silence_observation, otherwise it is the unit matrix (zeros); it overrides its leaf's id, a
 *                  later silence mixture on the same leaf overrides an earlier one, as the text does.
 *   then           matrix_of_mixture[m] = id of leaf_of_mixture[m].
 * pinv: one-sided Jacobi SVD in f64 of G as it is (G is symmetric only up to rounding); singular values not above
 * 1e-12 * the largest are dropped (svdThreshold, src/Math/Lapack/Svd.hh:27).
 * Out: *n_matrices, ids[] ascending, matrices [*n_matrices][D][D+1] (full) or [*n_matrices][D] (shift) -- both arrays
 * must hold n_tree_ids + n_silence entries -- and matrix_of_mixture [n_mixtures].
 * GMM_ERR_INVALID_ARGUMENT, never an abort, naming the id: a cycle (an id reached twice), a child out of range, an id
 * with one child, a parent[] that does not mirror the children, a leaf number >= n_leaves, the root with a parent;
 * likewise a silence mixture or a leaf index out of range, silence mixtures not ascending, and a mixture whose leaf
 * neither the tree nor a silence mixture covers (the reference would look up matrix id 0 for it). */
int gmm_mllr_estimate(uint32_t dimension, int kind, uint32_t n_leaves, const double* Z, const double* G,
                      const double* count, const double* beta, const double* shift, const uint32_t* leaf_of_mixture,
                      uint32_t n_mixtures, uint32_t n_tree_ids, const uint32_t* left, const uint32_t* right,
                      const uint32_t* parent, const uint32_t* leaf_number, uint32_t root,
                      const uint32_t* silence_mixtures, uint32_t n_silence, double min_observation,
                      double min_silence_observation, uint32_t* n_matrices, uint32_t* ids, double* matrices,
                      uint32_t* matrix_of_mixture);

/* adaptMixtureSet (cc:146-170, 59-79), host only: out_means [n_means][D] f32.  For every (mixture, density) entry of
 * `set` the mean of the density is transformed with the matrix whose id is matrix_of_mixture[mixture] (ids ascending,
 * matrices in gmm_mllr_estimate's layout):
 *   full kind    out[i] = (f32) sum_j W[i][j] * m_j, f64 products added in ascending j starting from 0.0, m_0 = 1.0,
 *                narrowed once;
 *   shift kind   out[i] = (f32)(shift[i] + (f64) mu_i).
 * A mean referenced by more than one entry is GMM_ERR_UNSUPPORTED naming the mean (the reference would transform it
 * once per entry; its comment says the case is not handled).  A mean referenced by no entry is copied.
 * GMM_ERR_INVALID_ARGUMENT for an id that is not in ids[] (naming the mixture) or model indices out of range. */
int gmm_mllr_adapt_means(const gmm_mixture_set* set, const double* matrices, const uint32_t* ids, uint32_t n_matrices,
                         const uint32_t* matrix_of_mixture, int kind, float* out_means);

#ifdef __cplusplus
}
#endif

#endif /* RASR_GMM_MLLR_H */
