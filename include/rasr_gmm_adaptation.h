/*
 * rasr_gmm_adaptation.h -- constrained-MLLR / affine feature transforms of speaker-adaptive training (C-ABI):
 * accumulation per speaker (or cluster) key ON THE DEVICE, and the estimation of the transform on the host.
 *
 * Aligned (frame, mixture) pairs, a density per pair and a weight -- what rasr_gmm.h and rasr_gmm_estimator.h already
 * produce on the device -- are accumulated into the f64 statistics of Mm::AffineFeatureTransformAccumulator, one
 * set of tables per key, n_keys sets side by side.  Replaces
 *   AffineFeatureTransformAccumulator::accumulate   src/Mm/AffineFeatureTransformAccumulator.cc:40-121
 *   AffineFeatureTransformAccumulator::finalize     src/Mm/AffineFeatureTransformAccumulator.cc:123-143
 *   AffineFeatureTransformAccumulator::estimate     src/Mm/AffineFeatureTransformAccumulator.cc:150-311
 *   AffineFeatureTransformAccumulator::combine      src/Mm/AffineFeatureTransformAccumulator.cc:345-365
 * (driven per key by Speech::AffineFeatureTransformEstimator / KeyedEstimator).  Not covered: the hlda criterion and a
 * feature dimension other than the model dimension, score() and its log-determinant, the binary and XML accumulator
 * files (read / write / dump), applying a transform to frames.  MLLR mean transforms over a regression tree are
 * rasr_gmm_mllr.h; BandMllrAdaptation, SemiTiedAdaptation, the estimator and adaptor files, building the tree from a
 * CART and a RASR-side adapter remain out.
 *
 * THE TABLES of one key, D the dimension of the mixture set (feature dimension = model dimension):
 *   beta                 the summed weight
 *   k    [D][D+1]        row i: sum of (mu_i / v_i) * xi
 *   G    [D][D+1][D+1]   matrix i: sum of xi xi^T / v_i   (upper triangle accumulated; symmetric when read)
 *   mean [D+1]           sum of xi
 *   cov  [D+1][D+1]      sum of xi xi^T                   (upper triangle accumulated; symmetric when read)
 * with xi = (1, x_0, ..., x_{D-1}) the extended feature, mu and v the mean and the diagonal covariance of the pair's
 * density.  A mixture set with exactly ONE covariance puts the handle into the reference's "global variance
 * optimisation" mode (cc:54-60, latched there by the first pair; here from the start): G is never accumulated and
 * has no device table; gmm_affine_get derives it from cov (finalize, cc:124-133).
 *
 * THE NUMERIC CONTRACT: deterministic order, no floating-point atomics -- rasr_gmm_estimator.h's, per (key, table).
 * With xi_j = (f64) of the f32 feature (xi_0 = 1.0), mu_i and v_i widened f32 -> f64, w the pair's f64 weight, every
 * operation rounded once in IEEE f64 and nothing fused, a pair updates, in the reference's operand order,
 *     beta        = beta + w
 *     k[i][j]     = k[i][j]    + ((mu[i] / v[i]) * xi[j]) * w
 *     G[i][j][k]  = G[i][j][k] + ((xi[j] * xi[k]) / v[i]) * w      (j <= k; not in pooled mode)
 *     mean[j]     = mean[j]    + xi[j] * w
 *     cov[j][k]   = cov[j][k]  + (xi[j] * xi[k]) * w               (j <= k)
 * (the unweighted form is the weighted one with w = 1, which is exact).  The division is a division: never a
 * multiplication by a stored reciprocal.  A key's tables receive that key's non-skipped pairs in pair order.  With
 * more than GMM_AFFINE_CHUNK pairs of one key in a call, they are cut into consecutive pieces of GMM_AFFINE_CHUNK;
 * piece 0 is accumulated onto the current value, every later piece from 0, and the later pieces' results are then
 * added in piece order.  The result depends neither on the launch geometry nor on the run; tests/affine_restatement.py
 * restates it in numpy.
 * The reference binary is built with -ffast-math: its own last bits are whatever its compiler made of the inner loop
 * (the invariant division may be hoisted as a reciprocal, sums reassociated), so the reference's text in the STATED
 * order above is the contract, not the bits of one build of it.
 *
 * Errors as in rasr_gmm.h: a negative status, the message via gmm_last_error().
 */
#ifndef RASR_GMM_ADAPTATION_H
#define RASR_GMM_ADAPTATION_H

#include <stdint.h>

#include "rasr_gmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs per piece of one key in one call; part of the numeric contract above. */
#define GMM_AFFINE_CHUNK 512

/* The largest dimension a handle takes (the kernels stage a batch of extended features in LDS). */
#define GMM_AFFINE_MAX_DIMENSION 256

typedef struct gmm_affine_accumulator gmm_affine_accumulator;

/* n_keys sets of zeroed f64 tables on `device` for the model `set` (its dimension, means, variances and the density ->
 * mean / covariance and mixture tables are copied), and the scratch of a call of up to max_pairs pairs.  The size
 * -- n_keys * D * (D+1)(D+2)/2 * 8 bytes of G tables unless pooled, the small tables, and the later pieces' slabs of a
 * max_pairs call -- is checked against the device's free memory before anything is allocated: a handle past three
 * quarters of it is GMM_ERR_UNSUPPORTED, and the message names the size.  GMM_ERR_UNSUPPORTED also for D >
 * GMM_AFFINE_MAX_DIMENSION; GMM_ERR_INVALID_ARGUMENT for n_keys == 0, D == 0 or indices out of range. */
int gmm_affine_create(const gmm_mixture_set* set, uint32_t n_keys, uint32_t max_pairs, int device,
                      gmm_affine_accumulator** out);
int gmm_affine_destroy(gmm_affine_accumulator* acc);

/* Zeroes all keys' tables and the skipped count. */
int gmm_affine_reset(gmm_affine_accumulator* acc);

/* accumulate(feature, density, mixtureSet[, weight]) (cc:40-121) for a list of pairs: pair i adds frame pair_frame[i]
 * (row at frames + pair_frame[i] * frame_stride floats) with weight pair_weight[i] (f64; NULL: weight 1) and one
 * density of mixture pair_mixture[i] to the tables of key pair_key[i] (NULL: key 0).  The density is resolved exactly
 * as gmm_estimator_accumulate_device resolves it:
 *   pair_density != NULL            the in-mixture index pair_density[i]; `scorer` is ignored;
 *   else scorer != NULL             the scorer's best density of the pair (gmm_best_density_pairs_device's kernel);
 *   else                            every mixture must hold exactly one density: GMM_ERR_INVALID_ARGUMENT otherwise.
 * A Baum-Welch caller expands its pairs with gmm_density_posteriors_pairs_* and passes densities and weights.
 * A pair is skipped and counted (gmm_affine_skipped), and its frame is never read, when its frame, mixture, density
 * or key is out of range or the scorer answers 0xffffffff (empty mixture, no finite candidate).
 * All pointers are DEVICE pointers; the call is enqueued on `stream` (a hipStream_t; NULL = default stream), does not
 * synchronize the host and allocates nothing.
 * Errors: GMM_ERR_CAPACITY for n_pairs > max_pairs; GMM_ERR_UNSUPPORTED for a scorer on another device, on a mixture
 * shard, density-sharded, or of a type without the pairs kernel; GMM_ERR_INVALID_ARGUMENT for a scorer whose
 * dimension, mixture count or entry count differs from the set's.  A refused call changes nothing.
 * The call uses the handle's scratch: calls on one handle are made from one thread and on one stream, or ordered by
 * the caller. */
int gmm_affine_accumulate_device(gmm_affine_accumulator* acc, gmm_scorer* scorer, const float* frames,
                                 uint32_t n_frames, uint32_t frame_stride, const uint32_t* pair_frame,
                                 const uint32_t* pair_mixture, const uint32_t* pair_density, const double* pair_weight,
                                 const uint32_t* pair_key, uint32_t n_pairs, void* stream);

/* The same call with HOST arrays: copies them in and is synchronous. */
int gmm_affine_accumulate_host(gmm_affine_accumulator* acc, gmm_scorer* scorer, const float* frames, uint32_t n_frames,
                               uint32_t frame_stride, const uint32_t* pair_frame, const uint32_t* pair_mixture,
                               const uint32_t* pair_density, const double* pair_weight, const uint32_t* pair_key,
                               uint32_t n_pairs);

/* Pairs skipped since creation or the last reset.  Waits for the last accumulate call. */
int gmm_affine_skipped(gmm_affine_accumulator* acc, uint64_t* skipped);

/* Device bytes of the handle: *table_bytes the keys' accumulators (no G table in pooled mode), *scratch_bytes the
 * later pieces' slabs and the pair scratch of a max_pairs call; *pooled 1 in global variance optimisation mode.  Any
 * pointer may be NULL. */
int gmm_affine_info(const gmm_affine_accumulator* acc, uint64_t* table_bytes, uint64_t* scratch_bytes, int* pooled);

/* Waits for the last call and copies one key's tables to the host, finalized as cc:123-143 does: beta [1], k
 * [D][D+1], G [D][D+1][D+1] and cov [D+1][D+1] as full symmetric matrices, mean [D+1].  In pooled mode G[i][j][k] =
 * cov[j][k] / (f64) variance[i], one division per element.  Reading does not change the handle, which can go on
 * accumulating.  Any pointer may be NULL. */
int gmm_affine_get(gmm_affine_accumulator* acc, uint32_t key, double* beta, double* k, double* G, double* mean,
                   double* cov);

/* combine (cc:345-365) from raw host tables in gmm_affine_get's layout: every element of the key's tables becomes
 * dst = dst + src * weight, one multiply and one add, each rounded (of G and cov the upper triangles are read).  G is
 * added only when the handle is not in pooled mode; a NULL pointer leaves its table as it is.  Frame-sharded ranks
 * exchange their tables this way, with no collective, as the estimator files do. */
int gmm_affine_add(gmm_affine_accumulator* acc, uint32_t key, const double* beta, const double* k, const double* G,
                   const double* mean, const double* cov, double weight);

typedef enum gmm_affine_criterion {
    GMM_AFFINE_NAIVE     = 0,
    GMM_AFFINE_MMI_PRIME = 1,
    GMM_AFFINE_HLDA      = 2 /* GMM_ERR_UNSUPPORTED */
} gmm_affine_criterion;

/* estimate (cc:177-311) on finalized tables (gmm_affine_get's layout), host only: no device, no handle.
 * initial_transform: initial_columns == D + 1: [D][D+1], column 0 the offset; == D: [D][D], which gains a zero offset
 * column (cc:198-199); NULL: the identity (cc:169-172).  out_transform: [D][D+1] f32, column 0 the offset.
 *   naive       row i = G[i]^-1 k[i] (cc:226-230);
 *   mmiPrime    `iterations` sweeps of Gales' row update (cc:244-299) with feature = model dimension, so the cofactor
 *               row is the column of the inverse of the linear part; beta < min_observation_weight returns the
 *               initial transform (cc:204; for every criterion but naive).
 * The row update is restated as the reference's text computes it: in l1 and l2 the factor `1 / 2` is an integer
 * division, so the quadratic term vanishes and the root is chosen by beta * log|alpha * eps1 + eps2| alone.
 * mean and cov enter only the reference's reduced-dimension branch and are not read here (they may be NULL).
 * The inverses are f64 Gauss-Jordan eliminations with partial pivoting; a singular G[i] is GMM_ERR_INVALID_ARGUMENT
 * naming the row, a singular linear part likewise.  hlda is GMM_ERR_UNSUPPORTED. */
int gmm_affine_estimate(uint32_t dimension, double beta, const double* k, const double* G, const double* mean,
                        const double* cov, int criterion, uint32_t iterations, double min_observation_weight,
                        const double* initial_transform, uint32_t initial_columns, float* out_transform);

#ifdef __cplusplus
}
#endif

#endif /* RASR_GMM_ADAPTATION_H */
