/*
 * rasr_gmm_estimator.h -- maximum-likelihood accumulation (Viterbi and Baum-Welch) for mixture-set training (C-ABI).
 *
 * The step between an alignment and the next model: aligned (frame, mixture) pairs are accumulated into the
 * f64 statistics of the mixture set's means, covariances and mixture weights ON THE DEVICE, written in the
 * format of RASR's binary estimator files, combined, and estimated (rasr_gmm_io.h).  Replaces
 *   AbstractMixtureSetEstimator::setTopology            src/Mm/AbstractMixtureSetEstimator.cc:78-115
 *   AbstractMixtureSetEstimator::accumulate (Viterbi)   src/Mm/AbstractMixtureSetEstimator.cc:117-131
 *   AbstractMixtureSetEstimator::accumulate (Baum-Welch) src/Mm/AbstractMixtureSetEstimator.cc:127-147, 386-402
 *   AbstractMixtureSetEstimator::densityIndex           src/Mm/AbstractMixtureSetEstimator.cc:370-384
 *   AbstractMixtureEstimator::accumulate                src/Mm/MixtureEstimator.cc (weights_[index] += weight)
 *   GaussDensityEstimator::accumulate                   src/Mm/GaussDensityEstimator.cc (mean, then covariance)
 *   VectorAccumulator / plusWeighted, plusSquareWeighted src/Mm/VectorAccumulator.hh, src/Mm/Utilities.hh:110-146
 *   AbstractMixtureSetEstimator::write                  src/Mm/AbstractMixtureSetEstimator.cc:416-420, 481-509
 *   MixtureSetEstimatorIndexMap                         src/Mm/AbstractMixtureSetEstimator.cc:804-817
 *   accumulate(Core::BinaryInputStreams&, os)           src/Mm/AbstractMixtureSetEstimator.cc:171-290 (combine)
 * Not covered: the trainer's logging statistics (weightStats_, dnsPosteriorStats_, finalWeightStats_,
 * scoreStatistics_) and the discriminative estimators.
 *
 * THE NUMERIC CONTRACT: deterministic order, no floating-point atomics.
 * An accumulator (one mean, one covariance, one mixture entry) that receives n <= GMM_ESTIMATOR_CHUNK
 * contributions in a call is updated exactly as the reference's sequential loop updates it, in pair order,
 * starting from its current value, with one IEEE f64 rounding per operation and nothing fused:
 *     mean sum[d]        = sum[d] + w * (f64) x[d]                      (plusWeighted)
 *     covariance sum[d]  = sum[d] + (w * (f64) x[d]) * (f64) x[d]       (plusSquareWeighted)
 *     weight             = weight + w
 * (the unweighted forms are these with w = 1).  With n > GMM_ESTIMATOR_CHUNK the call's contributions to that
 * accumulator are cut into consecutive pieces of GMM_ESTIMATOR_CHUNK, in pair order; piece 0 is accumulated onto
 * the current value as above, every later piece is accumulated from 0, and the later pieces' results are then
 * added to the accumulator in piece order.  The result therefore depends neither on the launch geometry nor on
 * the run, and a few lines of numpy restate it (tests/test_estimator_accumulate.py).
 *
 * Errors as in rasr_gmm.h: a negative status, the message via gmm_last_error().
 */
#ifndef RASR_GMM_ESTIMATOR_H
#define RASR_GMM_ESTIMATOR_H

#include <stdint.h>

#include "rasr_gmm_io.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Contributions per piece of one accumulator in one call; part of the numeric contract above. */
#define GMM_ESTIMATOR_CHUNK 512

typedef struct gmm_estimator gmm_estimator;

/* setTopology (AbstractMixtureSetEstimator.cc:78-115): one accumulator per mean, covariance and mixture entry of
 * `topology` (only its dimension and index tables are used, means / variances / log weights may be NULL), as zeroed
 * f64 tables on `device`: mean sums [n_means][D], mean weights [n_means], covariance sums [n_covariances][D],
 * covariance weights [n_covariances], mixture-entry weights [n_entries]; and the scratch of a call of up to
 * max_pairs pairs (for gmm_estimator_accumulate_posteriors_*: of up to max_pairs CONTRIBUTIONS, see there).
 * GMM_ERR_INVALID_ARGUMENT for indices out of range. */
int gmm_estimator_create(const gmm_mixture_set* topology, uint32_t max_pairs, int device, gmm_estimator** out);
int gmm_estimator_destroy(gmm_estimator* estimator);

/* AbstractMixtureSetEstimator::reset (cc:292-297): zeroes the tables and the skipped count. */
int gmm_estimator_reset(gmm_estimator* estimator);

/* accumulate(mixtureIndex, featureVector[, weight]) in Viterbi mode (cc:117-131) for a list of pairs: pair i adds
 * frame pair_frame[i] (row at frames + pair_frame[i] * frame_stride floats) with weight pair_weight[i] (f64; NULL:
 * weight 1) to one density of mixture pair_mixture[i]: to that mixture entry's weight, to the sums of the density's
 * mean and to the squared sums of its covariance (MixtureEstimator / GaussDensityEstimator::accumulate).  All
 * pointers are DEVICE pointers; the call is enqueued on `stream` (a hipStream_t; NULL = default stream), does not
 * synchronize the host and allocates nothing.  The density:
 *   pair_density != NULL            the in-mixture index pair_density[i]; `scorer` is ignored;
 *   else scorer != NULL             bestDensity of the pair from the scorer (densityIndex, cc:370-384: the sparse
 *                                   best-density kernel of gmm_best_density_pairs_device);
 *   else                            every mixture must hold exactly one density (the verify_ at cc:382), which is
 *                                   taken: GMM_ERR_INVALID_ARGUMENT otherwise.
 * A pair is skipped and counted (gmm_estimator_skipped), and its data are never touched, when pair_frame[i] >=
 * n_frames, pair_mixture[i] is out of range, a given density is out of range for its mixture, or the scorer answers
 * 0xffffffff (empty mixture, no finite candidate).
 * Errors: GMM_ERR_CAPACITY for n_pairs > max_pairs; GMM_ERR_UNSUPPORTED for a scorer on another device, on a
 * mixture shard, density-sharded, or of a type gmm_best_density_pairs_device does not take (it takes
 * SIMD-diagonal-maximum, diagonal-maximum, diagonal-sum); GMM_ERR_INVALID_ARGUMENT for a scorer whose dimension,
 * mixture count or entry count differs from the topology's.
 * The call uses the handle's scratch: calls on one handle are made from one thread and on one stream, or ordered
 * by the caller. */
int gmm_estimator_accumulate_device(gmm_estimator* estimator, gmm_scorer* scorer, const float* frames,
                                    uint32_t n_frames, uint32_t frame_stride, const uint32_t* pair_frame,
                                    const uint32_t* pair_mixture, const uint32_t* pair_density,
                                    const double* pair_weight, uint32_t n_pairs, void* stream);

/* The same call with HOST arrays: copies them in and is synchronous. */
int gmm_estimator_accumulate_host(gmm_estimator* estimator, gmm_scorer* scorer, const float* frames,
                                  uint32_t n_frames, uint32_t frame_stride, const uint32_t* pair_frame,
                                  const uint32_t* pair_mixture, const uint32_t* pair_density,
                                  const double* pair_weight, uint32_t n_pairs);

/* AbstractMixtureSetEstimator::weightThreshold_ = Core::Type<f32>::epsilon (cc:63; src/Core/Types.hh:148:
 * 1.19209290e-07F, i.e. 2^-23 = FLT_EPSILON), widened to the f64 it is compared in */
#define GMM_ESTIMATOR_DEFAULT_WEIGHT_THRESHOLD 1.1920928955078125e-07

/* accumulate(mixtureIndex, featureVector, weight) in Baum-Welch mode (cc:127-147, 386-402) for a list of pairs: pair
 * i is spread over ALL densities of mixture pair_mixture[i] by their posterior probabilities.  It expands into the
 * contributions (i, j), one per density j of the mixture, with
 *     finalWeight = pair_weight[i] * (double) post_ij      (one f64 multiply; NULL pair_weight: 1)
 * where post_ij is the f32 posterior of gmm_density_posteriors_pairs_device for that pair, bit for bit.  A
 * contribution is accumulated iff finalWeight > weight_threshold (a strict f64 compare; NaN does not pass), and then
 * adds exactly as a Viterbi pair of weight finalWeight on density j does: to the entry weight, the mean sums and the
 * covariance squared sums.  Without a scorer (scorer == NULL) every mixture must hold exactly one density
 * (GMM_ERR_INVALID_ARGUMENT otherwise, the verify_ at cc:398): its posterior is 1.0 and the threshold still applies.
 * ORDER: the contributions of a call are ordered by (pair index, density in mixture), the reference's loop order, and
 * the numeric contract at the top of this file holds for that list as it does for a Viterbi call's pairs: every
 * accumulator sequentially in f64 in contribution order, pieces of GMM_ESTIMATOR_CHUNK, no floating-point atomics.
 * CAPACITY: a call needs n_pairs * K_max <= max_pairs, K_max the largest entry count of the topology's mixtures (at
 * least 1; 1 without a scorer), the product taken in 64 bits: max_pairs counts contribution slots for this call.
 * GMM_ERR_CAPACITY otherwise.
 * SKIPPED: a pair is skipped and counted once when its frame or mixture is out of range or its mixture is empty; its
 * data are never touched.  A pair whose contributions all stay under the threshold is not skipped.
 * The other errors are gmm_estimator_accumulate_device's, and GMM_ERR_UNSUPPORTED for every scorer type but
 * diagonal-sum (gmm_density_posteriors_pairs_device).  A refused call changes neither the tables nor the count.
 * All pointers are DEVICE pointers; the call is enqueued on `stream` and does not synchronize the host.  The
 * handle's FIRST posterior call allocates the posterior scratch (the rows, the contributions' frames and weights:
 * max_pairs elements each), which the handle keeps: handles that only see Viterbi calls never pay for it, and later
 * calls allocate nothing.  The posterior and Viterbi calls may be mixed on one handle, under the same one-stream rule. */
int gmm_estimator_accumulate_posteriors_device(gmm_estimator* estimator, gmm_scorer* scorer, const float* frames,
                                               uint32_t n_frames, uint32_t frame_stride, const uint32_t* pair_frame,
                                               const uint32_t* pair_mixture, const double* pair_weight, uint32_t n_pairs,
                                               double weight_threshold, void* stream);

/* The same call with HOST arrays: copies them in and is synchronous. */
int gmm_estimator_accumulate_posteriors_host(gmm_estimator* estimator, gmm_scorer* scorer, const float* frames,
                                             uint32_t n_frames, uint32_t frame_stride, const uint32_t* pair_frame,
                                             const uint32_t* pair_mixture, const double* pair_weight, uint32_t n_pairs,
                                             double weight_threshold);

/* Pairs skipped since creation or the last reset.  Waits for the last accumulate call. */
int gmm_estimator_skipped(gmm_estimator* estimator, uint64_t* skipped);

/* Copies the tables to host f64 arrays (sizes as in gmm_estimator_create; any pointer may be NULL).  Waits for the
 * last accumulate call first (every accumulate call records an event on its stream). */
int gmm_estimator_get(gmm_estimator* estimator, double* mean_sums, double* mean_weights, double* covariance_sums,
                      double* covariance_weights, double* entry_weights);

/* The bytes of AbstractMixtureSetEstimator::write (cc:416-420 header: the "MIXSET" magic in 8 bytes, version 2;
 * cc:481-509 body): means, covariances and densities renumbered by first appearance while walking the mixtures
 * and then their densities (MixtureSetEstimatorIndexMap, cc:804-817) -- whatever no mixture references is left
 * out --, each accumulator as size, f64 sums, f64 weight; the mixtures' entries with the renumbered density index
 * and their f64 weight.  *size receives the byte count; up to `capacity` bytes are copied into `data` (may be NULL
 * to ask the size): GMM_ERR_CAPACITY if capacity is smaller (with data non-NULL). */
int gmm_estimator_serialize(gmm_estimator* estimator, void* data, uint64_t capacity, uint64_t* size);
int gmm_estimator_write(gmm_estimator* estimator, const char* filename);

/* gmm_estimator_serialize, then gmm_mixture_set_estimate of those bytes (config NULL = defaults; release *out
 * with gmm_mixture_set_free): MixtureSetEstimatorReader (src/Mm/MixtureSetReader.cc:52-74) on what write() wrote. */
int gmm_estimator_estimate(gmm_estimator* estimator, const gmm_estimator_config* config, gmm_mixture_set* out);

/* The trainer's combine action, accumulate(Core::BinaryInputStreams&, os) (cc:171-290): n estimator files (their
 * bytes data[i], size[i]) of the same version, the same dimension and an equal topology (counts, density table,
 * the mixtures' density indices) are added accumulator by accumulator in file order -- the first file supplies
 * the starting value, the others are added to it one by one (sum = sum + other, weight = weight + other) -- and
 * written as one file (version 2).  Host only, no device needed.  *out_size receives the byte count; up to
 * `capacity` bytes go to `out` (may be NULL to ask the size; GMM_ERR_CAPACITY if smaller).
 * GMM_ERR_INVALID_ARGUMENT for n == 0, a bad magic, a version or topology mismatch, or a truncated file.
 * Frame-sharded multi-GPU training needs no collective this way: every rank writes its file, one process
 * combines them. */
int gmm_estimator_combine(const void* const* data, const uint64_t* size, uint32_t n, void* out, uint64_t capacity,
                          uint64_t* out_size);

#ifdef __cplusplus
}
#endif

#endif /* RASR_GMM_ESTIMATOR_H */
