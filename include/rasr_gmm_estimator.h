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
 * and, for discriminative (EBW) training, the joint numerator / denominator accumulation and the file of
 *   DiscriminativeMixtureSetEstimator::accumulateDenominator  src/Mm/DiscriminativeMixtureSetEstimator.cc:187-203
 *   DiscriminativeMixtureSetEstimator::accumulateObjectiveFunction, read, write, accumulate   cc:105-119, 162-177, 205-207
 *   EbwDiscriminativeMixtureEstimator::accumulateDenominator, write, accumulate   EbwDiscriminativeMixtureEstimator.cc
 *   EbwDiscriminativeMean/CovarianceEstimator::accumulateDenominator, write   EbwDiscriminativeGaussDensityEstimator.cc
 * (the section "Discriminative training" below).
 * Not covered: the trainer's logging statistics (weightStats_, dnsPosteriorStats_, finalWeightStats_,
 * scoreStatistics_); of the discriminative estimators, I-smoothing, Rprop and the hlda-style criteria (the EBW
 * estimate is the section "The EBW estimate" at the end).
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

/* AbstractMixtureSetEstimator::reset (cc:292-297): zeroes the tables and the skipped count (and, after a
 * discriminative call, the denominator tables and the objective function: DiscriminativeMixtureSetEstimator::reset). */
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

/* ---- Discriminative training: numerator and denominator statistics in one call ----
 *
 * A lattice gives the same (frame, mixture) pair a numerator weight and a denominator weight.  The handle keeps a
 * second set of tables, the DENOMINATOR tables (mean sums and weights, covariance sums and weights, entry weights:
 * the shapes of gmm_estimator_create), beside the tables the maximum-likelihood calls add to, which are the
 * NUMERATOR tables; and the f64 objective function.  The denominator tables are allocated and zeroed by the handle's
 * first discriminative call (that one call, also in its _device form, zeroes them on the default stream and waits for
 * it on the host before it enqueues its work), so a handle that only sees maximum-likelihood calls never pays for them;
 * gmm_estimator_reset zeroes them and the objective function too.  Maximum-likelihood and discriminative calls may be
 * mixed on one handle under the one-stream rule: a maximum-likelihood call adds to the numerator tables.
 *
 * gmm_estimator_accumulate_discriminative_* is gmm_estimator_accumulate_* (Viterbi mode: the density given, the
 * scorer's best, or the single one) with pair_weight_num and pair_weight_den in the place of pair_weight: pair i adds
 * to the numerator tables with weight pair_weight_num[i] (the estimator's accumulate) and to the denominator tables
 * with weight pair_weight_den[i] (accumulateDenominator, DiscriminativeMixtureSetEstimator.cc:187-192).  Either
 * array may be NULL: that side receives nothing from the call and its tables are not touched.  Both NULL is
 * GMM_ERR_INVALID_ARGUMENT (there is no "weight 1" default here).  A weight that is NaN marks a pair as ABSENT on that
 * side (an arc that only one of the two lattices holds): the side skips it.  Every other weight, 0 included, is
 * LIVE and is added as the reference adds it.  This is a convention of these calls alone: the reference, and
 * gmm_estimator_accumulate_*, would add the NaN to the sums.  The equality with two maximum-likelihood calls stated
 * below is therefore with each side's list taken WITHOUT its NaN pairs.
 *
 * gmm_estimator_accumulate_discriminative_posteriors_* is the Baum-Welch form (cc:193-202) of
 * gmm_estimator_accumulate_posteriors_*: the pair's f32 density posteriors are computed ONCE, and each side gets
 *     finalWeight_side = pair_weight_side[i] * (double) post_ij         (one f64 multiply)
 * A contribution slot (i, j) is live for a side iff finalWeight_side > weight_threshold (a strict f64 compare; NaN
 * does not pass, so a NaN weight is absent here as well).
 *
 * A side adds only its live contributions; it never adds 0 * x for one it skips (that would be NaN for an infinite
 * x and would turn a -0.0 sum into +0.0).
 *
 * ORDER.  The contribution list of a call is the slots live on AT LEAST ONE side, in (pair, density in mixture)
 * order.  Per accumulator that JOINT list is cut into pieces of GMM_ESTIMATOR_CHUNK; within a piece each side adds
 * its own live contributions sequentially, with the operations of the contract at the top of this file; piece 0
 * starts from the side's table value, every later piece from 0, and the later pieces' results are added to the table
 * in piece order, per side (also the result, 0, of a piece in which the side has no live contribution).  Hence:
 *   - an accumulator with at most GMM_ESTIMATOR_CHUNK joint contributions in the call is updated, on each side,
 *     exactly as the reference's sequential loop updates it -- and so exactly as two maximum-likelihood calls on two
 *     handles would, one with the numerator's pairs and one with the denominator's;
 *   - beyond that a side's result is that joint-piece sum bit for bit (the pieces are cut from the joint list, not
 *     from the side's own), within 2 n 2^-53 sum|term| of the sequential sum.
 * No floating-point atomics; the result depends neither on the launch geometry nor on the run.
 *
 * CAPACITY, SKIPPED, ERRORS: as the maximum-likelihood calls (n_pairs <= max_pairs; n_pairs * K_max <= max_pairs and
 * diagonal-sum only for the posterior form).  A bad pair is skipped and counted ONCE, not once per side; a pair
 * absent or under the threshold on both sides is not skipped.  A refused call changes neither table set nor the
 * count.  All pointers are DEVICE pointers for the _device forms, which are enqueued on `stream`; the _host forms
 * copy in and are synchronous. */
int gmm_estimator_accumulate_discriminative_device(gmm_estimator* estimator, gmm_scorer* scorer, const float* frames,
                                                   uint32_t n_frames, uint32_t frame_stride, const uint32_t* pair_frame,
                                                   const uint32_t* pair_mixture, const uint32_t* pair_density,
                                                   const double* pair_weight_num, const double* pair_weight_den,
                                                   uint32_t n_pairs, void* stream);
int gmm_estimator_accumulate_discriminative_host(gmm_estimator* estimator, gmm_scorer* scorer, const float* frames,
                                                 uint32_t n_frames, uint32_t frame_stride, const uint32_t* pair_frame,
                                                 const uint32_t* pair_mixture, const uint32_t* pair_density,
                                                 const double* pair_weight_num, const double* pair_weight_den,
                                                 uint32_t n_pairs);
int gmm_estimator_accumulate_discriminative_posteriors_device(gmm_estimator* estimator, gmm_scorer* scorer,
                                                              const float* frames, uint32_t n_frames,
                                                              uint32_t frame_stride, const uint32_t* pair_frame,
                                                              const uint32_t* pair_mixture, const double* pair_weight_num,
                                                              const double* pair_weight_den, uint32_t n_pairs,
                                                              double weight_threshold, void* stream);
int gmm_estimator_accumulate_discriminative_posteriors_host(gmm_estimator* estimator, gmm_scorer* scorer,
                                                            const float* frames, uint32_t n_frames, uint32_t frame_stride,
                                                            const uint32_t* pair_frame, const uint32_t* pair_mixture,
                                                            const double* pair_weight_num, const double* pair_weight_den,
                                                            uint32_t n_pairs, double weight_threshold);

/* accumulateObjectiveFunction (cc:205-207): objectiveFunction_ += f, on the host.  gmm_estimator_objective reads it. */
int gmm_estimator_accumulate_objective(gmm_estimator* estimator, double f);
int gmm_estimator_objective(gmm_estimator* estimator, double* objective);

/* gmm_estimator_get for the denominator tables (zeros on a handle that has seen no discriminative call). */
int gmm_estimator_get_denominator(gmm_estimator* estimator, double* mean_sums, double* mean_weights,
                                  double* covariance_sums, double* covariance_weights, double* entry_weights);

/* The bytes of the discriminative estimator's write: those of gmm_estimator_serialize (same magic, version 2, same
 * renumbering) with every mean's accumulator followed by its denominator accumulator
 * (EbwDiscriminativeGaussDensityEstimator.cc:55-58), every covariance's likewise (cc:150-153), every mixture's
 * (density, weight) entries followed by its f64 denominator weights (EbwDiscriminativeMixtureEstimator.cc:148-154),
 * and the f64 objective function as the last field (DiscriminativeMixtureSetEstimator.cc:115-119). */
int gmm_estimator_serialize_discriminative(gmm_estimator* estimator, void* data, uint64_t capacity, uint64_t* size);
int gmm_estimator_write_discriminative(gmm_estimator* estimator, const char* filename);

/* gmm_estimator_combine for such files: the denominator accumulators, the denominator weights
 * (EbwDiscriminativeMixtureEstimator.cc:172-186) and the objective functions
 * (DiscriminativeMixtureSetEstimator.cc:162-177) are added in file order as well.  The header does not tell the two
 * formats apart: a file is refused (GMM_ERR_INVALID_ARGUMENT) unless it parses as a discriminative file to its last
 * byte, which a maximum-likelihood file does not. */
int gmm_estimator_combine_discriminative(const void* const* data, const uint64_t* size, uint32_t n, void* out,
                                         uint64_t capacity, uint64_t* out_size);

/* ---- The EBW estimate (host only, f64, no device needed) ----
 *
 * The next mixture set from a discriminative estimator file and the PREVIOUS mixture set
 * (DiscriminativeMixtureSetEstimator::estimate, DiscriminativeMixtureSetEstimator.cc:136-160):
 *   - distributePreviousMixtureSet's topology checks (cc:51-86): dimension, counts, every mixture's density count;
 *     previous index i is the file's index i.  GMM_ERR_INVALID_ARGUMENT otherwise;
 *   - removeDensitiesWithLowWeight (cc:138-140, DiscriminativeMixtureEstimator.cc:34-49) when minimum_observation_weight
 *     or minimum_relative_weight is not 0: by numerator weight and previous mixture weight, the heaviest kept;
 *   - the iteration constants of src/Mm/IterationConstants.cc: Xi (cc:169-200, beta), sigma-minimum (cc:271-293:
 *     sigma_minimum, or if negative sigma_minimum_factor * the smallest previous variance), minimumDk (cc:298-334),
 *     type global-rwth (cc:356-386, 478-485) or local-rwth (cc:408-438, 522-529) with step_size and minimum_icd.
 *     cambridge is GMM_ERR_UNSUPPORTED (the reference's maximumRoot begins with require(false), cc:595), and so is a
 *     density held by more than one mixture entry (the require at cc:127);
 *   - means (EbwDiscriminativeGaussDensityEstimator.cc:73-89): (dtSum + ic * previous) / (dtWeight + ic), narrowed
 *     to f32; the previous mean where dtWeight + ic <= 0;
 *   - covariances (cc:165-198) with the f64 -> f32 narrowing and applyMinimumVariance; a covariance weight or a variance
 *     that is not positive is GMM_ERR_INVALID_ARGUMENT, not an abort;
 *   - mixture weights by the Cambridge scheme with number_of_iterations rounds and the normalisation
 *     (EbwDiscriminativeMixtureEstimator.cc:39-91, 123-136).
 * ORDER.  The reference iterates unordered containers; here the order is fixed: covariances in ascending index of
 * the estimated set; a covariance's densities in ascending (mixture, density in mixture); a covariance's means in order
 * of first appearance among those densities; dimensions ascending.  (A mixture's local-rwth constant starts from
 * the D-k-min of the first covariance, in that order, that holds one of its densities; a mean shared by several
 * densities keeps the constant of the last of them.)
 * Not restated: finalize's pruning of the estimated set by minimum_relative_weight (cc:92-98), I-smoothing, Rprop, the
 * hlda-style criteria, the logging channels.
 * Release *out with gmm_mixture_set_free. */
enum { GMM_EBW_GLOBAL_RWTH = 0, GMM_EBW_LOCAL_RWTH = 1, GMM_EBW_CAMBRIDGE = 2 };
typedef struct gmm_ebw_config {
    double   minimum_observation_weight; /* 5 */
    double   minimum_relative_weight;    /* 0 */
    double   minimum_variance;           /* 0 */
    int      normalize_mixture_weights;  /* 1 */
    int      iteration_constants_type;   /* GMM_EBW_GLOBAL_RWTH */
    double   step_size;                  /* 1.1 */
    double   minimum_icd;                /* 1 */
    double   beta;                       /* 1 */
    double   sigma_minimum;              /* < 0: sigma_minimum_factor * the smallest previous variance */
    double   sigma_minimum_factor;       /* 1e-5 */
    uint32_t number_of_iterations;       /* 100 */
} gmm_ebw_config;
void gmm_default_ebw_config(gmm_ebw_config* config);
int gmm_estimator_estimate_ebw(const void* data, uint64_t size, const gmm_mixture_set* previous,
                               const gmm_ebw_config* config, gmm_mixture_set* out);
/* The f64 iteration constant of every density of the estimated set (its mean estimator's), in density order. */
int gmm_estimator_ebw_iteration_constants(const void* data, uint64_t size, const gmm_mixture_set* previous,
                                          const gmm_ebw_config* config, double* constants, uint32_t capacity,
                                          uint32_t* n);
/* gmm_estimator_serialize_discriminative, then gmm_estimator_estimate_ebw of those bytes. */
int gmm_estimator_estimate_ebw_handle(gmm_estimator* estimator, const gmm_mixture_set* previous,
                                      const gmm_ebw_config* config, gmm_mixture_set* out);

#ifdef __cplusplus
}
#endif

#endif /* RASR_GMM_ESTIMATOR_H */
