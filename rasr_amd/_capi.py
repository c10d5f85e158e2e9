"""ctypes binding of the C-ABI in include/rasr_gmm.h (librasr_gmm.so).

The library is the product: there is no Python or CPU fallback.  If the shared
object is missing, loading raises immediately (build it with `make` or
`python -c "import __graft_entry__ as g; g.build()"`).
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RASR_GMM_LIB selects another build of the same library (kernel A/B variants, scripts/ab_bench.py)
LIB_PATH = os.environ.get("RASR_GMM_LIB") or os.path.join(_HERE, "lib", "librasr_gmm.so")

GMM_OK = 0
GMM_ERR_INVALID_ARGUMENT = -1
GMM_ERR_UNSUPPORTED = -2
GMM_ERR_DEVICE = -3
GMM_ERR_OUT_OF_MEMORY = -4
GMM_ERR_CAPACITY = -5
GMM_ESTIMATOR_CHUNK = 512  # include/rasr_gmm_estimator.h: part of the accumulation's numeric contract
GMM_AFFINE_CHUNK = 512  # include/rasr_gmm_adaptation.h: part of the affine accumulation's numeric contract
GMM_MLLR_CHUNK = 512  # include/rasr_gmm_mllr.h: part of the MLLR accumulation's numeric contract
GMM_MLLR_FULL = 1  # the kinds of MLLR statistics (a mask for gmm_mllr_create)
GMM_MLLR_SHIFT = 2
GMM_MLLR_NO_ID = 0xFFFFFFFF  # "none" in the tree arrays of gmm_mllr_estimate
GMM_ALIGN_MAX_STATES = 6144  # include/rasr_gmm_align.h: the most states of one segment
GMM_ALIGN_MAX_STATES_POSTERIOR = 2432  # the most states of one segment in a Baum-Welch (posteriors) call
GMM_ALIGN_MAX_IN_ARCS = 65535  # the most arcs entering one state
GMM_ALIGN_NONE = 0xFFFFFFFF  # the per-frame outputs of a segment without an alignment
GMM_ALIGN_MAX_ITERATIONS = 256  # the most thresholds of a search schedule
STATE_POSTERIOR_CHUNK = 256  # include/rasr_gmm.h GMM_STATE_POSTERIOR_CHUNK: part of the state posteriors' contract
# GMM_ESTIMATOR_DEFAULT_WEIGHT_THRESHOLD: Core::Type<f32>::epsilon, the Baum-Welch weightThreshold_
DEFAULT_WEIGHT_THRESHOLD = 2.0 ** -23
GMM_FLAG_NATIVE_F32 = 1  # gmm_scorer_config.flags
GMM_FLAG_SPLIT_TILE16 = 2
GMM_FLAG_SPLIT_TILE32 = 4
GMM_FLAG_REFERENCE_ORDER = 8  # diagonal-maximum / batch-float in the reference's f32 operation order
GMM_FLAG_FULL_KEYS = 16  # batch-int / -fast: (score, density) keys instead of the score-only class layout
GMM_FLAG_NO_SCORE_ONLY_TWIN = 32  # SIMD: no score-only copy of the model (callers that always want best densities)
GMM_FLAG_CACHE_ARCHIVE_READ_ONLY = 64  # preselection: read the cached clustering, never write it
GMM_FLAG_ACCEPT_SPREAD_BOUND = 128  # float types: keep the matrix-core kernel, the predicted bound in place of 1e-4
GMM_FLAG_SPLIT_WIDE_GENERIC = 256  # scoreSplitWide: the generic form for every chunk, uniform ones too
FLOAT_CONTRACT = 1e-4  # the float types' relative bound
GMM_CLUSTERING = {0: "built", 1: "written", 2: "cached"}  # gmm_scorer_clustering_source

# Mm::Module_::FeatureScorerType values (src/Mm/Module.hh:48-70)
BATCH_DIAGONAL_MAXIMUM_FLOAT = 0
BATCH_PRESELECTION_FLOAT = 1
BATCH_PRESELECTION_INT = 2
BATCH_DIAGONAL_MAXIMUM_INT = 3
BATCH_DIAGONAL_MAXIMUM_FAST = 4
DIAGONAL_MAXIMUM = 5
SIMD_DIAGONAL_MAXIMUM = 9
DIAGONAL_SUM = 12  # diagonalSum (no registration string in the reference factory)

SCORER_TYPES = {
    "batch-diagonal-maximum-float": BATCH_DIAGONAL_MAXIMUM_FLOAT,
    "batch-diagonal-maximum-int": BATCH_DIAGONAL_MAXIMUM_INT,
    "batch-diagonal-maximum-fast": BATCH_DIAGONAL_MAXIMUM_FAST,
    "preselection-batch-float": BATCH_PRESELECTION_FLOAT,
    "preselection-batch-int": BATCH_PRESELECTION_INT,
    "diagonal-maximum": DIAGONAL_MAXIMUM,
    "SIMD-diagonal-maximum": SIMD_DIAGONAL_MAXIMUM,
    "diagonal-sum": DIAGONAL_SUM,
}

_u32p = ctypes.POINTER(ctypes.c_uint32)
_f32p = ctypes.POINTER(ctypes.c_float)
_f64p = ctypes.POINTER(ctypes.c_double)


class MixtureSetDesc(ctypes.Structure):
    _fields_ = [
        ("dimension", ctypes.c_uint32),
        ("n_means", ctypes.c_uint32),
        ("means", _f32p),
        ("n_covariances", ctypes.c_uint32),
        ("variances", _f32p),
        ("n_densities", ctypes.c_uint32),
        ("density_mean", _u32p),
        ("density_covariance", _u32p),
        ("n_mixtures", ctypes.c_uint32),
        ("mixture_offsets", _u32p),
        ("mixture_densities", _u32p),
        ("mixture_log_weights", _f64p),
    ]


class ScorerConfig(ctypes.Structure):
    _fields_ = [
        ("mixture_weight_scale", ctypes.c_float),
        ("gaussian_scale", ctypes.c_float),
        ("score_scale", ctypes.c_float),
        ("max_frames", ctypes.c_uint32),
        ("mixture_begin", ctypes.c_uint32),
        ("mixture_end", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("clusters", ctypes.c_uint32),
        ("select_clusters", ctypes.c_uint32),
        ("clustering_iterations", ctypes.c_uint32),
        ("backoff_score", ctypes.c_float),
        ("cache_archive", ctypes.c_char_p),
    ]


class EstimatorConfig(ctypes.Structure):
    _fields_ = [
        ("minimum_observation_weight", ctypes.c_double),
        ("minimum_relative_weight", ctypes.c_double),
        ("minimum_variance", ctypes.c_double),
        ("allow_zero_weights", ctypes.c_uint32),
        ("normalize_mixture_weights", ctypes.c_uint32),
    ]


class EbwConfig(ctypes.Structure):  # gmm_ebw_config
    _fields_ = [
        ("minimum_observation_weight", ctypes.c_double),
        ("minimum_relative_weight", ctypes.c_double),
        ("minimum_variance", ctypes.c_double),
        ("normalize_mixture_weights", ctypes.c_int),
        ("iteration_constants_type", ctypes.c_int),
        ("step_size", ctypes.c_double),
        ("minimum_icd", ctypes.c_double),
        ("beta", ctypes.c_double),
        ("sigma_minimum", ctypes.c_double),
        ("sigma_minimum_factor", ctypes.c_double),
        ("number_of_iterations", ctypes.c_uint32),
    ]


class AlignGraphs(ctypes.Structure):  # gmm_align_graphs
    _fields_ = [
        ("n_segments", ctypes.c_uint32),
        ("state_offset", ctypes.c_void_p),
        ("arc_offset", ctypes.c_void_p),
        ("arc_target", ctypes.c_void_p),
        ("arc_mixture", ctypes.c_void_p),
        ("arc_weight", ctypes.c_void_p),
        ("initial_state", ctypes.c_void_p),
        ("final_weight", ctypes.c_void_p),
        ("frame_begin", ctypes.c_void_p),
        ("n_frames", ctypes.c_void_p),
    ]


class AlignSearchStruct(ctypes.Structure):  # gmm_align_search
    _fields_ = [
        ("min_pruning", ctypes.c_float),
        ("max_pruning", ctypes.c_float),
        ("increment_factor", ctypes.c_float),
        ("min_average_hypotheses", ctypes.c_double),
        ("until_no_score_difference", ctypes.c_int),
        ("n_best", ctypes.c_uint32),
    ]


EBW_TYPES = {"global-rwth": 0, "local-rwth": 1, "cambridge": 2}

GMM_HOST_KEEP_BEST = 1
GMM_HOST_FRAME_MAJOR = 2
GMM_HOST_LAZY_BEST = 4
GMM_HOST_ASYNC = 8
# gmm_scorer_create_sharded: the per-frame reduce of mixtures split between GPUs
GMM_EXCHANGE = {"auto": 0, "rccl": 1, "copy": 2}

# (name, restype, argtypes) for every function declared in include/rasr_gmm.h, rasr_gmm_io.h, rasr_gmm_estimator.h,
# rasr_gmm_adaptation.h, rasr_gmm_mllr.h and rasr_gmm_align.h
PROTOTYPES = [
    ("gmm_default_config", None, [ctypes.POINTER(ScorerConfig)]),
    ("gmm_scorer_create", ctypes.c_int,
     [ctypes.POINTER(MixtureSetDesc), ctypes.c_int, ctypes.POINTER(ScorerConfig), ctypes.c_int,
      ctypes.POINTER(ctypes.c_void_p)]),
    ("gmm_scorer_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("gmm_scorer_n_mixtures", ctypes.c_uint32, [ctypes.c_void_p]),
    ("gmm_scorer_dimension", ctypes.c_uint32, [ctypes.c_void_p]),
    ("gmm_scorer_n_covariances", ctypes.c_uint32, [ctypes.c_void_p]),
    ("gmm_scorer_type_of", ctypes.c_int, [ctypes.c_void_p]),
    ("gmm_score_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint32, ctypes.c_void_p]),
    ("gmm_score_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint32]),
    ("gmm_score_host_ring", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]),
    ("gmm_host_call_wait", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64]),
    ("gmm_fetch_best_density", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32]),
    ("gmm_best_density_pairs", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    ("gmm_best_density_pairs_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_density_posteriors_pairs_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_density_posteriors_pairs_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    ("gmm_state_posteriors_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_double,
      ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_state_posteriors_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_double,
      ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_host_alloc", ctypes.c_int, [ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]),
    ("gmm_host_free", ctypes.c_int, [ctypes.c_void_p]),
    ("gmm_scorer_quantization", ctypes.c_int, [ctypes.c_void_p, _f32p, _f32p]),
    ("gmm_scorer_multiply_and_quantize", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_prepare_quantized_host", ctypes.c_int,
     [ctypes.POINTER(MixtureSetDesc), ctypes.c_int, _f32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p]),
    ("gmm_scorer_launch_info", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, _u32p, ctypes.POINTER(ctypes.c_char_p)]),
    ("gmm_scorer_chunk_forms", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, _u32p, _u32p]),
    ("gmm_scorer_set_chunk_target", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    ("gmm_scorer_k_steps", ctypes.c_int, [ctypes.c_void_p, _u32p]),
    ("gmm_float_spread_bound", ctypes.c_int,
     [ctypes.POINTER(MixtureSetDesc), ctypes.c_int, ctypes.POINTER(ScorerConfig), _f64p, _f64p]),
    ("gmm_scorer_spread_bound", ctypes.c_int, [ctypes.c_void_p, _f64p, _f64p]),
    ("gmm_scorer_set_timing", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("gmm_scorer_kernel_time", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), _u32p, ctypes.c_int]),
    ("gmm_scorer_density_clustering", ctypes.c_int,
     [ctypes.c_void_p, _u32p, _u32p, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_scorer_cluster_selection", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    ("gmm_scorer_clustering_source", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]),
    ("gmm_cache_archive_read_item", ctypes.c_int,
     [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("gmm_cache_archive_write_item", ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64]),
    ("gmm_density_clustering_seeds", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, _u32p]),
    ("gmm_shard_pack_keys", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
      ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_shard_unpack_keys", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
      ctypes.c_void_p]),
    ("gmm_density_shard_plan", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, _u32p]),
    ("gmm_scorer_create_sharded", ctypes.c_int,
     [ctypes.POINTER(MixtureSetDesc), ctypes.c_int, ctypes.POINTER(ScorerConfig), ctypes.c_void_p, ctypes.c_uint32,
      ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    ("gmm_scorer_shard_info", ctypes.c_int, [ctypes.c_void_p, _u32p, ctypes.POINTER(ctypes.c_int)]),
    ("gmm_last_error", ctypes.c_char_p, []),
    # include/rasr_gmm_io.h
    ("gmm_mixture_set_read", ctypes.c_int,
     [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(MixtureSetDesc)]),
    ("gmm_mixture_set_parse", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(MixtureSetDesc)]),
    ("gmm_mixture_set_free", ctypes.c_int, [ctypes.POINTER(MixtureSetDesc)]),
    ("gmm_default_estimator_config", None, [ctypes.POINTER(EstimatorConfig)]),
    ("gmm_mixture_set_estimate", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(EstimatorConfig), ctypes.POINTER(MixtureSetDesc)]),
    ("gmm_mixture_set_read_config", ctypes.c_int,
     [ctypes.c_char_p, ctypes.POINTER(EstimatorConfig), ctypes.c_uint32, ctypes.c_uint32,
      ctypes.POINTER(MixtureSetDesc)]),
    ("gmm_mixture_set_write", ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(MixtureSetDesc), ctypes.c_uint32]),
    # include/rasr_gmm_estimator.h
    ("gmm_estimator_create", ctypes.c_int,
     [ctypes.POINTER(MixtureSetDesc), ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    ("gmm_estimator_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("gmm_estimator_reset", ctypes.c_int, [ctypes.c_void_p]),
    ("gmm_estimator_accumulate_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    ("gmm_estimator_accumulate_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    ("gmm_estimator_accumulate_posteriors_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p]),
    ("gmm_estimator_accumulate_posteriors_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_double]),
    ("gmm_estimator_skipped", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("gmm_estimator_get", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_estimator_serialize", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("gmm_estimator_write", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    ("gmm_estimator_estimate", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(EstimatorConfig), ctypes.POINTER(MixtureSetDesc)]),
    ("gmm_estimator_combine", ctypes.c_int,
     [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("gmm_estimator_accumulate_discriminative_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    ("gmm_estimator_accumulate_discriminative_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    ("gmm_estimator_accumulate_discriminative_posteriors_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p]),
    ("gmm_estimator_accumulate_discriminative_posteriors_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_double]),
    ("gmm_estimator_accumulate_objective", ctypes.c_int, [ctypes.c_void_p, ctypes.c_double]),
    ("gmm_estimator_objective", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    ("gmm_estimator_get_denominator", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_estimator_serialize_discriminative", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("gmm_estimator_write_discriminative", ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    ("gmm_estimator_combine_discriminative", ctypes.c_int,
     [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    ("gmm_default_ebw_config", None, [ctypes.POINTER(EbwConfig)]),
    ("gmm_estimator_estimate_ebw", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(MixtureSetDesc), ctypes.POINTER(EbwConfig),
      ctypes.POINTER(MixtureSetDesc)]),
    ("gmm_estimator_ebw_iteration_constants", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(MixtureSetDesc), ctypes.POINTER(EbwConfig), ctypes.c_void_p,
      ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    ("gmm_estimator_estimate_ebw_handle", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(MixtureSetDesc), ctypes.POINTER(EbwConfig), ctypes.POINTER(MixtureSetDesc)]),
    # include/rasr_gmm_adaptation.h
    ("gmm_affine_create", ctypes.c_int,
     [ctypes.POINTER(MixtureSetDesc), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    ("gmm_affine_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("gmm_affine_reset", ctypes.c_int, [ctypes.c_void_p]),
    ("gmm_affine_accumulate_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    ("gmm_affine_accumulate_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    ("gmm_affine_skipped", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("gmm_affine_info", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]),
    ("gmm_affine_get", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, _f64p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_affine_add", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, _f64p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_double]),
    ("gmm_affine_estimate", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
      ctypes.c_uint32, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    # include/rasr_gmm_mllr.h
    ("gmm_mllr_create", ctypes.c_int,
     [ctypes.POINTER(MixtureSetDesc), ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32,
      ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    ("gmm_mllr_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("gmm_mllr_reset", ctypes.c_int, [ctypes.c_void_p]),
    ("gmm_mllr_accumulate_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]),
    ("gmm_mllr_accumulate_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    ("gmm_mllr_skipped", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("gmm_mllr_info", ctypes.c_int,
     [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]),
    ("gmm_mllr_get", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_mllr_add", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double]),
    ("gmm_mllr_estimate", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_double,
      ctypes.c_double, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_mllr_adapt_means", ctypes.c_int,
     [ctypes.POINTER(MixtureSetDesc), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int,
      ctypes.c_void_p]),
    # include/rasr_gmm_align.h
    ("gmm_aligner_create", ctypes.c_int,
     [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int,
      ctypes.POINTER(ctypes.c_void_p)]),
    ("gmm_aligner_destroy", ctypes.c_int, [ctypes.c_void_p]),
    ("gmm_aligner_set_segments", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(AlignGraphs)]),
    ("gmm_aligner_align_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_aligner_align_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p,
      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    ("gmm_aligner_posteriors_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_float,
      ctypes.c_uint32] + [ctypes.c_void_p] * 9),
    ("gmm_aligner_posteriors_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_float,
      ctypes.c_uint32] + [ctypes.c_void_p] * 8),
    ("gmm_default_align_search", None, [ctypes.POINTER(AlignSearchStruct)]),
    ("gmm_aligner_align_search_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(AlignSearchStruct)]
     + [ctypes.c_void_p] * 8),
    ("gmm_aligner_align_search_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(AlignSearchStruct)]
     + [ctypes.c_void_p] * 7),
    ("gmm_aligner_posteriors_search_device", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(AlignSearchStruct), ctypes.c_float,
      ctypes.c_uint32] + [ctypes.c_void_p] * 11),
    ("gmm_aligner_posteriors_search_host", ctypes.c_int,
     [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(AlignSearchStruct), ctypes.c_float,
      ctypes.c_uint32] + [ctypes.c_void_p] * 10),
    ("gmm_version", ctypes.c_char_p, []),
    ("gmm_kernel_id", ctypes.c_char_p, []),
]

_lib = None


def load_library(path: str | None = None) -> ctypes.CDLL:
    """Load librasr_gmm.so (raises if it has not been built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"rasr_amd native library not found at {p}: the MI355X scorer has no fallback; "
            "build it with `make` (or __graft_entry__.build())")
    # Two HIP runtimes end up in a Python process: the image's ROCm (librasr_gmm.so's libamdhip64.so.7)
    # and the one bundled with torch.  When librasr_gmm.so is loaded before torch, torch's HIP calls partly
    # bind to the ROCm copy and, once torch has initialised the device, hipGetDeviceCount in the ROCm copy
    # fails ("no HIP device available"; scripts/debug/probe_order.py).  Loading torch first keeps each
    # library on its own runtime.  (C++ callers such as RASR have one runtime and are unaffected.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(p)
    for name, res, args in PROTOTYPES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


class GmmError(RuntimeError):
    code = None  # the status the call returned (GMM_ERR_*)


def check(rc: int, what: str = "") -> None:
    if rc != GMM_OK:
        msg = load_library().gmm_last_error()
        err = GmmError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        err.code = rc
        raise err
