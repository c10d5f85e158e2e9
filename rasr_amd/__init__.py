"""rasr_amd -- MI355X-native diagonal-GMM acoustic scorer behind RASR's
Mm::FeatureScorer plugin surface.

The product is the C-ABI library rasr_amd/lib/librasr_gmm.so (HIP kernels for
gfx950 + host-side model preparation); this package only binds it.
"""
from ._capi import (BATCH_DIAGONAL_MAXIMUM_FAST, BATCH_DIAGONAL_MAXIMUM_FLOAT, BATCH_DIAGONAL_MAXIMUM_INT,
                    DEFAULT_WEIGHT_THRESHOLD, DIAGONAL_MAXIMUM, LIB_PATH, SCORER_TYPES, SIMD_DIAGONAL_MAXIMUM, STATE_POSTERIOR_CHUNK,
                    GmmError, load_library)
from .aligner import Aligner, AlignSearch, batch_graphs, linear_hmm_graph
from .adaptation import AffineTransformAccumulator, estimate_affine_transform
from .estimator import (Estimator, combine_discriminative_estimators, combine_estimators, ebw_config,
                        ebw_iteration_constants, estimate_ebw)
from .mllr import MLLR_KINDS, MllrAccumulator, adapt_means, estimate_mllr
from .mixture_set import (MixtureSet, estimate_mixture_set, estimator_config, parse_mixture_set, ragged_counts,
                          read_mixture_set, synthetic_frames,
                          synthetic_mixture_set, write_mixture_set)
from .scorer import Scorer, default_config, float_spread_bound, pinned_empty, prepare_quantized_host

__all__ = [
    "BATCH_DIAGONAL_MAXIMUM_FAST", "BATCH_DIAGONAL_MAXIMUM_FLOAT", "BATCH_DIAGONAL_MAXIMUM_INT", "DIAGONAL_MAXIMUM",
    "SIMD_DIAGONAL_MAXIMUM", "SCORER_TYPES", "LIB_PATH", "GmmError", "load_library", "MixtureSet", "ragged_counts",
    "synthetic_frames", "synthetic_mixture_set", "Scorer", "default_config", "pinned_empty", "prepare_quantized_host",
    "read_mixture_set", "parse_mixture_set", "write_mixture_set", "estimate_mixture_set", "estimator_config",
    "Estimator", "combine_estimators", "combine_discriminative_estimators", "estimate_ebw", "ebw_iteration_constants",
    "ebw_config", "DEFAULT_WEIGHT_THRESHOLD", "STATE_POSTERIOR_CHUNK", "float_spread_bound",
    "AffineTransformAccumulator", "estimate_affine_transform",
    "MLLR_KINDS", "MllrAccumulator", "estimate_mllr", "adapt_means",
    "Aligner", "AlignSearch", "batch_graphs", "linear_hmm_graph",
]
