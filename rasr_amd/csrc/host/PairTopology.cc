// PairTopology.cc -- see PairTopology.hh.  The one place that validates a mixture set's index tables for the
// estimator, the affine and the MLLR accumulators.
#include "PairTopology.hh"

#include <algorithm>

namespace rasr_gmm {

int expandPairTopology(const gmm_mixture_set& ms, const char* prefix, PairTopology& out, std::string* message) {
    const std::string p    = std::string(prefix) + ": ";
    const uint32_t    nMix = ms.n_mixtures;
    auto invalid = [&](const std::string& what) {
        *message = p + what;
        return static_cast<int>(GMM_ERR_INVALID_ARGUMENT);
    };
    out.mixOff.assign(ms.mixture_offsets, ms.mixture_offsets + nMix + 1);
    if (out.mixOff[0] != 0)
        return invalid("mixture_offsets[0] is not 0");
    for (uint32_t m = 0; m < nMix; ++m)
        if (out.mixOff[m + 1] < out.mixOff[m])
            return invalid("mixture_offsets decrease at mixture " + std::to_string(m));
    out.nEntries = out.mixOff[nMix];
    for (uint32_t d = 0; d < ms.n_densities; ++d)
        if (ms.density_mean[d] >= ms.n_means || ms.density_covariance[d] >= ms.n_covariances)
            return invalid("density " + std::to_string(d) + " refers to a mean or covariance out of range");
    out.entryMean.resize(out.nEntries);
    out.entryCov.resize(out.nEntries);
    for (uint32_t i = 0; i < out.nEntries; ++i) {
        const uint32_t d = ms.mixture_densities[i];
        if (d >= ms.n_densities)
            return invalid("mixture entry " + std::to_string(i) + " refers to a density out of range");
        out.entryMean[i] = ms.density_mean[d];
        out.entryCov[i]  = ms.density_covariance[d];
    }
    out.oneDensityPerMixture = true;
    out.maxEntries           = 1;
    for (uint32_t m = 0; m < nMix; ++m) {
        const uint32_t n         = out.mixOff[m + 1] - out.mixOff[m];
        out.oneDensityPerMixture = out.oneDensityPerMixture && n == 1;
        out.maxEntries           = std::max(out.maxEntries, n);
    }
    return GMM_OK;
}

}  // namespace rasr_gmm
