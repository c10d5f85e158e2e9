// PairTopology.hh -- a gmm_mixture_set's index tables validated and expanded per mixture entry: what every handle that
// accumulates (frame, mixture, density) pairs resolves a pair with (gmm_pairaccum.hh).  Plain C++, no HIP.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/rasr_gmm.h"

namespace rasr_gmm {

struct PairTopology {
    std::vector<uint32_t> mixOff;                // [nMix + 1]
    std::vector<uint32_t> entryMean, entryCov;   // [nEntries]: the mean / covariance of the entry's density
    uint32_t              nEntries   = 0;
    uint32_t              maxEntries = 1;        // the largest entry count of a mixture (at least 1)
    bool                  oneDensityPerMixture = false;
};

// GMM_OK, or GMM_ERR_INVALID_ARGUMENT with *message = "<prefix>: ..." for offsets that do not start at 0 or decrease,
// a density whose mean or covariance is out of range, a mixture entry whose density is out of range.  The pointers of
// ms that the counts make necessary are not NULL (the callers' own checks).
int expandPairTopology(const gmm_mixture_set& ms, const char* prefix, PairTopology& out, std::string* message);

}  // namespace rasr_gmm
