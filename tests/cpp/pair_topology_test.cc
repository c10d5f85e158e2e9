// pair_topology_test.cc -- host/PairTopology.cc alone (no GPU, no HIP): the expansion of a mixture set's index tables
// per mixture entry, and the code and the exact message of every malformed input under each of the three prefixes the
// library uses.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../rasr_amd/csrc/host/PairTopology.hh"

using namespace rasr_gmm;

namespace {

int failures = 0;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

// 4 mixtures / 6 densities / D = 3; density 2 is shared by mixtures 0 and 2, mixture 1 is empty
struct Model {
    std::vector<uint32_t> densityMean{0, 1, 2, 3, 4, 1};
    std::vector<uint32_t> densityCov{0, 0, 1, 1, 2, 2};
    std::vector<uint32_t> mixOff{0, 3, 3, 5, 7};
    std::vector<uint32_t> mixDens{0, 1, 2, 2, 3, 4, 5};
    gmm_mixture_set set() const {
        gmm_mixture_set ms{};
        ms.dimension          = 3;
        ms.n_means            = 5;
        ms.n_covariances      = 3;
        ms.n_densities        = 6;
        ms.n_mixtures         = static_cast<uint32_t>(mixOff.size() - 1);
        ms.density_mean       = densityMean.data();
        ms.density_covariance = densityCov.data();
        ms.mixture_offsets    = mixOff.data();
        ms.mixture_densities  = mixDens.data();
        return ms;
    }
};

const char* const kPrefixes[3] = {"estimator topology", "affine accumulator", "mllr accumulator"};

void expectInvalid(const Model& m, const std::string& text) {
    for (const char* prefix : kPrefixes) {
        PairTopology t;
        std::string  message = "untouched";
        const gmm_mixture_set ms = m.set();
        CHECK(expandPairTopology(ms, prefix, t, &message) == GMM_ERR_INVALID_ARGUMENT);
        CHECK(message == std::string(prefix) + ": " + text);
    }
}

}  // namespace

int main() {
    {
        const Model m;
        for (const char* prefix : kPrefixes) {
            PairTopology t;
            std::string  message;
            const gmm_mixture_set ms = m.set();
            CHECK(expandPairTopology(ms, prefix, t, &message) == GMM_OK);
            CHECK(message.empty());
            CHECK(t.mixOff == m.mixOff);
            CHECK(t.nEntries == 7);
            CHECK((t.entryMean == std::vector<uint32_t>{0, 1, 2, 2, 3, 4, 1}));
            CHECK((t.entryCov == std::vector<uint32_t>{0, 0, 1, 1, 1, 2, 2}));
            CHECK(!t.oneDensityPerMixture);
            CHECK(t.maxEntries == 3);
        }
    }
    {  // one density per mixture; the largest mixture counts at least 1
        Model m;
        m.mixOff  = {0, 1, 2};
        m.mixDens = {4, 2};
        PairTopology t;
        std::string  message;
        const gmm_mixture_set ms = m.set();
        CHECK(expandPairTopology(ms, kPrefixes[0], t, &message) == GMM_OK);
        CHECK(t.oneDensityPerMixture && t.maxEntries == 1 && t.nEntries == 2);
        CHECK((t.entryMean == std::vector<uint32_t>{4, 2}) && (t.entryCov == std::vector<uint32_t>{2, 1}));
    }
    {  // no mixture at all
        Model m;
        m.mixOff = {0};
        m.mixDens.clear();
        PairTopology t;
        std::string  message;
        const gmm_mixture_set ms = m.set();
        CHECK(expandPairTopology(ms, kPrefixes[1], t, &message) == GMM_OK);
        CHECK(t.oneDensityPerMixture && t.maxEntries == 1 && t.nEntries == 0 && t.entryMean.empty());
    }
    {
        Model m;
        m.mixOff[0] = 1;
        expectInvalid(m, "mixture_offsets[0] is not 0");
    }
    {
        Model m;
        m.mixOff = {0, 3, 2, 5, 7};
        expectInvalid(m, "mixture_offsets decrease at mixture 1");
    }
    {
        Model m;
        m.densityMean[4] = 5;
        expectInvalid(m, "density 4 refers to a mean or covariance out of range");
    }
    {
        Model m;
        m.densityCov[1] = 3;
        expectInvalid(m, "density 1 refers to a mean or covariance out of range");
    }
    {
        Model m;
        m.mixDens[5] = 6;
        expectInvalid(m, "mixture entry 5 refers to a density out of range");
    }
    if (failures) {
        std::printf("pair_topology_test: %d check(s) failed\n", failures);
        return EXIT_FAILURE;
    }
    std::printf("pair_topology_test: ok\n");
    return EXIT_SUCCESS;
}
