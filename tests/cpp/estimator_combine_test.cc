// estimator_combine_test.cc -- host check (no GPU, no HIP) of the estimator file writer and gmm_estimator_combine
// (include/rasr_gmm_estimator.h, rasr_amd/csrc/host/MixtureSetEstimatorFile.cc): files of one topology with shared
// means and unreferenced accumulators are written, combined two and three at a time and compared byte for byte
// with the file of the in-order f64 sums; the malformed inputs must be refused; the result must estimate.
// Linked against the two file units only, so it also runs under -fsanitize=address,undefined
// (make ESTCOMBINE_FLAGS="-fsanitize=address,undefined -g" build/tests/estimator_combine_test).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../rasr_amd/csrc/gmm_estimator.hh"

// what gmm_api.cc provides in the library
static std::string g_lastError;
namespace rasr_gmm {
void setLastError(const std::string& msg) { g_lastError = msg; }
}  // namespace rasr_gmm
extern "C" const char* gmm_last_error(void) { return g_lastError.c_str(); }

namespace {

int g_failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failures;                                                   \
        }                                                                   \
    } while (0)

struct Topology {
    uint32_t              D = 5, nMeans = 5, nCovs = 3;
    std::vector<uint32_t> dnsMean{3, 1, 1, 0, 4}, dnsCov{1, 1, 1, 0, 2};  // densities 1 and 2 share mean 1; density 4,
    std::vector<uint32_t> mixOff{0, 2, 2, 5}, mixDens{3, 1, 2, 3, 0};     // mean 2 / 4 and covariance 2 are unreferenced
};

struct Stats {
    std::vector<double> meanSums, meanWeights, covSums, covWeights, entryWeights;
};

// a deterministic fill with values that do not add exactly
Stats makeStats(const Topology& t, uint32_t seed) {
    uint64_t x    = 0x9e3779b97f4a7c15ull * (seed + 1);
    auto     next = [&x]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return static_cast<double>(x >> 11) / 9007199254740992.0 * 1000.0 + 1e-3;
    };
    Stats s;
    for (size_t i = 0; i < static_cast<size_t>(t.nMeans) * t.D; ++i)
        s.meanSums.push_back(next() - 500.0);
    for (size_t i = 0; i < t.nMeans; ++i)
        s.meanWeights.push_back(next());
    for (size_t i = 0; i < static_cast<size_t>(t.nCovs) * t.D; ++i)
        s.covSums.push_back(next() * 1000.0);
    for (size_t i = 0; i < t.nCovs; ++i)
        s.covWeights.push_back(next());
    for (size_t i = 0; i < t.mixDens.size(); ++i)
        s.entryWeights.push_back(next());
    return s;
}

std::vector<unsigned char> write(const Topology& t, const Stats& s) {
    rasr_gmm::EstimatorTables e{};
    e.D            = t.D;
    e.nMeans       = t.nMeans;
    e.nCovs        = t.nCovs;
    e.nDens        = static_cast<uint32_t>(t.dnsMean.size());
    e.nMix         = static_cast<uint32_t>(t.mixOff.size() - 1);
    e.dnsMean      = t.dnsMean.data();
    e.dnsCov       = t.dnsCov.data();
    e.mixOff       = t.mixOff.data();
    e.mixDens      = t.mixDens.data();
    e.meanSums     = s.meanSums.data();
    e.meanWeights  = s.meanWeights.data();
    e.covSums      = s.covSums.data();
    e.covWeights   = s.covWeights.data();
    e.entryWeights = s.entryWeights.data();
    return rasr_gmm::writeEstimatorFile(e);
}

void addInto(std::vector<double>& a, const std::vector<double>& b) {
    for (size_t i = 0; i < a.size(); ++i)
        a[i] = a[i] + b[i];
}

int combine(const std::vector<std::vector<unsigned char>>& files, std::vector<unsigned char>& out) {
    std::vector<const void*> data;
    std::vector<uint64_t>    size;
    for (const auto& f : files) {
        data.push_back(f.data());
        size.push_back(f.size());
    }
    uint64_t n  = 0;
    int      rc = gmm_estimator_combine(data.data(), size.data(), static_cast<uint32_t>(files.size()), nullptr, 0, &n);
    if (rc != GMM_OK)
        return rc;
    out.assign(n, 0);
    if (n > 1) {  // too small a buffer is refused and not written
        unsigned char guard[1] = {0x5a};
        uint64_t      m        = 0;
        CHECK(gmm_estimator_combine(data.data(), size.data(), static_cast<uint32_t>(files.size()), guard, 1, &m) ==
              GMM_ERR_CAPACITY);
        CHECK(guard[0] == 0x5a && m == n);
    }
    return gmm_estimator_combine(data.data(), size.data(), static_cast<uint32_t>(files.size()), out.data(), out.size(), &n);
}

}  // namespace

int main() {
    const Topology t;
    const Stats    a = makeStats(t, 1), b = makeStats(t, 2), c = makeStats(t, 3);
    const auto     fa = write(t, a), fb = write(t, b), fc = write(t, c);

    // the writer: magic, version 2, dimension; 3 of 5 means and 2 of 3 covariances are referenced, renumbered by
    // first appearance (mean 0 first: mixture 0 starts with density 3)
    CHECK(fa.size() > 20 && std::memcmp(fa.data(), "MIXSET\0\0", 8) == 0);
    uint32_t word[3];
    std::memcpy(word, fa.data() + 8, 12);
    CHECK(word[0] == 2 && word[1] == t.D && word[2] == 3);
    double firstSum;
    std::memcpy(&firstSum, fa.data() + 24, 8);
    CHECK(firstSum == a.meanSums[0 * t.D]);

    // two and three files: the in-order f64 sums, byte for byte
    Stats s2 = a;
    for (auto p : {&Stats::meanSums, &Stats::meanWeights, &Stats::covSums, &Stats::covWeights, &Stats::entryWeights})
        addInto(s2.*p, b.*p);
    Stats s3 = s2;
    for (auto p : {&Stats::meanSums, &Stats::meanWeights, &Stats::covSums, &Stats::covWeights, &Stats::entryWeights})
        addInto(s3.*p, c.*p);
    std::vector<unsigned char> out;
    CHECK(combine({fa, fb}, out) == GMM_OK && out == write(t, s2));
    CHECK(combine({fa, fb, fc}, out) == GMM_OK && out == write(t, s3));
    std::vector<unsigned char> one;
    CHECK(combine({fa}, one) == GMM_OK && one == fa);

    // the combined file estimates
    gmm_estimator_config cfg;
    gmm_default_estimator_config(&cfg);
    cfg.minimum_observation_weight = 0;
    cfg.allow_zero_weights         = 1;
    gmm_mixture_set ms;
    // mixture 1 is empty: the reader refuses it (densityIndexWithMaxWeight's verify), as the reference does
    CHECK(gmm_mixture_set_estimate(out.data(), out.size(), &cfg, &ms) == GMM_ERR_INVALID_ARGUMENT);
    Topology full = t;
    full.mixOff   = {0, 2, 5};
    // covariance weights must match their means' for the estimate: use consistent statistics
    Stats k = a;
    std::fill(k.meanWeights.begin(), k.meanWeights.end(), 0.0);
    std::fill(k.covWeights.begin(), k.covWeights.end(), 0.0);
    for (size_t e = 0; e < full.mixDens.size(); ++e) {
        k.meanWeights[full.dnsMean[full.mixDens[e]]] += k.entryWeights[e];
        k.covWeights[full.dnsCov[full.mixDens[e]]] += k.entryWeights[e];
    }
    const auto fk = write(full, k);
    CHECK(combine({fk, fk}, out) == GMM_OK);
    const int rcEst = gmm_mixture_set_estimate(out.data(), out.size(), &cfg, &ms);
    CHECK(rcEst == GMM_OK);
    if (rcEst == GMM_OK) {
        CHECK(ms.n_mixtures == 2 && ms.n_means == 3 && ms.n_covariances == 2 && ms.n_densities == 4);
        gmm_mixture_set_free(&ms);
    }

    // refused inputs
    auto expectInvalid = [&](std::vector<std::vector<unsigned char>> files, const char* what) {
        std::vector<unsigned char> o;
        const int                  rc = combine(files, o);
        if (rc != GMM_ERR_INVALID_ARGUMENT) {
            std::printf("FAILED: %s gave %d\n", what, rc);
            ++g_failures;
        }
    };
    auto v = fb;
    v[8]   = 1;  // version
    expectInvalid({fa, v}, "version mismatch");
    Topology t6 = t;
    t6.D        = 6;
    expectInvalid({fa, write(t6, makeStats(t6, 4))}, "dimension mismatch");
    Topology td = t;
    td.dnsCov   = {1, 1, 1, 1, 2};  // density 3 on another covariance
    expectInvalid({fa, write(td, b)}, "density table mismatch");
    Topology tm = t;
    tm.mixDens  = {3, 1, 2, 0, 3};
    expectInvalid({fa, write(tm, b)}, "mixture mismatch");
    for (size_t cut : {size_t(0), size_t(7), size_t(12), size_t(30), fb.size() / 2, fb.size() - 1})
        expectInvalid({fa, std::vector<unsigned char>(fb.begin(), fb.begin() + static_cast<long>(cut))}, "truncation");
    v    = fb;
    v[0] = 'N';
    expectInvalid({fa, v}, "bad magic");
    expectInvalid({v, fa}, "bad magic (first file)");
    expectInvalid({}, "no files");
    // a huge accumulator size in a short file must not be allocated
    v = std::vector<unsigned char>(fb.begin(), fb.begin() + 24);
    const uint32_t huge = 0xfffffff0u;
    std::memcpy(v.data() + 20, &huge, 4);
    expectInvalid({fa, v}, "oversized accumulator");

    if (g_failures) {
        std::printf("estimator_combine_test: %d FAILED\n", g_failures);
        return 1;
    }
    std::printf("estimator_combine_test: ok\n");
    return 0;
}
