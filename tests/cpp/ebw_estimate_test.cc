// ebw_estimate_test.cc -- host check (no GPU, no HIP) of the discriminative (EBW) estimator file: the writer
// (writeDiscriminativeEstimatorFile) and gmm_estimator_combine_discriminative (include/rasr_gmm_estimator.h,
// rasr_amd/csrc/host/MixtureSetEstimatorFile.cc).  A topology with shared means and unreferenced accumulators is written
// and compared byte for byte with the layout spelled out here; files are combined one, two and three at a time and
// compared with the file of the in-order f64 sums; every proper prefix of a file, a maximum-likelihood file, trailing
// bytes and mismatched files must be refused.  Then gmm_estimator_estimate_ebw on a ragged topology (4 mixtures of 1, 3, 2
// and 1 densities, pooled and one covariance per density, both constant types): equal numerator and denominator
// statistics give back the previous means exactly and the previous variances to f32 rounding; a density under the
// minimum observation weight leaves the model; the refusals.
// Linked against the two file units only, so it also runs under -fsanitize=address,undefined
// (make EBWEST_FLAGS="-fsanitize=address,undefined -g" build/tests/ebw_estimate_test).
#include <cmath>
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

typedef std::vector<unsigned char> Bytes;

struct Topology {
    uint32_t              D = 5, nMeans = 5, nCovs = 3;
    std::vector<uint32_t> dnsMean{3, 1, 1, 0, 4}, dnsCov{1, 1, 1, 0, 2};  // densities 1 and 2 share mean 1; density 4,
    std::vector<uint32_t> mixOff{0, 2, 2, 5}, mixDens{3, 1, 2, 3, 0};     // mean 2 / 4 and covariance 2 are unreferenced
    // first appearance over the mixtures' densities 3, 1, 2, 3, 0: new index -> old index
    std::vector<uint32_t> meanOrder{0, 1, 3}, covOrder{0, 1}, densOrder{3, 1, 2, 0};
    std::vector<uint32_t> fileDensMean{0, 1, 1, 2}, fileDensCov{0, 1, 1, 1};  // per new density: new mean, new covariance
    std::vector<uint32_t> fileMixDens{0, 1, 2, 0, 3};                         // per entry: new density
};

struct Stats {
    std::vector<double> meanSums, meanWeights, covSums, covWeights, entryWeights;
};

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

Stats add(const Stats& a, const Stats& b) {
    Stats r = a;
    for (size_t i = 0; i < r.meanSums.size(); ++i)
        r.meanSums[i] = r.meanSums[i] + b.meanSums[i];
    for (size_t i = 0; i < r.meanWeights.size(); ++i)
        r.meanWeights[i] = r.meanWeights[i] + b.meanWeights[i];
    for (size_t i = 0; i < r.covSums.size(); ++i)
        r.covSums[i] = r.covSums[i] + b.covSums[i];
    for (size_t i = 0; i < r.covWeights.size(); ++i)
        r.covWeights[i] = r.covWeights[i] + b.covWeights[i];
    for (size_t i = 0; i < r.entryWeights.size(); ++i)
        r.entryWeights[i] = r.entryWeights[i] + b.entryWeights[i];
    return r;
}

rasr_gmm::EstimatorTables tables(const Topology& t, const Stats& s) {
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
    return e;
}

Bytes write(const Topology& t, const Stats& num, const Stats& den, double objective) {
    rasr_gmm::DenominatorTables d{};
    d.meanSums     = den.meanSums.data();
    d.meanWeights  = den.meanWeights.data();
    d.covSums      = den.covSums.data();
    d.covWeights   = den.covWeights.data();
    d.entryWeights = den.entryWeights.data();
    d.objective    = objective;
    return rasr_gmm::writeDiscriminativeEstimatorFile(tables(t, num), d);
}

template <class T>
void put(Bytes& b, T v) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
    b.insert(b.end(), p, p + sizeof(T));
}
void putAccumulator(Bytes& b, const double* sums, uint32_t n, double weight) {
    put<uint32_t>(b, n);
    for (uint32_t k = 0; k < n; ++k)
        put<double>(b, sums[k]);
    put<double>(b, weight);
}

// the layout, spelled out: discriminative = false gives the maximum-likelihood file of the numerator
Bytes expected(const Topology& t, const Stats& num, const Stats& den, double objective, bool discriminative) {
    Bytes b{'M', 'I', 'X', 'S', 'E', 'T', 0, 0};
    put<uint32_t>(b, 2);
    put<uint32_t>(b, t.D);
    put<uint32_t>(b, static_cast<uint32_t>(t.meanOrder.size()));
    for (uint32_t m : t.meanOrder) {
        putAccumulator(b, &num.meanSums[m * t.D], t.D, num.meanWeights[m]);
        if (discriminative)
            putAccumulator(b, &den.meanSums[m * t.D], t.D, den.meanWeights[m]);
    }
    put<uint32_t>(b, static_cast<uint32_t>(t.covOrder.size()));
    for (uint32_t c : t.covOrder) {
        putAccumulator(b, &num.covSums[c * t.D], t.D, num.covWeights[c]);
        if (discriminative)
            putAccumulator(b, &den.covSums[c * t.D], t.D, den.covWeights[c]);
    }
    put<uint32_t>(b, static_cast<uint32_t>(t.densOrder.size()));
    for (size_t d = 0; d < t.densOrder.size(); ++d) {
        put<uint32_t>(b, t.fileDensMean[d]);
        put<uint32_t>(b, t.fileDensCov[d]);
    }
    put<uint32_t>(b, static_cast<uint32_t>(t.mixOff.size() - 1));
    for (size_t m = 0; m + 1 < t.mixOff.size(); ++m) {
        put<uint32_t>(b, t.mixOff[m + 1] - t.mixOff[m]);
        for (uint32_t e = t.mixOff[m]; e < t.mixOff[m + 1]; ++e) {
            put<uint32_t>(b, t.fileMixDens[e]);
            put<double>(b, num.entryWeights[e]);
        }
        if (discriminative)
            for (uint32_t e = t.mixOff[m]; e < t.mixOff[m + 1]; ++e)
                put<double>(b, den.entryWeights[e]);
    }
    if (discriminative)
        put<double>(b, objective);
    return b;
}

int combine(const std::vector<Bytes>& files, Bytes& out, bool discriminative = true) {
    std::vector<const void*> data;
    std::vector<uint64_t>    size;
    for (const Bytes& f : files) {
        data.push_back(f.data());
        size.push_back(f.size());
    }
    uint64_t   n  = 0;
    const auto fn = discriminative ? gmm_estimator_combine_discriminative : gmm_estimator_combine;
    int        rc = fn(data.data(), size.data(), static_cast<uint32_t>(files.size()), nullptr, 0, &n);
    if (rc != GMM_OK)
        return rc;
    out.assign(n, 0);
    if (n > 8) {  // the capacity check
        Bytes small(n - 1);
        uint64_t m = 0;
        CHECK(fn(data.data(), size.data(), static_cast<uint32_t>(files.size()), small.data(), n - 1, &m) == GMM_ERR_CAPACITY);
    }
    return fn(data.data(), size.data(), static_cast<uint32_t>(files.size()), out.data(), n, &n);
}

// ---- the estimate ----

struct Model {  // a previous mixture set in the file's numbering: mixtures of 1, 3, 2, 1 densities, a mean per density
    uint32_t              D = 5, nCovs;
    std::vector<uint32_t> dnsMean{0, 1, 2, 3, 4, 5, 6}, dnsCov, mixOff{0, 1, 4, 6, 7}, mixDens{0, 1, 2, 3, 4, 5, 6};
    std::vector<float>    means, variances;
    std::vector<double>   logWeights;
    explicit Model(bool pooled) : nCovs(pooled ? 1 : 7) {
        for (uint32_t d = 0; d < 7; ++d)
            dnsCov.push_back(pooled ? 0 : d);
        for (uint32_t i = 0; i < 7 * D; ++i)
            means.push_back(0.25f * static_cast<float>(i % 11) - 1.0f);
        for (uint32_t i = 0; i < nCovs * D; ++i)
            variances.push_back(0.5f + 0.125f * static_cast<float>(i % 7));
        const double w[7] = {1.0, 0.5, 0.3, 0.2, 0.6, 0.4, 1.0};
        for (double v : w)
            logWeights.push_back(std::log(v));
    }
    gmm_mixture_set set() const {
        gmm_mixture_set m{};
        m.dimension           = D;
        m.n_means             = 7;
        m.means               = const_cast<float*>(means.data());
        m.n_covariances       = nCovs;
        m.variances           = const_cast<float*>(variances.data());
        m.n_densities         = 7;
        m.density_mean        = const_cast<uint32_t*>(dnsMean.data());
        m.density_covariance  = const_cast<uint32_t*>(dnsCov.data());
        m.n_mixtures          = 4;
        m.mixture_offsets     = const_cast<uint32_t*>(mixOff.data());
        m.mixture_densities   = const_cast<uint32_t*>(mixDens.data());
        m.mixture_log_weights = const_cast<double*>(logWeights.data());
        return m;
    }
    // statistics of `weight[d]` observations per density lying on the model: sums w * mean, squares w * (var + mean^2)
    Stats stats(const std::vector<double>& weight) const {
        Stats s;
        s.meanSums.assign(7 * D, 0.0);
        s.meanWeights.assign(7, 0.0);
        s.covSums.assign(nCovs * D, 0.0);
        s.covWeights.assign(nCovs, 0.0);
        s.entryWeights = weight;
        for (uint32_t d = 0; d < 7; ++d) {
            const uint32_t c = dnsCov[d];
            s.meanWeights[d] += weight[d];
            s.covWeights[c] += weight[d];
            for (uint32_t k = 0; k < D; ++k) {
                const double mu = means[d * D + k];
                s.meanSums[d * D + k] += weight[d] * mu;
                s.covSums[c * D + k] += weight[d] * (variances[c * D + k] + mu * mu);
            }
        }
        return s;
    }
    Bytes file(const Stats& num, const Stats& den) const {
        Topology t;
        t.D = D, t.nMeans = 7, t.nCovs = nCovs;
        t.dnsMean = dnsMean, t.dnsCov = dnsCov, t.mixOff = mixOff, t.mixDens = mixDens;
        return write(t, num, den, 0.0);
    }
};

void estimateChecks(bool pooled, int type) {
    const Model           model(pooled);
    const gmm_mixture_set prev = model.set();
    gmm_ebw_config        cfg;
    gmm_default_ebw_config(&cfg);
    cfg.iteration_constants_type = type;
    const std::vector<double> w{40, 30, 50, 20, 25, 35, 45};
    // numerator == denominator: dtSum = 0, dtWeight = 0, so every mean is (ic * previous) / ic
    {
        const Stats     s = model.stats(w);
        const Bytes     f = model.file(s, s);
        gmm_mixture_set out{};
        CHECK(gmm_estimator_estimate_ebw(f.data(), f.size(), &prev, &cfg, &out) == GMM_OK);
        CHECK(out.n_means == 7 && out.n_densities == 7 && out.n_covariances == model.nCovs && out.n_mixtures == 4);
        CHECK(out.mixture_offsets && out.mixture_offsets[4] == 7);
        for (uint32_t i = 0; out.means && i < 7 * model.D; ++i)
            CHECK(out.means[i] == model.means[i]);
        for (uint32_t i = 0; out.variances && i < model.nCovs * model.D; ++i)
            CHECK(std::fabs(out.variances[i] - model.variances[i]) <= 1e-5f * model.variances[i]);
        for (uint32_t m = 0; out.mixture_log_weights && m < 4; ++m) {  // normalised weights
            double sum = 0;
            for (uint32_t e = out.mixture_offsets[m]; e < out.mixture_offsets[m + 1]; ++e)
                sum += std::exp(out.mixture_log_weights[e]);
            CHECK(std::fabs(sum - 1.0) < 1e-12);
        }
        gmm_mixture_set_free(&out);
        double   ic[7];
        uint32_t n = 0;
        CHECK(gmm_estimator_ebw_iteration_constants(f.data(), f.size(), &prev, &cfg, ic, 7, &n) == GMM_OK && n == 7);
        for (uint32_t d = 0; d < n; ++d)
            CHECK(ic[d] >= 1.0 && std::isfinite(ic[d]));
        CHECK(gmm_estimator_ebw_iteration_constants(f.data(), f.size(), &prev, &cfg, ic, 6, &n) == GMM_ERR_CAPACITY);
    }
    // a real update, and densities under the minimum observation weight: the first and the last of mixture 1 leave
    {
        std::vector<double> low = w;
        low[1] = 1.0, low[3] = 2.0;
        Stats num = model.stats(low), den = model.stats(w);
        for (double& v : den.meanSums)
            v *= 0.45;
        for (double& v : den.meanWeights)
            v *= 0.5;
        for (double& v : den.covSums)
            v *= 0.5;
        for (double& v : den.covWeights)
            v *= 0.5;
        for (double& v : den.entryWeights)
            v *= 0.5;
        const Bytes     f = model.file(num, den);
        gmm_mixture_set out{};
        CHECK(gmm_estimator_estimate_ebw(f.data(), f.size(), &prev, &cfg, &out) == GMM_OK);
        CHECK(out.n_densities == 5 && out.n_means == 5 && out.n_covariances == (pooled ? 1u : 5u));
        CHECK(out.mixture_offsets && out.mixture_offsets[1] == 1 && out.mixture_offsets[2] == 2 && out.mixture_offsets[4] == 5);
        bool moved = false;
        for (uint32_t i = 0; out.means && i < 5 * model.D; ++i) {
            CHECK(std::isfinite(out.means[i]));
            moved = moved || out.means[i] != model.means[(i / model.D == 0 ? 0 : i / model.D + (i / model.D >= 2 ? 2 : 1)) * model.D + i % model.D];
        }
        CHECK(moved);
        for (uint32_t i = 0; out.variances && i < out.n_covariances * model.D; ++i)
            CHECK(out.variances[i] > 0);
        gmm_mixture_set_free(&out);
        cfg.minimum_variance = 100.0;
        CHECK(gmm_estimator_estimate_ebw(f.data(), f.size(), &prev, &cfg, &out) == GMM_OK);
        for (uint32_t i = 0; out.variances && i < out.n_covariances * model.D; ++i)
            CHECK(out.variances[i] == 100.0f);
        gmm_mixture_set_free(&out);
        cfg.minimum_variance = 0.0;
        // refusals
        CHECK(gmm_estimator_estimate_ebw(f.data(), f.size() - 1, &prev, &cfg, &out) == GMM_ERR_INVALID_ARGUMENT);
        const Model           other(!pooled);
        const gmm_mixture_set otherSet = other.set();
        CHECK(gmm_estimator_estimate_ebw(f.data(), f.size(), &otherSet, &cfg, &out) == GMM_ERR_INVALID_ARGUMENT);
        cfg.iteration_constants_type = GMM_EBW_CAMBRIDGE;
        CHECK(gmm_estimator_estimate_ebw(f.data(), f.size(), &prev, &cfg, &out) == GMM_ERR_UNSUPPORTED);
        cfg.iteration_constants_type = type;
        // a density held by two mixture entries: the same counts, mixture 2 holds density 2 (which stays in mixture 1) again
        Bytes shared = f;
        const size_t lastMixture = 4 + 12 + 8 + 8;                      // count, entry, denominator weight, objective
        const size_t mixture2    = lastMixture + 4 + 2 * 12 + 2 * 8;    // back from the end to mixture 2's count
        const uint32_t one       = 2;
        std::memcpy(&shared[shared.size() - mixture2 + 4], &one, 4);  // its first entry's density index
        CHECK(gmm_estimator_estimate_ebw(shared.data(), shared.size(), &prev, &cfg, &out) == GMM_ERR_UNSUPPORTED);
    }
}

}  // namespace

int main() {
    for (int pooled = 0; pooled < 2; ++pooled)
        for (int type : {GMM_EBW_GLOBAL_RWTH, GMM_EBW_LOCAL_RWTH})
            estimateChecks(pooled != 0, type);

    const Topology t;
    const Stats    n0 = makeStats(t, 0), d0 = makeStats(t, 1), n1 = makeStats(t, 2), d1 = makeStats(t, 3), n2 = makeStats(t, 4),
                d2 = makeStats(t, 5);
    const Bytes f0 = write(t, n0, d0, 1e16), f1 = write(t, n1, d1, 1.0), f2 = write(t, n2, d2, -1e16);

    // the writer against the layout; the maximum-likelihood writer unchanged beside it
    CHECK(f0 == expected(t, n0, d0, 1e16, true));
    const Bytes ml0 = rasr_gmm::writeEstimatorFile(tables(t, n0));
    CHECK(ml0 == expected(t, n0, d0, 0, false));
    CHECK(f0.size() == ml0.size() + 5 * (4 + 8 * t.D + 8) + 5 * 8 + 8);

    // read and written back; two and three files in order
    Bytes out;
    CHECK(combine({f0}, out) == GMM_OK && out == f0);
    CHECK(combine({f0, f1}, out) == GMM_OK && out == expected(t, add(n0, n1), add(d0, d1), 1e16 + 1.0, true));
    CHECK(combine({f0, f1, f2}, out) == GMM_OK &&
          out == expected(t, add(add(n0, n1), n2), add(add(d0, d1), d2), (1e16 + 1.0) + -1e16, true));
    Bytes other;
    CHECK(combine({f2, f1, f0}, other) == GMM_OK && other != out);  // the order shows

    // refusals: every proper prefix, trailing bytes, a maximum-likelihood file, mismatched files, no file
    for (size_t cut = 0; cut < f0.size(); ++cut)
        CHECK(combine({Bytes(f0.begin(), f0.begin() + static_cast<long>(cut))}, out) == GMM_ERR_INVALID_ARGUMENT);
    Bytes longer = f0;
    longer.push_back(0);
    CHECK(combine({longer}, out) == GMM_ERR_INVALID_ARGUMENT);
    CHECK(combine({ml0}, out) == GMM_ERR_INVALID_ARGUMENT);
    CHECK(combine({f0, ml0}, out) == GMM_ERR_INVALID_ARGUMENT);
    CHECK(combine({ml0}, out, false) == GMM_OK && out == ml0);  // gmm_estimator_combine still takes it
    Bytes version = f1;
    version[8]    = 1;
    CHECK(combine({f0, version}, out) == GMM_ERR_INVALID_ARGUMENT);
    Topology u;
    u.mixOff = {0, 2, 3, 5};  // another mixture layout over the same densities
    CHECK(combine({f0, write(u, n1, d1, 0.0)}, out) == GMM_ERR_INVALID_ARGUMENT);
    Topology v;
    v.dnsCov = {1, 1, 0, 0, 2};  // another density table
    CHECK(combine({f0, write(v, n1, d1, 0.0)}, out) == GMM_ERR_INVALID_ARGUMENT);
    Bytes index = f0;  // a density index out of range in the last mixture's last entry
    std::memset(&index[index.size() - 8 - 3 * 8 - 12], 0x7f, 4);
    CHECK(combine({index}, out) == GMM_ERR_INVALID_ARGUMENT);
    CHECK(combine({}, out) == GMM_ERR_INVALID_ARGUMENT);

    if (g_failures) {
        std::printf("ebw_estimate_test: %d FAILED\n", g_failures);
        return 1;
    }
    std::printf("ebw_estimate_test: ok\n");
    return 0;
}
