// affine_estimate_test.cc -- host check (no GPU, no HIP) of gmm_affine_estimate (include/rasr_gmm_adaptation.h,
// rasr_amd/csrc/host/AffineTransformEstimate.cc): the naive estimate solves G[i] w = k[i]; an mmiPrime sweep leaves
// every updated row a solution of Gales' row equation; the early return, the [D][D] initial transform, a singular G,
// hlda and the null arguments.  Linked against the estimate unit only, so it also runs under
// -fsanitize=address,undefined (make AFFINEEST_FLAGS="-fsanitize=address,undefined -g" build/tests/affine_estimate_test).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rasr_gmm_adaptation.h"

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

struct Tables {
    uint32_t            D;
    double              beta;
    std::vector<double> k, G, mean, cov;
};

// tables of n synthetic pairs: features from a fixed generator, per-row variances, means near the features
Tables makeTables(uint32_t D, uint32_t n, uint32_t seed) {
    uint64_t x    = 0x9e3779b97f4a7c15ull * (seed + 1);
    auto     next = [&x]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return static_cast<double>(x >> 11) / 9007199254740992.0 * 2.0 - 1.0;
    };
    const size_t D1 = D + 1;
    Tables       t{D, 0.0, std::vector<double>(D * D1, 0.0), std::vector<double>(D * D1 * D1, 0.0),
             std::vector<double>(D1, 0.0), std::vector<double>(D1 * D1, 0.0)};
    std::vector<double> v(D), xi(D1), mu(D);
    for (uint32_t i = 0; i < D; ++i)
        v[i] = 0.5 + std::fabs(next());
    for (uint32_t p = 0; p < n; ++p) {
        xi[0] = 1.0;
        for (uint32_t j = 0; j < D; ++j) {
            xi[j + 1] = 2.0 * next() + 0.3;
            mu[j]     = 0.8 * xi[j + 1] - 0.2 + 0.3 * next();
        }
        t.beta += 1.0;
        for (size_t i = 0; i < D; ++i)
            for (size_t j = 0; j < D1; ++j) {
                t.k[i * D1 + j] += mu[i] / v[i] * xi[j];
                for (size_t l = 0; l < D1; ++l)
                    t.G[i * D1 * D1 + j * D1 + l] += xi[j] * xi[l] / v[i];
            }
        for (size_t j = 0; j < D1; ++j) {
            t.mean[j] += xi[j];
            for (size_t l = 0; l < D1; ++l)
                t.cov[j * D1 + l] += xi[j] * xi[l];
        }
    }
    return t;
}

int estimate(const Tables& t, int criterion, uint32_t iterations, double minWeight, const double* initial, uint32_t columns,
             std::vector<float>& out) {
    out.assign(static_cast<size_t>(t.D) * (t.D + 1), -77.0f);
    return gmm_affine_estimate(t.D, t.beta, t.k.data(), t.G.data(), t.mean.data(), t.cov.data(), criterion, iterations,
                               minWeight, initial, columns, out.data());
}

void testNaive(uint32_t D) {
    const Tables       t = makeTables(D, 60 + 8 * D, D);
    const size_t       D1 = D + 1;
    std::vector<float> W;
    CHECK(estimate(t, GMM_AFFINE_NAIVE, 0, 0.0, nullptr, 0, W) == GMM_OK);
    // G[i] w_i = k[i], up to the f32 narrowing of w
    for (size_t i = 0; i < D; ++i)
        for (size_t j = 0; j < D1; ++j) {
            double s = 0.0, scale = std::fabs(t.k[i * D1 + j]);
            for (size_t l = 0; l < D1; ++l) {
                s += t.G[i * D1 * D1 + j * D1 + l] * W[i * D1 + l];
                scale += std::fabs(t.G[i * D1 * D1 + j * D1 + l] * W[i * D1 + l]);
            }
            CHECK(std::fabs(s - t.k[i * D1 + j]) <= 1e-6 * scale);
        }
    // naive ignores the observation weight threshold (cc:204)
    std::vector<float> W2;
    CHECK(estimate(t, GMM_AFFINE_NAIVE, 0, 1e30, nullptr, 0, W2) == GMM_OK);
    CHECK(std::memcmp(W.data(), W2.data(), W.size() * sizeof(float)) == 0);
}

void testMmiPrime(uint32_t D) {
    const Tables       t = makeTables(D, 60 + 8 * D, 100 + D);
    const size_t       D1 = D + 1;
    std::vector<float> W0, W1, W5;
    CHECK(estimate(t, GMM_AFFINE_MMI_PRIME, 0, 0.0, nullptr, 0, W0) == GMM_OK);
    for (size_t i = 0; i < D; ++i)  // no sweep: the identity
        for (size_t j = 0; j < D1; ++j)
            CHECK(W0[i * D1 + j] == (j == i + 1 ? 1.0f : 0.0f));
    CHECK(estimate(t, GMM_AFFINE_MMI_PRIME, 1, 0.0, nullptr, 0, W1) == GMM_OK);
    CHECK(estimate(t, GMM_AFFINE_MMI_PRIME, 5, 0.0, nullptr, 0, W5) == GMM_OK);
    bool finite = true, moved = false;
    for (size_t x = 0; x < W5.size(); ++x) {
        finite = finite && std::isfinite(W1[x]) && std::isfinite(W5[x]);
        moved  = moved || W1[x] != W5[x];
    }
    CHECK(finite);
    CHECK(moved || D == 1);  // D = 1: the row update does not depend on the cofactor's scale, one sweep converges
    // the last row of the last sweep solves G w = alpha * cofactors + k with cofactors[0] = 0: its first equation is
    // the plain one, sum_l G[0][l] w[l] = k[0]
    const size_t i = D - 1;
    double       s = 0.0, scale = std::fabs(t.k[i * D1]);
    for (size_t l = 0; l < D1; ++l) {
        s += t.G[i * D1 * D1 + l] * W5[i * D1 + l];
        scale += std::fabs(t.G[i * D1 * D1 + l] * W5[i * D1 + l]);
    }
    CHECK(std::fabs(s - t.k[i * D1]) <= 1e-6 * scale);
    // below the observation weight: the initial transform, [D][D] gaining its zero offset column
    std::vector<double> init(static_cast<size_t>(D) * D);
    for (size_t x = 0; x < init.size(); ++x)
        init[x] = 0.25 * static_cast<double>(x) - 1.0;
    std::vector<float> We;
    CHECK(estimate(t, GMM_AFFINE_MMI_PRIME, 3, t.beta + 1.0, init.data(), D, We) == GMM_OK);
    for (size_t r = 0; r < D; ++r) {
        CHECK(We[r * D1] == 0.0f);
        for (size_t j = 0; j < D; ++j)
            CHECK(We[r * D1 + j + 1] == static_cast<float>(init[r * D + j]));
    }
    // and [D][D+1] as it is
    std::vector<double> init1(static_cast<size_t>(D) * D1);
    for (size_t x = 0; x < init1.size(); ++x)
        init1[x] = 0.5 * static_cast<double>(x) + 2.0;
    CHECK(estimate(t, GMM_AFFINE_MMI_PRIME, 3, t.beta + 1.0, init1.data(), D + 1, We) == GMM_OK);
    for (size_t x = 0; x < init1.size(); ++x)
        CHECK(We[x] == static_cast<float>(init1[x]));
}

void testRefusals() {
    Tables             t = makeTables(4, 80, 7);
    std::vector<float> W;
    CHECK(estimate(t, GMM_AFFINE_HLDA, 1, 0.0, nullptr, 0, W) == GMM_ERR_UNSUPPORTED);
    CHECK(g_lastError.find("hlda") != std::string::npos);
    CHECK(estimate(t, 9, 1, 0.0, nullptr, 0, W) == GMM_ERR_INVALID_ARGUMENT);
    std::vector<double> init(4 * 7, 0.0);
    CHECK(estimate(t, GMM_AFFINE_NAIVE, 1, 0.0, init.data(), 7, W) == GMM_ERR_INVALID_ARGUMENT);
    CHECK(gmm_affine_estimate(4, t.beta, nullptr, t.G.data(), nullptr, nullptr, 0, 1, 0.0, nullptr, 0, W.data()) ==
          GMM_ERR_INVALID_ARGUMENT);
    CHECK(gmm_affine_estimate(0, t.beta, t.k.data(), t.G.data(), nullptr, nullptr, 0, 1, 0.0, nullptr, 0, W.data()) ==
          GMM_ERR_INVALID_ARGUMENT);
    // mean and cov are optional
    CHECK(gmm_affine_estimate(4, t.beta, t.k.data(), t.G.data(), nullptr, nullptr, GMM_AFFINE_MMI_PRIME, 2, 0.0, nullptr, 0,
                              W.data()) == GMM_OK);
    // a singular G: row 2's matrix with two equal rows and columns
    const size_t D1 = 5;
    for (size_t l = 0; l < D1; ++l)
        t.G[2 * D1 * D1 + 3 * D1 + l] = t.G[2 * D1 * D1 + 1 * D1 + l];
    for (size_t l = 0; l < D1; ++l)
        t.G[2 * D1 * D1 + l * D1 + 3] = t.G[2 * D1 * D1 + l * D1 + 1];
    t.G[2 * D1 * D1 + 3 * D1 + 3] = t.G[2 * D1 * D1 + 1 * D1 + 1];
    t.G[2 * D1 * D1 + 3 * D1 + 1] = t.G[2 * D1 * D1 + 1 * D1 + 1];
    t.G[2 * D1 * D1 + 1 * D1 + 3] = t.G[2 * D1 * D1 + 1 * D1 + 1];
    std::fill(W.begin(), W.end(), -77.0f);
    CHECK(estimate(t, GMM_AFFINE_NAIVE, 1, 0.0, nullptr, 0, W) == GMM_ERR_INVALID_ARGUMENT);
    CHECK(g_lastError.find("row 2") != std::string::npos && g_lastError.find("singular") != std::string::npos);
    // all zeros is singular too
    std::fill(t.G.begin(), t.G.end(), 0.0);
    CHECK(estimate(t, GMM_AFFINE_MMI_PRIME, 1, 0.0, nullptr, 0, W) == GMM_ERR_INVALID_ARGUMENT);
    CHECK(g_lastError.find("row 0") != std::string::npos);
}

}  // namespace

int main() {
    for (uint32_t D : {1u, 3u, 16u, 39u}) {
        testNaive(D);
        testMmiPrime(D);
    }
    testRefusals();
    if (g_failures) {
        std::printf("affine_estimate_test: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("affine_estimate_test: ok\n");
    return 0;
}
