// mllr_estimate_test.cc -- host check (no GPU, no HIP) of gmm_mllr_estimate and gmm_mllr_adapt_means
// (include/rasr_gmm_mllr.h, rasr_amd/csrc/host/MllrEstimate.cc) on a ragged tree: features that are an exact affine
// map of the means give that map back through Z * pinv(G), also where G is rank deficient; the thresholds decide which
// id serves a leaf; the silence mixtures take ids of their own; the adapted means; the refusals.  Linked against the
// estimate unit only, so it also runs under -fsanitize=address,undefined
// (make MLLREST_FLAGS="-fsanitize=address,undefined -g" build/tests/mllr_estimate_test).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/rasr_gmm_mllr.h"

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

constexpr uint32_t N = GMM_MLLR_NO_ID;

struct Rng {
    uint64_t x;
    double   next() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return static_cast<double>(x >> 11) / 9007199254740992.0 * 2.0 - 1.0;
    }
};

// A ragged tree of 7 ids: 0 = (1, 2), 2 = (3, 4), 4 = (5, 6); the leaves 1, 3, 5, 6 carry the leaf numbers 0, 1, 2, 3.
// Leaf 4 lies outside the tree (the silence leaf).
struct Tree {
    std::vector<uint32_t> left{1, N, 3, N, 5, N, N}, right{2, N, 4, N, 6, N, N}, parent{N, 0, 0, 2, 2, 4, 4},
            leafNumber{N, 0, N, 1, N, 2, 3};
    uint32_t root = 0;
};

struct Case {
    uint32_t              D, nLeaves = 5, nMix = 12;
    std::vector<double>   Z, G, count, beta, shift, A, b;
    std::vector<uint32_t> leafOfMixture{0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1};
};

// per leaf `pairs[leaf]` pairs: mean drawn, x = A mu + b exactly in f64 (distinct means only `distinct` of them)
Case makeCase(uint32_t D, const std::vector<uint32_t>& pairs, uint32_t distinct) {
    Case         c;
    const size_t D1 = D + 1;
    c.D = D;
    Rng rng{0x9e3779b97f4a7c15ull * (D + 3)};
    c.A.assign(D * D, 0.0);
    c.b.assign(D, 0.0);
    for (size_t i = 0; i < D; ++i) {
        c.b[i] = rng.next();
        for (size_t j = 0; j < D; ++j)
            c.A[i * D + j] = (i == j ? 1.5 : 0.0) + 0.1 * rng.next();
    }
    c.Z.assign(c.nLeaves * D * D1, 0.0);
    c.G.assign(c.nLeaves * D1 * D1, 0.0);
    c.count.assign(c.nLeaves, 0.0);
    c.beta.assign(c.nLeaves * D, 0.0);
    c.shift.assign(c.nLeaves * D, 0.0);
    std::vector<double> pool(static_cast<size_t>(distinct) * D);
    for (double& v : pool)
        v = 2.0 * rng.next();
    std::vector<double> m(D1), x(D);
    for (uint32_t leaf = 0; leaf < c.nLeaves; ++leaf)
        for (uint32_t p = 0; p < pairs[leaf]; ++p) {
            const double* mu = &pool[static_cast<size_t>((p + leaf) % distinct) * D];
            m[0] = 1.0;
            for (size_t j = 0; j < D; ++j)
                m[j + 1] = mu[j];
            for (size_t i = 0; i < D; ++i) {
                x[i] = c.b[i];
                for (size_t j = 0; j < D; ++j)
                    x[i] += c.A[i * D + j] * mu[j];
            }
            const double w = 1.0;
            c.count[leaf] += 1.0;
            for (size_t i = 0; i < D; ++i) {
                for (size_t j = 0; j < D1; ++j)
                    c.Z[(leaf * D + i) * D1 + j] += w * x[i] * m[j];
                c.beta[leaf * D + i] += w / 0.5;
                c.shift[leaf * D + i] += w * (x[i] - mu[i]) / 0.5;
            }
            for (size_t i = 0; i < D1; ++i)
                for (size_t j = 0; j < D1; ++j)
                    c.G[(leaf * D1 + i) * D1 + j] += w * m[i] * m[j];
        }
    return c;
}

struct Result {
    int                   rc;
    uint32_t              n = 0;
    std::vector<uint32_t> ids, ofMixture;
    std::vector<double>   matrices;
};

Result estimate(const Case& c, const Tree& t, int kind, const std::vector<uint32_t>& silence, double minObs, double minSil) {
    Result r;
    const size_t cap = t.left.size() + silence.size();
    r.ids.assign(cap, 777);
    r.matrices.assign(cap * c.D * (c.D + 1), -77.0);
    r.ofMixture.assign(c.nMix, 777);
    r.rc = gmm_mllr_estimate(c.D, kind, c.nLeaves, c.Z.data(), c.G.data(), c.count.data(), c.beta.data(), c.shift.data(),
                             c.leafOfMixture.data(), c.nMix, static_cast<uint32_t>(t.left.size()), t.left.data(), t.right.data(),
                             t.parent.data(), t.leafNumber.data(), t.root, silence.data(), static_cast<uint32_t>(silence.size()),
                             minObs, minSil, &r.n, r.ids.data(), r.matrices.data(), r.ofMixture.data());
    return r;
}

// the matrix at position at equals [b A] to a relative 1e-8
bool isMap(const Case& c, const Result& r, uint32_t at) {
    const size_t D = c.D, D1 = D + 1;
    bool         ok = true;
    for (size_t i = 0; i < D; ++i)
        for (size_t j = 0; j < D1; ++j) {
            const double want = j == 0 ? c.b[i] : c.A[i * D + j - 1];
            ok = ok && std::fabs(r.matrices[(at * D + i) * D1 + j] - want) <= 1e-8;
        }
    return ok;
}

bool isUnit(const Case& c, const Result& r, uint32_t at) {
    const size_t D = c.D, D1 = D + 1;
    bool         ok = true;
    for (size_t i = 0; i < D; ++i)
        for (size_t j = 0; j < D1; ++j)
            ok = ok && r.matrices[(at * D + i) * D1 + j] == (j == i + 1 ? 1.0 : 0.0);
    return ok;
}

void testFull(uint32_t D) {
    const Tree t;
    // leaves 0 .. 3 hold 40, 3, 30, 2 pairs; the silence leaf 50
    const Case c = makeCase(D, {40 + 4 * D, 3, 30 + 4 * D, 2, 50 + 4 * D}, 2 * D + 8);
    const double big = 30 + 4 * D;
    // threshold 4.5: leaf 0 (id 1) and leaf 2 (id 5) pass; leaf 1 (id 3, 3 pairs) climbs to id 2; leaf 3 (id 6, 2
    // pairs) climbs to id 4.  The silence mixtures 4 and 9 sit on leaf 4: ids 7 and 8, the later one serves the leaf.
    Result r = estimate(c, t, GMM_MLLR_FULL, {4, 9}, 4.5, 10.0);
    CHECK(r.rc == GMM_OK);
    CHECK(r.n == 6);
    const uint32_t wantIds[6] = {1, 2, 4, 5, 7, 8};
    for (uint32_t i = 0; i < 6 && i < r.n; ++i) {
        CHECK(r.ids[i] == wantIds[i]);
        CHECK(isMap(c, r, i));
    }
    const uint32_t wantMix[12] = {1, 2, 5, 4, 8, 1, 2, 5, 4, 8, 1, 2};
    for (uint32_t m = 0; m < 12; ++m)
        CHECK(r.ofMixture[m] == wantMix[m]);
    // a count equal to the threshold does not pass (strict): leaf 2 then climbs to id 4 too
    r = estimate(c, t, GMM_MLLR_FULL, {4}, big, 1e9);
    CHECK(r.rc == GMM_OK && r.n == 4);
    CHECK(r.ids[0] == 1 && r.ids[1] == 2 && r.ids[2] == 4 && r.ids[3] == 7);
    CHECK(r.ofMixture[2] == 4 && r.ofMixture[3] == 4 && r.ofMixture[1] == 2 && r.ofMixture[4] == 7);
    CHECK(isMap(c, r, 2) && isUnit(c, r, 3));  // silence below its threshold: the unit matrix
    // the root below the threshold: the unit matrix at the root's id serves every tree leaf
    r = estimate(c, t, GMM_MLLR_FULL, {4}, 1e9, 10.0);
    CHECK(r.rc == GMM_OK && r.n == 2 && r.ids[0] == 0 && r.ids[1] == 7);
    CHECK(isUnit(c, r, 0) && isMap(c, r, 1));
    for (uint32_t m = 0; m < 12; ++m)
        CHECK(r.ofMixture[m] == (c.leafOfMixture[m] == 4 ? 7u : 0u));
    // a rank deficient G: D - 1 distinct means span a subspace only; the map is still reproduced ON those means
    const Case  d = makeCase(D, {60, 60, 60, 60, 60}, D > 1 ? D - 1 : 1);
    r = estimate(d, t, GMM_MLLR_FULL, {4}, 1e9, 10.0);  // the silence leaf's own tables
    CHECK(r.rc == GMM_OK && r.n == 2);
    const size_t D1 = D + 1;
    bool         finite = true;
    for (size_t x = 0; x < D * D1; ++x)
        finite = finite && std::isfinite(r.matrices[D * D1 + x]);
    CHECK(finite);
    // W G = Z on the retained subspace
    double worst = 0.0, scale = 0.0;
    for (size_t i = 0; i < D; ++i)
        for (size_t j = 0; j < D1; ++j) {
            double s = 0.0;
            for (size_t k = 0; k < D1; ++k)
                s += r.matrices[D * D1 + i * D1 + k] * d.G[(4 * D1 + k) * D1 + j];
            worst = std::fmax(worst, std::fabs(s - d.Z[(4 * D + i) * D1 + j]));
            scale = std::fmax(scale, std::fabs(d.Z[(4 * D + i) * D1 + j]));
        }
    CHECK(worst <= 1e-9 * scale);
}

void testShift(uint32_t D) {
    const Tree   t;
    const Case   c = makeCase(D, {40, 3, 30, 2, 50}, 2 * D + 8);
    const Result r = estimate(c, t, GMM_MLLR_SHIFT, {4}, 4.5, 1e9);
    CHECK(r.rc == GMM_OK && r.n == 5);
    CHECK(r.ids[0] == 1 && r.ids[1] == 2 && r.ids[2] == 4 && r.ids[3] == 5 && r.ids[4] == 7);
    for (size_t d = 0; d < D; ++d) {
        CHECK(r.matrices[0 * D + d] == c.shift[0 * D + d] / c.beta[0 * D + d]);  // id 1 = leaf 0
        // id 4 = leaves 2 + 3, left first
        CHECK(r.matrices[2 * D + d] == (c.shift[2 * D + d] + c.shift[3 * D + d]) / (c.beta[2 * D + d] + c.beta[3 * D + d]));
        CHECK(r.matrices[4 * D + d] == 0.0);  // silence below its threshold: zeros
    }
}

void testAdapt() {
    const uint32_t D = 3;
    // 4 means, 3 densities, 2 mixtures; mean 3 is referenced by no entry
    std::vector<float>    means{1, 2, 3, -1, 0.5f, 4, 0.25f, -2, 8, 9, 9, 9}, variances{1, 1, 1};
    std::vector<uint32_t> dMean{0, 1, 2}, dCov{0, 0, 0}, off{0, 2, 3}, dens{0, 1, 2};
    std::vector<double>   logw{0, 0, 0};
    gmm_mixture_set       ms{};
    ms.dimension = D;
    ms.n_means = 4;
    ms.means = means.data();
    ms.n_covariances = 1;
    ms.variances = variances.data();
    ms.n_densities = 3;
    ms.density_mean = dMean.data();
    ms.density_covariance = dCov.data();
    ms.n_mixtures = 2;
    ms.mixture_offsets = off.data();
    ms.mixture_densities = dens.data();
    ms.mixture_log_weights = logw.data();
    std::vector<double> W(2 * D * (D + 1));
    for (size_t x = 0; x < W.size(); ++x)
        W[x] = 0.125 * static_cast<double>(x % 7) - 0.25;
    const uint32_t     ids[2] = {3, 9}, ofMix[2] = {9, 3};
    std::vector<float> out(12, -77.0f);
    CHECK(gmm_mllr_adapt_means(&ms, W.data(), ids, 2, ofMix, GMM_MLLR_FULL, out.data()) == GMM_OK);
    for (uint32_t mean = 0; mean < 3; ++mean) {
        const double* w = W.data() + (mean < 2 ? 1 : 0) * D * (D + 1);
        for (uint32_t i = 0; i < D; ++i) {
            double s = 0.0;
            s += w[i * 4 + 0] * 1.0;
            for (uint32_t j = 0; j < D; ++j)
                s += w[i * 4 + j + 1] * static_cast<double>(means[mean * D + j]);
            CHECK(out[mean * D + i] == static_cast<float>(s));
        }
    }
    CHECK(out[9] == 9.0f && out[10] == 9.0f && out[11] == 9.0f);  // copied
    CHECK(gmm_mllr_adapt_means(&ms, W.data(), ids, 2, ofMix, GMM_MLLR_SHIFT, out.data()) == GMM_OK);
    CHECK(out[0] == static_cast<float>(W[3] + 1.0) && out[8] == static_cast<float>(W[2] + 8.0) && out[9] == 9.0f);
    // an id that is not given; ids not ascending; a shared mean
    const uint32_t missing[2] = {9, 4};
    CHECK(gmm_mllr_adapt_means(&ms, W.data(), ids, 2, missing, GMM_MLLR_FULL, out.data()) == GMM_ERR_INVALID_ARGUMENT);
    CHECK(g_lastError.find("mixture 1") != std::string::npos);
    const uint32_t descending[2] = {9, 3};
    CHECK(gmm_mllr_adapt_means(&ms, W.data(), descending, 2, ofMix, GMM_MLLR_FULL, out.data()) == GMM_ERR_INVALID_ARGUMENT);
    dMean[2] = 1;
    CHECK(gmm_mllr_adapt_means(&ms, W.data(), ids, 2, ofMix, GMM_MLLR_FULL, out.data()) == GMM_ERR_UNSUPPORTED);
    CHECK(g_lastError.find("mean 1") != std::string::npos);
    CHECK(gmm_mllr_adapt_means(&ms, W.data(), ids, 2, ofMix, 3, out.data()) == GMM_ERR_INVALID_ARGUMENT);
    CHECK(gmm_mllr_adapt_means(nullptr, W.data(), ids, 2, ofMix, GMM_MLLR_FULL, out.data()) == GMM_ERR_INVALID_ARGUMENT);
}

void testRefusals() {
    const Case c = makeCase(3, {20, 20, 20, 20, 20}, 12);
    auto       refused = [&](const Tree& t, const char* word) {
        const Result r = estimate(c, t, GMM_MLLR_FULL, {4}, 1.0, 1.0);
        CHECK(r.rc == GMM_ERR_INVALID_ARGUMENT);
        CHECK(g_lastError.find(word) != std::string::npos);
    };
    Tree t;
    t.right[4] = 2;  // a cycle: id 2 again below id 4
    refused(t, "id 2 is reached twice");
    t = Tree();
    t.left[2] = 9;
    refused(t, "id 2 has a child out of range");
    t = Tree();
    t.leafNumber[5] = 5;
    refused(t, "leaf id 5");
    t = Tree();
    t.parent[0] = 4;
    refused(t, "root id 0 has a parent");
    t = Tree();
    t.right[4] = N;
    refused(t, "id 4 has one child");
    t = Tree();
    t.parent[6] = 2;
    refused(t, "parent of id 6");
    t = Tree();
    t.root = 7;
    refused(t, "root id 7");
    // a silence mixture out of range, silence mixtures not ascending, an uncovered leaf, a leaf index out of range
    t = Tree();
    CHECK(estimate(c, t, GMM_MLLR_FULL, {12}, 1.0, 1.0).rc == GMM_ERR_INVALID_ARGUMENT);
    CHECK(estimate(c, t, GMM_MLLR_FULL, {9, 4}, 1.0, 1.0).rc == GMM_ERR_INVALID_ARGUMENT);
    CHECK(estimate(c, t, GMM_MLLR_FULL, {}, 1.0, 1.0).rc == GMM_ERR_INVALID_ARGUMENT);
    CHECK(g_lastError.find("mixture 4") != std::string::npos);
    Case bad = c;
    bad.leafOfMixture[7] = 5;
    CHECK(estimate(bad, t, GMM_MLLR_FULL, {4}, 1.0, 1.0).rc == GMM_ERR_INVALID_ARGUMENT);
    CHECK(estimate(c, t, 0, {4}, 1.0, 1.0).rc == GMM_ERR_INVALID_ARGUMENT);
    uint32_t n = 0;
    CHECK(gmm_mllr_estimate(3, GMM_MLLR_FULL, 5, nullptr, c.G.data(), c.count.data(), nullptr, nullptr, c.leafOfMixture.data(),
                            12, 7, t.left.data(), t.right.data(), t.parent.data(), t.leafNumber.data(), 0, nullptr, 0, 1.0, 1.0,
                            &n, nullptr, nullptr, nullptr) == GMM_ERR_INVALID_ARGUMENT);
    // a single-leaf tree: the root is the leaf
    Tree one;
    one.left = {N};
    one.right = {N};
    one.parent = {N};
    one.leafNumber = {0};
    Case single = makeCase(3, {30, 0, 0, 0, 0}, 12);
    single.nLeaves = 1;
    single.leafOfMixture.assign(12, 0);
    Result r = estimate(single, one, GMM_MLLR_FULL, {}, 10.0, 1.0);
    CHECK(r.rc == GMM_OK && r.n == 1 && r.ids[0] == 0 && isMap(single, r, 0));
    r = estimate(single, one, GMM_MLLR_FULL, {}, 30.0, 1.0);
    CHECK(r.rc == GMM_OK && r.n == 1 && r.ids[0] == 0 && isUnit(single, r, 0));
}

}  // namespace

int main() {
    for (uint32_t D : {1u, 3u, 16u, 39u}) {
        testFull(D);
        testShift(D);
    }
    testAdapt();
    testRefusals();
    if (g_failures) {
        std::printf("mllr_estimate_test: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("mllr_estimate_test: ok\n");
    return 0;
}
