// MllrEstimate.cc -- gmm_mllr_estimate and gmm_mllr_adapt_means (include/rasr_gmm_mllr.h): the MLLR matrices of one
// key from its leaf tables over a binary regression tree (AdaptorEstimator::propagate, estimateWMatrices and adaptor()
// of the full and the shift estimator, src/Mm/MllrAdaptation.hh:223-242, .cc:358-379, 444-531, 671-827), and the
// adapted means (adaptMixtureSet, cc:59-79, 146-170).  Plain C++: no HIP, no device, no LAPACK (the pseudo-inverse is
// a one-sided Jacobi SVD in f64), so the unit is also built and run alone (tests/cpp/mllr_estimate_test.cc).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/rasr_gmm_mllr.h"

namespace rasr_gmm {
void setLastError(const std::string& msg);  // gmm_api.cc
}
using rasr_gmm::setLastError;

namespace {

constexpr uint32_t kNone         = GMM_MLLR_NO_ID;
constexpr double   kSvdThreshold = 1e-12;  // Math/Lapack/Svd.hh:27

int fail(int code, const std::string& msg) {
    setLastError(msg);
    return code;
}

// g [n][n] -> its pseudo-inverse in place.  One-sided (Hestenes) Jacobi: the columns of u = g are rotated in pairs
// until they are mutually orthogonal, v collects the rotations, so g = (u / sigma) diag(sigma) v^T with sigma the
// column norms of u, and pinv(g) = sum over the retained j of v[:, j] u[:, j]^T / sigma_j^2.
void pseudoInvert(std::vector<double>& g, size_t n) {
    std::vector<double> u(g), v(n * n, 0.0);
    for (size_t i = 0; i < n; ++i)
        v[i * n + i] = 1.0;
    // the rounding of an n-term dot product: below it a pair of columns is orthogonal as far as f64 can tell
    const double tol = static_cast<double>(n) * 2.220446049250313e-16;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (size_t p = 0; p + 1 < n; ++p)
            for (size_t q = p + 1; q < n; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (size_t k = 0; k < n; ++k) {
                    alpha += u[k * n + p] * u[k * n + p];
                    beta += u[k * n + q] * u[k * n + q];
                    gamma += u[k * n + p] * u[k * n + q];
                }
                const double scale = std::sqrt(alpha * beta);
                if (!(scale > 0.0) || !(std::fabs(gamma) > tol * scale))
                    continue;
                rotated           = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t    = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c    = 1.0 / std::sqrt(1.0 + t * t);
                const double s    = c * t;
                for (size_t k = 0; k < n; ++k) {
                    const double up = u[k * n + p], uq = u[k * n + q];
                    u[k * n + p]    = c * up - s * uq;
                    u[k * n + q]    = s * up + c * uq;
                    const double vp = v[k * n + p], vq = v[k * n + q];
                    v[k * n + p]    = c * vp - s * vq;
                    v[k * n + q]    = s * vp + c * vq;
                }
            }
        if (!rotated)
            break;
    }
    std::vector<double> sigma2(n, 0.0);
    double              largest = 0.0;
    for (size_t j = 0; j < n; ++j) {
        for (size_t k = 0; k < n; ++k)
            sigma2[j] += u[k * n + j] * u[k * n + j];
        largest = std::fmax(largest, std::sqrt(sigma2[j]));
    }
    std::fill(g.begin(), g.end(), 0.0);
    for (size_t j = 0; j < n; ++j) {
        if (!(std::sqrt(sigma2[j]) > kSvdThreshold * largest))
            continue;
        for (size_t a = 0; a < n; ++a) {
            const double f = v[a * n + j] / sigma2[j];
            for (size_t b = 0; b < n; ++b)
                g[a * n + b] += f * u[b * n + j];
        }
    }
}

// w [D][D+1] = z [D][D+1] * pinv(g [D+1][D+1])  (cc:683-685)
void estimateFull(const double* z, const double* g, size_t D, double* w) {
    const size_t        D1 = D + 1;
    std::vector<double> gInverse(g, g + D1 * D1);
    pseudoInvert(gInverse, D1);
    for (size_t i = 0; i < D; ++i)
        for (size_t j = 0; j < D1; ++j) {
            double s = 0.0;
            for (size_t k = 0; k < D1; ++k)
                s += z[i * D1 + k] * gInverse[k * D1 + j];
            w[i * D1 + j] = s;
        }
}

// adaptationUnitMatrix: zero offset column, identity; the shift kind's zero row
void unitMatrix(int kind, size_t D, double* w) {
    const size_t cells = kind == GMM_MLLR_FULL ? D * (D + 1) : D;
    std::fill(w, w + cells, 0.0);
    if (kind == GMM_MLLR_FULL)
        for (size_t i = 0; i < D; ++i)
            w[i * (D + 1) + i + 1] = 1.0;
}

}  // namespace

extern "C" int gmm_mllr_estimate(uint32_t dimension, int kind, uint32_t nLeaves, const double* Z, const double* G,
                                 const double* count, const double* beta, const double* shift,
                                 const uint32_t* leafOfMixture, uint32_t nMixtures, uint32_t nTreeIds, const uint32_t* left,
                                 const uint32_t* right, const uint32_t* parent, const uint32_t* leafNumber, uint32_t root,
                                 const uint32_t* silenceMixtures, uint32_t nSilence, double minObservation,
                                 double minSilenceObservation, uint32_t* nMatrices, uint32_t* ids, double* matrices,
                                 uint32_t* matrixOfMixture) {
    const size_t D = dimension, D1 = D + 1;
    if (kind != GMM_MLLR_FULL && kind != GMM_MLLR_SHIFT)
        return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: kind " + std::to_string(kind) + " is neither full nor shift");
    const bool full = kind == GMM_MLLR_FULL;
    if (D == 0 || nLeaves == 0 || nTreeIds == 0 || !count || !left || !right || !parent || !leafNumber || !nMatrices ||
        !ids || !matrices || (nMixtures && (!leafOfMixture || !matrixOfMixture)) || (nSilence && !silenceMixtures) ||
        (full ? !Z || !G : !beta || !shift))
        return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: null argument, or a dimension, leaf or id count of 0");
    *nMatrices = 0;
    for (uint32_t m = 0; m < nMixtures; ++m)
        if (leafOfMixture[m] >= nLeaves)
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: mixture " + std::to_string(m) + " maps to leaf " +
                                                          std::to_string(leafOfMixture[m]) + " of " + std::to_string(nLeaves));
    for (uint32_t s = 0; s < nSilence; ++s) {
        if (silenceMixtures[s] >= nMixtures)
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: silence mixture " + std::to_string(silenceMixtures[s]) + " out of range");
        if (s && silenceMixtures[s] <= silenceMixtures[s - 1])
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: the silence mixtures are not ascending at " +
                                                          std::to_string(silenceMixtures[s]));
    }
    if (static_cast<uint64_t>(nTreeIds) + nSilence > 0xfffffffeull)
        return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: too many ids");

    // the tree: a walk from the root that checks what the reference's recursion takes for granted, and leaves the
    // reachable ids in post-order (children before their parent: propagate's order)
    if (root >= nTreeIds)
        return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: root id " + std::to_string(root) + " out of range");
    if (parent[root] != kNone)
        return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: root id " + std::to_string(root) + " has a parent");
    std::vector<uint8_t>  seen(nTreeIds, 0);
    std::vector<uint32_t> order, stack{root};
    order.reserve(nTreeIds);
    seen[root] = 1;
    while (!stack.empty()) {
        const uint32_t id = stack.back();
        stack.pop_back();
        order.push_back(id);
        const uint32_t l = left[id], r = right[id];
        if (l == kNone && r == kNone) {
            if (leafNumber[id] >= nLeaves)
                return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: leaf id " + std::to_string(id) + " has leaf number " +
                                                              std::to_string(leafNumber[id]) + " of " + std::to_string(nLeaves));
            continue;
        }
        if (l == kNone || r == kNone)
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: id " + std::to_string(id) + " has one child only");
        for (const uint32_t child : {l, r}) {
            if (child >= nTreeIds)
                return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: id " + std::to_string(id) + " has a child out of range");
            if (seen[child])
                return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: id " + std::to_string(child) + " is reached twice (a cycle)");
            if (parent[child] != id)
                return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: the parent of id " + std::to_string(child) + " is not id " +
                                                              std::to_string(id));
            seen[child] = 1;
        }
        stack.push_back(l);
        stack.push_back(r);
    }
    // order: a node before everything below it; reversed: right subtree, left subtree ... every child before its
    // parent, which is all the elementwise node = left + right needs
    std::reverse(order.begin(), order.end());

    // propagate (hh:223-242): nodeData[leaf id] = leafData[leaf number]; nodeData[id] = left; += right
    const size_t        cells = full ? D * D1 + D1 * D1 : 2 * D;  // Z | G, or beta | shift
    std::vector<double> node(static_cast<size_t>(nTreeIds) * cells, 0.0), nodeCount(nTreeIds, 0.0);
    auto leafCells = [&](uint32_t leaf, double* dst) {
        if (full) {
            std::copy(Z + leaf * D * D1, Z + (leaf + 1) * D * D1, dst);
            std::copy(G + leaf * D1 * D1, G + (leaf + 1) * D1 * D1, dst + D * D1);
        } else {
            std::copy(beta + leaf * D, beta + (leaf + 1) * D, dst);
            std::copy(shift + leaf * D, shift + (leaf + 1) * D, dst + D);
        }
    };
    for (const uint32_t id : order) {
        double* dst = &node[id * cells];
        if (left[id] == kNone) {
            leafCells(leafNumber[id], dst);
            nodeCount[id] = count[leafNumber[id]];
            continue;
        }
        const double *a = &node[left[id] * cells], *b = &node[right[id] * cells];
        for (size_t x = 0; x < cells; ++x)
            dst[x] = a[x] + b[x];
        nodeCount[id] = nodeCount[left[id]] + nodeCount[right[id]];
    }

    // adaptor(): the id of every leaf
    std::vector<uint32_t> matrixId(nLeaves, kNone);
    std::vector<uint32_t> used;  // tree ids whose matrix is needed
    if (!(nodeCount[root] > minObservation)) {
        used.push_back(root);
        for (uint32_t id = 0; id < nTreeIds; ++id)
            if (seen[id] && left[id] == kNone)
                matrixId[leafNumber[id]] = root;
    } else {
        for (uint32_t leafId = 0; leafId < nTreeIds; ++leafId) {
            if (!seen[leafId] || left[leafId] != kNone)
                continue;
            uint32_t id = leafId;
            while (id != root && !(nodeCount[id] > minObservation))
                id = parent[id];
            used.push_back(id);
            matrixId[leafNumber[leafId]] = id;
        }
        std::sort(used.begin(), used.end());
        used.erase(std::unique(used.begin(), used.end()), used.end());
    }
    const size_t matrixCells = full ? D * D1 : D;
    uint32_t     n = 0;
    auto estimateFrom = [&](const double* tables, double* w) {  // tables: Z | G, or beta | shift
        if (full) {
            estimateFull(tables, tables + D * D1, D, w);
        } else {
            for (size_t d = 0; d < D; ++d)
                w[d] = tables[D + d] / tables[d];  // shift[d] / beta[d], cc:373
        }
    };
    for (const uint32_t id : used) {
        ids[n] = id;
        if (nodeCount[id] > minObservation)
            estimateFrom(&node[id * cells], matrices + n * matrixCells);
        else
            unitMatrix(kind, D, matrices + n * matrixCells);
        ++n;
    }
    // the silence mixtures: ids past the tree's, each from its own leaf's tables alone (cc:488-509, 785-805)
    std::vector<double> own(cells);
    for (uint32_t s = 0; s < nSilence; ++s) {
        const uint32_t leaf = leafOfMixture[silenceMixtures[s]];
        ids[n]              = nTreeIds + s;
        if (count[leaf] > minSilenceObservation) {
            leafCells(leaf, own.data());
            estimateFrom(own.data(), matrices + n * matrixCells);
        } else {
            unitMatrix(kind, D, matrices + n * matrixCells);
        }
        matrixId[leaf] = nTreeIds + s;
        ++n;
    }
    for (uint32_t m = 0; m < nMixtures; ++m) {
        if (matrixId[leafOfMixture[m]] == kNone)
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr estimate: mixture " + std::to_string(m) + " maps to leaf " +
                                                          std::to_string(leafOfMixture[m]) +
                                                          ", which neither the tree nor a silence mixture covers");
        matrixOfMixture[m] = matrixId[leafOfMixture[m]];
    }
    *nMatrices = n;
    return GMM_OK;
}

extern "C" int gmm_mllr_adapt_means(const gmm_mixture_set* ms, const double* matrices, const uint32_t* ids,
                                    uint32_t nMatrices, const uint32_t* matrixOfMixture, int kind, float* outMeans) {
    if (kind != GMM_MLLR_FULL && kind != GMM_MLLR_SHIFT)
        return fail(GMM_ERR_INVALID_ARGUMENT, "mllr adapt: kind " + std::to_string(kind) + " is neither full nor shift");
    if (!ms || !matrices || !ids || !outMeans || !ms->means || !ms->mixture_offsets || (ms->n_mixtures && !matrixOfMixture) ||
        (ms->n_densities && !ms->density_mean) || ms->dimension == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "mllr adapt: null argument or dimension 0");
    const size_t   D = ms->dimension, D1 = D + 1;
    const uint32_t nEntries = ms->mixture_offsets[ms->n_mixtures];
    if (nEntries && !ms->mixture_densities)
        return fail(GMM_ERR_INVALID_ARGUMENT, "mllr adapt: null argument");
    for (uint32_t i = 1; i < nMatrices; ++i)
        if (ids[i] <= ids[i - 1])
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr adapt: the matrix ids are not ascending at " + std::to_string(ids[i]));
    const bool   full        = kind == GMM_MLLR_FULL;
    const size_t matrixCells = full ? D * D1 : D;
    std::copy(ms->means, ms->means + static_cast<size_t>(ms->n_means) * D, outMeans);  // unreferenced means: copied
    std::vector<uint8_t> done(ms->n_means, 0);
    std::vector<double>  m(D1);
    for (uint32_t mix = 0; mix < ms->n_mixtures; ++mix) {
        const uint32_t e0 = ms->mixture_offsets[mix], e1 = ms->mixture_offsets[mix + 1];
        if (e1 < e0 || e1 > nEntries)
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr adapt: mixture_offsets decrease at mixture " + std::to_string(mix));
        if (e0 == e1)
            continue;
        const uint32_t* at = std::lower_bound(ids, ids + nMatrices, matrixOfMixture[mix]);
        if (at == ids + nMatrices || *at != matrixOfMixture[mix])
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr adapt: mixture " + std::to_string(mix) + " names matrix id " +
                                                          std::to_string(matrixOfMixture[mix]) + ", which is not given");
        const double* w = matrices + static_cast<size_t>(at - ids) * matrixCells;
        for (uint32_t e = e0; e < e1; ++e) {
            const uint32_t d = ms->mixture_densities[e];
            if (d >= ms->n_densities || ms->density_mean[d] >= ms->n_means)
                return fail(GMM_ERR_INVALID_ARGUMENT, "mllr adapt: mixture entry " + std::to_string(e) +
                                                              " refers to a density or mean out of range");
            const uint32_t mean = ms->density_mean[d];
            if (done[mean])
                return fail(GMM_ERR_UNSUPPORTED, "mllr adapt: mean " + std::to_string(mean) +
                                                         " is referenced by more than one mixture entry");
            done[mean]      = 1;
            const float* mu = ms->means + mean * D;
            float*       o  = outMeans + mean * D;
            if (!full) {
                for (size_t i = 0; i < D; ++i)
                    o[i] = static_cast<float>(w[i] + static_cast<double>(mu[i]));
                continue;
            }
            m[0] = 1.0;
            for (size_t j = 0; j < D; ++j)
                m[j + 1] = static_cast<double>(mu[j]);
            for (size_t i = 0; i < D; ++i) {
                double s = 0.0;
                for (size_t j = 0; j < D1; ++j)
                    s += w[i * D1 + j] * m[j];
                o[i] = static_cast<float>(s);
            }
        }
    }
    return GMM_OK;
}
