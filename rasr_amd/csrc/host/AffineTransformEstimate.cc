// AffineTransformEstimate.cc -- gmm_affine_estimate (include/rasr_gmm_adaptation.h): the affine feature transform of
// one key from its finalized tables, AffineFeatureTransformAccumulator::estimate
// (src/Mm/AffineFeatureTransformAccumulator.cc:177-311) for the criteria naive and mmiPrime with feature dimension =
// model dimension.  Plain C++: no HIP, no device, no LAPACK (the inverses are f64 Gauss-Jordan eliminations with
// partial pivoting), so the unit is also built and run alone (tests/cpp/affine_estimate_test.cc).
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/rasr_gmm_adaptation.h"

namespace rasr_gmm {
void setLastError(const std::string& msg);  // gmm_api.cc
}
using rasr_gmm::setLastError;

namespace {

int fail(int code, const std::string& msg) {
    setLastError(msg);
    return code;
}

// a [n][n] -> its inverse in place; false for a singular matrix: a pivot that is not finite or, after the elimination's
// own rounding, not above n * 2^-52 * max|a| (two equal rows leave residues of that size, not zeros)
bool invert(std::vector<double>& a, size_t n) {
    double scale = 0.0;
    for (const double x : a)
        scale = std::fmax(scale, std::fabs(x));
    const double tiny = static_cast<double>(n) * 2.220446049250313e-16 * scale;
    std::vector<double> inv(n * n, 0.0);
    for (size_t i = 0; i < n; ++i)
        inv[i * n + i] = 1.0;
    for (size_t c = 0; c < n; ++c) {
        size_t p = c;
        for (size_t r = c + 1; r < n; ++r)
            if (std::fabs(a[r * n + c]) > std::fabs(a[p * n + c]))
                p = r;
        const double pivot = a[p * n + c];
        if (!(std::fabs(pivot) > tiny) || !std::isfinite(pivot))
            return false;
        if (p != c)
            for (size_t j = 0; j < n; ++j) {
                std::swap(a[p * n + j], a[c * n + j]);
                std::swap(inv[p * n + j], inv[c * n + j]);
            }
        for (size_t j = 0; j < n; ++j) {
            a[c * n + j] /= pivot;
            inv[c * n + j] /= pivot;
        }
        for (size_t r = 0; r < n; ++r) {
            const double f = a[r * n + c];
            if (r == c || f == 0.0)
                continue;
            for (size_t j = 0; j < n; ++j) {
                a[r * n + j] -= f * a[c * n + j];
                inv[r * n + j] -= f * inv[c * n + j];
            }
        }
    }
    a.swap(inv);
    return true;
}

// y = m x, m [n][n]
void multiply(const double* m, const double* x, size_t n, double* y) {
    for (size_t j = 0; j < n; ++j) {
        double s = 0.0;
        for (size_t l = 0; l < n; ++l)
            s += m[j * n + l] * x[l];
        y[j] = s;
    }
}

}  // namespace

extern "C" int gmm_affine_estimate(uint32_t dimension, double beta, const double* k, const double* G, const double* mean,
                                   const double* cov, int criterion, uint32_t iterations, double minObservationWeight,
                                   const double* initialTransform, uint32_t initialColumns, float* outTransform) {
    (void)mean;
    (void)cov;  // the global covariance enters only the branch targetDimension < featureDimension_ (cc:252-263)
    const size_t D = dimension, D1 = D + 1;
    if (criterion == GMM_AFFINE_HLDA)
        return fail(GMM_ERR_UNSUPPORTED, "affine transform: the hlda criterion is not supported");
    if (criterion != GMM_AFFINE_NAIVE && criterion != GMM_AFFINE_MMI_PRIME)
        return fail(GMM_ERR_INVALID_ARGUMENT, "affine transform: unknown criterion " + std::to_string(criterion));
    if (D == 0 || !k || !G || !outTransform)
        return fail(GMM_ERR_INVALID_ARGUMENT, "affine transform: null argument or dimension 0");
    if (initialTransform && initialColumns != D && initialColumns != D1)
        return fail(GMM_ERR_INVALID_ARGUMENT, "affine transform: the initial transform has " + std::to_string(initialColumns) +
                                                      " columns, neither D nor D + 1");
    // the initial value: the identity (cc:169-172), or the caller's; [D][D] gains a zero offset column (cc:198-199)
    std::vector<double> W(D * D1, 0.0);
    for (size_t i = 0; i < D; ++i)
        for (size_t j = 0; j < D1; ++j) {
            if (!initialTransform)
                W[i * D1 + j] = j == i + 1 ? 1.0 : 0.0;
            else if (initialColumns == D1)
                W[i * D1 + j] = initialTransform[i * D1 + j];
            else
                W[i * D1 + j] = j == 0 ? 0.0 : initialTransform[i * D + (j - 1)];
        }
    auto finish = [&]() {
        for (size_t x = 0; x < D * D1; ++x)
            outTransform[x] = static_cast<float>(W[x]);
        return GMM_OK;
    };
    if (criterion != GMM_AFFINE_NAIVE && beta < minObservationWeight)  // cc:204
        return finish();

    std::vector<std::vector<double>> gInverse(D);
    for (size_t i = 0; i < D; ++i) {
        gInverse[i].assign(G + i * D1 * D1, G + (i + 1) * D1 * D1);
        if (!invert(gInverse[i], D1))
            return fail(GMM_ERR_INVALID_ARGUMENT, "affine transform: G of row " + std::to_string(i) + " is singular");
    }
    if (criterion == GMM_AFFINE_NAIVE) {  // cc:226-230
        for (size_t i = 0; i < D; ++i)
            multiply(gInverse[i].data(), k + i * D1, D1, &W[i * D1]);
        return finish();
    }

    std::vector<double> linear(D * D), cofactors(D1), rhs(D1);
    for (uint32_t it = 0; it < iterations; ++it)
        for (size_t row = 0; row < D; ++row) {
            // the extended cofactor row: scaling is arbitrary, so the column of the inverse of the linear part (cc:246-267)
            for (size_t i = 0; i < D; ++i)
                for (size_t j = 0; j < D; ++j)
                    linear[i * D + j] = W[i * D1 + j + 1];
            if (!invert(linear, D))
                return fail(GMM_ERR_INVALID_ARGUMENT, "affine transform: the linear part is singular at row " + std::to_string(row));
            cofactors[0] = 0.0;
            for (size_t j = 0; j < D; ++j)
                cofactors[j + 1] = linear[j * D + row];
            const double* gi = gInverse[row].data();
            const double* kr = k + row * D1;
            double        epsilon1 = 0.0, epsilon2 = 0.0;
            for (size_t j = 0; j < D1; ++j)
                for (size_t l = 0; l < D1; ++l) {
                    epsilon1 += cofactors[j] * gi[j * D1 + l] * cofactors[l];
                    epsilon2 += cofactors[j] * gi[j * D1 + l] * kr[l];
                }
            const double root   = std::sqrt(epsilon2 * epsilon2 + 4 * epsilon1 * beta);
            const double alpha1 = (-epsilon2 + root) / (2 * epsilon1);
            const double alpha2 = (-epsilon2 - root) / (2 * epsilon1);
            // The reference writes "- 1 / 2 * alpha * alpha * epsilon1" (cc:283-284): 1 / 2 is an integer division, 0, so
            // the quadratic term is not there and the root is chosen by beta * log|alpha * epsilon1 + epsilon2| alone.
            // Kept as the reference computes it.
            const double l1    = beta * std::log(std::fabs(alpha1 * epsilon1 + epsilon2));
            const double l2    = beta * std::log(std::fabs(alpha2 * epsilon1 + epsilon2));
            const double alpha = l1 > l2 ? alpha1 : alpha2;
            for (size_t j = 0; j < D1; ++j)
                rhs[j] = cofactors[j] * alpha + kr[j];
            multiply(gi, rhs.data(), D1, &W[row * D1]);  // cc:288-289
        }
    return finish();
}
