// gmm_adapt.cc -- the handle behind include/rasr_gmm_adaptation.h: the keys' f64 accumulators on the device (their
// layout, pooled mode), create's own argument rules, pass 4 of a call (gmm_kernels_adapt.hip), get / add / info.
// Everything a handle that accumulates keyed pairs shares with the others is gmm_pairaccum.hh's.
// The estimation of a transform from the tables is host/AffineTransformEstimate.cc (no HIP).
#include <algorithm>
#include <memory>
#include <new>

#include "gmm_adapt.hh"

using namespace rasr_gmm;

struct gmm_affine_accumulator {
    PairAccumCore core;
    KeyedPairs    keyed;
    bool          pooled = false;
    size_t        smallCells = 0, gCells = 0;  // per key; gCells == 0 in pooled mode
    std::vector<float> pooledVariance;         // [D]: globalModelVariance_ (pooled mode)
    // the accumulators, and the later pieces' slabs of one call
    DeviceBuffer<double> dSmall, dG, dSlabSmall, dSlabG;
};

namespace {

constexpr PairNouns kNouns{"affine accumulator", "mixture set", "affine accumulator"};

int zeroTables(gmm_affine_accumulator* h) {
    GMM_HIP_CHECK(hipMemset(h->dSmall.get(), 0, h->keyed.nKeys * h->smallCells * sizeof(double)));
    if (h->gCells)
        GMM_HIP_CHECK(hipMemset(h->dG.get(), 0, h->keyed.nKeys * h->gCells * sizeof(double)));
    GMM_HIP_CHECK(hipMemset(h->core.dSkipped.get(), 0, sizeof(unsigned long long)));
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // done before a call on any other stream
    return GMM_OK;
}

int create(gmm_affine_accumulator* h, const gmm_mixture_set& ms, uint32_t nKeys, uint32_t maxPairs, int device) {
    PairTopology topo;
    int          rc = initCore(h->core, kNouns, ms, maxPairs, device, topo);
    if (rc != GMM_OK)
        return rc;
    const uint32_t D = ms.dimension;
    // mixture->nCovariances() == 1 (cc:54): global variance optimisation, no G accumulated
    h->pooled = ms.n_covariances == 1;
    if (h->pooled)
        h->pooledVariance.assign(ms.variances, ms.variances + D);
    h->smallCells = affineSmallCells(D);
    h->gCells     = h->pooled ? 0 : static_cast<size_t>(D) * affineTriangle(D);

    GMM_HIP_CHECK(hipSetDevice(device));
    if ((rc = keyedSizes(h->core, h->keyed, kNouns, nKeys, 1, false, (h->smallCells + h->gCells) * sizeof(double), maxPairs)) ||
        (rc = allocCore(h->core, topo, true)) || (rc = allocKeyed(h->core, h->keyed, ms, nullptr)))
        return rc;
    const size_t slots = pieceSlabSlots(maxPairs);
    GMM_HIP_CHECK(h->dSmall.alloc(nKeys * h->smallCells));
    GMM_HIP_CHECK(h->dG.alloc(nKeys * h->gCells));
    GMM_HIP_CHECK(h->dSlabSmall.alloc(slots * h->smallCells));
    GMM_HIP_CHECK(h->dSlabG.alloc(slots * h->gCells));
    return zeroTables(h);
}

int accumulateOn(gmm_affine_accumulator* h, gmm_scorer* scorer, const PairCall& call, hipStream_t stream) {
    PairAccumCore& c = h->core;
    KeyedPairs&    k = h->keyed;
    uint32_t       pieces = 0;
    const int      rc = indexKeyedPairs(c, k, scorer, call, stream, &pieces);
    if (rc != GMM_OK)
        return rc;
    AffineArgs a{};
    a.keysSorted  = c.dKeysSorted.get();
    a.frames      = call.frames;
    a.means       = k.dMeans.get();
    a.variances   = k.dVariances.get();
    a.sFrame      = k.dSFrame.get();
    a.sMean       = k.dSMean.get();
    a.sCov        = k.dSCov.get();
    a.sWeight     = k.dSWeight.get();
    a.pieces      = k.dPieces.get();
    a.nPieces     = k.dNPieces.get();
    a.small       = h->dSmall.get();
    a.G           = h->gCells ? h->dG.get() : nullptr;
    a.slabSmall   = h->dSlabSmall.get();
    a.slabG       = h->gCells ? h->dSlabG.get() : nullptr;
    a.nPairs      = call.nPairs;
    a.nKeys       = h->keyed.nKeys;
    a.D           = h->core.D;
    a.frameStride = call.frameStride;
    a.maxPieces   = pieces;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchAffineAccumulate(a, stream)));
    GMM_HIP_CHECK(static_cast<hipError_t>(launchCombinePieces(a.keysSorted, a.pieces, a.nPieces, pieces, call.nPairs, a.small,
                                                             a.slabSmall, h->smallCells, stream)));
    if (a.G)
        GMM_HIP_CHECK(static_cast<hipError_t>(launchCombinePieces(a.keysSorted, a.pieces, a.nPieces, pieces, call.nPairs, a.G,
                                                                 a.slabG, h->gCells, stream)));
    return GMM_OK;
}

// one key's raw tables on the host: small [smallCells], g [gCells] (empty in pooled mode)
int fetchKey(gmm_affine_accumulator* h, uint32_t key, std::vector<double>& small, std::vector<double>* g) {
    small.resize(h->smallCells);
    GMM_HIP_CHECK(hipMemcpy(small.data(), h->dSmall.get() + static_cast<size_t>(key) * h->smallCells,
                            h->smallCells * sizeof(double), hipMemcpyDeviceToHost));
    if (g) {
        g->resize(h->gCells);
        if (h->gCells)
            GMM_HIP_CHECK(hipMemcpy(g->data(), h->dG.get() + static_cast<size_t>(key) * h->gCells, h->gCells * sizeof(double),
                                    hipMemcpyDeviceToHost));
    }
    return GMM_OK;
}

int checkKey(gmm_affine_accumulator* h, uint32_t key) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null affine accumulator");
    if (key >= h->keyed.nKeys)
        return fail(GMM_ERR_INVALID_ARGUMENT, "key " + std::to_string(key) + " out of range: the affine accumulator holds " +
                                                      std::to_string(h->keyed.nKeys) + " keys");
    GMM_HIP_CHECK(hipSetDevice(h->core.device));
    return waitDone(h->core);
}

}  // namespace

extern "C" {

int gmm_affine_create(const gmm_mixture_set* ms, uint32_t nKeys, uint32_t maxPairs, int device, gmm_affine_accumulator** out) {
    if (!ms || !out || !ms->mixture_offsets || !ms->means || !ms->variances ||
        (ms->n_densities && (!ms->density_mean || !ms->density_covariance)))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (ms->mixture_offsets[ms->n_mixtures] && !ms->mixture_densities)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    if (nKeys == 0 || ms->dimension == 0 || ms->n_covariances == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "affine accumulator: n_keys, the dimension and the covariance count must not be 0");
    if (ms->dimension > GMM_AFFINE_MAX_DIMENSION)
        return fail(GMM_ERR_UNSUPPORTED, "affine accumulator: dimension " + std::to_string(ms->dimension) + " exceeds " +
                                                 std::to_string(GMM_AFFINE_MAX_DIMENSION));
    std::unique_ptr<gmm_affine_accumulator> h(new (std::nothrow) gmm_affine_accumulator);
    if (!h)
        return fail(GMM_ERR_OUT_OF_MEMORY, "out of host memory");
    const int rc = create(h.get(), *ms, nKeys, maxPairs, device);
    if (rc != GMM_OK)
        return rc;
    *out = h.release();
    return GMM_OK;
}

int gmm_affine_destroy(gmm_affine_accumulator* h) {
    if (!h)
        return GMM_OK;
    destroyWait(h->core);
    delete h;
    return GMM_OK;
}

int gmm_affine_reset(gmm_affine_accumulator* h) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null affine accumulator");
    GMM_HIP_CHECK(hipSetDevice(h->core.device));
    const int rc = waitDone(h->core);
    return rc != GMM_OK ? rc : zeroTables(h);
}

int gmm_affine_accumulate_device(gmm_affine_accumulator* h, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                 uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                 const uint32_t* pairDensity, const double* pairWeight, const uint32_t* pairKey,
                                 uint32_t nPairs, void* stream) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, pairDensity, pairKey, pairWeight, nullptr, nPairs};
    const int      rc = checkPairCall(h ? &h->core : nullptr, kNouns, scorer, call);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    return deviceCall(h->core, nPairs, stream, nothingToPrepare,
                      [&](hipStream_t st) { return accumulateOn(h, scorer, call, st); });
}

int gmm_affine_accumulate_host(gmm_affine_accumulator* h, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                               uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                               const uint32_t* pairDensity, const double* pairWeight, const uint32_t* pairKey, uint32_t nPairs) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, pairDensity, pairKey, pairWeight, nullptr, nPairs};
    const int      rc = checkPairCall(h ? &h->core : nullptr, kNouns, scorer, call);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    return hostCall(h->core, call, nothingToPrepare,
                    [&](const PairCall& staged) { return accumulateOn(h, scorer, staged, nullptr); });
}

int gmm_affine_skipped(gmm_affine_accumulator* h, uint64_t* skipped) {
    if (!h || !skipped)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    return readSkipped(h->core, skipped);
}

int gmm_affine_info(const gmm_affine_accumulator* h, uint64_t* tableBytes, uint64_t* scratchBytes, int* pooled) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null affine accumulator");
    if (tableBytes)
        *tableBytes = h->keyed.tableBytes;
    if (scratchBytes)
        *scratchBytes = h->keyed.scratchBytes;
    if (pooled)
        *pooled = h->pooled ? 1 : 0;
    return GMM_OK;
}

int gmm_affine_get(gmm_affine_accumulator* h, uint32_t key, double* beta, double* k, double* G, double* mean, double* cov) {
    int rc = checkKey(h, key);
    if (rc != GMM_OK)
        return rc;
    std::vector<double> small, g;
    if ((rc = fetchKey(h, key, small, G ? &g : nullptr)) != GMM_OK)
        return rc;
    const size_t  D = h->core.D, D1 = D + 1, T = affineTriangle(h->core.D);
    const double* tri = small.data() + 1 + D1;  // cov's upper triangle
    if (beta)
        *beta = small[0];
    if (mean)
        std::copy(small.begin() + 1, small.begin() + 1 + D1, mean);
    if (k)
        std::copy(small.begin() + 1 + D1 + T, small.end(), k);
    // finalize (cc:135-142): the lower triangles mirror the upper ones
    if (cov)
        for (size_t j = 0, c = 0; j < D1; ++j)
            for (size_t l = j; l < D1; ++l, ++c)
                cov[j * D1 + l] = cov[l * D1 + j] = tri[c];
    if (G)
        for (size_t i = 0; i < D; ++i) {
            double*      Gi = G + i * D1 * D1;
            const double v  = h->pooled ? static_cast<double>(h->pooledVariance[i]) : 0.0;
            for (size_t j = 0, c = 0; j < D1; ++j)
                for (size_t l = j; l < D1; ++l, ++c)  // pooled: cov[j][k] / Sum(globalModelVariance_[i]), cc:129
                    Gi[j * D1 + l] = Gi[l * D1 + j] = h->pooled ? tri[c] / v : g[i * T + c];
        }
    return GMM_OK;
}

int gmm_affine_add(gmm_affine_accumulator* h, uint32_t key, const double* beta, const double* k, const double* G,
                   const double* mean, const double* cov, double weight) {
    int rc = checkKey(h, key);
    if (rc != GMM_OK)
        return rc;
    const bool          addG = G && !h->pooled;  // cc:359
    std::vector<double> small, g;
    if ((rc = fetchKey(h, key, small, addG ? &g : nullptr)) != GMM_OK)
        return rc;
    const size_t D = h->core.D, D1 = D + 1, T = affineTriangle(h->core.D);
    // dst = dst + src * weight: one multiply, one add (the unit is built with -ffp-contract=off)
    auto add = [weight](double& dst, double src) {
        const double scaled = src * weight;
        dst                 = dst + scaled;
    };
    if (beta)
        add(small[0], *beta);
    if (mean)
        for (size_t j = 0; j < D1; ++j)
            add(small[1 + j], mean[j]);
    if (cov)
        for (size_t j = 0, c = 0; j < D1; ++j)
            for (size_t l = j; l < D1; ++l, ++c)
                add(small[1 + D1 + c], cov[j * D1 + l]);
    if (k)
        for (size_t x = 0; x < D * D1; ++x)
            add(small[1 + D1 + T + x], k[x]);
    GMM_HIP_CHECK(hipMemcpy(h->dSmall.get() + static_cast<size_t>(key) * h->smallCells, small.data(),
                            h->smallCells * sizeof(double), hipMemcpyHostToDevice));
    if (addG) {
        for (size_t i = 0; i < D; ++i)
            for (size_t j = 0, c = 0; j < D1; ++j)
                for (size_t l = j; l < D1; ++l, ++c)
                    add(g[i * T + c], G[i * D1 * D1 + j * D1 + l]);
        GMM_HIP_CHECK(hipMemcpy(h->dG.get() + static_cast<size_t>(key) * h->gCells, g.data(), h->gCells * sizeof(double),
                                hipMemcpyHostToDevice));
    }
    return GMM_OK;
}

}  // extern "C"
