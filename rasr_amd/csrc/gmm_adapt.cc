// gmm_adapt.cc -- the handle behind include/rasr_gmm_adaptation.h: the model's tables and the keys' f64 accumulators on
// the device, the argument checks, the launch sequence of a call (gmm_kernels_adapt.hip), get / add.
// The estimation of a transform from the tables is host/AffineTransformEstimate.cc (no HIP).
#include <algorithm>
#include <cstdio>
#include <memory>
#include <new>

#include "gmm_adapt.hh"
#include "gmm_estimator.hh"
#include "gmm_scorer.hh"

using namespace rasr_gmm;

struct gmm_affine_accumulator {
    int      device = 0;
    uint32_t D = 0, nKeys = 0, maxPairs = 0, maxPieces = 0, nMix = 0, nEntries = 0, nMeans = 0, nCovs = 0;
    bool     pooled = false, oneDensityPerMixture = false;
    size_t   smallCells = 0, gCells = 0;  // per key; gCells == 0 in pooled mode
    uint64_t tableBytes = 0, scratchBytes = 0;
    std::vector<float> pooledVariance;  // [D]: globalModelVariance_ (pooled mode)
    // the model (device)
    DeviceBuffer<uint32_t> dMixOff, dEntryMean, dEntryCov;
    DeviceBuffer<float>    dMeans, dVariances;
    // the accumulators
    DeviceBuffer<double>             dSmall, dG;
    DeviceBuffer<unsigned long long> dSkipped;
    // scratch of one call of up to maxPairs pairs
    DeviceBuffer<uint32_t> dBest, dKey, dMean, dCov, dPairIndex, dKeysSorted, dIndexSorted, dSFrame, dSMean, dSCov, dPieces,
            dNPieces;
    DeviceBuffer<double> dSWeight, dSlabSmall, dSlabG;
    DeviceBuffer<void>   dSortTemp;
    size_t               sortTempBytes = 0;
    // the host call's pair lists
    DeviceBuffer<uint32_t> dPairFrame, dPairMix, dPairDensity, dPairKey;
    DeviceBuffer<double>   dPairWeight;
    // recorded by every accumulate call on its stream; get / skipped / add / reset wait for it
    Event done;
    bool  pending = false;
};

namespace {

// bits of the keys 0 .. nKeys (nKeys: the skipped pairs' sentinel)
uint32_t keyBits(uint32_t nKeys) {
    uint32_t b = 1;
    while (b < 32 && (nKeys >> b))
        ++b;
    return b;
}

int zeroTables(gmm_affine_accumulator* h) {
    GMM_HIP_CHECK(hipMemset(h->dSmall.get(), 0, h->nKeys * h->smallCells * sizeof(double)));
    if (h->gCells)
        GMM_HIP_CHECK(hipMemset(h->dG.get(), 0, h->nKeys * h->gCells * sizeof(double)));
    GMM_HIP_CHECK(hipMemset(h->dSkipped.get(), 0, sizeof(unsigned long long)));
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // done before a call on any other stream
    return GMM_OK;
}

int waitDone(gmm_affine_accumulator* h) {
    if (h->pending) {
        GMM_HIP_CHECK(hipEventSynchronize(h->done.get()));
        h->pending = false;
    }
    return GMM_OK;
}

int create(gmm_affine_accumulator* h, const gmm_mixture_set& ms, uint32_t nKeys, uint32_t maxPairs, int device) {
    h->device   = device;
    h->D        = ms.dimension;
    h->nKeys    = nKeys;
    h->maxPairs = maxPairs;
    h->nMix     = ms.n_mixtures;
    h->nMeans   = ms.n_means;
    h->nCovs    = ms.n_covariances;
    const uint32_t D = h->D;
    std::vector<uint32_t> mixOff(ms.mixture_offsets, ms.mixture_offsets + ms.n_mixtures + 1);
    if (mixOff[0] != 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "affine accumulator: mixture_offsets[0] is not 0");
    for (uint32_t m = 0; m < h->nMix; ++m)
        if (mixOff[m + 1] < mixOff[m])
            return fail(GMM_ERR_INVALID_ARGUMENT, "affine accumulator: mixture_offsets decrease at mixture " + std::to_string(m));
    h->nEntries = mixOff[h->nMix];
    for (uint32_t d = 0; d < ms.n_densities; ++d)
        if (ms.density_mean[d] >= h->nMeans || ms.density_covariance[d] >= h->nCovs)
            return fail(GMM_ERR_INVALID_ARGUMENT, "affine accumulator: density " + std::to_string(d) +
                                                          " refers to a mean or covariance out of range");
    std::vector<uint32_t> entryMean(h->nEntries), entryCov(h->nEntries);
    for (uint32_t i = 0; i < h->nEntries; ++i) {
        const uint32_t d = ms.mixture_densities[i];
        if (d >= ms.n_densities)
            return fail(GMM_ERR_INVALID_ARGUMENT, "affine accumulator: mixture entry " + std::to_string(i) +
                                                          " refers to a density out of range");
        entryMean[i] = ms.density_mean[d];
        entryCov[i]  = ms.density_covariance[d];
    }
    h->oneDensityPerMixture = true;
    for (uint32_t m = 0; m < h->nMix; ++m)
        h->oneDensityPerMixture = h->oneDensityPerMixture && mixOff[m + 1] - mixOff[m] == 1;
    // mixture->nCovariances() == 1 (cc:54): global variance optimisation, no G accumulated
    h->pooled = h->nCovs == 1;
    if (h->pooled)
        h->pooledVariance.assign(ms.variances, ms.variances + D);
    h->smallCells = affineSmallCells(D);
    h->gCells     = h->pooled ? 0 : static_cast<size_t>(D) * affineTriangle(D);
    h->maxPieces  = affineMaxPieces(maxPairs, nKeys);

    GMM_HIP_CHECK(hipSetDevice(device));
    const uint64_t P = maxPairs, slots = affineSlabSlots(maxPairs), perKey = (h->smallCells + h->gCells) * sizeof(double);
    h->tableBytes   = static_cast<uint64_t>(nKeys) * perKey;
    size_t sortBytes = 0;
    if (P)
        GMM_HIP_CHECK(static_cast<hipError_t>(accumSortTempBytes(maxPairs, keyBits(nKeys), &sortBytes)));
    h->sortTempBytes = sortBytes;
    h->scratchBytes  = slots * perKey + P * (15 * sizeof(uint32_t) + 2 * sizeof(double)) +
                      (static_cast<uint64_t>(h->maxPieces) + 1) * sizeof(uint32_t) + sortBytes;
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess)
        freeB = 0;
    const uint64_t need = h->tableBytes + h->scratchBytes;
    if (need > freeB / 4 * 3) {
        char msg[320];
        std::snprintf(msg, sizeof(msg),
                      "affine accumulator: %u keys x %.1f KiB of tables and the scratch of %u pairs need %.2f GiB of device "
                      "memory (%.2f GiB free): lower n_keys or max_pairs",
                      nKeys, static_cast<double>(perKey) / 1024.0, maxPairs, static_cast<double>(need) / (1u << 30),
                      static_cast<double>(freeB) / (1u << 30));
        return fail(GMM_ERR_UNSUPPORTED, msg);
    }

    int rc;
    if ((rc = upload(h->dMixOff, mixOff)) || (rc = upload(h->dEntryMean, entryMean)) || (rc = upload(h->dEntryCov, entryCov)))
        return rc;
    std::vector<float> means(ms.means, ms.means + static_cast<size_t>(h->nMeans) * D);
    std::vector<float> variances(ms.variances, ms.variances + static_cast<size_t>(h->nCovs) * D);
    if ((rc = upload(h->dMeans, means)) || (rc = upload(h->dVariances, variances)))
        return rc;
    GMM_HIP_CHECK(h->dSmall.alloc(nKeys * h->smallCells));
    GMM_HIP_CHECK(h->dG.alloc(nKeys * h->gCells));
    GMM_HIP_CHECK(h->dSkipped.alloc(1));
    if ((rc = zeroTables(h)) != GMM_OK)
        return rc;
    for (DeviceBuffer<uint32_t>* b : {&h->dBest, &h->dKey, &h->dMean, &h->dCov, &h->dPairIndex, &h->dKeysSorted, &h->dIndexSorted,
                                      &h->dSFrame, &h->dSMean, &h->dSCov, &h->dPairFrame, &h->dPairMix, &h->dPairDensity,
                                      &h->dPairKey})
        GMM_HIP_CHECK(b->alloc(P));
    GMM_HIP_CHECK(h->dSWeight.alloc(P));
    GMM_HIP_CHECK(h->dPairWeight.alloc(P));
    GMM_HIP_CHECK(h->dPieces.alloc(h->maxPieces));
    GMM_HIP_CHECK(h->dNPieces.allocZeroed(1));
    GMM_HIP_CHECK(h->dSlabSmall.alloc(slots * h->smallCells));
    GMM_HIP_CHECK(h->dSlabG.alloc(slots * h->gCells));
    GMM_HIP_CHECK(h->dSortTemp.alloc(h->sortTempBytes));
    GMM_HIP_CHECK(h->done.create(hipEventDisableTiming));
    return GMM_OK;
}

// the checks of an accumulate call that need no device (gmm_estimator.cc, checkCall)
int checkCall(const gmm_affine_accumulator* h, const gmm_scorer* scorer, const float* frames, uint32_t frameStride,
              const uint32_t* pairFrame, const uint32_t* pairMix, const uint32_t* pairDensity, uint32_t nPairs) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null affine accumulator");
    if (nPairs > h->maxPairs)
        return fail(GMM_ERR_CAPACITY, "n_pairs " + std::to_string(nPairs) + " exceeds the affine accumulator's max_pairs " +
                                              std::to_string(h->maxPairs));
    if (nPairs && (!frames || !pairFrame || !pairMix))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    if (frameStride < h->D)
        return fail(GMM_ERR_INVALID_ARGUMENT, "frame_stride below the dimension");
    if (pairDensity)
        return GMM_OK;
    if (!scorer) {
        if (!h->oneDensityPerMixture)
            return fail(GMM_ERR_INVALID_ARGUMENT, "no density given and no scorer: every mixture must hold exactly one density");
        return GMM_OK;
    }
    if (scorer->device != h->device)
        return fail(GMM_ERR_UNSUPPORTED, "the scorer is on another device than the affine accumulator");
    const gmm_scorer_config& c = scorer->cfg;
    if (!(c.mixture_begin == 0 && (c.mixture_end == 0 || c.mixture_end == h->nMix)))
        return fail(GMM_ERR_UNSUPPORTED, "the scorer holds a mixture shard: the affine accumulator needs the whole mixture range");
    const int rc = checkPairs(scorer);
    if (rc != GMM_OK)
        return rc;
    if (scorer->D != h->D || scorer->nMix != h->nMix || scorer->pairs->nEntries != h->nEntries)
        return fail(GMM_ERR_INVALID_ARGUMENT,
                    "the scorer's dimension, mixture count or entry count differs from the affine accumulator's mixture set");
    return GMM_OK;
}

int accumulateOn(gmm_affine_accumulator* h, gmm_scorer* scorer, const float* frames, uint32_t nFrames, uint32_t frameStride,
                 const uint32_t* pairFrame, const uint32_t* pairMix, const uint32_t* pairDensity, const double* pairWeight,
                 const uint32_t* pairKey, uint32_t nPairs, hipStream_t stream) {
    if (!pairDensity && scorer) {  // densityIndex() = bestDensity of the pair
        PairArgs a  = pairArgsOf(scorer, frames, nFrames, frameStride);
        a.pairFrame = pairFrame;
        a.pairMix   = pairMix;
        a.best      = h->dBest.get();
        a.nPairs    = nPairs;
        GMM_HIP_CHECK(launchBestPairs(a, stream));
        pairDensity = h->dBest.get();
    }
    AffineResolveArgs r{};
    r.pairFrame   = pairFrame;
    r.pairMix     = pairMix;
    r.pairDensity = pairDensity;
    r.pairKey     = pairKey;
    r.mixOff      = h->dMixOff.get();
    r.entryMean   = h->dEntryMean.get();
    r.entryCov    = h->dEntryCov.get();
    r.key         = h->dKey.get();
    r.mean        = h->dMean.get();
    r.cov         = h->dCov.get();
    r.pairIndex   = h->dPairIndex.get();
    r.skipped     = h->dSkipped.get();
    r.nPairs      = nPairs;
    r.nFrames     = nFrames;
    r.nMix        = h->nMix;
    r.nKeys       = h->nKeys;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchAffineResolve(r, stream)));
    GMM_HIP_CHECK(static_cast<hipError_t>(launchAccumSort(h->dSortTemp.get(), h->sortTempBytes, h->dKey.get(),
                                                         h->dPairIndex.get(), h->dKeysSorted.get(), h->dIndexSorted.get(),
                                                         nPairs, keyBits(h->nKeys), stream)));
    AffineArgs a{};
    a.keysSorted  = h->dKeysSorted.get();
    a.indexSorted = h->dIndexSorted.get();
    a.pairFrame   = pairFrame;
    a.pairWeight  = pairWeight;
    a.pairMean    = h->dMean.get();
    a.pairCov     = h->dCov.get();
    a.frames      = frames;
    a.means       = h->dMeans.get();
    a.variances   = h->dVariances.get();
    a.sFrame      = h->dSFrame.get();
    a.sMean       = h->dSMean.get();
    a.sCov        = h->dSCov.get();
    a.sWeight     = h->dSWeight.get();
    a.pieces      = h->dPieces.get();
    a.nPieces     = h->dNPieces.get();
    a.small       = h->dSmall.get();
    a.G           = h->gCells ? h->dG.get() : nullptr;
    a.slabSmall   = h->dSlabSmall.get();
    a.slabG       = h->gCells ? h->dSlabG.get() : nullptr;
    a.nPairs      = nPairs;
    a.nKeys       = h->nKeys;
    a.D           = h->D;
    a.frameStride = frameStride;
    a.maxPieces   = affineMaxPieces(nPairs, h->nKeys);
    GMM_HIP_CHECK(static_cast<hipError_t>(launchAffineIndexPieces(a, stream)));
    GMM_HIP_CHECK(static_cast<hipError_t>(launchAffineAccumulate(a, stream)));
    GMM_HIP_CHECK(static_cast<hipError_t>(launchAffineCombine(a, stream)));
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
    if (key >= h->nKeys)
        return fail(GMM_ERR_INVALID_ARGUMENT, "key " + std::to_string(key) + " out of range: the affine accumulator holds " +
                                                      std::to_string(h->nKeys) + " keys");
    GMM_HIP_CHECK(hipSetDevice(h->device));
    return waitDone(h);
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
    (void)hipSetDevice(h->device);
    if (h->pending)
        (void)hipEventSynchronize(h->done.get());  // no kernel of a call may outlive its scratch
    delete h;
    return GMM_OK;
}

int gmm_affine_reset(gmm_affine_accumulator* h) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null affine accumulator");
    GMM_HIP_CHECK(hipSetDevice(h->device));
    const int rc = waitDone(h);
    return rc != GMM_OK ? rc : zeroTables(h);
}

int gmm_affine_accumulate_device(gmm_affine_accumulator* h, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                 uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                 const uint32_t* pairDensity, const double* pairWeight, const uint32_t* pairKey,
                                 uint32_t nPairs, void* stream) {
    int rc = checkCall(h, scorer, frames, frameStride, pairFrame, pairMix, pairDensity, nPairs);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = accumulateOn(h, scorer, frames, nFrames, frameStride, pairFrame, pairMix, pairDensity, pairWeight, pairKey, nPairs, st);
    // recorded even after a failed launch: what was enqueued before it still uses the scratch
    GMM_HIP_CHECK(hipEventRecord(h->done.get(), st));
    h->pending = true;
    return rc;
}

int gmm_affine_accumulate_host(gmm_affine_accumulator* h, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                               uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                               const uint32_t* pairDensity, const double* pairWeight, const uint32_t* pairKey, uint32_t nPairs) {
    int rc = checkCall(h, scorer, frames, frameStride, pairFrame, pairMix, pairDensity, nPairs);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(h->device));
    if ((rc = waitDone(h)) != GMM_OK)
        return rc;
    // the frames, dense (row length D); the pair lists into the handle's staging
    DeviceBuffer<float> dFrames;
    const size_t        D = h->D, n = nPairs;
    GMM_HIP_CHECK(dFrames.alloc(std::max<size_t>(static_cast<size_t>(nFrames) * D, 1)));
    if (nFrames)
        GMM_HIP_CHECK(hipMemcpy2D(dFrames.get(), D * sizeof(float), frames, static_cast<size_t>(frameStride) * sizeof(float),
                                  D * sizeof(float), nFrames, hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(h->dPairFrame.get(), pairFrame, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(h->dPairMix.get(), pairMix, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (pairDensity)
        GMM_HIP_CHECK(hipMemcpy(h->dPairDensity.get(), pairDensity, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (pairKey)
        GMM_HIP_CHECK(hipMemcpy(h->dPairKey.get(), pairKey, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (pairWeight)
        GMM_HIP_CHECK(hipMemcpy(h->dPairWeight.get(), pairWeight, n * sizeof(double), hipMemcpyHostToDevice));
    rc = accumulateOn(h, scorer, dFrames.get(), nFrames, h->D, h->dPairFrame.get(), h->dPairMix.get(),
                      pairDensity ? h->dPairDensity.get() : nullptr, pairWeight ? h->dPairWeight.get() : nullptr,
                      pairKey ? h->dPairKey.get() : nullptr, nPairs, nullptr);
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // before dFrames is released
    return rc;
}

int gmm_affine_skipped(gmm_affine_accumulator* h, uint64_t* skipped) {
    if (!h || !skipped)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    GMM_HIP_CHECK(hipSetDevice(h->device));
    const int rc = waitDone(h);
    if (rc != GMM_OK)
        return rc;
    unsigned long long v = 0;
    GMM_HIP_CHECK(hipMemcpy(&v, h->dSkipped.get(), sizeof(v), hipMemcpyDeviceToHost));
    *skipped = v;
    return GMM_OK;
}

int gmm_affine_info(const gmm_affine_accumulator* h, uint64_t* tableBytes, uint64_t* scratchBytes, int* pooled) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null affine accumulator");
    if (tableBytes)
        *tableBytes = h->tableBytes;
    if (scratchBytes)
        *scratchBytes = h->scratchBytes;
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
    const size_t  D = h->D, D1 = D + 1, T = affineTriangle(h->D);
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
    const size_t D = h->D, D1 = D + 1, T = affineTriangle(h->D);
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
