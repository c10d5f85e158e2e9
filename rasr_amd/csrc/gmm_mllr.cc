// gmm_mllr.cc -- the handle behind include/rasr_gmm_mllr.h: the model's tables and the (key, leaf) sets' f64 accumulators
// on the device, the argument checks, the launch sequence of a call (gmm_kernels_mllr.hip), get / add.
// The estimation of the matrices from the tables and the adapted means are host/MllrEstimate.cc (no HIP).
#include <algorithm>
#include <cstdio>
#include <memory>
#include <new>

#include "gmm_estimator.hh"
#include "gmm_mllr.hh"
#include "gmm_scorer.hh"

using namespace rasr_gmm;

struct gmm_mllr_accumulator {
    int        device = 0;
    int        kinds  = 0;
    uint32_t   D = 0, nKeys = 0, nLeaves = 0, nSets = 0, maxPairs = 0, maxPieces = 0, nMix = 0, nEntries = 0, nMeans = 0, nCovs = 0;
    bool       oneDensityPerMixture = false;
    MllrLayout layout{};
    uint64_t   tableBytes = 0, scratchBytes = 0;
    // the model (device)
    DeviceBuffer<uint32_t> dMixOff, dEntryMean, dEntryCov, dLeaf;
    DeviceBuffer<float>    dMeans, dVariances;
    // the accumulators
    DeviceBuffer<double>             dTables;
    DeviceBuffer<unsigned long long> dSkipped;
    // scratch of one call of up to maxPairs pairs
    DeviceBuffer<uint32_t> dBest, dSet, dMean, dCov, dPairIndex, dSetsSorted, dIndexSorted, dSFrame, dSMean, dSCov, dPieces,
            dNPieces;
    DeviceBuffer<double> dSWeight, dSlab;
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

// bits of the sets 0 .. nSets (nSets: the skipped pairs' sentinel)
uint32_t setBits(uint32_t nSets) {
    uint32_t b = 1;
    while (b < 32 && (nSets >> b))
        ++b;
    return b;
}

int zeroTables(gmm_mllr_accumulator* h) {
    GMM_HIP_CHECK(hipMemset(h->dTables.get(), 0, h->nSets * h->layout.cells() * sizeof(double)));
    GMM_HIP_CHECK(hipMemset(h->dSkipped.get(), 0, sizeof(unsigned long long)));
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // done before a call on any other stream
    return GMM_OK;
}

int waitDone(gmm_mllr_accumulator* h) {
    if (h->pending) {
        GMM_HIP_CHECK(hipEventSynchronize(h->done.get()));
        h->pending = false;
    }
    return GMM_OK;
}

int create(gmm_mllr_accumulator* h, const gmm_mixture_set& ms, const uint32_t* leafOfMixture, uint32_t nLeaves,
           uint32_t nKeys, int kinds, uint32_t maxPairs, int device) {
    h->device   = device;
    h->kinds    = kinds;
    h->D        = ms.dimension;
    h->nKeys    = nKeys;
    h->nLeaves  = nLeaves;
    h->maxPairs = maxPairs;
    h->nMix     = ms.n_mixtures;
    h->nMeans   = ms.n_means;
    h->nCovs    = ms.n_covariances;
    h->layout   = MllrLayout{ms.dimension, (kinds & GMM_MLLR_FULL) != 0, (kinds & GMM_MLLR_SHIFT) != 0};
    const uint32_t D = h->D;
    std::vector<uint32_t> mixOff(ms.mixture_offsets, ms.mixture_offsets + ms.n_mixtures + 1);
    if (mixOff[0] != 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "mllr accumulator: mixture_offsets[0] is not 0");
    for (uint32_t m = 0; m < h->nMix; ++m)
        if (mixOff[m + 1] < mixOff[m])
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr accumulator: mixture_offsets decrease at mixture " + std::to_string(m));
    h->nEntries = mixOff[h->nMix];
    for (uint32_t d = 0; d < ms.n_densities; ++d)
        if (ms.density_mean[d] >= h->nMeans || ms.density_covariance[d] >= h->nCovs)
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr accumulator: density " + std::to_string(d) +
                                                          " refers to a mean or covariance out of range");
    std::vector<uint32_t> entryMean(h->nEntries), entryCov(h->nEntries);
    for (uint32_t i = 0; i < h->nEntries; ++i) {
        const uint32_t d = ms.mixture_densities[i];
        if (d >= ms.n_densities)
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr accumulator: mixture entry " + std::to_string(i) +
                                                          " refers to a density out of range");
        entryMean[i] = ms.density_mean[d];
        entryCov[i]  = ms.density_covariance[d];
    }
    std::vector<uint32_t> leaf(leafOfMixture, leafOfMixture + h->nMix);
    for (uint32_t m = 0; m < h->nMix; ++m)
        if (leaf[m] >= nLeaves)
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr accumulator: mixture " + std::to_string(m) + " maps to leaf " +
                                                          std::to_string(leaf[m]) + " of " + std::to_string(nLeaves));
    h->oneDensityPerMixture = true;
    for (uint32_t m = 0; m < h->nMix; ++m)
        h->oneDensityPerMixture = h->oneDensityPerMixture && mixOff[m + 1] - mixOff[m] == 1;
    const uint64_t sets = static_cast<uint64_t>(nKeys) * nLeaves;
    const uint64_t perSet = h->layout.cells() * sizeof(double);
    GMM_HIP_CHECK(hipSetDevice(device));
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess)
        freeB = 0;
    const uint64_t P = maxPairs, slots = affineSlabSlots(maxPairs);
    // the sets are sort keys with a sentinel behind them: past 32 bits no device holds the tables anyway
    const bool     keyable = sets < 0xffffffffull;
    h->nSets     = keyable ? static_cast<uint32_t>(sets) : 0;
    h->maxPieces = affineMaxPieces(maxPairs, h->nSets);
    size_t sortBytes = 0;
    if (P && keyable)
        GMM_HIP_CHECK(static_cast<hipError_t>(accumSortTempBytes(maxPairs, setBits(h->nSets), &sortBytes)));
    h->sortTempBytes = sortBytes;
    h->tableBytes    = sets * perSet;
    h->scratchBytes  = slots * perSet + P * (15 * sizeof(uint32_t) + 2 * sizeof(double)) +
                      (static_cast<uint64_t>(h->maxPieces) + 1) * sizeof(uint32_t) + sortBytes;
    const double need = static_cast<double>(sets) * static_cast<double>(perSet) + static_cast<double>(h->scratchBytes);
    if (!keyable || need > static_cast<double>(freeB / 4 * 3)) {
        char msg[360];
        std::snprintf(msg, sizeof(msg),
                      "mllr accumulator: %u keys x %u leaves x %.1f KiB of tables and the scratch of %u pairs need %.2f GiB of "
                      "device memory (%.2f GiB free): lower n_keys, n_leaves or max_pairs",
                      nKeys, nLeaves, static_cast<double>(perSet) / 1024.0, maxPairs, need / (1u << 30),
                      static_cast<double>(freeB) / (1u << 30));
        return fail(GMM_ERR_UNSUPPORTED, msg);
    }

    int rc;
    if ((rc = upload(h->dMixOff, mixOff)) || (rc = upload(h->dEntryMean, entryMean)) || (rc = upload(h->dEntryCov, entryCov)) ||
        (rc = upload(h->dLeaf, leaf)))
        return rc;
    std::vector<float> means(ms.means, ms.means + static_cast<size_t>(h->nMeans) * D);
    std::vector<float> variances(ms.variances, ms.variances + static_cast<size_t>(h->nCovs) * D);
    if ((rc = upload(h->dMeans, means)) || (rc = upload(h->dVariances, variances)))
        return rc;
    GMM_HIP_CHECK(h->dTables.alloc(h->nSets * h->layout.cells()));
    GMM_HIP_CHECK(h->dSkipped.alloc(1));
    if ((rc = zeroTables(h)) != GMM_OK)
        return rc;
    for (DeviceBuffer<uint32_t>* b : {&h->dBest, &h->dSet, &h->dMean, &h->dCov, &h->dPairIndex, &h->dSetsSorted, &h->dIndexSorted,
                                      &h->dSFrame, &h->dSMean, &h->dSCov, &h->dPairFrame, &h->dPairMix, &h->dPairDensity,
                                      &h->dPairKey})
        GMM_HIP_CHECK(b->alloc(P));
    GMM_HIP_CHECK(h->dSWeight.alloc(P));
    GMM_HIP_CHECK(h->dPairWeight.alloc(P));
    GMM_HIP_CHECK(h->dPieces.alloc(h->maxPieces));
    GMM_HIP_CHECK(h->dNPieces.allocZeroed(1));
    GMM_HIP_CHECK(h->dSlab.alloc(slots * h->layout.cells()));
    GMM_HIP_CHECK(h->dSortTemp.alloc(h->sortTempBytes));
    GMM_HIP_CHECK(h->done.create(hipEventDisableTiming));
    return GMM_OK;
}

// the checks of an accumulate call that need no device (gmm_adapt.cc, checkCall)
int checkCall(const gmm_mllr_accumulator* h, const gmm_scorer* scorer, const float* frames, uint32_t frameStride,
              const uint32_t* pairFrame, const uint32_t* pairMix, const uint32_t* pairDensity, uint32_t nPairs) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null mllr accumulator");
    if (nPairs > h->maxPairs)
        return fail(GMM_ERR_CAPACITY, "n_pairs " + std::to_string(nPairs) + " exceeds the mllr accumulator's max_pairs " +
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
        return fail(GMM_ERR_UNSUPPORTED, "the scorer is on another device than the mllr accumulator");
    const gmm_scorer_config& c = scorer->cfg;
    if (!(c.mixture_begin == 0 && (c.mixture_end == 0 || c.mixture_end == h->nMix)))
        return fail(GMM_ERR_UNSUPPORTED, "the scorer holds a mixture shard: the mllr accumulator needs the whole mixture range");
    const int rc = checkPairs(scorer);
    if (rc != GMM_OK)
        return rc;
    if (scorer->D != h->D || scorer->nMix != h->nMix || scorer->pairs->nEntries != h->nEntries)
        return fail(GMM_ERR_INVALID_ARGUMENT,
                    "the scorer's dimension, mixture count or entry count differs from the mllr accumulator's mixture set");
    return GMM_OK;
}

int accumulateOn(gmm_mllr_accumulator* h, gmm_scorer* scorer, const float* frames, uint32_t nFrames, uint32_t frameStride,
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
    MllrResolveArgs r{};
    r.pairFrame     = pairFrame;
    r.pairMix       = pairMix;
    r.pairDensity   = pairDensity;
    r.pairKey       = pairKey;
    r.mixOff        = h->dMixOff.get();
    r.entryMean     = h->dEntryMean.get();
    r.entryCov      = h->dEntryCov.get();
    r.leafOfMixture = h->dLeaf.get();
    r.set           = h->dSet.get();
    r.mean          = h->dMean.get();
    r.cov           = h->dCov.get();
    r.pairIndex     = h->dPairIndex.get();
    r.skipped       = h->dSkipped.get();
    r.nPairs        = nPairs;
    r.nFrames       = nFrames;
    r.nMix          = h->nMix;
    r.nKeys         = h->nKeys;
    r.nLeaves       = h->nLeaves;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchMllrResolve(r, stream)));
    GMM_HIP_CHECK(static_cast<hipError_t>(launchAccumSort(h->dSortTemp.get(), h->sortTempBytes, h->dSet.get(),
                                                         h->dPairIndex.get(), h->dSetsSorted.get(), h->dIndexSorted.get(),
                                                         nPairs, setBits(h->nSets), stream)));
    const uint32_t maxPieces = affineMaxPieces(nPairs, h->nSets);
    AffineArgs     g{};  // pass 3: the affine index pass, the sets in the place of its keys
    g.keysSorted  = h->dSetsSorted.get();
    g.indexSorted = h->dIndexSorted.get();
    g.pairFrame   = pairFrame;
    g.pairWeight  = pairWeight;
    g.pairMean    = h->dMean.get();
    g.pairCov     = h->dCov.get();
    g.sFrame      = h->dSFrame.get();
    g.sMean       = h->dSMean.get();
    g.sCov        = h->dSCov.get();
    g.sWeight     = h->dSWeight.get();
    g.pieces      = h->dPieces.get();
    g.nPieces     = h->dNPieces.get();
    g.nPairs      = nPairs;
    g.nKeys       = h->nSets;
    g.maxPieces   = maxPieces;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchAffineIndexPieces(g, stream)));
    MllrArgs a{};
    a.setsSorted  = h->dSetsSorted.get();
    a.sFrame      = h->dSFrame.get();
    a.sMean       = h->dSMean.get();
    a.sCov        = h->dSCov.get();
    a.sWeight     = h->dSWeight.get();
    a.frames      = frames;
    a.means       = h->dMeans.get();
    a.variances   = h->dVariances.get();
    a.pieces      = h->dPieces.get();
    a.nPieces     = h->dNPieces.get();
    a.tables      = h->dTables.get();
    a.slab        = h->dSlab.get();
    a.layout      = h->layout;
    a.nPairs      = nPairs;
    a.nSets       = h->nSets;
    a.frameStride = frameStride;
    a.maxPieces   = maxPieces;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchMllrAccumulate(a, stream)));
    GMM_HIP_CHECK(static_cast<hipError_t>(launchMllrCombine(a, stream)));
    return GMM_OK;
}

// waits for the last call; cells: the raw range of the set (key, leaf) on the host
int fetchSet(gmm_mllr_accumulator* h, uint32_t key, uint32_t leaf, std::vector<double>& cells) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null mllr accumulator");
    if (key >= h->nKeys || leaf >= h->nLeaves)
        return fail(GMM_ERR_INVALID_ARGUMENT, "key " + std::to_string(key) + " or leaf " + std::to_string(leaf) +
                                                      " out of range: the mllr accumulator holds " + std::to_string(h->nKeys) +
                                                      " keys x " + std::to_string(h->nLeaves) + " leaves");
    GMM_HIP_CHECK(hipSetDevice(h->device));
    const int rc = waitDone(h);
    if (rc != GMM_OK)
        return rc;
    const size_t C = h->layout.cells();
    cells.resize(C);
    GMM_HIP_CHECK(hipMemcpy(cells.data(), h->dTables.get() + (static_cast<size_t>(key) * h->nLeaves + leaf) * C,
                            C * sizeof(double), hipMemcpyDeviceToHost));
    return GMM_OK;
}

int checkKinds(const gmm_mllr_accumulator* h, bool wantsFull, bool wantsShift) {
    if (h && ((wantsFull && !h->layout.full) || (wantsShift && !h->layout.shift)))
        return fail(GMM_ERR_INVALID_ARGUMENT, "the mllr accumulator does not hold the tables of that kind");
    return GMM_OK;
}

}  // namespace

extern "C" {

int gmm_mllr_create(const gmm_mixture_set* ms, const uint32_t* leafOfMixture, uint32_t nLeaves, uint32_t nKeys, int kinds,
                    uint32_t maxPairs, int device, gmm_mllr_accumulator** out) {
    if (!ms || !out || !ms->mixture_offsets || !ms->means || !ms->variances || (ms->n_mixtures && !leafOfMixture) ||
        (ms->n_densities && (!ms->density_mean || !ms->density_covariance)))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (ms->mixture_offsets[ms->n_mixtures] && !ms->mixture_densities)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    if (nKeys == 0 || nLeaves == 0 || kinds == 0 || (kinds & ~(GMM_MLLR_FULL | GMM_MLLR_SHIFT)) || ms->dimension == 0 ||
        ms->n_covariances == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT,
                    "mllr accumulator: n_keys, n_leaves, the dimension and the covariance count must not be 0, kinds a mask "
                    "of GMM_MLLR_FULL and GMM_MLLR_SHIFT");
    if (ms->dimension > GMM_MLLR_MAX_DIMENSION)
        return fail(GMM_ERR_UNSUPPORTED, "mllr accumulator: dimension " + std::to_string(ms->dimension) + " exceeds " +
                                                 std::to_string(GMM_MLLR_MAX_DIMENSION));
    std::unique_ptr<gmm_mllr_accumulator> h(new (std::nothrow) gmm_mllr_accumulator);
    if (!h)
        return fail(GMM_ERR_OUT_OF_MEMORY, "out of host memory");
    const int rc = create(h.get(), *ms, leafOfMixture, nLeaves, nKeys, kinds, maxPairs, device);
    if (rc != GMM_OK)
        return rc;
    *out = h.release();
    return GMM_OK;
}

int gmm_mllr_destroy(gmm_mllr_accumulator* h) {
    if (!h)
        return GMM_OK;
    (void)hipSetDevice(h->device);
    if (h->pending)
        (void)hipEventSynchronize(h->done.get());  // no kernel of a call may outlive its scratch
    delete h;
    return GMM_OK;
}

int gmm_mllr_reset(gmm_mllr_accumulator* h) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null mllr accumulator");
    GMM_HIP_CHECK(hipSetDevice(h->device));
    const int rc = waitDone(h);
    return rc != GMM_OK ? rc : zeroTables(h);
}

int gmm_mllr_accumulate_device(gmm_mllr_accumulator* h, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
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

int gmm_mllr_accumulate_host(gmm_mllr_accumulator* h, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
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

int gmm_mllr_skipped(gmm_mllr_accumulator* h, uint64_t* skipped) {
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

int gmm_mllr_info(const gmm_mllr_accumulator* h, uint64_t* tableBytes, uint64_t* scratchBytes, int* kinds) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null mllr accumulator");
    if (tableBytes)
        *tableBytes = h->tableBytes;
    if (scratchBytes)
        *scratchBytes = h->scratchBytes;
    if (kinds)
        *kinds = h->kinds;
    return GMM_OK;
}

int gmm_mllr_get(gmm_mllr_accumulator* h, uint32_t key, uint32_t leaf, double* Z, double* G, double* countFull,
                 double* countShift, double* beta, double* shift) {
    int rc = checkKinds(h, Z || G || countFull, countShift || beta || shift);
    if (rc != GMM_OK)
        return rc;
    std::vector<double> c;
    if ((rc = fetchSet(h, key, leaf, c)) != GMM_OK)
        return rc;
    const MllrLayout& L = h->layout;
    const size_t      D = L.D;
    if (Z)
        std::copy(c.begin() + L.z(), c.begin() + L.z() + L.zCells(), Z);
    if (G)
        std::copy(c.begin() + L.g(), c.begin() + L.g() + L.gCells(), G);
    if (countFull)
        *countFull = c[L.countFull()];
    if (countShift)
        *countShift = c[L.countShift()];
    if (beta)
        std::copy(c.begin() + L.beta(), c.begin() + L.beta() + D, beta);
    if (shift)
        std::copy(c.begin() + L.shiftSum(), c.begin() + L.shiftSum() + D, shift);
    return GMM_OK;
}

int gmm_mllr_add(gmm_mllr_accumulator* h, uint32_t key, uint32_t leaf, const double* Z, const double* G,
                 const double* countFull, const double* countShift, const double* beta, const double* shift, double weight) {
    int rc = checkKinds(h, Z || G || countFull, countShift || beta || shift);
    if (rc != GMM_OK)
        return rc;
    std::vector<double> c;
    if ((rc = fetchSet(h, key, leaf, c)) != GMM_OK)
        return rc;
    const MllrLayout& L = h->layout;
    const size_t      D = L.D;
    // dst = dst + src * weight: one multiply, one add (the unit is built with -ffp-contract=off)
    auto add = [weight, &c](size_t at, const double* src, size_t n) {
        for (size_t x = 0; src && x < n; ++x) {
            const double scaled = src[x] * weight;
            c[at + x]           = c[at + x] + scaled;
        }
    };
    add(L.z(), Z, L.zCells());
    add(L.g(), G, L.gCells());
    add(L.beta(), beta, D);
    add(L.shiftSum(), shift, D);
    if (countFull)  // count_ += a.count_ (cc:276)
        c[L.countFull()] = c[L.countFull()] + *countFull;
    if (countShift)
        c[L.countShift()] = c[L.countShift()] + *countShift;
    GMM_HIP_CHECK(hipMemcpy(h->dTables.get() + (static_cast<size_t>(key) * h->nLeaves + leaf) * c.size(), c.data(),
                            c.size() * sizeof(double), hipMemcpyHostToDevice));
    return GMM_OK;
}

}  // extern "C"
