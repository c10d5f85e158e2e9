// gmm_estimator.cc -- the handle behind include/rasr_gmm_estimator.h: topology and f64 tables on the device, the
// argument checks, the launch sequence of a call (gmm_kernels_accum.hip), get / serialize / write / estimate.
// The file format (serialize, combine) is host/MixtureSetEstimatorFile.cc.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

#include "gmm_estimator.hh"
#include "gmm_scorer.hh"

using namespace rasr_gmm;

struct gmm_estimator {
    int      device = 0;
    uint32_t D = 0, nMeans = 0, nCovs = 0, nDens = 0, nMix = 0, nEntries = 0, maxPairs = 0;
    bool     oneDensityPerMixture = false;
    // the topology's index tables (host: serialize; device: resolvePairs)
    std::vector<uint32_t>  dnsMean, dnsCov, mixOff, mixDens;
    DeviceBuffer<uint32_t> dMixOff, dEntryMean, dEntryCov;
    // the accumulators
    DeviceBuffer<double>             dMeanSums, dMeanWeights, dCovSums, dCovWeights, dEntryWeights;
    DeviceBuffer<unsigned long long> dSkipped;
    // scratch of one call of up to maxPairs pairs
    DeviceBuffer<uint32_t> dBest, dKeyMean, dKeyCov, dKeyEntry, dPairIndex, dKeysSorted, dIndexSorted;
    DeviceBuffer<double>   dSlabSums, dSlabWeights;
    DeviceBuffer<void>     dSortTemp;
    size_t                 sortTempBytes = 0;
    // the host call's pair lists
    DeviceBuffer<uint32_t> dPairFrame, dPairMix, dPairDensity;
    DeviceBuffer<double>   dPairWeight;
    // Baum-Welch calls: the posterior rows and the contributions' frames and weights, maxPairs elements each,
    // allocated by the handle's first posterior call
    uint32_t               maxEntries = 1;  // K_max: the largest entry count of a mixture (at least 1)
    bool                   posteriorScratch = false;
    DeviceBuffer<float>    dPostRows;
    DeviceBuffer<uint32_t> dContribFrame;
    DeviceBuffer<double>   dContribWeight;
    // discriminative calls: the denominator tables (the numerator's shapes) and the second slab, allocated and zeroed
    // by the handle's first discriminative call; the posterior form's second weight list with the posterior scratch
    bool                 denominatorTables = false;
    DeviceBuffer<double> dDenMeanSums, dDenMeanWeights, dDenCovSums, dDenCovWeights, dDenEntryWeights;
    DeviceBuffer<double> dDenSlabSums, dDenSlabWeights, dPairWeightDen;
    bool                 denominatorPosteriorScratch = false;
    DeviceBuffer<double> dContribWeightDen;
    double               objective = 0.0;  // objectiveFunction_ (host)
    // recorded by every accumulate call on its stream; get / skipped / serialize wait for it
    Event done;
    bool  pending = false;
};

namespace {

// bits of the keys 0 .. nDest (nDest: the skipped pairs' sentinel)
uint32_t keyBits(uint32_t nDest) {
    uint32_t b = 1;
    while (b < 32 && (nDest >> b))
        ++b;
    return b;
}

int zeroDenominatorTables(gmm_estimator* e) {
    const size_t D = e->D;
    if (e->nMeans) {
        GMM_HIP_CHECK(hipMemset(e->dDenMeanSums.get(), 0, e->nMeans * D * sizeof(double)));
        GMM_HIP_CHECK(hipMemset(e->dDenMeanWeights.get(), 0, e->nMeans * sizeof(double)));
    }
    if (e->nCovs) {
        GMM_HIP_CHECK(hipMemset(e->dDenCovSums.get(), 0, e->nCovs * D * sizeof(double)));
        GMM_HIP_CHECK(hipMemset(e->dDenCovWeights.get(), 0, e->nCovs * sizeof(double)));
    }
    if (e->nEntries)
        GMM_HIP_CHECK(hipMemset(e->dDenEntryWeights.get(), 0, e->nEntries * sizeof(double)));
    return GMM_OK;
}

int zeroTables(gmm_estimator* e) {
    const size_t D = e->D;
    if (e->nMeans) {
        GMM_HIP_CHECK(hipMemset(e->dMeanSums.get(), 0, e->nMeans * D * sizeof(double)));
        GMM_HIP_CHECK(hipMemset(e->dMeanWeights.get(), 0, e->nMeans * sizeof(double)));
    }
    if (e->nCovs) {
        GMM_HIP_CHECK(hipMemset(e->dCovSums.get(), 0, e->nCovs * D * sizeof(double)));
        GMM_HIP_CHECK(hipMemset(e->dCovWeights.get(), 0, e->nCovs * sizeof(double)));
    }
    if (e->nEntries)
        GMM_HIP_CHECK(hipMemset(e->dEntryWeights.get(), 0, e->nEntries * sizeof(double)));
    GMM_HIP_CHECK(hipMemset(e->dSkipped.get(), 0, sizeof(unsigned long long)));
    if (e->denominatorTables) {
        const int rc = zeroDenominatorTables(e);
        if (rc != GMM_OK)
            return rc;
    }
    e->objective = 0.0;
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // done before a call on any other stream
    return GMM_OK;
}

int waitDone(gmm_estimator* e) {
    if (e->pending) {
        GMM_HIP_CHECK(hipEventSynchronize(e->done.get()));
        e->pending = false;
    }
    return GMM_OK;
}

int create(gmm_estimator* e, const gmm_mixture_set& ms, uint32_t maxPairs, int device) {
    e->device   = device;
    e->D        = ms.dimension;
    e->nMeans   = ms.n_means;
    e->nCovs    = ms.n_covariances;
    e->nDens    = ms.n_densities;
    e->nMix     = ms.n_mixtures;
    e->maxPairs = maxPairs;
    e->mixOff.assign(ms.mixture_offsets, ms.mixture_offsets + ms.n_mixtures + 1);
    if (e->mixOff[0] != 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "estimator topology: mixture_offsets[0] is not 0");
    for (uint32_t m = 0; m < e->nMix; ++m)
        if (e->mixOff[m + 1] < e->mixOff[m])
            return fail(GMM_ERR_INVALID_ARGUMENT, "estimator topology: mixture_offsets decrease at mixture " + std::to_string(m));
    e->nEntries = e->mixOff[e->nMix];
    if (e->nDens)
        e->dnsMean.assign(ms.density_mean, ms.density_mean + e->nDens);
    if (e->nDens)
        e->dnsCov.assign(ms.density_covariance, ms.density_covariance + e->nDens);
    if (e->nEntries)
        e->mixDens.assign(ms.mixture_densities, ms.mixture_densities + e->nEntries);
    for (uint32_t d = 0; d < e->nDens; ++d)
        if (e->dnsMean[d] >= e->nMeans || e->dnsCov[d] >= e->nCovs)
            return fail(GMM_ERR_INVALID_ARGUMENT, "estimator topology: density " + std::to_string(d) +
                                                          " refers to a mean or covariance out of range");
    std::vector<uint32_t> entryMean(e->nEntries), entryCov(e->nEntries);
    for (uint32_t i = 0; i < e->nEntries; ++i) {
        if (e->mixDens[i] >= e->nDens)
            return fail(GMM_ERR_INVALID_ARGUMENT, "estimator topology: mixture entry " + std::to_string(i) +
                                                          " refers to a density out of range");
        entryMean[i] = e->dnsMean[e->mixDens[i]];
        entryCov[i]  = e->dnsCov[e->mixDens[i]];
    }
    e->oneDensityPerMixture = true;
    for (uint32_t m = 0; m < e->nMix; ++m) {
        e->oneDensityPerMixture = e->oneDensityPerMixture && e->mixOff[m + 1] - e->mixOff[m] == 1;
        e->maxEntries           = std::max(e->maxEntries, e->mixOff[m + 1] - e->mixOff[m]);
    }

    GMM_HIP_CHECK(hipSetDevice(device));
    int rc;
    if ((rc = upload(e->dMixOff, e->mixOff)) || (rc = upload(e->dEntryMean, entryMean)) || (rc = upload(e->dEntryCov, entryCov)))
        return rc;
    const size_t D = e->D, P = maxPairs, slots = accumSlabSlots(maxPairs);
    GMM_HIP_CHECK(e->dMeanSums.alloc(e->nMeans * D));
    GMM_HIP_CHECK(e->dMeanWeights.alloc(e->nMeans));
    GMM_HIP_CHECK(e->dCovSums.alloc(e->nCovs * D));
    GMM_HIP_CHECK(e->dCovWeights.alloc(e->nCovs));
    GMM_HIP_CHECK(e->dEntryWeights.alloc(e->nEntries));
    GMM_HIP_CHECK(e->dSkipped.alloc(1));
    if ((rc = zeroTables(e)) != GMM_OK)
        return rc;
    for (DeviceBuffer<uint32_t>* b : {&e->dBest, &e->dKeyMean, &e->dKeyCov, &e->dKeyEntry, &e->dPairIndex, &e->dKeysSorted,
                                      &e->dIndexSorted, &e->dPairFrame, &e->dPairMix, &e->dPairDensity})
        GMM_HIP_CHECK(b->alloc(P));
    GMM_HIP_CHECK(e->dPairWeight.alloc(P));
    GMM_HIP_CHECK(e->dSlabSums.alloc(slots * D));
    GMM_HIP_CHECK(e->dSlabWeights.alloc(slots));
    // the sorts' temporary storage: the largest of the three key ranges at max_pairs
    for (uint32_t nDest : {e->nMeans, e->nCovs, e->nEntries}) {
        size_t bytes = 0;
        if (P)
            GMM_HIP_CHECK(static_cast<hipError_t>(accumSortTempBytes(maxPairs, keyBits(nDest), &bytes)));
        e->sortTempBytes = std::max(e->sortTempBytes, bytes);
    }
    GMM_HIP_CHECK(e->dSortTemp.alloc(e->sortTempBytes));
    GMM_HIP_CHECK(e->done.create(hipEventDisableTiming));
    return GMM_OK;
}

// the checks of an accumulate call that need no device
int checkCall(const gmm_estimator* e, const gmm_scorer* scorer, const float* frames, uint32_t frameStride,
              const uint32_t* pairFrame, const uint32_t* pairMix, const uint32_t* pairDensity, uint32_t nPairs) {
    if (!e)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null estimator");
    if (nPairs > e->maxPairs)
        return fail(GMM_ERR_CAPACITY, "n_pairs " + std::to_string(nPairs) + " exceeds the estimator's max_pairs " +
                                              std::to_string(e->maxPairs));
    if (nPairs && (!frames || !pairFrame || !pairMix))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    if (frameStride < e->D)
        return fail(GMM_ERR_INVALID_ARGUMENT, "frame_stride below the dimension");
    if (pairDensity)
        return GMM_OK;
    if (!scorer) {
        if (!e->oneDensityPerMixture)  // verify_(mixture->nDensities() == 1), AbstractMixtureSetEstimator.cc:382
            return fail(GMM_ERR_INVALID_ARGUMENT, "no density given and no scorer: every mixture must hold exactly one density");
        return GMM_OK;
    }
    if (scorer->device != e->device)
        return fail(GMM_ERR_UNSUPPORTED, "the scorer is on another device than the estimator");
    const gmm_scorer_config& c = scorer->cfg;
    if (!(c.mixture_begin == 0 && (c.mixture_end == 0 || c.mixture_end == e->nMix)))
        return fail(GMM_ERR_UNSUPPORTED, "the scorer holds a mixture shard: the estimator needs the whole mixture range");
    const int rc = checkPairs(scorer);
    if (rc != GMM_OK)
        return rc;
    if (scorer->D != e->D || scorer->nMix != e->nMix || scorer->pairs->nEntries != e->nEntries)
        return fail(GMM_ERR_INVALID_ARGUMENT, "the scorer's dimension, mixture count or entry count differs from the estimator's topology");
    return GMM_OK;
}

// the three inverted indexes of a call whose keys are written (dKeyMean / dKeyCov / dKeyEntry, dPairIndex = 0, 1, ...):
// per index the stable sort, the ordered sums of the pieces, the pieces' combination.  n contributions; pairFrame and
// pairWeight are indexed by contribution
int accumulateKeyed(gmm_estimator* e, const float* frames, uint32_t frameStride, const uint32_t* pairFrame,
                    const double* pairWeight, uint32_t nPairs, hipStream_t stream) {
    AccumArgs a{};
    a.keysSorted  = e->dKeysSorted.get();
    a.indexSorted = e->dIndexSorted.get();
    a.pairFrame   = pairFrame;
    a.pairWeight  = pairWeight;
    a.frames      = frames;
    a.slabSums    = e->dSlabSums.get();
    a.slabWeights = e->dSlabWeights.get();
    a.nPairs      = nPairs;
    a.D           = e->D;
    a.frameStride = frameStride;
    struct Index {
        const uint32_t* keys;
        uint32_t        nDest;
        double *        sums, *weights;
        int             mode;
    };
    const Index indexes[3] = {{e->dKeyMean.get(), e->nMeans, e->dMeanSums.get(), e->dMeanWeights.get(), kAccumSum},
                              {e->dKeyCov.get(), e->nCovs, e->dCovSums.get(), e->dCovWeights.get(), kAccumSquare},
                              {e->dKeyEntry.get(), e->nEntries, nullptr, e->dEntryWeights.get(), kAccumWeightOnly}};
    for (const Index& x : indexes) {
        if (x.nDest == 0)
            continue;
        GMM_HIP_CHECK(static_cast<hipError_t>(launchAccumSort(e->dSortTemp.get(), e->sortTempBytes, x.keys, e->dPairIndex.get(),
                                                             e->dKeysSorted.get(), e->dIndexSorted.get(), nPairs,
                                                             keyBits(x.nDest), stream)));
        a.nDest   = x.nDest;
        a.sums    = x.sums;
        a.weights = x.weights;
        a.mode    = x.mode;
        GMM_HIP_CHECK(static_cast<hipError_t>(launchAccumulateSegments(a, stream)));
        GMM_HIP_CHECK(static_cast<hipError_t>(launchCombinePieces(a, stream)));
    }
    return GMM_OK;
}

int accumulateOn(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames, uint32_t frameStride,
                 const uint32_t* pairFrame, const uint32_t* pairMix, const uint32_t* pairDensity,
                 const double* pairWeight, uint32_t nPairs, hipStream_t stream) {
    if (nPairs == 0)
        return GMM_OK;
    if (!pairDensity && scorer) {  // the Viterbi branch: densityIndex() = bestDensity of the pair
        PairArgs a  = pairArgsOf(scorer, frames, nFrames, frameStride);
        a.pairFrame = pairFrame;
        a.pairMix   = pairMix;
        a.best      = e->dBest.get();
        a.nPairs    = nPairs;
        GMM_HIP_CHECK(launchBestPairs(a, stream));
        pairDensity = e->dBest.get();
    }
    ResolveArgs r{};
    r.pairFrame   = pairFrame;
    r.pairMix     = pairMix;
    r.pairDensity = pairDensity;
    r.mixOff      = e->dMixOff.get();
    r.entryMean   = e->dEntryMean.get();
    r.entryCov    = e->dEntryCov.get();
    r.keyMean     = e->dKeyMean.get();
    r.keyCov      = e->dKeyCov.get();
    r.keyEntry    = e->dKeyEntry.get();
    r.pairIndex   = e->dPairIndex.get();
    r.skipped     = e->dSkipped.get();
    r.nPairs      = nPairs;
    r.nFrames     = nFrames;
    r.nMix        = e->nMix;
    r.nMeans      = e->nMeans;
    r.nCovs       = e->nCovs;
    r.nEntries    = e->nEntries;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchResolvePairs(r, stream)));
    return accumulateKeyed(e, frames, frameStride, pairFrame, pairWeight, nPairs, stream);
}

// the checks of a posterior call that need no device: checkCall's, diagonal-sum only, contribution slots
int checkPosteriorCall(const gmm_estimator* e, const gmm_scorer* scorer, const float* frames, uint32_t frameStride,
                       const uint32_t* pairFrame, const uint32_t* pairMix, uint32_t nPairs) {
    if (!e)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null estimator");
    // n_pairs <= n_pairs * K_max: checkCall's own capacity check cannot fire before this one
    const uint64_t slots = static_cast<uint64_t>(nPairs) * (scorer ? e->maxEntries : 1u);
    if (slots > e->maxPairs)
        return fail(GMM_ERR_CAPACITY, std::to_string(nPairs) + " pairs of up to " + std::to_string(scorer ? e->maxEntries : 1u) +
                                              " densities exceed the estimator's max_pairs " + std::to_string(e->maxPairs) +
                                              " (contribution slots for this call)");
    int rc = checkCall(e, scorer, frames, frameStride, pairFrame, pairMix, nullptr, nPairs);
    if (rc == GMM_OK && scorer)
        rc = checkPosteriors(scorer);
    return rc;
}

// the posterior scratch, on the handle's first posterior call
int ensurePosteriorScratch(gmm_estimator* e) {
    if (e->posteriorScratch)
        return GMM_OK;
    GMM_HIP_CHECK(e->dPostRows.alloc(e->maxPairs));
    GMM_HIP_CHECK(e->dContribFrame.alloc(e->maxPairs));
    GMM_HIP_CHECK(e->dContribWeight.alloc(e->maxPairs));
    e->posteriorScratch = true;
    return GMM_OK;
}

// the Baum-Welch call: posteriors and expansion into contribution slots (one kernel), then the keyed tail over them
int accumulatePosteriorsOn(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                           uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                           const double* pairWeight, uint32_t nPairs, double threshold, hipStream_t stream) {
    PosteriorArgs q{};
    if (scorer)
        q.pair = pairArgsOf(scorer, frames, nFrames, frameStride);
    else {
        q.pair.nFrames   = nFrames;
        q.pair.nMixtures = e->nMix;
        q.pair.mixOff    = e->dMixOff.get();
    }
    q.pair.pairFrame = pairFrame;
    q.pair.pairMix   = pairMix;
    q.pair.nPairs    = nPairs;
    q.posteriors     = e->dPostRows.get();
    q.rowStride      = scorer ? e->maxEntries : 1u;
    q.pairWeight     = pairWeight;
    q.threshold      = threshold;
    q.entryMean      = e->dEntryMean.get();
    q.entryCov       = e->dEntryCov.get();
    q.keyMean        = e->dKeyMean.get();
    q.keyCov         = e->dKeyCov.get();
    q.keyEntry       = e->dKeyEntry.get();
    q.contribIndex   = e->dPairIndex.get();
    q.contribFrame   = e->dContribFrame.get();
    q.contribWeight  = e->dContribWeight.get();
    q.skipped        = e->dSkipped.get();
    q.nMeans         = e->nMeans;
    q.nCovs          = e->nCovs;
    q.nEntries       = e->nEntries;
    GMM_HIP_CHECK(scorer ? launchDensityPosteriors(q, stream) : launchExpandSingleDensity(q, stream));
    return accumulateKeyed(e, frames, frameStride, e->dContribFrame.get(), e->dContribWeight.get(), nPairs * q.rowStride,
                           stream);
}

// the denominator tables and the second slab, on the handle's first discriminative call
int ensureDenominatorTables(gmm_estimator* e) {
    if (e->denominatorTables)
        return GMM_OK;
    const size_t D = e->D, slots = accumSlabSlots(e->maxPairs);
    GMM_HIP_CHECK(e->dDenMeanSums.alloc(e->nMeans * D));
    GMM_HIP_CHECK(e->dDenMeanWeights.alloc(e->nMeans));
    GMM_HIP_CHECK(e->dDenCovSums.alloc(e->nCovs * D));
    GMM_HIP_CHECK(e->dDenCovWeights.alloc(e->nCovs));
    GMM_HIP_CHECK(e->dDenEntryWeights.alloc(e->nEntries));
    GMM_HIP_CHECK(e->dDenSlabSums.alloc(slots * D));
    GMM_HIP_CHECK(e->dDenSlabWeights.alloc(slots));
    GMM_HIP_CHECK(e->dPairWeightDen.alloc(e->maxPairs));
    const int rc = zeroDenominatorTables(e);
    if (rc != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // done before the call on any other stream
    e->denominatorTables = true;
    return GMM_OK;
}

int ensureDenominatorPosteriorScratch(gmm_estimator* e) {
    if (e->denominatorPosteriorScratch)
        return GMM_OK;
    GMM_HIP_CHECK(e->dContribWeightDen.alloc(e->maxPairs));
    e->denominatorPosteriorScratch = true;
    return GMM_OK;
}

// accumulateKeyed with two accumulators per destination (gmm_kernels_accum_dual.hip): the same three sorts, once.
// weightNum / weightDen are indexed by contribution, NaN where the contribution is not live on the side, NULL for a
// side that receives nothing
int accumulateKeyedDual(gmm_estimator* e, const float* frames, uint32_t frameStride, const uint32_t* pairFrame,
                        const double* weightNum, const double* weightDen, uint32_t nPairs, hipStream_t stream) {
    DualAccumArgs a{};
    a.keysSorted     = e->dKeysSorted.get();
    a.indexSorted    = e->dIndexSorted.get();
    a.pairFrame      = pairFrame;
    a.frames         = frames;
    a.weight[0]      = weightNum;
    a.weight[1]      = weightDen;
    a.slabSums[0]    = e->dSlabSums.get();
    a.slabSums[1]    = e->dDenSlabSums.get();
    a.slabWeights[0] = e->dSlabWeights.get();
    a.slabWeights[1] = e->dDenSlabWeights.get();
    a.nPairs         = nPairs;
    a.D              = e->D;
    a.frameStride    = frameStride;
    struct Index {
        const uint32_t* keys;
        uint32_t        nDest;
        double *        sums, *weights, *denSums, *denWeights;
        int             mode;
    };
    const Index indexes[3] = {
            {e->dKeyMean.get(), e->nMeans, e->dMeanSums.get(), e->dMeanWeights.get(), e->dDenMeanSums.get(),
             e->dDenMeanWeights.get(), kAccumSum},
            {e->dKeyCov.get(), e->nCovs, e->dCovSums.get(), e->dCovWeights.get(), e->dDenCovSums.get(),
             e->dDenCovWeights.get(), kAccumSquare},
            {e->dKeyEntry.get(), e->nEntries, nullptr, e->dEntryWeights.get(), nullptr, e->dDenEntryWeights.get(),
             kAccumWeightOnly}};
    for (const Index& x : indexes) {
        if (x.nDest == 0)
            continue;
        GMM_HIP_CHECK(static_cast<hipError_t>(launchAccumSort(e->dSortTemp.get(), e->sortTempBytes, x.keys, e->dPairIndex.get(),
                                                             e->dKeysSorted.get(), e->dIndexSorted.get(), nPairs,
                                                             keyBits(x.nDest), stream)));
        a.nDest      = x.nDest;
        a.sums[0]    = x.sums;
        a.sums[1]    = x.denSums;
        a.weights[0] = x.weights;
        a.weights[1] = x.denWeights;
        a.mode       = x.mode;
        GMM_HIP_CHECK(static_cast<hipError_t>(launchAccumulateSegmentsDual(a, stream)));
        GMM_HIP_CHECK(static_cast<hipError_t>(launchCombinePiecesDual(a, stream)));
    }
    return GMM_OK;
}

// the joint Viterbi call: accumulateOn with two weight lists
int accumulateDiscriminativeOn(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                               uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                               const uint32_t* pairDensity, const double* weightNum, const double* weightDen,
                               uint32_t nPairs, hipStream_t stream) {
    if (!pairDensity && scorer) {  // the Viterbi branch: densityIndex() = bestDensity of the pair
        PairArgs a  = pairArgsOf(scorer, frames, nFrames, frameStride);
        a.pairFrame = pairFrame;
        a.pairMix   = pairMix;
        a.best      = e->dBest.get();
        a.nPairs    = nPairs;
        GMM_HIP_CHECK(launchBestPairs(a, stream));
        pairDensity = e->dBest.get();
    }
    DualResolveArgs q{};
    ResolveArgs&    r = q.r;
    r.pairFrame       = pairFrame;
    r.pairMix         = pairMix;
    r.pairDensity     = pairDensity;
    r.mixOff          = e->dMixOff.get();
    r.entryMean       = e->dEntryMean.get();
    r.entryCov        = e->dEntryCov.get();
    r.keyMean         = e->dKeyMean.get();
    r.keyCov          = e->dKeyCov.get();
    r.keyEntry        = e->dKeyEntry.get();
    r.pairIndex       = e->dPairIndex.get();
    r.skipped         = e->dSkipped.get();
    r.nPairs          = nPairs;
    r.nFrames         = nFrames;
    r.nMix            = e->nMix;
    r.nMeans          = e->nMeans;
    r.nCovs           = e->nCovs;
    r.nEntries        = e->nEntries;
    q.weightNum       = weightNum;
    q.weightDen       = weightDen;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchResolvePairsDual(q, stream)));
    return accumulateKeyedDual(e, frames, frameStride, pairFrame, weightNum, weightDen, nPairs, stream);
}

// the joint Baum-Welch call: the posterior rows once (the kernel of gmm_density_posteriors_pairs_device), their
// expansion into contribution slots with one finalWeight per side, then the dual keyed tail
int accumulateDiscriminativePosteriorsOn(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                         uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                         const double* weightNum, const double* weightDen, uint32_t nPairs,
                                         double threshold, hipStream_t stream) {
    const uint32_t rowStride = scorer ? e->maxEntries : 1u;
    if (scorer) {
        PosteriorArgs q{};
        q.pair           = pairArgsOf(scorer, frames, nFrames, frameStride);
        q.pair.pairFrame = pairFrame;
        q.pair.pairMix   = pairMix;
        q.pair.nPairs    = nPairs;
        q.posteriors     = e->dPostRows.get();
        q.rowStride      = rowStride;
        GMM_HIP_CHECK(launchDensityPosteriors(q, stream));
    }
    DualExpandArgs x{};
    x.pairFrame        = pairFrame;
    x.pairMix          = pairMix;
    x.weightNum        = weightNum;
    x.weightDen        = weightDen;
    x.posteriors       = scorer ? e->dPostRows.get() : nullptr;
    x.mixOff           = e->dMixOff.get();
    x.entryMean        = e->dEntryMean.get();
    x.entryCov         = e->dEntryCov.get();
    x.keyMean          = e->dKeyMean.get();
    x.keyCov           = e->dKeyCov.get();
    x.keyEntry         = e->dKeyEntry.get();
    x.contribIndex     = e->dPairIndex.get();
    x.contribFrame     = e->dContribFrame.get();
    x.contribWeightNum = e->dContribWeight.get();
    x.contribWeightDen = e->dContribWeightDen.get();
    x.skipped          = e->dSkipped.get();
    x.threshold        = threshold;
    x.nPairs           = nPairs;
    x.rowStride        = rowStride;
    x.nFrames          = nFrames;
    x.nMix             = e->nMix;
    x.nMeans           = e->nMeans;
    x.nCovs            = e->nCovs;
    x.nEntries         = e->nEntries;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchExpandDual(x, stream)));
    return accumulateKeyedDual(e, frames, frameStride, e->dContribFrame.get(), weightNum ? e->dContribWeight.get() : nullptr,
                               weightDen ? e->dContribWeightDen.get() : nullptr, nPairs * rowStride, stream);
}

// the checks of a discriminative call that need no device, and what its first call on a handle allocates
int checkSides(const double* weightNum, const double* weightDen) {
    if (!weightNum && !weightDen)
        return fail(GMM_ERR_INVALID_ARGUMENT, "pair_weight_num and pair_weight_den are both NULL: the call has no side to add to");
    return GMM_OK;
}

// host copies of the tables, after the last call
struct HostTables {
    std::vector<double> meanSums, meanWeights, covSums, covWeights, entryWeights;
};
int fetch(gmm_estimator* e, double* meanSums, double* meanWeights, double* covSums, double* covWeights, double* entryWeights) {
    GMM_HIP_CHECK(hipSetDevice(e->device));
    const int rc = waitDone(e);
    if (rc != GMM_OK)
        return rc;
    const size_t D = e->D;
    const struct {
        double*       dst;
        const double* src;
        size_t        n;
    } copies[5] = {{meanSums, e->dMeanSums.get(), e->nMeans * D},    {meanWeights, e->dMeanWeights.get(), e->nMeans},
                   {covSums, e->dCovSums.get(), e->nCovs * D},       {covWeights, e->dCovWeights.get(), e->nCovs},
                   {entryWeights, e->dEntryWeights.get(), e->nEntries}};
    for (const auto& c : copies)
        if (c.dst && c.n)
            GMM_HIP_CHECK(hipMemcpy(c.dst, c.src, c.n * sizeof(double), hipMemcpyDeviceToHost));
    return GMM_OK;
}

// the denominator tables; zeros for a handle that has seen no discriminative call (they are not allocated then)
int fetchDenominator(gmm_estimator* e, double* meanSums, double* meanWeights, double* covSums, double* covWeights,
                     double* entryWeights) {
    GMM_HIP_CHECK(hipSetDevice(e->device));
    const int rc = waitDone(e);
    if (rc != GMM_OK)
        return rc;
    const size_t D = e->D;
    const struct {
        double*       dst;
        const double* src;
        size_t        n;
    } copies[5] = {{meanSums, e->dDenMeanSums.get(), e->nMeans * D}, {meanWeights, e->dDenMeanWeights.get(), e->nMeans},
                   {covSums, e->dDenCovSums.get(), e->nCovs * D},    {covWeights, e->dDenCovWeights.get(), e->nCovs},
                   {entryWeights, e->dDenEntryWeights.get(), e->nEntries}};
    for (const auto& c : copies)
        if (c.dst && c.n) {
            if (e->denominatorTables)
                GMM_HIP_CHECK(hipMemcpy(c.dst, c.src, c.n * sizeof(double), hipMemcpyDeviceToHost));
            else
                std::fill(c.dst, c.dst + c.n, 0.0);
        }
    return GMM_OK;
}

int serialize(gmm_estimator* e, std::vector<unsigned char>& bytes, bool discriminative = false) {
    HostTables h;
    h.meanSums.resize(static_cast<size_t>(e->nMeans) * e->D);
    h.meanWeights.resize(e->nMeans);
    h.covSums.resize(static_cast<size_t>(e->nCovs) * e->D);
    h.covWeights.resize(e->nCovs);
    h.entryWeights.resize(e->nEntries);
    const int rc = fetch(e, h.meanSums.data(), h.meanWeights.data(), h.covSums.data(), h.covWeights.data(), h.entryWeights.data());
    if (rc != GMM_OK)
        return rc;
    EstimatorTables t{};
    t.D            = e->D;
    t.nMeans       = e->nMeans;
    t.nCovs        = e->nCovs;
    t.nDens        = e->nDens;
    t.nMix         = e->nMix;
    t.dnsMean      = e->dnsMean.data();
    t.dnsCov       = e->dnsCov.data();
    t.mixOff       = e->mixOff.data();
    t.mixDens      = e->mixDens.data();
    t.meanSums     = h.meanSums.data();
    t.meanWeights  = h.meanWeights.data();
    t.covSums      = h.covSums.data();
    t.covWeights   = h.covWeights.data();
    t.entryWeights = h.entryWeights.data();
    if (!discriminative) {
        bytes = writeEstimatorFile(t);
        return GMM_OK;
    }
    HostTables d;
    d.meanSums.resize(h.meanSums.size());
    d.meanWeights.resize(h.meanWeights.size());
    d.covSums.resize(h.covSums.size());
    d.covWeights.resize(h.covWeights.size());
    d.entryWeights.resize(h.entryWeights.size());
    const int rd = fetchDenominator(e, d.meanSums.data(), d.meanWeights.data(), d.covSums.data(), d.covWeights.data(),
                                    d.entryWeights.data());
    if (rd != GMM_OK)
        return rd;
    DenominatorTables den{};
    den.meanSums     = d.meanSums.data();
    den.meanWeights  = d.meanWeights.data();
    den.covSums      = d.covSums.data();
    den.covWeights   = d.covWeights.data();
    den.entryWeights = d.entryWeights.data();
    den.objective    = e->objective;
    bytes            = writeDiscriminativeEstimatorFile(t, den);
    return GMM_OK;
}

int copyBytesOut(const std::vector<unsigned char>& bytes, void* data, uint64_t capacity, uint64_t* size) {
    *size = bytes.size();
    if (!data)
        return GMM_OK;
    if (capacity < bytes.size())
        return fail(GMM_ERR_CAPACITY, "estimator file of " + std::to_string(bytes.size()) + " bytes, capacity " +
                                              std::to_string(capacity));
    std::memcpy(data, bytes.data(), bytes.size());
    return GMM_OK;
}

int writeBytes(const std::vector<unsigned char>& bytes, const char* filename) {
    std::FILE* f = std::fopen(filename, "wb");
    if (!f)
        return fail(GMM_ERR_INVALID_ARGUMENT, std::string("estimator file: cannot open \"") + filename + "\" for writing");
    const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (std::fclose(f) != 0 || !ok)
        return fail(GMM_ERR_INVALID_ARGUMENT, std::string("estimator file: error writing \"") + filename + "\"");
    return GMM_OK;
}

}  // namespace

extern "C" {

int gmm_estimator_create(const gmm_mixture_set* ms, uint32_t maxPairs, int device, gmm_estimator** out) {
    if (!ms || !out || !ms->mixture_offsets || (ms->n_densities && (!ms->density_mean || !ms->density_covariance)))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (ms->mixture_offsets[ms->n_mixtures] && !ms->mixture_densities)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    std::unique_ptr<gmm_estimator> e(new (std::nothrow) gmm_estimator);
    if (!e)
        return fail(GMM_ERR_OUT_OF_MEMORY, "out of host memory");
    const int rc = create(e.get(), *ms, maxPairs, device);
    if (rc != GMM_OK)
        return rc;
    *out = e.release();
    return GMM_OK;
}

int gmm_estimator_destroy(gmm_estimator* e) {
    if (!e)
        return GMM_OK;
    (void)hipSetDevice(e->device);
    if (e->pending)
        (void)hipEventSynchronize(e->done.get());  // no kernel of a call may outlive its scratch
    delete e;
    return GMM_OK;
}

int gmm_estimator_reset(gmm_estimator* e) {
    if (!e)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null estimator");
    GMM_HIP_CHECK(hipSetDevice(e->device));
    const int rc = waitDone(e);
    return rc != GMM_OK ? rc : zeroTables(e);
}

int gmm_estimator_accumulate_device(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                    uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                    const uint32_t* pairDensity, const double* pairWeight, uint32_t nPairs, void* stream) {
    int rc = checkCall(e, scorer, frames, frameStride, pairFrame, pairMix, pairDensity, nPairs);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(e->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc             = accumulateOn(e, scorer, frames, nFrames, frameStride, pairFrame, pairMix, pairDensity, pairWeight, nPairs, st);
    // recorded even after a failed launch: what was enqueued before it still uses the scratch
    GMM_HIP_CHECK(hipEventRecord(e->done.get(), st));
    e->pending = true;
    return rc;
}

int gmm_estimator_accumulate_host(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                  uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                  const uint32_t* pairDensity, const double* pairWeight, uint32_t nPairs) {
    int rc = checkCall(e, scorer, frames, frameStride, pairFrame, pairMix, pairDensity, nPairs);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(e->device));
    if ((rc = waitDone(e)) != GMM_OK)
        return rc;
    // the frames, dense (row length D); the pair lists into the handle's staging
    DeviceBuffer<float> dFrames;
    const size_t        D = e->D;
    GMM_HIP_CHECK(dFrames.alloc(std::max<size_t>(static_cast<size_t>(nFrames) * D, 1)));
    if (nFrames && D)
        GMM_HIP_CHECK(hipMemcpy2D(dFrames.get(), D * sizeof(float), frames, static_cast<size_t>(frameStride) * sizeof(float),
                                  D * sizeof(float), nFrames, hipMemcpyHostToDevice));
    const size_t n = nPairs;
    GMM_HIP_CHECK(hipMemcpy(e->dPairFrame.get(), pairFrame, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(e->dPairMix.get(), pairMix, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (pairDensity)
        GMM_HIP_CHECK(hipMemcpy(e->dPairDensity.get(), pairDensity, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (pairWeight)
        GMM_HIP_CHECK(hipMemcpy(e->dPairWeight.get(), pairWeight, n * sizeof(double), hipMemcpyHostToDevice));
    rc = accumulateOn(e, scorer, dFrames.get(), nFrames, e->D, e->dPairFrame.get(), e->dPairMix.get(),
                      pairDensity ? e->dPairDensity.get() : nullptr, pairWeight ? e->dPairWeight.get() : nullptr, nPairs,
                      nullptr);
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // before dFrames is released
    return rc;
}

int gmm_estimator_accumulate_posteriors_device(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                               uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                               const double* pairWeight, uint32_t nPairs, double threshold, void* stream) {
    int rc = checkPosteriorCall(e, scorer, frames, frameStride, pairFrame, pairMix, nPairs);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(e->device));
    if ((rc = ensurePosteriorScratch(e)) != GMM_OK)
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc             = accumulatePosteriorsOn(e, scorer, frames, nFrames, frameStride, pairFrame, pairMix, pairWeight, nPairs, threshold, st);
    GMM_HIP_CHECK(hipEventRecord(e->done.get(), st));
    e->pending = true;
    return rc;
}

int gmm_estimator_accumulate_posteriors_host(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                             uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                             const double* pairWeight, uint32_t nPairs, double threshold) {
    int rc = checkPosteriorCall(e, scorer, frames, frameStride, pairFrame, pairMix, nPairs);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(e->device));
    if ((rc = waitDone(e)) != GMM_OK || (rc = ensurePosteriorScratch(e)) != GMM_OK)
        return rc;
    DeviceBuffer<float> dFrames;
    const size_t        D = e->D, n = nPairs;
    GMM_HIP_CHECK(dFrames.alloc(std::max<size_t>(static_cast<size_t>(nFrames) * D, 1)));
    if (nFrames && D)
        GMM_HIP_CHECK(hipMemcpy2D(dFrames.get(), D * sizeof(float), frames, static_cast<size_t>(frameStride) * sizeof(float),
                                  D * sizeof(float), nFrames, hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(e->dPairFrame.get(), pairFrame, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(e->dPairMix.get(), pairMix, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (pairWeight)
        GMM_HIP_CHECK(hipMemcpy(e->dPairWeight.get(), pairWeight, n * sizeof(double), hipMemcpyHostToDevice));
    rc = accumulatePosteriorsOn(e, scorer, dFrames.get(), nFrames, e->D, e->dPairFrame.get(), e->dPairMix.get(),
                                pairWeight ? e->dPairWeight.get() : nullptr, nPairs, threshold, nullptr);
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // before dFrames is released
    return rc;
}

int gmm_estimator_accumulate_discriminative_device(gmm_estimator* e, gmm_scorer* scorer, const float* frames,
                                                   uint32_t nFrames, uint32_t frameStride, const uint32_t* pairFrame,
                                                   const uint32_t* pairMix, const uint32_t* pairDensity,
                                                   const double* weightNum, const double* weightDen, uint32_t nPairs,
                                                   void* stream) {
    int rc = checkCall(e, scorer, frames, frameStride, pairFrame, pairMix, pairDensity, nPairs);
    if (rc == GMM_OK)
        rc = checkSides(weightNum, weightDen);
    if (rc != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(e->device));
    if ((rc = ensureDenominatorTables(e)) != GMM_OK || nPairs == 0)
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = accumulateDiscriminativeOn(e, scorer, frames, nFrames, frameStride, pairFrame, pairMix, pairDensity, weightNum,
                                    weightDen, nPairs, st);
    GMM_HIP_CHECK(hipEventRecord(e->done.get(), st));
    e->pending = true;
    return rc;
}

int gmm_estimator_accumulate_discriminative_host(gmm_estimator* e, gmm_scorer* scorer, const float* frames,
                                                 uint32_t nFrames, uint32_t frameStride, const uint32_t* pairFrame,
                                                 const uint32_t* pairMix, const uint32_t* pairDensity,
                                                 const double* weightNum, const double* weightDen, uint32_t nPairs) {
    int rc = checkCall(e, scorer, frames, frameStride, pairFrame, pairMix, pairDensity, nPairs);
    if (rc == GMM_OK)
        rc = checkSides(weightNum, weightDen);
    if (rc != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(e->device));
    if ((rc = waitDone(e)) != GMM_OK || (rc = ensureDenominatorTables(e)) != GMM_OK || nPairs == 0)
        return rc;
    DeviceBuffer<float> dFrames;
    const size_t        D = e->D, n = nPairs;
    GMM_HIP_CHECK(dFrames.alloc(std::max<size_t>(static_cast<size_t>(nFrames) * D, 1)));
    if (nFrames && D)
        GMM_HIP_CHECK(hipMemcpy2D(dFrames.get(), D * sizeof(float), frames, static_cast<size_t>(frameStride) * sizeof(float),
                                  D * sizeof(float), nFrames, hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(e->dPairFrame.get(), pairFrame, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(e->dPairMix.get(), pairMix, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (pairDensity)
        GMM_HIP_CHECK(hipMemcpy(e->dPairDensity.get(), pairDensity, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (weightNum)
        GMM_HIP_CHECK(hipMemcpy(e->dPairWeight.get(), weightNum, n * sizeof(double), hipMemcpyHostToDevice));
    if (weightDen)
        GMM_HIP_CHECK(hipMemcpy(e->dPairWeightDen.get(), weightDen, n * sizeof(double), hipMemcpyHostToDevice));
    rc = accumulateDiscriminativeOn(e, scorer, dFrames.get(), nFrames, e->D, e->dPairFrame.get(), e->dPairMix.get(),
                                    pairDensity ? e->dPairDensity.get() : nullptr, weightNum ? e->dPairWeight.get() : nullptr,
                                    weightDen ? e->dPairWeightDen.get() : nullptr, nPairs, nullptr);
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // before dFrames is released
    return rc;
}

int gmm_estimator_accumulate_discriminative_posteriors_device(gmm_estimator* e, gmm_scorer* scorer, const float* frames,
                                                              uint32_t nFrames, uint32_t frameStride,
                                                              const uint32_t* pairFrame, const uint32_t* pairMix,
                                                              const double* weightNum, const double* weightDen,
                                                              uint32_t nPairs, double threshold, void* stream) {
    int rc = checkPosteriorCall(e, scorer, frames, frameStride, pairFrame, pairMix, nPairs);
    if (rc == GMM_OK)
        rc = checkSides(weightNum, weightDen);
    if (rc != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(e->device));
    if ((rc = ensureDenominatorTables(e)) != GMM_OK || nPairs == 0)
        return rc;
    if ((rc = ensurePosteriorScratch(e)) != GMM_OK || (rc = ensureDenominatorPosteriorScratch(e)) != GMM_OK)
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = accumulateDiscriminativePosteriorsOn(e, scorer, frames, nFrames, frameStride, pairFrame, pairMix, weightNum,
                                              weightDen, nPairs, threshold, st);
    GMM_HIP_CHECK(hipEventRecord(e->done.get(), st));
    e->pending = true;
    return rc;
}

int gmm_estimator_accumulate_discriminative_posteriors_host(gmm_estimator* e, gmm_scorer* scorer, const float* frames,
                                                            uint32_t nFrames, uint32_t frameStride,
                                                            const uint32_t* pairFrame, const uint32_t* pairMix,
                                                            const double* weightNum, const double* weightDen,
                                                            uint32_t nPairs, double threshold) {
    int rc = checkPosteriorCall(e, scorer, frames, frameStride, pairFrame, pairMix, nPairs);
    if (rc == GMM_OK)
        rc = checkSides(weightNum, weightDen);
    if (rc != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(e->device));
    if ((rc = waitDone(e)) != GMM_OK || (rc = ensureDenominatorTables(e)) != GMM_OK || nPairs == 0)
        return rc;
    if ((rc = ensurePosteriorScratch(e)) != GMM_OK || (rc = ensureDenominatorPosteriorScratch(e)) != GMM_OK)
        return rc;
    DeviceBuffer<float> dFrames;
    const size_t        D = e->D, n = nPairs;
    GMM_HIP_CHECK(dFrames.alloc(std::max<size_t>(static_cast<size_t>(nFrames) * D, 1)));
    if (nFrames && D)
        GMM_HIP_CHECK(hipMemcpy2D(dFrames.get(), D * sizeof(float), frames, static_cast<size_t>(frameStride) * sizeof(float),
                                  D * sizeof(float), nFrames, hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(e->dPairFrame.get(), pairFrame, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(e->dPairMix.get(), pairMix, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (weightNum)
        GMM_HIP_CHECK(hipMemcpy(e->dPairWeight.get(), weightNum, n * sizeof(double), hipMemcpyHostToDevice));
    if (weightDen)
        GMM_HIP_CHECK(hipMemcpy(e->dPairWeightDen.get(), weightDen, n * sizeof(double), hipMemcpyHostToDevice));
    rc = accumulateDiscriminativePosteriorsOn(e, scorer, dFrames.get(), nFrames, e->D, e->dPairFrame.get(), e->dPairMix.get(),
                                              weightNum ? e->dPairWeight.get() : nullptr,
                                              weightDen ? e->dPairWeightDen.get() : nullptr, nPairs, threshold, nullptr);
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // before dFrames is released
    return rc;
}

int gmm_estimator_accumulate_objective(gmm_estimator* e, double f) {
    if (!e)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null estimator");
    e->objective += f;  // objectiveFunction_ += (Sum) f
    return GMM_OK;
}

int gmm_estimator_objective(gmm_estimator* e, double* objective) {
    if (!e || !objective)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    *objective = e->objective;
    return GMM_OK;
}

int gmm_estimator_get_denominator(gmm_estimator* e, double* meanSums, double* meanWeights, double* covSums,
                                  double* covWeights, double* entryWeights) {
    if (!e)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null estimator");
    return fetchDenominator(e, meanSums, meanWeights, covSums, covWeights, entryWeights);
}

int gmm_estimator_serialize_discriminative(gmm_estimator* e, void* data, uint64_t capacity, uint64_t* size) {
    if (!e || !size)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<unsigned char> bytes;
    const int                  rc = serialize(e, bytes, true);
    return rc != GMM_OK ? rc : copyBytesOut(bytes, data, capacity, size);
}

int gmm_estimator_write_discriminative(gmm_estimator* e, const char* filename) {
    if (!e || !filename)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<unsigned char> bytes;
    const int                  rc = serialize(e, bytes, true);
    return rc != GMM_OK ? rc : writeBytes(bytes, filename);
}

int gmm_estimator_estimate_ebw_handle(gmm_estimator* e, const gmm_mixture_set* previous, const gmm_ebw_config* config,
                                      gmm_mixture_set* out) {
    if (!e || !out)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<unsigned char> bytes;
    const int                  rc = serialize(e, bytes, true);
    return rc != GMM_OK ? rc : gmm_estimator_estimate_ebw(bytes.data(), bytes.size(), previous, config, out);
}

int gmm_estimator_skipped(gmm_estimator* e, uint64_t* skipped) {
    if (!e || !skipped)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    GMM_HIP_CHECK(hipSetDevice(e->device));
    const int rc = waitDone(e);
    if (rc != GMM_OK)
        return rc;
    unsigned long long v = 0;
    GMM_HIP_CHECK(hipMemcpy(&v, e->dSkipped.get(), sizeof(v), hipMemcpyDeviceToHost));
    *skipped = v;
    return GMM_OK;
}

int gmm_estimator_get(gmm_estimator* e, double* meanSums, double* meanWeights, double* covSums, double* covWeights,
                      double* entryWeights) {
    if (!e)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null estimator");
    return fetch(e, meanSums, meanWeights, covSums, covWeights, entryWeights);
}

int gmm_estimator_serialize(gmm_estimator* e, void* data, uint64_t capacity, uint64_t* size) {
    if (!e || !size)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<unsigned char> bytes;
    const int                  rc = serialize(e, bytes);
    if (rc != GMM_OK)
        return rc;
    return copyBytesOut(bytes, data, capacity, size);
}

int gmm_estimator_write(gmm_estimator* e, const char* filename) {
    if (!e || !filename)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<unsigned char> bytes;
    const int                  rc = serialize(e, bytes);
    if (rc != GMM_OK)
        return rc;
    return writeBytes(bytes, filename);
}

int gmm_estimator_estimate(gmm_estimator* e, const gmm_estimator_config* config, gmm_mixture_set* out) {
    if (!e || !out)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<unsigned char> bytes;
    const int                  rc = serialize(e, bytes);
    if (rc != GMM_OK)
        return rc;
    return gmm_mixture_set_estimate(bytes.data(), bytes.size(), config, out);
}

}  // extern "C"
