// gmm_estimator.cc -- the handle behind include/rasr_gmm_estimator.h: the f64 tables on the device, the three inverted
// indexes of a call (gmm_kernels_accum.hip), the posterior and the discriminative paths, get / serialize / write /
// estimate.  What a handle that accumulates pairs shares with the others is gmm_pairaccum.hh's.
// The file format (serialize, combine) is host/MixtureSetEstimatorFile.cc.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

#include "gmm_pairaccum.hh"

namespace rasr_gmm {

// the sizes of one set of tables
struct TableShape {
    size_t nMeans, nCovs, nEntries, D, slabSlots;
};

// one set of the f64 accumulators with the later pieces' slab of a call.  The handle holds two: the tables of the
// maximum-likelihood calls, which are the numerator's, and the denominator's
struct TableSet {
    DeviceBuffer<double> meanSums, meanWeights, covSums, covWeights, entryWeights, slabSums, slabWeights;
    bool                 allocated = false;  // and zeroed: set by the handle

    int alloc(const TableShape& n) {
        GMM_HIP_CHECK(meanSums.alloc(n.nMeans * n.D));
        GMM_HIP_CHECK(meanWeights.alloc(n.nMeans));
        GMM_HIP_CHECK(covSums.alloc(n.nCovs * n.D));
        GMM_HIP_CHECK(covWeights.alloc(n.nCovs));
        GMM_HIP_CHECK(entryWeights.alloc(n.nEntries));
        GMM_HIP_CHECK(slabSums.alloc(n.slabSlots * n.D));
        GMM_HIP_CHECK(slabWeights.alloc(n.slabSlots));
        return GMM_OK;
    }
    // enqueued on the null stream
    int zero(const TableShape& n) {
        if (n.nMeans) {
            GMM_HIP_CHECK(hipMemset(meanSums.get(), 0, n.nMeans * n.D * sizeof(double)));
            GMM_HIP_CHECK(hipMemset(meanWeights.get(), 0, n.nMeans * sizeof(double)));
        }
        if (n.nCovs) {
            GMM_HIP_CHECK(hipMemset(covSums.get(), 0, n.nCovs * n.D * sizeof(double)));
            GMM_HIP_CHECK(hipMemset(covWeights.get(), 0, n.nCovs * sizeof(double)));
        }
        if (n.nEntries)
            GMM_HIP_CHECK(hipMemset(entryWeights.get(), 0, n.nEntries * sizeof(double)));
        return GMM_OK;
    }
    // host copies of the tables a destination is given for; zeros from a set that was never allocated
    int fetch(const TableShape& n, double* hMeanSums, double* hMeanWeights, double* hCovSums, double* hCovWeights,
              double* hEntryWeights) const {
        const struct {
            double*       dst;
            const double* src;
            size_t        n;
        } copies[5] = {{hMeanSums, meanSums.get(), n.nMeans * n.D},
                       {hMeanWeights, meanWeights.get(), n.nMeans},
                       {hCovSums, covSums.get(), n.nCovs * n.D},
                       {hCovWeights, covWeights.get(), n.nCovs},
                       {hEntryWeights, entryWeights.get(), n.nEntries}};
        for (const auto& c : copies)
            if (c.dst && c.n) {
                if (allocated)
                    GMM_HIP_CHECK(hipMemcpy(c.dst, c.src, c.n * sizeof(double), hipMemcpyDeviceToHost));
                else
                    std::fill(c.dst, c.dst + c.n, 0.0);
            }
        return GMM_OK;
    }
};

}  // namespace rasr_gmm

using namespace rasr_gmm;

struct gmm_estimator {
    PairAccumCore core;
    uint32_t      nMeans = 0, nCovs = 0, nDens = 0;
    // the topology's index tables on the host (serialize)
    std::vector<uint32_t> dnsMean, dnsCov, mixOff, mixDens;
    // the accumulators: side[0] from create; side[1], the denominator's, and the host call's second weight list
    // (core.dPairWeightDen) are allocated and zeroed by the handle's first discriminative call
    TableSet side[2];
    // scratch of one call of up to maxPairs pairs: the three keys of a pair
    DeviceBuffer<uint32_t> dKeyMean, dKeyCov, dKeyEntry;
    // Baum-Welch calls: the posterior rows and the contributions' frames and weights, maxPairs elements each,
    // allocated by the handle's first posterior call; the second weight list by its first joint posterior call
    uint32_t               maxEntries = 1;  // K_max: the largest entry count of a mixture (at least 1)
    bool                   posteriorScratch = false;
    DeviceBuffer<float>    dPostRows;
    DeviceBuffer<uint32_t> dContribFrame;
    DeviceBuffer<double>   dContribWeight[2];
    double                 objective = 0.0;  // objectiveFunction_ (host)

    TableShape shape() const { return {nMeans, nCovs, core.nEntries, core.D, accumSlabSlots(core.maxPairs)}; }
};

namespace {

constexpr PairNouns kNouns{"estimator", "topology", "estimator topology"};

// both sides, the skipped count and the objective function
int zeroTables(gmm_estimator* e) {
    for (TableSet& t : e->side)
        if (t.allocated) {
            const int rc = t.zero(e->shape());
            if (rc != GMM_OK)
                return rc;
        }
    GMM_HIP_CHECK(hipMemset(e->core.dSkipped.get(), 0, sizeof(unsigned long long)));
    e->objective = 0.0;
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // done before a call on any other stream
    return GMM_OK;
}

int create(gmm_estimator* e, const gmm_mixture_set& ms, uint32_t maxPairs, int device) {
    PairAccumCore& c = e->core;
    PairTopology   topo;
    int            rc = initCore(c, kNouns, ms, maxPairs, device, topo);
    if (rc != GMM_OK)
        return rc;
    e->nMeans     = ms.n_means;
    e->nCovs      = ms.n_covariances;
    e->nDens      = ms.n_densities;
    e->maxEntries = topo.maxEntries;
    e->mixOff     = topo.mixOff;
    if (e->nDens)
        e->dnsMean.assign(ms.density_mean, ms.density_mean + e->nDens);
    if (e->nDens)
        e->dnsCov.assign(ms.density_covariance, ms.density_covariance + e->nDens);
    if (c.nEntries)
        e->mixDens.assign(ms.mixture_densities, ms.mixture_densities + c.nEntries);

    GMM_HIP_CHECK(hipSetDevice(device));
    // the sorts' temporary storage: the largest of the three key ranges at max_pairs
    for (uint32_t nDest : {e->nMeans, e->nCovs, c.nEntries}) {
        size_t bytes = 0;
        if (maxPairs)
            GMM_HIP_CHECK(static_cast<hipError_t>(accumSortTempBytes(maxPairs, keyBits(nDest), &bytes)));
        c.sortTempBytes = std::max(c.sortTempBytes, bytes);
    }
    if ((rc = allocCore(c, topo, false)) != GMM_OK)
        return rc;
    for (DeviceBuffer<uint32_t>* b : {&e->dKeyMean, &e->dKeyCov, &e->dKeyEntry})
        GMM_HIP_CHECK(b->alloc(maxPairs));
    if ((rc = e->side[0].alloc(e->shape())) != GMM_OK)
        return rc;
    e->side[0].allocated = true;
    return zeroTables(e);
}

// the three inverted indexes of a call whose keys are written (dKeyMean / dKeyCov / dKeyEntry, dPairIndex = 0, 1, ...):
// per index the stable sort, the ordered sums of the pieces, the pieces' combination, for one side (the tables of
// side[0]) or two.  n contributions; pairFrame and the weight lists are indexed by contribution (gmm_estimator.hh says
// what NULL and NaN mean for either side count)
int accumulateKeyed(gmm_estimator* e, const float* frames, uint32_t frameStride, const uint32_t* pairFrame,
                    const double* const (&weight)[2], uint32_t sides, uint32_t nPairs, hipStream_t stream) {
    AccumArgs a{};
    a.keysSorted  = e->core.dKeysSorted.get();
    a.indexSorted = e->core.dIndexSorted.get();
    a.pairFrame   = pairFrame;
    a.frames      = frames;
    a.nPairs      = nPairs;
    a.D           = e->core.D;
    a.frameStride = frameStride;
    a.sides       = sides;
    for (uint32_t s = 0; s < sides; ++s) {
        a.weight[s]      = weight[s];
        a.slabSums[s]    = e->side[s].slabSums.get();
        a.slabWeights[s] = e->side[s].slabWeights.get();
    }
    struct Index {
        const uint32_t*      keys;
        uint32_t             nDest;
        DeviceBuffer<double> TableSet::*sums, TableSet::*weights;
        int                  mode;
    };
    const Index indexes[3] = {{e->dKeyMean.get(), e->nMeans, &TableSet::meanSums, &TableSet::meanWeights, kAccumSum},
                              {e->dKeyCov.get(), e->nCovs, &TableSet::covSums, &TableSet::covWeights, kAccumSquare},
                              {e->dKeyEntry.get(), e->core.nEntries, nullptr, &TableSet::entryWeights, kAccumWeightOnly}};
    for (const Index& x : indexes) {
        if (x.nDest == 0)
            continue;
        GMM_HIP_CHECK(static_cast<hipError_t>(launchAccumSort(e->core.dSortTemp.get(), e->core.sortTempBytes, x.keys, e->core.dPairIndex.get(),
                                                             e->core.dKeysSorted.get(), e->core.dIndexSorted.get(), nPairs,
                                                             keyBits(x.nDest), stream)));
        a.nDest = x.nDest;
        a.mode  = x.mode;
        for (uint32_t s = 0; s < sides; ++s) {
            a.sums[s]    = x.sums ? (e->side[s].*x.sums).get() : nullptr;
            a.weights[s] = (e->side[s].*x.weights).get();
        }
        GMM_HIP_CHECK(static_cast<hipError_t>(launchAccumulateSegments(a, stream)));
        GMM_HIP_CHECK(static_cast<hipError_t>(launchCombinePieces(a, stream)));
    }
    return GMM_OK;
}

// the Viterbi call, one side (weight) or two (weight, weightDen): the best densities where the scorer gives them, a
// pair -> the keys of its mean, covariance and mixture entry, then the keyed tail
int accumulateOn(gmm_estimator* e, gmm_scorer* scorer, PairCall call, uint32_t sides, hipStream_t stream) {
    const int rc = bestDensities(e->core, scorer, call, stream);  // the Viterbi branch
    if (rc != GMM_OK)
        return rc;
    const double* const weight[2] = {call.weight, call.weightDen};
    ResolveArgs         r{};
    r.pairFrame   = call.pairFrame;
    r.pairMix     = call.pairMix;
    r.pairDensity = call.pairDensity;
    r.weight[0]   = weight[0];
    r.weight[1]   = weight[1];
    r.mixOff      = e->core.dMixOff.get();
    r.entryMean   = e->core.dEntryMean.get();
    r.entryCov    = e->core.dEntryCov.get();
    r.keyMean     = e->dKeyMean.get();
    r.keyCov      = e->dKeyCov.get();
    r.keyEntry    = e->dKeyEntry.get();
    r.pairIndex   = e->core.dPairIndex.get();
    r.skipped     = e->core.dSkipped.get();
    r.nPairs      = call.nPairs;
    r.nFrames     = call.nFrames;
    r.nMix        = e->core.nMix;
    r.nMeans      = e->nMeans;
    r.nCovs       = e->nCovs;
    r.nEntries    = e->core.nEntries;
    r.sides       = sides;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchResolvePairs(r, stream)));
    return accumulateKeyed(e, call.frames, call.frameStride, call.pairFrame, weight, sides, call.nPairs, stream);
}

// the checks of a posterior call that need no device: checkPairCall's, diagonal-sum only, contribution slots
int checkPosteriorCall(const gmm_estimator* e, const gmm_scorer* scorer, const PairCall& call) {
    if (!e)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null estimator");
    // n_pairs <= n_pairs * K_max: checkPairCall's own capacity check cannot fire before this one
    const uint32_t nPairs = call.nPairs;
    const uint64_t slots  = static_cast<uint64_t>(nPairs) * (scorer ? e->maxEntries : 1u);
    if (slots > e->core.maxPairs)
        return fail(GMM_ERR_CAPACITY, std::to_string(nPairs) + " pairs of up to " + std::to_string(scorer ? e->maxEntries : 1u) +
                                              " densities exceed the estimator's max_pairs " + std::to_string(e->core.maxPairs) +
                                              " (contribution slots for this call)");
    int rc = checkPairCall(&e->core, kNouns, scorer, call);
    if (rc == GMM_OK && scorer)
        rc = checkPosteriors(scorer);
    return rc;
}

// the posterior scratch, on the handle's first posterior call
int ensurePosteriorScratch(gmm_estimator* e) {
    if (e->posteriorScratch)
        return GMM_OK;
    GMM_HIP_CHECK(e->dPostRows.alloc(e->core.maxPairs));
    GMM_HIP_CHECK(e->dContribFrame.alloc(e->core.maxPairs));
    GMM_HIP_CHECK(e->dContribWeight[0].alloc(e->core.maxPairs));
    e->posteriorScratch = true;
    return GMM_OK;
}

// the Baum-Welch call: posteriors and expansion into contribution slots (one kernel), then the keyed tail over them
int accumulatePosteriorsOn(gmm_estimator* e, gmm_scorer* scorer, const PairCall& call, double threshold,
                           hipStream_t stream) {
    PosteriorArgs q{};
    if (scorer)
        q.pair = pairArgsOf(scorer, call.frames, call.nFrames, call.frameStride);
    else {
        q.pair.nFrames   = call.nFrames;
        q.pair.nMixtures = e->core.nMix;
        q.pair.mixOff    = e->core.dMixOff.get();
    }
    q.pair.pairFrame = call.pairFrame;
    q.pair.pairMix   = call.pairMix;
    q.pair.nPairs    = call.nPairs;
    q.posteriors     = e->dPostRows.get();
    q.rowStride      = scorer ? e->maxEntries : 1u;
    q.pairWeight     = call.weight;
    q.threshold      = threshold;
    q.entryMean      = e->core.dEntryMean.get();
    q.entryCov       = e->core.dEntryCov.get();
    q.keyMean        = e->dKeyMean.get();
    q.keyCov         = e->dKeyCov.get();
    q.keyEntry       = e->dKeyEntry.get();
    q.contribIndex   = e->core.dPairIndex.get();
    q.contribFrame   = e->dContribFrame.get();
    q.contribWeight  = e->dContribWeight[0].get();
    q.skipped        = e->core.dSkipped.get();
    q.nMeans         = e->nMeans;
    q.nCovs          = e->nCovs;
    q.nEntries       = e->core.nEntries;
    GMM_HIP_CHECK(scorer ? launchDensityPosteriors(q, stream) : launchExpandSingleDensity(q, stream));
    return accumulateKeyed(e, call.frames, call.frameStride, e->dContribFrame.get(), {e->dContribWeight[0].get(), nullptr},
                           1, call.nPairs * q.rowStride, stream);
}

// the denominator tables with their slab and the host call's second weight list, on the handle's first discriminative
// call
int ensureDenominatorTables(gmm_estimator* e) {
    TableSet& den = e->side[1];
    if (den.allocated)
        return GMM_OK;
    int rc = den.alloc(e->shape());
    if (rc != GMM_OK)
        return rc;
    GMM_HIP_CHECK(e->core.dPairWeightDen.alloc(e->core.maxPairs));
    if ((rc = den.zero(e->shape())) != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // done before the call on any other stream
    den.allocated = true;
    return GMM_OK;
}

// the joint Baum-Welch call: the posterior rows once (the kernel of gmm_density_posteriors_pairs_device), their
// expansion into contribution slots with one finalWeight per side, then the keyed tail for two sides
int accumulateDiscriminativePosteriorsOn(gmm_estimator* e, gmm_scorer* scorer, const PairCall& call,
                                         double threshold, hipStream_t stream) {
    const uint32_t rowStride = scorer ? e->maxEntries : 1u;
    if (scorer) {
        PosteriorArgs q{};
        q.pair           = pairArgsOf(scorer, call.frames, call.nFrames, call.frameStride);
        q.pair.pairFrame = call.pairFrame;
        q.pair.pairMix   = call.pairMix;
        q.pair.nPairs    = call.nPairs;
        q.posteriors     = e->dPostRows.get();
        q.rowStride      = rowStride;
        GMM_HIP_CHECK(launchDensityPosteriors(q, stream));
    }
    ExpandArgs x{};
    x.pairFrame        = call.pairFrame;
    x.pairMix          = call.pairMix;
    x.weight[0]        = call.weight;
    x.weight[1]        = call.weightDen;
    x.posteriors       = scorer ? e->dPostRows.get() : nullptr;
    x.mixOff           = e->core.dMixOff.get();
    x.entryMean        = e->core.dEntryMean.get();
    x.entryCov         = e->core.dEntryCov.get();
    x.keyMean          = e->dKeyMean.get();
    x.keyCov           = e->dKeyCov.get();
    x.keyEntry         = e->dKeyEntry.get();
    x.contribIndex     = e->core.dPairIndex.get();
    x.contribFrame     = e->dContribFrame.get();
    x.contribWeight[0] = e->dContribWeight[0].get();
    x.contribWeight[1] = e->dContribWeight[1].get();
    x.skipped          = e->core.dSkipped.get();
    x.threshold        = threshold;
    x.nPairs           = call.nPairs;
    x.rowStride        = rowStride;
    x.nFrames          = call.nFrames;
    x.nMix             = e->core.nMix;
    x.nMeans           = e->nMeans;
    x.nCovs            = e->nCovs;
    x.nEntries         = e->core.nEntries;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchExpandPosteriorRows(x, stream)));
    return accumulateKeyed(e, call.frames, call.frameStride, e->dContribFrame.get(),
                           {call.weight ? e->dContribWeight[0].get() : nullptr,
                            call.weightDen ? e->dContribWeight[1].get() : nullptr},
                           2, call.nPairs * rowStride, stream);
}

// what a joint Baum-Welch call needs: the denominator tables even for a call of no pairs, the scratch for one with pairs
int ensureDiscriminativePosteriors(gmm_estimator* e, uint32_t nPairs) {
    int rc = ensureDenominatorTables(e);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    if ((rc = ensurePosteriorScratch(e)) != GMM_OK)
        return rc;
    if (!e->dContribWeight[1].get())
        GMM_HIP_CHECK(e->dContribWeight[1].alloc(e->core.maxPairs));
    return GMM_OK;
}

// the check of a discriminative call that needs no device
int checkSides(const double* weightNum, const double* weightDen) {
    if (!weightNum && !weightDen)
        return fail(GMM_ERR_INVALID_ARGUMENT, "pair_weight_num and pair_weight_den are both NULL: the call has no side to add to");
    return GMM_OK;
}

// host copies of a side's tables, after the last call
struct HostTables {
    std::vector<double> meanSums, meanWeights, covSums, covWeights, entryWeights;
    explicit HostTables(const TableShape& n)
        : meanSums(n.nMeans * n.D), meanWeights(n.nMeans), covSums(n.nCovs * n.D), covWeights(n.nCovs), entryWeights(n.nEntries) {}
};
// side 1: zeros for a handle that has seen no discriminative call (the tables are not allocated then)
int fetch(gmm_estimator* e, int side, double* meanSums, double* meanWeights, double* covSums, double* covWeights,
          double* entryWeights) {
    GMM_HIP_CHECK(hipSetDevice(e->core.device));
    const int rc = waitDone(e->core);
    if (rc != GMM_OK)
        return rc;
    return e->side[side].fetch(e->shape(), meanSums, meanWeights, covSums, covWeights, entryWeights);
}
int fetch(gmm_estimator* e, int side, HostTables& h) {
    return fetch(e, side, h.meanSums.data(), h.meanWeights.data(), h.covSums.data(), h.covWeights.data(), h.entryWeights.data());
}

int serialize(gmm_estimator* e, std::vector<unsigned char>& bytes, bool discriminative = false) {
    HostTables h(e->shape());
    const int  rc = fetch(e, 0, h);
    if (rc != GMM_OK)
        return rc;
    EstimatorTables t{};
    t.D            = e->core.D;
    t.nMeans       = e->nMeans;
    t.nCovs        = e->nCovs;
    t.nDens        = e->nDens;
    t.nMix         = e->core.nMix;
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
    HostTables d(e->shape());
    const int  rd = fetch(e, 1, d);
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
    destroyWait(e->core);
    delete e;
    return GMM_OK;
}

int gmm_estimator_reset(gmm_estimator* e) {
    if (!e)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null estimator");
    GMM_HIP_CHECK(hipSetDevice(e->core.device));
    const int rc = waitDone(e->core);
    return rc != GMM_OK ? rc : zeroTables(e);
}

int gmm_estimator_accumulate_device(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                    uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                    const uint32_t* pairDensity, const double* pairWeight, uint32_t nPairs, void* stream) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, pairDensity, nullptr, pairWeight, nullptr, nPairs};
    const int      rc = checkPairCall(e ? &e->core : nullptr, kNouns, scorer, call);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    return deviceCall(e->core, nPairs, stream, nothingToPrepare,
                      [&](hipStream_t st) { return accumulateOn(e, scorer, call, 1, st); });
}

int gmm_estimator_accumulate_host(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                  uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                  const uint32_t* pairDensity, const double* pairWeight, uint32_t nPairs) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, pairDensity, nullptr, pairWeight, nullptr, nPairs};
    const int      rc = checkPairCall(e ? &e->core : nullptr, kNouns, scorer, call);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    return hostCall(e->core, call, nothingToPrepare,
                    [&](const PairCall& staged) { return accumulateOn(e, scorer, staged, 1, nullptr); });
}

int gmm_estimator_accumulate_posteriors_device(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                               uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                               const double* pairWeight, uint32_t nPairs, double threshold, void* stream) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, nullptr, nullptr, pairWeight, nullptr, nPairs};
    const int      rc = checkPosteriorCall(e, scorer, call);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    return deviceCall(e->core, nPairs, stream, [&] { return ensurePosteriorScratch(e); },
                      [&](hipStream_t st) { return accumulatePosteriorsOn(e, scorer, call, threshold, st); });
}

int gmm_estimator_accumulate_posteriors_host(gmm_estimator* e, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                                             uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                                             const double* pairWeight, uint32_t nPairs, double threshold) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, nullptr, nullptr, pairWeight, nullptr, nPairs};
    const int      rc = checkPosteriorCall(e, scorer, call);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    return hostCall(e->core, call, [&] { return ensurePosteriorScratch(e); }, [&](const PairCall& staged) {
        return accumulatePosteriorsOn(e, scorer, staged, threshold, nullptr);
    });
}

int gmm_estimator_accumulate_discriminative_device(gmm_estimator* e, gmm_scorer* scorer, const float* frames,
                                                   uint32_t nFrames, uint32_t frameStride, const uint32_t* pairFrame,
                                                   const uint32_t* pairMix, const uint32_t* pairDensity,
                                                   const double* weightNum, const double* weightDen, uint32_t nPairs,
                                                   void* stream) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, pairDensity, nullptr, weightNum, weightDen, nPairs};
    int            rc = checkPairCall(e ? &e->core : nullptr, kNouns, scorer, call);
    if (rc == GMM_OK)
        rc = checkSides(weightNum, weightDen);
    if (rc != GMM_OK)
        return rc;
    return deviceCall(e->core, nPairs, stream, [&] { return ensureDenominatorTables(e); },
                      [&](hipStream_t st) { return accumulateOn(e, scorer, call, 2, st); });
}

int gmm_estimator_accumulate_discriminative_host(gmm_estimator* e, gmm_scorer* scorer, const float* frames,
                                                 uint32_t nFrames, uint32_t frameStride, const uint32_t* pairFrame,
                                                 const uint32_t* pairMix, const uint32_t* pairDensity,
                                                 const double* weightNum, const double* weightDen, uint32_t nPairs) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, pairDensity, nullptr, weightNum, weightDen, nPairs};
    int            rc = checkPairCall(e ? &e->core : nullptr, kNouns, scorer, call);
    if (rc == GMM_OK)
        rc = checkSides(weightNum, weightDen);
    if (rc != GMM_OK)
        return rc;
    return hostCall(e->core, call, [&] { return ensureDenominatorTables(e); },
                    [&](const PairCall& staged) { return accumulateOn(e, scorer, staged, 2, nullptr); });
}

int gmm_estimator_accumulate_discriminative_posteriors_device(gmm_estimator* e, gmm_scorer* scorer, const float* frames,
                                                              uint32_t nFrames, uint32_t frameStride,
                                                              const uint32_t* pairFrame, const uint32_t* pairMix,
                                                              const double* weightNum, const double* weightDen,
                                                              uint32_t nPairs, double threshold, void* stream) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, nullptr, nullptr, weightNum, weightDen, nPairs};
    int            rc = checkPosteriorCall(e, scorer, call);
    if (rc == GMM_OK)
        rc = checkSides(weightNum, weightDen);
    if (rc != GMM_OK)
        return rc;
    return deviceCall(e->core, nPairs, stream, [&] { return ensureDiscriminativePosteriors(e, nPairs); }, [&](hipStream_t st) {
        return accumulateDiscriminativePosteriorsOn(e, scorer, call, threshold, st);
    });
}

int gmm_estimator_accumulate_discriminative_posteriors_host(gmm_estimator* e, gmm_scorer* scorer, const float* frames,
                                                            uint32_t nFrames, uint32_t frameStride,
                                                            const uint32_t* pairFrame, const uint32_t* pairMix,
                                                            const double* weightNum, const double* weightDen,
                                                            uint32_t nPairs, double threshold) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, nullptr, nullptr, weightNum, weightDen, nPairs};
    int            rc = checkPosteriorCall(e, scorer, call);
    if (rc == GMM_OK)
        rc = checkSides(weightNum, weightDen);
    if (rc != GMM_OK)
        return rc;
    return hostCall(e->core, call, [&] { return ensureDiscriminativePosteriors(e, nPairs); }, [&](const PairCall& staged) {
        return accumulateDiscriminativePosteriorsOn(e, scorer, staged, threshold, nullptr);
    });
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
    return fetch(e, 1, meanSums, meanWeights, covSums, covWeights, entryWeights);
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
    return readSkipped(e->core, skipped);
}

int gmm_estimator_get(gmm_estimator* e, double* meanSums, double* meanWeights, double* covSums, double* covWeights,
                      double* entryWeights) {
    if (!e)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null estimator");
    return fetch(e, 0, meanSums, meanWeights, covSums, covWeights, entryWeights);
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
