// gmm_pairaccum.cc -- the host core of the handles that accumulate aligned pairs (gmm_pairaccum.hh): creation of the
// shared device state, the checks of a call, the staging of a host call, the event of the last call, and for the keyed
// handles the memory budget and passes 1-3.  The rules that every such handle keeps live here once:
//   - the event is recorded even after a failed launch (recordDone);
//   - a host call waits for the last call before it overwrites the staging (hostCall);
//   - a scorer that holds a mixture shard is refused (checkPairCall);
//   - a density 0xffffffff (no best density) is out of range (the resolve kernels).
#include <algorithm>
#include <cstdio>

#include "gmm_pairaccum.hh"

namespace rasr_gmm {

uint32_t keyBits(uint32_t n) {
    uint32_t b = 1;
    while (b < 32 && (n >> b))
        ++b;
    return b;
}

int initCore(PairAccumCore& c, const PairNouns& nouns, const gmm_mixture_set& ms, uint32_t maxPairs, int device,
             PairTopology& topo) {
    c.device   = device;
    c.D        = ms.dimension;
    c.nMix     = ms.n_mixtures;
    c.maxPairs = maxPairs;
    std::string message;
    const int   rc = expandPairTopology(ms, nouns.topology, topo, &message);
    if (rc != GMM_OK)
        return fail(rc, message);
    c.nEntries             = topo.nEntries;
    c.oneDensityPerMixture = topo.oneDensityPerMixture;
    return GMM_OK;
}

int allocCore(PairAccumCore& c, const PairTopology& topo, bool keyed) {
    int rc;
    if ((rc = upload(c.dMixOff, topo.mixOff)) || (rc = upload(c.dEntryMean, topo.entryMean)) ||
        (rc = upload(c.dEntryCov, topo.entryCov)))
        return rc;
    const size_t P = c.maxPairs;
    GMM_HIP_CHECK(c.dSkipped.alloc(1));
    for (DeviceBuffer<uint32_t>* b :
         {&c.dBest, &c.dPairIndex, &c.dKeysSorted, &c.dIndexSorted, &c.dPairFrame, &c.dPairMix, &c.dPairDensity})
        GMM_HIP_CHECK(b->alloc(P));
    if (keyed)
        GMM_HIP_CHECK(c.dPairKey.alloc(P));
    GMM_HIP_CHECK(c.dPairWeight.alloc(P));
    GMM_HIP_CHECK(c.dSortTemp.alloc(c.sortTempBytes));
    GMM_HIP_CHECK(c.done.create(hipEventDisableTiming));
    return GMM_OK;
}

int waitDone(PairAccumCore& c) {
    if (c.pending) {
        GMM_HIP_CHECK(hipEventSynchronize(c.done.get()));
        c.pending = false;
    }
    return GMM_OK;
}

void destroyWait(PairAccumCore& c) {
    (void)hipSetDevice(c.device);
    if (c.pending)
        (void)hipEventSynchronize(c.done.get());
}

int readSkipped(PairAccumCore& c, uint64_t* skipped) {
    GMM_HIP_CHECK(hipSetDevice(c.device));
    const int rc = waitDone(c);
    if (rc != GMM_OK)
        return rc;
    unsigned long long v = 0;
    GMM_HIP_CHECK(hipMemcpy(&v, c.dSkipped.get(), sizeof(v), hipMemcpyDeviceToHost));
    *skipped = v;
    return GMM_OK;
}

int checkPairCall(const PairAccumCore* c, const PairNouns& nouns, const gmm_scorer* scorer, const PairCall& call) {
    const auto handle = [&nouns] { return std::string(nouns.handle); };  // a message is built only where a check fails
    if (!c)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null " + handle());
    if (call.nPairs > c->maxPairs)
        return fail(GMM_ERR_CAPACITY, "n_pairs " + std::to_string(call.nPairs) + " exceeds the " + handle() + "'s max_pairs " +
                                              std::to_string(c->maxPairs));
    if (call.nPairs && (!call.frames || !call.pairFrame || !call.pairMix))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    if (call.frameStride < c->D)
        return fail(GMM_ERR_INVALID_ARGUMENT, "frame_stride below the dimension");
    if (call.pairDensity)
        return GMM_OK;
    if (!scorer) {
        if (!c->oneDensityPerMixture)  // verify_(mixture->nDensities() == 1), AbstractMixtureSetEstimator.cc:382
            return fail(GMM_ERR_INVALID_ARGUMENT, "no density given and no scorer: every mixture must hold exactly one density");
        return GMM_OK;
    }
    if (scorer->device != c->device)
        return fail(GMM_ERR_UNSUPPORTED, "the scorer is on another device than the " + handle());
    const gmm_scorer_config& cfg = scorer->cfg;
    if (!(cfg.mixture_begin == 0 && (cfg.mixture_end == 0 || cfg.mixture_end == c->nMix)))
        return fail(GMM_ERR_UNSUPPORTED, "the scorer holds a mixture shard: the " + handle() + " needs the whole mixture range");
    const int rc = checkPairs(scorer);
    if (rc != GMM_OK)
        return rc;
    if (scorer->D != c->D || scorer->nMix != c->nMix || scorer->pairs->nEntries != c->nEntries)
        return fail(GMM_ERR_INVALID_ARGUMENT, "the scorer's dimension, mixture count or entry count differs from the " +
                                                      handle() + "'s " + nouns.model);
    return GMM_OK;
}

int bestDensities(PairAccumCore& c, gmm_scorer* scorer, PairCall& call, hipStream_t stream) {
    if (call.pairDensity || !scorer)
        return GMM_OK;
    PairArgs a  = pairArgsOf(scorer, call.frames, call.nFrames, call.frameStride);
    a.pairFrame = call.pairFrame;
    a.pairMix   = call.pairMix;
    a.best      = c.dBest.get();
    a.nPairs    = call.nPairs;
    GMM_HIP_CHECK(launchBestPairs(a, stream));
    call.pairDensity = c.dBest.get();  // densityIndex() = bestDensity of the pair
    return GMM_OK;
}

int recordDone(PairAccumCore& c, hipStream_t stream) {
    GMM_HIP_CHECK(hipEventRecord(c.done.get(), stream));
    c.pending = true;
    return GMM_OK;
}

int stageHostCall(PairAccumCore& c, const PairCall& host, StagedCall& staged) {
    const size_t D = c.D, n = host.nPairs;
    GMM_HIP_CHECK(staged.frames.alloc(std::max<size_t>(static_cast<size_t>(host.nFrames) * D, 1)));
    if (host.nFrames && D)
        GMM_HIP_CHECK(hipMemcpy2D(staged.frames.get(), D * sizeof(float), host.frames,
                                  static_cast<size_t>(host.frameStride) * sizeof(float), D * sizeof(float), host.nFrames,
                                  hipMemcpyHostToDevice));
    PairCall& s   = staged.call;
    s             = host;
    s.frames      = staged.frames.get();
    s.frameStride = c.D;
    // a list that is given goes into its staging buffer, and the staged call names the buffer
    auto stage = [n](auto* buffer, auto& list) {
        if (!list)
            return hipSuccess;
        const hipError_t e = hipMemcpy(buffer, list, n * sizeof(*buffer), hipMemcpyHostToDevice);
        list               = buffer;
        return e;
    };
    GMM_HIP_CHECK(stage(c.dPairFrame.get(), s.pairFrame));
    GMM_HIP_CHECK(stage(c.dPairMix.get(), s.pairMix));
    GMM_HIP_CHECK(stage(c.dPairDensity.get(), s.pairDensity));
    GMM_HIP_CHECK(stage(c.dPairKey.get(), s.pairKey));
    GMM_HIP_CHECK(stage(c.dPairWeight.get(), s.weight));
    GMM_HIP_CHECK(stage(c.dPairWeightDen.get(), s.weightDen));
    return GMM_OK;
}

int keyedSizes(PairAccumCore& c, KeyedPairs& k, const PairNouns& nouns, uint32_t nKeys, uint32_t nLeaves, bool leaves,
               uint64_t perSet, uint32_t maxPairs) {
    const uint64_t sets = static_cast<uint64_t>(nKeys) * nLeaves;
    size_t         freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess)
        freeB = 0;
    const uint64_t P = maxPairs, slots = pieceSlabSlots(maxPairs);
    // the sets are sort keys with a sentinel behind them: past 32 bits no device holds the tables anyway (without
    // leaves the sets are the keys, and the sentinel n_keys always fits)
    const bool keyable = !leaves || sets < 0xffffffffull;
    k.nKeys     = nKeys;
    k.nLeaves   = nLeaves;
    k.nSets     = keyable ? static_cast<uint32_t>(sets) : 0;
    k.maxPieces = pieceBound(maxPairs, k.nSets);
    size_t sortBytes = 0;
    if (P && keyable)
        GMM_HIP_CHECK(static_cast<hipError_t>(accumSortTempBytes(maxPairs, keyBits(k.nSets), &sortBytes)));
    c.sortTempBytes = sortBytes;
    k.tableBytes    = sets * perSet;
    k.scratchBytes  = slots * perSet + P * (15 * sizeof(uint32_t) + 2 * sizeof(double)) +
                     (static_cast<uint64_t>(k.maxPieces) + 1) * sizeof(uint32_t) + sortBytes;
    const double need = static_cast<double>(sets) * static_cast<double>(perSet) + static_cast<double>(k.scratchBytes);
    if (keyable && need <= static_cast<double>(freeB / 4 * 3))
        return GMM_OK;
    char       msg[360], of[48] = "";
    const char *lower = "";
    if (leaves) {
        std::snprintf(of, sizeof(of), " x %u leaves", nLeaves);
        lower = ", n_leaves";
    }
    std::snprintf(msg, sizeof(msg),
                  "%s: %u keys%s x %.1f KiB of tables and the scratch of %u pairs need %.2f GiB of device memory (%.2f GiB "
                  "free): lower n_keys%s or max_pairs",
                  nouns.topology, nKeys, of, static_cast<double>(perSet) / 1024.0, maxPairs, need / (1u << 30),
                  static_cast<double>(freeB) / (1u << 30), lower);
    return fail(GMM_ERR_UNSUPPORTED, msg);
}

int allocKeyed(PairAccumCore& c, KeyedPairs& k, const gmm_mixture_set& ms, const uint32_t* leafOfMixture) {
    const size_t       D = c.D, P = c.maxPairs;
    std::vector<float> means(ms.means, ms.means + static_cast<size_t>(ms.n_means) * D);
    std::vector<float> variances(ms.variances, ms.variances + static_cast<size_t>(ms.n_covariances) * D);
    int                rc;
    if ((rc = upload(k.dMeans, means)) || (rc = upload(k.dVariances, variances)))
        return rc;
    if (leafOfMixture && (rc = upload(k.dLeaf, std::vector<uint32_t>(leafOfMixture, leafOfMixture + c.nMix))))
        return rc;
    for (DeviceBuffer<uint32_t>* b : {&k.dKey, &k.dMean, &k.dCov, &k.dSFrame, &k.dSMean, &k.dSCov})
        GMM_HIP_CHECK(b->alloc(P));
    GMM_HIP_CHECK(k.dSWeight.alloc(P));
    GMM_HIP_CHECK(k.dPieces.alloc(k.maxPieces));
    GMM_HIP_CHECK(k.dNPieces.allocZeroed(1));
    return GMM_OK;
}

int indexKeyedPairs(PairAccumCore& c, KeyedPairs& k, gmm_scorer* scorer, PairCall call, hipStream_t stream,
                    uint32_t* callPieces) {
    const int rc = bestDensities(c, scorer, call, stream);
    if (rc != GMM_OK)
        return rc;
    KeyedResolveArgs r{};
    r.pairFrame     = call.pairFrame;
    r.pairMix       = call.pairMix;
    r.pairDensity   = call.pairDensity;
    r.pairKey       = call.pairKey;
    r.mixOff        = c.dMixOff.get();
    r.entryMean     = c.dEntryMean.get();
    r.entryCov      = c.dEntryCov.get();
    r.leafOfMixture = k.dLeaf.get();
    r.key           = k.dKey.get();
    r.mean          = k.dMean.get();
    r.cov           = k.dCov.get();
    r.pairIndex     = c.dPairIndex.get();
    r.skipped       = c.dSkipped.get();
    r.nPairs        = call.nPairs;
    r.nFrames       = call.nFrames;
    r.nMix          = c.nMix;
    r.nKeys         = k.nKeys;
    r.nLeaves       = k.nLeaves;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchKeyedResolve(r, stream)));
    GMM_HIP_CHECK(static_cast<hipError_t>(launchAccumSort(c.dSortTemp.get(), c.sortTempBytes, k.dKey.get(), c.dPairIndex.get(),
                                                         c.dKeysSorted.get(), c.dIndexSorted.get(), call.nPairs,
                                                         keyBits(k.nSets), stream)));
    *callPieces = pieceBound(call.nPairs, k.nSets);
    IndexPiecesArgs x{};
    x.keysSorted  = c.dKeysSorted.get();
    x.indexSorted = c.dIndexSorted.get();
    x.pairFrame   = call.pairFrame;
    x.pairWeight  = call.weight;
    x.pairMean    = k.dMean.get();
    x.pairCov     = k.dCov.get();
    x.sFrame      = k.dSFrame.get();
    x.sMean       = k.dSMean.get();
    x.sCov        = k.dSCov.get();
    x.sWeight     = k.dSWeight.get();
    x.pieces      = k.dPieces.get();
    x.nPieces     = k.dNPieces.get();
    x.nPairs      = call.nPairs;
    x.nKeys       = k.nSets;
    x.maxPieces   = *callPieces;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchIndexPieces(x, stream)));
    return GMM_OK;
}

}  // namespace rasr_gmm
