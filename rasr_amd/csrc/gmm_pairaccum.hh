// gmm_pairaccum.hh -- what the three handles that accumulate aligned (frame, mixture[, density][, key]) pairs share:
// gmm_estimator.cc, gmm_adapt.cc and gmm_mllr.cc embed PairAccumCore (the model's index tables, the call scratch, the
// host call's staging, the event of the last call) and use its checks and call shapes (gmm_pairaccum.cc); the two
// keyed handles (affine, MLLR) also embed KeyedPairs and run its passes 1-3 and 5 (gmm_kernels_keyed.hip).
#pragma once

#include "../../include/rasr_gmm_adaptation.h"
#include "../../include/rasr_gmm_mllr.h"
#include "gmm_estimator.hh"
#include "gmm_scorer.hh"
#include "host/PairTopology.hh"

namespace rasr_gmm {

// ---- the keyed passes (gmm_kernels_keyed.hip): a sort key per pair, a table per key ----

// pairs of one key are cut into pieces of kPieceChunk; piece 0 is summed onto the table, a later piece into a slab row
constexpr uint32_t kPieceChunk = 512;
static_assert(GMM_AFFINE_CHUNK == kPieceChunk, "include/rasr_gmm_adaptation.h states the piece length");
static_assert(GMM_MLLR_CHUNK == kPieceChunk, "include/rasr_gmm_mllr.h states the piece length");
constexpr uint32_t kPieceBlock = 256;  // lanes of a combine workgroup = cells it owns

// slots of the later pieces' slabs of a call of nPairs pairs: the later piece whose first pair sits at sorted
// position i uses slot i / kPieceChunk, which no other later piece shares (gmm_estimator.hh, accumSlabSlots)
constexpr uint32_t pieceSlabSlots(uint32_t nPairs) {
    return nPairs / kPieceChunk + 1;
}
// pieces of a call of nPairs pairs over nKeys keys, at most
constexpr uint32_t pieceBound(uint32_t nPairs, uint32_t nKeys) {
    return nPairs / kPieceChunk + (nKeys < nPairs ? nKeys : nPairs);
}

// pass 1: every pair resolved to its sort key pairKey * nLeaves + leafOfMixture[mixture], its mean and its covariance;
// a pair that is out of range in any way gets the sentinel nKeys * nLeaves (which sorts behind every key) and is
// counted in *skipped.  A handle without leaves passes nLeaves 1 and no leaf table
struct KeyedResolveArgs {
    const uint32_t* pairFrame;      // [nPairs]
    const uint32_t* pairMix;        // [nPairs]
    const uint32_t* pairDensity;    // [nPairs] in-mixture index, or NULL: 0
    const uint32_t* pairKey;        // [nPairs] or NULL: 0
    const uint32_t* mixOff;         // [nMix + 1]
    const uint32_t* entryMean;      // [nEntries]
    const uint32_t* entryCov;       // [nEntries]
    const uint32_t* leafOfMixture;  // [nMix] or NULL: 0
    uint32_t*       key;            // [nPairs] out
    uint32_t*       mean;           // [nPairs] out
    uint32_t*       cov;            // [nPairs] out
    uint32_t*       pairIndex;      // [nPairs] out: 0, 1, ...
    unsigned long long* skipped;    // += skipped pairs
    uint32_t        nPairs, nFrames, nMix, nKeys, nLeaves;
};
int launchKeyedResolve(const KeyedResolveArgs& a, ihipStream_t* stream);

// pass 3 (pass 2 is gmm_estimator.hh's launchAccumSort): the sorted positions' frame, mean, covariance and weight
// gathered into contiguous arrays, and the sorted position of every piece's first pair listed, in any order
struct IndexPiecesArgs {
    const uint32_t* keysSorted;   // [nPairs] key, ascending; nKeys: skipped pairs (at the end)
    const uint32_t* indexSorted;  // [nPairs] pair of the sorted position, ascending within a key
    const uint32_t* pairFrame;    // [nPairs]
    const double*   pairWeight;   // [nPairs] or NULL: 1
    const uint32_t* pairMean;     // [nPairs] resolved mean
    const uint32_t* pairCov;      // [nPairs] resolved covariance
    uint32_t*       sFrame;       // [nPairs] out
    uint32_t*       sMean;        // [nPairs] out
    uint32_t*       sCov;         // [nPairs] out
    double*         sWeight;      // [nPairs] out
    uint32_t*       pieces;       // [pieceBound] out
    uint32_t*       nPieces;      // [1], zeroed by the launch
    uint32_t        nPairs, nKeys, maxPieces;
};
int launchIndexPieces(const IndexPiecesArgs& a, ihipStream_t* stream);

// pass 5 (pass 4 is the handle's own accumulate kernel): a key with more than one piece adds its slab rows to its
// row of table in piece order; table [nKeys][cells], slab [pieceSlabSlots][cells]
int launchCombinePieces(const uint32_t* keysSorted, const uint32_t* pieces, const uint32_t* nPieces, uint32_t maxPieces,
                        uint32_t nPairs, double* table, const double* slab, size_t cells, ihipStream_t* stream);

namespace dev {

// pairs of the piece that starts at sorted position i with key k: the positions [i, i + n) hold k, n <= kPieceChunk
__device__ __forceinline__ uint32_t pieceLength(const uint32_t* keys, uint32_t i, uint32_t k, uint32_t nPairs) {
    uint32_t lo = i + 1, hi = min(i + kPieceChunk, nPairs);  // the first position past i whose key is not k
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] == k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - i;
}

}  // namespace dev

// ---- the host core (gmm_pairaccum.cc) ----

// how a handle is named in the messages of the shared checks
struct PairNouns {
    const char* handle;    // "estimator": "null estimator", "... the estimator's max_pairs ..."
    const char* model;     // "topology": "... differs from the estimator's topology"
    const char* topology;  // "estimator topology": the prefix of expandPairTopology's messages
};

// one accumulate call's arguments, host or device pointers alike
struct PairCall {
    const float*    frames;       // [nFrames][frameStride]
    uint32_t        nFrames, frameStride;
    const uint32_t* pairFrame;    // [nPairs]
    const uint32_t* pairMix;      // [nPairs]
    const uint32_t* pairDensity;  // [nPairs] or NULL
    const uint32_t* pairKey;      // [nPairs] or NULL (keyed handles)
    const double*   weight;       // [nPairs] or NULL
    const double*   weightDen;    // [nPairs] or NULL (discriminative calls)
    uint32_t        nPairs;
};

struct PairAccumCore {
    int      device = 0;
    uint32_t D = 0, nMix = 0, nEntries = 0, maxPairs = 0;
    bool     oneDensityPerMixture = false;
    // the model's index tables and the skipped count (device)
    DeviceBuffer<uint32_t>           dMixOff, dEntryMean, dEntryCov;
    DeviceBuffer<unsigned long long> dSkipped;
    // scratch of one call of up to maxPairs pairs
    DeviceBuffer<uint32_t> dBest, dPairIndex, dKeysSorted, dIndexSorted;
    DeviceBuffer<void>     dSortTemp;
    size_t                 sortTempBytes = 0;
    // the host call's pair lists: dPairKey of a keyed handle only, dPairWeightDen allocated by the estimator's first
    // discriminative call
    DeviceBuffer<uint32_t> dPairFrame, dPairMix, dPairDensity, dPairKey;
    DeviceBuffer<double>   dPairWeight, dPairWeightDen;
    // recorded by every accumulate call on its stream; whatever reads or zeroes the tables waits for it
    Event done;
    bool  pending = false;
};

// bits of the sort keys 0 .. n (n: the skipped pairs' sentinel)
uint32_t keyBits(uint32_t n);

// the fields from ms, its validated topology into topo (fail() with the nouns' prefix); touches no device
int initCore(PairAccumCore& c, const PairNouns& nouns, const gmm_mixture_set& ms, uint32_t maxPairs, int device,
             PairTopology& topo);
// the device side, on the current device: the index tables uploaded, the scratch (c.sortTempBytes is set), the staging
// and the event
int allocCore(PairAccumCore& c, const PairTopology& topo, bool keyed);

int waitDone(PairAccumCore& c);
void destroyWait(PairAccumCore& c);  // before the handle is deleted: no kernel of a call may outlive its scratch
int readSkipped(PairAccumCore& c, uint64_t* skipped);  // waits for the last call

// the checks of an accumulate call that need no device; c NULL: "null <handle>"
int checkPairCall(const PairAccumCore* c, const PairNouns& nouns, const gmm_scorer* scorer, const PairCall& call);
// no density given but a scorer: call.pairDensity becomes the scorer's best density of every pair (dBest)
int bestDensities(PairAccumCore& c, gmm_scorer* scorer, PairCall& call, hipStream_t stream);
// after a call's launches, failed ones too: what was enqueued before a failure still uses the scratch
int recordDone(PairAccumCore& c, hipStream_t stream);

// the host call's arguments on the device: the frames dense (row length D) in a buffer of the call's own, the lists
// that are not NULL in the handle's staging.  The caller has waited for the last call (waitDone)
struct StagedCall {
    DeviceBuffer<float> frames;
    PairCall            call;
};
int stageHostCall(PairAccumCore& c, const PairCall& host, StagedCall& staged);

// A *_device entry point after its checks: prepare() (what the first call of a kind allocates), then launch(stream)
// and the event.  A call of no pairs ends after prepare()
template <class Prepare, class Launch>
int deviceCall(PairAccumCore& c, uint32_t nPairs, void* stream, Prepare&& prepare, Launch&& launch) {
    GMM_HIP_CHECK(hipSetDevice(c.device));
    int rc = prepare();
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc             = launch(st);
    const int rr   = recordDone(c, st);
    return rr != GMM_OK ? rr : rc;
}

// A *_host entry point after its checks: the last call awaited (it may still read the staging), prepare(), the
// arguments staged, launch(device call) on the null stream, synchronous
template <class Prepare, class Launch>
int hostCall(PairAccumCore& c, const PairCall& host, Prepare&& prepare, Launch&& launch) {
    GMM_HIP_CHECK(hipSetDevice(c.device));
    int rc = waitDone(c);
    if (rc != GMM_OK || (rc = prepare()) != GMM_OK || host.nPairs == 0)
        return rc;
    StagedCall s;
    if ((rc = stageHostCall(c, host, s)) != GMM_OK)
        return rc;
    rc = launch(s.call);
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // before the frames are released
    return rc;
}
inline int nothingToPrepare() {
    return GMM_OK;
}

// ---- what the two keyed handles add: the model's values, the resolved and the gathered pairs, the piece list ----

struct KeyedPairs {
    uint32_t nKeys = 0, nLeaves = 1, nSets = 0, maxPieces = 0;  // nSets = nKeys * nLeaves sort keys
    uint64_t tableBytes = 0, scratchBytes = 0;                 // what the handle's info call reports
    DeviceBuffer<float>    dMeans, dVariances;
    DeviceBuffer<uint32_t> dLeaf;  // [nMix], a handle with leaves only
    DeviceBuffer<uint32_t> dKey, dMean, dCov, dSFrame, dSMean, dSCov, dPieces, dNPieces;
    DeviceBuffer<double>   dSWeight;
};

// The sizes of a handle of nKeys [x nLeaves] sets of perSet bytes each and calls of up to maxPairs pairs, into k and
// c.sortTempBytes; GMM_ERR_UNSUPPORTED where the tables and the scratch need more than three quarters of the current
// device's free memory (leaves: the message names the leaves too)
int keyedSizes(PairAccumCore& c, KeyedPairs& k, const PairNouns& nouns, uint32_t nKeys, uint32_t nLeaves, bool leaves,
               uint64_t perSet, uint32_t maxPairs);
// the means and variances of ms (and leafOfMixture, or NULL) uploaded, the keyed scratch
int allocKeyed(PairAccumCore& c, KeyedPairs& k, const gmm_mixture_set& ms, const uint32_t* leafOfMixture);
// passes 1 to 3 of a call: after them dKeysSorted, dSFrame / dSMean / dSCov / dSWeight and the piece list are the
// call's; returns the call's piece bound
int indexKeyedPairs(PairAccumCore& c, KeyedPairs& k, gmm_scorer* scorer, PairCall call, hipStream_t stream,
                    uint32_t* callPieces);

}  // namespace rasr_gmm
