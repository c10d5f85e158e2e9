// gmm_mllr.cc -- the handle behind include/rasr_gmm_mllr.h: the (key, leaf) sets' f64 accumulators on the device
// (their layout, the kinds), create's own argument rules, pass 4 of a call (gmm_kernels_mllr.hip), get / add / info.
// Everything a handle that accumulates keyed pairs shares with the others is gmm_pairaccum.hh's.
// The estimation of the matrices from the tables and the adapted means are host/MllrEstimate.cc (no HIP).
#include <algorithm>
#include <memory>
#include <new>

#include "gmm_mllr.hh"

using namespace rasr_gmm;

struct gmm_mllr_accumulator {
    PairAccumCore core;
    KeyedPairs    keyed;
    int           kinds = 0;
    MllrLayout    layout{};
    // the accumulators, and the later pieces' slab of one call
    DeviceBuffer<double> dTables, dSlab;
};

namespace {

constexpr PairNouns kNouns{"mllr accumulator", "mixture set", "mllr accumulator"};

int zeroTables(gmm_mllr_accumulator* h) {
    GMM_HIP_CHECK(hipMemset(h->dTables.get(), 0, h->keyed.nSets * h->layout.cells() * sizeof(double)));
    GMM_HIP_CHECK(hipMemset(h->core.dSkipped.get(), 0, sizeof(unsigned long long)));
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // done before a call on any other stream
    return GMM_OK;
}

int create(gmm_mllr_accumulator* h, const gmm_mixture_set& ms, const uint32_t* leafOfMixture, uint32_t nLeaves,
           uint32_t nKeys, int kinds, uint32_t maxPairs, int device) {
    PairTopology topo;
    int          rc = initCore(h->core, kNouns, ms, maxPairs, device, topo);
    if (rc != GMM_OK)
        return rc;
    h->kinds  = kinds;
    h->layout = MllrLayout{ms.dimension, (kinds & GMM_MLLR_FULL) != 0, (kinds & GMM_MLLR_SHIFT) != 0};
    for (uint32_t m = 0; m < ms.n_mixtures; ++m)
        if (leafOfMixture[m] >= nLeaves)
            return fail(GMM_ERR_INVALID_ARGUMENT, "mllr accumulator: mixture " + std::to_string(m) + " maps to leaf " +
                                                          std::to_string(leafOfMixture[m]) + " of " + std::to_string(nLeaves));
    GMM_HIP_CHECK(hipSetDevice(device));
    if ((rc = keyedSizes(h->core, h->keyed, kNouns, nKeys, nLeaves, true, h->layout.cells() * sizeof(double), maxPairs)) ||
        (rc = allocCore(h->core, topo, true)) || (rc = allocKeyed(h->core, h->keyed, ms, leafOfMixture)))
        return rc;
    GMM_HIP_CHECK(h->dTables.alloc(h->keyed.nSets * h->layout.cells()));
    GMM_HIP_CHECK(h->dSlab.alloc(pieceSlabSlots(maxPairs) * h->layout.cells()));
    return zeroTables(h);
}

int accumulateOn(gmm_mllr_accumulator* h, gmm_scorer* scorer, const PairCall& call, hipStream_t stream) {
    PairAccumCore& c = h->core;
    KeyedPairs&    k = h->keyed;
    uint32_t       pieces = 0;
    const int      rc = indexKeyedPairs(c, k, scorer, call, stream, &pieces);
    if (rc != GMM_OK)
        return rc;
    MllrArgs a{};
    a.setsSorted  = c.dKeysSorted.get();
    a.sFrame      = k.dSFrame.get();
    a.sMean       = k.dSMean.get();
    a.sCov        = k.dSCov.get();
    a.sWeight     = k.dSWeight.get();
    a.frames      = call.frames;
    a.means       = k.dMeans.get();
    a.variances   = k.dVariances.get();
    a.pieces      = k.dPieces.get();
    a.nPieces     = k.dNPieces.get();
    a.tables      = h->dTables.get();
    a.slab        = h->dSlab.get();
    a.layout      = h->layout;
    a.nPairs      = call.nPairs;
    a.nSets       = k.nSets;
    a.frameStride = call.frameStride;
    a.maxPieces   = pieces;
    GMM_HIP_CHECK(static_cast<hipError_t>(launchMllrAccumulate(a, stream)));
    GMM_HIP_CHECK(static_cast<hipError_t>(launchCombinePieces(a.setsSorted, a.pieces, a.nPieces, pieces, call.nPairs, a.tables,
                                                             a.slab, h->layout.cells(), stream)));
    return GMM_OK;
}

// waits for the last call; cells: the raw range of the set (key, leaf) on the host
int fetchSet(gmm_mllr_accumulator* h, uint32_t key, uint32_t leaf, std::vector<double>& cells) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null mllr accumulator");
    const KeyedPairs& k = h->keyed;
    if (key >= k.nKeys || leaf >= k.nLeaves)
        return fail(GMM_ERR_INVALID_ARGUMENT, "key " + std::to_string(key) + " or leaf " + std::to_string(leaf) +
                                                      " out of range: the mllr accumulator holds " + std::to_string(k.nKeys) +
                                                      " keys x " + std::to_string(k.nLeaves) + " leaves");
    GMM_HIP_CHECK(hipSetDevice(h->core.device));
    const int rc = waitDone(h->core);
    if (rc != GMM_OK)
        return rc;
    const size_t C = h->layout.cells();
    cells.resize(C);
    GMM_HIP_CHECK(hipMemcpy(cells.data(), h->dTables.get() + (static_cast<size_t>(key) * k.nLeaves + leaf) * C,
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
    destroyWait(h->core);
    delete h;
    return GMM_OK;
}

int gmm_mllr_reset(gmm_mllr_accumulator* h) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null mllr accumulator");
    GMM_HIP_CHECK(hipSetDevice(h->core.device));
    const int rc = waitDone(h->core);
    return rc != GMM_OK ? rc : zeroTables(h);
}

int gmm_mllr_accumulate_device(gmm_mllr_accumulator* h, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
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

int gmm_mllr_accumulate_host(gmm_mllr_accumulator* h, gmm_scorer* scorer, const float* frames, uint32_t nFrames,
                             uint32_t frameStride, const uint32_t* pairFrame, const uint32_t* pairMix,
                             const uint32_t* pairDensity, const double* pairWeight, const uint32_t* pairKey, uint32_t nPairs) {
    const PairCall call{frames, nFrames, frameStride, pairFrame, pairMix, pairDensity, pairKey, pairWeight, nullptr, nPairs};
    const int      rc = checkPairCall(h ? &h->core : nullptr, kNouns, scorer, call);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    return hostCall(h->core, call, nothingToPrepare,
                    [&](const PairCall& staged) { return accumulateOn(h, scorer, staged, nullptr); });
}

int gmm_mllr_skipped(gmm_mllr_accumulator* h, uint64_t* skipped) {
    if (!h || !skipped)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    return readSkipped(h->core, skipped);
}

int gmm_mllr_info(const gmm_mllr_accumulator* h, uint64_t* tableBytes, uint64_t* scratchBytes, int* kinds) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null mllr accumulator");
    if (tableBytes)
        *tableBytes = h->keyed.tableBytes;
    if (scratchBytes)
        *scratchBytes = h->keyed.scratchBytes;
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
    GMM_HIP_CHECK(hipMemcpy(h->dTables.get() + (static_cast<size_t>(key) * h->keyed.nLeaves + leaf) * c.size(), c.data(),
                            c.size() * sizeof(double), hipMemcpyHostToDevice));
    return GMM_OK;
}

}  // extern "C"
