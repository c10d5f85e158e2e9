// gmm_group.cc -- the density-sharded handle (gmm_scorer_create_sharded) and the RCCL loader.
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library is opened at run time (Rccl below)

#include <algorithm>
#include <cstdlib>

#include "gmm_scorer.hh"
#include "gmm_shard.hh"

namespace rasr_gmm {
namespace {

// RCCL, opened on first use by a density-sharded handle with the RCCL exchange: single-GPU users of the library
// need no RCCL installation, and the library has no link-time dependency on it
struct Rccl {
    ncclResult_t (*commInitAll)(ncclComm_t*, int, const int*)                                           = nullptr;
    ncclResult_t (*commDestroy)(ncclComm_t)                                                             = nullptr;
    ncclResult_t (*allReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*groupStart)()                                                                        = nullptr;
    ncclResult_t (*groupEnd)()                                                                          = nullptr;
    const char* (*errorString)(ncclResult_t)                                                            = nullptr;
    std::string error;  // empty: loaded
};

const Rccl& rccl() {
    static const Rccl r = [] {
        Rccl x;
        void*                    h = nullptr;
        std::vector<std::string> names{"librccl.so.1", "librccl.so"};
        if (const char* rocm = std::getenv("ROCM_PATH"))
            names.push_back(std::string(rocm) + "/lib/librccl.so.1");
        names.push_back("/opt/rocm/lib/librccl.so.1");
        for (const std::string& name : names)
            if ((h = dlopen(name.c_str(), RTLD_NOW | RTLD_GLOBAL)))
                break;
        if (!h) {
            const char* e = dlerror();
            x.error = std::string("cannot open librccl.so.1: ") + (e ? e : "?");
            return x;
        }
        x.commInitAll = reinterpret_cast<decltype(x.commInitAll)>(dlsym(h, "ncclCommInitAll"));
        x.commDestroy = reinterpret_cast<decltype(x.commDestroy)>(dlsym(h, "ncclCommDestroy"));
        x.allReduce   = reinterpret_cast<decltype(x.allReduce)>(dlsym(h, "ncclAllReduce"));
        x.groupStart  = reinterpret_cast<decltype(x.groupStart)>(dlsym(h, "ncclGroupStart"));
        x.groupEnd    = reinterpret_cast<decltype(x.groupEnd)>(dlsym(h, "ncclGroupEnd"));
        x.errorString = reinterpret_cast<decltype(x.errorString)>(dlsym(h, "ncclGetErrorString"));
        if (!x.commInitAll || !x.commDestroy || !x.allReduce || !x.groupStart || !x.groupEnd || !x.errorString)
            x.error = "librccl.so lacks an nccl* entry point";
        return x;
    }();
    return r;
}

#define GMM_NCCL_CHECK(expr)                                                                        \
    do {                                                                                            \
        ncclResult_t r_ = (expr);                                                                   \
        if (r_ != ncclSuccess)                                                                      \
            return fail(GMM_ERR_DEVICE, std::string(#expr) + ": " + rccl().errorString(r_));      \
    } while (0)

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// Density-sharded handles (gmm_scorer_create_sharded, BASELINE config 4 for a C / C++ caller): one process,
// part r of the density shard plan (gmm_shard.hh) on devices[r].  A call, on the caller's stream S of
// devices[0]:
//   every part, on its own stream after S's start event: frames -> its device (peer copy; none on devices[0]),
//     its sub-model scored into [nLocal][n], the split mixtures it holds packed into keys [nSplit][n]
//     (INT64_MAX for the ones it does not hold), then
//   the per-frame reduce of the keys, either
//     RCCL: on every GPU the keys of its other parts folded into its first part's (minIntoShardKeys), then an
//       all-reduce(MIN) over those first parts, one rank per distinct GPU (ncclGroupStart/End, one comm per GPU);
//       with every part on one GPU that is a one-rank all-reduce, which is how a one-GPU box runs this path, or
//     COPY: peer copies of every part's keys to devices[0] and minShardKeys there;
//   every part copies its whole mixtures (local rows [rowLo, rowHi)) into the full table's rows;
//   S waits for every part, unpacks the split mixtures' keys into their rows.
// The full table's other rows come straight from the parts: no all-gather (the caller reads one table).
struct DensityPart {
    std::unique_ptr<gmm_scorer> scorer;  // sub-model (null: the part holds no mixture)
    int          device = 0;
    DensityShard shard;
    uint32_t     nLocal = 0, rowLo = 0, rowHi = 0;             // rows [rowLo, rowHi): whole mixtures
    std::vector<std::pair<uint32_t, uint32_t>> held;           // (split slot, local row)
    DeviceBuffer<uint32_t> dHeldOffset;                        // [held] in-mixture index of the row's first entry
    Stream       stream;
    Event        done;
    Event        keysReady;  // RCCL: this part's keys packed (parts other than their GPU's first)
    std::vector<uint32_t> fold;          // RCCL: the other parts on this part's GPU (this part is their first)
    DeviceBuffer<float>    dFrames;  // [maxF][D] (parts not on devices[0])
    DeviceBuffer<float>    dScores;  // [nLocal][maxF]
    DeviceBuffer<uint32_t> dBest;
    DeviceBuffer<int64_t>  dKeys;    // [nSplit][maxF]
};

struct DensityGroup {
    std::vector<ncclComm_t>  comms;  // RCCL: one per entry of ranks
    std::vector<uint32_t>    split;  // mixtures held by more than one part
    int                      exchange = GMM_EXCHANGE_AUTO;
    std::vector<uint32_t>    ranks;  // RCCL: the first part on each distinct GPU, in device-list order
    int                      lead     = 0;  // devices[0]
    DeviceBuffer<int64_t>    dGather;       // COPY: [parts][nSplit][maxF] on the lead
    DeviceBuffer<int64_t>    dReduced;      // COPY: [nSplit][maxF]
    Event                    start, finish;  // on the caller's stream (lead)
    std::vector<DensityPart> parts;

    // the orderings: the part streams idle, then the communicators, then every part released with its device
    // current, then (as members, after this body) the lead's buffers and events with the lead current
    ~DensityGroup() {
        for (DensityPart& p : parts) {
            (void)hipSetDevice(p.device);
            if (p.stream)
                (void)hipStreamSynchronize(p.stream.get());
        }
        for (ncclComm_t c : comms)
            if (c)
                (void)rccl().commDestroy(c);
        while (!parts.empty()) {
            (void)hipSetDevice(parts.back().device);
            parts.pop_back();
        }
        (void)hipSetDevice(lead);
    }
};

int groupScore(gmm_scorer* s, const float* frames, uint32_t n, uint32_t frameStride, float* scores, uint32_t* best,
               uint32_t scoreStride, hipStream_t stream) {
    DensityGroup&  g        = *s->group;
    const size_t   nS       = g.split.size(), keyN = nS * n, D = s->D;
    const bool     withBest = best && s->hasAssignment();
    const uint32_t P        = static_cast<uint32_t>(g.parts.size());
    // the parts' buffers are free once the previous call's reads of them (on its stream) are done
    GMM_HIP_CHECK(hipStreamWaitEvent(stream, g.finish.get(), 0));
    GMM_HIP_CHECK(hipEventRecord(g.start.get(), stream));
    for (DensityPart& p : g.parts) {
        GMM_HIP_CHECK(hipSetDevice(p.device));
        GMM_HIP_CHECK(hipStreamWaitEvent(p.stream.get(), g.start.get(), 0));
        const float* f  = frames;
        uint32_t     fs = frameStride;
        if (p.dFrames.get()) {
            GMM_HIP_CHECK(hipMemcpy2DAsync(p.dFrames.get(), D * sizeof(float), frames, static_cast<size_t>(frameStride) * sizeof(float),
                                           D * sizeof(float), n, hipMemcpyDefault, p.stream.get()));
            f = p.dFrames.get(), fs = s->D;
        }
        int rc;
        if (p.scorer && (rc = scoreImpl(p.scorer.get(), f, n, fs, p.dScores.get(), withBest ? p.dBest.get() : nullptr, n, p.stream.get())) != GMM_OK)
            return rc;
        if (nS) {
            GMM_HIP_CHECK(launchFillShardKeys(p.dKeys.get(), keyN, p.stream.get()));
            for (size_t h = 0; h < p.held.size(); ++h) {
                const uint32_t slot = p.held[h].first, row = p.held[h].second;
                GMM_HIP_CHECK(launchPackShardKeys(p.dScores.get() + static_cast<size_t>(row) * n,
                                                  withBest ? p.dBest.get() + static_cast<size_t>(row) * n : nullptr,
                                                  p.dHeldOffset.get() + h, 1, n, n, p.dKeys.get() + static_cast<size_t>(slot) * n,
                                                  p.stream.get()));
            }
            if (p.keysReady)
                GMM_HIP_CHECK(hipEventRecord(p.keysReady.get(), p.stream.get()));
        }
    }
    // the per-frame reduce of the split mixtures
    const int64_t* reduced = nullptr;
    if (nS && g.exchange == GMM_EXCHANGE_RCCL) {
        // on every GPU: its other parts' keys folded into its first part's, on that part's stream
        for (uint32_t r : g.ranks) {
            DensityPart& lead = g.parts[r];
            GMM_HIP_CHECK(hipSetDevice(lead.device));
            for (uint32_t f : lead.fold) {
                GMM_HIP_CHECK(hipStreamWaitEvent(lead.stream.get(), g.parts[f].keysReady.get(), 0));
                GMM_HIP_CHECK(launchMinIntoShardKeys(lead.dKeys.get(), g.parts[f].dKeys.get(), keyN, lead.stream.get()));
            }
        }
        // across GPUs: all-reduce(MIN) in place, one rank per GPU
        const Rccl& x = rccl();
        GMM_NCCL_CHECK(x.groupStart());
        ncclResult_t nr = ncclSuccess;
        hipError_t   hr = hipSuccess;
        for (size_t i = 0; i < g.ranks.size() && nr == ncclSuccess && hr == hipSuccess; ++i) {
            DensityPart& p = g.parts[g.ranks[i]];
            if ((hr = hipSetDevice(p.device)) == hipSuccess)
                nr = x.allReduce(p.dKeys.get(), p.dKeys.get(), keyN, ncclInt64, ncclMin, g.comms[i], p.stream.get());
        }
        const ncclResult_t ne = x.groupEnd();  // always closes the group, also after a failed enqueue
        if (hr != hipSuccess)
            return fail(GMM_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(hr));
        GMM_NCCL_CHECK(nr);
        GMM_NCCL_CHECK(ne);
        reduced = g.parts[0].dKeys.get();  // part 0 is the first part on the lead device
    }
    else if (nS) {
        for (uint32_t i = 0; i < P; ++i) {
            DensityPart& p = g.parts[i];
            GMM_HIP_CHECK(hipSetDevice(p.device));
            GMM_HIP_CHECK(hipMemcpyPeerAsync(g.dGather.get() + i * keyN, g.lead, p.dKeys.get(), p.device, keyN * sizeof(int64_t), p.stream.get()));
        }
        reduced = g.dReduced.get();
    }
    // whole mixtures straight into the full table
    for (DensityPart& p : g.parts) {
        GMM_HIP_CHECK(hipSetDevice(p.device));
        const size_t rows = p.rowHi - p.rowLo;
        if (rows) {
            const size_t dst = static_cast<size_t>(p.shard.mixBegin + p.rowLo) * scoreStride, src = static_cast<size_t>(p.rowLo) * n;
            GMM_HIP_CHECK(hipMemcpy2DAsync(scores + dst, static_cast<size_t>(scoreStride) * 4, p.dScores.get() + src, static_cast<size_t>(n) * 4,
                                           static_cast<size_t>(n) * 4, rows, hipMemcpyDefault, p.stream.get()));
            if (withBest)
                GMM_HIP_CHECK(hipMemcpy2DAsync(best + dst, static_cast<size_t>(scoreStride) * 4, p.dBest.get() + src,
                                               static_cast<size_t>(n) * 4, static_cast<size_t>(n) * 4, rows, hipMemcpyDefault,
                                               p.stream.get()));
        }
        GMM_HIP_CHECK(hipEventRecord(p.done.get(), p.stream.get()));
    }
    GMM_HIP_CHECK(hipSetDevice(g.lead));
    for (DensityPart& p : g.parts)
        GMM_HIP_CHECK(hipStreamWaitEvent(stream, p.done.get(), 0));
    if (nS && g.exchange != GMM_EXCHANGE_RCCL)
        GMM_HIP_CHECK(launchMinShardKeys(g.dGather.get(), P, keyN, g.dReduced.get(), stream));
    for (size_t i = 0; i < nS; ++i) {
        const size_t row = static_cast<size_t>(g.split[i]) * scoreStride;
        GMM_HIP_CHECK(launchUnpackShardKeys(reduced + i * n, 1, n, scores + row, withBest ? best + row : nullptr, scoreStride,
                                            stream));
    }
    GMM_HIP_CHECK(hipEventRecord(g.finish.get(), stream));
    return GMM_OK;
}

// the handle whose prepared model answers model queries (quantization, launch info): a part's
const gmm_scorer* modelOf(const gmm_scorer* s) {
    if (s && s->group)
        for (const DensityPart& p : s->group->parts)
            if (p.scorer)
                return p.scorer.get();
    return s;
}

std::vector<gmm_scorer*> partsOf(gmm_scorer* s) {
    std::vector<gmm_scorer*> v;
    if (s->group)
        for (DensityPart& p : s->group->parts)
            if (p.scorer)
                v.push_back(p.scorer.get());
    return v;
}

void DensityGroupDelete::operator()(DensityGroup* g) const {
    delete g;
}

}  // namespace rasr_gmm

using namespace rasr_gmm;

namespace {
bool minReducible(gmm_scorer_type t) {
    return t == GMM_SIMD_DIAGONAL_MAXIMUM || t == GMM_DIAGONAL_MAXIMUM || t == GMM_BATCH_DIAGONAL_MAXIMUM_FLOAT ||
           t == GMM_BATCH_DIAGONAL_MAXIMUM_INT || t == GMM_BATCH_DIAGONAL_MAXIMUM_FAST;
}
}  // namespace

extern "C" {

int gmm_scorer_create_sharded(const gmm_mixture_set* ms, gmm_scorer_type type, const gmm_scorer_config* config,
                              const int* devices, uint32_t nDevices, int exchange, gmm_scorer** out) {
    if (!ms || !out || !devices || nDevices == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument or no devices");
    *out = nullptr;
    if (exchange != GMM_EXCHANGE_AUTO && exchange != GMM_EXCHANGE_RCCL && exchange != GMM_EXCHANGE_COPY)
        return fail(GMM_ERR_INVALID_ARGUMENT, "unknown exchange");
    gmm_scorer_config cfg;
    gmm_default_config(&cfg);
    if (config)
        cfg = *config;
    if (!minReducible(type))
        return fail(GMM_ERR_UNSUPPORTED, "density sharding combines split mixtures by a minimum: SIMD-diagonal-maximum, "
                                         "diagonal-maximum and batch-diagonal-maximum-* only");
    if (cfg.mixture_begin != 0 || cfg.mixture_end != 0)
        return fail(GMM_ERR_UNSUPPORTED, "a density-sharded handle shards the whole mixture set (mixture_begin/end 0)");
    if (!(cfg.score_scale > 0.0f))
        return fail(GMM_ERR_UNSUPPORTED, "density sharding needs a positive score scale (the minimum commutes with it)");
    if (cfg.max_frames == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "max_frames must be > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(GMM_ERR_DEVICE, "no HIP device available");
    for (uint32_t i = 0; i < nDevices; ++i)
        if (devices[i] < 0 || devices[i] >= ndev)
            return fail(GMM_ERR_INVALID_ARGUMENT, "device index out of range");
    if (nDevices == 1)  // the unsharded scorer itself
        return gmm_scorer_create(ms, type, &cfg, devices[0], out);

    std::vector<DensityShard> plan;
    std::string               err = planDensityShards(ms->mixture_offsets, ms->n_mixtures, nDevices, plan);
    if (!err.empty())
        return fail(GMM_ERR_INVALID_ARGUMENT, err);
    std::unique_ptr<DensityGroup> g(new DensityGroup);
    g->split = splitMixtures(plan);
    g->lead  = devices[0];
    // AUTO: RCCL when the parts span several GPUs and librccl opens, else the copy exchange (it needs no library);
    // only an explicit GMM_EXCHANGE_RCCL turns a missing RCCL into an error
    std::vector<int> gpus;
    for (uint32_t i = 0; i < nDevices; ++i)
        if (std::find(gpus.begin(), gpus.end(), devices[i]) == gpus.end())
            gpus.push_back(devices[i]);
    if (g->split.empty())
        g->exchange = GMM_EXCHANGE_AUTO;
    else if (exchange == GMM_EXCHANGE_AUTO)
        g->exchange = (gpus.size() > 1 && rccl().error.empty()) ? GMM_EXCHANGE_RCCL : GMM_EXCHANGE_COPY;
    else
        g->exchange = exchange;
    if (g->exchange == GMM_EXCHANGE_RCCL && !rccl().error.empty())
        return fail(GMM_ERR_UNSUPPORTED, "the RCCL exchange: " + rccl().error);
    const size_t maxF = cfg.max_frames, nS = g->split.size();
    const auto   isSplit = [&](uint32_t m) { return std::binary_search(g->split.begin(), g->split.end(), m); };
    g->parts.resize(nDevices);
    for (uint32_t r = 0; r < nDevices; ++r) {
        DensityPart& p = g->parts[r];
        p.device       = devices[r];
        p.shard        = plan[r];
        p.nLocal       = p.shard.mixEnd - p.shard.mixBegin;
        GMM_HIP_CHECK(hipSetDevice(p.device));
        GMM_HIP_CHECK(p.stream.create(hipStreamNonBlocking));
        GMM_HIP_CHECK(p.done.create(hipEventDisableTiming));
        if (p.nLocal) {
            // the part's sub-model: mixtures [mixBegin, mixEnd) cut to the entry range, the same densities, means
            // and covariances (so model-global preparation -- the quantization scale -- is the unsharded one)
            const uint32_t        mb = p.shard.mixBegin, eb = p.shard.entryBegin, ee = p.shard.entryEnd;
            std::vector<uint32_t> lo(p.nLocal + 1);
            for (uint32_t j = 0; j <= p.nLocal; ++j)
                lo[j] = std::min(std::max(ms->mixture_offsets[mb + j], eb), ee);
            lo[0] = std::max(eb, ms->mixture_offsets[mb]);
            const uint32_t base = lo[0];
            for (uint32_t& v : lo)
                v -= base;
            gmm_mixture_set sub     = *ms;
            sub.n_mixtures          = p.nLocal;
            sub.mixture_offsets     = lo.data();
            sub.mixture_densities   = ms->mixture_densities + base;
            sub.mixture_log_weights = ms->mixture_log_weights + base;
            gmm_scorer* part = nullptr;
            int         rc   = gmm_scorer_create(&sub, type, &cfg, p.device, &part);
            if (rc != GMM_OK)
                return rc;
            p.scorer.reset(part);
            GMM_HIP_CHECK(hipSetDevice(p.device));
            GMM_HIP_CHECK(p.dScores.alloc(p.nLocal * maxF));
            GMM_HIP_CHECK(p.dBest.alloc(p.nLocal * maxF));
            p.rowLo = isSplit(mb) ? 1 : 0;
            p.rowHi = isSplit(p.shard.mixEnd - 1) ? p.nLocal - 1 : p.nLocal;
            p.rowHi = std::max(p.rowHi, p.rowLo);
            std::vector<uint32_t> offsets;
            for (uint32_t i = 0; i < nS; ++i)
                if (g->split[i] >= mb && g->split[i] < p.shard.mixEnd) {
                    p.held.emplace_back(i, g->split[i] - mb);
                    offsets.push_back(g->split[i] == mb ? p.shard.firstOffset : 0);
                }
            if ((rc = upload(p.dHeldOffset, offsets)) != GMM_OK)
                return rc;
        }
        if (nS)
            GMM_HIP_CHECK(p.dKeys.alloc(nS * maxF));
        if (p.device != g->lead) {
            GMM_HIP_CHECK(p.dFrames.alloc(maxF * ms->dimension));
            // xGMI peer access both ways: frames out of the lead, tables and keys into it
            int can = 0;
            GMM_HIP_CHECK(hipDeviceCanAccessPeer(&can, g->lead, p.device));
            if (!can)
                return fail(GMM_ERR_UNSUPPORTED, "devices without peer access");
            for (int a : {g->lead, p.device}) {
                GMM_HIP_CHECK(hipSetDevice(a));
                const hipError_t e = hipDeviceEnablePeerAccess(a == g->lead ? p.device : g->lead, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                    return fail(GMM_ERR_DEVICE, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
                (void)hipGetLastError();
            }
        }
    }
    if (g->exchange == GMM_EXCHANGE_RCCL) {
        // one rank per GPU: the first part on each GPU; the others fold their keys into it first
        for (int d : gpus)
            for (uint32_t r = 0; r < nDevices; ++r)
                if (devices[r] == d) {
                    g->ranks.push_back(r);
                    for (uint32_t f = r + 1; f < nDevices; ++f)
                        if (devices[f] == d) {
                            g->parts[r].fold.push_back(f);
                            GMM_HIP_CHECK(hipSetDevice(d));
                            GMM_HIP_CHECK(g->parts[f].keysReady.create(hipEventDisableTiming));
                        }
                    break;
                }
        g->comms.assign(gpus.size(), nullptr);
        GMM_NCCL_CHECK(rccl().commInitAll(g->comms.data(), static_cast<int>(gpus.size()), gpus.data()));
    }
    GMM_HIP_CHECK(hipSetDevice(g->lead));
    if (g->exchange == GMM_EXCHANGE_COPY) {
        GMM_HIP_CHECK(g->dGather.alloc(nDevices * nS * maxF));
        GMM_HIP_CHECK(g->dReduced.alloc(nS * maxF));
    }
    GMM_HIP_CHECK(g->start.create(hipEventDisableTiming));
    GMM_HIP_CHECK(g->finish.create(hipEventDisableTiming));

    // the handle: no model of its own (modelOf answers for it); the full table's size
    bool ok       = false;
    auto s        = std::make_unique<gmm_scorer>();
    s->type       = type;
    s->flavor     = flavorOf(type, &ok);
    s->device     = g->lead;
    s->cfg        = cfg;
    s->cfg.cache_archive = nullptr;  // valid only during create (the parts took their copies)
    s->D          = ms->dimension;
    s->C          = ms->n_covariances;
    s->nMix       = ms->n_mixtures;
    s->plan       = kernelPlanOf(*s);
    s->nFramesPad = paddedFrames(s->plan, cfg.max_frames);
    for (const DensityPart& p : g->parts)  // gmm_scorer_spread_bound: the largest of the parts
        if (p.scorer && !(p.scorer->spreadPredicted <= s->spreadPredicted))
            s->spreadStat = p.scorer->spreadStat, s->spreadPredicted = p.scorer->spreadPredicted;
    s->group.reset(g.release());
    *out = s.release();
    return GMM_OK;
}

int gmm_scorer_shard_info(const gmm_scorer* s, uint32_t* nParts, int* exchange) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    if (nParts)
        *nParts = s->group ? static_cast<uint32_t>(s->group->parts.size()) : 1u;
    if (exchange)
        *exchange = s->group ? s->group->exchange : GMM_EXCHANGE_AUTO;
    return GMM_OK;
}

}  // extern "C"
