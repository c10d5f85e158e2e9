// gmm_score.cc -- one scoring call: the kernel choice, the chunk table, and per family the frame preparation and
// the scorer launch.  gmm_score_device enqueues two kernels on the caller's stream: the frame preparation
// (quantize / scale the feature vectors, the per-frame Context of the reference, SimdFeatureScorer.cc:22-35) and
// the scorer.  No host synchronisation, no allocation on that path.
#include <algorithm>
#include <cstdlib>

#include "gmm_scorer.hh"

namespace rasr_gmm {

// ---- the kernel choice (kernelPlanOf at creation, planFor per call).  The answer fixes the frame tile, hence nFrameTiles, the grid and the rows of the frame
// tables (paddedFrames); the launchers are told the kernel and do not choose again. ----

KernelPlan kernelPlanOf(const gmm_scorer& s) {
    const bool presel = isPreselection(s.type);
    KernelPlan p;
    p.launches = presel ? 3 : 2;
    if (const auto* q = s.quantized()) {
        p.kernel = presel ? Kernel::I8Presel : (q->scoreOnly == kScoreOnlySlots ? Kernel::I8Cls : Kernel::I8Seg);
        p.framesPerBlock = presel ? kI8PreselFramesPerBlock
                                  : (p.kernel == Kernel::I8Cls ? kI8ClsFramesPerBlock : kI8FramesPerBlock);
        p.smallTiles     = !presel;
        p.name           = "scoreI8";
    }
    else if (std::holds_alternative<DirectModel>(s.model))
        p = {Kernel::Direct, kDirectFramesPerBlock, false, p.launches, "scoreDirect"};
    else if (const auto* m = std::get_if<SplitModel>(&s.model)) {
        const bool     rows32 = m->splitRows == 32;
        const uint32_t wide   = splitWideFrames(m->kSteps16);
        p.framesPerBlock      = kSplitFramesPerBlock;
        if (s.flavor == Flavor::DiagonalSum)
            p.kernel = rows32 ? Kernel::Split32Sum : Kernel::SplitSum, p.name = rows32 ? "scoreSplit32Sum" : "scoreSplitSum";
        else if (rows32)
            p.kernel = Kernel::Split32, p.name = "scoreSplit32";
        else if (presel)
            p.kernel = Kernel::SplitPresel, p.name = "scoreSplit";
        else if (wide != 0)
            p.kernel = Kernel::SplitWide, p.framesPerBlock = wide, p.name = "scoreSplitWide";
        else
            p.kernel = Kernel::SplitPair, p.name = "scoreSplit";
    }
    else if (std::holds_alternative<std::monostate>(s.model) && isQuantized(s.flavor))
        p = {Kernel::I8Seg, kI8FramesPerBlock, false, p.launches, "scoreI8"};  // a sharded handle without mixtures
    return p;
}

uint32_t paddedFrames(const KernelPlan& plan, uint32_t maxFrames) {
    const auto roundUp = [](uint32_t n, uint32_t q) { return (n + q - 1) / q * q; };
    // scoreI8Cls workgroups of kI8ClsFramesPerBlock frames: the frame tables hold whole workgroups
    if (plan.kernel == Kernel::I8Cls && plan.framesPerBlock > kFramePadQuantum)
        return roundUp(maxFrames, plan.framesPerBlock);
    return roundUp(maxFrames, kFramePadQuantum);
}

// the frame tile of one call: the quantized kernels take 256-frame tiles for calls of up to 256 frames and
// 64-frame ones (one wave per workgroup, one covariance) for calls of up to 64 (I8Args::smallTile)
LaunchPlan planFor(const gmm_scorer& s, uint32_t nFrames) {
    LaunchPlan p{s.plan.kernel, s.plan.framesPerBlock, 0, 0, 0};
    if (s.plan.smallTiles && nFrames <= kI8SmallFrames) {
        p.smallTile      = nFrames <= kI8TinyFrames && !s.multiCov() ? 2 : 1;
        p.framesPerBlock = p.smallTile == 2 ? kI8TinyFrames : kI8SmallFrames;
    }
    p.nFrameTiles = (nFrames + p.framesPerBlock - 1) / p.framesPerBlock;
    p.nFramesRead = p.nFrameTiles * p.framesPerBlock;
    return p;
}

int waitAsync(gmm_scorer* s) {
    if (!s->host.asyncCall)
        return GMM_OK;
    s->host.asyncCall  = 0;
    const hipError_t e = hipEventSynchronize(s->host.asyncDone.get());
    if (e != hipSuccess)
        return fail(GMM_ERR_DEVICE, std::string("hipEventSynchronize (GMM_HOST_ASYNC call): ") + hipGetErrorString(e));
    return GMM_OK;
}

namespace {

// scoreSplitWide: the chunks of the table `off` by kernel form (ChunkTable::Part), in the order of their tile counts.
// The mixtures keep their order and their chunks; a model whose chunks all take one form gets one part without a list
int splitWideParts(const gmm_scorer& s, const std::vector<uint32_t>& off, ChunkTable& ct) {
    const auto*    model   = std::get_if<SplitModel>(&s.model);
    const bool     generic = (s.cfg.flags & GMM_FLAG_SPLIT_WIDE_GENERIC) != 0 || !model;
    std::map<uint32_t, std::vector<uint32_t>> byT;  // uniform tile count (0: none) -> chunks
    for (uint32_t c = 0; c + 1 < off.size(); ++c) {
        uint32_t T = generic ? 0u : s.mixTileOff[off[c] + 1] - s.mixTileOff[off[c]];
        for (uint32_t m = off[c]; T != 0 && m < off[c + 1]; ++m)
            if (s.mixTileOff[m + 1] - s.mixTileOff[m] != T)
                T = 0;
        if (T != 0 && !splitWideUniformT(model->kSteps16, T))
            T = 0;
        byT[T].push_back(c);
    }
    for (auto& [T, list] : byT) {
        ChunkTable::Part part;
        part.uniformT = T;
        part.nChunks  = static_cast<uint32_t>(list.size());
        if (byT.size() > 1) {
            const int rc = upload(part.dList, list);
            if (rc != GMM_OK)
                return rc;
        }
        ct.parts.push_back(std::move(part));
    }
    return GMM_OK;
}

// Cut the shard's mixtures into chunks of about equal tile count so that
// chunks x frame-tiles gives enough workgroups to fill 256 CUs several times.
int chunkTableFor(gmm_scorer* s, uint32_t nFrameTiles, const ChunkTable** out) {
    auto it = s->chunks.find(nFrameTiles);
    if (it != s->chunks.end()) {
        *out = &it->second;
        return GMM_OK;
    }
#ifndef GMM_TARGET_BLOCKS
#define GMM_TARGET_BLOCKS 8192
#endif
#ifndef GMM_SPLIT_TARGET_BLOCKS
// the split kernels' cap: fewer, longer chunks reload a wave's 128 frame operands less often (A/B at 32768 frames:
// 2048 -> 4.653 ms, 4096 -> 4.700, 8192 -> 4.753; at 8192 frames 1.299 / 1.309 / 1.318, profiles/r04/s13)
#define GMM_SPLIT_TARGET_BLOCKS 2048
#endif
    // RASR_GMM_TARGET_BLOCKS: tuning override (scripts/sweep_chunks.sh, scripts/sweep_small_batches.sh)
    static const uint32_t kOverride = [] {
        const char* e = std::getenv("RASR_GMM_TARGET_BLOCKS");
        const long  v = e ? std::strtol(e, nullptr, 10) : 0;
        return v > 0 ? static_cast<uint32_t>(v) : 0u;
    }();
    // Small calls (few frame tiles) with many one-mixture chunks reload the frame operands once per mixture:
    // fewer, larger chunks there (measured, profiles/r03/sweep_small_batches.txt: split kernel at 256 frames
    // 0.048 ms with 1024 blocks vs 0.063 with 8192, at 1024 frames 0.160 vs 0.175; quantized kernel at 1024
    // frames 0.0695 with 2048 vs 0.0729); large calls keep GMM_TARGET_BLOCKS
    const Kernel   k       = s->plan.kernel;
    const uint32_t kTargetBlocks =
            s->chunkTarget ? s->chunkTarget  // gmm_scorer_set_chunk_target
            : kOverride    ? kOverride
            : isSplitKernel(k) ? std::clamp<uint32_t>(nFrameTiles * 256u, 1024u,
                                             k == Kernel::SplitSum ? uint32_t(GMM_TARGET_BLOCKS)           // 64-frame waves: 8192 (A/B)
                                                                   : uint32_t(GMM_SPLIT_TARGET_BLOCKS))
            : k == Kernel::I8Seg || k == Kernel::I8Cls ? std::clamp<uint32_t>(nFrameTiles * 1024u, 2048u, uint32_t(GMM_TARGET_BLOCKS))
                                                       : uint32_t(GMM_TARGET_BLOCKS);
    uint32_t target = std::max<uint32_t>(1, (kTargetBlocks + nFrameTiles - 1) / nFrameTiles);
    // whole rounds of the 8 XCDs: mapBlock gives XCD x the chunks x, x + 8, ..., so a count just past a multiple of 8
    // leaves most XCDs idle for the last chunk (12 chunks of 171 192-frame tiles: 7.59 ms against 5.51 for 16 chunks
    // of 128 256-frame tiles at D = 45, profiles/r05/s15)
    if (target > 8)
        target = (target + 7u) / 8u * 8u;
    target                  = std::min<uint32_t>(target, std::max<uint32_t>(1, s->nMix));
    uint32_t perChunk = std::max<uint32_t>(1, (s->nTiles + target - 1) / target);
    // scoreSplitWide: a chunk's tiles within its 32-bit byte offsets (more, shorter chunks where a model is that large)
    const uint32_t chunkCap = k == Kernel::SplitWide ? kSplitWideChunkTiles : 0xffffffffu;
    perChunk                = std::min(perChunk, chunkCap / 2u);
    std::vector<uint32_t> off{0};
    uint32_t              acc = 0;
    for (uint32_t m = 0; m < s->nMix; ++m) {
        acc += s->mixTileOff[m + 1] - s->mixTileOff[m];
        if (acc > chunkCap)  // one mixture of more than half the cap
            return fail(GMM_ERR_CAPACITY, "a mixture has more tiles than a scoreSplitWide chunk can address");
        if (acc >= perChunk && m + 1 < s->nMix) {
            off.push_back(m + 1);
            acc = 0;
        }
    }
    off.push_back(s->nMix);
    ChunkTable ct;
    ct.nChunks = static_cast<uint32_t>(off.size() - 1);
    int rc     = upload(ct.dMixOff, off);
    if (rc != GMM_OK)
        return rc;
    if (k == Kernel::SplitWide && (rc = splitWideParts(*s, off, ct)) != GMM_OK)
        return rc;
    *out = &s->chunks.emplace(nFrameTiles, std::move(ct)).first->second;
    return GMM_OK;
}

// HIP events around the scorer kernel, on the kernel's own stream (bench.py roofline timing).
struct TimedSpan {
    gmm_scorer* s;
    hipStream_t stream;
    hipEvent_t  e = nullptr;
    hipError_t begin() {
        if (!s->timing)
            return hipSuccess;
        if (s->eventsUsed == s->events.size()) {
            std::pair<Event, Event> ev;
            hipError_t              err = ev.first.create();
            if (err != hipSuccess || (err = ev.second.create()) != hipSuccess)
                return err;
            s->events.push_back(std::move(ev));
        }
        e = s->events[s->eventsUsed].second.get();
        return hipEventRecord(s->events[s->eventsUsed++].first.get(), stream);
    }
    hipError_t end() { return s->timing ? hipEventRecord(e, stream) : hipSuccess; }
};

// one call, as every family sees it
struct Call {
    const float*      frames;
    uint32_t          nFrames, frameStride;
    float*            scores;
    uint32_t*         best;
    uint32_t          scoreStride;
    hipStream_t       stream;
    LaunchPlan        plan;
    const ChunkTable* ct;
};

// the selection of every frame of the call: mask words for whole 64-frame blocks (padding frames too)
int selectClusters(gmm_scorer* s, const Call& c) {
    Preselection& p = *s->presel;
    GMM_HIP_CHECK(launchSelectClusters(isQuantized(s->flavor), c.frames, c.nFrames, c.frameStride, c.plan.nFramesRead, s->D,
                                       p.clustering.paddedDimension, s->dIsv.get(), p.dClusterMeans.get(),
                                       p.clustering.nClusters, p.clustering.nSelected, p.dSelT.get(), c.stream));
    if (p.dSelC)  // the quantized kernel's per-wave tables
        GMM_HIP_CHECK(launchCompactSelection(p.dSelT.get(), c.plan.nFramesRead, p.clustering.nClusters, p.dSelC.get(),
                                             c.stream));
    p.lastFrames = c.nFrames;
    return GMM_OK;
}

// what the families' *Args share: the caller's tables, the call's geometry, the CSR offsets
template <class Args>
Args argsOf(const gmm_scorer& s, const Call& c) {
    Args a{};
    if constexpr (std::is_same_v<Args, DirectArgs>)
        a.mixOff = s.dMixTileOff.get();
    else {
        a.mixTileOff = s.dMixTileOff.get();
        a.nFramesPad = s.nFramesPad;
        a.mixBase    = 0;
    }
    a.chunkMixOff = c.ct->dMixOff.get();
    a.scores      = c.scores;
    a.nFrames     = c.nFrames;
    a.scoreStride = c.scoreStride;
    a.nChunks     = c.ct->nChunks;
    a.nFrameTiles = c.plan.nFrameTiles;
    a.outScale    = s.cfg.score_scale;
    return a;
}

// ---- per family: prepareFrames (the frame-side operands of the call) and launch (its *Args, its scorer) ----

hipError_t prepareFrames(const gmm_scorer& s, const QuantizedModel& m, const Call& c) {
    return launchPrepareFramesI8(c.frames, c.nFrames, c.frameStride, s.nFramesPad, c.plan.nFramesRead, s.D, s.C, m.kSteps,
                                 s.dIsv.get(), m.dFrameQ.get(), m.dFrameSS.get(), c.stream);
}

hipError_t launch(const gmm_scorer& s, const QuantizedModel& m, const Call& c) {
    const bool simd = s.flavor == Flavor::Simd;
    I8Args     a = argsOf<I8Args>(s, c);
    a.tileA       = m.dTileA.get();
    a.tileP       = m.dTileP.get();
    a.tileCov     = m.dTileCov.get();
    a.frameQ      = m.dFrameQ.get();
    a.frameSS     = m.dFrameSS.get();
    a.best        = simd ? c.best : nullptr;
    a.idxBits     = m.idxBits;
    a.flavor      = simd ? 0 : 1;
    a.s2          = m.scalingSquared;
    // finalize by multiplication and two corrections (gmm_kernels_i8.hip finalizeStoreI8): b = 2 s^2 (the SIMD
    // scorer's 0.5 / s2, the batch scorers' scale_, both exactly 2 s2 in f32) and RN(1 / b) by IEEE division;
    // scales far outside a real model's range keep the division
    a.finB       = simd ? 2.0f * m.scalingSquared : m.batchScale;
    a.finInv     = 1.0f / a.finB;
    a.finInvLo   = static_cast<float>(1.0 / static_cast<double>(a.finB) - static_cast<double>(a.finInv));
    a.finDivide  = (a.finB >= 1e-30f && a.finB <= 1e30f) ? 0 : 1;
    a.batchScale = m.batchScale;
    a.presel     = c.plan.kernel == Kernel::I8Presel ? 1 : 0;
    if (s.presel) {
        a.selT      = s.presel->dSelT.get();
        a.selC      = s.presel->dSelC.get();
        a.tileClu   = s.presel->dTileClu.get();
        a.nClusters = s.presel->clustering.nClusters;
    }
    a.mixOddMask = m.dMixOddMask.get();
    a.scoreOnly  = m.scoreOnly;
    a.smallTile  = c.plan.smallTile;
    return launchScoreI8(a, m.kSteps, s.multiCov(), c.stream);
}

hipError_t prepareFrames(const gmm_scorer&, const DirectModel&, const Call&) {
    return hipSuccess;  // the kernel reads the caller's frames
}

hipError_t launch(const gmm_scorer& s, const DirectModel& m, const Call& c) {
    DirectArgs a = argsOf<DirectArgs>(s, c);
    a.mean        = m.dMean.get();
    a.isv         = s.dIsv.get();
    a.entryCov    = m.dCov.get();
    a.constant    = m.dConst.get();
    a.logNorm     = m.dLogNorm.get();
    a.frames      = c.frames;
    a.best        = s.flavor == Flavor::DiagonalMaximum ? c.best : nullptr;
    a.frameStride = c.frameStride;
    a.D           = s.D;
    a.Dp          = m.L;
    a.batch       = s.flavor == Flavor::BatchFloat ? 1 : 0;
    a.multiCov    = s.multiCov() ? 1 : 0;
    return launchScoreDirect(a, c.stream);
}

hipError_t prepareFrames(const gmm_scorer& s, const SplitModel& m, const Call& c) {
    if (m.splitCov)
        return launchPrepareFramesSplitCov(c.frames, c.nFrames, c.frameStride, c.plan.nFramesRead, s.D, m.kSteps16,
                                           m.dCentre.get(), m.dDimScale.get(), m.dLimbExp.get(), m.dFrameH.get(),
                                           m.dFrameExp.get(), c.stream);
    return launchPrepareFramesSplit(c.frames, c.nFrames, c.frameStride, c.plan.nFramesRead, s.D, m.splitRows, m.kSteps16,
                                    s.dIsv.get(), m.dCentre.get(), m.dDimScale.get(), m.dLimbExp.get(), m.dFrameH.get(),
                                    m.dFrameXX.get(), m.dFrameExp.get(), c.stream);
}

hipError_t launch(const gmm_scorer& s, const SplitModel& m, const Call& c) {
    SplitArgs a = argsOf<SplitArgs>(s, c);
    a.tileH       = m.dTileH.get();
    a.frameH      = m.dFrameH.get();
    a.frameXX     = m.dFrameXX.get();
    a.frameExp    = m.dFrameExp.get();
    a.best        = s.flavor != Flavor::BatchFloat ? c.best : nullptr;
    a.flavor      = s.flavor == Flavor::DiagonalMaximum ? 2 : (s.flavor == Flavor::DiagonalSum ? 4 : 3);
    a.tileBits    = m.keyBits;
    a.offsetK0    = m.offsetK0;
    a.presel      = c.plan.kernel == Kernel::SplitPresel ? 1 : 0;
    if (s.presel) {
        a.selT      = s.presel->dSelT.get();
        a.tileClu   = s.presel->dTileClu.get();
        a.nClusters = s.presel->clustering.nClusters;
    }
    a.backoff = s.cfg.backoff_score;
    if (c.ct->parts.empty())
        return launchScoreSplit(a, c.plan.kernel, m.kSteps16, c.stream);
    for (const ChunkTable::Part& part : c.ct->parts) {  // scoreSplitWide: its forms, each over its own chunks
        a.nChunks   = part.nChunks;
        a.chunkList = part.dList.get();
        a.uniformT  = part.uniformT;
        const hipError_t e = launchScoreSplit(a, c.plan.kernel, m.kSteps16, c.stream);
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

hipError_t prepareFrames(const gmm_scorer& s, const F32Model& m, const Call& c) {
    return launchPrepareFramesF32(c.frames, c.nFrames, c.frameStride, s.nFramesPad, c.plan.nFramesRead, s.D, s.C, m.kSteps,
                                  m.foldNorm ? 1 : 0, s.dIsv.get(), m.dCentre.get(), m.dFrameX.get(), m.dFrameXX.get(),
                                  c.stream);
}

hipError_t launch(const gmm_scorer& s, const F32Model& m, const Call& c) {
    F32Args a = argsOf<F32Args>(s, c);
    a.tileA       = static_cast<const float*>(m.dTileA.get());
    a.tileCov     = m.dTileCov.get();
    a.rowDns      = m.dRowDns.get();
    a.frameX      = m.dFrameX.get();
    a.frameXX     = m.dFrameXX.get();
    a.best        = s.flavor == Flavor::DiagonalMaximum ? c.best : nullptr;
    a.flavor      = s.flavor == Flavor::DiagonalMaximum ? 2 : 3;
    a.tileBits    = m.tileBits;
    a.offsetK0    = m.offsetK0;
    return launchScoreF32(a, m.kSteps, s.multiCov(), c.stream);
}

// a handle without a model never gets here (nMix == 0, or its group scores)
hipError_t prepareFrames(const gmm_scorer&, std::monostate, const Call&) { return hipErrorInvalidValue; }
hipError_t launch(const gmm_scorer&, std::monostate, const Call&) { return hipErrorInvalidValue; }

}  // namespace

int scoreImpl(gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride, float* scores,
              uint32_t* best, uint32_t scoreStride, hipStream_t stream) {
    if (nFrames == 0 || s->nMix == 0)
        return GMM_OK;
    if (nFrames > s->cfg.max_frames)
        return fail(GMM_ERR_CAPACITY, "n_frames exceeds config.max_frames");
    if (!frames || !scores || frameStride < s->D || scoreStride < nFrames)
        return fail(GMM_ERR_INVALID_ARGUMENT, "invalid frames/scores/stride");
    GMM_HIP_CHECK(hipSetDevice(s->device));
    if (s->group)
        return groupScore(s, frames, nFrames, frameStride, scores, best, scoreStride, stream);
    if (!best && s->scoresOnly)
        return scoreImpl(s->scoresOnly.get(), frames, nFrames, frameStride, scores, nullptr, scoreStride, stream);
    Call c{frames, nFrames, frameStride, scores, best, scoreStride, stream, planFor(*s, nFrames), nullptr};
    int  rc = chunkTableFor(s, c.plan.nFrameTiles, &c.ct);
    if (rc != GMM_OK)
        return rc;
    if (s->presel && (rc = selectClusters(s, c)) != GMM_OK)
        return rc;
    GMM_HIP_CHECK(std::visit([&](const auto& m) { return prepareFrames(*s, m, c); }, s->model));
    TimedSpan span{s, stream};
    GMM_HIP_CHECK(span.begin());
    GMM_HIP_CHECK(std::visit([&](const auto& m) { return launch(*s, m, c); }, s->model));
    GMM_HIP_CHECK(span.end());
    return GMM_OK;
}

}  // namespace rasr_gmm

using namespace rasr_gmm;

extern "C" {

int gmm_score_device(gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride, float* scores,
                     uint32_t* best, uint32_t scoreStride, void* stream) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    const int wrc = waitAsync(s);  // a GMM_HOST_ASYNC call still uses the frame staging
    if (wrc != GMM_OK)
        return wrc;
    return scoreImpl(s, frames, nFrames, frameStride, scores, best, scoreStride, static_cast<hipStream_t>(stream));
}

int gmm_scorer_launch_info(const gmm_scorer* s, uint32_t nFrames, uint32_t* nLaunches, const char** name) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    s = modelOf(s);  // a sharded handle: per part
    if (nLaunches) {
        // a scoreSplitWide model of uniform and other chunks: a scorer launch per kernel form (known once a call
        // of that many frame tiles has built the chunk table)
        const auto it = s->chunks.find(planFor(*s, std::max(nFrames, 1u)).nFrameTiles);
        const size_t parts = it != s->chunks.end() ? it->second.parts.size() : 0;
        *nLaunches = s->plan.launches + static_cast<uint32_t>(parts > 1 ? parts - 1 : 0);
    }
    if (name)
        *name = s->plan.name;
    return GMM_OK;
}

int gmm_scorer_set_chunk_target(gmm_scorer* s, uint32_t targetBlocks) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    const int wrc = waitAsync(s);
    if (wrc != GMM_OK)
        return wrc;
    for (gmm_scorer* p : s->group ? partsOf(s) : std::vector<gmm_scorer*>{s}) {
        GMM_HIP_CHECK(hipSetDevice(p->device));
        GMM_HIP_CHECK(hipDeviceSynchronize());  // no call in flight reads the tables this drops
        p->chunkTarget = targetBlocks;
        p->chunks.clear();
    }
    return GMM_OK;
}

int gmm_scorer_chunk_forms(gmm_scorer* s, uint32_t nFrames, uint32_t* nUniform, uint32_t* nGeneric) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    uint32_t uniform = 0, generic = 0;
    for (gmm_scorer* p : s->group ? partsOf(s) : std::vector<gmm_scorer*>{s}) {
        if (p->nMix == 0)
            continue;
        GMM_HIP_CHECK(hipSetDevice(p->device));
        const ChunkTable* ct = nullptr;
        const int         rc = chunkTableFor(p, planFor(*p, std::max(nFrames, 1u)).nFrameTiles, &ct);
        if (rc != GMM_OK)
            return rc;
        if (ct->parts.empty())
            generic += ct->nChunks;
        for (const ChunkTable::Part& part : ct->parts)
            (part.uniformT ? uniform : generic) += part.nChunks;
    }
    if (nUniform)
        *nUniform = uniform;
    if (nGeneric)
        *nGeneric = generic;
    return GMM_OK;
}

int gmm_scorer_k_steps(const gmm_scorer* s, uint32_t* kSteps) {
    if (!s || !kSteps)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer or output");
    s = modelOf(s);  // a sharded handle: per part
    if (const auto* q = s->quantized())
        *kSteps = q->kSteps;
    else if (const auto* m = std::get_if<SplitModel>(&s->model))
        *kSteps = m->kSteps16;
    else if (const auto* f = std::get_if<F32Model>(&s->model))
        *kSteps = f->kSteps;
    else if (const auto* d = std::get_if<DirectModel>(&s->model))
        *kSteps = (d->L - 4u) / 4u;  // L = 4 nb + 4 (directBlocks)
    else
        return fail(GMM_ERR_UNSUPPORTED, "the handle holds no model");
    return GMM_OK;
}

}  // extern "C"
