// gmm_hostcall.cc -- the host-buffer calls of include/rasr_gmm.h: gmm_score_host / gmm_score_host_ring (the
// chunked copy-out pipeline and the one-stream small-call path), the best densities a call kept
// (gmm_fetch_best_density) and the sparse (frame, mixture) pairs (gmm_best_density_pairs*).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gmm_scorer.hh"

using namespace rasr_gmm;

namespace {

// gmm_score_host / gmm_score_host_ring.  The caller's frames are the rows ring[(first + i) % ringSize],
// i < nFrames, and the scores of call frame i go to column (first + i) % ringSize of the caller's
// [nMix][scoreStride] tables (gmm_score_host: ringSize = nFrames, first = 0).  The frames are scored on
// hostCompute in frame chunks (one chunk for small tables); the copy-out of chunk k on hostCopy overlaps
// the scoring of chunk k+1.  A chunk that straddles the ring's wrap is copied out as two segments, so every
// copy has contiguous destination columns.  A pinned destination is written by the DMA engines directly;
// a pageable one goes through a pinned double-buffered staging ring: the D2H of piece j+1 is in flight
// while the copy threads move piece j into the caller's rows (the runtime's own pageable path is one
// thread, ~10 GB/s).  With GMM_HOST_KEEP_BEST the best densities stay in dHostBest (no copy) for
// gmm_fetch_best_density.
constexpr size_t   kHostPipelineBytes = size_t(8) << 20;
constexpr uint32_t kHostChunkFrames   = 8192;
constexpr uint32_t kHostMaxChunks     = 8;
constexpr size_t   kHostStageBytes    = size_t(16) << 20;

int ensureHostPipeline(gmm_scorer* s, uint32_t nChunks) {
    HostPipeline& h = s->host;
    if (!h.compute) {
        GMM_HIP_CHECK(h.compute.create(hipStreamNonBlocking));
        GMM_HIP_CHECK(h.copy.create(hipStreamNonBlocking));
        GMM_HIP_CHECK(h.start.create(hipEventDisableTiming));
        for (Event& ev : h.stageDone)
            GMM_HIP_CHECK(ev.create(hipEventDisableTiming));
    }
    while (h.chunkDone.size() < nChunks) {
        Event ev;
        GMM_HIP_CHECK(ev.create(hipEventDisableTiming));
        h.chunkDone.push_back(std::move(ev));
    }
    return GMM_OK;
}

int ensureHostStage(gmm_scorer* s, size_t rowBytes) {
    const size_t want = std::max(kHostStageBytes, rowBytes);
    if (s->host.hStageBytes >= want)
        return GMM_OK;
    GMM_HIP_CHECK(s->host.hStage.reset());
    s->host.hStageBytes = 0;
    GMM_HIP_CHECK(s->host.hStage.alloc(2 * want, hipHostMallocDefault));
    s->host.hStageBytes = want;
    if (!s->host.copyPool)
        s->host.copyPool.reset(new HostCopyPool(hostCopyThreads()));
    return GMM_OK;
}

// the call's frame range [t0, t0 + n) of chunk k, cut at the ring's wrap
void appendSegments(const HostRing& r, uint32_t k, uint32_t t0, uint32_t n, std::vector<HostSegment>& out) {
    const uint32_t wrap = r.ringSize - r.first;  // call frame that lands in column 0
    if (t0 < wrap && t0 + n > wrap) {
        out.push_back(HostSegment{k, t0, wrap - t0, r.first + t0});
        out.push_back(HostSegment{k, wrap, t0 + n - wrap, 0});
    }
    else
        out.push_back(HostSegment{k, t0, n, t0 < wrap ? r.first + t0 : t0 - wrap});
}

// device tables -> caller tables at the segments' ring positions, on hostCopy after each segment's chunk;
// synchronizes hostCopy.  Mixture-major: the device tables [nMix][nFrames] (dHostScores, dHostBest) into
// columns of [nMix][scoreStride]; frame-major: their transposes [nFrames][nMix] (dHostScoresT, dHostBestT)
// into rows of [ringSize][scoreStride].
int copyOutTables(gmm_scorer* s, const std::vector<HostSegment>& segs, uint32_t nFrames, bool frameMajor, float* scores,
                  uint32_t* best, uint32_t scoreStride, bool async = false) {
    struct Table {
        char*       dst;
        const char* src;
    };
    struct Copy {  // one 2D copy: `height` rows of `width` bytes
        uint32_t    chunk;
        const char* src;
        size_t      sPitch;
        char*       dst;
        size_t      dPitch, width, height;
    };
    const char* srcS = reinterpret_cast<const char*>(frameMajor ? s->host.dScoresT.get() : s->host.dScores.get());
    const char* srcB = reinterpret_cast<const char*>(frameMajor ? s->host.dBestT.get() : s->host.dBest.get());
    std::vector<Copy> direct, staged;
    const size_t      M = s->nMix, dPitch = static_cast<size_t>(scoreStride) * 4;
    for (Table t : {Table{reinterpret_cast<char*>(scores), srcS}, Table{reinterpret_cast<char*>(best), srcB}}) {
        if (!t.dst)
            continue;
        const bool pinned = isPinnedHost(t.dst);
        for (const HostSegment& g : segs) {
            const Copy c = frameMajor ? Copy{g.chunk, t.src + static_cast<size_t>(g.t0) * M * 4, M * 4,
                                             t.dst + static_cast<size_t>(g.col) * dPitch, dPitch, M * 4, g.n}
                                      : Copy{g.chunk, t.src + static_cast<size_t>(g.t0) * 4, static_cast<size_t>(nFrames) * 4,
                                             t.dst + static_cast<size_t>(g.col) * 4, dPitch, static_cast<size_t>(g.n) * 4, M};
            if (c.width && c.height)
                (pinned ? direct : staged).push_back(c);
        }
    }
    for (size_t i = 0; i < direct.size(); ++i) {
        const Copy& c = direct[i];
        if (i == 0 || direct[i - 1].chunk != c.chunk)
            GMM_HIP_CHECK(hipStreamWaitEvent(s->host.copy.get(), s->host.chunkDone[c.chunk].get(), 0));
        GMM_HIP_CHECK(hipMemcpy2DAsync(c.dst, c.dPitch, c.src, c.sPitch, c.width, c.height, hipMemcpyDeviceToHost, s->host.copy.get()));
    }
    if (!staged.empty()) {
        size_t maxW = 4;
        for (const Copy& c : staged)
            maxW = std::max(maxW, c.width);
        int rc;
        if ((rc = ensureHostStage(s, maxW)) != GMM_OK)
            return rc;
        struct Piece {
            Copy   c;
            size_t r0, r1;
        };
        std::vector<Piece> pieces;
        for (const Copy& c : staged) {
            const size_t rows = std::max<size_t>(1, s->host.hStageBytes / c.width);
            for (size_t r0 = 0; r0 < c.height; r0 += rows)
                pieces.push_back(Piece{c, r0, std::min(c.height, r0 + rows)});
        }
        char* stage[2] = {s->host.hStage.get(), s->host.hStage.get() + s->host.hStageBytes};
        auto  issue    = [&](size_t j) -> int {
            const Piece& p = pieces[j];
            if (j == 0 || pieces[j - 1].c.chunk != p.c.chunk)
                GMM_HIP_CHECK(hipStreamWaitEvent(s->host.copy.get(), s->host.chunkDone[p.c.chunk].get(), 0));
            GMM_HIP_CHECK(hipMemcpy2DAsync(stage[j & 1], p.c.width, p.c.src + p.r0 * p.c.sPitch, p.c.sPitch, p.c.width,
                                           p.r1 - p.r0, hipMemcpyDeviceToHost, s->host.copy.get()));
            GMM_HIP_CHECK(hipEventRecord(s->host.stageDone[j & 1].get(), s->host.copy.get()));
            return GMM_OK;
        };
        if ((rc = issue(0)) != GMM_OK)
            return rc;
        for (size_t j = 0; j < pieces.size(); ++j) {
            // stage[(j+1)&1] was drained by the host copy of piece j-1 (synchronous, below)
            if (j + 1 < pieces.size() && (rc = issue(j + 1)) != GMM_OK)
                return rc;
            GMM_HIP_CHECK(hipEventSynchronize(s->host.stageDone[j & 1].get()));
            const Piece& p   = pieces[j];
            const char*  src = stage[j & 1];
            s->host.copyPool->parallelFor(p.r1 - p.r0, [&](size_t b, size_t e) {
                for (size_t r = b; r < e; ++r)
                    std::memcpy(p.c.dst + (p.r0 + r) * p.c.dPitch, src + r * p.c.width, p.c.width);
            });
        }
    }
    if (async)  // page-locked destinations only (checked by the caller): nothing was staged
        return GMM_OK;
    GMM_HIP_CHECK(hipStreamSynchronize(s->host.copy.get()));
    return GMM_OK;
}

// frame-major copies of the device tables' columns [t0, t0 + n) (gmm_kernels_layout.hip)
int transposeChunk(gmm_scorer* s, bool scores, bool best, uint32_t t0, uint32_t n, uint32_t nFrames) {
    const uint32_t M = s->nMix;
    if (scores)
        GMM_HIP_CHECK(launchTransposeWords(reinterpret_cast<const uint32_t*>(s->host.dScores.get()) + t0, M, n, nFrames,
                                           reinterpret_cast<uint32_t*>(s->host.dScoresT.get()) + static_cast<size_t>(t0) * M, M,
                                           s->host.compute.get()));
    if (best)
        GMM_HIP_CHECK(launchTransposeWords(s->host.dBest.get() + t0, M, n, nFrames, s->host.dBestT.get() + static_cast<size_t>(t0) * M, M,
                                           s->host.compute.get()));
    return GMM_OK;
}

// Small calls (up to kSmallHostFrames frames: the drop-in's buffer sizes 1..64, RASR's default is 4) are bound by
// their fixed cost, not by PCIe bandwidth: the pipeline below spends two copy-engine transfers, two cross-stream
// events and two synchronizations on a few kilobytes.  With a page-locked ring and page-locked tables mapped at
// the same address on the device (gmm_host_alloc, hipHostMalloc), such a call runs on one stream with no copy
// engine: a kernel gathers the frame rows from the ring, the scorer runs as for any call, and the transpose (frame
// major) or a strided copy kernel (mixture major) stores the tables straight into the caller's rows over PCIe;
// one synchronization.  RASR_GMM_SMALL_HOST=0 turns it off (A/B).
constexpr uint32_t kSmallHostFrames = 64;

bool smallHostPathEnabled() {
    static const bool on = [] {
        const char* e = std::getenv("RASR_GMM_SMALL_HOST");
        return !(e && e[0] == '0');
    }();
    return on;
}

void keepBestOf(gmm_scorer* s, const HostRing& r, const std::vector<HostSegment>& segs, bool frameMajor, bool lazyBest) {
    s->host.keptBestCall   = s->host.call;
    s->host.keptRing       = r;
    s->host.keptSegs       = segs;
    s->host.keptFrameMajor = frameMajor;
    s->host.keptLazy       = lazyBest;
    s->host.keptComputed   = !lazyBest;
}

// the call's end: GMM_HOST_ASYNC records it on `last`, the stream that finishes last; otherwise wait for the scoring
int endHostCall(gmm_scorer* s, bool async, hipStream_t last) {
    if (!async) {
        GMM_HIP_CHECK(hipStreamSynchronize(s->host.compute.get()));
        return GMM_OK;
    }
    if (!s->host.asyncDone)
        GMM_HIP_CHECK(s->host.asyncDone.create(hipEventDisableTiming));
    GMM_HIP_CHECK(hipEventRecord(s->host.asyncDone.get(), last));
    s->host.asyncCall = s->host.call;
    return GMM_OK;
}

int scoreHostSmall(gmm_scorer* s, const HostRing& r, float* scores, uint32_t* best, uint32_t scoreStride, bool keepBest,
                   bool lazyBest, bool frameMajor, bool async) {
    const uint32_t nFrames = r.nFrames, M = s->nMix;
    int            rc      = ensureHostPipeline(s, 1);
    if (rc != GMM_OK)
        return rc;
    std::vector<HostSegment> segs;
    appendSegments(r, 0, 0, nFrames, segs);
    const uint32_t D = s->D;
    GMM_HIP_CHECK(hipEventRecord(s->host.start.get(), nullptr));
    GMM_HIP_CHECK(hipStreamWaitEvent(s->host.compute.get(), s->host.start.get(), 0));
    for (const HostSegment& g : segs)
        GMM_HIP_CHECK(launchCopyWords2D(reinterpret_cast<const uint32_t*>(r.frames + static_cast<size_t>(g.col) * r.frameStride),
                                        r.frameStride, reinterpret_cast<uint32_t*>(s->host.dFrames.get() + static_cast<size_t>(g.t0) * D),
                                        D, g.n, D, s->host.compute.get()));
    const bool withBest = best || (keepBest && !lazyBest);
    if ((rc = scoreImpl(s, s->host.dFrames.get(), nFrames, D, s->host.dScores.get(), withBest ? s->host.dBest.get() : nullptr, nFrames,
                        s->host.compute.get())) != GMM_OK)
        return rc;
    struct Table {
        uint32_t*       dst;
        const uint32_t* src;
    };
    for (Table t : {Table{reinterpret_cast<uint32_t*>(scores), reinterpret_cast<const uint32_t*>(s->host.dScores.get())},
                    Table{best, s->host.dBest.get()}}) {
        if (!t.dst)
            continue;
        for (const HostSegment& g : segs) {
            if (frameMajor)
                GMM_HIP_CHECK(launchTransposeWords(t.src + g.t0, M, g.n, nFrames, t.dst + static_cast<size_t>(g.col) * scoreStride,
                                                   scoreStride, s->host.compute.get()));
            else
                GMM_HIP_CHECK(launchCopyWords2D(t.src + g.t0, nFrames, t.dst + g.col, scoreStride, M, g.n, s->host.compute.get()));
        }
    }
    if (keepBest)  // gmm_fetch_best_density's copies wait for this call's scorer
        GMM_HIP_CHECK(hipEventRecord(s->host.chunkDone[0].get(), s->host.compute.get()));
    const int end = endHostCall(s, async, s->host.compute.get());
    if (end == GMM_OK && keepBest)
        keepBestOf(s, r, segs, frameMajor, lazyBest);
    return end;
}

int scoreHostImpl(gmm_scorer* s, const HostRing& r, float* scores, uint32_t* best, uint32_t scoreStride, bool keepBest,
                  bool lazyBest, bool frameMajor, bool async) {
    if (r.nFrames <= kSmallHostFrames && !s->presel && !s->group && smallHostPathEnabled() && isDeviceMappedHost(r.frames) &&
        isDeviceMappedHost(scores) && (!best || isDeviceMappedHost(best)))
        return scoreHostSmall(s, r, scores, best, scoreStride, keepBest, lazyBest, frameMajor, async);
    const uint32_t fpb = modelOf(s)->plan.framesPerBlock, nFrames = r.nFrames;  // a sharded handle: its parts'
    // frame chunks for large tables; one chunk for preselection (gmm_scorer_cluster_selection reports the
    // last call's whole batch)
    const bool large   = static_cast<size_t>(nFrames) * std::max<uint32_t>(s->nMix, 1) * sizeof(float) >= kHostPipelineBytes;
    uint32_t   nChunks = s->presel || !large ? 1u : std::clamp<uint32_t>(nFrames / kHostChunkFrames, 1u, kHostMaxChunks);
    const uint32_t per = ((nFrames + nChunks - 1) / nChunks + fpb - 1) / fpb * fpb;
    nChunks            = (nFrames + per - 1) / per;
    int rc             = ensureHostPipeline(s, nChunks);
    if (rc != GMM_OK)
        return rc;
    std::vector<HostSegment> segs, rows;
    appendSegments(r, 0, 0, nFrames, rows);  // the frame rows: at most two contiguous runs of the ring
    for (uint32_t k = 0; k < nChunks; ++k)
        appendSegments(r, k, k * per, std::min(per, nFrames - k * per), segs);
    const size_t D = s->D;
    // after the legacy stream's earlier work (gmm_score_device callers on stream 0 share the staging)
    GMM_HIP_CHECK(hipEventRecord(s->host.start.get(), nullptr));
    GMM_HIP_CHECK(hipStreamWaitEvent(s->host.compute.get(), s->host.start.get(), 0));
    for (const HostSegment& g : rows)
        GMM_HIP_CHECK(hipMemcpy2DAsync(s->host.dFrames.get() + g.t0 * D, D * sizeof(float),
                                       r.frames + static_cast<size_t>(g.col) * r.frameStride,
                                       static_cast<size_t>(r.frameStride) * sizeof(float), D * sizeof(float), g.n,
                                       hipMemcpyHostToDevice, s->host.compute.get()));
    const bool withBest = best || (keepBest && !lazyBest);
    for (uint32_t k = 0; k < nChunks; ++k) {
        const uint32_t t0 = k * per, n = std::min(per, nFrames - t0);
        rc = scoreImpl(s, s->host.dFrames.get() + t0 * D, n, s->D, s->host.dScores.get() + t0, withBest ? s->host.dBest.get() + t0 : nullptr,
                       nFrames, s->host.compute.get());
        if (rc == GMM_OK && frameMajor)
            rc = transposeChunk(s, true, best != nullptr, t0, n, nFrames);
        if (rc != GMM_OK)
            return rc;
        GMM_HIP_CHECK(hipEventRecord(s->host.chunkDone[k].get(), s->host.compute.get()));
    }
    if ((rc = copyOutTables(s, segs, nFrames, frameMajor, scores, best, scoreStride, async)) != GMM_OK)
        return rc;
    const int end = endHostCall(s, async, s->host.copy.get());  // the copies wait for every chunk: their end is the call's end
    if (end == GMM_OK && keepBest)
        keepBestOf(s, r, segs, frameMajor, lazyBest);
    return end;
}

// On an error after work was queued, wait for both pipeline streams before returning: no DMA into the
// caller's buffers and no kernel reading dHostFrames may outlive the call (later calls order only against
// the null stream).
int scoreHost(gmm_scorer* s, const HostRing& r, float* scores, uint32_t* best, uint32_t scoreStride, uint32_t flags,
              uint64_t* callId) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    if ((flags & ~(GMM_HOST_KEEP_BEST | GMM_HOST_FRAME_MAJOR | GMM_HOST_LAZY_BEST | GMM_HOST_ASYNC)) != 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "unknown flags");
    const bool async = (flags & GMM_HOST_ASYNC) != 0;
    if (async && ((scores && !isPinnedHost(scores)) || (best && !isPinnedHost(best))))
        return fail(GMM_ERR_INVALID_ARGUMENT, "GMM_HOST_ASYNC needs page-locked score / best tables (gmm_host_alloc)");
    int wrc = waitAsync(s);  // the previous asynchronous call's staging and tables
    if (wrc != GMM_OK)
        return wrc;
    const bool frameMajor = (flags & GMM_HOST_FRAME_MAJOR) != 0;
    if ((flags & GMM_HOST_KEEP_BEST) && (flags & GMM_HOST_LAZY_BEST))
        return fail(GMM_ERR_INVALID_ARGUMENT, "GMM_HOST_KEEP_BEST and GMM_HOST_LAZY_BEST together");
    if ((flags & (GMM_HOST_KEEP_BEST | GMM_HOST_LAZY_BEST)) && best)
        return fail(GMM_ERR_INVALID_ARGUMENT, "GMM_HOST_KEEP_BEST / GMM_HOST_LAZY_BEST with a best_density table");
    // batch types: nothing to keep
    const bool keepBest = (flags & (GMM_HOST_KEEP_BEST | GMM_HOST_LAZY_BEST)) && s->hasAssignment();
    const bool lazyBest = keepBest && (flags & GMM_HOST_LAZY_BEST);
    // a new host call replaces the best densities a previous one kept
    s->host.keptBestCall = 0;
    const uint64_t id = ++s->host.call;
    if (callId)
        *callId = id;
    if (r.nFrames == 0)
        return GMM_OK;
    if (r.nFrames > s->cfg.max_frames)
        return fail(GMM_ERR_CAPACITY, "n_frames exceeds config.max_frames");
    if (!r.frames || !scores || r.frameStride < s->D || r.first >= r.ringSize || r.nFrames > r.ringSize ||
        scoreStride < (frameMajor ? s->nMix : r.ringSize))
        return fail(GMM_ERR_INVALID_ARGUMENT, "invalid frames/scores/stride/ring");
    GMM_HIP_CHECK(hipSetDevice(s->device));
    const size_t maxF = s->cfg.max_frames;
    const size_t table = maxF * std::max<uint32_t>(s->nMix, 1);
    if (!s->host.dFrames) {
        GMM_HIP_CHECK(s->host.dFrames.alloc(maxF * s->D));
        GMM_HIP_CHECK(s->host.dScores.alloc(table));
        GMM_HIP_CHECK(s->host.dBest.alloc(table));
    }
    if (frameMajor && !s->host.dScoresT) {
        GMM_HIP_CHECK(s->host.dScoresT.alloc(table));
        GMM_HIP_CHECK(s->host.dBestT.alloc(table));
    }
    const int rc = scoreHostImpl(s, r, scores, best, scoreStride, keepBest, lazyBest, frameMajor, async);
    if (rc != GMM_OK)
        for (hipStream_t st : {s->host.compute.get(), s->host.copy.get()})
            if (st)
                (void)hipStreamSynchronize(st);
    return rc;
}

}  // namespace

extern "C" {

int gmm_score_host(gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride, float* scores,
                   uint32_t* best, uint32_t scoreStride) {
    return scoreHost(s, HostRing{frames, std::max<uint32_t>(nFrames, 1), 0, nFrames, frameStride}, scores, best,
                     scoreStride, 0, nullptr);
}

int gmm_score_host_ring(gmm_scorer* s, const float* ring, uint32_t ringSize, uint32_t first, uint32_t nFrames,
                        uint32_t frameStride, float* scores, uint32_t* best, uint32_t scoreStride, uint32_t flags,
                        uint64_t* callId) {
    return scoreHost(s, HostRing{ring, ringSize, first, nFrames, frameStride}, scores, best, scoreStride, flags, callId);
}

int gmm_host_call_wait(gmm_scorer* s, uint64_t callId) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    return callId != 0 && callId == s->host.asyncCall ? waitAsync(s) : GMM_OK;
}

int gmm_fetch_best_density(gmm_scorer* s, uint64_t callId, uint32_t* best, uint32_t scoreStride) {
    if (!s || !best)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    const int wrc = waitAsync(s);
    if (wrc != GMM_OK)
        return wrc;
    if (!s->hasAssignment())
        return fail(GMM_ERR_UNSUPPORTED, "scorer type has no best densities (batch types)");
    if (callId == 0 || callId != s->host.keptBestCall)
        return fail(GMM_ERR_INVALID_ARGUMENT, "no best densities kept for this call (a later host call replaced them)");
    if (scoreStride < (s->host.keptFrameMajor ? s->nMix : s->host.keptRing.ringSize))
        return fail(GMM_ERR_INVALID_ARGUMENT, "score_stride below the call's table layout");
    GMM_HIP_CHECK(hipSetDevice(s->device));
    int rc = GMM_OK;
    if (!s->host.keptComputed) {
        // GMM_HOST_LAZY_BEST: score the call's frames (still in dHostFrames) again, with best densities, in one
        // launch; its scores land in the device table only (the caller's copy stays the score-only one)
        const uint32_t n = s->host.keptRing.nFrames;
        rc = scoreImpl(s, s->host.dFrames.get(), n, s->D, s->host.dScores.get(), s->host.dBest.get(), n, s->host.compute.get());
        if (rc != GMM_OK) {
            (void)hipStreamSynchronize(s->host.compute.get());
            return rc;
        }
        if (!s->host.keptFrameMajor)
            for (const HostSegment& g : s->host.keptSegs)
                GMM_HIP_CHECK(hipEventRecord(s->host.chunkDone[g.chunk].get(), s->host.compute.get()));
        s->host.keptComputed = true;
    }
    if (s->host.keptFrameMajor) {  // transpose the kept best densities now; every chunk's copy waits for it
        if ((rc = transposeChunk(s, false, true, 0, s->host.keptRing.nFrames, s->host.keptRing.nFrames)) != GMM_OK)
            return rc;
        for (const HostSegment& g : s->host.keptSegs)
            GMM_HIP_CHECK(hipEventRecord(s->host.chunkDone[g.chunk].get(), s->host.compute.get()));
    }
    // (mixture-major: the call's chunks were complete when it returned, the copies wait on events reached)
    rc = copyOutTables(s, s->host.keptSegs, s->host.keptRing.nFrames, s->host.keptFrameMajor, nullptr, best, scoreStride);
    if (rc != GMM_OK)
        (void)hipStreamSynchronize(s->host.copy.get());
    return rc;
}

}  // extern "C"

namespace rasr_gmm {
PairArgs pairArgsOf(const gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride) {
    PairArgs a{};
    a.frames      = frames;
    a.nFrames     = nFrames;
    a.frameStride = frameStride;
    const PairTables& t = *s->pairs;
    a.mixOff      = t.dMixOff.get();
    a.entryCov    = t.dCov.get();
    a.qMean       = t.dQMean.get();
    a.qConst      = t.dQConst.get();
    a.fMean       = t.dFMean.get();
    a.fConst      = t.dFConst.get();
    a.fLogNorm    = t.dLogNorm.get();
    a.isv         = t.kind == kPairSimd ? s->dIsv.get() : t.dIsv.get();
    a.nMixtures   = s->nMix;
    a.D           = s->D;
    a.Dp          = s->quantized() ? s->quantized()->paddedDimension : 0;
    a.L           = t.L;
    a.nb          = t.nb;
    a.isvStride   = t.isvStride;
    a.kind        = t.kind;
    return a;
}

int checkPairs(const gmm_scorer* s) {
    if (!s->hasAssignment())
        return fail(GMM_ERR_UNSUPPORTED, "scorer type has no best densities (batch types)");
    if (s->group || !s->pairs)
        return fail(GMM_ERR_UNSUPPORTED, "no sparse best-density path for this scorer (density-sharded handle, or a "
                                         "float model of dimension > 128): use gmm_fetch_best_density");
    return GMM_OK;
}

int checkPosteriors(const gmm_scorer* s) {
    const int rc = checkPairs(s);
    if (rc != GMM_OK)
        return rc;
    if (s->pairs->kind != kPairDiagonalSum)  // the base class's criticalError, AssigningFeatureScorer.hh:135-138
        return fail(GMM_ERR_UNSUPPORTED, "density posteriors are defined for the diagonal-sum scorer only");
    return GMM_OK;
}
}  // namespace rasr_gmm

namespace {
// the checks of gmm_density_posteriors_pairs_* that need no device
int checkPosteriorCall(const gmm_scorer* s, const float* frames, uint32_t frameStride, const uint32_t* pairFrame,
                       const uint32_t* pairMixture, uint32_t nPairs, const float* posteriors, uint32_t rowStride) {
    if (!s || (nPairs && (!frames || !pairFrame || !pairMixture || !posteriors)))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    const int rc = checkPosteriors(s);
    if (rc != GMM_OK)
        return rc;
    if (frameStride < s->D)
        return fail(GMM_ERR_INVALID_ARGUMENT, "frame_stride below the dimension");
    if (rowStride < s->pairs->maxEntries)
        return fail(GMM_ERR_CAPACITY, "row_stride " + std::to_string(rowStride) + " below the largest mixture's " +
                                              std::to_string(s->pairs->maxEntries) + " entries");
    return GMM_OK;
}
}  // namespace

extern "C" {

int gmm_density_posteriors_pairs_device(gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride,
                                        const uint32_t* pairFrame, const uint32_t* pairMixture, uint32_t nPairs,
                                        float* posteriors, uint32_t rowStride, float* logDenominator, void* stream) {
    const int rc = checkPosteriorCall(s, frames, frameStride, pairFrame, pairMixture, nPairs, posteriors, rowStride);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(s->device));
    PosteriorArgs a{};
    a.pair           = pairArgsOf(s, frames, nFrames, frameStride);
    a.pair.pairFrame = pairFrame;
    a.pair.pairMix   = pairMixture;
    a.pair.nPairs    = nPairs;
    a.posteriors     = posteriors;
    a.logDen         = logDenominator;
    a.rowStride      = rowStride;
    GMM_HIP_CHECK(launchDensityPosteriors(a, static_cast<hipStream_t>(stream)));
    return GMM_OK;
}

int gmm_density_posteriors_pairs_host(gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride,
                                      const uint32_t* pairFrame, const uint32_t* pairMixture, uint32_t nPairs,
                                      float* posteriors, uint32_t rowStride, float* logDenominator) {
    const int rc = checkPosteriorCall(s, frames, frameStride, pairFrame, pairMixture, nPairs, posteriors, rowStride);
    if (rc != GMM_OK || nPairs == 0)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(s->device));
    // the frames, dense (row length D); the pair lists; the rows
    const size_t           D = s->D, n = nPairs, rows = n * rowStride;
    DeviceBuffer<float>    dFrames, dPost, dLogDen;
    DeviceBuffer<uint32_t> dPairs;
    GMM_HIP_CHECK(dFrames.alloc(std::max<size_t>(static_cast<size_t>(nFrames) * D, 1)));
    GMM_HIP_CHECK(dPairs.alloc(2 * n));
    GMM_HIP_CHECK(dPost.alloc(std::max<size_t>(rows, 1)));
    GMM_HIP_CHECK(dLogDen.alloc(n));
    if (nFrames && D)
        GMM_HIP_CHECK(hipMemcpy2D(dFrames.get(), D * sizeof(float), frames, static_cast<size_t>(frameStride) * sizeof(float),
                                  D * sizeof(float), nFrames, hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(dPairs.get(), pairFrame, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    GMM_HIP_CHECK(hipMemcpy(dPairs.get() + n, pairMixture, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    PosteriorArgs a{};
    a.pair           = pairArgsOf(s, dFrames.get(), nFrames, s->D);
    a.pair.pairFrame = dPairs.get();
    a.pair.pairMix   = dPairs.get() + n;
    a.pair.nPairs    = nPairs;
    a.posteriors     = dPost.get();
    a.logDen         = dLogDen.get();
    a.rowStride      = rowStride;
    GMM_HIP_CHECK(launchDensityPosteriors(a, nullptr));
    // the copies on the default stream wait for the kernel and are synchronous: the buffers may go afterwards
    if (rows)
        GMM_HIP_CHECK(hipMemcpy(posteriors, dPost.get(), rows * sizeof(float), hipMemcpyDeviceToHost));
    if (logDenominator)
        GMM_HIP_CHECK(hipMemcpy(logDenominator, dLogDen.get(), n * sizeof(float), hipMemcpyDeviceToHost));
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));
    return GMM_OK;
}

int gmm_best_density_pairs(gmm_scorer* s, uint64_t callId, const uint32_t* positions, const uint32_t* mixtures,
                           uint32_t nPairs, uint32_t* best) {
    if (!s || (nPairs && (!positions || !mixtures || !best)))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    const int wrc = waitAsync(s);
    if (wrc != GMM_OK)
        return wrc;
    int rc = checkPairs(s);
    if (rc != GMM_OK)
        return rc;
    if (callId == 0 || callId != s->host.keptBestCall)
        return fail(GMM_ERR_INVALID_ARGUMENT, "no frames kept for this call (a later host call replaced them)");
    if (nPairs == 0)
        return GMM_OK;
    const HostRing& r = s->host.keptRing;
    GMM_HIP_CHECK(hipSetDevice(s->device));
    PairTables& pt = *s->pairs;
    if (pt.stageCap < nPairs) {
        GMM_HIP_CHECK(pt.hStage.reset());
        pt.stageCap       = 0;
        const size_t cap = std::max<size_t>(nPairs, 256);
        GMM_HIP_CHECK(pt.hStage.alloc(3 * cap, hipHostMallocMapped));
        pt.stageCap = cap;
    }
    uint32_t* st = pt.hStage.get();
    for (uint32_t i = 0; i < nPairs; ++i) {
        // ring position -> frame of the call (the call's frame t sits at ring position (first + t) % ringSize)
        const uint32_t pos = positions[i];
        const uint32_t t   = pos < r.ringSize ? (pos + r.ringSize - r.first) % r.ringSize : 0xffffffffu;
        if (t >= r.nFrames)
            return fail(GMM_ERR_INVALID_ARGUMENT, "position not scored by this call");
        if (mixtures[i] >= s->nMix)
            return fail(GMM_ERR_INVALID_ARGUMENT, "mixture index out of range");
        st[i]          = t;
        st[nPairs + i] = mixtures[i];
    }
    uint32_t* dst = nullptr;
    GMM_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&dst), st, 0));
    PairArgs a  = pairArgsOf(s, s->host.dFrames.get(), r.nFrames, s->D);
    a.pairFrame = dst;
    a.pairMix   = dst + nPairs;
    a.best      = dst + 2 * static_cast<size_t>(nPairs);
    a.nPairs    = nPairs;
    // after the call's own frame staging on hostCompute (the kernel reads dHostFrames)
    GMM_HIP_CHECK(launchBestPairs(a, s->host.compute.get()));
    GMM_HIP_CHECK(hipStreamSynchronize(s->host.compute.get()));
    std::memcpy(best, st + 2 * static_cast<size_t>(nPairs), nPairs * sizeof(uint32_t));
    return GMM_OK;
}

int gmm_best_density_pairs_device(gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride,
                                  const uint32_t* pairFrame, const uint32_t* pairMixture, uint32_t nPairs,
                                  uint32_t* best, void* stream) {
    if (!s || (nPairs && (!frames || !pairFrame || !pairMixture || !best)))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    int rc = checkPairs(s);
    if (rc != GMM_OK)
        return rc;
    if (frameStride < s->D)
        return fail(GMM_ERR_INVALID_ARGUMENT, "frame_stride below the dimension");
    if (nPairs == 0)
        return GMM_OK;
    GMM_HIP_CHECK(hipSetDevice(s->device));
    PairArgs a  = pairArgsOf(s, frames, nFrames, frameStride);
    a.pairFrame = pairFrame;
    a.pairMix   = pairMixture;
    a.best      = best;
    a.nPairs    = nPairs;
    GMM_HIP_CHECK(launchBestPairs(a, static_cast<hipStream_t>(stream)));
    return GMM_OK;
}

}  // extern "C"
