// gmm_align.cc -- the handle behind include/rasr_gmm_align.h: its device memory (the batch's tables and the
// backpointer scratch, all allocated at creation), set_segments (host/AlignGraph.cc validates and builds, this unit
// uploads), the checks and the launch of an align call (gmm_kernels_align.hip), the host call's staging.
#include <cfloat>
#include <cmath>
#include <memory>
#include <new>

#include "gmm_align.hh"
#include "gmm_scorer.hh"

using namespace rasr_gmm;

struct gmm_aligner {
    AlignCapacity cap{};
    int           device = 0;
    // the batch: what the last accepted set_segments left (nSegments == 0: none yet)
    uint32_t nSegments = 0, rowStates = 0;
    uint64_t frameEnd = 0;
    DeviceBuffer<AlignSegment> dSegments;
    DeviceBuffer<uint32_t>     dOrder, dInOffset, dInSource, dInArc, dInMixture;
    DeviceBuffer<float>        dInWeight, dFinalWeight;
    // the backpointers of one call
    DeviceBuffer<uint32_t> dCells;
    // Baum-Welch mode.  `posterior` keeps the batch's tables for it on the host (AlignPlan's second half; the first is
    // dropped): the first posterior call allocates everything below and uploads them, set_segments does after that
    AlignPlan              posterior;
    uint32_t               maxSegmentStates = 0;
    bool                   posteriorReady = false;
    DeviceBuffer<uint32_t> dArcOffset, dArcTarget, dArcMixture, dGroupOffset, dGroupMixture, dGroupArcOffset, dGroupSource,
            dGroupTarget, dColSegment, dColFrameOffset;
    DeviceBuffer<float>    dArcWeight, dGroupWeight;
    // its scratch: per cell, per segment, per ordered frame, per item wave
    DeviceBuffer<double>   dFwPot, dBwPot, dSegTotalInv;
    DeviceBuffer<uint8_t>  dMark;
    DeviceBuffer<uint32_t> dSegHas, dFrameCount;
    DeviceBuffer<float>    dFrameMin, dFrameInv, dWaveWeights;
    uint32_t               rowGroups = 0;
    // recorded by every align call on its stream; set_segments and destroy wait for it
    Event done;
    bool  pending = false;
};

namespace {

int waitDone(gmm_aligner* h) {
    if (h->pending) {
        GMM_HIP_CHECK(hipEventSynchronize(h->done.get()));
        h->pending = false;
    }
    return GMM_OK;
}

int create(gmm_aligner* h) {
    GMM_HIP_CHECK(hipSetDevice(h->device));
    const AlignCapacity& c = h->cap;
    GMM_HIP_CHECK(h->dSegments.alloc(c.maxSegments));
    GMM_HIP_CHECK(h->dOrder.alloc(c.maxSegments));
    GMM_HIP_CHECK(h->dInOffset.alloc(static_cast<size_t>(c.maxStates) + 1));
    GMM_HIP_CHECK(h->dFinalWeight.alloc(c.maxStates));
    GMM_HIP_CHECK(h->dInSource.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dInArc.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dInMixture.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dInWeight.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dCells.alloc(c.maxCells));
    GMM_HIP_CHECK(h->done.create(hipEventDisableTiming));
    return GMM_OK;
}

template <class T>
hipError_t put(DeviceBuffer<T>& dst, const std::vector<T>& src) {
    return src.empty() ? hipSuccess : hipMemcpy(dst.get(), src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
}

// the checks of both align calls; nothing is written or enqueued before they pass
int checkAlignCall(const gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                   const void* outMixture, const void* outState, const void* outArc, const void* outScore,
                   const void* outHypotheses) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null aligner");
    if (!scores)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: null scores");
    if (!outMixture && !outState && !outArc && !outScore && !outHypotheses)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: no output requested");
    if (h->nSegments == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: no segments set");
    if (scoreStride < nTableFrames)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: score_stride below n_table_frames");
    if (h->frameEnd > nTableFrames)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: a segment ends at column " + std::to_string(h->frameEnd) +
                                                      ", past n_table_frames " + std::to_string(nTableFrames));
    return GMM_OK;
}

// the search outputs of a search call; search == nullptr: the fixed-threshold call
struct SearchCall {
    const AlignSearch* search        = nullptr;
    float*             outThreshold  = nullptr;
    uint32_t*          outIterations = nullptr;
};

// The checks of gmm_align_search, before anything is written; fills `out`.  The schedule is counted with the f32
// multiply the kernels use.
int checkSearch(const gmm_align_search* s, AlignSearch& out) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: null search");
    if (std::isnan(s->min_pruning) || std::isnan(s->max_pruning) || std::isnan(s->increment_factor) ||
        std::isnan(s->min_average_hypotheses))
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: a NaN in the search");
    if (s->min_pruning < FLT_MIN)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: min_pruning below FLT_MIN");
    if (!std::isfinite(s->max_pruning))
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: max_pruning is not finite");
    if (s->min_pruning > s->max_pruning)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: min_pruning above max_pruning");
    if (s->increment_factor <= 1.0f && s->min_pruning != s->max_pruning)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: increment_factor <= 1 with min_pruning != max_pruning");
    if (s->n_best == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: n_best 0");
    if (s->increment_factor > 1.0f) {
        uint32_t       count = 0;
        volatile float t = s->min_pruning;  // volatile: one f32 rounding per step whatever the host's evaluation method
        while (t <= s->max_pruning && count <= GMM_ALIGN_MAX_ITERATIONS) {
            ++count;
            t = t * s->increment_factor;
        }
        if (count > GMM_ALIGN_MAX_ITERATIONS)
            return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: a schedule of more than GMM_ALIGN_MAX_ITERATIONS thresholds");
    }
    out.minPruning        = s->min_pruning;
    out.maxPruning        = s->max_pruning;
    out.factor            = s->increment_factor;
    out.minAverage        = s->min_average_hypotheses;
    out.untilNoDifference = s->until_no_score_difference != 0;
    out.nBest             = s->n_best;
    return GMM_OK;
}

int alignOn(gmm_aligner* h, const float* scores, uint32_t scoreStride, float pruning, uint32_t* outMixture,
            uint32_t* outState, uint32_t* outArc, float* outScore, uint32_t* outHypotheses, hipStream_t stream,
            const SearchCall& sc = SearchCall{}) {
    AlignArgs a{};
    a.segments      = h->dSegments.get();
    a.order         = h->dOrder.get();
    a.inOffset      = h->dInOffset.get();
    a.inSource      = h->dInSource.get();
    a.inArc         = h->dInArc.get();
    a.inMixture     = h->dInMixture.get();
    a.inWeight      = h->dInWeight.get();
    a.finalWeight   = h->dFinalWeight.get();
    a.scores        = scores;
    a.scoreStride   = scoreStride;
    a.pruning       = pruning;
    a.cells         = h->dCells.get();
    a.outMixture    = outMixture;
    a.outState      = outState;
    a.outArc        = outArc;
    a.outScore      = outScore;
    a.outHypotheses = outHypotheses;
    a.nSegments     = h->nSegments;
    a.rowStates     = h->rowStates;
    const hipError_t e = sc.search ? launchAlignSearch(AlignSearchArgs{a, *sc.search, sc.outThreshold, sc.outIterations}, stream)
                                   : launchAlign(a, stream);
    // what was enqueued uses the handle's tables and scratch
    GMM_HIP_CHECK(hipEventRecord(h->done.get(), stream));
    h->pending = true;
    GMM_HIP_CHECK(e);
    return GMM_OK;
}

// the ordered frames of a batch fit 32 bits (the frame ranges are disjoint columns of a table)
size_t maxFrames(const AlignCapacity& c) {
    return static_cast<size_t>(c.maxCells < 0xffffffffull ? c.maxCells : 0xffffffffull);
}

// the batch's tables of the Baum-Welch mode, from the host copy
int uploadPosterior(gmm_aligner* h) {
    const AlignPlan& p = h->posterior;
    GMM_HIP_CHECK(put(h->dArcOffset, p.arcOffset));
    GMM_HIP_CHECK(put(h->dArcTarget, p.arcTarget));
    GMM_HIP_CHECK(put(h->dArcMixture, p.arcMixture));
    GMM_HIP_CHECK(put(h->dArcWeight, p.arcWeight));
    GMM_HIP_CHECK(put(h->dGroupOffset, p.groupOffset));
    GMM_HIP_CHECK(put(h->dGroupMixture, p.groupMixture));
    GMM_HIP_CHECK(put(h->dGroupArcOffset, p.groupArcOffset));
    GMM_HIP_CHECK(put(h->dGroupSource, p.groupSource));
    GMM_HIP_CHECK(put(h->dGroupTarget, p.groupTarget));
    GMM_HIP_CHECK(put(h->dGroupWeight, p.groupWeight));
    GMM_HIP_CHECK(put(h->dColSegment, p.colSegment));
    const std::vector<uint32_t> frameOffset(p.colFrameOffset.begin(), p.colFrameOffset.end());
    GMM_HIP_CHECK(put(h->dColFrameOffset, frameOffset));
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));
    return GMM_OK;
}

// the first posterior call: the mode's tables and scratch, sized from the capacities
int preparePosterior(gmm_aligner* h) {
    if (h->posteriorReady)
        return GMM_OK;
    const AlignCapacity& c = h->cap;
    const size_t         frames = maxFrames(c);
    GMM_HIP_CHECK(h->dArcOffset.alloc(static_cast<size_t>(c.maxStates) + 1));
    GMM_HIP_CHECK(h->dArcTarget.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dArcMixture.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dArcWeight.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dGroupOffset.alloc(static_cast<size_t>(c.maxSegments) + 1));
    GMM_HIP_CHECK(h->dGroupMixture.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dGroupArcOffset.alloc(static_cast<size_t>(c.maxArcs) + 1));
    GMM_HIP_CHECK(h->dGroupSource.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dGroupTarget.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dGroupWeight.alloc(c.maxArcs));
    GMM_HIP_CHECK(h->dColSegment.alloc(c.maxSegments));
    GMM_HIP_CHECK(h->dColFrameOffset.alloc(static_cast<size_t>(c.maxSegments) + 1));
    GMM_HIP_CHECK(h->dFwPot.alloc(c.maxCells));
    GMM_HIP_CHECK(h->dBwPot.alloc(c.maxCells));
    GMM_HIP_CHECK(h->dMark.alloc(c.maxCells));
    GMM_HIP_CHECK(h->dSegTotalInv.alloc(c.maxSegments));
    GMM_HIP_CHECK(h->dSegHas.alloc(c.maxSegments));
    GMM_HIP_CHECK(h->dFrameCount.alloc(frames + 1));
    GMM_HIP_CHECK(h->dFrameMin.alloc(frames));
    GMM_HIP_CHECK(h->dFrameInv.alloc(frames));
    h->rowGroups = c.nMixtures < c.maxArcs ? c.nMixtures : c.maxArcs;
    GMM_HIP_CHECK(h->dWaveWeights.alloc(static_cast<size_t>(kAlignItemWaves) * h->rowGroups));
    const int rc = uploadPosterior(h);
    if (rc != GMM_OK)
        return rc;
    h->posteriorReady = true;
    return GMM_OK;
}

// the checks of both posterior calls; nothing is written or enqueued before they pass
int checkPosteriorCall(const gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                       uint32_t maxItems, const void* itemFrame, const void* itemMixture, const void* itemWeight,
                       const void* columnOffset, const void* nItems, const void* outScore, const void* outHypotheses,
                       const void* logTotal) {
    const bool items = itemFrame || itemMixture || itemWeight;
    const int  rc = checkAlignCall(h, scores, nTableFrames, scoreStride, itemFrame, columnOffset, nItems,
                                   outScore ? outScore : logTotal, outHypotheses);
    if (rc != GMM_OK)
        return rc;
    if (items && !(itemFrame && itemMixture && itemWeight))
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: out_item_frame, out_item_mixture and out_item_weight go together");
    if (items && maxItems == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: item arrays with max_items 0");
    if (h->maxSegmentStates > GMM_ALIGN_MAX_STATES_POSTERIOR)
        return fail(GMM_ERR_UNSUPPORTED, "aligner: a segment has " + std::to_string(h->maxSegmentStates) +
                                                 " states, more than GMM_ALIGN_MAX_STATES_POSTERIOR " +
                                                 std::to_string(GMM_ALIGN_MAX_STATES_POSTERIOR));
    if (h->posterior.nFrames > 0xffffffffull)
        return fail(GMM_ERR_UNSUPPORTED, "aligner: 2^32 frames or more in one batch");
    return GMM_OK;
}

int posteriorsOn(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride, float pruning,
                 float minPosterior, uint32_t maxItems, uint32_t* itemFrame, uint32_t* itemMixture, double* itemWeight,
                 uint32_t* columnOffset, uint32_t* nItems, float* outScore, uint32_t* outHypotheses, double* logTotal,
                 hipStream_t stream, const SearchCall& sc = SearchCall{}) {
    const int rc = preparePosterior(h);
    if (rc != GMM_OK)
        return rc;
    AlignPosteriorArgs a{};
    a.segments        = h->dSegments.get();
    a.order           = h->dOrder.get();
    a.inOffset        = h->dInOffset.get();
    a.inSource        = h->dInSource.get();
    a.inMixture       = h->dInMixture.get();
    a.inWeight        = h->dInWeight.get();
    a.finalWeight     = h->dFinalWeight.get();
    a.arcOffset       = h->dArcOffset.get();
    a.arcTarget       = h->dArcTarget.get();
    a.arcMixture      = h->dArcMixture.get();
    a.arcWeight       = h->dArcWeight.get();
    a.groupOffset     = h->dGroupOffset.get();
    a.groupMixture    = h->dGroupMixture.get();
    a.groupArcOffset  = h->dGroupArcOffset.get();
    a.groupSource     = h->dGroupSource.get();
    a.groupTarget     = h->dGroupTarget.get();
    a.groupWeight     = h->dGroupWeight.get();
    a.colSegment      = h->dColSegment.get();
    a.colFrameOffset  = h->dColFrameOffset.get();
    a.scores          = scores;
    a.scoreStride     = scoreStride;
    a.nTableFrames    = nTableFrames;
    a.pruning         = pruning;
    a.minPosterior    = minPosterior;
    a.maxItems        = maxItems;
    a.fwPot           = h->dFwPot.get();
    a.bwPot           = h->dBwPot.get();
    a.mark            = h->dMark.get();
    a.segTotalInv     = h->dSegTotalInv.get();
    a.segHas          = h->dSegHas.get();
    a.frameMin        = h->dFrameMin.get();
    a.frameInv        = h->dFrameInv.get();
    a.frameCount      = h->dFrameCount.get();
    a.waveWeights     = h->dWaveWeights.get();
    a.rowGroups       = h->rowGroups;
    a.outItemFrame    = itemFrame;
    a.outItemMixture  = itemMixture;
    a.outItemWeight   = itemWeight;
    a.outColumnOffset = columnOffset;
    a.outNItems       = nItems;
    a.outScore        = outScore;
    a.outHypotheses   = outHypotheses;
    a.outLogTotal     = logTotal;
    a.nSegments       = h->nSegments;
    a.rowStates       = h->rowStates;
    a.nFrames         = static_cast<uint32_t>(h->posterior.nFrames);
    const hipError_t e =
            sc.search ? launchAlignPosteriorsSearch(AlignPosteriorSearchArgs{a, *sc.search, sc.outThreshold, sc.outIterations},
                                                    stream)
                      : launchAlignPosteriors(a, stream);
    GMM_HIP_CHECK(hipEventRecord(h->done.get(), stream));
    h->pending = true;
    GMM_HIP_CHECK(e);
    return GMM_OK;
}

}  // namespace

extern "C" {

int gmm_aligner_create(uint32_t maxSegments, uint32_t maxStates, uint32_t maxArcs, uint64_t maxCells, uint32_t nMixtures,
                       int device, gmm_aligner** out) {
    if (!out)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (maxSegments == 0 || maxStates == 0 || maxArcs == 0 || maxCells == 0 || nMixtures == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT,
                    "aligner: max_segments, max_states, max_arcs, max_cells and n_mixtures must not be 0");
    std::unique_ptr<gmm_aligner> h(new (std::nothrow) gmm_aligner);
    if (!h)
        return fail(GMM_ERR_OUT_OF_MEMORY, "out of host memory");
    h->cap    = AlignCapacity{maxSegments, maxStates, maxArcs, maxCells, nMixtures};
    h->device = device;
    const int rc = create(h.get());
    if (rc != GMM_OK)
        return rc;
    *out = h.release();
    return GMM_OK;
}

int gmm_aligner_destroy(gmm_aligner* h) {
    if (!h)
        return GMM_OK;
    // no kernel of a call may outlive the tables and the scratch
    if (hipSetDevice(h->device) == hipSuccess)
        (void)waitDone(h);
    delete h;
    return GMM_OK;
}

int gmm_aligner_set_segments(gmm_aligner* h, const gmm_align_graphs* graphs) {
    if (!h || !graphs)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    AlignPlan   plan;
    std::string message;
    int         rc = buildAlignPlan(*graphs, h->cap, plan, &message);
    if (rc != GMM_OK)
        return fail(rc, message);
    GMM_HIP_CHECK(hipSetDevice(h->device));
    if ((rc = waitDone(h)) != GMM_OK)  // the last call still reads the tables
        return rc;
    h->nSegments = 0;  // a failed upload leaves no batch
    GMM_HIP_CHECK(put(h->dSegments, plan.segments));
    GMM_HIP_CHECK(put(h->dOrder, plan.order));
    GMM_HIP_CHECK(put(h->dInOffset, plan.inOffset));
    GMM_HIP_CHECK(put(h->dInSource, plan.inSource));
    GMM_HIP_CHECK(put(h->dInArc, plan.inArc));
    GMM_HIP_CHECK(put(h->dInMixture, plan.inMixture));
    GMM_HIP_CHECK(put(h->dInWeight, plan.inWeight));
    GMM_HIP_CHECK(put(h->dFinalWeight, plan.finalWeight));
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));  // done before a call on any other stream
    const uint32_t nSegments = static_cast<uint32_t>(plan.segments.size());
    // the Baum-Welch mode's tables stay on the host until a posterior call has made room for them on the device
    for (std::vector<uint32_t>* v : {&plan.order, &plan.inOffset, &plan.inSource, &plan.inArc, &plan.inMixture})
        std::vector<uint32_t>().swap(*v);
    std::vector<float>().swap(plan.inWeight);
    std::vector<float>().swap(plan.finalWeight);
    std::vector<AlignSegment>().swap(plan.segments);
    h->posterior = std::move(plan);
    if (h->posteriorReady && (rc = uploadPosterior(h)) != GMM_OK)
        return rc;
    h->maxSegmentStates = h->posterior.maxSegmentStates;
    h->rowStates        = (h->posterior.maxSegmentStates + 63u) & ~63u;
    h->frameEnd         = h->posterior.frameEnd;
    h->nSegments        = nSegments;
    return GMM_OK;
}

int gmm_aligner_align_device(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                             float pruning, uint32_t* outMixture, uint32_t* outState, uint32_t* outArc, float* outScore,
                             uint32_t* outHypotheses, void* stream) {
    const int rc = checkAlignCall(h, scores, nTableFrames, scoreStride, outMixture, outState, outArc, outScore, outHypotheses);
    if (rc != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(h->device));
    return alignOn(h, scores, scoreStride, pruning, outMixture, outState, outArc, outScore, outHypotheses,
                   static_cast<hipStream_t>(stream));
}

// the staging of both host align calls, behind their checks; hs: the search with its HOST outputs
static int alignHost(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride, float pruning,
                     uint32_t* outMixture, uint32_t* outState, uint32_t* outArc, float* outScore, uint32_t* outHypotheses,
                     const SearchCall& hs) {
    int rc;
    GMM_HIP_CHECK(hipSetDevice(h->device));
    if ((rc = waitDone(h)) != GMM_OK)
        return rc;
    // the table, dense; the per-column outputs start from the host arrays, whose columns of no segment are kept
    const size_t           F = nTableFrames, M = h->cap.nMixtures, S = h->nSegments;
    DeviceBuffer<float>    dTable, dScore, dThreshold;
    DeviceBuffer<uint32_t> dColumns, dHypotheses, dIterations;  // dColumns: mixture, state, arc
    uint32_t* const        host[3] = {outMixture, outState, outArc};
    uint32_t*              dev[3]  = {nullptr, nullptr, nullptr};
    GMM_HIP_CHECK(dTable.alloc(M * F));
    GMM_HIP_CHECK(dColumns.alloc(3 * F));
    GMM_HIP_CHECK(dScore.alloc(S));
    GMM_HIP_CHECK(dHypotheses.alloc(S));
    SearchCall sc = hs;
    if (hs.outThreshold) {
        GMM_HIP_CHECK(dThreshold.alloc(S));
        sc.outThreshold = dThreshold.get();
    }
    if (hs.outIterations) {
        GMM_HIP_CHECK(dIterations.alloc(S));
        sc.outIterations = dIterations.get();
    }
    if (F)
        GMM_HIP_CHECK(hipMemcpy2D(dTable.get(), F * sizeof(float), scores, static_cast<size_t>(scoreStride) * sizeof(float),
                                  F * sizeof(float), M, hipMemcpyHostToDevice));
    for (int o = 0; o < 3; ++o)
        if (host[o]) {
            dev[o] = dColumns.get() + o * F;
            GMM_HIP_CHECK(hipMemcpy(dev[o], host[o], F * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
    rc = alignOn(h, dTable.get(), nTableFrames, pruning, dev[0], dev[1], dev[2], outScore ? dScore.get() : nullptr,
                 outHypotheses ? dHypotheses.get() : nullptr, nullptr, sc);
    if (rc != GMM_OK) {
        (void)hipStreamSynchronize(nullptr);  // the buffers go with this scope
        return rc;
    }
    // the copies on the default stream wait for the kernel and are synchronous
    for (int o = 0; o < 3; ++o)
        if (host[o])
            GMM_HIP_CHECK(hipMemcpy(host[o], dev[o], F * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (outScore)
        GMM_HIP_CHECK(hipMemcpy(outScore, dScore.get(), S * sizeof(float), hipMemcpyDeviceToHost));
    if (outHypotheses)
        GMM_HIP_CHECK(hipMemcpy(outHypotheses, dHypotheses.get(), S * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (hs.outThreshold)
        GMM_HIP_CHECK(hipMemcpy(hs.outThreshold, dThreshold.get(), S * sizeof(float), hipMemcpyDeviceToHost));
    if (hs.outIterations)
        GMM_HIP_CHECK(hipMemcpy(hs.outIterations, dIterations.get(), S * sizeof(uint32_t), hipMemcpyDeviceToHost));
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));
    return GMM_OK;
}

int gmm_aligner_align_host(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride, float pruning,
                           uint32_t* outMixture, uint32_t* outState, uint32_t* outArc, float* outScore,
                           uint32_t* outHypotheses) {
    const int rc = checkAlignCall(h, scores, nTableFrames, scoreStride, outMixture, outState, outArc, outScore, outHypotheses);
    if (rc != GMM_OK)
        return rc;
    return alignHost(h, scores, nTableFrames, scoreStride, pruning, outMixture, outState, outArc, outScore, outHypotheses,
                     SearchCall{});
}

void gmm_default_align_search(gmm_align_search* s) {
    if (!s)
        return;
    s->min_pruning               = 50.0f;
    s->max_pruning               = FLT_MAX;
    s->increment_factor          = 2.0f;
    s->min_average_hypotheses    = 0.0;
    s->until_no_score_difference = 1;
    s->n_best                    = 0x7fffffffu;
}

int gmm_aligner_align_search_device(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                    const gmm_align_search* search, uint32_t* outMixture, uint32_t* outState,
                                    uint32_t* outArc, float* outScore, uint32_t* outHypotheses, float* outThreshold,
                                    uint32_t* outIterations, void* stream) {
    int rc = checkAlignCall(h, scores, nTableFrames, scoreStride, outMixture, outState, outArc, outScore, outHypotheses);
    if (rc != GMM_OK)
        return rc;
    AlignSearch as{};
    if ((rc = checkSearch(search, as)) != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(h->device));
    return alignOn(h, scores, scoreStride, 0.0f, outMixture, outState, outArc, outScore, outHypotheses,
                   static_cast<hipStream_t>(stream), SearchCall{&as, outThreshold, outIterations});
}

int gmm_aligner_align_search_host(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                  const gmm_align_search* search, uint32_t* outMixture, uint32_t* outState,
                                  uint32_t* outArc, float* outScore, uint32_t* outHypotheses, float* outThreshold,
                                  uint32_t* outIterations) {
    int rc = checkAlignCall(h, scores, nTableFrames, scoreStride, outMixture, outState, outArc, outScore, outHypotheses);
    if (rc != GMM_OK)
        return rc;
    AlignSearch as{};
    if ((rc = checkSearch(search, as)) != GMM_OK)
        return rc;
    return alignHost(h, scores, nTableFrames, scoreStride, 0.0f, outMixture, outState, outArc, outScore, outHypotheses,
                     SearchCall{&as, outThreshold, outIterations});
}

int gmm_aligner_posteriors_device(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                  float pruning, float minPosterior, uint32_t maxItems, uint32_t* itemFrame,
                                  uint32_t* itemMixture, double* itemWeight, uint32_t* columnOffset, uint32_t* nItems,
                                  float* outScore, uint32_t* outHypotheses, double* logTotal, void* stream) {
    const int rc = checkPosteriorCall(h, scores, nTableFrames, scoreStride, maxItems, itemFrame, itemMixture, itemWeight,
                                      columnOffset, nItems, outScore, outHypotheses, logTotal);
    if (rc != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(h->device));
    return posteriorsOn(h, scores, nTableFrames, scoreStride, pruning, minPosterior, maxItems, itemFrame, itemMixture,
                        itemWeight, columnOffset, nItems, outScore, outHypotheses, logTotal,
                        static_cast<hipStream_t>(stream));
}

// the staging of both host posterior calls, behind their checks; hs: the search with its HOST outputs
static int posteriorsHost(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride, float pruning,
                          float minPosterior, uint32_t maxItems, uint32_t* itemFrame, uint32_t* itemMixture,
                          double* itemWeight, uint32_t* columnOffset, uint32_t* nItems, float* outScore,
                          uint32_t* outHypotheses, double* logTotal, const SearchCall& hs) {
    int rc;
    GMM_HIP_CHECK(hipSetDevice(h->device));
    if ((rc = waitDone(h)) != GMM_OK)
        return rc;
    const size_t           F = nTableFrames, M = h->cap.nMixtures, S = h->nSegments, I = itemFrame ? maxItems : 0;
    DeviceBuffer<float>    dTable, dScore, dThreshold;
    DeviceBuffer<uint32_t> dItems, dColumnOffset, dCount, dHypotheses, dIterations;  // dItems: frame, mixture
    DeviceBuffer<double>   dWeight, dLogTotal;
    SearchCall             sc = hs;
    if (hs.outThreshold) {
        GMM_HIP_CHECK(dThreshold.alloc(S));
        sc.outThreshold = dThreshold.get();
    }
    if (hs.outIterations) {
        GMM_HIP_CHECK(dIterations.alloc(S));
        sc.outIterations = dIterations.get();
    }
    GMM_HIP_CHECK(dTable.alloc(M * F));
    GMM_HIP_CHECK(dItems.alloc(2 * I));
    GMM_HIP_CHECK(dWeight.alloc(I));
    GMM_HIP_CHECK(dColumnOffset.alloc(F + 1));
    GMM_HIP_CHECK(dCount.alloc(1));
    GMM_HIP_CHECK(dScore.alloc(S));
    GMM_HIP_CHECK(dHypotheses.alloc(S));
    GMM_HIP_CHECK(dLogTotal.alloc(S));
    if (F)
        GMM_HIP_CHECK(hipMemcpy2D(dTable.get(), F * sizeof(float), scores, static_cast<size_t>(scoreStride) * sizeof(float),
                                  F * sizeof(float), M, hipMemcpyHostToDevice));
    rc = posteriorsOn(h, dTable.get(), nTableFrames, nTableFrames, pruning, minPosterior, maxItems,
                      I ? dItems.get() : nullptr, I ? dItems.get() + I : nullptr, I ? dWeight.get() : nullptr,
                      columnOffset ? dColumnOffset.get() : nullptr, dCount.get(), outScore ? dScore.get() : nullptr,
                      outHypotheses ? dHypotheses.get() : nullptr, logTotal ? dLogTotal.get() : nullptr, nullptr, sc);
    if (rc != GMM_OK) {
        (void)hipStreamSynchronize(nullptr);  // the buffers go with this scope
        return rc;
    }
    uint32_t count = 0;
    GMM_HIP_CHECK(hipMemcpy(&count, dCount.get(), sizeof(count), hipMemcpyDeviceToHost));
    if (nItems)
        *nItems = count;
    if (outScore)
        GMM_HIP_CHECK(hipMemcpy(outScore, dScore.get(), S * sizeof(float), hipMemcpyDeviceToHost));
    if (outHypotheses)
        GMM_HIP_CHECK(hipMemcpy(outHypotheses, dHypotheses.get(), S * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (logTotal)
        GMM_HIP_CHECK(hipMemcpy(logTotal, dLogTotal.get(), S * sizeof(double), hipMemcpyDeviceToHost));
    if (hs.outThreshold)
        GMM_HIP_CHECK(hipMemcpy(hs.outThreshold, dThreshold.get(), S * sizeof(float), hipMemcpyDeviceToHost));
    if (hs.outIterations)
        GMM_HIP_CHECK(hipMemcpy(hs.outIterations, dIterations.get(), S * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (I && count > maxItems) {
        GMM_HIP_CHECK(hipStreamSynchronize(nullptr));
        return fail(GMM_ERR_CAPACITY, "aligner: the call produces " + std::to_string(count) + " items, more than max_items " +
                                              std::to_string(maxItems));
    }
    if (I && count) {
        GMM_HIP_CHECK(hipMemcpy(itemFrame, dItems.get(), count * sizeof(uint32_t), hipMemcpyDeviceToHost));
        GMM_HIP_CHECK(hipMemcpy(itemMixture, dItems.get() + I, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
        GMM_HIP_CHECK(hipMemcpy(itemWeight, dWeight.get(), count * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (columnOffset)
        GMM_HIP_CHECK(hipMemcpy(columnOffset, dColumnOffset.get(), (F + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));
    return GMM_OK;
}

int gmm_aligner_posteriors_host(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                float pruning, float minPosterior, uint32_t maxItems, uint32_t* itemFrame,
                                uint32_t* itemMixture, double* itemWeight, uint32_t* columnOffset, uint32_t* nItems,
                                float* outScore, uint32_t* outHypotheses, double* logTotal) {
    const int rc = checkPosteriorCall(h, scores, nTableFrames, scoreStride, maxItems, itemFrame, itemMixture, itemWeight,
                                      columnOffset, nItems, outScore, outHypotheses, logTotal);
    if (rc != GMM_OK)
        return rc;
    return posteriorsHost(h, scores, nTableFrames, scoreStride, pruning, minPosterior, maxItems, itemFrame, itemMixture,
                          itemWeight, columnOffset, nItems, outScore, outHypotheses, logTotal, SearchCall{});
}

int gmm_aligner_posteriors_search_device(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                         const gmm_align_search* search, float minPosterior, uint32_t maxItems,
                                         uint32_t* itemFrame, uint32_t* itemMixture, double* itemWeight,
                                         uint32_t* columnOffset, uint32_t* nItems, float* outScore, uint32_t* outHypotheses,
                                         double* logTotal, float* outThreshold, uint32_t* outIterations, void* stream) {
    int rc = checkPosteriorCall(h, scores, nTableFrames, scoreStride, maxItems, itemFrame, itemMixture, itemWeight,
                                columnOffset, nItems, outScore, outHypotheses, logTotal);
    if (rc != GMM_OK)
        return rc;
    AlignSearch as{};
    if ((rc = checkSearch(search, as)) != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(h->device));
    return posteriorsOn(h, scores, nTableFrames, scoreStride, 0.0f, minPosterior, maxItems, itemFrame, itemMixture,
                        itemWeight, columnOffset, nItems, outScore, outHypotheses, logTotal,
                        static_cast<hipStream_t>(stream), SearchCall{&as, outThreshold, outIterations});
}

int gmm_aligner_posteriors_search_host(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                       const gmm_align_search* search, float minPosterior, uint32_t maxItems,
                                       uint32_t* itemFrame, uint32_t* itemMixture, double* itemWeight,
                                       uint32_t* columnOffset, uint32_t* nItems, float* outScore, uint32_t* outHypotheses,
                                       double* logTotal, float* outThreshold, uint32_t* outIterations) {
    int rc = checkPosteriorCall(h, scores, nTableFrames, scoreStride, maxItems, itemFrame, itemMixture, itemWeight,
                                columnOffset, nItems, outScore, outHypotheses, logTotal);
    if (rc != GMM_OK)
        return rc;
    AlignSearch as{};
    if ((rc = checkSearch(search, as)) != GMM_OK)
        return rc;
    return posteriorsHost(h, scores, nTableFrames, scoreStride, 0.0f, minPosterior, maxItems, itemFrame, itemMixture,
                          itemWeight, columnOffset, nItems, outScore, outHypotheses, logTotal,
                          SearchCall{&as, outThreshold, outIterations});
}

}  // extern "C"
