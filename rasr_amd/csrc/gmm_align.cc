// gmm_align.cc -- the handle behind include/rasr_gmm_align.h: its device memory (the batch's tables and the
// backpointer scratch, all allocated at creation), set_segments (host/AlignGraph.cc validates and builds, this unit
// uploads), the checks and the launch of an align call (gmm_kernels_align.hip), the host call's staging.
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

int alignOn(gmm_aligner* h, const float* scores, uint32_t scoreStride, float pruning, uint32_t* outMixture,
            uint32_t* outState, uint32_t* outArc, float* outScore, uint32_t* outHypotheses, hipStream_t stream) {
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
    const hipError_t e = launchAlign(a, stream);
    // what was enqueued uses the handle's tables and scratch
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
    h->rowStates = (plan.maxSegmentStates + 63u) & ~63u;
    h->frameEnd  = plan.frameEnd;
    h->nSegments = static_cast<uint32_t>(plan.segments.size());
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

int gmm_aligner_align_host(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride, float pruning,
                           uint32_t* outMixture, uint32_t* outState, uint32_t* outArc, float* outScore,
                           uint32_t* outHypotheses) {
    int rc = checkAlignCall(h, scores, nTableFrames, scoreStride, outMixture, outState, outArc, outScore, outHypotheses);
    if (rc != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipSetDevice(h->device));
    if ((rc = waitDone(h)) != GMM_OK)
        return rc;
    // the table, dense; the per-column outputs start from the host arrays, whose columns of no segment are kept
    const size_t           F = nTableFrames, M = h->cap.nMixtures, S = h->nSegments;
    DeviceBuffer<float>    dTable, dScore;
    DeviceBuffer<uint32_t> dColumns, dHypotheses;  // dColumns: mixture, state, arc
    uint32_t* const        host[3] = {outMixture, outState, outArc};
    uint32_t*              dev[3]  = {nullptr, nullptr, nullptr};
    GMM_HIP_CHECK(dTable.alloc(M * F));
    GMM_HIP_CHECK(dColumns.alloc(3 * F));
    GMM_HIP_CHECK(dScore.alloc(S));
    GMM_HIP_CHECK(dHypotheses.alloc(S));
    if (F)
        GMM_HIP_CHECK(hipMemcpy2D(dTable.get(), F * sizeof(float), scores, static_cast<size_t>(scoreStride) * sizeof(float),
                                  F * sizeof(float), M, hipMemcpyHostToDevice));
    for (int o = 0; o < 3; ++o)
        if (host[o]) {
            dev[o] = dColumns.get() + o * F;
            GMM_HIP_CHECK(hipMemcpy(dev[o], host[o], F * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
    rc = alignOn(h, dTable.get(), nTableFrames, pruning, dev[0], dev[1], dev[2], outScore ? dScore.get() : nullptr,
                 outHypotheses ? dHypotheses.get() : nullptr, nullptr);
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
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));
    return GMM_OK;
}

}  // extern "C"
