// gmm_align.cc -- the handle behind include/rasr_gmm_align.h: its device memory (the batch's tables and the
// backpointer scratch, all allocated at creation), set_segments (host/AlignGraph.cc validates and builds, this unit
// uploads), the checks and the launch of the calls of both modes (gmm_kernels_align.hip, gmm_kernels_align_posterior.hip)
// and the host calls' staging.  A call travels as small structs: the table, the mode's outputs, the search part.
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

// the outputs of a Viterbi call, device or host pointers as the call is; each may be NULL
struct ViterbiOut {
    uint32_t *mixture, *state, *arc;  // [table columns]
    float*    score;                  // [nSegments]
    uint32_t* hypotheses;             // [nSegments]
};

// what a Baum-Welch call adds to the table and the threshold: the item filter and capacity, and the outputs
struct PosteriorOut {
    float     minPosterior;
    uint32_t  maxItems;
    uint32_t *itemFrame, *itemMixture;
    double*   itemWeight;
    uint32_t *columnOffset, *nItems;
    float*    score;
    uint32_t* hypotheses;
    double*   logTotal;
};

// the checks of all calls; nothing is written or enqueued before they pass
int checkCall(const gmm_aligner* h, const AlignTable& t, bool anyOutput) {
    if (!h)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null aligner");
    if (!t.scores)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: null scores");
    if (!anyOutput)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: no output requested");
    if (h->nSegments == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: no segments set");
    if (t.scoreStride < t.nTableFrames)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: score_stride below n_table_frames");
    if (h->frameEnd > t.nTableFrames)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: a segment ends at column " + std::to_string(h->frameEnd) +
                                                      ", past n_table_frames " + std::to_string(t.nTableFrames));
    return GMM_OK;
}

int checkModeCall(const gmm_aligner* h, const AlignTable& t, const ViterbiOut& o) {
    return checkCall(h, t, o.mixture || o.state || o.arc || o.score || o.hypotheses);
}

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

// the batch part of both modes' arguments
void fillBatch(const gmm_aligner* h, AlignBatch& b) {
    b.segments    = h->dSegments.get();
    b.order       = h->dOrder.get();
    b.inOffset    = h->dInOffset.get();
    b.inSource    = h->dInSource.get();
    b.inArc       = h->dInArc.get();
    b.inMixture   = h->dInMixture.get();
    b.inWeight    = h->dInWeight.get();
    b.finalWeight = h->dFinalWeight.get();
    b.nSegments   = h->nSegments;
    b.rowStates   = h->rowStates;
}

// what was enqueued uses the handle's tables and scratch: the event is recorded whether or not the launch failed
int recordDone(gmm_aligner* h, hipError_t launched, hipStream_t stream) {
    GMM_HIP_CHECK(hipEventRecord(h->done.get(), stream));
    h->pending = true;
    GMM_HIP_CHECK(launched);
    return GMM_OK;
}

int callOn(gmm_aligner* h, const AlignTable& table, float pruning, const ViterbiOut& o, const AlignSearchCall& search,
            hipStream_t stream) {
    AlignArgs a{};
    fillBatch(h, a);
    static_cast<AlignTable&>(a) = table;
    a.search                    = search;
    a.pruning                   = pruning;
    a.cells                     = h->dCells.get();
    a.outMixture                = o.mixture;
    a.outState                  = o.state;
    a.outArc                    = o.arc;
    a.outScore                  = o.score;
    a.outHypotheses             = o.hypotheses;
    return recordDone(h, launchAlign(a, stream), stream);
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
int checkModeCall(const gmm_aligner* h, const AlignTable& t, const PosteriorOut& o) {
    const bool items = o.itemFrame || o.itemMixture || o.itemWeight;
    const int  rc = checkCall(h, t, o.itemFrame || o.columnOffset || o.nItems || o.score || o.logTotal || o.hypotheses);
    if (rc != GMM_OK)
        return rc;
    if (items && !(o.itemFrame && o.itemMixture && o.itemWeight))
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: out_item_frame, out_item_mixture and out_item_weight go together");
    if (items && o.maxItems == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "aligner: item arrays with max_items 0");
    if (h->maxSegmentStates > GMM_ALIGN_MAX_STATES_POSTERIOR)
        return fail(GMM_ERR_UNSUPPORTED, "aligner: a segment has " + std::to_string(h->maxSegmentStates) +
                                                 " states, more than GMM_ALIGN_MAX_STATES_POSTERIOR " +
                                                 std::to_string(GMM_ALIGN_MAX_STATES_POSTERIOR));
    if (h->posterior.nFrames > 0xffffffffull)
        return fail(GMM_ERR_UNSUPPORTED, "aligner: 2^32 frames or more in one batch");
    return GMM_OK;
}

int callOn(gmm_aligner* h, const AlignTable& table, float pruning, const PosteriorOut& o, const AlignSearchCall& search,
           hipStream_t stream) {
    const int rc = preparePosterior(h);
    if (rc != GMM_OK)
        return rc;
    AlignPosteriorArgs a{};
    fillBatch(h, a);
    static_cast<AlignTable&>(a) = table;
    a.search                    = search;
    a.arcOffset                 = h->dArcOffset.get();
    a.arcTarget                 = h->dArcTarget.get();
    a.arcMixture                = h->dArcMixture.get();
    a.arcWeight                 = h->dArcWeight.get();
    a.groupOffset               = h->dGroupOffset.get();
    a.groupMixture              = h->dGroupMixture.get();
    a.groupArcOffset            = h->dGroupArcOffset.get();
    a.groupSource               = h->dGroupSource.get();
    a.groupTarget               = h->dGroupTarget.get();
    a.groupWeight               = h->dGroupWeight.get();
    a.colSegment                = h->dColSegment.get();
    a.colFrameOffset            = h->dColFrameOffset.get();
    a.pruning                   = pruning;
    a.minPosterior              = o.minPosterior;
    a.maxItems                  = o.maxItems;
    a.fwPot                     = h->dFwPot.get();
    a.bwPot                     = h->dBwPot.get();
    a.mark                      = h->dMark.get();
    a.segTotalInv               = h->dSegTotalInv.get();
    a.segHas                    = h->dSegHas.get();
    a.frameMin                  = h->dFrameMin.get();
    a.frameInv                  = h->dFrameInv.get();
    a.frameCount                = h->dFrameCount.get();
    a.waveWeights               = h->dWaveWeights.get();
    a.rowGroups                 = h->rowGroups;
    a.outItemFrame              = o.itemFrame;
    a.outItemMixture            = o.itemMixture;
    a.outItemWeight             = o.itemWeight;
    a.outColumnOffset           = o.columnOffset;
    a.outNItems                 = o.nItems;
    a.outScore                  = o.score;
    a.outHypotheses             = o.hypotheses;
    a.outLogTotal               = o.logTotal;
    a.nFrames                   = static_cast<uint32_t>(h->posterior.nFrames);
    return recordDone(h, launchAlignPosteriors(a, stream), stream);
}

// An optional output of a host call, staged on the device: room for it if the host pointer is set, the device pointer or
// NULL for the launch, the copy back of its first elements
template <class T>
struct Staged {
    T*              host = nullptr;
    size_t          size = 0;
    DeviceBuffer<T> dev;

    hipError_t alloc(T* hostPointer, size_t n) {
        host = hostPointer;
        size = n;
        return host ? dev.alloc(n) : hipSuccess;
    }
    T*         get() const { return host ? dev.get() : nullptr; }
    hipError_t send() const {
        return host && size ? hipMemcpy(dev.get(), host, size * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    }
    hipError_t fetch(size_t n) const {
        return host && n ? hipMemcpy(host, dev.get(), n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
    }
    hipError_t fetch() const { return fetch(size); }
};

// The staging that both host calls share: the device is set and the last call's kernels are done before anything is
// staged; the table, dense; the per-segment outputs of both modes and of the search
struct HostCall {
    DeviceBuffer<float> dTable;
    Staged<float>       score, threshold;
    Staged<uint32_t>    hypotheses, iterations;
    AlignTable          table{};   // the staged table
    AlignSearchCall     search{};  // the search with the staged outputs

    int begin(gmm_aligner* h, const AlignTable& t, float* outScore, uint32_t* outHypotheses, const AlignSearchCall& hs) {
        GMM_HIP_CHECK(hipSetDevice(h->device));
        const int rc = waitDone(h);
        if (rc != GMM_OK)
            return rc;
        const size_t F = t.nTableFrames, M = h->cap.nMixtures, S = h->nSegments;
        GMM_HIP_CHECK(dTable.alloc(M * F));
        GMM_HIP_CHECK(score.alloc(outScore, S));
        GMM_HIP_CHECK(hypotheses.alloc(outHypotheses, S));
        GMM_HIP_CHECK(threshold.alloc(hs.outThreshold, S));
        GMM_HIP_CHECK(iterations.alloc(hs.outIterations, S));
        if (F)
            GMM_HIP_CHECK(hipMemcpy2D(dTable.get(), F * sizeof(float), t.scores,
                                      static_cast<size_t>(t.scoreStride) * sizeof(float), F * sizeof(float), M,
                                      hipMemcpyHostToDevice));
        table                = AlignTable{dTable.get(), t.nTableFrames, t.nTableFrames};
        search               = hs;
        search.outThreshold  = threshold.get();
        search.outIterations = iterations.get();
        return GMM_OK;
    }
    // the copies on the default stream wait for the kernels and are synchronous
    int fetch() const {
        GMM_HIP_CHECK(score.fetch());
        GMM_HIP_CHECK(hypotheses.fetch());
        GMM_HIP_CHECK(threshold.fetch());
        GMM_HIP_CHECK(iterations.fetch());
        return GMM_OK;
    }
};

// both host align calls, behind their checks; hs: the search with its HOST outputs
int callHost(gmm_aligner* h, const AlignTable& table, float pruning, const ViterbiOut& o, const AlignSearchCall& hs) {
    HostCall call;
    int      rc = call.begin(h, table, o.score, o.hypotheses, hs);
    if (rc != GMM_OK)
        return rc;
    // the per-column outputs start from the host arrays, whose columns of no segment are kept
    Staged<uint32_t> columns[3];
    uint32_t* const  host[3] = {o.mixture, o.state, o.arc};
    for (int c = 0; c < 3; ++c) {
        GMM_HIP_CHECK(columns[c].alloc(host[c], table.nTableFrames));
        GMM_HIP_CHECK(columns[c].send());
    }
    const ViterbiOut staged{columns[0].get(), columns[1].get(), columns[2].get(), call.score.get(),
                            call.hypotheses.get()};
    rc = callOn(h, call.table, pruning, staged, call.search, nullptr);
    if (rc != GMM_OK) {
        (void)hipStreamSynchronize(nullptr);  // the buffers go with this scope
        return rc;
    }
    for (const Staged<uint32_t>& c : columns)
        GMM_HIP_CHECK(c.fetch());
    if ((rc = call.fetch()) != GMM_OK)
        return rc;
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));
    return GMM_OK;
}

// both host posterior calls, behind their checks; hs: the search with its HOST outputs
int callHost(gmm_aligner* h, const AlignTable& table, float pruning, const PosteriorOut& o, const AlignSearchCall& hs) {
    HostCall call;
    int      rc = call.begin(h, table, o.score, o.hypotheses, hs);
    if (rc != GMM_OK)
        return rc;
    const size_t           I = o.itemFrame ? o.maxItems : 0;
    Staged<uint32_t>       itemFrame, itemMixture, columnOffset;
    Staged<double>         itemWeight, logTotal;
    DeviceBuffer<uint32_t> dCount;  // read back whether or not the caller asks for it
    GMM_HIP_CHECK(itemFrame.alloc(o.itemFrame, I));
    GMM_HIP_CHECK(itemMixture.alloc(o.itemMixture, I));
    GMM_HIP_CHECK(itemWeight.alloc(o.itemWeight, I));
    GMM_HIP_CHECK(columnOffset.alloc(o.columnOffset, static_cast<size_t>(table.nTableFrames) + 1));
    GMM_HIP_CHECK(logTotal.alloc(o.logTotal, h->nSegments));
    GMM_HIP_CHECK(dCount.alloc(1));
    const PosteriorOut staged{o.minPosterior,   o.maxItems,         itemFrame.get(), itemMixture.get(),
                              itemWeight.get(), columnOffset.get(), dCount.get(),    call.score.get(),
                              call.hypotheses.get(), logTotal.get()};
    rc = callOn(h, call.table, pruning, staged, call.search, nullptr);
    if (rc != GMM_OK) {
        (void)hipStreamSynchronize(nullptr);  // the buffers go with this scope
        return rc;
    }
    uint32_t count = 0;
    GMM_HIP_CHECK(hipMemcpy(&count, dCount.get(), sizeof(count), hipMemcpyDeviceToHost));
    if (o.nItems)
        *o.nItems = count;
    if ((rc = call.fetch()) != GMM_OK)
        return rc;
    GMM_HIP_CHECK(logTotal.fetch());
    if (I && count > o.maxItems) {
        GMM_HIP_CHECK(hipStreamSynchronize(nullptr));
        return fail(GMM_ERR_CAPACITY, "aligner: the call produces " + std::to_string(count) + " items, more than max_items " +
                                              std::to_string(o.maxItems));
    }
    GMM_HIP_CHECK(itemFrame.fetch(count));
    GMM_HIP_CHECK(itemMixture.fetch(count));
    GMM_HIP_CHECK(itemWeight.fetch(count));
    GMM_HIP_CHECK(columnOffset.fetch());
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));
    return GMM_OK;
}

// the search part of a search call before its checks: on, with the call's two outputs; `rule` is checkSearch's to fill
AlignSearchCall searchOn(float* outThreshold, uint32_t* outIterations) {
    return AlignSearchCall{AlignSearch{}, outThreshold, outIterations, 1};
}

// A call of either mode behind its entry point: the mode's checks and, in a search call (sc.on), the search's on the
// caller's `rule`; then the launch on *stream on the handle's device or, without a stream, the host path
template <class Out>
int runCall(gmm_aligner* h, const AlignTable& table, float pruning, const Out& out, const gmm_align_search* rule,
            AlignSearchCall sc, const hipStream_t* stream) {
    int rc = checkModeCall(h, table, out);
    if (rc == GMM_OK && sc.on)
        rc = checkSearch(rule, sc.rule);
    if (rc != GMM_OK)
        return rc;
    if (!stream)
        return callHost(h, table, pruning, out, sc);
    GMM_HIP_CHECK(hipSetDevice(h->device));
    return callOn(h, table, pruning, out, sc, *stream);
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

// The calls: each builds the structs of the call for runCall.  A search call has no threshold of its
// own: the kernels ignore `pruning`

int gmm_aligner_align_device(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                             float pruning, uint32_t* outMixture, uint32_t* outState, uint32_t* outArc, float* outScore,
                             uint32_t* outHypotheses, void* stream) {
    const hipStream_t on = static_cast<hipStream_t>(stream);
    return runCall<ViterbiOut>(h, {scores, scoreStride, nTableFrames}, pruning,
                               {outMixture, outState, outArc, outScore, outHypotheses}, nullptr,
                               AlignSearchCall{}, &on);
}

int gmm_aligner_align_host(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride, float pruning,
                           uint32_t* outMixture, uint32_t* outState, uint32_t* outArc, float* outScore,
                           uint32_t* outHypotheses) {
    return runCall<ViterbiOut>(h, {scores, scoreStride, nTableFrames}, pruning,
                               {outMixture, outState, outArc, outScore, outHypotheses}, nullptr,
                               AlignSearchCall{}, nullptr);
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
    const hipStream_t on = static_cast<hipStream_t>(stream);
    return runCall<ViterbiOut>(h, {scores, scoreStride, nTableFrames}, 0.0f,
                               {outMixture, outState, outArc, outScore, outHypotheses}, search,
                               searchOn(outThreshold, outIterations), &on);
}

int gmm_aligner_align_search_host(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                  const gmm_align_search* search, uint32_t* outMixture, uint32_t* outState,
                                  uint32_t* outArc, float* outScore, uint32_t* outHypotheses, float* outThreshold,
                                  uint32_t* outIterations) {
    return runCall<ViterbiOut>(h, {scores, scoreStride, nTableFrames}, 0.0f,
                               {outMixture, outState, outArc, outScore, outHypotheses}, search,
                               searchOn(outThreshold, outIterations), nullptr);
}

int gmm_aligner_posteriors_device(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                  float pruning, float minPosterior, uint32_t maxItems, uint32_t* itemFrame,
                                  uint32_t* itemMixture, double* itemWeight, uint32_t* columnOffset, uint32_t* nItems,
                                  float* outScore, uint32_t* outHypotheses, double* logTotal, void* stream) {
    const hipStream_t on = static_cast<hipStream_t>(stream);
    return runCall<PosteriorOut>(h, {scores, scoreStride, nTableFrames}, pruning,
                                 {minPosterior, maxItems, itemFrame, itemMixture, itemWeight, columnOffset, nItems,
                                  outScore, outHypotheses, logTotal},
                                 nullptr, AlignSearchCall{}, &on);
}

int gmm_aligner_posteriors_host(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                float pruning, float minPosterior, uint32_t maxItems, uint32_t* itemFrame,
                                uint32_t* itemMixture, double* itemWeight, uint32_t* columnOffset, uint32_t* nItems,
                                float* outScore, uint32_t* outHypotheses, double* logTotal) {
    return runCall<PosteriorOut>(h, {scores, scoreStride, nTableFrames}, pruning,
                                 {minPosterior, maxItems, itemFrame, itemMixture, itemWeight, columnOffset, nItems,
                                  outScore, outHypotheses, logTotal},
                                 nullptr, AlignSearchCall{}, nullptr);
}

int gmm_aligner_posteriors_search_device(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                         const gmm_align_search* search, float minPosterior, uint32_t maxItems,
                                         uint32_t* itemFrame, uint32_t* itemMixture, double* itemWeight,
                                         uint32_t* columnOffset, uint32_t* nItems, float* outScore, uint32_t* outHypotheses,
                                         double* logTotal, float* outThreshold, uint32_t* outIterations, void* stream) {
    const hipStream_t on = static_cast<hipStream_t>(stream);
    return runCall<PosteriorOut>(h, {scores, scoreStride, nTableFrames}, 0.0f,
                                 {minPosterior, maxItems, itemFrame, itemMixture, itemWeight, columnOffset, nItems,
                                  outScore, outHypotheses, logTotal},
                                 search, searchOn(outThreshold, outIterations), &on);
}

int gmm_aligner_posteriors_search_host(gmm_aligner* h, const float* scores, uint32_t nTableFrames, uint32_t scoreStride,
                                       const gmm_align_search* search, float minPosterior, uint32_t maxItems,
                                       uint32_t* itemFrame, uint32_t* itemMixture, double* itemWeight,
                                       uint32_t* columnOffset, uint32_t* nItems, float* outScore, uint32_t* outHypotheses,
                                       double* logTotal, float* outThreshold, uint32_t* outIterations) {
    return runCall<PosteriorOut>(h, {scores, scoreStride, nTableFrames}, 0.0f,
                                 {minPosterior, maxItems, itemFrame, itemMixture, itemWeight, columnOffset, nItems,
                                  outScore, outHypotheses, logTotal},
                                 search, searchOn(outThreshold, outIterations), nullptr);
}

}  // extern "C"
