// gmm_scorer.hh -- what the translation units behind include/rasr_gmm.h share: the handle, the owners of its
// device / pinned memory, events and streams, the error helpers and the functions that cross unit borders
// (gmm_create.cc, gmm_score.cc, gmm_hostcall.cc, gmm_group.cc, gmm_state.cc, gmm_api.cc).
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/rasr_gmm.h"
#include "gmm_hostio.hh"
#include "gmm_kernels.hh"
#include "gmm_prepare.hh"
#include "gmm_presel.hh"

namespace rasr_gmm {

void setLastError(const std::string& msg);  // gmm_api.cc: the one thread-local behind gmm_last_error

inline int fail(int code, const std::string& msg) {
    setLastError(msg);
    return code;
}

#define GMM_HIP_CHECK(expr)                                                                         \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(GMM_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

// ---- owners: move-only, released in the destructor (no ordering among them; see ~gmm_scorer, ~DensityGroup) ----

template <class H, auto Free>
class Owned {
public:
    Owned() = default;
    Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    Owned& operator=(Owned&& o) noexcept {
        std::swap(p_, o.p_);
        return *this;
    }
    ~Owned() { (void)reset(); }
    H        get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    hipError_t reset() { return p_ ? Free(std::exchange(p_, nullptr)) : hipSuccess; }

protected:
    H p_ = nullptr;
};

// n elements of device memory (DeviceBuffer<void>: n bytes)
template <class T>
struct DeviceBuffer : Owned<T*, hipFree> {
    static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void_v<T>, char, T>);
    hipError_t alloc(size_t n) {
        (void)this->reset();
        return n ? hipMalloc(reinterpret_cast<void**>(&this->p_), n * kElem) : hipSuccess;
    }
    hipError_t allocFilled(size_t n, int byte) {
        const hipError_t e = alloc(n);
        return e != hipSuccess || n == 0 ? e : hipMemset(this->p_, byte, n * kElem);
    }
    hipError_t allocZeroed(size_t n) { return allocFilled(n, 0); }
};

// page-locked host memory (hipHostMalloc)
template <class T>
struct PinnedBuffer : Owned<T*, hipHostFree> {
    hipError_t alloc(size_t n, unsigned flags) {
        (void)this->reset();
        return hipHostMalloc(reinterpret_cast<void**>(&this->p_), n * sizeof(T), flags);
    }
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) {
        (void)reset();
        return hipEventCreateWithFlags(&p_, flags);
    }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) {
        (void)reset();
        return hipStreamCreateWithFlags(&p_, flags);
    }
};

// dst = src and padElems zero elements after it (U: the element type of a DeviceBuffer<void>'s table)
template <class T, class U>
int upload(DeviceBuffer<T>& dst, const std::vector<U>& src, size_t padElems = 0) {
    static_assert(std::is_void_v<T> || std::is_same_v<T, U>, "element type");
    GMM_HIP_CHECK(dst.allocZeroed((src.size() + padElems) * sizeof(U) / dst.kElem));
    if (!src.empty())
        GMM_HIP_CHECK(hipMemcpy(dst.get(), src.data(), src.size() * sizeof(U), hipMemcpyHostToDevice));
    return GMM_OK;
}

// ---- the kernel choice (gmm_score.cc planFor: the only place that makes it) ----

// the model's part, fixed at creation; a call's plan (LaunchPlan) refines the quantized kernels' frame tile
struct KernelPlan {
    Kernel      kernel         = Kernel::F32;
    uint32_t    framesPerBlock = kF32FramesPerBlock;  // frames per workgroup of a full-size call
    bool        smallTiles     = false;               // quantized, no preselection: 256- / 64-frame tiles for small calls
    uint32_t    launches       = 2;                   // per call: [cluster selection,] frame preparation, scorer
    const char* name           = "scoreF32";          // gmm_scorer_launch_info (bench.py, the PMC summaries)
};

struct LaunchPlan {
    Kernel   kernel;
    uint32_t framesPerBlock;  // of this call
    int      smallTile;       // I8Args::smallTile
    uint32_t nFrameTiles, nFramesRead;  // workgroup columns; frame rows the scorer reads (whole workgroups)
};

// ---- the handle ----

struct ChunkTable {
    uint32_t               nChunks = 0;
    DeviceBuffer<uint32_t> dMixOff;
    // scoreSplitWide: the chunks by the form of the kernel that takes them, one launch each on the call's stream.  A
    // chunk is uniform when its mixtures all have the same tile count T and the kernel is compiled for T
    // (splitWideUniformT).  Empty for every other kernel: one launch over the whole table
    struct Part {
        uint32_t               uniformT = 0;  // 0: the generic form
        uint32_t               nChunks  = 0;
        DeviceBuffer<uint32_t> dList;         // the part's chunks; empty where the part is the whole table
    };
    std::vector<Part> parts;
};

// SIMD-diagonal-maximum, batch-*-int, preselection-batch-int (gmm_kernels_i8.hip)
struct QuantizedModel {
    uint32_t kSteps = 0, idxBits = 1, paddedDimension = 0;
    int      scoreOnly = kScoreOnlyNone;  // score-only layout (no best densities, cheaper epilogue): kScoreOnly*
    float    scaling = 0, scalingSquared = 0, invQ = 0, batchScale = 0;
    std::vector<float>     isvScaled;  // [C][D]
    DeviceBuffer<void>     dTileA, dTileP;
    DeviceBuffer<uint32_t> dTileCov, dMixOddMask;
    DeviceBuffer<int8_t>   dFrameQ;   // frame staging
    DeviceBuffer<int32_t>  dFrameSS;
};

// float types on the split-f16 kernels (gmm_kernels_split.hip)
struct SplitModel {
    uint32_t kSteps16 = 0;    // K steps (32 wide for 16-row tiles, 16 wide for 32-row)
    uint32_t splitRows = 16;  // tile height
    bool     splitCov = false;  // several covariances (covariance-free frame operand)
    uint32_t keyBits = 1;
    float    offsetK0 = 0;
    DeviceBuffer<void>    dTileH, dFrameH;
    DeviceBuffer<float>   dCentre, dDimScale, dFrameXX;  // centre of the expanded quadratic form [D]
    DeviceBuffer<int32_t> dLimbExp, dFrameExp;
};

// float types on the native f32 MFMA kernel (gmm_kernels_f32.hip)
struct F32Model {
    uint32_t kSteps = 0, tileBits = 1;
    bool     foldNorm = false;
    float    offsetK0 = 0;
    DeviceBuffer<void>     dTileA;
    DeviceBuffer<uint32_t> dTileCov, dRowDns;
    DeviceBuffer<float>    dCentre, dFrameX, dFrameXX;
};

// float types in the reference's operation order (GMM_FLAG_REFERENCE_ORDER, gmm_kernels_direct.hip)
struct DirectModel {
    uint32_t               L = 0;  // row length
    DeviceBuffer<float>    dMean, dConst, dLogNorm;
    DeviceBuffer<uint32_t> dCov;
};

// density preselection (preselection-batch-*)
struct Preselection {
    DensityClustering      clustering;
    int                    source = GMM_CLUSTERING_BUILT;  // built, built and written, or read from the archive
    DeviceBuffer<void>     dClusterMeans;
    DeviceBuffer<uint32_t> dSelT;     // [nFramesPad/64][clusters][16]
    DeviceBuffer<uint8_t>  dSelC;     // quantized: [nFramesPad/128][clusters][16] wave-table entries
    DeviceBuffer<void>     dTileClu;  // [tiles + pad][16]: u16 cluster * 64 (float), u32 cluster * 16 (int)
    uint32_t               lastFrames = 0;
};

// sparse best densities (gmm_best_density_pairs, gmm_kernels_pairs.hip): entry-major tables of the assigning
// types in the reference's arithmetic; absent where the model has none (e.g. float D > 128)
struct PairTables {
    int                    kind = kPairSimd;
    uint32_t               L = 0, nb = 0, isvStride = 0;
    uint32_t               nEntries = 0;  // mixture entries of the shard (rows of the tables below)
    uint32_t               maxEntries = 0;  // of one mixture: the least row of gmm_density_posteriors_pairs_*
    DeviceBuffer<uint32_t> dMixOff, dCov;
    DeviceBuffer<uint8_t>  dQMean;
    DeviceBuffer<int32_t>  dQConst;
    DeviceBuffer<float>    dFMean, dFConst, dLogNorm, dIsv;
    // host pair lists: a page-locked staging buffer the kernel reads and writes in place (frame, mixture, best)
    PinnedBuffer<uint32_t> hStage;
    size_t                 stageCap = 0;  // pairs
};

// gmm_state_posteriors_* (gmm_state.cc), allocated by the handle's first call for max_frames: per (piece of
// kStatePieceMixtures mixtures, frame) the piece's minimum, its mixture, its sum and its active cells
struct StateScratch {
    uint32_t               nPieces = 0, stride = 0;  // rows; row length (max_frames)
    DeviceBuffer<double>   dPartMin, dPartSum;
    DeviceBuffer<uint32_t> dPartIdx, dPartCount;
};

// gmm_score_host_ring: the caller's frames are the rows ring[(first + i) % ringSize], i < nFrames
struct HostRing {
    const float* frames;
    uint32_t     ringSize, first, nFrames, frameStride;
};

// [t0, t0 + n) of a call, copied to destination columns [col, col + n)
struct HostSegment {
    uint32_t chunk, t0, n, col;
};

// gmm_score_host* (gmm_hostcall.cc), created by the first host call: device staging of the call's tables; for large
// calls scoring and copy-out streams, one event per frame chunk, a double-buffered pinned staging ring for pageable
// destinations and its copy threads
struct HostPipeline {
    DeviceBuffer<float>    dFrames, dScores, dScoresT;  // ...T: frame-major copies (GMM_HOST_FRAME_MAJOR)
    DeviceBuffer<uint32_t> dBest, dBestT;
    Stream                 compute, copy;
    Event                  start, stageDone[2];
    std::vector<Event>     chunkDone;
    PinnedBuffer<char>     hStage;  // 2 x hStageBytes
    size_t                 hStageBytes = 0;
    std::unique_ptr<HostCopyPool> copyPool;
    // id of the last host call; the one whose best densities dBest keeps (GMM_HOST_KEEP_BEST) with its ring
    // mapping and copy segments, for gmm_fetch_best_density
    uint64_t                 call = 0, keptBestCall = 0;
    HostRing                 keptRing{};
    std::vector<HostSegment> keptSegs;
    bool                     keptFrameMajor = false;
    bool                     keptLazy = false, keptComputed = false;  // GMM_HOST_LAZY_BEST: computed on fetch
    // GMM_HOST_ASYNC: the host call in flight (0: none) and its completion, recorded on copy
    uint64_t asyncCall = 0;
    Event    asyncDone;
};

struct DensityGroup;  // gmm_group.cc
struct DensityGroupDelete {
    void operator()(DensityGroup* g) const;
};

}  // namespace rasr_gmm

struct gmm_scorer {
    using Flavor = rasr_gmm::Flavor;
    gmm_scorer_type   type;
    Flavor            flavor;
    int               device = 0;
    gmm_scorer_config cfg{};
    uint32_t          D = 0, C = 0, nMix = 0, mixBase = 0;
    uint32_t          nMixSet = 0;  // mixtures of the whole set (nMix: of the handle's shard)
    uint32_t          nTiles = 0;  // what chunks are cut by: tiles, or entries (direct)
    uint32_t          nFramesPad = 0;
    // float types: the model's spread statistic and predicted relative error (gmm_prepare.hh kSpreadKappa), which
    // decided between the expanded-form kernels and the reference-order one; 0 with GMM_FLAG_REFERENCE_ORDER
    double            spreadStat = 0, spreadPredicted = 0;
    std::vector<uint32_t>            mixTileOff;  // host copy
    rasr_gmm::DeviceBuffer<uint32_t> dMixTileOff;
    rasr_gmm::DeviceBuffer<float>    dIsv;  // every family's inverse deviations, in its own layout
    rasr_gmm::KernelPlan             plan;
    std::map<uint32_t, rasr_gmm::ChunkTable> chunks;  // keyed by frame tiles per call
    uint32_t          chunkTarget = 0;  // gmm_scorer_set_chunk_target: workgroups a call aims at, 0: the kernel's own
    // kernel timing (gmm_scorer_set_timing)
    bool                                                   timing = false;
    std::vector<std::pair<rasr_gmm::Event, rasr_gmm::Event>> events;
    size_t                                                 eventsUsed = 0;
    // exactly one of the families; none for a density-sharded handle, whose parts hold the models
    std::variant<std::monostate, rasr_gmm::QuantizedModel, rasr_gmm::SplitModel, rasr_gmm::F32Model,
                 rasr_gmm::DirectModel>
            model;
    std::unique_ptr<rasr_gmm::Preselection> presel;
    std::unique_ptr<rasr_gmm::PairTables>   pairs;
    std::unique_ptr<rasr_gmm::StateScratch> state;  // empty until the first gmm_state_posteriors_* call
    rasr_gmm::HostPipeline                  host;  // empty until the first host call
    // density-sharded handle (gmm_scorer_create_sharded): the parts score, this handle holds the full-table host
    // staging on devices[0]
    std::unique_ptr<rasr_gmm::DensityGroup, rasr_gmm::DensityGroupDelete> group;
    // SIMD-diagonal-maximum: the same model on the score-only class layout, which every call without a best
    // density table runs (gmm_score_device with best_density NULL, GMM_HOST_LAZY_BEST host calls): the
    // reference's score(e) without the index-carrying pack, bit-identical scores
    std::unique_ptr<gmm_scorer> scoresOnly;
    // the caller's cache_archive string is only valid during create: keep a copy, and cfg.cache_archive stays null
    std::string cacheArchive;

    const rasr_gmm::QuantizedModel* quantized() const { return std::get_if<rasr_gmm::QuantizedModel>(&model); }
    bool multiCov() const { return C > 1; }
    // types with an assignment (AssigningFeatureScorer: SIMD-diagonal-maximum, diagonal-maximum, diagonal-sum)
    bool hasAssignment() const {
        return flavor == Flavor::Simd || flavor == Flavor::DiagonalMaximum || flavor == Flavor::DiagonalSum;
    }

    ~gmm_scorer() {
        if (host.asyncCall && host.asyncDone)
            (void)hipEventSynchronize(host.asyncDone.get());  // no DMA into a caller's table may outlive the scorer
    }
};

namespace rasr_gmm {

// the quantized flavours (SIMD-diagonal-maximum, batch-*-int): also of a handle without a model (sharded)
inline bool isQuantized(Flavor f) {
    return f == Flavor::Simd || f == Flavor::BatchInt;
}
inline bool isPreselection(gmm_scorer_type t) {
    return t == GMM_BATCH_PRESELECTION_FLOAT || t == GMM_BATCH_PRESELECTION_INT;
}
Flavor flavorOf(gmm_scorer_type t, bool* ok);  // gmm_create.cc

// gmm_score.cc
KernelPlan kernelPlanOf(const gmm_scorer& s);                         // from type, flags and the model's scalars
uint32_t   paddedFrames(const KernelPlan& plan, uint32_t maxFrames);  // rows of the frame tables (nFramesPad)
LaunchPlan planFor(const gmm_scorer& s, uint32_t nFrames);
int        scoreImpl(gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride, float* scores,
                     uint32_t* best, uint32_t scoreStride, hipStream_t stream);
// the GMM_HOST_ASYNC call in flight, if any, is complete on return: its staging (frames, prepared frames,
// device tables) is free for the next call of any kind
int waitAsync(gmm_scorer* s);

// gmm_hostcall.cc: the sparse best-density path (also the Viterbi branch of gmm_estimator_accumulate_*)
int      checkPairs(const gmm_scorer* s);  // GMM_ERR_UNSUPPORTED: batch types, sharded handles, no pair tables
PairArgs pairArgsOf(const gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride);
// checkPairs, and GMM_ERR_UNSUPPORTED for every type but diagonal-sum (gmm_density_posteriors_pairs_*, the Baum-Welch
// branch of gmm_estimator_accumulate_posteriors_*)
int checkPosteriors(const gmm_scorer* s);

// gmm_group.cc
int groupScore(gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride, float* scores,
               uint32_t* best, uint32_t scoreStride, hipStream_t stream);
// the handle whose prepared model answers model queries (quantization, launch info): a part's
const gmm_scorer* modelOf(const gmm_scorer* s);
std::vector<gmm_scorer*> partsOf(gmm_scorer* s);  // the parts of a sharded handle that hold mixtures

}  // namespace rasr_gmm
