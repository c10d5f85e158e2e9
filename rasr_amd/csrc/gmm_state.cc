// gmm_state.cc -- gmm_state_posteriors_*: the checks, the handle's scratch and the launch of gmm_kernels_state.hip;
// the host call stages frames, scores them with the handle's own scoring path and copies the outputs out.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "gmm_scorer.hh"

using namespace rasr_gmm;

static_assert(kStatePieceMixtures == GMM_STATE_POSTERIOR_CHUNK, "the kernels' piece is the contract's chunk");

namespace {

// the checks of both calls that need no device; nothing is written or allocated before they pass
int checkStateCall(const gmm_scorer* s, const void* input, uint32_t nFrames, uint32_t inputStrideOk, double scale,
                   const float* post32, const double* post64, uint32_t postStride, const double* logZ,
                   const double* minScore, const uint32_t* minIndex, const uint32_t* nActive) {
    if (!s || !input)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    if (s->group)
        return fail(GMM_ERR_UNSUPPORTED, "state posteriors are not defined for a density-sharded handle");
    if (s->nMix != s->nMixSet)
        return fail(GMM_ERR_UNSUPPORTED, "the handle holds a mixture shard: a shard cannot normalise over the mixtures");
    if (!post32 && !post64 && !logZ && !minScore && !minIndex && !nActive)
        return fail(GMM_ERR_INVALID_ARGUMENT, "no output requested");
    if (std::isnan(scale))
        return fail(GMM_ERR_INVALID_ARGUMENT, "scale is NaN");
    if (nFrames > s->cfg.max_frames)
        return fail(GMM_ERR_CAPACITY, "n_frames exceeds config.max_frames");
    if (!inputStrideOk || ((post32 || post64) && postStride < nFrames))
        return fail(GMM_ERR_INVALID_ARGUMENT, "stride below n_frames");
    return GMM_OK;
}

int ensureStateScratch(gmm_scorer* s) {
    if (s->state)
        return GMM_OK;
    auto           st = std::make_unique<StateScratch>();
    st->nPieces       = (s->nMix + kStatePieceMixtures - 1) / kStatePieceMixtures;
    st->stride        = s->cfg.max_frames;
    const size_t n    = static_cast<size_t>(st->nPieces) * st->stride;
    GMM_HIP_CHECK(st->dPartMin.alloc(n));
    GMM_HIP_CHECK(st->dPartSum.alloc(n));
    GMM_HIP_CHECK(st->dPartIdx.alloc(n));
    GMM_HIP_CHECK(st->dPartCount.alloc(n));
    s->state = std::move(st);
    return GMM_OK;
}

int statePosteriorsOn(gmm_scorer* s, const float* scores, uint32_t nFrames, uint32_t scoreStride, const double* priors,
                      double scale, double pruningThreshold, float* post32, double* post64, uint32_t postStride,
                      double* logZ, double* minScore, uint32_t* minIndex, uint32_t* nActive, hipStream_t stream) {
    if (nFrames == 0 || s->nMix == 0)
        return GMM_OK;
    // one workgroup per (256 frames, piece)
    const uint64_t groups = static_cast<uint64_t>((nFrames + 255u) / 256u) * ((s->nMix + kStatePieceMixtures - 1) / kStatePieceMixtures);
    if (groups > 0x7fffffffull)
        return fail(GMM_ERR_UNSUPPORTED, "too many (frame block, piece) workgroups for one launch");
    GMM_HIP_CHECK(hipSetDevice(s->device));
    const int rc = ensureStateScratch(s);
    if (rc != GMM_OK)
        return rc;
    const StateScratch& st = *s->state;
    StateArgs           a{};
    a.scores           = scores;
    a.priors           = priors;
    a.scale            = scale;
    a.pruningThreshold = pruningThreshold;
    a.post32           = post32;
    a.post64           = post64;
    a.logZ             = logZ;
    a.minScore         = minScore;
    a.minIndex         = minIndex;
    a.nActive          = nActive;
    a.partMin          = st.dPartMin.get();
    a.partIdx          = st.dPartIdx.get();
    a.partSum          = st.dPartSum.get();
    a.partCount        = st.dPartCount.get();
    a.nFrames          = nFrames;
    a.nMixtures        = s->nMix;
    a.scoreStride      = scoreStride;
    a.postStride       = postStride;
    a.partStride       = st.stride;
    a.nPieces          = st.nPieces;
    GMM_HIP_CHECK(launchStatePosteriors(a, stream));
    return GMM_OK;
}

}  // namespace

extern "C" {

int gmm_state_posteriors_device(gmm_scorer* s, const float* scores, uint32_t nFrames, uint32_t scoreStride,
                                const double* priors, double scale, double pruningThreshold, float* post32,
                                double* post64, uint32_t postStride, double* logZ, double* minScore, uint32_t* minIndex,
                                uint32_t* nActive, void* stream) {
    const int rc = checkStateCall(s, scores, nFrames, scoreStride >= nFrames, scale, post32, post64, postStride, logZ,
                                  minScore, minIndex, nActive);
    if (rc != GMM_OK)
        return rc;
    if (post32 == scores && postStride != scoreStride)
        return fail(GMM_ERR_INVALID_ARGUMENT, "posteriors_f32 aliases scores with another stride");
    if (static_cast<const void*>(post64) == static_cast<const void*>(scores))
        return fail(GMM_ERR_INVALID_ARGUMENT, "posteriors_f64 cannot alias scores");
    return statePosteriorsOn(s, scores, nFrames, scoreStride, priors, scale, pruningThreshold, post32, post64, postStride,
                             logZ, minScore, minIndex, nActive, static_cast<hipStream_t>(stream));
}

int gmm_state_posteriors_host(gmm_scorer* s, const float* frames, uint32_t nFrames, uint32_t frameStride,
                              const double* priors, double scale, double pruningThreshold, float* post32, double* post64,
                              uint32_t postStride, double* logZ, double* minScore, uint32_t* minIndex, uint32_t* nActive) {
    int rc = checkStateCall(s, frames, nFrames, true, scale, post32, post64, postStride, logZ, minScore, minIndex, nActive);
    if (rc != GMM_OK)
        return rc;
    if (frameStride < s->D)
        return fail(GMM_ERR_INVALID_ARGUMENT, "frame_stride below the dimension");
    if (nFrames == 0 || s->nMix == 0)
        return GMM_OK;
    if ((rc = waitAsync(s)) != GMM_OK)  // a GMM_HOST_ASYNC call still uses the frame staging of the scoring path
        return rc;
    GMM_HIP_CHECK(hipSetDevice(s->device));
    // the frames, dense; the score table, dense, which the f32 posteriors replace in place; the other outputs
    const size_t           D = s->D, F = nFrames, M = s->nMix;
    DeviceBuffer<float>    dFrames, dTable;
    DeviceBuffer<double>   dPriors, dPost64, dPerFrame;  // dPerFrame: logZ, minimum score
    DeviceBuffer<uint32_t> dPerFrameU;                   // minimum index, active cells
    GMM_HIP_CHECK(dFrames.alloc(F * D));
    GMM_HIP_CHECK(dTable.alloc(M * F));
    GMM_HIP_CHECK(dPerFrame.alloc(2 * F));
    GMM_HIP_CHECK(dPerFrameU.alloc(2 * F));
    if (post64)
        GMM_HIP_CHECK(dPost64.alloc(M * F));
    if (priors) {
        GMM_HIP_CHECK(dPriors.alloc(M));
        GMM_HIP_CHECK(hipMemcpy(dPriors.get(), priors, M * sizeof(double), hipMemcpyHostToDevice));
    }
    GMM_HIP_CHECK(hipMemcpy2D(dFrames.get(), D * sizeof(float), frames, static_cast<size_t>(frameStride) * sizeof(float),
                              D * sizeof(float), F, hipMemcpyHostToDevice));
    if ((rc = scoreImpl(s, dFrames.get(), nFrames, s->D, dTable.get(), nullptr, nFrames, nullptr)) == GMM_OK)
        rc = statePosteriorsOn(s, dTable.get(), nFrames, nFrames, dPriors.get(), scale, pruningThreshold,
                               post32 ? dTable.get() : nullptr, dPost64.get(), nFrames, dPerFrame.get(),
                               dPerFrame.get() + F, dPerFrameU.get(), dPerFrameU.get() + F, nullptr);
    if (rc != GMM_OK) {
        (void)hipStreamSynchronize(nullptr);  // the buffers go with this scope
        return rc;
    }
    // the copies on the default stream wait for the kernels and are synchronous: the buffers may go afterwards
    if (post32)
        GMM_HIP_CHECK(hipMemcpy2D(post32, static_cast<size_t>(postStride) * sizeof(float), dTable.get(), F * sizeof(float),
                                  F * sizeof(float), M, hipMemcpyDeviceToHost));
    if (post64)
        GMM_HIP_CHECK(hipMemcpy2D(post64, static_cast<size_t>(postStride) * sizeof(double), dPost64.get(),
                                  F * sizeof(double), F * sizeof(double), M, hipMemcpyDeviceToHost));
    if (logZ)
        GMM_HIP_CHECK(hipMemcpy(logZ, dPerFrame.get(), F * sizeof(double), hipMemcpyDeviceToHost));
    if (minScore)
        GMM_HIP_CHECK(hipMemcpy(minScore, dPerFrame.get() + F, F * sizeof(double), hipMemcpyDeviceToHost));
    if (minIndex)
        GMM_HIP_CHECK(hipMemcpy(minIndex, dPerFrameU.get(), F * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (nActive)
        GMM_HIP_CHECK(hipMemcpy(nActive, dPerFrameU.get() + F, F * sizeof(uint32_t), hipMemcpyDeviceToHost));
    GMM_HIP_CHECK(hipStreamSynchronize(nullptr));
    return GMM_OK;
}

}  // extern "C"
