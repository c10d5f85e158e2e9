// gmm_api.cc -- C-ABI of the MI355X GMM feature scorer (include/rasr_gmm.h): the entry points that are one screen
// each -- accessors, kernel timing, quantization and clustering queries, cache-archive items, the exchange keys --
// and the library's last error, version and kernel id.  Creation, scoring, the host calls and the density-sharded
// handle have their own units (gmm_scorer.hh lists them).
#include <algorithm>
#include <cstring>

#include "gmm_scorer.hh"
#include "kernel_id.h"  // build/kernel_id.h (Makefile): GMM_KERNEL_ID

using namespace rasr_gmm;

namespace {
thread_local std::string gLastError;
}  // namespace

namespace rasr_gmm {
// shared with the other C-ABI translation units (gmm_scorer.hh fail(), host/MixtureSetFile.cc, gmm_shard.cc)
void setLastError(const std::string& msg) {
    gLastError = msg;
}
}  // namespace rasr_gmm

extern "C" {

void gmm_default_config(gmm_scorer_config* cfg) {
    if (!cfg)
        return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->mixture_weight_scale = 1.0f;
    cfg->gaussian_scale       = 1.0f;
    cfg->score_scale          = 1.0f;
    cfg->max_frames           = 4;  // "buffer-size" default, BatchFeatureScorer.cc:28-29
    cfg->clusters              = 256;  // DensityClustering.cc:19-32
    cfg->select_clusters       = 32;
    cfg->clustering_iterations = 5;
    cfg->backoff_score         = 40000.0f;
}

uint32_t gmm_scorer_n_mixtures(const gmm_scorer* s) {
    return s ? s->nMix : 0;
}

uint32_t gmm_scorer_dimension(const gmm_scorer* s) {
    return s ? s->D : 0;
}

uint32_t gmm_scorer_n_covariances(const gmm_scorer* s) {
    return s ? s->C : 0;
}

int gmm_scorer_type_of(const gmm_scorer* s) {
    return s ? static_cast<int>(s->type) : -1;
}

int gmm_host_alloc(size_t bytes, void** ptr) {
    if (!ptr)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null ptr");
    *ptr = nullptr;
    if (bytes == 0)
        return GMM_OK;
    GMM_HIP_CHECK(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
    return GMM_OK;
}

int gmm_host_free(void* ptr) {
    if (ptr)
        GMM_HIP_CHECK(hipHostFree(ptr));
    return GMM_OK;
}

int gmm_scorer_quantization(const gmm_scorer* s, float* scaling, float* invQ) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    s = modelOf(s);  // a sharded handle: its parts share the model-global quantization scale
    const QuantizedModel* q = s->quantized();
    if (!q)
        return fail(GMM_ERR_UNSUPPORTED, "scorer type is not quantized");
    if (scaling)
        *scaling = q->scaling;
    if (invQ)
        *invQ = q->invQ;
    return GMM_OK;
}

int gmm_scorer_multiply_and_quantize(const gmm_scorer* s, const float* feature, uint8_t* out) {
    if (!s || !feature || !out)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    s = modelOf(s);
    const QuantizedModel* q = s->quantized();
    if (!q)
        return fail(GMM_ERR_UNSUPPORTED, "scorer type is not quantized");
    const uint32_t Dp = q->paddedDimension;
    for (uint32_t c = 0; c < s->C; ++c) {
        uint8_t* r = out + static_cast<size_t>(c) * Dp;
        for (uint32_t k = 0; k < s->D; ++k)
            r[k] = refQuantize(feature[k] * q->isvScaled[static_cast<size_t>(c) * s->D + k]);
        for (uint32_t k = s->D; k < Dp; ++k)
            r[k] = 0;
    }
    return GMM_OK;
}

int gmm_prepare_quantized_host(const gmm_mixture_set* ms, gmm_scorer_type type, float* scaling, float* isv,
                               float* logNorm, uint8_t* preparedMean, int32_t* constantWeight) {
    if (!ms)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null mixture set");
    bool   ok     = false;
    Flavor flavor = flavorOf(type, &ok);
    if (!ok || !isQuantized(flavor))
        return fail(GMM_ERR_UNSUPPORTED, "type is not a quantized scorer");
    PreparedQuantized p;
    std::string       err = prepareQuantized(*ms, flavor, ShardRange{}, p);
    if (!err.empty())
        return fail(GMM_ERR_INVALID_ARGUMENT, err);
    if (scaling)
        *scaling = p.scaling;
    if (isv)
        std::copy(p.isvScaled.begin(), p.isvScaled.end(), isv);
    if (logNorm)
        std::copy(p.logNormScaled.begin(), p.logNormScaled.end(), logNorm);
    if (preparedMean)
        std::copy(p.preparedMean.begin(), p.preparedMean.end(), preparedMean);
    if (constantWeight)
        std::copy(p.constantWeight.begin(), p.constantWeight.end(), constantWeight);
    return GMM_OK;
}

int gmm_scorer_set_timing(gmm_scorer* s, int enable) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    s->timing     = enable != 0;
    s->eventsUsed = 0;
    if (s->scoresOnly)
        gmm_scorer_set_timing(s->scoresOnly.get(), enable);
    for (gmm_scorer* part : partsOf(s))  // sharded: every part times its own kernels
        gmm_scorer_set_timing(part, enable);
    return GMM_OK;
}

int gmm_scorer_kernel_time(gmm_scorer* s, double* totalMs, uint32_t* nLaunches, int reset) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    if (s->group) {  // sharded: the parts run concurrently -- the slowest part's total, its launch count
        double   worst = 0;
        uint32_t n     = 0;
        for (gmm_scorer* part : partsOf(s)) {
            double   t = 0;
            uint32_t k = 0;
            const int rc = gmm_scorer_kernel_time(part, &t, &k, reset);
            if (rc != GMM_OK)
                return rc;
            if (t > worst || n == 0)
                worst = t, n = k;
        }
        if (totalMs)
            *totalMs = worst;
        if (nLaunches)
            *nLaunches = n;
        return GMM_OK;
    }
    GMM_HIP_CHECK(hipSetDevice(s->device));
    double total = 0;
    for (size_t i = 0; i < s->eventsUsed; ++i) {
        GMM_HIP_CHECK(hipEventSynchronize(s->events[i].second.get()));
        float ms = 0;
        GMM_HIP_CHECK(hipEventElapsedTime(&ms, s->events[i].first.get(), s->events[i].second.get()));
        total += ms;
    }
    uint32_t launches = static_cast<uint32_t>(s->eventsUsed);
    if (s->scoresOnly) {  // calls without best densities ran on the twin
        double   t = 0;
        uint32_t k = 0;
        int      rc;
        if ((rc = gmm_scorer_kernel_time(s->scoresOnly.get(), &t, &k, reset)) != GMM_OK)
            return rc;
        total += t;
        launches += k;
    }
    if (totalMs)
        *totalMs = total;
    if (nLaunches)
        *nLaunches = launches;
    if (reset)
        s->eventsUsed = 0;
    return GMM_OK;
}

int gmm_scorer_density_clustering(const gmm_scorer* s, uint32_t* nClusters, uint32_t* paddedDimension,
                                  uint8_t* clusterOfEntry, void* clusterMeans) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    if (!s->presel)
        return fail(GMM_ERR_UNSUPPORTED, "scorer type has no density preselection");
    const DensityClustering& dc = s->presel->clustering;
    if (nClusters)
        *nClusters = dc.nClusters;
    if (paddedDimension)
        *paddedDimension = dc.paddedDimension;
    if (clusterOfEntry)
        std::copy(dc.clusterOfEntry.begin(), dc.clusterOfEntry.end(), clusterOfEntry);
    if (clusterMeans) {
        if (dc.quantized)
            std::copy(dc.meansQ.begin(), dc.meansQ.end(), static_cast<uint8_t*>(clusterMeans));
        else
            std::copy(dc.meansF.begin(), dc.meansF.end(), static_cast<float*>(clusterMeans));
    }
    return GMM_OK;
}

int gmm_scorer_clustering_source(const gmm_scorer* s, int* source) {
    if (!s || !source)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    if (!s->presel)
        return fail(GMM_ERR_UNSUPPORTED, "scorer type has no density preselection");
    *source = s->presel->source;
    return GMM_OK;
}

int gmm_cache_archive_read_item(const char* path, const char* name, void* data, uint64_t capacity, uint64_t* size) {
    if (!path || !name || !size)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<char> item;
    if (!readArchiveItem(path, name, item))
        return fail(GMM_ERR_INVALID_ARGUMENT, std::string("no item ") + name + " in cache archive " + path);
    *size = item.size();
    if (data)
        std::memcpy(data, item.data(), std::min<uint64_t>(capacity, item.size()));
    return GMM_OK;
}

int gmm_cache_archive_write_item(const char* path, const char* name, const void* data, uint64_t size) {
    if (!path || !name || !name[0] || (size && !data))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument or empty item name");
    const char* p = static_cast<const char*>(data);
    if (!writeArchiveItem(path, name, std::vector<char>(p, p + size)))
        return fail(GMM_ERR_INVALID_ARGUMENT, std::string("cannot write cache archive ") + path);
    return GMM_OK;
}

int gmm_scorer_cluster_selection(gmm_scorer* s, uint32_t nFrames, uint8_t* selection) {
    if (!s || !selection)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    if (!s->presel)
        return fail(GMM_ERR_UNSUPPORTED, "scorer type has no density preselection");
    if (nFrames > s->presel->lastFrames)
        return fail(GMM_ERR_INVALID_ARGUMENT, "n_frames exceeds the frames of the last score call");
    GMM_HIP_CHECK(hipSetDevice(s->device));
    GMM_HIP_CHECK(hipDeviceSynchronize());
    const uint32_t        nC     = s->presel->clustering.nClusters;
    const uint32_t        blocks = (nFrames + 63) / 64;
    std::vector<uint32_t> words(static_cast<size_t>(blocks) * nC * 16);
    if (!words.empty())
        GMM_HIP_CHECK(hipMemcpy(words.data(), s->presel->dSelT.get(), words.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t t = 0; t < nFrames; ++t)
        for (uint32_t c = 0; c < nC; ++c) {
            const uint32_t w = words[(static_cast<size_t>(t / 64) * nC + c) * 16 + t % 16];
            selection[static_cast<size_t>(t) * nC + c] = ((w >> (8 * ((t % 64) / 16))) & 0xffu) == 0 ? 1 : 0;
        }
    return GMM_OK;
}

int gmm_density_clustering_seeds(uint32_t nEntries, uint32_t nClusters, uint32_t* seeds) {
    if (!seeds || nClusters == 0 || nClusters > nEntries)
        return fail(GMM_ERR_INVALID_ARGUMENT, "need 0 < n_clusters <= n_entries and an output array");
    const std::vector<uint32_t> v = clusteringSeeds(nEntries, nClusters);
    std::copy(v.begin(), v.end(), seeds);
    return GMM_OK;
}

int gmm_shard_pack_keys(const float* scores, const uint32_t* best, const uint32_t* bestOffset, uint32_t rows,
                        uint32_t nFrames, uint32_t stride, int64_t* keys, void* stream) {
    if (rows == 0 || nFrames == 0)
        return GMM_OK;
    if (!scores || !keys || stride < nFrames)
        return fail(GMM_ERR_INVALID_ARGUMENT, "invalid scores/keys/stride");
    GMM_HIP_CHECK(launchPackShardKeys(scores, best, bestOffset, rows, nFrames, stride, keys, static_cast<hipStream_t>(stream)));
    return GMM_OK;
}

int gmm_shard_unpack_keys(const int64_t* keys, uint32_t rows, uint32_t nFrames, float* scores, uint32_t* best,
                          uint32_t stride, void* stream) {
    if (rows == 0 || nFrames == 0)
        return GMM_OK;
    if (!scores || !keys || stride < nFrames)
        return fail(GMM_ERR_INVALID_ARGUMENT, "invalid scores/keys/stride");
    GMM_HIP_CHECK(launchUnpackShardKeys(keys, rows, nFrames, scores, best, stride, static_cast<hipStream_t>(stream)));
    return GMM_OK;
}

const char* gmm_last_error(void) {
    return gLastError.c_str();
}

const char* gmm_version(void) {
    return "rasr_amd-gmm 0.2 (gfx950)";
}

const char* gmm_kernel_id(void) {
    return GMM_KERNEL_ID;
}

}  // extern "C"
