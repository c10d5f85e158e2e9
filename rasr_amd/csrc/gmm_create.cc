// gmm_create.cc -- gmm_scorer_create: one handle = one prepared model resident on one GPU (tiles, row constants,
// scaled inverse deviations) plus frame staging buffers sized for config.max_frames.  Every kernel family builds
// its model from its Prepared* struct (gmm_prepare.hh); a new family adds a model struct (gmm_scorer.hh), a build
// function here, prepareFrames / launch in gmm_score.cc and its arm of kernelPlanOf.
#include <algorithm>
#include <cstdio>

#include "gmm_scorer.hh"

using namespace rasr_gmm;

namespace rasr_gmm {

Flavor flavorOf(gmm_scorer_type t, bool* ok) {
    *ok = true;
    switch (t) {
        case GMM_SIMD_DIAGONAL_MAXIMUM: return Flavor::Simd;
        case GMM_BATCH_DIAGONAL_MAXIMUM_INT:
        case GMM_BATCH_DIAGONAL_MAXIMUM_FAST:
        case GMM_BATCH_PRESELECTION_INT: return Flavor::BatchInt;
        case GMM_DIAGONAL_MAXIMUM: return Flavor::DiagonalMaximum;
        case GMM_BATCH_DIAGONAL_MAXIMUM_FLOAT:
        case GMM_BATCH_PRESELECTION_FLOAT: return Flavor::BatchFloat;
        case GMM_DIAGONAL_SUM: return Flavor::DiagonalSum;
    }
    *ok = false;
    return Flavor::Simd;
}

}  // namespace rasr_gmm

namespace {

// The quantized scorer with several covariances (and the native f32 kernel) prepares the frames once per
// covariance, as the reference's Context does (SimdFeatureScorer.cc:22-35): a C x frames table.  A table past three
// quarters of the device's free memory is refused with its size (an untied 800k model at 32768 frames would need
// terabytes); the float types on the covariance-free split layout need no such table.
int checkCovarianceTable(size_t bytes, uint32_t C, uint32_t maxFrames) {
    if (C <= 1)
        return GMM_OK;
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess)
        freeB = 0;
    if (bytes <= freeB / 4 * 3)
        return GMM_OK;
    char msg[320];
    std::snprintf(msg, sizeof(msg),
                  "%u covariances x %u frames need %.1f GiB of per-covariance frame operands (%.1f GiB free): lower "
                  "max_frames / buffer-size, or use a float scorer type (covariance-free layout, no such table)",
                  C, maxFrames, static_cast<double>(bytes) / (1u << 30), static_cast<double>(freeB) / (1u << 30));
    return fail(GMM_ERR_UNSUPPORTED, msg);
}

// preselection: the clustering over all entries' prepared means, the tiles' row cluster offsets and the
// per-call mask table.  rowEntry / fill: the scorer tiling (16 rows) and, for the split layout, the
// entry a padding row repeats (a padding row must be deselected with the row it copies).
int setupPreselection(gmm_scorer* s, const gmm_mixture_set& ms, const void* entryMeans, uint32_t Dp,
                      const std::vector<uint32_t>& rowEntry, const std::vector<uint32_t>* fill) {
    const bool     quantized = isQuantized(s->flavor);
    const uint32_t nEntries  = ms.mixture_offsets[ms.n_mixtures];
    s->presel                = std::make_unique<Preselection>();
    Preselection& ps         = *s->presel;
    // DensityClustering::build (DensityClustering.tcc:122-155): the cached clustering if the archive holds a matching
    // one, else build it and cache it
    const std::string& archive = s->cacheArchive;
    std::vector<char> item;
    const uint32_t    nClusters = std::min(s->cfg.clusters, nEntries);  // "reducing number of clusters", cc:51-54
    const bool        cached    = !archive.empty() && nEntries > 0 && s->cfg.select_clusters >= 1 &&
                         s->cfg.select_clusters <= nClusters && readArchiveItem(archive, "density-clustering", item) &&
                         decodeClusteringItem(item, quantized, Dp, nClusters, nEntries, s->cfg.select_clusters,
                                              ps.clustering);
    if (!cached) {
        std::string err = buildDensityClustering(quantized, entryMeans, nEntries, Dp, s->cfg.clusters,
                                                 s->cfg.select_clusters, s->cfg.clustering_iterations, ps.clustering);
        if (!err.empty())
            return fail(GMM_ERR_INVALID_ARGUMENT, err);
        // a write failure leaves the scorer as it is (the reference logs it and goes on)
        if (!archive.empty() && !(s->cfg.flags & GMM_FLAG_CACHE_ARCHIVE_READ_ONLY) &&
            writeArchiveItem(archive, "density-clustering", encodeClusteringItem(ps.clustering, nEntries)))
            ps.source = GMM_CLUSTERING_WRITTEN;
    }
    else
        ps.source = GMM_CLUSTERING_CACHED;
    const DensityClustering& dc = ps.clustering;
    const uint32_t           T  = static_cast<uint32_t>(rowEntry.size() / kTileRows);
    // per tile row: the byte offset of its cluster in a wave's mask table -- the float kernel's word table
    // (u16, 64 B per cluster), the quantized kernel's byte table (u32, 16 B per cluster, whose entry nClusters is
    // "never selected": the padding rows' cluster, so a frame that selected none of a mixture's rows keeps all
    // ones; one u32 per row so a lane group's 4 rows are one aligned 16-byte word)
    const auto clusterOf = [&](uint32_t t, uint32_t r) -> uint32_t {
        uint32_t e = rowEntry[static_cast<size_t>(t) * kTileRows + r];
        if (e == UINT32_MAX && fill)
            e = (*fill)[t];
        return e == UINT32_MAX ? (quantized ? dc.nClusters : 0u) : dc.clusterOfEntry[e];
    };
    int rc;
    if (quantized) {
        // the slot kernel's LDS entries are u16 (the LUT byte offset), the key-layout kernel's u8
        const uint32_t        per = 16u * (s->quantized()->scoreOnly == kScoreOnlySlots ? 2u : kI8PreselEntryBytes);
        std::vector<uint32_t> clu(static_cast<size_t>(T + kTilePad) * kTileRows, dc.nClusters * per);
        for (uint32_t t = 0; t < T; ++t)
            for (uint32_t r = 0; r < kTileRows; ++r)
                clu[static_cast<size_t>(t) * kTileRows + r] = clusterOf(t, r) * per;
        rc = upload(ps.dTileClu, clu);
    }
    else {
        std::vector<uint16_t> clu(static_cast<size_t>(T + kTilePad) * kTileRows, 0);
        for (uint32_t t = 0; t < T; ++t)
            for (uint32_t r = 0; r < kTileRows; ++r)
                clu[static_cast<size_t>(t) * kTileRows + r] = static_cast<uint16_t>(clusterOf(t, r) * 64u);
        rc = upload(ps.dTileClu, clu);
    }
    if (rc != GMM_OK || (rc = quantized ? upload(ps.dClusterMeans, dc.meansQ) : upload(ps.dClusterMeans, dc.meansF)) != GMM_OK)
        return rc;
    GMM_HIP_CHECK(ps.dSelT.allocFilled(static_cast<size_t>(s->nFramesPad / 64) * dc.nClusters * 16, 0xff));
    if (quantized && kI8PreselNF == 8)
        GMM_HIP_CHECK(ps.dSelC.allocZeroed(static_cast<size_t>(s->nFramesPad / 128) * dc.nClusters * 16));
    return GMM_OK;
}

// gmm_best_density_pairs' entry-major tables (the assigning types): SIMD-diagonal-maximum the reference's prepared
// u8 means and constant weights of the shard's entries (q: the scorer's own preparation, dIsv its isv * s rows);
// diagonal-maximum / diagonal-sum the direct scorer's reference-order rows (prepareDirect).  A model the direct
// layout does not take (D > 128) has no sparse path: gmm_best_density_pairs reports it, the caller refills.
int setupPairs(gmm_scorer* s, const gmm_mixture_set& ms, ShardRange shard, const PreparedQuantized* q) {
    if (shard.begin == 0 && shard.end == 0)
        shard.end = ms.n_mixtures;
    const uint32_t eb = ms.mixture_offsets[shard.begin], ee = ms.mixture_offsets[shard.end];
    std::vector<uint32_t> mixOff(shard.end - shard.begin + 1), cov(ee - eb);
    for (uint32_t m = shard.begin; m <= shard.end; ++m)
        mixOff[m - shard.begin] = ms.mixture_offsets[m] - eb;
    for (uint32_t e = eb; e < ee; ++e)
        cov[e - eb] = ms.density_covariance[ms.mixture_densities[e]];
    auto t = std::make_unique<PairTables>();
    int  rc = GMM_OK;
    if (s->flavor == Flavor::Simd) {
        if (!q)
            return GMM_OK;
        const size_t         Dp = q->paddedDimension;
        std::vector<uint8_t> mean(q->preparedMean.begin() + eb * Dp, q->preparedMean.begin() + ee * Dp);
        std::vector<int32_t> cst(q->constantWeight.begin() + eb, q->constantWeight.begin() + ee);
        if ((rc = upload(t->dQMean, mean)) || (rc = upload(t->dQConst, cst)))
            return rc;
        t->isvStride = q->kSteps * kI8K;  // dIsv: [C][kSteps * 64]
        t->kind      = kPairSimd;
    }
    else if (s->flavor == Flavor::DiagonalMaximum || s->flavor == Flavor::DiagonalSum) {
        PreparedDirect p;
        const uint32_t nb = directBlocks(ms.dimension, false);
        if (nb == 0 || !prepareDirect(ms, Flavor::DiagonalMaximum, s->cfg.mixture_weight_scale, s->cfg.gaussian_scale,
                                      shard, nb, p).empty())
            return GMM_OK;
        if ((rc = upload(t->dFMean, p.mean)) || (rc = upload(t->dFConst, p.constant)) ||
            (rc = upload(t->dLogNorm, p.logNorm)) || (rc = upload(t->dIsv, p.isv)))
            return rc;
        t->L    = p.L;
        t->nb   = p.nb;
        t->kind = s->flavor == Flavor::DiagonalSum ? kPairDiagonalSum : kPairDiagonalMaximum;
    }
    else
        return GMM_OK;
    if ((rc = upload(t->dMixOff, mixOff)) || (rc = upload(t->dCov, cov)))
        return rc;
    t->nEntries = ee - eb;
    for (size_t m = 0; m + 1 < mixOff.size(); ++m)
        t->maxEntries = std::max(t->maxEntries, mixOff[m + 1] - mixOff[m]);
    s->pairs = std::move(t);
    return GMM_OK;
}

// what every family does once its model's scalars are in place: the kernel choice, and with it the frame tables' rows
void planModel(gmm_scorer* s, uint32_t nMix, uint32_t nTiles, const std::vector<uint32_t>& mixTileOff) {
    s->nMix       = nMix;
    s->nTiles     = nTiles;
    s->mixTileOff = mixTileOff;
    s->plan       = kernelPlanOf(*s);
    s->nFramesPad = paddedFrames(s->plan, s->cfg.max_frames);
}

// classLayout: lay the model out for the score-only kernel (gmm_prepare.cc buildSlotLayout) whatever the type (the
// SIMD scorer's scoresOnly twin); batch-int/-fast use it by default
int buildQuantized(gmm_scorer* s, const gmm_mixture_set& ms, ShardRange shard, bool classLayout) {
    const bool        presel = isPreselection(s->type);
    PreparedQuantized p;
    // batch types have no best densities: the score-only slot layout where it applies
    // (preselection-batch-int included: the kernel masks the slot layout's candidates)
    const bool  scoreOnlyLayout = classLayout || (s->flavor == Flavor::BatchInt && !(s->cfg.flags & GMM_FLAG_FULL_KEYS));
    std::string err = prepareQuantized(ms, s->flavor, shard, p, scoreOnlyLayout ? kScoreOnlySlots : kScoreOnlyNone);
    if (!err.empty())
        return fail(GMM_ERR_INVALID_ARGUMENT, err);
    QuantizedModel& m = s->model.emplace<QuantizedModel>();
    m.scoreOnly       = p.scoreOnly;
    m.kSteps          = p.kSteps;
    m.idxBits         = p.idxBits;
    m.paddedDimension = p.paddedDimension;
    m.scaling         = p.scaling;
    m.scalingSquared  = p.scalingSquared;
    m.invQ            = p.inverseQuantizationFactor;
    m.batchScale      = p.batchScale;
    m.isvScaled       = p.isvScaled;
    planModel(s, p.nMixtures, p.tiling.nTiles, p.tiling.mixTileOffset);
    int rc;
    if (p.scoreOnly && (rc = upload(m.dMixOddMask, p.mixOddMask)) != GMM_OK)
        return rc;
    // preselection-batch-int compares keys biased by 2^31 as unsigned (gmm_kernels_i8.hip, PRESEL)
    if (presel)
        for (int32_t& v : p.tileP)
            v = static_cast<int32_t>(static_cast<uint32_t>(v) ^ 0x80000000u);
    // kTilePad zero tiles at the end: the kernels prefetch two tiles ahead without bound checks
    if ((rc = upload(m.dTileA, p.tileA, kTilePad * kLanes * 16 * p.kSteps)) ||
        (rc = upload(m.dTileP, p.tileP, kTilePad * kTileRows)) ||
        (rc = upload(m.dTileCov, p.tiling.tileCovariance, kTilePad)) || (rc = upload(s->dMixTileOff, s->mixTileOff)) ||
        (rc = upload(s->dIsv, p.isvDevice)))
        return rc;
    const size_t nQ = static_cast<size_t>(s->C) * s->nFramesPad;
    if ((rc = checkCovarianceTable(nQ * (m.kSteps * kI8K + sizeof(int32_t)), s->C, s->cfg.max_frames)) != GMM_OK)
        return rc;
    GMM_HIP_CHECK(m.dFrameQ.allocZeroed(nQ * m.kSteps * kI8K));
    GMM_HIP_CHECK(m.dFrameSS.allocZeroed(nQ));
    // BatchPreselectionIntFeatureScorer::init: clustering_->build(means_) over the u8 means
    if (presel && (rc = setupPreselection(s, ms, p.preparedMean.data(), p.paddedDimension, p.tiling.rowEntry, nullptr)) != GMM_OK)
        return rc;
    return classLayout ? GMM_OK : setupPairs(s, ms, shard, &p);
}

int buildDirect(gmm_scorer* s, const gmm_mixture_set& ms, ShardRange shard) {
    PreparedDirect p;
    std::string    err = prepareDirect(ms, s->flavor, s->cfg.mixture_weight_scale, s->cfg.gaussian_scale, shard,
                                       directBlocks(ms.dimension, s->flavor == Flavor::BatchFloat), p);
    if (!err.empty())
        return fail(GMM_ERR_INVALID_ARGUMENT, err);
    DirectModel& m = s->model.emplace<DirectModel>();
    m.L            = p.L;
    planModel(s, p.nMixtures, p.nEntries, p.mixOff);  // chunks are cut by entries (chunkTableFor)
    int rc;
    if ((rc = upload(m.dMean, p.mean)) || (rc = upload(s->dIsv, p.isv)) || (rc = upload(m.dCov, p.entryCov)) ||
        (rc = upload(m.dConst, p.constant)) || (rc = upload(m.dLogNorm, p.logNorm)) ||
        (rc = upload(s->dMixTileOff, s->mixTileOff)))
        return rc;
    return setupPairs(s, ms, shard, nullptr);
}

int buildSplit(gmm_scorer* s, const gmm_mixture_set& ms, ShardRange shard, const PreparedFloat& p) {
    const bool  presel = isPreselection(s->type);
    SplitModel& m      = s->model.emplace<SplitModel>();
    m.splitCov         = p.splitCov;
    m.kSteps16         = p.kSteps16;
    m.splitRows        = p.splitRows;
    m.keyBits          = p.splitKeyBits;
    m.offsetK0         = p.offsetK0;
    planModel(s, p.nMixtures, p.tiling.nTiles, p.tiling.mixTileOffset);
    const std::vector<int32_t> limbs(p.limbExp, p.limbExp + kSplitLimbs);
    const size_t nH = static_cast<size_t>(s->nFramesPad) * p.kSteps16 * (p.splitRows == 32 ? 16 : 32);
    int          rc;
    if ((rc = upload(m.dTileH, p.tileH, kTilePad * kLanes * 8 * p.kSteps16)) || (rc = upload(m.dDimScale, p.dimScale)) ||
        (rc = upload(m.dLimbExp, limbs)) || (rc = upload(s->dMixTileOff, s->mixTileOff)) ||
        (rc = upload(s->dIsv, p.isvDevice)) || (rc = upload(m.dCentre, p.centre)))
        return rc;
    GMM_HIP_CHECK(m.dFrameH.allocZeroed(nH * sizeof(uint16_t)));
    GMM_HIP_CHECK(m.dFrameXX.allocZeroed(s->nFramesPad));
    GMM_HIP_CHECK(m.dFrameExp.allocZeroed(s->nFramesPad));
    if (presel) {
        // BatchPreselectionFloatFeatureScorer::init: clustering over means_ = mean * isv (f32),
        // 0-padded to the batch-float padded dimension (BlockSize 8, BatchFeatureScorer.cc:145-170)
        const uint32_t     D = ms.dimension, Dp = (D + 7u) / 8u * 8u;
        const uint32_t     nEntries = ms.mixture_offsets[ms.n_mixtures];
        std::vector<float> em(static_cast<size_t>(nEntries) * Dp, 0.0f);
        for (uint32_t e = 0; e < nEntries; ++e) {
            const float* mean = ms.means + static_cast<size_t>(ms.density_mean[ms.mixture_densities[e]]) * D;
            for (uint32_t k = 0; k < D; ++k)
                em[static_cast<size_t>(e) * Dp + k] = mean[k] * p.isv[k];
        }
        if ((rc = setupPreselection(s, ms, em.data(), Dp, p.tiling.rowEntry, &p.splitFillEntry)) != GMM_OK)
            return rc;
    }
    return setupPairs(s, ms, shard, nullptr);
}

int buildF32(gmm_scorer* s, const gmm_mixture_set& ms, ShardRange shard, const PreparedFloat& p) {
    F32Model& m = s->model.emplace<F32Model>();
    m.kSteps    = p.kSteps;
    m.foldNorm  = p.foldNorm;
    m.tileBits  = p.tileBits;
    m.offsetK0  = p.offsetK0;
    planModel(s, p.nMixtures, p.tiling.nTiles, p.tiling.mixTileOffset);
    int rc;
    if ((rc = upload(m.dTileA, p.tileA, kTilePad * kLanes * p.kSteps)) ||
        (rc = upload(m.dTileCov, p.tiling.tileCovariance, kTilePad)) ||
        (rc = upload(m.dRowDns, p.tiling.rowDensityInMixture, kTilePad * kTileRows)) ||
        (rc = upload(s->dMixTileOff, s->mixTileOff)) || (rc = upload(s->dIsv, p.isvDevice)) ||
        (rc = upload(m.dCentre, p.centre)))
        return rc;
    const size_t nX = static_cast<size_t>(s->C) * s->nFramesPad;
    if ((rc = checkCovarianceTable(nX * (m.kSteps * 4 + 1) * sizeof(float), s->C, s->cfg.max_frames)) != GMM_OK)
        return rc;
    GMM_HIP_CHECK(m.dFrameX.allocZeroed(nX * m.kSteps * 4));
    GMM_HIP_CHECK(m.dFrameXX.allocZeroed(nX));
    return setupPairs(s, ms, shard, nullptr);
}

// the float layout of a type and config (host only): what buildFloat uploads and gmm_float_spread_bound measures
std::string prepareFloatFor(const gmm_mixture_set& ms, gmm_scorer_type type, Flavor flavor, const gmm_scorer_config& cfg,
                            ShardRange shard, PreparedFloat& p) {
    const uint32_t flags = cfg.flags;
    return prepareFloat(ms, flavor, cfg.mixture_weight_scale, cfg.gaussian_scale, shard, p,
                        (flags & GMM_FLAG_NATIVE_F32) == 0,
                        (isPreselection(type) || (flags & GMM_FLAG_SPLIT_TILE16)) ? 16u
                                                                                  : ((flags & GMM_FLAG_SPLIT_TILE32) ? 32u : 0u));
}

int buildFloat(gmm_scorer* s, const gmm_mixture_set& ms, ShardRange shard) {
    const bool    presel = isPreselection(s->type);
    PreparedFloat p;
    std::string   err = prepareFloatFor(ms, s->type, s->flavor, s->cfg, shard, p);
    if (!err.empty())
        return fail(GMM_ERR_INVALID_ARGUMENT, err);
    if (presel && (!p.split || p.splitRows != 16))
        return fail(GMM_ERR_UNSUPPORTED, "preselection-batch-float needs the 16-row split-f16 layout (one "
                                         "covariance, dimension <= 83, <= 1024 densities per mixture)");
    // the contract's condition (gmm_prepare.hh kSpreadKappa): a model predicted above it leaves the expanded form
    s->spreadStat      = p.spreadStat;
    s->spreadPredicted = p.spreadPredicted;
    if (!(p.spreadPredicted <= kFloatContract) && !(s->cfg.flags & GMM_FLAG_ACCEPT_SPREAD_BOUND)) {
        if (s->type == GMM_DIAGONAL_MAXIMUM || s->type == GMM_BATCH_DIAGONAL_MAXIMUM_FLOAT)
            return buildDirect(s, ms, shard);  // exact, at the vector ALUs' rate (dimension <= 126 <= 128)
        char msg[400];
        std::snprintf(msg, sizeof(msg),
                      "predicted relative error %.3g of the float kernels on this model (spread statistic %.3g x kappa "
                      "%.3g) exceeds the %.0e contract, and %s has no reference-order path: set "
                      "GMM_FLAG_ACCEPT_SPREAD_BOUND to accept the predicted bound in place of the contract",
                      p.spreadPredicted, p.spreadStat, kSpreadKappa, kFloatContract,
                      presel ? "preselection-batch-float" : "diagonal-sum");
        return fail(GMM_ERR_UNSUPPORTED, msg);
    }
    return p.split ? buildSplit(s, ms, shard, p) : buildF32(s, ms, shard, p);
}

int createScorer(const gmm_mixture_set* ms, gmm_scorer_type type, const gmm_scorer_config* config, int device,
                 bool classLayout, gmm_scorer** out) {
    if (!ms || !out)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    bool   ok     = false;
    Flavor flavor = flavorOf(type, &ok);
    if (!ok)
        return fail(GMM_ERR_UNSUPPORTED, "unknown feature scorer type");
    gmm_scorer_config cfg;
    gmm_default_config(&cfg);
    if (config)
        cfg = *config;
    if (cfg.max_frames == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "max_frames must be > 0");
    // BatchUnrolledIntFeatureScorer (BatchFeatureScorer.cc:550-604): padded dimension > 48 is refused by the
    // reference itself (cc:552-555); below 48 its unrolled loop still loads 3 x 16 bytes per row and steps the
    // means by 48 bytes (cc:591) across rows laid out at the padded dimension (cc:367-375), reading other rows
    // and past its allocation -- undefined, so refused here; at exactly 48 it is batch-int's arithmetic.
    if (type == GMM_BATCH_DIAGONAL_MAXIMUM_FAST && (ms->dimension + 15) / 16 * 16 > 48)
        return fail(GMM_ERR_UNSUPPORTED, "This feature scorer supports only features with max. 48 components");
    if (type == GMM_BATCH_DIAGONAL_MAXIMUM_FAST && (ms->dimension + 15) / 16 * 16 < 48)
        return fail(GMM_ERR_UNSUPPORTED, "batch-diagonal-maximum-fast needs 33..48 components (padded dimension 48): "
                                         "the reference's fixed 48-byte loads are undefined for smaller dimensions; "
                                         "use batch-diagonal-maximum-int");
    const bool presel = isPreselection(type);
    const bool direct = (cfg.flags & GMM_FLAG_REFERENCE_ORDER) != 0;
    if (direct && type != GMM_DIAGONAL_MAXIMUM && type != GMM_BATCH_DIAGONAL_MAXIMUM_FLOAT)
        return fail(GMM_ERR_UNSUPPORTED, "the reference-order flag applies to diagonal-maximum and "
                                         "batch-diagonal-maximum-float only");
    if (presel && (cfg.clusters == 0 || cfg.clusters > 256))
        return fail(GMM_ERR_INVALID_ARGUMENT, "clusters must be in [1, 256]");
    if (presel && (cfg.flags & (GMM_FLAG_NATIVE_F32 | GMM_FLAG_SPLIT_TILE32)))
        return fail(GMM_ERR_UNSUPPORTED, "preselection runs on the 16-row split-f16 / quantized kernels only");
    const ShardRange shard{cfg.mixture_begin, cfg.mixture_end};

    auto s               = std::make_unique<gmm_scorer>();
    s->type              = type;
    s->flavor            = flavor;
    s->device            = device;
    s->cfg               = cfg;
    s->cacheArchive      = cfg.cache_archive ? cfg.cache_archive : "";
    s->cfg.cache_archive = nullptr;
    s->D                 = ms->dimension;
    s->C                 = ms->n_covariances;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(GMM_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev)
        return fail(GMM_ERR_INVALID_ARGUMENT, "device index out of range");
    GMM_HIP_CHECK(hipSetDevice(device));

    const int rc = isQuantized(flavor) ? buildQuantized(s.get(), *ms, shard, classLayout)
                   : direct            ? buildDirect(s.get(), *ms, shard)
                                       : buildFloat(s.get(), *ms, shard);
    if (rc != GMM_OK)
        return rc;
    s->mixBase = shard.begin == 0 && shard.end == 0 ? 0 : shard.begin;
    s->nMixSet = ms->n_mixtures;
    GMM_HIP_CHECK(hipDeviceSynchronize());
    *out = s.release();
    return GMM_OK;
}

}  // namespace

extern "C" {

int gmm_scorer_create(const gmm_mixture_set* ms, gmm_scorer_type type, const gmm_scorer_config* config,
                      int device, gmm_scorer** out) {
    int rc = createScorer(ms, type, config, device, false, out);
    if (rc != GMM_OK || type != GMM_SIMD_DIAGONAL_MAXIMUM || ((*out)->cfg.flags & GMM_FLAG_FULL_KEYS))
        return rc;
    gmm_scorer* s = *out;
    if (s->multiCov() || s->quantized()->kSteps != 1)
        return GMM_OK;  // the class layout covers one covariance and D <= 64 (the key layout serves the rest)
    if (s->cfg.flags & GMM_FLAG_NO_SCORE_ONLY_TWIN)
        return GMM_OK;  // callers that always ask for best densities (aligners): no second copy of the model
    // best effort: the twin only speeds up calls without best densities, so a twin that cannot be built (e.g. the
    // device has no room for a second copy of the model) leaves a valid scorer on the key layout
    gmm_scorer* twin = nullptr;
    if (createScorer(ms, type, &s->cfg, device, true, &twin) != GMM_OK) {
        (void)hipGetLastError();
        (void)hipSetDevice(device);
        setLastError("");
        return GMM_OK;
    }
    if (twin->quantized()->scoreOnly)
        s->scoresOnly.reset(twin);
    else  // some row's |2 dot + Q| may leave the class layout's range
        gmm_scorer_destroy(twin);
    return GMM_OK;
}

int gmm_float_spread_bound(const gmm_mixture_set* ms, gmm_scorer_type type, const gmm_scorer_config* config,
                           double* statistic, double* predicted) {
    if (!ms)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null mixture set");
    bool         ok     = false;
    const Flavor flavor = flavorOf(type, &ok);
    if (!ok || isQuantized(flavor))
        return fail(GMM_ERR_UNSUPPORTED, "the spread bound applies to the float scorer types");
    gmm_scorer_config cfg;
    gmm_default_config(&cfg);
    if (config)
        cfg = *config;
    PreparedFloat     p;
    const std::string err = prepareFloatFor(*ms, type, flavor, cfg, ShardRange{cfg.mixture_begin, cfg.mixture_end}, p);
    if (!err.empty())
        return fail(GMM_ERR_INVALID_ARGUMENT, err);
    if (statistic)
        *statistic = p.spreadStat;
    if (predicted)
        *predicted = p.spreadPredicted;
    return GMM_OK;
}

int gmm_scorer_spread_bound(const gmm_scorer* s, double* statistic, double* predicted) {
    if (!s)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null scorer");
    if (isQuantized(s->flavor))
        return fail(GMM_ERR_UNSUPPORTED, "the spread bound applies to the float scorer types");
    if (statistic)
        *statistic = s->spreadStat;
    if (predicted)
        *predicted = s->spreadPredicted;
    return GMM_OK;
}

int gmm_scorer_destroy(gmm_scorer* s) {
    if (!s)
        return GMM_OK;
    (void)hipSetDevice(s->device);
    delete s;
    return GMM_OK;
}

}  // extern "C"
