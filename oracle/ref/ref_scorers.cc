// ref_scorers.cc -- TEST INFRASTRUCTURE ONLY.
//
// Stand-alone driver of the REFERENCE's own feature scorers.  The reference sources are compiled in
// place (oracle/ref/Makefile); this file only builds an Mm::MixtureSet in memory from a request file,
// instantiates the reference's scorer classes directly, and writes what they compute to a reply file.
// oracle/reference.py is the only caller.  Nothing here restates any arithmetic of the reference: every
// number in a reply was produced by reference code (a few are read out of non-public members, which is
// what the two access macros below are for; GCC lays members out independently of their access).
//
//   ref_scorers [--*.param=value ...] score REQUEST REPLY
//   ref_scorers [--*.param=value ...] pms   FILE.pms[.gz] REPLY OFFSET REDUCED_DIMENSION
//
// Scorer parameters travel as configuration resources on the command line (scorer.buffer-size,
// scorer.mixture-weight-scale, scorer.gaussian-scale, scorer.density-clustering.clusters, ...), the way
// the reference's own tools receive them.
//
// Request (little-endian): "RSRQ", u32 version 1, u32 kind, u32 D, nMeans, nCovariances, nDensities,
// nMixtures, nEntries, nFrames; then the orc_mixture_set tables (oracle/gmm_oracle.h) in declaration
// order: f32 means, f32 variances, u32 density_mean, u32 density_covariance, u32 mixture_offsets
// [nMixtures+1], u32 mixture_densities, f64 mixture_log_weights; then f32 frames [nFrames][D].
// Reply: "RSRP", then records {u32 name length, name, u32 type (0 f32, 1 u32, 2 s32, 3 u8, 4 f64),
// u32 rank, u32 dims[rank], data} until the end of the file.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define private public
#define protected public
#include <Core/Application.hh>
#include <Core/CompressedStream.hh>
#include <Mm/BatchFeatureScorer.hh>
#include <Mm/CovarianceFeatureScorerElement.hh>
#include <Mm/DensityClustering.hh>
#include <Mm/GaussDiagonalMaximumFeatureScorer.hh>
#include <Mm/MixtureSet.hh>
#include <Mm/SimdFeatureScorer.hh>
#undef private
#undef protected

namespace {

enum Kind { kSimd = 0, kDiagonalMaximum, kDiagonalSum, kBatchInt, kBatchFloat, kBatchFast, kPreselInt, kPreselFloat };
enum Type { tF32 = 0, tU32, tS32, tU8, tF64 };

struct Reply {
    std::ofstream os;
    explicit Reply(const std::string& path) : os(path.c_str(), std::ios::binary) {
        os.write("RSRP", 4);
    }
    void u32(uint32_t v) {
        os.write(reinterpret_cast<const char*>(&v), 4);
    }
    void put(const std::string& name, Type t, const std::vector<uint32_t>& dims, const void* data) {
        static const size_t width[] = {4, 4, 4, 1, 8};
        u32(name.size());
        os.write(name.data(), name.size());
        u32(t);
        u32(dims.size());
        size_t n = 1;
        for (size_t i = 0; i < dims.size(); ++i) {
            u32(dims[i]);
            n *= dims[i];
        }
        if (n)
            os.write(static_cast<const char*>(data), n * width[t]);
    }
    template<class T> static Type typeOf();
    template<class T>
    void put(const std::string& name, const std::vector<T>& v, std::vector<uint32_t> dims = std::vector<uint32_t>()) {
        if (dims.empty())
            dims.push_back(v.size());
        put(name, typeOf<T>(), dims, v.empty() ? 0 : &v[0]);
    }
    template<class T>
    void scalar(const std::string& name, T v) {
        put(name, typeOf<T>(), std::vector<uint32_t>(), &v);
    }
};
template<> Type Reply::typeOf<float>() { return tF32; }
template<> Type Reply::typeOf<uint32_t>() { return tU32; }
template<> Type Reply::typeOf<int32_t>() { return tS32; }
template<> Type Reply::typeOf<uint8_t>() { return tU8; }
template<> Type Reply::typeOf<double>() { return tF64; }

std::vector<uint32_t> dims(uint32_t a, uint32_t b) {
    std::vector<uint32_t> d;
    d.push_back(a);
    d.push_back(b);
    return d;
}

struct Request {
    uint32_t kind, D, nMeans, nCov, nDns, nMix, nEntries, nFrames;
    std::vector<float>    means, variances, frames;
    std::vector<uint32_t> dnsMean, dnsCov, mixOffsets, mixDensities;
    std::vector<double>   logWeights;

    template<class T>
    static bool get(std::ifstream& is, std::vector<T>& v, size_t n) {
        v.resize(n);
        if (n)
            is.read(reinterpret_cast<char*>(&v[0]), n * sizeof(T));
        return bool(is);
    }
    bool read(const std::string& path) {
        std::ifstream is(path.c_str(), std::ios::binary);
        char          magic[4];
        uint32_t      head[10];
        if (!is.read(magic, 4) || std::memcmp(magic, "RSRQ", 4) != 0)
            return false;
        if (!is.read(reinterpret_cast<char*>(head), sizeof(head)) || head[0] != 1)
            return false;
        kind = head[1], D = head[2], nMeans = head[3], nCov = head[4], nDns = head[5], nMix = head[6];
        nEntries = head[7], nFrames = head[8];
        bool ok = get(is, means, size_t(nMeans) * D) && get(is, variances, size_t(nCov) * D) &&
                  get(is, dnsMean, nDns) && get(is, dnsCov, nDns) && get(is, mixOffsets, nMix + 1) &&
                  get(is, mixDensities, nEntries) && get(is, logWeights, nEntries) &&
                  get(is, frames, size_t(nFrames) * D);
        if (!ok || mixOffsets[0] != 0 || mixOffsets[nMix] != nEntries)
            return false;
        for (uint32_t i = 0; i < nDns; ++i)
            if (dnsMean[i] >= nMeans || dnsCov[i] >= nCov)
                return false;
        for (uint32_t m = 0; m < nMix; ++m)
            if (mixOffsets[m] > mixOffsets[m + 1])
                return false;
        for (uint32_t e = 0; e < nEntries; ++e)
            if (mixDensities[e] >= nDns)
                return false;
        return true;
    }
    Mm::FeatureVector frame(uint32_t t) const {
        return Mm::FeatureVector(frames.begin() + size_t(t) * D, frames.begin() + size_t(t + 1) * D);
    }
};

// The calls of SURVEY.md section 8(c): covariances, means, densities, then mixtures with log weights.
Core::Ref<Mm::MixtureSet> buildMixtureSet(const Request& r) {
    Core::Ref<Mm::MixtureSet> ms(new Mm::MixtureSet(r.D));
    for (uint32_t c = 0; c < r.nCov; ++c)
        ms->addCovariance(new Mm::DiagonalCovariance(
                std::vector<Mm::VarianceType>(r.variances.begin() + size_t(c) * r.D, r.variances.begin() + size_t(c + 1) * r.D)));
    for (uint32_t i = 0; i < r.nMeans; ++i) {
        Mm::Mean* mean = new Mm::Mean();
        mean->assign(r.means.begin() + size_t(i) * r.D, r.means.begin() + size_t(i + 1) * r.D);
        ms->addMean(mean);
    }
    for (uint32_t i = 0; i < r.nDns; ++i)
        ms->addDensity(new Mm::GaussDensity(r.dnsMean[i], r.dnsCov[i]));
    for (uint32_t m = 0; m < r.nMix; ++m) {
        Mm::Mixture* mix = new Mm::Mixture();
        for (uint32_t e = r.mixOffsets[m]; e < r.mixOffsets[m + 1]; ++e)
            mix->addLogDensity(r.mixDensities[e], r.logWeights[e]);
        ms->addMixture(mix);
    }
    return ms;
}

// CovarianceFeatureScorerElement as every scorer's init makes it from a covariance, before any scaling
void putCovarianceElements(Reply& out, const Mm::MixtureSet& ms) {
    std::vector<float> isv, logNorm;
    for (uint32_t c = 0; c < ms.nCovariances(); ++c) {
        Mm::CovarianceFeatureScorerElement e;
        e = *ms.covariance(c);
        isv.insert(isv.end(), e.inverseSquareRootDiagonal().begin(), e.inverseSquareRootDiagonal().end());
        logNorm.push_back(e.logNormalizationFactor());
    }
    out.put("isv", isv, dims(ms.nCovariances(), ms.dimension()));
    out.put("log_norm", logNorm);
}

void scoreSimd(const Core::Configuration& c, const Request& r, Core::Ref<const Mm::MixtureSet> ms, Reply& out) {
    Mm::SimdGaussDiagonalMaximumFeatureScorer fs(c, ms);
    {  // getScaling() reads the unscaled covariance table, as init() calls it: a second instance, table put back
        Mm::SimdGaussDiagonalMaximumFeatureScorer probe(c, ms);
        for (size_t i = 0; i < probe.covarianceTable_.size(); ++i)
            probe.covarianceTable_[i] = *ms->covariance(i);
        out.scalar<float>("simd_scaling", probe.getScaling(*ms));
    }
    out.scalar<float>("simd_scaling_squared", fs.scalingSquared_);
    out.scalar<float>("simd_inverse_quantization_factor", fs.inverseQuantizationFactor_);
    std::vector<float> isv, logNorm;
    for (size_t i = 0; i < fs.covarianceTable_.size(); ++i) {
        const std::vector<Mm::VarianceType>& v = fs.covarianceTable_[i].inverseSquareRootDiagonal();
        isv.insert(isv.end(), v.begin(), v.end());
        logNorm.push_back(fs.covarianceTable_[i].logNormalizationFactor());
    }
    out.put("simd_isv_scaled", isv, dims(r.nCov, r.D));
    out.put("simd_log_norm_scaled", logNorm);
    std::vector<uint8_t>  prepared;
    std::vector<int32_t>  constant;
    std::vector<uint32_t> entryCov;
    uint32_t              padded = 0;
    for (size_t m = 0; m < fs.mixtureTable_.size(); ++m)
        for (size_t d = 0; d < fs.mixtureTable_[m].nDensities(); ++d) {
            const Mm::SimdGaussDiagonalMaximumFeatureScorer::MixtureElement::Density& dns = fs.mixtureTable_[m].density(d);
            padded = dns.preparedMean_.size();
            prepared.insert(prepared.end(), dns.preparedMean_.begin(), dns.preparedMean_.end());
            constant.push_back(dns.constantWeight_);
            entryCov.push_back(dns.covarianceIndex_);
        }
    out.put("simd_prepared_mean", prepared, dims(constant.size(), padded));
    out.put("simd_constant_weight", constant);
    out.put("simd_entry_covariance", entryCov);

    std::vector<float>    scores(size_t(r.nMix) * r.nFrames);
    std::vector<uint32_t> best(scores.size());
    std::vector<int32_t>  raw(scores.size());
    std::vector<uint8_t>  quantized;
    uint32_t              qWidth = 0;
    for (uint32_t t = 0; t < r.nFrames; ++t) {
        Mm::FeatureVector x = r.frame(t);
        std::vector<Mm::SimdGaussDiagonalMaximumFeatureScorer::PreparedFeatureVector> q = fs.multiplyAndQuantize(x);
        for (size_t i = 0; i < q.size(); ++i) {
            qWidth = q[i].size();
            quantized.insert(quantized.end(), q[i].begin(), q[i].end());
        }
        Mm::AssigningFeatureScorer::AssigningScorer s = fs.getAssigningScorer(x);
        for (uint32_t m = 0; m < r.nMix; ++m) {
            scores[size_t(m) * r.nFrames + t] = s->score(m);
            best[size_t(m) * r.nFrames + t]   = s->bestDensity(m);
            raw[size_t(m) * r.nFrames + t]    = fs.quantizedScore(fs.mixtureTable_[m], q).first;
        }
    }
    out.put("scores", scores, dims(r.nMix, r.nFrames));
    out.put("best", best, dims(r.nMix, r.nFrames));
    out.put("raw", raw, dims(r.nMix, r.nFrames));
    std::vector<uint32_t> qd;
    qd.push_back(r.nFrames), qd.push_back(r.nCov), qd.push_back(qWidth);
    out.put("simd_quantized_frames", quantized, qd);
}

template<class Scorer>
void scoreAssigning(const Core::Configuration& c, const Request& r, Core::Ref<const Mm::MixtureSet> ms, Reply& out) {
    Scorer fs(c, ms);
    out.scalar<float>("mixture_weight_scale", fs.mixtureWeightScale_);
    out.scalar<float>("sqrt_gaussian_scale", fs.gaussianScale_);
    std::vector<float>    scores(size_t(r.nMix) * r.nFrames);
    std::vector<uint32_t> best(scores.size());
    for (uint32_t t = 0; t < r.nFrames; ++t) {
        Mm::AssigningFeatureScorer::AssigningScorer s = fs.getAssigningScorer(r.frame(t));
        for (uint32_t m = 0; m < r.nMix; ++m) {
            scores[size_t(m) * r.nFrames + t] = s->score(m);
            best[size_t(m) * r.nFrames + t]   = s->bestDensity(m);
        }
    }
    out.put("scores", scores, dims(r.nMix, r.nFrames));
    out.put("best", best, dims(r.nMix, r.nFrames));
}

// The buffered protocol with a ring of nFrames + 1 slots (scorer.buffer-size): every frame is added, then
// flush() hands out one context per frame, oldest first (BatchFeatureScorer.cc:46-50, 89-96).
template<class Scorer>
void runBatch(Scorer& fs, const Request& r, Reply& out) {
    if (uint32_t(fs.bufferSize_) != r.nFrames + 1) {
        std::cerr << "ref_scorers: scorer.buffer-size must be frames + 1" << std::endl;
        std::exit(3);
    }
    fs.reset();
    for (uint32_t t = 0; t < r.nFrames; ++t)
        fs.addFeature(r.frame(t));
    std::vector<float> scores(size_t(r.nMix) * r.nFrames);
    for (uint32_t t = 0; t < r.nFrames; ++t) {
        Mm::FeatureScorer::Scorer s = fs.flush();
        for (uint32_t m = 0; m < r.nMix; ++m)
            scores[size_t(m) * r.nFrames + t] = s->score(m);
    }
    out.put("scores", scores, dims(r.nMix, r.nFrames));
    out.scalar<uint32_t>("batch_padded_dimension", fs.paddedDimension_);
}

template<class Scorer>
void putIntTables(const Scorer& fs, const Request& r, Reply& out) {
    const uint32_t dp = fs.paddedDimension_;
    out.scalar<float>("batch_scale", fs.scale_);
    out.put("batch_variance", std::vector<float>(fs.variance_, fs.variance_ + dp));
    out.put("batch_means", std::vector<uint8_t>(fs.means_, fs.means_ + size_t(fs.nDensities_) * dp), dims(fs.nDensities_, dp));
    out.put("batch_constants", std::vector<int32_t>(fs.constants_, fs.constants_ + fs.nDensities_));
    out.put("batch_features", std::vector<uint8_t>(fs.features_, fs.features_ + size_t(r.nFrames) * dp), dims(r.nFrames, dp));
}

template<class Scorer>
void putFloatTables(const Scorer& fs, const Request& r, Reply& out) {
    const uint32_t dp = fs.paddedDimension_;
    out.put("batch_variance", std::vector<float>(fs.variance_, fs.variance_ + dp));
    out.put("batch_means", std::vector<float>(fs.means_, fs.means_ + size_t(fs.nDensities_) * dp), dims(fs.nDensities_, dp));
    out.put("batch_constants", std::vector<float>(fs.constants_, fs.constants_ + fs.nDensities_));
    out.put("batch_features", std::vector<float>(fs.features_, fs.features_ + size_t(r.nFrames) * dp), dims(r.nFrames, dp));
}

template<class Scorer, class Mean>
void putClustering(const Scorer& fs, const Request& r, Reply& out) {
    const uint32_t nc = fs.clustering_->nClusters_, dp = fs.paddedDimension_;
    out.scalar<uint32_t>("presel_clusters", nc);
    out.scalar<uint32_t>("presel_selected", fs.clustering_->nSelected_);
    out.scalar<float>("presel_backoff", fs.clustering_->backoffScore_);
    out.put("presel_cluster_of_entry", std::vector<uint8_t>(fs.clustering_->clusterIndexForDensity_.begin(),
                                                             fs.clustering_->clusterIndexForDensity_.end()));
    out.put("presel_cluster_means", std::vector<Mean>(fs.clustering_->clusterMeans_, fs.clustering_->clusterMeans_ + size_t(nc) * dp),
            dims(nc, dp));
    std::vector<uint8_t> sel(size_t(r.nFrames) * nc);
    for (size_t i = 0; i < sel.size(); ++i)
        sel[i] = fs.activeClusters_[i] ? 1 : 0;
    out.put("presel_selection", sel, dims(r.nFrames, nc));
}

int runScore(const Core::Configuration& c, const std::string& requestPath, const std::string& replyPath) {
    Request r;
    if (!r.read(requestPath)) {
        std::cerr << "ref_scorers: malformed request " << requestPath << std::endl;
        return 2;
    }
    Core::Ref<Mm::MixtureSet> ms = buildMixtureSet(r);
    Reply                     out(replyPath);
    out.scalar<uint32_t>("kind", r.kind);
    putCovarianceElements(out, *ms);
    switch (r.kind) {
        case kSimd: scoreSimd(c, r, ms, out); break;
        case kDiagonalMaximum: scoreAssigning<Mm::GaussDiagonalMaximumFeatureScorer>(c, r, ms, out); break;
        case kDiagonalSum: scoreAssigning<Mm::GaussDiagonalSumFeatureScorer>(c, r, ms, out); break;
        case kBatchInt: {
            Mm::BatchIntFeatureScorer fs(c, ms);
            runBatch(fs, r, out);
            putIntTables(fs, r, out);
        } break;
        case kBatchFast: {
            Mm::BatchUnrolledIntFeatureScorer fs(c, ms);
            runBatch(fs, r, out);
            putIntTables(fs, r, out);
        } break;
        case kBatchFloat: {
            Mm::BatchFloatFeatureScorer fs(c, ms);
            runBatch(fs, r, out);
            putFloatTables(fs, r, out);
        } break;
        case kPreselInt: {
            Mm::BatchPreselectionIntFeatureScorer fs(c, ms);
            runBatch(fs, r, out);
            putIntTables(fs, r, out);
            putClustering<Mm::BatchPreselectionIntFeatureScorer, uint8_t>(fs, r, out);
        } break;
        case kPreselFloat: {
            Mm::BatchPreselectionFloatFeatureScorer fs(c, ms);
            runBatch(fs, r, out);
            putFloatTables(fs, r, out);
            putClustering<Mm::BatchPreselectionFloatFeatureScorer, float>(fs, r, out);
        } break;
        default:
            std::cerr << "ref_scorers: unknown scorer kind " << r.kind << std::endl;
            return 2;
    }
    out.os.flush();
    return out.os ? 0 : 4;
}

// Mm::Module_::readMixtureSet's steps (src/Mm/Module.cc:152-182) around MixtureSet::read(std::istream&) on the
// reference's CompressedInputStream, which is what its FormatReader reaches for ".pms" and ".gz".
int runPms(const std::string& path, const std::string& replyPath, uint32_t offset, uint32_t reduced) {
    Core::CompressedInputStream is(path);
    Mm::MixtureSet              ms;
    bool                        good = ms.read(is);
    Reply                       out(replyPath);
    out.scalar<uint32_t>("good", good ? 1 : 0);
    if (good) {
        if (offset > 0)
            ms.setOffset(offset);
        if (reduced > 0)
            ms.setDimension(reduced);
        std::vector<float>    means, variances;
        std::vector<uint32_t> dnsMean, dnsCov, offsets(1, 0), mixDns;
        std::vector<double>   logWeights;
        for (uint32_t i = 0; i < ms.nMeans(); ++i)
            means.insert(means.end(), ms.mean(i)->begin(), ms.mean(i)->end());
        for (uint32_t i = 0; i < ms.nCovariances(); ++i)
            variances.insert(variances.end(), ms.covariance(i)->diagonal().begin(), ms.covariance(i)->diagonal().end());
        for (uint32_t i = 0; i < ms.nDensities(); ++i) {
            dnsMean.push_back(ms.density(i)->meanIndex());
            dnsCov.push_back(ms.density(i)->covarianceIndex());
        }
        for (uint32_t m = 0; m < ms.nMixtures(); ++m) {
            for (size_t d = 0; d < ms.mixture(m)->nDensities(); ++d) {
                mixDns.push_back(ms.mixture(m)->densityIndex(d));
                logWeights.push_back(ms.mixture(m)->logWeight(d));
            }
            offsets.push_back(mixDns.size());
        }
        out.scalar<uint32_t>("dimension", ms.dimension());
        out.put("means", means);
        out.put("variances", variances);
        out.put("density_mean", dnsMean);
        out.put("density_covariance", dnsCov);
        out.put("mixture_offsets", offsets);
        out.put("mixture_densities", mixDns);
        out.put("mixture_log_weights", logWeights);
    }
    out.os.flush();
    return out.os ? 0 : 4;
}

class RefScorers : public Core::Application {
public:
    RefScorers() {
        setTitle("ref-scorers");
        setDefaultLoadConfigurationFile(false);
        setDefaultOutputXmlHeader(false);
    }
    virtual int main(const std::vector<std::string>& arguments) {
        size_t i = 0;
        while (i < arguments.size() && arguments[i] != "score" && arguments[i] != "pms")
            ++i;
        if (i + 2 < arguments.size() && arguments[i] == "score")
            return runScore(select("scorer"), arguments[i + 1], arguments[i + 2]);
        if (i + 4 < arguments.size() && arguments[i] == "pms")
            return runPms(arguments[i + 1], arguments[i + 2], std::strtoul(arguments[i + 3].c_str(), 0, 10),
                          std::strtoul(arguments[i + 4].c_str(), 0, 10));
        std::cerr << "usage: ref_scorers [--*.param=value] score REQUEST REPLY | pms FILE REPLY OFFSET DIMENSION" << std::endl;
        return 2;
    }
};

}  // namespace

APPLICATION(RefScorers)
