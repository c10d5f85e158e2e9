// MixtureSetEstimatorFile.cc -- mixture sets from RASR's binary estimator (accumulator) files.
//
// Every file name whose extension is not ".pms" or ".gz" is read by the reference as a maximum-
// likelihood mixture-set estimator file and the mixture set is estimated from it:
//   MixtureSetReader::read                     src/Mm/MixtureSetReader.hh:105-117 (default reader)
//   MixtureSetEstimatorReader::read            src/Mm/MixtureSetReader.cc:52-74
//   Module_::createMixtureSetEstimator         src/Mm/Module.cc:211-227 ("estimator-type" maximum-likelihood)
//   AbstractMixtureSetEstimator::read          src/Mm/AbstractMixtureSetEstimator.cc:404-414, 433-479
//   AbstractMixtureSetEstimator::estimate      src/Mm/AbstractMixtureSetEstimator.cc:299-337
//   MixtureSetEstimatorIndexMap                src/Mm/AbstractMixtureSetEstimator.cc:804-817
//   Mean/CovarianceEstimator::estimate         src/Mm/GaussDensityEstimator.cc:148-227
//   AbstractMixtureEstimator::read/estimate    src/Mm/MixtureEstimator.cc:47-66, 112-123, 140-161
//   VectorAccumulator::read                    src/Mm/VectorAccumulator.hh (size, f64 sums, weight)
//   Mixture::addDensity / normalizeWeights     src/Mm/Mixture.cc:63-74, logExpNorm Utilities.hh:44-51
// Core::BinaryInputStream: native (little-endian) byte order, no compression.
//
// The other direction (include/rasr_gmm_estimator.h): writeEstimatorFile is the writer of such a file,
//   AbstractMixtureSetEstimator::write         src/Mm/AbstractMixtureSetEstimator.cc:416-420, 481-509
// and gmm_estimator_combine the trainer's combine action over several of them,
//   accumulate(Core::BinaryInputStreams&, os)  src/Mm/AbstractMixtureSetEstimator.cc:171-290.
// The discriminative (EBW) estimator's file is the same layout, same magic and version 2, with
//   EbwDiscriminativeMeanEstimator::write        src/Mm/EbwDiscriminativeGaussDensityEstimator.cc:55-58   every mean's
//                                                accumulator followed by its denominator accumulator
//   EbwDiscriminativeCovarianceEstimator::write  cc:150-153   every covariance likewise
//   EbwDiscriminativeMixtureEstimator::write     src/Mm/EbwDiscriminativeMixtureEstimator.cc:148-154   a mixture's
//                                                (density, weight) entries followed by its f64 denominator weights
//   DiscriminativeMixtureSetEstimator::write     src/Mm/DiscriminativeMixtureSetEstimator.cc:115-119   the f64 objective
//                                                function as the file's last field (read for version > 1, cc:105-113)
// (writeDiscriminativeEstimatorFile), combined by gmm_estimator_combine_discriminative as in
//   EbwDiscriminativeMean/CovarianceEstimator::accumulate  EbwDiscriminativeGaussDensityEstimator.cc:40-44, 135-139
//   EbwDiscriminativeMixtureEstimator::accumulate(is, os)  EbwDiscriminativeMixtureEstimator.cc:172-186
//   DiscriminativeMixtureSetEstimator::accumulate(is, os)  DiscriminativeMixtureSetEstimator.cc:162-177.
// Nothing in the header tells the two formats apart: the discriminative reader refuses a file that does not parse as
// one to its last byte (a maximum-likelihood file does not).
//
// The arithmetic follows the reference in f64 with the reference's operation order, results stored as
// f32 means / variances and f64 log weights.  One order is not defined by the reference: the covariance
// estimate sums the squared mean statistics of the covariance's means in the iteration order of an
// unordered_set of pointers (GaussDensityEstimator.hh CovarianceToMeanSetMap); here they are summed in mean
// index order (f64 sums of positive terms: the order moves the f32 variance only on an exact rounding tie).
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <string>
#include <vector>

#include "../../../include/rasr_gmm_io.h"
#include "../gmm_estimator.hh"

namespace rasr_gmm {
void setLastError(const std::string& msg);
}
using rasr_gmm::setLastError;

namespace {

struct Reader {  // Core::BinaryInputStream over a byte buffer
    const unsigned char* p;
    const unsigned char* end;
    bool                 fail = false;
    template <class T>
    T get() {
        T v{};
        if (static_cast<size_t>(end - p) < sizeof(T)) {
            fail = true;
            p    = end;
            return v;
        }
        std::memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
};

struct Accumulator {  // VectorAccumulator<..., Sum = f64>
    std::vector<double> sum;
    double              weight = 0;
    void read(Reader& r, uint32_t version) {
        const uint32_t n = r.get<uint32_t>();
        if (r.fail || static_cast<uint64_t>(n) * 8 > static_cast<uint64_t>(r.end - r.p)) {
            r.fail = true;
            return;
        }
        sum.resize(n);
        for (uint32_t k = 0; k < n; ++k)
            sum[k] = r.get<double>();
        weight = version > 0 ? r.get<double>() : static_cast<double>(r.get<uint32_t>());
    }
};

struct DensityEst {
    uint32_t mean = 0, cov = 0;
};
struct MixtureEst {
    std::vector<uint32_t> dens;     // density estimator indices
    std::vector<double>   weights;  // Weight per density
    std::vector<double>   denWeights;  // denWeights_ (discriminative files)
    double                weight() const {  // getWeight: std::accumulate(..., 0.0)
        double s = 0.0;
        for (double w : weights)
            s += w;
        return s;
    }
};

// Core::differenceUlp(f64, f64), src/Core/Utility.cc:75-87
int64_t differenceUlp(double af, double bf) {
    int64_t a, b;
    std::memcpy(&a, &af, 8);
    std::memcpy(&b, &bf, 8);
    if (a < 0)
        a = static_cast<int64_t>((static_cast<uint64_t>(1) << 63) - static_cast<uint64_t>(a));
    if (b < 0)
        b = static_cast<int64_t>((static_cast<uint64_t>(1) << 63) - static_cast<uint64_t>(b));
    const int64_t d = a - b;
    return d < 0 ? -d : d;
}

template <class T>
T* copyOut(const std::vector<T>& v) {
    T* p = static_cast<T*>(std::malloc(std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (p && !v.empty())
        std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

// first-appearance index of a pointer (PointerIndexMap::add)
struct IndexMap {
    std::vector<int64_t>  index;  // estimator -> new index or -1
    std::vector<uint32_t> order;  // new index -> estimator
    explicit IndexMap(size_t n) : index(n, -1) {}
    void add(uint32_t e) {
        if (index[e] < 0) {
            index[e] = static_cast<int64_t>(order.size());
            order.push_back(e);
        }
    }
};

int fail(int code, const std::string& msg) {
    setLastError("mixture set estimator: " + msg);
    return code;
}

struct Writer {  // Core::BinaryOutputStream into a byte vector
    std::vector<unsigned char> bytes;
    template <class T>
    void put(T v) {
        const unsigned char* p = reinterpret_cast<const unsigned char*>(&v);
        bytes.insert(bytes.end(), p, p + sizeof(T));
    }
    void header(uint32_t dimension) {  // writeHeader (cc:416-420) and the dimension (cc:485)
        const char magic[8] = {'M', 'I', 'X', 'S', 'E', 'T', 0, 0};
        bytes.insert(bytes.end(), magic, magic + 8);
        put<uint32_t>(2);  // version_
        put<uint32_t>(dimension);
    }
    void accumulator(const double* sum, size_t n, double weight) {  // VectorAccumulator::write
        put<uint32_t>(static_cast<uint32_t>(n));
        for (size_t k = 0; k < n; ++k)
            put<double>(sum[k]);
        put<double>(weight);
    }
};

// one estimator file as gmm_estimator_combine reads it
struct EstimatorFile {
    uint32_t                 version = 0, dimension = 0;
    std::vector<Accumulator> means, covs;
    std::vector<Accumulator> denMeans, denCovs;  // discriminative files: the denominator accumulators
    std::vector<DensityEst>  dens;
    std::vector<MixtureEst>  mix;
    double                   objective = 0;  // discriminative files
};

// "" or what is wrong with the file
std::string readEstimatorFile(const void* data, uint64_t size, EstimatorFile& f, bool discriminative = false) {
    static const unsigned char empty = 0;
    const unsigned char* b = data ? static_cast<const unsigned char*>(data) : &empty;
    Reader r{b, b + (data ? size : 0)};
    char magic[8];
    for (char& c : magic)
        c = static_cast<char>(r.get<uint8_t>());
    if (r.fail || std::memcmp(magic, "MIXSET", 7) != 0)
        return "magic \"MIXSET\" expected";
    f.version   = r.get<uint32_t>();
    f.dimension = r.get<uint32_t>();
    for (int which = 0; which < 2; ++which) {
        std::vector<Accumulator>& accs = which ? f.covs : f.means;
        std::vector<Accumulator>& den  = which ? f.denCovs : f.denMeans;
        const uint32_t            n    = r.get<uint32_t>();
        for (uint32_t i = 0; i < n && !r.fail; ++i) {
            accs.emplace_back();
            accs.back().read(r, f.version);
            if (discriminative && !r.fail) {
                den.emplace_back();
                den.back().read(r, f.version);
            }
        }
    }
    const uint32_t nDens = r.get<uint32_t>();
    for (uint32_t i = 0; i < nDens && !r.fail; ++i) {
        DensityEst d;
        d.mean = r.get<uint32_t>();
        d.cov  = r.get<uint32_t>();
        if (!r.fail && discriminative && (d.mean >= f.means.size() || d.cov >= f.covs.size()))
            return "a density refers to a mean or covariance out of range";
        f.dens.push_back(d);
    }
    const uint32_t nMix = r.get<uint32_t>();
    for (uint32_t m = 0; m < nMix && !r.fail; ++m) {
        MixtureEst     x;
        const uint32_t n = r.get<uint32_t>();
        if (r.fail || static_cast<uint64_t>(n) * 8 > static_cast<uint64_t>(r.end - r.p)) {
            r.fail = true;
            break;
        }
        for (uint32_t j = 0; j < n && !r.fail; ++j) {
            x.dens.push_back(r.get<uint32_t>());
            x.weights.push_back(f.version > 0 ? r.get<double>() : static_cast<double>(r.get<uint32_t>()));
            if (!r.fail && discriminative && x.dens.back() >= nDens)
                return "a mixture refers to a density out of range";
        }
        if (discriminative)
            for (uint32_t j = 0; j < n && !r.fail; ++j)
                x.denWeights.push_back(r.get<double>());
        f.mix.push_back(std::move(x));
    }
    if (discriminative && f.version > 1)
        f.objective = r.get<double>();
    if (r.fail)
        return "truncated file";
    if (discriminative && r.p != r.end)
        return "bytes left after the objective function: not a discriminative estimator file";
    for (const std::vector<Accumulator>* accs : {&f.means, &f.covs, &f.denMeans, &f.denCovs})
        for (const Accumulator& a : *accs)
            if (a.sum.size() != f.dimension)
                return "an accumulator's size differs from the dimension";
    return "";
}

}  // namespace

namespace rasr_gmm {

std::vector<unsigned char> writeEstimatorFile(const EstimatorTables& t) {
    // MixtureSetEstimatorIndexMap (cc:804-817): first appearance over the mixtures, then their densities
    IndexMap meanMap(t.nMeans), covMap(t.nCovs), densMap(t.nDens);
    for (uint32_t e = 0; e < t.mixOff[t.nMix]; ++e) {
        const uint32_t d = t.mixDens[e];
        meanMap.add(t.dnsMean[d]);
        covMap.add(t.dnsCov[d]);
        densMap.add(d);
    }
    const size_t D = t.D;
    Writer       w;
    w.header(t.D);
    w.put<uint32_t>(static_cast<uint32_t>(meanMap.order.size()));
    for (uint32_t m : meanMap.order)
        w.accumulator(t.meanSums + m * D, D, t.meanWeights[m]);
    w.put<uint32_t>(static_cast<uint32_t>(covMap.order.size()));
    for (uint32_t c : covMap.order)
        w.accumulator(t.covSums + c * D, D, t.covWeights[c]);
    w.put<uint32_t>(static_cast<uint32_t>(densMap.order.size()));
    for (uint32_t d : densMap.order) {  // GaussDensityEstimator::write: mean index, covariance index
        w.put<uint32_t>(static_cast<uint32_t>(meanMap.index[t.dnsMean[d]]));
        w.put<uint32_t>(static_cast<uint32_t>(covMap.index[t.dnsCov[d]]));
    }
    w.put<uint32_t>(t.nMix);
    for (uint32_t m = 0; m < t.nMix; ++m) {  // AbstractMixtureEstimator::write: count, then (density index, weight)
        w.put<uint32_t>(t.mixOff[m + 1] - t.mixOff[m]);
        for (uint32_t e = t.mixOff[m]; e < t.mixOff[m + 1]; ++e) {
            w.put<uint32_t>(static_cast<uint32_t>(densMap.index[t.mixDens[e]]));
            w.put<double>(t.entryWeights[e]);
        }
    }
    return std::move(w.bytes);
}

std::vector<unsigned char> writeDiscriminativeEstimatorFile(const EstimatorTables& t, const DenominatorTables& den) {
    IndexMap meanMap(t.nMeans), covMap(t.nCovs), densMap(t.nDens);
    for (uint32_t e = 0; e < t.mixOff[t.nMix]; ++e) {
        const uint32_t d = t.mixDens[e];
        meanMap.add(t.dnsMean[d]);
        covMap.add(t.dnsCov[d]);
        densMap.add(d);
    }
    const size_t D = t.D;
    Writer       w;
    w.header(t.D);
    w.put<uint32_t>(static_cast<uint32_t>(meanMap.order.size()));
    for (uint32_t m : meanMap.order) {  // EbwDiscriminativeMeanEstimator::write: Precursor, then denAccumulator_
        w.accumulator(t.meanSums + m * D, D, t.meanWeights[m]);
        w.accumulator(den.meanSums + m * D, D, den.meanWeights[m]);
    }
    w.put<uint32_t>(static_cast<uint32_t>(covMap.order.size()));
    for (uint32_t c : covMap.order) {  // EbwDiscriminativeCovarianceEstimator::write
        w.accumulator(t.covSums + c * D, D, t.covWeights[c]);
        w.accumulator(den.covSums + c * D, D, den.covWeights[c]);
    }
    w.put<uint32_t>(static_cast<uint32_t>(densMap.order.size()));
    for (uint32_t d : densMap.order) {
        w.put<uint32_t>(static_cast<uint32_t>(meanMap.index[t.dnsMean[d]]));
        w.put<uint32_t>(static_cast<uint32_t>(covMap.index[t.dnsCov[d]]));
    }
    w.put<uint32_t>(t.nMix);
    for (uint32_t m = 0; m < t.nMix; ++m) {  // EbwDiscriminativeMixtureEstimator::write: Precursor, then denWeights_
        w.put<uint32_t>(t.mixOff[m + 1] - t.mixOff[m]);
        for (uint32_t e = t.mixOff[m]; e < t.mixOff[m + 1]; ++e) {
            w.put<uint32_t>(static_cast<uint32_t>(densMap.index[t.mixDens[e]]));
            w.put<double>(t.entryWeights[e]);
        }
        for (uint32_t e = t.mixOff[m]; e < t.mixOff[m + 1]; ++e)
            w.put<double>(den.entryWeights[e]);
    }
    w.put<double>(den.objective);  // DiscriminativeMixtureSetEstimator::write: os << (Sum) objectiveFunction()
    return std::move(w.bytes);
}

}  // namespace rasr_gmm

extern "C" {

void gmm_default_estimator_config(gmm_estimator_config* c) {
    if (!c)
        return;
    c->minimum_observation_weight = 5.0;  // AbstractMixtureSetEstimator.cc:25-28
    c->minimum_relative_weight    = 0.0;  // :30-33
    c->minimum_variance           = 0.0;  // :35-38
    c->allow_zero_weights         = 0;    // :50-53
    c->normalize_mixture_weights  = 1;    // :55-58
}

int gmm_mixture_set_estimate(const void* data, uint64_t size, const gmm_estimator_config* config,
                             gmm_mixture_set* out) {
    if (!out || (!data && size))
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    std::memset(out, 0, sizeof(*out));
    gmm_estimator_config cfg;
    gmm_default_estimator_config(&cfg);
    if (config)
        cfg = *config;
    static const unsigned char empty = 0;
    Reader r{data ? static_cast<const unsigned char*>(data) : &empty,
             (data ? static_cast<const unsigned char*>(data) : &empty) + size};

    // ---- AbstractMixtureSetEstimator::readHeader / read ----
    char magic[8];
    for (char& c : magic)
        c = static_cast<char>(r.get<uint8_t>());
    // strcmp(_magic, "MIXSET") (MixtureSetEstimator.hh:36): the six letters then a NUL within the 8 bytes
    if (r.fail || std::memcmp(magic, "MIXSET", 7) != 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "magic \"MIXSET\" expected (criticalError, AbstractMixtureSetEstimator.cc:404-411)");
    const uint32_t version   = r.get<uint32_t>();
    const uint32_t dimension = r.get<uint32_t>();
    const uint32_t nMeans    = r.get<uint32_t>();
    if (r.fail)
        return fail(GMM_ERR_INVALID_ARGUMENT, "error reading mixture set estimator (header)");
    std::vector<Accumulator> means, covs;
    for (uint32_t i = 0; i < nMeans && !r.fail; ++i) {
        means.emplace_back();
        means.back().read(r, version);
    }
    const uint32_t nCovs = r.get<uint32_t>();
    for (uint32_t i = 0; i < nCovs && !r.fail; ++i) {
        covs.emplace_back();
        covs.back().read(r, version);
    }
    const uint32_t          nDens = r.get<uint32_t>();
    std::vector<DensityEst> dens;
    for (uint32_t i = 0; i < nDens && !r.fail; ++i) {
        DensityEst d;
        d.mean = r.get<uint32_t>();
        d.cov  = r.get<uint32_t>();
        if (!r.fail && (d.mean >= nMeans || d.cov >= nCovs))
            return fail(GMM_ERR_INVALID_ARGUMENT, "density estimator " + std::to_string(i) + " refers to mean " +
                                                          std::to_string(d.mean) + " / covariance " + std::to_string(d.cov) +
                                                          " (file holds " + std::to_string(nMeans) + " / " +
                                                          std::to_string(nCovs) + ")");
        dens.push_back(d);
    }
    const uint32_t          nMix = r.get<uint32_t>();
    std::vector<MixtureEst> mix;
    for (uint32_t m = 0; m < nMix && !r.fail; ++m) {
        MixtureEst     x;
        const uint32_t n = r.get<uint32_t>();
        if (r.fail || static_cast<uint64_t>(n) * 8 > static_cast<uint64_t>(r.end - r.p)) {
            r.fail = true;
            break;
        }
        for (uint32_t j = 0; j < n && !r.fail; ++j) {
            const uint32_t di = r.get<uint32_t>();
            const double   w  = version > 0 ? r.get<double>() : static_cast<double>(r.get<uint32_t>());
            if (!r.fail && di >= nDens)
                return fail(GMM_ERR_INVALID_ARGUMENT, "mixture " + std::to_string(m) + " refers to density estimator " +
                                                              std::to_string(di) + " of " + std::to_string(nDens));
            x.dens.push_back(di);
            x.weights.push_back(w);
        }
        mix.push_back(std::move(x));
    }
    if (r.fail)  // is.fail(): "error reading mixture set estimator" (cc:469-471), the reader fails (MixtureSetReader.cc:68-71)
        return fail(GMM_ERR_INVALID_ARGUMENT, "error reading mixture set estimator (truncated file)");
    for (const Accumulator& a : means)
        if (a.sum.size() != dimension)
            return fail(GMM_ERR_INVALID_ARGUMENT, "a mean accumulator has " + std::to_string(a.sum.size()) +
                                                          " components, dimension is " + std::to_string(dimension));
    for (const Accumulator& a : covs)
        if (a.sum.size() != dimension)
            return fail(GMM_ERR_INVALID_ARGUMENT, "a covariance accumulator has " + std::to_string(a.sum.size()) +
                                                          " components, dimension is " + std::to_string(dimension));

    // ---- estimate (cc:305-337) ----
    if (!cfg.allow_zero_weights)  // checkEventsWithZeroWeight (cc:422-431): zero-weight mixture -> criticalError
        for (uint32_t m = 0; m < nMix; ++m)
            if (mix[m].weight() == 0)
                return fail(GMM_ERR_INVALID_ARGUMENT, "Mixture " + std::to_string(m) + " has zero weight.");
    // CovarianceToMeanSetMap over the density estimators in index-map order, before the removal
    std::vector<std::set<uint32_t>> meanSet(nCovs);
    {
        IndexMap dm(nDens);
        for (const MixtureEst& x : mix)
            for (uint32_t d : x.dens)
                dm.add(d);
        for (uint32_t d : dm.order)
            meanSet[dens[d].cov].insert(dens[d].mean);
    }
    // removeDensitiesWithLowWeight (MixtureEstimator.cc:47-66)
    for (uint32_t m = 0; m < nMix; ++m) {
        MixtureEst& x = mix[m];
        if (x.dens.empty())  // densityIndexWithMaxWeight: verify(!densityEstimators_.empty())
            return fail(GMM_ERR_INVALID_ARGUMENT, "mixture " + std::to_string(m) + " has no densities");
        size_t densityMax = 0;
        for (size_t j = 1; j < x.dens.size(); ++j)
            if (x.weights[j] > x.weights[densityMax])
                densityMax = j;
        const double minWeight = std::max(cfg.minimum_observation_weight, x.weight() * cfg.minimum_relative_weight);
        for (size_t j = 0; j < x.dens.size();) {
            if (!(x.weights[j] >= minWeight) && j != densityMax) {
                x.dens.erase(x.dens.begin() + static_cast<long>(j));
                x.weights.erase(x.weights.begin() + static_cast<long>(j));
                if (densityMax > j)
                    --densityMax;
            }
            else
                ++j;
        }
    }
    // MixtureSetEstimatorIndexMap after the removal: first appearance over mixtures, densities in order
    IndexMap meanMap(nMeans), covMap(nCovs), densMap(nDens);
    for (const MixtureEst& x : mix)
        for (uint32_t d : x.dens) {
            meanMap.add(dens[d].mean);
            covMap.add(dens[d].cov);
            densMap.add(d);
        }

    std::vector<uint32_t> mixOff{0}, mixDens;
    std::vector<double>   mixLogW;
    for (const MixtureEst& x : mix) {
        std::vector<double> lw;
        for (size_t j = 0; j < x.dens.size(); ++j) {
            mixDens.push_back(static_cast<uint32_t>(densMap.index[x.dens[j]]));
            // Mixture::addDensity: log(weight), Core::Type<Weight>::min for weight <= 0
            lw.push_back(x.weights[j] > 0 ? std::log(x.weights[j]) : -std::numeric_limits<double>::max());
        }
        if (cfg.normalize_mixture_weights && !lw.empty()) {  // Mixture::normalizeWeights, logExpNorm
            size_t maxIt = 0;
            for (size_t j = 1; j < lw.size(); ++j)
                if (lw[maxIt] < lw[j])
                    maxIt = j;
            double result = 0;
            for (size_t j = 0; j < lw.size(); ++j)
                if (j != maxIt)
                    result += std::exp(lw[j] - lw[maxIt]);
            const double logNorm = std::log1p(result) + lw[maxIt];
            for (double& v : lw)
                v = v - logNorm;
        }
        mixLogW.insert(mixLogW.end(), lw.begin(), lw.end());
        mixOff.push_back(static_cast<uint32_t>(mixDens.size()));
    }
    std::vector<uint32_t> dnsMean, dnsCov;
    for (uint32_t d : densMap.order) {
        dnsMean.push_back(static_cast<uint32_t>(meanMap.index[dens[d].mean]));
        dnsCov.push_back(static_cast<uint32_t>(covMap.index[dens[d].cov]));
    }
    const size_t       D = dimension;
    std::vector<float> meanOut(meanMap.order.size() * D, 0.0f), varOut(covMap.order.size() * D, 1.0f);
    for (size_t i = 0; i < meanMap.order.size(); ++i) {  // MeanEstimator::estimate: sum / weight, zero if weight 0
        const Accumulator& a = means[meanMap.order[i]];
        if (a.weight == 0)
            continue;
        for (size_t k = 0; k < D; ++k)
            meanOut[i * D + k] = static_cast<float>(a.sum[k] / a.weight);
    }
    const float minVariance = static_cast<float>(cfg.minimum_variance);  // VarianceType minVariance_
    for (size_t i = 0; i < covMap.order.size(); ++i) {  // CovarianceEstimator::estimate (cc:201-227)
        const uint32_t     c = covMap.order[i];
        const Accumulator& a = covs[c];
        if (a.weight == 0)  // new DiagonalCovariance(size): variances 1
            continue;
        // GaussDensityEstimator / CovarianceEstimator: verify(accumulator_.weight() > 0) (GaussDensityEstimator.cc:216)
        if (!(a.weight > 0) || !std::isfinite(a.weight))
            return fail(GMM_ERR_INVALID_ARGUMENT, "covariance " + std::to_string(c) + " has weight " +
                                                          std::to_string(a.weight) + " (verify(weight > 0) failed)");
        std::vector<double> wmss(D, 0.0);  // WeighedMeanSquareSum: x + y * y / meanWeight
        double              wmssWeight = 0;
        for (uint32_t mi : meanSet[c]) {
            const Accumulator& ma = means[mi];
            if (ma.weight > 0) {
                for (size_t k = 0; k < D; ++k)
                    wmss[k] = wmss[k] + ma.sum[k] * ma.sum[k] / ma.weight;
                wmssWeight += ma.weight;
            }
        }
        if (differenceUlp(a.weight, wmssWeight) > static_cast<int64_t>(1e12))  // verify(isAlmostEqualUlp(...))
            return fail(GMM_ERR_INVALID_ARGUMENT, "covariance " + std::to_string(c) + " has weight " +
                                                          std::to_string(a.weight) + " but its means weigh " +
                                                          std::to_string(wmssWeight) + " (verify failed)");
        for (size_t k = 0; k < D; ++k) {
            float v = static_cast<float>((a.sum[k] - wmss[k]) / a.weight);  // normalizedMinus<Sum>
            if (minVariance != 0 && v < minVariance)                        // applyMinimumVariance
                v = minVariance;
            varOut[i * D + k] = v;
        }
    }

    gmm_mixture_set res;
    res.dimension           = dimension;
    res.n_means             = static_cast<uint32_t>(meanMap.order.size());
    res.means               = copyOut(meanOut);
    res.n_covariances       = static_cast<uint32_t>(covMap.order.size());
    res.variances           = copyOut(varOut);
    res.n_densities         = static_cast<uint32_t>(densMap.order.size());
    res.density_mean        = copyOut(dnsMean);
    res.density_covariance  = copyOut(dnsCov);
    res.n_mixtures          = nMix;
    res.mixture_offsets     = copyOut(mixOff);
    res.mixture_densities   = copyOut(mixDens);
    res.mixture_log_weights = copyOut(mixLogW);
    *out                    = res;
    if (!res.means || !res.variances || !res.density_mean || !res.density_covariance || !res.mixture_offsets ||
        !res.mixture_densities || !res.mixture_log_weights) {
        gmm_mixture_set_free(out);
        return fail(GMM_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    return GMM_OK;
}

static int combineFiles(const void* const* data, const uint64_t* size, uint32_t n, void* out, uint64_t capacity,
                        uint64_t* outSize, bool discriminative) {
    if (!data || !size || !outSize)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0)
        return fail(GMM_ERR_INVALID_ARGUMENT, "combine: no estimator files");
    EstimatorFile sum;
    for (uint32_t i = 0; i < n; ++i) {
        EstimatorFile     f;
        const std::string where = "combine: file " + std::to_string(i) + ": ";
        const std::string err   = readEstimatorFile(data[i], size[i], f, discriminative);
        if (!err.empty())
            return fail(GMM_ERR_INVALID_ARGUMENT, where + err);
        if (i == 0) {  // the first file supplies the starting value
            sum = std::move(f);
            continue;
        }
        if (f.version != sum.version)
            return fail(GMM_ERR_INVALID_ARGUMENT, where + "Different versions.");
        if (f.dimension != sum.dimension)
            return fail(GMM_ERR_INVALID_ARGUMENT, where + "Mismatch in dimension.");
        if (f.means.size() != sum.means.size() || f.covs.size() != sum.covs.size() || f.dens.size() != sum.dens.size() ||
            f.mix.size() != sum.mix.size())
            return fail(GMM_ERR_INVALID_ARGUMENT, where + "Mismatch in number of means, covariances, densities or mixtures.");
        for (size_t d = 0; d < f.dens.size(); ++d)  // accumulateDensity: equal mean and covariance indices
            if (f.dens[d].mean != sum.dens[d].mean || f.dens[d].cov != sum.dens[d].cov)
                return fail(GMM_ERR_INVALID_ARGUMENT, where + "density " + std::to_string(d) + " differs (topology mismatch)");
        for (size_t m = 0; m < f.mix.size(); ++m)  // accumulateMixture: equal density indices
            if (f.mix[m].dens != sum.mix[m].dens)
                return fail(GMM_ERR_INVALID_ARGUMENT, where + "mixture " + std::to_string(m) + " differs (topology mismatch)");
        // VectorAccumulator::operator+=: sum = sum + other, weight = weight + other
        const auto add = [](Accumulator& dst, const Accumulator& src) {
            for (size_t k = 0; k < dst.sum.size(); ++k)
                dst.sum[k] = dst.sum[k] + src.sum[k];
            dst.weight = dst.weight + src.weight;
        };
        for (size_t a = 0; a < f.means.size(); ++a)
            add(sum.means[a], f.means[a]);
        for (size_t a = 0; a < f.covs.size(); ++a)
            add(sum.covs[a], f.covs[a]);
        // the denominator accumulators (EbwDiscriminativeMean/CovarianceEstimator::accumulate); none in an ML file
        for (size_t a = 0; a < f.denMeans.size(); ++a)
            add(sum.denMeans[a], f.denMeans[a]);
        for (size_t a = 0; a < f.denCovs.size(); ++a)
            add(sum.denCovs[a], f.denCovs[a]);
        for (size_t m = 0; m < f.mix.size(); ++m) {
            for (size_t j = 0; j < f.mix[m].weights.size(); ++j)
                sum.mix[m].weights[j] = sum.mix[m].weights[j] + f.mix[m].weights[j];
            for (size_t j = 0; j < f.mix[m].denWeights.size(); ++j)  // weight += _weight, EbwDiscriminativeMixtureEstimator.cc:176-182
                sum.mix[m].denWeights[j] = sum.mix[m].denWeights[j] + f.mix[m].denWeights[j];
        }
        sum.objective += f.objective;  // DiscriminativeMixtureSetEstimator.cc:168-174
    }
    Writer w;
    w.header(sum.dimension);
    for (int which = 0; which < 2; ++which) {
        const std::vector<Accumulator>& accs = which ? sum.covs : sum.means;
        const std::vector<Accumulator>& den  = which ? sum.denCovs : sum.denMeans;
        w.put<uint32_t>(static_cast<uint32_t>(accs.size()));
        for (size_t i = 0; i < accs.size(); ++i) {
            w.accumulator(accs[i].sum.data(), accs[i].sum.size(), accs[i].weight);
            if (discriminative)
                w.accumulator(den[i].sum.data(), den[i].sum.size(), den[i].weight);
        }
    }
    w.put<uint32_t>(static_cast<uint32_t>(sum.dens.size()));
    for (const DensityEst& d : sum.dens) {
        w.put<uint32_t>(d.mean);
        w.put<uint32_t>(d.cov);
    }
    w.put<uint32_t>(static_cast<uint32_t>(sum.mix.size()));
    for (const MixtureEst& x : sum.mix) {
        w.put<uint32_t>(static_cast<uint32_t>(x.dens.size()));
        for (size_t j = 0; j < x.dens.size(); ++j) {
            w.put<uint32_t>(x.dens[j]);
            w.put<double>(x.weights[j]);
        }
        for (double dw : x.denWeights)
            w.put<double>(dw);
    }
    if (discriminative)
        w.put<double>(sum.objective);
    *outSize = w.bytes.size();
    if (!out)
        return GMM_OK;
    if (capacity < w.bytes.size())
        return fail(GMM_ERR_CAPACITY, "combine: " + std::to_string(w.bytes.size()) + " bytes, capacity " + std::to_string(capacity));
    std::memcpy(out, w.bytes.data(), w.bytes.size());
    return GMM_OK;
}

// ---- the EBW estimate (include/rasr_gmm_estimator.h, "The EBW estimate") ----

void gmm_default_ebw_config(gmm_ebw_config* c) {
    if (!c)
        return;
    c->minimum_observation_weight = 5.0;   // AbstractMixtureSetEstimator.cc:25-28
    c->minimum_relative_weight    = 0.0;   // :30-33
    c->minimum_variance           = 0.0;   // :35-38
    c->normalize_mixture_weights  = 1;     // :55-58
    c->iteration_constants_type   = GMM_EBW_GLOBAL_RWTH;  // IterationConstants.cc:659-663
    c->step_size                  = 1.1;   // :665-673
    c->minimum_icd                = 1.0;   // :675-678
    c->beta                       = 1.0;   // :163-167
    c->sigma_minimum              = -1.0;  // unset: sigma_minimum_factor * the smallest previous variance (:289-293)
    c->sigma_minimum_factor       = 1e-5;  // :253-258
    c->number_of_iterations       = 100;   // EbwDiscriminativeMixtureEstimator.cc:24-27
}

static int ebwEstimate(const void* data, uint64_t size, const gmm_mixture_set* prev, const gmm_ebw_config* config,
                       gmm_mixture_set* out, std::vector<double>* constantsOut) {
    if ((!data && size) || !prev)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    gmm_ebw_config cfg;
    gmm_default_ebw_config(&cfg);
    if (config)
        cfg = *config;
    if (cfg.iteration_constants_type == GMM_EBW_CAMBRIDGE)  // maximumRoot begins with require(false), IterationConstants.cc:595
        return fail(GMM_ERR_UNSUPPORTED, "EBW estimate: iteration constants of type cambridge are not supported");
    if (cfg.iteration_constants_type != GMM_EBW_GLOBAL_RWTH && cfg.iteration_constants_type != GMM_EBW_LOCAL_RWTH)
        return fail(GMM_ERR_INVALID_ARGUMENT, "EBW estimate: unknown iteration constants type");
    EstimatorFile     f;
    const std::string err = readEstimatorFile(data, size, f, true);
    if (!err.empty())
        return fail(GMM_ERR_INVALID_ARGUMENT, "EBW estimate: " + err);
    // distributePreviousMixtureSet (DiscriminativeMixtureSetEstimator.cc:51-86): previous index i is file index i
    const size_t D = f.dimension;
    if (prev->dimension != f.dimension || prev->n_mixtures != f.mix.size() || prev->n_densities != f.dens.size() ||
        prev->n_means != f.means.size() || prev->n_covariances != f.covs.size())
        return fail(GMM_ERR_INVALID_ARGUMENT, "EBW estimate: previous mixture set differs in topology");
    std::vector<std::vector<double>> prevW(f.mix.size());
    for (size_t m = 0; m < f.mix.size(); ++m) {
        const uint32_t e0 = prev->mixture_offsets[m], n = prev->mixture_offsets[m + 1] - e0;
        if (n != f.mix[m].dens.size())  // setPreviousMixture: require(mixture->nDensities() == nDensities())
            return fail(GMM_ERR_INVALID_ARGUMENT, "EBW estimate: previous mixture set differs in topology (mixture " +
                                                          std::to_string(m) + ")");
        for (uint32_t j = 0; j < n; ++j)
            prevW[m].push_back(std::exp(prev->mixture_log_weights[e0 + j]));  // Mixture::weight
    }
    // removeDensitiesWithLowWeight (cc:136-140; DiscriminativeMixtureEstimator.cc:34-49, the unconditional --densityMax
    // included)
    if (cfg.minimum_observation_weight != 0 || cfg.minimum_relative_weight != 0)
        for (size_t m = 0; m < f.mix.size(); ++m) {
            MixtureEst& x = f.mix[m];
            if (x.dens.empty())
                return fail(GMM_ERR_INVALID_ARGUMENT, "EBW estimate: mixture " + std::to_string(m) + " has no densities");
            uint32_t densityMax = 0;
            for (uint32_t j = 1; j < x.dens.size(); ++j)
                if (x.weights[j] > x.weights[densityMax])
                    densityMax = j;
            for (uint32_t j = 0; j < x.dens.size();) {
                const bool enough = x.weights[j] >= cfg.minimum_observation_weight;
                const bool enoughRelative = prevW[m][j] >= cfg.minimum_relative_weight;
                if ((!enough || !enoughRelative) && j != densityMax) {
                    x.dens.erase(x.dens.begin() + j);
                    x.weights.erase(x.weights.begin() + j);
                    x.denWeights.erase(x.denWeights.begin() + j);
                    prevW[m].erase(prevW[m].begin() + j);
                    --densityMax;
                }
                else
                    ++j;
            }
        }
    // MixtureSetEstimatorIndexMap after the removal; the densities of every covariance in (mixture, density) order
    IndexMap meanMap(f.means.size()), covMap(f.covs.size()), densMap(f.dens.size());
    struct Aug {
        uint32_t dens, mix;
        double   prevWeight;
    };
    std::vector<std::vector<Aug>> cim(f.covs.size());
    std::vector<char>             seen(f.dens.size(), 0);
    for (size_t m = 0; m < f.mix.size(); ++m)
        for (size_t j = 0; j < f.mix[m].dens.size(); ++j) {
            const uint32_t d = f.mix[m].dens[j];
            if (seen[d])  // require(set.find(augmented) == set.end()), IterationConstants.cc:127
                return fail(GMM_ERR_UNSUPPORTED, "EBW estimate: density " + std::to_string(d) + " is shared by more than one mixture entry");
            seen[d] = 1;
            meanMap.add(f.dens[d].mean);
            covMap.add(f.dens[d].cov);
            densMap.add(d);
            cim[f.dens[d].cov].push_back(Aug{d, static_cast<uint32_t>(m), prevW[m][j]});
        }
    const auto dtW = [&](uint32_t mean) { return f.means[mean].weight - f.denMeans[mean].weight; };
    // Xi (IterationConstants.cc:169-200)
    std::vector<double> xi(f.mix.size());
    for (size_t m = 0; m < f.mix.size(); ++m) {
        double maxAbs = 0, maxNumDen = 0;
        for (uint32_t d : f.mix[m].dens) {
            const uint32_t mean = f.dens[d].mean;
            const double   w = dtW(mean), a = std::fabs(w), den = f.denMeans[mean].weight;
            if (maxAbs < a) {
                maxAbs    = a;
                maxNumDen = std::max(w + den, den);
            }
        }
        const double denominator = (maxAbs < maxNumDen && maxNumDen > 0) ? 1 + (maxAbs - 1) * maxAbs / maxNumDen : 1;
        xi[m]                    = cfg.beta / denominator;
    }
    // sigma-minimum (cc:271-293): over the covariances that hold a density
    float minPrev = std::numeric_limits<float>::max();
    for (uint32_t c : covMap.order)
        for (size_t k = 0; k < D; ++k)
            minPrev = std::min(minPrev, prev->variances[c * D + k]);
    const double sigmaMin = cfg.sigma_minimum >= 0 ? cfg.sigma_minimum : cfg.sigma_minimum_factor * minPrev;
    // the iteration constants b and the densities' constants, covariances in ascending OUTPUT index
    std::vector<double> icMean(f.means.size(), 1.0);  // iterationConstant_(1)
    std::vector<double> localB(f.mix.size(), 0.0);
    std::vector<char>   localSet(f.mix.size(), 0);
    std::vector<double> globalB(f.covs.size(), 0.0);
    for (uint32_t c : covMap.order) {
        // minimumDk (cc:298-334)
        std::vector<double> numerator(D), denominator(D, 0.0);
        for (size_t k = 0; k < D; ++k)
            numerator[k] = 0 - (f.covs[c].sum[k] - f.denCovs[c].sum[k]);
        for (const Aug& a : cim[c]) {
            const uint32_t mean = f.dens[a.dens].mean;
            const double   w    = dtW(mean);
            for (size_t k = 0; k < D; ++k) {
                const double dtSum = f.means[mean].sum[k] - f.denMeans[mean].sum[k];
                const float  pm    = prev->means[mean * D + k];
                const double t2    = 2 * dtSum - w * pm;
                const double t3    = dtSum - w * pm;
                numerator[k] += sigmaMin * w;
                numerator[k] += t2 * pm;
                numerator[k] += xi[a.mix] * t3 * t3;
                denominator[k] += (prev->variances[c * D + k] - sigmaMin) * a.prevWeight;
            }
        }
        double ratioMax = numerator[0] / denominator[0];
        for (size_t k = 1; k < D; ++k) {
            const double r = numerator[k] / denominator[k];
            if (ratioMax < r)
                ratioMax = r;
        }
        const double dkMin = ratioMax > 0 ? ratioMax : 0;
        double       ic    = 1;  // Icb::default_
        for (const Aug& a : cim[c]) {
            double dk = 1 / xi[a.mix];
            dk -= dtW(f.dens[a.dens].mean);
            if (a.prevWeight > 0)
                dk /= a.prevWeight;
            if (cfg.iteration_constants_type == GMM_EBW_GLOBAL_RWTH)  // cc:371-383
                ic = std::max(ic, std::max(dk, dkMin));
            else {  // cc:425-437
                if (!localSet[a.mix]) {
                    localSet[a.mix] = 1;
                    localB[a.mix]   = cfg.step_size * std::max(1.0, dkMin);
                }
                localB[a.mix] = std::max(cfg.step_size * dk, localB[a.mix]);
            }
        }
        globalB[c] = ic * cfg.step_size;
    }
    for (uint32_t c : covMap.order)  // IterationConstants::set (cc:701-714), GlobalRwth / LocalRwth ::set
        for (const Aug& a : cim[c]) {
            double ic = cfg.iteration_constants_type == GMM_EBW_GLOBAL_RWTH ? globalB[c] : localB[a.mix];
            ic *= a.prevWeight;  // usePooledVariances_
            ic = std::max(cfg.minimum_icd, ic);
            if (!(ic >= 0) || !std::isfinite(ic))  // setIterationConstant's verifies
                return fail(GMM_ERR_INVALID_ARGUMENT, "EBW estimate: iteration constant of density " + std::to_string(a.dens) + " is not a finite non-negative number");
            icMean[f.dens[a.dens].mean] = ic;
        }
    if (constantsOut) {
        constantsOut->clear();
        for (uint32_t d : densMap.order)
            constantsOut->push_back(icMean[f.dens[d].mean]);
    }
    if (!out)
        return GMM_OK;
    std::memset(out, 0, sizeof(*out));
    // mixture weights, the Cambridge scheme (EbwDiscriminativeMixtureEstimator.cc:39-91, 123-136)
    std::vector<uint32_t> mixOff{0}, mixDens;
    std::vector<double>   mixLogW;
    for (size_t m = 0; m < f.mix.size(); ++m) {
        const MixtureEst&   x = f.mix[m];
        const size_t        n = x.dens.size();
        std::vector<double> w;
        if (n > 1 && x.weight() > 2.2204460492503131e-16) {
            w.resize(n);
            double kMax = 0;
            for (size_t j = 0; j < n; ++j) {
                w[j] = prevW[m][j];
                if (w[j] > 2.2204460492503131e-16)
                    kMax = std::max(kMax, x.denWeights[j] / w[j]);
                else
                    w[j] = 0;
            }
            std::vector<double> k(n, 0.0);
            for (size_t j = 0; j < n; ++j)
                if (w[j] > 0)
                    k[j] = kMax - x.denWeights[j] / w[j];
            for (uint32_t iter = 0; iter < cfg.number_of_iterations; ++iter) {
                for (size_t j = 0; j < n; ++j) {
                    if (w[j] > 0)
                        w[j] = x.weights[j] + k[j] * w[j];
                    if (w[j] < 0)
                        w[j] = 0;
                }
                if (cfg.normalize_mixture_weights) {
                    double sum = 0;
                    for (double v : w)
                        sum += v;
                    if (sum > 2.2250738585072014e-308)
                        for (double& v : w)
                            v = v / sum;
                    else
                        for (double& v : w)
                            v = 1 / static_cast<double>(n);
                }
            }
        }
        else
            w.assign(n, cfg.normalize_mixture_weights ? 1 / static_cast<double>(n) : 1);
        std::vector<double> lw;
        for (size_t j = 0; j < n; ++j) {
            mixDens.push_back(static_cast<uint32_t>(densMap.index[x.dens[j]]));
            lw.push_back(w[j] > 0 ? std::log(w[j]) : -std::numeric_limits<double>::max());  // Mixture::addDensity
        }
        if (cfg.normalize_mixture_weights && !lw.empty()) {  // Mixture::normalizeWeights, logExpNorm
            size_t maxIt = 0;
            for (size_t j = 1; j < lw.size(); ++j)
                if (lw[maxIt] < lw[j])
                    maxIt = j;
            double result = 0;
            for (size_t j = 0; j < lw.size(); ++j)
                if (j != maxIt)
                    result += std::exp(lw[j] - lw[maxIt]);
            const double logNorm = std::log1p(result) + lw[maxIt];
            for (double& v : lw)
                v = v - logNorm;
        }
        mixLogW.insert(mixLogW.end(), lw.begin(), lw.end());
        mixOff.push_back(static_cast<uint32_t>(mixDens.size()));
    }
    std::vector<uint32_t> dnsMean, dnsCov;
    for (uint32_t d : densMap.order) {
        dnsMean.push_back(static_cast<uint32_t>(meanMap.index[f.dens[d].mean]));
        dnsCov.push_back(static_cast<uint32_t>(covMap.index[f.dens[d].cov]));
    }
    // means (EbwDiscriminativeGaussDensityEstimator.cc:73-89), by file index: the covariances need them too
    std::vector<float> newMean(f.means.size() * D);
    for (size_t mean = 0; mean < f.means.size(); ++mean) {
        const double ic = icMean[mean], weight = dtW(static_cast<uint32_t>(mean)) + ic;
        for (size_t k = 0; k < D; ++k) {
            const float pm = prev->means[mean * D + k];
            if (weight > 0) {
                const double buffer = (f.means[mean].sum[k] - f.denMeans[mean].sum[k]) + ic * pm;
                newMean[mean * D + k] = static_cast<float>(buffer / weight);
            }
            else
                newMean[mean * D + k] = pm;
        }
    }
    std::vector<float> meanOut(meanMap.order.size() * D), varOut(covMap.order.size() * D);
    for (size_t i = 0; i < meanMap.order.size(); ++i)
        std::memcpy(&meanOut[i * D], &newMean[meanMap.order[i] * D], D * sizeof(float));
    // covariances (cc:165-198): a covariance's means in order of first appearance among its densities
    const float minVariance = static_cast<float>(cfg.minimum_variance);
    for (size_t i = 0; i < covMap.order.size(); ++i) {
        const uint32_t      c = covMap.order[i];
        std::vector<double> buffer(D);
        for (size_t k = 0; k < D; ++k)
            buffer[k] = f.covs[c].sum[k] - f.denCovs[c].sum[k];
        double            weight = 0;
        std::vector<char> done(f.means.size(), 0);
        for (const Aug& a : cim[c]) {
            const uint32_t mean = f.dens[a.dens].mean;
            if (done[mean])
                continue;
            done[mean]         = 1;
            const double ic    = icMean[mean];
            const double tmpW  = dtW(mean) + ic;
            weight += tmpW;
            for (size_t k = 0; k < D; ++k) {
                const float pm          = prev->means[mean * D + k];
                double      previousSum = prev->variances[c * D + k];
                previousSum += pm * pm;  // an f32 product
                previousSum *= ic;
                const double newSum = tmpW * newMean[mean * D + k] * newMean[mean * D + k];
                buffer[k] += previousSum - newSum;
            }
        }
        if (!(weight > 0))  // verify(weight > 0)
            return fail(GMM_ERR_INVALID_ARGUMENT, "EBW estimate: covariance " + std::to_string(c) + " has weight " + std::to_string(weight));
        for (size_t k = 0; k < D; ++k) {
            float v = static_cast<float>(buffer[k] / weight);
            if (!(v > 0))  // verify(result->isPositiveDefinite())
                return fail(GMM_ERR_INVALID_ARGUMENT, "EBW estimate: covariance " + std::to_string(c) + " component " +
                                                              std::to_string(k) + " is not positive (" + std::to_string(v) + ")");
            if (minVariance != 0 && v < minVariance)
                v = minVariance;
            varOut[i * D + k] = v;
        }
    }
    gmm_mixture_set res;
    res.dimension           = f.dimension;
    res.n_means             = static_cast<uint32_t>(meanMap.order.size());
    res.means               = copyOut(meanOut);
    res.n_covariances       = static_cast<uint32_t>(covMap.order.size());
    res.variances           = copyOut(varOut);
    res.n_densities         = static_cast<uint32_t>(densMap.order.size());
    res.density_mean        = copyOut(dnsMean);
    res.density_covariance  = copyOut(dnsCov);
    res.n_mixtures          = static_cast<uint32_t>(f.mix.size());
    res.mixture_offsets     = copyOut(mixOff);
    res.mixture_densities   = copyOut(mixDens);
    res.mixture_log_weights = copyOut(mixLogW);
    *out                    = res;
    if (!res.means || !res.variances || !res.density_mean || !res.density_covariance || !res.mixture_offsets ||
        !res.mixture_densities || !res.mixture_log_weights) {
        gmm_mixture_set_free(out);
        return fail(GMM_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    return GMM_OK;
}

int gmm_estimator_estimate_ebw(const void* data, uint64_t size, const gmm_mixture_set* previous,
                               const gmm_ebw_config* config, gmm_mixture_set* out) {
    if (!out)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    return ebwEstimate(data, size, previous, config, out, nullptr);
}

int gmm_estimator_ebw_iteration_constants(const void* data, uint64_t size, const gmm_mixture_set* previous,
                                          const gmm_ebw_config* config, double* constants, uint32_t capacity,
                                          uint32_t* n) {
    if (!n)
        return fail(GMM_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<double> ic;
    const int           rc = ebwEstimate(data, size, previous, config, nullptr, &ic);
    if (rc != GMM_OK)
        return rc;
    *n = static_cast<uint32_t>(ic.size());
    if (!constants)
        return GMM_OK;
    if (capacity < ic.size())
        return fail(GMM_ERR_CAPACITY, "EBW iteration constants: " + std::to_string(ic.size()) + " densities, capacity " + std::to_string(capacity));
    std::memcpy(constants, ic.data(), ic.size() * sizeof(double));
    return GMM_OK;
}

int gmm_estimator_combine(const void* const* data, const uint64_t* size, uint32_t n, void* out, uint64_t capacity,
                          uint64_t* outSize) {
    return combineFiles(data, size, n, out, capacity, outSize, false);
}

int gmm_estimator_combine_discriminative(const void* const* data, const uint64_t* size, uint32_t n, void* out,
                                         uint64_t capacity, uint64_t* outSize) {
    return combineFiles(data, size, n, out, capacity, outSize, true);
}

}  // extern "C"
