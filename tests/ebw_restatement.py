"""Plain-numpy restatement of the discriminative accumulation contract of include/rasr_gmm_estimator.h (section
"Discriminative training") and of the discriminative estimator file, written from the contract.

Contributions are rows (entry, frame, w_num, w_den) in call order -- (pair) for a Viterbi call, (pair, density in
mixture) for a posterior call -- with NaN for a side on which the contribution is not live.  A row live on neither
side is not part of the call's contribution list.

joint():       the contract: per accumulator the JOINT list (live on at least one side) cut into pieces of CHUNK, each
               side adding its own live rows sequentially within a piece, piece 0 from the table value, later pieces
               from 0 and then added to the table in piece order.
sequential():  one side alone, one f64 add chain in contribution order (the reference's loop).
"""
import struct

import numpy as np

CHUNK = 512
KINDS = (("mean_sums", "mean_weights"), ("covariance_sums", "covariance_weights"), (None, "entry_weights"))


def zero_tables(ms):
    D = ms.dimension
    return {"mean_sums": np.zeros((ms.means.shape[0], D)), "mean_weights": np.zeros(ms.means.shape[0]),
            "covariance_sums": np.zeros((ms.n_covariances, D)), "covariance_weights": np.zeros(ms.n_covariances),
            "entry_weights": np.zeros(ms.n_entries)}


def _destinations(ms, entries):
    dens = ms.mixture_densities[entries]
    return (ms.density_mean[dens].astype(np.int64), ms.density_covariance[dens].astype(np.int64),
            np.asarray(entries, dtype=np.int64))


def _term(kind, w, x):
    if kind == 0:
        return w * x  # plusWeighted
    return (w * x) * x  # plusSquareWeighted


def joint(ms, frames, entries, pair_frame, w_num, w_den, num, den, chunk=CHUNK):
    """Adds the call to copies of the table sets `num` and `den` by the joint-piece rule; w_num / w_den are arrays
    (NaN: not live) or None (the side takes no part).  Returns (num, den)."""
    n = len(entries)
    sides = []
    for w, t in ((w_num, num), (w_den, den)):
        sides.append((None if w is None else np.asarray(w, dtype=np.float64), {k: v.copy() for k, v in t.items()}))
    live = np.zeros(n, dtype=bool)
    for w, _ in sides:
        if w is not None:
            live |= ~np.isnan(w)
    x64 = np.asarray(frames, dtype=np.float32).astype(np.float64)
    dest = _destinations(ms, np.asarray(entries, dtype=np.int64))
    for kind, (sums_key, weights_key) in enumerate(KINDS):
        for k in np.unique(dest[kind][live]):
            rows = np.flatnonzero(live & (dest[kind] == k))  # the joint list of this accumulator
            for w, t in sides:
                if w is None:
                    continue
                for p0 in range(0, len(rows), chunk):
                    first = p0 == 0
                    acc = t[sums_key][k].copy() if (sums_key and first) else (np.zeros(ms.dimension) if sums_key else None)
                    wsum = t[weights_key][k] if first else np.float64(0.0)
                    for r in rows[p0:p0 + chunk]:
                        if np.isnan(w[r]):
                            continue
                        if sums_key:
                            acc = acc + _term(kind, w[r], x64[pair_frame[r]])
                        wsum = wsum + w[r]
                    if first:
                        if sums_key:
                            t[sums_key][k] = acc
                        t[weights_key][k] = wsum
                    else:  # a slab row, added in piece order
                        if sums_key:
                            t[sums_key][k] = t[sums_key][k] + acc
                        t[weights_key][k] = t[weights_key][k] + wsum
    return sides[0][1], sides[1][1]


def sequential(ms, frames, entries, pair_frame, w, tables):
    """One side alone: its live rows added in order, one chain per accumulator."""
    t = {k: v.copy() for k, v in tables.items()}
    if w is None:
        return t
    w = np.asarray(w, dtype=np.float64)
    x64 = np.asarray(frames, dtype=np.float32).astype(np.float64)
    dest = _destinations(ms, np.asarray(entries, dtype=np.int64))
    for r in np.flatnonzero(~np.isnan(w)):
        x = x64[pair_frame[r]]
        t["mean_sums"][dest[0][r]] = t["mean_sums"][dest[0][r]] + _term(0, w[r], x)
        t["mean_weights"][dest[0][r]] = t["mean_weights"][dest[0][r]] + w[r]
        t["covariance_sums"][dest[1][r]] = t["covariance_sums"][dest[1][r]] + _term(1, w[r], x)
        t["covariance_weights"][dest[1][r]] = t["covariance_weights"][dest[1][r]] + w[r]
        t["entry_weights"][dest[2][r]] = t["entry_weights"][dest[2][r]] + w[r]
    return t


def abs_term_sums(ms, frames, entries, pair_frame, w):
    """Per accumulator, (number of live rows, sum of |term|) of one side: the section-11 bound's ingredients."""
    t = zero_tables(ms)
    cnt = {"mean": np.zeros(ms.means.shape[0], dtype=np.int64), "cov": np.zeros(ms.n_covariances, dtype=np.int64)}
    w = np.asarray(w, dtype=np.float64)
    x64 = np.asarray(frames, dtype=np.float32).astype(np.float64)
    dest = _destinations(ms, np.asarray(entries, dtype=np.int64))
    for r in np.flatnonzero(~np.isnan(w)):
        x = x64[pair_frame[r]]
        t["mean_sums"][dest[0][r]] += np.abs(_term(0, w[r], x))
        t["covariance_sums"][dest[1][r]] += np.abs(_term(1, w[r], x))
        cnt["mean"][dest[0][r]] += 1
        cnt["cov"][dest[1][r]] += 1
    return cnt, t


def posterior_rows(ms, pair_frame, pair_mixture, n_frames, posteriors, w_num, w_den, threshold):
    """The contribution rows of a posterior call from the density posteriors [n_pairs, K]: (entries, frames, wN, wD)
    in (pair, density in mixture) order, and the number of bad pairs.  finalWeight = w * (f64) post, live iff
    finalWeight > threshold."""
    off = ms.mixture_offsets.astype(np.int64)
    entries, fr, wn, wd = [], [], [], []
    skipped = 0
    for i in range(len(pair_frame)):
        f, m = int(pair_frame[i]), int(pair_mixture[i])
        if f >= n_frames or m >= len(off) - 1 or off[m + 1] == off[m]:
            skipped += 1
            continue
        for j in range(off[m + 1] - off[m]):
            post = np.float64(posteriors[i, j])
            fw = [np.nan, np.nan]
            for s, w in enumerate((w_num, w_den)):
                if w is not None:
                    v = np.float64(w[i]) * post
                    if v > threshold:
                        fw[s] = v
            entries.append(off[m] + j)
            fr.append(f)
            wn.append(fw[0])
            wd.append(fw[1])
    return (np.array(entries, dtype=np.int64), np.array(fr, dtype=np.int64),
            None if w_num is None else np.array(wn), None if w_den is None else np.array(wd), skipped)


# ---- the discriminative estimator file ----

def _first_appearance(ms):
    mean_new, cov_new, dens_new = {}, {}, {}
    for d in ms.mixture_densities:
        d = int(d)
        mean_new.setdefault(int(ms.density_mean[d]), len(mean_new))
        cov_new.setdefault(int(ms.density_covariance[d]), len(cov_new))
        dens_new.setdefault(d, len(dens_new))
    return mean_new, cov_new, dens_new


def _acc(sums, weight):
    return struct.pack("<I", len(sums)) + np.asarray(sums, dtype="<f8").tobytes() + struct.pack("<d", weight)


def write_file(ms, num, den, objective):
    """Magic, version 2, dimension; means, covariances, densities renumbered by first appearance over the mixtures'
    densities; every mean / covariance accumulator followed by its denominator accumulator; every mixture's (density,
    weight) entries followed by its denominator weights; the objective function last."""
    mean_new, cov_new, dens_new = _first_appearance(ms)
    out = [b"MIXSET\0\0", struct.pack("<II", 2, ms.dimension)]
    for new, sk, wk in ((mean_new, "mean_sums", "mean_weights"), (cov_new, "covariance_sums", "covariance_weights")):
        out.append(struct.pack("<I", len(new)))
        for old in new:  # insertion order = new index order
            out.append(_acc(num[sk][old], num[wk][old]))
            out.append(_acc(den[sk][old], den[wk][old]))
    out.append(struct.pack("<I", len(dens_new)))
    for d in dens_new:
        out.append(struct.pack("<II", mean_new[int(ms.density_mean[d])], cov_new[int(ms.density_covariance[d])]))
    off = ms.mixture_offsets.astype(np.int64)
    out.append(struct.pack("<I", len(off) - 1))
    for m in range(len(off) - 1):
        out.append(struct.pack("<I", off[m + 1] - off[m]))
        for e in range(off[m], off[m + 1]):
            out.append(struct.pack("<Id", dens_new[int(ms.mixture_densities[e])], num["entry_weights"][e]))
        for e in range(off[m], off[m + 1]):
            out.append(struct.pack("<d", den["entry_weights"][e]))
    out.append(struct.pack("<d", objective))
    return b"".join(out)


def read_file(data):
    """The file back as a dict of lists in FILE numbering (means / covariances: (num sums, num weight, den sums, den
    weight); mixtures: (density indices, weights, denominator weights)); raises ValueError on leftover bytes."""
    pos = 0

    def get(fmt):
        nonlocal pos
        v = struct.unpack_from(fmt, data, pos)
        pos += struct.calcsize(fmt)
        return v

    def acc():
        (n,) = get("<I")
        s = np.array(get("<%dd" % n))
        (w,) = get("<d")
        return s, w
    assert data[:8] == b"MIXSET\0\0"
    pos = 8
    version, dim = get("<II")
    f = {"version": version, "dimension": dim, "means": [], "covariances": [], "densities": [], "mixtures": []}
    for key in ("means", "covariances"):
        for _ in range(get("<I")[0]):
            f[key].append(acc() + acc())
    for _ in range(get("<I")[0]):
        f["densities"].append(get("<II"))
    for _ in range(get("<I")[0]):
        (n,) = get("<I")
        dw = [get("<Id") for _ in range(n)]
        f["mixtures"].append(([d for d, _ in dw], [w for _, w in dw], list(get("<%dd" % n))))
    (f["objective"],) = get("<d")
    if pos != len(data):
        raise ValueError("bytes left")
    return f


# ---- the EBW estimate ----

EBW_DEFAULTS = dict(minimum_observation_weight=5.0, minimum_relative_weight=0.0, minimum_variance=0.0,
                    normalize_mixture_weights=True, iteration_constants_type="global-rwth", step_size=1.1,
                    minimum_icd=1.0, beta=1.0, sigma_minimum=-1.0, sigma_minimum_factor=1e-5, number_of_iterations=100)
EPS64, TINY64, LOWEST64 = 2.2204460492503131e-16, 2.2250738585072014e-308, -1.7976931348623157e308


def estimate(prev, num, den, **config):
    """The estimate of include/rasr_gmm_estimator.h "The EBW estimate" from the tables (indexed as `prev`, whose
    numbering must be the file's: first appearance over the mixtures' densities) in plain Python f64 / numpy f32
    scalars, in the header's fixed order.  Returns (model dict in the estimated set's numbering, iteration constants per
    estimated density).  math.exp / math.log are the C library's, as in the library."""
    import math
    c = dict(EBW_DEFAULTS, **config)
    D = prev.dimension
    off = prev.mixture_offsets.astype(np.int64)
    f32 = np.float32
    mixes = []  # per mixture: lists of [density, num weight, den weight, previous weight]
    for m in range(len(off) - 1):
        mixes.append([[int(prev.mixture_densities[e]), float(num["entry_weights"][e]), float(den["entry_weights"][e]),
                       math.exp(float(prev.mixture_log_weights[e]))] for e in range(off[m], off[m + 1])])
    if c["minimum_observation_weight"] != 0 or c["minimum_relative_weight"] != 0:
        for x in mixes:
            dmax = 0
            for j in range(1, len(x)):
                if x[j][1] > x[dmax][1]:
                    dmax = j
            j = 0
            while j < len(x):
                if (not x[j][1] >= c["minimum_observation_weight"] or not x[j][3] >= c["minimum_relative_weight"]) \
                        and j != dmax:
                    del x[j]
                    dmax = (dmax - 1) % (1 << 32)
                else:
                    j += 1
    mean_of = lambda d: int(prev.density_mean[d])  # noqa: E731
    cov_of = lambda d: int(prev.density_covariance[d])  # noqa: E731
    mean_new, cov_new, dens_new, cim = {}, {}, {}, {}
    for m, x in enumerate(mixes):
        for d, _, _, pw in x:
            assert d not in dens_new
            mean_new.setdefault(mean_of(d), len(mean_new))
            cov_new.setdefault(cov_of(d), len(cov_new))
            dens_new[d] = len(dens_new)
            cim.setdefault(cov_of(d), []).append((d, m, pw))

    def dtw(mean):
        return float(num["mean_weights"][mean]) - float(den["mean_weights"][mean])

    def dtsum(mean, k):
        return float(num["mean_sums"][mean, k]) - float(den["mean_sums"][mean, k])
    xi = []
    for x in mixes:
        max_abs, max_nd = 0.0, 0.0
        for d, _, _, _ in x:
            w, dw = dtw(mean_of(d)), float(den["mean_weights"][mean_of(d)])
            if max_abs < abs(w):
                max_abs, max_nd = abs(w), max(w + dw, dw)
        denom = 1 + (max_abs - 1) * max_abs / max_nd if (max_abs < max_nd and max_nd > 0) else 1.0
        xi.append(c["beta"] / denom)
    min_prev = min(f32(prev.variances[cv, k]) for cv in cov_new for k in range(D))
    sigma_min = c["sigma_minimum"] if c["sigma_minimum"] >= 0 else c["sigma_minimum_factor"] * float(min_prev)
    glob, local = {}, {}
    is_global = c["iteration_constants_type"] == "global-rwth"
    assert is_global or c["iteration_constants_type"] == "local-rwth"
    for cv in cov_new:  # ascending estimated index
        numer = [0 - (float(num["covariance_sums"][cv, k]) - float(den["covariance_sums"][cv, k])) for k in range(D)]
        denom = [0.0] * D
        for d, m, pw in cim[cv]:
            mean = mean_of(d)
            w = dtw(mean)
            for k in range(D):
                pm = float(prev.means[mean, k])
                t2 = 2 * dtsum(mean, k) - w * pm
                t3 = dtsum(mean, k) - w * pm
                numer[k] += sigma_min * w
                numer[k] += t2 * pm
                numer[k] += xi[m] * t3 * t3
                denom[k] += (float(prev.variances[cv, k]) - sigma_min) * pw
        with np.errstate(all="ignore"):
            ratios = [float(np.float64(a) / np.float64(b)) for a, b in zip(numer, denom)]
        rmax = ratios[0]
        for r in ratios[1:]:
            if rmax < r:
                rmax = r
        dk_min = rmax if rmax > 0 else 0.0
        ic = 1.0
        for d, m, pw in cim[cv]:
            dk = 1 / xi[m]
            dk -= dtw(mean_of(d))
            if pw > 0:
                dk /= pw
            if is_global:
                inner = dk_min if dk < dk_min else dk
                ic = inner if ic < inner else ic
            else:
                if m not in local:
                    local[m] = c["step_size"] * (dk_min if 1.0 < dk_min else 1.0)
                cand = c["step_size"] * dk
                local[m] = local[m] if cand < local[m] else cand
        glob[cv] = ic * c["step_size"]
    ic_mean = {}
    for cv in cov_new:
        for d, m, pw in cim[cv]:
            ic = (glob[cv] if is_global else local[m]) * pw
            ic = ic if c["minimum_icd"] < ic else c["minimum_icd"]
            ic_mean[mean_of(d)] = ic
    constants = np.array([ic_mean[mean_of(d)] for d in dens_new])
    # mixture weights
    log_w, mix_dens, mix_off = [], [], [0]
    norm = c["normalize_mixture_weights"]
    for x in mixes:
        n = len(x)
        total = 0.0
        for _, wn, _, _ in x:
            total += wn
        if n > 1 and total > EPS64:
            w, kmax = [], 0.0
            for _, _, wd, pw in x:
                if pw > EPS64:
                    kmax = max(kmax, wd / pw)
                    w.append(pw)
                else:
                    w.append(0.0)
            k = [kmax - x[j][2] / w[j] if w[j] > 0 else 0.0 for j in range(n)]
            for _ in range(c["number_of_iterations"]):
                for j in range(n):
                    if w[j] > 0:
                        w[j] = x[j][1] + k[j] * w[j]
                    if w[j] < 0:
                        w[j] = 0.0
                if norm:
                    s = 0.0
                    for v in w:
                        s += v
                    w = [v / s for v in w] if s > TINY64 else [1 / float(n)] * n
        else:
            w = [1 / float(n) if norm else 1.0] * n
        lw = [math.log(v) if v > 0 else LOWEST64 for v in w]
        if norm and lw:
            mx = 0
            for j in range(1, n):
                if lw[mx] < lw[j]:
                    mx = j
            r = 0.0
            for j in range(n):
                if j != mx:
                    r += math.exp(lw[j] - lw[mx])
            ln = math.log1p(r) + lw[mx]
            lw = [v - ln for v in lw]
        log_w += lw
        mix_dens += [dens_new[d] for d, _, _, _ in x]
        mix_off.append(len(mix_dens))
    # means
    new_mean = {}
    for mean in mean_new:
        ic = ic_mean[mean]
        weight = dtw(mean) + ic
        row = []
        for k in range(D):
            pm = f32(prev.means[mean, k])
            row.append(f32((dtsum(mean, k) + ic * float(pm)) / weight) if weight > 0 else pm)
        new_mean[mean] = row
    # covariances
    variances = []
    min_var = f32(c["minimum_variance"])
    for cv in cov_new:
        buf = [float(num["covariance_sums"][cv, k]) - float(den["covariance_sums"][cv, k]) for k in range(D)]
        weight, done = 0.0, set()
        for d, _, _ in cim[cv]:
            mean = mean_of(d)
            if mean in done:
                continue
            done.add(mean)
            ic = ic_mean[mean]
            tmp_w = dtw(mean) + ic
            weight += tmp_w
            for k in range(D):
                pm = f32(prev.means[mean, k])
                previous = float(f32(prev.variances[cv, k]))
                previous += float(f32(pm * pm))
                previous *= ic
                nm = float(new_mean[mean][k])
                buf[k] += previous - tmp_w * nm * nm
        assert weight > 0
        row = [f32(b / weight) for b in buf]
        assert all(v > 0 for v in row)
        variances.append([min_var if (min_var != 0 and v < min_var) else v for v in row])
    model = {"means": np.array([new_mean[m] for m in mean_new], dtype=np.float32).reshape(len(mean_new), D),
             "variances": np.array(variances, dtype=np.float32).reshape(len(cov_new), D),
             "density_mean": np.array([mean_new[mean_of(d)] for d in dens_new], dtype=np.uint32),
             "density_covariance": np.array([cov_new[cov_of(d)] for d in dens_new], dtype=np.uint32),
             "mixture_offsets": np.array(mix_off, dtype=np.uint32),
             "mixture_densities": np.array(mix_dens, dtype=np.uint32),
             "mixture_log_weights": np.array(log_w, dtype=np.float64)}
    return model, constants
