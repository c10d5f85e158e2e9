"""The numeric contract of include/rasr_gmm_mllr.h restated in numpy f64 (helper of the MLLR tests).

Accumulation: a loop over the pairs of one (key, leaf) set in pair order; per pair every cell of every table gets one
term, formed with one IEEE f64 rounding per operation in the reference's operand order (numpy's elementwise f64
operations round once and fuse nothing):
    Z[i][j] += (w * x_i) * m_j;  G[i][j] += (w * m_i) * m_j  (all cells);  count_full += 1.0;
    count_shift += w;  beta[d] += w / v_d;  shift[d] += (w * (f64)(x_d -f32 mu_d)) / v_d
with m = (1, mu) and the piece rule (more than CHUNK pairs of one set in a call: pieces of CHUNK, piece 0 onto the
current value, later pieces from 0 and then added in piece order); `add` (operator+=, scaled), `propagate`, `estimate`
(estimateWMatrices and adaptor(), with np.linalg.pinv(G, rcond=1e-12)) and `adapt_means` (adaptMixtureSet).
"""
import numpy as np

CHUNK = 512
NO_ID = 0xFFFFFFFF
NAMES = ("Z", "G", "count_full", "count_shift", "beta", "shift")
KIND_NAMES = {"full": ("Z", "G", "count_full"), "shift": ("count_shift", "beta", "shift")}


def zero_tables(D):
    return {"Z": np.zeros((D, D + 1)), "G": np.zeros((D + 1, D + 1)), "count_full": np.float64(0.0),
            "count_shift": np.float64(0.0), "beta": np.zeros(D), "shift": np.zeros(D)}


def copy_tables(t):
    return {n: np.array(t[n], np.float64).copy() if np.ndim(t[n]) else np.float64(t[n]) for n in NAMES}


def resolve(ms, n_frames, n_keys, pf, pm, pd, pk):
    """Per pair its mixture entry, or -1 (skipped): frame, mixture, density or key out of range."""
    off = ms.mixture_offsets.astype(np.int64)
    entry = np.full(len(pf), -1, np.int64)
    for i in range(len(pf)):
        f, m, d, k = int(pf[i]), int(pm[i]), int(pd[i]), int(pk[i])
        if f < n_frames and m < ms.n_mixtures and k < n_keys and d < off[m + 1] - off[m]:
            entry[i] = off[m] + d
    return entry


def _add_pairs(t, xs, mus, vs, ws):
    """The pairs of one piece onto the tables t, in order."""
    cf, cs = t["count_full"], t["count_shift"]
    Z, G, beta, shift = t["Z"], t["G"], t["beta"], t["shift"]
    for x32, mu32, v32, w in zip(xs, mus, vs, ws):
        w = np.float64(w)
        x, v = x32.astype(np.float64), v32.astype(np.float64)
        m = np.concatenate([[1.0], mu32.astype(np.float64)])
        Z += (w * x)[:, None] * m[None, :]
        G += (w * m)[:, None] * m[None, :]
        cf = cf + np.float64(1.0)
        cs = cs + w
        beta += w / v
        shift += (w * (x32 - mu32).astype(np.float64)) / v  # the difference in f32, widened afterwards
    t["count_full"], t["count_shift"] = cf, cs


def accumulate(ms, leaf_of_mixture, n_leaves, frames, pf, pm, pd, pw=None, pk=None, n_keys=1, tables=None, chunk=CHUNK):
    """(tables[key][leaf], skipped) after one call on `tables` (zeros if None); chunk=None: purely sequential."""
    D = ms.dimension
    n = len(pf)
    pf, pm = np.asarray(pf), np.asarray(pm)
    pk = np.zeros(n, np.uint32) if pk is None else np.asarray(pk)
    pw = np.ones(n) if pw is None else np.asarray(pw, np.float64)
    leaf_of_mixture = np.asarray(leaf_of_mixture, np.int64)
    out = ([[copy_tables(t) for t in row] for row in tables] if tables is not None
           else [[zero_tables(D) for _ in range(n_leaves)] for _ in range(n_keys)])
    entry = resolve(ms, frames.shape[0], n_keys, pf, pm, pd, pk)
    ok = entry >= 0
    leaf = np.full(n, -1, np.int64)
    leaf[ok] = leaf_of_mixture[pm[ok].astype(np.int64)]
    for key in range(n_keys):
        for lf in range(n_leaves):
            idx = np.nonzero(ok & (pk == key) & (leaf == lf))[0]
            if len(idx) == 0:
                continue
            dens = ms.mixture_densities[entry[idx]]
            xs = np.ascontiguousarray(frames[pf[idx].astype(np.int64)][:, :D], np.float32)
            mus = ms.means[ms.density_mean[dens]]
            vs = ms.variances[ms.density_covariance[dens]]
            ws = pw[idx]
            c = chunk or len(idx)
            parts = []
            for q, s in enumerate(range(0, len(idx), c)):
                t = out[key][lf] if q == 0 else zero_tables(D)
                _add_pairs(t, xs[s:s + c], mus[s:s + c], vs[s:s + c], ws[s:s + c])
                parts.append(t)
            t = parts[0]
            for part in parts[1:]:
                for name in NAMES:
                    t[name] = t[name] + part[name]
    return out, int((~ok).sum())


def add(dst, src, weight):
    """gmm_mllr_add: tables dst + src * weight, one multiply and one add each; the counts dst + src."""
    w = np.float64(weight)
    out = copy_tables(dst)
    for name in ("Z", "G", "beta", "shift"):
        out[name] = out[name] + np.asarray(src[name], np.float64) * w
    for name in ("count_full", "count_shift"):
        out[name] = out[name] + np.float64(src[name])
    return out


def propagate(leaf_tables, tree, names):
    """node tables {id: {name: value}}: a leaf id its leaf's tables, a node left + right (elementwise), from the root."""
    node = {}

    def walk(i):
        if tree["left"][i] == NO_ID:
            node[i] = {n: np.array(leaf_tables[tree["leaf_number"][i]][n], np.float64) for n in names}
            return
        walk(int(tree["left"][i]))
        walk(int(tree["right"][i]))
        a, b = node[int(tree["left"][i])], node[int(tree["right"][i])]
        node[i] = {n: a[n] + b[n] for n in names}
    walk(int(tree["root"]))
    return node


def unit_matrix(D, kind):
    return np.concatenate([np.zeros((D, 1)), np.eye(D)], axis=1) if kind == "full" else np.zeros(D)


def matrix_of(t, kind):
    if kind == "full":
        return np.asarray(t["Z"], np.float64) @ np.linalg.pinv(np.asarray(t["G"], np.float64), rcond=1e-12)
    return np.asarray(t["shift"], np.float64) / np.asarray(t["beta"], np.float64)


def estimate(leaf_tables, leaf_of_mixture, tree, silence_mixtures=(), min_observation=1000.0,
             min_silence_observation=500.0, kind="full"):
    """{"ids", "matrices", "matrix_of_mixture"}: estimateWMatrices and adaptor() for one key."""
    names = KIND_NAMES[kind]
    count = "count_full" if kind == "full" else "count_shift"
    D = len(leaf_tables[0]["beta"]) if kind == "shift" else leaf_tables[0]["Z"].shape[0]
    node = propagate(leaf_tables, tree, names)
    root = int(tree["root"])
    matrices, matrix_id = {}, {}
    leaves = sorted(i for i in node if tree["left"][i] == NO_ID)
    if not node[root][count] > min_observation:
        matrices[root] = unit_matrix(D, kind)
        for i in leaves:
            matrix_id[int(tree["leaf_number"][i])] = root
    else:
        for leaf_id in leaves:
            i = leaf_id
            while i != root and not node[i][count] > min_observation:
                i = int(tree["parent"][i])
            if i not in matrices:
                matrices[i] = matrix_of(node[i], kind)
            matrix_id[int(tree["leaf_number"][leaf_id])] = i
    silence_id = len(tree["left"])
    for m in sorted(int(s) for s in silence_mixtures):
        leaf = int(leaf_of_mixture[m])
        t = leaf_tables[leaf]
        matrices[silence_id] = matrix_of(t, kind) if t[count] > min_silence_observation else unit_matrix(D, kind)
        matrix_id[leaf] = silence_id
        silence_id += 1
    ids = sorted(matrices)
    return {"kind": kind, "ids": np.array(ids, np.uint32), "matrices": np.stack([matrices[i] for i in ids]),
            "matrix_of_mixture": np.array([matrix_id[int(l)] for l in leaf_of_mixture], np.uint32)}


def adapt_means(ms, est):
    """The adapted means [n_means, D] f32: per (mixture, density) entry (f32) sum_j W[i][j] * m_j, f64 products added
    in ascending j from 0.0 (full), (f32)(shift[i] + (f64) mu_i) (shift); a mean no entry names is copied."""
    D = ms.dimension
    out = ms.means.copy()
    ids = [int(i) for i in est["ids"]]
    off = ms.mixture_offsets.astype(np.int64)
    for mix in range(ms.n_mixtures):
        if off[mix] == off[mix + 1]:
            continue
        W = np.asarray(est["matrices"][ids.index(int(est["matrix_of_mixture"][mix]))], np.float64)
        for e in range(off[mix], off[mix + 1]):
            mean = int(ms.density_mean[ms.mixture_densities[e]])
            mu = ms.means[mean].astype(np.float64)
            if est["kind"] == "shift":
                out[mean] = (W + mu).astype(np.float32)
                continue
            m = np.concatenate([[1.0], mu])
            s = np.zeros(D)
            for j in range(D + 1):
                s = s + W[:, j] * m[j]
            out[mean] = s.astype(np.float32)
    return out
