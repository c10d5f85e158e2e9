"""The numeric contract of include/rasr_gmm_adaptation.h restated in numpy f64 (helper of the affine tests).

Accumulation: a loop over a key's pairs in pair order; per pair every cell of every table gets one term, formed with
one IEEE f64 rounding per operation in the reference's operand order (numpy's elementwise f64 operations round once
and fuse nothing):
    beta += w;  k[i][j] += ((mu[i] / v[i]) * xi[j]) * w;  G[i][j][k] += ((xi[j] * xi[k]) / v[i]) * w  (j <= k);
    mean[j] += xi[j] * w;  cov[j][k] += (xi[j] * xi[k]) * w  (j <= k)
with the piece rule (more than CHUNK pairs of one key in a call: pieces of CHUNK, piece 0 onto the current value, later
pieces from 0 and then added in piece order), `finalize` (AffineFeatureTransformAccumulator.cc:123-143), `combine`
(cc:345-365) and `estimate` (cc:177-311, naive and mmiPrime, np.linalg.inv for the inverses).
Raw tables hold the upper triangles of G and cov as flat arrays (rows first); `finalize` returns full matrices.
"""
import numpy as np

CHUNK = 512


def triangle(D):
    """(J, K): the cells (j, k), j <= k, of a (D+1) x (D+1) upper triangle, rows first."""
    return np.triu_indices(D + 1)


def zero_tables(D, pooled):
    T = (D + 1) * (D + 2) // 2
    return {"beta": np.float64(0.0), "k": np.zeros((D, D + 1)), "G": None if pooled else np.zeros((D, T)),
            "mean": np.zeros(D + 1), "cov": np.zeros(T)}


def copy_tables(t):
    return {n: (None if v is None else np.array(v, np.float64).copy() if n != "beta" else np.float64(v)) for n, v in t.items()}


def resolve(ms, n_frames, n_keys, pf, pm, pd, pk):
    """Per pair its mixture entry, or -1 (skipped): frame, mixture, density or key out of range."""
    off = ms.mixture_offsets.astype(np.int64)
    entry = np.full(len(pf), -1, np.int64)
    for i in range(len(pf)):
        f, m, d, k = int(pf[i]), int(pm[i]), int(pd[i]), int(pk[i])
        if f < n_frames and m < ms.n_mixtures and k < n_keys and d < off[m + 1] - off[m]:
            entry[i] = off[m] + d
    return entry


def _add_pairs(t, D, J, K, xs, mus, vs, ws):
    """The pairs of one piece onto the raw tables t, in order."""
    beta, k, G, mean, cov = t["beta"], t["k"], t["G"], t["mean"], t["cov"]
    for x, mu, v, w in zip(xs, mus, vs, ws):
        w = np.float64(w)
        xi = np.concatenate([[1.0], x.astype(np.float64)])
        mu = mu.astype(np.float64)
        v = v.astype(np.float64)
        beta = beta + w
        k += ((mu / v)[:, None] * xi[None, :]) * w
        p = xi[J] * xi[K]
        if G is not None:
            G += (p[None, :] / v[:, None]) * w
        mean += xi * w
        cov += p * w
    t["beta"] = beta


def accumulate(ms, frames, pf, pm, pd, pw=None, pk=None, n_keys=1, tables=None, chunk=CHUNK):
    """(raw tables per key, skipped) after one call on `tables` (zeros if None); chunk=None: purely sequential."""
    D = ms.dimension
    pooled = ms.n_covariances == 1
    J, K = triangle(D)
    n = len(pf)
    pk = np.zeros(n, np.uint32) if pk is None else np.asarray(pk)
    pw = np.ones(n) if pw is None else np.asarray(pw, np.float64)
    out = [copy_tables(t) for t in tables] if tables is not None else [zero_tables(D, pooled) for _ in range(n_keys)]
    entry = resolve(ms, frames.shape[0], n_keys, pf, pm, pd, pk)
    ok = entry >= 0
    for key in range(n_keys):
        idx = np.nonzero(ok & (pk == key))[0]
        if len(idx) == 0:
            continue
        dens = ms.mixture_densities[entry[idx]]
        xs = frames[np.asarray(pf)[idx].astype(np.int64)][:, :D]
        mus = ms.means[ms.density_mean[dens]]
        vs = ms.variances[ms.density_covariance[dens]]
        ws = pw[idx]
        c = chunk or len(idx)
        parts = []
        for q, s in enumerate(range(0, len(idx), c)):
            t = out[key] if q == 0 else zero_tables(D, pooled)
            _add_pairs(t, D, J, K, xs[s:s + c], mus[s:s + c], vs[s:s + c], ws[s:s + c])
            parts.append(t)
        t = parts[0]
        for part in parts[1:]:
            t["beta"] = t["beta"] + part["beta"]
            for name in ("k", "G", "mean", "cov"):
                if t[name] is not None:
                    t[name] += part[name]
    return out, int((~ok).sum())


def _full(tri, D):
    J, K = triangle(D)
    m = np.zeros(tri.shape[:-1] + (D + 1, D + 1))
    m[..., J, K] = tri
    m[..., K, J] = tri
    return m


def finalize(t, ms):
    """One key's raw tables -> what gmm_affine_get returns: G and cov full symmetric; pooled: G[i] = cov / v[i]."""
    D = ms.dimension
    g = t["G"]
    if g is None:
        g = t["cov"][None, :] / ms.variances[0].astype(np.float64)[:, None]
    return {"beta": float(t["beta"]), "k": t["k"].copy(), "G": _full(g, D), "mean": t["mean"].copy(),
            "cov": _full(t["cov"], D)}


def combine(dst, src, weight, D):
    """combine: raw tables dst += finalized (or raw-equivalent) tables src * weight, one multiply and one add each."""
    J, K = triangle(D)
    w = np.float64(weight)
    out = copy_tables(dst)
    out["beta"] = out["beta"] + np.float64(src["beta"]) * w
    out["k"] = out["k"] + src["k"] * w
    out["mean"] = out["mean"] + src["mean"] * w
    out["cov"] = out["cov"] + src["cov"][J, K] * w
    if out["G"] is not None:
        out["G"] = out["G"] + src["G"][:, J, K] * w
    return out


def estimate(tables, criterion="mmiPrime", iterations=1, min_observation_weight=0.0, initial=None, half=0):
    """estimate (cc:177-311) in f64: the [D, D+1] transform.  half: the factor the reference writes as `1 / 2`, an
    integer division, 0; half=0.5 is what the text seems to mean and is only used to show the difference."""
    k, G, beta = np.asarray(tables["k"], np.float64), np.asarray(tables["G"], np.float64), float(tables["beta"])
    D = k.shape[0]
    if initial is None:
        W = np.concatenate([np.zeros((D, 1)), np.eye(D)], axis=1)
    else:
        W = np.array(initial, np.float64)
        if W.shape[1] == D:
            W = np.concatenate([np.zeros((D, 1)), W], axis=1)
    assert W.shape == (D, D + 1)
    if criterion != "naive" and beta < min_observation_weight:
        return W
    g_inv = np.stack([np.linalg.inv(G[i]) for i in range(D)])
    if criterion == "naive":
        return np.stack([g_inv[i] @ k[i] for i in range(D)])
    assert criterion == "mmiPrime"
    for _ in range(iterations):
        for row in range(D):
            cof = np.concatenate([[0.0], np.linalg.inv(W[:, 1:])[:, row]])
            e1 = cof @ g_inv[row] @ cof
            e2 = cof @ g_inv[row] @ k[row]
            root = np.sqrt(e2 * e2 + 4 * e1 * beta)
            a1 = (-e2 + root) / (2 * e1)
            a2 = (-e2 - root) / (2 * e1)
            l1 = beta * np.log(abs(a1 * e1 + e2)) - half * a1 * a1 * e1
            l2 = beta * np.log(abs(a2 * e1 + e2)) - half * a2 * a2 * e1
            alpha = a1 if l1 > l2 else a2
            W[row] = g_inv[row] @ (cof * alpha + k[row])
    return W


def ulp32(x):
    """The spacing of f32 at |x|."""
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)
