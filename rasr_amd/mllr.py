"""Python handle over the MLLR mean transform statistics of include/rasr_gmm_mllr.h.

`MllrAccumulator` turns aligned (frame, mixture[, density][, weight][, key]) pairs into the f64 tables of
Mm::FullAdaptorViterbiEstimator / Mm::ShiftAdaptorViterbiEstimator on the GPU, one set per (speaker key, regression
leaf); `estimate_mllr` estimates one key's matrices over a binary regression tree on the host, and `adapt_means`
returns a new MixtureSet with the adapted means, ready for `Scorer(...)`.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

from . import _capi, _pairs
from .mixture_set import MixtureSet

MLLR_KINDS = {"full": _capi.GMM_MLLR_FULL, "shift": _capi.GMM_MLLR_SHIFT}
NO_ID = _capi.GMM_MLLR_NO_ID


_ptr = _pairs.ptr


def _kind(kind) -> int:
    if kind not in MLLR_KINDS:
        raise ValueError(f"unknown MLLR kind {kind}")
    return MLLR_KINDS[kind]


def _u32(a, n=None, what="array"):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.ndim != 1 or (n is not None and a.shape[0] != n):
        raise ValueError(f"{what} must be a 1-d array" + ("" if n is None else f" of {n} entries"))
    return a


class MllrAccumulator:
    """gmm_mllr_accumulator: n_keys * n_leaves sets of tables of the kinds in `kinds` ("full", "shift" or both) for the
    mixture set `mixture_set` on one GPU, and the scratch of calls of up to max_pairs pairs.  leaf_of_mixture
    [n_mixtures]: the regression leaf of every mixture (the reference's leafIndex_)."""

    def __init__(self, mixture_set: MixtureSet, leaf_of_mixture, n_leaves: int, n_keys: int, max_pairs: int,
                 kinds=("full",), device: int = 0):
        self._lib = _capi.load_library()
        self.mixture_set = mixture_set
        self.leaf_of_mixture = _u32(leaf_of_mixture, mixture_set.n_mixtures, "leaf_of_mixture")
        self.n_leaves = int(n_leaves)
        self.n_keys = int(n_keys)
        self.max_pairs = int(max_pairs)
        self.kinds = tuple([kinds] if isinstance(kinds, str) else kinds)
        self.device = int(device)
        self._h = None
        mask = 0
        for k in self.kinds:
            mask |= _kind(k)
        desc = mixture_set.desc()
        h = ctypes.c_void_p()
        _capi.check(self._lib.gmm_mllr_create(ctypes.byref(desc), _ptr(self.leaf_of_mixture), self.n_leaves, self.n_keys,
                                              mask, self.max_pairs, self.device, ctypes.byref(h)), "gmm_mllr_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gmm_mllr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def reset(self) -> None:
        """Zeroes every set's tables and the skipped count."""
        _capi.check(self._lib.gmm_mllr_reset(self._h), "gmm_mllr_reset")

    def info(self) -> dict:
        """gmm_mllr_info: table_bytes (the sets' accumulators), scratch_bytes, kinds."""
        t, s, k = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        _capi.check(self._lib.gmm_mllr_info(self._h, ctypes.byref(t), ctypes.byref(s), ctypes.byref(k)), "gmm_mllr_info")
        return {"table_bytes": int(t.value), "scratch_bytes": int(s.value),
                "kinds": tuple(n for n, bit in MLLR_KINDS.items() if k.value & bit)}

    def accumulate_device(self, frames, pair_frame, pair_mixture, pair_density=None, pair_weight=None, pair_key=None,
                          scorer=None, stream=None, n_frames=None) -> None:
        """gmm_mllr_accumulate_device: the arguments of AffineTransformAccumulator.accumulate_device.  frames torch cuda
        f32 [F, >=D]; pair_frame / pair_mixture / pair_density / pair_key int32 or uint32 cuda tensors of n_pairs;
        pair_weight a float64 cuda tensor or None (weight 1); pair_key None: key 0.  Without pair_density the density
        is the scorer's best density of the pair (`scorer`: a Scorer), or, without a scorer, the only density of the
        mixture.  Asynchronous on `stream`."""
        f = int(frames.shape[0] if n_frames is None else n_frames)
        n, s, p = _pairs.device_pairs(
            frames, (("pair_frame", pair_frame), ("pair_mixture", pair_mixture), ("pair_density", pair_density),
                     ("pair_key", pair_key)), (("pair_weight", pair_weight),), stream)
        rc = self._lib.gmm_mllr_accumulate_device(
            self._h, scorer.handle if scorer is not None else None, p[0], f, int(frames.stride(0)), p[1], p[2], p[3], p[5],
            p[4], n, s)
        _capi.check(rc, "gmm_mllr_accumulate_device")

    def accumulate_host(self, frames, pair_frame, pair_mixture, pair_density=None, pair_weight=None, pair_key=None,
                        scorer=None) -> None:
        """gmm_mllr_accumulate_host: the same call on numpy arrays, synchronous."""
        frames, (pf, pm, pd, pk), (pw,), n = _pairs.host_pairs(
            frames, (pair_frame, pair_mixture, pair_density, pair_key), (pair_weight,))
        rc = self._lib.gmm_mllr_accumulate_host(
            self._h, scorer.handle if scorer is not None else None, _ptr(frames), frames.shape[0], frames.shape[1],
            _ptr(pf), _ptr(pm), _ptr(pd), _ptr(pw), _ptr(pk), n)
        _capi.check(rc, "gmm_mllr_accumulate_host")

    @property
    def skipped(self) -> int:
        """Pairs skipped since creation or the last reset (frame, mixture, density or key out of range, no best
        density)."""
        v = ctypes.c_uint64()
        _capi.check(self._lib.gmm_mllr_skipped(self._h, ctypes.byref(v)), "gmm_mllr_skipped")
        return int(v.value)

    def tables(self, key: int = 0, leaf: int = 0) -> dict:
        """gmm_mllr_get: the tables of one (key, leaf) as f64 numpy arrays, of the kinds the handle holds: Z [D, D+1],
        G [D+1, D+1], count_full (a float); count_shift (a float), beta [D], shift [D]."""
        D = self.mixture_set.dimension
        out, cf, cs = {}, ctypes.c_double(), ctypes.c_double()
        full, shift = "full" in self.kinds, "shift" in self.kinds
        if full:
            out.update(Z=np.zeros((D, D + 1)), G=np.zeros((D + 1, D + 1)))
        if shift:
            out.update(beta=np.zeros(D), shift=np.zeros(D))
        _capi.check(self._lib.gmm_mllr_get(self._h, int(key), int(leaf), _ptr(out.get("Z")), _ptr(out.get("G")),
                                           ctypes.byref(cf) if full else None, ctypes.byref(cs) if shift else None,
                                           _ptr(out.get("beta")), _ptr(out.get("shift"))), "gmm_mllr_get")
        if full:
            out["count_full"] = float(cf.value)
        if shift:
            out["count_shift"] = float(cs.value)
        return out

    def leaf_tables(self, key: int = 0) -> list:
        """`tables(key, leaf)` of every leaf: what `estimate_mllr` takes."""
        return [self.tables(key, leaf) for leaf in range(self.n_leaves)]

    def add(self, key: int, leaf: int, tables: dict, weight: float = 1.0) -> None:
        """gmm_mllr_add: the tables of (key, leaf) become dst + src * weight, element by element, the counts dst + src;
        `tables` as `tables()` returns them (of another handle, another rank); a missing entry leaves its table."""
        D = self.mixture_set.dimension
        arr = {}
        for name, shape in (("Z", (D, D + 1)), ("G", (D + 1, D + 1)), ("beta", (D,)), ("shift", (D,))):
            a = tables.get(name)
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != shape:
                    raise ValueError(f"{name} must have the shape {shape}")
            arr[name] = a
        counts = {n: (None if tables.get(n) is None else ctypes.c_double(float(tables[n])))
                  for n in ("count_full", "count_shift")}

        def ref(c):
            return None if c is None else ctypes.cast(ctypes.byref(c), ctypes.c_void_p)
        _capi.check(self._lib.gmm_mllr_add(self._h, int(key), int(leaf), _ptr(arr["Z"]), _ptr(arr["G"]),
                                           ref(counts["count_full"]), ref(counts["count_shift"]), _ptr(arr["beta"]),
                                           _ptr(arr["shift"]), float(weight)), "gmm_mllr_add")


def estimate_mllr(leaf_tables, leaf_of_mixture, tree: dict, silence_mixtures=(), min_observation: float = 1000.0,
                  min_silence_observation: float = 500.0, kind: str = "full") -> dict:
    """gmm_mllr_estimate (host only): one key's matrices over a binary regression tree.

    leaf_tables: `MllrAccumulator.leaf_tables(key)`, one dict per leaf.  tree: {"left", "right", "parent",
    "leaf_number"} arrays over the node ids (NO_ID = 0xffffffff for none) and "root".  silence_mixtures: ascending.
    The defaults of the thresholds are the reference's (min-observation, min-silence-observation).
    Returns {"kind", "ids" [n] ascending, "matrices" [n, D, D+1] (full: column 0 the offset) or [n, D] (shift),
    "matrix_of_mixture" [n_mixtures]}."""
    lib = _capi.load_library()
    k = _kind(kind)
    n_leaves = len(leaf_tables)
    if n_leaves == 0:
        raise ValueError("no leaf tables")
    names = ("Z", "G", "count_full") if kind == "full" else ("beta", "shift", "count_shift")
    stacked = {n: np.ascontiguousarray(np.stack([np.asarray(t[n], np.float64) for t in leaf_tables])) for n in names}
    D = stacked[names[1]].shape[-1] - (1 if kind == "full" else 0)
    want = {"Z": (n_leaves, D, D + 1), "G": (n_leaves, D + 1, D + 1), "beta": (n_leaves, D), "shift": (n_leaves, D),
            "count_full": (n_leaves,), "count_shift": (n_leaves,)}
    for n in names:
        if stacked[n].shape != want[n]:
            raise ValueError(f"{n} must have the shape {want[n][1:]} in every leaf")
    leaf = _u32(leaf_of_mixture, what="leaf_of_mixture")
    left = _u32(tree["left"], what="left")
    n_ids = left.shape[0]
    right, parent, number = (_u32(tree[n], n_ids, n) for n in ("right", "parent", "leaf_number"))
    silence = _u32(silence_mixtures, what="silence_mixtures")
    cap = n_ids + silence.shape[0]
    ids = np.zeros(cap, np.uint32)
    matrices = np.zeros((cap, D, D + 1) if kind == "full" else (cap, D))
    of_mixture = np.zeros(leaf.shape[0], np.uint32)
    n = ctypes.c_uint32()
    _capi.check(lib.gmm_mllr_estimate(
        D, k, n_leaves, _ptr(stacked.get("Z")), _ptr(stacked.get("G")), _ptr(stacked[names[2]]), _ptr(stacked.get("beta")),
        _ptr(stacked.get("shift")), _ptr(leaf), leaf.shape[0], n_ids, _ptr(left), _ptr(right), _ptr(parent), _ptr(number),
        int(tree["root"]), _ptr(silence), silence.shape[0], float(min_observation), float(min_silence_observation),
        ctypes.byref(n), _ptr(ids), _ptr(matrices), _ptr(of_mixture)), "gmm_mllr_estimate")
    return {"kind": kind, "ids": ids[:n.value].copy(), "matrices": matrices[:n.value].copy(),
            "matrix_of_mixture": of_mixture}


def adapt_means(mixture_set: MixtureSet, estimate: dict) -> MixtureSet:
    """gmm_mllr_adapt_means (host only): a NEW MixtureSet whose means are `mixture_set`'s transformed by `estimate`
    (what `estimate_mllr` returns); everything else is shared with `mixture_set`, which is left as it is."""
    lib = _capi.load_library()
    kind = estimate["kind"]
    k = _kind(kind)
    D = mixture_set.dimension
    ids = _u32(estimate["ids"], what="ids")
    matrices = np.ascontiguousarray(estimate["matrices"], dtype=np.float64)
    if matrices.shape != ((ids.shape[0], D, D + 1) if kind == "full" else (ids.shape[0], D)):
        raise ValueError("matrices must be [n, D, D+1] (full) or [n, D] (shift), one per id")
    of_mixture = _u32(estimate["matrix_of_mixture"], mixture_set.n_mixtures, "matrix_of_mixture")
    out = np.zeros_like(mixture_set.means)
    desc = mixture_set.desc()
    _capi.check(lib.gmm_mllr_adapt_means(ctypes.byref(desc), _ptr(matrices), _ptr(ids), ids.shape[0], _ptr(of_mixture), k,
                                         _ptr(out)), "gmm_mllr_adapt_means")
    return dataclasses.replace(mixture_set, means=out, _keep=[])
