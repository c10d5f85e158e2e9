"""Python handle over the affine feature transform (constrained MLLR) statistics of include/rasr_gmm_adaptation.h.

`AffineTransformAccumulator` turns aligned (frame, mixture[, density][, weight][, key]) pairs into the f64 tables of
Mm::AffineFeatureTransformAccumulator on the GPU, one set per speaker key; `estimate_affine_transform` estimates the
transform of one key from its tables on the host (criteria naive and mmiPrime).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi, _pairs
from .mixture_set import MixtureSet

CRITERIA = {"naive": 0, "mmiPrime": 1, "hlda": 2}  # gmm_affine_criterion


_ptr = _pairs.ptr


class AffineTransformAccumulator:
    """gmm_affine_accumulator: n_keys sets of tables (beta, k, G, mean, cov) for the mixture set `mixture_set` on one
    GPU, and the scratch of calls of up to max_pairs pairs.  A mixture set with one covariance is in pooled mode:
    no G table is held, `tables` derives G from cov."""

    def __init__(self, mixture_set: MixtureSet, n_keys: int, max_pairs: int, device: int = 0):
        self._lib = _capi.load_library()
        self.mixture_set = mixture_set
        self.n_keys = int(n_keys)
        self.max_pairs = int(max_pairs)
        self.device = int(device)
        self._h = None
        desc = mixture_set.desc()
        h = ctypes.c_void_p()
        _capi.check(self._lib.gmm_affine_create(ctypes.byref(desc), self.n_keys, self.max_pairs, self.device,
                                                ctypes.byref(h)), "gmm_affine_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gmm_affine_destroy(self._h)
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
        """Zeroes every key's tables and the skipped count."""
        _capi.check(self._lib.gmm_affine_reset(self._h), "gmm_affine_reset")

    def info(self) -> dict:
        """gmm_affine_info: table_bytes (the keys' accumulators), scratch_bytes, pooled."""
        t, s, p = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
        _capi.check(self._lib.gmm_affine_info(self._h, ctypes.byref(t), ctypes.byref(s), ctypes.byref(p)), "gmm_affine_info")
        return {"table_bytes": int(t.value), "scratch_bytes": int(s.value), "pooled": bool(p.value)}

    def accumulate_device(self, frames, pair_frame, pair_mixture, pair_density=None, pair_weight=None, pair_key=None,
                          scorer=None, stream=None, n_frames=None) -> None:
        """gmm_affine_accumulate_device: frames torch cuda f32 [F, >=D]; pair_frame / pair_mixture / pair_density /
        pair_key int32 or uint32 cuda tensors of n_pairs; pair_weight a float64 cuda tensor or None (weight 1);
        pair_key None: key 0.  Without pair_density the density is the scorer's best density of the pair (`scorer`: a
        Scorer), or, without a scorer, the only density of the mixture.  Asynchronous on `stream`."""
        f = int(frames.shape[0] if n_frames is None else n_frames)
        n, s, p = _pairs.device_pairs(
            frames, (("pair_frame", pair_frame), ("pair_mixture", pair_mixture), ("pair_density", pair_density),
                     ("pair_key", pair_key)), (("pair_weight", pair_weight),), stream)
        rc = self._lib.gmm_affine_accumulate_device(
            self._h, scorer.handle if scorer is not None else None, p[0], f, int(frames.stride(0)), p[1], p[2], p[3], p[5],
            p[4], n, s)
        _capi.check(rc, "gmm_affine_accumulate_device")

    def accumulate(self, frames, pair_frame, pair_mixture, pair_density=None, pair_weight=None, pair_key=None,
                   scorer=None) -> None:
        """gmm_affine_accumulate_host: the same call on numpy arrays, synchronous."""
        frames, (pf, pm, pd, pk), (pw,), n = _pairs.host_pairs(
            frames, (pair_frame, pair_mixture, pair_density, pair_key), (pair_weight,))
        rc = self._lib.gmm_affine_accumulate_host(
            self._h, scorer.handle if scorer is not None else None, _ptr(frames), frames.shape[0], frames.shape[1],
            _ptr(pf), _ptr(pm), _ptr(pd), _ptr(pw), _ptr(pk), n)
        _capi.check(rc, "gmm_affine_accumulate_host")

    @property
    def skipped(self) -> int:
        """Pairs skipped since creation or the last reset (frame, mixture, density or key out of range, no best
        density)."""
        v = ctypes.c_uint64()
        _capi.check(self._lib.gmm_affine_skipped(self._h, ctypes.byref(v)), "gmm_affine_skipped")
        return int(v.value)

    def tables(self, key: int = 0) -> dict:
        """gmm_affine_get: one key's finalized tables as f64 numpy arrays: beta (a float), k [D, D+1], G [D, D+1, D+1]
        and cov [D+1, D+1] symmetric, mean [D+1]."""
        D = self.mixture_set.dimension
        beta = ctypes.c_double()
        out = {"k": np.zeros((D, D + 1)), "G": np.zeros((D, D + 1, D + 1)), "mean": np.zeros(D + 1),
               "cov": np.zeros((D + 1, D + 1))}
        _capi.check(self._lib.gmm_affine_get(self._h, int(key), ctypes.byref(beta), _ptr(out["k"]), _ptr(out["G"]),
                                             _ptr(out["mean"]), _ptr(out["cov"])), "gmm_affine_get")
        out["beta"] = float(beta.value)
        return out

    def add(self, key: int, tables: dict, weight: float = 1.0) -> None:
        """gmm_affine_add (combine): the key's tables become dst + src * weight, element by element; `tables` as
        `tables()` returns them (of another handle, another rank).  G is added only outside pooled mode."""
        D = self.mixture_set.dimension
        beta = ctypes.c_double(float(tables["beta"]))
        arr = {}
        for name, shape in (("k", (D, D + 1)), ("G", (D, D + 1, D + 1)), ("mean", (D + 1,)), ("cov", (D + 1, D + 1))):
            a = tables.get(name)
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != shape:
                    raise ValueError(f"{name} must have the shape {shape}")
            arr[name] = a
        _capi.check(self._lib.gmm_affine_add(self._h, int(key), ctypes.byref(beta), _ptr(arr["k"]), _ptr(arr["G"]),
                                             _ptr(arr["mean"]), _ptr(arr["cov"]), float(weight)), "gmm_affine_add")


def estimate_affine_transform(tables: dict, criterion: str = "mmiPrime", iterations: int = 1,
                              min_observation_weight: float = 0.0, initial_transform=None) -> np.ndarray:
    """gmm_affine_estimate (host only): the [D, D+1] f32 transform, column 0 the offset, from one key's finalized
    tables (`AffineTransformAccumulator.tables`).  criterion: "naive" or "mmiPrime" ("hlda" is refused);
    initial_transform [D, D] or [D, D+1], None: the identity."""
    lib = _capi.load_library()
    if criterion not in CRITERIA:
        raise ValueError(f"unknown criterion {criterion}")
    k = np.ascontiguousarray(tables["k"], dtype=np.float64)
    D = k.shape[0]
    G = np.ascontiguousarray(tables["G"], dtype=np.float64)
    if k.shape != (D, D + 1) or G.shape != (D, D + 1, D + 1):
        raise ValueError("k must be [D, D+1] and G [D, D+1, D+1]")
    mean = None if tables.get("mean") is None else np.ascontiguousarray(tables["mean"], dtype=np.float64)
    cov = None if tables.get("cov") is None else np.ascontiguousarray(tables["cov"], dtype=np.float64)
    init, cols = None, 0
    if initial_transform is not None:
        init = np.ascontiguousarray(initial_transform, dtype=np.float64)
        if init.ndim != 2 or init.shape[0] != D:
            raise ValueError("initial_transform must be [D, D] or [D, D+1]")
        cols = init.shape[1]
    out = np.zeros((D, D + 1), np.float32)
    _capi.check(lib.gmm_affine_estimate(D, float(tables["beta"]), _ptr(k), _ptr(G), _ptr(mean), _ptr(cov),
                                        CRITERIA[criterion], int(iterations), float(min_observation_weight), _ptr(init),
                                        cols, _ptr(out)), "gmm_affine_estimate")
    return out
