"""Python handle over the maximum-likelihood accumulation of include/rasr_gmm_estimator.h.

`Estimator` turns aligned (frame, mixture) pairs into the f64 statistics of a mixture set on the GPU
(AbstractMixtureSetEstimator::accumulate in Viterbi mode, or in Baum-Welch mode with the density posteriors of a
diagonal-sum scorer), writes them as a RASR estimator file and estimates
the next mixture set; `combine_estimators` adds several such files (the trainer's combine action, host only).

For discriminative (EBW) training the same handle accumulates a pair's numerator and denominator weight in ONE call
(`accumulate_discriminative_*`), keeps the objective function, and writes and combines the discriminative
estimator's files (`to_bytes_discriminative`, `combine_discriminative_estimators`).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _capi, _pairs
from .mixture_set import MixtureSet, _from_desc, estimator_config


_ptr = _pairs.ptr


class Estimator:
    """gmm_estimator: one accumulator per mean, covariance and mixture entry of `topology` (a MixtureSet, of which
    only the dimension and the index tables are used) on one GPU, and the scratch of calls of up to max_pairs."""

    def __init__(self, topology: MixtureSet, max_pairs: int, device: int = 0):
        self._lib = _capi.load_library()
        self.topology = topology
        self.max_pairs = int(max_pairs)
        self.device = int(device)
        self._h = None
        desc = topology.desc()
        h = ctypes.c_void_p()
        _capi.check(self._lib.gmm_estimator_create(ctypes.byref(desc), self.max_pairs, self.device, ctypes.byref(h)),
                    "gmm_estimator_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gmm_estimator_destroy(self._h)
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
        """Zeroes the tables and the skipped count."""
        _capi.check(self._lib.gmm_estimator_reset(self._h), "gmm_estimator_reset")

    def accumulate_device(self, frames, pair_frame, pair_mixture, pair_density=None, pair_weight=None, scorer=None,
                          stream=None, n_frames=None) -> None:
        """gmm_estimator_accumulate_device: frames torch cuda f32 [F, >=D]; pair_frame / pair_mixture / pair_density
        int32 or uint32 cuda tensors of n_pairs; pair_weight a float64 cuda tensor or None (weight 1).  Without
        pair_density the density is the scorer's best density of the pair (`scorer`: a Scorer), or, without a scorer,
        the only density of the mixture.  Asynchronous on `stream` (torch stream or raw handle)."""
        f = int(frames.shape[0] if n_frames is None else n_frames)
        n, s, p = _pairs.device_pairs(
            frames, (("pair_frame", pair_frame), ("pair_mixture", pair_mixture), ("pair_density", pair_density)),
            (("pair_weight", pair_weight),), stream)
        rc = self._lib.gmm_estimator_accumulate_device(
            self._h, scorer.handle if scorer is not None else None, p[0], f, int(frames.stride(0)), *p[1:], n, s)
        _capi.check(rc, "gmm_estimator_accumulate_device")

    def accumulate_host(self, frames, pair_frame, pair_mixture, pair_density=None, pair_weight=None, scorer=None) -> None:
        """gmm_estimator_accumulate_host: the same call on numpy arrays, synchronous."""
        frames, lists, weights, n = _pairs.host_pairs(frames, (pair_frame, pair_mixture, pair_density), (pair_weight,))
        rc = self._lib.gmm_estimator_accumulate_host(
            self._h, scorer.handle if scorer is not None else None, _ptr(frames), frames.shape[0], frames.shape[1],
            *map(_ptr, lists + weights), n)
        _capi.check(rc, "gmm_estimator_accumulate_host")

    def accumulate_posteriors_device(self, frames, pair_frame, pair_mixture, pair_weight=None, scorer=None,
                                     weight_threshold=None, stream=None, n_frames=None) -> None:
        """gmm_estimator_accumulate_posteriors_device (Baum-Welch mode): every pair is spread over all densities of
        its mixture by the posteriors of `scorer` (a diagonal-sum Scorer; without one every mixture holds one density
        of posterior 1); a contribution counts iff pair_weight * posterior > weight_threshold (None: the default,
        DEFAULT_WEIGHT_THRESHOLD).  Tensors as accumulate_device; needs n_pairs * (largest mixture) <= max_pairs."""
        f = int(frames.shape[0] if n_frames is None else n_frames)
        n, s, p = _pairs.device_pairs(frames, (("pair_frame", pair_frame), ("pair_mixture", pair_mixture)),
                                      (("pair_weight", pair_weight),), stream)
        thr = _capi.DEFAULT_WEIGHT_THRESHOLD if weight_threshold is None else float(weight_threshold)
        rc = self._lib.gmm_estimator_accumulate_posteriors_device(
            self._h, scorer.handle if scorer is not None else None, p[0], f, int(frames.stride(0)), *p[1:], n, thr, s)
        _capi.check(rc, "gmm_estimator_accumulate_posteriors_device")

    def accumulate_posteriors_host(self, frames, pair_frame, pair_mixture, pair_weight=None, scorer=None,
                                   weight_threshold=None) -> None:
        """gmm_estimator_accumulate_posteriors_host: the same call on numpy arrays, synchronous."""
        frames, lists, weights, n = _pairs.host_pairs(frames, (pair_frame, pair_mixture), (pair_weight,))
        thr = _capi.DEFAULT_WEIGHT_THRESHOLD if weight_threshold is None else float(weight_threshold)
        rc = self._lib.gmm_estimator_accumulate_posteriors_host(
            self._h, scorer.handle if scorer is not None else None, _ptr(frames), frames.shape[0], frames.shape[1],
            *map(_ptr, lists + weights), n, thr)
        _capi.check(rc, "gmm_estimator_accumulate_posteriors_host")

    # ---- discriminative training: numerator and denominator weights in one call ----

    def accumulate_discriminative_device(self, frames, pair_frame, pair_mixture, pair_density=None, pair_weight_num=None,
                                         pair_weight_den=None, scorer=None, stream=None, n_frames=None) -> None:
        """gmm_estimator_accumulate_discriminative_device (Viterbi mode): accumulate_device with a numerator and a
        denominator weight per pair (float64 cuda tensors).  A side given as None receives nothing (both None is an
        error); a NaN weight marks the pair as absent on that side."""
        f = int(frames.shape[0] if n_frames is None else n_frames)
        n, s, p = _pairs.device_pairs(
            frames, (("pair_frame", pair_frame), ("pair_mixture", pair_mixture), ("pair_density", pair_density)),
            (("pair_weight_num", pair_weight_num), ("pair_weight_den", pair_weight_den)), stream)
        rc = self._lib.gmm_estimator_accumulate_discriminative_device(
            self._h, scorer.handle if scorer is not None else None, p[0], f, int(frames.stride(0)), *p[1:], n, s)
        _capi.check(rc, "gmm_estimator_accumulate_discriminative_device")

    def accumulate_discriminative_host(self, frames, pair_frame, pair_mixture, pair_density=None, pair_weight_num=None,
                                       pair_weight_den=None, scorer=None) -> None:
        """gmm_estimator_accumulate_discriminative_host: the same call on numpy arrays, synchronous."""
        frames, lists, weights, n = _pairs.host_pairs(frames, (pair_frame, pair_mixture, pair_density),
                                                      (pair_weight_num, pair_weight_den))
        rc = self._lib.gmm_estimator_accumulate_discriminative_host(
            self._h, scorer.handle if scorer is not None else None, _ptr(frames), frames.shape[0], frames.shape[1],
            *map(_ptr, lists + weights), n)
        _capi.check(rc, "gmm_estimator_accumulate_discriminative_host")

    def accumulate_discriminative_posteriors_device(self, frames, pair_frame, pair_mixture, pair_weight_num=None,
                                                    pair_weight_den=None, scorer=None, weight_threshold=None,
                                                    stream=None, n_frames=None) -> None:
        """gmm_estimator_accumulate_discriminative_posteriors_device (Baum-Welch mode): the density posteriors of
        `scorer` are computed once per pair; a contribution is live on a side iff that side's pair weight * posterior
        > weight_threshold.  Tensors as accumulate_discriminative_device."""
        f = int(frames.shape[0] if n_frames is None else n_frames)
        n, s, p = _pairs.device_pairs(
            frames, (("pair_frame", pair_frame), ("pair_mixture", pair_mixture)),
            (("pair_weight_num", pair_weight_num), ("pair_weight_den", pair_weight_den)), stream)
        thr = _capi.DEFAULT_WEIGHT_THRESHOLD if weight_threshold is None else float(weight_threshold)
        rc = self._lib.gmm_estimator_accumulate_discriminative_posteriors_device(
            self._h, scorer.handle if scorer is not None else None, p[0], f, int(frames.stride(0)), *p[1:], n, thr, s)
        _capi.check(rc, "gmm_estimator_accumulate_discriminative_posteriors_device")

    def accumulate_discriminative_posteriors_host(self, frames, pair_frame, pair_mixture, pair_weight_num=None,
                                                  pair_weight_den=None, scorer=None, weight_threshold=None) -> None:
        """gmm_estimator_accumulate_discriminative_posteriors_host: the same call on numpy arrays, synchronous."""
        frames, lists, weights, n = _pairs.host_pairs(frames, (pair_frame, pair_mixture), (pair_weight_num, pair_weight_den))
        thr = _capi.DEFAULT_WEIGHT_THRESHOLD if weight_threshold is None else float(weight_threshold)
        rc = self._lib.gmm_estimator_accumulate_discriminative_posteriors_host(
            self._h, scorer.handle if scorer is not None else None, _ptr(frames), frames.shape[0], frames.shape[1],
            *map(_ptr, lists + weights), n, thr)
        _capi.check(rc, "gmm_estimator_accumulate_discriminative_posteriors_host")

    def accumulate_objective(self, f: float) -> None:
        """gmm_estimator_accumulate_objective: objective function += f (host)."""
        _capi.check(self._lib.gmm_estimator_accumulate_objective(self._h, float(f)), "gmm_estimator_accumulate_objective")

    @property
    def objective(self) -> float:
        v = ctypes.c_double()
        _capi.check(self._lib.gmm_estimator_objective(self._h, ctypes.byref(v)), "gmm_estimator_objective")
        return float(v.value)

    def get_denominator(self) -> dict:
        """The denominator tables, keys and shapes as get() (zeros before the first discriminative call)."""
        t = self.topology
        D = t.dimension
        out = {"mean_sums": np.zeros((t.means.shape[0], D), np.float64),
               "mean_weights": np.zeros(t.means.shape[0], np.float64),
               "covariance_sums": np.zeros((t.n_covariances, D), np.float64),
               "covariance_weights": np.zeros(t.n_covariances, np.float64),
               "entry_weights": np.zeros(t.n_entries, np.float64)}
        _capi.check(self._lib.gmm_estimator_get_denominator(
            self._h, _ptr(out["mean_sums"]), _ptr(out["mean_weights"]), _ptr(out["covariance_sums"]),
            _ptr(out["covariance_weights"]), _ptr(out["entry_weights"])), "gmm_estimator_get_denominator")
        return out

    def to_bytes_discriminative(self) -> bytes:
        """gmm_estimator_serialize_discriminative: the file the discriminative (EBW) estimator's write produces."""
        size = ctypes.c_uint64()
        _capi.check(self._lib.gmm_estimator_serialize_discriminative(self._h, None, 0, ctypes.byref(size)),
                    "gmm_estimator_serialize_discriminative")
        buf = ctypes.create_string_buffer(max(int(size.value), 1))
        _capi.check(self._lib.gmm_estimator_serialize_discriminative(self._h, buf, size.value, ctypes.byref(size)),
                    "gmm_estimator_serialize_discriminative")
        return buf.raw[:size.value]

    def write_discriminative(self, path) -> None:
        _capi.check(self._lib.gmm_estimator_write_discriminative(self._h, os.fsencode(path)),
                    "gmm_estimator_write_discriminative")

    def estimate_ebw(self, previous: MixtureSet, **config) -> MixtureSet:
        """gmm_estimator_estimate_ebw_handle: the EBW estimate from the numerator and denominator tables and the
        previous mixture set (keywords: ebw_config)."""
        d = _capi.MixtureSetDesc()
        cfg = ebw_config(**config)
        prev = previous.desc()
        _capi.check(self._lib.gmm_estimator_estimate_ebw_handle(self._h, ctypes.byref(prev), ctypes.byref(cfg),
                                                                ctypes.byref(d)), "gmm_estimator_estimate_ebw_handle")
        try:
            return _from_desc(d)
        finally:
            self._lib.gmm_mixture_set_free(ctypes.byref(d))

    @property
    def skipped(self) -> int:
        """Pairs skipped since creation or the last reset (out-of-range frame, mixture or density, no best density)."""
        v = ctypes.c_uint64()
        _capi.check(self._lib.gmm_estimator_skipped(self._h, ctypes.byref(v)), "gmm_estimator_skipped")
        return int(v.value)

    def get(self) -> dict:
        """The tables as f64 numpy arrays: mean_sums [n_means, D], mean_weights [n_means], covariance_sums
        [n_covariances, D], covariance_weights [n_covariances], entry_weights [n_entries]."""
        t = self.topology
        D = t.dimension
        out = {"mean_sums": np.zeros((t.means.shape[0], D), np.float64),
               "mean_weights": np.zeros(t.means.shape[0], np.float64),
               "covariance_sums": np.zeros((t.n_covariances, D), np.float64),
               "covariance_weights": np.zeros(t.n_covariances, np.float64),
               "entry_weights": np.zeros(t.n_entries, np.float64)}
        _capi.check(self._lib.gmm_estimator_get(self._h, _ptr(out["mean_sums"]), _ptr(out["mean_weights"]),
                                                _ptr(out["covariance_sums"]), _ptr(out["covariance_weights"]),
                                                _ptr(out["entry_weights"])), "gmm_estimator_get")
        return out

    def to_bytes(self) -> bytes:
        """gmm_estimator_serialize: the estimator file AbstractMixtureSetEstimator::write produces."""
        size = ctypes.c_uint64()
        _capi.check(self._lib.gmm_estimator_serialize(self._h, None, 0, ctypes.byref(size)), "gmm_estimator_serialize")
        buf = ctypes.create_string_buffer(max(int(size.value), 1))
        _capi.check(self._lib.gmm_estimator_serialize(self._h, buf, size.value, ctypes.byref(size)),
                    "gmm_estimator_serialize")
        return buf.raw[:size.value]

    def write(self, path) -> None:
        _capi.check(self._lib.gmm_estimator_write(self._h, os.fsencode(path)), "gmm_estimator_write")

    def estimate(self, **estimator) -> MixtureSet:
        """gmm_estimator_estimate: the mixture set estimated from the tables (keywords: estimator_config)."""
        d = _capi.MixtureSetDesc()
        cfg = estimator_config(**estimator)
        _capi.check(self._lib.gmm_estimator_estimate(self._h, ctypes.byref(cfg), ctypes.byref(d)), "gmm_estimator_estimate")
        try:
            return _from_desc(d)
        finally:
            self._lib.gmm_mixture_set_free(ctypes.byref(d))


def ebw_config(**kw) -> _capi.EbwConfig:
    """gmm_ebw_config with the reference defaults, overridden by keyword (the struct's fields;
    iteration_constants_type as "global-rwth" / "local-rwth" / "cambridge")."""
    cfg = _capi.EbwConfig()
    _capi.load_library().gmm_default_ebw_config(ctypes.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown EBW parameter {k}")
        setattr(cfg, k, _capi.EBW_TYPES[v] if k == "iteration_constants_type" else v)
    return cfg


def estimate_ebw(data: bytes, previous: MixtureSet, **config) -> MixtureSet:
    """gmm_estimator_estimate_ebw: the EBW estimate from a discriminative estimator file's bytes (host only)."""
    lib = _capi.load_library()
    d = _capi.MixtureSetDesc()
    cfg, prev = ebw_config(**config), previous.desc()
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    _capi.check(lib.gmm_estimator_estimate_ebw(buf, len(data), ctypes.byref(prev), ctypes.byref(cfg), ctypes.byref(d)),
                "gmm_estimator_estimate_ebw")
    try:
        return _from_desc(d)
    finally:
        lib.gmm_mixture_set_free(ctypes.byref(d))


def ebw_iteration_constants(data: bytes, previous: MixtureSet, **config) -> np.ndarray:
    """gmm_estimator_ebw_iteration_constants: the f64 iteration constant of every density of the estimated set."""
    lib = _capi.load_library()
    cfg, prev = ebw_config(**config), previous.desc()
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    n = ctypes.c_uint32()
    _capi.check(lib.gmm_estimator_ebw_iteration_constants(buf, len(data), ctypes.byref(prev), ctypes.byref(cfg), None, 0,
                                                          ctypes.byref(n)), "gmm_estimator_ebw_iteration_constants")
    out = np.zeros(n.value, np.float64)
    _capi.check(lib.gmm_estimator_ebw_iteration_constants(buf, len(data), ctypes.byref(prev), ctypes.byref(cfg), _ptr(out),
                                                          n.value, ctypes.byref(n)), "gmm_estimator_ebw_iteration_constants")
    return out


def combine_discriminative_estimators(files) -> bytes:
    """gmm_estimator_combine_discriminative: combine_estimators for discriminative estimator files (the denominator
    accumulators, the denominator weights and the objective functions are added in file order too)."""
    return _combine(files, "gmm_estimator_combine_discriminative")


def combine_estimators(files) -> bytes:
    """gmm_estimator_combine: the bytes of several estimator files of one topology added in order (host only)."""
    return _combine(files, "gmm_estimator_combine")


def _combine(files, name) -> bytes:
    lib = _capi.load_library()
    fn = getattr(lib, name)
    files = [bytes(f) for f in files]
    n = len(files)
    bufs = [ctypes.create_string_buffer(f, max(len(f), 1)) for f in files]
    data = (ctypes.c_void_p * max(n, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
    sizes = (ctypes.c_uint64 * max(n, 1))(*[len(f) for f in files])
    size = ctypes.c_uint64()
    _capi.check(fn(data, sizes, n, None, 0, ctypes.byref(size)), name)
    out = ctypes.create_string_buffer(max(int(size.value), 1))
    _capi.check(fn(data, sizes, n, out, size.value, ctypes.byref(size)), name)
    return out.raw[:size.value]
