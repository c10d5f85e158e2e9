#!/usr/bin/env python3
"""Time of one device-side accumulation call (gmm_estimator_accumulate_device) against the only other way to the
same statistics: the whole best-density table of the same frames (gmm_score_device with best densities), which a
caller then has to copy off the GPU and accumulate on the host.

Model: the bench model (5000 mixtures x 160 densities, D = 39, pooled covariance).  Call: 32768 pairs, one per frame,
the density taken from the scorer.  Per scorer type (SIMD-diagonal-maximum, diagonal-maximum), with HIP events on the
library's stream in this one process:
  accumulate_ms   one gmm_estimator_accumulate_device call (best-density kernel + resolve + 3 sorts + sums)
  sort_sum_ms     the same call with the densities given: the resolve, sort and sum passes alone
  table_ms        one gmm_score_device call with best densities over the same frames
Prints one JSON line.  DESIGN.md section 11 records the numbers.

--mode posteriors: the Baum-Welch call instead (gmm_estimator_accumulate_posteriors_device), diagonal-sum scorer, by
default 8192 pairs, one per frame, so max_pairs = 8192 x 160 contribution slots:
  accumulate_posteriors_ms   the whole call (posterior kernel with the expansion + 3 sorts + sums over all slots)
  posterior_kernel_ms        gmm_density_posteriors_pairs_device alone
  viterbi_accumulate_ms      gmm_estimator_accumulate_device of the same pairs with the same scorer
and the contribution slots of a call and how many of them pass the default weight threshold.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rasr_amd as ra  # noqa: E402
from rasr_amd import _capi  # noqa: E402


def _library_hip():
    """The HIP runtime librasr_gmm.so runs on: the process's only libamdhip64, or, where the library brought its own
    beside torch's copy (rasr_amd/_capi.py), the one mapped from outside the torch package."""
    _capi.load_library()
    paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    if not paths:
        raise RuntimeError("no HIP runtime is mapped")
    own = [p for p in paths if "/torch/" not in p]
    hip = ctypes.CDLL((own or paths)[0])
    hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventDestroy.argtypes = [ctypes.c_void_p]
    return hip


class EventTimer:
    def __init__(self, hip):
        self.hip = hip
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            if hip.hipEventCreate(ctypes.byref(e)) != 0:
                raise RuntimeError("hipEventCreate failed")

    def ms_per_call(self, fn, calls, warmup):
        for _ in range(warmup):
            fn()
        assert self.hip.hipEventRecord(self.a, None) == 0
        for _ in range(calls):
            fn()
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return ms.value / calls

    def close(self):
        for e in (self.a, self.b):
            self.hip.hipEventDestroy(e)


def _clock_mhz(torch):
    out = {}
    try:
        out["current_mhz"] = int(torch.cuda.clock_rate())
    except Exception:
        pass
    rate = getattr(torch.cuda.get_device_properties(0), "clock_rate", None)
    if rate:
        out["max_mhz"] = int(rate) // 1000
    return out


def posterior_rates(args, torch, timer, ms, frames, pair_frame, pair_mixture):
    F, K = int(pair_frame.numel()), args.densities
    lib = _capi.load_library()
    sc = ra.Scorer(ms, "diagonal-sum", max_frames=F)
    est = ra.Estimator(ms, max_pairs=F * K)
    post = torch.empty((F, K), dtype=torch.float32, device=frames.device)
    logden = torch.empty(F, dtype=torch.float32, device=frames.device)

    def kernel():  # the C call on kept tensors: Scorer.density_posteriors_device allocates its outputs
        rc = lib.gmm_density_posteriors_pairs_device(
            sc.handle, ctypes.c_void_p(frames.data_ptr()), F, int(frames.stride(0)),
            ctypes.c_void_p(pair_frame.data_ptr()), ctypes.c_void_p(pair_mixture.data_ptr()), F,
            ctypes.c_void_p(post.data_ptr()), K, ctypes.c_void_p(logden.data_ptr()), None)
        _capi.check(rc, "gmm_density_posteriors_pairs_device")
    torch.cuda.synchronize()
    r = {"model": f"{args.mixtures} x {args.densities} densities, D = {args.dim}, pooled", "pairs": F,
         "calls": args.calls, "clock": _clock_mhz(torch), "device": torch.cuda.get_device_name(0)}
    r["accumulate_posteriors_ms"] = timer.ms_per_call(
        lambda: est.accumulate_posteriors_device(frames, pair_frame, pair_mixture, scorer=sc, stream=0), args.calls,
        args.warmup)
    r["posterior_kernel_ms"] = timer.ms_per_call(kernel, args.calls, args.warmup)
    r["viterbi_accumulate_ms"] = timer.ms_per_call(
        lambda: est.accumulate_device(frames, pair_frame, pair_mixture, scorer=sc, stream=0), args.calls, args.warmup)
    assert est.skipped == 0
    torch.cuda.synchronize()
    r["contribution_slots"] = F * K
    r["contributions_over_threshold"] = int((post.double() > ra.DEFAULT_WEIGHT_THRESHOLD).sum().item())
    r["clock_after"] = _clock_mhz(torch)
    sc.close()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--mixtures", type=int, default=5000)
    p.add_argument("--densities", type=int, default=160)
    p.add_argument("--dim", type=int, default=39)
    p.add_argument("--frames", type=int, default=None, help="default: 32768, 8192 in posteriors mode")
    p.add_argument("--mode", choices=["viterbi", "posteriors"], default="viterbi")
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    import torch
    dev = torch.device("cuda:0")
    hip = _library_hip()
    timer = EventTimer(hip)
    F = args.frames or (8192 if args.mode == "posteriors" else 32768)
    ms = ra.synthetic_mixture_set(args.mixtures, args.densities, args.dim, seed=2024)
    frames = torch.from_numpy(ra.synthetic_frames(F, args.dim, seed=7)).to(dev)
    rng = np.random.default_rng(8)
    pair_frame = torch.arange(F, dtype=torch.int32, device=dev)  # one pair per frame
    pair_mixture = torch.from_numpy(rng.integers(0, args.mixtures, size=F).astype(np.int32)).to(dev)
    if args.mode == "posteriors":
        print(json.dumps(posterior_rates(args, torch, timer, ms, frames, pair_frame, pair_mixture)))
        timer.close()
        return
    est = ra.Estimator(ms, max_pairs=F)
    result = {"model": f"{args.mixtures} x {args.densities} densities, D = {args.dim}, pooled", "pairs": F,
              "calls": args.calls, "clock": _clock_mhz(torch), "device": torch.cuda.get_device_name(0), "types": {}}
    for kind in ("SIMD-diagonal-maximum", "diagonal-maximum"):
        sc = ra.Scorer(ms, kind, max_frames=F)
        best = torch.empty(F, dtype=torch.int32, device=dev)
        sc.best_pairs_device(frames, pair_frame, pair_mixture, best)
        scores = torch.empty((args.mixtures, F), dtype=torch.float32, device=dev)
        table = torch.empty((args.mixtures, F), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        r = {}
        r["accumulate_ms"] = timer.ms_per_call(
            lambda: est.accumulate_device(frames, pair_frame, pair_mixture, scorer=sc), args.calls, args.warmup)
        r["sort_sum_ms"] = timer.ms_per_call(
            lambda: est.accumulate_device(frames, pair_frame, pair_mixture, pair_density=best), args.calls, args.warmup)
        r["table_ms"] = timer.ms_per_call(lambda: sc.score_device(frames, scores, table), args.calls, args.warmup)
        r["accumulate_faster_than_table"] = bool(r["accumulate_ms"] < r["table_ms"])
        assert est.skipped == 0
        result["types"][kind] = r
        sc.close()
        del scores, table
    timer.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
