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


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--mixtures", type=int, default=5000)
    p.add_argument("--densities", type=int, default=160)
    p.add_argument("--dim", type=int, default=39)
    p.add_argument("--frames", type=int, default=32768)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    import torch
    dev = torch.device("cuda:0")
    hip = _library_hip()
    timer = EventTimer(hip)
    F = args.frames
    ms = ra.synthetic_mixture_set(args.mixtures, args.densities, args.dim, seed=2024)
    frames = torch.from_numpy(ra.synthetic_frames(F, args.dim, seed=7)).to(dev)
    rng = np.random.default_rng(8)
    pair_frame = torch.arange(F, dtype=torch.int32, device=dev)  # one pair per frame
    pair_mixture = torch.from_numpy(rng.integers(0, args.mixtures, size=F).astype(np.int32)).to(dev)
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
