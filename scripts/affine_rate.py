#!/usr/bin/env python3
"""Time of one device-side affine feature transform accumulation call (gmm_affine_accumulate_device) beside the
maximum-likelihood accumulation of the same pairs (gmm_estimator_accumulate_device) as the yardstick.

Model: the bench model (5000 mixtures x 160 densities, D = 39).  Call: 32768 pairs, one per frame, densities given,
8 keys.  With HIP events on the library's stream in this one process, 20 calls after 3 warm-ups:
  pooled_ms             (a) the pooled model: no G work, the small tables only
  mixture_specific_ms   (b) the same model with tying="mixture-specific": D * (D+1)(D+2)/2 f64 divisions per pair
  estimator_ms          (c) gmm_estimator_accumulate_device on the same pairs (pooled model)
and for (b) the count of f64 divisions of a call, n_pairs * D * (D+1)(D+2)/2, and the implied divisions per second.
Prints one JSON line.  DESIGN.md section 13 records the numbers.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rasr_amd as ra  # noqa: E402
from estimator_rate import EventTimer, _clock_mhz, _library_hip  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--mixtures", type=int, default=5000)
    p.add_argument("--densities", type=int, default=160)
    p.add_argument("--dim", type=int, default=39)
    p.add_argument("--pairs", type=int, default=32768)
    p.add_argument("--keys", type=int, default=8)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    import torch
    dev = torch.device("cuda:0")
    timer = EventTimer(_library_hip())
    F, D = args.pairs, args.dim
    pooled = ra.synthetic_mixture_set(args.mixtures, args.densities, D, seed=2024)
    tied = ra.synthetic_mixture_set(args.mixtures, args.densities, D, seed=2024, tying="mixture-specific")
    frames = torch.from_numpy(ra.synthetic_frames(F, D, seed=7)).to(dev)
    rng = np.random.default_rng(8)
    pair_frame = torch.arange(F, dtype=torch.int32, device=dev)  # one pair per frame
    pair_mixture = torch.from_numpy(rng.integers(0, args.mixtures, size=F).astype(np.int32)).to(dev)
    pair_density = torch.from_numpy(rng.integers(0, args.densities, size=F).astype(np.int32)).to(dev)
    pair_key = torch.from_numpy(rng.integers(0, args.keys, size=F).astype(np.int32)).to(dev)
    result = {"model": f"{args.mixtures} x {args.densities} densities, D = {D}", "pairs": F, "keys": args.keys,
              "calls": args.calls, "clock": _clock_mhz(torch), "device": torch.cuda.get_device_name(0)}
    for name, ms in (("pooled_ms", pooled), ("mixture_specific_ms", tied)):
        acc = ra.AffineTransformAccumulator(ms, args.keys, max_pairs=F)
        torch.cuda.synchronize()
        result[name] = timer.ms_per_call(
            lambda: acc.accumulate_device(frames, pair_frame, pair_mixture, pair_density, None, pair_key, stream=0),
            args.calls, args.warmup)
        assert acc.skipped == 0
        result[name.replace("_ms", "_bytes")] = acc.info()
        acc.close()
    est = ra.Estimator(pooled, max_pairs=F)
    torch.cuda.synchronize()
    result["estimator_ms"] = timer.ms_per_call(
        lambda: est.accumulate_device(frames, pair_frame, pair_mixture, pair_density, stream=0), args.calls, args.warmup)
    assert est.skipped == 0
    divisions = F * D * (D + 1) * (D + 2) // 2
    result["g_divisions_per_call"] = divisions
    result["g_divisions_per_second"] = divisions / (result["mixture_specific_ms"] * 1e-3)
    result["clock_after"] = _clock_mhz(torch)
    timer.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
