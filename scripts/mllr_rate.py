#!/usr/bin/env python3
"""Time of one device-side MLLR accumulation call (gmm_mllr_accumulate_device) beside the affine feature transform
accumulation (gmm_affine_accumulate_device, pooled model) and the maximum-likelihood accumulation
(gmm_estimator_accumulate_device) of the same pairs as the yardsticks, and the host time of the estimate and of the
adapted means.

Model: the bench model (5000 mixtures x 160 densities, D = 39).  Call: 32768 pairs, one per frame, densities given,
8 keys x 16 regression leaves (mixture m on leaf m mod 16).  With HIP events on the library's stream in this one
process, 20 calls after 3 warm-ups:
  full_ms, shift_ms, both_ms   gmm_mllr_accumulate_device with the kinds full, shift, full | shift
  affine_pooled_ms             gmm_affine_accumulate_device on the same pairs and keys (pooled model: no G work)
  estimator_ms                 gmm_estimator_accumulate_device on the same pairs
and on the host (time.perf_counter, one run each):
  estimate_full_s              gmm_mllr_estimate of key 0 over a balanced tree of 16 leaves, min-observation 100
  adapt_means_s                gmm_mllr_adapt_means of the 800000 means with that estimate
Prints one JSON line.  DESIGN.md section 15 records the numbers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rasr_amd as ra  # noqa: E402
from estimator_rate import EventTimer, _clock_mhz, _library_hip  # noqa: E402

NO_ID = 0xFFFFFFFF


def balanced_tree(n_leaves):
    """Heap order: id i has the children 2 i + 1 and 2 i + 2; the last n_leaves ids are the leaves."""
    n = 2 * n_leaves - 1
    left = np.full(n, NO_ID, np.uint32)
    right = np.full(n, NO_ID, np.uint32)
    parent = np.full(n, NO_ID, np.uint32)
    number = np.full(n, NO_ID, np.uint32)
    for i in range(n):
        if 2 * i + 2 < n:
            left[i], right[i] = 2 * i + 1, 2 * i + 2
            parent[2 * i + 1] = parent[2 * i + 2] = i
        else:
            number[i] = i - (n - n_leaves)
    return {"left": left, "right": right, "parent": parent, "leaf_number": number, "root": 0}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--mixtures", type=int, default=5000)
    p.add_argument("--densities", type=int, default=160)
    p.add_argument("--dim", type=int, default=39)
    p.add_argument("--pairs", type=int, default=32768)
    p.add_argument("--keys", type=int, default=8)
    p.add_argument("--leaves", type=int, default=16)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    import torch
    dev = torch.device("cuda:0")
    timer = EventTimer(_library_hip())
    F, D = args.pairs, args.dim
    ms = ra.synthetic_mixture_set(args.mixtures, args.densities, D, seed=2024)
    leaf = (np.arange(args.mixtures) % args.leaves).astype(np.uint32)
    frames = torch.from_numpy(ra.synthetic_frames(F, D, seed=7)).to(dev)
    rng = np.random.default_rng(8)
    pair_frame = torch.arange(F, dtype=torch.int32, device=dev)  # one pair per frame
    pair_mixture = torch.from_numpy(rng.integers(0, args.mixtures, size=F).astype(np.int32)).to(dev)
    pair_density = torch.from_numpy(rng.integers(0, args.densities, size=F).astype(np.int32)).to(dev)
    pair_key = torch.from_numpy(rng.integers(0, args.keys, size=F).astype(np.int32)).to(dev)
    result = {"model": f"{args.mixtures} x {args.densities} densities, D = {D}", "pairs": F, "keys": args.keys,
              "leaves": args.leaves, "calls": args.calls, "clock": _clock_mhz(torch),
              "device": torch.cuda.get_device_name(0)}
    tables = None
    for name, kinds in (("full_ms", ("full",)), ("shift_ms", ("shift",)), ("both_ms", ("full", "shift"))):
        acc = ra.MllrAccumulator(ms, leaf, args.leaves, args.keys, max_pairs=F, kinds=kinds)
        torch.cuda.synchronize()
        result[name] = timer.ms_per_call(
            lambda: acc.accumulate_device(frames, pair_frame, pair_mixture, pair_density, None, pair_key, stream=0),
            args.calls, args.warmup)
        assert acc.skipped == 0
        result[name.replace("_ms", "_bytes")] = acc.info()
        if name == "full_ms":
            tables = acc.leaf_tables(0)
        acc.close()
    aff = ra.AffineTransformAccumulator(ms, args.keys, max_pairs=F)
    torch.cuda.synchronize()
    result["affine_pooled_ms"] = timer.ms_per_call(
        lambda: aff.accumulate_device(frames, pair_frame, pair_mixture, pair_density, None, pair_key, stream=0),
        args.calls, args.warmup)
    aff.close()
    est = ra.Estimator(ms, max_pairs=F)
    torch.cuda.synchronize()
    result["estimator_ms"] = timer.ms_per_call(
        lambda: est.accumulate_device(frames, pair_frame, pair_mixture, pair_density, stream=0), args.calls, args.warmup)
    assert est.skipped == 0
    for name in ("full_ms", "shift_ms", "both_ms"):
        result[name.replace("_ms", "_over_affine_pooled")] = result[name] / result["affine_pooled_ms"]
        result[name.replace("_ms", "_over_estimator")] = result[name] / result["estimator_ms"]
    result["multiply_adds_per_call_full"] = F * (D * (D + 1) + (D + 1) ** 2)
    result["clock_after"] = _clock_mhz(torch)
    timer.close()
    # the host side, once per speaker
    t0 = time.perf_counter()
    e = ra.estimate_mllr(tables, leaf, balanced_tree(args.leaves), (), min_observation=100.0, kind="full")
    result["estimate_full_s"] = time.perf_counter() - t0
    result["estimate_matrices"] = int(len(e["ids"]))
    t0 = time.perf_counter()
    adapted = ra.adapt_means(ms, e)
    result["adapt_means_s"] = time.perf_counter() - t0
    result["adapt_means_multiply_adds"] = int(adapted.means.shape[0]) * D * (D + 1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
