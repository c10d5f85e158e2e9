#!/usr/bin/env python3
"""Time of one joint numerator / denominator accumulation call (gmm_estimator_accumulate_discriminative_device)
against the other way to the same two table sets: two maximum-likelihood calls of the same pairs on two handles.

Model: the bench model (5000 mixtures x 160 densities, D = 39, pooled covariance).  Viterbi call: 32768 pairs, one per
frame, the density taken from a SIMD-diagonal-maximum scorer, both weights given.  Posterior call: 8192 pairs,
diagonal-sum scorer, max_pairs = 8192 x 160 contribution slots.  HIP events on the library's stream around `--calls`
calls after `--warmup` warm-ups, in this one process (scripts/estimator_rate.py's timer):
  joint_ms                 one gmm_estimator_accumulate_discriminative_device call
  two_calls_ms             two gmm_estimator_accumulate_device calls (numerator handle, denominator handle)
  joint_posteriors_ms      one gmm_estimator_accumulate_discriminative_posteriors_device call
  two_posterior_calls_ms   two gmm_estimator_accumulate_posteriors_device calls on two handles
and the ratios joint / two calls.  Prints one JSON line.  DESIGN.md section 14 records the numbers.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from estimator_rate import EventTimer, _clock_mhz, _library_hip  # noqa: E402

import rasr_amd as ra  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--mixtures", type=int, default=5000)
    p.add_argument("--densities", type=int, default=160)
    p.add_argument("--dim", type=int, default=39)
    p.add_argument("--pairs", type=int, default=32768)
    p.add_argument("--posterior-pairs", type=int, default=8192)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    import torch
    dev = torch.device("cuda:0")
    timer = EventTimer(_library_hip())
    F, P, K = args.pairs, args.posterior_pairs, args.densities
    ms = ra.synthetic_mixture_set(args.mixtures, K, args.dim, seed=2024)
    frames = torch.from_numpy(ra.synthetic_frames(F, args.dim, seed=7)).to(dev)
    rng = np.random.default_rng(8)
    pair_frame = torch.arange(F, dtype=torch.int32, device=dev)  # one pair per frame
    pair_mixture = torch.from_numpy(rng.integers(0, args.mixtures, size=F).astype(np.int32)).to(dev)
    w_num = torch.from_numpy(rng.uniform(0.1, 1.0, size=F)).to(dev)
    w_den = torch.from_numpy(rng.uniform(0.1, 1.0, size=F)).to(dev)
    r = {"model": f"{args.mixtures} x {K} densities, D = {args.dim}, pooled", "pairs": F, "posterior_pairs": P,
         "calls": args.calls, "clock": _clock_mhz(torch), "device": torch.cuda.get_device_name(0)}

    sc = ra.Scorer(ms, "SIMD-diagonal-maximum", max_frames=F)
    joint, num, den = (ra.Estimator(ms, max_pairs=F) for _ in range(3))
    torch.cuda.synchronize()

    def two_calls():
        num.accumulate_device(frames, pair_frame, pair_mixture, pair_weight=w_num, scorer=sc, stream=0)
        den.accumulate_device(frames, pair_frame, pair_mixture, pair_weight=w_den, scorer=sc, stream=0)
    r["joint_ms"] = timer.ms_per_call(
        lambda: joint.accumulate_discriminative_device(frames, pair_frame, pair_mixture, pair_weight_num=w_num,
                                                       pair_weight_den=w_den, scorer=sc, stream=0),
        args.calls, args.warmup)
    r["two_calls_ms"] = timer.ms_per_call(two_calls, args.calls, args.warmup)
    r["joint_over_two_calls"] = r["joint_ms"] / r["two_calls_ms"]
    assert joint.skipped == 0 and num.skipped == 0 and den.skipped == 0
    for e in (joint, num, den):
        e.close()
    sc.close()

    sc = ra.Scorer(ms, "diagonal-sum", max_frames=P)
    joint, num, den = (ra.Estimator(ms, max_pairs=P * K) for _ in range(3))
    pf, pm, wn, wd = pair_frame[:P], pair_mixture[:P], w_num[:P].contiguous(), w_den[:P].contiguous()
    torch.cuda.synchronize()

    def two_posterior_calls():
        num.accumulate_posteriors_device(frames, pf, pm, wn, scorer=sc, stream=0)
        den.accumulate_posteriors_device(frames, pf, pm, wd, scorer=sc, stream=0)
    r["joint_posteriors_ms"] = timer.ms_per_call(
        lambda: joint.accumulate_discriminative_posteriors_device(frames, pf, pm, wn, wd, scorer=sc, stream=0),
        args.calls, args.warmup)
    r["two_posterior_calls_ms"] = timer.ms_per_call(two_posterior_calls, args.calls, args.warmup)
    r["joint_posteriors_over_two_calls"] = r["joint_posteriors_ms"] / r["two_posterior_calls_ms"]
    assert joint.skipped == 0 and num.skipped == 0 and den.skipped == 0
    r["clock_after"] = _clock_mhz(torch)
    timer.close()
    print(json.dumps(r))


if __name__ == "__main__":
    main()
