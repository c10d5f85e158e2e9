#!/usr/bin/env python3
"""Time of one alignment call (gmm_aligner_align_device) over the score table of the bench shape, against the cost of
the table itself: the scoring calls that fill it and a device-to-device copy of it.

Model: the bench model (5000 mixtures x 160 densities, D = 39, pooled covariance); 32768 frames, so the table is
5000 x 32768 f32 = 655 MB.  The same table is cut into segments three ways, each a left-to-right loop / forward / skip
HMM over random mixtures (rasr_amd.linear_hmm_graph), transition weights 3 / 0.5 / 4:
  a   64 segments x 512 frames,  300 states each     the workgroup form, 2 states in some lanes
  b 1024 segments x 32 frames,    30 states each     the single-wave form
  c    8 segments x 4096 frames, 1500 states each    8 workgroups: latency-bound by construction, reported per frame step
Each cut runs twice: without pruning, and with the threshold (found by bisection on the device) that keeps about a tenth
of the unpruned hypotheses.  With HIP events on the null stream in this one process, 20 calls after 3 warm-ups:
  align_ms, frames_per_s, us_per_frame_step (align_ms / the frames of one segment), hypotheses (per call)
  score_ms        the handle's scores-only gmm_score_device call per scorer type, for the same 32768 frames
  table_copy_ms   hipMemcpyAsync device to device of the table
Prints one JSON line and writes it to profiles/aligner_rate.json.  DESIGN.md section 16 records the numbers.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rasr_amd as ra  # noqa: E402
from estimator_rate import EventTimer, _clock_mhz, _library_hip  # noqa: E402

CUTS = (("a", 64, 512, 300), ("b", 1024, 32, 30), ("c", 8, 4096, 1500))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--mixtures", type=int, default=5000)
    p.add_argument("--densities", type=int, default=160)
    p.add_argument("--dim", type=int, default=39)
    p.add_argument("--frames", type=int, default=32768)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "aligner_rate.json"))
    args = p.parse_args()
    import torch
    dev = torch.device("cuda:0")
    hip = _library_hip()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    timer = EventTimer(hip)
    M, F = args.mixtures, args.frames
    ms = ra.synthetic_mixture_set(M, args.densities, args.dim, seed=2024)
    frames = torch.from_numpy(ra.synthetic_frames(F, args.dim, seed=7)).to(dev)
    scores = torch.empty((M, F), dtype=torch.float32, device=dev)
    work = torch.empty((M, F), dtype=torch.float32, device=dev)
    result = {"model": f"{M} x {args.densities} densities, D = {args.dim}, pooled", "frames": F, "calls": args.calls,
              "table_bytes": M * F * 4, "clock": _clock_mhz(torch), "device": torch.cuda.get_device_name(0),
              "score_ms": {}, "cuts": {}}
    for kind in ("diagonal-maximum", "SIMD-diagonal-maximum"):
        sc = ra.Scorer(ms, kind, max_frames=F)
        torch.cuda.synchronize()
        result["score_ms"][kind] = timer.ms_per_call(lambda: sc.score_device(frames, scores, stream=0), args.calls,
                                                     args.warmup)
        sc.close()
    # scores: the SIMD-diagonal-maximum table
    result["table_copy_ms"] = timer.ms_per_call(
        lambda: hip.hipMemcpyAsync(ctypes.c_void_p(work.data_ptr()), ctypes.c_void_p(scores.data_ptr()), M * F * 4, 3, None),
        args.calls, args.warmup)
    del work
    outs = [torch.empty(F, dtype=torch.int32, device=dev) for _ in range(3)]
    rng = np.random.default_rng(11)
    for name, n_segments, n_frames, n_states in CUTS:
        n_segments = min(n_segments, F // n_frames)
        graphs = [ra.linear_hmm_graph(rng.integers(0, M, size=n_states - 1), 3.0, 0.5, 4.0, 0.0) for _ in range(n_segments)]
        b = ra.batch_graphs(graphs, np.arange(n_segments) * n_frames, [n_frames] * n_segments)
        al = ra.Aligner(n_segments, int(b["state_offset"][-1]), int(b["arc_offset"][-1]), n_segments * n_frames * n_states, M)
        al.set_segments(**b)

        def call(threshold):
            return al.align(scores, threshold, out_mixture=outs[0], out_state=outs[1], out_arc=outs[2], stream=0)

        def hypotheses(threshold):
            r = call(threshold)
            torch.cuda.synchronize()
            return int(r["hypotheses"].to(torch.int64).sum().item()), int((r["score"] < 3e38).sum().item())

        full, reached = hypotheses(float("inf"))
        lo, hi = 0.0, 4096.0  # the threshold that keeps about a tenth, by bisection
        for _ in range(14):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if hypotheses(mid)[0] < full // 10 else (lo, mid)
        cut = {"segments": n_segments, "frames_per_segment": n_frames, "states_per_segment": n_states,
               "cells": n_segments * n_frames * n_states}
        for tag, threshold in (("unpruned", float("inf")), ("pruned", hi)):
            t = timer.ms_per_call(lambda: call(threshold), args.calls, args.warmup)
            h, ok = hypotheses(threshold)
            cut[tag] = {"threshold": threshold, "align_ms": t, "frames_per_s": n_segments * n_frames / (t * 1e-3),
                        "us_per_frame_step": t * 1e3 / n_frames, "hypotheses": h, "segments_aligned": ok,
                        "align_over_score": {k: t / v for k, v in result["score_ms"].items()}}
        result["cuts"][name] = cut
        al.close()
    result["clock_after"] = _clock_mhz(torch)
    timer.close()
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
