#!/usr/bin/env python3
"""Time of one Baum-Welch alignment call (gmm_aligner_posteriors_device) beside the Viterbi call
(gmm_aligner_align_device) on the same handle, table and batch, in one run.

Model, table and graphs are those of scripts/aligner_rate.py (same seeds), cuts a and b:
  a   64 segments x 512 frames,  300 states each     the workgroup form
  b 1024 segments x 32 frames,    30 states each     the single-wave form
Each cut runs without pruning and with the threshold found there by bisection on the Viterbi call (about a tenth of the
unpruned hypotheses).  HIP events on the null stream in this one process, 20 calls after 3 warm-ups.  The posterior call
is made through the C interface with outputs allocated once (Aligner.posteriors would read the count back, a
synchronisation per call); the count is read after the timed calls.
Per cut and threshold: align_ms, posteriors_ms, their ratio, frames_per_s of both, n_items, hypotheses of both.
Prints one JSON line and writes it to profiles/aligner_posterior_rate.json.  DESIGN.md section 17 records the numbers.
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
from rasr_amd import _capi  # noqa: E402
from estimator_rate import EventTimer, _clock_mhz, _library_hip  # noqa: E402

CUTS = (("a", 64, 512, 300), ("b", 1024, 32, 30))


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--mixtures", type=int, default=5000)
    p.add_argument("--densities", type=int, default=160)
    p.add_argument("--dim", type=int, default=39)
    p.add_argument("--frames", type=int, default=32768)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "aligner_posterior_rate.json"))
    args = p.parse_args()
    import torch
    dev = torch.device("cuda:0")
    timer = EventTimer(_library_hip())
    lib = _capi.load_library()
    M, F = args.mixtures, args.frames
    ms = ra.synthetic_mixture_set(M, args.densities, args.dim, seed=2024)
    frames = torch.from_numpy(ra.synthetic_frames(F, args.dim, seed=7)).to(dev)
    scores = torch.empty((M, F), dtype=torch.float32, device=dev)
    sc = ra.Scorer(ms, "SIMD-diagonal-maximum", max_frames=F)
    sc.score_device(frames, scores, stream=0)
    torch.cuda.synchronize()
    sc.close()
    result = {"model": f"{M} x {args.densities} densities, D = {args.dim}, pooled", "frames": F, "calls": args.calls,
              "clock": _clock_mhz(torch), "device": torch.cuda.get_device_name(0), "cuts": {}}
    outs = [torch.empty(F, dtype=torch.int32, device=dev) for _ in range(3)]
    rng = np.random.default_rng(11)
    for name, n_segments, n_frames, n_states in CUTS:
        n_segments = min(n_segments, F // n_frames)
        graphs = [ra.linear_hmm_graph(rng.integers(0, M, size=n_states - 1), 3.0, 0.5, 4.0, 0.0) for _ in range(n_segments)]
        b = ra.batch_graphs(graphs, np.arange(n_segments) * n_frames, [n_frames] * n_segments)
        cells = n_segments * n_frames * n_states
        al = ra.Aligner(n_segments, int(b["state_offset"][-1]), int(b["arc_offset"][-1]), cells, M)
        al.set_segments(**b)
        cap = cells
        item = {"frame": torch.empty(cap, dtype=torch.int32, device=dev), "mixture": torch.empty(cap, dtype=torch.int32, device=dev),
                "weight": torch.empty(cap, dtype=torch.float64, device=dev),
                "column_offset": torch.empty(F + 1, dtype=torch.int32, device=dev),
                "n_items": torch.zeros(1, dtype=torch.int32, device=dev),
                "score": torch.empty(n_segments, dtype=torch.float32, device=dev),
                "hypotheses": torch.empty(n_segments, dtype=torch.int32, device=dev),
                "log_total": torch.empty(n_segments, dtype=torch.float64, device=dev)}
        pointers = [ctypes.c_void_p(t.data_ptr()) for t in item.values()]

        def viterbi(threshold):
            return al.align(scores, threshold, out_mixture=outs[0], out_state=outs[1], out_arc=outs[2], stream=0)

        def posteriors(threshold):
            _capi.check(lib.gmm_aligner_posteriors_device(al.handle, ctypes.c_void_p(scores.data_ptr()), F,
                                                          int(scores.stride(0)), float(threshold), 0.0, cap, *pointers, None),
                        "gmm_aligner_posteriors_device")

        def hypotheses(threshold):
            r = viterbi(threshold)
            torch.cuda.synchronize()
            return int(r["hypotheses"].to(torch.int64).sum().item())

        full = hypotheses(float("inf"))
        lo, hi = 0.0, 4096.0  # the threshold of scripts/aligner_rate.py: about a tenth of the hypotheses
        for _ in range(14):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if hypotheses(mid) < full // 10 else (lo, mid)
        cut = {"segments": n_segments, "frames_per_segment": n_frames, "states_per_segment": n_states, "cells": cells}
        for tag, threshold in (("unpruned", float("inf")), ("pruned", hi)):
            tv = timer.ms_per_call(lambda: viterbi(threshold), args.calls, args.warmup)
            tp = timer.ms_per_call(lambda: posteriors(threshold), args.calls, args.warmup)
            torch.cuda.synchronize()
            cut[tag] = {"threshold": threshold, "align_ms": tv, "posteriors_ms": tp, "posteriors_over_align": tp / tv,
                        "align_frames_per_s": n_segments * n_frames / (tv * 1e-3),
                        "posteriors_frames_per_s": n_segments * n_frames / (tp * 1e-3),
                        "n_items": int(item["n_items"].item()), "viterbi_hypotheses": hypotheses(threshold),
                        "posterior_hypotheses": int(item["hypotheses"].to(torch.int64).sum().item()),
                        "segments_aligned": int((item["score"] < 3e38).sum().item())}
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
