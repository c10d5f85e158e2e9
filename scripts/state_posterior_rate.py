#!/usr/bin/env python3
"""Time of one state-posterior call (gmm_state_posteriors_device) over the score table of the bench shape, against
the table's own cost: a device-to-device copy of it and the scoring calls that produce it.

Model: the bench model (5000 mixtures x 160 densities, D = 39, pooled covariance); 32768 frames, so the table is
5000 x 32768 f32 = 655 MB.  With HIP events on the library's stream in this one process, 20 calls after 3 warm-ups:
  posteriors_f32_in_place_ms   the call with posteriors_f32 == scores (priors given, no pruning); the table it runs on
                               is a copy of the scores that the first call turns into posteriors, so later calls read
                               values in [0, 1]: the work per cell is the same
  posteriors_f64_ms            the call with an f64 output table (1.3 GB written) from the untouched scores
  ..._64_frames_ms             both at 64 frames (one workgroup column: 20 workgroups of 64 live lanes per pass)
  table_copy_ms                hipMemcpyAsync device to device of the f32 table: the call reads it three times and, in
                               place, writes it once, so four copies' bytes are its floor
  score_ms                     the handle's scores-only gmm_score_device call per scorer type
Prints one JSON line.  DESIGN.md section 12 records the numbers.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rasr_amd as ra  # noqa: E402
from estimator_rate import EventTimer, _clock_mhz, _library_hip  # noqa: E402
from rasr_amd import _capi  # noqa: E402

DBL_MAX = float(np.finfo(np.float64).max)


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
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    timer = EventTimer(hip)
    lib = _capi.load_library()
    M, F = args.mixtures, args.frames
    ms = ra.synthetic_mixture_set(M, args.densities, args.dim, seed=2024)
    frames = torch.from_numpy(ra.synthetic_frames(F, args.dim, seed=7)).to(dev)
    priors = torch.from_numpy(np.random.default_rng(9).random(M) * 8.0).to(dev)
    scores = torch.empty((M, F), dtype=torch.float32, device=dev)
    work = torch.empty((M, F), dtype=torch.float32, device=dev)
    post64 = torch.empty((M, F), dtype=torch.float64, device=dev)
    log_z = torch.empty(F, dtype=torch.float64, device=dev)
    n_active = torch.empty(F, dtype=torch.int32, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    result = {"model": f"{M} x {args.densities} densities, D = {args.dim}, pooled", "frames": F, "calls": args.calls,
              "table_bytes": M * F * 4, "clock": _clock_mhz(torch), "device": torch.cuda.get_device_name(0),
              "score_ms": {}}
    sc = None
    for kind in ("diagonal-maximum", "SIMD-diagonal-maximum"):
        if sc is not None:
            sc.close()
        sc = ra.Scorer(ms, kind, max_frames=F)
        torch.cuda.synchronize()
        result["score_ms"][kind] = timer.ms_per_call(lambda: sc.score_device(frames, scores, stream=0), args.calls,
                                                     args.warmup)
    # scores: the SIMD-diagonal-maximum table; sc: that handle

    def call(table, n_frames, f32, f64):
        rc = lib.gmm_state_posteriors_device(sc.handle, ptr(table), n_frames, F, ptr(priors), 1.0, DBL_MAX, f32, f64, F,
                                             ptr(log_z), None, None, ptr(n_active), None)
        _capi.check(rc, "gmm_state_posteriors_device")

    def copy():
        assert hip.hipMemcpyAsync(ptr(work), ptr(scores), M * F * 4, 3, None) == 0  # hipMemcpyDeviceToDevice

    torch.cuda.synchronize()
    result["table_copy_ms"] = timer.ms_per_call(copy, args.calls, args.warmup)
    for n, tag in ((F, ""), (min(F, 64), "_64_frames")):
        result[f"posteriors_f64{tag}_ms"] = timer.ms_per_call(lambda: call(scores, n, None, ptr(post64)), args.calls,
                                                              args.warmup)
        copy()
        result[f"posteriors_f32_in_place{tag}_ms"] = timer.ms_per_call(lambda: call(work, n, ptr(work), None),
                                                                       args.calls, args.warmup)
    torch.cuda.synchronize()
    assert int(n_active.view(torch.int32)[0].item()) == M
    t = result["posteriors_f32_in_place_ms"]
    result["in_place_over_four_copies"] = t / (4 * result["table_copy_ms"])
    result["in_place_over_two_copies"] = t / (2 * result["table_copy_ms"])  # a copy reads and writes: the same bytes
    result["in_place_over_score"] = {k: t / v for k, v in result["score_ms"].items()}
    result["clock_after"] = _clock_mhz(torch)
    timer.close()
    sc.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
