#!/usr/bin/env python3
"""Time of the search calls (gmm_aligner_align_search_device, gmm_aligner_posteriors_search_device) in the form of
scripts/aligner_rate.py: the SIMD-diagonal-maximum table of a synthetic model, left-to-right loop / forward / skip HMMs
over random mixtures (transition weights 3 / 0.5 / 4), HIP events on the null stream, `--calls` calls after `--warmup`.

  search_vs_host_loop   the default schedule (50, 100, 200, ... with the score-difference rule) on 30- and 300-state
                        segments, Viterbi mode: the one search call against the only way to the same result without it,
                        a host loop over gmm_aligner_align_device -- per round a launch, a read-back of the per-segment
                        scores and hypothesis counts, and set_segments with the segments that have not stopped.  The host
                        loop is timed with a wall clock around it (it synchronises every round); both in ms per batch.
                        The loop's result is checked against the search call's (scores, thresholds, iterations).
  n_best_frame          one segment of 128 and of 2432 states (every state reached in every frame: the start state
                        reaches all), min == max threshold: us per frame with n_best = n_states / 2 against the same
                        call with n-best inactive, both modes.
Prints one JSON line and writes it to profiles/aligner_search_rate.json.  DESIGN.md sections 16 and 17 record the numbers.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rasr_amd as ra  # noqa: E402
from estimator_rate import EventTimer, _clock_mhz, _library_hip  # noqa: E402

FLT_MAX = float(np.finfo(np.float32).max)


def almost_equal(a, b):
    a, b = np.float32(a), np.float32(b)
    with np.errstate(all="ignore"):
        return bool(np.abs(np.float32(a - b)) < np.float32(np.float32(np.float32(np.abs(a) + np.abs(b))
                                                                      + np.float32(np.finfo(np.float32).tiny))
                                                           * np.float32(np.finfo(np.float32).eps)))


def host_loop(torch, graphs, begin, frames, scores, search, n_mixtures, handles):
    """Search::Aligner::feed(vector) on the host over the fixed-threshold call: returns per segment (score, threshold,
    iterations).  handles[k] is an Aligner big enough for the whole batch (one per round, so that set_segments of a round
    does not wait for anything but its own handle)."""
    n = len(graphs)
    score, threshold, iterations = np.full(n, FLT_MAX, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int64)
    previous = np.full(n, FLT_MAX, np.float32)
    todo, t, rounds = list(range(n)), np.float32(search.min_pruning), 0
    while todo and t <= np.float32(search.max_pruning):
        al = handles[rounds % len(handles)]
        al.set_segments(**ra.batch_graphs([graphs[i] for i in todo], [begin[i] for i in todo], [frames[i] for i in todo]))
        r = al.align(scores, float(t), stream=0)
        sc, hyp = r["score"].cpu().numpy(), r["hypotheses"].cpu().numpy()  # the read-back: the round's synchronisation
        rounds += 1
        nxt = []
        for k, i in enumerate(todo):
            score[i], threshold[i], iterations[i] = sc[k], t, iterations[i] + 1
            ok = sc[k] != np.float32(FLT_MAX) and hyp[k] / frames[i] >= search.min_average_hypotheses
            if ok and (not search.until_no_score_difference or (iterations[i] > 1 and almost_equal(sc[k], previous[i]))):
                continue
            previous[i] = sc[k]
            nxt.append(i)
        todo, t = nxt, np.float32(t * np.float32(search.increment_factor))
    return score, threshold, iterations, rounds


def fan_graph(rng, n_states, n_mixtures):
    """State 0 reaches every state; the others loop, go forward and skip: all states are reached in every frame."""
    arcs = {0: [(k, int(rng.integers(0, n_mixtures)), float(rng.random() * 3)) for k in range(1, n_states)]}
    for k in range(1, n_states):
        arcs[k] = [(q, int(rng.integers(0, n_mixtures)), w) for q, w in ((k, 3.0), (k + 1, 0.5), (k + 2, 4.0)) if q < n_states]
    offset = np.concatenate(([0], np.cumsum([len(arcs[k]) for k in range(n_states)]))).astype(np.uint32)
    flat = [a for k in range(n_states) for a in arcs[k]]
    final = np.zeros(n_states, dtype=np.float32)
    final[0] = np.inf
    return {"n_states": n_states, "arc_offset": offset, "arc_target": np.asarray([a[0] for a in flat], dtype=np.uint32),
            "arc_mixture": np.asarray([a[1] for a in flat], dtype=np.uint32),
            "arc_weight": np.asarray([a[2] for a in flat], dtype=np.float32), "final_weight": final, "initial_state": 0}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--mixtures", type=int, default=5000)
    p.add_argument("--densities", type=int, default=16)
    p.add_argument("--dim", type=int, default=39)
    p.add_argument("--frames", type=int, default=32768)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "aligner_search_rate.json"))
    args = p.parse_args()
    import torch
    dev = torch.device("cuda:0")
    timer = EventTimer(_library_hip())
    M, F = args.mixtures, args.frames
    ms = ra.synthetic_mixture_set(M, args.densities, args.dim, seed=2024)
    feats = torch.from_numpy(ra.synthetic_frames(F, args.dim, seed=7)).to(dev)
    scores = torch.empty((M, F), dtype=torch.float32, device=dev)
    sc = ra.Scorer(ms, "SIMD-diagonal-maximum", max_frames=F)
    sc.score_device(feats, scores, stream=0)
    torch.cuda.synchronize()
    sc.close()
    result = {"model": f"{M} x {args.densities} densities, D = {args.dim}, pooled", "frames": F, "calls": args.calls,
              "clock": _clock_mhz(torch), "device": torch.cuda.get_device_name(0), "search_vs_host_loop": {},
              "n_best_frame": {}}
    rng = np.random.default_rng(11)
    search = ra.AlignSearch()
    for name, n_segments, n_frames, n_states in (("30_states", 1024, 32, 30), ("300_states", 64, 512, 300)):
        n_segments = min(n_segments, F // n_frames)
        graphs = [ra.linear_hmm_graph(rng.integers(0, M, size=n_states - 1), 3.0, 0.5, 4.0, 0.0) for _ in range(n_segments)]
        begin, frames = [int(i * n_frames) for i in range(n_segments)], [n_frames] * n_segments
        b = ra.batch_graphs(graphs, begin, frames)
        size = (n_segments, int(b["state_offset"][-1]), int(b["arc_offset"][-1]), n_segments * n_frames * n_states, M)
        al = ra.Aligner(*size)
        al.set_segments(**b)
        outs = [torch.empty(F, dtype=torch.int32, device=dev) for _ in range(3)]
        call = lambda: al.align(scores, out_mixture=outs[0], out_state=outs[1], out_arc=outs[2], stream=0,  # noqa: E731
                                search=search)
        ms_search = timer.ms_per_call(call, args.calls, args.warmup)
        r = call()
        torch.cuda.synchronize()
        handles = [ra.Aligner(*size) for _ in range(2)]
        for _ in range(args.warmup):
            loop = host_loop(torch, graphs, begin, frames, scores, search, M, handles)
        t0 = time.perf_counter()
        for _ in range(args.calls):
            loop = host_loop(torch, graphs, begin, frames, scores, search, M, handles)
        ms_loop = (time.perf_counter() - t0) * 1e3 / args.calls
        it = r["iterations"].cpu().numpy()
        same = (np.array_equal(r["score"].cpu().numpy().view(np.uint32), loop[0].view(np.uint32))
                and np.array_equal(r["threshold"].cpu().numpy(), loop[1]) and np.array_equal(it, loop[2]))
        result["search_vs_host_loop"][name] = {
            "segments": n_segments, "frames_per_segment": n_frames, "states_per_segment": n_states,
            "search_call_ms": ms_search, "host_loop_ms": ms_loop, "host_loop_rounds": loop[3],
            "iterations_min": int(it.min()), "iterations_max": int(it.max()), "iterations_mean": float(it.mean()),
            "segments_aligned": int((r["score"] < 3e38).sum().item()), "host_loop_equals_search_call": bool(same)}
        for h in handles + [al]:
            h.close()
    for n_states in (128, 2432):
        n_frames = 256
        g = fan_graph(rng, n_states, M)
        b = ra.batch_graphs([g], [0], [n_frames])
        al = ra.Aligner(1, n_states, int(b["arc_offset"][-1]), n_frames * n_states, M)
        al.set_segments(**b)
        entry = {"frames": n_frames}
        for mode in ("viterbi", "posteriors"):
            for tag, n_best in (("off", 0x7FFFFFFF), ("on", n_states // 2)):
                s = ra.AlignSearch(min_pruning=FLT_MAX, max_pruning=FLT_MAX, increment_factor=1.0, n_best=n_best)
                if mode == "viterbi":
                    call = lambda: al.align(scores, stream=0, search=s)  # noqa: E731
                else:
                    # the count and the score only: no item arrays; the first warm-up call makes the first-use allocation
                    lib, h = al._lib, al.handle
                    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
                    d_s = torch.zeros(1, dtype=torch.float32, device=dev)
                    st = s._struct()
                    call = lambda: lib.gmm_aligner_posteriors_search_device(  # noqa: E731
                        h, ctypes.c_void_p(scores.data_ptr()), F, int(scores.stride(0)), ctypes.byref(st), 0.0, 0, None, None,
                        None, None, ctypes.c_void_p(d_n.data_ptr()), ctypes.c_void_p(d_s.data_ptr()), None, None, None,
                        None, None)
                t = timer.ms_per_call(call, args.calls, args.warmup)
                entry[f"{mode}_n_best_{tag}_us_per_frame"] = t * 1e3 / n_frames
        result["n_best_frame"][f"{n_states}_states"] = entry
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
