"""Python handle over the Viterbi alignment of include/rasr_gmm_align.h.

`Aligner` aligns a batch of segments, each with its own automaton, against a score table that is already on the GPU
(Search::Aligner in Viterbi mode with acoustic pruning) and returns one mixture index per table column as a device
tensor, which goes into `Estimator.accumulate_device` and its siblings as `pair_mixture` without a copy.

A GRAPH here is a dict of numpy arrays describing one segment's automaton, states 0 .. n_states-1:
    n_states, arc_offset [n_states + 1] (CSR by source state), arc_target, arc_mixture, arc_weight [n_arcs],
    final_weight [n_states] (+inf: not final), initial_state.
`linear_hmm_graph` builds one; `batch_graphs` concatenates several into the arguments of `Aligner.set_segments`.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

from . import _capi
from ._pairs import ptr as _ptr

MAX_STATES = _capi.GMM_ALIGN_MAX_STATES
MAX_STATES_POSTERIOR = _capi.GMM_ALIGN_MAX_STATES_POSTERIOR
MAX_IN_ARCS = _capi.GMM_ALIGN_MAX_IN_ARCS
MAX_ITERATIONS = _capi.GMM_ALIGN_MAX_ITERATIONS
NONE = _capi.GMM_ALIGN_NONE


@dataclasses.dataclass
class AlignSearch:
    """gmm_align_search: the pruning-threshold search of Search::Aligner::feed and its n-best pruning, with the
    reference's defaults (include/rasr_gmm_align.h, "THE SEARCH")."""
    min_pruning: float = 50.0                 # min-acoustic-pruning
    max_pruning: float = float(np.finfo(np.float32).max)  # max-acoustic-pruning
    increment_factor: float = 2.0             # acoustic-pruning-increment-factor
    min_average_hypotheses: float = 0.0       # min-average-number-of-states
    until_no_score_difference: bool = True    # increase-pruning-until-no-score-difference
    n_best: int = 0x7FFFFFFF                  # n-best-pruning

    def _struct(self) -> "_capi.AlignSearchStruct":
        return _capi.AlignSearchStruct(float(self.min_pruning), float(self.max_pruning), float(self.increment_factor),
                                       float(self.min_average_hypotheses), int(bool(self.until_no_score_difference)),
                                       int(self.n_best))


def linear_hmm_graph(mixtures, loop, forward, skip, exit, repeat: int = 1) -> dict:
    """The automaton of a left-to-right sequence of HMM states with loop, forward and skip transitions.

    mixtures[i] is the emission of HMM state i; loop[i], forward[i], skip[i] and exit[i] are the transition weights (costs)
    out of it (scalars are broadcast).  With repeat > 1 every HMM state stands `repeat` times in a row (RASR's state
    repetitions).  With n positions in all, the automaton has the states 0 .. n: state 0 is the start, state k >= 1 means
    "position k-1 has just been emitted".  An arc into state k emits the mixture of position k-1:
        start    -> 1           weight 0
        k (>= 1) -> k           loop[k-1]
                 -> k + 1       forward[k-1]      (k < n)
                 -> k + 2       skip[k-1]         (k + 1 < n)
    State n is final with weight exit[n-1].  Arcs are listed by ascending target, so the result is an interval graph
    (include/rasr_gmm_align.h): the device's path equals the reference aligner's."""
    mix = np.repeat(np.asarray(mixtures, dtype=np.uint32).reshape(-1), int(repeat))
    n = int(mix.shape[0])
    if n == 0:
        raise ValueError("linear_hmm_graph needs at least one HMM state")

    def per_position(w):
        w = np.asarray(w, dtype=np.float32).reshape(-1)
        return np.full(n, w[0], dtype=np.float32) if w.shape[0] == 1 else np.repeat(w, int(repeat))

    loop, forward, skip, exit = (per_position(w) for w in (loop, forward, skip, exit))
    if any(w.shape[0] != n for w in (loop, forward, skip, exit)):
        raise ValueError("loop, forward, skip and exit must be scalars or have one entry per HMM state")
    offset, target, label, weight = [0], [1], [mix[0]], [np.float32(0.0)]
    for k in range(1, n + 1):
        offset.append(len(target))
        for step, w in ((0, loop), (1, forward), (2, skip)):
            if k + step <= n:
                target.append(k + step)
                label.append(mix[k + step - 1])
                weight.append(w[k - 1])
    offset.append(len(target))
    final = np.full(n + 1, np.inf, dtype=np.float32)
    final[n] = exit[n - 1]
    return {"n_states": n + 1, "arc_offset": np.asarray(offset, dtype=np.uint32),
            "arc_target": np.asarray(target, dtype=np.uint32), "arc_mixture": np.asarray(label, dtype=np.uint32),
            "arc_weight": np.asarray(weight, dtype=np.float32), "final_weight": final, "initial_state": 0}


def batch_graphs(graphs, frame_begin, n_frames) -> dict:
    """Concatenates graphs (see the module text) into the keyword arguments of Aligner.set_segments; segment s takes the
    table columns frame_begin[s] .. frame_begin[s] + n_frames[s]."""
    state_offset = np.concatenate(([0], np.cumsum([g["n_states"] for g in graphs]))).astype(np.uint32)
    arcs = np.concatenate(([0], np.cumsum([g["arc_target"].shape[0] for g in graphs])))
    return {
        "state_offset": state_offset,
        "arc_offset": np.concatenate([np.asarray(g["arc_offset"][:-1], dtype=np.int64) + a for g, a in zip(graphs, arcs)]
                                     + [arcs[-1:]]).astype(np.uint32),
        "arc_target": np.concatenate([g["arc_target"] for g in graphs]).astype(np.uint32),
        "arc_mixture": np.concatenate([g["arc_mixture"] for g in graphs]).astype(np.uint32),
        "arc_weight": np.concatenate([g["arc_weight"] for g in graphs]).astype(np.float32),
        "final_weight": np.concatenate([g["final_weight"] for g in graphs]).astype(np.float32),
        "initial_state": np.asarray([g.get("initial_state", 0) for g in graphs], dtype=np.uint32),
        "frame_begin": np.asarray(frame_begin, dtype=np.uint32),
        "n_frames": np.asarray(n_frames, dtype=np.uint32),
    }


class Aligner:
    """gmm_aligner: all device memory for batches of up to max_segments segments, max_states states and max_arcs arcs in
    all, max_cells = the largest sum over a batch's segments of n_frames * n_states, over tables of n_mixtures rows."""

    def __init__(self, max_segments: int, max_states: int, max_arcs: int, max_cells: int, n_mixtures: int,
                 device: int = 0):
        self._lib = _capi.load_library()
        self.n_mixtures = int(n_mixtures)
        self.device = int(device)
        self.n_segments = 0
        self._h = None
        h = ctypes.c_void_p()
        _capi.check(self._lib.gmm_aligner_create(int(max_segments), int(max_states), int(max_arcs), int(max_cells),
                                                 self.n_mixtures, self.device, ctypes.byref(h)), "gmm_aligner_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gmm_aligner_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_segments(self, state_offset, arc_offset, arc_target, arc_mixture, arc_weight, final_weight, frame_begin,
                     n_frames, initial_state=None) -> None:
        """gmm_aligner_set_segments on numpy arrays (batch_graphs builds them); synchronous.  A refused call (GmmError
        with .code) leaves the previously set segments in place."""
        u32 = [None if a is None else np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
               for a in (state_offset, arc_offset, arc_target, arc_mixture, initial_state, frame_begin, n_frames)]
        f32 = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (arc_weight, final_weight)]
        so, ao, at, am, ini, fb, nf = u32
        n_segments = int(fb.shape[0])
        if so.shape[0] != n_segments + 1 or nf.shape[0] != n_segments or (ini is not None and ini.shape[0] != n_segments):
            raise ValueError("state_offset needs n_segments + 1 entries, n_frames and initial_state n_segments")
        n_states = int(so[-1]) if n_segments else 0
        if ao.shape[0] != n_states + 1 or f32[1].shape[0] != n_states:
            raise ValueError("arc_offset needs n_states + 1 entries, final_weight n_states")
        n_arcs = int(ao[-1])
        if any(a.shape[0] != n_arcs for a in (at, am, f32[0])):
            raise ValueError("arc_target, arc_mixture and arc_weight need arc_offset[-1] entries")
        g = _capi.AlignGraphs(n_segments, _ptr(so), _ptr(ao), _ptr(at), _ptr(am), _ptr(f32[0]), _ptr(ini), _ptr(f32[1]),
                              _ptr(fb), _ptr(nf))
        _capi.check(self._lib.gmm_aligner_set_segments(self._h, ctypes.byref(g)), "gmm_aligner_set_segments")
        self.n_segments = n_segments

    def align(self, scores, pruning_threshold: float = float("inf"), n_table_frames=None, out_mixture=None,
              out_state=None, out_arc=None, stream=None, search=None) -> dict:
        """Aligns the batch over `scores`, a [n_mixtures, >= n_table_frames] float32 table.

        With `search` (an AlignSearch) the call is gmm_aligner_align_search_*: every segment runs the reference's
        threshold schedule and n-best pruning inside the one call, pruning_threshold is ignored, and the result also
        holds "threshold" [n_segments] float32 (the last pass's) and "iterations" [n_segments] int32.

        A torch CUDA tensor: gmm_aligner_align_device, asynchronous on `stream` (a torch stream or a raw handle; default
        the current one); the outputs are CUDA tensors.  A numpy array: gmm_aligner_align_host, synchronous, numpy
        outputs.  Returns {"mixture", "state", "arc"}: [n_table_frames] int32 each (NONE, as -1, in every column of a
        segment without an alignment; columns of no segment keep what out_mixture / out_state / out_arc held, NONE in
        tensors allocated here, so the accumulate calls skip them),
        "score" [n_segments] float32 (FLT_MAX without an alignment) and "hypotheses" [n_segments] int32."""
        host = isinstance(scores, np.ndarray)
        if host:
            scores = np.ascontiguousarray(scores, dtype=np.float32)
            if scores.ndim != 2 or scores.shape[0] != self.n_mixtures:
                raise ValueError("scores must be [n_mixtures, >= n_table_frames]")
            kind, ptr, stride, tail = "array", _ptr, scores.shape[1], ()

            def new(n, t, fill=None):
                return np.empty(n, dtype=t) if fill is None else np.full(n, fill, dtype=t)

            def bad(t):
                return not isinstance(t, np.ndarray) or t.size < f or t.itemsize != 4 or not t.flags.c_contiguous
        else:
            import torch
            if (scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1
                    or scores.shape[0] != self.n_mixtures):
                raise ValueError("scores must be a float32 [n_mixtures, >= n_table_frames] tensor with unit column stride")
            if stream is None:
                stream = torch.cuda.current_stream(scores.device)
            s = getattr(stream, "cuda_stream", stream)
            kind, stride, tail = "tensor", int(scores.stride(0)), (ctypes.c_void_p(s) if s else None,)

            def ptr(t):
                return ctypes.c_void_p(t.data_ptr())

            def new(n, t, fill=None):
                t = getattr(torch, t)
                return (torch.empty(n, dtype=t, device=scores.device) if fill is None
                        else torch.full((n,), fill, dtype=t, device=scores.device))

            def bad(t):
                return t.numel() < f or t.element_size() != 4 or t.dtype.is_floating_point or not t.is_contiguous()
        f = int(scores.shape[1] if n_table_frames is None else n_table_frames)
        out = {}
        for k, t in (("mixture", out_mixture), ("state", out_state), ("arc", out_arc)):
            if t is None:
                t = new(f, "int32", -1)
            elif bad(t):
                raise ValueError(f"out_{k} must be a contiguous int32 / uint32 {kind} of n_table_frames entries")
            out[k] = t
        shapes = (("score", "float32"), ("hypotheses", "int32"))
        name = "gmm_aligner_align_"
        if search is not None:
            shapes += (("threshold", "float32"), ("iterations", "int32"))
            name += "search_"
            pruning = ctypes.byref(search._struct())
        else:
            pruning = float(pruning_threshold)
        out.update((k, new(self.n_segments, t)) for k, t in shapes)
        name += "host" if host else "device"
        rc = getattr(self._lib, name)(self._h, ptr(scores), f, stride, pruning, *(ptr(t) for t in out.values()), *tail)
        _capi.check(rc, name)
        return out

    def posteriors(self, scores, pruning_threshold: float = float("inf"), min_posterior: float = 0.0, max_items=None,
                   n_table_frames=None, stream=None, search=None) -> dict:
        """Baum-Welch alignment of the batch over `scores` (gmm_aligner_posteriors_*): the per-frame mixture posteriors
        as a compact item list ordered by (table column, mixture).

        With `search` (an AlignSearch) the call is gmm_aligner_posteriors_search_*: pruning_threshold is ignored, and the
        result also holds "threshold" [n_segments] float32 (the last pass's) and "iterations" [n_segments] int32.

        Returns {"frame", "mixture"} (int32) and {"weight"} (float64, holding float32 values), trimmed to the number of
        items -- as they stand pair_frame, pair_mixture and pair_weight of Estimator.accumulate_posteriors_device --,
        "column_offset" [n_table_frames + 1] int32 (CSR into the list by table column), "n_items", "score" [n_segments]
        float32 (FLT_MAX without an alignment), "hypotheses" [n_segments] int32 and "log_total" [n_segments] float64
        (DBL_MAX without an alignment).  An item is kept iff its weight > min_posterior.
        max_items is the capacity of the item arrays (default: n_table_frames * min(n_mixtures, 64)); a call that
        produces more raises GmmError with code GMM_ERR_CAPACITY and the exact count in .n_items.
        A torch CUDA tensor: the device call on `stream`; READING THE ITEM COUNT to trim the arrays IS ITS ONE
        SYNCHRONISATION with the host.  A numpy array: the host call, synchronous, numpy outputs.  The first call on a
        handle allocates the scratch of this mode."""
        host = isinstance(scores, np.ndarray)
        if host:
            scores = np.ascontiguousarray(scores, dtype=np.float32)
            if scores.ndim != 2 or scores.shape[0] != self.n_mixtures:
                raise ValueError("scores must be [n_mixtures, >= n_table_frames]")
        else:
            import torch
            if (scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1
                    or scores.shape[0] != self.n_mixtures):
                raise ValueError("scores must be a float32 [n_mixtures, >= n_table_frames] tensor with unit column stride")
        f = int(scores.shape[1] if n_table_frames is None else n_table_frames)
        cap = int(max(1, f * min(self.n_mixtures, 64)) if max_items is None else max_items)
        if cap <= 0:
            raise ValueError("max_items must be positive")
        shapes = (("frame", cap, "int32"), ("mixture", cap, "int32"), ("weight", cap, "float64"),
                  ("column_offset", f + 1, "int32"), ("n_items", 1, "int32"), ("score", self.n_segments, "float32"),
                  ("hypotheses", self.n_segments, "int32"), ("log_total", self.n_segments, "float64"))
        name = "gmm_aligner_posteriors_"
        if search is not None:
            shapes += (("threshold", self.n_segments, "float32"), ("iterations", self.n_segments, "int32"))
            name += "search_"
            pruning = ctypes.byref(search._struct())
        else:
            pruning = float(pruning_threshold)
        if host:
            out = {k: np.zeros(n, dtype=t) for k, n, t in shapes}
            rc = getattr(self._lib, name + "host")(
                self._h, _ptr(scores), f, scores.shape[1], pruning, float(min_posterior), cap,
                *(_ptr(out[k]) for k, _, _ in shapes))
            n = int(out["n_items"][0])
            try:
                _capi.check(rc, name + "host")
            except _capi.GmmError as err:
                err.n_items = n  # exact when the code is GMM_ERR_CAPACITY
                raise
        else:
            out = {k: torch.zeros(n, dtype=getattr(torch, t), device=scores.device) for k, n, t in shapes}
            if stream is None:
                stream = torch.cuda.current_stream(scores.device)
            s = getattr(stream, "cuda_stream", stream)
            rc = getattr(self._lib, name + "device")(
                self._h, ctypes.c_void_p(scores.data_ptr()), f, int(scores.stride(0)), pruning,
                float(min_posterior), cap, *(ctypes.c_void_p(out[k].data_ptr()) for k, _, _ in shapes),
                ctypes.c_void_p(s) if s else None)
            _capi.check(rc, name + "device")
            n = int(out["n_items"].item())  # the one synchronisation
            if n > cap:
                err = _capi.GmmError(f"gmm_aligner_posteriors_device: the call produces {n} items, more than max_items "
                                     f"{cap}")
                err.code, err.n_items = _capi.GMM_ERR_CAPACITY, n
                raise err
        for k in ("frame", "mixture", "weight"):
            out[k] = out[k][:n]
        out["n_items"] = n
        return out
