"""The argument checks that the accumulate calls of Estimator, AffineTransformAccumulator and MllrAccumulator share:
`device_pairs` for the torch (device) calls, `host_pairs` for the numpy (host) calls."""
from __future__ import annotations

import ctypes

import numpy as np


def ptr(a):
    """The data pointer of a numpy array, None for None."""
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def device_pairs(frames, lists, weights, stream=None):
    """Checks a device call's tensors: frames float32 [F, >= D]; `lists` (name, int32 / uint32 tensor or None) and
    `weights` (name, float64 tensor or None), the first list giving n_pairs.  Returns (n_pairs, the raw stream handle
    or None for the null stream, the data pointers of frames, the lists and the weights in that order)."""
    import torch
    n = int(lists[0][1].numel())
    if frames.dtype != torch.float32 or frames.dim() != 2 or frames.stride(1) != 1:
        raise ValueError("frames must be a float32 [F, >= D] tensor with unit column stride")
    for name, t in lists:
        if t is not None and (t.numel() != n or t.element_size() != 4 or t.dtype.is_floating_point
                              or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int32 / uint32 tensor of n_pairs entries")
    for name, t in weights:
        if t is not None and (t.numel() != n or t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float64 tensor of n_pairs entries")
    if stream is None:
        stream = torch.cuda.current_stream(frames.device)
    s = getattr(stream, "cuda_stream", stream)
    tensors = [frames] + [t for _, t in lists] + [t for _, t in weights]
    return n, (ctypes.c_void_p(s) if s else None), [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in tensors]


def host_pairs(frames, lists, weights):
    """Converts a host call's arrays: frames to contiguous float32 [F, >= D], `lists` to uint32 and `weights` to float64
    (None stays None), all 1-d of the first list's length.  Returns (frames, the lists, the weights, n_pairs)."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    if frames.ndim != 2:
        raise ValueError("frames must be [F, >= D]")
    lists = [None if a is None else np.ascontiguousarray(a, dtype=np.uint32) for a in lists]
    weights = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in weights]
    n = lists[0].shape[0] if lists[0].ndim else -1
    if lists[0].ndim != 1 or any(a is not None and a.shape != (n,) for a in lists[1:] + weights):
        raise ValueError("the pair arrays must be 1-d arrays of one length")
    return frames, lists, weights, n
