#!/usr/bin/env python3
"""Write tests/golden/ref/*.npz: sweep cases with the REFERENCE's own replies frozen.

The producer is oracle/_ref/ref_scorers, the reference's scorers compiled by oracle/ref/Makefile -- never
the oracle.  Each file holds the model, the frames, every reply of the case's scorer types (oracle/ref_cases.py:
FIXTURES), the reference's 1/sqrt(var) table (it depends on the CPU's rsqrtss, as in tests/golden), the CPU
vendor and `producer = "reference"`.  `--out DIR` writes a set made on another host CPU (committed as
tests/golden/ref/cpu_<vendor>/), for which a built executable is enough: no reference tree is read.
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_cases as rc  # noqa: E402
from oracle import reference as ref  # noqa: E402


# Left to the live sweep, for the size cap: the tables that are the model or the frames times 1/sqrt(var), row by
# row (every one of them is compared there); what selects, weighs and scores stays in the fixture.
BULK = ("batch_means", "batch_features", "simd_quantized_frames")


def size_cap():
    """No fixture may be larger than the largest file under tests/golden/ outside tests/golden/ref."""
    files = [p for p in glob.glob(os.path.join(ROOT, "tests", "golden", "**", "*"), recursive=True)
             if os.path.isfile(p) and os.sep + "ref" + os.sep not in p]
    return max(os.path.getsize(p) for p in files)


def main():
    if not ref.available():
        sys.exit("make_ref_golden: " + ref.unavailable_reason())
    out = os.path.join(ROOT, "tests", "golden", "ref")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(out, exist_ok=True)
    cap = size_cap()
    for name, (dimension, tying, weights, replies) in rc.FIXTURES.items():
        ms, frames, frames_float = rc.build_case(dimension, tying, weights, counts=rc.COUNTS_SMALL)
        rows = np.flatnonzero((frames.view(np.uint32) != frames_float.view(np.uint32)).any(1)).astype(np.uint32)
        arrays = dict(means=ms.means, variances=ms.variances, density_mean=ms.density_mean,
                      density_covariance=ms.density_covariance, mixture_offsets=ms.mixture_offsets,
                      mixture_densities=ms.mixture_densities, mixture_log_weights=ms.mixture_log_weights,
                      frames=frames, float_rows=rows, float_row_values=frames_float[rows],
                      cpu_vendor=np.array(ref.cpu_vendor()), producer=np.array("reference"),
                      replies=np.array([rc.reply_key(k, m, g, "")[:-1] for k, m, g in replies]))
        scalars = {}
        for kind, mws, gs in replies:
            fr = frames_float if kind in rc.FLOAT_KINDS else frames
            r = ref.score(ms, fr, kind, **rc.score_kwargs(kind, mws, gs))
            arrays.setdefault("isv", r["isv"])
            assert rc.bits_equal(arrays["isv"], r["isv"])
            for key, value in r.items():
                if key in ("isv", "kind") + BULK:
                    continue
                if np.ndim(value) == 0:  # f32 / u32 scalars, exact in f64; two zip members instead of one each
                    scalars[rc.reply_key(kind, mws, gs, key)] = float(value)
                else:
                    arrays[rc.reply_key(kind, mws, gs, key)] = value
        arrays["scalar_names"] = np.array(list(scalars.keys()))
        arrays["scalar_values"] = np.array(list(scalars.values()), np.float64)
        path = os.path.join(out, name + ".npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(f"wrote {name}: {size} bytes (cap {cap})")
        if size > cap:
            sys.exit(f"make_ref_golden: {name} is larger than the largest committed golden file")


if __name__ == "__main__":
    main()
