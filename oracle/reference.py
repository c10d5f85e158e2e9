"""TEST INFRASTRUCTURE ONLY -- runs the REFERENCE's own scorers (oracle/_ref/ref_scorers).

oracle/ref/Makefile compiles the reference's sources in place into that stand-alone executable; this
module writes a request file, starts the executable with `subprocess`, and parses its reply.  Nothing of
the reference is loaded into the calling process.  The executable exists only where the reference tree
was present at build time (or where a built one was carried to); `available()` says whether it can be
run here, and `unavailable_reason()` why not.
"""
from __future__ import annotations

import os
import platform
import struct
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
BINARY = os.path.join(_HERE, "_ref", "ref_scorers")

# registration names of src/Mm/Module.cc:84-107 ("diagonal-sum" has no registration; its class is driven directly)
KINDS = {
    "SIMD-diagonal-maximum": 0,
    "diagonal-maximum": 1,
    "diagonal-sum": 2,
    "batch-diagonal-maximum-int": 3,
    "batch-diagonal-maximum-float": 4,
    "batch-diagonal-maximum-fast": 5,
    "preselection-batch-int": 6,
    "preselection-batch-float": 7,
}
_DTYPES = {0: np.float32, 1: np.uint32, 2: np.int32, 3: np.uint8, 4: np.float64}
_reason = None


def cpu_vendor() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("vendor_id"):
                return line.split(":")[1].strip()
    except OSError:
        pass
    return platform.processor()


def unavailable_reason():
    """None where the executable runs on this host, else one line saying why it does not."""
    global _reason
    if _reason is None:
        if not os.path.exists(BINARY):
            _reason = f"{BINARY} absent (built by `make all` only where the reference tree is present)"
        else:
            try:
                p = subprocess.run([BINARY], capture_output=True, timeout=60)
                # no arguments: the usage line and status 2; anything else (loader failure, a refused
                # executable mapping, a signal) means it does not run here
                _reason = "" if p.returncode == 2 and b"usage" in p.stderr else \
                    f"{BINARY} does not run here (status {p.returncode}: {p.stderr[-200:]!r})"
            except (OSError, subprocess.SubprocessError) as e:
                _reason = f"{BINARY} does not run here ({e})"
    return _reason or None


def available() -> bool:
    return unavailable_reason() is None


def _parse_reply(path):
    raw = open(path, "rb").read()
    if raw[:4] != b"RSRP":
        raise RuntimeError("reference reply: bad magic")
    out, pos = {}, 4
    while pos < len(raw):
        (n,) = struct.unpack_from("<I", raw, pos)
        name = raw[pos + 4:pos + 4 + n].decode()
        pos += 4 + n
        code, rank = struct.unpack_from("<II", raw, pos)
        dims = struct.unpack_from(f"<{rank}I", raw, pos + 8)
        pos += 8 + 4 * rank
        dt = np.dtype(_DTYPES[code]).newbyteorder("<")
        count = int(np.prod(dims, dtype=np.int64)) if rank else 1
        a = np.frombuffer(raw, dt, count, pos).astype(_DTYPES[code]).reshape(dims)
        pos += count * dt.itemsize
        out[name] = a.copy() if rank else a.reshape(())[()]
    return out


def _run(args, reply):
    # the reference's channels: nothing on stdout but what goes wrong
    quiet = ["--*.log.channel=nil", "--*.warning.channel=stderr", "--*.error.channel=stderr",
             "--*.statistics.channel=nil", "--*.system-info.channel=nil", "--*.configuration.channel=nil",
             "--*.version.channel=nil", "--*.time.channel=nil", "--*.progress.channel=nil",
             "--*.dot.channel=nil", "--*.memory-info.channel=nil"]
    p = subprocess.run([BINARY] + quiet + args, capture_output=True, timeout=600, cwd=os.path.dirname(reply))
    if p.returncode != 0:
        raise RuntimeError(f"ref_scorers {args[-3:]}: status {p.returncode}\n{p.stdout[-2000:].decode(errors='replace')}"
                           f"\n{p.stderr[-2000:].decode(errors='replace')}")
    return _parse_reply(reply)


def score(ms, frames, kind: str, mixture_weight_scale: float = 1.0, gaussian_scale: float = 1.0,
          clusters: int = 256, select: int = 32, iterations: int = 5, backoff: float = 40000.0):
    """Run the reference scorer `kind` over `frames`; returns the reply as a dict of numpy arrays.

    Always: scores [M][F] (mixture-major, as the oracle), isv [C][D] and log_norm [C] (the reference's
    CovarianceFeatureScorerElement of every covariance, unscaled).  Assigning types add best [M][F]; the
    SIMD type raw [M][F], simd_scaling, simd_prepared_mean, simd_constant_weight, ...; the batch types
    their prepared tables (batch_*); preselection its clustering and selection (presel_*)."""
    if not available():
        raise RuntimeError(unavailable_reason())
    f = np.ascontiguousarray(frames, dtype="<f4")
    means = np.ascontiguousarray(ms.means, dtype="<f4")
    var = np.ascontiguousarray(ms.variances, dtype="<f4")
    dm = np.ascontiguousarray(ms.density_mean, dtype="<u4")
    dc = np.ascontiguousarray(ms.density_covariance, dtype="<u4")
    mo = np.ascontiguousarray(ms.mixture_offsets, dtype="<u4")
    md = np.ascontiguousarray(ms.mixture_densities, dtype="<u4")
    lw = np.ascontiguousarray(ms.mixture_log_weights, dtype="<f8")
    D = means.shape[1]
    assert f.ndim == 2 and f.shape[1] == D and var.shape[1] == D
    head = struct.pack("<4s10I", b"RSRQ", 1, KINDS[kind], D, means.shape[0], var.shape[0], dm.shape[0],
                       mo.shape[0] - 1, md.shape[0], f.shape[0], 0)
    with tempfile.TemporaryDirectory(prefix="ref_scorers_") as tmp:
        req, rep = os.path.join(tmp, "request.bin"), os.path.join(tmp, "reply.bin")
        with open(req, "wb") as o:
            o.write(head)
            for a in (means, var, dm, dc, mo, md, lw, f):
                o.write(a.tobytes())
        args = [f"--*.scorer.buffer-size={f.shape[0] + 1}",
                f"--*.scorer.mixture-weight-scale={float(mixture_weight_scale)!r}",
                f"--*.scorer.gaussian-scale={float(gaussian_scale)!r}",
                f"--*.scorer.density-clustering.clusters={int(clusters)}",
                f"--*.scorer.density-clustering.select-clusters={int(select)}",
                f"--*.scorer.density-clustering.iterations={int(iterations)}",
                f"--*.scorer.density-clustering.backoff-score={float(backoff)!r}",
                "score", req, rep]
        return _run(args, rep)


def pms_read(path: str, dimension_offset: int = 0, reduced_dimension: int = 0):
    """The reference's MixtureSet::read on its CompressedInputStream, then setOffset / setDimension as
    Mm::Module_::readMixtureSet applies them.  (good, tables): tables as oracle.pms.pms_read's."""
    if not available():
        raise RuntimeError(unavailable_reason())
    with tempfile.TemporaryDirectory(prefix="ref_scorers_") as tmp:
        rep = os.path.join(tmp, "reply.bin")
        r = _run(["pms", os.path.abspath(path), rep, str(int(dimension_offset)), str(int(reduced_dimension))], rep)
    if not int(r["good"]):
        return False, None
    D = int(r["dimension"])
    t = {k: r[k] for k in ("density_mean", "density_covariance", "mixture_offsets", "mixture_densities",
                           "mixture_log_weights")}
    t["means"] = r["means"].reshape(-1, D) if D else r["means"].reshape(0, 0)
    t["variances"] = r["variances"].reshape(-1, D) if D else r["variances"].reshape(0, 0)
    return True, t
