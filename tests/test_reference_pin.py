"""The oracle held to the REFERENCE's own scorers (no GPU).

oracle/ref/Makefile compiles the reference's sources into the stand-alone oracle/_ref/ref_scorers
(oracle/reference.py runs it).  The live sweep compares every reply of that executable with the oracle's
restatement; it runs only where the executable exists and starts.  The fixtures under tests/golden/ref are
replies of that executable frozen by scripts/make_ref_golden.py; the oracle must reproduce them everywhere.

Measured on the sweep (683 model/type/scale cases, 59 of them with empty mixtures; Intel and AMD hosts alike):
every type BIT-EQUAL -- scores, best densities, raw minima, the prepared tables, clustering and selection --
the four float types included, so no ulp bound is needed and none is asserted: the float types are held to bit
equality like the integer ones.

One mismatch was found and fixed in the oracle: batch-diagonal-maximum-float on a frame holding a nan.  The
reference's `_mm_min_ps(_mm_load_ss(score), s1)` (BatchFeatureScorer.cc:226) is compiled, under its -ffast-math,
with the operands exchanged (`minps score, sum`), so a nan sum leaves the stored FLT_MAX; the oracle returned nan.

Empty mixtures, asked of the reference: it accepts them.  SIMD / batch-int / -fast / preselection-int give
0.5 * INT_MAX / s^2 resp. INT_MAX / scale_ with best density 0xFFFFFFFF, diagonal-maximum 0.5 * FLT_MAX,
diagonal-sum +inf, batch-float FLT_MAX (not halved), preselection-float the backoff score.  The oracle agrees
bit for bit, so the "empty" profile is part of the sweep.
"""
import functools
import glob
import os

import numpy as np
import pytest

import oracle
import rasr_amd as ra
from oracle import pms
from oracle import ref_cases as rc
from oracle import reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
REF_GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "ref", "*.npz")) +
                    glob.glob(os.path.join(HERE, "golden", "ref", "cpu_*", "*.npz")))
ALL_KINDS = rc.INT_KINDS + rc.FLOAT_KINDS
SWEEP_CASES = {"SIMD-diagonal-maximum": 105, "batch-diagonal-maximum-int": 35, "batch-diagonal-maximum-fast": 18,
               "preselection-batch-int": 35, "diagonal-maximum": 210, "diagonal-sum": 210,
               "batch-diagonal-maximum-float": 35, "preselection-batch-float": 35}
PMS_FILES = ["tiny_v2.pms", "tiny_v2.pms.gz", "whitespace_v2.pms", "comment_v1.pms"]


def _need_reference():
    if not ref.available():
        pytest.skip(ref.unavailable_reason())


@functools.lru_cache(maxsize=None)
def _sweep():
    """Run every case once: {kind: dict(cases, mismatches [(case, key, ulp)], max_ulp)}, and the isv mismatches."""
    stats = {k: dict(cases=0, mismatches=[], max_ulp=0) for k in ALL_KINDS}
    isv_bad = []
    for profile, dims, tyings in (("full", rc.DIMENSIONS, rc.TYINGS), ("small", rc.DIMENSIONS, rc.TYINGS),
                                  ("empty", (39, 7, 45), rc.TYINGS)):
        for d in dims:
            for tying in tyings:
                for weights in rc.WEIGHTS:
                    if profile == "empty" and weights == "uniform":
                        continue  # log(1 / 0) for the empty mixtures' (absent) weights: nothing to draw
                    ms, frames, frames_float = rc.build_case(d, tying, weights, counts=rc.PROFILES[profile])
                    isv_checked = False
                    for kind in rc.kinds_for(d, tying):
                        fr = frames_float if kind in rc.FLOAT_KINDS else frames
                        for mws, gs in (rc.SCALES if kind in rc.SCALED_KINDS else rc.SCALES[:1]):
                            kw = rc.score_kwargs(kind, mws, gs)
                            if kind.startswith("preselection") and profile == "empty":
                                kw.update(clusters=4, select=2)
                            r = ref.score(ms, fr, kind, **kw)
                            o = rc.oracle_reply(ms, fr, kind, **kw)
                            case = (profile, d, tying, weights, mws, gs)
                            st = stats[kind]
                            st["cases"] += 1
                            if not isv_checked:
                                isv_checked = True
                                if not rc.bits_equal(rc.isv_table(ms), r["isv"]):
                                    isv_bad.append(case)
                            assert set(o) == set(r) - {"kind"}, (kind, set(o) ^ set(r))  # every key of the reply
                            for key, value in o.items():
                                if not rc.bits_equal(value, r[key]):
                                    u = rc.ulp_distance(value, r[key]) if np.asarray(value).dtype.kind == "f" else -1
                                    st["mismatches"].append((case, key, u))
                                    if key == "scores":
                                        st["max_ulp"] = max(st["max_ulp"], u)
    return stats, isv_bad


def test_live_sweep_covers_the_issue():
    _need_reference()
    stats, isv_bad = _sweep()
    total = sum(s["cases"] for s in stats.values())
    print(f"\nreference pin: {total} cases on a {ref.cpu_vendor()} host")
    for kind in ALL_KINDS:
        s = stats[kind]
        assert s["cases"] > 0
        verdict = "bit-equal" if not s["mismatches"] else f"{len(s['mismatches'])} mismatches, max {s['max_ulp']} ulp"
        print(f"  {kind:32s} {s['cases']:4d} cases  {verdict}")
    # the count the documents quote: a change of the sweep changes it here first
    assert {k: stats[k]["cases"] for k in ALL_KINDS} == SWEEP_CASES and total == 683
    assert not isv_bad, f"1/sqrt(var) differs from the reference's: {isv_bad[:3]}"


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_live_sweep_bit_equal(kind):
    """Integer types: scores, raw minima, best densities, the four prepared SIMD tables, the batch tables, the
    clustering and the selection.  Float types: the restatement claims the reference's operation order under the
    reference's flags, and the sweep found it bit-equal (see the module docstring), so the same is asserted."""
    _need_reference()
    s = _sweep()[0][kind]
    assert s["cases"] > 0
    assert not s["mismatches"], f"{kind}: {len(s['mismatches'])} replies differ, first {s['mismatches'][:4]}"


@pytest.mark.parametrize("name", PMS_FILES)
@pytest.mark.parametrize("offset,reduced", [(0, 0), (1, 2), (0, 6)])
def test_pms_reader_matches_reference(built, name, offset, reduced):
    """The reference's MixtureSet::read (through its CompressedInputStream) against oracle/pms_istream.cc and the
    product's rasr_amd/csrc/host/MixtureSetFile.cc: all tables equal, bit for bit."""
    _need_reference()
    path = os.path.join(HERE, "golden", "pms", name)
    good, t = ref.pms_read(path, offset, reduced)
    status, o = pms.pms_read(path, offset, reduced)
    assert good and status == pms.OK
    got = ra.read_mixture_set(path, offset, reduced)
    for key, value in t.items():
        assert value.shape == o[key].shape and value.tobytes() == o[key].tobytes(), key
        assert value.tobytes() == getattr(got, key).tobytes(), key


# ---------------------------------------------------------------------------------------------------------
# fixtures made by the reference executable: run everywhere, no executable needed
# ---------------------------------------------------------------------------------------------------------
def load_fixture(path):
    """(ms, frames, frames_float, replies {(kind, mws, gs): {key: array}}, z)"""
    z = np.load(path, allow_pickle=False)
    ms = ra.MixtureSet(z["means"], z["variances"], z["density_mean"], z["density_covariance"], z["mixture_offsets"],
                       z["mixture_densities"], z["mixture_log_weights"])
    frames = z["frames"]
    frames_float = frames.copy()
    frames_float[z["float_rows"]] = z["float_row_values"]
    replies = {}
    for tag in z["replies"]:
        kind, mws, gs = str(tag).split("@")
        replies[(kind, float(mws), float(gs))] = {}
    for name in list(z.files) + [str(n) for n in z["scalar_names"]]:
        parts = name.split("@")
        if len(parts) == 4:
            scalar = dict(zip((str(n) for n in z["scalar_names"]), z["scalar_values"]))
            value = z[name] if name in z.files else scalar[name]
            replies[(parts[0], float(parts[1]), float(parts[2]))][parts[3]] = value
    return ms, frames, frames_float, replies, z


def same_rsqrt_or_skip(ms, z):
    """tests/test_golden.py's rule: a fixture binds only where this CPU's rsqrtss gives the fixture's table."""
    if not rc.bits_equal(rc.isv_table(ms), z["isv"]):
        pytest.skip(f"host rsqrtss differs from the fixture's 1/sqrt(var) table `isv` ({z['cpu_vendor']})")


def test_ref_fixtures_present_and_made_by_the_reference():
    assert len(REF_GOLDEN) >= 8
    kinds, tyings = set(), set()
    for path in REF_GOLDEN:
        z = np.load(path, allow_pickle=False)
        assert str(z["producer"]) == "reference", path
        kinds |= {str(t).split("@")[0] for t in z["replies"]}
        tyings.add("pooled" if z["variances"].shape[0] == 1 else
                   "none" if z["variances"].shape[0] == z["density_mean"].shape[0] else "mixture-specific")
        assert 8 <= z["mixture_offsets"].shape[0] - 1 <= 12 and z["frames"].shape[0] == 64
    assert kinds == set(ALL_KINDS) and tyings == set(rc.TYINGS)


@pytest.mark.parametrize("path", REF_GOLDEN, ids=lambda p: os.path.relpath(p, os.path.join(HERE, "golden", "ref")))
def test_oracle_reproduces_ref_fixture(path):
    ms, frames, frames_float, replies, z = load_fixture(path)
    same_rsqrt_or_skip(ms, z)
    assert replies
    for (kind, mws, gs), r in replies.items():
        fr = frames_float if kind in rc.FLOAT_KINDS else frames
        o = rc.oracle_reply(ms, fr, kind, **rc.score_kwargs(kind, mws, gs))
        checked = 0
        for key, value in r.items():
            if key in o:
                assert rc.bits_equal(np.asarray(o[key]), np.asarray(value, dtype=np.asarray(o[key]).dtype)), (kind, key)
                checked += 1
        assert checked >= 1 and "scores" in r
