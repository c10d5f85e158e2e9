"""The discriminative (EBW) estimator file on the host: gmm_estimator_combine_discriminative reads, adds and writes the
layout of include/rasr_gmm_estimator.h ("Discriminative training").  The files come from the restatement's writer
(tests/ebw_restatement.py); the handle's own serializer is compared with the same writer in
tests/test_estimator_discriminative.py (GPU) and tests/cpp/ebw_estimate_test.cc (host).

Tiny ragged topology: D = 5, 4 mixtures of 1, 3, 2 and 1 densities, with a pooled covariance and with one per density.
"""
import struct

import numpy as np
import pytest

import ebw_restatement as er
import rasr_amd as ra
from rasr_amd import _capi

D, COUNTS = 5, [1, 3, 2, 1]


def topology(tying):
    return ra.synthetic_mixture_set(len(COUNTS), COUNTS, D, seed=5, tying=tying)


def random_tables(ms, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal(v.shape) * 10 for k, v in er.zero_tables(ms).items()}


def code(fn):
    with pytest.raises(ra.GmmError) as err:
        fn()
    return err.value.code


@pytest.mark.parametrize("tying", ["pooled", "none"])
def test_round_trip(tying):
    ms = topology(tying)
    num, den = random_tables(ms, 1), random_tables(ms, 2)
    data = er.write_file(ms, num, den, -12.5)
    # read and written back: the same bytes
    assert ra.combine_discriminative_estimators([data]) == data
    f = er.read_file(data)
    assert f["version"] == 2 and f["dimension"] == D and f["objective"] == -12.5
    assert len(f["means"]) == 7 and len(f["covariances"]) == (1 if tying == "pooled" else 7)
    assert [len(m[0]) for m in f["mixtures"]] == COUNTS
    # the maximum-likelihood bytes are the same file without the denominator fields: sizes differ by exactly those
    n_acc = len(f["means"]) + len(f["covariances"])
    ml_size = len(data) - n_acc * (4 + 8 * D + 8) - 8 * sum(COUNTS) - 8
    assert ml_size == 8 + 8 + 4 + 4 + n_acc * (4 + 8 * D + 8) + 4 + 8 * 7 + 4 + 4 * 4 + 12 * 7


@pytest.mark.parametrize("tying", ["pooled", "none"])
def test_combine_three_files_in_order(tying):
    ms = topology(tying)
    parts = [(random_tables(ms, 10 + i), random_tables(ms, 20 + i), [1e16, 1.0, -1e16][i]) for i in range(3)]
    files = [er.write_file(ms, n, d, o) for n, d, o in parts]
    # the first file is the starting value, the others are added to it one by one
    num = {k: (parts[0][0][k] + parts[1][0][k]) + parts[2][0][k] for k in parts[0][0]}
    den = {k: (parts[0][1][k] + parts[1][1][k]) + parts[2][1][k] for k in parts[0][1]}
    obj = (1e16 + 1.0) + -1e16  # 0.0: the order shows
    assert obj != 1.0
    got = ra.combine_discriminative_estimators(files)
    assert got == er.write_file(ms, num, den, obj)
    # another file order, another rounding somewhere
    assert ra.combine_discriminative_estimators(files[::-1]) != got


def test_refusals():
    ms = topology("pooled")
    num, den = random_tables(ms, 1), random_tables(ms, 2)
    data = er.write_file(ms, num, den, 3.0)
    bad = _capi.GMM_ERR_INVALID_ARGUMENT
    # version mismatch between the files
    other = bytearray(data)
    other[8:12] = struct.pack("<I", 1)
    assert code(lambda: ra.combine_discriminative_estimators([data, bytes(other)])) == bad
    # topology mismatch: another mixture layout, and another density table
    assert code(lambda: ra.combine_discriminative_estimators(
        [data, er.write_file(topology("none"), random_tables(topology("none"), 1), random_tables(topology("none"), 2), 0.0)])) == bad
    ms2 = ra.synthetic_mixture_set(4, [1, 2, 3, 1], D, seed=5, tying="pooled")
    assert code(lambda: ra.combine_discriminative_estimators(
        [data, er.write_file(ms2, random_tables(ms2, 1), random_tables(ms2, 2), 0.0)])) == bad
    # truncation, anywhere
    for cut in (0, 7, 19, 100, len(data) - 9, len(data) - 8, len(data) - 1):
        assert code(lambda: ra.combine_discriminative_estimators([data[:cut]])) == bad
    # bytes after the objective function
    assert code(lambda: ra.combine_discriminative_estimators([data + b"\0"])) == bad
    assert code(lambda: ra.combine_discriminative_estimators([])) == bad


@pytest.mark.parametrize("tying", ["pooled", "none"])
def test_formats_are_not_interchangeable(tying):
    """A maximum-likelihood file handed to the discriminative reader is refused; gmm_estimator_combine still reads and
    writes maximum-likelihood bytes."""
    ms = topology(tying)
    num, den = random_tables(ms, 1), random_tables(ms, 2)
    f = er.read_file(er.write_file(ms, num, den, 0.0))
    ml = [b"MIXSET\0\0", struct.pack("<II", 2, D)]
    for key in ("means", "covariances"):
        ml.append(struct.pack("<I", len(f[key])))
        for s, w, _, _ in f[key]:
            ml.append(struct.pack("<I", D) + s.astype("<f8").tobytes() + struct.pack("<d", w))
    ml.append(struct.pack("<I", len(f["densities"])))
    ml += [struct.pack("<II", *d) for d in f["densities"]]
    ml.append(struct.pack("<I", len(f["mixtures"])))
    for dens, w, _ in f["mixtures"]:
        ml.append(struct.pack("<I", len(dens)))
        ml += [struct.pack("<Id", d, x) for d, x in zip(dens, w)]
    ml = b"".join(ml)
    assert ra.combine_estimators([ml]) == ml
    assert ra.combine_estimators([ml, ml]) != ml
    assert code(lambda: ra.combine_discriminative_estimators([ml])) == _capi.GMM_ERR_INVALID_ARGUMENT


def test_cpp_program():
    """tests/cpp/ebw_estimate_test.cc: the writer and the combine on the two file units alone (built by make)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([os.path.join(root, "build", "tests", "ebw_estimate_test")], capture_output=True, text=True)
    assert r.returncode == 0 and "ebw_estimate_test: ok" in r.stdout, r.stdout + r.stderr
