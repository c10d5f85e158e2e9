"""The yardstick of the device aligner, checked without a device: tests/aligner_restatement.py against brute force, its
two scan orders against each other, rasr_amd.linear_hmm_graph against the interval conditions, and the host-only graph
unit (tests/cpp/align_graph_test.cc) as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import aligner_restatement as ar
from rasr_amd.aligner import batch_graphs, linear_hmm_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _integer_table(rng, n_mixtures, n_frames):
    return rng.integers(0, 4, size=(n_mixtures, n_frames)).astype(np.float32)


def _same(a, b):
    assert np.float32(a["score"]).view(np.uint32) == np.float32(b["score"]).view(np.uint32)
    assert a["hypotheses"] == b["hypotheses"]
    assert (a["arc"] is None) == (b["arc"] is None)
    if a["arc"] is not None:
        assert np.array_equal(a["arc"], b["arc"])


def _random_small_graph(rng, n_states, n_mixtures):
    """Any graph: random arcs, back arcs and parallel arcs included, random final states."""
    arcs = [(int(rng.integers(0, n_states)), int(rng.integers(0, n_states)), int(rng.integers(0, n_mixtures)),
             float(rng.integers(0, 3))) for _ in range(int(rng.integers(1, 3 * n_states + 1)))]
    final = np.where(rng.random(n_states) < 0.5, rng.integers(0, 3, size=n_states), np.inf)
    return ar.graph_from_arcs(n_states, arcs, final, initial_state=int(rng.integers(0, n_states)))


@pytest.mark.parametrize("order", ["reference", "state"])
def test_restatement_against_brute_force(order):
    """At most 4 states and 5 frames: the score is the minimum over all enumerated paths, each summed left to right in
    f32, and the returned path attains it.  Both integer tables (ties) and real-valued ones."""
    rng = np.random.default_rng(5)
    reached = 0
    for case in range(120):
        n_states, n_frames = int(rng.integers(1, 5)), int(rng.integers(1, 6))
        g = _random_small_graph(rng, n_states, 3)
        table = _integer_table(rng, 3, n_frames) if case % 2 else (rng.random((3, n_frames)) * 4).astype(np.float32)
        r = ar.align(g, table, order=order)
        assert np.float32(r["score"]).view(np.uint32) == ar.brute_force(g, table).view(np.uint32)
        if r["arc"] is not None:
            reached += 1
            assert len(r["arc"]) == n_frames
            assert ar.path_score(g, table, r["arc"]).view(np.uint32) == np.float32(r["score"]).view(np.uint32)
            assert np.array_equal(r["mixture"], g["arc_mixture"][r["arc"]])
            assert np.array_equal(r["state"], g["arc_target"][r["arc"]])
        else:
            assert r["score"] == ar.F32_MAX
    assert 30 < reached < 120  # both outcomes are exercised


@pytest.mark.parametrize("pruning", [np.inf, 2.0, 0.0])
@pytest.mark.parametrize("parallel", [False, True])
def test_orders_agree_on_interval_graphs(pruning, parallel):
    """Integer weights and scores make exact ties frequent; on interval graphs the two orders give one path."""
    rng = np.random.default_rng(17 + int(parallel))
    ties = 0
    for _ in range(40):
        n_states, n_frames = int(rng.integers(2, 14)), int(rng.integers(1, 16))
        g = ar.random_interval_graph(rng, n_states, 5, parallel=parallel)
        assert ar.is_interval_graph(g)
        table = _integer_table(rng, 5, n_frames)
        a, b = ar.align(g, table, pruning, "reference"), ar.align(g, table, pruning, "state")
        _same(a, b)
        # ties are real: another scan rule (a strict > replace) would have found another path somewhere
        ties += a["arc"] is not None and len(set(a["arc"].tolist())) > 1
    assert ties > 5


def test_orders_differ_on_a_non_interval_graph():
    """State 0 lists its arc to state 2 BEFORE its arc to state 1, so the reference's list of frame 0 is [2, 1]; both reach
    state 3 at equal cost in frame 1.  The reference lets the later candidate win -- the one from state 1 --, the state
    order the one from state 2.  Same score, another path."""
    g = ar.graph_from_arcs(4, [(0, 2, 0, 0.0), (0, 1, 1, 0.0), (1, 3, 2, 0.0), (2, 3, 3, 0.0)], [np.inf, np.inf, np.inf, 0.0])
    assert not ar.is_interval_graph(g)
    table = np.zeros((4, 2), dtype=np.float32)
    a, b = ar.align(g, table, order="reference"), ar.align(g, table, order="state")
    assert a["score"] == b["score"] == 0.0 and a["hypotheses"] == b["hypotheses"] == 3
    assert a["state"].tolist() == [1, 3] and a["mixture"].tolist() == [1, 2]
    assert b["state"].tolist() == [2, 3] and b["mixture"].tolist() == [0, 3]


def test_pruning_and_failure_in_the_restatement():
    """A threshold of 0 keeps the frame's minima only; a segment shorter than its shortest path has no alignment."""
    g = linear_hmm_graph([0, 1, 2], 1.0, 0.0, 5.0, 0.0)
    table = np.zeros((3, 3), dtype=np.float32)
    full, tight = ar.align(g, table), ar.align(g, table, 0.0)
    assert full["state"].tolist() == [1, 2, 3] and full["score"] == 0.0 and tight["state"].tolist() == [1, 2, 3]
    assert full["hypotheses"] == 1 + 3 + 3 and tight["hypotheses"] == 3
    short = ar.align(g, table[:, :1])
    assert short["arc"] is None and short["score"] == ar.F32_MAX and short["hypotheses"] == 1


@pytest.mark.parametrize("n,repeat", [(1, 1), (2, 1), (5, 1), (3, 2), (4, 3)])
def test_linear_hmm_graph_is_an_interval_graph(n, repeat):
    rng = np.random.default_rng(n)
    mixtures = rng.integers(0, 50, size=n)
    loop, forward, skip, exit = (rng.random(n).astype(np.float32) for _ in range(4))
    g = linear_hmm_graph(mixtures, loop, forward, skip, exit, repeat)
    N = n * repeat
    assert g["n_states"] == N + 1 and g["arc_offset"].shape == (N + 2,) and g["initial_state"] == 0
    assert ar.is_interval_graph(g)
    assert np.isinf(g["final_weight"][:N]).all() and g["final_weight"][N] == exit[-1]
    # an arc into state k emits position k-1's mixture; its weight is the source position's
    positions = np.repeat(mixtures, repeat)
    assert np.array_equal(g["arc_mixture"], positions[g["arc_target"] - 1])
    source = np.repeat(np.arange(N + 1), np.diff(g["arc_offset"].astype(np.int64)))
    for kind, w in ((0, loop), (1, forward), (2, skip)):
        sel = (source >= 1) & (g["arc_target"] - source == kind)
        assert np.array_equal(g["arc_weight"][sel], np.repeat(w, repeat)[source[sel] - 1])
        assert sel.sum() == max(N - kind, 0)
    assert g["arc_target"][0] == 1 and g["arc_weight"][0] == 0.0 and g["arc_offset"][1] == 1
    # scalars are broadcast; the batch concatenation offsets the arcs
    g2 = linear_hmm_graph(mixtures, 1.0, 2.0, 3.0, 4.0, repeat)
    assert set(g2["arc_weight"].tolist()) <= {0.0, 1.0, 2.0, 3.0} and g2["final_weight"][N] == 4.0
    b = batch_graphs([g, g2], [0, 10], [3, 4])
    assert b["state_offset"].tolist() == [0, N + 1, 2 * N + 2]
    assert b["arc_offset"].shape == (2 * N + 3,) and b["arc_offset"][-1] == 2 * g["arc_target"].shape[0]
    assert np.array_equal(b["arc_offset"][N + 1:] - b["arc_offset"][N + 1], g2["arc_offset"])


def test_align_graph_unit(built):
    """tests/cpp/align_graph_test.cc: the graph validation and the incoming lists alone (built by make)."""
    r = subprocess.run([os.path.join(ROOT, "build", "tests", "align_graph_test")], capture_output=True, text=True)
    assert r.returncode == 0 and "align_graph_test: ok" in r.stdout, r.stdout + r.stderr
