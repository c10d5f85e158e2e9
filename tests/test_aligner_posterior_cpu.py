"""tests/aligner_posterior_restatement.py against an enumeration of every accepting path in float64 (no GPU): the
per-(frame, mixture) posteriors, the total and the score, within the bounds of DESIGN.md section 17."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import aligner_posterior_restatement as bw  # noqa: E402
from aligner_restatement import graph_from_arcs  # noqa: E402

INF = np.inf


def enumerate_paths(graph, table):
    """(-log of the total mass, [n_frames, n_mixtures] posteriors) over all paths of table.shape[1] arcs from the initial
    state to a final state; an arc weighs float32(w + emission), as the trellis of the contract does."""
    n_frames, n_mixtures = table.shape[1], table.shape[0]
    off, target, label = graph["arc_offset"], graph["arc_target"], graph["arc_mixture"]
    paths = []

    def walk(state, arcs, cost):
        if len(arcs) == n_frames:
            if graph["final_weight"][state] != INF:
                paths.append((arcs, cost + float(graph["final_weight"][state])))
            return
        t = len(arcs)
        for a in range(int(off[state]), int(off[state + 1])):
            step = np.float32(np.float32(graph["arc_weight"][a]) + np.float32(table[label[a], t]))
            walk(int(target[a]), arcs + [a], cost + float(step))

    walk(int(graph.get("initial_state", 0)), [], 0.0)
    if not paths:
        return None, np.zeros((n_frames, n_mixtures))
    costs = np.asarray([c for _, c in paths])
    low = costs.min()
    mass = np.exp(-(costs - low))
    post = np.zeros((n_frames, n_mixtures))
    for (arcs, _), m in zip(paths, mass):
        for t, a in enumerate(arcs):
            post[t, int(label[a])] += m
    return low - np.log(mass.sum()), post / mass.sum()


def tiny_graph(rng, n_states, n_mixtures):
    """Random arcs with parallel arcs (of equal and of different mixtures) and mixtures shared between states."""
    arcs = []
    for s in range(n_states):
        for q in range(n_states):
            if rng.random() < 0.55 or q == min(s + 1, n_states - 1):
                m = int(rng.integers(0, n_mixtures))
                arcs.append((s, q, m, float(rng.random() * 3)))
                if rng.random() < 0.35:  # a parallel arc
                    arcs.append((s, q, m if rng.random() < 0.5 else int(rng.integers(0, n_mixtures)), float(rng.random() * 3)))
    final = np.full(n_states, INF, dtype=np.float32)
    final[-1] = rng.random()
    if n_states > 2 and rng.random() < 0.5:
        final[1] = rng.random() * 2
    return graph_from_arcs(n_states, arcs, final)


CASES = [(seed, n_states, n_frames) for seed, (n_states, n_frames) in
         enumerate([(1, 1), (1, 4), (2, 3), (3, 5), (4, 6), (5, 6), (5, 4), (3, 6), (4, 2), (5, 5)])]


@pytest.mark.parametrize("seed,n_states,n_frames", CASES)
def test_restatement_matches_enumeration(seed, n_states, n_frames):
    rng = np.random.default_rng(1000 + seed)
    n_mixtures = 3  # fewer mixtures than arcs: states share them
    graph = tiny_graph(rng, n_states, n_mixtures)
    table = (rng.random((n_mixtures, n_frames)) * 6).astype(np.float32)
    total, post = enumerate_paths(graph, table)
    got = bw.posteriors(graph, table)
    if total is None:
        assert not got["has"] and got["score"] == bw.F32_MAX and got["log_total"] == bw.F64_MAX
        assert all(not items for items in got["items"])
        return
    assert got["has"]
    d = bw.max_in_degree(graph)
    b_total = bw.potential_bound(n_frames, d, max(got["max_potential"], abs(total)))
    b_score = bw.forward_bound(n_frames, d, max(got["max_score"], abs(total)))
    b_weight = bw.weight_bound(n_frames, d, got["max_potential"], got["max_log_posterior"], got["max_group"],
                               got["max_items"])
    err_w = np.abs(bw.dense(got, n_mixtures) - post).max()
    print(f"log_total {abs(got['log_total'] - total):.3e} <= {b_total:.3e}; score {abs(float(got['score']) - total):.3e}"
          f" <= {b_score:.3e}; weights {err_w:.3e} <= {b_weight:.3e}")
    assert abs(got["log_total"] - total) <= b_total
    assert abs(float(got["score"]) - total) <= b_score
    assert err_w <= b_weight
    # every frame's kept weights sum to 1 within the sum's own roundings
    for items in got["items"]:
        assert abs(sum(float(w) for _, w in items) - 1.0) <= (len(items) + 4) * 2 * bw.EPS32


def test_parallel_arcs_and_shared_mixtures_are_exercised():
    """The random cases above do contain what they are meant to."""
    parallel = shared = False
    for seed, n_states, _ in CASES:
        g = tiny_graph(np.random.default_rng(1000 + seed), n_states, 3)
        pairs, by_mixture = set(), {}
        for s in range(n_states):
            for a in range(int(g["arc_offset"][s]), int(g["arc_offset"][s + 1])):
                key = (s, int(g["arc_target"][a]))
                parallel |= key in pairs
                pairs.add(key)
                by_mixture.setdefault(int(g["arc_mixture"][a]), set()).add(int(g["arc_target"][a]))
        shared |= any(len(v) > 1 for v in by_mixture.values())
    assert parallel and shared


def test_single_path_gives_weight_one():
    """A chain: one accepting path, so every frame has one item of weight exactly 1.0."""
    n = 6
    graph = graph_from_arcs(n + 1, [(k, k + 1, (3 * k) % 5, 0.25 * k) for k in range(n)],
                            [INF] * n + [0.5])
    table = (np.random.default_rng(7).random((5, n)) * 9).astype(np.float32)
    got = bw.posteriors(graph, table)
    assert got["has"] and got["hypotheses"] == n
    assert [items for items in got["items"]] == [[((3 * k) % 5, np.float32(1.0))] for k in range(n)]
    total, _ = enumerate_paths(graph, table)
    assert abs(got["log_total"] - total) <= bw.potential_bound(n, 1, abs(total))


def test_pruning_removes_states_and_reports_margins():
    """With a finite threshold fewer hypotheses survive, the margins are finite, and a threshold below every final
    state's distance leaves no alignment."""
    rng = np.random.default_rng(11)
    graph = tiny_graph(rng, 5, 3)
    table = (rng.random((3, 6)) * 6).astype(np.float32)
    full = bw.posteriors(graph, table)
    cut = bw.posteriors(graph, table, pruning=1.0)
    assert cut["hypotheses"] < full["hypotheses"]
    assert len(cut["margin"]) == 6 and all(np.isfinite(m) for m in cut["margin"])
    assert all(np.isinf(m) for m in full["margin"])
    # a chain whose only final state is pruned on the last frame by a cheaper sibling
    graph = graph_from_arcs(3, [(0, 1, 0, 0.0), (0, 2, 1, 0.0), (1, 1, 0, 0.0), (2, 2, 1, 0.0)], [INF, INF, 0.0])
    table = np.asarray([[0.0, 0.0], [0.0, 9.0]], dtype=np.float32)
    none = bw.posteriors(graph, table, pruning=1.0)
    assert not none["has"] and none["score"] == bw.F32_MAX and none["log_total"] == bw.F64_MAX
    assert none["items"] == [[], []]


def test_min_posterior_filters_without_renormalising():
    rng = np.random.default_rng(5)
    graph = tiny_graph(rng, 4, 3)
    table = (rng.random((3, 5)) * 2).astype(np.float32)
    full = bw.dense(bw.posteriors(graph, table), 3)
    cut = bw.dense(bw.posteriors(graph, table, min_posterior=0.25), 3)
    assert (full > 0).sum() > (cut > 0).sum() > 0
    assert np.array_equal(cut, np.where(full > np.float32(0.25), full, 0.0))
