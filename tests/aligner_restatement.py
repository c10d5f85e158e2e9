"""Search::Aligner in Viterbi mode with acoustic pruning (src/Search/Aligner.cc:135-158, 189-309, 376-436, 585-592),
written literally with numpy.float32 scalars: a hypothesis list, first-activation append, the >= replace, prune with
stable compaction, the final scan, the trace-back.  This file is the yardstick of tests/test_aligner.py; it is UNPINNED
(no compiled reference aligner stands behind it), and tests/test_aligner_cpu.py checks it against brute force.

    order="reference"   the reference: the hypotheses of a frame stand in first-activation order, the next frame walks them
                        in that order.
    order="state"       the library's stated scan (include/rasr_gmm_align.h): the candidates of a state arrive in
                        (source state, arc position) order -- the same walk over a list kept in ascending state order.
The two agree on interval graphs and can differ, in the path among exact ties only, elsewhere.

A graph is one segment's automaton as rasr_amd.aligner describes it (a dict of numpy arrays).
"""
import itertools

import numpy as np

F32_MAX = np.float32(np.finfo(np.float32).max)
NONE = 0xFFFFFFFF


def align(graph, table, pruning=np.inf, order="reference"):
    """Aligns table [n_mixtures, n_frames] (this segment's columns).  Returns a dict: "score" (float32; F32_MAX without
    an alignment), "hypotheses" (the sum over the frames of the survivors), and "arc" / "mixture" / "state": per frame
    the arc taken (its index in the graph's arc arrays), its mixture and its target, or None without an alignment."""
    assert order in ("reference", "state")
    off = [int(x) for x in graph["arc_offset"]]
    target = [int(x) for x in graph["arc_target"]]
    label = [int(x) for x in graph["arc_mixture"]]
    weight = [np.float32(x) for x in np.asarray(graph["arc_weight"], dtype=np.float32)]
    final = [np.float32(x) for x in np.asarray(graph["final_weight"], dtype=np.float32)]
    table = np.asarray(table, dtype=np.float32)
    pruning = np.float32(pruning)
    n_frames = table.shape[1]
    # a hypothesis: [state, score, trace (index into the previous frame's list), arc]
    frames = [[[int(graph.get("initial_state", 0)), np.float32(0.0), None, None]]]  # addStartupHypothesis
    n_hypotheses = 0
    with np.errstate(all="ignore"):
        for t in range(n_frames):
            column = [np.float32(x) for x in table[:, t]] if table.shape[0] <= 64 else table[:, t]
            cur, of_state = [], {}
            for shi, (state, score, _, _) in enumerate(frames[-1]):  # expand
                for a in range(off[state], off[state + 1]):
                    sco = np.float32(np.float32(score + weight[a]) + np.float32(column[label[a]]))
                    at = of_state.get(target[a])
                    if at is None:  # the first candidate creates the hypothesis, appended
                        of_state[target[a]] = len(cur)
                        cur.append([target[a], sco, shi, a])
                    elif cur[at][1] >= sco:  # a later equal candidate wins
                        cur[at][1:] = [sco, shi, a]
            if order == "state":
                cur.sort(key=lambda h: h[0])
            minimum = F32_MAX  # minimumScore
            for h in cur:
                if minimum > h[1]:
                    minimum = h[1]
            threshold = np.float32(minimum + pruning)
            cur = [h for h in cur if h[1] <= threshold]  # prune: survivors keep their order
            n_hypotheses += len(cur)
            frames.append(cur)
        best, best_hyp = F32_MAX, None  # getAlignmentFsaViterbi
        for shi, (state, score, _, _) in enumerate(frames[-1]):
            value = np.float32(final[state] + score)
            if value < best:
                best, best_hyp = value, shi
    out = {"score": best, "hypotheses": n_hypotheses, "arc": None, "mixture": None, "state": None}
    if best_hyp is None:
        return out
    arcs, shi = [], best_hyp
    for t in range(n_frames, 0, -1):
        arcs.append(frames[t][shi][3])
        shi = frames[t][shi][2]
    arcs.reverse()
    out["arc"] = np.asarray(arcs, dtype=np.uint32)
    out["mixture"] = np.asarray([label[a] for a in arcs], dtype=np.uint32)
    out["state"] = np.asarray([target[a] for a in arcs], dtype=np.uint32)
    return out


def path_score(graph, table, arcs):
    """The score of a path given by its arcs: ((0 + w) + e) per frame, left to right, then final_weight + score."""
    score, state = np.float32(0.0), int(graph.get("initial_state", 0))
    with np.errstate(all="ignore"):
        for t, a in enumerate(arcs):
            assert graph["arc_offset"][state] <= a < graph["arc_offset"][state + 1], "the arc does not leave the state"
            score = np.float32(np.float32(score + np.float32(graph["arc_weight"][a]))
                               + np.float32(table[graph["arc_mixture"][a], t]))
            state = int(graph["arc_target"][a])
        return np.float32(np.float32(graph["final_weight"][state]) + score)


def brute_force(graph, table):
    """The minimum of path_score over every path of table.shape[1] arcs from the initial state (small graphs only);
    F32_MAX if none is below it."""
    n_frames = table.shape[1]
    best = F32_MAX

    def walk(state, arcs):
        nonlocal best
        if len(arcs) == n_frames:
            value = path_score(graph, table, arcs)
            if value < best:
                best = value
            return
        for a in range(int(graph["arc_offset"][state]), int(graph["arc_offset"][state + 1])):
            walk(int(graph["arc_target"][a]), arcs + [a])

    walk(int(graph.get("initial_state", 0)), [])
    return best


def is_interval_graph(graph):
    """Every state's arcs by ascending target over a contiguous interval [lo, hi]; lo and hi non-decreasing over the
    states that have arcs."""
    lo_prev = hi_prev = -1
    for s in range(int(graph["n_states"])):
        targets = [int(x) for x in graph["arc_target"][int(graph["arc_offset"][s]):int(graph["arc_offset"][s + 1])]]
        if not targets:
            continue
        if targets != sorted(targets) or set(targets) != set(range(targets[0], targets[-1] + 1)):
            return False
        if targets[0] < lo_prev or targets[-1] < hi_prev:
            return False
        lo_prev, hi_prev = targets[0], targets[-1]
    return True


def graph_from_arcs(n_states, arcs, final_weight, initial_state=0):
    """A graph from (source, target, mixture, weight) tuples; the arcs of a state keep the order given."""
    by_source = [[a for a in arcs if a[0] == s] for s in range(n_states)]
    flat = list(itertools.chain.from_iterable(by_source))
    return {"n_states": n_states,
            "arc_offset": np.concatenate(([0], np.cumsum([len(b) for b in by_source]))).astype(np.uint32),
            "arc_target": np.asarray([a[1] for a in flat], dtype=np.uint32),
            "arc_mixture": np.asarray([a[2] for a in flat], dtype=np.uint32),
            "arc_weight": np.asarray([a[3] for a in flat], dtype=np.float32),
            "final_weight": np.asarray(final_weight, dtype=np.float32), "initial_state": initial_state}


def random_interval_graph(rng, n_states, n_mixtures, max_span=3, integer=True, parallel=False):
    """A random interval graph: state s reaches [lo_s, hi_s] with lo, hi non-decreasing (loops and forward jumps; with
    `parallel` some targets are reached by two arcs of different mixtures, which keeps the targets ascending)."""
    arcs, lo, hi = [], 0, 0
    for s in range(n_states):
        lo = min(max(lo, int(rng.integers(max(s - 1, 0), s + 2))), n_states - 1)
        hi = min(max(hi, lo + int(rng.integers(0, max_span + 1))), n_states - 1)
        for q in range(lo, hi + 1):
            for _ in range(2 if parallel and rng.random() < 0.3 else 1):
                w = float(rng.integers(0, 4)) if integer else float(rng.random() * 4)
                arcs.append((s, q, int(rng.integers(0, n_mixtures)), w))
    final = np.full(n_states, np.inf, dtype=np.float32)
    final[-1] = 0.0
    final[rng.integers(0, n_states, size=max(1, n_states // 8))] = rng.integers(0, 3, size=max(1, n_states // 8))
    return graph_from_arcs(n_states, arcs, final)
