"""The search contract of include/rasr_gmm_align.h ("THE SEARCH": gmm_aligner_align_search_*,
gmm_aligner_posteriors_search_*), restated with numpy.float32 scalars: the threshold schedule and stop rule of
Search::Aligner::feed(vector) (src/Search/Aligner.cc:594-621), Core::isAlmostEqual (src/Core/Utility.hh:316-321) and the
n-best step of prune (src/Search/Aligner.cc:254-276) with the order of equal scores fixed by the state index.

A pass is the fixed-threshold contract with the n-best step in its prune: viterbi_pass is tests/aligner_restatement.py's
align, posterior_pass is tests/aligner_posterior_restatement.py's posteriors, each with that one step added
(tests/test_aligner_search_cpu.py holds them equal to the originals where n-best is inactive).  This file is the
yardstick of tests/test_aligner_search.py; like the two it builds on it is UNPINNED: the reference's Search module does
not compile stand-alone, so no compiled reference aligner stands behind it.

A graph is one segment's automaton as rasr_amd.aligner describes it (a dict of numpy arrays); a search is any object
with the fields of rasr_amd.AlignSearch.
"""
import numpy as np

import aligner_posterior_restatement as bw
import aligner_restatement as ar

F32_MAX = ar.F32_MAX
F32_MIN = np.float32(np.finfo(np.float32).tiny)
F32_EPS = np.float32(np.finfo(np.float32).eps)
MAX_ITERATIONS = 256  # GMM_ALIGN_MAX_ITERATIONS
N_BEST_OFF = 0x7FFFFFFF


def almost_equal(a, b):
    """Core::isAlmostEqual(f32, f32): every operation one f32 rounding, left to right."""
    a, b = np.float32(a), np.float32(b)
    with np.errstate(all="ignore"):
        d = np.abs(np.float32(a - b))
        e = np.float32(np.float32(np.float32(np.abs(a) + np.abs(b)) + F32_MIN) * F32_EPS)
        return bool(d < e)


def schedule(search, cap=MAX_ITERATIONS + 1):
    """The thresholds t = min, t * factor, ... <= max as float32, at most `cap` of them."""
    out, t = [], np.float32(search.min_pruning)
    factor, top = np.float32(search.increment_factor), np.float32(search.max_pruning)
    with np.errstate(all="ignore"):
        while t <= top and len(out) < cap:
            out.append(t)
            if factor <= 1:
                break
            t = np.float32(t * factor)
    return out


def refused(search):
    """The refusals of the search calls (GMM_ERR_INVALID_ARGUMENT), None passed as the struct aside."""
    f = [np.float32(search.min_pruning), np.float32(search.max_pruning), np.float32(search.increment_factor)]
    if any(np.isnan(x) for x in f) or np.isnan(search.min_average_hypotheses):
        return True
    if f[0] < F32_MIN or not np.isfinite(f[1]) or f[0] > f[1] or (f[2] <= 1 and f[0] != f[1]) or search.n_best == 0:
        return True
    return len(schedule(search)) > MAX_ITERATIONS


def run_search(search, n_frames, one_pass):
    """The loop of feed(vector).  one_pass(threshold) runs a pass and returns a result with "score" and "hypotheses".
    Returns the last pass's result with "threshold" and "iterations" added."""
    previous, iterations, result = F32_MAX, 0, None
    factor = np.float32(search.increment_factor)
    for t in schedule(search, cap=1 << 30):
        iterations += 1
        result = dict(one_pass(t))
        result["threshold"], result["iterations"] = t, iterations
        if factor <= 1:
            break
        score = np.float32(result["score"])
        ok = score != F32_MAX and float(result["hypotheses"]) / float(n_frames) >= search.min_average_hypotheses
        if ok and not search.until_no_score_difference:
            break
        if ok and iterations > 1 and almost_equal(score, previous):
            break
        previous = score
    return result


def n_best_step(states, scores, n_best, threshold):
    """prune's n-best step on the reached states of a frame (any order): with n_best below their number, every state
    behind the first n_best in (score, state index) order gets threshold + 1.  Returns the new scores, in place order."""
    scores = [np.float32(s) for s in scores]
    if n_best >= len(states):
        return scores
    # Python compares -0.0 == 0.0, as the contract does; a NaN makes the order unspecified
    order = sorted(range(len(states)), key=lambda i: (float(scores[i]), states[i]))
    with np.errstate(all="ignore"):
        demoted = np.float32(np.float32(threshold) + np.float32(1.0))
    for i in order[n_best:]:
        scores[i] = demoted
    return scores


def viterbi_pass(graph, table, pruning, n_best=N_BEST_OFF, order="reference"):
    """aligner_restatement.align with the n-best step in prune; also returns "tie_at_cut": whether some frame had equal
    scores on both sides of the n-best cut."""
    off = [int(x) for x in graph["arc_offset"]]
    target = [int(x) for x in graph["arc_target"]]
    label = [int(x) for x in graph["arc_mixture"]]
    weight = [np.float32(x) for x in np.asarray(graph["arc_weight"], dtype=np.float32)]
    final = [np.float32(x) for x in np.asarray(graph["final_weight"], dtype=np.float32)]
    table = np.asarray(table, dtype=np.float32)
    pruning = np.float32(pruning)
    n_frames = table.shape[1]
    frames = [[[int(graph.get("initial_state", 0)), np.float32(0.0), None, None]]]
    n_hypotheses, tie = 0, False
    with np.errstate(all="ignore"):
        for t in range(n_frames):
            column = table[:, t]
            cur, of_state = [], {}
            for shi, (state, score, _, _) in enumerate(frames[-1]):
                for a in range(off[state], off[state + 1]):
                    sco = np.float32(np.float32(score + weight[a]) + np.float32(column[label[a]]))
                    at = of_state.get(target[a])
                    if at is None:
                        of_state[target[a]] = len(cur)
                        cur.append([target[a], sco, shi, a])
                    elif cur[at][1] >= sco:
                        cur[at][1:] = [sco, shi, a]
            if order == "state":
                cur.sort(key=lambda h: h[0])
            minimum = F32_MAX
            for h in cur:
                if minimum > h[1]:
                    minimum = h[1]
            threshold = np.float32(minimum + pruning)
            if n_best < len(cur):
                ranked = sorted(float(h[1]) for h in cur)
                tie = tie or ranked[n_best - 1] == ranked[n_best]
                for h, s in zip(cur, n_best_step([h[0] for h in cur], [h[1] for h in cur], n_best, threshold)):
                    h[1] = s
            cur = [h for h in cur if h[1] <= threshold]
            n_hypotheses += len(cur)
            frames.append(cur)
        best, best_hyp = F32_MAX, None
        for shi, (state, score, _, _) in enumerate(frames[-1]):
            value = np.float32(final[state] + score)
            if value < best:
                best, best_hyp = value, shi
    out = {"score": best, "hypotheses": n_hypotheses, "arc": None, "mixture": None, "state": None, "tie_at_cut": tie}
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


def align_search(graph, table, search, order="reference"):
    """gmm_aligner_align_search_* on one segment: viterbi_pass's result of the last pass, "threshold", "iterations"."""
    table = np.asarray(table, dtype=np.float32)
    return run_search(search, table.shape[1], lambda t: viterbi_pass(graph, table, t, search.n_best, order))


def posterior_pass(graph, table, pruning, min_posterior=0.0, n_best=N_BEST_OFF):
    """aligner_posterior_restatement.posteriors with the n-best step in prune (the demoted score stays the state's f32
    score if it survives; the f64 potentials do not see it).  The same result dict, and "tie_at_cut"."""
    off = [int(x) for x in graph["arc_offset"]]
    target = [int(x) for x in graph["arc_target"]]
    label = [int(x) for x in graph["arc_mixture"]]
    weight = [np.float32(x) for x in np.asarray(graph["arc_weight"], dtype=np.float32)]
    final = [np.float32(x) for x in np.asarray(graph["final_weight"], dtype=np.float32)]
    table = np.asarray(table, dtype=np.float32)
    pruning = np.float32(pruning)
    min_posterior = np.float32(min_posterior)
    n_frames = table.shape[1]
    initial = int(graph.get("initial_state", 0))
    F64_MAX = bw.F64_MAX
    out = {"score": F32_MAX, "hypotheses": 0, "has": False, "log_total": F64_MAX, "items": [[] for _ in range(n_frames)],
           "margin": [], "max_score": 0.0, "max_potential": 0.0, "max_log_posterior": 0.0, "max_group": 0, "max_items": 0,
           "tie_at_cut": False}
    with np.errstate(all="ignore"):
        active = [{initial: (np.float32(0.0), np.float64(0.0))}]
        arc_score = []
        for t in range(n_frames):
            column = table[:, t]
            scores_t, cands = {}, {}
            for p in sorted(active[-1]):
                score_p, fw_p = active[-1][p]
                for a in range(off[p], off[p + 1]):
                    if a not in scores_t:
                        scores_t[a] = np.float32(weight[a] + np.float32(column[label[a]]))
                    cands.setdefault(target[a], []).append(
                        (np.float32(score_p + scores_t[a]), bw.extend64(fw_p, scores_t[a])))
            arc_score.append(scores_t)
            reached = {}
            for q, lst in cands.items():
                score = lst[0][0]
                for cand, _ in lst[1:]:
                    score = bw.collect32(score, cand)
                reached[q] = (score, bw.batch64([v for _, v in lst]))
                out["max_score"] = max(out["max_score"], abs(float(score)))
            minimum = F32_MAX
            for q in sorted(reached):
                if minimum > reached[q][0]:
                    minimum = reached[q][0]
            threshold = np.float32(minimum + pruning)
            if n_best < len(reached):
                states = sorted(reached)
                ranked = sorted(float(reached[q][0]) for q in states)
                out["tie_at_cut"] = out["tie_at_cut"] or ranked[n_best - 1] == ranked[n_best]
                for q, s in zip(states, n_best_step(states, [reached[q][0] for q in states], n_best, threshold)):
                    reached[q] = (s, reached[q][1])
            out["margin"].append(min([abs(float(s) - float(threshold)) for s, _ in reached.values()] or [np.inf]))
            active.append({q: v for q, v in reached.items() if v[0] <= threshold})
            out["hypotheses"] += len(active[-1])
        result, has = F32_MAX, False
        for q in sorted(active[-1]):
            if final[q] != np.inf:
                v = np.float32(final[q] + active[-1][q][0])
                result = v if result == F32_MAX else bw.collect32(result, v)
                has = True
        if not has:
            return out
        out["score"], out["has"] = result, True
        bwp = [None] * n_frames
        bwp[-1] = {q: (np.float64(final[q]) if final[q] != np.inf else F64_MAX) for q in active[-1]}

        def backward(p, t_next):
            return bw.batch64([bw.extend64(bwp[t_next][target[a]], arc_score[t_next][a])
                               for a in range(off[p], off[p + 1]) if target[a] in active[t_next + 1]])

        for t in range(n_frames - 2, -1, -1):
            bwp[t] = {p: backward(p, t + 1) for p in active[t + 1]}
        total = backward(initial, 0)
        out["log_total"] = total
        total_inv = -total
        for pots in bwp + [{q: v[1] for q, v in d.items()} for d in active] + [{0: total}]:
            for v in pots.values():
                if v < F64_MAX:
                    out["max_potential"] = max(out["max_potential"], abs(float(v)))
        for t in range(n_frames):
            groups, sizes = {}, {}
            for p in sorted(active[t]):
                fw_p = active[t][p][1]
                for a in range(off[p], off[p + 1]):
                    q = target[a]
                    if q not in active[t + 1]:
                        continue
                    x = ((fw_p + np.float64(arc_score[t][a])) + bwp[t][q]) + total_inv
                    lp = np.float32(x) if x < np.float64(F32_MAX) else F32_MAX
                    m = label[a]
                    groups[m] = bw.collect32(groups[m], lp) if m in groups else lp
                    sizes[m] = sizes.get(m, 0) + 1
            mixtures = sorted(groups)
            out["max_items"] = max(out["max_items"], len(mixtures))
            out["max_group"] = max([out["max_group"]] + list(sizes.values()))
            lps = []
            for m in mixtures:
                lp = groups[m]
                lp = np.float32(0.0) if lp < 0 else (F32_MAX if lp > F32_MAX else lp)
                if lp < F32_MAX:
                    out["max_log_posterior"] = max(out["max_log_posterior"], float(lp))
                lps.append(lp)
            minimum = F32_MAX
            for lp in lps:
                if minimum > lp:
                    minimum = lp
            ws = []
            for lp in lps:
                w = np.float32(lp - minimum)
                ws.append(np.float32(0.0) if np.isinf(w) else np.float32(np.exp(-np.float64(w))))
            total_w = np.float32(0.0)
            for w in ws:
                total_w = np.float32(total_w + w)
            inv = np.float32(np.float32(1.0) / total_w) if total_w != 0 else np.float32(1.0)
            for m, w in zip(mixtures, ws):
                w = np.float32(w * inv)
                if w > min_posterior:
                    out["items"][t].append((m, w))
    return out


def posteriors_search(graph, table, search, min_posterior=0.0):
    """gmm_aligner_posteriors_search_* on one segment: posterior_pass's result of the last pass, "threshold",
    "iterations"."""
    table = np.asarray(table, dtype=np.float32)
    return run_search(search, table.shape[1], lambda t: posterior_pass(graph, table, t, min_posterior, search.n_best))


def csr_graph(n_states, arcs, final_weight, initial_state=0):
    """aligner_restatement.graph_from_arcs for (source, target, mixture, weight) tuples already sorted by source, in
    linear time."""
    src = np.asarray([a[0] for a in arcs], dtype=np.int64)
    assert (np.diff(src) >= 0).all()
    return {"n_states": n_states,
            "arc_offset": np.concatenate(([0], np.cumsum(np.bincount(src, minlength=n_states)))).astype(np.uint32),
            "arc_target": np.asarray([a[1] for a in arcs], dtype=np.uint32),
            "arc_mixture": np.asarray([a[2] for a in arcs], dtype=np.uint32),
            "arc_weight": np.asarray([a[3] for a in arcs], dtype=np.float32),
            "final_weight": np.asarray(final_weight, dtype=np.float32), "initial_state": initial_state}


def diagonal_chain(n_positions, mixtures, loop=1.0, forward=0.0):
    """rasr_amd.linear_hmm_graph without skips: states 0 .. n, state k >= 1 means "position k-1 has just been emitted",
    an arc into state k emits mixtures[k-1]; the last state is final with weight 0.  Over exactly n_positions frames the
    only path to the final state takes `forward` in every frame (the diagonal)."""
    n = int(n_positions)
    arcs = [(0, 1, int(mixtures[0]), 0.0)]
    for k in range(1, n + 1):
        arcs.append((k, k, int(mixtures[k - 1]), float(loop)))
        if k < n:
            arcs.append((k, k + 1, int(mixtures[k]), float(forward)))
    final = np.full(n + 1, np.inf, dtype=np.float32)
    final[n] = 0.0
    return csr_graph(n + 1, arcs, final)
