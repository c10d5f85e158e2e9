"""The Baum-Welch contract of include/rasr_gmm_align.h (gmm_aligner_posteriors_*), restated with numpy scalars: float32
where the contract says f32, float64 np.exp / np.log1p on the exactly widened argument, every other operation one
rounded numpy scalar operation.  It follows Search::Aligner in baum-welch mode (src/Search/Aligner.cc:160-187, 206-309,
376-396, 438-452, 696-779), Fsa::posterior64 (src/Fsa/Sssp.cc:67-222), LogSemiring::collect
(src/Fsa/tRealSemiring.cc:130-146) and Alignment::combineItems .. filterWeightsGT (src/Speech/Alignment.cc:442-578),
with the two orders fixed that the reference's std::sort leaves open.  This file is the yardstick of
tests/test_aligner_posterior.py; it is UNPINNED (no compiled reference aligner stands behind it), and
tests/test_aligner_posterior_cpu.py checks it against an enumeration of all paths.

The bounds of DESIGN.md section 17 are here too (forward_bound, potential_bound, weight_bound), so that both test files
use one formula.

A graph is one segment's automaton as rasr_amd.aligner describes it (a dict of numpy arrays).
"""
import numpy as np

F32_MAX = np.float32(np.finfo(np.float32).max)
F64_MAX = np.float64(np.finfo(np.float64).max)
EPS32 = 2.0 ** -24  # half an ulp of 1.0f: the relative error of one f32 rounding
EPS64 = 2.0 ** -53


def collect32(a, b):
    """LogSemiring<f32>::collect; F32_MAX is the zero."""
    if b == F32_MAX:
        return a
    if a == F32_MAX:
        return b
    lo = b if b < a else a
    hi = b if a < b else a
    y = np.float32(np.log1p(np.exp(np.float64(np.float32(lo - hi)))))
    return np.float32(lo - y)


def extend64(potential, arc_score):
    s = np.float64(potential) + np.float64(arc_score)
    return F64_MAX if np.isinf(s) else s


def batch64(values):
    """posterior64's batch collect over the values in the order given; the zero is F64_MAX."""
    mn, at = F64_MAX, None
    for i, v in enumerate(values):
        if v <= mn:
            mn, at = v, i
    s = np.float64(0.0)
    for i, v in enumerate(values):
        if i != at:
            s = s + np.exp(mn - v)
    pot = mn - np.log1p(s)
    return pot if pot < F64_MAX else F64_MAX


def posteriors(graph, table, pruning=np.inf, min_posterior=0.0):
    """table [n_mixtures, n_frames]: this segment's columns.  Returns a dict:
    "score" (float32; F32_MAX without an alignment), "hypotheses", "has" (bool), "log_total" (float64; F64_MAX without),
    "items": per frame a list of (mixture, float32 weight), ascending mixture, the kept items only,
    "margin": per frame the smallest |score - threshold| over the reached states (inf if the threshold is not finite),
    "max_score": the largest |score| of a reached state, "max_potential": the largest |potential| below F64_MAX,
    "max_log_posterior": the largest collected log posterior below F32_MAX, "max_group": the most trellis arcs collected
    into one item, "max_items": the most items of one frame before the filter."""
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
    out = {"score": F32_MAX, "hypotheses": 0, "has": False, "log_total": F64_MAX, "items": [[] for _ in range(n_frames)],
           "margin": [], "max_score": 0.0, "max_potential": 0.0, "max_log_posterior": 0.0, "max_group": 0, "max_items": 0}
    with np.errstate(all="ignore"):
        # 1 the search (f32) and the forward potentials (f64); active[t + 1]: state -> (score, fw) after frame t
        active = [{initial: (np.float32(0.0), np.float64(0.0))}]
        arc_score = []  # per frame: arc -> f32 w + emission
        for t in range(n_frames):
            column = table[:, t]
            scores_t, cands = {}, {}
            for p in sorted(active[-1]):  # (source state, arc position) order
                score_p, fw_p = active[-1][p]
                for a in range(off[p], off[p + 1]):
                    if a not in scores_t:
                        scores_t[a] = np.float32(weight[a] + np.float32(column[label[a]]))
                    cands.setdefault(target[a], []).append((np.float32(score_p + scores_t[a]), extend64(fw_p, scores_t[a])))
            arc_score.append(scores_t)
            reached = {}
            for q, lst in cands.items():
                score = lst[0][0]
                for cand, _ in lst[1:]:
                    score = collect32(score, cand)
                reached[q] = (score, batch64([v for _, v in lst]))
                out["max_score"] = max(out["max_score"], abs(float(score)))
            minimum = F32_MAX
            for q in sorted(reached):
                if minimum > reached[q][0]:
                    minimum = reached[q][0]
            threshold = np.float32(minimum + pruning)
            out["margin"].append(min([abs(float(s) - float(threshold)) for s, _ in reached.values()] or [np.inf]))
            active.append({q: v for q, v in reached.items() if v[0] <= threshold})
            out["hypotheses"] += len(active[-1])
        # end
        result, has = F32_MAX, False
        for q in sorted(active[-1]):
            if final[q] != np.inf:
                v = np.float32(final[q] + active[-1][q][0])
                result = v if result == F32_MAX else collect32(result, v)
                has = True
        if not has:
            return out
        out["score"], out["has"] = result, True
        # 3 the backward potentials
        bw = [None] * n_frames
        bw[-1] = {q: (np.float64(final[q]) if final[q] != np.inf else F64_MAX) for q in active[-1]}

        def backward(p, t_next):
            return batch64([extend64(bw[t_next][target[a]], arc_score[t_next][a]) for a in range(off[p], off[p + 1])
                            if target[a] in active[t_next + 1]])

        for t in range(n_frames - 2, -1, -1):
            bw[t] = {p: backward(p, t + 1) for p in active[t + 1]}
        total = backward(initial, 0)
        out["log_total"] = total
        total_inv = -total
        for pots in bw + [{q: v[1] for q, v in d.items()} for d in active] + [{0: total}]:
            for v in pots.values():
                if v < F64_MAX:
                    out["max_potential"] = max(out["max_potential"], abs(float(v)))
        # 4 the items
        for t in range(n_frames):
            groups, sizes = {}, {}
            for p in sorted(active[t]):
                fw_p = active[t][p][1]
                for a in range(off[p], off[p + 1]):
                    q = target[a]
                    if q not in active[t + 1]:
                        continue
                    x = ((fw_p + np.float64(arc_score[t][a])) + bw[t][q]) + total_inv
                    lp = np.float32(x) if x < np.float64(F32_MAX) else F32_MAX
                    m = label[a]
                    groups[m] = collect32(groups[m], lp) if m in groups else lp
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


def ulp32(x):
    return float(np.spacing(np.float32(max(abs(float(x)), 1.0))))


def max_in_degree(graph):
    return int(max(np.bincount(np.asarray(graph["arc_target"], dtype=np.int64), minlength=1).max(), 1))


def forward_bound(n_frames, in_degree, max_score):
    """how far two evaluations of the f32 search that follow the contract, or one and the exact
    value, can be apart in a score after n_frames frames: per frame and candidate one arcScore add, one extension and one
    collect (three roundings inside), all at most ulp32 of the largest score; one more frame for the final collect."""
    return 3.0 * (n_frames + 1) * in_degree * ulp32(max_score)


def potential_bound(n_frames, in_degree, max_potential):
    """The same for an f64 potential: per frame and arc one extension, one exp and one addition, and the log1p and the
    subtraction of the state, each within two units of 2^-53 relative to the largest potential."""
    return 8.0 * (n_frames + 1) * (in_degree + 2) * EPS64 * max(max_potential, 1.0)


def weight_bound(n_frames, in_degree, max_potential, max_log_posterior, max_group, max_items):
    """The same for a normalised weight (all are at most 1).  An arc's log posterior: the potentials' bound, and one f32
    rounding of a value up to max_log_posterior (a last-bit difference of an f64 transcendental can move it across a
    rounding boundary: a whole ulp).  An item: max_group arcs, each collect two more such roundings and the one of
    log1p's value (at most ulp32(1)).  A weight: the item's and the minimum's error enter exp (slope at most 1), in the
    numerator and in the sum; the exp's rounding, the sum's max_items additions, the division and the product are one
    relative 2^-24 each."""
    arc = potential_bound(n_frames, in_degree, max_potential) + ulp32(max_log_posterior)
    item = max(max_group, 1) * (arc + 2.0 * ulp32(max_log_posterior) + 2.0 * EPS32)
    return 4.0 * item + (max_items + 4) * 2.0 * EPS32


def dense(result, n_mixtures):
    """The items as a [n_frames, n_mixtures] float64 table, 0 where there is none."""
    table = np.zeros((len(result["items"]), n_mixtures), dtype=np.float64)
    for t, items in enumerate(result["items"]):
        for m, w in items:
            table[t, m] = float(w)
    return table
