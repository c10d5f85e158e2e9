"""The device Baum-Welch aligner (gmm_aligner_posteriors_*, rasr_amd/csrc/gmm_kernels_align_posterior.hip) against the
restatement of its contract (tests/aligner_posterior_restatement.py).

Exact: out_hypotheses (the active marks), out_n_items, out_column_offset and the item membership, the order of the list.
The device's and numpy's f64 exp / log1p may differ in the last bit, so out_score, out_log_total and the weights are held
to the bounds of DESIGN.md section 17 (forward_bound, potential_bound, weight_bound of the restatement module: formulas of
the segment length, the in-degree and the largest log posterior), the weights on the densified [column, mixture] table; an
item may be on one side only if its weight there is within the bound.  Each test prints the measured maxima and how many
values differ in their bits at all.  The yardstick is the restatement, never the device's own output."""
import ctypes
import functools

import numpy as np
import pytest

import aligner_posterior_restatement as bw
import aligner_restatement as ar
import rasr_amd as ra
from rasr_amd import _capi
from rasr_amd.aligner import MAX_STATES_POSTERIOR, batch_graphs

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
CANARY64 = 0x5A5A5A5A5A5A5A5A
INF = np.float32(np.inf)
M = 61  # table rows


def _csr(n_states, arcs, final, initial=0):
    """graph_from_arcs for arcs already sorted by source (linear time)."""
    src = np.asarray([a[0] for a in arcs], dtype=np.int64)
    assert (np.diff(src) >= 0).all()
    return {"n_states": n_states,
            "arc_offset": np.concatenate(([0], np.cumsum(np.bincount(src, minlength=n_states)))).astype(np.uint32),
            "arc_target": np.asarray([a[1] for a in arcs], dtype=np.uint32),
            "arc_mixture": np.asarray([a[2] for a in arcs], dtype=np.uint32),
            "arc_weight": np.asarray([a[3] for a in arcs], dtype=np.float32),
            "final_weight": np.asarray(final, dtype=np.float32), "initial_state": initial}


def _fan(rng, n_states, n_mixtures=M, every_final=True):
    """State 0 reaches every state, the others run loop / forward / skip: from the first frame on all states are
    active, so every lane and every state of a lane works.  The arcs into a state emit the state's mixture, except a
    second, parallel forward arc of another mixture here and there."""
    if n_states == 1:
        return _csr(1, [(0, 0, 5, 0.75)], [0.5])
    mix = rng.integers(0, n_mixtures, size=n_states)
    w = lambda: float(rng.random() * 3)  # noqa: E731
    arcs = [(0, k, int(mix[k]), w()) for k in range(1, n_states)]
    for k in range(1, n_states):
        arcs.append((k, k, int(mix[k]), w()))
        if k + 1 < n_states:
            arcs.append((k, k + 1, int(mix[k + 1]), w()))
            if rng.random() < 0.2:
                arcs.append((k, k + 1, int(rng.integers(0, n_mixtures)), w()))
        if k + 2 < n_states:
            arcs.append((k, k + 2, int(mix[k + 2]), w()))
    final = (rng.random(n_states) * 2).astype(np.float32) if every_final else np.full(n_states, INF, dtype=np.float32)
    final[-1] = 0.25
    final[0] = INF
    return _csr(n_states, arcs, final)


def _general(rng, n_states, n_mixtures=M, density=0.5):
    """Arcs in any direction (not an interval graph), parallel arcs of equal and of different mixtures, few mixtures
    shared by many states, and states that reach no final state."""
    arcs = []
    for s in range(n_states):
        for q in rng.permutation(n_states):
            if rng.random() < density:
                m = int(rng.integers(0, min(n_mixtures, 4)))
                arcs.append((s, int(q), m, float(rng.random() * 3)))
                if rng.random() < 0.3:
                    arcs.append((s, int(q), m if rng.random() < 0.5 else int(rng.integers(0, n_mixtures)),
                                 float(rng.random() * 3)))
    final = np.full(n_states, INF, dtype=np.float32)
    final[rng.integers(0, n_states)] = rng.random()
    return _csr(n_states, arcs, final)


def _layout(n_frames, first=3, gap=2):
    begin, at = [], first
    for f in n_frames:
        begin.append(at)
        at += f + gap
    return begin, at + 1


def _table(rng, F, scale=6.0):
    t = (rng.random((M, F)) * scale).astype(np.float32)
    t.setflags(write=False)
    return t


def make_aligner(graphs, frame_begin, n_frames, n_mix=M):
    b = batch_graphs(graphs, frame_begin, n_frames)
    cells = int(sum(int(f) * g["n_states"] for f, g in zip(n_frames, graphs)))
    aligner = ra.Aligner(len(graphs), int(b["state_offset"][-1]), max(int(b["arc_offset"][-1]), 1), cells, n_mix)
    aligner.set_segments(**b)
    return aligner


def device_posteriors(gpu, aligner, n_segments, table, pruning=np.inf, min_posterior=0.0, max_items=None, stride_pad=5):
    """One gmm_aligner_posteriors_device call through the C interface over table [n_mixtures, F], held with a row
    stride of F + stride_pad; every output starts as a canary.  Returns numpy arrays, untrimmed, and the status."""
    import torch
    n_mix, F = table.shape
    cap = int(F * M if max_items is None else max_items)
    d_table = torch.full((n_mix, F + stride_pad), float("nan"), dtype=torch.float32, device=gpu)
    d_table[:, :F] = torch.from_numpy(np.array(table)).to(gpu)

    def canary(n, wide=False):
        a = np.full(n, CANARY64 if wide else CANARY, dtype=np.uint64 if wide else np.uint32)
        return torch.from_numpy(a.view(np.int64 if wide else np.int32)).to(gpu)

    outs = {"frame": canary(cap + 3), "mixture": canary(cap + 3), "weight": canary(cap + 3, True),
            "column_offset": canary(F + 2), "n_items": canary(2), "score": canary(n_segments + 1),
            "hypotheses": canary(n_segments + 1), "log_total": canary(n_segments + 1, True)}
    rc = aligner._lib.gmm_aligner_posteriors_device(
        aligner.handle, ctypes.c_void_p(d_table.data_ptr()), F, F + stride_pad, float(pruning), float(min_posterior), cap,
        *(ctypes.c_void_p(outs[k].data_ptr()) for k in ("frame", "mixture", "weight", "column_offset", "n_items", "score",
                                                         "hypotheses", "log_total")), None)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in outs.items()}
    for k in ("frame", "mixture", "column_offset", "n_items", "hypotheses"):
        out[k] = out[k].view(np.uint32)
    out["score_bits"] = out["score"].view(np.uint32)
    out["score"] = out["score"].view(np.float32)
    out["weight_bits"] = out["weight"].view(np.uint64)
    out["weight"] = out["weight"].view(np.float64)
    out["log_total_bits"] = out["log_total"].view(np.uint64)
    out["log_total"] = out["log_total"].view(np.float64)
    out["capacity"] = cap
    return out, rc


def reference(graphs, frame_begin, n_frames, table, pruning=np.inf, min_posterior=0.0):
    return [bw.posteriors(g, table[:, b:b + f], pruning, min_posterior) for g, b, f in zip(graphs, frame_begin, n_frames)]


def check(out, graphs, frame_begin, n_frames, table, refs, min_posterior=0.0, label=""):
    """The device's outputs against the restatement's per segment; everything outside them must hold its canary."""
    F, S = table.shape[1], len(graphs)
    n = int(out["n_items"][0])
    assert out["n_items"][1] == CANARY
    assert n <= out["capacity"], "the test's own capacity"
    # the list: CSR, ascending (column, mixture), f32 values, canaries behind it
    off = out["column_offset"]
    assert off[F + 1] == CANARY and off[0] == 0 and off[F] == n and (np.diff(off[:F + 1].astype(np.int64)) >= 0).all()
    frame, mixture, weight = out["frame"][:n], out["mixture"][:n], out["weight"][:n]
    assert np.array_equal(np.repeat(np.arange(F, dtype=np.uint32), np.diff(off[:F + 1].astype(np.int64))), frame)
    key = frame.astype(np.int64) * M + mixture
    assert (np.diff(key) > 0).all(), "ordered by (column, mixture), no duplicates"
    assert (mixture < M).all() and np.array_equal(weight.astype(np.float32).astype(np.float64), weight)
    assert (out["frame"][n:] == CANARY).all() and (out["mixture"][n:] == CANARY).all()
    assert (out["weight_bits"][n:] == CANARY64).all()
    assert out["score_bits"][S] == CANARY and out["hypotheses"][S] == CANARY and out["log_total_bits"][S] == CANARY64
    dev = np.zeros((F, M))
    dev[frame, mixture] = weight
    present = np.zeros((F, M), dtype=bool)
    present[frame, mixture] = True
    covered = np.zeros(F, dtype=bool)
    worst = {"weight": 0.0, "score": 0.0, "log_total": 0.0, "bits": 0}
    for s, (g, b, f, ref) in enumerate(zip(graphs, frame_begin, n_frames, refs)):
        covered[b:b + f] = True
        assert out["hypotheses"][s] == ref["hypotheses"], (s, out["hypotheses"][s], ref["hypotheses"])
        if not ref["has"]:
            assert out["score_bits"][s] == bw.F32_MAX.view(np.uint32) and out["log_total"][s] == bw.F64_MAX
            assert not present[b:b + f].any()
            continue
        d = bw.max_in_degree(g)
        b_score = bw.forward_bound(f, d, ref["max_score"])
        b_total = bw.potential_bound(f, d, ref["max_potential"])
        b_weight = bw.weight_bound(f, d, ref["max_potential"], ref["max_log_posterior"], ref["max_group"], ref["max_items"])
        e_score = abs(float(out["score"][s]) - float(ref["score"]))
        e_total = abs(out["log_total"][s] - ref["log_total"])
        want = bw.dense(ref, M)
        want_present = want != 0 if min_posterior >= 0 else None
        e_weight = np.abs(dev[b:b + f] - want).max()
        worst["bits"] += int(out["score_bits"][s] != np.float32(ref["score"]).view(np.uint32))
        worst["bits"] += int(out["log_total"][s] != ref["log_total"])
        worst["bits"] += int((dev[b:b + f] != want).sum())
        for k, e in (("score", e_score), ("log_total", e_total), ("weight", e_weight)):
            worst[k] = max(worst[k], float(e))
        assert e_score <= b_score, (s, e_score, b_score)
        assert e_total <= b_total, (s, e_total, b_total)
        assert e_weight <= b_weight, (s, e_weight, b_weight)
        if want_present is not None:
            # membership: exact, but for an item within the bound of the filter's threshold on either side
            differs = present[b:b + f] != want_present
            near = np.minimum(np.abs(dev[b:b + f] - min_posterior), np.abs(want - min_posterior)) <= b_weight
            assert not (differs & ~near).any(), s
            worst["bits"] += int(differs.sum())
    assert not present[~covered].any(), "columns of no segment are empty"
    print(f"{label} measured: weight {worst['weight']:.3e}, score {worst['score']:.3e}, log_total {worst['log_total']:.3e}; "
          f"{worst['bits']} value(s) differ in their bits; {n} items")
    return worst


def run(gpu, graphs, n_frames, seed, pruning=np.inf, min_posterior=0.0, label="", gap=2, scale=6.0):
    begin, F = _layout(n_frames, gap=gap)
    table = _table(np.random.default_rng(seed), F, scale)
    refs = reference(graphs, begin, n_frames, table, pruning, min_posterior)
    if np.isfinite(pruning):
        # no pruning decision may flip legitimately: every reached state is further from the threshold than the search
        # can be off.  Checked on the restatement alone; a seed that fails this is an error of the test's, not a skip
        for g, f, ref in zip(graphs, n_frames, refs):
            bound = bw.forward_bound(f, bw.max_in_degree(g), ref["max_score"])
            assert min(ref["margin"]) > bound, ("choose another seed", min(ref["margin"]), bound)
    aligner = make_aligner(graphs, begin, n_frames)
    out, rc = device_posteriors(gpu, aligner, len(graphs), table, pruning, min_posterior)
    assert rc == 0, _capi.load_library().gmm_last_error()
    check(out, graphs, begin, n_frames, table, refs, min_posterior, label)
    return aligner, out, refs, begin, table


# ---- shapes: the single-wave boundary, several states per lane, the limit; ragged, gaps, a padded stride ----

SHAPE_STATES = (1, 2, 127, 128, 129, 257, 600, MAX_STATES_POSTERIOR)
SHAPE_FRAMES = (4, 1, 5, 6, 5, 4, 3, 2)


@functools.lru_cache(maxsize=None)
def _shape_graphs():
    rng = np.random.default_rng(31)
    return [_fan(rng, n) for n in SHAPE_STATES]


def test_shapes_batch(gpu):
    run(gpu, _shape_graphs(), list(SHAPE_FRAMES), seed=32, label="shapes")


def test_shapes_pruned(gpu):
    graphs = _shape_graphs()[:7]
    _, out, refs, _, _ = run(gpu, graphs, list(SHAPE_FRAMES[:7]), seed=33, pruning=4.0, label="shapes pruned")
    full = reference(graphs, *_layout_frames(SHAPE_FRAMES[:7], 33))
    assert sum(r["hypotheses"] for r in refs) < sum(r["hypotheses"] for r in full), "the threshold prunes"


def _layout_frames(n_frames, seed):
    begin, F = _layout(list(n_frames))
    return begin, list(n_frames), _table(np.random.default_rng(seed), F)


def test_one_above_the_limit_is_refused(gpu):
    g = _fan(np.random.default_rng(1), MAX_STATES_POSTERIOR + 1)
    aligner = make_aligner([g], [0], [2])  # set_segments takes it: the Viterbi call can align it
    table = _table(np.random.default_rng(2), 2)
    out, rc = device_posteriors(gpu, aligner, 1, table)
    assert rc == _capi.GMM_ERR_UNSUPPORTED
    assert b"GMM_ALIGN_MAX_STATES_POSTERIOR" in _capi.load_library().gmm_last_error()
    assert out["n_items"][0] == CANARY and out["score_bits"][0] == CANARY and (out["frame"] == CANARY).all()
    import torch
    r = aligner.align(torch.from_numpy(np.array(table)).to(gpu))
    assert r["score"].cpu().numpy()[0] == ar.align(g, table, order="state")["score"]


# ---- graphs ----

@pytest.mark.parametrize("seed", [41, 42, 43])
def test_general_graphs(gpu, seed):
    """Not interval graphs; parallel arcs with equal and with different mixtures; mixtures shared by several states;
    reached states that reach no final state (one final state among many)."""
    rng = np.random.default_rng(seed)
    graphs = [_general(rng, n) for n in (3, 7, 20, 5)]
    run(gpu, graphs, [5, 6, 7, 3], seed=seed + 100, label=f"general {seed}")


@pytest.mark.parametrize("seed,pruning", [(51, 3.0), (52, 6.0), (53, 4.0)])
def test_general_graphs_pruned(gpu, seed, pruning):
    rng = np.random.default_rng(seed)
    graphs = [_general(rng, n) for n in (6, 12, 20)]
    run(gpu, graphs, [6, 5, 7], seed=seed + 100, pruning=pruning, label=f"general pruned {seed}")


def test_dead_ends(gpu):
    """0 -> 1 -> 2 (final) and 0 -> 3 -> 3: state 3 is reached in every frame and never reaches a final state; its arcs
    give no items."""
    g = _csr(4, [(0, 0, 1, 0.5), (0, 1, 2, 0.25), (0, 3, 3, 0.0), (1, 1, 2, 0.5), (1, 2, 4, 1.0), (2, 2, 4, 0.125),
                 (3, 3, 3, 0.0)], [INF, INF, 0.0, INF])
    _, out, refs, begin, _ = run(gpu, [g], [5], seed=61, label="dead ends")
    n = int(out["n_items"][0])
    assert 3 not in out["mixture"][:n] and refs[0]["hypotheses"] > 5


def test_no_alignment_leaves_neighbours_alone(gpu):
    """The middle segment's only final state is pruned on its last frame: no items, FLT_MAX, DBL_MAX; the segments
    around it are as without it."""
    rng = np.random.default_rng(71)
    lost = _csr(3, [(0, 1, 0, 0.0), (0, 2, 1, 0.0), (1, 1, 0, 0.0), (2, 2, 1, 0.0)], [INF, INF, 0.0])
    graphs = [_fan(rng, 9), lost, _fan(rng, 14)]
    begin, F = _layout([4, 3, 5])
    table = np.array(_table(rng, F))
    table[0, begin[1]:begin[1] + 3] = 0.0
    table[1, begin[1]:begin[1] + 3] = [0.0, 0.0, 9.0]
    refs = reference(graphs, begin, [4, 3, 5], table, 2.0)
    assert not refs[1]["has"] and refs[0]["has"] and refs[2]["has"]
    for g, f, ref in zip(graphs, [4, 3, 5], refs):
        assert min(ref["margin"]) > bw.forward_bound(f, bw.max_in_degree(g), ref["max_score"])
    aligner = make_aligner(graphs, begin, [4, 3, 5])
    out, rc = device_posteriors(gpu, aligner, 3, table, 2.0)
    assert rc == 0
    check(out, graphs, begin, [4, 3, 5], table, refs, label="no alignment")
    off = out["column_offset"]
    assert off[begin[1]] == off[begin[1] + 3] and off[begin[1]] > 0 and off[table.shape[1]] > off[begin[1]]


def test_composition_order_does_not_matter(gpu):
    rng = np.random.default_rng(81)
    a, b = _fan(rng, 140), _general(rng, 9)
    table = _table(rng, 20)
    outs = []
    for graphs, begin, frames in (([a, b], [1, 9], [6, 5]), ([b, a], [9, 1], [5, 6])):
        aligner = make_aligner(graphs, begin, frames)
        out, rc = device_posteriors(gpu, aligner, 2, table, 5.0)
        assert rc == 0
        outs.append(out)
    first, second = outs
    for k in ("frame", "mixture", "weight_bits", "column_offset", "n_items"):
        assert np.array_equal(first[k], second[k]), k
    for k in ("score_bits", "hypotheses", "log_total_bits"):
        assert np.array_equal(first[k][:2], second[k][1::-1]), k
    assert first["n_items"][0] > 11


@pytest.mark.parametrize("min_posterior", [0.0, 0.25])
def test_min_posterior(gpu, min_posterior):
    rng = np.random.default_rng(91)
    graphs = [_general(rng, 8), _fan(rng, 30)]
    _, out, refs, _, _ = run(gpu, graphs, [6, 5], seed=92, min_posterior=min_posterior, scale=2.0,
                             label=f"min_posterior {min_posterior}")
    n = int(out["n_items"][0])
    assert (out["weight"][:n] > min_posterior).all()
    if min_posterior:
        full = reference(graphs, *_layout([6, 5])[:1], [6, 5], _table(np.random.default_rng(92), _layout([6, 5])[1], 2.0))
        assert n < sum(len(i) for r in full for i in r["items"])


def test_max_items_one_below_the_need(gpu):
    """The device call: the count is exact, nothing is written past max_items.  The host call: GMM_ERR_CAPACITY with
    the exact count."""
    rng = np.random.default_rng(95)
    graphs = [_fan(rng, 12)]
    aligner, out, _, begin, table = run(gpu, graphs, [5], seed=96, label="max_items")
    need = int(out["n_items"][0])
    short, rc = device_posteriors(gpu, aligner, 1, table, max_items=need - 1)
    assert rc == 0 and short["n_items"][0] == need
    assert (short["frame"][need - 1:] == CANARY).all() and (short["weight_bits"][need - 1:] == CANARY64).all()
    assert np.array_equal(short["frame"][:need - 1], out["frame"][:need - 1])
    with pytest.raises(_capi.GmmError) as e:
        aligner.posteriors(np.array(table), max_items=need - 1)
    assert e.value.code == _capi.GMM_ERR_CAPACITY and e.value.n_items == need
    host = aligner.posteriors(np.array(table), max_items=need)
    assert host["n_items"] == need
    assert np.array_equal(host["weight"].view(np.uint64), out["weight_bits"][:need])
    assert np.array_equal(host["frame"].view(np.uint32), out["frame"][:need])
    assert np.array_equal(host["column_offset"].view(np.uint32), out["column_offset"][:table.shape[1] + 1])
    assert host["log_total"].view(np.uint64)[0] == out["log_total_bits"][0]


def test_python_device_call_and_repeat(gpu):
    """Aligner.posteriors on a tensor returns the trimmed list; two identical calls on one handle give identical bits."""
    import torch
    rng = np.random.default_rng(97)
    graphs = [_fan(rng, 200), _general(rng, 6)]
    aligner, out, _, begin, table = run(gpu, graphs, [5, 4], seed=98, pruning=6.0, label="repeat")
    again, rc = device_posteriors(gpu, aligner, 2, table, 6.0)
    assert rc == 0
    for k in ("frame", "mixture", "weight_bits", "column_offset", "n_items", "score_bits", "hypotheses", "log_total_bits"):
        assert np.array_equal(out[k], again[k]), k
    n = int(out["n_items"][0])
    r = aligner.posteriors(torch.from_numpy(np.array(table)).to(gpu), 6.0)
    assert r["n_items"] == n and r["frame"].shape[0] == n and r["weight"].dtype == torch.float64
    assert np.array_equal(r["weight"].cpu().numpy().view(np.uint64), out["weight_bits"][:n])
    assert np.array_equal(r["mixture"].cpu().numpy().view(np.uint32), out["mixture"][:n])
    assert np.array_equal(r["score"].cpu().numpy().view(np.uint32), out["score_bits"][:2])
    with pytest.raises(_capi.GmmError) as e:
        aligner.posteriors(torch.from_numpy(np.array(table)).to(gpu), 6.0, max_items=n - 1)
    assert e.value.code == _capi.GMM_ERR_CAPACITY and e.value.n_items == n


def test_viterbi_call_before_and_after(gpu):
    import torch
    rng = np.random.default_rng(99)
    graphs = [_fan(rng, 150), _general(rng, 10)]
    begin, F = _layout([6, 5])
    table = _table(rng, F)
    aligner = make_aligner(graphs, begin, [6, 5])
    d_table = torch.from_numpy(np.array(table)).to(gpu)
    want = [ar.align(g, table[:, b:b + f], 5.0, "state") for g, b, f in zip(graphs, begin, [6, 5])]

    def viterbi():
        r = {k: v.cpu().numpy() for k, v in aligner.align(d_table, 5.0).items()}
        for s, (b, f, ref) in enumerate(zip(begin, [6, 5], want)):
            assert r["score"][s].view(np.uint32) == np.float32(ref["score"]).view(np.uint32)
            assert r["hypotheses"][s] == ref["hypotheses"]
            assert np.array_equal(r["mixture"][b:b + f].view(np.uint32), ref["mixture"])
            assert np.array_equal(r["state"][b:b + f].view(np.uint32), ref["state"])

    viterbi()
    out, rc = device_posteriors(gpu, aligner, 2, table, 5.0)
    assert rc == 0
    check(out, graphs, begin, [6, 5], table, reference(graphs, begin, [6, 5], table, 5.0), label="between Viterbi calls")
    viterbi()


def test_single_path_gives_ones_and_the_viterbi_mixtures(gpu):
    import torch
    n = 9
    g = _csr(n + 1, [(k, k + 1, (7 * k) % M, 0.25 * k) for k in range(n)], [INF] * n + [0.5])
    aligner, out, refs, begin, table = run(gpu, [g], [n], seed=101, label="single path")
    assert int(out["n_items"][0]) == n and (out["weight"][:n] == 1.0).all()
    mixtures = aligner.align(torch.from_numpy(np.array(table)).to(gpu))["mixture"].cpu().numpy().view(np.uint32)
    assert np.array_equal(out["mixture"][:n], mixtures[begin[0]:begin[0] + n])
    assert np.array_equal(out["frame"][:n], np.arange(begin[0], begin[0] + n))
