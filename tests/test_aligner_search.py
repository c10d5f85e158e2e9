"""The search calls (gmm_aligner_align_search_*, gmm_aligner_posteriors_search_*; the retry loop and the n-best step of
rasr_amd/csrc/gmm_align_step.hh) against the restatement of their contract (tests/aligner_search_restatement.py).

Viterbi mode: bit for bit -- scores, thresholds, iterations, hypotheses and the three column outputs.  Baum-Welch mode:
thresholds, iterations, hypotheses, item membership, order and CSR exactly; out_score, out_log_total and the weights by
the comparison rule of tests/test_aligner_posterior.py (its check(), with the bounds of DESIGN.md section 17), because
the device's and numpy's f64 exp / log1p may differ in the last bit.  The identity tests compare the device with itself
through the fixed-threshold calls and do not depend on the restatement."""
import ctypes
import functools

import numpy as np
import pytest

import aligner_posterior_restatement as bw
import aligner_restatement as ar
import aligner_search_restatement as sr
import rasr_amd as ra
import test_aligner as ta
import test_aligner_posterior as tp
from rasr_amd import _capi
from rasr_amd.aligner import MAX_STATES, MAX_STATES_POSTERIOR, NONE, AlignSearch, batch_graphs

pytestmark = pytest.mark.gpu

CANARY = ta.CANARY
F32_MAX = float(sr.F32_MAX)
MV = ta.M  # table rows of the Viterbi tests
MP = tp.M  # of the Baum-Welch tests (tp.check's)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def make_aligner(graphs, begin, frames, n_mix):
    b = batch_graphs(graphs, begin, frames)
    cells = int(sum(int(f) * g["n_states"] for f, g in zip(frames, graphs)))
    al = ra.Aligner(len(graphs), int(b["state_offset"][-1]), max(int(b["arc_offset"][-1]), 1), cells, n_mix)
    al.set_segments(**b)
    al.arc_begin = b["arc_offset"][b["state_offset"][:-1]]
    return al


def _device_table(gpu, table, stride_pad=5):
    import torch
    n_mix, F = table.shape
    d = torch.full((n_mix, F + stride_pad), float("nan"), dtype=torch.float32, device=gpu)
    d[:, :F] = torch.from_numpy(np.array(table)).to(gpu)
    return d


def device_align(gpu, al, table, search=None, pruning=np.inf):
    """Aligner.align on the device (the search call with `search`), the column outputs starting as CANARY."""
    import torch
    F = table.shape[1]
    outs = [torch.from_numpy(np.full(F, CANARY, dtype=np.uint32).view(np.int32)).to(gpu) for _ in range(3)]
    r = al.align(_device_table(gpu, table), pruning, n_table_frames=F, out_mixture=outs[0], out_state=outs[1],
                 out_arc=outs[2], search=search)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in r.items()}
    for k in ("mixture", "state", "arc", "hypotheses", "iterations"):
        if k in out:
            out[k] = out[k].view(np.uint32)
    out["arc_begin"] = al.arc_begin
    return out


def check_align(out, graphs, begin, frames, table, refs):
    """Viterbi: every output against the restatement's, bit for bit; the columns of no segment hold CANARY."""
    ta.check(out, graphs, begin, frames, table, refs=refs)
    for s, ref in enumerate(refs):
        assert bits(out["threshold"][s]) == bits(ref["threshold"]), (s, out["threshold"][s], ref["threshold"])
        assert out["iterations"][s] == ref["iterations"], (s, out["iterations"][s], ref["iterations"])


def device_posteriors(gpu, al, n_segments, table, search=None, pruning=np.inf, min_posterior=0.0, stride_pad=5):
    """tp.device_posteriors for the search call: gmm_aligner_posteriors_search_device through the C interface, every
    output a canary first; without `search` the fixed-threshold call."""
    import torch
    if search is None:
        return tp.device_posteriors(gpu, al, n_segments, table, pruning, min_posterior, stride_pad=stride_pad)[0]
    n_mix, F = table.shape
    cap = F * MP
    d_table = _device_table(gpu, table, stride_pad)

    def canary(n, wide=False):
        a = np.full(n, tp.CANARY64 if wide else CANARY, dtype=np.uint64 if wide else np.uint32)
        return torch.from_numpy(a.view(np.int64 if wide else np.int32)).to(gpu)

    outs = {"frame": canary(cap + 3), "mixture": canary(cap + 3), "weight": canary(cap + 3, True),
            "column_offset": canary(F + 2), "n_items": canary(2), "score": canary(n_segments + 1),
            "hypotheses": canary(n_segments + 1), "log_total": canary(n_segments + 1, True),
            "threshold": canary(n_segments + 1), "iterations": canary(n_segments + 1)}
    rc = al._lib.gmm_aligner_posteriors_search_device(
        al.handle, ctypes.c_void_p(d_table.data_ptr()), F, F + stride_pad, ctypes.byref(search._struct()),
        float(min_posterior), cap, *(ctypes.c_void_p(v.data_ptr()) for v in outs.values()), None)
    assert rc == 0, _capi.load_library().gmm_last_error()
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in outs.items()}
    for k in ("frame", "mixture", "column_offset", "n_items", "hypotheses", "iterations"):
        out[k] = out[k].view(np.uint32)
    out["score_bits"], out["score"] = out["score"].view(np.uint32), out["score"].view(np.float32)
    out["weight_bits"], out["weight"] = out["weight"].view(np.uint64), out["weight"].view(np.float64)
    out["log_total_bits"], out["log_total"] = out["log_total"].view(np.uint64), out["log_total"].view(np.float64)
    out["threshold_bits"], out["threshold"] = out["threshold"].view(np.uint32), out["threshold"].view(np.float32)
    out["capacity"] = cap
    return out


def check_posteriors(out, graphs, begin, frames, table, refs, label=""):
    S = len(graphs)
    tp.check(out, graphs, begin, frames, table, refs, label=label)
    assert out["threshold_bits"][S] == CANARY and out["iterations"][S] == CANARY
    for s, ref in enumerate(refs):
        assert out["threshold_bits"][s] == bits(ref["threshold"]), (s, out["threshold"][s], ref["threshold"])
        assert out["iterations"][s] == ref["iterations"], (s, out["iterations"][s], ref["iterations"])


def same_posteriors(a, b, graphs=None):
    """Two device results: every output equal in its bits."""
    n = int(a["n_items"][0])
    assert n == int(b["n_items"][0])
    for k in ("frame", "mixture", "weight_bits"):
        assert np.array_equal(a[k][:n], b[k][:n]), k
    for k in ("column_offset", "score_bits", "hypotheses", "log_total_bits"):
        assert np.array_equal(a[k], b[k]), k


# ---- the generator of segments with known pass counts ----

def _diagonal(rng, n, extra, at, n_mix):
    """A diagonal chain of n positions over n frames (its own mixtures 0 .. n-1) and its table columns: small noise,
    and `extra` on the diagonal's emission in frame `at`: the passes with a threshold below about extra - 1 lose the
    only path to the final state."""
    g = sr.diagonal_chain(n, np.arange(n))
    columns = (rng.random((n_mix, n)) * 0.25).astype(np.float32)
    columns[at, at] += np.float32(extra)
    return g, columns


# (positions = frames, extra cost, frame): with thresholds 4, 8, 16, 32, 64 the first ok pass is 1, 2, 4, none
MIXED = ((30, 0.0, 9), (40, 6.5, 20), (37, 30.0, 11), (33, 1000.0, 7), (1, 0.0, 0))


@functools.lru_cache(maxsize=None)
def _mixed(n_mix):
    rng = np.random.default_rng(101)
    graphs, columns = zip(*(_diagonal(rng, n, extra, at, n_mix) for n, extra, at in MIXED))
    frames = [m[0] for m in MIXED]
    begin, F = ta._layout(frames)
    table = (rng.random((n_mix, F)) * 0.25).astype(np.float32)
    for b, f, c in zip(begin, frames, columns):
        table[:, b:b + f] = c
    table.setflags(write=False)
    return list(graphs), begin, frames, table


def _mixed_search(until, min_average=0.0, n_best=sr.N_BEST_OFF):
    return AlignSearch(min_pruning=4.0, max_pruning=64.0, increment_factor=2.0, min_average_hypotheses=min_average,
                       until_no_score_difference=until, n_best=n_best)


@functools.lru_cache(maxsize=None)
def _mixed_refs(mode, until, min_average, n_best=sr.N_BEST_OFF):
    graphs, begin, frames, table = _mixed(MV if mode == "viterbi" else MP)
    s = _mixed_search(until, min_average, n_best)
    one = sr.align_search if mode == "viterbi" else sr.posteriors_search
    return [one(g, table[:, b:b + f], s) for g, b, f in zip(graphs, begin, frames)]


def _mixed_counts(mode, until, min_average):
    """The restatement's results of the mixed batch, and the pass counts the test is about, asserted on them."""
    refs = _mixed_refs(mode, until, min_average)
    it = [r["iterations"] for r in refs]
    exhausted = refs[3]["threshold"] == 64.0 and it[3] == 5 and refs[3]["score"] == sr.F32_MAX
    assert exhausted, "a segment whose schedule runs out without an alignment"
    if not until and min_average == 0.0:
        assert 1 in it and 2 in it and max(it[:3]) >= 4, it
    elif until:
        assert min(it) >= 2 and max(it[:3]) >= 5, it
    else:  # the hypotheses asked for force one more pass on a segment; the one-frame segment never has them
        plain = [r["iterations"] for r in _mixed_refs(mode, until, 0.0)]
        assert any(a == b + 1 for a, b in zip(it[:3], plain)) and it[4] == 5 and refs[4]["score"] != sr.F32_MAX, (it, plain)
    return refs


@pytest.mark.parametrize("until,min_average", [(False, 0.0), (True, 0.0), (False, 6.0)])
def test_mixed_batch_viterbi(gpu, until, min_average):
    """One launch over segments of 1, 2, 4 (or 2, 3, 5 with the score-difference rule) and 5 exhausted passes."""
    graphs, begin, frames, table = _mixed(MV)
    refs = _mixed_counts("viterbi", until, min_average)
    assert refs[3]["arc"] is None and all(r["arc"] is not None for r in refs[:3])
    al = make_aligner(graphs, begin, frames, MV)
    out = device_align(gpu, al, table, _mixed_search(until, min_average))
    check_align(out, graphs, begin, frames, table, refs)
    assert (out["mixture"][begin[3]:begin[3] + frames[3]] == NONE).all()


@pytest.mark.parametrize("until,min_average", [(False, 0.0), (True, 0.0), (False, 20.0)])
def test_mixed_batch_posteriors(gpu, until, min_average):
    graphs, begin, frames, table = _mixed(MP)
    refs = _mixed_counts("posteriors", until, min_average)
    assert not refs[3]["has"] and all(r["has"] for r in refs[:3])
    al = make_aligner(graphs, begin, frames, MP)
    out = device_posteriors(gpu, al, len(graphs), table, _mixed_search(until, min_average))
    check_posteriors(out, graphs, begin, frames, table, refs, label=f"mixed until={until}")


# ---- identity with the fixed-threshold calls (no restatement) ----

@pytest.mark.parametrize("t", [5.0, F32_MAX])
def test_identity_with_the_fixed_threshold_calls(gpu, t):
    """min == max == t and the default n_best: the search calls are the fixed-threshold calls, bit for bit."""
    rng = np.random.default_rng(103)
    graphs = [tp._fan(rng, n) for n in (1, 40, 128, 129, 300)] + [ta._hmm(rng, 20, n_mixtures=MP)]
    frames = [2, 9, 6, 7, 8, 25]
    begin, F = ta._layout(frames)
    table = tp._table(rng, F)
    al = make_aligner(graphs, begin, frames, MP)
    s = AlignSearch(min_pruning=t, max_pruning=t, increment_factor=1.0)
    a, b = device_align(gpu, al, table, s), device_align(gpu, al, table, pruning=t)
    for k in ("mixture", "state", "arc", "score", "hypotheses"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert (bits(a["threshold"]) == bits(t)).all() and (a["iterations"] == 1).all()
    assert (a["hypotheses"] > 0).all()
    pa = device_posteriors(gpu, al, len(graphs), table, s)
    pb = device_posteriors(gpu, al, len(graphs), table, pruning=t)
    same_posteriors(pa, pb)
    assert (pa["threshold_bits"][:-1] == bits(t)).all() and (pa["iterations"][:-1] == 1).all()
    # a factor above 1 with min == max: one pass as well, by the schedule
    s2 = AlignSearch(min_pruning=t, max_pruning=t, increment_factor=2.0)
    c = device_align(gpu, al, table, s2)
    assert (c["iterations"] == 1).all() and np.array_equal(c["arc"], b["arc"])


def test_rerun_at_the_returned_threshold(gpu):
    """A searched result with n-best inactive: the fixed-threshold call at out_threshold[s] reproduces segment s."""
    graphs, begin, frames, table = _mixed(MP)
    al = make_aligner(graphs, begin, frames, MP)
    a = device_align(gpu, al, table, _mixed_search(True))
    pa = device_posteriors(gpu, al, len(graphs), table, _mixed_search(True))
    assert len(set(a["threshold"].tolist())) >= 3
    for t in sorted(set(a["threshold"].tolist()) | set(pa["threshold"][:-1].tolist())):
        b = device_align(gpu, al, table, pruning=t)
        pb = device_posteriors(gpu, al, len(graphs), table, pruning=t)
        for s, (bb, f) in enumerate(zip(begin, frames)):
            if a["threshold"][s] == t:
                assert bits(a["score"][s]) == bits(b["score"][s]) and a["hypotheses"][s] == b["hypotheses"][s]
                for k in ("mixture", "state", "arc"):
                    assert np.array_equal(a[k][bb:bb + f], b[k][bb:bb + f]), (s, k)
            if pa["threshold"][s] == t:
                for k in ("score_bits", "hypotheses", "log_total_bits"):
                    assert pa[k][s] == pb[k][s], (s, k)
                assert np.array_equal(np.diff(pa["column_offset"][bb:bb + f + 1].astype(np.int64)),
                                      np.diff(pb["column_offset"][bb:bb + f + 1].astype(np.int64)))
                ia = slice(int(pa["column_offset"][bb]), int(pa["column_offset"][bb + f]))
                ib = slice(int(pb["column_offset"][bb]), int(pb["column_offset"][bb + f]))
                for k in ("frame", "mixture", "weight_bits"):
                    assert np.array_equal(pa[k][ia], pb[k][ib]), (s, k)


# ---- sizes at which the kernel forms differ ----

SIZE_FRAMES = (1, 2, 40, 2, 7, 2)


def _size_search(n_best):
    return AlignSearch(min_pruning=0.5, max_pruning=8.0, increment_factor=2.0, n_best=n_best)


@functools.lru_cache(maxsize=None)
def _sizes(mode, n_best):
    """1 state, 64, 128 (the last single-wave size), 129, 300 (lanes own two states) and the mode's state limit; 1, 2 and
    40 frames; fan graphs, so every state is reached from the first frame on.  The restatement's results, once."""
    limit = MAX_STATES if mode == "viterbi" else MAX_STATES_POSTERIOR
    rng = np.random.default_rng(107)
    graphs = [tp._fan(rng, n) for n in (1, 64, 128, 129, 300, limit)]
    frames = list(SIZE_FRAMES)
    begin, F = ta._layout(frames)
    table = tp._table(rng, F, scale=3.0)
    one = sr.align_search if mode == "viterbi" else sr.posteriors_search
    refs = [one(g, table[:, b:b + f], _size_search(n_best)) for g, b, f in zip(graphs, begin, frames)]
    return graphs, begin, frames, table, refs


@pytest.mark.parametrize("n_best", [sr.N_BEST_OFF, 70])
def test_sizes_viterbi(gpu, n_best):
    graphs, begin, frames, table, refs = _sizes("viterbi", n_best)
    it = [r["iterations"] for r in refs]
    pair = [2, 4]  # 128 states (one wave) and 300 (the workgroup): side by side below, with different pass counts
    assert it[pair[0]] != it[pair[1]] and max(it) > min(it), it
    al = make_aligner(graphs, begin, frames, MP)
    out = device_align(gpu, al, table, _size_search(n_best))
    check_align(out, graphs, begin, frames, table, refs)
    if n_best == 70:  # active in the 128-state segment and at the state limit
        off = _sizes("viterbi", sr.N_BEST_OFF)[4]
        assert all(r["hypotheses"] <= 70 * f for r, f in zip(refs, frames))
        assert refs[2]["hypotheses"] < off[2]["hypotheses"] and refs[5]["hypotheses"] < off[5]["hypotheses"]
    # a single-wave and a workgroup segment side by side, alone in a batch
    al2 = make_aligner([graphs[i] for i in pair], [begin[i] for i in pair], [frames[i] for i in pair], MP)
    out2 = device_align(gpu, al2, table, _size_search(n_best))
    check_align(out2, [graphs[i] for i in pair], [begin[i] for i in pair], [frames[i] for i in pair], table,
                [refs[i] for i in pair])


@pytest.mark.parametrize("n_best", [sr.N_BEST_OFF, 70])
def test_sizes_posteriors(gpu, n_best):
    graphs, begin, frames, table, refs = _sizes("posteriors", n_best)
    pair = [1, 4]  # 64 states (one wave) and 300 (the workgroup): side by side below, with different pass counts
    assert refs[pair[0]]["iterations"] != refs[pair[1]]["iterations"], [r["iterations"] for r in refs]
    al = make_aligner(graphs, begin, frames, MP)
    out = device_posteriors(gpu, al, len(graphs), table, _size_search(n_best))
    check_posteriors(out, graphs, begin, frames, table, refs, label=f"sizes n_best={n_best}")
    if n_best == 70:
        off = _sizes("posteriors", sr.N_BEST_OFF)[4]
        assert all(r["hypotheses"] <= 70 * f for r, f in zip(refs, frames))
        assert all(r["hypotheses"] < u["hypotheses"] for r, u in zip(refs[2:], off[2:]))
    sub = [[x[i] for i in pair] for x in (graphs, begin, frames, refs)]
    al2 = make_aligner(sub[0], sub[1], sub[2], MP)
    out2 = device_posteriors(gpu, al2, 2, table, _size_search(n_best))
    check_posteriors(out2, sub[0], sub[1], sub[2], table, sub[3], label=f"pair n_best={n_best}")


# ---- n-best ----

N_BEST = (1, 2, 63, 64, 65, 400)


@functools.lru_cache(maxsize=None)
def _n_best_batch():
    """Wide interval graphs and general graphs with small-integer weights over an integer table: exact ties at the cut."""
    rng = np.random.default_rng(109)
    graphs = [ar.random_interval_graph(rng, n, 7, max_span=span, parallel=bool(i % 2))
              for i, (n, span) in enumerate(((120, 50), (300, 90), (40, 10)))]
    graphs += [ta._general_graph(rng, n, 7, fan, True) for n, fan in ((129, 6), (300, 8))]
    assert all(ar.is_interval_graph(g) for g in graphs[:3]) and not any(ar.is_interval_graph(g) for g in graphs[3:])
    frames = [9, 8, 12, 7, 6]
    begin, F = ta._layout(frames, first=1, gap=1)
    table = rng.integers(0, 4, size=(7, F)).astype(np.float32)
    table.setflags(write=False)
    return graphs, begin, frames, table


@functools.lru_cache(maxsize=None)
def _n_best_refs(mode, n_best, t_min, t_max):
    graphs, begin, frames, table = _n_best_batch()
    s = AlignSearch(min_pruning=t_min, max_pruning=t_max, increment_factor=2.0, n_best=n_best)
    if mode == "viterbi":
        return [sr.align_search(g, table[:, b:b + f], s, "reference" if i < 3 else "state")
                for i, (g, b, f) in enumerate(zip(graphs, begin, frames))]
    return [sr.posteriors_search(g, table[:, b:b + f], s) for g, b, f in zip(graphs, begin, frames)]


@pytest.mark.parametrize("n_best", N_BEST)
def test_n_best_viterbi(gpu, n_best):
    graphs, begin, frames, table = _n_best_batch()
    refs = _n_best_refs("viterbi", n_best, 6.0, 6.0)
    al = make_aligner(graphs, begin, frames, 7)
    s = AlignSearch(min_pruning=6.0, max_pruning=6.0, increment_factor=2.0, n_best=n_best)
    out = device_align(gpu, al, table, s)
    check_align(out, graphs, begin, frames, table, refs)
    assert sum(r["hypotheses"] for r in refs) <= n_best * sum(frames)
    if n_best < 400:
        assert any(r["tie_at_cut"] for r in refs), "equal scores on both sides of the cut"
        assert any(r["hypotheses"] == n_best * f for r, f in zip(refs[:2], frames)) or n_best > 2
    else:  # inactive: the fixed-threshold call
        assert max(g["n_states"] for g in graphs) <= n_best
        b = device_align(gpu, al, table, pruning=6.0)
        for k in ("mixture", "state", "arc", "score", "hypotheses"):
            assert np.array_equal(out[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("n_best", N_BEST)
def test_n_best_posteriors(gpu, n_best):
    graphs, begin, frames, table = _n_best_batch()
    refs = _n_best_refs("posteriors", n_best, 6.0, 6.0)
    wide = np.zeros((MP, table.shape[1]), dtype=np.float32)  # tp.check's table height; the graphs use rows 0 .. 6
    wide[:7] = table
    al = make_aligner(graphs, begin, frames, MP)
    s = AlignSearch(min_pruning=6.0, max_pruning=6.0, increment_factor=2.0, n_best=n_best)
    out = device_posteriors(gpu, al, len(graphs), wide, s)
    check_posteriors(out, graphs, begin, frames, wide, refs, label=f"n_best={n_best}")
    assert sum(r["hypotheses"] for r in refs) <= n_best * sum(frames)
    if n_best == 400:
        same_posteriors(out, device_posteriors(gpu, al, len(graphs), wide, pruning=6.0))


def _run_n_best(gpu, mode, refs, search):
    """The n-best batch through the mode's search call, against refs."""
    graphs, begin, frames, table = _n_best_batch()
    if mode == "viterbi":
        al = make_aligner(graphs, begin, frames, 7)
        check_align(device_align(gpu, al, table, search), graphs, begin, frames, table, refs)
        return
    wide = np.zeros((MP, table.shape[1]), dtype=np.float32)
    wide[:7] = table
    al = make_aligner(graphs, begin, frames, MP)
    out = device_posteriors(gpu, al, len(graphs), wide, search)
    check_posteriors(out, graphs, begin, frames, wide, refs, label=f"{mode} n_best={search.n_best}")


@pytest.mark.parametrize("mode", ["viterbi", "posteriors"])
def test_n_best_with_the_search_loop(gpu, mode):
    """n-best inside a growing schedule: 1, 2, 4, 8 with the score-difference rule."""
    refs = _n_best_refs(mode, 20, 1.0, 8.0)
    frames = _n_best_batch()[2]
    assert max(r["iterations"] for r in refs) >= 3
    if mode == "viterbi":
        assert any(r["tie_at_cut"] for r in refs) and len({r["iterations"] for r in refs}) >= 2
    # n-best is active: a frame of the last pass keeps exactly 20 states
    assert any(r["hypotheses"] == 20 * f for r, f in zip(refs, frames))
    _run_n_best(gpu, mode, refs, AlignSearch(min_pruning=1.0, max_pruning=8.0, increment_factor=2.0, n_best=20))


@pytest.mark.parametrize("mode", ["viterbi", "posteriors"])
def test_n_best_survivors_above_2_pow_24(gpu, mode):
    """min_pruning = max_pruning = 2^25: threshold + 1 == threshold, the demoted states stay with the new score.  In
    Baum-Welch mode only the f32 scores see it: marks, potentials and so the items are those without n-best.  There the
    collected minimum is negative, the threshold falls below 2^25, where the f32 spacing is 2 and threshold + 1 is a
    tie that rounds to even -- up, for every second threshold; so that mode takes 2^26, where the sum always rounds
    back."""
    frames = _n_best_batch()[2]
    t = float(2.0 ** 25) if mode == "viterbi" else float(2.0 ** 26)
    refs = _n_best_refs(mode, 2, t, t)
    full = _n_best_refs(mode, 400, t, t)
    assert [r["hypotheses"] for r in refs] == [r["hypotheses"] for r in full], "nothing is pruned"
    assert any(bits(r["score"]) != bits(u["score"]) for r, u in zip(refs, full)), "but the scores moved"
    assert sum(r["hypotheses"] for r in refs) > 2 * sum(frames)
    if mode == "posteriors":
        assert any(r["has"] for r in refs)
        assert all(repr(r["items"]) == repr(u["items"]) and r["log_total"] == u["log_total"] for r, u in zip(refs, full))
    _run_n_best(gpu, mode, refs, AlignSearch(min_pruning=t, max_pruning=t, increment_factor=2.0, n_best=2))


# ---- the host calls, NULL outputs, the refusals ----

def test_host_calls_equal_the_device_calls(gpu):
    graphs, begin, frames, table = _mixed(MP)
    al = make_aligner(graphs, begin, frames, MP)
    s = _mixed_search(True, n_best=9)
    dev = device_align(gpu, al, table, s)
    outs = [np.full(table.shape[1], CANARY, dtype=np.uint32) for _ in range(3)]
    padded = np.full((MP, table.shape[1] + 3), np.nan, dtype=np.float32)
    padded[:, :table.shape[1]] = table
    r = al.align(padded, n_table_frames=table.shape[1], out_mixture=outs[0], out_state=outs[1], out_arc=outs[2], search=s)
    for k in ("mixture", "state", "arc", "score", "hypotheses", "threshold", "iterations"):
        assert np.array_equal(np.asarray(r[k]).view(np.uint32), dev[k].view(np.uint32)), k
    covered = np.zeros(table.shape[1], dtype=bool)
    for b, f in zip(begin, frames):
        covered[b:b + f] = True
    assert (outs[0][~covered] == CANARY).all() and (dev["mixture"][~covered] == CANARY).all()
    pd = device_posteriors(gpu, al, len(graphs), table, s)
    ph = al.posteriors(padded, n_table_frames=table.shape[1], search=s)
    n = ph["n_items"]
    assert n == int(pd["n_items"][0]) and n > 0
    assert np.array_equal(ph["frame"].view(np.uint32), pd["frame"][:n])
    assert np.array_equal(ph["mixture"].view(np.uint32), pd["mixture"][:n])
    assert np.array_equal(ph["weight"].view(np.uint64), pd["weight_bits"][:n])
    S = len(graphs)
    assert np.array_equal(ph["column_offset"].view(np.uint32), pd["column_offset"][:-1])
    assert np.array_equal(ph["score"].view(np.uint32), pd["score_bits"][:S])
    assert np.array_equal(ph["log_total"].view(np.uint64), pd["log_total_bits"][:S])
    assert np.array_equal(ph["hypotheses"].view(np.uint32), pd["hypotheses"][:S])
    assert np.array_equal(ph["threshold"].view(np.uint32), pd["threshold_bits"][:S])
    assert np.array_equal(ph["iterations"].view(np.uint32), pd["iterations"][:S])


def test_null_outputs_and_refusals(gpu):
    import torch
    graphs, begin, frames, table = _mixed(MP)
    F, S = table.shape[1], len(graphs)
    al = make_aligner(graphs, begin, frames, MP)
    lib = _capi.load_library()
    d_table = torch.from_numpy(np.array(table)).to(gpu)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    want = device_align(gpu, al, table, _mixed_search(True))

    def fresh():
        return (torch.from_numpy(np.full(F, CANARY, dtype=np.uint32).view(np.int32)).to(gpu),
                torch.full((S,), -3.0, dtype=torch.float32, device=gpu))

    # NULL out_threshold / out_iterations, one at a time and both
    good = _mixed_search(True)._struct()
    for with_t, with_i in ((False, False), (True, False), (False, True)):
        d_out, d_score = fresh()
        d_thr = torch.full((S,), -3.0, dtype=torch.float32, device=gpu)
        d_it = torch.full((S,), -3, dtype=torch.int32, device=gpu)
        rc = lib.gmm_aligner_align_search_device(al.handle, p(d_table), F, F, ctypes.byref(good), p(d_out), None, None,
                                                 p(d_score), None, p(d_thr) if with_t else None,
                                                 p(d_it) if with_i else None, None)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want["mixture"])
        assert np.array_equal(bits(d_score.cpu().numpy()), bits(want["score"]))
        assert np.array_equal(bits(d_thr.cpu().numpy()), bits(want["threshold"])) if with_t else (d_thr == -3).all().item()
        assert np.array_equal(d_it.cpu().numpy().view(np.uint32), want["iterations"]) if with_i else (d_it == -3).all().item()
    d_n = torch.zeros(1, dtype=torch.int32, device=gpu)
    rc = lib.gmm_aligner_posteriors_search_device(al.handle, p(d_table), F, F, ctypes.byref(good), 0.0, 0, None, None,
                                                  None, None, p(d_n), None, None, None, None, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(d_n.item()) > 0

    # the refusals: nothing is written
    tiny = float(np.float32(1.0) + np.float32(2.0 ** -23))
    nan, fmin = float("nan"), float(sr.F32_MIN)
    bad = [dict(min_pruning=nan), dict(max_pruning=nan), dict(increment_factor=nan), dict(min_average_hypotheses=nan),
           dict(min_pruning=fmin / 2), dict(min_pruning=0.0), dict(min_pruning=-4.0), dict(max_pruning=float("inf")),
           dict(min_pruning=65.0), dict(increment_factor=1.0), dict(increment_factor=0.25), dict(n_best=0),
           dict(increment_factor=tiny), dict(min_pruning=fmin, max_pruning=F32_MAX, increment_factor=1.9)]
    INVALID = _capi.GMM_ERR_INVALID_ARGUMENT
    d_out, d_score = fresh()
    host_out, host_score = np.full(F, CANARY, dtype=np.uint32), np.full(S, -3.0, dtype=np.float32)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    host_table = np.array(table)
    for kw in bad + [None]:
        if kw is None:
            ref = None
        else:
            s = _mixed_search(True)
            for k, v in kw.items():
                setattr(s, k, v)
            assert sr.refused(s), kw
            ref = ctypes.byref(s._struct())
        rc = lib.gmm_aligner_align_search_device(al.handle, p(d_table), F, F, ref, p(d_out), None, None, p(d_score), None,
                                                 None, None, None)
        assert rc == INVALID, kw
        rc = lib.gmm_aligner_posteriors_search_device(al.handle, p(d_table), F, F, ref, 0.0, 0, None, None, None, None,
                                                      p(d_n), p(d_score), None, None, None, None, None)
        assert rc == INVALID, kw
        rc = lib.gmm_aligner_align_search_host(al.handle, hp(host_table), F, F, ref, hp(host_out), None, None,
                                               hp(host_score), None, None, None)
        assert rc == INVALID, kw
        rc = lib.gmm_aligner_posteriors_search_host(al.handle, hp(host_table), F, F, ref, 0.0, 0, None, None, None,
                                                    None, None, hp(host_score), None, None, None, None)
        assert rc == INVALID, kw
    # the sibling's refusals still hold, and come with a good search
    rc = lib.gmm_aligner_align_search_device(al.handle, None, F, F, ctypes.byref(good), p(d_out), None, None, None, None,
                                             None, None, None)
    assert rc == INVALID
    rc = lib.gmm_aligner_align_search_device(al.handle, p(d_table), F, F, ctypes.byref(good), None, None, None, None, None,
                                             p(d_score), p(d_out), None)
    assert rc == INVALID, "out_threshold and out_iterations alone are no output requested"
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().view(np.uint32) == CANARY).all() and (d_score.cpu().numpy() == -3.0).all()
    assert (host_out == CANARY).all() and (host_score == -3.0).all()
    # the largest schedule of a factor of 2 is taken: 254 thresholds from FLT_MIN to FLT_MAX
    s = AlignSearch(min_pruning=fmin, max_pruning=F32_MAX, increment_factor=2.0, until_no_score_difference=False)
    assert not sr.refused(s)
    out = device_align(gpu, al, table, s)
    assert (out["iterations"] >= 1).all() and (out["iterations"] <= 254).all()
    defaults = _capi.AlignSearchStruct()
    lib.gmm_default_align_search(ctypes.byref(defaults))
    d = AlignSearch()._struct()
    assert all(getattr(defaults, f) == getattr(d, f) for f, _ in _capi.AlignSearchStruct._fields_)


# ---- end to end ----

def test_chain_into_the_estimator(gpu):
    """Scorer -> searched Viterbi columns -> Estimator.accumulate_device, and searched Baum-Welch items ->
    accumulate_posteriors_device, against the same calls on the restatement's columns and items."""
    import torch
    n_mix, D, F = 40, 5, 90
    ms = ra.synthetic_mixture_set(n_mix, 1, D, seed=3)
    feats = ra.synthetic_frames(F, D, seed=4)
    sc = ra.Scorer(ms, "diagonal-sum", max_frames=F)
    d_frames = torch.from_numpy(feats).to(gpu)
    d_table = torch.empty((n_mix, F + 6), dtype=torch.float32, device=gpu)
    sc.score_device(d_frames, d_table)
    rng = np.random.default_rng(113)
    graphs = [ta._hmm(rng, 20, n_mixtures=n_mix), ta._hmm(rng, 12, n_mixtures=n_mix), ta._hmm(rng, 16, n_mixtures=n_mix)]
    begin, frames = [2, 40, 50], [30, 3, 36]  # segment 1: 11 positions in 3 frames, exhausted without an alignment
    al = make_aligner(graphs, begin, frames, n_mix)
    s = AlignSearch(min_pruning=2.0, max_pruning=4096.0, increment_factor=2.0, n_best=12)
    r = al.align(d_table, n_table_frames=F, search=s)
    rp = al.posteriors(d_table, n_table_frames=F, search=s)
    torch.cuda.synchronize()
    table = d_table.cpu().numpy()[:, :F]
    refs = [sr.align_search(g, table[:, b:b + f], s) for g, b, f in zip(graphs, begin, frames)]
    prefs = [sr.posteriors_search(g, table[:, b:b + f], s) for g, b, f in zip(graphs, begin, frames)]
    aligned = sum(f for x, f in zip(refs, frames) if x["arc"] is not None)
    assert refs[1]["arc"] is None and refs[1]["iterations"] == 12 and aligned >= 30
    assert not prefs[1]["has"] and any(x["has"] for x in prefs) and max(x["iterations"] for x in refs) >= 2
    assert np.array_equal(r["iterations"].cpu().numpy(), [x["iterations"] for x in refs])
    assert np.array_equal(rp["iterations"].cpu().numpy(), [x["iterations"] for x in prefs])
    # Viterbi: bit-equal tables
    pf, pm = [], []
    for x, b, f in zip(refs, begin, frames):
        if x["arc"] is not None:
            pf.extend(range(b, b + f))
            pm.extend(x["mixture"].tolist())
    est, want = ra.Estimator(ms, F), ra.Estimator(ms, F)
    est.accumulate_device(d_frames, torch.arange(F, dtype=torch.int32, device=gpu), r["mixture"],
                          torch.zeros(F, dtype=torch.int32, device=gpu))
    want.accumulate_device(d_frames, torch.tensor(pf, dtype=torch.int32, device=gpu),
                           torch.tensor(pm, dtype=torch.int32, device=gpu),
                           torch.zeros(len(pf), dtype=torch.int32, device=gpu))
    torch.cuda.synchronize()
    got_t, want_t = est.get(), want.get()
    for k in want_t:
        assert np.array_equal(got_t[k].view(np.uint64), want_t[k].view(np.uint64)), k
    assert want_t["entry_weights"].sum() == aligned and est.skipped == F - aligned
    # Baum-Welch: the same items; the weights within the bound of DESIGN.md section 17, so the tables within that bound
    # times the items and the largest |x|^2
    items = [(b + t, m, float(w)) for x, b in zip(prefs, begin) for t, row in enumerate(x["items"]) for m, w in row]
    n = rp["n_items"]
    assert n == len(items)
    assert np.array_equal(rp["frame"].cpu().numpy(), [i[0] for i in items])
    assert np.array_equal(rp["mixture"].cpu().numpy(), [i[1] for i in items])
    bound = max(bw.weight_bound(f, bw.max_in_degree(g), x["max_potential"], x["max_log_posterior"], x["max_group"],
                                x["max_items"]) for g, f, x in zip(graphs, frames, prefs) if x["has"])
    assert np.abs(rp["weight"].cpu().numpy() - np.asarray([i[2] for i in items])).max() <= bound
    dev_e, ref_e = ra.Estimator(ms, max_pairs=n), ra.Estimator(ms, max_pairs=n)
    dev_e.accumulate_posteriors_device(d_frames, rp["frame"], rp["mixture"], rp["weight"], scorer=sc)
    ref_e.accumulate_posteriors_device(d_frames, torch.tensor([i[0] for i in items], dtype=torch.int32, device=gpu),
                                       torch.tensor([i[1] for i in items], dtype=torch.int32, device=gpu),
                                       torch.tensor([i[2] for i in items], dtype=torch.float64, device=gpu), scorer=sc)
    torch.cuda.synchronize()
    got_t, want_t = dev_e.get(), ref_e.get()
    slack = bound * n * max(1.0, float(np.abs(feats).max()) ** 2) * 4
    for k in want_t:
        assert np.abs(got_t[k].astype(np.float64) - want_t[k].astype(np.float64)).max() <= slack, k
    assert want_t["entry_weights"].sum() > 20
