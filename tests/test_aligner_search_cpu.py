"""The yardstick of the search calls, checked without a device: the schedule and stop rule of
tests/aligner_search_restatement.py on hand-made score sequences, almost_equal on hand-computed pairs, the n-best step
against a straightforward sort, and the two passes against the restatements they extend where n-best is inactive.
(The refusals of the C calls need a handle, so they are in tests/test_aligner_search.py.)"""
import types

import numpy as np
import pytest

import aligner_posterior_restatement as bw
import aligner_restatement as ar
import aligner_search_restatement as sr

F32_MAX = sr.F32_MAX


def search(**kw):
    d = dict(min_pruning=50.0, max_pruning=float(F32_MAX), increment_factor=2.0, min_average_hypotheses=0.0,
             until_no_score_difference=True, n_best=sr.N_BEST_OFF)
    d.update(kw)
    return types.SimpleNamespace(**d)


def replay(s, passes, n_frames=10):
    """run_search over a hand-made list of (score, hypotheses) per pass; returns the result and the thresholds asked."""
    asked = []

    def one_pass(t):
        asked.append(float(t))
        score, hyp = passes[len(asked) - 1]
        return {"score": np.float32(score), "hypotheses": hyp}

    return sr.run_search(s, n_frames, one_pass), asked


def test_stops_at_the_first_pass_without_score_difference():
    r, asked = replay(search(until_no_score_difference=False), [(12.5, 30)])
    assert r["iterations"] == 1 and asked == [50.0] and r["threshold"] == 50.0


def test_never_fewer_than_two_passes_with_score_difference():
    r, asked = replay(search(), [(12.5, 30), (12.5, 40)])
    assert r["iterations"] == 2 and asked == [50.0, 100.0] and r["threshold"] == np.float32(100.0)
    # a changed score asks for one more; FLT_MAX (no final state) is never ok, equal to the previous or not
    r, asked = replay(search(), [(F32_MAX, 3), (F32_MAX, 5), (13.0, 30), (12.5, 40), (12.5, 41)])
    assert r["iterations"] == 5 and asked == [50.0, 100.0, 200.0, 400.0, 800.0] and r["hypotheses"] == 41


def test_min_average_hypotheses_retry():
    # 10 frames: 39 hypotheses are 3.9 a frame, below 4; 40 are enough
    r, _ = replay(search(until_no_score_difference=False, min_average_hypotheses=4.0), [(7.0, 39), (7.0, 40)])
    assert r["iterations"] == 2
    r, _ = replay(search(min_average_hypotheses=4.0), [(7.0, 39), (7.0, 39), (7.0, 40), (7.0, 44)])
    assert r["iterations"] == 3, "the pass before the first ok one still sets `previous`"


def test_exhaustion():
    s = search(min_pruning=4.0, max_pruning=64.0)
    r, asked = replay(s, [(F32_MAX, 1)] * 5)
    assert asked == [4.0, 8.0, 16.0, 32.0, 64.0] and r["iterations"] == 5 and r["threshold"] == 64.0
    assert r["score"] == F32_MAX
    # max between two thresholds: 4, 8, 16
    assert replay(search(min_pruning=4.0, max_pruning=31.0), [(F32_MAX, 1)] * 3)[1] == [4.0, 8.0, 16.0]


def test_factor_at_most_one_runs_one_pass():
    for factor in (1.0, 0.5, -2.0):
        r, asked = replay(search(min_pruning=7.0, max_pruning=7.0, increment_factor=factor), [(F32_MAX, 0)])
        assert r["iterations"] == 1 and asked == [7.0]


def test_schedule_and_refusals():
    assert len(sr.schedule(search(min_pruning=float(sr.F32_MIN), max_pruning=float(F32_MAX)))) == 254
    assert not sr.refused(search(min_pruning=float(sr.F32_MIN)))
    assert not sr.refused(search()) and not sr.refused(search(min_pruning=3.0, max_pruning=3.0, increment_factor=1.0))
    tiny = float(np.float32(1.0) + np.float32(2.0 ** -23))
    assert sr.refused(search(increment_factor=tiny)), "far more than 256 thresholds"
    assert not sr.refused(search(min_pruning=50.0, max_pruning=50.001, increment_factor=tiny))
    for kw in (dict(min_pruning=np.nan), dict(max_pruning=np.nan), dict(increment_factor=np.nan),
               dict(min_average_hypotheses=np.nan), dict(min_pruning=0.0), dict(min_pruning=float(sr.F32_MIN) / 2),
               dict(min_pruning=-1.0), dict(max_pruning=np.inf), dict(min_pruning=51.0, max_pruning=50.0),
               dict(increment_factor=1.0), dict(increment_factor=0.5), dict(n_best=0)):
        assert sr.refused(search(**kw)), kw


def test_almost_equal():
    """Hand-computed: e = ((|a| + |b|) + FLT_MIN) * 2^-23 in f32.
    a = b = 1: d = 0 < 2^-22.  a = 1, b = 1 + 2^-23: d = 2^-23, e = (2 + 2^-23) * 2^-23 > 2^-22 > d: true.
    a = 1, b = 1 + 2^-21: d = 2^-21, e just above 2^-22: false.  a = b = 0: d = 0 < FLT_MIN * 2^-23 (a subnormal): true.
    a = 1000, b = 1000.0001 (in f32 1000 + 2^-13): d = 2^-13 = 1.22e-4 against e = 2000 * 2^-23 = 2.38e-4: true;
    b = 1000.001: d = 9.8e-4: false.
    FLT_MAX against FLT_MAX: d = 0 and |a| + |b| overflows, e = inf * 2^-23 = inf, so the formula (and the reference's
    code) gives 0 < inf, TRUE -- not the "inf < inf" one might expect; the stop rule never asks, FLT_MAX is not ok.
    +inf against +inf: d = inf - inf = NaN, false."""
    one = np.float32(1.0)
    assert sr.almost_equal(one, one)
    assert sr.almost_equal(one, one + np.float32(2.0 ** -23))
    assert not sr.almost_equal(one, one + np.float32(2.0 ** -21))
    assert sr.almost_equal(0.0, 0.0)
    assert sr.almost_equal(1000.0, np.float32(1000.0001)) and not sr.almost_equal(1000.0, 1000.001)
    assert not sr.almost_equal(-1.0, 1.0)
    assert sr.almost_equal(F32_MAX, F32_MAX)
    assert not sr.almost_equal(np.inf, np.inf)


def _plain_n_best(states, scores, n_best, threshold):
    """The n_best smallest (score, state) pairs stay, by a full sort of pairs."""
    keep = set(sorted(zip([float(s) for s in scores], states))[:n_best])
    return [np.float32(s) if (float(s), q) in keep else np.float32(np.float32(threshold) + np.float32(1.0))
            for q, s in zip(states, scores)]


def test_n_best_step_against_a_sort():
    rng = np.random.default_rng(3)
    ties = 0
    for _ in range(200):
        n = int(rng.integers(1, 40))
        states = [int(q) for q in rng.permutation(100)[:n]]
        scores = rng.integers(0, 6, size=n).astype(np.float32)  # many equal scores
        n_best = int(rng.integers(1, n + 3))
        threshold = np.float32(scores.min() + np.float32(rng.integers(0, 8)))
        got = sr.n_best_step(states, scores, n_best, threshold)
        want = _plain_n_best(states, scores, n_best, threshold) if n_best < n else list(scores)
        assert [float(x) for x in got] == [float(x) for x in want]
        if n_best < n:
            ranked = sorted(float(s) for s in scores)
            ties += ranked[n_best - 1] == ranked[n_best]
            # the lowest state indices among the equal scores at the cut stay
            cut = ranked[n_best - 1]
            stay = sorted(q for q, s, g in zip(states, scores, got) if s == cut and float(g) == cut)
            assert stay == sorted(q for q, s in zip(states, scores) if s == cut)[:len(stay)]
            assert sum(float(g) <= float(threshold) for g in got) <= n_best
    assert ties > 20
    # -0 and +0 are one score: the state index decides
    got = sr.n_best_step([4, 2], [np.float32(0.0), np.float32(-0.0)], 1, np.float32(5.0))
    assert float(got[0]) == 6.0 and float(got[1]) == 0.0


def test_n_best_survival_above_2_pow_24():
    """threshold = 2^25: threshold + 1 == threshold in f32, so the demoted states survive with the new score (between
    2^24 and 2^25 the sum is a tie that rounds to even: up for an odd threshold, which prunes)."""
    threshold = np.float32(2.0 ** 25)
    got = sr.n_best_step([0, 1, 2, 3], [3.0, 1.0, 2.0, 1.0], 2, threshold)
    assert [float(x) for x in got] == [2.0 ** 25, 1.0, 2.0 ** 25, 1.0]
    assert all(x <= threshold for x in got)
    odd = np.float32(2.0 ** 24 + 2.0)  # odd mantissa: + 1 is a tie and rounds up
    assert [float(x) for x in sr.n_best_step([0, 1], [3.0, 1.0], 1, odd)] == [2.0 ** 24 + 4.0, 1.0]
    small = sr.n_best_step([0, 1, 2, 3], [3.0, 1.0, 2.0, 1.0], 2, np.float32(2.0 ** 23))
    assert sum(x <= np.float32(2.0 ** 23) for x in small) == 2


@pytest.mark.parametrize("order", ["reference", "state"])
def test_viterbi_pass_without_n_best_is_the_restatement(order):
    rng = np.random.default_rng(17)
    for i in range(12):
        g = ar.random_interval_graph(rng, int(rng.integers(2, 30)), 7, parallel=bool(i % 2))
        table = rng.integers(0, 4, size=(7, int(rng.integers(1, 12)))).astype(np.float32)
        for pruning in (np.inf, 2.0):
            a, b = ar.align(g, table, pruning, order), sr.viterbi_pass(g, table, pruning, order=order)
            assert np.float32(a["score"]).view(np.uint32) == np.float32(b["score"]).view(np.uint32)
            assert a["hypotheses"] == b["hypotheses"] and (a["arc"] is None) == (b["arc"] is None)
            assert a["arc"] is None or np.array_equal(a["arc"], b["arc"])
            # n_best at the number of states is inactive too; one below it may not be
            c = sr.viterbi_pass(g, table, pruning, n_best=g["n_states"], order=order)
            assert c["hypotheses"] == a["hypotheses"] and not c["tie_at_cut"]


def test_posterior_pass_without_n_best_is_the_restatement():
    rng = np.random.default_rng(19)
    for i in range(8):
        g = ar.random_interval_graph(rng, int(rng.integers(2, 20)), 7, integer=False, parallel=bool(i % 2))
        table = (rng.random((7, int(rng.integers(1, 9)))) * 4).astype(np.float32)
        for pruning in (np.inf, 3.0):
            a, b = bw.posteriors(g, table, pruning), sr.posterior_pass(g, table, pruning)
            for k in a:
                assert repr(a[k]) == repr(b[k]), k


def test_n_best_prunes_in_a_pass():
    rng = np.random.default_rng(23)
    g = ar.random_interval_graph(rng, 40, 7)
    table = rng.integers(0, 4, size=(7, 15)).astype(np.float32)
    full = sr.viterbi_pass(g, table, np.inf)
    for n_best in (1, 2, 5):
        r = sr.viterbi_pass(g, table, 100.0, n_best)
        assert r["hypotheses"] <= n_best * 15 and (r["hypotheses"] < full["hypotheses"] or n_best == 5)
        p = sr.posterior_pass(g, table, 100.0, n_best=n_best)
        assert p["hypotheses"] <= n_best * 15


def test_search_on_a_diagonal_chain():
    """The generator of the GPU tests: the diagonal made expensive in one frame fails every pass whose threshold is
    below the extra cost."""
    rng = np.random.default_rng(29)
    n = 12
    g = sr.diagonal_chain(n, np.arange(n))
    table = (rng.random((n, n)) * 0.25).astype(np.float32)
    table[6, 6] += 30.0
    s = search(min_pruning=4.0, max_pruning=64.0)
    r = sr.align_search(g, table, s)
    assert r["iterations"] == 5 and r["threshold"] == 64.0 and r["arc"] is not None  # fails at 4, 8, 16; 32 and 64 agree
    s.until_no_score_difference = False
    assert sr.align_search(g, table, s)["iterations"] == 4
    s.max_pruning = 16.0
    r = sr.align_search(g, table, s)
    assert r["iterations"] == 3 and r["arc"] is None and r["score"] == F32_MAX and r["threshold"] == 16.0
    p = sr.posteriors_search(g, table, search(min_pruning=4.0, max_pruning=64.0))
    assert p["iterations"] == 5 and p["has"]
