"""Lifecycle of a scorer handle through the C-ABI: what the host code owns and decides, on the smallest models.

  * create, score, destroy, create again -- every scorer type and kernel flag: the second handle's tables equal the
    first's bit for bit and both match the oracle (the tolerances of tests/test_gpu_parity.py: bit-exact for the
    quantized types and the reference-order kernels, 1e-4 relative for the other float kernels);
  * a creation that fails after the model tables were uploaded (the clustering build rejects select_clusters >
    clusters) or before any upload (batch-diagonal-maximum-fast at D = 16) releases what it built: the error text
    is the library's, and a valid scorer created afterwards in the same process is correct;
  * the kernel choice and the launchers agree at the frame-tile switches: gmm_score_device calls of 1 / 64 / 65 /
    256 / 257 frames on one quantized handle (the 64-, 256- and full-size tiles), 255 / 256 / 257 on the wide split
    kernel, into device tables with score_stride > n_frames whose columns past n_frames keep their sentinel;
  * the density-sharded handle with both parts on one GPU, copy and RCCL exchange, created twice in a row.

Model: 5 mixtures x 4 densities, D = 16, 3 frames, max_frames 64 unless a test says otherwise
(batch-diagonal-maximum-fast exists for 33..48 components only: D = 40).
"""
import numpy as np
import pytest

import oracle
import rasr_amd as ra

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4  # tests/test_gpu_parity.py, float kernels
CLUSTERS, SELECT = 4, 2


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _model(d=16, covariances=1):
    return ra.synthetic_mixture_set(5, 4, d, seed=7, n_covariances=covariances, weights="random")


_REFS = {}


def _reference(kind, d, covariances, n_frames, seed=21):
    """(model, frames, oracle scores, oracle best or None), computed once per case."""
    key = (kind, d, covariances, n_frames, seed)
    if key not in _REFS:
        ms = _model(d, covariances)
        frames = ra.synthetic_frames(n_frames, d, seed=seed)
        best = None
        if kind == "SIMD-diagonal-maximum":
            s, best, _ = oracle.OracleSimd(ms).score(frames)
        elif kind == "batch-diagonal-maximum-int":
            s = oracle.batch_int_score(ms, frames)
        elif kind == "batch-diagonal-maximum-fast":
            s = oracle.batch_fast_score(ms, frames)
        elif kind == "diagonal-maximum":
            s, best = oracle.OracleFloat(ms).score(frames)
        elif kind == "batch-diagonal-maximum-float":
            s = oracle.batch_float_score(ms, frames)
        elif kind == "diagonal-sum":
            s, best = oracle.OracleFloatSum(ms).score(frames)
        else:
            ref = oracle.OraclePresel(ms, kind.rsplit("-", 1)[1], clusters=CLUSTERS, select=SELECT)
            s = ref.score(frames, selection=ref.select(frames))
        _REFS[key] = (ms, frames, s, best)
    return _REFS[key]


def _check(kind, exact, ms, frames, s, b, ref_s, ref_b):
    if exact:
        assert np.array_equal(_bits(s), _bits(ref_s))
        if ref_b is not None and b is not None:
            assert np.array_equal(b, ref_b)
        return
    if kind == "preselection-batch-float":  # a mixture without a selected density scores the backoff, exactly
        assert np.array_equal(s == np.float32(40000.0), ref_s == np.float32(40000.0))
    if ref_b is not None and b is not None:
        from test_gpu_parity import _check_float
        _check_float(s, b, ref_s, ref_b, ms, frames, None)
    else:
        err = np.abs(s.astype(np.float64) - ref_s) / np.maximum(1.0, np.abs(ref_s.astype(np.float64)))
        assert err.max() <= REL_TOL, f"max rel err {err.max()}"


EXACT = {"SIMD-diagonal-maximum", "batch-diagonal-maximum-int", "batch-diagonal-maximum-fast", "preselection-batch-int"}
PRESEL = {"clusters": CLUSTERS, "select_clusters": SELECT}
# (type, dimension, covariances, Scorer options, ask for best densities)
LIFECYCLE = [
    pytest.param("SIMD-diagonal-maximum", 16, 1, {}, True, id="simd"),
    pytest.param("SIMD-diagonal-maximum", 16, 1, {}, False, id="simd-scores-only-twin"),
    pytest.param("SIMD-diagonal-maximum", 16, 1, {"no_score_only_twin": True}, False, id="simd-no-twin"),
    pytest.param("SIMD-diagonal-maximum", 16, 3, {}, True, id="simd-3cov"),
    pytest.param("batch-diagonal-maximum-int", 16, 1, {}, True, id="batch-int"),
    pytest.param("batch-diagonal-maximum-int", 16, 1, {"full_keys": True}, True, id="batch-int-full-keys"),
    pytest.param("batch-diagonal-maximum-fast", 40, 1, {}, True, id="batch-fast"),
    pytest.param("diagonal-maximum", 16, 1, {}, True, id="diagonal-maximum"),
    pytest.param("diagonal-maximum", 16, 3, {}, True, id="diagonal-maximum-3cov"),
    pytest.param("diagonal-maximum", 16, 1, {"native_f32": True}, True, id="native-f32"),
    pytest.param("diagonal-maximum", 16, 1, {"split_tile16": True}, True, id="split-tile16"),
    pytest.param("diagonal-maximum", 16, 1, {"split_tile32": True}, True, id="split-tile32"),
    pytest.param("diagonal-maximum", 16, 1, {"reference_order": True}, True, id="reference-order"),
    pytest.param("batch-diagonal-maximum-float", 16, 1, {}, True, id="batch-float"),
    pytest.param("diagonal-sum", 16, 1, {}, True, id="diagonal-sum"),
    pytest.param("preselection-batch-float", 16, 1, PRESEL, True, id="preselection-float"),
    pytest.param("preselection-batch-int", 16, 1, PRESEL, True, id="preselection-int"),
]


@pytest.mark.parametrize("kind,d,covariances,opts,want_best", LIFECYCLE)
def test_create_score_destroy_create(gpu, kind, d, covariances, opts, want_best):
    ms, frames, ref_s, ref_b = _reference(kind, d, covariances, 3)
    exact = kind in EXACT or opts.get("reference_order", False)
    tables = []
    for _ in range(2):
        sc = ra.Scorer(ms, kind, max_frames=64, **opts)
        s, b = sc.score_host(frames, want_best=want_best)
        sc.close()
        if ref_b is None:
            b = None
        _check(kind, exact, ms, frames, s, b, ref_s, ref_b)
        tables.append((s, b))
    assert np.array_equal(_bits(tables[0][0]), _bits(tables[1][0]))
    if tables[0][1] is not None:
        assert np.array_equal(tables[0][1], tables[1][1])


def _valid_scorer_is_correct():
    ms, frames, ref_s, ref_b = _reference("SIMD-diagonal-maximum", 16, 1, 3)
    sc = ra.Scorer(ms, "SIMD-diagonal-maximum", max_frames=64)
    s, b = sc.score_host(frames)
    sc.close()
    assert np.array_equal(_bits(s), _bits(ref_s)) and np.array_equal(b, ref_b)


@pytest.mark.parametrize("kind", ["preselection-batch-int", "preselection-batch-float"])
def test_half_built_handle_is_released(gpu, kind):
    """select_clusters > clusters: the clustering build refuses it after the tiles, row constants and frame staging
    of the model are on the device."""
    with pytest.raises(ra.GmmError) as e:
        ra.Scorer(_model(), kind, max_frames=64, clusters=4, select_clusters=5)
    assert str(e.value) == "gmm_scorer_create failed (-1): select-clusters must be in [1, clusters]"
    _valid_scorer_is_correct()


def test_refused_before_any_upload(gpu):
    with pytest.raises(ra.GmmError) as e:
        ra.Scorer(_model(), "batch-diagonal-maximum-fast", max_frames=64)
    assert str(e.value) == ("gmm_scorer_create failed (-2): batch-diagonal-maximum-fast needs 33..48 components (padded "
                            "dimension 48): the reference's fixed 48-byte loads are undefined for smaller dimensions; "
                            "use batch-diagonal-maximum-int")
    _valid_scorer_is_correct()


SENTINEL = -12345.0
BEST_SENTINEL = -559038737  # 0xdeadbeef as int32


def _score_into_wider_table(sc, frames, want_best):
    """gmm_score_device into device tables with score_stride = n_frames + 5, so the scorer kernel itself runs with
    score_stride > n_frames; the spare columns are pre-filled and must keep their sentinel."""
    import torch
    n, m = len(frames), sc.n_mixtures()
    d_frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).cuda()
    d_scores = torch.full((m, n + 5), SENTINEL, dtype=torch.float32, device="cuda")
    d_best = torch.full((m, n + 5), BEST_SENTINEL, dtype=torch.int32, device="cuda") if want_best else None
    sc.score_device(d_frames, d_scores, d_best)
    torch.cuda.synchronize()
    s = d_scores.cpu().numpy()
    assert (s[:, n:] == np.float32(SENTINEL)).all(), "columns past n_frames written"
    b = None
    if want_best:
        b = d_best.cpu().numpy()
        assert (b[:, n:] == BEST_SENTINEL).all(), "columns past n_frames of the best densities written"
        b = np.ascontiguousarray(b[:, :n]).view(np.uint32)
    return np.ascontiguousarray(s[:, :n]), b


@pytest.mark.parametrize("kind,d,want_best", [("SIMD-diagonal-maximum", 16, True), ("SIMD-diagonal-maximum", 16, False),
                                              ("batch-diagonal-maximum-int", 16, False),
                                              ("batch-diagonal-maximum-fast", 40, False)])
def test_quantized_frame_tile_switches(gpu, kind, d, want_best):
    """64 / 256 / full-size frame tiles of the quantized kernels (the key layout with best densities, the slot
    layout without) on one handle."""
    ms, frames, ref_s, ref_b = _reference(kind, d, 1, 257)
    sc = ra.Scorer(ms, kind, max_frames=600)
    for n in (1, 64, 65, 256, 257):
        s, b = _score_into_wider_table(sc, frames[:n], want_best)
        assert np.array_equal(_bits(s), _bits(ref_s[:, :n])), f"{n} frames"
        if want_best:
            assert np.array_equal(b, ref_b[:, :n]), f"{n} frames"
    sc.close()


@pytest.mark.parametrize("kind", ["diagonal-maximum", "batch-diagonal-maximum-float"])
def test_wide_split_kernel_frame_tiles(gpu, kind):
    """D = 39: 4 K steps, the 256-frame one-wave workgroups of scoreSplitWide."""
    ms, frames, ref_s, ref_b = _reference(kind, 39, 1, 257)
    sc = ra.Scorer(ms, kind, max_frames=600)
    assert sc.main_kernel() == "scoreSplitWide"
    for n in (255, 256, 257):
        s, b = _score_into_wider_table(sc, frames[:n], ref_b is not None)
        _check(kind, False, ms, frames[:n], s, b, ref_s[:, :n], None if ref_b is None else ref_b[:, :n])
    sc.close()


@pytest.mark.parametrize("kind", ["SIMD-diagonal-maximum", "batch-diagonal-maximum-int"])
def test_sharded_handle_on_one_gpu(gpu, kind):
    ms, frames, _, _ = _reference(kind, 16, 1, 3)
    whole = ra.Scorer(ms, kind, max_frames=64)
    ref_s, ref_b = whole.score_host(frames)
    whole.close()
    for exchange in ("copy", "rccl"):
        for _ in range(2):
            try:
                sc = ra.Scorer(ms, kind, max_frames=64, devices=[0, 0], exchange=exchange)
            except ra.GmmError as e:
                if exchange == "rccl" and "the RCCL exchange: " in str(e):
                    pytest.skip(f"RCCL does not load: {e}")
                raise
            assert sc.shard_info() == (2, exchange)
            s, b = sc.score_host(frames)
            sc.close()
            assert np.array_equal(_bits(s), _bits(ref_s))
            if kind == "SIMD-diagonal-maximum":
                assert np.array_equal(b, ref_b)
