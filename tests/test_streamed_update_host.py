"""Host-side tests (no GPU) of the streamed update: the chunk planner and the compact-stencil helper as pure
functions with known answers, the keyword validation of `EnSRF(..., streamed=True)`, and the new entry points of the C ABI."""
import ctypes

import numpy as np
import pytest

from efa_xray_amd import _lib


def _check_plan(ncol, chunk_cols):
    plan = _lib.plan_chunks(ncol, chunk_cols)
    if ncol == 0:
        assert plan == []
        return plan
    assert plan[0][0] == 0 and plan[-1][1] == ncol
    for (lo, hi), (lo2, _) in zip(plan, plan[1:]):
        assert hi == lo2                      # contiguous
    for lo, hi in plan:
        assert lo < hi and lo % 16 == 0       # every cut on a multiple of 16
    for lo, hi in plan[:-1]:
        assert hi % 16 == 0 and hi - lo == plan[0][1] - plan[0][0]   # only the last chunk is ragged
    return plan


def test_chunk_planner_known_answers():
    assert _check_plan(10, 16) == [(0, 10)]                          # ncol < 16: one ragged chunk
    assert _check_plan(10, 1000) == [(0, 10)]
    assert _check_plan(64, 16) == [(0, 16), (16, 32), (32, 48), (48, 64)]   # ncol = 16 k
    assert _check_plan(64, 32) == [(0, 32), (32, 64)]
    assert _check_plan(64, 64) == [(0, 64)]
    assert _check_plan(64, 10 ** 9) == [(0, 64)]
    assert _check_plan(70, 32) == [(0, 32), (32, 64), (64, 70)]      # the last chunk takes the ragged rest
    assert _check_plan(70, 47) == [(0, 32), (32, 64), (64, 70)]      # a budget is cut down to a multiple of 16
    assert _check_plan(50, 1) == [(0, 16), (16, 32), (32, 48), (48, 50)]    # below one block: one block per chunk
    assert _check_plan(50, 15) == _check_plan(50, 16)
    assert _check_plan(0, 16) == []
    assert len(_check_plan(361 * 720, 4096)) == -(-361 * 720 // 4096)
    for bad in ((10, 0), (10, -3), (-1, 16)):
        with pytest.raises(ValueError):
            _lib.plan_chunks(*bad)


def test_chunk_planner_random_shapes():
    rng = np.random.default_rng(5)
    for _ in range(200):
        _check_plan(int(rng.integers(0, 5000)), int(rng.integers(1, 700)))


def test_default_chunk_is_about_64_mb_and_a_multiple_of_16():
    for n_lead, M in ((1, 50), (8, 80), (3, 2), (40, 256)):
        cc = _lib.default_chunk_cols(n_lead, M)
        assert cc % 16 == 0 and cc >= 16
        assert (64 << 20) - 16 * n_lead * M * 8 < cc * n_lead * M * 8 <= (64 << 20)
    assert _lib.default_chunk_cols(10 ** 6, 256) == 16               # never below one block


def _compact_restated(idx):
    """NumPy-free restatement: the distinct non-negative entries ascending, and each entry's position among them."""
    flat = [int(v) for v in np.asarray(idx).reshape(-1)]
    rows = sorted(set(v for v in flat if v >= 0))
    pos = dict((r, i) for i, r in enumerate(rows))
    return rows, np.array([pos[v] if v >= 0 else -1 for v in flat], dtype=np.int64).reshape(np.asarray(idx).shape)


def test_compact_stencil_against_a_restatement():
    # -1 entries, rows shared by obs and within one ob, and the time-bracket pairs (entries 0-3 and 4-7 name the same four
    # columns one slab apart)
    ncol = 100
    idx = np.array([[5, 6, 15, 16, 5 + ncol, 6 + ncol, 15 + ncol, 16 + ncol],      # a bracket pair
                    [5, 6, 15, 16, -1, -1, -1, -1],                                  # an exact valid time: second half unused
                    [7, 7, 7, 7, 7 + ncol, 7 + ncol, 7 + ncol, 7 + ncol],            # one row four times
                    [-1, -1, -1, -1, -1, -1, -1, -1],
                    [250, 16, 6, 0, 299, 216, 206, 200]], dtype=np.int64)
    rows, cidx = _lib.compact_stencil(idx)
    want_rows, want_cidx = _compact_restated(idx)
    assert rows.tolist() == want_rows and rows.dtype == np.int64
    assert np.array_equal(cidx, want_cidx) and cidx.dtype == np.int64 and cidx.shape == idx.shape
    assert (cidx[idx < 0] == -1).all() and np.array_equal(rows[cidx[idx >= 0]], idx[idx >= 0])
    assert len(rows) <= 8 * len(idx)
    # applying the compact stencil to the gathered rows is applying the stencil to the state, entry by entry in the same order
    rng = np.random.default_rng(3)
    X = rng.standard_normal((300, 7))
    wts = rng.uniform(0.1, 1.0, idx.shape)
    Xc = X[rows]
    for k in range(len(idx)):
        a = b = None
        for j in range(8):
            if idx[k, j] < 0:
                continue
            ta, tb = wts[k, j] * X[idx[k, j]], wts[k, j] * Xc[cidx[k, j]]
            a, b = (ta, tb) if a is None else (a + ta, b + tb)
        assert (a is None and b is None) or np.array_equal(a, b)
    rng = np.random.default_rng(4)
    for _ in range(20):
        idx = rng.integers(-1, 40, (int(rng.integers(1, 30)), 8))
        rows, cidx = _lib.compact_stencil(idx)
        want_rows, want_cidx = _compact_restated(idx)
        assert rows.tolist() == want_rows and np.array_equal(cidx, want_cidx)
    rows, cidx = _lib.compact_stencil(np.full((3, 8), -1))
    assert rows.size == 0 and (cidx == -1).all()


def _tiny_state_and_obs():
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(20, 60, 4), np.linspace(200, 280, 5), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((2, 1, 4, 5, 6)), lat, lon)
    obs = [Observation(value=1.0, error=1.0, lat=30.0, lon=220.0, obtype="var0", time=0, localize_radius=1000.0)]
    return state, obs


def test_streamed_keywords_and_the_three_value_errors():
    from efa_xray_amd import EnSRF
    from efa_xray_amd.assimilation.adaptive_inflation import AdaptiveInflation
    state, obs = _tiny_state_and_obs()
    flt = EnSRF(state, obs, verbose=False)
    assert flt.streamed is False and flt.stream_chunk_cols is None      # the default stays as it is
    flt = EnSRF(state, obs, verbose=False, streamed=True)
    assert flt.streamed is True and flt.stream_chunk_cols is None and flt.stream_pinned_limit == 4096 << 20
    flt = EnSRF(state, obs, verbose=False, loc="GC", streamed=True, stream_chunk_cols=np.int64(48), stream_pinned_limit_mb=0,
                rtps=0.5, outlier_threshold=3.0, vert_coord=np.zeros((2, 1)), path="sweep", obs_batch=8, inflation=1.1)
    assert flt.stream_chunk_cols == 48 and flt.stream_pinned_limit == 0
    # 1: a chunk size that is not a positive integer
    for bad in (0, -16, 2.5, "16", True, 16.0):
        with pytest.raises(ValueError):
            EnSRF(state, obs, verbose=False, streamed=True, stream_chunk_cols=bad)
    with pytest.raises(ValueError):
        EnSRF(state, obs, verbose=False, stream_chunk_cols=0)            # checked whether or not the mode is on
    for bad in (-1, "x", None, float("nan")):
        with pytest.raises(ValueError):
            EnSRF(state, obs, verbose=False, streamed=True, stream_pinned_limit_mb=bad)
    # 2: streamed with adaptive inflation
    ai = AdaptiveInflation(state, ("spatial", None, (1.0, 0.6)))
    with pytest.raises(ValueError, match="adaptive_inflation"):
        EnSRF(state, obs, verbose=False, loc="GC", streamed=True, adaptive_inflation=ai)
    EnSRF(state, obs, verbose=False, loc="GC", adaptive_inflation=ai)    # (unstreamed: accepted as before)
    # 3: update_arrays on a streamed filter -- refused before anything touches a device
    flt = EnSRF(state, obs, verbose=False, streamed=True)
    with pytest.raises(ValueError, match="streamed"):
        flt.update_arrays(np.zeros(41), np.zeros((41, 6)))
    with pytest.raises(TypeError):
        EnSRF(state, obs, verbose=False, stream=True)                    # unknown keywords are still refused


def test_new_symbols_are_declared_exported_and_refuse_a_null_context():
    lib = _lib.load_library()
    for name in ("efa_ensrf_cycle_host", "efa_pinned_alloc", "efa_pinned_free"):
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        vals = [0 if a in (ctypes.c_int, ctypes.c_long, ctypes.c_size_t) else None for a in args]
        rc = fn(*vals)
        assert rc < 0, name
        assert b"null context" in lib.efa_last_error(), name
    p = ctypes.c_void_p(1)
    assert lib.efa_pinned_alloc(None, 64, ctypes.byref(p)) == _lib.EFA_ERR_INVALID
