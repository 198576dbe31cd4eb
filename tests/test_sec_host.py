"""Sampling error correction without a GPU: the NumPy model (tests/_sec.py) anchored to the oracle and so to the
reference's goldens, the default table against independent quadrature values, the lookup, and the settings that are refused."""
import numpy as np
import pytest

import _sec
from conftest import load_golden
from oracle import ensrf_oracle as orc
from test_gpu_parity import oracle_kwargs, prior_arrays


@pytest.mark.parametrize("name", ["G2", "G6"])
def test_model_with_a_table_of_ones_is_the_oracle_bit_for_bit(name):
    g = load_golden(name)
    N, xbm, Xbp = prior_arrays(g)
    ref = orc.ensrf_update(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], **oracle_kwargs(g))
    for T in (2, 201):
        got = _sec.ensrf_update(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], np.ones(T), **oracle_kwargs(g))
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (name, T)
        for key in ref[2]:
            assert np.array_equal(got[2][key], ref[2][key], equal_nan=True), (name, T, key)
    # ... which is the reference's own result
    assert np.array_equal(ref[0], g["xam"])
    # and the steep table is another filter altogether
    steep = _sec.ensrf_update(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], _sec.steep_table(201), **oracle_kwargs(g))
    assert np.abs(steep[0] - ref[0]).max() > 1e-3 * np.abs(ref[0]).max()


# alpha(r; M) by midpoint quadrature of the definition, 4000 nodes in w up to 12 and 4001 nodes in rho
TABLE_VALUES = [(10, 0.5, 0.7485), (10, 0.9, 0.8929), (20, 0.2, 0.8456), (20, 0.5, 0.8704), (20, 0.9, 0.9579), (80, 0.5, 0.9672),
                (80, 0.9, 0.9912)]


@pytest.mark.parametrize("M", [10, 20, 80])
def test_default_table_matches_the_quadrature_values(M):
    from efa_xray_amd import sampling_error_table
    a = sampling_error_table(M)
    assert a.shape == (201,) and a.dtype == np.float64
    for m, r, want in TABLE_VALUES:
        if m == M:
            j = int(round(r * 200))
            assert abs(j / 200.0 - r) < 1e-15
            assert abs(a[j] - want) <= 1e-3, (M, r, a[j], want)
    assert np.all(np.diff(a) >= 0.0), "monotone non-decreasing in r"
    assert a[-1] == 1.0 and a[0] == a[1] and np.all(np.isfinite(a)) and np.all(a >= 0.0)
    again = sampling_error_table(M)
    assert np.array_equal(a, again) and again is not a           # deterministic, cached, and the cache is not handed out
    a[3] = -1.0
    assert sampling_error_table(M)[3] >= 0.0


def test_default_table_definition_by_direct_quadrature():
    """One node straight from the definition in the variables it is stated in (w, rho), coarser than the values above."""
    from efa_xray_amd import sampling_error_table
    M, r = 12, 0.4
    w = (np.arange(3000) + 0.5) * (12.0 / 3000)
    rho = -1.0 + (np.arange(2001) + 0.5) * (2.0 / 2001)
    inner = np.array([((np.cosh(w) - p * r) ** (-(M - 1.0))).sum() for p in rho])
    f = (1.0 - rho ** 2) ** ((M - 1) / 2.0) * inner
    want = (rho * f).sum() / (r * f.sum())
    assert abs(sampling_error_table(M)[80] - want) <= 1e-3


def test_default_table_sizes_and_arguments():
    from efa_xray_amd import sampling_error_table
    for M in (2, 3, 256):
        a = sampling_error_table(M, 33)
        assert a.shape == (33,) and np.all(np.isfinite(a)) and np.all(np.diff(a) >= 0.0) and a[-1] == 1.0 and a[0] > 0.0
    assert np.array_equal(sampling_error_table(50, 2), [1.0, 1.0])
    assert sampling_error_table(256)[100] > sampling_error_table(20)[100]      # more members: less to correct
    for bad in (dict(M=1), dict(M=2.5), dict(M=True), dict(M=20, T=1), dict(M=20, T=513), dict(M=20, T=3.5)):
        with pytest.raises(ValueError):
            sampling_error_table(**bad)


def test_lookup_at_nodes_midpoints_beyond_one_and_nan():
    rng = np.random.default_rng(3)
    for T in (2, 3, 201, 512):
        alpha = rng.uniform(0.0, 2.0, T)
        nodes = np.arange(T) / (T - 1.0)
        # (a node's t = r (T-1) may round one ulp below j: the value is then read at the end of the interval before it, which
        # is the same number to |slope| T eps < 2 * 512 * 2.3e-16)
        assert np.allclose(_sec.lookup(alpha, nodes), alpha, rtol=0, atol=1e-12)
        assert np.allclose(_sec.lookup(alpha, -nodes), alpha, rtol=0, atol=1e-12)             # |r|
        mid = 0.5 * (nodes[1:] + nodes[:-1])
        assert np.allclose(_sec.lookup(alpha, mid), 0.5 * (alpha[1:] + alpha[:-1]), rtol=0, atol=1e-12)
        assert np.array_equal(_sec.lookup(alpha, [1.0, 1.0 + 1e-12, 7.0, -3.0, np.inf]), np.full(5, alpha[-1]))
        assert _sec.lookup(alpha, 0.0) == alpha[0]
        assert np.isnan(_sec.lookup(alpha, np.nan))
        # continuous across a node
        j = T // 2
        eps = 1e-9
        lo, hi = _sec.lookup(alpha, nodes[j] - eps), _sec.lookup(alpha, min(nodes[j] + eps, 1.0))
        assert abs(lo - alpha[j]) < 1e-5 and abs(hi - alpha[j]) < 1e-5
    assert np.array_equal(_sec.lookup(np.ones(201), rng.uniform(-1.5, 1.5, 1000)), np.ones(1000))   # exactly 1: the oracle's bits
    # the correlation: 0 where either norm is 0, NaN where a norm is NaN
    r = _sec.correlation(np.array([1.0, 0.0, 2.0, np.nan]), np.array([4.0, 0.0, 1.0, np.nan]), 1.0)
    assert r[0] == 0.5 and r[1] == 0.0 and r[2] == 2.0 and np.isnan(r[3])
    assert _sec.correlation(np.array([3.0]), np.array([2.0]), 0.0)[0] == 0.0


def _state_obs(dtype=np.float64, M=6):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(30, 40, 3), np.linspace(250, 260, 4), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((2, 1, 3, 4, M)).astype(dtype), lat, lon)
    ob = Observation(value=1.0, error=1.0, lat=35.0, lon=255.0, assimilate_this=True, localize_radius=1000.0)
    ob.estimate = lambda s: s.to_vect()[0]
    return state, [ob]


def test_ensrf_refuses_unsupported_settings_before_any_device_work(monkeypatch):
    from efa_xray_amd import EnSRF, AdaptiveInflation, sampling_error_table
    from efa_xray_amd.distributed import ShardedEnSRF
    state, obs = _state_obs()

    def stop(self):
        raise AssertionError("device work before the check")

    monkeypatch.setattr(EnSRF, "_context", stop)
    # accepted: the default table, a table, off; with the settings it combines with; a float32 state
    flt = EnSRF(state, obs, loc="GC", sampling_error_correction=True, verbose=False)
    assert np.array_equal(flt.sec_table, sampling_error_table(6))
    tab = EnSRF(state, obs, loc="GC", sampling_error_correction=[0.5, 1.0], rtps=0.9, outlier_threshold=3.0, inflation=1.1,
                verbose=False)
    assert tab.sec_table.tolist() == [0.5, 1.0]
    EnSRF(state, obs, loc="GC", sampling_error_correction=np.linspace(0, 1, 512), rtpp=0.5, verbose=False)
    assert EnSRF(_state_obs(np.float32)[0], obs, loc="GC", sampling_error_correction=True, verbose=False).sec_table is not None
    for off in (None, False):
        assert EnSRF(state, obs, loc=False, sampling_error_correction=off, verbose=False).sec_table is None
    # refused combinations
    for loc in (False, None):
        with pytest.raises(ValueError, match="loc='GC'"):
            EnSRF(state, obs, loc=loc, sampling_error_correction=True, verbose=False)
    with pytest.raises(ValueError, match="adaptive_inflation"):
        EnSRF(state, obs, loc="GC", sampling_error_correction=True, verbose=False,
              adaptive_inflation=AdaptiveInflation(state, ("spatial", None, (1.0, 0.6))))
    with pytest.raises(ValueError, match="vert_coord"):
        EnSRF(state, obs, loc="GC", sampling_error_correction=True, vert_coord=np.zeros((2, 1)), verbose=False)
    with pytest.raises(ValueError, match="time_localize"):
        EnSRF(state, obs, loc="GC", sampling_error_correction=True, time_localize=True, verbose=False)
    with pytest.raises(ValueError, match="var_impact"):
        EnSRF(state, obs, loc="GC", sampling_error_correction=True, var_impact={"gauge": {state.vars()[0]: 0.5}}, verbose=False)
    with pytest.raises(ValueError, match="streamed"):
        EnSRF(state, obs, loc="GC", sampling_error_correction=True, streamed=True, verbose=False)
    with pytest.raises(ValueError, match="update_arrays"):
        flt.update_arrays(np.zeros(state.nstate() + 1), np.zeros((state.nstate() + 1, state.nmems())))
    sh = ShardedEnSRF(None, 2, 12, state.nmems())
    X = state.to_vect()
    obd = dict(value=np.zeros(1), error=np.ones(1), assim=np.ones(1, dtype=bool), loc="GC")
    idx, wts = np.zeros((1, 1), dtype=np.int64), np.ones((1, 1))
    for sec in (True, [0.5, 1.0]):
        with pytest.raises(ValueError, match="sampling_error_correction"):
            sh.update(X, X.copy(), idx, wts, obd, sampling_error_correction=sec)
        with pytest.raises(ValueError, match="sampling_error_correction"):
            sh.assimilate(X, X.copy(), np.zeros((1, state.nmems())), obd, sampling_error_correction=sec)
    # invalid tables
    for bad in ([1.0], [], np.ones(513), np.ones((2, 3)), [0.5, -0.1], [0.5, np.nan], [np.inf, 1.0], "table", [0.5, "x"], 1.0):
        with pytest.raises(ValueError, match="sampling_error_correction"):
            EnSRF(state, obs, loc="GC", sampling_error_correction=bad, verbose=False)


def test_sec_entry_point_is_registered():
    import ctypes
    from efa_xray_amd import _lib
    res, args = _lib.SIGNATURES["efa_ctx_set_sampling_error_correction"]
    assert res is ctypes.c_int and len(args) == 3
    lib = _lib.load_library()
    assert lib.efa_abi_version() == 1
    assert lib.efa_ctx_set_sampling_error_correction(None, None, 0) < 0
    assert b"null context" in lib.efa_last_error()


def test_sec_kernels_use_no_scratch_where_their_plain_counterparts_use_none():
    """Every kGcSec instantiation of the two one-pass sweep forms against the plain kernel of the same width, vector form and
    member form: no scratch and no spilled register where that one has none.  All 2..256 members, float64 and
    float32 rows."""
    import re
    from efa_xray_amd import _lib
    from _codeobj import kernel_table
    tab = kernel_table(_lib.LIB_PATH)

    def rows_per_quad_stripped(n):
        return re.sub(r"Li\d+E(EEvNS)", r"\1", n)

    plain_quad = {rows_per_quad_stripped(n): k for n, k in tab.items() if "k_sweep_gcILi0E" in n}
    seen = {"quad": 0, "lane": 0}
    for n, k in tab.items():
        if "k_sweep_gcILi4E" in n:
            p = plain_quad[rows_per_quad_stripped(n.replace("k_sweep_gcILi4E", "k_sweep_gcILi0E"))]
            seen["quad"] += 1
        elif "k_sweep_gc_laneILi4E" in n:
            p = tab[n.replace("k_sweep_gc_laneILi4E", "k_sweep_gc_laneILi0E")]
            seen["lane"] += 1
        else:
            continue
        if p[".private_segment_fixed_size"] == 0 and p.get(".vgpr_spill_count", 0) == 0:
            assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, (n, k[".vgpr_count"])
        assert k[".group_segment_fixed_size"] <= p[".group_segment_fixed_size"] + 8 * (512 + 32), n    # the table and y'.y' in LDS
    assert seen == {"quad": 19 * 4, "lane": 26 * 3}, seen
    # the per-batch sweep's two kernels
    assert sum("11k_sweep_secILi4E" in n for n in tab) == 19 * 2
