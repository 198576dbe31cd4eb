"""The LETKF without a GPU: the NumPy model of tests/_letkf.py against itself by a second route and against the
unlocalised ETKF model in the limit of very wide tapers, its edge rules, the declaration of the three entry points, and the
refusals of the `LETKF` class, each before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import _etkf
import _letkf


def _case(M=16, P=64, ny=5, nx=7, n_lead=3, **kw):
    c = _letkf.make_case(M, P, ny, nx, n_lead, **kw)
    c["ym"], c["Yp"] = _etkf.ob_priors(c["HX"])
    return c


def _weights(c, route=_letkf.solve_point, hw=None):
    return _letkf.weights(c["grid_lat"], c["grid_lon"], c["ym"], c["Yp"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"],
                          c["ob_hw"] if hw is None else hw, route=route)


@pytest.mark.parametrize("M,P", [(3, 5), (16, 64), (17, 33), (40, 400)])
def test_the_two_model_routes_agree_on_every_column(M, P):
    c = _case(M, P)
    T1, w1, st, _ = _weights(c)
    T2, w2, _, _ = _weights(c, route=_letkf.solve_point_svd)
    assert st["cond"].max() < 1e4
    assert np.abs(T1 - T2).max() <= 1e-10 * np.abs(T1).max()
    assert np.abs(w1 - w2).max() <= 1e-10 * max(np.abs(w1).max(), 1e-300)


def test_very_wide_tapers_give_the_unlocalised_etkf():
    c = _case(16, 64)
    T, w, st, rho = _weights(c, hw=np.full(c["P"], 1e12))
    a = c["assim"]
    assert np.abs(rho[:, a] - 1.0).max() <= 2.3e-16 and np.all(rho[:, ~a] == 0.0)
    ref = _etkf.etkf_solution(c["ym"], c["Yp"], c["value"], c["error"], a)
    assert np.abs(T - ref["T"]).max() <= 1e-13 * np.abs(ref["T"]).max()
    assert np.abs(w - ref["w"]).max() <= 1e-13 * np.abs(ref["w"]).max()
    assert np.all(st["n_local"] == int(a.sum()))
    assert np.allclose(st["dfs"], ref["dfs"], rtol=1e-12)


def test_a_column_out_of_every_obs_reach_keeps_its_rows_exactly():
    c = _case(16, 40, 6, 7, 3, hw=(100.0, 400.0))
    out = _letkf.letkf_cycle(c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                             c["grid_lon"], c["n_lead"])
    none = np.flatnonzero(out["stats"]["n_local"] == 0)
    some = np.flatnonzero(out["stats"]["n_local"] > 0)
    assert none.size and some.size
    for col in none:
        rows = col + c["ncol"] * np.arange(c["n_lead"])
        assert np.array_equal(out["post"][rows], c["X"][rows])
        assert np.array_equal(out["T"][col], np.eye(c["M"])) and not out["w"][col].any()
    rows = some[0] + c["ncol"] * np.arange(c["n_lead"])
    assert not np.array_equal(out["post"][rows], c["X"][rows])


def test_every_transform_is_symmetric_and_keeps_the_member_mean():
    c = _case(17, 33)
    assert np.abs(c["Yp"].sum(axis=1)).max() < 1e-12          # the rows of Yp are centred
    T, _, _, _ = _weights(c)
    assert np.abs(T - np.swapaxes(T, 1, 2)).max() <= 1e-14
    assert np.abs(T.sum(axis=2) - 1.0).max() <= 1e-12


def test_a_nan_value_poisons_w_of_the_columns_it_reaches_only():
    c = _case(16, 40, 6, 7, 3, hw=(100.0, 400.0))
    T0, w0, st0, rho = _weights(c)
    k = int(np.flatnonzero(c["assim"] & (rho != 0.0).any(axis=0))[0])
    value = c["value"].copy()
    value[k] = np.nan
    c2 = dict(c, value=value)
    T1, w1, _, _ = _weights(c2)
    hit = rho[:, k] != 0.0
    assert hit.any() and not hit.all()
    assert np.isnan(w1[hit]).all() and np.array_equal(w1[~hit], w0[~hit]) and np.array_equal(T1, T0)


def test_entry_points_are_declared_and_bound():
    from efa_xray_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efa_hip.h")).read(), flags=re.S)
    for name, nargs in (("efa_letkf_cycle_dev", 25), ("efa_letkf_cycle_f32_dev", 25), ("efa_letkf_weights_dev", 16)):
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, text)
        assert m, name + " is not declared in include/efa_hip.h"
        assert len(m.group(1).split(",")) == nargs
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
    assert _lib.SIGNATURES["efa_letkf_cycle_dev"][1] == _lib.SIGNATURES["efa_letkf_cycle_f32_dev"][1]
    assert hasattr(_lib.Context, "letkf_cycle") and hasattr(_lib.Context, "letkf_weights")


def _state(M=6, dtype=None):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(20, 40, 3), np.linspace(250, 270, 4), indexing="ij")
    st = EnsembleState.from_array(rng.standard_normal((1, 1, 3, 4, M)), lat, lon)
    return st if dtype is None else st.astype(dtype)


def test_letkf_is_exported_and_takes_the_ensrf_keywords():
    import efa_xray_amd
    from efa_xray_amd import LETKF, EnSRF, _lib
    assert "LETKF" in efa_xray_amd.__all__ and issubclass(LETKF, EnSRF)
    f = LETKF(_state(), [], verbose=False, rtps=0.5, outlier_threshold=3.0)
    assert f.loc == "GC" and f.relaxation == (_lib.RELAX_RTPS, 0.5) and f.outlier_threshold == 3.0 and f.last_solve is None
    assert LETKF(_state(), [], verbose=False, loc="GC", rtpp=0.25, streamed=False).relaxation == (_lib.RELAX_RTPP, 0.25)


@pytest.mark.parametrize("kw,reason", [
    (dict(loc=None), "ETKF"), (dict(loc=False), "ETKF"), (dict(loc="gc"), "ETKF"),
    (dict(adaptive_inflation=object()), "serial order"),
    (dict(vert_coord=np.zeros((1, 1))), "slab group"),
    (dict(time_localize=True), "slab group"),
    (dict(var_impact={"t": {"t": 1.0}}), "slab group"),
    (dict(sampling_error_correction=True), "serial gain"),
    (dict(streamed=True), "resident"),
    (dict(path="transform"), "route"),
    (dict(obs_batch=8), "per-batch"),
])
def test_letkf_refuses_what_it_does_not_serve_before_any_device_work(kw, reason):
    from efa_xray_amd import LETKF
    with pytest.raises(ValueError) as e:
        LETKF(_state(), [], verbose=False, device=10 ** 6, **kw)       # (no such device: nothing may touch one)
    assert reason in str(e.value)


def test_letkf_refuses_more_than_136_members_and_update_arrays():
    from efa_xray_amd import LETKF
    with pytest.raises(ValueError) as e:
        LETKF(_state(137), [], verbose=False, device=10 ** 6)
    assert "136" in str(e.value) and "LDS" in str(e.value)
    f = LETKF(_state(136), [], verbose=False, device=10 ** 6)
    with pytest.raises(ValueError):
        f.update_arrays(np.zeros(12), np.zeros((12, 136)))


def test_etkf_points_to_the_letkf_for_localisation():
    from efa_xray_amd import ETKF
    with pytest.raises(ValueError) as e:
        ETKF(_state(), [], verbose=False, loc="GC")
    assert "LETKF" in str(e.value) and "out of scope" in str(e.value)
