"""The LETKF under vertical, temporal and cross-variable localisation without a GPU: the export and the refusals
of `SlabLETKF`, each before any device work, the declaration of the entry points, the NumPy model of tests/_letkf_slab.py against
a second route and against tests/_letkf.py when every factor is 1, and the grouping rule."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import _etkf
import _letkf
import _letkf_slab as ls


def _state(M=6, nvars=1, ntimes=1):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(20, 40, 3), np.linspace(250, 270, 4), indexing="ij")
    return EnsembleState.from_array(rng.standard_normal((nvars, ntimes, 3, 4, M)), lat, lon)


def test_slab_letkf_is_exported_and_is_a_letkf():
    import efa_xray_amd
    from efa_xray_amd import LETKF, SlabLETKF, EnSRF
    assert "SlabLETKF" in efa_xray_amd.__all__ and issubclass(SlabLETKF, LETKF) and issubclass(SlabLETKF, EnSRF)
    st = _state(nvars=2, ntimes=3)
    names = st.vars()
    f = SlabLETKF(st, [], verbose=False, vert_coord=np.arange(6.0).reshape(2, 3), time_localize=True,
                  var_impact={names[0]: {names[1]: 0.5}}, weight_stride=2, rtps=0.5, device=10 ** 6)
    assert f.vert_coord.shape == (2, 3) and f.slab is not None and f.weight_stride == (2, 2) and f.last_solve is None
    plain = SlabLETKF(st, [], verbose=False, device=10 ** 6)
    assert plain.vert_coord is None and plain.slab is None


@pytest.mark.parametrize("kw,reason", [
    (dict(loc=None), "ETKF"), (dict(loc="gc"), "ETKF"),
    (dict(adaptive_inflation=object()), "serial order"),
    (dict(sampling_error_correction=True), "serial gain"),
    (dict(streamed=True), "resident"),
    (dict(path="transform"), "route"),
    (dict(obs_batch=8), "per-batch"),
    (dict(weight_stride=0), "weight_stride"),
    (dict(vert_coord=np.zeros((3, 3))), "vert_coord"),                  # EnSRF's own validation: the shape is (nvars, ntimes)
    (dict(var_impact={"nosuch": {"alsonot": 0.5}}), "not a state variable"),
    (dict(var_impact=[1, 2]), "dict"),
])
def test_slab_letkf_refuses_before_any_device_work(kw, reason):
    from efa_xray_amd import SlabLETKF
    with pytest.raises(ValueError) as e:
        SlabLETKF(_state(nvars=2, ntimes=3), [], verbose=False, device=10 ** 6, **kw)      # (no such device: nothing may touch one)
    assert reason in str(e.value)


def test_slab_letkf_refuses_more_than_136_members_and_update_arrays():
    from efa_xray_amd import SlabLETKF
    with pytest.raises(ValueError) as e:
        SlabLETKF(_state(137), [], verbose=False, device=10 ** 6, time_localize=True)
    assert "136" in str(e.value)
    f = SlabLETKF(_state(8), [], verbose=False, device=10 ** 6)
    with pytest.raises(ValueError):
        f.update_arrays(np.zeros(12), np.zeros((12, 8)))


@pytest.mark.parametrize("kw", [dict(vert_coord=np.zeros((1, 1))), dict(time_localize=True), dict(var_impact={"t": {"t": 1.0}})])
def test_letkf_itself_still_refuses_the_three_keywords_and_names_the_class(kw):
    from efa_xray_amd import LETKF
    with pytest.raises(ValueError) as e:
        LETKF(_state(), [], verbose=False, device=10 ** 6, **kw)
    assert "slab group" in str(e.value) and "SlabLETKF" in str(e.value)


def test_entry_points_are_declared_and_bound():
    from efa_xray_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efa_hip.h")).read(), flags=re.S)
    for name, nargs in (("efa_letkf_slab_cycle_dev", 25), ("efa_letkf_slab_cycle_f32_dev", 25), ("efa_letkf_slab_cycle_interp_dev", 28),
                        ("efa_letkf_slab_cycle_interp_f32_dev", 28), ("efa_letkf_slab_weights_dev", 16), ("efa_letkf_slab_groups", 4)):
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, text)
        assert m, name + " is not declared in include/efa_hip.h"
        assert len(m.group(1).split(",")) == nargs
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert hasattr(_lib.load_library(), name)
    for plain in ("cycle_dev", "cycle_f32_dev", "cycle_interp_dev", "cycle_interp_f32_dev", "weights_dev"):
        assert _lib.SIGNATURES["efa_letkf_slab_" + plain][1] == _lib.SIGNATURES["efa_letkf_" + plain][1]
    for meth in ("letkf_slab_cycle", "letkf_slab_weights", "letkf_slab_groups"):
        assert hasattr(_lib.Context, meth)
    assert "EFA_ERR_ALLOC = -5" in text and _lib.EFA_ERR_ALLOC == -5


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _case(M=16, P=64, ny=5, nx=7, nvars=2, ntimes=3, **kw):
    c = ls.make_case(M, P, ny, nx, nvars, ntimes, **kw)
    c["ym"], c["Yp"] = _etkf.ob_priors(c["HX"])
    return c


def test_the_two_model_routes_agree_with_all_three_factors():
    c = _case()
    S = ls.slab_table(c["n_lead"], c["P"], c["loc"])
    group_of, rep = ls.groups(c["n_lead"], c["P"], c["loc"])
    assert len(rep) == 6 and S.min() == 0.0 and 0.0 < np.median(S) < 1.0
    rho = _letkf.taper(c["grid_lat"], c["grid_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"])
    args = (rho, S, rep, c["ym"], c["Yp"], c["value"], c["error"], c["assim"])
    T1, w1, st = ls.point_weights(*args)
    T2, w2, _ = ls.point_weights(*args, route=_letkf.solve_point_svd)
    assert st["cond"].max() < 1e4
    assert np.abs(T1 - T2).max() <= 1e-10 * np.abs(T1).max()
    assert np.abs(w1 - w2).max() <= 1e-10 * np.abs(w1).max()
    # the groups differ from one another: the factors do something
    assert np.abs(T1[0] - T1[-1]).max() > 1e-3


def test_all_factors_one_is_the_plain_model_exactly():
    c = _case(17, 33, 5, 7, 2, 2)
    P, n_lead = c["P"], c["n_lead"]
    loc = dict(lead_vert=np.arange(n_lead, dtype=float), ob_vert=np.full(P, np.nan), ob_vert_halfwidth=np.ones(P),
               lead_time=np.arange(n_lead, dtype=float), ob_time=np.zeros(P), ob_time_halfwidth=np.full(P, np.nan),
               impact=np.ones((2, 2)), lead_var=np.repeat([0, 1], 2), ob_group=np.zeros(P, int), ob_var=np.zeros(P, int))
    assert np.all(ls.slab_table(n_lead, P, loc) == 1.0) and np.all(ls.obs_factor(P, loc) == 1.0)
    group_of, rep = ls.groups(n_lead, P, loc)
    assert not group_of.any() and list(rep) == [0]
    args = (c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"], c["grid_lon"], n_lead)
    a, b = ls.slab_cycle(*args, loc), _letkf.letkf_cycle(*args)
    for k in ("post", "ym", "Yp"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["T"][0], b["T"]) and np.array_equal(a["w"][0], b["w"])
    assert np.array_equal(a["stats"]["n_local"][0], b["stats"]["n_local"])
    for k in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
        assert np.array_equal(a["diag"][k], b["diag"][k], equal_nan=True)


def test_a_zero_impact_leaves_the_other_variable_exactly():
    c = _case(16, 40, 5, 7, 2, 2, parts="c")
    loc = dict(c["loc"], impact=np.array([[1.0, 0.0], [1.0, 1.0]]), ob_group=np.zeros(c["P"], int), ob_var=np.zeros(c["P"], int))
    out = ls.slab_cycle(c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                        c["grid_lon"], c["n_lead"], loc)
    assert list(out["group_of"]) == [0, 0, 1, 1]
    q = np.arange(2 * c["ncol"], 4 * c["ncol"])
    assert np.array_equal(out["post"][q], c["X"][q]) and not out["stats"]["n_local"][1].any() and out["stats"]["n_local"][0].any()
    assert not np.array_equal(out["post"][:2 * c["ncol"]], c["X"][:2 * c["ncol"]])


def test_the_grouping_rule():
    P = 5
    ob = dict(ob_vert=np.array([500.0, np.nan, 300.0, 850.0, 850.0]), ob_vert_halfwidth=np.full(P, 200.0))
    g, rep = ls.groups(6, P, dict(ob, lead_vert=[0.0, 0.0, 1.0, 1.0, 2.0, 2.0]))
    assert list(g) == [0, 0, 1, 1, 2, 2] and list(rep) == [0, 2, 4]
    # numbered by first appearance; every NaN is one key; -0.0 and 0.0 are two bit patterns
    g, rep = ls.groups(6, P, dict(ob, lead_vert=[2.0, np.nan, 2.0, -np.nan, 0.0, -0.0]))
    assert list(g) == [0, 1, 0, 1, 2, 3] and list(rep) == [0, 1, 4, 5]
    # a part that cannot give a factor other than 1 does not split: no ob with both a coordinate and a half-width ...
    g, _ = ls.groups(4, P, dict(lead_vert=[1.0, 2.0, 3.0, 4.0], ob_vert=np.full(P, np.nan), ob_vert_halfwidth=np.ones(P)))
    assert not g.any()
    # ... no ob with both a time and a temporal half-width, an impact table of ones
    g, _ = ls.groups(4, P, dict(lead_time=[0.0, 6.0, 0.0, 6.0], ob_time=np.zeros(P), ob_time_halfwidth=np.full(P, np.nan),
                                impact=np.ones((2, 2)), lead_var=[0, 0, 1, 1], ob_group=np.zeros(P, int), ob_var=np.zeros(P, int)))
    assert not g.any()
    # the three parts together: 37 levels x 4 variables without var_impact would be 37 groups, here 2 levels x 2 times x 2 variables
    loc = dict(ob, lead_vert=np.repeat([850.0, 500.0], 4), lead_time=np.tile([0.0, 6.0], 4), ob_time=np.zeros(P),
               ob_time_halfwidth=np.full(P, 9.0), impact=np.array([[1.0, 0.5], [1.0, 1.0]]), lead_var=np.tile([0, 0, 1, 1], 2),
               ob_group=np.zeros(P, int), ob_var=np.zeros(P, int))
    g, rep = ls.groups(8, P, loc)
    assert list(g) == list(range(8))
    g, rep = ls.groups(8, P, dict(loc, impact=None))
    assert list(g) == [0, 1, 0, 1, 2, 3, 2, 3]
    # equal keys imply equal columns of S
    S = ls.slab_table(8, P, dict(loc, impact=None))
    assert all(np.array_equal(S[:, s], S[:, rep[g[s]]]) for s in range(8))
