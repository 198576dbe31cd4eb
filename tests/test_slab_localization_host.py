"""Temporal and cross-variable localisation without a GPU: the NumPy helper (tests/_slabloc.py) against the oracle
and the vertical helper, the keyword checks of EnSRF / Observation (every ValueError before any device work), the time-lag
conversion, and the C entry points' registration."""
import inspect

import numpy as np
import pytest

import _slabloc as sl
import _vertloc as vl
from conftest import load_golden
from efa_xray_amd.assimilation.ensrf import ob_slab, slab_setting, time_lags
from oracle import ensrf_oracle as orc
from test_gpu_parity import oracle_kwargs, prior_arrays


def _golden_args(name):
    g = load_golden(name)
    N, xbm, Xbp = prior_arrays(g)
    kw = oracle_kwargs(g)
    assert kw["loc"] == "GC"
    return g, N, xbm, Xbp, kw


def _same(got, ref):
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    for key in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
        assert np.array_equal(got[2][key], ref[2][key], equal_nan=True), key


@pytest.mark.parametrize("name", ["G2", "G5"])
def test_helper_equals_oracle_bit_for_bit_without_factors(name):
    g, N, xbm, Xbp, kw = _golden_args(name)
    P = len(g["ob_value"])
    nvar, nt = kw["state_shape"][:2]
    ref = orc.ensrf_update(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], **kw)
    args = dict(ob_lat=kw["ob_lat"], ob_lon=kw["ob_lon"], ob_halfwidth=kw["ob_halfwidth"], grid_lat=kw["grid_lat"],
                grid_lon=kw["grid_lon"], state_shape=kw["state_shape"])
    lead_time = np.tile(np.arange(nt) * 6.0, nvar)
    for extra in (dict(),
                  dict(lead_time=lead_time, ob_time=np.full(P, np.nan), ob_time_halfwidth=np.ones(P)),      # no ob has a time
                  dict(lead_time=lead_time, ob_time=np.zeros(P), ob_time_halfwidth=np.full(P, np.nan)),     # no ob has a tau
                  dict(lead_var=np.repeat(np.arange(nvar), nt), ob_group=np.zeros(P, int), ob_var=np.full(P, -1),
                       impact=np.ones((1, nvar)))):                                                        # all ones
        _same(sl.ensrf_update_slab(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], **args, **extra), ref)


@pytest.mark.parametrize("name", ["G2", "G5"])
def test_helper_equals_the_vertical_helper_bit_for_bit_with_vertical_information_only(name):
    g, N, xbm, Xbp, kw = _golden_args(name)
    P = len(g["ob_value"])
    nvar, nt = kw["state_shape"][:2]
    rng = np.random.default_rng(5)
    lead = np.linspace(0.0, 3.0, nvar * nt)
    ov = rng.uniform(-0.3, 3.3, P)
    ov[0] = np.nan
    oh = rng.uniform(0.6, 1.2, P)
    oh[P // 2] = np.nan
    args = dict(ob_lat=kw["ob_lat"], ob_lon=kw["ob_lon"], ob_halfwidth=kw["ob_halfwidth"], grid_lat=kw["grid_lat"],
                grid_lon=kw["grid_lon"], state_shape=kw["state_shape"], lead_vert=lead, ob_vert=ov, ob_vert_halfwidth=oh)
    ref = vl.ensrf_update_vert(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], **args)
    _same(sl.ensrf_update_slab(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], **args), ref)
    # ... and with a temporal and a variable part that carry no factor
    _same(sl.ensrf_update_slab(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], lead_time=np.zeros(nvar * nt),
                               ob_time=np.full(P, np.nan), ob_time_halfwidth=np.ones(P), lead_var=np.repeat(np.arange(nvar), nt),
                               ob_group=np.full(P, -1), ob_var=np.zeros(P, int), impact=np.zeros((1, nvar)), **args), ref)


def test_helper_matches_a_hand_computed_case():
    """One column, two variables x two times (slabs a@0h, a@6h, b@0h, b@6h), two obs at the column: ob 0 of obtype a at 0 h with
    tau = 6 h and impact 0.5 on b; ob 1 without a time, of an obtype that names no variable and has no impact row.  The
    horizontal taper is 1 everywhere, so ob 0 tapers the slabs by [1, g, 0.5, 0.5 g] with g = GC(r = 1) = 5/24, ob 1 (target: no
    time, no variable) by 1 and itself by 1; ob 1 tapers everything by 1."""
    M = 4
    X = np.array([[1.0, 2.0, 0.0, -1.0], [0.5, -0.5, 1.5, 2.5], [0.0, 1.0, -1.0, 2.0], [3.0, 1.0, 2.0, 0.0]])
    HX = X[[0, 3]] + np.array([[0.1, -0.1, 0.0, 0.2], [0.0, 0.3, -0.2, 0.1]])
    xbm, Xbp = orc.format_prior_state(X, HX)
    val, err, asm = np.array([1.0, 0.0]), np.array([0.5, 1.0]), np.array([True, True])
    pt = dict(ob_lat=np.array([40.0, 40.0]), ob_lon=np.array([260.0, 260.0]), ob_halfwidth=np.array([500.0, 500.0]),
              grid_lat=np.array([[40.0]]), grid_lon=np.array([[260.0]]), state_shape=(2, 2, 1, 1))
    got = sl.ensrf_update_slab(xbm, Xbp, 4, val, err, asm, lead_time=np.array([0.0, 6.0, 0.0, 6.0]), ob_time=np.array([0.0, np.nan]),
                               ob_time_halfwidth=np.array([6.0, np.nan]), lead_var=np.array([0, 0, 1, 1]), ob_group=np.array([0, -1]),
                               ob_var=np.array([0, -1]), impact=np.array([[1.0, 0.5]]), **pt)
    g = 5.0 / 24.0
    xm, Xp = xbm.copy(), Xbp.copy()
    for k, taper in ((0, np.array([1.0, g, 0.5, 0.5 * g, 1.0, 1.0])), (1, np.ones(6))):
        ye = Xp[4 + k].copy()
        varye = ye.var()
        kmat = taper * (Xp @ ye / (M - 1)) / (varye + err[k])
        xm = xm + kmat * (val[k] - xm[4 + k])
        Xp = Xp - np.outer(kmat / (1.0 + np.sqrt(err[k] / (varye + err[k]))), ye)
    np.testing.assert_allclose(got[0], xm, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(got[1], Xp, rtol=1e-14, atol=1e-14)
    S = sl.slab_factor_table(4, 2, lead_time=np.array([0.0, 6.0, 0.0, 6.0]), ob_time=np.array([0.0, np.nan]),
                             ob_time_halfwidth=np.array([6.0, np.nan]), lead_var=np.array([0, 0, 1, 1]), ob_group=np.array([0, -1]),
                             impact=np.array([[1.0, 0.5]]))
    np.testing.assert_allclose(S, [[1.0, g, 0.5, 0.5 * g], [1.0, 1.0, 1.0, 1.0]], rtol=1e-15)
    # beyond 2 tau the factor is exactly 0
    assert sl.temporal_factor(np.array([12.0, 13.0, np.nan]), 0.0, 6.0).tolist() == [0.0, 0.0, 1.0]


# ---- the Python surface ----------------------------------------------------------------------------------------------
def _state_obs(validtime=None, time_localize_radius=None, **ok):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(20, 60, 4), np.linspace(200, 280, 5), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((3, 2, 4, 5, 6)), lat, lon, varnames=["t2m", "precip", "psfc"],
                                     validtime=validtime)
    obs = [Observation(value=0.0, error=1.0, lat=40.0, lon=240.0, assimilate_this=True, localize_radius=800.0, **ok)]
    obs[0].time_localize_radius = time_localize_radius
    return state, obs


def test_time_localize_radius_is_an_attribute_and_the_constructor_is_as_it_was():
    """The constructor's parameter list is pinned (the reference's plus vert_localize_radius): the temporal half-width is an
    attribute of the ob, None until it is set, and survives a copy."""
    from copy import deepcopy
    from efa_xray_amd import Observation
    assert "time_localize_radius" not in inspect.signature(Observation.__init__).parameters
    ob = Observation(time=3.0)
    assert ob.time_localize_radius is None
    ob.time_localize_radius = 2
    assert ob.time_localize_radius == 2 and deepcopy(ob).time_localize_radius == 2 and Observation().time_localize_radius is None
    ob.time_localize_radius = None
    assert ob.time_localize_radius is None


@pytest.mark.parametrize("bad", [0.0, -1.0, np.inf, np.nan, "x"])
def test_a_bad_temporal_halfwidth_is_refused(bad):
    from efa_xray_amd import EnSRF, Observation
    ob = Observation(time=0.0)
    ob.time_localize_radius = 3.0
    with pytest.raises(ValueError, match="time_localize_radius"):
        ob.time_localize_radius = bad
    assert ob.time_localize_radius == 3.0                    # (a refused value leaves the old one)

    class Duck(Observation):                                 # an ob class of the caller's own, without the check: EnSRF checks again
        time_localize_radius = None

    state, obs = _state_obs(time=0, obtype="t2m")
    duck = Duck(value=0.0, error=1.0, lat=40.0, lon=240.0, time=0, obtype="t2m", assimilate_this=True, localize_radius=800.0)
    duck.time_localize_radius = bad
    with pytest.raises(ValueError, match="time_localize_radius"):
        EnSRF(state, [duck], loc="GC", time_localize=True, verbose=False)


def test_ensrf_refuses_unsupported_slab_settings_before_any_device_work(monkeypatch):
    from efa_xray_amd import EnSRF
    from efa_xray_amd.assimilation.adaptive_inflation import AdaptiveInflation
    state, obs = _state_obs(time=0, obtype="t2m", time_localize_radius=3.0)

    def stop(self):
        raise AssertionError("device work before the check")

    monkeypatch.setattr(EnSRF, "_context", stop)
    ok = {"t2m": {"precip": 0.0, "psfc": 0.25}, "gauge": {"t2m": 0.5}}
    EnSRF(state, obs, loc="GC", time_localize=True, var_impact=ok, verbose=False)
    EnSRF(state, obs, loc="GC", var_impact={"t2m": {"t2m": 1.0}}, verbose=False)
    EnSRF(state, obs, loc=False, time_localize=False, var_impact={}, verbose=False)     # off: nothing to refuse
    for kw in (dict(time_localize=True), dict(var_impact=ok)):
        for loc in (False, None):
            with pytest.raises(ValueError, match="loc='GC'"):
                EnSRF(state, obs, loc=loc, verbose=False, **kw)
        with pytest.raises(ValueError, match="adaptive_inflation"):
            EnSRF(state, obs, loc="GC", verbose=False, adaptive_inflation=AdaptiveInflation(state, ("spatial", None, (1.0, 0.6))), **kw)
    for bad in (-0.1, 1.5, np.nan, np.inf, "x"):
        with pytest.raises(ValueError, match="var_impact"):
            EnSRF(state, obs, loc="GC", var_impact={"t2m": {"precip": bad}}, verbose=False)
    with pytest.raises(ValueError, match="must be 1"):
        EnSRF(state, obs, loc="GC", var_impact={"t2m": {"t2m": 0.5}}, verbose=False)
    with pytest.raises(ValueError, match="not a state variable"):
        EnSRF(state, obs, loc="GC", var_impact={"t2m": {"u10": 0.5}}, verbose=False)
    with pytest.raises(ValueError, match="dict"):
        EnSRF(state, obs, loc="GC", var_impact=[("t2m", 0.5)], verbose=False)
    obs[0].time = np.inf
    with pytest.raises(ValueError, match="not finite"):
        EnSRF(state, obs, loc="GC", time_localize=True, verbose=False)
    obs[0].time = None                                   # an ob without a time is allowed: it tapers nothing in time
    EnSRF(state, obs, loc="GC", time_localize=True, verbose=False)
    with pytest.raises(TypeError):
        EnSRF(state, obs, loc="GC", time_localise=True, verbose=False)


def test_time_lags_of_datetime64_and_numeric_validtime():
    from efa_xray_amd import Observation
    vt = np.array(["2020-01-01T00", "2020-01-01T06"], dtype="datetime64[s]")
    lags = time_lags(vt, [vt[0], vt[1], "2020-01-01T03:30", np.datetime64("2019-12-31T12", "h"), None])
    assert lags[:4].tolist() == [0.0, 6.0, 3.5, -12.0] and np.isnan(lags[4])
    with pytest.raises(ValueError, match="not finite"):
        time_lags(vt, [np.datetime64("NaT")])
    num = time_lags(np.array([3600.0, 7200.0, 10800.0]), [3600, 9000.0, None])
    assert num[:2].tolist() == [0.0, 5400.0] and np.isnan(num[2])
    with pytest.raises(ValueError, match="not finite"):
        time_lags(np.arange(3.0), [np.nan])
    # the arrays the context gets: slabs variable-major, then valid time
    state, obs = _state_obs(validtime=vt, time=vt[1], obtype="precip", time_localize_radius=4.0)
    obs.append(Observation(obtype="gauge", time=None, lat=40.0, lon=240.0))
    obs.append(Observation(obtype="wind", time="2020-01-01T01", lat=40.0, lon=240.0))
    kw = ob_slab(state, obs, slab_setting(state, "GC", True, {"precip": {"t2m": 0.0}, "gauge": {"psfc": 0.5}}))
    assert kw["n_lead"] == 6 and kw["P"] == 3
    assert kw["lead_time"].tolist() == [0.0, 6.0] * 3 and kw["lead_var"].tolist() == [0, 0, 1, 1, 2, 2]
    assert kw["ob_time"][0] == 6.0 and np.isnan(kw["ob_time"][1]) and kw["ob_time"][2] == 1.0
    assert kw["ob_time_halfwidth"][0] == 4.0 and np.isnan(kw["ob_time_halfwidth"][1:]).all()
    assert kw["ob_group"].tolist() == [0, 1, -1] and kw["ob_var"].tolist() == [1, -1, -1]
    assert kw["impact"].tolist() == [[0.0, 1.0, 1.0], [1.0, 1.0, 0.5]]
    only_var = ob_slab(state, obs, slab_setting(state, "GC", False, {"precip": {"t2m": 0.0}}))
    assert "lead_time" not in only_var and "impact" in only_var
    assert slab_setting(state, "GC", False, None) is None and slab_setting(state, False, False, {}) is None


def test_slab_entry_points_are_registered():
    import ctypes
    from efa_xray_amd import _lib
    res, args = _lib.SIGNATURES["efa_ctx_set_slab_localization"]
    assert res is ctypes.c_int and len(args) == 12
    assert len(_lib.SIGNATURES["efa_slab_factor_table"][1]) == 4
    lib = _lib.load_library()
    assert lib.efa_ctx_set_slab_localization(None, 1, None, None, 0, 0, None, None, None, None, 0, None) < 0
    assert b"null context" in lib.efa_last_error()
    assert lib.efa_slab_factor_table(None, 0, 0, None) < 0
    assert b"null context" in lib.efa_last_error()
