"""Vertical localisation without a GPU: the NumPy helper (tests/_vertloc.py) against the oracle and a hand-computed
case, the keyword checks of EnSRF / ShardedEnSRF / Observation, and the C entry point's registration."""
import inspect

import numpy as np
import pytest

import _vertloc as vl
from oracle import ensrf_oracle as orc


def _case(seed=3, nvar=2, nt=2, ny=5, nx=6, M=8, P=12):
    rng = np.random.default_rng(seed)
    N = nvar * nt * ny * nx
    glat, glon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(250, 270, nx), indexing="ij")
    X = rng.standard_normal((N, M)) * 2.0 + 1.0
    rows = rng.choice(N, P, replace=False)
    HX = X[rows] + 0.1 * rng.standard_normal((P, M))
    xbm, Xbp = orc.format_prior_state(X, HX)
    col = rows % (ny * nx)
    ob = dict(ob_value=HX.mean(axis=1) + rng.standard_normal(P), ob_error=rng.uniform(0.5, 2.0, P),
              ob_assim=rng.random(P) < 0.8, ob_lat=glat.reshape(-1)[col] + 0.1, ob_lon=glon.reshape(-1)[col] - 0.1,
              ob_halfwidth=rng.uniform(800, 2000, P))
    return xbm, Xbp, N, ob, glat, glon, (nvar, nt, ny, nx)


def test_helper_equals_oracle_bit_for_bit_without_vertical_information():
    xbm, Xbp, N, ob, glat, glon, shape = _case()
    ref = orc.ensrf_update(xbm, Xbp, N, ob["ob_value"], ob["ob_error"], ob["ob_assim"], loc="GC", ob_lat=ob["ob_lat"],
                           ob_lon=ob["ob_lon"], ob_halfwidth=ob["ob_halfwidth"], grid_lat=glat, grid_lon=glon, state_shape=shape)
    P = len(ob["ob_value"])
    for lead, ov, oh in ((None, None, None),
                         (np.linspace(0, 3, 4), np.full(P, np.nan), np.ones(P)),          # coordinates on no ob
                         (np.linspace(0, 3, 4), np.linspace(0, 3, P), np.full(P, np.nan))):  # no half-width on any
        got = vl.ensrf_update_vert(xbm, Xbp, N, lead_vert=lead, ob_vert=ov, ob_vert_halfwidth=oh, grid_lat=glat, grid_lon=glon,
                                   state_shape=shape, **ob)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
            assert np.array_equal(got[2][key], ref[2][key], equal_nan=True)


def test_helper_on_sampled_rows_equals_the_whole_state():
    xbm, Xbp, N, ob, glat, glon, shape = _case(seed=5)
    P = len(ob["ob_value"])
    lead = np.array([0.0, 1.0, np.nan, 2.5])
    ov, oh = np.linspace(-0.5, 3.0, P), np.full(P, 1.2)
    full = vl.ensrf_update_vert(xbm, Xbp, N, lead_vert=lead, ob_vert=ov, ob_vert_halfwidth=oh, grid_lat=glat, grid_lon=glon,
                                state_shape=shape, **ob)
    rows = np.array([0, 7, 31, 60, 61, 119])
    sel = np.concatenate([rows, N + np.arange(P)])
    part = vl.ensrf_update_vert(xbm[sel], Xbp[sel], len(rows), lead_vert=lead, ob_vert=ov, ob_vert_halfwidth=oh, grid_lat=glat,
                                grid_lon=glon, state_shape=shape, rows=rows, **ob)
    np.testing.assert_allclose(part[0], full[0][sel], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(part[1], full[1][sel], rtol=1e-13, atol=1e-13)


def test_helper_matches_a_hand_computed_two_slab_two_ob_case():
    """One column, two slabs (z = 0 and 1), two obs that are the slabs' own values: ob 0 at z = 0 with c = 1, ob 1 without a
    vertical coordinate.  The horizontal taper is 1 everywhere (same point), so only the vertical factor differs from the
    horizontal-only update: ob 0 tapers slab 1 by GC(r = 1) = 5/24, and ob 1 (no coordinate) tapers everything by 1."""
    M = 4
    X = np.array([[1.0, 2.0, 0.0, -1.0], [0.5, -0.5, 1.5, 2.5]])
    HX = X.copy()
    xbm, Xbp = orc.format_prior_state(X, HX)
    val, err, asm = np.array([1.0, 0.0]), np.array([0.5, 1.0]), np.array([True, True])
    glat, glon = np.array([[40.0]]), np.array([[260.0]])
    ob = dict(ob_value=val, ob_error=err, ob_assim=asm, ob_lat=np.array([40.0, 40.0]), ob_lon=np.array([260.0, 260.0]),
              ob_halfwidth=np.array([500.0, 500.0]))
    lead = np.array([0.0, 1.0])
    got = vl.ensrf_update_vert(xbm, Xbp, 2, lead_vert=lead, ob_vert=np.array([0.0, np.nan]), ob_vert_halfwidth=np.array([1.0, np.nan]),
                               grid_lat=glat, grid_lon=glon, state_shape=(2, 1, 1, 1), **ob)
    # by hand: rows [slab 0, slab 1, ob 0, ob 1]; ob 0 tapers them by [1, g, 1, 1] with g = GC(r = 1) = -1/4 + 1/2 + 5/8 - 5/3 + 1
    g = -0.25 + 0.5 + 0.625 - 5.0 / 3.0 + 1.0
    xm = xbm.copy()
    Xp = Xbp.copy()
    for k, taper in ((0, np.array([1.0, g, 1.0, 1.0])), (1, np.ones(4))):
        ye = Xp[2 + k].copy()
        varye = ye.var()
        kmat = taper * (Xp @ ye / (M - 1)) / (varye + err[k])
        innov = val[k] - xm[2 + k]
        xm = xm + kmat * innov
        beta = 1.0 / (1.0 + np.sqrt(err[k] / (varye + err[k])))
        Xp = Xp - np.outer(beta * kmat, ye)
    assert abs(g - 5.0 / 24.0) < 1e-15
    np.testing.assert_allclose(got[0], xm, rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(got[1], Xp, rtol=1e-14, atol=1e-14)
    # and the vertical factor did something: without it slab 1 moves differently
    plain = orc.ensrf_update(xbm, Xbp, 2, val, err, asm, loc="GC", ob_lat=ob["ob_lat"], ob_lon=ob["ob_lon"],
                             ob_halfwidth=ob["ob_halfwidth"], grid_lat=glat, grid_lon=glon, state_shape=(2, 1, 1, 1))
    assert not np.allclose(plain[0][1], got[0][1])
    assert np.array_equal(plain[2]["prior_mean"][:1], got[2]["prior_mean"][:1])


def test_vertical_factor_nan_and_cutoff():
    f = vl.vertical_factor(np.array([0.0, 0.5, 2.0, 3.0, np.nan]), 0.0, 1.0)
    assert f[0] == 1.0 and 0.0 < f[1] < 1.0 and f[2] == 0.0 and f[3] == 0.0 and f[4] == 1.0


# ---- the Python surface ----------------------------------------------------------------------------------------------
def _state_obs(loc_radius=800.0, **vk):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(20, 60, 4), np.linspace(200, 280, 5), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((3, 2, 4, 5, 6)), lat, lon)
    obs = [Observation(value=0.0, error=1.0, lat=40.0, lon=240.0, assimilate_this=True, localize_radius=loc_radius, **vk)]
    return state, obs


def test_observation_keeps_its_positional_signature():
    from efa_xray_amd import Observation
    names = list(inspect.signature(Observation.__init__).parameters)[1:]
    assert names == ["value", "obtype", "time", "error", "lat", "lon", "vert", "prior_mean", "post_mean", "prior_var", "post_var",
                     "assimilate_this", "description", "localize_radius", "vert_localize_radius"]
    ob = Observation(1.0, "T", 0, 2.0, 10.0, 20.0, 850.0, None, None, None, None, True, "d", 300.0)
    assert (ob.vert, ob.localize_radius, ob.vert_localize_radius, ob.assimilate_this) == (850.0, 300.0, None, True)
    assert Observation(vert=1.0, vert_localize_radius=2).vert_localize_radius == 2


@pytest.mark.parametrize("bad", [0.0, -1.0, np.inf, np.nan, "x"])
def test_observation_rejects_a_bad_vertical_halfwidth(bad):
    from efa_xray_amd import Observation
    with pytest.raises(ValueError):
        Observation(vert=1.0, vert_localize_radius=bad)


def test_ensrf_rejects_unsupported_vertical_settings():
    from efa_xray_amd import EnSRF
    from efa_xray_amd.assimilation.adaptive_inflation import AdaptiveInflation
    state, obs = _state_obs(vert=1.0, vert_localize_radius=1.0)
    Z = np.arange(6.0).reshape(3, 2)
    for loc in (False, None):
        with pytest.raises(ValueError, match="loc='GC'"):
            EnSRF(state, obs, loc=loc, vert_coord=Z, verbose=False)
    with pytest.raises(ValueError, match="shape"):
        EnSRF(state, obs, loc="GC", vert_coord=Z.T, verbose=False)
    with pytest.raises(ValueError, match="shape"):
        EnSRF(state, obs, loc="GC", vert_coord=Z.reshape(-1), verbose=False)
    with pytest.raises(ValueError, match="infinite"):
        EnSRF(state, obs, loc="GC", vert_coord=np.where(Z > 4, np.inf, Z), verbose=False)
    with pytest.raises(ValueError, match="adaptive_inflation"):
        EnSRF(state, obs, loc="GC", vert_coord=Z, verbose=False, adaptive_inflation=AdaptiveInflation(state, ("spatial", None, (1.0, 0.6))))
    for bad in (0.0, -2.0, np.inf, np.nan):
        obs[0].vert_localize_radius = bad                     # (set after construction: checked again by EnSRF)
        with pytest.raises(ValueError, match="vert_localize_radius"):
            EnSRF(state, obs, loc="GC", vert_coord=Z, verbose=False)
    obs[0].vert_localize_radius = 1.0
    Zn = Z.copy()
    Zn[1, 0] = np.nan                                         # NaN slabs are allowed
    EnSRF(state, obs, loc="GC", vert_coord=Zn, verbose=False)
    EnSRF(state, obs, loc="GC", vert_coord=None, verbose=False, adaptive_inflation=AdaptiveInflation(state, ("spatial", None, (1.0, 0.6))))


def test_sharded_ensrf_rejects_unsupported_vertical_settings():
    from efa_xray_amd.distributed import ShardedEnSRF
    sh = ShardedEnSRF(engine=None, n_lead=4, ncol=10, M=5)
    ob = dict(value=np.zeros(3), error=np.ones(3), assim=np.ones(3, bool), loc="GC", lat=np.zeros(3), lon=np.zeros(3),
              halfwidth=np.ones(3), vert=np.array([0.0, np.nan, 1.0]), vert_halfwidth=np.array([1.0, 1.0, np.nan]))
    z, ov, oh = sh._vertical(ob, np.arange(4.0).reshape(2, 2), 3)
    assert z.shape == (4,) and np.isnan(ov[1]) and np.isnan(oh[2])
    assert sh._vertical(ob, None, 3) == (None, None, None)
    with pytest.raises(ValueError, match="n_lead"):
        sh._vertical(ob, np.arange(3.0), 3)
    with pytest.raises(ValueError, match="loc='GC'"):
        sh._vertical(dict(ob, loc=None), np.arange(4.0), 3)
    with pytest.raises(ValueError, match="vert_halfwidth"):
        sh._vertical(dict(ob, vert_halfwidth=np.array([1.0, 0.0, 1.0])), np.arange(4.0), 3)
    with pytest.raises(ValueError, match="one value per observation"):
        sh._vertical(dict(ob, vert=np.zeros(2)), np.arange(4.0), 3)


def test_vertical_entry_point_is_registered():
    from efa_xray_amd import _lib
    res, args = _lib.SIGNATURES["efa_ctx_set_vertical_localization"]
    assert res is __import__("ctypes").c_int and len(args) == 6
    lib = _lib.load_library()
    assert hasattr(lib, "efa_ctx_set_vertical_localization")
    assert lib.efa_ctx_set_vertical_localization(None, 1, None, 0, None, None) < 0
    assert b"null context" in lib.efa_last_error()
