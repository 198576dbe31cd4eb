"""Observation impact (EFSO) without a GPU: the NumPy helper tests/_efso.py against cases worked by hand and its
unlocalised closed form, the C entry point's declaration, binding and export, and the argument checks of `observation_impact`
that come before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import _efso
from conftest import ROOT
from oracle.ensrf_oracle import gaspari_cohn, localize_state


def test_efso_on_a_case_worked_by_hand():
    """2 rows (one column, two slabs), 1 ob, M = 3.  Xf' = [[-1, 0, 1], [2, -2, 0]], Ya' = [1, -1, 0]: dots -1 and 4.
    v = (0.5, -2), d = 3, r = 2, the ob on the column (horizontal taper 1), slab coordinates 0 and 10, ob at 0 with vertical
    half-width 1: factors GC(0) = 1 and GC(10 >= 2) = exactly 0.  J = (1/2)(3/2)(1 * 0.5 * -1 + 0 * -2 * 4) = -0.375, and the
    absolute sum A = (1/2)(3/2)(0.5 * (1 + 0 + 0)) = 0.375.  Without the vertical factor the second row enters:
    J = 0.75 (-0.5 - 8) = -6.375, A = 0.75 (0.5 * 1 + 2 * (2 + 2 + 0)) = 6.375."""
    Xf = np.array([[4.0, 5.0, 6.0], [12.0, 8.0, 10.0]])
    Ya = np.array([[3.0, 1.0, 2.0]])
    v = np.array([0.5, -2.0])
    geo = dict(grid_lat=[40.0], grid_lon=[260.0], ob_lat=[40.0], ob_lon=[260.0], ob_halfwidth=[500.0], n_lead=2)
    assert gaspari_cohn(np.array([10.0]), 1.0)[0] == 0.0
    J, A = _efso.efso(Xf, Ya, v, [3.0], [2.0], [1], lead_vert=[0.0, 10.0], ob_vert=[0.0], ob_vert_halfwidth=[1.0], **geo)
    assert J[0] == -0.375 and A[0] == 0.375
    J, A = _efso.efso(Xf, Ya, v, [3.0], [2.0], [1], **geo)
    assert J[0] == -6.375 and A[0] == 6.375
    # a NaN slab takes factor 1, an ob without vertical information the horizontal taper alone
    J, _ = _efso.efso(Xf, Ya, v, [3.0], [2.0], [1], lead_vert=[0.0, np.nan], ob_vert=[0.0], ob_vert_halfwidth=[1.0], **geo)
    assert J[0] == -6.375
    J, _ = _efso.efso(Xf, Ya, v, [3.0], [2.0], [1], lead_vert=[0.0, 10.0], ob_vert=[np.nan], ob_vert_halfwidth=[1.0], **geo)
    assert J[0] == -6.375
    # unlocalised: every row with weight 1
    J, A = _efso.efso(Xf, Ya, v, [3.0], [2.0], [1])
    assert J[0] == -6.375 and A[0] == 6.375


def test_efso_unlocalised_closed_form_and_unused_obs():
    rng = np.random.default_rng(5)
    rows, M, P = 300, 9, 12
    Xf = rng.standard_normal((rows, M)) + 10.0
    Ya = rng.standard_normal((P, M)) - 3.0
    v = rng.standard_normal(rows)
    d = rng.standard_normal(P)
    r = rng.uniform(0.5, 2.0, P)
    used = np.ones(P, dtype=bool)
    used[[2, 7]] = False
    J, A = _efso.efso(Xf, Ya, v, d, r, used)
    Xp = Xf - Xf.mean(axis=1, keepdims=True)
    Yp = Ya - Ya.mean(axis=1, keepdims=True)
    closed = d / r / (M - 1) * (Yp @ (Xp.T @ v))
    assert np.all(np.abs(J - closed)[used] <= 1e-12 * A[used])
    assert np.all(A[used] > 0) and np.all(A[used] >= np.abs(J[used]))
    assert np.all(J[~used] == 0.0) and np.all(A[~used] == 0.0)


def test_efso_taper_is_the_oracles():
    rng = np.random.default_rng(6)
    glat, glon = np.meshgrid(np.linspace(30, 50, 4), np.linspace(250, 270, 5), indexing="ij")
    glat, glon = glat.reshape(-1), glon.reshape(-1)
    ncol, n_lead, M = glat.size, 3, 6
    Xf = rng.standard_normal((n_lead * ncol, M))
    Ya = rng.standard_normal((1, M))
    v = rng.standard_normal(n_lead * ncol)
    J, _ = _efso.efso(Xf, Ya, v, [1.5], [0.7], [1], grid_lat=glat, grid_lon=glon, ob_lat=[41.0], ob_lon=[262.0],
                      ob_halfwidth=[700.0], n_lead=n_lead)
    rho = np.tile(localize_state(glat, glon, 41.0, 262.0, 700.0), n_lead)
    assert 0 < np.count_nonzero(rho) < rho.size
    Xp = Xf - Xf.mean(axis=1, keepdims=True)
    Yp = Ya - Ya.mean(axis=1, keepdims=True)
    want = (1.0 / (M - 1)) * (1.5 / 0.7) * np.sum(rho * v * (Xp @ Yp[0]))
    assert abs(J[0] - want) <= 1e-14 * abs(want)
    assert _efso.tolerance(2000, 1000) == 1e-9 and _efso.tolerance(10 ** 7, 100) == 4e9 * 2.0 ** -53


def test_entry_point_is_declared_bound_exported_and_refuses_a_null_context():
    from efa_xray_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efa_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+efa_obs_impact_dev\s*\(([^)]*)\)", text)
    assert m, "efa_obs_impact_dev is not declared in include/efa_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _lib.SIGNATURES["efa_obs_impact_dev"]
    assert res is ctypes.c_int and len(args) == len(params) == 19
    lib = _lib.load_library()
    assert hasattr(lib, "efa_obs_impact_dev")
    assert hasattr(_lib.Context, "obs_impact")
    rc = lib.efa_obs_impact_dev(None, 0, 0, 0, None, None, None, None, None, None, 0, None, None, None, None, None, 0, 0, None)
    assert rc == _lib.EFA_ERR_INVALID
    assert b"null context" in lib.efa_last_error()
    import efa_xray_amd
    from efa_xray_amd.postprocess import observation_impact
    assert efa_xray_amd.observation_impact is observation_impact and "observation_impact" in efa_xray_amd.__all__


def _states(dtype=np.float64):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(1)
    nvar, nt, ny, nx, M = 2, 3, 4, 5, 6
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    prior = EnsembleState.from_array(rng.standard_normal((nvar, nt, ny, nx, M)), lat, lon)
    post = EnsembleState.from_array(rng.standard_normal((nvar, nt, ny, nx, M)), lat, lon)
    if dtype != np.float64:
        prior, post = prior.astype(dtype), post.astype(dtype)
    ob = Observation(value=1.0, obtype=prior.vars()[0], time=prior.ensemble_times()[0], error=1.0, lat=35.0, lon=255.0,
                     localize_radius=500.0)
    ob.assimilated = True
    ver = dict((n, np.zeros((nt, ny, nx))) for n in prior.vars())
    return prior, post, [ob], ver


def test_observation_impact_refuses_bad_arguments_before_any_device_call():
    from efa_xray_amd import observation_impact
    prior, post, obs, ver = _states()
    name = prior.vars()[0]
    p32, q32, _, _ = _states(np.float32)
    with pytest.raises(ValueError, match="float64"):
        observation_impact(p32, q32, obs, ver)
    with pytest.raises(ValueError, match="float64"):
        observation_impact(prior, q32, obs, ver)
    bad = dict(ver)
    bad[name] = np.zeros((3, 4, 4))
    with pytest.raises(ValueError, match="shape"):
        observation_impact(prior, post, obs, bad)
    with pytest.raises(ValueError, match="non-negative"):
        observation_impact(prior, post, obs, ver, norm={name: -1.0})
    with pytest.raises(ValueError, match="non-negative"):
        observation_impact(prior, post, obs, ver, norm={name: np.array([1.0, -2.0, 1.0]).reshape(3, 1, 1)})
    with pytest.raises(ValueError, match="loc='GC'"):
        observation_impact(prior, post, obs, ver, vert_coord=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="vert_coord"):
        observation_impact(prior, post, obs, ver, loc="GC", vert_coord=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="loc="):
        observation_impact(prior, post, obs, ver, loc="cutoff")
    assert not hasattr(obs[0], "impact") or obs[0].impact is None


def test_error_terms_weights_and_actual():
    """v = c (e^a + e^b) and actual = sum c (e^a^2 - e^b^2), zero where the verification is NaN or the variable is missing."""
    from efa_xray_amd.postprocess.impact import _error_terms
    prior, post, _, _ = _states()
    names = prior.vars()
    nt, ny, nx = 3, 4, 5
    rng = np.random.default_rng(2)
    ver = {names[0]: rng.standard_normal((nt, ny, nx))}
    ver[names[0]][1, 2, 3] = np.nan
    c = rng.uniform(0.0, 2.0, (nt, 1, 1))
    v, actual = _error_terms(prior, post, ver, {names[0]: c})
    v = v.reshape(2, nt, ny, nx)
    eb = prior.variables[names[0]].mean(axis=-1) - ver[names[0]]
    ea = post.variables[names[0]].mean(axis=-1) - ver[names[0]]
    ok = ~np.isnan(ver[names[0]])
    assert np.all(v[1] == 0.0) and v[0][1, 2, 3] == 0.0
    assert np.allclose(v[0][ok], (c * (ea + eb))[ok], rtol=1e-15, atol=0)
    assert np.isclose(actual, np.sum((c * (ea ** 2 - eb ** 2))[ok]), rtol=1e-13)


def test_impact_kernels_fit_their_register_budget():
    """No vector spills in any instantiation of the localised kernel; two waves per SIMD (<= 256 registers) up to 96 members, as
    its launch bounds say, and the configs[2] width (80 members) with room to spare."""
    from efa_xray_amd import _lib
    from _codeobj import gc_kernel_fragment, kernel_table
    lib = kernel_table(_lib.LIB_PATH)
    shapes = [(mp, False) for mp in range(4, 105, 4)] + [(64, True)]   # 4 .. 104 members; the pieces of 64 above
    tab = {}
    for fam in ("plain", "vloc"):
        for mp, wide in shapes:
            (n,) = [n for n in lib if gc_kernel_fragment("impact", fam, "f64", mp, wide) in n]
            tab[n] = (mp, lib[n])
    assert len(tab) == 2 * 26 + 2            # plain and vertical; with the slab table's 26 + 1 that is every instantiation
    assert len([n for n in lib if "k_sweep_gc_lane_impact" in n]) == 2 * 26 + 2 + 26 + 1
    for n, (mp, k) in tab.items():
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0, (n, k[".vgpr_count"])
        if mp <= 96:
            assert k[".vgpr_count"] <= 256, (n, k[".vgpr_count"])
        assert 2 * k[".group_segment_fixed_size"] <= 160 * 1024, (n, k[".group_segment_fixed_size"])
    for fam in ("plain", "vloc"):
        (k,) = [k for n, (mp, k) in tab.items() if gc_kernel_fragment("impact", fam, "f64", 80, False) in n]
        assert k[".vgpr_count"] <= 232
