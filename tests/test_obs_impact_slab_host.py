"""Observation impact under the temporal and variable tapers without a GPU: the NumPy helper tests/_efso_slab.py on
a case worked by hand, the new entry point's declaration, binding and export, the keyword checks of `observation_impact` that come
before any device call, and the register and LDS budget of the new kernels read from the code object."""
import ctypes
import os
import re

import numpy as np
import pytest

import _efso
import _efso_slab
from conftest import ROOT
from oracle.ensrf_oracle import gaspari_cohn
from test_obs_impact_host import _states


def test_efso_slab_on_a_case_worked_by_hand():
    """One column, 2 slabs (times 0 and 6, variables 0 and 1), 2 obs, M = 3.  Xf' = [[-1, 0, 1], [2, -2, 0]], v = (0.5, -2), both
    obs on the column (horizontal taper 1).
    Ob 0: Ya' = [1, -1, 0], dots -1 and 4, d / r = 3 / 2; time 0 with tau 6, so T = GC(0) = 1 and t = GC(6, 6) = 5/24; its obtype
    has impact 1 on variable 0 and 0.5 on variable 1: S = (1, t / 2).  J = (1/2)(3/2)(0.5 * -1 + (t / 2) * -2 * 4) = 0.75 (-0.5 - 4 t)
    = -1, A = 0.75 (0.5 * 1 + (t / 2) * 2 * 4) = 1.
    Ob 1: Ya' = [-1, 0, 1], dots 2 and -2, d / r = 2 / 4; no time and no impact row: S = (1, 1).  J = (1/2)(1/2)(0.5 * 2 + -2 * -2)
    = 1.25, and A = 0.25 (0.5 * 2 + 2 * 2) = 1.25."""
    Xf = np.array([[4.0, 5.0, 6.0], [12.0, 8.0, 10.0]])
    Ya = np.array([[3.0, 1.0, 2.0], [1.0, 2.0, 3.0]])
    v = np.array([0.5, -2.0])
    geo = dict(grid_lat=[40.0], grid_lon=[260.0], ob_lat=[40.0, 40.0], ob_lon=[260.0, 260.0], ob_halfwidth=[500.0, 800.0], n_lead=2)
    slab = dict(lead_time=[0.0, 6.0], ob_time=[0.0, np.nan], ob_time_halfwidth=[6.0, 6.0], lead_var=[0, 1], ob_group=[0, -1],
                impact=[[1.0, 0.5]])
    t = gaspari_cohn(np.array([6.0]), 6.0)[0]
    assert abs(t - 5.0 / 24.0) <= 1e-16
    J, A = _efso_slab.efso_slab(Xf, Ya, v, [3.0, 2.0], [2.0, 4.0], [1, 1], **geo, **slab)
    assert J[0] == 0.75 * (0.5 * -1.0 + (t * 0.5) * -2.0 * 4.0) and abs(J[0] + 1.0) <= 1e-15
    assert A[0] == 0.75 * (0.5 * 1.0 + (t * 0.5) * 2.0 * 4.0) and abs(A[0] - 1.0) <= 1e-15
    assert J[1] == 1.25 and A[1] == 1.25
    # tau 2.5: slab 1 lies beyond 2 tau, its factor is exactly 0 and only row 0 is left
    J, A = _efso_slab.efso_slab(Xf, Ya, v, [3.0, 2.0], [2.0, 4.0], [1, 1], **geo, **dict(slab, ob_time_halfwidth=[2.5, 6.0]))
    assert J[0] == -0.375 and A[0] == 0.375 and J[1] == 1.25
    # impact 0 on variable 1 does the same; an ob that is not used comes back as 0.0
    J, A = _efso_slab.efso_slab(Xf, Ya, v, [3.0, 2.0], [2.0, 4.0], [1, 0], **geo, **dict(slab, impact=[[1.0, 0.0]]))
    assert J[0] == -0.375 and A[0] == 0.375 and J[1] == 0.0 and A[1] == 0.0
    # the vertical factor enters the table as well: slab 1 out of the vertical reach of ob 1
    J, _ = _efso_slab.efso_slab(Xf, Ya, v, [3.0, 2.0], [2.0, 4.0], [1, 1], lead_vert=[0.0, 10.0], ob_vert=[np.nan, 0.0],
                                ob_vert_halfwidth=[1.0, 1.0], **geo, **slab)
    assert abs(J[0] + 1.0) <= 1e-15 and J[1] == 0.25 * (0.5 * 2.0)
    # without any factor it is _efso.efso
    J, A = _efso_slab.efso_slab(Xf, Ya, v, [3.0, 2.0], [2.0, 4.0], [1, 1], **geo)
    Jr, Ar = _efso.efso(Xf, Ya, v, [3.0, 2.0], [2.0, 4.0], [1, 1], **geo)
    assert np.array_equal(J, Jr) and np.array_equal(A, Ar) and J[0] == -6.375


def test_entry_point_is_declared_bound_exported_and_refuses_a_null_context():
    from efa_xray_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efa_hip.h")).read(), flags=re.S)
    params = {}
    for name in ("efa_obs_impact_dev", "efa_obs_impact_slab_dev"):
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, text)
        assert m, "%s is not declared in include/efa_hip.h" % name
        params[name] = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params["efa_obs_impact_slab_dev"] == params["efa_obs_impact_dev"]         # the same parameter list
    res, args = _lib.SIGNATURES["efa_obs_impact_slab_dev"]
    assert res is ctypes.c_int and len(args) == 19 and args == _lib.SIGNATURES["efa_obs_impact_dev"][1]
    lib = _lib.load_library()
    assert hasattr(lib, "efa_obs_impact_slab_dev") and hasattr(_lib.Context, "obs_impact_slab")
    assert lib.efa_abi_version() == 1
    rc = lib.efa_obs_impact_slab_dev(None, 0, 0, 0, None, None, None, None, None, None, 0, None, None, None, None, None, 0, 0, None)
    assert rc == _lib.EFA_ERR_INVALID
    assert b"null context" in lib.efa_last_error()


def test_observation_impact_refuses_its_keywords_as_ensrf_does():
    """The same ValueErrors as EnSRF(...), from the same functions, before any device call."""
    import inspect
    from efa_xray_amd import EnSRF, observation_impact
    prior, post, obs, ver = _states()
    a, b = prior.vars()
    names = list(inspect.signature(observation_impact).parameters)
    assert names[-2:] == ["time_localize", "var_impact"] and names[:8] == ["prior", "post", "obs", "verification", "norm", "loc",
                                                                            "vert_coord", "device"]
    cases = [
        (dict(time_localize=True), "time_localize needs loc='GC'"),
        (dict(var_impact={a: {b: 0.5}}), "var_impact needs loc='GC'"),
        (dict(loc="GC", var_impact=[(a, b, 0.5)]), "var_impact must be a dict"),
        (dict(loc="GC", var_impact={a: 0.5}), "must be a dict"),
        (dict(loc="GC", var_impact={a: {"nosuch": 0.5}}), "not a state variable"),
        (dict(loc="GC", var_impact={a: {b: 1.5}}), r"in \[0, 1\]"),
        (dict(loc="GC", var_impact={a: {b: "x"}}), "expected a number"),
        (dict(loc="GC", var_impact={a: {a: 0.5}}), "must be 1"),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg) as e_imp:
            observation_impact(prior, post, obs, ver, **kw)
        with pytest.raises(ValueError, match=msg) as e_srf:
            EnSRF(prior, obs, verbose=False, **kw)
        assert str(e_imp.value) == str(e_srf.value)
    obs[0].time_localize_radius = 3.0
    obs[0].time = "not a time"
    with pytest.raises(ValueError, match="observation times"):
        observation_impact(prior, post, obs, ver, loc="GC", time_localize=True)
    p32, q32, o32, _ = _states(np.float32)
    with pytest.raises(ValueError, match="float64"):                        # float32 states still raise
        observation_impact(p32, q32, o32, ver, loc="GC", time_localize=True)
    assert not hasattr(obs[0], "impact") or obs[0].impact is None


def test_slab_impact_kernels_fit_their_register_budget():
    """The 27 instantiations of the slab-table form (4 .. 104 members and the pieces of 64): no vector spills, no scratch, at most
    256 registers up to 96 members (two waves per SIMD, as the launch bounds say), two workgroups of LDS per CU; the plain and the
    vertical form keep their 54."""
    from efa_xray_amd import _lib
    from _codeobj import gc_kernel_fragment, kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    slab = {}
    for mp, wide in [(mp, False) for mp in range(4, 105, 4)] + [(64, True)]:
        (n,) = [n for n in tab if gc_kernel_fragment("impact", "slab", "f64", mp, wide) in n]
        slab[n] = (mp, tab[n])
    assert len(slab) == 26 + 1
    assert len([n for n in tab if "k_sweep_gc_lane_impact" in n]) == 2 * 26 + 2 + len(slab)
    widths = set()
    for n, (mp, k) in slab.items():
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0, (n, k[".vgpr_count"])
        widths.add(mp)
        if mp <= 96:
            assert k[".vgpr_count"] <= 256, (n, k[".vgpr_count"])
        assert 2 * k[".group_segment_fixed_size"] <= 160 * 1024, (n, k[".group_segment_fixed_size"])
    assert widths == set(range(4, 105, 4))
    (k,) = [k for n, (mp, k) in slab.items() if gc_kernel_fragment("impact", "slab", "f64", 80, False) in n]
    assert k[".vgpr_count"] <= 232                                            # the budget 7i gives the configs[2] width
