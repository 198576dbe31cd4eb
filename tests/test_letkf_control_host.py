"""The LETKF's deterministic control analysis without a device: the two routes of the NumPy model of
tests/_letkf_control.py against each other, the control that equals the ensemble mean, the front end's refusals, the symbol's three
declarations, and the scratch of every k_letkf instantiation."""
import os
import re

import numpy as np
import pytest

import _etkf as ek
import _letkf as lk
import _letkf_control as lc
import _letkf_slab as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _the_feature_exists():
    """The model below describes efa_ctx_set_letkf_control: without the entry point there is nothing for it to describe."""
    from efa_xray_amd import _lib
    assert "efa_ctx_set_letkf_control" in _lib.SIGNATURES, "the library has no control analysis"


def _routes(c, tapers):
    xc, yc = lc.control_inputs(c)
    args = (c["X"], c["HX"], xc, yc, c["value"], c["error"], c["assim"]) + tapers
    return lc.control_cycle(*args, route="eigh"), lc.control_cycle(*args, route="solve"), xc, yc


# ---- 1. the two routes of the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead", [(2, 1, 3, 5, 1), (15, 40, 4, 5, 3), (16, 64, 5, 7, 3), (31, 64, 4, 5, 2)])
def test_the_two_routes_agree(M, P, ny, nx, n_lead):
    c = lk.make_case(M, P, ny, nx, n_lead)
    a, b, xc, yc = _routes(c, lc.plain_tapers(c))
    print("M=%d P=%d: cond(A) max %.3g, %d of %d columns reached" % (M, P, a["cond"], a["reached"].sum(), a["reached"].size))
    assert a["cond"] <= 1e4
    for k in ("xc_post", "yc_post"):
        scale = np.abs(a[k]).max()
        err = np.abs(a[k] - b[k]).max()
        print("%s: max abs err %.3e, scale %.3e" % (k, err, scale))
        assert err <= 1e-10 * scale
    assert a["reached"].any() and np.any(a["xc_post"] != xc)
    un = np.flatnonzero(~a["reached"][0])
    rows = (un[None, :] + c["ncol"] * np.arange(n_lead)[:, None]).reshape(-1)
    assert np.array_equal(a["xc_post"][rows], xc[rows]), "an unreached column's control rows changed"
    assert np.array_equal(a["yc_post"][~a["ob_reached"]], yc[~a["ob_reached"]])


def test_the_two_routes_agree_under_slab_groups():
    c = ls.make_case(16, 64, 5, 7, 2, 3, parts="vtc")
    tapers = lc.slab_tapers(c)
    assert tapers[0].shape[0] >= 2
    a, b, _, _ = _routes(c, tapers)
    assert a["cond"] <= 1e4
    for k in ("xc_post", "yc_post"):
        assert np.abs(a[k] - b[k]).max() <= 1e-10 * np.abs(a[k]).max()


# ---- 2. a control that equals the ensemble mean is the ensemble's own analysis mean ---------------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead", [(3, 5, 3, 5, 2), (16, 64, 5, 7, 3)])
def test_a_control_equal_to_the_mean_gives_the_posterior_mean(M, P, ny, nx, n_lead):
    c = lk.make_case(M, P, ny, nx, n_lead)
    ym = ek.ob_priors(c["HX"])[0]
    got = lc.control_cycle(c["X"], c["HX"], c["X"].mean(axis=1), ym, c["value"], c["error"], c["assim"], *lc.plain_tapers(c))
    ref = lk.letkf_cycle(c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                         c["grid_lon"], n_lead)
    want = ref["post"].mean(axis=1)
    assert np.abs(got["xc_post"] - want).max() <= 1e-10 * np.abs(want).max()
    assert np.abs(got["yc_post"] - ref["ym"]).max() <= 1e-10 * np.abs(ref["ym"]).max()


def test_a_nan_estimate_poisons_exactly_the_columns_it_reaches_in_the_model():
    c = lk.make_case(16, 64, 5, 7, 3, hw=(100.0, 400.0))
    tapers = lc.plain_tapers(c)
    rho = tapers[0][0]
    k = int(np.argmax((rho != 0.0).sum(axis=0)))
    hit = rho[:, k] != 0.0
    assert hit.any() and not hit.all()
    xc, yc = lc.control_inputs(c)
    bad = np.array(yc)
    bad[k] = np.nan
    fin = lc.control_cycle(c["X"], c["HX"], xc, yc, c["value"], c["error"], c["assim"], *tapers)
    nan = lc.control_cycle(c["X"], c["HX"], xc, bad, c["value"], c["error"], c["assim"], *tapers)
    rows = lambda cols: (np.flatnonzero(cols)[None, :] + c["ncol"] * np.arange(c["n_lead"])[:, None]).reshape(-1)
    assert np.all(np.isnan(nan["xc_post"][rows(hit)]))
    assert np.array_equal(nan["xc_post"][rows(~hit)], fin["xc_post"][rows(~hit)])


# ---- 3. the front end without a device ------------------------------------------------------------------------------------------------
def _tiny(M=6, nvar=1):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(3)
    lat, lon = np.meshgrid(np.linspace(20, 60, 4), np.linspace(200, 280, 5), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((nvar, 1, 4, 5, M)), lat, lon)
    obs = [Observation(value=0.5, error=1.0, lat=40.0, lon=240.0, localize_radius=1000.0)]
    return state, obs, lat, lon


def test_the_keyword_validates_the_control_before_any_device_work(monkeypatch):
    from efa_xray_amd import EnsembleState, LETKF, SlabLETKF, EnSRF, ETKF
    from efa_xray_amd.assimilation.assimilation import Assimilation

    def no_device(self):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(Assimilation, "_context", no_device)
    state, obs, lat, lon = _tiny()
    rng = np.random.default_rng(4)
    ctrl = EnsembleState.from_array(rng.standard_normal((1, 1, 4, 5, 1)), lat, lon)
    for cls in (LETKF, SlabLETKF):
        f = cls(state, obs, verbose=False, control=ctrl)
        assert f.control is ctrl and f.last_control is None
        assert cls(state, obs, verbose=False).control is None
        for bad in (1.5, np.zeros(20), state,                                                # not a state; more than one member
                    EnsembleState.from_array(rng.standard_normal((2, 1, 4, 5, 1)), lat, lon),  # other variables
                    EnsembleState.from_array(rng.standard_normal((1, 1, 4, 5, 1)), lat, lon, varnames=["other"]),
                    EnsembleState.from_array(rng.standard_normal((1, 1, 4, 5, 1)), lat + 1.0, lon),  # another grid
                    EnsembleState.from_array(rng.standard_normal((1, 1, 5, 4, 1)), lat.T, lon.T)):
            with pytest.raises(ValueError, match="control"):
                cls(state, obs, verbose=False, control=bad)
        for stride in (2, (2, 3)):
            with pytest.raises(ValueError, match="weight interpolation of w\\^c"):
                cls(state, obs, verbose=False, control=ctrl, weight_stride=stride)
        assert cls(state, obs, verbose=False, control=ctrl, weight_stride=1).control is ctrl   # the plain filter
    for cls, kw in ((EnSRF, dict(loc="GC")), (ETKF, {})):
        with pytest.raises((TypeError, ValueError)):
            cls(state, obs, verbose=False, control=ctrl, **kw)


# ---- 4. the symbol: declared, bound, exported ---------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_and_exported():
    from efa_xray_amd import _lib
    header = open(os.path.join(ROOT, "include", "efa_hip.h")).read()
    m = re.search(r"int\s+efa_ctx_set_letkf_control\s*\(([^;]*)\)\s*;", header)
    assert m, "include/efa_hip.h does not declare efa_ctx_set_letkf_control"
    assert len(m.group(1).split(",")) == 7
    restype, argtypes = _lib.SIGNATURES["efa_ctx_set_letkf_control"]
    assert len(argtypes) == 7
    lib = _lib.load_library()
    assert lib.efa_ctx_set_letkf_control.argtypes == argtypes
    assert hasattr(_lib.Context, "set_letkf_control")


# ---- 5. no instantiation of k_letkf uses scratch -------------------------------------------------------------------------------------
def test_no_k_letkf_instantiation_uses_scratch():
    import _codeobj
    from efa_xray_amd import _lib
    table = _codeobj.kernel_table(_lib.LIB_PATH)
    ks = {n: k for n, k in table.items() if "k_letkfI" in n}
    # template <MODE, E, NTMAX, SLAB, CTRL>: members (f64, f32) x 3 sizes x slab x control, perturbations x 3 x control, weights x 3 x slab
    ctl = [n for n in ks if re.search(r"k_letkfILi\dE[df]Li\d+ELb[01]ELb1EEE", n)]
    print("%d instantiations of k_letkf, %d with the control" % (len(ks), len(ctl)))
    assert len(ks) == 24 + 6 + 6 and len(ctl) == 12 + 3
    for n, k in sorted(ks.items()):
        print(n, "vgpr", k[".vgpr_count"], "agpr", k.get(".agpr_count", 0), "scratch", k[".private_segment_fixed_size"])
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, n
