"""The batch observation-space solver (ETKF) without a GPU: the NumPy model of tests/_etkf.py against itself (two
formulations), against a consistent serial EnSRF and against the closed form of one observation; the constructor's refusals;
the new symbol and option in the header, the ctypes table and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import _etkf as ek
from conftest import ROOT
from oracle import ensrf_oracle as orc

SIZES = [(2, 1), (3, 5), (16, 64), (17, 33), (50, 1000), (100, 257), (20, 20000)]


def _case(M, P, N=40):
    c = ek.make_case(M, P, N=N)
    ym, Yp = ek.ob_priors(c["HX"])
    return c, ym, Yp


@pytest.mark.parametrize("M,P", SIZES)
def test_two_formulations_agree(M, P):
    c, ym, Yp = _case(M, P)
    a = ek.etkf_solution(ym, Yp, c["value"], c["error"], c["assim"])
    b = ek.etkf_solution_svd(ym, Yp, c["value"], c["error"], c["assim"])
    assert a["cond"] <= 1e4, "the builder must keep cond(A) <= 1e4, got %g" % a["cond"]
    assert np.max(np.abs(a["T"] - b["T"])) <= 1e-11 * max(1.0, np.max(np.abs(b["T"])))
    assert np.max(np.abs(a["w"] - b["w"])) <= 1e-11 * max(1.0, np.max(np.abs(b["w"])))


@pytest.mark.parametrize("M,P", [(3, 5), (17, 33), (50, 200), (20, 2000)])
def test_model_equals_a_consistent_serial_ensrf(M, P):
    """/(M-1) in both places makes the serial loop an exact Kalman update, which the batch solve reproduces; the reference's
    loop (np.var in the denominator) is a different filter."""
    c, ym, Yp = _case(M, P)
    X = c["X"]
    xbm, Xbp = orc.format_prior_state(X, c["HX"])
    N = X.shape[0]
    sol = ek.etkf_solution(ym, Yp, c["value"], c["error"], c["assim"])
    xam, Xap = ek.etkf_apply(xbm, Xbp, sol["T"], sol["w"])
    sxam, sXap = ek.serial_consistent(xbm, Xbp, N, c["value"], c["error"], c["assim"])
    inc = np.max(np.abs(sxam - xbm))
    assert np.max(np.abs(xam - sxam)) <= 1e-10 * inc
    cov, scov = Xap @ Xap.T, sXap @ sXap.T
    assert np.max(np.abs(cov - scov)) <= 1e-10 * np.max(np.abs(Xbp @ Xbp.T))
    # ... and not the reference's loop: the difference is of the order of the increment itself
    ref_xam, _, _ = orc.ensrf_update(xbm, Xbp, N, c["value"], c["error"], c["assim"])[:3]
    assert np.max(np.abs(ref_xam - xam)) > 1e-4 * inc


@pytest.mark.parametrize("M,P", SIZES)
def test_transform_is_symmetric_and_keeps_the_mean(M, P):
    c, ym, Yp = _case(M, P)
    sol = ek.etkf_solution(ym, Yp, c["value"], c["error"], c["assim"])
    T = sol["T"]
    scale = max(1.0, np.max(np.abs(T)))
    assert np.max(np.abs(T - T.T)) <= 1e-10 * scale
    assert np.max(np.abs(T @ np.ones(M) - 1.0)) <= 1e-10      # as far as the rows of Yp sum to zero: these do
    Xp = c["X"] - c["X"].mean(axis=1, keepdims=True)
    assert np.max(np.abs((Xp @ T).sum(axis=1))) <= 1e-10 * np.max(np.abs(Xp)) * M
    assert np.all(sol["mu"] >= (M - 1.0) * (1.0 - 1e-12))
    assert 0.0 <= sol["dfs"] <= min(M - 1, sol["n_active"]) + 1e-9


def test_closed_form_of_one_observation():
    """P = 1: C = y y^T / r, the one non-trivial eigenpair is (|y|^2 / r, y / |y|); the mean update is the Kalman gain with
    the (M-1) covariance and the perturbations shrink along y by sqrt(r / (s2 + r)), s2 = |y|^2 / (M-1)."""
    rng = np.random.default_rng(5)
    M = 9
    hx = rng.standard_normal(M) * 1.7 + 0.3
    ym, Yp = ek.ob_priors(hx[None, :])
    r, value = 0.8, 1.9
    sol = ek.etkf_solution(ym, Yp, [value], [r], [True])
    y = Yp[0]
    s2 = y @ y / (M - 1.0)
    u = y / np.sqrt(y @ y)
    T = np.eye(M) + (np.sqrt(r / (s2 + r)) - 1.0) * np.outer(u, u)
    w = y * (value - ym[0]) / ((M - 1.0) * (s2 + r))
    assert np.allclose(sol["T"], T, rtol=0, atol=1e-13)
    assert np.allclose(sol["w"], w, rtol=0, atol=1e-13)
    assert sol["n_active"] == 1 and np.isclose(sol["dfs"], s2 / (s2 + r), rtol=1e-12)
    assert np.isclose(sol["chi2"], (value - ym[0]) ** 2 / (s2 + r), rtol=1e-12)
    yam, Yap = ek.etkf_apply(ym, Yp, sol["T"], sol["w"])
    assert np.isclose(yam[0], ym[0] + s2 / (s2 + r) * (value - ym[0]), rtol=1e-12)
    assert np.isclose(Yap[0] @ Yap[0] / (M - 1.0), s2 * r / (s2 + r), rtol=1e-12)


def test_unflagged_observations_are_not_read():
    c, ym, Yp = _case(17, 33)
    a = ek.etkf_solution(ym, Yp, c["value"], c["error"], c["assim"])
    value, error = c["value"].copy(), c["error"].copy()
    value[~c["assim"]] = np.nan
    error[~c["assim"]] = np.inf
    b = ek.etkf_solution(ym, Yp, value, error, c["assim"])
    assert np.array_equal(a["T"], b["T"]) and np.array_equal(a["w"], b["w"])


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def _state_and_obs(M=6):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(30, 40, 4), np.linspace(250, 260, 5), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((1, 1, 4, 5, M)), lat, lon)
    obs = [Observation(value=0.1, error=1.0, lat=35.0, lon=255.0, localize_radius=500.0)]
    return state, obs


@pytest.mark.parametrize("kw", [dict(loc="GC"), dict(loc=True), dict(adaptive_inflation=object()), dict(vert_coord=np.zeros((1, 1))),
                                dict(time_localize=True), dict(var_impact={"a": {"a": 1.0}}), dict(sampling_error_correction=True),
                                dict(path="transform"), dict(obs_batch=8)])
def test_constructor_refusals(kw):
    from efa_xray_amd import ETKF
    state, obs = _state_and_obs()
    with pytest.raises(ValueError) as e:
        ETKF(state, obs, verbose=False, **kw)
    if "loc" in kw:
        assert "out of scope" in str(e.value)


def test_constructor_accepts_what_the_issue_lists():
    from efa_xray_amd import ETKF, EnSRF
    state, obs = _state_and_obs()
    f = ETKF(state, obs, verbose=False, device=0, rtps=0.9, outlier_threshold=3.0, streamed=True, stream_chunk_cols=16,
             stream_pinned_limit_mb=64, inflation=1.1, loc=None)
    assert isinstance(f, EnSRF) and f.last_solve is None and f.loc is False
    ETKF(state.astype(np.float32), obs, verbose=False, rtpp=0.5)
    with pytest.raises(ValueError):
        ETKF(state, obs, verbose=False, rtps=0.5, rtpp=0.5)
    with pytest.raises(TypeError):
        ETKF(state, obs, verbose=False, no_such_option=1)
    with pytest.raises(ValueError):
        f.update_arrays(np.zeros(1), np.zeros((1, 6)))


class _Recorder(object):
    def __init__(self):
        self.options = []

    def set_option(self, key, value):
        self.options.append((key, value))

    def __getattr__(self, name):          # every other setter: accepted and ignored
        return lambda *a, **k: None


def test_both_filters_set_the_solver_on_every_call():
    from efa_xray_amd import ETKF, EnSRF
    state, obs = _state_and_obs()
    for cls, want in ((EnSRF, 0), (ETKF, 1)):
        rec = _Recorder()
        cls(state, obs, verbose=False)._configure(rec)
        assert [v for k, v in rec.options if k == "obs_solver"][-1] == want


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_declared_bound_and_exported():
    import efa_xray_amd
    from efa_xray_amd import _lib
    assert "ETKF" in efa_xray_amd.__all__ and efa_xray_amd.ETKF.__module__ == "efa_xray_amd.assimilation.etkf"
    text = open(os.path.join(ROOT, "include", "efa_hip.h")).read()
    assert re.search(r"int\s+efa_etkf_solution\s*\(\s*efa_ctx\s*\*", text)
    assert '"obs_solver"' in text and "#define EFA_ABI_VERSION 1" in text
    res, args = _lib.SIGNATURES["efa_etkf_solution"]
    assert res is ctypes.c_int and len(args) == 7 and args[1] is ctypes.c_int
    assert args[2:6] == [_lib.c_double_p] * 4
    lib = _lib.load_library()
    assert hasattr(lib, "efa_etkf_solution")
    assert hasattr(_lib.Context, "etkf_solution")


def test_option_and_entry_refuse_a_null_context():
    from efa_xray_amd import _lib
    lib = _lib.load_library()
    assert lib.efa_ctx_set_option(None, b"obs_solver", 1) == _lib.EFA_ERR_INVALID
    assert b"null context" in lib.efa_last_error()
    v = ctypes.c_long(7)
    assert lib.efa_ctx_get_option(None, b"obs_solver", ctypes.byref(v)) == _lib.EFA_ERR_INVALID and v.value == 7
    sweeps = ctypes.c_long(-1)
    assert lib.efa_etkf_solution(None, 4, None, None, None, None, ctypes.byref(sweeps)) == _lib.EFA_ERR_INVALID
    assert b"null context" in lib.efa_last_error() and sweeps.value == -1
