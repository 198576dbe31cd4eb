"""Ensemble sensitivity and observation targeting, the part that needs no GPU: the NumPy model the GPU tests compare
with against the explicit covariance update, the exports and prototypes, and the Python argument checks."""
import os
import re

import numpy as np
import pytest

import _sensitivity as sm
from conftest import ROOT

PARITY = 1e-10   # the project's float64 parity figure


@pytest.mark.parametrize("rows,M,K,n", [(300, 8, 2, 4), (2000, 20, 3, 5), (500, 7, 16, 8)])
def test_model_equals_the_explicit_covariance_update(rows, M, K, n):
    """The stateless recursion (dots of the raw rows with u_0 .. u_{t-1}) against P <- P - P[:, i] P[i, :] / (P_ii + R) on the
    covariance of the stacked [X; J], picks as the model makes them.  500 x 7 with 8 picks: the conditioned ensemble loses rank."""
    n_lead = 4
    X, J, R, w = sm.make_case(100 + rows, rows, M, K, n_lead)
    m = sm.model(X, J, n_lead, R, w, None, n)
    assert np.all(m["picked_row"] >= 0) and m["margins"].size == n
    var, cov, traj = sm.explicit(X, J, n_lead, R, m["picked_row"])
    var0, varJ0 = m["var0"], m["varJ0"]
    e_var = np.max(np.abs(m["var"] - var) / var0)
    e_cov = np.max(np.abs(m["cov"] - cov) / np.sqrt(var0[None, :] * varJ0[:, None]))
    e_vj = np.max(np.abs(m["metric_var"] - traj) / varJ0[None, :])
    print("%d x %d x %d x %d: var %.2e cov %.2e varJ %.2e, pick margins %.1e .. %.1e"
          % (rows, M, K, n, e_var, e_cov, e_vj, m["margins"].min(), m["margins"].max()))
    assert e_var <= PARITY and e_cov <= PARITY and e_vj <= PARITY
    # every pick reduces the weighted metric variance by its score
    total = m["metric_var"] @ w
    assert np.allclose(total[:-1] - total[1:], m["picked_score"], rtol=1e-9, atol=0.0)


def test_model_rules():
    X, J, R, w = sm.make_case(5, 40, 6, 2, 2)
    X[3] = 0.1                     # a constant row whose mean does not round back to the member
    X[7, 2] = np.nan
    X[9] = X[8]                    # a tie
    cand = np.ones(40, dtype=bool)
    cand[20:] = False
    m = sm.model(X, J, 2, R, w, cand, 3)
    for f in ("var", "score"):
        assert m[f][3] == 0.0 and np.isnan(m[f][7])
    for f in ("cov", "sens", "corr", "dvar"):
        assert np.all(m[f][:, 3] == 0.0) and np.all(np.isnan(m[f][:, 7]))
    assert np.all(m["score"][20:] == 0.0)
    assert not np.isin(m["picked_row"], [3, 7, 9]).any() and np.all(m["picked_row"] < 20)
    none = sm.model(X, J, 2, R, w, np.zeros(40, dtype=bool), 3)
    assert np.all(none["picked_row"] == -1) and np.all(none["picked_score"] == 0.0)
    assert np.array_equal(none["metric_var"], np.tile(none["varJ0"], (4, 1)))


def test_exports_and_prototypes():
    import efa_xray_amd
    from efa_xray_amd import _lib, postprocess
    for name in ("ensemble_sensitivity", "observation_targets"):
        assert name in efa_xray_amd.__all__ and callable(getattr(efa_xray_amd, name))
        assert name in postprocess.__all__ and getattr(postprocess, name) is getattr(efa_xray_amd, name)
    a, b = _lib.SIGNATURES["efa_sensitivity_dev"], _lib.SIGNATURES["efa_sensitivity_f32_dev"]
    assert len(a[1]) == len(b[1]) == 21
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efa_hip.h")).read(), flags=re.S)
    for name in ("efa_sensitivity_dev", "efa_sensitivity_f32_dev"):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert proto is not None and len(proto.group(1).split(",")) == 21, name
    # the prototypes sit above load_library: the sanitiser walk of the C ABI reads the table from there
    src = open(os.path.join(ROOT, "efa_xray_amd", "_lib.py")).read()
    assert src.index('"efa_sensitivity_f32_dev"') < src.index("def load_library")


# .vgpr_count of k_sens_pass<NU, AL, E> before it took the pair type and the row reductions from efa_quadrow.h, per NU:
# (unaligned float64, unaligned float32, aligned float64, aligned float32); every instantiation was free of scratch and spills
VGPRS_BEFORE = {
    1: (84, 84, 80, 80), 2: (100, 100, 96, 96), 3: (112, 112, 96, 100), 4: (112, 108, 100, 100), 5: (120, 124, 104, 104),
    6: (128, 128, 108, 108), 7: (136, 136, 112, 112), 8: (144, 148, 116, 116), 9: (164, 160, 132, 128), 10: (176, 176, 140, 136),
    11: (184, 172, 140, 140), 12: (196, 188, 156, 148), 13: (212, 200, 164, 160), 14: (220, 220, 168, 160), 15: (236, 228, 168, 172),
    16: (240, 236, 180, 176), 17: (256, 236, 188, 188), 18: (272, 260, 196, 192), 19: (287, 277, 204, 200), 20: (285, 287, 208, 208),
    21: (305, 295, 220, 212), 22: (312, 304, 228, 220), 23: (300, 296, 232, 228), 24: (310, 308, 240, 244), 25: (326, 317, 244, 244),
    26: (338, 328, 256, 252), 27: (352, 339, 260, 260), 28: (378, 350, 268, 268), 29: (400, 364, 280, 276), 30: (392, 382, 288, 285),
    31: (422, 398, 294, 283), 32: (414, 412, 292, 296)}


def test_sens_pass_keeps_its_occupancy_step():
    """All 128 instantiations of k_sens_pass stay free of scratch and spills, none on a lower occupancy step than before."""
    from efa_xray_amd import _lib
    from _codeobj import assert_no_worse_than, kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    for nu, before in VGPRS_BEFORE.items():
        for (al, e), v in zip(((0, "d"), (0, "f"), (1, "d"), (1, "f")), before):
            (k,) = [k for n, k in tab.items() if "11k_sens_passILi%dELb%dE%sE" % (nu, al, e) in n]
            assert_no_worse_than(k, v)


def _state(dtype=None, M=6):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(3)
    lat, lon = np.meshgrid(np.linspace(30, 50, 4), np.linspace(230, 260, 5), indexing="ij")
    return EnsembleState.from_array(rng.standard_normal((2, 2, 4, 5, M)), lat, lon, varnames=["t", "q"], dtype=dtype)


def test_python_argument_checks_raise_before_the_device_is_touched(monkeypatch):
    from efa_xray_amd import _lib, ensemble_sensitivity, observation_targets

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "get_context", no_device)
    st = _state()
    J = np.random.default_rng(0).standard_normal((2, 6))
    err = dict(t=1.0, q=0.5)
    bad_sens = [dict(metrics=J[:, :5]), dict(metrics=np.zeros((0, 6))), dict(metrics=np.full((1, 6), np.nan)),
                dict(metrics=dict(a=J[0], b=J[1, :3])), dict(metrics=np.zeros((33, 6))), dict(metrics="nonsense")]
    for kw in bad_sens:
        with pytest.raises(ValueError):
            ensemble_sensitivity(st, **kw)
    ok = dict(metrics=J, n_targets=3, ob_error=err)
    bad = [dict(n_targets=-1), dict(n_targets=31), dict(n_targets=1.5), dict(n_targets="x"), dict(ob_error=dict(t=1.0)),
           dict(ob_error=dict(t=1.0, q=0.0)), dict(ob_error=dict(t=1.0, q=np.inf)), dict(ob_error=dict(t=1.0, q=0.5, z=1.0)),
           dict(ob_error=1.0), dict(weights=[1.0]), dict(weights=[1.0, -1.0]), dict(weights=[1.0, np.nan]),
           dict(weights=dict(a=1.0)), dict(candidates=np.ones((2, 4, 5), dtype=bool)), dict(candidates=dict(z=True)),
           dict(candidates=dict(t=np.ones((3, 4, 5), dtype=bool))), dict(metrics=J[:, :4])]
    for kw in bad:
        a = dict(ok)
        a.update(kw)
        with pytest.raises(ValueError):
            observation_targets(st, **a)
    with pytest.raises(ValueError):
        observation_targets(_state(M=1), np.zeros((1, 1)), 1, err)
    mixed = _state()
    mixed.variables["q"] = mixed.variables["q"].astype(np.float32)
    with pytest.raises(ValueError):
        observation_targets(mixed, J, 1, err)
    # named metrics with named weights pass the checks and reach the device
    with pytest.raises(AssertionError, match="device was touched"):
        observation_targets(st, dict(a=J[0], b=J[1]), 2, err, candidates=dict(t=np.ones((1, 4, 5), dtype=bool)), weights=dict(b=2.0))
    with pytest.raises(AssertionError, match="device was touched"):
        ensemble_sensitivity(_state(np.float32), J)
