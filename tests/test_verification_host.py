"""Ensemble verification, the part that needs no GPU: the NumPy model the GPU tests compare with against closed
forms, the tie-break hash, the exports and prototypes, and the Python argument checks."""
import math
import os
import re

import numpy as np
import pytest

import _verification as vm
from conftest import ROOT


def test_model_two_members_closed_form():
    rng = np.random.default_rng(1)
    for fair in (False, True):
        X = rng.standard_normal((50, 2)) + 3.0
        y = rng.standard_normal(50) + 3.0
        m = vm.model(X, y, 1, [0], fair=fair)
        d1, d2 = X[:, 0] - y, X[:, 1] - y
        D = 2.0 if fair else 4.0
        ref = (np.abs(d1) + np.abs(d2)) / 2 - np.abs(d1 - d2) / D
        assert np.allclose(m["crps"], ref, rtol=1e-14, atol=1e-16)


@pytest.mark.parametrize("M", [2, 5, 8, 33])
def test_model_half_integers_give_a_flat_histogram(M):
    ys = np.arange(-0.5, M, 1.0)                  # M + 1 half-integers
    X = np.tile(np.arange(M, dtype=np.float64), (ys.size, 1))
    m = vm.model(X, ys, 1, [0])
    assert np.array_equal(m["below"], np.ceil(ys).astype(np.int32)) and np.all(m["equal"] == 0)
    assert np.array_equal(m["rank"], m["below"]) and np.all(m["hist"][0] == 1) and m["n"][0] == M + 1


@pytest.mark.parametrize("M", [3, 9, 40])
def test_model_crps_is_the_pairwise_definition_and_fair_scales_the_second_term(M):
    X, y = vm.make_case(M, 2, 20, M)
    std = vm.model(X, y, 2, [0, 0], fair=False)
    fair = vm.model(X, y, 2, [0, 0], fair=True)
    for i in range(X.shape[0]):
        d = X[i] - y[i]
        for m, f in ((std, False), (fair, True)):
            assert abs(m["crps"][i] - vm.crps_pairwise(d, f)) <= 4 * M * vm.U * m["mean_abs_d"][i]
    second_std = std["mean_abs_d"] - std["crps"]
    second_fair = fair["mean_abs_d"] - fair["crps"]
    assert np.allclose(second_fair, second_std * M / (M - 1), rtol=1e-9, atol=1e-300)


def test_hash_stays_in_range_and_is_uniform():
    rng = np.random.default_rng(7)
    R = rng.integers(0, 2 ** 62, size=2000)
    for equal in (0, 1, 2, 9, 255, 256):
        p = vm.pick_array(12345, R, np.full(R.size, equal))
        assert p.min() >= 0 and p.max() <= equal
    # scalar and array forms agree
    assert [vm.pick(99, int(r), 9) for r in R[:200]] == list(vm.pick_array(99, R[:200], np.full(200, 9)))
    # 1e5 all-tied rows, M = 9: every bin within 5 sigma of uniform
    n, M = 100000, 9
    p = vm.pick_array(2024, np.arange(n), np.full(n, M))
    counts = np.bincount(p, minlength=M + 1)
    q = 1.0 / (M + 1)
    sigma = math.sqrt(n * q * (1 - q))
    assert counts.size == M + 1 and np.all(np.abs(counts - n * q) <= 5 * sigma), counts


def test_model_rules():
    X = np.array([[1.0, 2.0, 3.0], [0.1, 0.1, 0.1], [0.0, -0.0, 1.0], [1.0, np.nan, 2.0], [1e308, -1e308, 0.0], [1.0, 2.0, 3.0]])
    y = np.array([2.0, 0.1, 0.0, 1.0, -1e308, np.nan])
    m = vm.model(X, y, 1, [0], seed=3)
    assert (m["below"][0], m["equal"][0]) == (1, 1) and m["rank"][0] in (1, 2)
    assert m["equal"][1] == 3 and m["crps"][1] == 0.0 and m["var"][1] == 0.0 and m["err"][1] == 0.0
    assert (m["below"][2], m["equal"][2]) == (0, 2)
    for i in (3, 4, 5):
        assert m["rank"][i] == -1 and np.isnan(m["crps"][i])
    assert m["n"][0] == 3 and m["n_bad"][0] == 2 and m["hist"].sum() == 3
    off = vm.model(X, y, 1, [-1])
    assert off["hist"].shape == (0, 4) and np.all(off["rank"] == -1)


def test_exports_and_prototypes():
    import efa_xray_amd
    from efa_xray_amd import _lib, postprocess
    assert "ensemble_verification" in efa_xray_amd.__all__ and callable(efa_xray_amd.ensemble_verification)
    assert "ensemble_verification" in postprocess.__all__
    assert postprocess.ensemble_verification is efa_xray_amd.ensemble_verification
    a, b = _lib.SIGNATURES["efa_verify_dev"], _lib.SIGNATURES["efa_verify_f32_dev"]
    assert len(a[1]) == len(b[1]) == 23
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efa_hip.h")).read(), flags=re.S)
    for name in ("efa_verify_dev", "efa_verify_f32_dev"):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert proto is not None and len(proto.group(1).split(",")) == 23, name
    src = open(os.path.join(ROOT, "efa_xray_amd", "_lib.py")).read()
    assert src.index('"efa_verify_f32_dev"') < src.index("def load_library")
    assert hasattr(_lib.Context, "verify")
    assert "efa_verify.hip" in open(os.path.join(ROOT, "efa_xray_amd", "csrc", "Makefile")).read()


# .vgpr_count of k_verify<NU, E> before the row layout's helpers moved to efa_quadrow.h / efa_quadreduce.h, (float64, float32) per NU;
# NU = 32 spilled then (4 registers, no scratch)
VGPRS_BEFORE = {1: (96, 96), 2: (108, 108), 4: (134, 134), 8: (184, 183), 16: (268, 268), 32: (435, 449)}


def test_verify_kernels_hold_the_row_in_registers():
    """The six sizes of k_verify exist for both element types; none has scratch, up to NU = 16 (128 members) none spills, and none
    falls to a lower occupancy step than it had with its private copy of the row layout."""
    from efa_xray_amd import _lib
    from _codeobj import assert_no_worse_than, kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    for nu, before in VGPRS_BEFORE.items():
        for e, v in zip("df", before):
            (k,) = [k for n, k in tab.items() if "8k_verifyILi%dE%sE" % (nu, e) in n]
            assert_no_worse_than(k, v, before_clean=nu <= 16)
            assert k[".private_segment_fixed_size"] == 0, (k[".name"], k)
    assert len([n for n in tab if "8k_verifyILi" in n]) == 12
    assert [n for n in tab if "k_group_reduce" in n] and not [n for n in tab if "k_verify_reduce" in n]


def _state(M=4, dtype=None, nvar=2, nt=2, ny=3, nx=5):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    return EnsembleState.from_array(rng.standard_normal((nvar, nt, ny, nx, M)), lat, lon, varnames=["t2m", "psfc"][:nvar],
                                    dtype=dtype)


def test_argument_checks_raise_before_the_gpu_is_touched(monkeypatch):
    from efa_xray_amd import _lib, ensemble_verification
    from efa_xray_amd.postprocess import verification as vmod

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(_lib, "get_context", no_gpu)
    st = _state()
    good = {"t2m": np.zeros((2, 3, 5))}
    bad = [
        (dict(verification=[1, 2]), "mapping"),
        (dict(verification={"rh": np.zeros((2, 3, 5))}), "no variable"),
        (dict(verification={"t2m": np.zeros((2, 3, 4))}), "shape"),
        (dict(verification={"t2m": np.full((2, 3, 5), np.inf)}), "infinite"),
        (dict(verification={"t2m": "abc"}), "not an array"),
        (dict(by="time"), "by="),
        (dict(weights=np.ones((3, 4))), "weights has shape"),
        (dict(weights=-np.ones((3, 5))), "finite and >= 0"),
        (dict(weights=np.full((3, 5), np.nan)), "finite and >= 0"),
        (dict(weights="x"), "weights must be"),
        (dict(seed=-1), "seed"),
        (dict(seed=1.5), "seed"),
        (dict(seed="s"), "seed"),
        (dict(fields=("rank", "spread")), "fields names"),
        (dict(fields=("rank", "rank")), "twice"),
        (dict(fields=3), "fields must be"),
    ]
    for kw, word in bad:
        args = dict(verification=good)
        args.update(kw)
        with pytest.raises(ValueError, match=re.escape(word)):
            ensemble_verification(st, **args)
    with pytest.raises(ValueError, match="members"):
        ensemble_verification(_state(M=1), good)
    with pytest.raises(ValueError, match="members"):
        ensemble_verification(_state(M=257, nvar=1, nt=1, ny=1, nx=2), {"t2m": np.zeros((1, 1, 2))})
    with pytest.raises(ValueError, match="no variables"):
        ensemble_verification(type(st)({}, st.coords), {})
    mixed = type(st)(st.variables, st.coords)
    mixed.variables["psfc"] = mixed.variables["psfc"].astype(np.float32)
    with pytest.raises(ValueError, match="mix dtypes"):
        ensemble_verification(mixed, good)
    assert vmod.FIELDS == ("below", "equal", "rank", "crps", "err", "var")
