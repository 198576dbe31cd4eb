"""Ensemble products and probability verification, the part that needs no GPU: the NumPy model the GPU tests compare
with against numpy.quantile and the direct Brier score, the exports and prototypes, the Python argument checks, and the register
budget of the k_products instantiations."""
import os
import re

import numpy as np
import pytest

import _products as pm
from conftest import ROOT

U = pm.U


def _rows(seed, rows, M, ties):
    rng = np.random.default_rng(seed)
    X = 280.0 + 3.0 * rng.standard_normal((rows, M))
    if ties:
        X = np.round(X)                      # integer-valued members: many ties
    return X


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("M", [2, 3, 8, 9, 33, 100, 255, 256])
def test_model_quantiles_agree_with_numpy(M, ties):
    X = _rows(M, 60, M, ties)
    qs = (0.0, 0.1, 0.25, 0.5, 0.9, 0.999, 1.0)
    m = pm.model(X, 1, quantiles=qs)
    xs = np.sort(X, axis=1)
    for i, q in enumerate(qs):
        ref = np.quantile(X, q, axis=1)
        bound = 6 * U * np.maximum(np.abs(m["qlo"][i]), np.abs(m["qhi"][i]))
        assert np.all(np.abs(m["quant"][i] - ref) <= bound), (M, q)
        assert np.all((m["qlo"][i] <= m["quant"][i]) & (m["quant"][i] <= m["qhi"][i]))
    assert np.array_equal(m["quant"][0], xs[:, 0]) and np.array_equal(m["quant"][-1], xs[:, -1])
    if M % 2:
        assert np.array_equal(m["quant"][3], xs[:, M // 2])      # the median of an odd M is a member
    else:
        assert pm.levels(0.5, M)[2] == 0.5


def test_model_levels_and_rules():
    assert pm.levels(0.0, 7) == (0, 1, 0.0) and pm.levels(1.0, 7) == (6, 6, 0.0) and pm.levels(0.5, 7) == (3, 4, 0.0)
    assert pm.levels(1.0, 2) == (1, 1, 0.0)
    X = np.array([[1.0, 2.0, 3.0], [0.1, 0.1, 0.1], [0.0, -0.0, 1.0], [1.0, np.nan, 2.0], [1e308, -1e308, 0.0], [np.inf, 1.0, 2.0]])
    thr = np.array([[2.0, 0.0, np.nan]])
    m = pm.model(X, 1, quantiles=(0.0, 0.5, 1.0, 0.25), thr=thr)
    assert np.array_equal(m["bad"], [False, False, False, True, False, True])
    assert m["mean"][1] == 0.1 and m["sd"][1] == 0.0 and np.all(m["quant"][:, 1] == 0.1)
    assert np.array_equal(m["prob"][0, :3], [1 / 3, 0.0, 0.0])       # a member equal to t does not count
    assert np.array_equal(m["prob"][1, :3], [1.0, 1.0, 1 / 3])       # -0.0 > 0.0 is false
    assert np.all(np.isnan(m["prob"][2])) and np.all(np.isnan(m["prob"][:, 3])) and np.all(np.isnan(m["quant"][:, 5]))
    assert list(m["quant"][:3, 4]) == [-1e308, 0.0, 1e308]            # f == 0: no 0 * inf
    assert m["quant"][3, 4] == -5e307
    two = pm.model(np.array([[1e308, -1e308]]), 1, quantiles=(0.5,))   # x_hi - x_lo overflows: the min keeps the value at x_hi
    assert two["quant"][0, 0] == 1e308


@pytest.mark.parametrize("M", [2, 9, 40])
def test_model_brier_is_the_direct_mean_and_decomposes(M):
    X, y, thr = pm.make_case(M, 3, 50, M)
    m = pm.model(X, 3, thr=thr, y=y, slab_group=[0, 0, 0])
    assert m["n"].shape == (1, 2) and np.all(m["n"] == 150) and np.all(m["n_bad"] == 0)
    trow = np.repeat(thr, 50, axis=0).T
    for j in range(2):
        p = m["prob"][j]
        o = (y > trow[j]).astype(np.float64)
        direct = np.mean((p - o) ** 2)
        s = pm.scores(m["table"][0, j], m["sums"][0, j])
        assert abs(s["brier"] - direct) <= 1e-14
        assert abs(s["brier"] - (s["reliability"] - s["resolution"] + s["uncertainty"])) <= 1e-12
        assert abs(s["base_rate"] - o.mean()) <= 1e-14 and abs(s["forecast_rate"] - p.mean()) <= 1e-14
        assert np.array_equal(m["table"][0, j].sum(axis=1), np.bincount(m["k"][j], minlength=M + 1))


def test_library_scores_agree_with_the_model():
    from efa_xray_amd.postprocess.products import scores_from_table
    X, y, thr = pm.make_case(5, 2, 40, 11)
    m = pm.model(X, 2, thr=thr, y=y, slab_group=[0, 1])
    for g in range(2):
        for j in range(2):
            a, b = scores_from_table(m["table"][g, j], m["sums"][g, j]), pm.scores(m["table"][g, j], m["sums"][g, j])
            for key, v in b.items():
                assert np.isclose(a[key], v, rtol=1e-13, atol=1e-15, equal_nan=True), key
            assert np.array_equal(a["n_forecasts"], m["table"][g, j].sum(axis=1))
    empty = scores_from_table(np.zeros((12, 2), dtype=np.int64), np.zeros(4))
    assert np.isnan(empty["brier"]) and np.isnan(empty["reliability"]) and np.all(np.isnan(empty["observed_frequency"]))
    one_sided = scores_from_table(np.array([[3, 0], [2, 0]]), np.array([5.0, 0.4, 2.0, 0.0]))
    assert np.isnan(one_sided["brier_skill"]) and one_sided["base_rate"] == 0.0


def test_exports_and_prototypes():
    import efa_xray_amd
    from efa_xray_amd import _lib, postprocess
    for name in ("ensemble_products", "probability_verification"):
        assert name in efa_xray_amd.__all__ and callable(getattr(efa_xray_amd, name))
        assert name in postprocess.__all__ and getattr(postprocess, name) is getattr(efa_xray_amd, name)
    a, b = _lib.SIGNATURES["efa_products_dev"], _lib.SIGNATURES["efa_products_f32_dev"]
    assert len(a[1]) == len(b[1]) == 20
    allowed = (_lib.ctypes.c_int, _lib.ctypes.c_long, _lib.ctypes.c_double, _lib.ctypes.c_uint64)
    for t in a[1] + b[1]:
        assert t in allowed or t is _lib.ctypes.c_void_p or issubclass(t, _lib.ctypes._Pointer), t
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efa_hip.h")).read(), flags=re.S)
    for name in ("efa_products_dev", "efa_products_f32_dev"):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert proto is not None and len(proto.group(1).split(",")) == 20, name
    src = open(os.path.join(ROOT, "efa_xray_amd", "_lib.py")).read()
    assert src.index('"efa_products_f32_dev"') < src.index("def load_library")
    assert hasattr(_lib.Context, "products")
    assert "efa_products.hip" in open(os.path.join(ROOT, "efa_xray_amd", "csrc", "Makefile")).read()
    lib = _lib.load_library()
    assert lib.efa_abi_version() == 1
    for name in ("efa_products_dev", "efa_products_f32_dev"):
        assert getattr(lib, name)(*([None] + [0] * 2 + [None] + [0] * 3 + [None, 0] + [None] * 11)) == _lib.EFA_ERR_INVALID
        assert b"null context" in lib.efa_last_error()


def test_products_kernels_hold_the_row_in_registers():
    """Every k_products instantiation up to NU = 16 (128 members) runs without scratch; the six sizes exist for both element types,
    with and without the sort."""
    from efa_xray_amd import _lib
    from _codeobj import kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    seen = 0
    for nu in (1, 2, 4, 8, 16, 32):
        for e in "df":
            for s in (0, 1):
                hits = [k for n, k in tab.items() if "10k_productsILi%dE%sLb%dE" % (nu, e, s) in n]
                assert len(hits) == 1, (nu, e, s)
                k = hits[0]
                seen += 1
                if nu <= 16:
                    assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, (k[".name"], k)
                    assert k[".vgpr_count"] <= 256, (k[".name"], k[".vgpr_count"])
    assert seen == 24


# .vgpr_count of k_products<NU, E, SORT> before the row layout's helpers moved to efa_quadrow.h / efa_quadreduce.h, (float64, float32)
# per (NU, SORT); NU = 32 spilled then (8 to 10 registers, no scratch)
VGPRS_BEFORE = {(1, 0): (105, 105), (1, 1): (111, 111), (2, 0): (111, 111), (2, 1): (115, 113), (4, 0): (133, 133), (4, 1): (135, 135),
                (8, 0): (164, 164), (8, 1): (176, 175), (16, 0): (250, 250), (16, 1): (256, 256), (32, 0): (394, 394), (32, 1): (451, 451)}


def test_products_kernels_keep_their_occupancy_step():
    """No k_products instantiation needs more registers than its occupancy step before the shared headers allowed, and none that
    was free of scratch and spills has either now.  k_group_reduce (efa_quadreduce.h) is the only reduce kernel of its shape left,
    free of scratch and spills as the three it replaces were."""
    from efa_xray_amd import _lib
    from _codeobj import assert_no_worse_than, kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    for (nu, s), before in VGPRS_BEFORE.items():
        for e, v in zip("df", before):
            (k,) = [k for n, k in tab.items() if "10k_productsILi%dE%sLb%dE" % (nu, e, s) in n]
            assert_no_worse_than(k, v, before_clean=nu <= 16)
            assert k[".private_segment_fixed_size"] == 0, (k[".name"], k)
    red = [k for n, k in tab.items() if "k_group_reduce" in n]
    assert red and not [n for n in tab if "k_products_reduce" in n or "k_verify_reduce" in n or "k_nbr_reduce" in n]
    for k in red:
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, (k[".name"], k)


def _state(M=4, dtype=None, nvar=2, nt=2, ny=3, nx=5):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    return EnsembleState.from_array(rng.standard_normal((nvar, nt, ny, nx, M)), lat, lon, varnames=["t2m", "psfc"][:nvar],
                                    dtype=dtype)


def test_argument_checks_raise_before_the_gpu_is_touched(monkeypatch):
    from efa_xray_amd import _lib, ensemble_products, probability_verification

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(_lib, "get_context", no_gpu)
    st = _state()
    bad_products = [
        (dict(quantiles=(0.5, 1.5)), "lie in [0, 1]"),
        (dict(quantiles=(-0.1,)), "lie in [0, 1]"),
        (dict(quantiles=(np.nan,)), "lie in [0, 1]"),
        (dict(quantiles="ab"), "quantiles must be"),
        (dict(quantiles=((0.1, 0.2), (0.3, 0.4))), "quantiles must be"),
        (dict(quantiles=tuple(np.linspace(0, 1, 9))), "at most 8"),
        (dict(thresholds=[1.0, 2.0]), "mapping"),
        (dict(thresholds={"rh": [1.0]}), "no variable"),
        (dict(thresholds={"t2m": "x"}), "not a sequence of numbers"),
        (dict(thresholds={"t2m": [[1.0], [2.0]]}), "not a sequence of numbers"),
        (dict(thresholds={"t2m": list(range(9))}), "at most 8"),
        (dict(thresholds={"t2m": [0.0, np.inf]}), "not finite"),
        (dict(thresholds={"t2m": [np.nan]}), "not finite"),
    ]
    for kw, word in bad_products:
        with pytest.raises(ValueError, match=re.escape(word)):
            ensemble_products(st, **kw)
    good_v, good_t = {"t2m": np.zeros((2, 3, 5))}, {"t2m": [0.0]}
    bad_verif = [
        (dict(verification=[1, 2]), "mapping"),
        (dict(verification={"rh": np.zeros((2, 3, 5))}), "no variable"),
        (dict(verification={"t2m": np.zeros((2, 3, 4))}), "shape"),
        (dict(verification={"t2m": np.full((2, 3, 5), np.inf)}), "infinite"),
        (dict(thresholds=None), "mapping"),
        (dict(thresholds={"rh": [1.0]}), "no variable"),
        (dict(thresholds={"t2m": list(range(9))}), "at most 8"),
        (dict(thresholds={"t2m": [np.inf]}), "not finite"),
        (dict(by="time"), "by="),
        (dict(weights=np.ones((3, 4))), "weights has shape"),
        (dict(weights=-np.ones((3, 5))), "finite and >= 0"),
    ]
    for kw, word in bad_verif:
        args = dict(verification=good_v, thresholds=good_t)
        args.update(kw)
        with pytest.raises(ValueError, match=re.escape(word)):
            probability_verification(st, **args)
    for fn, args in ((ensemble_products, ()), (probability_verification, (good_v, good_t))):
        with pytest.raises(ValueError, match="members"):
            fn(_state(M=1), *args)
        with pytest.raises(ValueError, match="no variables"):
            fn(type(st)({}, st.coords), *[{} for _ in args])
        mixed = type(st)(st.variables, st.coords)
        mixed.variables["psfc"] = mixed.variables["psfc"].astype(np.float32)
        with pytest.raises(ValueError, match="mix dtypes"):
            fn(mixed, *args)
    with pytest.raises(ValueError, match="members"):
        ensemble_products(_state(M=257, nvar=1, nt=1, ny=1, nx=2))
    # no threshold at all: nothing to score, NaN scores, and still no library call
    out = probability_verification(st, good_v, {})
    assert out["brier"].shape == (2, 0) and out["table"].shape == (2, 0, 5, 2) and out["groups"] == ["t2m", "psfc"]
