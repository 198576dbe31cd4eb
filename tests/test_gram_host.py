"""The ensemble Gram matrix, EOFs and member clusters, the part that needs no GPU: the exports and prototypes, the
register budget of the k_gram instantiations, the pure host functions on NumPy-made Gram matrices, the norm / weights resolution
and the Python argument checks."""
import os
import re
import warnings

import numpy as np
import pytest

import _gram as gm
from conftest import ROOT


def test_exports_and_prototypes():
    import efa_xray_amd
    from efa_xray_amd import _lib, postprocess
    for name in ("ensemble_gram", "ensemble_eofs", "ensemble_clusters", "distances_from_gram", "eofs_from_gram",
                 "clusters_from_gram"):
        assert name in efa_xray_amd.__all__ and callable(getattr(efa_xray_amd, name))
        assert name in postprocess.__all__ and getattr(postprocess, name) is getattr(efa_xray_amd, name)
    a, b = _lib.SIGNATURES["efa_gram_dev"], _lib.SIGNATURES["efa_gram_f32_dev"]
    assert len(a[1]) == len(b[1]) == 12 and a == b
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "efa_hip.h")).read(), flags=re.S)
    for name, elem in (("efa_gram_dev", "double"), ("efa_gram_f32_dev", "float")):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert proto is not None and len(proto.group(1).split(",")) == 12, name
        assert re.search(r"const\s+%s\s*\*\s*X_dev" % elem, proto.group(1)), name
    src = open(os.path.join(ROOT, "efa_xray_amd", "_lib.py")).read()
    assert src.index('"efa_gram_f32_dev"') < src.index("def load_library")
    assert hasattr(_lib.Context, "gram")
    make = open(os.path.join(ROOT, "efa_xray_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\befa_gram\.hip\b", make, flags=re.M)
    lib = _lib.load_library()
    assert lib.efa_abi_version() == 1
    for name in ("efa_gram_dev", "efa_gram_f32_dev"):
        assert getattr(lib, name)(None, 0, 0, None, 0, 0, None, None, None, None, None, None) == _lib.EFA_ERR_INVALID
        assert b"null context" in lib.efa_last_error()


def test_gram_kernels_use_no_scratch():
    """Every k_gram instantiation -- 16 widths, aligned or not, both element types -- keeps its accumulators (8 (T + 1) registers)
    in registers: no scratch, no spill; the 8-wave kernels (more than 128 members) fit two waves per SIMD."""
    from efa_xray_amd import _lib
    from _codeobj import kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    seen = 0
    for t in range(1, 17):
        for al in (0, 1):
            for e in "df":
                hits = [k for n, k in tab.items() if "6k_gramILi%dELb%dE%sE" % (t, al, e) in n]
                assert len(hits) == 1, (t, al, e)
                k = hits[0]
                seen += 1
                assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, (k[".name"], k)
                assert k.get(".sgpr_spill_count", 0) == 0, (k[".name"], k)
                assert k[".max_flat_workgroup_size"] == (512 if t > 8 else 256), k[".name"]
                assert k[".vgpr_count"] <= (256 if t > 8 else 512), (k[".name"], k[".vgpr_count"])
                assert k[".vgpr_count"] >= 8 * (t + 1), (k[".name"], k[".vgpr_count"])
                assert k[".group_segment_fixed_size"] <= 160 * 1024
                # the accumulation streams are 256 x the workgroups a CU holds (512 registers per SIMD lane in granules of 8, 160 KB of LDS)
                waves = 8 if t > 8 else 4
                held = min((512 // (8 * ((k[".vgpr_count"] + 7) // 8))) * 4 // waves, (160 * 1024) // k[".group_segment_fixed_size"])
                if al:      # (the table is that of the aligned kernels; an unaligned one may hold one workgroup fewer)
                    assert 256 * held >= (256 if t > 8 else 1024 if t in (1, 2, 5) else 768), (k[".name"], held)
    assert seen == 64
    red = [k for n, k in tab.items() if "13k_gram_reduce" in n]
    assert len(red) == 1 and red[0][".private_segment_fixed_size"] == 0


# ---- the pure functions ----------------------------------------------------------------------------------------------------------
def _gram_of_points(P):
    """G with (M-1)(G_aa + G_bb - 2 G_ab) = |p_a - p_b|^2: the members are the points"""
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 1:
        P = P[:, None]
    Pc = P - P.mean(axis=0)
    return Pc @ Pc.T / (P.shape[0] - 1.0)


def test_distances_against_pairwise_differences():
    from efa_xray_amd import distances_from_gram
    rng = np.random.default_rng(0)
    n, M = 200, 17
    X = 280.0 + rng.standard_normal((n, M))
    c = rng.uniform(0.5, 2.0, n)
    m = gm.model(X, 1, [1.0], c)
    d2 = distances_from_gram(m["G"].astype(np.float64))
    direct = np.einsum("i,iab->ab", c, (X[:, :, None] - X[:, None, :]) ** 2)
    assert np.all(np.diag(d2) == 0.0) and np.array_equal(d2, d2.T) and np.all(d2 >= 0.0)
    assert np.allclose(d2, direct, rtol=1e-11, atol=0.0)
    # identical members: the clamp keeps rounding from going negative
    same = np.full((3, 3), 0.1)
    assert np.all(distances_from_gram(same) == 0.0)


def test_eofs_of_a_rank_two_matrix():
    from efa_xray_amd import eofs_from_gram
    M = 6
    v1 = np.array([3.0, -1.0, -1.0, -1.0, 0.0, 0.0])
    v2 = np.array([0.0, 1.0, -1.0, 0.0, 2.0, -2.0])
    v1, v2 = v1 / np.linalg.norm(v1), v2 / np.linalg.norm(v2)
    assert abs(v1 @ v2) < 1e-15 and abs(v1.sum()) < 1e-15 and abs(v2.sum()) < 1e-15
    G = 5.0 * np.outer(v1, v1) + 2.0 * np.outer(v2, v2)
    out = eofs_from_gram(G, 4)
    assert np.allclose(out["variance"], [5.0, 2.0, 0.0, 0.0], atol=1e-14) and np.all(out["variance"] >= 0.0)
    assert np.allclose(out["explained"][:2], [5.0 / 7.0, 2.0 / 7.0], rtol=1e-14)
    assert np.all(out["explained"][2:] == 0.0) and np.all(out["pcs"][2:] == 0.0)            # the null modes
    assert np.allclose(out["pcs"][0], np.sqrt(M - 1.0) * v1, atol=1e-14)
    assert np.allclose(out["pcs"][1], np.sqrt(M - 1.0) * v2, atol=1e-14)
    for k in range(2):      # the sign rule: the component of largest magnitude is positive, the lowest member among equals
        pc = out["pcs"][k]
        assert pc[int(np.argmax(np.abs(pc)))] > 0.0
        assert abs(pc.mean()) < 1e-14 and abs(pc @ pc / (M - 1.0) - 1.0) < 1e-14
    assert out["pcs"][1][4] > 0.0 and out["pcs"][1][5] < 0.0     # |2| = |-2|: member 4 decides
    flipped = eofs_from_gram(5.0 * np.outer(-v1, -v1), 1)
    assert np.allclose(flipped["pcs"][0], out["pcs"][0], atol=1e-14)
    zero = eofs_from_gram(np.zeros((4, 4)), 3)
    assert np.all(zero["variance"] == 0.0) and np.all(np.isnan(zero["explained"])) and np.all(zero["pcs"] == 0.0)


def _partition(labels):
    return sorted(tuple(np.nonzero(labels == c)[0]) for c in np.unique(labels))


def test_ward_on_six_points_worked_by_hand():
    """Points 0, 1, 3, 6, 10, 15 on a line; Ward's d2(A, B) = 2 |A||B|/(|A|+|B|) (c_A - c_B)^2.  Merges: (0, 1) at 1; then
    {0,1}-3 at 4/3 * 2.5^2 = 8.33 (before 3-6 at 9); then 6-10 at 16 (before 10-15 at 25 and {0,1,3}-6 at 32.7); then
    {6,10}-15 at 4/3 * 49 = 65.3 (before {0,1,3}-{6,10} at 106.7)."""
    from efa_xray_amd import clusters_from_gram
    G = _gram_of_points([0.0, 1.0, 3.0, 6.0, 10.0, 15.0])
    want = {6: [0, 1, 2, 3, 4, 5], 5: [0, 0, 1, 2, 3, 4], 4: [0, 0, 0, 1, 2, 3], 3: [0, 0, 0, 1, 1, 2], 2: [0, 0, 0, 1, 1, 1],
            1: [0] * 6}
    for k, labels in want.items():
        out = clusters_from_gram(G, k)
        assert list(out["labels"]) == labels, k
        assert list(out["sizes"]) == list(np.bincount(labels)), k
    two = clusters_from_gram(G, 2)
    assert list(two["medoids"]) == [1, 4] and np.allclose(two["within"], [5.0, 41.0], rtol=1e-13)
    all_ = clusters_from_gram(G, 6)
    assert list(all_["medoids"]) == [0, 1, 2, 3, 4, 5] and np.all(all_["within"] == 0.0)


def test_ward_agrees_with_scipy_where_it_imports():
    from efa_xray_amd import clusters_from_gram
    try:
        from scipy.cluster.hierarchy import fcluster, linkage
    except ImportError:
        return      # (the hand-worked case above stands in)
    rng = np.random.default_rng(4)
    for M, dim in ((12, 3), (40, 5), (97, 2)):
        P = rng.standard_normal((M, dim)) + 4.0 * rng.integers(0, 3, (M, 1))     # general position: no ties
        Z = linkage(P, "ward")
        G = _gram_of_points(P)
        for k in (1, 2, 3, 5, M // 2, M - 1, M):
            mine = clusters_from_gram(G, k)
            theirs = fcluster(Z, k, "maxclust")
            assert _partition(mine["labels"]) == _partition(theirs), (M, k)
            firsts = [int(np.nonzero(mine["labels"] == c)[0][0]) for c in range(k)]
            assert firsts == sorted(firsts)                    # numbered in the order of the lowest members
            d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
            for c in range(k):
                mem = np.nonzero(mine["labels"] == c)[0]
                s = d2[np.ix_(mem, mem)].sum(axis=1)
                assert mine["medoids"][c] == mem[int(np.argmin(s))] and np.isclose(mine["within"][c], s.min(), rtol=1e-9, atol=1e-9)


def test_ward_tie_rule_on_an_equilateral_case():
    from efa_xray_amd import clusters_from_gram, distances_from_gram
    G = np.eye(4)                    # every pair at d2 = 6: (0, 1) goes first, then {0, 1} takes 2 (its d2 stays 6, tying (2, 3))
    assert np.all(distances_from_gram(G)[~np.eye(4, dtype=bool)] == 6.0)
    assert list(clusters_from_gram(G, 3)["labels"]) == [0, 0, 1, 2]
    out = clusters_from_gram(G, 2)
    assert list(out["labels"]) == [0, 0, 0, 1] and list(out["sizes"]) == [3, 1]
    assert list(out["medoids"]) == [0, 3] and list(out["within"]) == [12.0, 0.0]       # equal sums: the lowest member


def test_pure_function_argument_errors():
    from efa_xray_amd import clusters_from_gram, distances_from_gram, eofs_from_gram
    G = np.eye(5)
    for bad, word in ((np.ones((3, 4)), "expected (M, M)"), (np.ones(3), "expected (M, M)"), (np.ones((1, 1)), "members"),
                      (np.full((3, 3), np.nan), "finite"), ("ab", "square array"), (np.zeros((257, 257)), "members")):
        for fn, args in ((distances_from_gram, ()), (eofs_from_gram, (1,)), (clusters_from_gram, (1,))):
            with pytest.raises(ValueError, match=re.escape(word)):
                fn(bad, *args)
    for n in (0, 5, -1, 1.5, "x", None):
        with pytest.raises(ValueError, match="n_modes"):
            eofs_from_gram(G, n)
    for n in (0, 6, 2.5, None):
        with pytest.raises(ValueError, match="n_clusters"):
            clusters_from_gram(G, n)
    assert eofs_from_gram(G, 4)["pcs"].shape == (4, 5) and clusters_from_gram(G, 5)["labels"].shape == (5,)


# ---- norm, weights and the argument checks -----------------------------------------------------------------------------------
def _state(M=4, dtype=None, nvar=2, nt=2, ny=3, nx=5):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    return EnsembleState.from_array(rng.standard_normal((nvar, nt, ny, nx, M)), lat, lon, varnames=["t2m", "psfc"][:nvar],
                                    dtype=dtype)


def test_resolve_norm():
    from efa_xray_amd.postprocess.modes import _resolve_norm
    st = _state()
    assert np.array_equal(_resolve_norm(st, None), np.ones(4))
    assert _resolve_norm(st, "std") is None
    assert np.array_equal(_resolve_norm(st, {"psfc": 0.01}), [0.0, 0.0, 0.01, 0.01])          # not named: 0
    assert np.array_equal(_resolve_norm(st, {"t2m": [1.0, 0.0], "psfc": 2}), [1.0, 0.0, 2.0, 2.0])     # valid times picked


class _FakeCtx:
    """ctx.gram of a state whose variable iv has weighted mean variance var[iv]"""

    def __init__(self, var, nt, M):
        self.var, self.nt, self.M, self.calls = var, nt, M, []

    def gram(self, N, M, X, scale, ncol=None, n_lead=1, col_weight=None):
        scale = np.asarray(scale, dtype=np.float64)
        self.calls.append(scale.copy())
        tr = sum(v * np.sum(scale[iv * self.nt:(iv + 1) * self.nt] ** 2) * ncol for iv, v in enumerate(self.var))
        used = int(np.count_nonzero(scale)) * ncol
        return np.eye(M) * tr / M, used, 0, np.array([float(used), float(np.sum(scale ** 2) * ncol)])


def test_uploaded_gram_measures_the_std_scales_one_variable_at_a_time():
    from efa_xray_amd.postprocess.modes import _uploaded_gram
    ctx = _FakeCtx([4.0, 0.25], nt=2, M=6)
    out = _uploaded_gram(ctx, None, (2, 2, 3, 5, 6), None, None)
    assert len(ctx.calls) == 3
    assert np.array_equal(ctx.calls[0], [1, 1, 0, 0]) and np.array_equal(ctx.calls[1], [0, 0, 1, 1])
    assert np.allclose(out["scales"], [[0.5, 0.5], [2.0, 2.0]], rtol=1e-15) and np.array_equal(ctx.calls[2], out["scales"].reshape(-1))
    assert np.isclose(np.trace(out["gram"]), 2 * 30.0) and out["n"] == 60 and out["weight_sum"] == 60.0
    # a variable without variance: scale 0 and a warning
    ctx = _FakeCtx([4.0, 0.0], nt=2, M=6)
    with pytest.warns(RuntimeWarning, match="scale 0"):
        out = _uploaded_gram(ctx, None, (2, 2, 3, 5, 6), None, None)
    assert np.array_equal(out["scales"], [[0.5, 0.5], [0.0, 0.0]])
    # given scales: one call, no warning
    ctx = _FakeCtx([4.0, 0.25], nt=2, M=6)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = _uploaded_gram(ctx, None, (2, 2, 3, 5, 6), np.array([1.0, 0.0, 2.0, 2.0]), None)
    assert len(ctx.calls) == 1 and np.array_equal(out["scales"], [[1.0, 0.0], [2.0, 2.0]])


def test_argument_checks_raise_before_the_gpu_is_touched(monkeypatch):
    from efa_xray_amd import _lib, ensemble_clusters, ensemble_eofs, ensemble_gram

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(_lib, "get_context", no_gpu)
    st = _state()
    bad = [
        (dict(norm="var"), "expected None, 'std'"),
        (dict(norm=3.0), "expected None, 'std'"),
        (dict(norm={"rh": 1.0}), "no variable"),
        (dict(norm={"t2m": -1.0}), "finite and >= 0"),
        (dict(norm={"t2m": np.nan}), "finite and >= 0"),
        (dict(norm={"t2m": [1.0, np.inf]}), "finite and >= 0"),
        (dict(norm={"t2m": [1.0, 2.0, 3.0]}), "expected a number or (ntimes,)"),
        (dict(norm={"t2m": "x"}), "not a number"),
        (dict(weights=np.ones((3, 4))), "not broadcastable"),
        (dict(weights=-np.ones((3, 5))), "finite and >= 0"),
        (dict(weights=np.full(5, np.nan)), "finite and >= 0"),
        (dict(weights="ab"), "not broadcastable"),
    ]
    calls = ((ensemble_gram, ()), (ensemble_eofs, (2,)), (ensemble_clusters, (2,)))
    for kw, word in bad:
        for fn, args in calls:
            with pytest.raises(ValueError, match=re.escape(word)):
                fn(st, *args, **kw)
    for n in (0, 4, 2.5, None, "x"):
        with pytest.raises(ValueError, match="n_modes"):
            ensemble_eofs(st, n)
    for n in (0, 5, 1.5, None):
        with pytest.raises(ValueError, match="n_clusters"):
            ensemble_clusters(st, n)
    for fn, args in calls:
        with pytest.raises(ValueError, match="members"):
            fn(_state(M=1), *args)
        with pytest.raises(ValueError, match="members"):
            fn(_state(M=257, nvar=1, nt=1, ny=1, nx=2), *args)
        with pytest.raises(ValueError, match="no variables"):
            fn(type(st)({}, st.coords), *args)
        mixed = type(st)(st.variables, st.coords)
        mixed.variables["psfc"] = mixed.variables["psfc"].astype(np.float32)
        with pytest.raises(ValueError, match="mix dtypes"):
            fn(mixed, *args)


def test_model_stays_inside_its_own_bound():
    """The derived bound against a plain float64 NumPy evaluation of the definitions: well inside."""
    for n, M, off in ((5, 3, 0.0), (200, 17, 0.0), (2000, 100, 1e6), (3, 2, 1e6)):
        rng = np.random.default_rng(n + M)
        X = off + rng.standard_normal((n, M))
        c = rng.uniform(0.5, 2.0, n)
        m = gm.model(X, 1, [1.0], c)
        Xp = X - X.sum(axis=1, keepdims=True) / M
        G = (Xp * c[:, None]).T @ Xp / (M - 1.0)
        assert m["n"] == n and gm.ratio(G, m) <= 0.25, (n, M, off)
