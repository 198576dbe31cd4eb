"""The LETKF with cross validation without a device: the NumPy model of tests/_letkf_cv.py (its two routes to
T[I,H], the recentring, the mean), the seeded cases' condition on their inputs, the front end's refusals, the symbol's three
declarations, and the scratch of k_letkf_cv."""
import os
import re

import numpy as np
import pytest

import _etkf as ek
import _letkf as lk
import _letkf_cv as cv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_TOL = 1e-10
SMALL = [case for case in cv.CASES if case[0] <= 40] + [cv.PERMUTED]
WELL_OBSERVED = [(16, 4, 64, 5, 7, 3), (40, 8, 400, 6, 7, 3)]     # many more obs in reach than members


@pytest.fixture(autouse=True)
def _the_feature_exists():
    """The model below describes efa_ctx_set_letkf_cross_validation: without the entry point there is nothing for it to describe."""
    from efa_xray_amd import _lib
    assert "efa_ctx_set_letkf_cross_validation" in _lib.SIGNATURES, "the library has no cross validation"


def _points(c, n=3):
    """(rho, ym, Yp) of the case at its first n columns and first n ob positions."""
    ym, Yp = ek.ob_priors(c["HX"])
    lat = np.concatenate([c["grid_lat"].reshape(-1)[:n], c["ob_lat"][:n]])
    lon = np.concatenate([c["grid_lon"].reshape(-1)[:n], c["ob_lon"][:n]])
    return lk.taper(lat, lon, c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"]), ym, Yp


# ---- 1. the model: two routes, the recentring, the mean -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL)
def test_the_two_routes_to_the_transform_agree(case):
    c, g = cv.make_case(*case, permuted=case is cv.PERMUTED)
    rho, ym, Yp = _points(c)
    seen = 0
    for i in range(rho.shape[0]):
        T, w, ex = cv.solve_point(rho[i], ym, Yp, c["value"], c["error"], c["assim"], g)
        if ex["n_local"] == 0:
            continue
        seen += 1
        T2 = cv.recentre(cv.transform_by_subfilter(rho[i], ym, Yp, c["value"], c["error"], c["assim"], g))
        err = np.abs(T2 - T).max()
        print("point %d: n_local %d, routes differ by %.2e of %.2e" % (i, ex["n_local"], err, np.abs(T).max()))
        assert err <= ROUTE_TOL * np.abs(T).max()
        if case in WELL_OBSERVED:       # gamma is nowhere small: the pseudo-inverse form as it stands
            T3 = cv.recentre(cv.transform_by_subfilter(rho[i], ym, Yp, c["value"], c["error"], c["assim"], g, form="pinv"))
            assert np.abs(T3 - T).max() <= ROUTE_TOL * np.abs(T).max()
        # ... and the held-out member's perturbation written out: x'_h - X'_I J G_k J C[I,h], before the recentring
        M = Yp.shape[1]
        C = ex["A"] - (M - 1.0) * np.eye(M)
        Traw = cv.transform(C, g)
        x = np.random.default_rng(i).standard_normal(M)
        x -= x.mean()
        for I, H in cv._sets(g):
            m = I.size
            J = np.eye(m) - 1.0 / m
            mu, V = np.linalg.eigh((m - 1.0) * np.eye(m) + J @ C[np.ix_(I, I)] @ J)
            gam = mu - (m - 1.0)
            coef = np.where(gam > 1e-8 * mu, (1.0 - np.sqrt((m - 1.0) / mu)) / np.where(gam > 1e-8 * mu, gam, 1.0), 0.5 / (m - 1.0))
            G = (V * coef) @ V.T                     # the definition's other form, with the division by gamma
            direct = x[H] - (x[I] @ J @ G @ J) @ C[np.ix_(I, H)]
            assert np.abs(direct - (x @ Traw)[H]).max() <= 1e-8 * max(1.0, np.abs(direct).max())
    assert seen, "the case: some point is reached"


@pytest.mark.parametrize("case", SMALL)
def test_recentred_rows_sum_to_zero_and_the_mean_is_the_plain_filters(case):
    c, g = cv.make_case(*case, permuted=case is cv.PERMUTED)
    ref = cv.cv_cycle(c, g)
    plain = lk.letkf_cycle(c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                           c["grid_lon"], c["n_lead"])
    st = ref["stats"]
    assert max(st["cond"].max(), st["cv_cond"].max(), ref["ob_stats"]["cond"].max(), ref["ob_stats"]["cv_cond"].max()) <= cv.COND_CAP
    M = c["M"]
    reached = st["n_local"] > 0
    assert reached.any()
    T = ref["T"][reached]
    assert np.abs(T.sum(axis=2)).max() <= 1e-13 * M, "T 1 = 0 after step 3"
    # before the recentring every column of a reached point's T has the identity block: the row means are what step 3 takes off
    rho, ym, Yp = _points(c, 2)
    for i in range(rho.shape[0]):
        _, _, ex = lk.solve_point(rho[i], ym, Yp, c["value"], c["error"], c["assim"])
        if ex["n_local"]:
            raw = cv.transform(ex["A"] - (M - 1.0) * np.eye(M), g)
            assert np.all(np.diag(raw) == 1.0)
            assert np.abs(cv.recentre(raw) - (raw - (raw @ np.ones(M) / M)[:, None])).max() <= 4 * np.finfo(float).eps
    # the posterior perturbations sum to zero, the mean is the plain model's: the same w, exactly
    assert np.array_equal(ref["w"], plain["w"])
    X = c["X"]
    ncol, n_lead = c["ncol"], c["n_lead"]
    for col in np.flatnonzero(reached)[:4]:
        rows = col + ncol * np.arange(n_lead)
        Xp = X[rows] - X[rows].mean(axis=1, keepdims=True)
        assert np.abs((Xp @ ref["T"][col]).sum(axis=1)).max() <= 1e-12 * M * np.abs(Xp).max()
    scale = np.abs(plain["post"]).max()
    assert np.abs(ref["post"].mean(axis=1) - plain["post"].mean(axis=1)).max() <= 1e-13 * scale
    assert np.abs(ref["ym"] - plain["ym"]).max() <= 1e-13 * max(1.0, np.abs(plain["ym"]).max())
    assert np.abs(ref["post"] - plain["post"]).max() > 1e-6 * scale, "cross validation changes the perturbations"
    # the cure for inbreeding: the cross-validated spread is the larger one
    assert ref["post"][_rows(c, reached)].var(axis=1).mean() > plain["post"][_rows(c, reached)].var(axis=1).mean()


def _rows(c, cols):
    return (np.flatnonzero(cols)[None, :] + c["ncol"] * np.arange(c["n_lead"])[:, None]).reshape(-1)


def test_the_large_cases_hold_the_condition_on_their_inputs():
    """cond(A) <= 1e4 for the full solve and every sub-solve at M = 80 and 136 (the model asserts it; the GPU tests rely on it)."""
    for case in [k for k in cv.CASES if k[0] > 40]:
        c, g = cv.make_case(*case)
        rho, ym, Yp = _points(c, 4)
        for i in range(rho.shape[0]):
            _, _, ex = cv.solve_point(rho[i], ym, Yp, c["value"], c["error"], c["assim"], g)
            assert ex["cond"] <= cv.COND_CAP and ex["cv_cond"] <= cv.COND_CAP


def test_labels_and_their_rules():
    assert np.array_equal(cv.labels(3, 7), [0, 1, 2, 0, 1, 2, 0])
    assert np.array_equal(cv.labels(np.array([1, 0, 1, 0]), 4), [1, 0, 1, 0])
    assert sorted(np.bincount(cv.permuted_labels(17, 4, 5))) == [4, 4, 4, 5]
    for bad, M in ((1, 6), (0, 6), (True, 6), (2.0, 6), ("2", 6), (np.array([0, 1, 2, 0]), 5), (np.array([0, 2, 0, 2, 0]), 5),
                   (np.array([0, 0, 0, 1]), 4), (np.array([-1, 0, 1, 0]), 4), (np.array([0.0, 1.0, 0.0, 1.0]), 4), (2, 3), (4, 3)):
        with pytest.raises(ValueError):
            cv.labels(bad, M)


# ---- 2. the front end ------------------------------------------------------------------------------------------------------------------
def _tiny(M=6):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(3)
    lat, lon = np.meshgrid(np.linspace(20, 60, 4), np.linspace(200, 280, 5), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((1, 1, 4, 5, M)), lat, lon)
    obs = [Observation(value=0.5, error=1.0, lat=40.0, lon=240.0, localize_radius=1000.0)]
    return state, obs, lat, lon


def test_the_keyword_validates_the_groups_before_any_device_work(monkeypatch):
    from efa_xray_amd import EnsembleState, LETKF, SlabLETKF, EnSRF, ETKF, ColumnInflation
    from efa_xray_amd.assimilation.assimilation import Assimilation

    def no_device(self):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(Assimilation, "_context", no_device)
    state, obs, lat, lon = _tiny()
    ctrl = EnsembleState.from_array(np.random.default_rng(4).standard_normal((1, 1, 4, 5, 1)), lat, lon)
    for cls in (LETKF, SlabLETKF):
        assert cls(state, obs, verbose=False).cross_validation is None
        assert np.array_equal(cls(state, obs, verbose=False, cross_validation=2).cross_validation, [0, 1, 0, 1, 0, 1])
        assert np.array_equal(cls(state, obs, verbose=False, cross_validation=np.int64(3)).cross_validation, [0, 1, 2, 0, 1, 2])
        lab = np.array([2, 0, 1, 1, 0, 2])
        f = cls(state, obs, verbose=False, cross_validation=lab, weight_stride=2, max_local_obs=3, rtps=0.9, outlier_threshold=3.0)
        assert np.array_equal(f.cross_validation, lab) and f.cross_validation.dtype == np.int32
        assert np.array_equal(cls(state, obs, verbose=False, cross_validation=list(lab)).cross_validation, lab)
        assert np.array_equal(cls(state, obs, verbose=False, cross_validation=6).cross_validation, np.arange(6)), "leave one out"
        for bad in (1, 0, -2, True, 2.0, "2", (0.0, 1.0, 0.0, 1.0, 0.0, 1.0), np.zeros((2, 3), dtype=int),
                    [0, 1, 0, 1, 0],                # five labels for six members
                    [0, 1, 3, 0, 1, 3],             # the label 2 is unused
                    [0, 0, 0, 0, 0, 0],             # one group
                    [-1, 0, 1, 0, 1, 0],            # a negative label
                    [0, 0, 0, 0, 0, 1],             # group 0 leaves one member outside it
                    7):                             # m % 7 on six members leaves the label 6 unused
            with pytest.raises(ValueError, match="cross_validation"):
                cls(state, obs, verbose=False, cross_validation=bad)
        with pytest.raises(ValueError, match="cross_validation and column_inflation"):
            cls(state, obs, verbose=False, cross_validation=2, column_inflation=ColumnInflation(sigma_b=0.04))
        with pytest.raises(ValueError, match="cross_validation and control"):
            cls(state, obs, verbose=False, cross_validation=2, control=ctrl)
    for kw in (dict(vert_coord=np.zeros((1, 1))), dict(time_localize=True), dict(var_impact={"a": {"a": 1.0}})):
        with pytest.raises(ValueError, match="cross_validation"):
            SlabLETKF(state, obs, verbose=False, cross_validation=2, **kw)
    small, sobs, _, _ = _tiny(M=3)
    with pytest.raises(ValueError, match="cross_validation"):
        LETKF(small, sobs, verbose=False, cross_validation=2)       # 3 members: a group of 2 leaves 1
    for cls, kw in ((EnSRF, dict(loc="GC")), (ETKF, {})):
        with pytest.raises((TypeError, ValueError)):
            cls(state, obs, verbose=False, cross_validation=2, **kw)


# ---- 3. the symbol: declared, bound, exported -------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_and_exported():
    from efa_xray_amd import _lib
    header = open(os.path.join(ROOT, "include", "efa_hip.h")).read()
    m = re.search(r"int\s+efa_ctx_set_letkf_cross_validation\s*\(([^;]*)\)\s*;", header)
    assert m, "include/efa_hip.h does not declare efa_ctx_set_letkf_cross_validation"
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == 6
    restype, argtypes = _lib.SIGNATURES["efa_ctx_set_letkf_cross_validation"]
    assert len(argtypes) == 6
    lib = _lib.load_library()
    assert lib.efa_ctx_set_letkf_cross_validation.argtypes == argtypes
    assert hasattr(_lib.Context, "set_letkf_cross_validation")


# ---- 4. k_letkf_cv uses no scratch ---------------------------------------------------------------------------------------------------
def test_k_letkf_cv_uses_no_scratch():
    import _codeobj
    from efa_xray_amd import _lib
    table = _codeobj.kernel_table(_lib.LIB_PATH)
    ks = {n: k for n, k in table.items() if "k_letkf_cvI" in n}
    assert len(ks) == 3, "k_letkf_cv at 256, 512 and 1024 threads: %r" % sorted(ks)
    for n, k in sorted(ks.items()):
        print(n, "vgpr", k[".vgpr_count"], "agpr", k.get(".agpr_count", 0), "sgpr", k[".sgpr_count"], "lds", k[".group_segment_fixed_size"],
              "scratch", k[".private_segment_fixed_size"])
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, n
