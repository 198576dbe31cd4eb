"""Per-column multiplicative inflation of the LETKF without a device: the NumPy model of tests/_letkf_infl.py
against the plain model on inflated inputs, the convergence of Miyoshi's (2011) estimator on synthetic innovations, and the
front end's refusals, shape checks and ob-factor rule."""
import numpy as np
import pytest

import _etkf as ek
import _letkf as lk
import _letkf_infl as lf


# ---- 1. a uniform factor is the plain filter on inputs inflated by sqrt(lambda) ------------------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead,lam", [(3, 5, 3, 5, 2, 1.44), (17, 33, 5, 7, 3, 1.44), (12, 40, 4, 5, 2, 0.7)])
def test_uniform_factor_equals_the_plain_model_on_inflated_inputs(M, P, ny, nx, n_lead, lam):
    c = lk.make_case(M, P, ny, nx, n_lead)
    geo = (c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"], c["grid_lon"], n_lead)
    got = lf.letkf_cycle(c["X"], c["HX"], *geo, lam=np.full(c["ncol"], lam), ob_infl=np.full(P, lam))
    want = lk.letkf_cycle(lf.inflate_rows(c["X"], lam), lf.inflate_rows(c["HX"], lam), *geo)
    for k in ("post", "ym", "Yp"):
        scale = np.abs(want[k]).max()
        err = np.abs(got[k] - want[k]).max()
        print("%s: max abs err %.3e, scale %.3e" % (k, err, scale))
        assert err <= 1e-10 * scale
    assert np.array_equal(got["stats"]["n_local"], want["stats"]["n_local"])
    assert np.abs(got["stats"]["dfs"] - want["stats"]["dfs"]).max() <= 1e-10 * max(1.0, want["stats"]["dfs"].max())
    # and a factor of 1 is the plain model itself
    one = lf.letkf_cycle(c["X"], c["HX"], *geo, lam=np.ones(c["ncol"]))
    plain = lk.letkf_cycle(c["X"], c["HX"], *geo)
    assert np.abs(one["post"] - plain["post"]).max() <= 1e-13 * np.abs(plain["post"]).max()


# ---- 2. the estimator converges to the factor the innovations were drawn with ---------------------------------------------------------
@pytest.mark.parametrize("sigma_b", [0.04, 0.2])
def test_the_estimator_converges(sigma_b):
    M, P, lam_true, cycles = 20, 60, 1.8, 4000
    rng = np.random.default_rng(2011)
    lam, hist = 1.0, np.empty(cycles)
    for t in range(cycles):
        Yp = rng.standard_normal((P, M))
        Yp -= Yp.mean(axis=1, keepdims=True)
        s2 = np.sum(Yp * Yp, axis=1) / (M - 1.0)
        r = rng.uniform(0.5, 2.0, P)
        rho = rng.uniform(0.05, 1.0, P)
        d = np.sqrt(lam_true * s2 + r) * rng.standard_normal(P)
        _, _, ex = lf.solve_point(rho, np.zeros(P), Yp, d, r, np.ones(P, dtype=bool), lam)
        lam = lf.estimate(lam, ex["p1"], ex["p2"], ex["p3"], sigma_b, 1e-2, 1e2)
        hist[t] = lam
    mean = hist[-1500:].mean()
    print("sigma_b=%g: mean of the last 1500 factors %.4f (true %.1f)" % (sigma_b, mean, lam_true))
    assert abs(mean - lam_true) <= 0.1


def test_estimate_edge_rules_of_the_model():
    assert lf.estimate(1.3, 5.0, 2.0, 3.0, 0.0, 1e-2, 1e2) == 1.3                 # sigma_b == 0: fixed
    assert lf.estimate(1.3, 5.0, 0.0, 3.0, 0.04, 1e-2, 1e2) == 1.3                # p2 == 0
    assert lf.estimate(1.3, np.nan, 2.0, 3.0, 0.04, 1e-2, 1e2) == 1.3             # a NaN innovation
    assert lf.estimate(1.3, 1e30, 2.0, 3.0, 10.0, 1e-2, 1e2) == 1e2               # clipped above
    assert lf.estimate(1.3, 0.0, 2.0, 3.0, 10.0, 1e-2, 1e2) == 1e-2               # and below (lam_o = -1.5, gain 0.95)


# ---- 3. the front end without a device ---------------------------------------------------------------------------------------------
def test_column_inflation_validates_its_arguments():
    from efa_xray_amd import ColumnInflation
    import efa_xray_amd
    assert "ColumnInflation" in efa_xray_amd.__all__
    ci = ColumnInflation()
    assert (ci.initial, ci.sigma_b, ci.lower, ci.upper, ci.values) == (1.0, 0.04, 1e-2, 1e2, None)
    for kw in (dict(sigma_b=-0.1), dict(sigma_b=np.nan), dict(lower=0.0), dict(lower=-1.0), dict(lower=2.0, upper=1.0),
               dict(upper=np.inf), dict(initial=0.0), dict(initial=1e3), dict(initial=np.nan),
               dict(values=np.array([[1.0, np.nan]])), dict(values=np.array([[1.0, 0.0]])), dict(values=np.array([[1.0, 1e3]]))):
        with pytest.raises(ValueError):
            ColumnInflation(**kw)


def test_values_are_created_in_the_solve_layout_and_checked_against_it(tmp_path):
    from efa_xray_amd import ColumnInflation
    ci = ColumnInflation(initial=1.2)
    f = ci.field((3, 5))
    assert f.shape == (3, 5) and np.all(f == 1.2) and ci.values is f
    assert ci.field((3, 5)) is f
    for shape in ((5, 3), (2, 3, 5), (15,)):
        with pytest.raises(ValueError, match="shape"):
            ci.field(shape)
    given = ColumnInflation(values=np.full((2, 4, 3), 1.5))
    assert given.field((2, 4, 3)).shape == (2, 4, 3)
    with pytest.raises(ValueError, match="shape"):
        given.field((4, 3))
    given.values[0, 0, 0] = np.nan          # a field that left the bounds is refused at the next update
    with pytest.raises(ValueError):
        given.field((2, 4, 3))
    with pytest.raises(ValueError):
        ColumnInflation().save(str(tmp_path / "none.npy"))
    path = str(tmp_path / "lam.npy")
    ci.values[1, 2] = 1.7
    ci.save(path)
    back = ColumnInflation().load(path)
    assert np.array_equal(back.values, ci.values) and back.values is not ci.values


def _tiny_state():
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(3)
    lat, lon = np.meshgrid(np.linspace(20, 60, 4), np.linspace(200, 280, 5), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((1, 1, 4, 5, 6)), lat, lon)
    obs = [Observation(value=0.5, error=1.0, lat=40.0, lon=240.0, localize_radius=1000.0)]
    return state, obs


def test_the_keyword_is_taken_by_the_letkf_classes_only():
    from efa_xray_amd import ColumnInflation, LETKF, SlabLETKF, EnSRF, ETKF
    from efa_xray_amd.assimilation.adaptive_inflation import AdaptiveInflation
    state, obs = _tiny_state()
    ci = ColumnInflation()
    assert LETKF(state, obs, verbose=False, column_inflation=ci).column_inflation is ci
    assert SlabLETKF(state, obs, verbose=False, column_inflation=ci).column_inflation is ci
    assert LETKF(state, obs, verbose=False).column_inflation is None
    with pytest.raises(ValueError, match="ColumnInflation"):
        LETKF(state, obs, verbose=False, column_inflation=1.2)
    for cls in (LETKF, SlabLETKF):
        with pytest.raises(ValueError, match="adaptive inflation follows the serial order of the observations"):
            cls(state, obs, verbose=False, adaptive_inflation=AdaptiveInflation(state, ("spatial", None, (1.0, 0.6))))
    for cls, kw in ((EnSRF, dict(loc="GC")), (ETKF, {})):
        with pytest.raises((TypeError, ValueError)):
            cls(state, obs, verbose=False, column_inflation=ci, **kw)


def test_ob_factors_on_a_hand_made_stencil():
    from efa_xray_amd.assimilation.letkf_inflation import ob_factors, expand_nodes
    ncol = 6
    field = np.array([[1.0, 1.1, 1.2, 1.3, 1.4, 1.5], [2.0, 2.1, 2.2, 2.3, 2.4, 2.5]])      # (ngroups, ncol)
    group_of = np.array([0, 1, 1])                                                         # three slabs
    idx = np.array([[0, 1, 6, 7], [14, 17, 0, 0], [5, 11, 12, 13]])                        # rows lead * ncol + col
    wts = np.array([[0.25, 0.25, 0.25, 0.25], [0.5, 0.5, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    want = np.array([0.25 * (1.0 + 1.1 + 2.0 + 2.1), 0.5 * (2.2 + 2.5), 1.5])
    got = ob_factors(field, group_of, idx, wts)
    assert np.allclose(got, want, rtol=1e-15, atol=0.0)
    lam_rows = field[group_of].reshape(-1)                                                 # the field expanded to state rows
    assert np.allclose(got, lf.ob_factors(lam_rows, idx, wts), rtol=1e-15, atol=0.0)
    assert ob_factors(field, group_of, np.array([[-1, 3]]), np.array([[0.0, 1.0]]))[0] == 1.3   # a weightless entry is not read
    # the node field to columns: bilinear in grid-index space, nodes reproduced, the last cell shorter
    node_y, node_x = np.array([0, 2, 4]), np.array([0, 3, 6])
    nodes = np.arange(9.0).reshape(3, 3)
    cols = expand_nodes(nodes, node_y, node_x, 5, 7)
    assert cols.shape == (5, 7) and np.array_equal(cols[np.ix_(node_y, node_x)], nodes)
    assert cols[1, 0] == 1.5 and cols[0, 1] == pytest.approx(1.0 / 3.0) and cols[3, 4] == pytest.approx(0.5 * 3 + 0.5 * 6 + 1 + 1.0 / 3.0)
    assert expand_nodes(nodes[None], node_y, node_x, 5, 7).shape == (1, 5, 7)
    one = expand_nodes(np.array([[1.3]]), np.array([0]), np.array([0]), 1, 1)
    assert one.shape == (1, 1) and one[0, 0] == 1.3
