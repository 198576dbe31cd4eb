"""LETKF weight interpolation without a GPU: the node sets and corner weights of the definition, the properties of
the NumPy model of tests/_letkf_interp.py that the GPU tests lean on, and the refusals of the Python surface."""
import numpy as np
import pytest

import _letkf as lk
import _letkf_interp as li


def _cycle(c, stride, **over):
    g = dict(c, **over)
    return li.interp_cycle(g["X"], g["HX"], g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"], g["grid_lat"],
                           g["grid_lon"], g["n_lead"], (g["ny"], g["nx"]), stride)


@pytest.mark.parametrize("n,s", [(1, 3), (2, 5), (5, 2), (4, 3), (6, 4), (7, 1)])
def test_node_sets_and_corner_weights(n, s):
    nodes = li.axis_nodes(n, s)
    want = sorted(set(range(0, n - 1, s)) | {n - 1})
    assert nodes.tolist() == want
    assert nodes.size == (1 if n == 1 else -(-(n - 1) // s) + 1)
    from efa_xray_amd import _lib
    assert np.array_equal(_lib.letkf_mesh_nodes(n, s), nodes)
    # the same axis as y against another as x, and the other way round
    for ny, nx, stride in ((n, 5, (s, 2)), (3, n, (4, s))):
        m = li.mesh(ny, nx, stride)
        beta = m["beta"]
        assert np.all(beta >= 0.0)
        assert np.all(np.abs(beta.sum(axis=1) - 1.0) <= np.finfo(float).eps)
        for c in m["node_col"]:
            assert np.sort(beta[c]).tolist() == [0.0, 0.0, 0.0, 1.0], "a node column has one weight of exactly 1"
        for k, c in enumerate(m["node_col"]):
            assert m["corner"][c, int(np.argmax(beta[c]))] == k, "... on its own node"
        # a column on a node line uses the nodes of that line only
        for iy in range(ny):
            for ix in range(nx):
                used = m["corner"][iy * nx + ix][beta[iy * nx + ix] != 0.0]
                ys, xs = m["node_y"][used // m["node_x"].size], m["node_x"][used % m["node_x"].size]
                if iy in m["node_y"]:
                    assert np.all(ys == iy)
                if ix in m["node_x"]:
                    assert np.all(xs == ix)
                assert ys.min() <= iy <= ys.max() and xs.min() <= ix <= xs.max()


def test_interpolated_pairs_keep_the_mean_and_the_centring():
    c = lk.make_case(16, 64, 5, 7, 2)
    r = _cycle(c, (2, 3))
    one = np.ones(16)
    assert np.abs(r["T"] @ one - 1.0).max() <= 1e-12, "T_c 1 = 1"
    assert np.abs(r["w"] @ one).max() <= 1e-12, "1^T w_c = 0"


def test_very_wide_tapers_make_the_interpolation_exact():
    c = lk.make_case(16, 64, 5, 7, 2)
    hw = np.full(c["P"], 1e12)
    r = _cycle(c, (2, 3), ob_hw=hw)
    scale = np.abs(r["plain_post"]).max()
    assert np.abs(r["post"] - r["plain_post"]).max() <= 1e-10 * scale
    assert np.abs(r["post"] - c["X"]).max() > 1e-3 * scale, "the update moves the state"


def test_unit_stride_is_the_plain_model():
    c = lk.make_case(17, 33, 5, 7, 3)
    r = _cycle(c, (1, 1))
    p = lk.letkf_cycle(c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                       c["grid_lon"], c["n_lead"])
    assert np.array_equal(r["post"], p["post"]) and np.array_equal(r["Yp"], p["Yp"]) and np.array_equal(r["ym"], p["ym"])
    # ... and the general route of the model, made to take a unit stride, agrees with it to the bit as well: one weight of exactly 1
    m = li.mesh(5, 7, (1, 1))
    Tc, wc, reached = li.column_pairs(m, p["T"], p["w"], p["stats"]["n_local"])
    assert np.array_equal(Tc, p["T"]) and np.array_equal(wc, p["w"])
    assert np.array_equal(li.apply_pairs(c["X"], 35, 3, Tc, wc, reached), p["post"])


@pytest.mark.parametrize("bad", [0, (2, 0), 2.5, (1, 2, 3), -1, True, "2"])
def test_a_bad_weight_stride_is_refused_before_any_device_work(bad):
    from efa_xray_amd import EnsembleState, LETKF, Observation
    rng = np.random.default_rng(3)
    lat, lon = np.meshgrid(np.linspace(20, 60, 4), np.linspace(200, 280, 5), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((1, 1, 4, 5, 6)), lat, lon)
    obs = [Observation(value=0.0, error=1.0, lat=40.0, lon=240.0, localize_radius=1000.0)]
    with pytest.raises(ValueError) as e:
        LETKF(state, obs, verbose=False, device=10 ** 6, weight_stride=bad)
    assert "weight_stride" in str(e.value)


@pytest.mark.parametrize("plain", [None, 1, (1, 1)])
def test_a_unit_weight_stride_is_the_plain_filter(plain):
    from efa_xray_amd import EnsembleState, LETKF, Observation
    rng = np.random.default_rng(3)
    lat, lon = np.meshgrid(np.linspace(20, 60, 4), np.linspace(200, 280, 5), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((1, 1, 4, 5, 6)), lat, lon)
    obs = [Observation(value=0.0, error=1.0, lat=40.0, lon=240.0, localize_radius=1000.0)]
    assert LETKF(state, obs, verbose=False, device=10 ** 6, weight_stride=plain).weight_stride is None
    assert LETKF(state, obs, verbose=False, device=10 ** 6, weight_stride=(2, 1)).weight_stride == (2, 1)
    assert LETKF(state, obs, verbose=False, device=10 ** 6, weight_stride=np.int64(3)).weight_stride == (3, 3)
