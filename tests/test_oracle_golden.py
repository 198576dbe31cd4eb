"""Pin the CPU oracle (oracle/ensrf_oracle.py) to the reference's own outputs.

The fixtures were produced by running the reference's modules in the build
container (tests/golden/make_goldens.py).  On the NumPy/OpenBLAS install that
made them the restatement is bit-identical; elsewhere BLAS summation order may
differ, so the portable assertion is rtol 1e-12 and bit-equality is reported.
"""
import numpy as np
import pytest

from conftest import load_golden
from oracle import ensrf_oracle as orc

RTOL = 1e-12


def _close(a, b, what):
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, what
    scale = max(np.nanmax(np.abs(b)), 1e-300) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=1e-14 * scale, equal_nan=True, err_msg=what)


def test_known_answers_scalar_functions():
    k = load_golden("KAT")
    assert np.array_equal(orc.gaspari_cohn(k["gc_d"], float(k["gc_c"])), k["gc_w"])
    assert np.array_equal(orc.gaspari_cohn(k["gc_d"], -float(k["gc_c"])), k["gc_w_neg"])
    # survey probe values
    w = orc.gaspari_cohn(np.array([0, 400, 800, 1200, 1599, 1600, 2000.0]), 800.0)
    np.testing.assert_allclose(w, [1, 0.684895833333, 0.208333333333, 0.0164930555556, 7.632e-13, 0, 0],
                               rtol=2e-4, atol=1e-16)
    hv = np.array([orc.haversine(tuple(a), tuple(b)) for a, b in zip(k["hv_a"], k["hv_b"])])
    assert np.array_equal(hv, k["hv_km"])
    assert abs(hv[0] - 325.1000863921916) < 1e-9
    assert hv[1] == 0.0
    d = orc.distance_to_point(k["dp_lat"], k["dp_lon"], *k["dp_pt"])
    assert np.array_equal(d, k["dp_km"])


def _check_oracle_against_reference(g, obs_taper="loop", step_hook=None):
    """The oracle's serial loop on fixture g against the reference's outputs; returns (bit-identical, diag)."""
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    X = g["X"].reshape(N, M)
    # forward operator output as the reference's compute_ob_priors saw it
    HX = np.array([(g["sten_wts"][k][:, None] * X[g["sten_idx"][k]]).sum(axis=0)
                   if g["sten_wts"][k][0] != 1.0 else X[g["sten_idx"][k][0]]
                   for k in range(len(g["ob_value"]))])
    assert np.array_equal(HX, g["HX"])
    xbm, Xbp = orc.format_prior_state(X, HX)
    if "xbm" in g:
        assert np.array_equal(xbm, g["xbm"]) and np.array_equal(Xbp, g["Xbp"])
    kw = {}
    if g["loc"] == "GC":
        kw = dict(loc="GC", ob_lat=g["ob_lat"], ob_lon=g["ob_lon"], ob_halfwidth=g["ob_radius"],
                  grid_lat=g["grid_lat"], grid_lon=g["grid_lon"], state_shape=(nvar, nt, ny, nx),
                  obs_taper=obs_taper)
    xam, Xap, diag = orc.ensrf_update(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"],
                                      step_hook=step_hook, **kw)
    post = orc.format_posterior_state(xam, Xap, N)
    _close(xam, g["xam"], "xam")
    if "Xap" in g:
        _close(Xap, g["Xap"], "Xap")
    _close(post, g["post"], "post")
    for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
        _close(diag[key], g[key], key)
    assert np.array_equal(diag["assimilated"], g["assimilated"])
    bit = np.array_equal(post, g["post"]) and np.array_equal(xam, g["xam"])
    if "Xap" in g:
        bit = bit and np.array_equal(Xap, g["Xap"])
    return bit, diag


def test_oracle_matches_reference(golden):
    g = golden
    bit, _ = _check_oracle_against_reference(g)
    print("%s bit-identical to reference: %s" % (g["name"], bit))


@pytest.mark.parametrize("name", ["G1", "G2", "G5"])
def test_faithful_cost_mode_same_bits(name):
    g = load_golden(name)
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    kw = {}
    if g["loc"] == "GC":
        kw = dict(loc="GC", ob_lat=g["ob_lat"], ob_lon=g["ob_lon"], ob_halfwidth=g["ob_radius"],
                  grid_lat=g["grid_lat"], grid_lon=g["grid_lon"], state_shape=(nvar, nt, ny, nx))
    a = orc.ensrf_update(g["xbm"], g["Xbp"], N, g["ob_value"], g["ob_error"], g["ob_assim"], **kw)
    b = orc.ensrf_update(g["xbm"], g["Xbp"], N, g["ob_value"], g["ob_error"], g["ob_assim"],
                         faithful_cost=True, **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for key in a[2]:
        assert np.array_equal(a[2][key], b[2][key], equal_nan=True)


# ---------------------------------------------------------------------------
# f1: forward operator, pinned by the reference's own nearest_points / interpolate /
# Observation.estimate run verbatim (fixtures G9 2-D lat/lon, G10 1-D lat/lon, G11 end to end)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["G9", "G10"])
def test_oracle_forward_operator_matches_reference(name):
    g = load_golden(name)
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    eye = np.eye(nt * ny * nx).reshape(nt, ny, nx, -1)
    bit = True
    for k in range(len(g["ob_lat"])):
        args = (g["grid_lat"], g["grid_lon"], g["validtime"], g["ob_time"][k], g["ob_lat"][k], g["ob_lon"][k])
        near = orc.nearest_points(g["grid_lat"], g["grid_lon"], g["ob_lat"][k], g["ob_lon"][k], npt=4)
        assert np.array_equal(np.stack(near, axis=-1), g["nearest"][k]), "ob %d: nearest four" % k
        hx = orc.interpolate(g["X"][g["ob_var"][k]], *args)
        w = orc.interpolate(eye, *args)
        _close(hx, g["HX"][k], "ob %d: estimate" % k)
        _close(w, g["weights"][k], "ob %d: stencil weights" % k)
        bit = bit and np.array_equal(hx, g["HX"][k]) and np.array_equal(w, g["weights"][k])
    # outside the valid times the reference returns None (ensemble.py:207-209)
    assert orc.interpolate(g["X"][0], g["grid_lat"], g["grid_lon"], g["validtime"],
                           g["validtime"][-1] + np.timedelta64(1, "s"), g["ob_lat"][0], g["ob_lon"][0]) is None
    print("%s forward operator bit-identical to reference: %s" % (name, bit))


def test_oracle_cycle_with_the_reference_forward_operator_end_to_end():
    """G11: EnSRF.update() with plain Observations (ensrf.py:33-151 incl. assimilation.py:36-49 ->
    observation.py:40-50 -> ensemble.py:170-239)."""
    g = load_golden("G11")
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    HX = np.array([orc.interpolate(g["X"][g["ob_var"][k]], g["grid_lat"], g["grid_lon"], g["validtime"],
                                   g["ob_time"][k], g["ob_lat"][k], g["ob_lon"][k]) for k in range(len(g["ob_lat"]))])
    _close(HX, g["HX"], "HX")
    for taper in ("loop", "vector"):
        post, xam, _, diag = orc.ensrf_cycle(g["X"].reshape(N, M), HX, g["ob_value"], g["ob_error"], g["ob_assim"],
                                             loc="GC", ob_lat=g["ob_lat"], ob_lon=g["ob_lon"], ob_halfwidth=g["ob_radius"],
                                             grid_lat=g["grid_lat"], grid_lon=g["grid_lon"], state_shape=(nvar, nt, ny, nx),
                                             obs_taper=taper)
        _close(xam, g["xam"], taper + " xam")
        _close(post, g["post"], taper + " post")
        for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
            _close(diag[key], g[key], taper + " " + key)
        assert np.array_equal(diag["assimilated"], g["assimilated"])


# ---------------------------------------------------------------------------
# the vector obs-obs taper (obs_taper="vector"): what lets the oracle follow thousands of obs
# ---------------------------------------------------------------------------
GC_GOLDENS = ["G2", "G3", "G5", "G6", "G8"]


def _taper_sets():
    """Obs sets for the loop-vs-vector comparison: the GC goldens' and seeded ones with the geometric edges."""
    sets = []
    for name in GC_GOLDENS:
        g = load_golden(name)
        sets.append((name, g["ob_lat"], g["ob_lon"], g["ob_radius"]))
    rng = np.random.default_rng(2718)
    lat = rng.uniform(-89, 89, 150)
    lon = rng.uniform(-180, 360, 150)
    hw = rng.uniform(200, 3000, 150)
    edges = [(lat[0], lon[0]),                                   # zero distance to ob 0
             (10.0, 359.95), (10.0, 0.05), (10.0, -0.05), (-20.0, 179.9), (-20.0, -179.9), (-20.0, 540.1),
             (33.0, 0.0), (33.0, 360.0), (0.0, -180.0), (0.0, 180.0),                 # longitude wrap
             (45.0, 10.0), (-45.0, 190.0), (-45.0, 189.999999), (89.99, 0.0), (-89.99, 180.0)]   # (near-)antipodes
    # r just inside / just outside 1 and 2 of ob "c" (along its meridian, where the distance is exact to rounding)
    c_lat, c_lon, c_hw = 12.5, 77.0, 900.0
    for r in (1.0 - 1e-9, 1.0 + 1e-9, 2.0 - 1e-9, 2.0 + 1e-9, 1.0 - 1e-6, 2.0 + 1e-6, 1.999, 0.999):
        edges.append((c_lat + np.degrees(r * c_hw / orc.EARTH_RADIUS_KM), c_lon))
    edges.append((c_lat, c_lon))
    e_lat = np.array([e[0] for e in edges])
    e_lon = np.array([e[1] for e in edges])
    e_hw = np.full(len(edges), c_hw)
    sets.append(("seeded", np.concatenate([lat, e_lat]), np.concatenate([lon, e_lon]), np.concatenate([hw, e_hw])))
    # a dense cluster: many pairs inside 2 x halfwidth, many co-located
    cl_lat = np.round(rng.uniform(40, 44, 120), 1)
    cl_lon = np.round(rng.uniform(250, 255, 120), 1)
    sets.append(("cluster", cl_lat, cl_lon, rng.uniform(30, 400, 120)))
    return sets


@pytest.mark.parametrize("which", range(len(GC_GOLDENS) + 2))
def test_vector_obs_taper_matches_the_haversine_loop(which):
    name, lat, lon, hw = _taper_sets()[which]
    worst, n_diff = 0.0, 0
    for k in range(len(lat)):
        a = orc.localize_obs(lat, lon, lat[k], lon[k], hw[k])
        b = orc.localize_obs_vec(lat, lon, lat[k], lon[k], hw[k])
        assert a.shape == b.shape
        d = np.abs(a - b)
        worst = max(worst, float(d.max()))
        n_diff += int((d != 0).sum())
        assert d.max() <= 1e-14, "%s ob %d: vector taper off by %.3e" % (name, k, d.max())
        flip = (a == 0) != (b == 0)
        assert np.all(np.abs(np.where(flip, a + b, 0.0)) <= 1e-30), "%s ob %d: zero vs non-zero taper" % (name, k)
        assert a[k] == 1.0 and b[k] == 1.0          # an ob against itself
    if name == "seeded":        # the edges land where they should
        n = len(lat)
        rs = orc.localize_obs_vec(lat, lon, lat[n - 1], lon[n - 1], hw[n - 1])[n - 9:n - 1]
        assert rs[0] > 0 and rs[1] > 0 and rs[3] == 0 and rs[5] == 0 and rs[6] > 0
        d0 = orc.localize_obs_vec(lat, lon, lat[0], lon[0], 3000.0)[150]
        assert d0 == 1.0                            # zero distance
    print("%s: %d obs, max |vector - loop| %.3e in %d elements" % (name, len(lat), worst, n_diff))


@pytest.mark.parametrize("name", GC_GOLDENS)
def test_vector_taper_oracle_matches_reference(name):
    bit, _ = _check_oracle_against_reference(load_golden(name), obs_taper="vector")
    print("%s (vector obs taper) bit-identical to reference: %s" % (name, bit))


# ---------------------------------------------------------------------------
# G12: the reference's Gaspari-Cohn update 2 500 obs deep (~40 Phase-A block hand-overs)
# ---------------------------------------------------------------------------
@pytest.mark.slow
def test_oracle_matches_reference_g12_loop_taper():
    """The bit-for-bit oracle (one haversine call per ob pair, about a minute) on G12."""
    from _g12 import load_g12
    bit, _ = _check_oracle_against_reference(load_g12())
    print("G12 bit-identical to reference: %s" % bit)


def test_oracle_matches_reference_g12_vector_taper():
    """The vector-taper oracle on G12, and the fixture's design margin: no assimilated ob's variance falls within a
    factor 2e-3 of its value at its 64-ob block's start, so the Phase-A leaders are not expected to give up on it."""
    from _g12 import load_g12
    from _phase_a_guard import GuardProbe, SAFE
    g = load_g12()
    N = int(np.prod(g["shape"][:-1]))
    probe = GuardProbe(N, g["ob_assim"])
    bit, diag = _check_oracle_against_reference(g, obs_taper="vector", step_hook=probe)
    np.testing.assert_array_equal(probe.var_step, diag["prior_var"])
    ratio = probe.min_ratio()
    print("G12 (vector obs taper) bit-identical to reference: %s; Phase-A guard min ratio %.3e" % (bit, ratio))
    assert ratio >= SAFE
    # what the fixture was built to hold
    P = len(g["ob_value"])
    assert P >= 2400 and g["assimilated"].sum() < P and g["assimilated"].sum() > 0.9 * P
    w = orc.localize_obs_vec(g["ob_lat"], g["ob_lon"], g["ob_lat"][777], g["ob_lon"][777], g["ob_radius"][777])
    assert (w != 0).sum() == 1


# ---------------------------------------------------------------------------
# the Phase-A guard predictor (tests/_phase_a_guard.py) on cases whose outcome the GPU tests pin
# ---------------------------------------------------------------------------
def test_guard_predictor_windows_and_blocks():
    from _phase_a_guard import window_starts, GuardProbe
    assert window_starts(10000, 100) == [0]
    assert window_starts(16384, 0) == [0]
    assert window_starts(20000, 0) == [0, 16384]
    assert window_starts(17000, 100) == [0, 16184]        # test_a_window_that_gives_up_is_redone...: second window at 16 184
    p = GuardProbe(5, np.ones(20000, dtype=bool))
    assert sorted(p.block_end)[:3] == [0, 64, 128] and 16384 in p.block_end
    assert p.block_end[16320] == 16384 and p.block_end[19968] == 20000


def test_guard_predictor_on_the_tripping_case_and_the_goldens():
    """Near-exact repeated obs (test_gpu_parity.py::test_gram_leader_cancellation_guard_falls_back) fall far below the
    threshold; the goldens' obs stay far above it."""
    from _phase_a_guard import obs_block_min_ratio, expected_kind
    rng = np.random.default_rng(77)
    X = rng.standard_normal((300, 1)) + 3.0 * rng.standard_normal((300, 24))
    HX = X[rng.choice(300, 90, replace=False)]
    HX[1:40] = HX[0] + 1e-4 * np.random.default_rng(3).standard_normal((39, 24))
    err = np.full(90, 1.0)
    err[:40] = 1e-8
    val = HX.mean(axis=1)
    r, _ = obs_block_min_ratio(HX, val, err, np.ones(90, dtype=bool))
    assert expected_kind(r, 24) == 1, r
    for name in GC_GOLDENS + ["G1", "G4", "G7"]:
        g = load_golden(name)
        nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
        loc = dict(ob_lat=g["ob_lat"], ob_lon=g["ob_lon"], ob_halfwidth=g["ob_radius"]) if g["loc"] == "GC" else {}
        r, d = obs_block_min_ratio(g["HX"], g["ob_value"], g["ob_error"], g["ob_assim"], **loc)
        _close(d["prior_var"], g["prior_var"], name + " prior_var (obs block alone)")
        print("%s: Phase-A guard min ratio %.3e" % (name, r))
        assert expected_kind(r, M) == 4, (name, r)
