"""The forward operator on the device (efa_interp_stencils, efa_forward_interp_dev) at its edges: ob counts around the 256-lane
workgroup of k_interp_weights, grids of fewer than 4 points, of 255 / 256 / 257 points and beyond k_grid_trig's 524 288-thread cap,
k_forward_cols past its cap, duplicate grid points, the 1 km rule at its boundary, both longitude frames, columns at the poles,
the time axis' ends, every ob_status, and column shards.

Yardsticks: EnsembleState.interp_stencil (pinned to the reference by fixtures G9 / G10) for the four points and the time weights,
the oracle's haversine for the space weights of the points the device chose, a NumPy gather for HX.  The reference's
pseudo-distance leaves near-ties open (tests/test_gpu_api.py::test_nearest_four_on_a_global_grid_with_mirror_ties), so the points
are compared as that test does: the same pseudo-distances in the same order, and the same points where the five nearest are
separated by more than 1e-9 relative.  Weights and HX are held to test_gpu_parity's bound (1e-10).
"""
import numpy as np
import pytest

from oracle import ensrf_oracle as orc
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu


def _ctx():
    from efa_xray_amd import _lib
    return _lib.get_context(0)


def _state(lat, lon, valids, nvar=1, M=1):
    """A state of zeros on the grid: the host yardstick needs only its coordinates."""
    from efa_xray_amd import EnsembleState
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    ny, nx = lat.shape if lat.ndim == 2 else (lat.size, lat.size)
    return EnsembleState.from_array(np.zeros((nvar, len(valids), ny, nx, M)), lat, lon, validtime=np.asarray(valids, dtype=np.float64))


def _pseudo(glat, glon, lat, lon):
    return np.hypot(np.sin(np.radians(glat)) - np.sin(np.radians(lat)), np.cos(np.radians(glon)) - np.cos(np.radians(lon))).reshape(-1)


def _space_weights(glat, glon, cols, lat, lon):
    """ensemble.py:178-200 on the given points, in their order (oracle.interp_space_weights' statements)."""
    d = np.array([orc.haversine((glat[c], glon[c]), (lat, lon)) for c in cols])
    if (d < 1.0).sum() > 0:
        w = np.zeros(d.shape)
        w[d.argmin()] = 1.0
        return w, d
    w = 1.0 / d
    return w / w.sum(), d


def _check_stencils(what, lat2, lon2, valids, nvar, ob_var, ob_time, ob_lat, ob_lon, idx, wts, st):
    """Every ob's stencil against the yardsticks; returns how many obs had their four points compared as a set."""
    state = _state(lat2, lon2, valids, nvar)
    names = state.vars()
    nt = len(valids)
    glat, glon = np.asarray(lat2, float).reshape(-1), np.asarray(lon2, float).reshape(-1)
    ncol = glat.size
    npt = min(4, ncol)
    n_set = 0
    assert not st.any(), (what, st.nonzero()[0][:5])
    for k in range(len(ob_lat)):
        d = _pseudo(glat, glon, ob_lat[k], ob_lon[k])
        order = np.argsort(d, kind="stable")
        ref = order[:npt]
        rows, w = state.interp_stencil(names[ob_var[k]], ob_time[k], ob_lat[k], ob_lon[k])
        tw = np.zeros(nt)
        np.add.at(tw, (rows // ncol) % nt, w)
        slots = np.nonzero(tw)[0]
        assert len(slots) in (1, 2), (what, k)
        # layout: entries 0-3 the earlier valid time, 4-7 the later one or the exact match; no time slot of weight 0
        used = idx[k] >= 0
        assert np.all(wts[k][~used] == 0.0) and np.all(wts[k][used] >= 0.0), (what, k)
        assert all(wts[k][4 * s:4 * s + 4].sum() > 0 for s in (0, 1) if used[4 * s]), (what, k)
        want_used = np.zeros(8, bool)
        want_used[4:4 + npt] = True
        if len(slots) == 2:
            want_used[:npt] = True
        assert np.array_equal(used, want_used), "%s ob %d: stencil layout %r" % (what, k, idx[k])
        for s, it in zip((1,) if len(slots) == 1 else (0, 1), slots):
            e = idx[k][4 * s:4 * s + npt]
            assert np.all(e // ncol == ob_var[k] * nt + it), "%s ob %d: variable / time of slot %d" % (what, k, s)
            cols = e % ncol
            assert len(set(cols.tolist())) == npt, "%s ob %d: a point twice" % (what, k)
            # the same pseudo-distances in the same order; the same points where there is no near-tie
            assert np.allclose(d[cols], d[ref], rtol=1e-11, atol=1e-15), "%s ob %d: not the nearest points" % (what, k)
            d5 = d[order[:npt + 1]]
            if np.all(np.diff(d5) > 1e-9 * d5[1:]):
                assert cols.tolist() == ref.tolist(), "%s ob %d: points %r, expected %r" % (what, k, cols, ref)
                n_set += int(s == 1)        # (slot 1 exists for every ob: counts each ob once)
            for a in range(npt - 1):                     # identical grid points tie on any libm: the lower flat index first
                if glat[cols[a]] == glat[cols[a + 1]] and glon[cols[a]] == glon[cols[a + 1]]:
                    assert cols[a] < cols[a + 1], "%s ob %d: tie not to the lower index" % (what, k)
            sw, _ = _space_weights(glat, glon, cols, ob_lat[k], ob_lon[k])
            assert_parity(wts[k][4 * s:4 * s + npt], tw[it] * sw, "%s ob %d slot %d weights" % (what, k, s))
        assert abs(wts[k].sum() - 1.0) < 1e-14, (what, k)
    return n_set


def _stencils(ctx, lat2, lon2, valids, nvar, ob_var, ob_time, ob_lat, ob_lon):
    lat2 = np.asarray(lat2, float)
    ny, nx = lat2.shape
    return ctx.interp_stencils(nvar, len(valids), ny, nx, lat2, lon2, valids, ob_var, ob_time, ob_lat, ob_lon)


def _check_hx(what, ctx, idx, wts, n_lead, ncol, M, seed=0):
    """efa_forward_interp_dev on a random state, unsharded, against a NumPy gather over the same stencil; returns (X, HX)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n_lead * ncol, M)) + 3.0 * rng.standard_normal((n_lead * ncol, 1))
    P = idx.shape[0]
    ref = np.zeros((P, M))
    for e in range(8):
        ok = idx[:, e] >= 0
        ref[ok] += wts[ok, e][:, None] * X[idx[ok, e]]
    HX = ctx.to_device(np.full((P, M), np.nan))
    ctx.forward_interp(ncol, 0, ncol, n_lead, M, ctx.to_device(X), HX)
    got = HX.download()
    assert_parity(got, ref, what + " HX")
    return X, got


def _grid(ny=14, nx=18):
    return np.meshgrid(np.linspace(30, 50, ny), np.linspace(230, 262, nx), indexing="ij")


VALIDS = np.array([0.0, 3600.0, 7200.0])


@pytest.mark.parametrize("P", [1, 255, 256, 257, 600])
def test_ob_counts_around_the_workgroup_of_k_interp_weights(P):
    ctx = _ctx()
    lat2, lon2 = _grid()
    rng = np.random.default_rng(P)
    ob_var = rng.integers(0, 2, P)
    ob_time = rng.choice([0.0, 1800.0, 3600.0, 5000.0, 7200.0], P)
    ob_lat, ob_lon = rng.uniform(31, 49, P), rng.uniform(231, 261, P)
    idx, wts, st = _stencils(ctx, lat2, lon2, VALIDS, 2, ob_var, ob_time, ob_lat, ob_lon)
    n = _check_stencils("P=%d" % P, lat2, lon2, VALIDS, 2, ob_var, ob_time, ob_lat, ob_lon, idx, wts, st)
    assert n >= P // 2
    _check_hx("P=%d" % P, ctx, idx, wts, 2 * 3, lat2.size, 5)


@pytest.mark.parametrize("n_grid", [1, 2, 3, 4, 5, 255, 256, 257])
def test_small_and_workgroup_sized_grids(n_grid):
    """Fewer than 4 points: n_grid entries per time slot, weights normalised over them; threads without a candidate must not
    win.  255 / 256 / 257 points: the last thread of k_nearest4 with no, one and two candidates."""
    ctx = _ctx()
    rng = np.random.default_rng(100 + n_grid)
    lat2, lon2 = rng.uniform(30, 50, (1, n_grid)), rng.uniform(230, 262, (1, n_grid))
    P = 12
    ob_var = np.zeros(P, int)
    ob_time = rng.choice([0.0, 1800.0, 7200.0], P)
    ob_lat, ob_lon = rng.uniform(31, 49, P), rng.uniform(231, 261, P)
    ob_lat[0], ob_lon[0] = lat2[0, n_grid - 1] + 0.3, lon2[0, n_grid - 1] + 0.3       # nearest: the last grid point
    idx, wts, st = _stencils(ctx, lat2, lon2, VALIDS, 1, ob_var, ob_time, ob_lat, ob_lon)
    _check_stencils("n_grid=%d" % n_grid, lat2, lon2, VALIDS, 1, ob_var, ob_time, ob_lat, ob_lon, idx, wts, st)
    npt = min(4, n_grid)
    assert np.all((idx >= 0).sum(axis=1) == npt * np.where(ob_time == 1800.0, 2, 1))
    assert np.all(np.abs(wts.sum(axis=1) - 1.0) < 1e-14) and np.all(wts >= 0.0)
    assert np.all(idx < 3 * n_grid)
    _check_hx("n_grid=%d" % n_grid, ctx, idx, wts, 3, n_grid, 3)


def test_grid_beyond_the_cap_of_k_grid_trig():
    """2 x 524 288 + 53 grid points: three trips of k_grid_trig's grid-stride loop, the last one ragged."""
    ctx = _ctx()
    n = 2 * 524288 + 53
    rng = np.random.default_rng(7)
    lat2, lon2 = rng.uniform(-60, 60, (1, n)), rng.uniform(5, 175, (1, n))
    P = 8
    ob_var = np.zeros(P, int)
    ob_time = np.zeros(P)
    at = np.array([0, 524287, 524288, 2 * 524288 - 1, 2 * 524288, n - 1, n - 30, 700000])     # every trip, first and last point
    ob_lat, ob_lon = lat2[0, at] + 0.02, lon2[0, at] + 0.02
    idx, wts, st = _stencils(ctx, lat2, lon2, [0.0], 1, ob_var, ob_time, ob_lat, ob_lon)
    _check_stencils("big grid", lat2, lon2, [0.0], 1, ob_var, ob_time, ob_lat, ob_lon, idx, wts, st)
    assert np.any(idx >= 2 * 524288)
    _check_hx("big grid", ctx, idx, wts, 1, n, 2)


def test_forward_cols_past_its_cap():
    """P = 4100 obs x M = 256 members: more than twice the 524 288 threads of k_forward_cols, a ragged third trip."""
    ctx = _ctx()
    lat2, lon2 = _grid(6, 7)
    P = 4100
    assert P * 256 > 2 * 524288
    rng = np.random.default_rng(9)
    ob_var = rng.integers(0, 2, P)
    ob_time = rng.uniform(0.0, 7200.0, P)
    ob_lat, ob_lon = rng.uniform(31, 49, P), rng.uniform(231, 261, P)
    idx, wts, st = _stencils(ctx, lat2, lon2, VALIDS, 2, ob_var, ob_time, ob_lat, ob_lon)
    assert not st.any() and np.all((idx >= 0).sum(axis=1) == 8)
    X, HX = _check_hx("forward cols past the cap", ctx, idx, wts, 6, lat2.size, 256)
    assert np.all(np.isfinite(HX)) and np.all(np.abs(HX).max(axis=1) > 0)


def test_duplicate_grid_points_tie_to_the_lower_index():
    ctx = _ctx()
    lat2, lon2 = _grid(5, 6)
    lat2, lon2 = lat2.copy(), lon2.copy()
    lat2[3, 2], lon2[3, 2] = lat2[1, 4], lon2[1, 4]          # flat 20 duplicates flat 10
    lat2[4, 5], lon2[4, 5] = lat2[1, 4], lon2[1, 4]          # and so does flat 29
    ob_lat, ob_lon = np.array([lat2[1, 4] + 0.5, 41.0]), np.array([lon2[1, 4] + 0.7, 250.0])
    idx, wts, st = _stencils(ctx, lat2, lon2, [0.0], 1, [0, 0], [0.0, 0.0], ob_lat, ob_lon)
    _check_stencils("duplicates", lat2, lon2, [0.0], 1, [0, 0], [0.0, 0.0], ob_lat, ob_lon, idx, wts, st)
    assert idx[0][4:7].tolist() == [10, 20, 29]
    assert_parity(wts[0][4:7], np.full(3, wts[0][4]), "equal distances, equal weights")


def test_one_km_rule_at_its_boundary():
    """An ob 0, 0.999 and 1.001 km from a grid point (along its meridian, where the distance is exact to rounding), and an ob
    within 1 km of two points: the nearer one takes weight 1."""
    ctx = _ctx()
    lat2, lon2 = _grid(5, 6)
    lat2, lon2 = lat2.copy(), lon2.copy()
    km = np.degrees(1.0 / orc.EARTH_RADIUS_KM)
    lat2[2, 4], lon2[2, 4] = lat2[2, 3] + 1.2 * km, lon2[2, 3]           # a second point 1.2 km north of (2, 3)
    base = (lat2[1, 1], lon2[1, 1])
    ob_lat = np.array([base[0], base[0] + 0.999 * km, base[0] + 1.001 * km, lat2[2, 3] + 0.5 * km, lat2[2, 3] + 0.7 * km])
    ob_lon = np.array([base[1], base[1], base[1], lon2[2, 3], lon2[2, 3]])
    P = len(ob_lat)
    idx, wts, st = _stencils(ctx, lat2, lon2, [0.0], 1, np.zeros(P, int), np.zeros(P), ob_lat, ob_lon)
    _check_stencils("1 km rule", lat2, lon2, [0.0], 1, np.zeros(P, int), np.zeros(P), ob_lat, ob_lon, idx, wts, st)
    flat = lambda y, x: y * 6 + x

    def only(k):
        nz = wts[k] != 0.0
        assert nz.sum() == 1 and wts[k][nz][0] == 1.0, (k, idx[k], wts[k])
        return int(idx[k][nz][0])

    assert only(0) == flat(1, 1) and only(1) == flat(1, 1)               # 0 km and 0.999 km: that point alone
    assert (wts[2] != 0.0).sum() == 4 and 0.99 < wts[2].max() < 1.0      # 1.001 km: inverse-distance weights
    assert only(3) == flat(2, 3)                                         # 0.5 km from (2, 3), 0.7 km from the point north of it
    assert only(4) == flat(2, 4)                                         # 0.7 km and 0.5 km


@pytest.mark.parametrize("grid_frame", ["-180..180", "0..360"])
def test_longitude_frames(grid_frame):
    """A grid in -180..180 with obs in 0..360 and the reverse: the pseudo-distance and the haversine take either."""
    ctx = _ctx()
    rng = np.random.default_rng(3)
    lat2, lon2 = np.meshgrid(np.linspace(-40, 50, 10), np.linspace(100, 250, 16), indexing="ij")
    P = 40
    ob_lat, ob_lon = rng.uniform(-38, 48, P), rng.uniform(102, 248, P)
    ob_lon[:4] = [179.9, 180.0, 180.1, 181.0]
    if grid_frame == "-180..180":
        lon2 = np.where(lon2 > 180, lon2 - 360, lon2)
    else:
        ob_lon = np.where(ob_lon > 180, ob_lon - 360, ob_lon)
    idx, wts, st = _stencils(ctx, lat2, lon2, [0.0], 1, np.zeros(P, int), np.zeros(P), ob_lat, ob_lon)
    _check_stencils(grid_frame, lat2, lon2, [0.0], 1, np.zeros(P, int), np.zeros(P), ob_lat, ob_lon, idx, wts, st)
    # the frame changes no weight beyond rounding: the other frame's stencil, point by point
    lon_other = np.where(lon2 < 0, lon2 + 360, lon2) if grid_frame == "-180..180" else lon2
    ob_other = np.where(ob_lon < 0, ob_lon + 360, ob_lon)
    idx2, wts2, st2 = _stencils(ctx, lat2, lon_other, [0.0], 1, np.zeros(P, int), np.zeros(P), ob_lat, ob_other)
    for k in range(P):
        d = _pseudo(lat2, lon_other, ob_lat[k], ob_other[k])
        d5 = np.sort(d)[:5]
        if np.all(np.diff(d5) > 1e-9 * d5[1:]):
            assert idx[k].tolist() == idx2[k].tolist(), k
            assert_parity(wts[k], wts2[k], "ob %d across frames" % k)


def test_columns_at_the_poles():
    ctx = _ctx()
    lat2, lon2 = np.meshgrid(np.array([-90.0, -88.0, -60.0, 0.0, 60.0, 88.0, 90.0]), np.linspace(0, 315, 8), indexing="ij")
    rng = np.random.default_rng(4)
    P = 30
    ob_lat, ob_lon = rng.uniform(-89.9, 89.9, P), rng.uniform(0, 359, P)
    ob_lat[:6] = [90.0, -90.0, 89.995, -89.995, 89.0, -89.0]
    ob_lon[:6] = [10.0, 200.0, 45.0, 90.0, 0.0, 180.0]
    idx, wts, st = _stencils(ctx, lat2, lon2, [0.0], 1, np.zeros(P, int), np.zeros(P), ob_lat, ob_lon)
    _check_stencils("poles", lat2, lon2, [0.0], 1, np.zeros(P, int), np.zeros(P), ob_lat, ob_lon, idx, wts, st)
    for k, row in ((0, 6), (1, 0), (2, 6), (3, 0)):        # at, or within 1 km of, a pole: one polar column with weight 1
        nz = wts[k] != 0.0
        assert nz.sum() == 1 and wts[k][nz][0] == 1.0 and idx[k][nz][0] // 8 == row, (k, idx[k], wts[k])
    _check_hx("poles", ctx, idx, wts, 1, lat2.size, 4)


@pytest.mark.parametrize("valids", [[5.0], [0.0, 3600.0, 7200.0], [-7200.0, -7000.0, -100.0, -50.0, 1.5, 900.0]],
                         ids=["nt1", "regular", "irregular-negative"])
def test_time_axis(valids):
    """nt = 1; t on the first, an interior and the last valid time (one slot of weight 1, no entry of weight 0); between
    irregularly spaced times on an axis that starts negative; the weights as coded (ensemble.py:218-224)."""
    ctx = _ctx()
    valids = np.array(valids)
    nt = len(valids)
    lat2, lon2 = _grid(5, 6)
    rng = np.random.default_rng(nt)
    times = list(valids)
    for a, b in zip(valids[:-1], valids[1:]):
        times += [a + 0.25 * (b - a), a + 0.5 * (b - a), np.nextafter(a, b), np.nextafter(b, a)]
    P = len(times)
    ob_time = np.array(times)
    ob_lat, ob_lon = rng.uniform(31, 49, P), rng.uniform(231, 261, P)
    idx, wts, st = _stencils(ctx, lat2, lon2, valids, 2, np.ones(P, int), ob_time, ob_lat, ob_lon)
    _check_stencils("time", lat2, lon2, valids, 2, np.ones(P, int), ob_time, ob_lat, ob_lon, idx, wts, st)
    for k in range(nt):                                   # on a valid time: entries 4-7 only, that time, weights sum to 1
        assert np.all(idx[k][:4] == -1) and np.all(idx[k][4:] // lat2.size == nt + k)
    for k in range(nt, P):                                # between two: as coded, the later time's weight is |t - t_later| / dt
        j = int(np.searchsorted(valids, ob_time[k]))
        later = abs(ob_time[k] - valids[j]) / abs(valids[j] - valids[j - 1])
        if later != 0.0 and later != 1.0:
            assert abs(wts[k][4:].sum() - later) <= 1e-15 and abs(wts[k][:4].sum() - (1.0 - later)) <= 1e-15
            assert np.all(idx[k][:4] // lat2.size == nt + j - 1) and np.all(idx[k][4:] // lat2.size == nt + j)
    _check_hx("time", ctx, idx, wts, 2 * nt, lat2.size, 3)


def test_every_ob_status_and_its_neighbours():
    """Status 1: t before the first valid time, after the last, NaN.  Status 3: var -1 and var = nvar.  Status 2: an ob with NaN
    lat.  A non-zero status leaves idx -1, wts 0 and an HX row of exactly 0.0; the obs beside it are as in a call without it."""
    ctx = _ctx()
    lat2, lon2 = _grid()
    rng = np.random.default_rng(21)
    P = 300                                               # two workgroups of k_interp_weights
    ob_var = rng.integers(0, 2, P)
    ob_time = rng.uniform(0.0, 7200.0, P)
    ob_lat, ob_lon = rng.uniform(31, 49, P), rng.uniform(231, 261, P)
    good = _stencils(ctx, lat2, lon2, VALIDS, 2, ob_var, ob_time, ob_lat, ob_lon)
    bad = {3: ("time", -1e-9, 1), 17: ("time", 7200.0 + 1e-9, 1), 40: ("time", np.nan, 1), 41: ("var", -1, 3), 255: ("var", 2, 3),
           256: ("lat", np.nan, 2), 299: ("time", np.nextafter(0.0, -1.0), 1)}
    v2, t2, la2 = ob_var.copy(), ob_time.copy(), ob_lat.copy()
    for k, (what, value, _) in bad.items():
        {"time": t2, "var": v2, "lat": la2}[what][k] = value
    idx, wts, st = _stencils(ctx, lat2, lon2, VALIDS, 2, v2, t2, la2, ob_lon)
    want = np.zeros(P, np.uint8)
    for k, (_, _, code) in bad.items():
        want[k] = code
    assert np.array_equal(st, want), (st.nonzero()[0], st[st != 0])
    ok = want == 0
    assert np.all(idx[~ok] == -1) and np.all(wts[~ok] == 0.0)
    assert np.array_equal(idx[ok], good[0][ok]) and np.array_equal(wts[ok], good[1][ok])
    _, HX = _check_hx("status", ctx, idx, wts, 6, lat2.size, 4)
    assert np.all(HX[~ok] == 0.0) and not np.any(np.signbit(HX[~ok]))
    assert np.all(np.abs(HX[ok]).max(axis=1) > 0)


def test_status_2_for_one_dimensional_lat_lon():
    """1-D lat/lon with ny != nx: the reference indexes y and x with the same number (ensemble.py:186-190), so a nearest index
    >= min(ny, nx) is out of range."""
    ctx = _ctx()
    ny, nx = 5, 9
    lat1, lon1 = np.linspace(30, 46, nx), np.linspace(230, 262, nx)
    ob_lat = np.array([30.5, 45.5, 33.0, 38.2])            # nearest four of ob 1: indices 5..8; of ob 3: 2..5
    ob_lon = np.array([231.0, 261.0, 236.0, 246.4])
    idx, wts, st = ctx.interp_stencils(1, 1, ny, nx, lat1, lon1, [0.0], np.zeros(4, int), np.zeros(4), ob_lat, ob_lon)
    assert st.tolist() == [0, 2, 0, 2], st
    assert np.all(idx[[1, 3]] == -1) and np.all(wts[[1, 3]] == 0.0)
    for k in (0, 2):
        cols = idx[k][4:]
        assert np.all(cols % nx == cols // nx) and np.all(cols // nx < ny) and abs(wts[k].sum() - 1.0) < 1e-14


@pytest.mark.parametrize("case", ["status 1", "status 2 (NaN lat)", "status 2 (1-D lat/lon)", "unknown variable"])
def test_update_names_the_first_ob_that_cannot_be_interpolated(case):
    """EnSRF.update() raises ValueError naming the first such ob.  A variable the state does not have never reaches the device
    (status 3 is the C ABI's own check): the Python API raises KeyError for it, as the reference's state[obtype] does."""
    from efa_xray_amd import EnSRF, EnsembleState, Observation
    rng = np.random.default_rng(2)
    one_d = case == "status 2 (1-D lat/lon)"
    ny, nx, M = (5, 9, 6)
    if one_d:
        lat, lon = np.linspace(30, 46, nx), np.linspace(230, 262, nx)
    else:
        lat, lon = np.meshgrid(np.linspace(30, 46, ny), np.linspace(230, 262, nx), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((1, 2, ny, nx, M)), lat, lon, validtime=np.array([0.0, 3600.0]))
    obs = [Observation(value=0.1 * k, obtype="var0", time=1800.0, error=1.0, lat=31.0 + 0.1 * k, lon=231.0 + 0.1 * k,
                       assimilate_this=True, localize_radius=1000.0) for k in range(8)]
    for k in (5, 7):
        if case == "status 1":
            obs[k].time = 3600.5
        elif case == "status 2 (NaN lat)":
            obs[k].lat = float("nan")
        elif one_d:
            obs[k].lat, obs[k].lon = 45.5, 261.0
        else:
            obs[k].obtype = "nope"
    with pytest.raises(KeyError if case == "unknown variable" else ValueError) as err:
        EnSRF(state, obs, verbose=False, loc="GC").update()
    if case != "unknown variable":
        assert "observation 5 " in str(err.value), str(err.value)


def test_column_shards():
    """An empty shard returns zeros; one-column shards and a ragged three-way split add up to the unsharded HX; a failed or a
    P = 0 efa_interp_stencils leaves nothing to apply (EFA_ERR_INVALID)."""
    from efa_xray_amd import _lib
    ctx = _ctx()
    lat2, lon2 = _grid(7, 9)
    ncol, n_lead, M, P = 63, 6, 5, 70
    rng = np.random.default_rng(5)
    ob_var, ob_time = rng.integers(0, 2, P), rng.uniform(0.0, 7200.0, P)
    ob_lat, ob_lon = rng.uniform(31, 49, P), rng.uniform(231, 261, P)
    idx, wts, st = _stencils(ctx, lat2, lon2, VALIDS, 2, ob_var, ob_time, ob_lat, ob_lon)
    X, full = _check_hx("shards", ctx, idx, wts, n_lead, ncol, M)
    X3 = X.reshape(n_lead, ncol, M)
    HX = ctx.to_device(np.full((P, M), np.nan))

    def shard(lo, hi):
        Xs = ctx.to_device(np.ascontiguousarray(X3[:, lo:hi].reshape(-1, M))) if hi > lo else ctx.to_device(np.zeros((1, M)))
        HX.upload(np.full((P, M), np.nan))
        ctx.forward_interp(ncol, lo, hi, n_lead, M, Xs, HX)
        return HX.download()

    for lo in (0, 17, ncol):
        z = shard(lo, lo)
        assert np.all(z == 0.0) and not np.any(np.signbit(z)), "empty shard [%d, %d)" % (lo, lo)
    acc = shard(0, 20) + shard(20, 21) + shard(21, ncol)          # ragged three-way split, one shard of one column
    assert_parity(acc, full, "three shards")
    acc = np.zeros_like(full)
    for c in range(ncol):                                         # one-column shards
        acc += shard(c, c + 1)
    assert_parity(acc, full, "one-column shards")
    # nothing to apply after a P = 0 call, or after a call that failed
    ctx.interp_stencils(2, 3, 7, 9, lat2, lon2, VALIDS, [], [], [], [])
    with pytest.raises(_lib.EfaError) as e0:
        ctx.forward_interp(ncol, 0, ncol, n_lead, M, ctx.to_device(X), HX)
    assert e0.value.status == _lib.EFA_ERR_INVALID
    _stencils(ctx, lat2, lon2, VALIDS, 2, ob_var, ob_time, ob_lat, ob_lon)
    with pytest.raises(_lib.EfaError) as e1:
        ctx.interp_stencils(2, 3, 7, 9, lat2, lon2, [0.0, 7200.0, 3600.0], ob_var, ob_time, ob_lat, ob_lon)   # not ascending
    assert e1.value.status == _lib.EFA_ERR_INVALID
    with pytest.raises(_lib.EfaError) as e2:
        ctx.forward_interp(ncol, 0, ncol, n_lead, M, ctx.to_device(X), HX)
    assert e2.value.status == _lib.EFA_ERR_INVALID
