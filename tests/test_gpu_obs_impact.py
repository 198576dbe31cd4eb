"""Observation impact (EFSO) on the MI355X: efa_obs_impact_dev against the NumPy helper tests/_efso.py.

Tolerance (derived, not measured): |J_k - ref_k| <= max(1e-9, 4 rows M 2^-53) A_k, A_k the sum of the absolute values of the
rows * M terms of J_k -- the worst-case forward bound of a float64 sum of that many terms in any order (1e-9 at every shape here).
A dropped row, a wrong taper weight or a wrong slab factor shows at 1e-3 A_k or more.  Every parity case also asserts that at least
half of the used obs have A_k > 0 (a zero result cannot pass) and that unused obs come back exactly 0.0."""
import functools

import numpy as np
import pytest

import _efso

pytestmark = pytest.mark.gpu

NY, NX = 13, 11            # 143 columns: the last block of 16 is ragged
Z_ROWS_PER_TRIP = 1024 * 4  # k_impact_z: at most 1024 workgroups of 4 waves, a row per wave and trip (efa_impact.hip kZBlocks)


def _ctx():
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    ctx.set_vertical_localization(None)
    ctx.set_adaptive_inflation(None)
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    return ctx


def _grid():
    glat, glon = np.meshgrid(np.linspace(25, 55, NY), np.linspace(240, 290, NX), indexing="ij")
    return glat.reshape(-1), glon.reshape(-1)


@functools.lru_cache(maxsize=None)
def _case(M, n_lead, P=150, seed=0):
    """Forecast members of mixed magnitude, obs inside and around the grid with half-widths of 300 to 3000 km (some blocks' lists
    exceed 32 and 64 entries, with a ragged last chunk), about 15 % of them unused, ob 3 used but 5000 km from the grid."""
    rng = np.random.default_rng(1000 * seed + 7 * M + n_lead)
    glat, glon = _grid()
    ncol = glat.size
    rows = n_lead * ncol
    Xf = 2.0 * rng.standard_normal((rows, M)) + 5.0 * rng.standard_normal((rows, 1)) + 280.0
    Ya = Xf[rng.choice(rows, P, replace=P > rows)] + 0.1 * rng.standard_normal((P, M))
    v = rng.standard_normal(rows)
    v[rng.random(rows) < 0.1] = 0.0           # rows that are not verified
    c = dict(M=M, n_lead=n_lead, P=P, rows=rows, ncol=ncol, Xf=Xf, Ya=Ya, v=v, glat=glat, glon=glon,
             d=rng.standard_normal(P), r=rng.uniform(0.5, 2.0, P), used=rng.random(P) >= 0.15,
             ob_lat=rng.uniform(22, 58, P), ob_lon=rng.uniform(236, 294, P), hw=rng.uniform(300.0, 3000.0, P))
    if P > 3:
        c["used"][3] = True
        c["ob_lat"][3], c["ob_lon"][3], c["hw"][3] = -10.0, 265.0, 300.0
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _vertical(n_lead, P, seed=0):
    """Slab coordinates 0 .. 3 with one NaN slab; ob 0 without a coordinate, ob 1 without a half-width; every fifth ob with a
    half-width so tight (cut-off 0.04, slabs 0.083 apart) that whole waves of 16 slabs have nothing to do."""
    rng = np.random.default_rng(seed)
    lead = np.linspace(0.0, 3.0, n_lead)
    if n_lead > 1:
        lead[n_lead // 2] = np.nan
    ov = rng.uniform(-0.3, 3.3, P)
    oh = 0.9 * rng.uniform(0.7, 1.3, P)
    oh[::5] = 0.02
    ov[0] = np.nan
    if P > 1:
        oh[1] = np.nan
    return lead, ov, oh


@functools.lru_cache(maxsize=None)
def _reference(M, n_lead, P=150, seed=0, vert=False, loc=True):
    c = _case(M, n_lead, P, seed)
    kw = {}
    if loc:
        kw = dict(grid_lat=c["glat"], grid_lon=c["glon"], ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"], n_lead=n_lead)
    if vert:
        lead, ov, oh = _vertical(n_lead, P, seed)
        kw.update(lead_vert=lead, ob_vert=ov, ob_vert_halfwidth=oh)
    J, A = _efso.efso(c["Xf"], c["Ya"], c["v"], c["d"], c["r"], c["used"], **kw)
    J.setflags(write=False)
    A.setflags(write=False)
    return J, A


def _run(ctx, c, loc=True, vert=None, used=None, cols=None):
    """efa_obs_impact_dev on the case (cols: a column shard [lo, hi)); vert: (lead, ob_vert, ob_vert_halfwidth) or None."""
    from efa_xray_amd import _lib
    ncol, n_lead, M, P = c["ncol"], c["n_lead"], c["M"], c["P"]
    lo, hi = cols if cols is not None else (0, ncol)
    Xf = c["Xf"].reshape(n_lead, ncol, M)[:, lo:hi].reshape(-1, M)
    v = c["v"].reshape(n_lead, ncol)[:, lo:hi].reshape(-1)
    ctx.set_vertical_localization(*vert) if vert is not None else ctx.set_vertical_localization(None)
    try:
        Xd, vd, Yd = ctx.to_device(Xf), ctx.to_device(v), ctx.to_device(c["Ya"])
        used = c["used"] if used is None else used
        if loc:
            J = ctx.obs_impact(Xf.shape[0], M, P, Xd, vd, Yd, c["d"], c["r"], used, _lib.LOC_GC, c["ob_lat"], c["ob_lon"], c["hw"],
                               c["glat"][lo:hi], c["glon"][lo:hi], n_lead)
        else:
            J = ctx.obs_impact(Xf.shape[0], M, P, Xd, vd, Yd, c["d"], c["r"], used)
        assert np.array_equal(Xd.download(), Xf) and np.array_equal(Yd.download(), c["Ya"])   # read only
        return J
    finally:
        ctx.set_vertical_localization(None)


def _assert_parity(what, J, ref, c, used=None):
    Jr, A = ref
    used = c["used"] if used is None else used
    tol = _efso.tolerance(c["rows"], c["M"])
    assert tol == 1e-9
    err = np.abs(J - Jr)
    worst = float(np.max(err[used] / np.maximum(A[used], 1e-300))) if used.any() else 0.0
    print("%s: max |J - ref| / A = %.3e (tolerance %.1e), max A / |J| = %.3g, used %d of %d, A > 0 on %d"
          % (what, worst, tol, float(np.max(A[used] / np.maximum(np.abs(Jr[used]), 1e-300))) if used.any() else 0.0,
             int(used.sum()), used.size, int(np.count_nonzero(A[used]))))
    assert np.all(np.isfinite(J))
    assert np.all(err <= tol * A), (what, worst)
    assert np.count_nonzero(A[used]) * 2 >= used.sum(), what
    assert np.all(J[~used] == 0.0), what


@pytest.mark.parametrize("n_lead", [1, 2, 3, 5, 9, 16, 17, 37])
@pytest.mark.parametrize("M", [2, 3, 7, 50, 80, 100, 104, 136, 137, 256])
def test_gc_ragged_shapes(M, n_lead):
    """Every lg_cols layout of a group of slabs (1, 2, 3, 5, 9 slabs), the 16-slab boundary and more than one group (17, 37);
    M odd, even and unpadded, both occupancies of the row-per-lane form (<= 96, 100 / 104) and the pieces above 104."""
    ctx = _ctx()
    c = _case(M, n_lead)
    J = _run(ctx, c)
    _assert_parity("GC M=%d n_lead=%d" % (M, n_lead), J, _reference(M, n_lead), c)
    assert J[3] == 0.0 and c["used"][3]            # used, but 5000 km from every column: exactly 0
    assert ctx.get_option("impact_us") > 0


@pytest.mark.parametrize("M", [7, 80, 137])
def test_gc_single_ob_and_every_ob_unused(M):
    ctx = _ctx()
    c = _case(M, 5, P=1, seed=1)
    used = np.ones(1, dtype=bool)
    ref = _efso.efso(c["Xf"], c["Ya"], c["v"], c["d"], c["r"], used, grid_lat=c["glat"], grid_lon=c["glon"], ob_lat=c["ob_lat"],
                     ob_lon=c["ob_lon"], ob_halfwidth=c["hw"], n_lead=5)
    _assert_parity("GC P=1 M=%d" % M, _run(ctx, c, used=used), ref, c, used)
    c = _case(M, 5)
    J = _run(ctx, c, used=np.zeros(c["P"], dtype=bool))     # status OK, all zeros
    assert J.shape == (c["P"],) and np.all(J == 0.0)
    J = _run(ctx, c, loc=False, used=np.zeros(c["P"], dtype=bool))
    assert np.all(J == 0.0)


@pytest.mark.parametrize("M", [2, 3, 7, 50, 80, 100, 104, 136, 137, 256])
def test_vertical_localisation(M):
    """n_lead = 37 with a NaN slab, an ob without a coordinate, one without a half-width, and half-widths so tight that whole
    waves are skipped."""
    ctx = _ctx()
    c = _case(M, 37)
    vert = _vertical(37, c["P"])
    J = _run(ctx, c, vert=vert)
    ref = _reference(M, 37, vert=True)
    _assert_parity("GC+vertical M=%d" % M, J, ref, c)
    plain = _reference(M, 37)
    assert np.max(np.abs(ref[0] - plain[0]) / np.maximum(plain[1], 1e-300)) > 1e-3     # the factor matters on this case
    assert J[3] == 0.0


def test_vertical_setting_must_match_the_call():
    from efa_xray_amd import _lib
    ctx = _ctx()
    c = _case(7, 5)
    lead, ov, oh = _vertical(5, c["P"])
    for vert, loc in (((lead, ov[:-1], oh[:-1]), True), ((lead[:-1], ov, oh), True), ((lead, ov, oh), False)):
        with pytest.raises(_lib.EfaError) as e:
            _run(ctx, c, loc=loc, vert=vert)
        assert e.value.status == _lib.EFA_ERR_INVALID and "vertical localisation" in str(e.value)
    assert ctx.get_option("impact_us") >= 0


def test_refusals():
    from efa_xray_amd import _lib
    ctx = _ctx()
    c = _case(7, 2)
    P = c["P"]
    k = int(np.nonzero(c["used"])[0][0])

    def call(**over):
        a = dict(rows=c["rows"], M=7, d=c["d"], r=c["r"], hw=c["hw"], n_lead=2)
        a.update(over)
        Xd, vd, Yd = ctx.to_device(c["Xf"]), ctx.to_device(c["v"]), ctx.to_device(c["Ya"])
        return ctx.obs_impact(a["rows"], a["M"], P, Xd, vd, Yd, a["d"], a["r"], c["used"], _lib.LOC_GC, c["ob_lat"], c["ob_lon"],
                              a["hw"], c["glat"], c["glon"], a["n_lead"])

    def spoiled(name, value):
        a = np.array(c[name])
        a[k] = value
        return a

    for over in (dict(M=1), dict(M=257), dict(rows=c["rows"] - 1), dict(n_lead=3), dict(d=spoiled("d", np.inf)),
                 dict(d=spoiled("d", np.nan)), dict(r=spoiled("r", 0.0)), dict(r=spoiled("r", -1.0)), dict(r=spoiled("r", np.nan)),
                 dict(hw=spoiled("hw", np.nan))):
        with pytest.raises(_lib.EfaError) as e:
            call(**over)
        assert e.value.status == _lib.EFA_ERR_INVALID, over
    # the same values on an ob that is not used are ignored
    u = int(np.nonzero(~c["used"])[0][0])
    d, r, hw = np.array(c["d"]), np.array(c["r"]), np.array(c["hw"])
    d[u], r[u], hw[u] = np.nan, -1.0, np.nan
    J = call(d=d, r=r, hw=hw)
    _assert_parity("unused ob with bad values", J, _reference(7, 2), c)


@pytest.mark.parametrize("M", [7, 100, 256])
def test_unlocalised_beyond_the_grid_cap(M):
    """rows = twice what one trip of the capped grid covers plus 53: two whole trips and a ragged third."""
    ctx = _ctx()
    rows = 2 * Z_ROWS_PER_TRIP + 53
    rng = np.random.default_rng(M)
    P = 40
    c = dict(M=M, n_lead=1, ncol=rows, rows=rows, P=P, Xf=2.0 * rng.standard_normal((rows, M)) + 5.0 * rng.standard_normal((rows, 1)),
             v=rng.standard_normal(rows), d=rng.standard_normal(P), r=rng.uniform(0.5, 2.0, P), used=rng.random(P) >= 0.15)
    c["Ya"] = c["Xf"][rng.choice(rows, P, replace=False)] + 0.1 * rng.standard_normal((P, M))
    c["v"][rng.random(rows) < 0.1] = 0.0
    ref = _efso.efso(c["Xf"], c["Ya"], c["v"], c["d"], c["r"], c["used"])
    J = _run(ctx, c, loc=False)
    _assert_parity("unlocalised M=%d rows=%d" % (M, rows), J, ref, c)
    assert np.array_equal(J, _run(ctx, c, loc=False))          # bit for bit


@pytest.mark.parametrize("M,vert", [(80, True), (137, False), (100, False)])
def test_two_calls_agree_bit_for_bit(M, vert):
    ctx = _ctx()
    c = _case(M, 37)
    v = _vertical(37, c["P"]) if vert else None
    a = _run(ctx, c, vert=v)
    b = _run(ctx, c, vert=v)
    assert np.array_equal(a, b)
    assert np.count_nonzero(a) > c["P"] // 2


@pytest.mark.parametrize("M", [50, 137])
def test_column_shards_add_up(M):
    ctx = _ctx()
    c = _case(M, 17)
    vert = _vertical(17, c["P"])
    whole = _run(ctx, c, vert=vert)
    parts = _run(ctx, c, vert=vert, cols=(0, 80)) + _run(ctx, c, vert=vert, cols=(80, c["ncol"]))
    _, A = _reference(M, 17, vert=True)
    worst = float(np.max(np.abs(parts - whole) / np.maximum(A, 1e-300)))
    print("shards M=%d: max |sum of shards - whole| / A = %.3e" % (M, worst))
    assert np.all(np.abs(parts - whole) <= _efso.tolerance(c["rows"], M) * A)
    _assert_parity("shards M=%d" % M, parts, _reference(M, 17, vert=True), c)


def test_a_cycle_after_an_impact_call_returns_the_same_bits():
    """A GC cycle, an impact call with a different obs geometry, the same cycle again: the second cycle's posterior and
    diagnostics are bit for bit those of a context that never made the impact call; gc_active_pairs and phase_a_kind too."""
    from efa_xray_amd import _lib
    glat, glon = _grid()
    ncol, n_lead, M, P = glat.size, 5, 20, 60
    rng = np.random.default_rng(11)
    N = n_lead * ncol
    X = 2.0 * rng.standard_normal((N, M)) + rng.standard_normal((N, 1))
    pick = rng.choice(N, P, replace=False)
    HX = X[pick] + 0.05 * rng.standard_normal((P, M))
    ob = dict(value=HX.mean(axis=1) + rng.standard_normal(P), error=rng.uniform(0.5, 2.0, P), assim=rng.random(P) < 0.9,
              lat=glat[pick % ncol] + rng.uniform(-0.5, 0.5, P), lon=glon[pick % ncol] + rng.uniform(-0.5, 0.5, P),
              hw=rng.uniform(600, 1500, P))
    c = _case(20, 5)

    def cycle(ctx):
        Xd, post, Yp, ym = ctx.to_device(X), ctx.empty((N, M)), ctx.to_device(HX), ctx.empty((P,))
        ctx.form_perts(P, M, Yp, ym, Yp)
        diag = ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, ob["value"], ob["error"], ob["assim"], _lib.LOC_GC, ob["lat"], ob["lon"],
                               ob["hw"], glat, glon, n_lead)
        return post.download(), diag, ctx.get_option("gc_active_pairs"), ctx.get_option("phase_a_kind")

    results = []
    for with_impact in (True, False):
        ctx = _lib.Context(0)
        try:
            first = cycle(ctx)
            if with_impact:
                J = _run(ctx, c)
                _assert_parity("between two cycles", J, _reference(20, 5), c)
            results.append((first, cycle(ctx)))
        finally:
            ctx.close()
    (a1, a2), (b1, b2) = results
    for got, want in ((a1, b1), (a2, b2)):
        assert np.array_equal(got[0], want[0])
        for key in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
            assert np.array_equal(got[1][key], want[1][key], equal_nan=True), key
        assert got[2:] == want[2:]
    assert a2[2] > 0


def test_observation_impact_end_to_end():
    """EnSRF(loc='GC', vert_coord=Z).update() on 2 variables x 3 times x 12 x 14 x 20 members with point obs, then
    observation_impact against the helper fed from NumPy means and ob.estimate."""
    from efa_xray_amd import EnSRF, EnsembleState, Observation, observation_impact
    _ctx()
    rng = np.random.default_rng(3)
    nvar, nt, ny, nx, M, P = 2, 3, 12, 14, 20, 30
    lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(250, 280, nx), indexing="ij")
    truth = rng.standard_normal((nvar, nt, ny, nx))
    arr = truth[..., None] + 0.5 * rng.standard_normal((nvar, nt, ny, nx, 1)) + rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon, validtime=np.array([0.0, 3600.0, 7200.0]))
    names = state.vars()
    Z = np.array([[0.0, 0.5, 1.0], [2.0, np.nan, 3.0]])
    obs = []
    for k in range(P):
        ob = Observation(value=float(rng.standard_normal()), obtype=names[k % nvar], time=float([0.0, 1800.0, 3600.0][k % 3]),
                         error=float(rng.uniform(0.5, 1.5)), lat=float(rng.uniform(31, 49)), lon=float(rng.uniform(251, 279)),
                         assimilate_this=(k % 6 != 1), localize_radius=float(rng.uniform(500, 1500)))
        if k % 4:
            ob.vert, ob.vert_localize_radius = float(rng.uniform(0, 3)), 1.2
        obs.append(ob)
    post, obs_out = EnSRF(state, obs, loc="GC", vert_coord=Z, verbose=False).update()
    ver = {names[0]: truth[0].copy(), names[1]: truth[1].copy()}
    ver[names[0]][1, 3, 4] = np.nan
    ver[names[1]][2] = np.nan
    norm = {names[0]: 2.0, names[1]: np.linspace(0.5, 1.5, ny).reshape(1, ny, 1)}
    out = observation_impact(state, post, obs_out, ver, norm=norm, loc="GC", vert_coord=Z)

    used = np.array([bool(o.assimilated) for o in obs_out])
    assert used.sum() == sum(k % 6 != 1 for k in range(P))
    v = np.zeros((nvar, nt, ny, nx))
    actual = 0.0
    for iv, n in enumerate(names):
        c = np.broadcast_to(np.asarray(norm[n], dtype=float), (nt, ny, nx))
        eb = state.variables[n].mean(axis=-1) - ver[n]
        ea = post.variables[n].mean(axis=-1) - ver[n]
        ok = ~np.isnan(ver[n])
        v[iv][ok] = (c * (ea + eb))[ok]
        actual += np.sum((c * (ea ** 2 - eb ** 2))[ok])
    Ya = np.array([o.estimate(post) for o in obs_out])
    d = np.array([o.value - np.mean(o.estimate(state)) for o in obs_out])
    ov = np.array([np.nan if getattr(o, "vert", None) is None else o.vert for o in obs_out])
    oh = np.array([np.nan if getattr(o, "vert_localize_radius", None) is None else o.vert_localize_radius for o in obs_out])
    Jr, A = _efso.efso(post.to_vect(), Ya, v.reshape(-1), d, np.array([o.error for o in obs_out]), used, grid_lat=lat.reshape(-1),
                       grid_lon=lon.reshape(-1), ob_lat=[o.lat for o in obs_out], ob_lon=[o.lon for o in obs_out],
                       ob_halfwidth=[o.localize_radius for o in obs_out], n_lead=nvar * nt, lead_vert=Z.reshape(-1), ob_vert=ov,
                       ob_vert_halfwidth=oh)
    J = out["impact"]
    tol = _efso.tolerance(post.nstate(), M)
    worst = float(np.max(np.abs(J - Jr)[used] / A[used]))
    print("end to end: max |J - ref| / A = %.3e, total %.6g, actual %.6g" % (worst, out["total"], out["actual"]))
    assert np.all(np.abs(J - Jr)[used] <= tol * A[used]) and np.count_nonzero(A[used]) * 2 >= used.sum()
    assert np.all(np.isnan(J[~used])) and not np.any(np.isnan(J[used]))
    for k, o in enumerate(obs_out):
        assert (o.impact is None) if not used[k] else (o.impact == J[k])
    assert out["total"] == float(np.sum(J[used])) and np.isclose(out["actual"], actual, rtol=1e-12)
    assert np.isfinite(out["total"]) and np.isfinite(out["actual"])
    from efa_xray_amd import _lib
    # the context's vertical setting is off again: a plain GC call of another P is accepted
    c = _case(7, 2)
    _assert_parity("after observation_impact", _run(_lib.get_context(0), c), _reference(7, 2), c)


def test_observation_impact_unlocalised_with_a_user_defined_operator():
    """loc=False and obs whose `estimate` is their own (a state row plus a member-dependent offset): through the objects."""
    from efa_xray_amd import EnSRF, EnsembleState, Observation, observation_impact
    _ctx()
    rng = np.random.default_rng(4)
    nvar, nt, ny, nx, M, P = 1, 2, 6, 7, 9, 12
    lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(250, 280, nx), indexing="ij")
    truth = rng.standard_normal((nvar, nt, ny, nx))
    state = EnsembleState.from_array(truth[..., None] + rng.standard_normal((nvar, nt, ny, nx, M)), lat, lon)

    class RowOb(Observation):
        def estimate(self, st):
            return st.to_vect()[self.row] + self.offset

    obs = []
    for k in range(P):
        ob = RowOb(value=float(rng.standard_normal()), error=float(rng.uniform(0.5, 1.5)), lat=40.0, lon=260.0,
                   assimilate_this=(k % 5 != 2))
        ob.row, ob.offset = int(rng.integers(state.nstate())), 0.01 * np.arange(M)
        obs.append(ob)
    post, obs_out = EnSRF(state, obs, verbose=False).update()
    name = state.vars()[0]
    out = observation_impact(state, post, obs_out, {name: truth[0]})
    used = np.array([bool(o.assimilated) for o in obs_out])
    eb = state.variables[name].mean(axis=-1) - truth[0]
    ea = post.variables[name].mean(axis=-1) - truth[0]
    Jr, A = _efso.efso(post.to_vect(), np.array([o.estimate(post) for o in obs_out]), (ea + eb).reshape(-1),
                       np.array([o.value - np.mean(o.estimate(state)) for o in obs_out]), np.array([o.error for o in obs_out]), used)
    J = out["impact"]
    assert used.sum() == sum(k % 5 != 2 for k in range(P)) and np.all(A[used] > 0)
    assert np.all(np.abs(J - Jr)[used] <= _efso.tolerance(state.nstate(), M) * A[used]) and np.all(np.isnan(J[~used]))
    assert np.isclose(out["actual"], np.sum(ea ** 2 - eb ** 2), rtol=1e-12) and out["total"] == float(np.sum(J[used]))
