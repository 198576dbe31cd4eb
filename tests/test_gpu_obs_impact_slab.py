"""Observation impact under the temporal and variable tapers on the MI355X: efa_obs_impact_slab_dev against the
NumPy helper tests/_efso_slab.py, on the cases of tests/test_gpu_obs_impact.py (143 ragged columns, 150 obs).

Tolerance (derived, not measured): |J_k - ref_k| <= _efso.tolerance(rows, M) A_k = 1e-9 A_k at every shape here, the worst-case
forward bound of a float64 sum of rows * M terms in any order; the device table's 1e-15 relative difference from NumPy's (7t) adds
at most 1e-15 A_k to that.  A dropped row or a wrong factor shows at 1e-3 A_k or more.  Every parity case also asserts that at
least half of the used obs have A_k > 0, that unused obs come back exactly 0.0, and that the reference under the factors differs
from the plain-GC reference by more than 1e-3 A_k somewhere."""
import functools

import numpy as np
import pytest

import _efso
import _efso_slab
import test_gpu_obs_impact as gi

pytestmark = pytest.mark.gpu

P_OBS = 150
N_LEADS = [1, 5, 16, 17, 37]          # every lg_cols layout class that differs, the 16-slab edge, more than one group
MEMBERS = [2, 7, 80, 100, 104, 137, 256]   # both occupancies of the row-per-lane form, the pieces of 64 with an odd M
STEP_H = 6.0                          # hours between the valid times of a variable's slabs


def _ctx():
    ctx = gi._ctx()
    ctx.set_slab_localization(None)
    return ctx


def _slab(n_lead, P=P_OBS, seed=0):
    """The setting of a case as the keywords of Context.set_slab_localization, after test_gpu_slab_localization._slab.  The slabs
    are min(3, n_lead) variables of consecutive valid times STEP_H apart.  Ob times spread over (and beyond) them; tau from a
    quarter of the span to three spans; every fifth ob with tau 1 h, below the slab spacing, so that whole waves drop out, and the
    first two of them after ob 0 midway between two valid times, so that they drop out altogether; ob 0 without a time, ob 1
    without a tau.  Obtypes: the first nvar - 1 variables (their own entry 1) and one that names no state variable; about a tenth
    of the obs of an obtype the table does not have.  The last variable has impact 0 from every obtype; one entry is 0.4 or 0.7."""
    rng = np.random.default_rng(3000 + 10 * seed + n_lead)
    nvar = min(3, n_lead)
    lead_var = np.sort(np.arange(n_lead) % nvar)                    # variable-major, sizes differing by at most one
    lead_time = np.concatenate([STEP_H * np.arange(np.count_nonzero(lead_var == v)) for v in range(nvar)])
    span = max(float(lead_time.max()), STEP_H)
    ot = rng.uniform(-STEP_H, span + STEP_H, P)
    tau = span * rng.uniform(0.25, 3.0, P)
    tau[::5] = 1.0
    ot[5:15:5] = 0.5 * STEP_H
    ot[0] = np.nan
    tau[1] = np.nan
    named = max(nvar - 1, 1)
    og = rng.integers(0, named + 1, P)
    og = np.where(rng.random(P) < 0.1, -1, og)
    C = rng.choice([1.0, 0.7, 0.25], (named + 1, nvar))
    C[np.arange(named), np.arange(named)] = 1.0
    if nvar > 1:
        C[:, nvar - 1] = 0.0
    if nvar > 2:
        C[0, 1] = 0.4
    else:
        C[named, 0] = 0.7
    return dict(n_lead=n_lead, P=P, lead_time=lead_time, ob_time=ot, ob_time_halfwidth=tau, lead_var=lead_var.astype(np.int32),
                ob_group=og.astype(np.int32), ob_var=np.where((og >= 0) & (og < named), og, -1).astype(np.int32), impact=C)


def _vert_only(n_lead, P=P_OBS):
    """A setting that is on and whose every factor is exactly 1 (slabs without a time): the table then carries the vertical factors
    alone, as variant slab_vert of tools/slab_localization_cost.py builds it."""
    return dict(n_lead=n_lead, P=P, lead_time=np.full(n_lead, np.nan), ob_time=np.zeros(P), ob_time_halfwidth=np.ones(P))


def _model_kw(slab, vert):
    kw = {k: v for k, v in slab.items() if k not in ("n_lead", "P", "ob_var")}
    if vert is not None:
        kw.update(lead_vert=vert[0], ob_vert=vert[1], ob_vert_halfwidth=vert[2])
    return kw


@functools.lru_cache(maxsize=None)
def _reference(M, n_lead, vert=False, seed=0):
    c = gi._case(M, n_lead)
    v = gi._vertical(n_lead, c["P"]) if vert else None
    J, A = _efso_slab.efso_slab(c["Xf"], c["Ya"], c["v"], c["d"], c["r"], c["used"], c["glat"], c["glon"], c["ob_lat"], c["ob_lon"],
                                c["hw"], n_lead, **_model_kw(_slab(n_lead, c["P"], seed), v))
    J.setflags(write=False)
    A.setflags(write=False)
    return J, A


def _run(ctx, c, slab, vert=None, used=None, cols=None, v=None, entry="obs_impact_slab", loc=True):
    """efa_obs_impact_slab_dev (or entry) on the case under the setting `slab` (None: off); cols: a column shard [lo, hi)"""
    from efa_xray_amd import _lib
    ncol, n_lead, M, P = c["ncol"], c["n_lead"], c["M"], c["P"]
    lo, hi = cols if cols is not None else (0, ncol)
    Xf = c["Xf"].reshape(n_lead, ncol, M)[:, lo:hi].reshape(-1, M)
    v = (c["v"] if v is None else v).reshape(n_lead, ncol)[:, lo:hi].reshape(-1)
    try:
        ctx.set_slab_localization(**slab) if slab is not None else ctx.set_slab_localization(None)
        ctx.set_vertical_localization(*vert) if vert is not None else ctx.set_vertical_localization(None)
        Xd, vd, Yd = ctx.to_device(Xf), ctx.to_device(v), ctx.to_device(c["Ya"])
        used = c["used"] if used is None else used
        call = getattr(ctx, entry)
        if loc:
            J = call(Xf.shape[0], M, P, Xd, vd, Yd, c["d"], c["r"], used, _lib.LOC_GC, c["ob_lat"], c["ob_lon"], c["hw"],
                     c["glat"][lo:hi], c["glon"][lo:hi], n_lead)
        else:
            J = call(Xf.shape[0], M, P, Xd, vd, Yd, c["d"], c["r"], used)
        assert np.array_equal(Xd.download(), Xf) and np.array_equal(Yd.download(), c["Ya"])   # read only
        return J
    finally:
        ctx.set_slab_localization(None)
        ctx.set_vertical_localization(None)


def _assert_factor_matters(ref, plain):
    assert np.max(np.abs(ref[0] - plain[0]) / np.maximum(plain[1], 1e-300)) > 1e-3


# ---- parity against the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lead", N_LEADS)
@pytest.mark.parametrize("M", MEMBERS)
def test_slab_parity(M, n_lead):
    ctx = _ctx()
    c = gi._case(M, n_lead)
    ref = _reference(M, n_lead)
    J = _run(ctx, c, _slab(n_lead))
    gi._assert_parity("slab M=%d n_lead=%d" % (M, n_lead), J, ref, c)
    _assert_factor_matters(ref, gi._reference(M, n_lead))
    assert J[3] == 0.0 and c["used"][3]                 # used, but 5000 km from every column
    assert ctx.get_option("impact_us") > 0


@pytest.mark.parametrize("M", MEMBERS)
def test_slab_and_vertical_parity(M):
    ctx = _ctx()
    c = gi._case(M, 37)
    ref = _reference(M, 37, vert=True)
    J = _run(ctx, c, _slab(37), vert=gi._vertical(37, c["P"]))
    gi._assert_parity("slab+vertical M=%d" % M, J, ref, c)
    _assert_factor_matters(ref, gi._reference(M, 37))
    _assert_factor_matters(ref, _reference(M, 37))      # and the vertical factor on top of the slab's


# ---- exact zeros ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n_lead", [(80, 37), (137, 17), (7, 1)])
def test_an_ob_out_of_reach_of_every_slab_is_exactly_zero(M, n_lead):
    """Obs 5 and 10 sit midway between two valid times with a cut-off of 2 h: factor 0 on every slab, while their horizontal taper
    reaches the grid (A_k > 0 under the plain GC taper)."""
    ctx = _ctx()
    c = gi._case(M, n_lead)
    used = np.array(c["used"])
    used[[5, 10]] = True
    slab = _slab(n_lead)
    S = _efso_slab.slab_factor_table(n_lead, c["P"], **{k: v for k, v in _model_kw(slab, None).items()})
    assert np.all(S[[5, 10]] == 0.0)
    _, A_plain = _efso.efso(c["Xf"], c["Ya"], c["v"], c["d"], c["r"], used, grid_lat=c["glat"], grid_lon=c["glon"], ob_lat=c["ob_lat"],
                            ob_lon=c["ob_lon"], ob_halfwidth=c["hw"], n_lead=n_lead)
    assert np.all(A_plain[[5, 10]] > 0.0)
    J = _run(ctx, c, slab, used=used)
    assert J[5] == 0.0 and J[10] == 0.0 and not np.signbit(J[[5, 10]]).any()
    assert np.count_nonzero(J) > c["P"] // 2


@pytest.mark.parametrize("M", [80, 104, 137])
def test_a_norm_on_the_impact_zero_variable_alone(M):
    """v non-zero only on the last variable, which takes impact 0 from every obtype of the table: every ob with an impact row comes
    back as exactly 0.0, the obs of an obtype the table does not have keep their impact."""
    ctx = _ctx()
    n_lead = 37
    c = gi._case(M, n_lead)
    slab = _slab(n_lead)
    last = np.repeat(slab["lead_var"] == slab["lead_var"].max(), c["ncol"])
    v = np.where(last, c["v"], 0.0)
    J = _run(ctx, c, slab, v=v)
    listed = slab["ob_group"] >= 0
    assert listed.sum() > 100 and (~listed & c["used"]).sum() >= 5
    assert np.all(J[listed] == 0.0)
    Jr, A = _efso_slab.efso_slab(c["Xf"], c["Ya"], v, c["d"], c["r"], c["used"], c["glat"], c["glon"], c["ob_lat"], c["ob_lon"], c["hw"],
                                 n_lead, **_model_kw(slab, None))
    assert np.all(Jr[listed] == 0.0) and np.count_nonzero(Jr[~listed]) >= 5
    assert np.all(np.abs(J - Jr) <= _efso.tolerance(c["rows"], M) * A)


# ---- determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,vert", [(80, True), (137, False), (100, False)])
def test_two_calls_agree_bit_for_bit(M, vert):
    ctx = _ctx()
    c = gi._case(M, 37)
    v = gi._vertical(37, c["P"]) if vert else None
    a = _run(ctx, c, _slab(37), vert=v)
    b = _run(ctx, c, _slab(37), vert=v)
    assert np.array_equal(a, b)
    assert np.count_nonzero(a) > c["P"] // 2


@pytest.mark.parametrize("M", [80, 137])
def test_column_shards_add_up(M):
    """The table does not depend on the columns: two shards under the same setting add up to the whole."""
    ctx = _ctx()
    c = gi._case(M, 17)
    slab = _slab(17)
    whole = _run(ctx, c, slab)
    parts = _run(ctx, c, slab, cols=(0, 80)) + _run(ctx, c, slab, cols=(80, c["ncol"]))
    ref = _reference(M, 17)
    worst = float(np.max(np.abs(parts - whole) / np.maximum(ref[1], 1e-300)))
    print("shards M=%d: max |sum of shards - whole| / A = %.3e" % (M, worst))
    assert np.all(np.abs(parts - whole) <= _efso.tolerance(c["rows"], M) * ref[1])
    gi._assert_parity("shards M=%d" % M, parts, ref, c)


# ---- the vertical factors through the table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [7, 80, 100, 137])
def test_vertical_factors_through_the_table_equal_the_vertical_kernel(M):
    """The table carrying the vertical factors alone (every temporal and variable factor exactly 1) through the new entry, against
    efa_obs_impact_dev under the vertical setting.  Asserted within the tolerance.  The agreement is bit for bit on the MI355X at
    all four widths (the test prints it): k_slab_factor multiplies the same vert_factor by exactly 1.0 twice, and the two kernels
    share every other statement.  It is not asserted: it rests on the compiler giving vert_factor the same code in two files."""
    ctx = _ctx()
    c = gi._case(M, 37)
    vert = gi._vertical(37, c["P"])
    new = _run(ctx, c, _vert_only(37), vert=vert)
    old = _run(ctx, c, None, vert=vert, entry="obs_impact")
    ref = gi._reference(M, 37, vert=True)
    print("vertical through the table M=%d: bit for bit %s, max |new - old| / A = %.3e"
          % (M, np.array_equal(new, old), float(np.max(np.abs(new - old) / np.maximum(ref[1], 1e-300)))))
    assert np.all(np.abs(new - old) <= _efso.tolerance(c["rows"], M) * ref[1])
    gi._assert_parity("vertical through the table M=%d" % M, new, ref, c)


# ---- context hygiene ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vert", [False, True])
def test_with_the_setting_off_it_is_the_old_entry_bit_for_bit(vert):
    ctx = _ctx()
    for M, n_lead in ((80, 37), (137, 5)):
        c = gi._case(M, n_lead)
        v = gi._vertical(n_lead, c["P"]) if vert else None
        assert np.array_equal(_run(ctx, c, None, vert=v), _run(ctx, c, None, vert=v, entry="obs_impact"))
    c = gi._case(7, 5)
    assert np.array_equal(_run(ctx, c, None, loc=False), _run(ctx, c, None, entry="obs_impact", loc=False))


def test_setting_must_match_the_call():
    from efa_xray_amd import _lib
    ctx = _ctx()
    c = gi._case(7, 5)
    P = c["P"]
    slab = _slab(5)
    lead, ov, oh = gi._vertical(5, P)
    short = {k: (v[:-1] if k.startswith("ob_") else v) for k, v in slab.items()}
    fewer = {k: (v[:-1] if k.startswith("lead_") else v) for k, v in slab.items()}
    for kw in (dict(slab=dict(short, P=P - 1)), dict(slab=dict(fewer, n_lead=4)), dict(slab=slab, loc=False),
               dict(slab=slab, vert=(lead, ov[:-1], oh[:-1])), dict(slab=slab, vert=(lead[:-1], ov, oh))):
        with pytest.raises(_lib.EfaError) as e:
            _run(ctx, c, **kw)
        assert e.value.status == _lib.EFA_ERR_INVALID and "slab localisation" in str(e.value), str(e.value)
    # the old entry still refuses while the setting is on
    with pytest.raises(_lib.EfaError) as e:
        _run(ctx, c, slab, entry="obs_impact")
    assert "efa_obs_impact_dev" in str(e.value)
    assert ctx.get_option("impact_us") >= 0


def test_cycles_and_the_old_entry_after_a_call_return_the_same_bits():
    """A plain GC cycle, a vertical cycle and an old-entry impact, then (on one of two fresh contexts) a new-entry call under the
    slab and the vertical setting with another obs geometry, then the three again: bit for bit what the context without the call
    returns, gc_active_pairs and phase_a_kind included."""
    from efa_xray_amd import _lib
    glat, glon = gi._grid()
    ncol, n_lead, M, P = glat.size, 5, 20, 60
    rng = np.random.default_rng(12)
    N = n_lead * ncol
    X = 2.0 * rng.standard_normal((N, M)) + rng.standard_normal((N, 1))
    pick = rng.choice(N, P, replace=False)
    HX = X[pick] + 0.05 * rng.standard_normal((P, M))
    ob = dict(value=HX.mean(axis=1) + rng.standard_normal(P), error=rng.uniform(0.5, 2.0, P), assim=rng.random(P) < 0.9,
              lat=glat[pick % ncol] + rng.uniform(-0.5, 0.5, P), lon=glon[pick % ncol] + rng.uniform(-0.5, 0.5, P),
              hw=rng.uniform(600, 1500, P))
    cyc_vert = gi._vertical(n_lead, P, seed=3)
    c = gi._case(20, 5)
    imp_vert = gi._vertical(5, c["P"])

    def cycle(ctx, vert):
        ctx.set_vertical_localization(*vert) if vert is not None else ctx.set_vertical_localization(None)
        try:
            Xd, post, Yp, ym = ctx.to_device(X), ctx.empty((N, M)), ctx.to_device(HX), ctx.empty((P,))
            ctx.form_perts(P, M, Yp, ym, Yp)
            diag = ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, ob["value"], ob["error"], ob["assim"], _lib.LOC_GC, ob["lat"], ob["lon"],
                                   ob["hw"], glat, glon, n_lead)
            return post.download(), diag, ctx.get_option("gc_active_pairs"), ctx.get_option("phase_a_kind")
        finally:
            ctx.set_vertical_localization(None)

    def probes(ctx):
        return cycle(ctx, None), cycle(ctx, cyc_vert), _run(ctx, c, None, vert=imp_vert, entry="obs_impact")

    results = []
    for with_call in (True, False):
        ctx = _lib.Context(0)
        try:
            first = probes(ctx)
            if with_call:
                J = _run(ctx, c, _slab(5), vert=imp_vert)
                gi._assert_parity("between the probes", J, _reference(20, 5, vert=True), c)
            results.append((first, probes(ctx)))
        finally:
            ctx.close()
    (a1, a2), (b1, b2) = results
    for got, want in ((a1, b1), (a2, b2), (a2, a1)):
        for g, w in zip(got[:2], want[:2]):
            assert np.array_equal(g[0], w[0])
            for key in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
                assert np.array_equal(g[1][key], w[1][key], equal_nan=True), key
            assert g[2:] == w[2:]
        assert np.array_equal(got[2], want[2])
    assert a2[0][2] > 0 and np.count_nonzero(a2[2]) > c["P"] // 2


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _assert_settings_off(what):
    """Both settings are off on the device's shared context, probed without setting or clearing anything: the factor table is
    refused as not set, and the old entry accepts a plain GC call of another P and n_lead, which either setting, left on, refuses."""
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    with pytest.raises(_lib.EfaError) as e:
        ctx.slab_factor_table(30, 6)
    assert "not set" in str(e.value), what
    c = gi._case(7, 2)
    J = ctx.obs_impact(c["rows"], 7, c["P"], ctx.to_device(c["Xf"]), ctx.to_device(c["v"]), ctx.to_device(c["Ya"]), c["d"], c["r"],
                       c["used"], _lib.LOC_GC, c["ob_lat"], c["ob_lon"], c["hw"], c["glat"], c["glon"], 2)
    gi._assert_parity(what, J, gi._reference(7, 2), c)


def test_observation_impact_end_to_end_under_the_keywords():
    """EnSRF(loc='GC', time_localize=True, var_impact=vi).update() on 2 variables x 3 times x 12 x 14 x 20 members, then
    observation_impact with the same keywords against the helper fed from host arrays.  Only the second variable is verified, which
    takes impact 0 from the first variable's obs: those come back as exactly 0.0."""
    from efa_xray_amd import EnSRF, EnsembleState, Observation, _lib, observation_impact
    _ctx()
    rng = np.random.default_rng(8)
    nvar, nt, ny, nx, M, P = 2, 3, 12, 14, 20, 30
    lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(250, 280, nx), indexing="ij")
    truth = rng.standard_normal((nvar, nt, ny, nx))
    arr = truth[..., None] + 0.5 * rng.standard_normal((nvar, nt, ny, nx, 1)) + rng.standard_normal((nvar, nt, ny, nx, M))
    times = np.array([0.0, 3600.0, 7200.0])
    state = EnsembleState.from_array(arr, lat, lon, validtime=times)
    names = state.vars()
    vi = {names[0]: {names[1]: 0.0}, names[1]: {names[0]: 0.4}}
    obs = []
    for k in range(P):
        ob = Observation(value=float(rng.standard_normal()), obtype=names[k % nvar], time=float([0.0, 1800.0, 3600.0][k % 3]),
                         error=float(rng.uniform(0.5, 1.5)), lat=float(rng.uniform(31, 49)), lon=float(rng.uniform(251, 279)),
                         assimilate_this=(k % 6 != 1), localize_radius=float(rng.uniform(500, 1500)))
        if k % 5:
            ob.time_localize_radius = float(rng.uniform(1500.0, 5000.0))
        obs.append(ob)
    post, obs_out = EnSRF(state, obs, loc="GC", time_localize=True, var_impact=vi, verbose=False).update()
    ver = {names[1]: truth[1].copy()}
    ver[names[1]][1, 3, 4] = np.nan
    out = observation_impact(state, post, obs_out, ver, loc="GC", time_localize=True, var_impact=vi)
    _assert_settings_off("right after the keyword call")          # before anything else sets or clears a setting

    used = np.array([bool(o.assimilated) for o in obs_out])
    assert used.sum() == sum(k % 6 != 1 for k in range(P))
    v = np.zeros((nvar, nt, ny, nx))
    ok = ~np.isnan(ver[names[1]])
    eb = state.variables[names[1]].mean(axis=-1) - ver[names[1]]
    ea = post.variables[names[1]].mean(axis=-1) - ver[names[1]]
    v[1][ok] = (ea + eb)[ok]
    Ya = np.array([o.estimate(post) for o in obs_out])
    d = np.array([o.value - np.mean(o.estimate(state)) for o in obs_out])
    tau = np.array([np.nan if o.time_localize_radius is None else o.time_localize_radius for o in obs_out])
    geo = (lat.reshape(-1), lon.reshape(-1), [o.lat for o in obs_out], [o.lon for o in obs_out], [o.localize_radius for o in obs_out],
           nvar * nt)
    err = np.array([o.error for o in obs_out])
    Jr, A = _efso_slab.efso_slab(post.to_vect(), Ya, v.reshape(-1), d, err, used, *geo, lead_time=np.tile(times, nvar),
                                 ob_time=np.array([o.time for o in obs_out], dtype=float), ob_time_halfwidth=tau,
                                 lead_var=np.repeat(np.arange(nvar), nt), ob_group=np.array([names.index(o.obtype) for o in obs_out]),
                                 impact=np.array([[1.0, 0.0], [0.4, 1.0]]))
    J = out["impact"]
    tol = _efso.tolerance(post.nstate(), M)
    worst = float(np.max(np.abs(J - Jr)[used] / np.maximum(A[used], 1e-300)))
    print("end to end: max |J - ref| / A = %.3e, total %.6g, actual %.6g" % (worst, out["total"], out["actual"]))
    assert np.all(np.abs(J - Jr)[used] <= tol * A[used])
    first = np.array([o.obtype == names[0] for o in obs_out])
    assert (first & used).sum() >= 10 and np.all(J[first & used] == 0.0)                    # exactly 0.0
    assert np.count_nonzero(A[~first & used]) == (~first & used).sum() and np.all(J[~first & used] != 0.0)
    assert np.all(np.isnan(J[~used]))
    for k, o in enumerate(obs_out):
        assert (o.impact is None) if not used[k] else (o.impact == J[k])
    # without the keywords the taper is another one: the first variable's obs get an impact they did not have
    plain = observation_impact(state, post, obs_out, ver, loc="GC")["impact"]
    Jp, Ap = _efso.efso(post.to_vect(), Ya, v.reshape(-1), d, err, used, grid_lat=geo[0], grid_lon=geo[1], ob_lat=geo[2], ob_lon=geo[3],
                        ob_halfwidth=geo[4], n_lead=nvar * nt)
    assert np.all(np.abs(plain - Jp)[used] <= tol * Ap[used])
    assert np.all(plain[first & used] != 0.0) and np.max(np.abs(plain - J)[used] / Ap[used]) > 1e-3
    # a keyword call that fails inside the library, after it has set the slab and the vertical setting (a used ob whose value, and
    # so its innovation, is infinite): both settings are cleared on the way out
    import copy
    broken = copy.deepcopy(obs_out)
    k_bad = int(np.nonzero(used)[0][0])
    broken[k_bad].value = np.inf
    for k, o in enumerate(broken):
        if k % 4:
            o.vert, o.vert_localize_radius = float(k % 3), 1.2
    Z = np.array([[0.0, 0.5, 1.0], [2.0, np.nan, 3.0]])
    with pytest.raises(_lib.EfaError) as e:
        observation_impact(state, post, broken, ver, loc="GC", vert_coord=Z, time_localize=True, var_impact=vi)
    assert "efa_obs_impact_slab_dev" in str(e.value) and "innovation is not finite" in str(e.value)
    _assert_settings_off("right after a keyword call that raised")
    # and the same call, mended, runs under the three factors
    broken[k_bad].value = obs_out[k_bad].value
    full = observation_impact(state, post, broken, ver, loc="GC", vert_coord=Z, time_localize=True, var_impact=vi)["impact"]
    _assert_settings_off("right after the keyword call with vert_coord")
    assert np.all(full[first & used] == 0.0) and np.max(np.abs(full - J)[used] / Ap[used]) > 1e-3
