"""Temporal and cross-variable localisation on the MI355X: seeded cases and GC goldens through both sweep forms,
both state forms and every Phase-A kind, with and without the vertical factor, against the NumPy helper (tests/_slabloc.py) to
1e-10 relative; float32 and streamed states; the cross-check against the vertical family; the cases that must leave results bit
for bit as without the setting; the context state; the factor table read back; the register budget."""
import numpy as np
import pytest

import _slabloc as sl
import test_gpu_f32_state as f32t
import test_gpu_streamed_update as stt
from conftest import load_golden
from oracle import ensrf_oracle as orc
from test_gpu_parity import _make_api_objects, assert_parity, golden_kwargs

pytestmark = pytest.mark.gpu

FAMILY = dict(plain=0, adaptive=1, vertical=2, slab=3)       # option "gc_family"
KIND = dict(chain=1, batch=2, gram=3, band=4)                # option "phase_a_kind"


def _ctx():
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    ctx.set_slab_localization(None)
    ctx.set_vertical_localization(None)
    ctx.set_adaptive_inflation(None)
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    for key, v in (("path", 0), ("gram", 2), ("pipeline", 1), ("gc_onepass", 1), ("geometry_reuse", 1)):
        ctx.set_option(key, v)
    return ctx


def _seeded(M, P=150, nvar=3, nt=7, ny=10, nx=14, seed=0):
    """21 slabs: two groups of 16 in the row-per-lane form, the second partial (its padding slots beyond lead_hi); 150 obs: two
    64-ob leader hand-overs and a partial third block."""
    rng = np.random.default_rng(seed + M)
    N = nvar * nt * ny * nx
    glat, glon = np.meshgrid(np.linspace(25, 55, ny), np.linspace(240, 290, nx), indexing="ij")
    X = rng.standard_normal((N, M)) * 2.0 + rng.standard_normal((N, 1))
    rows = rng.choice(N, P, replace=False)
    HX = X[rows] + 0.05 * rng.standard_normal((P, M))
    col = rows % (ny * nx)
    g = dict(ob_value=HX.mean(axis=1) + rng.standard_normal(P), ob_error=rng.uniform(0.5, 2.0, P), ob_assim=rng.random(P) < 0.9,
             ob_lat=glat.reshape(-1)[col] + rng.uniform(-0.5, 0.5, P), ob_lon=glon.reshape(-1)[col] + rng.uniform(-0.5, 0.5, P),
             ob_radius=rng.uniform(600, 1500, P), grid_lat=glat, grid_lon=glon, loc="GC", shape=np.array([nvar, nt, ny, nx, M]))
    return g, X, HX, (nvar, nt, ny, nx)


def _slab(shape, P, seed=0, time=True, var=True):
    """The setting of a seeded case, as the keywords of Context.set_slab_localization.  Slabs 6 h apart; ob times spread over (and
    beyond) them, ob 0 without a time, every 11th ob without tau, tau 4 .. 14 h (so many (ob, slab) pairs lie beyond 2 tau).
    Obtypes: the first nvar - 1 variables (their own entry 1), and one that names no state variable; about a tenth of the obs have
    no impact row.  The last variable has impact 0 from every obtype; one entry lies strictly between 0 and 1."""
    nvar, nt = shape[:2]
    rng = np.random.default_rng(1000 + seed)
    kw = dict(n_lead=nvar * nt, P=P)
    if time:
        kw["lead_time"] = np.tile(6.0 * np.arange(nt), nvar)
        ot = rng.uniform(-6.0, 6.0 * nt, P)
        ot[0] = np.nan
        tau = rng.uniform(4.0, 14.0, P)
        tau[3::11] = np.nan
        kw.update(ob_time=ot, ob_time_halfwidth=tau)
    if var:
        named = max(nvar - 1, 1)                              # obtypes that name a state variable: variables 0 .. named - 1
        og = rng.integers(0, named + 1, P)                    # group `named`: an obtype that names no state variable
        ov = np.where(og < named, og, -1)
        og = np.where(rng.random(P) < 0.1, -1, og)            # an obtype var_impact does not mention
        C = rng.choice([1.0, 0.7, 0.25], (named + 1, nvar))
        C[np.arange(named), np.arange(named)] = 1.0
        if nvar > 1:
            C[:, nvar - 1] = 0.0
            C[0, 1 % nvar] = 0.4 if nvar > 2 else 0.0
        kw.update(lead_var=np.repeat(np.arange(nvar), nt), ob_group=og.astype(np.int32), ob_var=ov.astype(np.int32), impact=C)
    return kw


def _vertical(n_lead, P, seed=0):
    rng = np.random.default_rng(2000 + seed)
    lead = np.linspace(0.0, 3.0, n_lead)
    lead[n_lead // 2] = np.nan
    ov = rng.uniform(-0.3, 3.3, P)
    ov[1] = np.nan
    return lead, ov, 0.9 * rng.uniform(0.7, 1.3, P)


def _helper_kw(slab, vert):
    kw = {k: v for k, v in (slab or {}).items() if k not in ("n_lead", "P")}
    if vert is not None:
        kw.update(lead_vert=vert[0], ob_vert=vert[1], ob_vert_halfwidth=vert[2])
    return kw


def _helper(X, HX, g, shape, slab, vert=None, obs_taper="loop"):
    xbm, Xbp = orc.format_prior_state(X, HX)
    N = X.shape[0]
    xam, Xap, diag = sl.ensrf_update_slab(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], g["ob_lat"], g["ob_lon"],
                                          g["ob_radius"], g["grid_lat"], g["grid_lon"], shape, obs_taper=obs_taper,
                                          **_helper_kw(slab, vert))
    return orc.format_posterior_state(xam, Xap, N), xam, Xap, diag


def _check(what, got_post, diag, ref):
    post, _, _, rdiag = ref
    assert_parity(got_post, post, what + " posterior")
    for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
        assert_parity(np.asarray(diag[key], float), rdiag[key], what + " " + key)


def _run(ctx, g, X, HX, slab, vert=None, fused=True):
    """member form: efa_ensrf_cycle_dev in place; perturbation form: efa_ensrf_update (host arrays)"""
    N, M = X.shape
    P = len(g["ob_value"])
    ctx.set_slab_localization(**slab) if slab else ctx.set_slab_localization(None)
    ctx.set_vertical_localization(*vert) if vert is not None else ctx.set_vertical_localization(None)
    try:
        if fused:
            Xd = ctx.to_device(X)
            Yp = ctx.to_device(HX)
            ym = ctx.empty((P,))
            ctx.form_perts(P, M, Yp, ym, Yp)
            diag = ctx.ensrf_cycle(N, M, P, Xd, Xd, ym, Yp, g["ob_value"], g["ob_error"], g["ob_assim"], **golden_kwargs(g))
            return Xd.download(), diag
        xbm, Xbp = orc.format_prior_state(X, HX)
        diag = ctx.ensrf_update_host(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], **golden_kwargs(g))
        return orc.format_posterior_state(xbm, Xbp, N), diag
    finally:
        ctx.set_slab_localization(None)
        ctx.set_vertical_localization(None)


# ---- both sweep forms, both state forms, with and without the vertical factor -------------------------------------------------
@pytest.mark.parametrize("with_vert", [False, True], ids=["slab", "slab+vert"])
@pytest.mark.parametrize("fused", [True, False], ids=["members", "perts"])
@pytest.mark.parametrize("M", [4, 20, 80, 100, 104, 51, 81, 128, 256])
def test_seeded_both_sweep_forms(M, fused, with_vert):
    """M in {4, 20, 80, 100, 104}: row-per-lane form; {51, 81} (odd), 128, 256: quad form."""
    ctx = _ctx()
    g, X, HX, shape = _seeded(M)
    P = len(g["ob_value"])
    slab = _slab(shape, P, seed=M)
    vert = _vertical(shape[0] * shape[1], P, seed=M) if with_vert else None
    ref = _helper(X, HX, g, shape, slab, vert)
    got, diag = _run(ctx, g, X, HX, slab, vert, fused)
    assert ctx.get_option("gc_family") == FAMILY["slab"]
    _check("M=%d %s" % (M, "members" if fused else "perts"), got, diag, ref)
    other, _ = _run(ctx, g, X, HX, None, vert, fused)            # the two factors took part
    assert ctx.get_option("gc_family") == FAMILY["vertical" if with_vert else "plain"]
    assert not np.array_equal(other, got)


@pytest.mark.parametrize("part", ["time", "var"])
def test_each_part_alone(part):
    ctx = _ctx()
    g, X, HX, shape = _seeded(20, seed=5)
    slab = _slab(shape, len(g["ob_value"]), seed=6, time=part == "time", var=part == "var")
    ref = _helper(X, HX, g, shape, slab)
    got, diag = _run(ctx, g, X, HX, slab)
    assert ctx.get_option("gc_family") == FAMILY["slab"]
    _check(part + " only", got, diag, ref)


# ---- every Phase-A kind -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [("band", 2, 1), ("gram", 1, 1), ("chain", 0, 1), ("batch", 2, 0)], ids=lambda k: k[0])
def test_every_phase_a_kind(kind):
    name, gram, pipe = kind
    ctx = _ctx()
    ctx.set_option("gram", gram)
    ctx.set_option("pipeline", pipe)
    try:
        g, X, HX, shape = _seeded(40, P=400, seed=7)
        slab = _slab(shape, 400, seed=9)
        vert = _vertical(shape[0] * shape[1], 400, seed=9)
        ref = _helper(X, HX, g, shape, slab, vert)
        got, diag = _run(ctx, g, X, HX, slab, vert, True)
        assert ctx.get_option("phase_a_kind") == KIND[name]
        _check("Phase A " + name, got, diag, ref)
    finally:
        _ctx()


def test_phase_a_windows_against_per_batch():
    """About 20 000 obs x 40 members: two persistent windows (the tapered table per window, its arrays offset by the window's first
    ob; the other rows through the table-mode sweep) against the per-batch kernels with one ob per batch, both with all factors."""
    ctx = _ctx()
    M, P = 40, 20000
    rng = np.random.default_rng(91)
    HX = 3.0 * rng.standard_normal((P, M)) + rng.standard_normal((P, 1))
    val = HX.mean(axis=1) + rng.standard_normal(P)
    err = rng.uniform(0.5, 2.0, P)
    asm = rng.random(P) < 0.95
    kw = dict(loc_mode=1, ob_lat=rng.uniform(-60, 60, P), ob_lon=rng.uniform(0, 360, P), ob_halfwidth=rng.uniform(300, 900, P))
    slab = _slab((3, 1), P, seed=92)
    ov = rng.uniform(0, 3, P)
    ov[::17] = np.nan
    res = {}
    try:
        for name, pipe in (("batch", 0), ("windows", 1)):
            ctx.set_option("pipeline", pipe)
            ctx.set_slab_localization(**slab)
            ctx.set_vertical_localization(np.zeros(3), ov, np.full(P, 0.6))
            Yp = ctx.to_device(HX)
            ym = ctx.empty((P,))
            ctx.form_perts(P, M, Yp, ym, Yp)
            diag = ctx.obs_phase(M, P, ym, Yp, val, err, asm, **kw)
            res[name] = (Yp.download(), ym.download(), diag, ctx.get_option("phase_a_kind"))
        assert res["windows"][3] != KIND["batch"] and res["batch"][3] == KIND["batch"]
        for i, what in ((0, "Yp"), (1, "ym")):
            assert_parity(res["windows"][i], res["batch"][i], "windows vs batch " + what)
        for key in ("post_mean", "post_var"):
            assert_parity(res["windows"][2][key], res["batch"][2][key], "windows vs batch " + key)
        ctx.set_slab_localization(None)                          # and the two factors took part: the vertical-only run differs
        Yp = ctx.to_device(HX)
        ym = ctx.empty((P,))
        ctx.form_perts(P, M, Yp, ym, Yp)
        ctx.obs_phase(M, P, ym, Yp, val, err, asm, **kw)
        assert not np.allclose(Yp.download(), res["windows"][0], rtol=1e-6)
    finally:
        _ctx()


# ---- goldens through the Python interface -----------------------------------------------------------------------------------------
def _golden(name):
    g = load_golden(name)
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    X = g["X"].reshape(N, M).copy()
    HX = (g["sten_wts"][:, :, None] * X[g["sten_idx"]]).sum(axis=1)
    return g, X, HX, (nvar, nt, ny, nx)


def _dress(state, obs, slab):
    """The seeded setting as attributes of the obs and as the var_impact keyword (state variables var0, var1, ...; validtime 0, 1, ...
    taken as 6 h steps by scaling the ob times)."""
    names = state.vars()
    types = names[:slab["impact"].shape[0] - 1] + ["gauge"]
    for k, ob in enumerate(obs):
        g = int(slab["ob_group"][k])
        ob.obtype = types[g] if g >= 0 else "unlisted"
        t, tau = slab["ob_time"][k], slab["ob_time_halfwidth"][k]
        ob.time = None if np.isnan(t) else float(t)
        ob.time_localize_radius = None if np.isnan(tau) else float(tau)
    return {t: {n: float(c) for n, c in zip(names, row)} for t, row in zip(types, slab["impact"])}


@pytest.mark.parametrize("name", ["G2", "G5", "G8", "G12"])
def test_goldens_through_update_and_update_arrays(name):
    from efa_xray_amd import EnSRF, EnsembleState
    _ctx()
    g, X, HX, shape = _golden(name)
    nvar, nt = shape[:2]
    P = len(g["ob_value"])
    slab = _slab(shape, P, seed=len(name))
    slab["ob_var"] = np.where(slab["ob_group"] >= 0, slab["ob_var"], -1)   # ("unlisted" names no state variable either)
    ref = _helper(X, HX, g, shape, slab, obs_taper="vector" if P > 1000 else "loop")
    for arrays in (False, True):
        state, obs = _make_api_objects(g)
        state = EnsembleState.from_array(g["X"], g["grid_lat"], g["grid_lon"], validtime=6.0 * np.arange(nt))
        var_impact = _dress(state, obs, slab)
        flt = EnSRF(state, obs, loc="GC", time_localize=True, var_impact=var_impact, verbose=False)
        if not arrays:
            post_state, obs_out = flt.update()
            diag = {key: np.array([np.nan if getattr(o, key) is None or (key.startswith("post") and not o.assimilated)
                                   else getattr(o, key) for o in obs_out], float)
                    for key in ("prior_mean", "prior_var", "post_mean", "post_var")}
            _check(name + " update()", post_state.to_vect(), diag, ref)
        else:
            xbm, Xbp = orc.format_prior_state(X, HX)
            xam, Xap = flt.update_arrays(xbm, Xbp)
            assert_parity(xam, ref[1], name + " update_arrays mean")
            assert_parity(Xap, ref[2], name + " update_arrays perturbations")
        assert _ctx().get_option("gc_family") == FAMILY["slab"]


# ---- float32 and streamed states --------------------------------------------------------------------------------------------------
def _point_case(dtype, seed=0):
    state = f32t._state(400 + seed, 20, dtype=dtype)
    obs = f32t._point_obs(state, 401 + seed, 36)
    rng = np.random.default_rng(402 + seed)
    for k, ob in enumerate(obs):
        if k % 5 != 2:                                           # (times in seconds, as validtime: tau too)
            ob.time_localize_radius = float(rng.uniform(1500.0, 4000.0))
    var_impact = {state.vars()[0]: {state.vars()[1]: 0.3}, state.vars()[1]: {state.vars()[0]: 0.0}}
    vert = np.array([[900.0, 700.0, np.nan], [500.0, 300.0, 200.0]])
    for k, ob in enumerate(obs):
        if k % 4:
            ob.vert, ob.vert_localize_radius = 200.0 + 30.0 * k, 400.0
    return state, obs, var_impact, vert


@pytest.mark.parametrize("with_vert", [False, True], ids=["slab", "slab+vert"])
def test_float32_state_resident_and_streamed(with_vert):
    """The rules of 7f / 7g: the float32 update is the float64 update of the widened state rounded once, and every streamed chunk
    setting equals the resident run bit for bit."""
    _ctx()
    state, obs, var_impact, vert = _point_case(np.float32)
    kw = dict(loc="GC", time_localize=True, var_impact=var_impact)
    if with_vert:
        kw["vert_coord"] = vert
    got = f32t._assert_f32_update(state, obs, "slab float32", streamed=[16, 48], **kw)
    plain = f32t._update(state, obs, loc="GC")
    assert not np.array_equal(got[1], plain[1])


@pytest.mark.parametrize("M", [6, 8])
def test_float32_rows_against_the_helper(M):
    """The float32 row-per-lane kernel under the slab table against the NumPy helper itself (the case above holds it to the float64
    kernels): 20 columns (a full and a partial column block), 3 slabs (one folded group), 40 obs of which a fifth are not
    assimilated; M = 6 (padded to 8: the masked loads) and M = 8; the rows at a 16-byte aligned base and at one that is only
    8-byte aligned.  Bound: that of test_gpu_f32_state, half a float32 ulp of the one rounding plus the float64 tolerance."""
    ctx = _ctx()
    shape = (1, 3, 4, 5)
    pb = f32t.Problem(4100 + M, M, 40, n_lead=3, ny=4, nx=5, gc=True)
    g = dict(ob_value=pb.value, ob_error=pb.error, ob_assim=pb.assim, ob_lat=pb.ob_lat, ob_lon=pb.ob_lon, ob_radius=pb.hw,
             grid_lat=pb.glat.reshape(4, 5), grid_lon=pb.glon.reshape(4, 5))
    slab = _slab(shape, pb.P, seed=M)
    ref = _helper(pb.X64, pb.HX, g, shape, slab)[0]
    assert np.max(np.abs(ref - _helper(pb.X64, pb.HX, g, shape, None)[0])) > 1e-3   # the factors matter on this case
    ctx.set_slab_localization(**slab)
    try:
        for offset in (0, 2):
            post, _, _, native = f32t._run(pb, True, offset=offset, ctx=ctx)
            assert native == 1 and ctx.get_option("gc_family") == FAMILY["slab"]
            f32t._assert_reference_bound(post, ref, "slab float32 M=%d offset=%d" % (M, offset))
    finally:
        ctx.set_slab_localization(None)


@pytest.mark.parametrize("with_vert", [False, True], ids=["slab", "slab+vert"])
def test_streamed_float64_equals_resident_bit_for_bit(with_vert):
    _ctx()
    state, obs, var_impact, vert = _point_case(np.float64, seed=3)
    kw = dict(loc="GC", time_localize=True, var_impact=var_impact)
    if with_vert:
        kw["vert_coord"] = vert
    ref = stt._compare(state, obs, "slab streamed", chunks=[16, 48, None], **kw)
    assert not stt._same_bits(ref[1], stt._run(state, obs, loc="GC")[1]), "the tapers did nothing"
    stt._compare(state, obs, "slab + rtps + outlier", chunks=[48], rtps=0.3, outlier_threshold=4.0, **kw)


# ---- cross-check against the vertical family --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["members", "perts"])
@pytest.mark.parametrize("M", [20, 81])
def test_temporal_only_equals_the_vertical_family_fed_the_same_lags(M, fused):
    """T and V are the same function of (coordinate, ob coordinate, half-width) where every ob with a time has a tau: the
    temporal-only run through the slab table against the vertical-only run (vert_coord = the slab lags, ob.vert = the ob lags,
    vert_localize_radius = tau) through the vertical family."""
    ctx = _ctx()
    g, X, HX, shape = _seeded(M, seed=13)
    P = len(g["ob_value"])
    slab = _slab(shape, P, seed=14, var=False)
    no_tau = np.isnan(slab["ob_time_halfwidth"])
    slab["ob_time"] = np.where(no_tau, np.nan, slab["ob_time"])  # (an ob with a time but no tau is still tapered as a TARGET in
    a, da = _run(ctx, g, X, HX, slab, None, fused)               #  time, not in the vertical: such obs are left out of this case)
    assert ctx.get_option("gc_family") == FAMILY["slab"]
    b, db = _run(ctx, g, X, HX, None, (slab["lead_time"], slab["ob_time"], np.where(no_tau, 1.0, slab["ob_time_halfwidth"])), fused)
    assert ctx.get_option("gc_family") == FAMILY["vertical"]
    assert_parity(a, b, "temporal vs vertical posterior")
    for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
        assert_parity(da[key], db[key], "temporal vs vertical " + key)


# ---- off is off ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_vert", [False, True], ids=["plain", "vert"])
@pytest.mark.parametrize("fused", [True, False], ids=["members", "perts"])
def test_a_setting_without_factors_is_bit_identical_to_off(fused, with_vert):
    ctx = _ctx()
    g, X, HX, shape = _seeded(20, seed=21)
    nvar, nt = shape[:2]
    P = len(g["ob_value"])
    vert = _vertical(nvar * nt, P, seed=22) if with_vert else None
    off, doff = _run(ctx, g, X, HX, None, vert, fused)
    fam = ctx.get_option("gc_family")
    assert fam == FAMILY["vertical" if with_vert else "plain"]
    ones = dict(n_lead=nvar * nt, P=P, lead_time=np.tile(6.0 * np.arange(nt), nvar), ob_time=np.linspace(0.0, 30.0, P),
                ob_time_halfwidth=np.full(P, np.nan), lead_var=np.repeat(np.arange(nvar), nt), ob_group=np.zeros(P, np.int32),
                ob_var=np.zeros(P, np.int32), impact=np.ones((1, nvar)))
    on, don = _run(ctx, g, X, HX, ones, vert, fused)
    assert ctx.get_option("gc_family") == fam                    # the family that serves the call without the setting
    assert np.array_equal(off, on)
    for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
        assert np.array_equal(doff[key], don[key], equal_nan=True)


@pytest.mark.parametrize("with_vert", [False, True], ids=["plain", "vert"])
def test_keywords_without_factors_are_bit_identical_to_no_keywords(with_vert):
    """time_localize=True with no ob carrying a time_localize_radius, var_impact all ones."""
    from efa_xray_amd import EnSRF
    ctx = _ctx()
    g = load_golden("G8")
    nvar, nt = [int(v) for v in g["shape"][:2]]
    kw = dict(loc="GC", verbose=False)
    if with_vert:
        kw["vert_coord"] = np.linspace(0.0, 3.0, nvar * nt).reshape(nvar, nt)
    res = []
    for extra in (dict(), dict(time_localize=True, var_impact={"var0": {"var0": 1.0, "var%d" % (nvar - 1): 1.0}})):
        state, obs = _make_api_objects(g)
        for k, ob in enumerate(obs):
            ob.obtype, ob.time = "var0", float(k % nt)
            if with_vert:
                ob.vert, ob.vert_localize_radius = 0.02 * k, 1.0
        post, out = EnSRF(state, obs, **dict(kw, **extra)).update()
        res.append((post.to_vect(), stt._diag(out), ctx.get_option("gc_family")))
    assert res[0][2] == res[1][2] == FAMILY["vertical" if with_vert else "plain"]
    assert np.array_equal(res[0][0], res[1][0])
    for key in stt.DIAG:
        assert np.array_equal(res[0][1][key], res[1][1][key], equal_nan=True)


# ---- context state ------------------------------------------------------------------------------------------------------------------
def test_set_run_clear_leaves_the_context_as_fresh():
    """After a slab run and its clearing, a plain GC run, a vertical-only run and an observation_impact call on the shared context
    equal the same calls made before the setting was ever used."""
    from efa_xray_amd import EnSRF
    from efa_xray_amd.postprocess.impact import observation_impact
    ctx = _ctx()
    g, X, HX, shape = _seeded(20, seed=61)
    P = len(g["ob_value"])
    vert = _vertical(shape[0] * shape[1], P, seed=62)
    state, obs, var_impact, _ = _point_case(np.float64, seed=7)
    truth = {n: state.variables[n].mean(axis=-1) + 0.1 for n in state.vars()}

    def probes():
        plain = _run(ctx, g, X, HX, None, None)
        vonly = _run(ctx, g, X, HX, None, vert)
        post, out = EnSRF(state, stt.deepcopy(obs), loc="GC", verbose=False).update()
        imp = observation_impact(state, post, out, truth, loc="GC")["impact"]
        return plain, vonly, imp

    before = probes()
    _run(ctx, g, X, HX, _slab(shape, P, seed=63), vert)
    # an EnSRF that leaves the setting ON behind it (the context is shared per device): the next entry points clear it themselves
    EnSRF(state, stt.deepcopy(obs), loc="GC", time_localize=True, var_impact=var_impact, verbose=False).update()
    post, out = EnSRF(state, stt.deepcopy(obs), loc="GC", verbose=False).update()
    EnSRF(state, stt.deepcopy(obs), loc="GC", time_localize=True, var_impact=var_impact, verbose=False).update()
    imp_after = observation_impact(state, post, out, truth, loc="GC")["impact"]
    after = probes()
    assert np.array_equal(imp_after, before[2], equal_nan=True)
    for (pa, da), (pb, db) in zip(before[:2], after[:2]):
        assert np.array_equal(pa, pb)
        for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
            assert np.array_equal(da[key], db[key], equal_nan=True)
    assert np.array_equal(before[2], after[2], equal_nan=True)


def test_context_refuses_unsupported_calls_while_set():
    from efa_xray_amd import _lib
    ctx = _ctx()
    g, X, HX, shape = _seeded(20, seed=51)
    P = len(g["ob_value"])
    n_lead = shape[0] * shape[1]
    slab = _slab(shape, P, seed=52)
    N, M = X.shape

    def cycle(**over):
        Xd = ctx.to_device(X)
        Yp = ctx.to_device(HX)
        ym = ctx.empty((P,))
        ctx.form_perts(P, M, Yp, ym, Yp)
        kw = dict(golden_kwargs(g), **over)
        ctx.ensrf_cycle(N, M, P, Xd, Xd, ym, Yp, g["ob_value"], g["ob_error"], g["ob_assim"], **kw)

    def refused(call, word):
        with pytest.raises(_lib.EfaError) as ei:
            call()
        assert ei.value.status == _lib.EFA_ERR_INVALID and word in str(ei.value), str(ei.value)

    try:
        ctx.set_slab_localization(**slab)
        refused(lambda: cycle(loc_mode=0), "GC localisation")
        ctx.set_option("gc_onepass", 0)
        refused(cycle, "gc_onepass")
        ctx.set_option("gc_onepass", 1)
        F = ctx.to_device(np.tile([1.0, 0.6], (N, 1)))
        ctx.set_adaptive_inflation(F, N)
        refused(cycle, "adaptive inflation")
        ctx.set_adaptive_inflation(None)
        kw = golden_kwargs(g)
        refused(lambda: ctx.obs_impact(N, M, P, ctx.to_device(X), ctx.to_device(np.ones(N)), ctx.to_device(HX), np.zeros(P),
                                       g["ob_error"], g["ob_assim"], **kw), "efa_obs_impact_dev")
        short = {k: (v[:-1] if k.startswith("ob_") else v) for k, v in slab.items()}
        ctx.set_slab_localization(**dict(short, P=P - 1))        # another P
        refused(cycle, "observations")
        fewer = {k: (v[:-1] if k.startswith("lead_") else v) for k, v in slab.items()}
        ctx.set_slab_localization(**dict(fewer, n_lead=n_lead - 1))   # another n_lead
        refused(cycle, "slabs")
        # the setter's own checks
        for bad in (dict(ob_time_halfwidth=np.where(np.arange(P) == 3, -1.0, 5.0)), dict(ob_time=np.where(np.arange(P) == 3, np.inf, 1.0)),
                    dict(impact=np.where(slab["impact"] == 0.4, 1.5, slab["impact"])), dict(impact=slab["impact"] * 0.5),
                    dict(ob_group=np.full(P, 9, np.int32)), dict(lead_var=np.full(n_lead, 3, np.int32))):
            refused(lambda: ctx.set_slab_localization(**dict(slab, **bad)), "slab localisation")
        ctx.set_slab_localization(None)
        cycle()                                                      # cleared: the plain call runs
        refused(lambda: ctx.slab_factor_table(P, n_lead), "not set")
    finally:
        _ctx()


# ---- the table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_vert", [False, True], ids=["slab", "slab+vert"])
def test_factor_table_read_back(with_vert):
    ctx = _ctx()
    nvar, nt, P = 3, 7, 150
    slab = _slab((nvar, nt), P, seed=71)
    vert = _vertical(nvar * nt, P, seed=72) if with_vert else None
    try:
        ctx.set_slab_localization(**slab)
        if with_vert:
            ctx.set_vertical_localization(*vert)
        S = ctx.slab_factor_table(P, nvar * nt)
    finally:
        _ctx()
    kw = _helper_kw(slab, vert)
    kw.pop("ob_var")
    ref = sl.slab_factor_table(nvar * nt, P, **kw)
    assert S.shape == ref.shape == (P, nvar * nt)
    assert np.array_equal(S == 0.0, ref == 0.0)                      # zeros are exact zeros, and nothing else is
    assert (ref == 0.0).sum() > P and (ref[:, : 2 * nt] == 0.0).any()    # a whole variable, and pairs beyond 2 tau
    assert ((ref > 0.0) & (ref < 1.0)).any() and (ref == 1.0).any()
    nz = ref != 0.0
    assert np.max(np.abs(S[nz] - ref[nz]) / ref[nz]) <= 1e-15


# ---- registers --------------------------------------------------------------------------------------------------------------------
def test_slab_kernels_register_budget():
    """The row-per-lane slab kernels at configs[2]'s and configs[3]'s member counts (80, 100), both state forms: no scratch, no
    spill, two waves per SIMD."""
    from efa_xray_amd import _lib
    from _codeobj import gc_kernel_fragment, kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    for mp in (80, 100):
        for fused in (0, 1):
            hits = [k for n, k in tab.items() if gc_kernel_fragment("lane", "slab", "f64", mp, fused) in n]
            assert len(hits) == 1
            k = hits[0]
            assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0, (mp, fused, k[".vgpr_count"])
            assert k[".vgpr_count"] <= 256
