"""Vertical localisation on the MI355X: the GC goldens and seeded cases through both sweep forms, both state
forms and every Phase-A kind, against the NumPy helper (tests/_vertloc.py) to 1e-10 relative; the cases that must leave results
bit for bit as without it; the context state; the register budget; one configs[2]-sized cycle on sampled rows."""
import numpy as np
import pytest

import _vertloc as vl
from conftest import load_golden
from oracle import ensrf_oracle as orc
from test_gpu_parity import _make_api_objects, assert_parity, golden_kwargs

pytestmark = pytest.mark.gpu


def _ctx():
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    ctx.set_vertical_localization(None)
    ctx.set_adaptive_inflation(None)
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    for key, v in (("path", 0), ("gram", 2), ("pipeline", 1), ("gc_onepass", 1), ("geometry_reuse", 1)):
        ctx.set_option(key, v)
    return ctx


def _vertical(n_lead, P, seed=0, nan_slab=True, hw=0.9):
    """Slab coordinates 0 .. 3 with one NaN slab, ob coordinates spread over them, ob 0 without a coordinate."""
    rng = np.random.default_rng(seed)
    lead = np.linspace(0.0, 3.0, n_lead)
    if nan_slab and n_lead > 1:
        lead[n_lead // 2] = np.nan
    ov = rng.uniform(-0.3, 3.3, P)
    ov[0] = np.nan
    oh = np.full(P, hw) * rng.uniform(0.7, 1.3, P)
    return lead, ov, oh


def _helper(X, HX, g, shape, lead, ov, oh, rows=None, obs_taper="loop"):
    xbm, Xbp = orc.format_prior_state(X, HX)
    N = X.shape[0]
    xam, Xap, diag = vl.ensrf_update_vert(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], g["ob_lat"], g["ob_lon"],
                                          g["ob_radius"], g["grid_lat"], g["grid_lon"], shape, lead_vert=lead, ob_vert=ov,
                                          ob_vert_halfwidth=oh, rows=rows, obs_taper=obs_taper)
    return orc.format_posterior_state(xam, Xap, N), xam, Xap, diag


def _check(what, got_post, diag, ref):
    post, _, _, rdiag = ref
    assert_parity(got_post, post, what + " posterior")
    for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
        assert_parity(np.asarray(diag[key], float), rdiag[key], what + " " + key)


def _golden(name):
    g = load_golden(name)
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    X = g["X"].reshape(N, M).copy()
    HX = (g["sten_wts"][:, :, None] * X[g["sten_idx"]]).sum(axis=1)
    return g, X, HX, (nvar, nt, ny, nx)


@pytest.mark.parametrize("name", ["G2", "G5", "G6", "G8", "G12"])
def test_goldens_through_update_and_update_arrays(name):
    from efa_xray_amd import EnSRF
    _ctx()
    g, X, HX, shape = _golden(name)
    nvar, nt = shape[:2]
    P = len(g["ob_value"])
    lead, ov, oh = _vertical(nvar * nt, P, seed=len(name))
    ref = _helper(X, HX, g, shape, lead, ov, oh, obs_taper="vector" if P > 1000 else "loop")
    state, obs = _make_api_objects(g)
    for k, ob in enumerate(obs):
        ob.vert = None if np.isnan(ov[k]) else float(ov[k])
        ob.vert_localize_radius = float(oh[k])
    Z = lead.reshape(nvar, nt)
    post_state, obs_out = EnSRF(state, obs, loc="GC", vert_coord=Z, verbose=False).update()
    diag = {key: np.array([np.nan if getattr(o, key) is None or (key.startswith("post") and not o.assimilated) else getattr(o, key)
                           for o in obs_out], float) for key in ("prior_mean", "prior_var", "post_mean", "post_var")}
    _check(name + " update()", post_state.to_vect(), diag, ref)
    # update_arrays on the augmented arrays (perturbation form)
    state, obs = _make_api_objects(g)
    for k, ob in enumerate(obs):
        ob.vert = None if np.isnan(ov[k]) else float(ov[k])
        ob.vert_localize_radius = float(oh[k])
    xbm, Xbp = orc.format_prior_state(X, HX)
    xam, Xap = EnSRF(state, obs, loc="GC", vert_coord=Z, verbose=False).update_arrays(xbm, Xbp)
    assert_parity(xam, ref[1], name + " update_arrays mean")
    assert_parity(Xap, ref[2], name + " update_arrays perturbations")


def _seeded(M, P=150, nvar=2, nt=5, ny=10, nx=14, seed=0):
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


def _run(ctx, g, X, HX, vert, fused=True):
    """member form: efa_ensrf_cycle_dev in place; perturbation form: efa_ensrf_update (host arrays)"""
    N, M = X.shape
    P = len(g["ob_value"])
    if vert is None:
        ctx.set_vertical_localization(None)
    else:
        ctx.set_vertical_localization(*vert)
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
        ctx.set_vertical_localization(None)


@pytest.mark.parametrize("fused", [True, False], ids=["members", "perts"])
@pytest.mark.parametrize("M", [4, 20, 80, 100, 104, 51, 81, 128, 256])
def test_seeded_both_sweep_forms(M, fused):
    """M in {4, 20, 80, 100, 104}: row-per-lane form; {51, 81} (odd), 128, 256: quad form."""
    ctx = _ctx()
    g, X, HX, shape = _seeded(M)
    P = len(g["ob_value"])
    vert = _vertical(shape[0] * shape[1], P, seed=M)
    ref = _helper(X, HX, g, shape, *vert)
    got, diag = _run(ctx, g, X, HX, vert, fused)
    _check("M=%d %s" % (M, "members" if fused else "perts"), got, diag, ref)
    plain, _ = _run(ctx, g, X, HX, None, fused)
    assert not np.array_equal(plain, got)                       # the vertical factor took part


@pytest.mark.parametrize("M", [6, 8])
def test_float32_rows_against_the_helper(M):
    """The float32 row-per-lane kernel with the vertical factor against the NumPy helper itself (test_gpu_f32_state holds it to the
    float64 kernels): 20 columns (a full and a partial column block), 3 slabs (one folded group), 40 obs of which a fifth are not
    assimilated; M = 6 (padded to 8: the masked loads) and M = 8; the rows at a 16-byte aligned base and at one that is only
    8-byte aligned.  Bound: that of test_gpu_f32_state, half a float32 ulp of the one rounding plus the float64 tolerance."""
    import test_gpu_f32_state as f32t
    ctx = _ctx()
    shape = (1, 3, 4, 5)
    pb = f32t.Problem(4000 + M, M, 40, n_lead=3, ny=4, nx=5, gc=True)
    g = dict(ob_value=pb.value, ob_error=pb.error, ob_assim=pb.assim, ob_lat=pb.ob_lat, ob_lon=pb.ob_lon, ob_radius=pb.hw,
             grid_lat=pb.glat.reshape(4, 5), grid_lon=pb.glon.reshape(4, 5))
    vert = _vertical(3, pb.P, seed=M, nan_slab=False)
    ref = _helper(pb.X64, pb.HX, g, shape, *vert)[0]
    assert np.max(np.abs(ref - _helper(pb.X64, pb.HX, g, shape, None, None, None)[0])) > 1e-3   # the factor matters on this case
    ctx.set_vertical_localization(*vert)
    try:
        for offset in (0, 2):
            post, _, _, native = f32t._run(pb, True, offset=offset, ctx=ctx)
            assert native == 1 and ctx.get_option("gc_family") == 2
            f32t._assert_reference_bound(post, ref, "vertical float32 M=%d offset=%d" % (M, offset))
    finally:
        ctx.set_vertical_localization(None)


@pytest.mark.parametrize("kind", [("band", 2, 1), ("gram", 1, 1), ("chain", 0, 1), ("batch", 2, 0)])
def test_every_phase_a_kind(kind):
    name, gram, pipe = kind
    ctx = _ctx()
    ctx.set_option("gram", gram)
    ctx.set_option("pipeline", pipe)
    try:
        g, X, HX, shape = _seeded(40, P=400, seed=7)
        vert = _vertical(shape[0] * shape[1], 400, seed=9)
        ref = _helper(X, HX, g, shape, *vert)
        got, diag = _run(ctx, g, X, HX, vert, True)
        print("Phase A %s: phase_a_kind %d" % (name, ctx.get_option("phase_a_kind")))
        if pipe == 0:
            assert ctx.get_option("phase_a_kind") == 2
        _check("Phase A " + name, got, diag, ref)
    finally:
        _ctx()


def test_phase_a_windows_against_per_batch():
    """About 20 000 obs x 40 members: two persistent windows (the vertically tapered table per window, the other rows through
    the table-mode sweep) against the per-batch kernels, both with the vertical factor."""
    ctx = _ctx()
    M, P = 40, 20000
    rng = np.random.default_rng(91)
    HX = 3.0 * rng.standard_normal((P, M)) + rng.standard_normal((P, 1))
    val = HX.mean(axis=1) + rng.standard_normal(P)
    err = rng.uniform(0.5, 2.0, P)
    asm = rng.random(P) < 0.95
    kw = dict(loc_mode=1, ob_lat=rng.uniform(-60, 60, P), ob_lon=rng.uniform(0, 360, P), ob_halfwidth=rng.uniform(300, 900, P))
    ov = rng.uniform(0, 3, P)
    ov[::17] = np.nan
    oh = np.full(P, 0.6)
    res = {}
    try:
        for name, pipe in (("batch", 0), ("windows", 1)):
            ctx.set_option("pipeline", pipe)
            ctx.set_vertical_localization(np.zeros(1), ov, oh)
            Yp = ctx.to_device(HX)
            ym = ctx.empty((P,))
            ctx.form_perts(P, M, Yp, ym, Yp)
            diag = ctx.obs_phase(M, P, ym, Yp, val, err, asm, **kw)
            res[name] = (Yp.download(), ym.download(), diag, ctx.get_option("phase_a_kind"))
        assert res["windows"][3] != 2 and res["batch"][3] == 2
        for i, what in ((0, "Yp"), (1, "ym")):
            assert_parity(res["windows"][i], res["batch"][i], "windows vs batch " + what)
        for key in ("post_mean", "post_var"):
            assert_parity(res["windows"][2][key], res["batch"][2][key], "windows vs batch " + key)
        # and the factor took part: the horizontal-only run differs
        ctx.set_vertical_localization(None)
        Yp = ctx.to_device(HX)
        ym = ctx.empty((P,))
        ctx.form_perts(P, M, Yp, ym, Yp)
        ctx.obs_phase(M, P, ym, Yp, val, err, asm, **kw)
        assert not np.allclose(Yp.download(), res["windows"][0], rtol=1e-6)
    finally:
        _ctx()


def test_two_column_shards_equal_the_unsharded_run():
    from efa_xray_amd.distributed import HipEngine, ShardedEnSRF
    _ctx()
    g, X, HX, shape = _seeded(20, P=120, seed=3)
    nvar, nt, ny, nx = shape
    n_lead, ncol, M = nvar * nt, ny * nx, 20
    P = len(g["ob_value"])
    lead, ov, oh = _vertical(n_lead, P, seed=4)
    eng = HipEngine(0)
    torch = eng.torch
    ob = dict(value=g["ob_value"], error=g["ob_error"], assim=g["ob_assim"], loc="GC", lat=g["ob_lat"], lon=g["ob_lon"],
              halfwidth=g["ob_radius"], vert=ov, vert_halfwidth=oh)
    Xl = X.reshape(n_lead, ncol, M)
    outs = []
    for bounds in ([(0, ncol)], [(0, 61), (61, ncol)]):
        parts = []
        for r, (lo, hi) in enumerate(bounds):
            sh = ShardedEnSRF(eng, n_lead, ncol, M, rank=0, world_size=1, bounds=[(0, ncol)])
            sh.lo, sh.hi, sh.rows_local = lo, hi, n_lead * (hi - lo)
            Xd = torch.from_numpy(np.ascontiguousarray(Xl[:, lo:hi].reshape(-1, M))).to(eng.device)
            post = torch.empty_like(Xd)
            HXd = torch.from_numpy(HX.copy()).to(eng.device)
            sh.assimilate(Xd, post, HXd, ob, g["grid_lat"].reshape(-1), g["grid_lon"].reshape(-1), vert_coord=lead.reshape(nvar, nt))
            torch.cuda.synchronize()
            parts.append(post.cpu().numpy().reshape(n_lead, hi - lo, M))
        outs.append(np.concatenate(parts, axis=1).reshape(-1, M))
    assert np.array_equal(outs[0], outs[1])
    ref = _helper(X, HX, g, shape, lead, ov, oh)
    assert_parity(outs[0], ref[0], "sharded posterior")
    eng.ctx.set_vertical_localization(None)


def test_rtps_with_vertical_localisation():
    from efa_xray_amd import _lib
    ctx = _ctx()
    g, X, HX, shape = _seeded(20, seed=11)
    vert = _vertical(shape[0] * shape[1], len(g["ob_value"]), seed=12)
    ref = _helper(X, HX, g, shape, *vert)
    ctx.set_relaxation(_lib.RELAX_RTPS, 0.7)
    try:
        got, _ = _run(ctx, g, X, HX, vert, True)
    finally:
        ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    post = ref[0]
    pm = post.mean(axis=1, keepdims=True)
    sb, sa = X.std(axis=1, ddof=1, keepdims=True), post.std(axis=1, ddof=1, keepdims=True)
    fac = np.where(sa > 0, 1.0 + 0.7 * (sb - sa) / np.where(sa > 0, sa, 1.0), 1.0)
    assert_parity(got, pm + fac * (post - pm), "RTPS + vertical")


@pytest.mark.parametrize("fused", [True, False], ids=["members", "perts"])
def test_no_ob_with_vert_is_bit_identical_to_off(fused):
    ctx = _ctx()
    g, X, HX, shape = _seeded(20, seed=21)
    P = len(g["ob_value"])
    lead = np.linspace(0, 3, shape[0] * shape[1])
    off, doff = _run(ctx, g, X, HX, None, fused)
    on, don = _run(ctx, g, X, HX, (lead, np.full(P, np.nan), np.ones(P)), fused)
    assert np.array_equal(off, on)
    for key in ("post_mean", "post_var"):
        assert np.array_equal(doff[key], don[key], equal_nan=True)


def test_rows_no_ob_reaches_stay_bit_identical_in_perturbation_form():
    """The last slab sits beyond every ob's vertical reach: its perturbations and means leave the state phase bit for bit."""
    ctx = _ctx()
    g, X, HX, shape = _seeded(20, seed=31)
    nvar, nt, ny, nx = shape
    N, P = X.shape[0], len(g["ob_value"])
    lead = np.linspace(0, 3, nvar * nt)
    lead[-1] = 50.0
    ctx.set_vertical_localization(lead, np.full(P, 1.0), np.full(P, 0.5))
    try:
        xbm, Xbp = orc.format_prior_state(X, HX)
        xm0, Xp0 = xbm.copy(), Xbp.copy()
        ctx.ensrf_update_host(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], **golden_kwargs(g))
    finally:
        ctx.set_vertical_localization(None)
    last = slice((nvar * nt - 1) * ny * nx, N)
    assert np.array_equal(xbm[last], xm0[last]) and np.array_equal(Xbp[last], Xp0[last])
    mid = slice(2 * ny * nx, 3 * ny * nx)
    assert not np.array_equal(Xbp[mid], Xp0[mid])


def test_changing_only_ob_vert_between_cycles_rebuilds_the_cached_taper():
    ctx = _ctx()
    g, X, HX, shape = _seeded(40, P=300, seed=41)
    n_lead, P = shape[0] * shape[1], 300
    lead, ov, oh = _vertical(n_lead, P, seed=42)
    for cycle, shift in enumerate((0.0, 0.8)):
        ov2 = ov + shift
        ref = _helper(X, HX, g, shape, lead, ov2, oh)
        got, diag = _run(ctx, g, X, HX, (lead, ov2, oh), True)
        _check("cycle %d" % cycle, got, diag, ref)


def test_plain_ensrf_after_a_vertical_one_equals_a_fresh_context():
    from efa_xray_amd import EnSRF, _lib
    g, X, HX, shape = _golden("G8")
    nvar, nt = shape[:2]
    P = len(g["ob_value"])
    lead, ov, oh = _vertical(nvar * nt, P, seed=5)
    _ctx()
    state, obs = _make_api_objects(g)
    fresh = EnSRF(state, obs, loc="GC", verbose=False).update()[0].to_vect()
    for k, ob in enumerate(obs):
        ob.vert = None if np.isnan(ov[k]) else float(ov[k])
        ob.vert_localize_radius = float(oh[k])
    EnSRF(state, obs, loc="GC", vert_coord=lead.reshape(nvar, nt), verbose=False).update()
    after = EnSRF(state, obs, loc="GC", verbose=False).update()[0].to_vect()
    assert np.array_equal(after, fresh)
    ctx = _lib.Context(0)                                      # a context of its own
    try:
        ref = ctx.to_device(X)
        Yp = ctx.to_device(HX)
        ym = ctx.empty((P,))
        ctx.form_perts(P, X.shape[1], Yp, ym, Yp)
        ctx.ensrf_cycle(X.shape[0], X.shape[1], P, ref, ref, ym, Yp, g["ob_value"], g["ob_error"], g["ob_assim"], **golden_kwargs(g))
        assert np.array_equal(ref.download(), fresh.reshape(X.shape))
    finally:
        ctx.close()


def test_context_refuses_unsupported_combinations():
    from efa_xray_amd import _lib
    ctx = _ctx()
    g, X, HX, shape = _seeded(20, seed=51)
    P = len(g["ob_value"])
    lead, ov, oh = _vertical(shape[0] * shape[1], P)
    N, M = X.shape

    def cycle(**over):
        Xd = ctx.to_device(X)
        Yp = ctx.to_device(HX)
        ym = ctx.empty((P,))
        ctx.form_perts(P, M, Yp, ym, Yp)
        kw = dict(golden_kwargs(g), **over)
        ctx.ensrf_cycle(N, M, P, Xd, Xd, ym, Yp, g["ob_value"], g["ob_error"], g["ob_assim"], **kw)

    try:
        ctx.set_vertical_localization(lead, ov[:-1], oh[:-1])          # P mismatch
        with pytest.raises(_lib.EfaError):
            cycle()
        ctx.set_vertical_localization(lead[:-1], ov, oh)               # n_lead mismatch
        with pytest.raises(_lib.EfaError):
            cycle()
        ctx.set_vertical_localization(lead, ov, oh)
        with pytest.raises(_lib.EfaError):
            cycle(loc_mode=0)
        ctx.set_option("gc_onepass", 0)
        with pytest.raises(_lib.EfaError):
            cycle()
        ctx.set_option("gc_onepass", 1)
        F = ctx.to_device(np.tile([1.0, 0.6], (N, 1)))
        ctx.set_adaptive_inflation(F, N)
        with pytest.raises(_lib.EfaError):
            cycle()
        ctx.set_adaptive_inflation(None)
        with pytest.raises(_lib.EfaError):
            ctx.set_vertical_localization(lead, ov, np.where(np.arange(P) == 3, -1.0, oh))
    finally:
        _ctx()


def test_vertical_kernels_register_budget():
    """No spills for the lane form at configs[2]'s and configs[3]'s member counts (80, 100), both state forms."""
    from efa_xray_amd import _lib
    from _codeobj import gc_kernel_fragment, kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    for mp in (80, 100):
        for fused in (0, 1):
            hits = [k for n, k in tab.items() if gc_kernel_fragment("lane", "vloc", "f64", mp, fused) in n]
            assert len(hits) == 1
            k = hits[0]
            assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0, (mp, fused, k[".vgpr_count"])
            assert k[".vgpr_count"] <= 256


def test_configs2_sized_cycle_on_sampled_rows():
    """38 468 160 rows (4 variables x 37 levels x 361 x 720) x 80 members x 5 000 obs, levels on the time slot, ln p as the
    vertical coordinate (one scale height as half-width): a few thousand sampled rows against the helper run on those rows and
    the obs block only (rows are independent given the obs trajectory)."""
    ctx = _ctx()
    nvar, nlev, ny, nx, M, P = 4, 37, 361, 720, 80, 5000
    ncol = ny * nx
    N = nvar * nlev * ncol
    glat, glon = np.meshgrid(np.linspace(-90, 90, ny), np.linspace(0, 359.5, nx), indexing="ij")
    rng = np.random.default_rng(2)
    X = ctx.empty((N, M))
    ctx.fill_synthetic(N, 0, M, 7, 1.0, X)
    HX = 2.0 * rng.standard_normal((P, M)) + rng.standard_normal((P, 1))
    g = dict(ob_value=HX.mean(axis=1) + rng.standard_normal(P), ob_error=rng.uniform(0.5, 2.0, P), ob_assim=rng.random(P) < 0.95,
             ob_lat=rng.uniform(-85, 85, P), ob_lon=rng.uniform(0, 360, P), ob_radius=np.full(P, 500.0), grid_lat=glat,
             grid_lon=glon, loc="GC", shape=np.array([nvar, nlev, ny, nx, M]))
    plev = np.geomspace(1000.0, 10.0, nlev)
    lead = np.tile(np.log(plev), nvar)
    lead[3 * nlev] = np.nan                                    # e.g. a surface field kept in the 3-D state
    ov = np.log(rng.uniform(10.0, 1000.0, P))
    ov[::50] = np.nan
    oh = np.full(P, 1.0)
    starts = np.sort(rng.choice(N // 64, 48, replace=False)) * 64
    rows = (starts[:, None] + np.arange(64)[None, :]).reshape(-1)
    prior = np.concatenate([X.download_rows(int(s), int(s) + 64) for s in starts])
    ctx.set_vertical_localization(lead, ov, oh)
    try:
        Yp = ctx.to_device(HX)
        ym = ctx.empty((P,))
        ctx.form_perts(P, M, Yp, ym, Yp)
        diag = ctx.ensrf_cycle(N, M, P, X, X, ym, Yp, g["ob_value"], g["ob_error"], g["ob_assim"], **golden_kwargs(g))
        got = np.concatenate([X.download_rows(int(s), int(s) + 64) for s in starts])
    finally:
        ctx.set_vertical_localization(None)
        X.free()
    xbm, Xbp = orc.format_prior_state(prior, HX)
    xam, Xap, rdiag = vl.ensrf_update_vert(xbm, Xbp, len(rows), g["ob_value"], g["ob_error"], g["ob_assim"], g["ob_lat"], g["ob_lon"],
                                           g["ob_radius"], glat, glon, (nvar, nlev, ny, nx), lead_vert=lead, ob_vert=ov,
                                           ob_vert_halfwidth=oh, rows=rows, obs_taper="vector")
    ref = orc.format_posterior_state(xam, Xap, len(rows))
    assert_parity(got, ref, "configs[2] sampled rows")
    assert_parity(diag["post_mean"], rdiag["post_mean"], "configs[2] post_mean")
    assert not np.array_equal(got, prior)
