"""The LETKF's deterministic control analysis on the MI355X against the NumPy model of tests/_letkf_control.py:
x_c^a and y_c^a to 1e-10 of each array's largest magnitude (cond(A) <= 1e4 asserted from the model) at the sizes where the Gram's
tile side grows (15, 31, 127 members) and where LDS is tight (136), the ensemble's bits with and without the control, the edge rules
of the issue one by one, the slab and inflation flavours, the refusals, and the classes.  Every test clears the setting."""
import ctypes
import functools

import numpy as np
import pytest

import _etkf as ek
import _letkf as lk
import _letkf_control as lc
import _letkf_slab as ls
from _letkf_gpu import TOL, COND_CAP, _reset, _obs_block, _close, _same_bits

pytestmark = pytest.mark.gpu

SIZES = [(2, 1, 3, 5, 1), (3, 5, 3, 5, 2), (15, 40, 4, 5, 3), (16, 64, 5, 7, 3), (17, 33, 5, 7, 3), (31, 64, 4, 5, 2),
         (40, 400, 6, 7, 3), (80, 700, 6, 7, 2), (127, 300, 3, 6, 1), (136, 300, 3, 6, 1)]
MID = (16, 64, 5, 7, 3)
SHORT = dict(hw=(100.0, 400.0))     # with MID: 3 of the 35 columns are out of every ob's reach
SENTINEL = -7.25
LOWER, UPPER = 1e-2, 1e2


@pytest.fixture
def ctx():
    from efa_xray_amd import _lib
    c = _reset(_lib.get_context(0))
    c.set_letkf_inflation(None)
    c.set_letkf_control(None)
    yield c
    c.set_letkf_control(None)
    c.set_letkf_inflation(None)
    _reset(c)


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _case(M, P, ny, nx, n_lead, hw=(300.0, 3000.0)):
    """The seeded case of tests/_letkf.py with the seeded control of tests/_letkf_control.py; computed once, left unchanged."""
    c = lk.make_case(M, P, ny, nx, n_lead, hw=hw)
    xc, yc = lc.control_inputs(c)
    c.update(xc=xc, yc=yc)
    return _freeze(c)


def _run_model(c, tapers=None, assim=None, **over):
    g = dict(c, **over)
    a = g["assim"] if assim is None else assim
    tapers = lc.plain_tapers(g, a) if tapers is None else tapers
    return lc.control_cycle(g["X"], g["HX"], g["xc"], g["yc"], g["value"], g["error"], a, *tapers, lam=g.get("lam"),
                            ob_infl=g.get("ob_infl"))


@functools.lru_cache(maxsize=None)
def _model(M, P, ny, nx, n_lead, hw=(300.0, 3000.0)):
    return _run_model(_case(M, P, ny, nx, n_lead, hw))


def _cycle(ctx, c, control=True, in_place=False, ctl_in_place=False, f32=False, slab=False, ngroups=1, lam=None, ob_infl=None,
           sigma_b=0.04, X=None, **over):
    """One cycle through the plain or the slab entry, with the control of the case (or of `over`) set or not: the ensemble's
    outputs, and xc_post / yc_post (pre-filled with a sentinel out of place)."""
    g = dict(c, **over)
    X = g["X"] if X is None else X
    N, M = X.shape
    P = g["P"]
    dt = np.float32 if f32 else np.float64
    Xd = ctx.to_device(np.ascontiguousarray(X, dtype=dt), dtype=dt)
    post = Xd if in_place else ctx.to_device(np.full((N, M), SENTINEL, dtype=dt), dtype=dt)
    ym, Yp, ym0, Yp0 = _obs_block(ctx, g["HX"], M)
    stats = ctx.empty((ngroups * g["ncol"], 3))
    fld = ist = obd = None
    xcd = xcp = ycd = ycp = None
    try:
        if lam is not None:
            fld = ctx.to_device(np.ascontiguousarray(lam, dtype=np.float64).reshape(-1))
            obd = None if ob_infl is None or not P else ctx.to_device(np.ascontiguousarray(ob_infl, dtype=np.float64))
            ist = ctx.to_device(np.full((fld.shape[0], 4), SENTINEL))
            ctx.set_letkf_inflation(fld, obd, P, sigma_b, LOWER, UPPER, ist)
        if control:
            xcd = ctx.to_device(np.ascontiguousarray(g["xc"], dtype=np.float64))
            xcp = xcd if ctl_in_place else ctx.to_device(np.full(N, SENTINEL))
            if P:
                ycd = ctx.to_device(np.ascontiguousarray(g["yc"], dtype=np.float64))
                ycp = ctx.to_device(np.full(P, SENTINEL))
            ctx.set_letkf_control(xcd, xcp, ycd, ycp)
        diag = ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"],
                               g["grid_lat"], g["grid_lon"], g["n_lead"], obs_block_out=True, col_stats=stats, f32=f32, _slab=slab)
    finally:
        ctx.set_letkf_control(None)
        ctx.set_letkf_inflation(None)
    out = dict(post=post.download(), ym=ym.download()[:P], Yp=Yp.download()[:P], diag=diag, stats=stats.download(), ym0=ym0, Yp0=Yp0,
               lam_a=None if fld is None else fld.download(), istats=None if ist is None else ist.download())
    if control:
        out.update(xc_post=xcp.download(), yc_post=ycp.download() if P else np.zeros(0))
    return out


def _rows(c, cols):
    return (np.flatnonzero(cols)[None, :] + c["ncol"] * np.arange(c["n_lead"])[:, None]).reshape(-1)


def _same_ensemble(on, off, what):
    _same_bits(on, off, what)
    if off["lam_a"] is not None:
        assert np.array_equal(on["lam_a"], off["lam_a"]), what + ": the inflation field differs"
        assert np.array_equal(on["istats"], off["istats"], equal_nan=True), what + ": the inflation statistics differ"


@functools.lru_cache(maxsize=None)
def _device(M, P, ny, nx, n_lead):
    """The parity case on the device with and without the control, once for the tests that read it."""
    from efa_xray_amd import _lib
    ctx = _reset(_lib.get_context(0))
    ctx.set_letkf_inflation(None)
    c = _case(M, P, ny, nx, n_lead)
    return _cycle(ctx, c), _cycle(ctx, c, control=False)


# ---- parity -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead", SIZES)
def test_control_analysis_matches_the_model(ctx, M, P, ny, nx, n_lead):
    c, ref = _case(M, P, ny, nx, n_lead), _model(M, P, ny, nx, n_lead)
    what = "M=%d P=%d" % (M, P)
    print("%s: cond(A) max %.3g, %d of %d columns reached" % (what, ref["cond"], ref["reached"].sum(), ref["reached"].size))
    assert ref["cond"] <= COND_CAP
    if (M, P) == (2, 1):
        assert (~ref["reached"]).sum() == 1, "the case: one unreached column"
    r, _ = _device(M, P, ny, nx, n_lead)
    _close(r["xc_post"], ref["xc_post"], what + " x_c^a")
    a = np.asarray(r["diag"]["assimilated"], bool)
    assert np.array_equal(a, c["assim"])
    _close(r["yc_post"][a], ref["yc_post"][a], what + " y_c^a")
    assert np.any(r["xc_post"] != c["xc"])


# ---- 1. float32 rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead", [(16, 64, 5, 7, 3), (40, 400, 6, 7, 3)])
def test_float32_rows_have_the_bits_of_the_float64_entry_on_the_widened_input(ctx, M, P, ny, nx, n_lead):
    c = _case(M, P, ny, nx, n_lead)
    X32 = np.ascontiguousarray(c["X"], dtype=np.float32)
    r32 = _cycle(ctx, c, f32=True, X=X32)
    r64 = _cycle(ctx, c, X=X32.astype(np.float64))
    assert r32["post"].dtype == np.float32
    assert np.array_equal(r32["xc_post"], r64["xc_post"]) and np.array_equal(r32["yc_post"], r64["yc_post"])
    assert np.array_equal(r32["post"], r64["post"].astype(np.float32))
    assert np.any(r32["xc_post"] != c["xc"]) and np.all(np.isfinite(r32["xc_post"]))


# ---- 2. edge rule 1: the ensemble is untouched ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead", SIZES)
def test_the_ensemble_keeps_its_bits(ctx, M, P, ny, nx, n_lead):
    on, off = _device(M, P, ny, nx, n_lead)
    _same_ensemble(on, off, "M=%d P=%d" % (M, P))


@pytest.mark.parametrize("f32", [False, True])
def test_the_ensemble_keeps_its_bits_under_a_non_finite_control_and_an_inflation_field(ctx, f32):
    c = _case(*MID)
    rng = np.random.default_rng(77)
    lam, ob_infl = rng.uniform(0.8, 1.6, c["ncol"]), rng.uniform(0.8, 1.6, c["P"])
    xc, yc = np.array(c["xc"]), np.array(c["yc"])
    xc[::7], xc[3::11] = np.nan, np.inf
    k = np.flatnonzero(c["assim"])
    yc[k[0]], yc[k[1]], yc[k[2]] = np.nan, np.inf, -np.inf
    off = _cycle(ctx, c, control=False, f32=f32, lam=lam, ob_infl=ob_infl)
    for what, over in (("finite", {}), ("non-finite", dict(xc=xc, yc=yc))):
        on = _cycle(ctx, c, f32=f32, lam=lam, ob_infl=ob_infl, **over)
        _same_ensemble(on, off, "%s control, f32=%s" % (what, f32))
    assert np.any(off["lam_a"] != lam) and not np.all(np.isfinite(on["xc_post"]))


# ---- 3. edge rule 2: relaxation does not reach the control ----------------------------------------------------------------------------
def test_relaxation_does_not_reach_the_control(ctx):
    from efa_xray_amd import _lib
    c = _case(*MID)
    plain = _cycle(ctx, c)
    for kind, alpha in ((_lib.RELAX_RTPS, 0.9), (_lib.RELAX_RTPP, 0.5)):
        ctx.set_relaxation(kind, alpha)
        r = _cycle(ctx, c)
        ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
        assert not np.array_equal(r["post"], plain["post"]), "the relaxation acted on the members"
        assert np.array_equal(r["xc_post"], plain["xc_post"]) and np.array_equal(r["yc_post"], plain["yc_post"])


# ---- 4. edge rule 3: unreached columns and ob positions ---------------------------------------------------------------------------------
def test_unreached_columns_keep_the_control_bit_for_bit(ctx):
    c, ref = _case(*MID, **SHORT), _model(*MID, **SHORT)
    reached = ref["reached"][0]
    assert (~reached).sum() == 3 and reached.size == 35
    un, re = _rows(c, ~reached), _rows(c, reached)
    for ctl_in_place in (False, True):
        r = _cycle(ctx, c, ctl_in_place=ctl_in_place, in_place=ctl_in_place)
        assert np.array_equal(r["xc_post"][un], c["xc"][un]), "an unreached column's control rows changed"
        _close(r["xc_post"][re], ref["xc_post"][re], "reached columns")
        assert np.any(r["xc_post"][re] != c["xc"][re])
        lone = ~ref["ob_reached"]
        assert np.array_equal(r["yc_post"][lone], c["yc"][lone]), "y_c^a of an ob position no ob reaches"
    # an ob position no ob reaches: every ob unflagged but one that is far from ob 0's position
    far = int(np.argmax(np.abs(c["ob_lat"] - c["ob_lat"][0]) + np.abs(c["ob_lon"] - c["ob_lon"][0])))
    assim = np.zeros(c["P"], dtype=bool)
    assim[far] = True
    ref1 = _run_model(c, assim=assim)
    assert not ref1["ob_reached"][0] and ref1["ob_reached"][far]
    r = _cycle(ctx, c, assim=assim)
    lone = ~ref1["ob_reached"]
    assert np.array_equal(r["yc_post"][lone], c["yc"][lone]) and r["yc_post"][far] != c["yc"][far]


# ---- 5. edge rule 4: NaN ---------------------------------------------------------------------------------------------------------------
def test_a_nan_estimate_poisons_exactly_the_columns_it_reaches(ctx):
    c = _case(*MID, **SHORT)
    rho = lc.plain_tapers(c)[0][0]
    k = int(np.argmax((rho != 0.0).sum(axis=0)))
    hit = rho[:, k] != 0.0
    assert hit.any() and not hit.all() and c["assim"][k]
    yc = np.array(c["yc"])
    yc[k] = np.nan
    fin = _cycle(ctx, c)
    r = _cycle(ctx, c, yc=yc)
    assert np.all(np.isnan(r["xc_post"][_rows(c, hit)])), "a column the NaN reaches kept a finite control row"
    clean = _rows(c, ~hit)
    assert np.array_equal(r["xc_post"][clean], fin["xc_post"][clean]), "a column the NaN does not reach changed"
    rho_o = lc.plain_tapers(c)[2]
    far = rho_o[:, k] == 0.0
    assert np.array_equal(r["yc_post"][far], fin["yc_post"][far]) and np.all(np.isnan(r["yc_post"][~far & (rho_o != 0.0).any(axis=1)]))
    _same_bits(r, fin, "the ensemble under the NaN")


def test_an_ob_that_is_not_assimilated_is_never_read(ctx):
    c = _case(*MID)
    off = ~c["assim"]
    assert off.any()
    value, error, yc = np.array(c["value"]), np.array(c["error"]), np.array(c["yc"])
    value[off], error[off], yc[off] = np.nan, np.nan, np.nan
    fin = _cycle(ctx, c)
    r = _cycle(ctx, c, value=value, error=error, yc=yc)
    assert np.array_equal(r["xc_post"], fin["xc_post"]) and np.all(np.isfinite(r["xc_post"]))
    a = c["assim"]
    assert np.array_equal(r["yc_post"][a], fin["yc_post"][a])


# ---- 6. edge rule 6: a control equal to the ensemble mean ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead", [(16, 64, 5, 7, 3), (127, 300, 3, 6, 1)])
def test_a_control_equal_to_the_mean_gives_the_posterior_mean(ctx, M, P, ny, nx, n_lead):
    c = _case(M, P, ny, nx, n_lead)
    ym0 = ek.ob_priors(c["HX"])[0]
    r = _cycle(ctx, c, xc=c["X"].mean(axis=1), yc=ym0)
    _close(r["xc_post"], r["post"].mean(axis=1), "x_c^a against the posterior members' mean")
    a = np.asarray(r["diag"]["assimilated"], bool)
    _close(r["yc_post"][a], np.asarray(r["diag"]["post_mean"])[a], "y_c^a against post_mean")
    _close(r["yc_post"], r["ym"], "y_c^a against the posterior obs means")


# ---- 7. edge rule 5: same inputs, same bits ------------------------------------------------------------------------------------------------
def test_same_bits_twice_and_in_place(ctx):
    c = _case(40, 400, 6, 7, 3)
    a, b = _cycle(ctx, c), _cycle(ctx, c)
    assert np.array_equal(a["xc_post"], b["xc_post"]) and np.array_equal(a["yc_post"], b["yc_post"])
    _same_bits(a, b, "twice")
    ip = _cycle(ctx, c, ctl_in_place=True, in_place=True)
    assert np.array_equal(ip["xc_post"], a["xc_post"]) and np.array_equal(ip["yc_post"], a["yc_post"])
    _same_bits(ip, a, "in place")


# ---- 8. the outlier check is the ensemble's ----------------------------------------------------------------------------------------------
def test_the_control_never_votes_in_the_outlier_check(ctx):
    c = _case(*MID)
    ctx.set_outlier_threshold(1.0)
    try:
        off = _cycle(ctx, c, control=False)
        yc = np.array(c["yc"]) + 1e6        # by its own innovations the control would reject every ob
        on = _cycle(ctx, c, yc=yc)
    finally:
        ctx.set_outlier_threshold(None)
    flags = np.asarray(off["diag"]["assimilated"], bool)
    assert 0 < flags.sum() < c["assim"].sum(), "the case: the ensemble rejects some of the requested obs, not all"
    assert np.array_equal(np.asarray(on["diag"]["assimilated"], bool), flags)
    _same_bits(on, off, "under the outlier check")
    ref = _run_model(c, assim=flags, yc=yc)
    assert ref["cond"] <= COND_CAP
    _close(on["xc_post"], ref["xc_post"], "x_c^a under the ensemble's flags")
    _close(on["yc_post"][flags], ref["yc_post"][flags], "y_c^a under the ensemble's flags")


# ---- 9. slab groups ------------------------------------------------------------------------------------------------------------------------
def _slab_on(ctx, c):
    loc, n_lead, P = c["loc"], c["n_lead"], c["P"]
    ctx.set_vertical_localization(loc["lead_vert"], loc["ob_vert"], loc["ob_vert_halfwidth"])
    ctx.set_slab_localization(n_lead, P, **{k: loc.get(k) for k in ("lead_time", "ob_time", "ob_time_halfwidth", "lead_var", "ob_group",
                                                                    "ob_var", "impact")})
    return ctx.letkf_slab_groups(n_lead)


def test_slab_groups_solve_the_control_under_their_own_tapers(ctx):
    M, P, ny, nx, nvars, ntimes = 16, 64, 5, 7, 2, 3
    c = ls.make_case(M, P, ny, nx, nvars, ntimes, parts="vtc")
    xc, yc = lc.control_inputs(c)
    c.update(xc=xc, yc=yc)
    group_of, ng = _slab_on(ctx, c)
    tapers = lc.slab_tapers(c)
    assert ng == tapers[0].shape[0] >= 2 and np.array_equal(group_of, tapers[1])
    ref = _run_model(c, tapers=tapers)
    assert ref["cond"] <= COND_CAP and ref["reached"].any()
    on = _cycle(ctx, c, slab=True, ngroups=ng)
    off = _cycle(ctx, c, control=False, slab=True, ngroups=ng)
    assert ctx.get_option("phase_a_kind") == 8
    _close(on["xc_post"], ref["xc_post"], "slab x_c^a")
    a = c["assim"]
    _close(on["yc_post"][a], ref["yc_post"][a], "slab y_c^a")
    _same_bits(on, off, "the ensemble under the slab call")
    plain = lc.control_cycle(c["X"], c["HX"], xc, yc, c["value"], c["error"], a, *lc.plain_tapers(c))
    assert np.abs(plain["xc_post"] - ref["xc_post"]).max() > 1e-6, "the case: the slab factors matter"


# ---- 10. under an inflation field ---------------------------------------------------------------------------------------------------------
def test_the_control_is_solved_under_the_inflation_field(ctx):
    c = _case(17, 33, 5, 7, 3)
    rng = np.random.default_rng(977)
    lam, ob_infl = rng.uniform(0.8, 1.6, c["ncol"]), rng.uniform(0.8, 1.6, c["P"])
    ref = _run_model(c, lam=lam[None], ob_infl=ob_infl)
    assert ref["cond"] <= COND_CAP
    on = _cycle(ctx, c, lam=lam, ob_infl=ob_infl, sigma_b=0.04)
    off = _cycle(ctx, c, control=False, lam=lam, ob_infl=ob_infl, sigma_b=0.04)
    _close(on["xc_post"], ref["xc_post"], "x_c^a under the field")
    a = c["assim"]
    _close(on["yc_post"][a], ref["yc_post"][a], "y_c^a under the ob factors")
    _same_ensemble(on, off, "under the field")
    assert np.any(on["lam_a"] != lam), "the field is estimated"
    flat = _model(17, 33, 5, 7, 3)
    assert np.abs(flat["xc_post"] - ref["xc_post"]).max() > 1e-6, "the case: the field matters"


# ---- 11. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_usable(ctx):
    from efa_xray_amd import _lib
    c = _case(*MID)
    want = _cycle(ctx, c)
    N, M = c["X"].shape
    P = c["P"]
    args = (c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"], c["grid_lon"], c["n_lead"])
    shape = dict(shape=(c["ny"], c["nx"]), stride=(2, 3))

    def served(what):
        r = _cycle(ctx, c)
        assert np.array_equal(r["xc_post"], want["xc_post"]) and np.array_equal(r["yc_post"], want["yc_post"]), what
        _same_bits(r, want, what)

    def refused(call, word):
        with pytest.raises(_lib.EfaError) as e:
            call()
        assert e.value.status == _lib.EFA_ERR_INVALID and word in str(e.value), str(e.value)

    Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
    X32 = ctx.to_device(np.ascontiguousarray(c["X"], dtype=np.float32), dtype=np.float32)
    post = ctx.to_device(np.full((N, M), SENTINEL))
    post32 = ctx.to_device(np.full((N, M), SENTINEL, dtype=np.float32), dtype=np.float32)
    ym, Yp, ym0, Yp0 = _obs_block(ctx, c["HX"], M)
    xcd, ycd = ctx.to_device(np.array(c["xc"])), ctx.to_device(np.array(c["yc"]))
    xcp, ycp = ctx.to_device(np.full(N, SENTINEL)), ctx.to_device(np.full(P, SENTINEL))
    xc_long, yc_long = ctx.to_device(np.zeros(N + 1)), ctx.to_device(np.zeros(P + 1))
    xcp_long, ycp_long = ctx.to_device(np.full(N + 1, SENTINEL)), ctx.to_device(np.full(P + 1, SENTINEL))

    def untouched():
        assert np.all(post.download() == SENTINEL) and np.all(post32.download() == SENTINEL)
        for a in (xcp, ycp, xcp_long, ycp_long):
            assert np.all(a.download() == SENTINEL)
        assert np.array_equal(ym.download()[:P], ym0) and np.array_equal(Yp.download()[:P], Yp0)

    try:
        # rows or P that differ from the call's
        ctx.set_letkf_control(xc_long, xcp_long, ycd, ycp)
        refused(lambda: ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, *args, obs_block_out=True), "rows")
        untouched()
        served("after a control sized for other rows")
        ctx.set_letkf_control(xcd, xcp, yc_long, ycp_long)
        refused(lambda: ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, *args, obs_block_out=True), "observations")
        refused(lambda: ctx.letkf_cycle(N, M, P, X32, post32, ym, Yp, *args, obs_block_out=True, f32=True), "observations")
        untouched()
        served("after a control sized for another P")
        # a partial overlap of xc_post with xc (and any overlap of yc_post with yc): the setter refuses, the setting stays off
        ctx.set_letkf_control(None)
        lib, h = ctx.lib, ctx.handle
        shifted = ctypes.c_void_p(xc_long.ptr.value + 8)
        assert lib.efa_ctx_set_letkf_control(h, xc_long.ptr, shifted, N, ycd.ptr, ycp.ptr, P) == _lib.EFA_ERR_INVALID
        assert lib.efa_ctx_set_letkf_control(h, xcd.ptr, xcp.ptr, N, ycd.ptr, ycd.ptr, P) == _lib.EFA_ERR_INVALID
        assert lib.efa_ctx_set_letkf_control(h, xcd.ptr, xcp.ptr, -1, ycd.ptr, ycp.ptr, P) == _lib.EFA_ERR_INVALID
        assert lib.efa_ctx_set_letkf_control(h, xcd.ptr, None, N, ycd.ptr, ycp.ptr, P) == _lib.EFA_ERR_INVALID
        served("after the setter's refusals")
        # the entries whose pairs have no place for w^c
        ctx.set_letkf_control(xcd, xcp, ycd, ycp)
        refused(lambda: ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, *args, obs_block_out=True, **shape), "control")
        refused(lambda: ctx.letkf_cycle(N, M, P, X32, post32, ym, Yp, *args, obs_block_out=True, f32=True, **shape), "control")
        refused(lambda: ctx.letkf_weights(M, P, ym, Yp, *args[:6], c["grid_lat"], c["grid_lon"]), "control")
        untouched()
        served("after the interp and weights refusals")
        cs = ls.make_case(M, P, c["ny"], c["nx"], 1, 3, parts="v")
        assert cs["n_lead"] == c["n_lead"]
        _slab_on(ctx, cs)
        ctx.set_letkf_control(xcd, xcp, ycd, ycp)
        refused(lambda: ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, *args, obs_block_out=True, _slab=True, **shape), "control")
        refused(lambda: ctx.letkf_cycle(N, M, P, X32, post32, ym, Yp, *args, obs_block_out=True, f32=True, _slab=True, **shape), "control")
        refused(lambda: ctx.letkf_slab_weights(M, P, ym, Yp, *args[:6], c["grid_lat"], c["grid_lon"], c["n_lead"]), "control")
        untouched()
        ctx.set_vertical_localization(None)
        ctx.set_slab_localization(None)
        served("after the slab interp and weights refusals")
        # efa_letkf_interp_apply_dev takes no obs and ignores the setting
        ctx.set_letkf_control(xcd, xcp, ycd, ycp)
        nodes = 3 * 3
        Tw = np.zeros((nodes, M, M + 1))
        Tw[:, np.arange(M), np.arange(M)] = 1.0
        ctx.letkf_interp_apply(N, M, Xd, post, (c["ny"], c["nx"]), (2, 3), c["n_lead"], ctx.to_device(Tw))
        assert np.allclose(post.download(), c["X"], rtol=1e-12, atol=1e-12), "the identity pairs were applied"
        assert np.all(xcp.download() == SENTINEL) and np.all(ycp.download() == SENTINEL)
    finally:
        ctx.set_letkf_control(None)
        ctx.set_vertical_localization(None)
        ctx.set_slab_localization(None)
    served("at the end")


def test_the_serial_and_etkf_entries_ignore_the_setting(ctx):
    from efa_xray_amd import _lib
    c = _case(*MID)
    N, M = c["X"].shape

    def calls():
        out = []
        for solver, loc in ((0, True), (1, False)):
            ctx.set_option("obs_solver", solver)
            Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
            ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
            geo = (_lib.LOC_GC, c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"], c["grid_lon"], c["n_lead"]) if loc else ()
            d = ctx.ensrf_cycle(N, M, c["P"], Xd, Xd, ym, Yp, c["value"], c["error"], c["assim"], *geo, obs_block_out=True)
            out.append((Xd.download(), Yp.download(), np.asarray(d["post_mean"])))
        ctx.set_option("obs_solver", 0)
        return out

    off = calls()
    xcd, ycd = ctx.to_device(np.array(c["xc"])), ctx.to_device(np.array(c["yc"]))
    xcp, ycp = ctx.to_device(np.full(N, SENTINEL)), ctx.to_device(np.full(c["P"], SENTINEL))
    try:
        ctx.set_letkf_control(xcd, xcp, ycd, ycp)
        on = calls()
    finally:
        ctx.set_letkf_control(None)
    for a, b in zip(on, off):
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)), "a serial / ETKF call changed under the setting"
    assert np.all(xcp.download() == SENTINEL) and np.all(ycp.download() == SENTINEL)


# ---- 12. the classes ---------------------------------------------------------------------------------------------------------------------
def _api_case(seed=11):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(seed)
    nvar, nt, ny, nx, M, P = 2, 2, 6, 7, 12, 30
    lat, lon = np.meshgrid(np.linspace(20, 60, ny), np.linspace(200, 280, nx), indexing="ij")
    arr = rng.standard_normal((nvar, nt, ny, nx, 1)) + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon)
    ctrl = EnsembleState.from_array(arr.mean(axis=-1, keepdims=True) + 0.5 * rng.standard_normal((nvar, nt, ny, nx, 1)), lat, lon)
    rows = rng.choice(state.nstate(), P, replace=False)

    class RowOb(Observation):
        def estimate(self, st):
            return st.to_vect()[self.row].copy()

    X = state.to_vect().astype(np.float64)
    obs = []
    for k in range(P):
        col = rows[k] % (ny * nx)
        ob = RowOb(value=float(X[rows[k]].mean() + rng.standard_normal()), error=float(rng.uniform(0.5, 2.0)),
                   lat=float(lat.reshape(-1)[col]), lon=float(lon.reshape(-1)[col]), assimilate_this=(k % 7 != 3),
                   localize_radius=float(rng.uniform(400.0, 1500.0)))
        ob.row = int(rows[k])
        ob.vert, ob.vert_localize_radius = float(rng.choice([850.0, 500.0])), float(rng.uniform(150.0, 600.0))
        obs.append(ob)
    return state, ctrl, obs, lat, lon, rows


@pytest.mark.parametrize("flavour", ["plain", "slab", "rtps_f32", "inflated"])
def test_the_classes_carry_the_control(ctx, flavour):
    from efa_xray_amd import LETKF, SlabLETKF
    state, ctrl, obs, lat, lon, rows = _api_case()
    state_off, _, obs_off, _, _, _ = _api_case()
    cls, kw = LETKF, {}
    vert = np.array([[850.0] * 2, [500.0] * 2])
    if flavour == "slab":
        cls, kw = SlabLETKF, dict(vert_coord=vert)
    if flavour == "rtps_f32":
        state, state_off, kw = state.astype(np.float32), state_off.astype(np.float32), dict(rtps=0.9)
    if flavour == "inflated":      # the constant hook scales the ensemble's perturbations (of the caller's state, in place) only
        kw = dict(inflation=1.2)
    xc = ctrl.to_vect()[:, 0].astype(np.float64)
    xc_before = xc.copy()
    f = cls(state, obs, verbose=False, control=ctrl, **kw)
    post, obs_out = f.update()
    post_off, _ = cls(state_off, obs_off, verbose=False, **kw).update()
    X = state.to_vect().astype(np.float64)      # the prior the filter saw
    assert np.array_equal(post.to_vect(), post_off.to_vect()), "the return value changed under the control"
    for a, b in zip(obs_out, obs_off):
        assert a.assimilated == b.assimilated and a.prior_mean == b.prior_mean and a.prior_var == b.prior_var
        assert (a.post_mean == b.post_mean and a.post_var == b.post_var) if a.assimilated else True
    lcn = f.last_control
    assert set(lcn) == {"state", "ob_prior", "ob_post"}
    P = len(obs)
    assert lcn["state"] is not ctrl and lcn["state"].nmems() == 1 and lcn["state"].vars() == ctrl.vars()
    assert np.array_equal(ctrl.to_vect()[:, 0], xc_before), "the control passed in was changed"
    assert lcn["ob_prior"].shape == (P,) and lcn["ob_post"].shape == (P,)
    assert np.array_equal(lcn["ob_prior"], xc[rows]), "H(x_c) of the user-defined operators: ob.estimate(ctrl)"
    asm = np.array([o.assimilate_this for o in obs])
    assert np.all(np.isnan(lcn["ob_post"][~asm])) and np.all(np.isfinite(lcn["ob_post"][asm]))
    HX = X[rows]
    c = dict(X=X, HX=HX, P=P, M=X.shape[1], n_lead=4, ncol=42, grid_lat=lat, grid_lon=lon, assim=asm,
             value=np.array([o.value for o in obs]), error=np.array([o.error for o in obs]), ob_lat=np.array([o.lat for o in obs]),
             ob_lon=np.array([o.lon for o in obs]), ob_hw=np.array([o.localize_radius for o in obs]), xc=xc, yc=xc[rows])
    tapers = None
    if flavour == "slab":
        c["loc"] = dict(lead_vert=vert.reshape(-1), ob_vert=np.array([o.vert for o in obs]),
                        ob_vert_halfwidth=np.array([o.vert_localize_radius for o in obs]))
        tapers = lc.slab_tapers(c)
        assert tapers[0].shape[0] == 2
    ref = _run_model(c, tapers=tapers)
    assert ref["cond"] <= COND_CAP
    if flavour == "rtps_f32":
        assert state.dtype == np.float32 and post.dtype == np.float32
    _close(lcn["state"].to_vect()[:, 0], ref["xc_post"], flavour + ": last_control['state']")
    _close(lcn["ob_post"][asm], ref["yc_post"][asm], flavour + ": last_control['ob_post']")
    # the setting does not outlive the update
    s2, _, o2, _, _, _ = _api_case()
    f2 = cls(s2.astype(np.float32) if flavour == "rtps_f32" else s2, o2, verbose=False, **kw)
    p2, _ = f2.update()
    assert f2.last_control is None and np.array_equal(p2.to_vect(), post_off.to_vect())


def test_default_operator_obs_interpolate_the_control(ctx):
    from efa_xray_amd import EnsembleState, Observation, LETKF
    rng = np.random.default_rng(21)
    nvar, nt, ny, nx, M, P = 1, 1, 5, 6, 10, 12
    lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(230, 260, nx), indexing="ij")
    arr = rng.standard_normal((nvar, nt, ny, nx, 1)) + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon, validtime=np.array([0.0]))
    ctrl = EnsembleState.from_array(arr.mean(axis=-1, keepdims=True) + 0.5 * rng.standard_normal((nvar, nt, ny, nx, 1)), lat, lon,
                                    validtime=np.array([0.0]))
    name = state.vars()[0]
    obs = [Observation(value=float(rng.standard_normal()), error=float(rng.uniform(0.5, 2.0)), lat=float(rng.uniform(31, 49)),
                       lon=float(rng.uniform(231, 259)), obtype=name, time=0.0, assimilate_this=True,
                       localize_radius=float(rng.uniform(600.0, 1500.0))) for _ in range(P)]
    f = LETKF(state, obs, verbose=False, control=ctrl)
    HX = np.asarray(f.compute_ob_estimates(), dtype=np.float64)
    yc = np.array([np.asarray(o.estimate(ctrl)).reshape(-1)[0] for o in obs], dtype=np.float64)     # the reference's interpolation
    f.update()
    lcn = f.last_control
    assert np.abs(lcn["ob_prior"] - yc).max() <= 1e-12 * np.abs(yc).max(), "H(x_c): the stencils on the one-member rows"
    xc = ctrl.to_vect()[:, 0].astype(np.float64)
    c = dict(X=state.to_vect(), HX=HX, P=P, M=M, n_lead=1, ncol=ny * nx, grid_lat=lat, grid_lon=lon, assim=np.ones(P, dtype=bool),
             value=np.array([o.value for o in obs]), error=np.array([o.error for o in obs]), ob_lat=np.array([o.lat for o in obs]),
             ob_lon=np.array([o.lon for o in obs]), ob_hw=np.array([o.localize_radius for o in obs]), xc=xc, yc=lcn["ob_prior"])
    ref = _run_model(c)
    assert ref["cond"] <= COND_CAP
    _close(lcn["state"].to_vect()[:, 0], ref["xc_post"], "LETKF.update: the control analysis")
    _close(lcn["ob_post"], ref["yc_post"], "LETKF.update: the control's ob estimates")
