"""Per-column multiplicative inflation of the LETKF on the MI355X against the NumPy model of
tests/_letkf_infl.py: the pairs, the posterior and the obs block under a random field and random ob factors to 1e-10 of each
array's largest magnitude (cond(A) <= 1e4 asserted from the model), lambda_a and the four statistics to 1e-12, the bits of today's
call at a field of ones, the plain call on inflated inputs at a uniform field, points no ob reaches, poisoned and degenerate
inputs, clipping, the slab and interp flavours, the refusals, the serial entries' indifference, and the classes.  Every test
restores the shared context's settings."""
import functools

import numpy as np
import pytest

import _etkf as ek
import _letkf as lk
import _letkf_infl as lf
import _letkf_interp as li
import _letkf_slab as ls
from _letkf_gpu import TOL, COND_CAP, _reset, _obs_block, _close, _check_diag, _same_bits

pytestmark = pytest.mark.gpu

SIZES = [(2, 1, 3, 5, 1), (3, 5, 3, 5, 2), (17, 33, 5, 7, 3), (40, 400, 6, 7, 3), (136, 300, 3, 6, 1)]
MID = (17, 33, 5, 7, 3)
SHORT = (16, 40, 6, 7, 3)       # with hw 100..400 km: test_gpu_letkf.py's case that mixes reached and unreached columns in a block
LOWER, UPPER = 1e-2, 1e2
SENTINEL = -7.25


@pytest.fixture
def ctx():
    from efa_xray_amd import _lib
    c = _reset(_lib.get_context(0))
    c.set_letkf_inflation(None)
    yield c
    c.set_letkf_inflation(None)
    _reset(c)


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _case(M, P, ny, nx, n_lead, seed=0, hw=(300.0, 3000.0)):
    """The seeded case of tests/_letkf.py with a random field and random ob factors in [0.8, 1.6]; computed once, left unchanged."""
    c = lk.make_case(M, P, ny, nx, n_lead, seed=seed, hw=hw)
    rng = np.random.default_rng(977 * M + P + seed)
    c.update(lam=rng.uniform(0.8, 1.6, c["ncol"]), ob_infl=rng.uniform(0.8, 1.6, P))
    return _freeze(c)


def _run_model(c, sigma_b=0.04, **over):
    g = dict(c, **over)
    return lf.letkf_cycle(g["X"], g["HX"], g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"], g["grid_lat"],
                          g["grid_lon"], g["n_lead"], g["lam"], g["ob_infl"], sigma_b, LOWER, UPPER)


@functools.lru_cache(maxsize=None)
def _model(M, P, ny, nx, n_lead, seed=0, hw=(300.0, 3000.0)):
    return _run_model(_case(M, P, ny, nx, n_lead, seed, hw))


def _set(ctx, lam, P, ob_infl=None, sigma_b=0.04, lower=LOWER, upper=UPPER, stats=True):
    """The setting from host arrays: (field, stats) on the device, the statistics pre-filled with a sentinel.  The field keeps the
    ob factors' array alive: the context holds addresses only."""
    lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(-1)
    fld = ctx.to_device(lam)
    obd = None if ob_infl is None or not P else ctx.to_device(np.ascontiguousarray(ob_infl, dtype=np.float64))
    st = ctx.to_device(np.full((lam.size, 4), SENTINEL)) if stats else None
    ctx.set_letkf_inflation(fld, obd, P, sigma_b, lower, upper, st)
    fld.ob_infl = obd
    return fld, st


def _cycle(ctx, c, lam=None, ob_infl=None, sigma_b=0.04, in_place=False, f32=False, stride=None, slab=False, ngroups=1, X=None, **over):
    """One cycle through the plain, interp or slab entry, under the field `lam` (None: the setting off): posterior, obs block,
    diagnostics, column statistics, lam_a and the inflation statistics."""
    g = dict(c, **over)
    X = g["X"] if X is None else X
    N, M = X.shape
    P = g["P"]
    dt = np.float32 if f32 else np.float64
    Xd = ctx.to_device(np.ascontiguousarray(X, dtype=dt), dtype=dt)
    post = Xd if in_place else ctx.to_device(np.full((N, M), SENTINEL, dtype=dt), dtype=dt)
    ym, Yp, ym0, Yp0 = _obs_block(ctx, g["HX"], M)
    npts, mesh = g["ncol"], {}
    if stride is not None:
        npts = li.axis_nodes(g["ny"], stride[0]).size * li.axis_nodes(g["nx"], stride[1]).size
        mesh = dict(shape=(g["ny"], g["nx"]), stride=stride)
    stats = ctx.empty((ngroups * npts, 3))
    fld = ist = None
    if lam is not None:
        fld, ist = _set(ctx, lam, P, ob_infl, sigma_b)
    try:
        diag = ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"],
                               g["grid_lat"], g["grid_lon"], g["n_lead"], obs_block_out=True, col_stats=stats, f32=f32, _slab=slab, **mesh)
    finally:
        ctx.set_letkf_inflation(None)
        out = dict(post=post.download(), lam_a=None if fld is None else fld.download(), istats=None if ist is None else ist.download())
    out.update(ym=ym.download()[:P], Yp=Yp.download()[:P], diag=diag, stats=stats.download(), ym0=ym0, Yp0=Yp0)
    return out


def _probe(ctx, c, lam, sigma_b=0.0, lat=None, lon=None, **over):
    """efa_letkf_weights_dev at the grid's columns (or the given points) under the field: T, w, stats, lam_a, inflation statistics."""
    g = dict(c, **over)
    M, P = g["M"], g["P"]
    ym, Yp, _, _ = _obs_block(ctx, g["HX"], M)
    fld, ist = _set(ctx, lam, P, None, sigma_b)
    try:
        T, w, st = ctx.letkf_weights(M, P, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"],
                                     g["grid_lat"] if lat is None else lat, g["grid_lon"] if lon is None else lon)
    finally:
        ctx.set_letkf_inflation(None)
    return T, w, st, fld.download(), ist.download()


EPS_RHO = 1e-14     # absolute error granted to a taper the model and the device each evaluate on their own (below)


def _check_estimate(lam_a, istats, lam_b, ref_p, ref_lam_a, what, ref_q=None, sigma_b=0.04, eps=EPS_RHO):
    """lambda_a and {p1, p2, p3, lambda_o} against the model: the sums to 1e-12 relative (at most P <= 400 non-negative terms each:
    P u = 4.4e-14), lambda_a and lambda_o to 1e-12 (1 + (p1 + p3)/p2), the forward bound with a 20-fold margin; a point no ob
    reaches keeps its factor's bits and reports (0, 0, 0, NaN).
    ref_q (the model's q_i = sum_k |d p_i / d rho_k|) adds what the TAPERS' own rounding does, where a case has tapers at the edge
    of their support: model and device evaluate Gaspari-Cohn's fifth-order polynomial separately, its terms are of magnitude <= 5,
    so the two values differ by some tens of u in ABSOLUTE terms (1e-14 granted, 3e-14 for a product with the two slab factors),
    which is a large RELATIVE error of a taper of 1e-9 and of the sums of a point that only such tapers reach.  Then p_i may move
    by eps q_i, and lambda_o and lambda_a by what the estimate does over that box of (p1, p2, p3) (its eight corners; the estimate
    is monotone in each)."""
    reached = ref_p[:, 2] != 0.0
    p = ref_p[reached]
    dp = np.zeros((p.shape[0], 3)) if ref_q is None else eps * ref_q[reached]
    for i, name in enumerate(("p1", "p2", "p3")):
        err = np.abs(istats[reached, i] - p[:, i])
        print("%s %s: max err / bound %.3e" % (what, name, (err / (1e-12 * p[:, i] + dp[:, i])).max() if err.size else 0.0))
        assert np.all(err <= 1e-12 * p[:, i] + dp[:, i]), "%s: %s" % (what, name)
    bound = 1e-12 * (1.0 + (p[:, 0] + p[:, 2]) / p[:, 1])
    extra_a, extra_o = np.zeros(p.shape[0]), np.zeros(p.shape[0])
    if ref_q is not None:
        lb = lam_b[reached]
        for k in range(p.shape[0]):
            for sg in np.ndindex(2, 2, 2):
                q1, q2, q3 = p[k, :3] + (2.0 * np.array(sg) - 1.0) * dp[k]
                if q2 > 0.0 and q3 > 0.0:
                    extra_a[k] = max(extra_a[k], abs(lf.estimate(lb[k], q1, q2, q3, sigma_b, -np.inf, np.inf) -
                                                     lf.estimate(lb[k], p[k, 0], p[k, 1], p[k, 2], sigma_b, -np.inf, np.inf)))
                    extra_o[k] = max(extra_o[k], abs((q1 - q3) / q2 - p[k, 3]))
                else:
                    extra_a[k] = extra_o[k] = np.inf        # the box reaches p2 <= 0 or p3 <= 0: nothing can be said
    err = np.abs(lam_a[reached] - ref_lam_a[reached])
    print("%s lambda_a: max err / bound %.3e, range %.3f..%.3f" % (what, (err / (bound + extra_a)).max() if err.size else 0.0,
                                                                  lam_a.min(), lam_a.max()))
    assert np.all(err <= bound + extra_a), what + ": lambda_a"
    assert np.all(np.abs(istats[reached, 3] - p[:, 3]) <= bound + extra_o), what + ": lambda_o"    # (p1 - p3)/p2: the same bound
    assert np.array_equal(lam_a[~reached], lam_b[~reached]), what + ": an unreached point's factor changed"
    assert np.all(istats[~reached, :3] == 0.0) and np.all(np.isnan(istats[~reached, 3])), what + ": unreached statistics"


# ---- 1. probe and cycle against the model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead", SIZES)
def test_probe_and_cycle_match_the_model(ctx, M, P, ny, nx, n_lead):
    c, ref = _case(M, P, ny, nx, n_lead), _model(M, P, ny, nx, n_lead)
    st = ref["stats"]
    what = "M=%d P=%d" % (M, P)
    print("%s: cond(A) max %.3g, n_local %d..%d" % (what, st["cond"].max(), st["n_local"].min(), st["n_local"].max()))
    assert st["cond"].max() <= COND_CAP
    r = _cycle(ctx, c, c["lam"], c["ob_infl"])
    _close(r["post"], ref["post"], what + " posterior members")
    _close(r["Yp"], ref["Yp"], what + " posterior obs perturbations")
    _close(r["ym"], ref["ym"], what + " posterior obs means")
    _check_diag(r["diag"], ref["diag"], what)
    assert np.array_equal(r["stats"][:, 0], st["n_local"].astype(np.float64))
    assert np.abs(r["stats"][:, 1] - st["dfs"]).max() <= TOL * max(1.0, st["dfs"].max()), what + ": dfs"
    T, w, pst, lam_fixed, _ = _probe(ctx, c, c["lam"])
    _close(T, ref["T"], "T")
    _close(w, ref["w"], "w")
    assert np.array_equal(pst, r["stats"]) and np.array_equal(lam_fixed, c["lam"]), "sigma_b = 0: the field keeps its bits"


# ---- 2. lambda_a and the four statistics ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead", SIZES)
def test_estimate_and_statistics_match_the_model(ctx, M, P, ny, nx, n_lead):
    c, ref = _case(M, P, ny, nx, n_lead), _model(M, P, ny, nx, n_lead)
    r = _cycle(ctx, c, c["lam"], c["ob_infl"])
    _check_estimate(r["lam_a"], r["istats"], c["lam"], ref["stats"]["p"], ref["lam_a"], "cycle M=%d" % M)
    assert np.any(r["lam_a"] != c["lam"]) and np.all((r["lam_a"] >= LOWER) & (r["lam_a"] <= UPPER))
    _, _, _, lam_a, ist = _probe(ctx, c, c["lam"], sigma_b=0.04)
    assert np.array_equal(lam_a, r["lam_a"]) and np.array_equal(ist, r["istats"], equal_nan=True), "the probe runs the same solve"


# ---- 3. a field of ones has the bits of the call without the setting ---------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("rtps", [None, 0.9])
def test_a_field_of_ones_has_the_bits_of_the_plain_call(ctx, f32, rtps):
    from efa_xray_amd import _lib
    c = _case(*MID)
    if rtps:
        ctx.set_relaxation(_lib.RELAX_RTPS, rtps)
    want = _cycle(ctx, c, f32=f32)
    ones = np.ones(c["ncol"])
    r0 = _cycle(ctx, c, ones, None, sigma_b=0.0, f32=f32)
    _same_bits(r0, want, "sigma_b = 0")
    assert np.array_equal(r0["lam_a"], ones)
    r1 = _cycle(ctx, c, ones, np.ones(c["P"]), sigma_b=0.04, f32=f32)
    _same_bits(r1, want, "sigma_b = 0.04")
    assert np.any(r1["lam_a"] != 1.0), "... and the field is estimated"


# ---- 4. a uniform field is the plain call on inflated inputs ----------------------------------------------------------------------------
def test_a_uniform_field_equals_the_plain_call_on_inflated_inputs(ctx):
    c = _case(*MID)
    lam = 1.44
    r = _cycle(ctx, c, np.full(c["ncol"], lam), np.full(c["P"], lam), sigma_b=0.0)
    plain = _cycle(ctx, c, X=lf.inflate_rows(c["X"], lam), HX=lf.inflate_rows(c["HX"], lam))
    for k in ("post", "ym", "Yp"):
        _close(r[k], plain[k], "uniform 1.44: " + k, tol=2 * TOL)       # two device results, each within TOL
    assert np.array_equal(r["stats"][:, 0], plain["stats"][:, 0])


# ---- 5. points no ob reaches -------------------------------------------------------------------------------------------------------
def test_unreached_columns_keep_their_rows_and_their_factor(ctx):
    c = _case(*SHORT, hw=(100.0, 400.0))
    lam = np.full(c["ncol"], 1.3)
    ref = _run_model(c, lam=lam)
    reached = ref["stats"]["n_local"] > 0
    assert any(reached[b:b + 16].any() and not reached[b:b + 16].all() for b in range(0, c["ncol"], 16))
    rows = lambda cols: (np.asarray(cols)[None, :] + c["ncol"] * np.arange(c["n_lead"])[:, None]).reshape(-1)
    un, re = rows(np.flatnonzero(~reached)), rows(np.flatnonzero(reached))
    for in_place in (False, True):
        r = _cycle(ctx, c, lam, c["ob_infl"], in_place=in_place)
        assert np.array_equal(r["post"][un], c["X"][un]), "an unreached column's rows changed"
        assert np.array_equal(r["lam_a"][~reached], lam[~reached]), "an unreached column's factor changed"
        _close(r["post"][re], ref["post"][re], "reached columns")
        _check_estimate(r["lam_a"], r["istats"], lam, ref["stats"]["p"], ref["lam_a"], "short reach", ref["stats"]["q"])
    assert np.all(r["lam_a"][reached] != 1.3)


def test_no_obs_and_all_unflagged_leave_state_and_field_bit_for_bit(ctx):
    c = _case(*MID)
    none = dict(P=0, HX=np.zeros((0, c["M"])), value=np.zeros(0), error=np.zeros(0), assim=np.zeros(0, dtype=bool),
                ob_lat=np.zeros(0), ob_lon=np.zeros(0), ob_hw=np.zeros(0))
    for what, over, ob in (("P = 0", none, None), ("all unflagged", dict(assim=np.zeros(c["P"], dtype=bool)), c["ob_infl"])):
        for stride in (None, (2, 3)):
            n = c["ncol"] if stride is None else li.axis_nodes(c["ny"], stride[0]).size * li.axis_nodes(c["nx"], stride[1]).size
            lam = np.linspace(0.8, 1.6, n)
            r = _cycle(ctx, c, lam, ob, stride=stride, **over)
            assert np.array_equal(r["post"], c["X"]), what + ": the state changed"
            assert np.array_equal(r["lam_a"], lam), what + ": the field changed"
            assert np.all(r["stats"] == 0.0)


# ---- 6. poisoned and degenerate inputs -----------------------------------------------------------------------------------------------
def test_a_nan_value_leaves_the_field_of_the_columns_it_reaches(ctx):
    c = _case(*SHORT, hw=(100.0, 400.0))
    rho = lk.taper(c["grid_lat"], c["grid_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"])
    k = int(np.argmax((rho != 0.0).sum(axis=0)))
    hit = rho[:, k] != 0.0
    assert hit.any() and not hit.all() and c["assim"][k]
    value = np.array(c["value"])
    value[k] = np.nan
    ref = _run_model(c, value=value)
    r = _cycle(ctx, c, c["lam"], c["ob_infl"], value=value)
    assert np.array_equal(r["lam_a"][hit], c["lam"][hit]), "a column the NaN reaches changed its factor"
    assert np.all(np.isnan(r["istats"][hit, 0])) and np.all(np.isnan(r["istats"][hit, 3])), "p1 and lambda_o record the NaN"
    assert np.all(np.abs(r["istats"][hit, 1:3] - ref["stats"]["p"][hit, 1:3]) <=
                  1e-12 * ref["stats"]["p"][hit, 1:3] + EPS_RHO * ref["stats"]["q"][hit, 1:3])
    clean = ~hit
    _check_estimate(r["lam_a"][clean], r["istats"][clean], c["lam"][clean], ref["stats"]["p"][clean], ref["lam_a"][clean], "clean columns",
                    ref["stats"]["q"][clean])
    assert np.any(r["lam_a"][clean] != c["lam"][clean])
    rows = (np.flatnonzero(clean)[None, :] + c["ncol"] * np.arange(c["n_lead"])[:, None]).reshape(-1)
    _close(r["post"][rows], ref["post"][rows], "rows of the clean columns")


def test_all_zero_perturbations_leave_the_field_and_a_finite_posterior(ctx):
    c = _case(*MID)
    HX = np.repeat((np.arange(c["P"]) % 5).astype(np.float64)[:, None], c["M"], axis=1)     # exact means, exact zeros
    ref = _run_model(c, HX=HX)
    reached = ref["stats"]["n_local"] > 0
    assert reached.any() and np.all(ref["stats"]["p"][reached, 1] == 0.0)
    r = _cycle(ctx, c, c["lam"], c["ob_infl"], HX=HX)
    assert np.all(r["Yp0"] == 0.0)
    assert np.array_equal(r["lam_a"], c["lam"]), "p2 = 0: no estimate"
    assert np.all(r["istats"][reached, 1] == 0.0) and np.all(r["istats"][reached, 2] > 0.0)
    assert np.all(np.isfinite(r["post"]))
    _close(r["post"], ref["post"], "posterior under A = (M-1)/lambda I")


# ---- 7. clipping ---------------------------------------------------------------------------------------------------------------------
def test_the_estimate_is_clipped_to_the_bounds_exactly(ctx):
    c = _case(*MID, hw=(3000.0, 6000.0))
    ym0 = ek.ob_priors(c["HX"])[0]
    huge = _cycle(ctx, c, c["lam"], c["ob_infl"], sigma_b=10.0, value=ym0 + 1e6)
    assert np.all(huge["stats"][:, 0] > 0) and np.all(huge["lam_a"] == UPPER)
    zero = _cycle(ctx, c, c["lam"], c["ob_infl"], sigma_b=10.0, value=ym0)
    ref = _run_model(c, sigma_b=10.0, value=ym0)
    assert np.all(ref["lam_a"] == LOWER), "the case: every column's estimate lies below the lower bound"
    assert np.all(zero["lam_a"] == LOWER)


# ---- 8. slab and interp ------------------------------------------------------------------------------------------------------------
def test_slab_groups_carry_their_own_factors(ctx):
    M, P, ny, nx, nvars, ntimes = 16, 64, 5, 7, 2, 3
    c = ls.make_case(M, P, ny, nx, nvars, ntimes, parts="vtc")
    loc, n_lead, ncol = c["loc"], c["n_lead"], c["ncol"]
    ctx.set_vertical_localization(loc["lead_vert"], loc["ob_vert"], loc["ob_vert_halfwidth"])
    ctx.set_slab_localization(n_lead, P, **{k: loc.get(k) for k in ("lead_time", "ob_time", "ob_time_halfwidth", "lead_var", "ob_group",
                                                                    "ob_var", "impact")})
    group_of, ng = ctx.letkf_slab_groups(n_lead)
    S = ls.slab_table(n_lead, P, loc)
    ref_group_of, rep = ls.groups(n_lead, P, loc)
    assert ng == len(rep) >= 2 and np.array_equal(group_of, ref_group_of)
    rng = np.random.default_rng(5)
    lam, ob_infl = rng.uniform(0.8, 1.6, (ng, ncol)), rng.uniform(0.8, 1.6, P)
    ym, Yp = ek.ob_priors(c["HX"])
    rho_h = lk.taper(c["grid_lat"].reshape(-1), c["grid_lon"].reshape(-1), c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"])
    T, w = np.empty((ng, ncol, M, M)), np.empty((ng, ncol, M))
    p, q, lam_ref, nloc = np.empty((ng, ncol, 4)), np.empty((ng, ncol, 3)), np.empty((ng, ncol)), np.empty((ng, ncol))
    for g in range(ng):
        T[g], w[g], st, lam_ref[g] = lf.points(rho_h * S[:, rep[g]][None, :], lam[g], ym, Yp, c["value"], c["error"], c["assim"], 0.04,
                                               LOWER, UPPER)
        assert st["cond"].max() <= COND_CAP
        p[g], q[g], nloc[g] = st["p"], st["q"], st["n_local"]
    post = ls._apply(c["X"], ncol, ref_group_of, T, w, nloc > 0)
    rho_o = lk.taper(c["ob_lat"], c["ob_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"]) * ls.obs_factor(P, loc)
    yam, Yap = lf.obs_block(rho_o, ym, Yp, c["value"], c["error"], c["assim"], ob_infl)
    r = _cycle(ctx, c, lam, ob_infl, slab=True, ngroups=ng)
    _close(r["post"], post, "slab posterior members")
    _close(r["Yp"], Yap, "slab posterior obs perturbations")
    _close(r["ym"], yam, "slab posterior obs means")
    assert np.array_equal(r["stats"][:, 0].reshape(ng, ncol), nloc), "statistics and field are laid out [group][column]"
    _check_estimate(r["lam_a"], r["istats"], lam.reshape(-1), p.reshape(-1, 4), lam_ref.reshape(-1), "slab", q.reshape(-1, 3), eps=3 * EPS_RHO)


def test_interp_carries_the_field_at_the_nodes(ctx):
    c = _case(*MID)
    stride = (2, 3)
    m = li.mesh(c["ny"], c["nx"], stride)
    nn = m["node_col"].size
    assert nn == 3 * 3
    lam = np.random.default_rng(9).uniform(0.8, 1.6, nn)
    ym, Yp = ek.ob_priors(c["HX"])
    nlat, nlon = c["grid_lat"].reshape(-1)[m["node_col"]], c["grid_lon"].reshape(-1)[m["node_col"]]
    rho = lk.taper(nlat, nlon, c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"])
    Tn, wn, st, lam_ref = lf.points(rho, lam, ym, Yp, c["value"], c["error"], c["assim"], 0.04, LOWER, UPPER)
    assert st["cond"].max() <= COND_CAP
    Tc, wc, reached = li.column_pairs(m, Tn, wn, st["n_local"])
    post = li.apply_pairs(c["X"], c["ncol"], c["n_lead"], Tc, wc, reached)
    r = _cycle(ctx, c, lam, c["ob_infl"], stride=stride)
    assert ctx.get_option("phase_a_kind") == 7
    _close(r["post"], post, "interpolated posterior from the inflated node pairs")
    _check_estimate(r["lam_a"], r["istats"], lam, st["p"], lam_ref, "nodes", st["q"])
    _, _, pst, lam_probe, ist = _probe(ctx, c, lam, sigma_b=0.04, lat=nlat, lon=nlon)
    assert np.array_equal(lam_probe, r["lam_a"]) and np.array_equal(ist, r["istats"], equal_nan=True) and np.array_equal(pst, r["stats"])
    # the obs block does not depend on the mesh
    full = _cycle(ctx, c, c["lam"], c["ob_infl"])
    assert np.array_equal(full["Yp"], r["Yp"]) and np.array_equal(full["ym"], r["ym"])


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_context_usable(ctx):
    from efa_xray_amd import _lib
    c = _case(*MID)
    want = _cycle(ctx, c)
    ncol, P = c["ncol"], c["P"]
    good, good_ob = np.array(c["lam"]), np.array(c["ob_infl"])

    def bad(a, i, v):
        a = np.array(a)
        a[i] = v
        return a

    cases = [("solve points", np.ones(ncol + 1), good_ob, {}), ("solve points", np.ones(ncol - 1), None, {}),
             ("field", bad(good, 3, 0.0), good_ob, {}), ("field", bad(good, ncol - 1, np.nan), None, {}),
             ("field", bad(good, 0, UPPER * 2), good_ob, {}), ("field", bad(good, 5, np.inf), None, {}),
             ("observation", good, bad(good_ob, 2, np.nan), {}), ("observation", good, bad(good_ob, P - 1, LOWER / 2), {}),
             ("observation", good, bad(good_ob, 0, UPPER * 2), {}), ("solve points", good, good_ob, dict(stride=(2, 3)))]
    for word, lam, ob, kw in cases:
        with pytest.raises(_lib.EfaError) as e:
            _cycle(ctx, c, lam, ob, **kw)
        assert e.value.status == _lib.EFA_ERR_INVALID and word in str(e.value), str(e.value)
    # nothing is written: the posterior buffer, the obs block, the field and the statistics keep what they held
    N, M = c["X"].shape
    Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
    post = ctx.to_device(np.full((N, M), SENTINEL))
    ym, Yp, ym0, Yp0 = _obs_block(ctx, c["HX"], M)
    lam = bad(good, 7, np.nan)
    fld, ist = _set(ctx, lam, P, good_ob)
    with pytest.raises(_lib.EfaError):
        ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"],
                        c["grid_lat"], c["grid_lon"], c["n_lead"], obs_block_out=True)
    with pytest.raises(_lib.EfaError) as e:
        ctx.letkf_weights(M, P, ym, Yp, c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                          c["grid_lon"])
    assert e.value.status == _lib.EFA_ERR_INVALID
    assert np.all(post.download() == SENTINEL) and np.all(ist.download() == SENTINEL)
    assert np.array_equal(fld.download(), lam, equal_nan=True)
    assert np.array_equal(ym.download()[:P], ym0) and np.array_equal(Yp.download()[:P], Yp0)
    # a field sized for another observation count, and the setter's own refusals (the setting stays as it was)
    f = ctx.to_device(good)
    ctx.set_letkf_inflation(f, None, P + 1, 0.04, LOWER, UPPER, None)
    with pytest.raises(_lib.EfaError) as e:
        ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"],
                        c["grid_lat"], c["grid_lon"], c["n_lead"], obs_block_out=True)
    assert e.value.status == _lib.EFA_ERR_INVALID and "observations" in str(e.value)
    ctx.set_letkf_inflation(None)
    for sigma_b, lo, hi in ((-0.1, LOWER, UPPER), (np.nan, LOWER, UPPER), (0.04, 0.0, UPPER), (0.04, -1.0, UPPER), (0.04, 2.0, 1.0),
                            (0.04, LOWER, np.inf), (0.04, np.nan, UPPER)):
        with pytest.raises(_lib.EfaError) as e:
            ctx.set_letkf_inflation(f, None, P, sigma_b, lo, hi, None)
        assert e.value.status == _lib.EFA_ERR_INVALID
    _same_bits(_cycle(ctx, c), want, "the plain call after the refusals")


# ---- 10. interaction --------------------------------------------------------------------------------------------------------------------
def test_same_bits_twice(ctx):
    c = _case(40, 400, 6, 7, 3)
    a, b = _cycle(ctx, c, c["lam"], c["ob_infl"]), _cycle(ctx, c, c["lam"], c["ob_infl"])
    _same_bits(a, b, "twice")
    assert np.array_equal(a["lam_a"], b["lam_a"]) and np.array_equal(a["istats"], b["istats"], equal_nan=True)
    ip = _cycle(ctx, c, c["lam"], c["ob_infl"], in_place=True)
    _same_bits(ip, a, "in place")
    assert np.array_equal(ip["lam_a"], a["lam_a"])


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
    fld, ist = _set(ctx, c["lam"], c["P"], c["ob_infl"])
    on = calls()
    for a, b in zip(on, off):
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)), "a serial / ETKF call changed under the setting"
    assert np.array_equal(fld.download(), c["lam"]) and np.all(ist.download() == SENTINEL)


# ---- 11. the classes --------------------------------------------------------------------------------------------------------------------
def _api_case(plain_obs=False):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(11)
    nvar, nt, ny, nx, M, P = 2, 2, 6, 7, 12, 30
    lat, lon = np.meshgrid(np.linspace(20, 60, ny), np.linspace(200, 280, nx), indexing="ij")
    arr = rng.standard_normal((nvar, nt, ny, nx, 1)) + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon)
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
    return state, obs, lat, lon


@pytest.mark.parametrize("flavour", ["plain", "stride", "slab"])
def test_the_classes_cycle_the_field(ctx, flavour):
    from efa_xray_amd import ColumnInflation, LETKF, SlabLETKF
    kw, shape = {}, (6, 7)
    cls = LETKF
    if flavour == "stride":
        kw, shape = dict(weight_stride=(2, 3)), (4, 3)
    if flavour == "slab":
        cls, kw, shape = SlabLETKF, dict(vert_coord=np.array([[850.0] * 2, [500.0] * 2])), (2, 6, 7)
    ci = ColumnInflation(initial=1.1)
    s0, o0, lat, lon = _api_case()
    f0 = cls(s0, o0, verbose=False, column_inflation=ci, **kw)
    p0, _ = f0.update()
    sol = f0.last_solve
    assert ci.values.shape == shape and sol["inflation"].shape == shape and sol["inflation_stats"].shape == shape + (4,)
    assert np.all(sol["inflation"] == 1.1) and np.array_equal(sol["inflation_post"], ci.values)
    reached = sol["n_local"] > 0
    assert reached.any() and np.all(ci.values[reached] != 1.1) and np.all(ci.values[~reached] == 1.1)
    first = ci.values.copy()
    s1, o1, _, _ = _api_case()
    f1 = cls(s1, o1, verbose=False, column_inflation=ci, **kw)
    f1.update()
    assert np.array_equal(f1.last_solve["inflation"], first), "the second update starts from the first one's lambda_a"
    assert np.any(ci.values != first)
    # the setting does not outlive the update: a filter without the keyword has today's bits, and a factor of one under
    # sigma_b = 0 equals it
    s2, o2, _, _ = _api_case()
    p2, _ = cls(s2, o2, verbose=False, **kw).update()
    s3, o3, _, _ = _api_case()
    fixed = ColumnInflation(initial=1.0, sigma_b=0.0)
    p3, _ = cls(s3, o3, verbose=False, column_inflation=fixed, **kw).update()
    assert np.array_equal(p3.to_vect(), p2.to_vect()) and np.all(fixed.values == 1.0)
    assert not np.array_equal(p0.to_vect(), p2.to_vect())
    with pytest.raises(ValueError, match="shape"):
        cls(s3, o3, verbose=False, column_inflation=ColumnInflation(values=np.ones((3, 3, 3, 3))), **kw).update()


def test_default_operator_obs_take_the_interpolated_field(ctx):
    """Observations with the shipped point interpolation are solved under that interpolation of the field: against the model
    with ob factors made from the stencils by the rule of the issue."""
    from efa_xray_amd import ColumnInflation, EnsembleState, Observation, LETKF
    rng = np.random.default_rng(21)
    nvar, nt, ny, nx, M, P = 1, 1, 5, 6, 10, 12
    lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(230, 260, nx), indexing="ij")
    arr = rng.standard_normal((nvar, nt, ny, nx, 1)) + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon, validtime=np.array([0.0]))
    name, t0 = state.vars()[0], 0.0
    obs = [Observation(value=float(rng.standard_normal()), error=float(rng.uniform(0.5, 2.0)), lat=float(rng.uniform(31, 49)),
                       lon=float(rng.uniform(231, 259)), obtype=name, time=t0, assimilate_this=True, localize_radius=float(rng.uniform(600.0, 1500.0)))
           for _ in range(P)]
    lam = rng.uniform(0.8, 1.6, (ny, nx))
    ci = ColumnInflation(values=lam.copy())
    f = LETKF(state, obs, verbose=False, column_inflation=ci)
    HX = np.asarray(f.compute_ob_estimates(), dtype=np.float64)
    idx, wts = f._interp_stencils_host(f._context())
    ob_infl = lf.ob_factors(lam.reshape(-1), idx, wts)
    assert np.all((ob_infl >= 0.8) & (ob_infl <= 1.6)) and np.ptp(ob_infl) > 0.0
    ref = lf.letkf_cycle(state.to_vect(), HX, np.array([o.value for o in obs]), np.array([o.error for o in obs]),
                         np.ones(P, dtype=bool), np.array([o.lat for o in obs]), np.array([o.lon for o in obs]),
                         np.array([o.localize_radius for o in obs]), lat, lon, 1, lam.reshape(-1), ob_infl, 0.04, LOWER, UPPER)
    assert ref["stats"]["cond"].max() <= COND_CAP
    post, _ = f.update()
    _close(post.to_vect(), ref["post"], "LETKF.update posterior under the field")
    _close(np.array([o.post_mean for o in obs], dtype=np.float64), ref["diag"]["post_mean"], "post_mean under the interpolated factors")
    _close(np.array([o.post_var for o in obs], dtype=np.float64), ref["diag"]["post_var"], "post_var under the interpolated factors")
    _check_estimate(ci.values.reshape(-1), f.last_solve["inflation_stats"].reshape(-1, 4), lam.reshape(-1), ref["stats"]["p"],
                    ref["lam_a"], "LETKF.update", ref["stats"]["q"])
