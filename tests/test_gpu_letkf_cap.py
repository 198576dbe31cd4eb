"""The LETKF's cap on the local observations of a solve on the MI355X against the NumPy model of
tests/_letkf_cap.py: every seeded case of the section to 1e-10 of each array's largest magnitude (cond(A) <= 1e4 and the absence of
a near-tie at the cap asserted from the model), n_local and n_reach as integers, caps that do not bite bit for bit, ties, a second
route through the uncapped probe, a NaN value, the combinations, the refusals, and the classes.  Every test clears the setting."""
import functools

import numpy as np
import pytest

import _etkf as ek
import _letkf as lk
import _letkf_cap as cp
import _letkf_control as lc
import _letkf_infl as lf
import _letkf_interp as li
import _outlier as qc
from _letkf_gpu import TOL, COND_CAP, _reset, _obs_block, _close, _check_diag, _same_bits
from test_relaxation_host import relax

pytestmark = pytest.mark.gpu

MID = ((16, 64, 5, 7, 3), (8,), None)
MID3 = ((16, 64, 5, 7, 3), (4, 0, 12), None)
SENTINEL = -7.25
LOWER, UPPER = 1e-2, 1e2


@pytest.fixture
def ctx():
    from efa_xray_amd import _lib
    c = _reset(_lib.get_context(0))
    c.set_letkf_inflation(None)
    c.set_letkf_control(None)
    c.set_letkf_obs_cap(None, None)
    yield c
    c.set_letkf_obs_cap(None, None)
    c.set_letkf_control(None)
    c.set_letkf_inflation(None)
    _reset(c)


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _case(shape, caps, hw):
    """(the seeded case, the obs' classes), computed once and left unchanged."""
    c, ob_class = cp.make_case(shape, caps, hw)
    if ob_class is not None:
        ob_class.setflags(write=False)
    return _freeze(c), ob_class


@functools.lru_cache(maxsize=None)
def _model(shape, caps, hw):
    c, ob_class = _case(shape, caps, hw)
    return cp.letkf_cycle(c, ob_class, caps)


def _cycle(ctx, c, caps=None, ob_class=None, want_reach=True, in_place=False, f32=False, X=None, stride=None, lam=None, ob_infl=None,
           sigma_b=0.04, control=None, **over):
    """One cycle through the plain or the interp entry with the cap set (caps None: off) and cleared: posterior, obs block,
    diagnostics, statistics of the columns or nodes, n_reach; with lam the inflation field, with control = (xc, yc) the control."""
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
    stats = ctx.empty((npts, 3))
    reach = ctx.to_device(np.full(npts, SENTINEL)) if caps is not None and want_reach else None
    fld = ist = obd = xcp = ycp = None
    try:
        if caps is not None:
            ctx.set_letkf_obs_cap(ob_class, caps, reach, P=P)
        if lam is not None:
            fld = ctx.to_device(np.ascontiguousarray(lam, dtype=np.float64).reshape(-1))
            obd = None if ob_infl is None or not P else ctx.to_device(np.ascontiguousarray(ob_infl, dtype=np.float64))
            ist = ctx.to_device(np.full((fld.shape[0], 4), SENTINEL))
            ctx.set_letkf_inflation(fld, obd, P, sigma_b, LOWER, UPPER, ist)
        if control is not None:
            xcd, ycd = ctx.to_device(np.ascontiguousarray(control[0])), ctx.to_device(np.ascontiguousarray(control[1]))
            xcp, ycp = ctx.to_device(np.full(N, SENTINEL)), ctx.to_device(np.full(P, SENTINEL))
            ctx.set_letkf_control(xcd, xcp, ycd, ycp)
        diag = ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"],
                               g["grid_lat"], g["grid_lon"], g["n_lead"], obs_block_out=True, col_stats=stats, f32=f32, **mesh)
    finally:
        ctx.set_letkf_obs_cap(None, None)
        ctx.set_letkf_control(None)
        ctx.set_letkf_inflation(None)
    out = dict(post=post.download(), ym=ym.download()[:P], Yp=Yp.download()[:P], diag=diag, stats=stats.download(), ym0=ym0, Yp0=Yp0,
               n_reach=None if reach is None else reach.download(), lam_a=None if fld is None else fld.download(),
               istats=None if ist is None else ist.download())
    if control is not None:
        out.update(xc_post=xcp.download(), yc_post=ycp.download())
    return out


def _probe(ctx, c, caps=None, ob_class=None, lat=None, lon=None, **over):
    """efa_letkf_weights_dev at the grid's columns (or the given points) with the cap set and cleared: T, w, stats, n_reach."""
    g = dict(c, **over)
    M, P = g["M"], g["P"]
    lat = g["grid_lat"] if lat is None else lat
    lon = g["grid_lon"] if lon is None else lon
    ym, Yp, _, _ = _obs_block(ctx, g["HX"], M)
    reach = ctx.to_device(np.full(np.asarray(lat).size, SENTINEL)) if caps is not None else None
    try:
        if caps is not None:
            ctx.set_letkf_obs_cap(ob_class, caps, reach, P=P)
        T, w, st = ctx.letkf_weights(M, P, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"], lat, lon)
    finally:
        ctx.set_letkf_obs_cap(None, None)
    return T, w, st, None if reach is None else reach.download()


def _rows(c, cols):
    return (np.flatnonzero(cols)[None, :] + c["ncol"] * np.arange(c["n_lead"])[:, None]).reshape(-1)


def _check_counts(r, reach, caps, what):
    """n_reach and n_local as integers: n_local = sum_c min(cap_c, reach_c) exactly."""
    assert np.array_equal(r["n_reach"], reach.sum(axis=1).astype(np.float64)), what + ": n_reach"
    assert np.array_equal(r["stats"][:, 0], cp.n_local(reach, caps).astype(np.float64)), what + ": n_local"


def _check_against_model(r, ref, caps, what):
    st = ref["stats"]
    print("%s: cond(A) max %.3g, n_local %d..%d of a reach of %d..%d, the cap bites at %d of %d columns and %d of %d ob positions, "
          "smallest gap %.2g / %.2g" % (what, st["cond"].max(), st["n_local"].min(), st["n_local"].max(), ref["reach"].sum(axis=1).min(),
                                        ref["reach"].sum(axis=1).max(), ref["bites"].sum(), ref["bites"].size, ref["ob_bites"].sum(),
                                        ref["ob_bites"].size, ref["gap"], ref["ob_gap"]))
    assert st["cond"].max() <= COND_CAP
    assert ref["bites"].any() and ref["ob_bites"].any(), "the case: the cap bites"
    _close(r["post"], ref["post"], what + " posterior members")
    _close(r["Yp"], ref["Yp"], what + " posterior obs perturbations")
    _close(r["ym"], ref["ym"], what + " posterior obs means")
    _check_diag(r["diag"], ref["diag"], what)
    assert np.array_equal(st["n_local"], cp.n_local(ref["reach"], caps)), "the model's own count"
    _check_counts(r, ref["reach"], caps, what)
    assert np.abs(r["stats"][:, 1] - st["dfs"]).max() <= TOL * max(1.0, st["dfs"].max()), what + ": dfs"


# ---- 1. parity with the model at every case of the section ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,caps,hw", cp.CASES)
def test_capped_cycle_and_weights_match_the_model(ctx, shape, caps, hw):
    (c, ob_class), ref = _case(shape, caps, hw), _model(shape, caps, hw)
    what = "M=%d P=%d caps=%r" % (shape[0], shape[1], caps)
    r = _cycle(ctx, c, caps, ob_class)
    _check_against_model(r, ref, caps, what)
    if hw is not None:
        assert (ref["bites"].sum(), ref["ob_bites"].sum()) == (73, 79) and ref["bites"].size == 99, "the case: the cap bites in part"
    T, w, st, reach = _probe(ctx, c, caps, ob_class)
    _close(T, ref["T"], what + " T")
    _close(w, ref["w"], what + " w")
    assert np.array_equal(st, r["stats"]) and np.array_equal(reach, r["n_reach"]), "the probe runs the same lists"
    plain = _cycle(ctx, c)
    assert np.any(plain["post"] != r["post"]) and np.any(plain["stats"][:, 0] > r["stats"][:, 0]), "the cap changed nothing"
    assert np.array_equal(plain["stats"][:, 0], r["n_reach"]), "n_reach is the uncapped run's n_local"


# ---- 2. caps that do not bite: bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("shape", [(16, 64, 5, 7, 3), (40, 400, 6, 7, 3)])
def test_caps_of_P_give_the_uncapped_run_bit_for_bit(ctx, shape, f32):
    c, _ = _case(shape, (8,), None)
    P = c["P"]
    X = np.ascontiguousarray(c["X"], dtype=np.float32) if f32 else c["X"]
    lam = np.random.default_rng(11).uniform(0.8, 1.6, c["ncol"])
    ob_infl = np.random.default_rng(12).uniform(0.8, 1.6, P)
    plain = _cycle(ctx, c, X=X, f32=f32, lam=lam, ob_infl=ob_infl)
    cls3 = np.arange(P, dtype=np.int32) % 3
    reach_max = int(plain["stats"][:, 0].max())
    for caps, cls in (((P,), None), ((P, P, P), cls3), ((0,), None), ((0, P, 0), cls3), ((2 ** 40,), None)):
        r = _cycle(ctx, c, caps, cls, X=X, f32=f32, lam=lam, ob_infl=ob_infl)
        what = "caps %r" % (caps,)
        _same_bits(r, plain, what)
        assert np.array_equal(r["lam_a"], plain["lam_a"]) and np.array_equal(r["istats"], plain["istats"], equal_nan=True), what
        assert np.array_equal(r["n_reach"], r["stats"][:, 0]), what + ": n_reach == n_local"
    T0, w0, st0, _ = _probe(ctx, c)
    T1, w1, st1, reach = _probe(ctx, c, (P,))
    assert np.array_equal(T0, T1) and np.array_equal(w0, w1) and np.array_equal(st0, st1) and np.array_equal(reach, st1[:, 0])
    # set, then cleared: nothing is left behind
    ctx.set_letkf_obs_cap(None, (3,), None, P=P)
    ctx.set_letkf_obs_cap(None, None)
    _same_bits(_cycle(ctx, c, X=X, f32=f32, lam=lam, ob_infl=ob_infl), plain, "set and cleared")
    # the largest reach of a column: the columns keep their bits (an ob position may reach more), one below it bites
    assert np.array_equal(_cycle(ctx, c, (reach_max,), X=X, f32=f32)["post"], _cycle(ctx, c, X=X, f32=f32)["post"])
    assert np.any(_cycle(ctx, c, (reach_max - 1,), X=X, f32=f32)["stats"][:, 0] < plain["stats"][:, 0]), "one below the reach bites"


# ---- 3. ties: equal tapers are ordered by lower ob index first ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tie_case():
    """Six obs at one position with one half-width, with different values, errors and HX rows, on a 3 x 5 grid."""
    c = lk.make_case(8, 6, 3, 5, 2)
    c.update(ob_lat=np.full(6, 41.0), ob_lon=np.full(6, 262.0), ob_hw=np.full(6, 3000.0), assim=np.ones(6, dtype=bool))
    return _freeze(c)


@pytest.mark.parametrize("first_off", [False, True])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5])
def test_equal_tapers_are_ordered_by_lower_index_first(ctx, N, first_off):
    c = _tie_case()
    assim = c["assim"].copy()
    assim[0] = not first_off
    if first_off and N == 5:
        N = 4           # five obs are left: a cap of 5 would not bite
    ref = cp.letkf_cycle(c, None, (N,), assim=assim)
    lo = 1 if first_off else 0
    assert ref["bites"].all() and ref["ob_bites"].all() and ref["gap"] == np.inf, "the case: a bit-equal tie at every point"
    assert np.all((ref["rho"] != 0) == (np.arange(6)[None, :] >= lo) & (np.arange(6)[None, :] < lo + N)), "the model: the first N"
    other = cp.letkf_cycle(c, None, (N,), assim=assim, last_first=True)
    scale = np.abs(ref["post"]).max()
    assert np.abs(other["post"] - ref["post"]).max() > 1e-6 * scale, "the opposite choice must give another posterior"
    r = _cycle(ctx, c, (N,), assim=assim)
    _close(r["post"], ref["post"], "ties N=%d posterior" % N)
    _close(r["Yp"], ref["Yp"], "ties N=%d obs perturbations" % N)
    _close(r["ym"], ref["ym"], "ties N=%d obs means" % N)
    assert np.abs(r["post"] - other["post"]).max() > 1e-6 * scale
    _check_counts(r, ref["reach"], (N,), "ties")
    assert np.all(r["stats"][:, 0] == N) and np.all(r["n_reach"] == 6 - lo)
    # the chosen obs by another route: the uncapped run with every other ob unflagged has the same bits up to the Gram's zeros
    keep = assim & (np.arange(6) < lo + N)
    cut = _cycle(ctx, c, assim=keep)
    _close(r["post"], cut["post"], "ties N=%d against the cut flags" % N)


# ---- 4. a second route: the uncapped probe under the flags cut to the model's selected set --------------------------------------------
@pytest.mark.parametrize("case", [MID, MID3])
def test_capped_weights_equal_the_uncapped_probe_under_the_selected_flags(ctx, case):
    shape, caps, hw = case
    (c, ob_class), ref = _case(*case), _model(*case)
    T, w, st, _ = _probe(ctx, c, caps, ob_class)
    glat, glon = c["grid_lat"].reshape(-1), c["grid_lon"].reshape(-1)
    Tc, wc = np.empty_like(T), np.empty_like(w)
    for i in range(c["ncol"]):
        keep = ref["rho"][i] != 0.0
        assert keep.sum() == st[i, 0] and np.all(c["assim"][keep])
        Ti, wi, sti, _ = _probe(ctx, c, lat=glat[i:i + 1], lon=glon[i:i + 1], assim=keep)
        assert sti[0, 0] == keep.sum()
        Tc[i], wc[i] = Ti[0], wi[0]
    _close(T, Tc, "T against the cut flags")        # (only the MFMA grouping of the Gram's rows differs)
    _close(w, wc, "w against the cut flags")


# ---- 5. a NaN value reaches exactly the points at which its ob wins ---------------------------------------------------------------------
def test_a_nan_value_reaches_the_points_where_its_ob_wins_only(ctx):
    shape, caps, hw = MID
    (c, _), ref = _case(*MID), _model(*MID)
    plain_rho = lk.taper(c["grid_lat"], c["grid_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"])
    wins, loses = ref["rho"] != 0.0, (ref["rho"] == 0.0) & (plain_rho != 0.0)
    ks = np.flatnonzero(wins.any(axis=0) & loses.any(axis=0))
    assert ks.size, "the case: an ob that wins at some columns and loses at others"
    k = int(ks[np.argmax(np.minimum(wins[:, ks].sum(axis=0), loses[:, ks].sum(axis=0)))])
    hit = wins[:, k]
    print("ob %d wins at %d columns and loses at %d" % (k, hit.sum(), loses[:, k].sum()))
    value = c["value"].copy()
    value[k] = np.nan
    a, b = _cycle(ctx, c, caps), _cycle(ctx, c, caps, value=value)
    assert np.isnan(b["post"][_rows(c, hit)]).all(), "NaN means where it wins"
    assert np.array_equal(b["post"][_rows(c, ~hit)], a["post"][_rows(c, ~hit)]), "the NaN reached a column at which its ob loses"
    _close(b["post"][_rows(c, ~hit)], ref["post"][_rows(c, ~hit)], "where it loses: parity")
    assert np.array_equal(a["stats"], b["stats"]) and np.array_equal(a["n_reach"], b["n_reach"])
    T0, w0, _, _ = _probe(ctx, c, caps)
    T1, w1, _, _ = _probe(ctx, c, caps, value=value)
    assert np.array_equal(T0, T1), "a NaN value reached T: the perturbations stay finite"
    assert np.isnan(w1[hit]).all() and np.array_equal(w1[~hit], w0[~hit])
    ob_hit = ref["ob_reach"].sum(axis=1) > 0        # the obs block likewise, at every ob's own position
    rho_o = lk.taper(c["ob_lat"], c["ob_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"])
    ob_wins = cp.select(rho_o, None, caps)[:, k] != 0.0
    assert ob_wins.any() and not ob_wins[ob_hit].all()
    assert np.isnan(b["ym"][ob_wins]).all() and np.array_equal(b["ym"][~ob_wins], a["ym"][~ob_wins])
    assert np.all(np.isfinite(b["Yp"])) and np.array_equal(b["Yp"], a["Yp"])


# ---- 6. the combinations against their models -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [MID, ((40, 400, 6, 7, 3), (10, 0, 40), None)])
def test_weight_stride_caps_the_nodes(ctx, case):
    shape, caps, hw = case
    c, ob_class = _case(*case)
    stride = (2, 3)
    with cp.capped(ob_class, caps) as log:
        ref = li.interp_cycle(c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                              c["grid_lon"], c["n_lead"], (c["ny"], c["nx"]), stride)
    assert len(log) == 3 and log[2]["bites"].any()       # the grid's, the obs', the nodes'
    assert max(ref["stats"]["cond"].max(), ref["node_stats"]["cond"].max()) <= COND_CAP
    r = _cycle(ctx, c, caps, ob_class, stride=stride)
    _close(r["post"], ref["post"], "weight_stride posterior")
    _close(r["Yp"], ref["Yp"], "weight_stride obs perturbations")
    _close(r["ym"], ref["ym"], "weight_stride obs means")
    _check_counts(r, log[2]["reach"], caps, "nodes")
    assert np.abs(ref["post"] - ref["plain_post"]).max() > 1e-6 * np.abs(ref["post"]).max(), "the case: interpolation matters"


def test_column_inflation_estimates_from_the_obs_that_remain(ctx):
    from test_gpu_letkf_inflation import _check_estimate
    shape, caps, hw = MID
    c, _ = _case(*MID)
    rng = np.random.default_rng(977)
    lam, ob_infl = rng.uniform(0.8, 1.6, c["ncol"]), rng.uniform(0.8, 1.6, c["P"])
    with cp.capped(None, caps) as log:
        ref = lf.letkf_cycle(c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                             c["grid_lon"], c["n_lead"], lam, ob_infl, 0.04, LOWER, UPPER)
    assert ref["stats"]["cond"].max() <= COND_CAP and log[0]["bites"].all()
    r = _cycle(ctx, c, caps, lam=lam, ob_infl=ob_infl, sigma_b=0.04)
    _close(r["post"], ref["post"], "inflation posterior")
    _close(r["Yp"], ref["Yp"], "inflation obs perturbations")
    _close(r["ym"], ref["ym"], "inflation obs means")
    _check_counts(r, log[0]["reach"], caps, "inflation")
    _check_estimate(r["lam_a"], r["istats"], lam, ref["stats"]["p"], ref["lam_a"], "capped", ref["stats"]["q"])
    assert np.any(r["lam_a"] != lam)
    plain = _cycle(ctx, c, lam=lam, ob_infl=ob_infl, sigma_b=0.04)
    assert np.all(r["istats"][:, 2] < plain["istats"][:, 2]), "p3 sums the tapers that remain"


def test_the_control_is_adjusted_by_the_obs_that_remain(ctx):
    shape, caps, hw = MID3
    c, ob_class = _case(*MID3)
    xc, yc = lc.control_inputs(c)
    with cp.capped(ob_class, caps):
        ref = lc.control_cycle(c["X"], c["HX"], xc, yc, c["value"], c["error"], c["assim"], *lc.plain_tapers(c))
    assert ref["cond"] <= COND_CAP
    r = _cycle(ctx, c, caps, ob_class, control=(xc, yc))
    _close(r["xc_post"], ref["xc_post"], "x_c^a")
    _close(r["yc_post"][c["assim"]], ref["yc_post"][c["assim"]], "y_c^a")
    _same_bits(r, _cycle(ctx, c, caps, ob_class), "the ensemble with and without the control")
    _close(r["post"], _model(*MID3)["post"], "posterior members")


def test_rtps_on_float32_rows(ctx):
    from efa_xray_amd import _lib
    case = ((40, 400, 6, 7, 3), (50,), None)
    (c, _), ref = _case(*case), None
    X32 = np.ascontiguousarray(c["X"], dtype=np.float32)
    ref = cp.letkf_cycle(dict(c, X=X32.astype(np.float64)), None, case[1])
    want = relax(X32.astype(np.float64), ref["post"], rtps=0.9)
    ctx.set_relaxation(_lib.RELAX_RTPS, 0.9)
    for in_place in (False, True):
        a = _cycle(ctx, c, case[1], X=X32, f32=True, in_place=in_place)
        b = _cycle(ctx, c, case[1], X=X32.astype(np.float64), in_place=in_place)
        assert a["post"].dtype == np.float32 and np.array_equal(a["post"], b["post"].astype(np.float32))
        _same_bits(a, b, "float32 against float64", keys=("ym", "Yp", "stats"))
        _close(b["post"], want, "rtps")
        _close(b["Yp"], ref["Yp"], "the obs block is not relaxed")


def test_an_ob_the_outlier_check_rejects_frees_its_place(ctx):
    t = 3.0
    case = ((17, 33, 5, 7, 3), (1,), None)
    c, _ = _case(*case)
    caps = (3,)
    ym, Yp = ek.ob_priors(c["HX"])
    value, bad = qc.inject(c["HX"], c["value"], c["error"], c["assim"], t, 3, seed=17)
    assert qc.clear_of_threshold(ym, Yp, value, c["error"], t)
    flags = qc.masked_flags(c["HX"], value, c["error"], c["assim"], t)
    assert not flags[bad].any() and flags.any()
    before = cp.letkf_cycle(dict(c, value=value), None, caps)              # as if nothing were rejected
    ref = cp.letkf_cycle(dict(c, value=value), None, caps, assim=flags)
    held = (before["rho"][:, bad] != 0.0).any(axis=1)
    assert held.any(), "the case: a rejected ob would have held a place"
    assert np.all(ref["stats"]["n_local"][held] == np.minimum(3, ref["reach"][held, 0])), "... which another ob takes"
    ctx.set_outlier_threshold(t)
    try:
        r = _cycle(ctx, c, caps, value=value)
    finally:
        ctx.set_outlier_threshold(None)
    assert np.array_equal(r["diag"]["assimilated"], flags), "rejected set"
    _same_bits(r, _cycle(ctx, c, caps, value=value, assim=flags), "outlier check against cleared flags")
    _check_against_model(r, ref, caps, "outlier check")


# ---- 7. the refusals, each followed by a served call; what ignores the setting; determinism ----------------------------------------
def test_the_setter_and_the_entries_refuse_and_the_context_goes_on(ctx):
    from efa_xray_amd import _lib
    (c, ob_class), ref = _case(*MID3), _model(*MID3)
    caps = MID3[1]
    P, M, N = c["P"], c["M"], c["X"].shape[0]
    want = _cycle(ctx, c, caps, ob_class)
    plain = _cycle(ctx, c)

    def served(what):
        _same_bits(_cycle(ctx, c, caps, ob_class), want, "after " + what)
        _same_bits(_cycle(ctx, c), plain, "the setting is off after " + what)

    def refused(what, fn, *needles):
        with pytest.raises(_lib.EfaError) as e:
            fn()
        assert e.value.status == _lib.EFA_ERR_INVALID, what
        for s in needles:
            assert s in str(e.value), "%s: %r not in %r" % (what, s, str(e.value))
        ctx.set_letkf_obs_cap(None, None)
        served(what)

    # the setter: the setting stays as it was (here: off)
    refused("nclass 0", lambda: ctx.set_letkf_obs_cap(None, np.zeros(0), None, P=P), "nclass")
    refused("nclass 33", lambda: ctx.set_letkf_obs_cap(None, np.ones(33), None, P=P), "nclass")
    refused("a negative cap", lambda: ctx.set_letkf_obs_cap(ob_class, (4, -1, 12), None), "cap")
    refused("a class beyond the range", lambda: ctx.set_letkf_obs_cap(np.where(np.arange(P) == 5, 3, ob_class), caps, None), "class")
    refused("a negative class", lambda: ctx.set_letkf_obs_cap(np.where(np.arange(P) == 7, -1, ob_class), caps, None), "class")
    refused("a negative count", lambda: ctx.set_letkf_obs_cap(None, (4,), None, P=-1), "negative")
    five = _probe(ctx, c, (5,))[2]
    ctx.set_letkf_obs_cap(None, (5,), None, P=P)        # a refusal leaves the earlier setting in force
    with pytest.raises(_lib.EfaError):
        ctx.set_letkf_obs_cap(None, (-5,), None, P=P)
    ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
    T, w, st = ctx.letkf_weights(M, P, ym, Yp, c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                                 c["grid_lon"])
    assert np.array_equal(st, five) and np.all(st[:, 0] <= 5), "the earlier setting was lost"
    ctx.set_letkf_obs_cap(None, None)
    served("a refused change of the setting")

    # a P or nsolve that differs from the call's
    def with_setting(cls, caps_, nreach, P_, fn):
        def run():
            reach = None if nreach is None else ctx.empty((nreach,))
            ctx.set_letkf_obs_cap(cls, caps_, reach, P=P_)
            fn()
        return run

    other = lk.make_case(16, 40, 5, 7, 3)
    refused("another P", with_setting(ob_class, caps, None, P, lambda: _cycle(ctx, other)), "observations")
    refused("another nsolve", with_setting(ob_class, caps, c["ncol"] + 1, P, lambda: _cycle(ctx, c)), "solve points")
    refused("nsolve of the grid with a mesh", with_setting(ob_class, caps, c["ncol"], P, lambda: _cycle(ctx, c, stride=(2, 3))),
            "solve points")
    refused("another P at the probe", with_setting(ob_class, caps, None, P, lambda: _probe(ctx, other)), "observations")
    refused("another nsolve at the probe", with_setting(ob_class, caps, c["ncol"], P,
                                                        lambda: _probe(ctx, c, lat=c["grid_lat"][:2], lon=c["grid_lon"][:2])), "solve points")


def test_the_slab_entries_refuse_while_the_setting_is_on(ctx):
    from efa_xray_amd import _lib
    import _letkf_slab as ls
    c = ls.make_case(16, 64, 5, 7, 2, 3, parts="vtc")
    loc = c["loc"]
    N, M, P = c["X"].shape[0], c["M"], c["P"]

    def slab_cycle():
        ctx.set_vertical_localization(loc["lead_vert"], loc["ob_vert"], loc["ob_vert_halfwidth"])
        Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
        ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
        try:
            ctx.letkf_cycle(N, M, P, Xd, Xd, ym, Yp, c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"],
                            c["grid_lat"], c["grid_lon"], c["n_lead"], _slab=True)
        finally:
            ctx.set_vertical_localization(None)
        return Xd.download()

    want = slab_cycle()
    ctx.set_letkf_obs_cap(None, (8,), None, P=P)
    with pytest.raises(_lib.EfaError) as e:
        slab_cycle()
    assert e.value.status == _lib.EFA_ERR_INVALID and "per group" in str(e.value)
    ctx.set_letkf_obs_cap(None, None)
    assert np.array_equal(slab_cycle(), want), "the slab cycle after the refusal"


def test_the_entries_that_ignore_the_setting_keep_their_bits(ctx):
    from efa_xray_amd import _lib
    c, ob_class = _case(*MID3)
    N, M, P = c["X"].shape[0], c["M"], c["P"]

    def ensrf():
        Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
        post = ctx.empty((N, M))
        ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
        ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, c["value"], c["error"], c["assim"], loc_mode=_lib.LOC_GC, ob_lat=c["ob_lat"], ob_lon=c["ob_lon"],
                        ob_halfwidth=c["ob_hw"], grid_lat=c["grid_lat"], grid_lon=c["grid_lon"], n_lead=c["n_lead"], obs_block_out=True)
        return post.download(), ym.download(), Yp.download()

    def interp_apply():
        stride = (2, 3)
        nn = li.axis_nodes(c["ny"], 2).size * li.axis_nodes(c["nx"], 3).size
        rng = np.random.default_rng(3)
        Tw = np.zeros((nn, M, M + 1))
        Tw[:, :, :M] = np.eye(M) + 0.01 * rng.standard_normal((nn, M, M))
        Tw[:, :, M] = 0.1 * rng.standard_normal((nn, M))
        Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
        post = ctx.empty((N, M))
        ctx.letkf_interp_apply(N, M, Xd, post, (c["ny"], c["nx"]), stride, c["n_lead"], ctx.to_device(Tw))
        return (post.download(),)

    for fn in (ensrf, interp_apply):
        off = fn()
        ctx.set_letkf_obs_cap(ob_class, MID3[1], None)      # sized for this P; no reach
        try:
            on = fn()
            ctx.set_letkf_obs_cap(None, (1,), ctx.empty((3,)), P=P + 9)      # ... and sized for another call altogether
            on2 = fn()
        finally:
            ctx.set_letkf_obs_cap(None, None)
        for a, b, d in zip(off, on, on2):
            assert np.array_equal(a, b) and np.array_equal(a, d), fn.__name__


@pytest.mark.parametrize("case", [MID3, ((20, 120, 9, 11, 2), (12,), (300.0, 800.0))])
def test_twice_the_same_bits_and_in_place(ctx, case):
    shape, caps, hw = case
    c, ob_class = _case(*case)
    a, b = _cycle(ctx, c, caps, ob_class), _cycle(ctx, c, caps, ob_class)
    _same_bits(a, b, "run twice")
    assert np.array_equal(a["n_reach"], b["n_reach"])
    _same_bits(_cycle(ctx, c, caps, ob_class, in_place=True), a, "in place")
    _same_bits(_cycle(ctx, c, caps, ob_class, want_reach=False), a, "without the reach array")


# ---- 8. the classes ------------------------------------------------------------------------------------------------------------------
def _api_case(dtype=np.float64, seed=5):
    """A state of two variables and obs of three obtypes (the two variables, point-interpolated, and none)."""
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(seed)
    nvar, nt, ny, nx, M, P = 2, 2, 6, 7, 12, 48
    lat, lon = np.meshgrid(np.linspace(20, 60, ny), np.linspace(200, 280, nx), indexing="ij")
    arr = rng.standard_normal((nvar, nt, ny, nx, 1)) + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon, dtype=dtype)
    N = state.nstate()
    rows = rng.choice(N, P, replace=False)

    class RowOb(Observation):
        def estimate(self, st):
            return st.to_vect()[self.row].copy()

    X = state.to_vect().astype(np.float64)
    types = ("radar", "radar", "radar", "synop", "radar", "buoy")
    obs = []
    for k in range(P):
        col = rows[k] % (ny * nx)
        ob = RowOb(value=float(X[rows[k]].mean() + rng.standard_normal()), obtype=types[k % 6], error=float(rng.uniform(0.5, 2.0)),
                   lat=float(lat.reshape(-1)[col]), lon=float(lon.reshape(-1)[col]), assimilate_this=(k % 7 != 3),
                   localize_radius=float(rng.uniform(1500.0, 3000.0)))
        ob.row = int(rows[k])
        obs.append(ob)
    return state, obs, lat, lon


def _api_model(state, obs, lat, lon, ob_class, caps, f):
    HX = np.asarray(f.compute_ob_estimates(), dtype=np.float64)
    c = dict(X=state.to_vect().astype(np.float64), HX=HX, value=np.array([o.value for o in obs]), error=np.array([o.error for o in obs]),
             assim=np.array([o.assimilate_this for o in obs]), ob_lat=np.array([o.lat for o in obs]), ob_lon=np.array([o.lon for o in obs]),
             ob_hw=np.array([o.localize_radius for o in obs]), grid_lat=lat, grid_lon=lon, n_lead=4)
    return cp.letkf_cycle(c, ob_class, caps)


@pytest.mark.parametrize("form", ["int", "dict"])
def test_letkf_class_against_the_model(ctx, form):
    from efa_xray_amd import LETKF, SlabLETKF
    state, obs, lat, lon = _api_case()
    if form == "int":
        arg, ob_class, caps = 6, None, (6,)
    else:
        arg = {"radar": 5, "metar": 2, "buoy": 40}     # no ob is a metar; synop is not named: no limit
        ob_class = np.array([{"radar": 0, "buoy": 1}.get(o.obtype, 2) for o in obs])
        caps = (5, 40, 0)
    f = LETKF(state, obs, verbose=False, max_local_obs=arg)
    ref = _api_model(state, obs, lat, lon, ob_class, caps, f)
    assert ref["stats"]["cond"].max() <= COND_CAP and ref["bites"].any() and ref["ob_bites"].any()
    post, _ = f.update()
    _close(post.to_vect(), ref["post"], "LETKF.update posterior")
    ls = f.last_solve
    assert sorted(ls) == ["dfs", "n_local", "n_reach", "sweeps"] and all(ls[k].shape == (6, 7) for k in ls)
    assert ls["n_reach"].dtype == np.int64
    assert np.array_equal(ls["n_reach"].reshape(-1), ref["reach"].sum(axis=1))
    assert np.array_equal(ls["n_local"].reshape(-1), cp.n_local(ref["reach"], caps))
    # SlabLETKF without its options is LETKF; the setting is gone after update()
    s2, o2, _, _ = _api_case()
    p2, _ = SlabLETKF(s2, o2, verbose=False, max_local_obs=arg).update()
    assert np.array_equal(p2.to_vect(), post.to_vect())
    s3, o3, _, _ = _api_case()
    g = LETKF(s3, o3, verbose=False)
    p3, _ = g.update()
    assert "n_reach" not in g.last_solve and np.array_equal(g.last_solve["n_local"], ls["n_reach"]), "the setting outlived update()"
    assert np.any(p3.to_vect() != post.to_vect())
    with pytest.raises(ValueError, match="a cap per group is the follow-up"):
        SlabLETKF(s3, o3, verbose=False, max_local_obs=arg, time_localize=True)


def test_letkf_class_combines_and_clears_the_setting_after_an_exception(ctx):
    from efa_xray_amd import LETKF, ColumnInflation
    state, obs, lat, lon = _api_case(dtype=np.float32)
    f = LETKF(state, obs, verbose=False, max_local_obs=6, weight_stride=(2, 3), rtps=0.9, outlier_threshold=4.0,
              column_inflation=ColumnInflation(sigma_b=0.04))
    post, _ = f.update()
    assert post.to_vect().dtype == np.float32 and np.all(np.isfinite(post.to_vect()))
    ls = f.last_solve
    assert ls["n_reach"].shape == ls["n_local"].shape == (ls["node_y"].size, ls["node_x"].size)
    assert np.array_equal(ls["n_local"], np.minimum(ls["n_reach"], 6)) and np.any(ls["n_reach"] > 6)
    # an exception inside the cycle: the setting does not outlive it
    s2, o2, _, _ = _api_case()
    want, _ = LETKF(s2, o2, verbose=False).update()
    s3, o3, _, _ = _api_case()
    bad = LETKF(s3, o3, verbose=False, max_local_obs=6)
    o3[0].error = -1.0
    with pytest.raises(Exception):
        bad.update()
    s4, o4, _, _ = _api_case()
    got, _ = LETKF(s4, o4, verbose=False).update()
    assert np.array_equal(got.to_vect(), want.to_vect()), "the setting outlived the exception"
