"""The LETKF with cross validation on the MI355X against the NumPy model of tests/_letkf_cv.py: every seeded case of
the section to 1e-10 of each array's largest magnitude (cond <= 1e4 of the full solve and of every sub-solve asserted by the model),
the pairs through letkf_weights, the properties of the section, the combinations, the refusals and the class.  Every test clears the
setting."""
import ctypes
import functools

import numpy as np
import pytest

import _letkf as lk
import _letkf_cap as cp
import _letkf_cv as cv
import _letkf_interp as li
import _outlier as qc
from _letkf_gpu import TOL, SWEEP_CAP, _reset, _obs_block, _close, _check_diag, _same_bits
from test_relaxation_host import relax

pytestmark = pytest.mark.gpu

MID = (16, 4, 64, 5, 7, 3)
SENTINEL = -7.25
ALL_CASES = [(k, False) for k in cv.CASES] + [(cv.PERMUTED, True)]


@pytest.fixture
def ctx():
    from efa_xray_amd import _lib
    c = _reset(_lib.get_context(0))

    def clear():
        c.set_letkf_inflation(None)
        c.set_letkf_control(None)
        c.set_letkf_obs_cap(None, None)
        c.set_letkf_cross_validation(None)

    clear()
    yield c
    clear()
    _reset(c)


@functools.lru_cache(maxsize=None)
def _case(case, permuted=False):
    """(the seeded case, its labels), computed once and left unchanged."""
    c, g = cv.make_case(*case, permuted=permuted)
    for v in list(c.values()) + [g]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c, g


@functools.lru_cache(maxsize=None)
def _model(case, permuted=False, stride=None):
    c, g = _case(case, permuted)
    return cv.cv_cycle(c, g, stride=stride)


@functools.lru_cache(maxsize=None)
def _plain_model(case, permuted=False):
    c, _ = _case(case, permuted)
    return lk.letkf_cycle(c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                          c["grid_lon"], c["n_lead"])


def _cycle(ctx, c, groups=None, want_stats=True, in_place=False, f32=False, X=None, stride=None, caps=None, **over):
    """One cycle through the plain or the interp entry with the setting on (groups None: off) and cleared: posterior, obs block,
    diagnostics, statistics of the columns or nodes, the sub-solves' statistics."""
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
    cvs = ctx.to_device(np.full((npts, 2), SENTINEL)) if groups is not None and want_stats else None
    try:
        if groups is not None:
            ctx.set_letkf_cross_validation(groups, cvs)
        if caps is not None:
            ctx.set_letkf_obs_cap(None, caps, None, P=P)
        diag = ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"],
                               g["grid_lat"], g["grid_lon"], g["n_lead"], obs_block_out=True, col_stats=stats, f32=f32, **mesh)
    finally:
        ctx.set_letkf_obs_cap(None, None)
        ctx.set_letkf_cross_validation(None)
    return dict(post=post.download(), ym=ym.download()[:P], Yp=Yp.download()[:P], diag=diag, stats=stats.download(), ym0=ym0, Yp0=Yp0,
                cv_stats=None if cvs is None else cvs.download())


def _probe(ctx, c, groups=None, lat=None, lon=None, **over):
    """efa_letkf_weights_dev at the grid's columns (or the given points) with the setting on and cleared: T, w, stats, cv_stats."""
    g = dict(c, **over)
    M, P = g["M"], g["P"]
    lat = g["grid_lat"] if lat is None else lat
    lon = g["grid_lon"] if lon is None else lon
    ym, Yp, _, _ = _obs_block(ctx, g["HX"], M)
    cvs = ctx.to_device(np.full((np.asarray(lat).size, 2), SENTINEL)) if groups is not None else None
    try:
        if groups is not None:
            ctx.set_letkf_cross_validation(groups, cvs)
        T, w, st = ctx.letkf_weights(M, P, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"], lat, lon)
    finally:
        ctx.set_letkf_cross_validation(None)
    return T, w, st, None if cvs is None else cvs.download()


def _rows(c, cols):
    return (np.flatnonzero(cols)[None, :] + c["ncol"] * np.arange(c["n_lead"])[:, None]).reshape(-1)


def _check_against_model(r, ref, K, what):
    st = ref["stats"]
    print("%s: cond(A) max %.3g, sub-solves %.3g (obs block %.3g), n_local %d..%d" % (
        what, st["cond"].max(), st["cv_cond"].max(), ref["ob_stats"]["cv_cond"].max(), st["n_local"].min(), st["n_local"].max()))
    _close(r["post"], ref["post"], what + " posterior members")
    _close(r["Yp"], ref["Yp"], what + " posterior obs perturbations")
    _close(r["ym"], ref["ym"], what + " posterior obs means")
    _check_diag(r["diag"], ref["diag"], what)
    assert np.array_equal(r["stats"][:, 0], st["n_local"].astype(np.float64)), what + ": n_local"
    assert np.abs(r["stats"][:, 1] - st["dfs"]).max() <= TOL * max(1.0, st["dfs"].max()), what + ": dfs"
    reached = st["n_local"] > 0
    assert np.all(r["stats"][reached, 2] >= 1) and np.all(r["stats"][:, 2] <= SWEEP_CAP), what + ": sweeps"
    if r["cv_stats"] is not None:
        sw, cond = r["cv_stats"][:, 0], r["cv_stats"][:, 1]
        assert np.array_equal(sw, np.round(sw)) and np.all(sw[reached] >= K) and np.all(sw <= K * SWEEP_CAP), what + ": cv_sweeps"
        assert np.all(sw[~reached] == 0) and np.all(cond[~reached] == 0), what + ": (0, 0) where no ob reaches"
        # max mu / min mu of symmetric matrices whose condition is <= 1e4: eigenvalues to a few ulps of the largest, the ratio to 1e-9
        assert np.abs(cond - st["cv_cond"]).max() <= 1e-9 * st["cv_cond"].max(), what + ": cv_cond"


# ---- 1. parity with the model at every case of the section ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,permuted", ALL_CASES)
def test_cross_validated_cycle_and_weights_match_the_model(ctx, case, permuted):
    (c, g), ref, plain = _case(case, permuted), _model(case, permuted), _plain_model(case, permuted)
    M, K = case[0], case[1]
    what = "M=%d K=%d P=%d%s" % (M, K, case[2], " permuted" if permuted else "")
    assert int(g.max()) + 1 == K and (permuted or np.array_equal(g, np.arange(M) % K))
    r = _cycle(ctx, c, g)
    _check_against_model(r, ref, K, what)
    T, w, st, cvs = _probe(ctx, c, g)
    _close(T, ref["T"], what + " T")
    _close(w, ref["w"], what + " w")
    assert np.array_equal(st, r["stats"]) and np.array_equal(cvs, r["cv_stats"]), "the probe runs the same solves"
    assert np.abs(T - np.swapaxes(T, 1, 2)).max() > 1e-6, "the case: T is not symmetric"
    # a kernel that ignores the setting would not pass: the cross-validated posterior is another one, its mean the plain filter's
    scale = np.abs(ref["post"]).max()
    assert np.abs(r["post"] - plain["post"]).max() > 1e-6 * scale, "the setting changed nothing"
    off = _cycle(ctx, c)
    assert np.abs(r["post"] - off["post"]).max() > 1e-6 * scale, "the setting changed nothing"
    _close(r["post"].mean(axis=1), off["post"].mean(axis=1), what + " posterior mean against the plain cycle's")
    _close(r["ym"], off["ym"], what + " posterior obs means against the plain cycle's")
    assert np.array_equal(off["stats"], r["stats"]), "n_local, dfs and sweeps are the full solve's"


# ---- 2. the properties -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _short_case():
    """Half-widths so short that some columns are out of every ob's reach."""
    c = lk.make_case(16, 12, 5, 7, 3, hw=(200.0, 500.0))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@pytest.mark.parametrize("f32", [False, True])
def test_columns_no_ob_reaches_keep_their_bits(ctx, f32):
    c = _short_case()
    g = np.arange(16) % 4
    X = np.ascontiguousarray(c["X"], dtype=np.float32) if f32 else c["X"]
    ref = cv.cv_cycle(dict(c, X=X.astype(np.float64)), g)
    out = ref["stats"]["n_local"] == 0
    assert out.any() and not out.all(), "the case: some columns are reached, some are not"
    for in_place in (False, True):
        r = _cycle(ctx, c, g, X=X, f32=f32, in_place=in_place)
        assert np.array_equal(r["post"][_rows(c, out)], X[_rows(c, out)]), "an unreached column changed"
        assert np.all(r["cv_stats"][out] == 0.0) and np.all(r["stats"][out] == 0.0)
        if not f32:
            _check_against_model(r, ref, 4, "short radii")
    T, w, st, _ = _probe(ctx, c, g)
    assert np.array_equal(T[out], np.broadcast_to(np.eye(16), T[out].shape)) and np.all(w[out] == 0.0), "the pair (I, 0)"


@pytest.mark.parametrize("case,permuted", [(MID, False), ((17, 4, 33, 5, 7, 17), False), (cv.PERMUTED, True)])
def test_twice_the_same_bits_and_in_place(ctx, case, permuted):
    c, g = _case(case, permuted)
    a, b = _cycle(ctx, c, g), _cycle(ctx, c, g)
    _same_bits(a, b, "run twice")
    assert np.array_equal(a["cv_stats"], b["cv_stats"])
    _same_bits(_cycle(ctx, c, g, in_place=True), a, "in place")
    _same_bits(_cycle(ctx, c, g, want_stats=False), a, "without the statistics array")
    Ta, wa, _, _ = _probe(ctx, c, g)
    Tb, wb, _, _ = _probe(ctx, c, g)
    assert np.array_equal(Ta, Tb) and np.array_equal(wa, wb)


@pytest.mark.parametrize("stride", [None, (2, 3)])
def test_float32_rows_are_the_float64_result_rounded_once(ctx, stride):
    c, g = _case((40, 8, 400, 6, 7, 3))
    X32 = np.ascontiguousarray(c["X"], dtype=np.float32)
    for in_place in (False, True):
        a = _cycle(ctx, c, g, X=X32, f32=True, in_place=in_place, stride=stride)
        b = _cycle(ctx, c, g, X=X32.astype(np.float64), in_place=in_place, stride=stride)
        assert a["post"].dtype == np.float32 and np.array_equal(a["post"], b["post"].astype(np.float32))
        _same_bits(a, b, "float32 against float64", keys=("ym", "Yp", "stats"))
        assert np.array_equal(a["cv_stats"], b["cv_stats"])


def test_a_nan_value_poisons_exactly_the_points_it_reaches(ctx):
    (c, g), ref = _case(MID), _model(MID)
    reach = (ref["rho"] != 0.0)
    ks = np.flatnonzero(c["assim"] & reach.any(axis=0) & ~reach.all(axis=0))
    assert ks.size, "the case: an ob that reaches some columns and not others"
    k = int(ks[np.argmax(np.minimum(reach[:, ks].sum(axis=0), (~reach[:, ks]).sum(axis=0)))])
    hit = reach[:, k]
    value = c["value"].copy()
    value[k] = np.nan
    a, b = _cycle(ctx, c, g), _cycle(ctx, c, g, value=value)
    assert np.isnan(b["post"][_rows(c, hit)]).all(), "NaN means where it reaches"
    assert np.array_equal(b["post"][_rows(c, ~hit)], a["post"][_rows(c, ~hit)]), "the NaN reached a column out of its ob's reach"
    assert np.array_equal(a["stats"], b["stats"]) and np.array_equal(a["cv_stats"], b["cv_stats"])
    T0, w0, _, _ = _probe(ctx, c, g)
    T1, w1, _, _ = _probe(ctx, c, g, value=value)
    assert np.array_equal(T0, T1), "a NaN value reached T: the perturbations stay finite"
    assert np.isnan(w1[hit]).all() and np.array_equal(w1[~hit], w0[~hit])
    rho_o = lk.taper(c["ob_lat"], c["ob_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"])
    ob_hit = rho_o[:, k] != 0.0
    assert ob_hit.any() and not ob_hit.all()
    assert np.isnan(b["ym"][ob_hit]).all() and np.array_equal(b["ym"][~ob_hit], a["ym"][~ob_hit])
    assert np.all(np.isfinite(b["Yp"])) and np.array_equal(b["Yp"], a["Yp"])


@pytest.mark.parametrize("case", [MID, (40, 8, 400, 6, 7, 3)])
def test_weight_stride_interpolates_the_cross_validated_pairs(ctx, case):
    stride = (2, 3)
    (c, g), ref = _case(case), _model(case, False, stride)
    r = _cycle(ctx, c, g, stride=stride)
    _check_against_model(r, ref, case[1], "weight_stride")
    assert np.abs(ref["post"] - _model(case)["post"]).max() > 1e-6 * np.abs(ref["post"]).max(), "the case: interpolation matters"
    _same_bits(r, _cycle(ctx, c, g), "the obs block does not see the mesh", keys=("ym", "Yp"))


def test_max_local_obs_caps_the_solves_under_cross_validation(ctx):
    c, g = _case(MID)
    caps = (8,)
    with cp.capped(None, caps) as log:
        ref = cv.cv_cycle(c, g)
    assert log[0]["bites"].any() and log[1]["bites"].any()
    r = _cycle(ctx, c, g, caps=caps)
    _check_against_model(r, ref, MID[1], "max_local_obs")
    assert np.abs(r["post"] - _model(MID)["post"]).max() > 1e-6 * np.abs(ref["post"]).max(), "the cap changed nothing"


def test_rtps_and_rtpp_act_as_on_an_interpolated_pair(ctx):
    from efa_xray_amd import _lib
    (c, g), ref = _case(MID), _model(MID)
    ctx.set_relaxation(_lib.RELAX_RTPS, 0.9)
    r = _cycle(ctx, c, g)
    _close(r["post"], relax(c["X"], ref["post"], rtps=0.9), "rtps 0.9")
    _close(r["Yp"], ref["Yp"], "the obs block is not relaxed")
    ctx.set_relaxation(_lib.RELAX_RTPP, 0.5)
    r = _cycle(ctx, c, g)
    _close(r["post"], cv.cv_cycle(c, g, rtpp=0.5)["post"], "rtpp 0.5")
    _close(r["post"], relax(c["X"], ref["post"], rtpp=0.5), "rtpp 0.5, the closed form")
    _close(r["Yp"], ref["Yp"], "the obs block is not relaxed")
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)


def test_outlier_threshold_equals_cleared_flags(ctx):
    t = 3.0
    case = (17, 4, 33, 5, 7, 17)
    c, g = _case(case)
    value, bad = qc.inject(c["HX"], c["value"], c["error"], c["assim"], t, 3, seed=17)
    import _etkf as ek
    ym, Yp = ek.ob_priors(c["HX"])
    assert qc.clear_of_threshold(ym, Yp, value, c["error"], t)
    flags = qc.masked_flags(c["HX"], value, c["error"], c["assim"], t)
    assert not flags[bad].any() and flags.any()
    ref = cv.cv_cycle(dict(c, value=value), g, assim=flags)
    ctx.set_outlier_threshold(t)
    try:
        r = _cycle(ctx, c, g, value=value)
    finally:
        ctx.set_outlier_threshold(None)
    assert np.array_equal(r["diag"]["assimilated"], flags), "rejected set"
    _same_bits(r, _cycle(ctx, c, g, value=value, assim=flags), "outlier check against cleared flags")
    _check_against_model(r, ref, case[1], "outlier check")


@pytest.mark.parametrize("f32", [False, True])
def test_set_and_cleared_gives_the_plain_run_bit_for_bit(ctx, f32):
    c, g = _case(MID)
    X = np.ascontiguousarray(c["X"], dtype=np.float32) if f32 else c["X"]
    for stride in (None, (2, 3)):
        plain = _cycle(ctx, c, X=X, f32=f32, stride=stride)
        on = _cycle(ctx, c, g, X=X, f32=f32, stride=stride)             # sets and clears
        assert np.any(on["post"] != plain["post"])
        _same_bits(_cycle(ctx, c, X=X, f32=f32, stride=stride), plain, "set and cleared")
    T0, w0, st0, _ = _probe(ctx, c)
    _probe(ctx, c, g)
    T1, w1, st1, _ = _probe(ctx, c)
    assert np.array_equal(T0, T1) and np.array_equal(w0, w1) and np.array_equal(st0, st1)


# ---- 3. the refusals, each followed by a served call; what ignores the setting ------------------------------------------------------
def _raw_set(ctx, groups, M, ngroups, stats_addr=None, nsolve=0):
    """The C entry as it is (the Python wrapper derives ngroups from the labels): its status."""
    from efa_xray_amd import _lib
    g = np.ascontiguousarray(groups, dtype=np.int32)
    return ctx.lib.efa_ctx_set_letkf_cross_validation(ctx.handle, g.ctypes.data_as(_lib.c_int32_p), int(M), int(ngroups),
                                                      None if stats_addr is None else ctypes.c_void_p(stats_addr), int(nsolve))


def test_the_setter_and_the_entries_refuse_and_the_context_goes_on(ctx):
    from efa_xray_amd import _lib
    (c, g), ref = _case(MID), _model(MID)
    M, P, N, ncol = c["M"], c["P"], c["X"].shape[0], c["ncol"]
    want = _cycle(ctx, c, g)
    plain = _cycle(ctx, c)

    def served(what):
        _same_bits(_cycle(ctx, c, g), want, "after " + what)
        _same_bits(_cycle(ctx, c), plain, "the setting is off after " + what)

    def refused(what, fn, *needles):
        with pytest.raises(_lib.EfaError) as e:
            fn()
        assert e.value.status == _lib.EFA_ERR_INVALID, what
        for s in needles:
            assert s in str(e.value), "%s: %r not in %r" % (what, s, str(e.value))
        ctx.set_letkf_cross_validation(None)
        ctx.set_letkf_inflation(None)
        ctx.set_letkf_control(None)
        served(what)

    # the setter: the setting stays as it was (here: off)
    refused("one group", lambda: ctx.set_letkf_cross_validation(np.zeros(M, dtype=np.int32)), "ngroups")
    refused("a negative label", lambda: ctx.set_letkf_cross_validation(np.where(np.arange(M) == 3, -1, g)), "label")
    refused("an unused label", lambda: ctx.set_letkf_cross_validation(np.where(g == 2, 5, g)), "unused")
    refused("an independent set of one", lambda: ctx.set_letkf_cross_validation((np.arange(M) == 0).astype(np.int32)), "independent")
    refused("three members", lambda: ctx.set_letkf_cross_validation(np.array([0, 1, 0])), "M=3")
    refused("137 members", lambda: ctx.set_letkf_cross_validation(np.arange(137) % 2), "M=137")
    spare = ctx.empty((ncol + 1, 2))
    base = ctx._addr(spare)
    base = int(getattr(base, "value", base))
    for what, status in (("a label beyond ngroups", _raw_set(ctx, np.where(np.arange(M) == 3, 4, g), M, 4)),
                         ("ngroups 1", _raw_set(ctx, np.zeros(M), M, 1)),
                         ("a misaligned statistics array", _raw_set(ctx, g, M, 4, base + 4, ncol)),
                         ("a negative nsolve", _raw_set(ctx, g, M, 4, base, -1))):
        assert status == _lib.EFA_ERR_INVALID, what
        served(what)
    # a refusal leaves the earlier setting in force
    two = np.arange(M) % 2
    T2, w2, _, _ = _probe(ctx, c, two)
    ctx.set_letkf_cross_validation(two)
    with pytest.raises(_lib.EfaError):
        ctx.set_letkf_cross_validation(np.zeros(M, dtype=np.int32))
    ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
    T, w, _ = ctx.letkf_weights(M, P, ym, Yp, c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                                c["grid_lon"])
    assert np.array_equal(T, T2) and np.array_equal(w, w2), "the earlier setting was lost"
    ctx.set_letkf_cross_validation(None)
    served("a refused change of the setting")

    # the entries: an M or nsolve that differs from the call's
    def with_setting(groups, nstats, fn):
        def run():
            ctx.set_letkf_cross_validation(groups, None if nstats is None else ctx.empty((nstats, 2)))
            fn()
        return run

    other = lk.make_case(17, 33, 5, 7, 3)
    refused("another M", with_setting(g, None, lambda: _cycle(ctx, other)), "members")
    refused("another nsolve", with_setting(g, ncol + 1, lambda: _cycle(ctx, c)), "solve points")
    refused("nsolve of the grid with a mesh", with_setting(g, ncol, lambda: _cycle(ctx, c, stride=(2, 3))), "solve points")
    refused("another M at the probe", with_setting(g, None, lambda: _probe(ctx, other)), "members")
    refused("another nsolve at the probe", with_setting(g, ncol, lambda: _probe(ctx, c, lat=c["grid_lat"][:2], lon=c["grid_lon"][:2])),
            "solve points")

    # an inflation field or a control beside the setting
    held = [ctx.to_device(np.ones(ncol)), ctx.to_device(np.zeros(N)), ctx.empty((N,)), ctx.to_device(np.zeros(P)), ctx.empty((P,))]

    def with_inflation(run=lambda: _cycle(ctx, c)):
        ctx.set_letkf_cross_validation(g)
        ctx.set_letkf_inflation(held[0], None, P, 0.0, 1e-2, 1e2, None)
        run()

    def with_control():
        ctx.set_letkf_cross_validation(g)
        ctx.set_letkf_control(*held[1:])
        _cycle(ctx, c)

    def probe_with_inflation():
        with_inflation(lambda: _probe(ctx, c))

    refused("an inflation field", with_inflation, "inflation")
    refused("a control", with_control, "control")
    refused("an inflation field at the probe", probe_with_inflation, "inflation")


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
    ctx.set_letkf_cross_validation(np.arange(M) % 4)
    with pytest.raises(_lib.EfaError) as e:
        slab_cycle()
    assert e.value.status == _lib.EFA_ERR_INVALID and "cross validation" in str(e.value)
    ctx.set_letkf_cross_validation(None)
    assert np.array_equal(slab_cycle(), want), "the slab cycle after the refusal"


def test_the_entries_that_ignore_the_setting_keep_their_bits(ctx):
    from efa_xray_amd import _lib
    c, g = _case(MID)
    N, M, P = c["X"].shape[0], c["M"], c["P"]

    def ensrf():
        Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
        post = ctx.empty((N, M))
        ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
        ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, c["value"], c["error"], c["assim"], loc_mode=_lib.LOC_GC, ob_lat=c["ob_lat"],
                        ob_lon=c["ob_lon"], ob_halfwidth=c["ob_hw"], grid_lat=c["grid_lat"], grid_lon=c["grid_lon"], n_lead=c["n_lead"],
                        obs_block_out=True)
        return post.download(), ym.download(), Yp.download()

    def interp_apply():
        nn = li.axis_nodes(c["ny"], 2).size * li.axis_nodes(c["nx"], 3).size
        rng = np.random.default_rng(3)
        Tw = np.zeros((nn, M, M + 1))
        Tw[:, :, :M] = np.eye(M) + 0.01 * rng.standard_normal((nn, M, M))
        Tw[:, :, M] = 0.1 * rng.standard_normal((nn, M))
        Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
        post = ctx.empty((N, M))
        ctx.letkf_interp_apply(N, M, Xd, post, (c["ny"], c["nx"]), (2, 3), c["n_lead"], ctx.to_device(Tw))
        return (post.download(),)

    for fn in (ensrf, interp_apply):
        off = fn()
        _cycle(ctx, c, g)                                   # a cross-validated cycle before it
        after = fn()
        ctx.set_letkf_cross_validation(g)                   # ... and the setting left on, sized for this M
        try:
            on = fn()
            ctx.set_letkf_cross_validation(np.arange(9) % 3, ctx.empty((5, 2)))      # ... and for another call altogether
            on2 = fn()
        finally:
            ctx.set_letkf_cross_validation(None)
        for a, b, d, e in zip(off, after, on, on2):
            assert np.array_equal(a, b) and np.array_equal(a, d) and np.array_equal(a, e), fn.__name__


# ---- 4. the class ------------------------------------------------------------------------------------------------------------------------
def _api_model(state, obs, lat, lon, g, f, **kw):
    HX = np.asarray(f.compute_ob_estimates(), dtype=np.float64)
    ny, nx = lat.shape
    c = dict(X=state.to_vect().astype(np.float64), HX=HX, value=np.array([o.value for o in obs]), error=np.array([o.error for o in obs]),
             assim=np.array([o.assimilate_this for o in obs]), ob_lat=np.array([o.lat for o in obs]), ob_lon=np.array([o.lon for o in obs]),
             ob_hw=np.array([o.localize_radius for o in obs]), grid_lat=lat, grid_lon=lon, n_lead=4, ny=ny, nx=nx)
    return cv.cv_cycle(c, g, **kw)


@pytest.mark.parametrize("form", ["int", "array"])
def test_letkf_class_against_the_model(ctx, form):
    from efa_xray_amd import LETKF, SlabLETKF
    from test_gpu_letkf_cap import _api_case
    state, obs, lat, lon = _api_case()
    M = 12
    arg = 3 if form == "int" else cv.permuted_labels(M, 4, 9)
    g = np.arange(M) % 3 if form == "int" else arg
    f = LETKF(state, obs, verbose=False, cross_validation=arg)
    ref = _api_model(state, obs, lat, lon, g, f)
    post, _ = f.update()
    _close(post.to_vect(), ref["post"], "LETKF.update posterior")
    ls = f.last_solve
    assert sorted(ls) == ["cv_cond", "cv_sweeps", "dfs", "n_local", "sweeps"] and all(ls[k].shape == (6, 7) for k in ls)
    assert ls["cv_sweeps"].dtype == np.int64 and ls["n_local"].dtype == np.int64
    K = int(g.max()) + 1
    reached = ref["stats"]["n_local"].reshape(6, 7) > 0
    assert np.array_equal(ls["n_local"].reshape(-1), ref["stats"]["n_local"])
    assert np.all(ls["cv_sweeps"][reached] >= K) and np.all(ls["cv_sweeps"] <= K * SWEEP_CAP) and np.all(ls["cv_sweeps"][~reached] == 0)
    assert np.abs(ls["cv_cond"].reshape(-1) - ref["stats"]["cv_cond"]).max() <= 1e-9 * ref["stats"]["cv_cond"].max()
    # SlabLETKF without its options is LETKF; the setting is gone after update()
    s2, o2, _, _ = _api_case()
    p2, _ = SlabLETKF(s2, o2, verbose=False, cross_validation=arg).update()
    assert np.array_equal(p2.to_vect(), post.to_vect())
    s3, o3, _, _ = _api_case()
    h = LETKF(s3, o3, verbose=False)
    p3, _ = h.update()
    assert "cv_sweeps" not in h.last_solve, "the setting outlived update()"
    assert np.abs(p3.to_vect() - post.to_vect()).max() > 1e-6 * np.abs(ref["post"]).max()
    _close(p3.to_vect().mean(axis=1), post.to_vect().mean(axis=1), "the posterior mean is the plain filter's")


def test_letkf_class_combines_and_clears_the_setting_after_an_exception(ctx):
    from efa_xray_amd import LETKF
    from test_gpu_letkf_cap import _api_case
    state, obs, lat, lon = _api_case(dtype=np.float32)
    f = LETKF(state, obs, verbose=False, cross_validation=4, max_local_obs=6, weight_stride=(2, 3), rtps=0.9, outlier_threshold=4.0)
    post, _ = f.update()
    assert post.to_vect().dtype == np.float32 and np.all(np.isfinite(post.to_vect()))
    ls = f.last_solve
    assert ls["cv_sweeps"].shape == ls["n_local"].shape == (ls["node_y"].size, ls["node_x"].size) and np.all(ls["n_local"] <= 6)
    s2, o2, _, _ = _api_case()
    want, _ = LETKF(s2, o2, verbose=False).update()
    s3, o3, _, _ = _api_case()
    bad = LETKF(s3, o3, verbose=False, cross_validation=4)
    o3[0].error = -1.0
    with pytest.raises(Exception):
        bad.update()
    s4, o4, _, _ = _api_case()
    got, _ = LETKF(s4, o4, verbose=False).update()
    assert np.array_equal(got.to_vect(), want.to_vect()), "the setting outlived the exception"
