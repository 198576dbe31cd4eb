"""The LETKF under vertical, temporal and cross-variable localisation on the MI355X against the NumPy model of
tests/_letkf_slab.py: the pairs of efa_letkf_slab_weights_dev per (point, group), the posterior members, the posterior obs block,
the diagnostics and the statistics to 1e-10 of the largest magnitude of each array (the project's bound for this filter, claimed up
to cond(A) <= 1e4: asserted from the model at every (point, group)); every factor alone; all factors 1 against the plain call bit
for bit; the grouping; a zero impact; a NaN value behind a zero factor; float32 rows, in place, relaxation, the outlier check,
determinism; weight interpolation per group; the refusals; and the Python class.  Every test restores the shared context."""
import functools

import numpy as np
import pytest

import _letkf as lk
import _letkf_slab as ls
import _outlier as qc
from _letkf_gpu import TOL, SWEEP_CAP, COND_CAP, _reset, _obs_block, _close, _check_diag, _same_bits
from test_relaxation_host import relax

pytestmark = pytest.mark.gpu

# (M, P, ny, nx, nvars, ntimes)
SIZES = [(2, 1, 3, 5, 1, 2), (3, 5, 3, 5, 2, 2), (16, 64, 5, 7, 2, 3), (17, 33, 5, 7, 3, 3), (40, 400, 6, 7, 2, 3), (80, 300, 5, 6, 2, 2),
         (136, 300, 3, 6, 1, 2)]
MID = (16, 64, 5, 7, 2, 3)


@pytest.fixture
def ctx():
    from efa_xray_amd import _lib
    c = _reset(_lib.get_context(0))
    yield c
    _reset(c)


def _freeze(c):
    for v in list(c.values()) + list(c.get("loc", {}).values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _case(M, P, ny, nx, nvars, ntimes, parts="vtc", seed=0):
    """The seeded case, computed once and left unchanged."""
    return _freeze(ls.make_case(M, P, ny, nx, nvars, ntimes, seed=seed, parts=parts))


def _run_model(c, loc=None, stride=None, **over):
    g = dict(c, **over)
    return ls.slab_cycle(g["X"], g["HX"], g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"], g["grid_lat"],
                         g["grid_lon"], g["n_lead"], g["loc"] if loc is None else loc, stride=stride, shape=(g["ny"], g["nx"]))


@functools.lru_cache(maxsize=None)
def _model(M, P, ny, nx, nvars, ntimes, parts="vtc", seed=0, stride=None):
    return _run_model(_case(M, P, ny, nx, nvars, ntimes, parts, seed), stride=stride)


def _set(ctx, c, loc=None):
    """The context's two settings from the case's `loc` (a part that is absent turns its setting off)."""
    loc = c["loc"] if loc is None else loc
    P, n_lead = c["P"], c["n_lead"]
    if loc.get("lead_vert") is not None:
        ctx.set_vertical_localization(loc["lead_vert"], loc["ob_vert"], loc["ob_vert_halfwidth"])
    else:
        ctx.set_vertical_localization(None)
    kw = {k: loc.get(k) for k in ("lead_time", "ob_time", "ob_time_halfwidth", "lead_var", "ob_group", "ob_var", "impact")}
    ctx.set_slab_localization(n_lead, P, **kw)


def _cycle(ctx, c, in_place=False, f32=False, X=None, stride=None, plain=False, ngroups=None, **over):
    """efa_letkf_slab_cycle_dev (or the plain call): dict of posterior, obs block, diagnostics, statistics (ngroups, npts, 3)."""
    g = dict(c, **over)
    X = g["X"] if X is None else X
    N, M = X.shape
    P = g["P"]
    dt = np.float32 if f32 else np.float64
    Xd = ctx.to_device(np.ascontiguousarray(X, dtype=dt), dtype=dt)
    post = Xd if in_place else ctx.empty((N, M), dtype=dt)
    ym, Yp, ym0, Yp0 = _obs_block(ctx, g["HX"], M)
    npts = g["ncol"]
    mesh = {}
    if stride is not None:
        from efa_xray_amd import _lib
        cut = (min(stride[0], max(g["ny"] - 1, 1)), min(stride[1], max(g["nx"] - 1, 1)))
        npts = _lib.letkf_mesh_nodes(g["ny"], cut[0]).size * _lib.letkf_mesh_nodes(g["nx"], cut[1]).size
        mesh = dict(shape=(g["ny"], g["nx"]), stride=stride)
    if ngroups is None:
        ngroups = 1 if plain else ctx.letkf_slab_groups(g["n_lead"])[1]
    stats = ctx.empty((ngroups * npts, 3))
    call = ctx.letkf_cycle if plain else ctx.letkf_slab_cycle
    diag = call(N, M, P, Xd, post, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"], g["grid_lat"],
                g["grid_lon"], g["n_lead"], obs_block_out=True, col_stats=stats, f32=f32, **mesh)
    return dict(post=post.download(), ym=ym.download()[:P], Yp=Yp.download()[:P], diag=diag,
                stats=stats.download().reshape(ngroups, npts, 3), ym0=ym0, Yp0=Yp0)


def _probe(ctx, c, **over):
    g = dict(c, **over)
    M, P = g["M"], g["P"]
    ym, Yp, _, _ = _obs_block(ctx, g["HX"], M)
    return ctx.letkf_slab_weights(M, P, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"], g["grid_lat"],
                                  g["grid_lon"], g["n_lead"])


def _check_stats(stats, st, what):
    assert st["cond"].max() <= COND_CAP, "cond(A) = %g: the float64 bound of 1e-10 is claimed up to 1e4" % st["cond"].max()
    assert stats.shape[:2] == st["n_local"].shape, what + ": statistics are laid out [ngroups][npts][3]"
    assert np.array_equal(stats[..., 0], st["n_local"].astype(np.float64)), what + ": n_local"
    assert np.abs(stats[..., 1] - st["dfs"]).max() <= TOL * max(1.0, st["dfs"].max()), what + ": dfs"
    reached = st["n_local"] > 0
    assert np.all(stats[..., 2][reached] >= 1) and np.all(stats[..., 2] < SWEEP_CAP) and np.all(stats[..., 2][~reached] == 0)


def _check_against_model(r, ref, what, post=None):
    st = ref["stats"]
    print("%s: %d groups, cond(A) max %.3g, n_local %d..%d, unreached (point, group) %d of %d" % (
        what, len(ref["rep"]), st["cond"].max(), st["n_local"].min(), st["n_local"].max(), int((st["n_local"] == 0).sum()),
        st["n_local"].size))
    _check_stats(r["stats"], st, what)
    _close(r["post"], ref["post"] if post is None else post, what + " posterior members")
    _close(r["Yp"], ref["Yp"], what + " posterior obs perturbations")
    _close(r["ym"], ref["ym"], what + " posterior obs means")
    _check_diag(r["diag"], ref["diag"], what)


def _rows(c, slabs, cols):
    return (np.asarray(slabs)[:, None] * c["ncol"] + np.asarray(cols)[None, :]).reshape(-1)


# ---- every size with all three factors; one size with each factor alone ---------------------------------------------------------------
@pytest.mark.parametrize("size,parts", [(s, "vtc") for s in SIZES] + [(MID, p) for p in ("v", "t", "c")])
def test_cycle_and_weights_match_the_model(ctx, size, parts):
    c, ref = _case(*size, parts=parts), _model(*size, parts=parts)
    _set(ctx, c)
    group_of, ng = ctx.letkf_slab_groups(c["n_lead"])
    assert ng == len(ref["rep"]) and np.array_equal(group_of, ref["group_of"]), "efa_letkf_slab_groups against the NumPy rule"
    if size == MID:
        assert ng == {"vtc": 6, "v": 2, "t": 3, "c": 2}[parts]
    r = _cycle(ctx, c)
    assert ctx.get_option("phase_a_kind") == 8
    _check_against_model(r, ref, "M=%d P=%d %s" % (size[0], size[1], parts))
    T, w, st = _probe(ctx, c)
    _close(T, ref["T"], "T")
    _close(w, ref["w"], "w")
    assert np.array_equal(st, r["stats"])
    assert np.array_equal(T, np.swapaxes(T, 2, 3)), "T is mirrored: symmetric to the bit"
    if size[1] > 3 and "v" in parts and "c" in parts:       # the three special obs are there, and do something
        lo = c["loc"]
        assert np.isnan(lo["ob_vert"][0]) and np.isnan(lo["ob_time"][1]) and lo["ob_group"][2] == -1 and lo["ob_var"][2] == -1
    _same_bits(r, _cycle(ctx, c), "twice")
    _same_bits(r, _cycle(ctx, c, in_place=True), "post_dev == X_dev")


# ---- every S = 1 exactly: one group, the plain call bit for bit ---------------------------------------------------------------------
def test_all_factors_one_equals_the_plain_call_bit_for_bit(ctx):
    from efa_xray_amd import _lib
    c = _case(17, 33, 5, 7, 3, 3)
    P, n_lead = c["P"], c["n_lead"]
    fresh = _lib.Context(0)
    try:
        want = _cycle(fresh, c, plain=True)
        want32 = _cycle(fresh, c, plain=True, f32=True, X=c["X"].astype(np.float32))
    finally:
        fresh.close()
    ones = dict(lead_vert=np.arange(n_lead, dtype=float), ob_vert=np.full(P, np.nan), ob_vert_halfwidth=np.ones(P),
                lead_time=np.arange(n_lead, dtype=float), ob_time=np.zeros(P), ob_time_halfwidth=np.full(P, np.nan),
                impact=np.ones((3, 3)), lead_var=np.repeat(np.arange(3), 3), ob_group=np.zeros(P, int), ob_var=np.zeros(P, int))
    vert_only = {k: ones[k] for k in ("lead_vert", "ob_vert", "ob_vert_halfwidth")}
    for name, loc in (("both settings", ones), ("the vertical setting alone", vert_only)):
        _set(ctx, c, loc)
        group_of, ng = ctx.letkf_slab_groups(n_lead)
        assert ng == 1 and not group_of.any()
        r = _cycle(ctx, c)
        _same_bits(dict(r, stats=r["stats"][0]), dict(want, stats=want["stats"][0]), name)
        r32 = _cycle(ctx, c, f32=True, X=c["X"].astype(np.float32))
        _same_bits(dict(r32, stats=r32["stats"][0]), dict(want32, stats=want32["stats"][0]), name + ", float32")
        assert np.all(ctx.slab_factor_table(P, n_lead) == 1.0) if "impact" in loc else True


# ---- grouping --------------------------------------------------------------------------------------------------------------------
def test_slabs_of_a_group_share_one_solve(ctx):
    c = _case(16, 64, 5, 7, 2, 3, parts="v")
    ncol = c["ncol"]
    loc = dict(c["loc"], lead_vert=np.array([0.0, 0.0, 1.0, 1.0, 2.0, 2.0]) * 300.0 + 250.0)
    X = np.array(c["X"])
    for s in (1, 3, 5):                 # the second slab of every group holds the rows of the first
        X[s * ncol:(s + 1) * ncol] = X[(s - 1) * ncol:s * ncol]
    _set(ctx, c, loc)
    group_of, ng = ctx.letkf_slab_groups(6)
    want, _ = ls.groups(6, c["P"], loc)
    assert ng == 3 and list(group_of) == [0, 0, 1, 1, 2, 2] and np.array_equal(group_of, want)
    ref = _run_model(c, loc=loc, X=X)
    for kw in (dict(), dict(stride=(2, 2))):
        r = _cycle(ctx, c, X=X, **kw)
        for s in (1, 3, 5):
            assert np.array_equal(r["post"][s * ncol:(s + 1) * ncol], r["post"][(s - 1) * ncol:s * ncol]), "two slabs of a group differ"
    _check_against_model(_cycle(ctx, c, X=X), ref, "three groups of two slabs")
    assert not np.array_equal(r["post"][0:ncol], r["post"][2 * ncol:3 * ncol])


# ---- a zero impact: the other variable's rows and statistics ---------------------------------------------------------------------
@pytest.mark.parametrize("rtps", [None, 0.9])
def test_a_zero_impact_returns_the_other_variable_bit_for_bit(ctx, rtps):
    from efa_xray_amd import _lib
    c = _case(16, 64, 5, 7, 2, 3, parts="c")
    P, ncol = c["P"], c["ncol"]
    loc = dict(c["loc"], impact=np.array([[1.0, 0.0], [1.0, 1.0]]), ob_group=np.zeros(P, int), ob_var=np.zeros(P, int))     # only t obs, t -> q = 0
    ref = _run_model(c, loc=loc)
    assert list(ref["group_of"]) == [0, 0, 0, 1, 1, 1]
    _set(ctx, c, loc)
    if rtps:
        ctx.set_relaxation(_lib.RELAX_RTPS, rtps)
    q, t = np.arange(3 * ncol, 6 * ncol), np.arange(3 * ncol)
    for kw in (dict(), dict(in_place=True), dict(stride=(2, 2)), dict(f32=True, X=c["X"].astype(np.float32))):
        r = _cycle(ctx, c, **kw)
        X = kw.get("X", c["X"])
        assert np.array_equal(r["post"][q], X[q]), "a q row changed (%r)" % (kw,)
        assert not r["stats"][1].any() and r["stats"][0, :, 0].any(), "the q group's statistics are (0, 0, 0)"
        assert not np.array_equal(r["post"][t], X[t])
    want = ref["post"] if not rtps else relax(c["X"], ref["post"], rtps=rtps)
    _close(_cycle(ctx, c)["post"], want, "t rows")


# ---- a NaN value behind a zero factor --------------------------------------------------------------------------------------------
def test_a_nan_value_stays_out_of_the_groups_its_factor_is_zero_on(ctx):
    c, ref = _case(*MID), _model(*MID)
    S, rep, group_of, ncol = ref["S"], ref["rep"], ref["group_of"], c["ncol"]
    Sg = S[:, rep]                                                           # (P, ngroups)
    cand = np.flatnonzero(c["assim"] & (Sg == 0.0).any(axis=1) & (Sg != 0.0).any(axis=1) & (ref["rho_h"] != 0.0).any(axis=0))
    assert cand.size, "no assimilated ob with a zero factor on one group and a non-zero one on another: pick another seed"
    k = int(cand[0])
    value = np.array(c["value"])
    value[k] = np.nan
    _set(ctx, c)
    a, b = _cycle(ctx, c), _cycle(ctx, c, value=value)
    T0, w0, _ = _probe(ctx, c)
    T1, w1, _ = _probe(ctx, c, value=value)
    assert np.array_equal(T0, T1), "a NaN value reached T"
    assert np.array_equal(a["stats"], b["stats"])
    for g in range(len(rep)):
        slabs = np.flatnonzero(group_of == g)
        hit = (ref["rho_h"][:, k] * Sg[k, g]) != 0.0
        if Sg[k, g] == 0.0:
            assert not hit.any()
        assert np.isnan(b["post"][_rows(c, slabs, np.flatnonzero(hit))]).all(), "group %d: a reached column is not NaN" % g
        keep = _rows(c, slabs, np.flatnonzero(~hit))
        assert np.array_equal(b["post"][keep], a["post"][keep]), "group %d: an unreached column changed" % g
        assert np.isnan(w1[g][hit]).all() and np.array_equal(w1[g][~hit], w0[g][~hit])


# ---- float32, relaxation, the outlier check ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rtps", [None, 0.9])
def test_float32_rows_are_the_float64_result_rounded_once(ctx, rtps):
    from efa_xray_amd import _lib
    c = _case(40, 400, 6, 7, 2, 3)
    _set(ctx, c)
    if rtps:
        ctx.set_relaxation(_lib.RELAX_RTPS, rtps)
    X32 = c["X"].astype(np.float32)
    for kw in (dict(), dict(in_place=True), dict(stride=(2, 3))):
        a = _cycle(ctx, c, X=X32, f32=True, **kw)
        b = _cycle(ctx, c, X=X32.astype(np.float64), **kw)
        assert a["post"].dtype == np.float32 and np.array_equal(a["post"], b["post"].astype(np.float32))
        _same_bits(a, b, "float32 against float64", keys=("ym", "Yp", "stats"))


@pytest.mark.parametrize("kind,alpha", [("rtpp", 0.5), ("rtps", 0.9)])
def test_relaxation_matches_the_closed_form_on_the_model_posterior(ctx, kind, alpha):
    from efa_xray_amd import _lib
    c, ref = _case(*MID), _model(*MID)
    _set(ctx, c)
    ctx.set_relaxation(_lib.RELAX_RTPP if kind == "rtpp" else _lib.RELAX_RTPS, alpha)
    want = relax(c["X"], ref["post"], **{kind: alpha})
    for in_place in (False, True):
        r = _cycle(ctx, c, in_place=in_place)
        _close(r["post"], want, "%s %s" % (kind, "in place" if in_place else "out of place"))
        _close(r["Yp"], ref["Yp"], "the obs block is not relaxed")
    T, _, _ = _probe(ctx, c)
    _close(T, ref["T"], "the probe's T is not relaxed")


def test_outlier_check_rejects_exactly_and_equals_cleared_flags(ctx):
    import _etkf as ek
    t = 3.0
    c = _case(17, 33, 5, 7, 3, 3)
    ym, Yp = ek.ob_priors(c["HX"])
    value, bad = qc.inject(c["HX"], c["value"], c["error"], c["assim"], t, 3, seed=17)
    assert qc.clear_of_threshold(ym, Yp, value, c["error"], t)
    flags = qc.masked_flags(c["HX"], value, c["error"], c["assim"], t)
    assert not flags[bad].any() and flags.any()
    _set(ctx, c)
    ctx.set_outlier_threshold(t)
    r = _cycle(ctx, c, value=value)
    ctx.set_outlier_threshold(None)
    assert np.array_equal(r["diag"]["assimilated"], flags), "rejected set"
    _same_bits(r, _cycle(ctx, c, value=value, assim=flags), "outlier check against cleared flags")
    _check_against_model(r, _run_model(c, value=value, assim=flags), "outlier check")


# ---- weight interpolation per group ---------------------------------------------------------------------------------------------------
INTERP = [((16, 64, 5, 7, 2, 3), (2, 2)), ((40, 200, 9, 10, 2, 2), (4, 4)), ((136, 300, 3, 6, 1, 2), (2, 3)), ((16, 64, 5, 7, 2, 3), (8, 8))]


@pytest.mark.parametrize("size,stride", INTERP)
def test_interpolated_weights_match_the_model_per_group(ctx, size, stride):
    c = _case(*size)
    cut = (min(stride[0], size[2] - 1), min(stride[1], size[3] - 1))
    ref = _model(*size, stride=cut)
    _set(ctx, c)
    plain = _cycle(ctx, c)
    r = _cycle(ctx, c, stride=stride)
    assert ctx.get_option("phase_a_kind") == 9
    _check_stats(r["stats"], ref["stats"], "node statistics")
    _close(r["post"], ref["post"], "posterior members, stride %r" % (stride,))
    _same_bits(r, plain, "the obs block and the diagnostics are the plain slab call's", keys=("ym", "Yp"))
    _same_bits(r, _cycle(ctx, c, stride=stride, in_place=True), "in place", keys=("post", "ym", "Yp", "stats"))
    if stride != cut:
        _same_bits(r, _cycle(ctx, c, stride=cut), "a stride beyond the axis is cut to it")
    un = ~ref["reached"]
    for g in range(len(ref["rep"])):
        rows = _rows(c, np.flatnonzero(ref["group_of"] == g), np.flatnonzero(un[g]))
        assert np.array_equal(r["post"][rows], c["X"][rows]), "group %d: a column whose corners are all unreached changed" % g
    one = _cycle(ctx, c, stride=(1, 1))
    assert ctx.get_option("phase_a_kind") == 8
    _same_bits(one, plain, "stride (1, 1) is the plain slab call")


# ---- the refusals, and the context afterwards ------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    from efa_xray_amd import _lib
    c = _case(17, 33, 5, 7, 3, 3)
    N, P, n_lead = c["X"].shape[0], c["P"], c["n_lead"]
    fresh = _lib.Context(0)
    try:
        _set(fresh, c)
        want = _cycle(fresh, c)
    finally:
        fresh.close()
    ng = want["stats"].shape[0]
    field = ctx.to_device(np.tile([1.0, 0.6], (N, 1)))
    lo = c["loc"]
    other_P = dict(lo, ob_vert=lo["ob_vert"][:-1], ob_vert_halfwidth=lo["ob_vert_halfwidth"][:-1])
    big = ls.make_case(137, 20, 3, 5, 1, 2)

    def wrong_P():
        _set(ctx, c)
        ctx.set_vertical_localization(other_P["lead_vert"], other_P["ob_vert"], other_P["ob_vert_halfwidth"])

    def wrong_lead():
        _set(ctx, c)
        ctx.set_vertical_localization(np.arange(n_lead + 1, dtype=float), lo["ob_vert"], lo["ob_vert_halfwidth"])

    cases = [
        ("neither", lambda: None, c),
        ("observations", wrong_P, c),
        ("slabs", wrong_lead, c),
        ("adaptive-inflation", lambda: (_set(ctx, c), ctx.set_adaptive_inflation(field, N)), c),
        ("sampling-error-correction", lambda: (_set(ctx, c), ctx.set_sampling_error_correction(np.linspace(0.0, 1.0, 16))), c),
        ("136", lambda: _set(ctx, big), big),
    ]
    for word, setup, case in cases:
        _reset(ctx)
        setup()
        calls = [lambda: _cycle(ctx, case, ngroups=ng), lambda: _cycle(ctx, case, ngroups=ng, stride=(2, 2)),
                 lambda: _cycle(ctx, case, ngroups=ng, f32=True, X=case["X"].astype(np.float32))]
        if word not in ("neither", "slabs"):
            calls.append(lambda: _probe(ctx, case))
        for call in calls:
            with pytest.raises(_lib.EfaError) as e:
                call()
            assert e.value.status == _lib.EFA_ERR_INVALID and word in str(e.value), str(e.value)
        if word == "neither":
            assert "efa_letkf_cycle_dev" in str(e.value), "the message points at the plain call"
            with pytest.raises(_lib.EfaError):
                ctx.letkf_slab_groups(n_lead)
        _reset(ctx)
        _set(ctx, c)
        _same_bits(_cycle(ctx, c), want, "after the refused %s call" % word)
    # the plain calls keep refusing while a setting is on, and name the new ones
    with pytest.raises(_lib.EfaError) as e:
        _cycle(ctx, c, plain=True)
    assert e.value.status == _lib.EFA_ERR_INVALID and "slab group" in str(e.value) and "efa_letkf_slab_cycle_dev" in str(e.value)


def test_ensrf_gc_under_the_vertical_setting_is_unchanged_by_a_slab_cycle(ctx):
    from efa_xray_amd import _lib
    c = _case(*MID, parts="v")

    def serial():
        N, M = c["X"].shape
        Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
        ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
        ctx.ensrf_cycle(N, M, c["P"], Xd, Xd, ym, Yp, c["value"], c["error"], c["assim"], _lib.LOC_GC, c["ob_lat"], c["ob_lon"], c["ob_hw"],
                        c["grid_lat"], c["grid_lon"], c["n_lead"])
        return Xd.download(), ctx.get_option("gc_family")

    _set(ctx, c)
    before, fam = serial()
    assert fam == 2, "a vertical-only EnSRF cycle runs the vertical family"
    _cycle(ctx, c)                       # builds the slab table for the vertical setting alone
    after, fam = serial()
    assert fam == 2 and np.array_equal(after, before)


# ---- the Python class ----------------------------------------------------------------------------------------------------------------
def _api_case(dtype=None):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(11)
    nvar, nt, ny, nx, M, P = 2, 3, 6, 7, 12, 30
    lat, lon = np.meshgrid(np.linspace(20, 60, ny), np.linspace(200, 280, nx), indexing="ij")
    arr = rng.standard_normal((nvar, nt, ny, nx, 1)) + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon, dtype=dtype)
    names = state.vars()
    N = state.nstate()
    rows = rng.choice(N, P, replace=False)

    class RowOb(Observation):
        def estimate(self, st):
            return st.to_vect()[self.row].copy()

    X = state.to_vect().astype(np.float64)
    obs = []
    for k in range(P):
        col = rows[k] % (ny * nx)
        ob = RowOb(value=float(X[rows[k]].mean() + rng.standard_normal()), error=float(rng.uniform(0.5, 2.0)),
                   lat=float(lat.reshape(-1)[col]), lon=float(lon.reshape(-1)[col]), assimilate_this=(k % 7 != 3),
                   localize_radius=float(rng.uniform(400.0, 1500.0)), obtype=names[k % 2] if k % 5 else "other")
        ob.row = int(rows[k])
        if k != 0:
            ob.vert, ob.vert_localize_radius = float(rng.choice([850.0, 500.0]) + rng.uniform(-50, 50)), float(rng.uniform(150.0, 600.0))
        if k != 1:
            ob.time, ob.time_localize_radius = float(rng.uniform(0.0, 2.0)), float(rng.uniform(0.8, 3.0))
        obs.append(ob)
    return state, obs, lat, lon


def _ob_diag(obs):
    d = {k: np.array([np.nan if getattr(o, k, None) is None else getattr(o, k) for o in obs], float)
         for k in ("prior_mean", "prior_var", "post_mean", "post_var")}
    d["assimilated"] = np.array([bool(o.assimilated) for o in obs])
    return d


def test_slab_letkf_class_against_the_model(ctx):
    from efa_xray_amd import LETKF, SlabLETKF
    from efa_xray_amd.assimilation.ensrf import ob_slab, ob_vertical, slab_setting
    state, obs, lat, lon = _api_case()
    names = state.vars()
    vert_coord = np.array([[850.0] * 3, [500.0] * 3])
    var_impact = {names[0]: {names[1]: 0.25}, names[1]: {names[0]: 0.0}}
    f = SlabLETKF(state, obs, verbose=False, vert_coord=vert_coord, time_localize=True, var_impact=var_impact)
    HX = np.asarray(f.compute_ob_estimates(), dtype=np.float64)
    kw = ob_slab(state, obs, slab_setting(state, "GC", True, var_impact))
    ov, oh = ob_vertical(obs)
    loc = dict(lead_vert=vert_coord.reshape(-1), ob_vert=ov, ob_vert_halfwidth=oh, lead_time=kw["lead_time"], ob_time=kw["ob_time"],
               ob_time_halfwidth=kw["ob_time_halfwidth"], lead_var=kw["lead_var"], ob_group=kw["ob_group"], ob_var=kw["ob_var"],
               impact=kw["impact"])
    assert (kw["ob_var"] == -1).any() and np.isnan(ov).any() and np.isnan(kw["ob_time"]).any()
    args = (np.array([o.value for o in obs]), np.array([o.error for o in obs]), np.array([o.assimilate_this for o in obs]),
            np.array([o.lat for o in obs]), np.array([o.lon for o in obs]), np.array([o.localize_radius for o in obs]), lat, lon, 6)
    ref = ls.slab_cycle(state.to_vect(), HX, *args, loc)
    assert ref["stats"]["cond"].max() <= COND_CAP and len(ref["rep"]) == 6
    post, obs_out = f.update()
    assert obs_out is obs and post is not state
    _close(post.to_vect(), ref["post"], "SlabLETKF.update posterior")
    _check_diag(_ob_diag(obs), ref["diag"], "SlabLETKF.update")
    sol = f.last_solve
    assert sorted(sol) == ["dfs", "group_of_slab", "n_local", "sweeps"]
    assert all(sol[k].shape == (6, 6, 7) for k in ("dfs", "n_local", "sweeps")) and sol["group_of_slab"].shape == (2, 3)
    assert np.array_equal(sol["group_of_slab"].reshape(-1), ref["group_of"])
    assert np.array_equal(sol["n_local"].reshape(6, -1), ref["stats"]["n_local"])
    _close(sol["dfs"].reshape(6, -1), ref["stats"]["dfs"], "last_solve dfs")
    # the settings are cleared after update(): the shared context serves a plain LETKF next
    s1, o1, _, _ = _api_case()
    p1, _ = LETKF(s1, o1, verbose=False).update()
    # with a stride: the statistics are the nodes'
    s2, o2, _, _ = _api_case()
    f2 = SlabLETKF(s2, o2, verbose=False, vert_coord=vert_coord, time_localize=True, var_impact=var_impact, weight_stride=(2, 3))
    p2, _ = f2.update()
    ref2 = ls.slab_cycle(state.to_vect(), HX, *args, loc, stride=(2, 3), shape=(6, 7))
    _close(p2.to_vect(), ref2["post"], "SlabLETKF.update with a weight stride")
    assert f2.last_solve["n_local"].shape == (6, 4, 3) and f2.last_solve["node_y"].size == 4 and f2.last_solve["node_x"].size == 3
    # with no option it is LETKF bit for bit
    s3, o3, _, _ = _api_case()
    f3 = SlabLETKF(s3, o3, verbose=False)
    p3, _ = f3.update()
    assert np.array_equal(p3.to_vect(), p1.to_vect()) and sorted(f3.last_solve) == ["dfs", "n_local", "sweeps"]
    for a, b in zip(o3, o1):
        assert a.post_mean == b.post_mean or (not a.assimilated and not b.assimilated)
