"""Individual Gaspari-Cohn taper weights of the device, read back through the C ABI with the taper probe (tests/_taper_probe.py)
and compared pair by pair with the reference's formulas in long double, along every route that evaluates geometry: the one-pass
active lists (row-per-lane and quad kernels), the per-batch taper table, vertical localisation, the streamed update, the
observation impact and the obs-obs taper of every Phase-A mode.  The probe's geometry has columns at the poles, both longitude
frames, points at r = 0, 1 -+ 1e-9, 2 -+ 1e-9 of every ob, half-widths of 0.5 km, -800 km, 9000 km and 25 000 km, and unassimilated
witness obs before and after the assimilated ones.

Every test prints and asserts its worst err / tol (tolerance per pair: the probe's docstring), its excluded-pair count (at most
0.1 %) and its near-cut-off pair count.
"""
import numpy as np
import pytest

import _efso
import _taper_probe as tp

pytestmark = pytest.mark.gpu

LD = tp.LD
_MODES = {"band": (1, 2, 4), "gram": (1, 1, 3), "pipeline": (1, 0, 1), "batch": (0, 0, 2)}   # test_gpu_parity._G12_MODES' four


def _ctx():
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    ctx.set_vertical_localization(None)
    ctx.set_adaptive_inflation(None)
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    ctx.set_outlier_threshold(None)
    for key, v in (("path", 0), ("gram", 2), ("pipeline", 1), ("gc_onepass", 1), ("obs_batch", 64), ("spin_limit", 4000000)):
        ctx.set_option(key, v)
    return ctx


def _loc(p):
    return dict(loc_mode=1, ob_lat=p.ob_lat, ob_lon=p.ob_lon, ob_halfwidth=p.ob_hw)


def _grid(p):
    return dict(grid_lat=p.grid_lat, grid_lon=p.grid_lon, n_lead=p.n_lead)


def _split(members):
    """(mean, perturbations) of member rows, the mean in long double."""
    m = np.asarray(members, dtype=LD).mean(axis=1)
    return m, (np.asarray(members, dtype=LD) - m[:, None]).astype(np.float64)


def _cycle(ctx, p, in_place=False):
    """efa_ensrf_cycle_dev on the probe, obs block returned: (posterior members, ym, Yp, diagnostics)."""
    X = ctx.to_device(p.X)
    post = X if in_place else ctx.empty(p.X.shape)
    ym, Yp = ctx.to_device(p.ym), ctx.to_device(p.Yp)
    diag = ctx.ensrf_cycle(p.rows, p.M, p.PT, X, post, ym, Yp, p.ob_value, p.ob_error, p.ob_assim, obs_block_out=True,
                           **dict(_loc(p), **_grid(p)))
    if not in_place:
        assert np.array_equal(X.download(), p.X)        # the prior is read only
    return post.download(), ym.download(), Yp.download(), diag


def _check_state(what, p, members):
    mean, perts = _split(members)
    prior_mean, _ = _split(p.X)
    return p.check(what + " state", p.state, mean, perts, prior_mean, need_cut=True)


def _check_obs_block(what, p, ym, Yp, diag):
    """The witnesses before and after the probing obs, and the diagnostics of both kinds of ob."""
    w, k, M = p.wit_idx, p.probe_idx, p.M
    res = p.check(what + " obs-obs", p.obs, ym[w], Yp[w], p.ym[w], need_cut=True)
    for name, sel in (("before", p.wit_before), ("after", ~p.wit_before)):
        reached = p.near(p.obs).any(axis=1) & sel
        assert reached.any(), "%s: no witness %s the probing obs is within reach of one" % (what, name)
        changed = np.any(Yp[w] != p.Yp[w], axis=1) & (ym[w] != p.ym[w])
        assert np.all(changed[reached]), "%s: %d witnesses %s the probing obs were not updated" % (
            what, int((reached & ~changed).sum()), name)
    scale = 16 * tp.EPS * M
    assert np.array_equal(diag["assimilated"], p.ob_assim.astype(bool))
    # a probing ob sees its own prior when its turn comes, and its own taper weight is 1
    np.testing.assert_allclose(diag["prior_mean"][k], p.ym[k], rtol=0, atol=scale * 8, err_msg=what)
    np.testing.assert_allclose(diag["prior_var"][k], (p.yy / M).astype(float), rtol=scale, err_msg=what)
    np.testing.assert_allclose(diag["post_mean"][k], (p.ym[k] + p.K * p.innov).astype(float), rtol=0, atol=scale * 8, err_msg=what)
    np.testing.assert_allclose(diag["post_var"][k], ((p.yy / M) * (1 - p.beta * p.K) ** 2).astype(float), rtol=scale, err_msg=what)
    np.testing.assert_allclose(ym[k], diag["post_mean"][k], rtol=0, atol=scale * 8, err_msg=what)
    assert np.all(np.isnan(diag["post_mean"][w])) and np.all(np.isnan(diag["post_var"][w]))
    # a witness before the probing obs reports its prior, one after them its final values (ensrf.py:66,70)
    first, last = w[p.wit_before], w[~p.wit_before]
    np.testing.assert_allclose(diag["prior_mean"][first], p.ym[first], rtol=0, atol=scale * 8, err_msg=what)
    np.testing.assert_allclose(diag["prior_var"][first], np.var(p.Yp[first], axis=1), rtol=scale, err_msg=what)
    np.testing.assert_allclose(diag["prior_mean"][last], ym[last], rtol=0, atol=scale * 8, err_msg=what)
    np.testing.assert_allclose(diag["prior_var"][last], np.var(Yp[last], axis=1), rtol=scale, atol=scale, err_msg=what)
    return res


def _check_counts(what, ctx, p, active_pairs=None):
    """gc_active_pairs of the last sweep and efa_gc_block_counts, total and per block, between the pairs that must be non-zero
    and the pairs that may be."""
    plo, phi, olo, ohi = p.block_bounds()
    k = p.probe_idx
    cnt, bp, total = ctx.gc_block_counts(p.grid_lat, p.grid_lon, p.ob_lat, p.ob_lon, p.ob_hw, p.ob_assim)
    print("%s: %d <= block_pairs total %d (gc_active_pairs %s) <= %d; longest list %d" % (
        what, plo.sum(), total, active_pairs, phi.sum(), cnt.max()))
    assert plo.sum() <= total <= phi.sum(), what
    assert int(bp.sum()) == total
    assert np.all((plo <= bp) & (bp <= phi)), "%s: block_pairs of block %d" % (what, int(np.argmax((plo > bp) | (bp > phi))))
    assert np.all((olo <= cnt) & (cnt <= ohi)), "%s: block_count of block %d" % (what, int(np.argmax((olo > cnt) | (cnt > ohi))))
    if active_pairs is not None:
        assert plo.sum() <= active_pairs <= phi.sum(), what
    # the witnesses (flag 0) are not counted, wherever they stand in the block
    _, _, none = ctx.gc_block_counts(p.grid_lat, p.grid_lon, p.ob_lat, p.ob_lon, p.ob_hw, np.zeros(p.PT, np.uint8))
    assert none == 0
    return cnt


# ---- state taper -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lane-regional", "lane-global", "odd-regional", "odd-global", "wide-regional", "wide-global"])
def test_one_pass_lists(name):
    """The active lists of k_gc_build feeding the row-per-lane kernel (even M <= 104) and the quad kernel (odd M, M = 256)."""
    ctx, p = _ctx(), tp.get_probe(name)
    post, ym, Yp, diag = _cycle(ctx, p)
    pairs = ctx.get_option("gc_active_pairs")
    _check_state(name, p, post)
    _check_obs_block(name, p, ym, Yp, diag)
    _check_counts(name, ctx, p, pairs)
    if p.reach == "regional":
        n = p.assert_untouched(name, p.state, (p.X, post))
        print("%s: %d untouched rows bit-identical" % (name, n))


def test_builder_queue_wraps_on_a_cluster_of_obs():
    """At least 150 obs reach one 16-column block: the builder's 128-entry per-wave queue wraps and its 64-ob steps repeat."""
    ctx, p = _ctx(), tp.get_probe("cluster")
    post, ym, Yp, diag = _cycle(ctx, p)
    pairs = ctx.get_option("gc_active_pairs")
    _check_state("cluster", p, post)
    _check_obs_block("cluster", p, ym, Yp, diag)
    cnt = _check_counts("cluster", ctx, p, pairs)
    olo, ohi = p.block_bounds()[2:]
    b = int(np.argmax(olo))
    print("cluster: block %d lists %d obs (between %d and %d)" % (b, cnt[b], olo[b], ohi[b]))
    assert olo[b] >= 150 and olo[b] <= cnt[b] <= ohi[b]
    p.assert_untouched("cluster", p.state, (p.X, post))


@pytest.mark.parametrize("batch", [64, 7])
def test_per_batch_taper_table(batch):
    """gc_onepass 0: k_taper_table, and the obs taper inside k_sweep."""
    ctx, p = _ctx(), tp.get_probe("lane-global")
    try:
        ctx.set_option("gc_onepass", 0)
        ctx.set_option("obs_batch", batch)
        post, ym, Yp, diag = _cycle(ctx, p)
    finally:
        ctx.set_option("gc_onepass", 1)
        ctx.set_option("obs_batch", 64)
    what = "table batch %d" % batch
    _check_state(what, p, post)
    _check_obs_block(what, p, ym, Yp, diag)


def test_per_batch_taper_table_past_its_grid_cap():
    """ncol = 16 437 columns x 64 obs of a batch: more than twice the table kernel's 524 288 threads, a third, ragged trip."""
    ctx, p = _ctx(), tp.get_probe("cap")
    try:
        ctx.set_option("gc_onepass", 0)
        post, ym, Yp, diag = _cycle(ctx, p)
    finally:
        ctx.set_option("gc_onepass", 1)
    _check_state("table past the cap", p, post)
    _check_obs_block("table past the cap", p, ym, Yp, diag)


@pytest.mark.parametrize("name", ["vertical", "vertical-regional"])
@pytest.mark.parametrize("mode", ["band", "batch"])
def test_vertical_localisation_three_slabs(mode, name):
    """n_lead = 3 with slab, ob coordinates and half-widths set, some NaN: weight = horizontal x vertical, factor 1 for NaN.  The
    band leader reads the dense obs-obs table (k_obs_taper_vert); the per-batch kernels read k_obs_taper_rows' table."""
    ctx, p = _ctx(), tp.get_probe(name)
    pipe, gram, want = _MODES[mode]
    try:
        ctx.set_option("pipeline", pipe)
        ctx.set_option("gram", gram)
        ctx.set_vertical_localization(p.lead_vert, p.ob_vert, p.ob_vhw)
        post, ym, Yp, diag = _cycle(ctx, p)
        kind = ctx.get_option("phase_a_kind")
    finally:
        ctx.set_vertical_localization(None)
        ctx.set_option("pipeline", 1)
        ctx.set_option("gram", 2)
    assert kind == want, (mode, kind)
    what = "%s %s" % (name, mode)
    _check_state(what, p, post)
    _check_obs_block(what, p, ym, Yp, diag)
    # a NaN slab equals the horizontal weights alone; a slab beyond an ob's vertical cut-off is not touched by it
    assert np.any(np.asarray(p.state["v"] == 0)) and np.any(np.asarray(p.state["v"] == 1))
    if p.reach == "regional":     # the vertical kernels' rows that no ob reaches, horizontally or vertically, bit for bit
        n = p.assert_untouched(what, p.state, (p.X, post))
        hz = p.untouched_rows(dict(p.state, v=LD(1)))
        print("%s: %d untouched rows bit-identical, %d of them by the vertical factor alone" % (what, n, n - int(hz.sum())))
        assert n > hz.sum()


@pytest.mark.parametrize("name", ["lane-regional", "odd-regional"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("form", ["members", "perts"])
def test_rows_no_ob_reaches_are_bit_identical(form, in_place, name):
    """efa_obs_phase_dev + efa_state_cycle_dev (member rows) and + efa_state_phase_dev (xm and Xp rows), in place and out of
    place: rows whose every pair lies beyond the cut-off come back bit for bit; every other row carries the right weights."""
    ctx, p = _ctx(), tp.get_probe(name)
    ym, Yp = ctx.to_device(p.ym), ctx.to_device(p.Yp)
    ctx.obs_phase(p.M, p.PT, ym, Yp, p.ob_value, p.ob_error, p.ob_assim, **_loc(p))
    what = "%s %s %s" % (name, form, "in place" if in_place else "out of place")
    if form == "members":
        X = ctx.to_device(p.X)
        out = X if in_place else ctx.to_device(np.full(p.X.shape, np.nan))
        ctx.state_cycle(p.rows, p.M, X, out, **_grid(p))
        post = out.download()
        _check_state(what, p, post)
        p.assert_untouched(what, p.state, (p.X, post))
    else:
        xm0, Xp0 = p.X.mean(axis=1), p.X - p.X.mean(axis=1, keepdims=True)
        xm, Xp = ctx.to_device(xm0), ctx.to_device(Xp0)
        xo = xm if in_place else ctx.to_device(np.full(xm0.shape, np.nan))
        Xo = Xp if in_place else ctx.to_device(np.full(Xp0.shape, np.nan))
        ctx.state_phase(p.rows, p.M, xm, Xp, xo, Xo, **_grid(p))
        xm1, Xp1 = xo.download(), Xo.download()
        p.check(what + " state", p.state, xm1, Xp1, xm0, need_cut=True)
        p.assert_untouched(what, p.state, (xm0, xm1), (Xp0, Xp1))


def test_streamed_update_in_chunks_of_16_columns_equals_the_resident_one():
    """efa_ensrf_cycle_host with chunk_cols 16: the active lists are rebuilt per column chunk; bit for bit the resident posterior."""
    ctx, p = _ctx(), tp.get_probe("lane-global")
    Yp = ctx.to_device(p.HX)
    ym = ctx.empty((p.PT,))
    ctx.form_perts(p.PT, p.M, Yp, ym, Yp)
    X = ctx.to_device(p.X)
    post = ctx.empty(p.X.shape)
    d0 = ctx.ensrf_cycle(p.rows, p.M, p.PT, X, post, ym, Yp, p.ob_value, p.ob_error, p.ob_assim, **dict(_loc(p), **_grid(p)))
    resident = post.download()
    prior = np.ascontiguousarray(p.X.reshape(1, p.ncol, p.M))
    out = np.full(prior.shape, np.nan)
    d1 = ctx.ensrf_cycle_host([prior], [out], p.ncol, p.M, p.HX, 16, p.ob_value, p.ob_error, p.ob_assim, grid_lat=p.grid_lat,
                              grid_lon=p.grid_lon, **_loc(p))
    assert ctx.stream_stats()["chunks"] == (p.ncol + 15) // 16
    assert np.array_equal(out.reshape(p.rows, p.M), resident)
    for key in d0:
        assert np.array_equal(d0[key], d1[key], equal_nan=True), key
    _check_state("streamed, 16-column chunks", p, out.reshape(p.rows, p.M))


@pytest.mark.parametrize("name", ["lane-global", "odd-global"])
def test_observation_impact_on_the_probe_geometry(name):
    """efa_obs_impact_dev's own list build on the probe's columns and final obs block, against tests/_efso.py at its bound."""
    ctx, p = _ctx(), tp.get_probe(name)
    _, ym, Yp, _ = _cycle(ctx, p)
    rng = np.random.default_rng(11)
    Ya = ym[:, None] + Yp
    v = rng.standard_normal(p.rows)
    d = p.ob_value - p.ym
    used = p.ob_assim.astype(bool)
    J = ctx.obs_impact(p.rows, p.M, p.PT, ctx.to_device(p.X), ctx.to_device(v), ctx.to_device(Ya), d, p.ob_error, used, 1,
                       p.ob_lat, p.ob_lon, p.ob_hw, p.grid_lat, p.grid_lon, 1)
    Jr, A = _efso.efso(p.X, Ya, v, d, p.ob_error, used, grid_lat=p.grid_lat, grid_lon=p.grid_lon, ob_lat=p.ob_lat,
                       ob_lon=p.ob_lon, ob_halfwidth=p.ob_hw, n_lead=1)
    tol = _efso.tolerance(p.rows, p.M)
    err = np.abs(J - Jr)
    worst = float(np.max(err[used] / np.maximum(A[used], 1e-300)))
    print("%s impact: max |J - ref| / A = %.3e (tolerance %.1e), A > 0 on %d of %d used obs" % (
        name, worst, tol, int(np.count_nonzero(A[used])), int(used.sum())))
    assert np.all(np.isfinite(J)) and np.all(err <= tol * A), (name, worst)
    assert np.count_nonzero(A[used]) == used.sum()          # every probing ob has a column at r = 0
    assert np.all(J[~used] == 0.0)


# ---- obs-obs taper ---------------------------------------------------------------------------------------------------
def _obs_phase(ctx, p):
    ym, Yp = ctx.to_device(p.ym), ctx.to_device(p.Yp)
    diag = ctx.obs_phase(p.M, p.PT, ym, Yp, p.ob_value, p.ob_error, p.ob_assim, **_loc(p))
    return ym.download(), Yp.download(), diag, ctx.get_option("phase_a_kind")


@pytest.mark.parametrize("batch", [64, 1])
@pytest.mark.parametrize("mode", list(_MODES))
def test_obs_obs_taper_every_phase_a_mode(mode, batch):
    """104 obs rows (a 64-ob hand-over), witnesses before and after the probing obs.  The probing obs are orthogonal, so the
    Gram-space leaders' cancellation guard must not trip: the kind is asserted."""
    ctx, p = _ctx(), tp.get_probe("obsobs")
    assert p.PT == 104
    pipe, gram, want = _MODES[mode]
    try:
        ctx.set_option("pipeline", pipe)
        ctx.set_option("gram", gram)
        ctx.set_option("obs_batch", batch)
        ym, Yp, diag, kind = _obs_phase(ctx, p)
    finally:
        ctx.set_option("pipeline", 1)
        ctx.set_option("gram", 2)
        ctx.set_option("obs_batch", 64)
    assert kind == want, (mode, kind)
    _check_obs_block("obs-obs %s batch %d" % (mode, batch), p, ym, Yp, diag)


@pytest.mark.parametrize("batch", [64, 1])
def test_obs_obs_taper_256_members(batch):
    """M = 256 goes to the per-batch kernels (kind 2)."""
    ctx, p = _ctx(), tp.get_probe("wide-global")
    try:
        ctx.set_option("obs_batch", batch)
        ym, Yp, diag, kind = _obs_phase(ctx, p)
    finally:
        ctx.set_option("obs_batch", 64)
    assert kind == 2, kind
    _check_obs_block("obs-obs 256 members batch %d" % batch, p, ym, Yp, diag)
