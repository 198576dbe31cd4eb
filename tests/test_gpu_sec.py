"""Sampling error correction (Anderson 2012) on the MI355X: the kGcSec family of both one-pass sweep forms and the
per-batch sweep's k_sweep_sec against the NumPy model (tests/_sec.py), which a table of ones ties to the reference's goldens.
Tolerance: the project's float64 criterion (test_gpu_parity.assert_parity) on the posterior, the obs block and every diagnostic."""
import functools

import numpy as np
import pytest

import _outlier as qc
import _sec
from conftest import load_golden
from oracle import ensrf_oracle as orc
from test_gpu_parity import _make_api_objects, assert_parity, golden_kwargs, oracle_kwargs, prior_arrays
from test_relaxation_host import relax

pytestmark = pytest.mark.gpu

DIAG = ("prior_mean", "prior_var", "post_mean", "post_var")


def _lib():
    from efa_xray_amd import _lib
    return _lib


def _reset(ctx):
    L = _lib()
    ctx.set_sampling_error_correction(None)
    ctx.set_adaptive_inflation(None)
    ctx.set_vertical_localization(None)
    ctx.set_slab_localization(None)
    ctx.set_outlier_threshold(None)
    ctx.set_relaxation(L.RELAX_NONE, 0.0)
    for key, val in (("path", 0), ("gc_onepass", 1), ("pipeline", 1), ("obs_batch", 64)):
        ctx.set_option(key, val)
    return ctx


@pytest.fixture
def ctx():
    c = _reset(_lib().get_context(0))
    yield c
    _reset(c)          # the context is shared per device: nothing of this module stays set on it


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _tables(M):
    return {"ones": np.ones(201), "default": _default_table(M), "steep2": _sec.steep_table(2), "steep512": _sec.steep_table(512)}


@functools.lru_cache(maxsize=None)
def _default_table(M):
    from efa_xray_amd import sampling_error_table
    return sampling_error_table(M)


def _check_diag(what, diag, ref):
    for key in DIAG:
        assert_parity(diag[key], ref[key], "%s %s" % (what, key))
    assert np.array_equal(np.asarray(diag["assimilated"], bool), np.asarray(ref["assimilated"], bool)), what


# ---- goldens ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden_model(name, table):
    """(xam, Xap, diag) of the model on a golden's inputs; computed once per (golden, table), never written to."""
    g = load_golden(name)
    N, xbm, Xbp = prior_arrays(g)
    M = Xbp.shape[1]
    out = _sec.ensrf_update(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], _tables(M)[table], **oracle_kwargs(g))
    for a in (out[0], out[1]):
        a.setflags(write=False)
    return out


def _run_golden_host(ctx, g, table):
    """efa_ensrf_update (perturbation form of the state phase) with the table set; the augmented arrays and the diagnostics."""
    N, xbm, Xbp = prior_arrays(g)
    ctx.set_sampling_error_correction(table)
    try:
        diag = ctx.ensrf_update_host(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], **golden_kwargs(g))
        kind, fam = ctx.get_option("phase_a_kind"), ctx.get_option("gc_family")
    finally:
        ctx.set_sampling_error_correction(None)
    return xbm, Xbp, diag, kind, fam


def _run_golden_members(ctx, g, table):
    """efa_ensrf_cycle_dev (member form) with the table set; posterior members, the obs block and the diagnostics."""
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N, P = nvar * nt * ny * nx, len(g["ob_value"])
    Xd = ctx.to_device(g["X"].reshape(N, M))
    Yp = ctx.to_device(np.ascontiguousarray(g["HX"], dtype=np.float64))
    ym = ctx.empty((max(P, 1),))
    ctx.form_perts(P, M, Yp, ym, Yp)
    ctx.set_sampling_error_correction(table)
    try:
        diag = ctx.ensrf_cycle(N, M, P, Xd, Xd, ym, Yp, g["ob_value"], g["ob_error"], g["ob_assim"], obs_block_out=True,
                               **golden_kwargs(g))
        kind, fam = ctx.get_option("phase_a_kind"), ctx.get_option("gc_family")
    finally:
        ctx.set_sampling_error_correction(None)
    return Xd.download(), ym.download(), Yp.download(), diag, kind, fam


@pytest.mark.parametrize("name", ["G2", "G6"])
def test_a_table_of_ones_gives_the_goldens_own_outputs(ctx, name):
    g = load_golden(name)
    N = prior_arrays(g)[0]
    xam, Xap, diag, kind, fam = _run_golden_host(ctx, g, np.ones(201))
    assert kind == 2 and fam == 4 and ctx.get_option("sec_on") == 0
    assert_parity(xam, g["xam"], name + " xam")                      # state rows and the obs block
    if "Xap" in g:
        assert_parity(Xap, g["Xap"], name + " Xap")
    assert_parity(orc.format_posterior_state(xam, Xap, N), g["post"], name + " post")
    _check_diag(name, diag, g)
    post, ym, Yp, diag, kind, fam = _run_golden_members(ctx, g, np.ones(2))
    assert kind == 2 and fam == 4
    assert_parity(post, g["post"], name + " member form")
    assert_parity(ym, g["xam"][N:], name + " member form obs means")
    _check_diag(name + " member form", diag, g)


@pytest.mark.parametrize("table", ["default", "steep2", "steep512"])
@pytest.mark.parametrize("name", ["G2", "G6"])
def test_goldens_inputs_with_a_table_match_the_model(ctx, name, table):
    g = load_golden(name)
    N = prior_arrays(g)[0]
    M = int(g["shape"][4])
    ref = _golden_model(name, table)
    if table != "default":          # the table must matter, or ignoring it would pass
        ones = _golden_model(name, "ones")
        assert np.abs(ref[0] - ones[0]).max() > 1e-3 * np.abs(ones[0]).max()
        assert np.abs(ref[1] - ones[1]).max() > 1e-3 * np.abs(ones[1]).max()
    tab = _tables(M)[table]
    xam, Xap, diag, kind, fam = _run_golden_host(ctx, g, tab)
    what = "%s %s" % (name, table)
    assert kind == 2 and fam == 4
    assert_parity(xam, ref[0], what + " xam")
    assert_parity(Xap, ref[1], what + " Xap")
    _check_diag(what, diag, ref[2])
    post, ym, Yp, diag, kind, fam = _run_golden_members(ctx, g, tab)
    assert_parity(post, orc.format_posterior_state(ref[0], ref[1], N), what + " member form")
    assert_parity(ym, ref[0][N:], what + " obs means")
    assert_parity(Yp, ref[1][N:], what + " obs perturbations")
    _check_diag(what + " member form", diag, ref[2])


def test_python_api_default_table_on_g2():
    from efa_xray_amd import EnSRF
    g = load_golden("G2")
    N = prior_arrays(g)[0]
    state, obs = _make_api_objects(g)
    try:
        post, obs_out = EnSRF(state, obs, loc="GC", sampling_error_correction=True, verbose=False).update()
        ref = _golden_model("G2", "default")
        assert_parity(post.to_vect(), orc.format_posterior_state(ref[0], ref[1], N), "API default table")
        got = {k: np.array([getattr(o, k, np.nan) if (o.assimilated or k.startswith("prior")) else np.nan for o in obs_out], float)
               for k in DIAG}
        got["assimilated"] = [o.assimilated for o in obs_out]
        _check_diag("API", got, ref[2])
        # the next filter on the same device runs without it
        state, obs = _make_api_objects(g)
        plain, _ = EnSRF(state, obs, loc="GC", verbose=False).update()
        assert_parity(plain.to_vect(), g["post"], "API afterwards, no correction")
        assert _lib().get_context(0).get_option("sec_on") == 0
    finally:
        _reset(_lib().get_context(0))


# ---- a small seeded problem at every ensemble size that takes another kernel --------------------------------------------------
SHAPE = (1, 2, 5, 7)                        # nvar, nt, ny, nx: two slabs of 35 columns (two column blocks of 16 and a rest of 3)
TABLE = 0.25 + 0.75 * (np.arange(37) / 36.0) ** 1.5
M_LIST = [2, 3, 20, 64, 65, 80, 100, 128, 129, 256]


class Problem(object):
    """6 obs in the west of a grid 80 degrees wide, half-widths 600-900 km: the eastern columns are beyond twice the half-width of
    every ob.  Ob 3 is not assimilated.  Values that float32 holds exactly, so the same prior serves both storages."""

    def __init__(self, M, seed=0):
        rng = np.random.default_rng(1000 * seed + M)
        nvar, nt, ny, nx = SHAPE
        self.M, self.shape = M, SHAPE
        self.ncol, self.n_lead = ny * nx, nvar * nt
        self.N = self.ncol * self.n_lead
        lat, lon = np.meshgrid(np.linspace(30.0, 50.0, ny), np.linspace(200.0, 280.0, nx), indexing="ij")
        self.grid_lat, self.grid_lon = lat, lon
        X = 5.0 * rng.standard_normal((self.N, 1)) + 2.0 * rng.standard_normal((self.N, M))
        self.X = X.astype(np.float32).astype(np.float64)
        iy = np.array([0, 2, 4, 1, 3, 2])
        ix = np.array([0, 1, 0, 1, 0, 0])
        lead = np.array([0, 1, 0, 1, 1, 0])
        self.P = 6
        self.rows = lead * self.ncol + iy * nx + ix
        self.HX = self.X[self.rows].copy()
        self.ob_lat, self.ob_lon = lat[iy, ix].copy(), lon[iy, ix].copy()
        self.radius = rng.uniform(600.0, 900.0, self.P)
        self.error = rng.uniform(0.5, 1.5, self.P)
        self.value = self.HX.mean(axis=1) + rng.standard_normal(self.P)
        self.assim = np.array([True, True, True, False, True, True])
        self.far = np.flatnonzero(np.tile(np.arange(nx) >= 4, ny * self.n_lead))     # rows no ob reaches

    def kw(self):
        return dict(loc_mode=1, ob_lat=self.ob_lat, ob_lon=self.ob_lon, ob_halfwidth=self.radius, grid_lat=self.grid_lat.reshape(-1),
                    grid_lon=self.grid_lon.reshape(-1), n_lead=self.n_lead)

    def okw(self):
        return dict(loc="GC", ob_lat=self.ob_lat, ob_lon=self.ob_lon, ob_halfwidth=self.radius, grid_lat=self.grid_lat,
                    grid_lon=self.grid_lon, state_shape=self.shape)

    def model(self, table, X=None, assim=None, value=None):
        X = self.X if X is None else X
        return _sec.ensrf_cycle(X, self.HX, self.value if value is None else value, self.error,
                                self.assim if assim is None else assim, table, **self.okw())


@functools.lru_cache(maxsize=None)
def _problem(M):
    return Problem(M)


@functools.lru_cache(maxsize=None)
def _problem_model(M):
    return _problem(M).model(TABLE)


def _cycle(ctx, pb, table, X=None, f32=False, value=None, assim=None, in_place=True):
    """Phase A and the member-form state phase with the table set (None: off); posterior, obs block, diagnostics, options."""
    X = pb.X if X is None else X
    Xd = ctx.to_device(X.astype(np.float32), dtype=np.float32) if f32 else ctx.to_device(X)
    Yp = ctx.to_device(pb.HX)
    ym = ctx.empty((pb.P,))
    ctx.form_perts(pb.P, pb.M, Yp, ym, Yp)
    ctx.set_sampling_error_correction(table)
    try:
        value = pb.value if value is None else value
        assim = pb.assim if assim is None else assim
        kw = pb.kw()
        if f32:
            diag = ctx.obs_phase(pb.M, pb.P, ym, Yp, value, pb.error, assim, 1, pb.ob_lat, pb.ob_lon, pb.radius)
            ctx.state_cycle_f32(pb.N, pb.M, Xd, Xd, kw["grid_lat"], kw["grid_lon"], pb.n_lead)
            ctx.synchronize()
        else:
            post = Xd if in_place else ctx.empty((pb.N, pb.M))
            diag = ctx.ensrf_cycle(pb.N, pb.M, pb.P, Xd, post, ym, Yp, value, pb.error, assim, obs_block_out=True, **kw)
            Xd = post
        opts = {k: ctx.get_option(k) for k in ("phase_a_kind", "gc_family", "gc_form", "f32_native")}
    finally:
        ctx.set_sampling_error_correction(None)
    return Xd.download(), ym.download(), Yp.download(), diag, opts


@pytest.mark.parametrize("M", M_LIST)
def test_every_kernel_form_and_both_storages_match_the_model(ctx, M):
    pb = _problem(M)
    post_ref, xam, Xap, dref = _problem_model(M)
    want_form = 2 if (M % 2 == 0 and M <= 104) else 1            # the row-per-lane kernel up to 104 members, an even number
    # float64, member form
    post, ym, Yp, diag, opts = _cycle(ctx, pb, TABLE)
    assert opts["phase_a_kind"] == 2 and opts["gc_family"] == 4 and opts["gc_form"] == want_form, opts
    assert_parity(post, post_ref, "M=%d posterior" % M)
    assert_parity(ym, xam[pb.N:], "M=%d obs means" % M)
    assert_parity(Yp, Xap[pb.N:], "M=%d obs perturbations" % M)
    _check_diag("M=%d" % M, diag, dref)
    # float64, perturbation form
    xbm, Xbp = orc.format_prior_state(pb.X, pb.HX)
    ctx.set_sampling_error_correction(TABLE)
    dh = ctx.ensrf_update_host(xbm, Xbp, pb.N, pb.value, pb.error, pb.assim, **pb.kw())
    assert ctx.get_option("gc_form") == want_form and ctx.get_option("gc_family") == 4
    ctx.set_sampling_error_correction(None)
    assert_parity(xbm, xam, "M=%d xam" % M)
    assert_parity(Xbp, Xap, "M=%d Xap" % M)
    _check_diag("M=%d perturbation form" % M, dh, dref)
    # float32 storage: the float64 posterior rounded once, on the float rows themselves where the row-per-lane kernel serves
    post32, _, _, d32, o32 = _cycle(ctx, pb, TABLE, f32=True)
    assert post32.dtype == np.float32 and o32["gc_family"] == 4 and o32["f32_native"] == (1 if want_form == 2 else 0), o32
    assert _bits_equal(post32, post.astype(np.float32)), "M=%d float32 storage" % M
    for key in DIAG:
        assert np.array_equal(d32[key], diag[key], equal_nan=True), key


def test_both_kernel_forms_are_covered():
    forms = {2 if (M % 2 == 0 and M <= 104) else 1 for M in M_LIST}
    assert forms == {1, 2}
    assert {M for M in M_LIST if M > 96 and M <= 104} and {M for M in M_LIST if M > 128}    # one wave per SIMD; the widest quad kernels


# ---- the properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [20, 65])
def test_a_table_of_zeros_moves_no_state_row(ctx, M):
    pb = _problem(M)
    post, ym, Yp, diag, opts = _cycle(ctx, pb, np.zeros(9))
    assert opts["gc_family"] == 4
    assert _bits_equal(post, pb.X), "member form: every state row is the prior bit for bit"
    xbm, Xbp = orc.format_prior_state(pb.X, pb.HX)
    x0, X0 = xbm.copy(), Xbp.copy()
    ctx.set_sampling_error_correction(np.zeros(9))
    dh = ctx.ensrf_update_host(xbm, Xbp, pb.N, pb.value, pb.error, pb.assim, **pb.kw())
    ctx.set_sampling_error_correction(None)
    assert _bits_equal(xbm[:pb.N], x0[:pb.N]) and _bits_equal(Xbp[:pb.N], X0[:pb.N]), "perturbation form likewise"
    # no ob moves another ob's row either: each is the scalar update of its own prior, which is the caller's
    ym0, Yp0 = orc.compute_ob_priors(pb.HX)
    for d in (diag, dh):
        assert_parity(d["prior_mean"], ym0, "prior mean")
        assert_parity(d["prior_var"], np.var(Yp0, axis=1), "prior var")
        a = pb.assim
        assert np.array_equal(np.asarray(d["assimilated"], bool), a)
        # the reference's scalar update (ensrf.py:91-141 on the ob's own row): the covariance divides by M - 1, the variance in
        # the denominator by M, so var R / (var + R) is this only as M grows
        var, pm, R = d["prior_var"][a], d["prior_mean"][a], pb.error[a]
        kmat = (var * M / (M - 1.0)) / (var + R)
        beta = 1.0 / (1.0 + np.sqrt(R / (var + R)))
        assert_parity(d["post_var"][a], (1.0 - beta * kmat) ** 2 * var, "post var: the scalar update of the ob's own prior")
        assert_parity(d["post_mean"][a], pm + kmat * (pb.value[a] - pm), "post mean")
        assert np.isnan(d["post_mean"][~a]).all()


@pytest.mark.parametrize("M", [20, 65])
def test_row_properties(ctx, M):
    pb = _problem(M)
    base, _, _, _, _ = _cycle(ctx, pb, TABLE)
    assert pb.far.size >= 2 * pb.n_lead
    assert _bits_equal(base[pb.far], pb.X[pb.far]), "rows beyond twice the half-width of every ob"
    near = np.setdiff1d(np.arange(pb.N), pb.far)
    assert (base[near] != pb.X[near]).any(axis=1).sum() > near.size // 4
    # a constant row (no spread: correlation 0 by definition) stays finite and as it is
    X = pb.X.copy()
    const = 7                               # slab 0, iy 1, ix 0: between two obs, not an ob's own row
    assert const not in pb.rows and const in near and (base[const] != pb.X[const]).any()
    X[const] = 3.0
    got, _, _, _, _ = _cycle(ctx, pb, TABLE, X=X)
    assert np.isfinite(got).all() and _bits_equal(got[const], X[const])
    keep = np.setdiff1d(np.arange(pb.N), [const])
    assert _bits_equal(got[keep], base[keep])
    # one poisoned row: NaN for that row alone, every other row bit for bit as without it
    X = pb.X.copy()
    bad = 21                                # slab 0, iy 3, ix 0
    assert bad not in pb.rows and bad in near and (base[bad] != pb.X[bad]).any()
    X[bad, M // 2] = np.nan
    got, _, _, diag, _ = _cycle(ctx, pb, TABLE, X=X)
    assert np.isnan(got[bad]).all()
    keep = np.setdiff1d(np.arange(pb.N), [bad])
    assert _bits_equal(got[keep], base[keep])
    assert np.isfinite(diag["post_mean"][pb.assim]).all()
    # ... and out of place as in place
    oop, _, _, _, _ = _cycle(ctx, pb, TABLE, in_place=False)
    assert _bits_equal(oop, base)


def test_with_rtps(ctx):
    pb = _problem(20)
    ctx.set_relaxation(_lib().RELAX_RTPS, 0.9)
    post, ym, Yp, diag, opts = _cycle(ctx, pb, TABLE)
    ctx.set_relaxation(_lib().RELAX_NONE, 0.0)
    post_ref, xam, Xap, dref = _problem_model(20)
    assert opts["gc_family"] == 4
    assert_parity(post, relax(pb.X, post_ref, rtps=0.9), "rtps 0.9 with the correction")
    assert_parity(ym, xam[pb.N:], "obs means")          # the obs block and the diagnostics are not relaxed
    assert_parity(Yp, Xap[pb.N:], "obs perturbations")
    _check_diag("rtps", diag, dref)


def test_with_the_outlier_check(ctx):
    pb = _problem(64)
    t = 3.0
    value, idx = qc.inject(pb.HX, pb.value, pb.error, pb.assim, t, 2, seed=4)
    ym0, Yp0 = orc.compute_ob_priors(pb.HX)
    assert qc.clear_of_threshold(ym0, Yp0, value, pb.error, t)
    kept = qc.masked_flags(pb.HX, value, pb.error, pb.assim, t)
    assert kept.sum() == pb.assim.sum() - 2 and not kept[idx].any()
    ctx.set_outlier_threshold(t)
    post, ym, Yp, diag, opts = _cycle(ctx, pb, TABLE, value=value)
    ctx.set_outlier_threshold(None)
    post_ref, xam, Xap, dref = pb.model(TABLE, assim=kept, value=value)
    assert opts["phase_a_kind"] == 2 and opts["gc_family"] == 4
    assert not np.asarray(diag["assimilated"], bool)[idx].any(), "the injected gross errors are rejected"
    assert_parity(post, post_ref, "outlier check with the correction")
    assert_parity(ym, xam[pb.N:], "obs means")
    assert_parity(Yp, Xap[pb.N:], "obs perturbations")
    _check_diag("outlier", diag, dref)


# ---- one context through on / off / another table; the C ABI's checks -----------------------------------------------------------
def test_one_context_on_off_and_another_table():
    L = _lib()
    pb = _problem(20)
    fresh = L.Context(0)
    one = L.Context(0)
    try:
        plain, ym_p, Yp_p, d_p, o_p = _cycle(fresh, pb, None)
        assert o_p["phase_a_kind"] != 2 and o_p["gc_family"] == 0
        assert one.get_option("sec_on") == 0
        one.set_sampling_error_correction(TABLE)
        assert one.get_option("sec_on") == 1
        one.set_sampling_error_correction(None)
        on, _, _, d_on, o_on = _cycle(one, pb, TABLE)
        assert o_on["phase_a_kind"] == 2 and o_on["gc_family"] == 4
        assert_parity(on, _problem_model(20)[0], "on")
        off, ym_o, Yp_o, d_off, o_off = _cycle(one, pb, None)
        assert o_off["phase_a_kind"] == o_p["phase_a_kind"] and o_off["gc_family"] == 0 and one.get_option("sec_on") == 0
        assert _bits_equal(off, plain) and _bits_equal(ym_o, ym_p) and _bits_equal(Yp_o, Yp_p), "off again: a fresh context's bits"
        for key in DIAG:
            assert np.array_equal(d_off[key], d_p[key], equal_nan=True), key
        other = _sec.steep_table(64)
        got, _, _, d2, o2 = _cycle(one, pb, other)
        assert o2["phase_a_kind"] == 2 and o2["gc_family"] == 4
        ref = pb.model(other)
        assert_parity(got, ref[0], "another table")
        _check_diag("another table", d2, ref[3])
        assert np.abs(got - on).max() > 1e-3 * np.abs(on).max(), "the new table took effect"
    finally:
        fresh.close()
        one.close()


def test_c_abi_refuses_bad_tables_and_combinations_before_any_launch():
    L = _lib()
    pb = _problem(20)
    c = L.Context(0)

    def refused(call, text):
        with pytest.raises(L.EfaError) as ei:
            call()
        assert ei.value.status == L.EFA_ERR_INVALID and text in str(ei.value), str(ei.value)

    try:
        c.set_sampling_error_correction(TABLE)
        for bad in (np.ones(1), np.ones(513), np.array([0.5, np.nan]), np.array([0.5, -1e-300]), np.array([np.inf, 1.0])):
            refused(lambda: c.set_sampling_error_correction(bad), "sampling error correction")
        assert c.get_option("sec_on") == 1, "a refused table leaves the setting as it was"
        X = c.to_device(pb.X)
        Yp0 = pb.HX - pb.HX.mean(axis=1, keepdims=True)
        ym0 = pb.HX.mean(axis=1)
        xbm, Xbp = orc.format_prior_state(pb.X, pb.HX)
        before = (xbm.copy(), Xbp.copy())

        def entries(loc_mode, tag):
            kw = pb.kw() if loc_mode else dict(loc_mode=0)
            okw = dict(loc_mode=loc_mode, ob_lat=pb.ob_lat, ob_lon=pb.ob_lon, ob_halfwidth=pb.radius) if loc_mode else dict(loc_mode=0)
            Yp, ym = c.to_device(Yp0), c.to_device(ym0)
            refused(lambda: c.obs_phase(pb.M, pb.P, ym, Yp, pb.value, pb.error, pb.assim, **okw), tag)
            refused(lambda: c.ensrf_cycle(pb.N, pb.M, pb.P, X, X, ym, Yp, pb.value, pb.error, pb.assim, **kw), tag)
            xm, Xp = c.to_device(xbm[:pb.N]), c.to_device(Xbp[:pb.N])
            refused(lambda: c.ensrf_update_dev(pb.N, pb.M, pb.P, xm, Xp, ym, Yp, pb.value, pb.error, pb.assim, **kw), tag)
            refused(lambda: c.ensrf_update_host(xbm, Xbp, pb.N, pb.value, pb.error, pb.assim, **kw), tag)
            assert _bits_equal(X.download(), pb.X) and _bits_equal(Yp.download(), Yp0) and _bits_equal(xbm, before[0])

        entries(0, "needs GC localisation")
        c.set_option("gc_onepass", 0)
        entries(1, "one-pass GC sweep")
        c.set_option("gc_onepass", 1)
        field = c.to_device(np.tile([1.0, 0.6], (pb.N, 1)))
        c.set_adaptive_inflation(field, pb.N)
        entries(1, "adaptive inflation")
        c.set_adaptive_inflation(None)
        c.set_vertical_localization(np.array([500.0, 850.0]), np.full(pb.P, 600.0), np.full(pb.P, 200.0))
        entries(1, "vertical localisation")
        c.set_vertical_localization(None)
        c.set_slab_localization(n_lead=pb.n_lead, P=pb.P, lead_time=np.array([0.0, 6.0]), ob_time=np.zeros(pb.P),
                                ob_time_halfwidth=np.full(pb.P, 4.0))
        entries(1, "slab localisation")
        c.set_slab_localization(None)
        # the state calls after an obs phase that ran without it
        c.set_sampling_error_correction(None)
        Yp, ym = c.to_device(Yp0), c.to_device(ym0)
        c.obs_phase(pb.M, pb.P, ym, Yp, pb.value, pb.error, pb.assim, 0)
        c.set_sampling_error_correction(TABLE)
        refused(lambda: c.state_cycle(pb.N, pb.M, X, X), "needs GC localisation")
        X32 = c.to_device(pb.X.astype(np.float32), dtype=np.float32)
        refused(lambda: c.state_cycle_f32(pb.N, pb.M, X32, X32), "needs GC localisation")
        # the streamed update does not offer it, on either storage
        for dt in (np.float64, np.float32):
            seg = [np.ascontiguousarray(pb.X.reshape(pb.n_lead, pb.ncol, pb.M), dtype=dt)]
            out = [np.empty_like(seg[0])]
            kw = pb.kw()
            kw.pop("n_lead")
            refused(lambda: c.ensrf_cycle_host(seg, out, pb.ncol, pb.M, pb.HX, 16, pb.value, pb.error, pb.assim, **kw), "streamed update")
        # with nothing in its way it runs
        c.set_sampling_error_correction(np.ones(2))
        got, _, _, _, o = _cycle(c, pb, np.ones(2))
        assert o["gc_family"] == 4
    finally:
        c.close()
