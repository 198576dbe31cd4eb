"""Adaptive inflation (Anderson 2009) on the MI355X: k_inflate_rows against its closed form, the field update
fused into both one-pass GC sweep forms against the NumPy oracle (tests/_anderson2009.py) on the GC goldens and seeded
cases, chained cycles, the cases that must leave everything as without it, the C-ABI forms and the register budget."""
import numpy as np
import pytest

import _anderson2009 as a09
from conftest import load_golden
from test_gpu_parity import assert_parity, golden_kwargs, _make_api_objects

pytestmark = pytest.mark.gpu

GC_GOLDENS = ["G2", "G3", "G5", "G6", "G8", "G12"]
MAXERR = {}


def _ctx():
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    ctx.set_adaptive_inflation(None)
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    ctx.set_option("path", 0)
    return ctx


def _field(N, seed=0):
    """Spatially varying mean in [1, 2], sd 0.6."""
    rng = np.random.default_rng(seed)
    lam = 1.0 + 0.5 * (1.0 + np.sin(0.37 * np.arange(N) + rng.uniform(0, 6.28)))
    return np.stack([lam, np.full(N, 0.6)], axis=1)


def assert_field(got, ref, what):
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    m = float(err.max()) if err.size else 0.0
    MAXERR[what] = m
    print("%s: max relative field error %.3e" % (what, m))
    assert m <= 1e-10, "%s: field relative error %.3e" % (what, m)


def _golden_case(name):
    g = load_golden(name)
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    X = g["X"].reshape(N, M).copy()
    idx, wts = g["sten_idx"], g["sten_wts"]

    def H(Xi):
        return (wts[:, :, None] * Xi[idx]).sum(axis=1)
    return g, X, H, (nvar, nt, ny, nx)


def _oracle(g, X, H, shape, field, **bounds):
    return a09.cycle(X, H, g["ob_value"], g["ob_error"], g["ob_assim"], g["ob_lat"], g["ob_lon"], g["ob_radius"],
                     g["grid_lat"], g["grid_lon"], shape, field, **bounds)


def _run_fused(ctx, g, X, H, field, **bounds):
    """Device prior inflation, HX from the inflated prior, efa_ensrf_cycle_dev with the field set (member form)."""
    N, M = X.shape
    P = len(g["ob_value"])
    Xd = ctx.to_device(X)
    F = ctx.to_device(field)
    ctx.inflate_rows(N, M, Xd, F)
    Xi = Xd.download()
    Yp = ctx.to_device(H(Xi))
    ym = ctx.empty((max(P, 1),))
    ctx.form_perts(P, M, Yp, ym, Yp)
    ctx.set_adaptive_inflation(F, N, **bounds)
    try:
        diag = ctx.ensrf_cycle(N, M, P, Xd, Xd, ym, Yp, g["ob_value"], g["ob_error"], g["ob_assim"], **golden_kwargs(g))
    finally:
        ctx.set_adaptive_inflation(None)
    return Xd.download(), F.download(), diag, Xi


def _run_perts(ctx, g, X, H, field):
    """The same through efa_ensrf_update (perturbation form of the state phase)."""
    from oracle import ensrf_oracle as orc
    N, M = X.shape
    Xi = a09.inflate(X, field[:, 0])
    xbm, Xbp = orc.format_prior_state(Xi, H(Xi))
    F = ctx.to_device(field)
    ctx.set_adaptive_inflation(F, N)
    try:
        diag = ctx.ensrf_update_host(xbm, Xbp, N, g["ob_value"], g["ob_error"], g["ob_assim"], **golden_kwargs(g))
    finally:
        ctx.set_adaptive_inflation(None)
    return orc.format_posterior_state(xbm, Xbp, N), F.download(), diag


def _check(name, got_post, got_field, diag, ref):
    post, fref, rdiag, _ = ref
    assert_parity(got_post, post, name + " posterior")
    for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
        assert_parity(diag[key], rdiag[key], name + " " + key)
    assert np.array_equal(np.asarray(diag["assimilated"], bool), rdiag["assimilated"])
    assert_field(got_field, fref, name)


# ---- k_inflate_rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 7, 80, 100, 256])
def test_inflate_rows_matches_closed_form(M):
    ctx = _ctx()
    rng = np.random.default_rng(M)
    N = 1037
    X = rng.standard_normal((N, M)) * 3.0 + 1.0
    field = _field(N, M)
    field[::5, 0] = 1.0                                    # untouched rows
    Xd = ctx.to_device(X)
    F = ctx.to_device(field)
    ctx.inflate_rows(N, M, Xd, F)
    got = Xd.download()
    assert_parity(got, a09.inflate(X, field[:, 0]), "inflate M=%d" % M)
    assert np.array_equal(got[::5], X[::5]), "rows with lambda 1 must stay bit for bit"
    sp = got.std(axis=1) / X.std(axis=1)
    assert np.allclose(sp, np.sqrt(field[:, 0]), rtol=1e-12)


# ---- goldens: both state phases, the Python API ----------------------------------------------------------------------
@pytest.mark.parametrize("name", GC_GOLDENS)
def test_fused_cycle_matches_oracle_on_goldens(name):
    g, X, H, shape = _golden_case(name)
    field = _field(X.shape[0], 1)
    ref = _oracle(g, X, H, shape, field)
    got, F, diag, Xi = _run_fused(_ctx(), g, X, H, field)
    assert_parity(Xi, ref[3], name + " inflated prior")
    _check(name + " fused", got, F, diag, ref)
    assert np.abs(F - field).max() > 1e-6, "the field did not move"


@pytest.mark.parametrize("name", GC_GOLDENS)
def test_perturbation_state_phase_matches_oracle_on_goldens(name):
    g, X, H, shape = _golden_case(name)
    field = _field(X.shape[0], 2)
    ref = _oracle(g, X, H, shape, field)
    got, F, diag = _run_perts(_ctx(), g, X, H, field)
    _check(name + " perts", got, F, diag, ref)


@pytest.mark.parametrize("name", ["G2", "G6", "G12"])
def test_ensrf_update_api_matches_oracle(name):
    from efa_xray_amd import EnSRF, AdaptiveInflation
    g, X, H, shape = _golden_case(name)
    state, obs = _make_api_objects(g)
    before = state.to_vect().copy()
    ai = AdaptiveInflation(state, ("adaptive", "/nonexistent/prior_inflation.nc", (1.0, 0.6)))
    field = _field(X.shape[0], 3)
    ai.inflation.from_vect(field)
    ref = _oracle(g, X, H, shape, field)
    got, _ = EnSRF(state, obs, verbose=False, loc="GC", adaptive_inflation=ai).update()
    assert_parity(got.to_vect(), ref[0], name + " EnSRF posterior")
    assert_field(ai.inflation.to_vect(), ref[1], name + " EnSRF field")
    assert np.array_equal(state.to_vect(), before), "the caller's state must not change"


# ---- seeded cases: both sweep forms ---------------------------------------------------------------------------------
def _synthetic(M, seed, ny=9, nx=23, n_lead=5, P=90):
    rng = np.random.default_rng(seed)
    lat = np.linspace(30.0, 52.0, ny)[:, None] * np.ones((1, nx))
    lon = np.linspace(-110.0, -70.0, nx)[None, :] * np.ones((ny, 1))
    N = n_lead * ny * nx
    X = rng.standard_normal((N, 1)) * 2 + rng.standard_normal((N, M)) * rng.uniform(0.5, 2.0, (N, 1))
    X[7] = 3.25                                           # a zero-spread row
    rows = rng.integers(0, N, P)
    col = rows % (ny * nx)
    g = dict(shape=np.array([n_lead, 1, ny, nx, M]), loc="GC", grid_lat=lat, grid_lon=lon,
             ob_lat=lat.reshape(-1)[col] + rng.uniform(-0.3, 0.3, P), ob_lon=lon.reshape(-1)[col] + rng.uniform(-0.3, 0.3, P),
             ob_radius=rng.uniform(300.0, 1500.0, P), ob_error=rng.uniform(0.2, 2.0, P), ob_assim=rng.random(P) > 0.1,
             sten_idx=rows[:, None], sten_wts=np.ones((P, 1)))
    g["ob_value"] = X[rows].mean(axis=1) + rng.standard_normal(P) * 2.0
    g["ob_radius"][~g["ob_assim"]] = np.nan

    def H(Xi):
        return Xi[rows].copy()
    return g, X, H, (n_lead, 1, ny, nx)


@pytest.mark.parametrize("M", [4, 20, 80, 100, 104, 51, 81, 128, 256])
@pytest.mark.parametrize("form", ["fused", "perts"])
def test_seeded_cases_both_sweep_forms(M, form):
    """Even M <= 104: the row-per-lane kernel; odd M and M > 104: the quad kernel."""
    g, X, H, shape = _synthetic(M, 40 + M)
    field = _field(X.shape[0], M)
    ref = _oracle(g, X, H, shape, field)
    ctx = _ctx()
    if form == "fused":
        got, F, diag, _ = _run_fused(ctx, g, X, H, field)
    else:
        got, F, diag = _run_perts(ctx, g, X, H, field)
    _check("seeded M=%d %s" % (M, form), got, F, diag, ref)
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(got)), "zero-spread rows must stay finite"
    assert np.array_equal(F[7], field[7]), "a zero-spread row has r = 0: its field stays"


def test_bounds_and_sd_lower_on_device():
    g, X, H, shape = _synthetic(40, 7)
    field = _field(X.shape[0], 9)
    bounds = dict(lower=1.2, upper=1.6, sd_lower=0.55)
    field[:, 0] = np.clip(field[:, 0], 1.2, 1.6)
    ref = _oracle(g, X, H, shape, field, **bounds)
    got, F, diag, _ = _run_fused(_ctx(), g, X, H, field, **bounds)
    _check("bounds", got, F, diag, ref)
    assert F[:, 0].min() >= 1.2 and F[:, 0].max() <= 1.6 and F[:, 1].min() >= 0.55


def test_three_chained_cycles():
    g, X, H, shape = _synthetic(80, 11)
    field = _field(X.shape[0], 11)
    rfield, rX = field.copy(), X.copy()
    ctx = _ctx()
    gX, gfield = X.copy(), field.copy()
    for cyc in range(3):
        g["ob_value"] = g["ob_value"] + 0.3 * cyc
        post, rfield, _, _ = _oracle(g, rX, H, shape, rfield)
        rX = post
        gX, gfield, _, _ = _run_fused(ctx, g, gX, H, gfield)
        assert_parity(gX, rX, "cycle %d posterior" % cyc)
        assert_field(gfield, rfield, "cycle %d" % cyc)


def test_unit_field_is_bit_identical_to_plain_gc():
    g, X, H, shape = _synthetic(80, 12)
    N, M = X.shape
    field = np.stack([np.ones(N), np.zeros(N)], axis=1)
    ctx = _ctx()
    got, F, _, _ = _run_fused(ctx, g, X, H, field)
    Xd = ctx.to_device(X)
    P = len(g["ob_value"])
    ym, Yp = ctx.empty((P,)), ctx.to_device(H(X))
    ctx.form_perts(P, M, Yp, ym, Yp)
    ctx.ensrf_cycle(N, M, P, Xd, Xd, ym, Yp, g["ob_value"], g["ob_error"], g["ob_assim"], **golden_kwargs(g))
    assert np.array_equal(got, Xd.download()), "a (1, 0) field must leave the posterior bit for bit"
    assert np.array_equal(F, field)


def test_nothing_assimilated_leaves_field_and_inflated_prior():
    g, X, H, shape = _synthetic(52, 13)
    g["ob_assim"][:] = False
    g["ob_radius"][:] = np.nan
    field = _field(X.shape[0], 13)
    got, F, diag, Xi = _run_fused(_ctx(), g, X, H, field)
    assert_parity(got, Xi, "nothing assimilated: the posterior is the inflated prior")
    assert np.array_equal(F, field)


def test_combined_with_rtps():
    from efa_xray_amd import _lib
    from test_relaxation_host import relax
    g, X, H, shape = _synthetic(80, 14)
    field = _field(X.shape[0], 14)
    post, fref, _, Xi = _oracle(g, X, H, shape, field)
    ctx = _ctx()
    ctx.set_relaxation(_lib.RELAX_RTPS, 0.9)
    try:
        got, F, _, _ = _run_fused(ctx, g, X, H, field)
    finally:
        ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    assert_parity(got, relax(Xi, post, rtps=0.9), "adaptive + rtps")
    assert_field(F, fref, "adaptive + rtps")


def test_two_call_resident_form_equals_fused_cycle():
    g, X, H, shape = _synthetic(80, 15)
    N, M = X.shape
    P = len(g["ob_value"])
    field = _field(N, 15)
    ctx = _ctx()
    got, F, _, _ = _run_fused(ctx, g, X, H, field)
    Xd, F2 = ctx.to_device(X), ctx.to_device(field)
    ctx.inflate_rows(N, M, Xd, F2)
    Yp = ctx.to_device(H(Xd.download()))
    ym = ctx.empty((P,))
    kw = golden_kwargs(g)
    post = ctx.empty((N, M))
    ctx.form_perts(P, M, Yp, ym, Yp)
    ctx.set_adaptive_inflation(F2, N)
    try:
        ctx.obs_phase(M, P, ym, Yp, g["ob_value"], g["ob_error"], g["ob_assim"], kw["loc_mode"], kw["ob_lat"], kw["ob_lon"],
                      kw["ob_halfwidth"])
        ctx.state_cycle(N, M, Xd, post, kw["grid_lat"], kw["grid_lon"], kw["n_lead"])
    finally:
        ctx.set_adaptive_inflation(None)
    assert np.array_equal(post.download(), got)
    assert np.array_equal(F2.download(), F)


def test_state_phase_refuses_what_it_cannot_update():
    from efa_xray_amd import _lib
    g, X, H, shape = _synthetic(20, 16)
    N, M = X.shape
    P = len(g["ob_value"])
    ctx = _ctx()
    F = ctx.to_device(_field(N))
    Xd = ctx.to_device(X)
    kw = golden_kwargs(g)
    try:
        ctx.set_adaptive_inflation(F, N + 1)
        with pytest.raises(_lib.EfaError, match="rows"):
            ctx.ensrf_cycle(N, M, P, Xd, Xd, ctx.empty((P,)), ctx.to_device(H(X)), g["ob_value"], g["ob_error"],
                            g["ob_assim"], **kw)
        ctx.set_adaptive_inflation(F, N)
        with pytest.raises(_lib.EfaError, match="GC localisation"):
            ctx.ensrf_cycle(N, M, P, Xd, Xd, ctx.empty((P,)), ctx.to_device(H(X)), g["ob_value"], g["ob_error"],
                            g["ob_assim"])
        ctx.set_option("gc_onepass", 0)
        with pytest.raises(_lib.EfaError, match="gc_onepass"):
            ctx.ensrf_cycle(N, M, P, Xd, Xd, ctx.empty((P,)), ctx.to_device(H(X)), g["ob_value"], g["ob_error"],
                            g["ob_assim"], **kw)
    finally:
        ctx.set_option("gc_onepass", 1)
        ctx.set_adaptive_inflation(None)


# ---- configs[2] size --------------------------------------------------------------------------------------------------
def test_config2_size_all_obs_on_a_slab():
    """configs[2]: 361 x 720 columns x 148 slabs x 80 members, 5 000 obs, GC 1 000 km, through the fused cycle with a
    varying field; every diagnostic of all 5 000 obs and the field and posterior of 48 columns x 8 slabs against the oracle
    (state rows are independent given the obs block, as in test_gpu_configs.py)."""
    ny, nx, n_lead, M, P = 361, 720, 148, 80, 5000
    ncol, N = ny * nx, ny * nx * n_lead
    rng = np.random.default_rng(2)
    lat = np.linspace(-90.0, 90.0, ny)
    lon = np.linspace(0.0, 359.5, nx)
    glat = np.repeat(lat, nx)
    glon = np.tile(lon, ny)
    ctx = _ctx()
    Xd = ctx.empty((N, M))
    ctx.fill_synthetic(N, 0, M, 2024, 1.0, Xd)
    # the field: smooth in the column, varying with the slab
    lam_col = 1.0 + 0.5 * (1.0 + np.sin(np.radians(glat) * 3.0) * np.cos(np.radians(glon) * 2.0))
    field = np.empty((N, 2))
    for l in range(n_lead):
        field[l * ncol:(l + 1) * ncol, 0] = 1.0 + (lam_col - 1.0) * (0.5 + 0.5 * ((l % 7) / 6.0))
    field[:, 1] = 0.6
    F = ctx.to_device(field)
    # obs at state rows near the middle latitudes
    orow = rng.integers(0, N, P)
    ocol = orow % ncol
    ob_lat = glat[ocol] + rng.uniform(-0.2, 0.2, P)
    ob_lon = glon[ocol] + rng.uniform(-0.2, 0.2, P)
    hw = np.full(P, 1000.0)
    err = rng.uniform(0.5, 1.5, P)
    assim = np.ones(P, bool)
    ctx.inflate_rows(N, M, Xd, F)
    HX = np.stack([Xd.download_rows(int(r), int(r) + 1)[0] for r in orow])
    val = HX.mean(axis=1) + rng.standard_normal(P)
    # the slab: 48 columns around the most observed column, 8 slabs
    cf = int(np.bincount(ocol, minlength=ncol).argmax())
    cf = min(max(cf - 24, 0), ncol - 48)
    leads = [0, 1, 37, 74, 100, 120, 146, 147]
    rows_f = np.concatenate([np.arange(l * ncol + cf, l * ncol + cf + 48) for l in leads])
    Xf = np.concatenate([Xd.download_rows(l * ncol + cf, l * ncol + cf + 48) for l in leads])
    post = ctx.empty((N, M))
    ym = ctx.empty((P,))
    Yp = ctx.to_device(HX)
    ctx.form_perts(P, M, Yp, ym, Yp)
    ctx.set_adaptive_inflation(F, N)
    try:
        diag = ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, val, err, assim, 1, ob_lat, ob_lon, hw, glat, glon, n_lead)
    finally:
        ctx.set_adaptive_inflation(None)
    got_post = np.concatenate([post.download_rows(l * ncol + cf, l * ncol + cf + 48) for l in leads])
    got_field = F.download()[rows_f]
    # the oracle on the slab of the inflated prior, with the obs priors of the whole run
    ref_post, ref_field, rdiag, _ = a09.cycle(Xf, lambda _: HX, val, err, assim, ob_lat, ob_lon, hw,
                                              glat[cf:cf + 48].reshape(1, 48), glon[cf:cf + 48].reshape(1, 48),
                                              (len(leads), 1, 1, 48), field[rows_f], prior_inflated=True)
    assert_parity(got_post, ref_post, "configs[2] slab posterior")
    assert_field(got_field, ref_field, "configs[2] slab")
    assert np.abs(got_field - field[rows_f]).max() > 1e-6, "the slab's field did not move"
    for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
        assert_parity(diag[key], rdiag[key], "configs[2] " + key)


# ---- register budget ---------------------------------------------------------------------------------------------------
def test_adaptive_sweep_fits_its_register_budget():
    """No scratch for the ADAPT lane kernels at configs[2]'s and configs[3]'s member counts (80, 100), both state forms."""
    from efa_xray_amd import _lib
    from _codeobj import gc_kernel_fragment, kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    for part in [gc_kernel_fragment("lane", "adapt", "f64", mp, fused) for mp in (80, 100) for fused in (1, 0)]:
        hits = [k for n, k in tab.items() if part in n]
        assert len(hits) == 1, part
        k = hits[0]
        assert k.get(".vgpr_spill_count", 0) == 0, (part, k[".vgpr_count"], k.get(".vgpr_spill_count"))
        assert k.get(".private_segment_fixed_size", 0) == 0, (part, k.get(".private_segment_fixed_size"))


# ---- the Python API with the default forward operator (prior inflated on the device) ---------------------------------------
def _g11_forward(g):
    """The reference's point interpolation of every G11 ob as a function of the member rows (linear in the state)."""
    from oracle import ensrf_oracle as orc
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    P = len(g["ob_value"])

    def H(Xi):
        Xs = np.asarray(Xi).reshape(nvar, nt, ny, nx, M)
        return np.stack([np.asarray(orc.interpolate(Xs[g["ob_var"][k]], g["grid_lat"], g["grid_lon"], g["validtime"],
                                                    g["ob_time"][k], g["ob_lat"][k], g["ob_lon"][k])).reshape(M)
                         for k in range(P)])
    return H


def test_ensrf_update_default_forward_operator_inflates_on_device():
    from efa_xray_amd import EnsembleState, Observation, EnSRF, AdaptiveInflation
    g = load_golden("G11")
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    names = [str(n) for n in g["var_names"]]
    state = EnsembleState.from_array(g["X"], g["grid_lat"], g["grid_lon"], varnames=names, validtime=g["validtime"])
    obs = [Observation(value=float(g["ob_value"][k]), obtype=names[g["ob_var"][k]], time=g["ob_time"][k],
                       error=float(g["ob_error"][k]), lat=float(g["ob_lat"][k]), lon=float(g["ob_lon"][k]),
                       assimilate_this=bool(g["ob_assim"][k]), localize_radius=float(g["ob_radius"][k]))
           for k in range(len(g["ob_value"]))]
    X = g["X"].reshape(N, M)
    H = _g11_forward(g)
    assert_parity(H(X), g["HX"], "G11 forward operator")
    field = _field(N, 5)
    ai = AdaptiveInflation(state, ("adaptive", None, (1.0, 0.6)))
    ai.inflation.from_vect(field)
    before = state.to_vect().copy()
    flt = EnSRF(state, obs, verbose=False, loc="GC", adaptive_inflation=ai)
    assert flt._default_forward_operator()
    got, _ = flt.update()
    ref = _oracle(g, X, H, (nvar, nt, ny, nx), field)
    assert_parity(got.to_vect(), ref[0], "G11 device-inflated posterior")
    assert_field(ai.inflation.to_vect(), ref[1], "G11 EnSRF field")
    assert np.array_equal(state.to_vect(), before), "the caller's state must not change"
