"""The batch observation-space solver (ETKF) on the MI355X, against the NumPy model of tests/_etkf.py: T, w, the
eigenvalues of A, the diagnostics and the posterior members to 1e-10 of the largest magnitude of each array, at every size at
which the code takes another path (one tile and several, odd M, P no multiple of the chunk, the last M that runs from LDS and
the first that does not, the widest M, more obs than a serial window holds); determinism, unread obs, the entry points against
one another bit for bit, float32 rows, relaxation, the outlier check, the refusals, and the Python class.  Every test sets
"obs_solver" back to 0: the per-device context is shared."""
import functools

import numpy as np
import pytest

import _etkf as ek
import _outlier as qc
from test_relaxation_host import relax

pytestmark = pytest.mark.gpu

TOL = 1e-10
SWEEP_CAP = 30
LDS_MAX_M = 136     # the eigen-solve's array lives in LDS up to here
SIZES = [(2, 1), (3, 5), (16, 64), (17, 33), (50, 1000), (100, 257), (128, 300), (LDS_MAX_M, 300), (LDS_MAX_M + 1, 300),
         (200, 300), (256, 520), (20, 20000)]
N_ROWS = 5000


def _reset(ctx, solver=0):
    from efa_xray_amd import _lib
    ctx.set_outlier_threshold(None)
    ctx.set_vertical_localization(None)
    ctx.set_slab_localization(None)
    ctx.set_sampling_error_correction(None)
    ctx.set_adaptive_inflation(None)
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    for key, v in (("path", 0), ("gram", 2), ("pipeline", 1), ("gc_onepass", 1), ("obs_solver", solver)):
        ctx.set_option(key, v)
    return ctx


@pytest.fixture
def ctx():
    from efa_xray_amd import _lib
    c = _reset(_lib.get_context(0), 1)
    yield c
    _reset(c, 0)


@functools.lru_cache(maxsize=None)
def _case(M, P, N=N_ROWS):
    """The seeded case and its model solution, computed once and left unchanged."""
    c = ek.make_case(M, P, N=N)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _obs_block(ctx, HX):
    """The obs block on the device as the front end forms it, and its host image (what the model is fed)."""
    P, M = HX.shape
    Yp = ctx.to_device(np.ascontiguousarray(HX))
    ym = ctx.empty((P,))
    ctx.form_perts(P, M, Yp, ym, Yp)
    return ym, Yp, ym.download(), Yp.download()


def _cycle(ctx, c, value=None, error=None, assim=None, in_place=False, X=None):
    """efa_ensrf_cycle_dev with the obs block copied back: dict of posterior, obs block, diagnostics, prior obs block."""
    X = c["X"] if X is None else X
    N, M = X.shape
    P = c["P"]
    Xd = ctx.to_device(np.ascontiguousarray(X))
    post = Xd if in_place else ctx.empty((N, M))
    ym, Yp, ym0, Yp0 = _obs_block(ctx, c["HX"])
    diag = ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, c["value"] if value is None else value, c["error"] if error is None else error,
                           c["assim"] if assim is None else assim, obs_block_out=True)
    return dict(post=post.download(), ym=ym.download(), Yp=Yp.download(), diag=diag, ym0=ym0, Yp0=Yp0)


def _close(got, want, what, tol=TOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.max(np.abs(want)) if want.size else 0.0
    err = np.max(np.abs(got - want)) if want.size else 0.0
    print("%s: max abs err %.3e, scale %.3e" % (what, err, scale))
    assert np.all(np.isfinite(got)), what + ": not finite"
    assert err <= tol * max(scale, np.finfo(float).tiny), "%s: %.3e > %g * %.3e" % (what, err, tol, scale)


def _check_diag(diag, ref, what):
    a = np.asarray(ref["assimilated"], bool)
    assert np.array_equal(np.asarray(diag["assimilated"], bool), a), what + ": assimilated"
    _close(diag["prior_mean"], ref["prior_mean"], what + " prior_mean")
    _close(diag["prior_var"], ref["prior_var"], what + " prior_var")
    if a.any():
        _close(np.asarray(diag["post_mean"])[a], ref["post_mean"][a], what + " post_mean")
        _close(np.asarray(diag["post_var"])[a], ref["post_var"][a], what + " post_var")
    assert np.all(np.isnan(np.asarray(diag["post_mean"])[~a])), what + ": post_mean written for an ob that is not assimilated"


def _same_bits(a, b, what):
    for k in ("post", "ym", "Yp"):
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s differs" % (what, k)
    for k in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
        assert np.array_equal(np.asarray(a["diag"][k]), np.asarray(b["diag"][k]), equal_nan=True), "%s: %s differs" % (what, k)


def _same_solution(a, b, what):
    for k in ("T", "w", "eigenvalues"):
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s differs" % (what, k)
    assert (a["n_active"], a["sweeps"]) == (b["n_active"], b["sweeps"]), what


# ---- every size: the solution, the diagnostics, the posterior; 1 sweeps below the cap; 2 the same bits twice ----------------------
@pytest.mark.parametrize("M,P", SIZES)
def test_solution_and_posterior_match_the_model(ctx, M, P):
    c = _case(M, P)
    r = _cycle(ctx, c)
    sol = ctx.etkf_solution(M)
    assert ctx.get_option("phase_a_kind") == 5
    ref = ek.etkf_solution(r["ym0"], r["Yp0"], c["value"], c["error"], c["assim"])
    assert ref["cond"] <= 1e4, "cond(A) = %g: the float64 bound of 1e-10 is claimed up to 1e4" % ref["cond"]
    print("M=%d P=%d sweeps=%d cond=%.3g" % (M, P, sol["sweeps"], ref["cond"]))
    assert 1 <= sol["sweeps"] < SWEEP_CAP
    _close(sol["T"], ref["T"], "T")
    _close(sol["w"], ref["w"], "w")
    _close(sol["eigenvalues"] + (M - 1.0), ref["mu"], "eigenvalues of A")
    assert sol["n_active"] == ref["n_active"] == int(c["assim"].sum())
    assert abs(sol["q"] - ref["q"]) <= TOL * abs(ref["q"])
    assert abs(sol["dfs"] - ref["dfs"]) <= TOL * max(1.0, ref["dfs"])
    assert abs(sol["chi2"] - ref["chi2"]) <= TOL * abs(ref["q"])       # q - g.w: the error is that of its terms
    rd = ek.etkf_diagnostics(r["ym0"], r["Yp0"], c["assim"], ref["T"], ref["w"])
    _check_diag(r["diag"], rd, "diagnostics")
    _close(r["ym"], rd["post_ym"], "posterior obs means")
    _close(r["Yp"], rd["post_Yp"], "posterior obs perturbations")
    _close(r["post"], ek.etkf_members(c["X"], ref["T"], ref["w"]), "posterior members")
    again = _cycle(ctx, c)
    _same_bits(r, again, "two identical calls")
    _same_solution(sol, ctx.etkf_solution(M), "two identical calls")


# ---- 3: obs that are not assimilated are not read -------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(17, 33), (100, 257)])
def test_unflagged_obs_may_carry_nan_or_inf(ctx, M, P):
    c = _case(M, P)
    off = ~c["assim"]
    assert off.any()
    base = _cycle(ctx, c)
    sol = ctx.etkf_solution(M)
    for bad_value, bad_error in ((np.nan, np.nan), (np.inf, -np.inf), (-np.inf, 0.0)):
        value, error = c["value"].copy(), c["error"].copy()
        value[off], error[off] = bad_value, bad_error
        r = _cycle(ctx, c, value=value, error=error)
        _same_bits(base, r, "unflagged obs holding %r / %r" % (bad_value, bad_error))
        _same_solution(sol, ctx.etkf_solution(M), "unflagged obs holding %r / %r" % (bad_value, bad_error))


# ---- 4: a NaN value of an assimilated ob reaches g only -------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(17, 33), (LDS_MAX_M + 1, 300)])
def test_nan_value_returns_and_leaves_the_eigenvalues(ctx, M, P):
    c = _case(M, P)
    _cycle(ctx, c)
    sol = ctx.etkf_solution(M)
    value = c["value"].copy()
    value[np.flatnonzero(c["assim"])[0]] = np.nan
    r = _cycle(ctx, c, value=value)
    bad = ctx.etkf_solution(M)
    assert 1 <= bad["sweeps"] < SWEEP_CAP and bad["sweeps"] == sol["sweeps"]
    assert np.array_equal(bad["eigenvalues"], sol["eigenvalues"]) and np.array_equal(bad["T"], sol["T"])
    assert np.all(np.isnan(bad["w"])) and np.all(np.isnan(r["post"])) and np.isnan(bad["chi2"])


# ---- 5: no ob assimilated: what the serial solver returns -----------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(17, 33), (200, 300)])
def test_nothing_assimilated_equals_the_serial_solver(ctx, M, P):
    """Bit for bit: the posterior, the obs block, the flags and prior_mean.  prior_var is the one number the two solvers compute
    with kernels of their own (each the two-pass ddof-0 variance, in its own summation order): 1e-10."""
    c = _case(M, P)
    none = np.zeros(P, dtype=bool)
    b = _cycle(ctx, c, assim=none)
    sol = ctx.etkf_solution(M)
    assert sol["n_active"] == 0 and sol["sweeps"] == 1 and np.array_equal(sol["T"], np.eye(M)) and not sol["w"].any()
    ctx.set_option("obs_solver", 0)
    s = _cycle(ctx, c, assim=none)
    for k in ("post", "ym", "Yp"):
        assert np.array_equal(b[k], s[k]), k
    _close(b["post"], c["X"], "posterior = prior")     # (member form: mean + perturbation, rebuilt by both alike)
    assert not b["diag"]["assimilated"].any() and not s["diag"]["assimilated"].any()
    assert np.array_equal(b["diag"]["prior_mean"], s["diag"]["prior_mean"])
    _close(b["diag"]["prior_var"], s["diag"]["prior_var"], "prior_var")
    assert np.all(np.isnan(b["diag"]["post_mean"])) and np.all(np.isnan(s["diag"]["post_mean"]))


# ---- 6, 7: the entry points against one another and the perturbation form --------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(50, 1000), (200, 300)])
def test_cycle_equals_obs_phase_plus_state_cycle(ctx, M, P):
    c = _case(M, P)
    N = c["N"]
    for in_place in (False, True):
        one = _cycle(ctx, c, in_place=in_place)
        Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
        post = Xd if in_place else ctx.empty((N, M))
        ym, Yp, _, _ = _obs_block(ctx, c["HX"])
        diag = ctx.obs_phase(M, P, ym, Yp, c["value"], c["error"], c["assim"])
        ctx.state_cycle(N, M, Xd, post)
        ctx.synchronize()
        two = dict(post=post.download(), ym=ym.download(), Yp=Yp.download(), diag=diag)
        _same_bits(one, two, "in place" if in_place else "out of place")


@pytest.mark.parametrize("M,P", [(17, 33), (100, 257), (200, 300)])
def test_perturbation_form_matches_the_model(ctx, M, P):
    c = _case(M, P)
    N = c["N"]
    ym, Yp, ym0, Yp0 = _obs_block(ctx, c["HX"])
    ctx.obs_phase(M, P, ym, Yp, c["value"], c["error"], c["assim"])
    ref = ek.etkf_solution(ym0, Yp0, c["value"], c["error"], c["assim"])
    xm = c["X"].mean(axis=1)
    Xp = c["X"] - xm[:, None]
    for in_place in (False, True):
        xm_d, Xp_d = ctx.to_device(xm), ctx.to_device(np.ascontiguousarray(Xp))
        xo, Xo = (xm_d, Xp_d) if in_place else (ctx.empty((N,)), ctx.empty((N, M)))
        ctx.state_phase(N, M, xm_d, Xp_d, xo, Xo)
        ctx.synchronize()
        xam, Xap = ek.etkf_apply(xm, Xp, ref["T"], ref["w"])
        _close(xo.download(), xam, "posterior means")
        _close(Xo.download(), Xap, "posterior perturbations")


# ---- 8: float32 rows: the float64 call on the widened rows, rounded once -------------------------------------------------
@pytest.mark.parametrize("M,P", [(100, 257), (200, 300)])
def test_f32_rows_are_the_f64_result_rounded_once(ctx, M, P):
    from efa_xray_amd import _lib
    c = _case(M, P)
    N = c["N"]
    X32 = np.ascontiguousarray(c["X"], dtype=np.float32)
    for relaxation in ((_lib.RELAX_NONE, 0.0), (_lib.RELAX_RTPS, 0.9)):
        ctx.set_relaxation(*relaxation)
        ym, Yp, _, _ = _obs_block(ctx, c["HX"])
        ctx.obs_phase(M, P, ym, Yp, c["value"], c["error"], c["assim"])
        Xw = ctx.to_device(X32.astype(np.float64))
        post64 = ctx.empty((N, M))
        ctx.state_cycle(N, M, Xw, post64)
        for in_place in (False, True):
            Xf = ctx.to_device(X32, dtype=np.float32)
            pf = Xf if in_place else ctx.empty((N, M), dtype=np.float32)
            ctx.state_cycle_f32(N, M, Xf, pf)
            ctx.synchronize()
            assert np.array_equal(pf.download(), post64.download().astype(np.float32)), (relaxation, in_place)


# ---- 9: relaxation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(50, 1000), (200, 300)])
@pytest.mark.parametrize("kind", ["rtpp", "rtps"])
def test_relaxation_matches_the_closed_form_on_the_model_posterior(ctx, M, P, kind):
    from efa_xray_amd import _lib
    c = _case(M, P)
    alpha = 0.5 if kind == "rtpp" else 0.9
    ctx.set_relaxation(_lib.RELAX_RTPP if kind == "rtpp" else _lib.RELAX_RTPS, alpha)
    for in_place in (False, True):
        r = _cycle(ctx, c, in_place=in_place)
        ref = ek.etkf_solution(r["ym0"], r["Yp0"], c["value"], c["error"], c["assim"])
        want = relax(c["X"], ek.etkf_members(c["X"], ref["T"], ref["w"]), **{kind: alpha})
        _close(r["post"], want, "%s %s" % (kind, "in place" if in_place else "out of place"))
        rd = ek.etkf_diagnostics(r["ym0"], r["Yp0"], c["assim"], ref["T"], ref["w"])
        _close(r["Yp"], rd["post_Yp"], "the obs block is not relaxed")


# ---- 10: the outlier check ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", [(17, 33), (100, 257), (20, 20000)])
def test_outlier_check_rejects_exactly_and_equals_cleared_flags(ctx, M, P):
    t = 3.0
    c = _case(M, P)
    ym, Yp = ek.ob_priors(c["HX"])
    value, bad = qc.inject(c["HX"], c["value"], c["error"], c["assim"], t, max(2, P // 100), seed=M)
    assert qc.clear_of_threshold(ym, Yp, value, c["error"], t)
    flags = qc.masked_flags(c["HX"], value, c["error"], c["assim"], t)
    assert not flags[bad].any() and flags.any()
    ctx.set_outlier_threshold(t)
    r = _cycle(ctx, c, value=value)
    sol = ctx.etkf_solution(M)
    ctx.set_outlier_threshold(None)
    assert np.array_equal(r["diag"]["assimilated"], flags), "rejected set"
    assert sol["n_active"] == int(flags.sum())
    cleared = _cycle(ctx, c, value=value, assim=flags)
    _same_bits(r, cleared, "outlier check against cleared flags")
    _same_solution(sol, ctx.etkf_solution(M), "outlier check against cleared flags")
    ref = ek.etkf_solution(r["ym0"], r["Yp0"], value, c["error"], flags)
    _close(sol["T"], ref["T"], "T")
    _close(r["post"], ek.etkf_members(c["X"], ref["T"], ref["w"]), "posterior members")


# ---- 11, 12: the refusals, and the context afterwards -----------------------------------------------------------------------------------
def _serial(ctx, c):
    _reset(ctx, 0)
    return _cycle(ctx, c)


def test_refusals_leave_the_context_usable(ctx):
    from efa_xray_amd import _lib
    M, P = 17, 33
    c = _case(M, P)
    N = c["N"]
    fresh = _lib.Context(0)
    try:
        want = _serial(fresh, c)
    finally:
        fresh.close()
    rng = np.random.default_rng(3)
    gc = dict(loc_mode=_lib.LOC_GC, ob_lat=rng.uniform(30, 50, P), ob_lon=rng.uniform(250, 280, P), ob_halfwidth=np.full(P, 800.0))
    zero_err = c["error"].copy()
    zero_err[np.flatnonzero(c["assim"])[1]] = 0.0
    nan_err = c["error"].copy()
    nan_err[np.flatnonzero(c["assim"])[0]] = np.nan

    def obs_phase(**kw):
        ym, Yp, _, _ = _obs_block(ctx, c["HX"])
        return ctx.obs_phase(M, P, ym, Yp, c["value"], kw.pop("error", c["error"]), c["assim"], **kw)

    def refused(setup, call):
        _reset(ctx, 1)
        setup()
        with pytest.raises(_lib.EfaError) as e:
            call()
        assert e.value.status == _lib.EFA_ERR_INVALID, str(e.value)
        with pytest.raises(_lib.EfaError):          # no batch solution was left behind
            ctx.etkf_solution(M)
        _same_bits(_serial(ctx, c), want, "serial solver after a refusal")

    field = ctx.to_device(np.tile([1.0, 0.6], (N, 1)))
    _serial(ctx, c)     # (whatever ran before this test: the last obs phase is now a serial one)
    refused(lambda: None, lambda: obs_phase(**gc))
    refused(lambda: ctx.set_adaptive_inflation(field, N), lambda: obs_phase())
    refused(lambda: ctx.set_option("path", _lib.PATH_SWEEP), lambda: obs_phase())
    refused(lambda: None, lambda: obs_phase(error=zero_err))
    refused(lambda: None, lambda: obs_phase(error=nan_err))
    refused(lambda: None, lambda: _cycle(ctx, c, error=zero_err))
    # a serial obs phase leaves no batch solution; neither does another M
    _reset(ctx, 1)
    _cycle(ctx, c)
    with pytest.raises(_lib.EfaError):
        ctx.etkf_solution(M + 1)
    assert ctx.etkf_solution(M)["sweeps"] >= 1
    _serial(ctx, c)
    with pytest.raises(_lib.EfaError):
        ctx.etkf_solution(M)
    with pytest.raises(_lib.EfaError):
        ctx.set_option("obs_solver", 2)


# ---- 13, 14: the Python class ---------------------------------------------------------------------------------------------------------------
def _api_case(dtype=None):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(11)
    nvar, nt, ny, nx, M, P = 2, 2, 6, 7, 12, 30
    lat, lon = np.meshgrid(np.linspace(20, 60, ny), np.linspace(200, 280, nx), indexing="ij")
    arr = rng.standard_normal((nvar, nt, ny, nx, 1)) + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon, dtype=dtype)
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
                   lat=float(lat.reshape(-1)[col]), lon=float(lon.reshape(-1)[col]), assimilate_this=(k % 7 != 3))
        ob.row = int(rows[k])
        obs.append(ob)
    return state, obs


def _ob_diag(obs):
    d = {k: np.array([np.nan if getattr(o, k, None) is None else getattr(o, k) for o in obs], float)
         for k in ("prior_mean", "prior_var", "post_mean", "post_var")}
    d["assimilated"] = np.array([bool(o.assimilated) for o in obs])
    return d


def test_etkf_class_against_the_model(ctx):
    from efa_xray_amd import ETKF
    state, obs = _api_case()
    f = ETKF(state, obs, verbose=False)
    HX = np.asarray(f.compute_ob_estimates(), dtype=np.float64)
    ym, Yp = ek.ob_priors(HX)
    value = np.array([o.value for o in obs])
    error = np.array([o.error for o in obs])
    assim = np.array([o.assimilate_this for o in obs])
    ref = ek.etkf_solution(ym, Yp, value, error, assim)
    post, obs_out = f.update()
    assert obs_out is obs and post is not state
    _close(post.to_vect(), ek.etkf_members(state.to_vect(), ref["T"], ref["w"]), "ETKF.update posterior")
    _check_diag(_ob_diag(obs), ek.etkf_diagnostics(ym, Yp, assim, ref["T"], ref["w"]), "ETKF.update")
    ls = f.last_solve
    assert sorted(ls) == ["chi2", "dfs", "eigenvalues", "n_active", "sweeps"]
    assert abs(ls["chi2"] - ref["chi2"]) <= TOL * ref["q"] and abs(ls["dfs"] - ref["dfs"]) <= TOL * max(1.0, ref["dfs"])
    _close(ls["eigenvalues"] + 11.0, ref["mu"], "last_solve eigenvalues")
    assert ls["n_active"] == int(assim.sum()) and 1 <= ls["sweeps"] < SWEEP_CAP
    # streamed: the resident run bit for bit
    state2, obs2 = _api_case()
    spost, _ = ETKF(state2, obs2, verbose=False, streamed=True, stream_chunk_cols=16).update()
    assert np.array_equal(spost.to_vect(), post.to_vect())
    for k, v in _ob_diag(obs2).items():
        assert np.array_equal(v, _ob_diag(obs)[k], equal_nan=True), k
    # a float32 state: the float64 update of the widened state, rounded once
    s32, o32 = _api_case(dtype=np.float32)
    p32, _ = ETKF(s32, o32, verbose=False).update()
    assert p32.to_vect().dtype == np.float32
    s64, o64 = _api_case(dtype=np.float32)
    p64, _ = ETKF(s64.astype(np.float64), o64, verbose=False).update()
    assert np.array_equal(p32.to_vect(), p64.to_vect().astype(np.float32))
    # rtps and inflation= run through the same plan
    s3, o3 = _api_case()
    p3, _ = ETKF(s3, o3, verbose=False, rtps=0.9).update()
    want = relax(state.to_vect(), ek.etkf_members(state.to_vect(), ref["T"], ref["w"]), rtps=0.9)
    _close(p3.to_vect(), want, "ETKF rtps")


def test_ensrf_is_unchanged_by_an_etkf_before_it(ctx):
    from efa_xray_amd import ETKF, EnSRF
    state, obs = _api_case()
    before, _ = EnSRF(state, obs, verbose=False).update()
    d_before = _ob_diag(obs)
    s2, o2 = _api_case()
    ETKF(s2, o2, verbose=False).update()
    assert ctx.get_option("obs_solver") == 1
    s3, o3 = _api_case()
    after, _ = EnSRF(s3, o3, verbose=False).update()
    assert ctx.get_option("obs_solver") == 0 and ctx.get_option("phase_a_kind") != 5
    assert np.array_equal(after.to_vect(), before.to_vect())
    for k, v in _ob_diag(o3).items():
        assert np.array_equal(v, d_before[k], equal_nan=True), k
    # ... and the two are different filters: the means differ by a visible share of the increment
    etkf_post, _ = ETKF(*_api_case(), verbose=False).update()
    inc = np.max(np.abs(before.to_vect().mean(axis=1) - state.to_vect().mean(axis=1)))
    assert np.max(np.abs(etkf_post.to_vect().mean(axis=1) - before.to_vect().mean(axis=1))) > 1e-3 * inc
