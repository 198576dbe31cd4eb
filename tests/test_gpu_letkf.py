"""The LETKF on the MI355X against the NumPy model of tests/_letkf.py: the per-point pairs of
efa_letkf_weights_dev, the posterior members, the posterior obs block, the diagnostics and the per-column statistics to 1e-10 of
the largest magnitude of each array (the project's float64 bound, claimed up to cond(A) <= 1e4: asserted from the model for every
column), at every size at which the kernel takes another path; short reach (columns no ob reaches come back bit for bit), the
chunk edges of the Gram, no work, determinism, the entries against one another bit for bit, unread obs, a NaN value, invalid
variances, relaxation, the outlier check, float32 rows, the unlocalised limit against the batch solver, the refusals, and the
Python class.  Every test restores the shared context's settings."""
import functools

import numpy as np
import pytest

import _etkf as ek
import _letkf as lk
import _outlier as qc
from _letkf_gpu import TOL, SWEEP_CAP, COND_CAP, _reset, _obs_block, _close, _check_diag, _same_bits
from test_relaxation_host import relax

pytestmark = pytest.mark.gpu

SIZES = [(2, 1, 3, 5, 1), (3, 5, 3, 5, 2), (16, 64, 5, 7, 3), (17, 33, 5, 7, 3), (40, 400, 6, 7, 3), (80, 700, 6, 7, 2),
         (100, 257, 5, 7, 1), (136, 300, 3, 6, 1)]
SHORT = (16, 40, 6, 7, 3)
SHORT_SEED = 0      # checked below from the model: a block of 16 columns mixes reached and unreached columns


@pytest.fixture
def ctx():
    from efa_xray_amd import _lib
    c = _reset(_lib.get_context(0))
    yield c
    _reset(c)


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _case(M, P, ny, nx, n_lead, seed=0, hw=(300.0, 3000.0)):
    """The seeded case, computed once and left unchanged."""
    return _freeze(lk.make_case(M, P, ny, nx, n_lead, seed=seed, hw=hw))


@functools.lru_cache(maxsize=None)
def _model(M, P, ny, nx, n_lead, seed=0, hw=(300.0, 3000.0)):
    """... and its model solution (the obs block of compute_ob_priors is what form_perts leaves on the device to the last bit or two)."""
    c = _case(M, P, ny, nx, n_lead, seed, hw)
    return lk.letkf_cycle(c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                          c["grid_lon"], n_lead)


def _cycle(ctx, c, in_place=False, obs_block_out=True, f32=False, X=None, **over):
    """efa_letkf_cycle_dev: dict of posterior, obs block, diagnostics, column statistics, prior obs block."""
    g = dict(c, **over)
    X = g["X"] if X is None else X
    N, M = X.shape
    P = g["P"]
    dt = np.float32 if f32 else np.float64
    Xd = ctx.to_device(np.ascontiguousarray(X, dtype=dt), dtype=dt)
    post = Xd if in_place else ctx.empty((N, M), dtype=dt)
    ym, Yp, ym0, Yp0 = _obs_block(ctx, g["HX"], M)
    stats = ctx.empty((g["ncol"], 3))
    diag = ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"],
                           g["grid_lat"], g["grid_lon"], g["n_lead"], obs_block_out=obs_block_out, col_stats=stats, f32=f32)
    return dict(post=post.download(), ym=ym.download()[:P], Yp=Yp.download()[:P], diag=diag, stats=stats.download(), ym0=ym0, Yp0=Yp0)


def _probe(ctx, c, lat=None, lon=None, **over):
    g = dict(c, **over)
    M, P = g["M"], g["P"]
    ym, Yp, _, _ = _obs_block(ctx, g["HX"], M)
    return ctx.letkf_weights(M, P, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"],
                             g["grid_lat"] if lat is None else lat, g["grid_lon"] if lon is None else lon)


def _check_against_model(r, ref, c, what):
    st = ref["stats"]
    print("%s: cond(A) max %.3g, n_local %d..%d, sweeps max %d" % (what, st["cond"].max(), st["n_local"].min(), st["n_local"].max(),
                                                                  int(r["stats"][:, 2].max())))
    assert st["cond"].max() <= COND_CAP, "cond(A) = %g: the float64 bound of 1e-10 is claimed up to 1e4" % st["cond"].max()
    _close(r["post"], ref["post"], what + " posterior members")
    _close(r["Yp"], ref["Yp"], what + " posterior obs perturbations")
    _close(r["ym"], ref["ym"], what + " posterior obs means")
    _check_diag(r["diag"], ref["diag"], what)
    assert np.array_equal(r["stats"][:, 0], st["n_local"].astype(np.float64)), what + ": n_local"
    assert np.abs(r["stats"][:, 1] - st["dfs"]).max() <= TOL * max(1.0, st["dfs"].max()), what + ": dfs"
    reached = st["n_local"] > 0
    assert np.all(r["stats"][reached, 2] >= 1) and np.all(r["stats"][:, 2] < SWEEP_CAP) and np.all(r["stats"][~reached, 2] == 0)


# ---- every size: the pairs, the posterior, the obs block, the diagnostics, the statistics ------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead", SIZES)
def test_cycle_and_weights_match_the_model(ctx, M, P, ny, nx, n_lead):
    c = _case(M, P, ny, nx, n_lead)
    ref = _model(M, P, ny, nx, n_lead)
    r = _cycle(ctx, c)
    assert ctx.get_option("phase_a_kind") == 6
    _check_against_model(r, ref, c, "M=%d P=%d" % (M, P))
    T, w, st = _probe(ctx, c)
    _close(T, ref["T"], "T")
    _close(w, ref["w"], "w")
    assert np.array_equal(st, r["stats"])
    assert np.array_equal(T, np.swapaxes(T, 1, 2)), "T is mirrored: symmetric to the bit"
    if M == 2:
        assert ref["stats"]["n_local"].min() == 0 and ref["stats"]["n_local"].max() == 1


def test_members_above_136_are_refused_and_the_context_goes_on(ctx):
    from efa_xray_amd import _lib
    c = _case(17, 33, 5, 7, 3)
    want = _cycle(ctx, c)
    big = lk.make_case(137, 20, 3, 5, 1)
    with pytest.raises(_lib.EfaError) as e:
        _cycle(ctx, big)
    assert e.value.status == _lib.EFA_ERR_INVALID and "136" in str(e.value) and "LDS" in str(e.value)
    with pytest.raises(_lib.EfaError) as e:
        _probe(ctx, big)
    assert e.value.status == _lib.EFA_ERR_INVALID
    _same_bits(_cycle(ctx, c), want, "after a refused M")


# ---- short reach: a block of 16 columns mixes reached and unreached columns ------------------------------------------------------
def _short():
    c = _case(*SHORT, seed=SHORT_SEED, hw=(100.0, 400.0))
    ref = _model(*SHORT, seed=SHORT_SEED, hw=(100.0, 400.0))
    reached = ref["stats"]["n_local"] > 0
    mixed = [b for b in range(0, c["ncol"], 16) if reached[b:b + 16].any() and not reached[b:b + 16].all()]
    assert mixed, "no block of 16 columns mixes reached and unreached columns: pick another seed"
    return c, ref, reached


@pytest.mark.parametrize("rtps", [None, 0.9])
def test_unreached_columns_keep_their_bits_and_reached_ones_match(ctx, rtps):
    from efa_xray_amd import _lib
    c, ref, reached = _short()
    if rtps:
        ctx.set_relaxation(_lib.RELAX_RTPS, rtps)
    want = ref["post"] if not rtps else relax(c["X"], ref["post"], rtps=rtps)
    for in_place in (False, True):
        r = _cycle(ctx, c, in_place=in_place)
        rows = lambda cols: (np.asarray(cols)[None, :] + c["ncol"] * np.arange(c["n_lead"])[:, None]).reshape(-1)
        un, re = rows(np.flatnonzero(~reached)), rows(np.flatnonzero(reached))
        assert np.array_equal(r["post"][un], c["X"][un]), "an unreached column changed"
        _close(r["post"][re], want[re], "reached columns")
        assert np.array_equal(r["stats"][:, 0], ref["stats"]["n_local"])
    _close(r["Yp"], ref["Yp"], "obs block (never relaxed)")


# ---- the chunk edges of the Gram: lists of exactly 31, 32, 33 and 65 obs for one column ------------------------------------------
@pytest.mark.parametrize("n", [31, 32, 33, 65])
def test_list_lengths_around_the_chunk_of_32(ctx, n):
    M = 17
    rng = np.random.default_rng(n)
    far = 7
    P = n + far
    lat = np.concatenate([40.0 + rng.uniform(-2.0, 2.0, n), np.full(far, -40.0)])
    lon = np.concatenate([260.0 + rng.uniform(-2.0, 2.0, n), np.full(far, 80.0)])
    perm = rng.permutation(P)
    c = lk.make_case(M, P, 1, 1, 1, seed=n)
    c.update(ob_lat=lat[perm], ob_lon=lon[perm], ob_hw=np.full(P, 800.0), assim=np.ones(P, dtype=bool))
    ym, Yp = ek.ob_priors(c["HX"])
    T, w, st = _probe(ctx, c, lat=np.array([40.0]), lon=np.array([260.0]))
    rT, rw, rst, _ = lk.weights([40.0], [260.0], ym, Yp, c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"])
    assert rst["n_local"][0] == n and st[0, 0] == n and rst["cond"][0] <= COND_CAP
    _close(T, rT, "T")
    _close(w, rw, "w")


# ---- no work ---------------------------------------------------------------------------------------------------------------------
def test_no_obs_and_all_unflagged_return_the_state_bit_for_bit(ctx):
    c = _case(17, 33, 5, 7, 3)
    empty = dict(c, P=0, HX=np.zeros((0, 17)), value=np.zeros(0), error=np.zeros(0), assim=np.zeros(0, dtype=bool),
                 ob_lat=np.zeros(0), ob_lon=np.zeros(0), ob_hw=np.zeros(0))
    for g in (empty, dict(c, assim=np.zeros(c["P"], dtype=bool))):
        for in_place in (False, True):
            r = _cycle(ctx, g, in_place=in_place)
            assert np.array_equal(r["post"], c["X"]) and not r["stats"].any()
            assert not np.asarray(r["diag"]["assimilated"]).any()
            assert np.array_equal(r["Yp"], r["Yp0"]) and np.array_equal(r["ym"], r["ym0"])


# ---- determinism, the entries against one another ----------------------------------------------------------------------------------
def test_same_bits_twice_in_place_and_without_the_obs_block(ctx):
    c = _case(40, 400, 6, 7, 3)
    a = _cycle(ctx, c)
    _same_bits(a, _cycle(ctx, c), "twice")
    _same_bits(a, _cycle(ctx, c, in_place=True), "in place")
    b = _cycle(ctx, c, obs_block_out=False)
    _same_bits(a, b, "obs_block_out 0", keys=("post", "stats"))
    assert np.array_equal(b["Yp"], b["Yp0"]) and np.array_equal(b["ym"], b["ym0"]), "obs_block_out 0 wrote the obs block"
    T1, w1, s1 = _probe(ctx, c)
    T2, w2, s2 = _probe(ctx, c)
    assert np.array_equal(T1, T2) and np.array_equal(w1, w2) and np.array_equal(s1, s2)


def test_partial_overlap_is_refused(ctx):
    from efa_xray_amd import _lib
    c = _case(17, 33, 5, 7, 3)
    N, M = c["X"].shape
    buf = ctx.empty((N + 1, M))
    ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
    with pytest.raises(_lib.EfaError) as e:
        ctx.letkf_cycle(N, M, c["P"], buf.ptr.value, buf.ptr.value + 8 * M, ym, Yp, c["value"], c["error"], c["assim"], c["ob_lat"],
                        c["ob_lon"], c["ob_hw"], c["grid_lat"], c["grid_lon"], c["n_lead"], f32=False)
    assert e.value.status == _lib.EFA_ERR_INVALID


# ---- obs that are not read, a NaN value, invalid variances ----------------------------------------------------------------------------
def test_unflagged_obs_are_never_read(ctx):
    c = _case(17, 33, 5, 7, 3)
    off = ~c["assim"]
    assert off.any()
    value, error, hw = c["value"].copy(), c["error"].copy(), c["ob_hw"].copy()
    value[off] = np.where(np.arange(off.sum()) % 2 == 0, np.nan, np.inf)
    error[off] = np.where(np.arange(off.sum()) % 2 == 0, -np.inf, np.nan)
    hw[off] = np.nan
    _same_bits(_cycle(ctx, c), _cycle(ctx, c, value=value, error=error, ob_hw=hw), "NaN / Inf in unflagged obs")


def test_a_nan_value_poisons_exactly_the_columns_it_reaches(ctx):
    c, ref, _ = _short()
    rho = ref["rho"]
    k = int(np.flatnonzero(c["assim"] & (rho != 0.0).any(axis=0))[0])
    hit = rho[:, k] != 0.0
    assert hit.any() and not hit.all()
    value = c["value"].copy()
    value[k] = np.nan
    a, b = _cycle(ctx, c), _cycle(ctx, c, value=value)
    rows = lambda cols: (np.asarray(cols)[None, :] + c["ncol"] * np.arange(c["n_lead"])[:, None]).reshape(-1)
    assert np.isnan(b["post"][rows(np.flatnonzero(hit))]).all()
    assert np.array_equal(b["post"][rows(np.flatnonzero(~hit))], a["post"][rows(np.flatnonzero(~hit))])
    assert np.array_equal(a["stats"], b["stats"], equal_nan=True)
    T0, w0, _ = _probe(ctx, c)
    T1, w1, _ = _probe(ctx, c, value=value)
    assert np.array_equal(T0, T1), "a NaN value reached T"
    assert np.isnan(w1[hit]).all() and np.array_equal(w1[~hit], w0[~hit])


@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
def test_an_invalid_error_variance_of_an_assimilated_ob_is_refused(ctx, bad):
    from efa_xray_amd import _lib
    c = _case(17, 33, 5, 7, 3)
    error = c["error"].copy()
    error[np.flatnonzero(c["assim"])[1]] = bad
    for call in (lambda: _cycle(ctx, c, error=error), lambda: _probe(ctx, c, error=error)):
        with pytest.raises(_lib.EfaError) as e:
            call()
        assert e.value.status == _lib.EFA_ERR_INVALID and "error variance" in str(e.value)


# ---- relaxation, the outlier check, float32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,alpha", [("rtpp", 0.5), ("rtps", 0.9)])
def test_relaxation_matches_the_closed_form_on_the_model_posterior(ctx, kind, alpha):
    from efa_xray_amd import _lib
    size = (40, 400, 6, 7, 3)
    c, ref = _case(*size), _model(*size)
    ctx.set_relaxation(_lib.RELAX_RTPP if kind == "rtpp" else _lib.RELAX_RTPS, alpha)
    want = relax(c["X"], ref["post"], **{kind: alpha})
    for in_place in (False, True):
        r = _cycle(ctx, c, in_place=in_place)
        _close(r["post"], want, "%s %s" % (kind, "in place" if in_place else "out of place"))
        _close(r["Yp"], ref["Yp"], "the obs block is not relaxed")
    T, w, _ = _probe(ctx, c)
    _close(T, ref["T"], "the probe's T is not relaxed")


def test_outlier_check_rejects_exactly_and_equals_cleared_flags(ctx):
    t = 3.0
    size = (17, 33, 5, 7, 3)
    c = _case(*size)
    ym, Yp = ek.ob_priors(c["HX"])
    value, bad = qc.inject(c["HX"], c["value"], c["error"], c["assim"], t, 3, seed=17)
    assert qc.clear_of_threshold(ym, Yp, value, c["error"], t)
    flags = qc.masked_flags(c["HX"], value, c["error"], c["assim"], t)
    assert not flags[bad].any() and flags.any()
    ctx.set_outlier_threshold(t)
    r = _cycle(ctx, c, value=value)
    ctx.set_outlier_threshold(None)
    assert np.array_equal(r["diag"]["assimilated"], flags), "rejected set"
    _same_bits(r, _cycle(ctx, c, value=value, assim=flags), "outlier check against cleared flags")
    ref = lk.letkf_cycle(c["X"], c["HX"], value, c["error"], flags, c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"], c["grid_lon"],
                         c["n_lead"])
    _check_against_model(r, ref, c, "outlier check")


@pytest.mark.parametrize("rtps", [None, 0.9])
def test_float32_rows_are_the_float64_result_rounded_once(ctx, rtps):
    from efa_xray_amd import _lib
    c = _case(40, 400, 6, 7, 3)
    if rtps:
        ctx.set_relaxation(_lib.RELAX_RTPS, rtps)
    X32 = c["X"].astype(np.float32)
    for in_place in (False, True):
        a = _cycle(ctx, c, X=X32, f32=True, in_place=in_place)
        b = _cycle(ctx, c, X=X32.astype(np.float64), in_place=in_place)
        assert a["post"].dtype == np.float32 and np.array_equal(a["post"], b["post"].astype(np.float32))
        _same_bits(a, b, "float32 against float64", keys=("ym", "Yp", "stats"))


# ---- the unlocalised limit: the batch solver of efa_ensrf_cycle_dev ----------------------------------------------------------------
def test_very_wide_tapers_agree_with_the_batch_solver(ctx):
    size = (40, 400, 6, 7, 3)
    c = _case(*size)
    r = _cycle(ctx, c, ob_hw=np.full(c["P"], 1e12))
    ctx.set_option("obs_solver", 1)
    N, M = c["X"].shape
    Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
    post = ctx.empty((N, M))
    ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
    diag = ctx.ensrf_cycle(N, M, c["P"], Xd, post, ym, Yp, c["value"], c["error"], c["assim"], obs_block_out=True)
    ctx.set_option("obs_solver", 0)
    _close(r["post"], post.download(), "posterior members")
    _close(r["Yp"], Yp.download(), "obs block")
    _close(r["ym"], ym.download(), "obs means")
    a = c["assim"]
    _close(np.asarray(r["diag"]["post_mean"])[a], np.asarray(diag["post_mean"])[a], "post_mean")
    _close(np.asarray(r["diag"]["post_var"])[a], np.asarray(diag["post_var"])[a], "post_var")
    assert np.all(r["stats"][:, 0] == a.sum())


# ---- the refusals, and the context afterwards ----------------------------------------------------------------------------------------
def test_refused_settings_leave_the_context_usable(ctx):
    from efa_xray_amd import _lib
    size = (17, 33, 5, 7, 3)
    c = _case(*size)
    N, P, n_lead = c["X"].shape[0], c["P"], c["n_lead"]
    fresh = _lib.Context(0)
    try:
        want = _cycle(fresh, c)
    finally:
        fresh.close()
    field = ctx.to_device(np.tile([1.0, 0.6], (N, 1)))
    settings = [
        ("adaptive-inflation", lambda: ctx.set_adaptive_inflation(field, N)),
        ("vertical", lambda: ctx.set_vertical_localization(np.arange(n_lead, dtype=float), np.zeros(P), np.ones(P))),
        ("slab", lambda: ctx.set_slab_localization(n_lead, P, lead_time=np.arange(n_lead, dtype=float), ob_time=np.zeros(P),
                                                   ob_time_halfwidth=np.full(P, 6.0))),
        ("sampling-error-correction", lambda: ctx.set_sampling_error_correction(np.linspace(0.0, 1.0, 16))),
    ]
    for word, setup in settings:
        _reset(ctx)
        setup()
        for call in (lambda: _cycle(ctx, c), lambda: _probe(ctx, c)):
            with pytest.raises(_lib.EfaError) as e:
                call()
            assert e.value.status == _lib.EFA_ERR_INVALID and word in str(e.value), str(e.value)
        _reset(ctx)
        _same_bits(_cycle(ctx, c), want, "after the refused %s setting" % word)
    # "obs_solver" is not read by the new calls
    ctx.set_option("obs_solver", 1)
    _same_bits(_cycle(ctx, c), want, "obs_solver 1")


def test_ensrf_gc_is_unchanged_by_a_letkf_cycle_before_it(ctx):
    from efa_xray_amd import _lib
    c = _case(17, 33, 5, 7, 3)

    def serial():
        N, M = c["X"].shape
        Xd = ctx.to_device(np.ascontiguousarray(c["X"]))
        ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
        ctx.ensrf_cycle(N, M, c["P"], Xd, Xd, ym, Yp, c["value"], c["error"], c["assim"], _lib.LOC_GC, c["ob_lat"], c["ob_lon"], c["ob_hw"],
                        c["grid_lat"], c["grid_lon"], c["n_lead"])
        return Xd.download()

    before = serial()
    _cycle(ctx, c)
    assert np.array_equal(serial(), before)
    assert ctx.get_option("phase_a_kind") != 6


# ---- the Python class ----------------------------------------------------------------------------------------------------------------
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
                   lat=float(lat.reshape(-1)[col]), lon=float(lon.reshape(-1)[col]), assimilate_this=(k % 7 != 3),
                   localize_radius=float(rng.uniform(400.0, 1500.0)))
        ob.row = int(rows[k])
        obs.append(ob)
    return state, obs, lat, lon


def _ob_diag(obs):
    d = {k: np.array([np.nan if getattr(o, k, None) is None else getattr(o, k) for o in obs], float)
         for k in ("prior_mean", "prior_var", "post_mean", "post_var")}
    d["assimilated"] = np.array([bool(o.assimilated) for o in obs])
    return d


def test_letkf_class_against_the_model(ctx):
    from efa_xray_amd import LETKF
    state, obs, lat, lon = _api_case()
    f = LETKF(state, obs, verbose=False)
    HX = np.asarray(f.compute_ob_estimates(), dtype=np.float64)
    args = (np.array([o.value for o in obs]), np.array([o.error for o in obs]), np.array([o.assimilate_this for o in obs]),
            np.array([o.lat for o in obs]), np.array([o.lon for o in obs]), np.array([o.localize_radius for o in obs]), lat, lon, 4)
    ref = lk.letkf_cycle(state.to_vect(), HX, *args)
    assert ref["stats"]["cond"].max() <= COND_CAP
    post, obs_out = f.update()
    assert obs_out is obs and post is not state
    _close(post.to_vect(), ref["post"], "LETKF.update posterior")
    _check_diag(_ob_diag(obs), ref["diag"], "LETKF.update")
    ls = f.last_solve
    assert sorted(ls) == ["dfs", "n_local", "sweeps"] and all(ls[k].shape == (6, 7) for k in ls)
    assert np.array_equal(ls["n_local"].reshape(-1), ref["stats"]["n_local"])
    _close(ls["dfs"].reshape(-1), ref["stats"]["dfs"], "last_solve dfs")
    assert ls["sweeps"].max() < SWEEP_CAP and np.array_equal(ls["sweeps"] == 0, ls["n_local"] == 0)
    # a float32 state: the float64 update of the widened state, rounded once
    s32, o32, _, _ = _api_case(dtype=np.float32)
    p32, _ = LETKF(s32, o32, verbose=False).update()
    assert p32.to_vect().dtype == np.float32
    s64, o64, _, _ = _api_case(dtype=np.float32)
    p64, _ = LETKF(s64.astype(np.float64), o64, verbose=False).update()
    assert np.array_equal(p32.to_vect(), p64.to_vect().astype(np.float32))
    # rtps through the same kernel
    s3, o3, _, _ = _api_case()
    p3, _ = LETKF(s3, o3, verbose=False, rtps=0.9).update()
    _close(p3.to_vect(), relax(state.to_vect(), ref["post"], rtps=0.9), "LETKF rtps")
