"""LETKF weight interpolation on the MI355X against the NumPy model of tests/_letkf_interp.py:
efa_letkf_cycle_interp_dev / _f32_dev (the solve at the nodes of a coarse mesh, the pairs interpolated to every column) and
efa_letkf_interp_apply_dev (the interpolate-and-apply kernel alone, on node pairs no solve would give).  The posterior members and
the node pairs to 1e-10 of the largest magnitude of each array (7y's float64 bound, claimed up to cond(A) <= 1e4: asserted from the
model at the nodes); the obs block, the diagnostics and everything the definition calls "bit for bit" with array_equal.  Every test
restores the shared context's settings."""
import functools

import numpy as np
import pytest

import _etkf as ek
import _letkf as lk
import _letkf_interp as li
import _outlier as qc
from _letkf_gpu import TOL, COND_CAP, _reset, _obs_block, _close, _same_bits
from test_relaxation_host import relax

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# (M, P, ny, nx, n_lead, stride): M below, at and just over a 16-tile and at the cap; ragged last cells; an n_lead that crosses a
# 16-row tile; a single-node axis; a stride beyond the grid; a unit stride on one axis
CASES = [(2, 1, 3, 5, 1, (2, 2)), (3, 5, 4, 6, 2, (3, 4)), (16, 64, 5, 7, 3, (2, 3)), (17, 33, 5, 7, 17, (4, 2)),
         (40, 400, 9, 10, 3, (4, 4)), (80, 300, 5, 6, 2, (2, 5)), (136, 300, 3, 6, 1, (2, 3)), (16, 64, 1, 7, 2, (3, 3)),
         (16, 64, 5, 7, 2, (8, 8)), (16, 64, 5, 7, 2, (1, 3))]
F32_CASE = (17, 33, 5, 7, 17, (4, 2))


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
    """The seeded case of tests/_letkf.py, computed once and left unchanged."""
    return _freeze(lk.make_case(M, P, ny, nx, n_lead, seed=seed, hw=hw))


def _run_model(c, stride, **over):
    g = dict(c, **over)
    return li.interp_cycle(g["X"], g["HX"], g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"], g["grid_lat"],
                           g["grid_lon"], g["n_lead"], (g["ny"], g["nx"]), stride)


@functools.lru_cache(maxsize=None)
def _model(M, P, ny, nx, n_lead, stride, seed=0, hw=(300.0, 3000.0)):
    return _run_model(_case(M, P, ny, nx, n_lead, seed, hw), stride)


def _nnodes(ny, nx, stride):
    return li.axis_nodes(ny, stride[0]).size * li.axis_nodes(nx, stride[1]).size


def _cycle(ctx, c, stride=None, in_place=False, f32=False, X=None, shape=None, **over):
    """efa_letkf_cycle_interp_dev (stride given) or efa_letkf_cycle_dev (None): posterior, obs block, diagnostics, statistics (of
    the nodes, or of the columns)."""
    g = dict(c, **over)
    X = g["X"] if X is None else X
    N, M = X.shape
    P = g["P"]
    dt = np.float32 if f32 else np.float64
    Xd = ctx.to_device(np.ascontiguousarray(X, dtype=dt), dtype=dt)
    post = Xd if in_place else ctx.empty((N, M), dtype=dt)
    ym, Yp, _, _ = _obs_block(ctx, g["HX"], M)
    kw = {}
    nst = g["ncol"]
    if stride is not None:
        kw = dict(shape=(g["ny"], g["nx"]) if shape is None else shape, stride=stride)
        nst = _nnodes(g["ny"], g["nx"], stride) if min(stride) >= 1 else 1
    stats = ctx.empty((nst, 3))
    diag = ctx.letkf_cycle(N, M, P, Xd, post, ym, Yp, g["value"], g["error"], g["assim"], g["ob_lat"], g["ob_lon"], g["ob_hw"],
                           g["grid_lat"], g["grid_lon"], g["n_lead"], obs_block_out=True, col_stats=stats, f32=f32, **kw)
    return dict(post=post.download(), ym=ym.download()[:P], Yp=Yp.download()[:P], diag=diag, stats=stats.download())


def _rows(c, cols):
    return (np.asarray(cols, dtype=np.int64)[None, :] + c["ncol"] * np.arange(c["n_lead"])[:, None]).reshape(-1)


def _check_against_model(r, ref, what):
    st = ref["node_stats"]
    print("%s: cond(A) max %.3g at the nodes, n_local %d..%d" % (what, st["cond"].max(), st["n_local"].min(), st["n_local"].max()))
    assert st["cond"].max() <= COND_CAP, "cond(A) = %g: the float64 bound of 1e-10 is claimed up to 1e4" % st["cond"].max()
    _close(r["post"], ref["post"], what + " posterior members")
    assert np.array_equal(r["stats"][:, 0], st["n_local"].astype(np.float64)), what + ": n_local of the nodes"
    assert np.abs(r["stats"][:, 1] - st["dfs"]).max() <= TOL * max(1.0, st["dfs"].max()), what + ": dfs of the nodes"


# ---- 1. the cycle against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,ny,nx,n_lead,stride", CASES)
def test_cycle_matches_the_model(ctx, M, P, ny, nx, n_lead, stride):
    c, ref = _case(M, P, ny, nx, n_lead), _model(M, P, ny, nx, n_lead, stride)
    r = _cycle(ctx, c, stride)
    assert ctx.get_option("phase_a_kind") == 7
    assert ctx.last_timing()["state_launches"] == 2
    _check_against_model(r, ref, "M=%d P=%d %dx%d stride %s" % (M, P, ny, nx, stride))
    # the node pairs, read back through the entry the cycle solves them with
    m = ref["mesh"]
    ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
    T, w, st = ctx.letkf_weights(M, P, ym, Yp, c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"],
                                 c["grid_lat"].reshape(-1)[m["node_col"]], c["grid_lon"].reshape(-1)[m["node_col"]])
    _close(T, ref["Tn"], "node T")
    _close(w, ref["wn"], "node w")
    assert np.array_equal(st, r["stats"]), "the node statistics are those of efa_letkf_weights_dev at the nodes"
    # the obs block and the diagnostics: the plain call's, bit for bit
    _same_bits(r, _cycle(ctx, c), "obs block and diagnostics against efa_letkf_cycle_dev", keys=("ym", "Yp"))


# ---- 2. the apply alone, on pairs no solve would give ---------------------------------------------------------------------------------
def _seeded_pairs(M, nn, seed):
    rng = np.random.default_rng(seed)
    Tw = rng.uniform(-1.0, 1.0, (nn, M, M + 1))       # T_n NOT symmetric: a transposed index cannot hide
    assert not np.allclose(Tw[:, :, :M], np.swapaxes(Tw[:, :, :M], 1, 2))
    return Tw


def _apply(ctx, X, shape, stride, n_lead, Tw, stats=None, in_place=False, f32=False):
    N, M = X.shape
    dt = np.float32 if f32 else np.float64
    Xd = ctx.to_device(np.ascontiguousarray(X, dtype=dt), dtype=dt)
    post = Xd if in_place else ctx.empty((N, M), dtype=dt)
    ctx.letkf_interp_apply(N, M, Xd, post, shape, stride, n_lead, ctx.to_device(np.ascontiguousarray(Tw)),
                           None if stats is None else ctx.to_device(np.ascontiguousarray(stats, dtype=np.float64)), f32=f32)
    return post.download()


def _apply_model(X, m, n_lead, Tw):
    """Plain float64 sums, and the forward bound of the dot products: 2 (4M + 8) 2^-53 sum_n beta_n sum_j |x'_j| |T_n[j,i]|, plus
    the same for the mean term.  (Length: a dot product of M terms of a T_c that is itself a sum of four products.)"""
    M = X.shape[1]
    ncol = m["ny"] * m["nx"]
    Tn, wn = Tw[:, :, :M], Tw[:, :, M]
    Tc, wc, _ = li.column_pairs(m, Tn, wn)
    post, bound = np.empty_like(X), np.empty_like(X)
    for c in range(ncol):
        rows = c + ncol * np.arange(n_lead)
        xm = X[rows].mean(axis=1)
        xp = X[rows] - xm[:, None]
        post[rows] = (xm + xp @ wc[c])[:, None] + xp @ Tc[c]
        aT = sum(m["beta"][c, n] * np.abs(Tn[m["corner"][c, n]]) for n in range(4) if m["beta"][c, n] != 0.0)
        aw = sum(m["beta"][c, n] * np.abs(wn[m["corner"][c, n]]) for n in range(4) if m["beta"][c, n] != 0.0)
        bound[rows] = 2.0 * (4 * M + 8) * U * (np.abs(xp) @ aT + (np.abs(xp) @ aw)[:, None])
    return post, bound


@pytest.mark.parametrize("n_lead", [1, 17])
@pytest.mark.parametrize("M", [3, 17, 40, 136])
def test_apply_on_seeded_nonsymmetric_pairs_within_the_dot_product_bound(ctx, M, n_lead):
    ny, nx, stride = 4, 6, (3, 4)
    m = li.mesh(ny, nx, stride)
    X = lk.make_case(M, 4, ny, nx, n_lead, seed=7)["X"]
    Tw = _seeded_pairs(M, m["node_col"].size, 1000 + M)
    want, bound = _apply_model(X, m, n_lead, Tw)
    for in_place in (False, True):
        got = _apply(ctx, X, (ny, nx), stride, n_lead, Tw, in_place=in_place)
        ratio = np.abs(got - want) / bound
        print("M=%d n_lead=%d in_place=%d: max |err| / bound = %.3g" % (M, n_lead, in_place, ratio.max()))
        assert np.all(np.isfinite(got)) and ratio.max() <= 1.0


# ---- 3. node columns and node lines read their own nodes only ---------------------------------------------------------------------
@pytest.mark.parametrize("iy,ix,nused", [(3, 4, 1), (0, 0, 1), (3, 2, 2), (1, 4, 2), (1, 5, 2), (2, 3, 4)])
def test_corners_of_weight_zero_are_not_read(ctx, iy, ix, nused):
    M, ny, nx, stride, n_lead = 17, 4, 6, (3, 4), 2
    m = li.mesh(ny, nx, stride)
    X = lk.make_case(M, 4, ny, nx, n_lead, seed=7)["X"]
    Tw = _seeded_pairs(M, m["node_col"].size, 1000 + M)
    want, bound = _apply_model(X, m, n_lead, Tw)
    col = iy * nx + ix
    used = m["corner"][col][m["beta"][col] != 0.0]
    assert used.size == nused
    poisoned = Tw.copy()
    poisoned[np.setdiff1d(np.arange(Tw.shape[0]), used)] = np.nan
    got = _apply(ctx, X, (ny, nx), stride, n_lead, poisoned)
    rows = col + ny * nx * np.arange(n_lead)
    assert np.all(np.isfinite(got[rows])), "a corner of weight 0 was read"
    assert np.all(np.abs(got[rows] - want[rows]) <= bound[rows])
    if nused < 4:
        assert np.isnan(got).any(), "the poison reaches the columns that do use those nodes"


# ---- 4. unreached columns ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corner_case():
    """9 x 10 columns (about 417 km x 570 km apart), obs of 300 km half-width (600 km of reach) clustered at the grid's first corner,
    and one ob of 100 km half-width on column (6, 6), the middle of the cell [4, 8] x [4, 8]."""
    c = dict(lk.make_case(16, 13, 9, 10, 2, seed=5))
    rng = np.random.default_rng(5)
    lat0, lon0 = c["grid_lat"][0, 0], c["grid_lon"][0, 0]
    c["ob_lat"] = np.append(lat0 + rng.uniform(-1.0, 1.0, 12), c["grid_lat"][6, 6])
    c["ob_lon"] = np.append(lon0 + rng.uniform(-1.0, 1.0, 12), c["grid_lon"][6, 6])
    c["ob_hw"] = np.append(np.full(12, 300.0), 100.0)
    c["assim"] = np.ones(13, dtype=bool)
    return _freeze(c)


@pytest.mark.parametrize("rtps", [None, 0.9])
def test_unreached_columns_keep_their_bits_and_a_short_ob_between_nodes_is_lost(ctx, rtps):
    from efa_xray_amd import _lib
    c = _corner_case()
    stride = (4, 4)
    ref = _run_model(c, stride)
    reached = ref["reached"]
    changed = np.any(ref["post"] != c["X"], axis=1).reshape(c["n_lead"], c["ncol"]).any(axis=0)
    assert (~reached).any() and reached.any() and changed[reached].all() and not changed[~reached].any()
    mid = 6 * c["nx"] + 6
    plain_reached = ref["stats"]["n_local"] > 0
    assert plain_reached[mid] and not reached[mid], "the short ob reaches its column, and none of the column's nodes"
    if rtps:
        ctx.set_relaxation(_lib.RELAX_RTPS, rtps)
    want = ref["post"] if not rtps else relax(c["X"], ref["post"], rtps=rtps)
    for in_place in (False, True):
        r = _cycle(ctx, c, stride, in_place=in_place)
        un, re = _rows(c, np.flatnonzero(~reached)), _rows(c, np.flatnonzero(reached))
        assert np.array_equal(r["post"][un], c["X"][un]), "an unreached column changed"
        _close(r["post"][re], want[re], "reached columns")
        assert np.all(np.any(r["post"][re] != c["X"][re], axis=1)), "a reached column's row did not change"
    p = _cycle(ctx, c)
    mrows = _rows(c, [mid])
    assert np.all(np.any(p["post"][mrows] != c["X"][mrows], axis=1)), "the plain LETKF updates the column under the short ob"
    assert np.array_equal(r["post"][mrows], c["X"][mrows]), "... and the interpolated one leaves it: the documented loss"


# ---- 5. a NaN value -----------------------------------------------------------------------------------------------------------------
def test_a_nan_value_poisons_exactly_the_columns_that_use_a_node_it_reaches(ctx):
    size, stride = (16, 40, 6, 7, 3), (2, 3)
    c = _case(*size, hw=(100.0, 400.0))
    ref = _model(*size, stride, hw=(100.0, 400.0))
    m, rho = ref["mesh"], ref["node_rho"]
    some = c["assim"] & (rho != 0.0).any(axis=0) & ~(rho != 0.0).all(axis=0)
    k = int(np.flatnonzero(some)[0])
    node_hit = np.append(rho[:, k] != 0.0, False)            # (corner -1: no such node)
    hit = ((m["beta"] != 0.0) & node_hit[m["corner"]]).any(axis=1)
    assert hit.any() and not hit.all()
    value, zero = c["value"].copy(), c["value"].copy()
    value[k], zero[k] = np.nan, 0.0
    a, b = _cycle(ctx, c, stride, value=zero), _cycle(ctx, c, stride, value=value)
    assert np.isnan(b["post"][_rows(c, np.flatnonzero(hit))]).all()
    clear = _rows(c, np.flatnonzero(~hit))
    assert np.array_equal(b["post"][clear], a["post"][clear])
    assert np.array_equal(a["stats"], b["stats"])


# ---- 6. reproducibility, in place, overlap --------------------------------------------------------------------------------------------
def test_same_bits_twice_and_in_place_and_a_partial_overlap_is_refused(ctx):
    from efa_xray_amd import _lib
    size, stride = (40, 400, 9, 10, 3), (4, 4)
    c = _case(*size)
    a = _cycle(ctx, c, stride)
    _same_bits(a, _cycle(ctx, c, stride), "twice")
    _same_bits(a, _cycle(ctx, c, stride, in_place=True), "in place")
    N, M = c["X"].shape
    buf = ctx.empty((N + 1, M))
    ym, Yp, _, _ = _obs_block(ctx, c["HX"], M)
    with pytest.raises(_lib.EfaError) as e:
        ctx.letkf_cycle(N, M, c["P"], buf.ptr.value, buf.ptr.value + 8 * M, ym, Yp, c["value"], c["error"], c["assim"], c["ob_lat"],
                        c["ob_lon"], c["ob_hw"], c["grid_lat"], c["grid_lon"], c["n_lead"], f32=False, shape=(9, 10), stride=stride)
    assert e.value.status == _lib.EFA_ERR_INVALID and "overlap" in str(e.value)
    Tw = ctx.to_device(np.zeros((_nnodes(9, 10, stride), M, M + 1)))
    with pytest.raises(_lib.EfaError) as e:
        ctx.letkf_interp_apply(N, M, buf.ptr.value, buf.ptr.value + 8 * M, (9, 10), stride, c["n_lead"], Tw, f32=False)
    assert e.value.status == _lib.EFA_ERR_INVALID and "overlap" in str(e.value)
    _same_bits(a, _cycle(ctx, c, stride), "after the refusals")


# ---- 7. float32 rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rtps", [None, 0.9])
def test_float32_rows_are_the_float64_result_rounded_once(ctx, rtps):
    from efa_xray_amd import _lib
    M, P, ny, nx, n_lead, stride = F32_CASE
    c = _case(M, P, ny, nx, n_lead)
    if rtps:
        ctx.set_relaxation(_lib.RELAX_RTPS, rtps)
    X32 = c["X"].astype(np.float32)
    for in_place in (False, True):
        a = _cycle(ctx, c, stride, X=X32, f32=True, in_place=in_place)
        b = _cycle(ctx, c, stride, X=X32.astype(np.float64), in_place=in_place)
        assert a["post"].dtype == np.float32 and np.array_equal(a["post"], b["post"].astype(np.float32))
        assert np.any(a["post"] != X32)
        _same_bits(a, b, "float32 against float64", keys=("ym", "Yp", "stats"))


# ---- 8. relaxation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,alpha", [("rtpp", 0.5), ("rtps", 0.9)])
def test_relaxation_matches_the_closed_form_on_the_interpolated_posterior(ctx, kind, alpha):
    from efa_xray_amd import _lib
    size, stride = (40, 400, 9, 10, 3), (4, 4)
    c, ref = _case(*size), _model(*size, stride)
    ctx.set_relaxation(_lib.RELAX_RTPP if kind == "rtpp" else _lib.RELAX_RTPS, alpha)
    want = relax(c["X"], ref["post"], **{kind: alpha})
    assert np.abs(want - ref["post"]).max() > 1e-3
    for in_place in (False, True):
        r = _cycle(ctx, c, stride, in_place=in_place)
        _close(r["post"], want, "%s %s" % (kind, "in place" if in_place else "out of place"))
        _close(r["Yp"], ref["Yp"], "the obs block is not relaxed")
    if kind == "rtpp":      # the closed form of the definition as well: (1 - alpha) T_c + alpha I, after the interpolation
        m = ref["mesh"]
        Tc, wc, reached = li.column_pairs(m, ref["Tn"], ref["wn"], ref["node_stats"]["n_local"])
        _close(r["post"], li.apply_pairs(c["X"], c["ncol"], c["n_lead"], Tc, wc, reached, rtpp=alpha), "RTPP on T_c")


# ---- 9. the outlier check -------------------------------------------------------------------------------------------------------------
def test_outlier_check_equals_cleared_flags(ctx):
    t = 3.0
    size, stride = (17, 33, 5, 7, 3), (2, 3)
    c = _case(*size)
    ym, Yp = ek.ob_priors(c["HX"])
    value, bad = qc.inject(c["HX"], c["value"], c["error"], c["assim"], t, 3, seed=17)
    assert qc.clear_of_threshold(ym, Yp, value, c["error"], t)
    flags = qc.masked_flags(c["HX"], value, c["error"], c["assim"], t)
    assert not flags[bad].any() and flags.any()
    ctx.set_outlier_threshold(t)
    r = _cycle(ctx, c, stride, value=value)
    ctx.set_outlier_threshold(None)
    assert np.array_equal(r["diag"]["assimilated"], flags), "rejected set"
    _same_bits(r, _cycle(ctx, c, stride, value=value, assim=flags), "outlier check against cleared flags")
    _check_against_model(r, _run_model(c, stride, value=value, assim=flags), "outlier check")


# ---- 10. a unit stride is the plain call ------------------------------------------------------------------------------------------------
def test_unit_stride_through_the_new_entry_is_the_plain_call_bit_for_bit(ctx):
    from efa_xray_amd import _lib
    c = _case(17, 33, 5, 7, 3)
    want = _cycle(ctx, c)
    _same_bits(_cycle(ctx, c, (1, 1)), want, "stride (1, 1)")
    assert ctx.get_option("phase_a_kind") == 6
    _same_bits(_cycle(ctx, c, (1, 1), in_place=True), want, "stride (1, 1), in place")
    ctx.set_relaxation(_lib.RELAX_RTPS, 0.9)
    X32 = c["X"].astype(np.float32)
    _same_bits(_cycle(ctx, c, (1, 1), X=X32, f32=True), _cycle(ctx, c, X=X32, f32=True), "stride (1, 1), float32, rtps")


# ---- 11. the refusals, and the context afterwards -----------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(ctx):
    from efa_xray_amd import _lib
    size, stride = (17, 33, 5, 7, 3), (2, 3)
    c, ref = _case(*size), _model(*size, stride)
    N, P, n_lead, M = c["X"].shape[0], c["P"], c["n_lead"], c["M"]
    want = _cycle(ctx, c, stride)
    _check_against_model(want, ref, "before any refusal")
    Tw = np.zeros((_nnodes(5, 7, stride), M, M + 1))
    big = lk.make_case(137, 20, 5, 7, 1)
    field = ctx.to_device(np.tile([1.0, 0.6], (N, 1)))
    calls = [
        ("stride", lambda: _cycle(ctx, c, (0, 3))),
        ("stride", lambda: _cycle(ctx, c, (2, -1))),
        ("stride", lambda: _apply(ctx, c["X"], (5, 7), (2, 0), n_lead, Tw)),
        ("rows", lambda: _cycle(ctx, c, stride, shape=(5, 8))),
        ("rows", lambda: _cycle(ctx, c, stride, shape=(7, 6))),
        ("rows", lambda: _apply(ctx, c["X"], (6, 7), stride, n_lead, np.zeros((_nnodes(6, 7, stride), M, M + 1)))),
        ("136", lambda: _cycle(ctx, big, stride)),
        ("136", lambda: _apply(ctx, big["X"], (5, 7), stride, 1, np.zeros((_nnodes(5, 7, stride), 137, 138)))),
    ]
    for word, call in calls:
        with pytest.raises(_lib.EfaError) as e:
            call()
        assert e.value.status == _lib.EFA_ERR_INVALID and word in str(e.value), str(e.value)
        _same_bits(_cycle(ctx, c, stride), want, "after a refused call (%s)" % word)
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
        for call in (lambda: _cycle(ctx, c, stride), lambda: _apply(ctx, c["X"], (5, 7), stride, n_lead, Tw)):
            with pytest.raises(_lib.EfaError) as e:
                call()
            assert e.value.status == _lib.EFA_ERR_INVALID and word in str(e.value), str(e.value)
        _reset(ctx)
        _same_bits(_cycle(ctx, c, stride), want, "after the refused %s setting" % word)
    for bad, word in ((0.0, "error variance"), (np.nan, "error variance")):
        error = c["error"].copy()
        error[np.flatnonzero(c["assim"])[1]] = bad
        with pytest.raises(_lib.EfaError) as e:
            _cycle(ctx, c, stride, error=error)
        assert e.value.status == _lib.EFA_ERR_INVALID and word in str(e.value)
    hw = c["ob_hw"].copy()
    hw[np.flatnonzero(c["assim"])[0]] = 0.0
    with pytest.raises(_lib.EfaError) as e:
        _cycle(ctx, c, stride, ob_hw=hw)
    assert e.value.status == _lib.EFA_ERR_INVALID
    _same_bits(_cycle(ctx, c, stride), want, "after the refused obs")


def test_ensrf_gc_is_unchanged_by_an_interpolated_cycle_before_it(ctx):
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
    _cycle(ctx, c, (2, 3))
    assert ctx.get_option("phase_a_kind") == 7
    assert np.array_equal(serial(), before)
    assert ctx.get_option("phase_a_kind") not in (6, 7)


# ---- 12. the Python class ---------------------------------------------------------------------------------------------------------------
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


def test_letkf_class_with_a_weight_stride_against_the_model(ctx):
    from efa_xray_amd import LETKF
    stride = (2, 3)
    state, obs, lat, lon = _api_case()
    f = LETKF(state, obs, verbose=False, weight_stride=stride)
    HX = np.asarray(f.compute_ob_estimates(), dtype=np.float64)
    ref = li.interp_cycle(state.to_vect(), HX, np.array([o.value for o in obs]), np.array([o.error for o in obs]),
                          np.array([o.assimilate_this for o in obs]), np.array([o.lat for o in obs]), np.array([o.lon for o in obs]),
                          np.array([o.localize_radius for o in obs]), lat, lon, 4, (6, 7), stride)
    st, m = ref["node_stats"], ref["mesh"]
    assert st["cond"].max() <= COND_CAP
    post, obs_out = f.update()
    assert obs_out is obs and post is not state
    _close(post.to_vect(), ref["post"], "LETKF.update posterior")
    a = np.asarray(ref["diag"]["assimilated"], bool)
    assert np.array_equal(np.array([bool(o.assimilated) for o in obs]), a)
    _close(np.array([o.post_mean for o in obs], dtype=np.float64)[a], ref["diag"]["post_mean"][a], "post_mean")
    ls = f.last_solve
    assert sorted(ls) == ["dfs", "n_local", "node_x", "node_y", "sweeps"]
    shape = (m["node_y"].size, m["node_x"].size)
    assert shape == (4, 3) and all(ls[k].shape == shape for k in ("dfs", "n_local", "sweeps"))
    assert np.array_equal(ls["node_y"], m["node_y"]) and np.array_equal(ls["node_x"], m["node_x"])
    assert np.array_equal(ls["n_local"].reshape(-1), st["n_local"])
    _close(ls["dfs"].reshape(-1), st["dfs"], "last_solve dfs")
    assert np.array_equal(ls["sweeps"] == 0, ls["n_local"] == 0)
    # rtps and a float32 state through the same kernel
    s3, o3, _, _ = _api_case()
    p3, _ = LETKF(s3, o3, verbose=False, rtps=0.9, weight_stride=stride).update()
    _close(p3.to_vect(), relax(state.to_vect(), ref["post"], rtps=0.9), "LETKF rtps")
    s32, o32, _, _ = _api_case(dtype=np.float32)
    p32, _ = LETKF(s32, o32, verbose=False, weight_stride=stride).update()
    s64, o64, _, _ = _api_case(dtype=np.float32)
    p64, _ = LETKF(s64.astype(np.float64), o64, verbose=False, weight_stride=stride).update()
    assert p32.to_vect().dtype == np.float32 and np.array_equal(p32.to_vect(), p64.to_vect().astype(np.float32))
    # a unit stride: today's result, bit for bit, and today's last_solve
    s1, o1, _, _ = _api_case()
    s0, o0, _, _ = _api_case()
    f1, f0 = LETKF(s1, o1, verbose=False, weight_stride=1), LETKF(s0, o0, verbose=False)
    p1, p0 = f1.update()[0], f0.update()[0]
    assert np.array_equal(p1.to_vect(), p0.to_vect())
    assert sorted(f1.last_solve) == ["dfs", "n_local", "sweeps"] and f1.last_solve["dfs"].shape == (6, 7)
    assert all(np.array_equal(f1.last_solve[k], f0.last_solve[k]) for k in f0.last_solve)
