"""GPU tests of row independence.  The rows of the state are independent given the obs-space trajectory;
sharding, streaming, the float32 route and the transform rest on that, and an error scaled by the array's maximum cannot see
most violations.  Three relations, on every route of tests/test_gpu_state_routes.py:

  1. update(D X) == D update(X), bit for bit, for D = diag(2^k_i): every operation on a row is linear in the row or
     homogeneous of degree 0, and a power of two changes no mantissa.  No tolerance, no reference.
  2. State rows of NaN, +Inf, zeros or one constant change no other row's bits, the diagnostics or the obs block: the reads past
     what a lane owns (clamped tile loads, zero-padded MFMA K slots, obs applied with a zero taper) must be dropped, not
     multiplied by zero.  The obs block stays the clean state's; nothing non-finite goes near Phase A (that is
     tests/test_gpu_obsprops.py, DESIGN.md 7n: NaN and Inf in the obs' values, errors and rows, through every Phase-A kernel).
  3. With obs and state rows of scales 1e-6..1e6 side by side every row and every ob agrees with the oracle to 1e-10 of ITS OWN
     scale (the generators keep the oracle's own error below 1e-12: tests/test_rowprops_host.py), and scaling ob k's
     (HX, value, error) by (2^j, 2^j, 4^j) leaves the state posterior's bits and scales the diagnostics exactly.

Worst err/tol of relation 3 seen on the MI355X: 4.6e-5 on the augmented arrays and diagnostics, 1.6e-3 on the member form's obs
perturbations (DESIGN.md 7l has the table); relations 1, 2 and 3b hold on every route."""
import itertools
from copy import deepcopy

import numpy as np
import pytest

import _rowprops as rp
from _rowprops import F32, F64
from test_gpu_state_routes import (ASSIM, ENTRIES, LOCS, N_LEAD, NCOL, NX, NY, P, PATHS, RELAX, ROWS, _ctx, _lib, _run,
                                   _settings, expected)

pytestmark = pytest.mark.gpu

_CLEAN = {}


def _problem(M):
    if ("pb", M) not in _CLEAN:
        _CLEAN["pb", M] = rp.RowProblem(M)
    return _CLEAN["pb", M]


def _options():
    L = _lib()
    path_opt = {"auto": L.PATH_AUTO, "transform": L.PATH_TRANSFORM, "sweep": L.PATH_SWEEP}
    relax_opt = {"none": (L.RELAX_NONE, 0.0), "rtpp": (L.RELAX_RTPP, 0.5), "rtps": (L.RELAX_RTPS, 0.5)}
    return path_opt, relax_opt


def _all_routes(pb, loc):
    """Every (path, relaxation, entry) of the problem, the float64 member form also in place; asserts the route of each run
    against `expected` and returns {(path, relax, entry): (posterior, diagnostics, obs block)}."""
    path_opt, relax_opt = _options()
    M, gc, out = pb.M, loc != "none", {}
    for path, relax in itertools.product(PATHS, RELAX):
        with _settings(path=path_opt[path], relax=relax_opt[relax], gc_onepass=0 if loc == "gc_batches" else 1):
            for e in ENTRIES + ["in_place"]:
                entry = "state_cycle" if e == "in_place" else e
                post, diag, obs_block, got_path, got_launches, got_native = _run(pb, gc, entry, in_place=(e == "in_place"))
                want_path, want_launches, want_native = expected(M, loc, path, relax, entry)
                w = "M=%d loc=%s path=%s relax=%s entry=%s" % (M, loc, path, relax, e)
                assert got_path == path_opt[want_path], w + ": another path"
                assert got_launches == want_launches, "%s: %d launches, expected %d" % (w, got_launches, want_launches)
                assert got_native == want_native, "%s: f32_native %r, expected %r" % (w, got_native, want_native)
                out[path, relax, e] = (post, diag, obs_block)
    return out


def _clean_routes(M, loc):
    if (M, loc) not in _CLEAN:
        _CLEAN[M, loc] = _all_routes(_problem(M), loc)
        ref = _CLEAN[M, loc]["auto", "none", "state_cycle"][0]
        assert np.isfinite(ref).all() and not np.array_equal(ref, _problem(M).X64)
    return _CLEAN[M, loc]


def _assert_obs_side(got, clean, what):
    rp.assert_diag_bits(got[1], clean[1], what)
    rp.assert_same_bits(got[2][0], clean[2][0], what + ": obs means")
    rp.assert_same_bits(got[2][1], clean[2][1], what + ": obs perturbations")


@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", rp.SIZES)
def test_scaling_rows_by_powers_of_two_is_exact(M, loc):
    """Relation 1 on every route."""
    pb = _problem(M)
    k = rp.row_exponents(ROWS, 500 + M)
    ps = pb.with_state(rp.scale_rows(pb.X32, k))
    clean = _clean_routes(M, loc)
    scaled = _all_routes(ps, loc)
    for key in clean:
        w = "M=%d loc=%s path=%s relax=%s entry=%s" % ((M, loc) + key)
        rp.assert_same_bits(scaled[key][0], rp.scale_rows(clean[key][0], k), w + ": update(D X) against D update(X)")
        _assert_obs_side(scaled[key], clean[key], w)


@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", rp.SIZES)
def test_poisoned_rows_change_no_other_row(M, loc):
    """Relation 2 on every route, for NaN, +Inf, zero and constant rows in turn: all the poisoned rows at once, then only the
    second row of each pair (a leak from a poisoned row into a poisoned neighbour would not show)."""
    pb = _problem(M)
    clean = _clean_routes(M, loc)
    gc = loc != "none"
    worst = 0.0
    for kind, rows in itertools.product(rp.POISON_KINDS, rp.POISON_SETS):
        pp = pb.with_state(rp.poison(pb.X32, kind, rows))
        got = _all_routes(pp, loc)
        ref = dict((relax, rp.oracle_members(pp, gc, relax)[0][rows]) for relax in RELAX) if kind == "const" else {}
        for key in clean:
            w = "M=%d loc=%s %s rows %s, path=%s relax=%s entry=%s" % ((M, loc, kind, rows.tolist()) + key)
            f32 = key[2] in ("f32_out", "f32_in")
            rp.assert_poisoned(kind, got[key][0], clean[key][0], w, ref_rows=ref.get(key[1]), f32=f32, poisoned=rows)
            if kind == "const":
                worst = max(worst, rp.rows_err(got[key][0][rows], ref[key[1]], f32=f32))
            _assert_obs_side(got[key], clean[key], w)
    print("M=%d loc=%s: constant rows, worst err/tol %.3g" % (M, loc, worst))


# ---------------------------------------------------------------------------
# relation 1, single cases on the same problem
# ---------------------------------------------------------------------------
def _scaled_pair(M, lo=-30, hi=30, **kw):
    pb = rp.RowProblem(M, **kw)
    k = rp.row_exponents(ROWS, 600 + M, lo, hi)
    return pb, pb.with_state(rp.scale_rows(pb.X32, k)), k


def _assert_entries_scale(pb, ps, k, gc, what):
    """Every entry point under the settings in force; returns the clean float64 member posterior."""
    L = _lib()
    for e in ENTRIES:
        a, b = _run(pb, gc, e), _run(ps, gc, e)
        w = "%s entry=%s" % (what, e)
        assert a[3:] == b[3:], w + ": another route"
        if gc:
            assert a[3] == L.PATH_SWEEP, w
        rp.assert_same_bits(b[0], rp.scale_rows(a[0], k), w)
        _assert_obs_side(b, a, w)
        if e == "state_cycle":
            ref = a
    return ref


def _vloc(rng):
    z = np.array([900.0, np.nan, 300.0])
    ov = rng.uniform(200.0, 1000.0, P)
    ov[::5] = np.nan
    return z, ov, rng.uniform(300.0, 700.0, P)


@pytest.mark.parametrize("onepass", [1, 0])
def test_scaling_with_vertical_localisation(onepass):
    """One-pass: every entry scales.  Per-batch: the library has no such route -- a vertical taper with `gc_onepass` 0 is refused
    (pinned by tests/test_gpu_vertical_localization.py) -- so what scaling must not change is the refusal itself: every
    entry refuses the scaled state as it refuses the clean one."""
    rng = np.random.default_rng(5)
    for M in (20, 7):
        pb, ps, k = _scaled_pair(M)
        plain = _run(pb, True, "state_cycle") if onepass else None
        with _settings(vloc=_vloc(rng), gc_onepass=onepass):
            if onepass:
                ref =_assert_entries_scale(pb, ps, k, True, "vertical localisation M=%d" % M)
                assert not np.array_equal(ref[0], plain[0]), "the vertical taper did nothing"
            else:
                for e, p in itertools.product(ENTRIES, (pb, ps)):
                    with pytest.raises(_lib().EfaError, match="gc_onepass"):
                        _run(p, True, e)


def test_scaling_rows_far_down_under_rtps():
    """Relation 1 with exponents down to -45 (float32 values and float64 squares stay normal: `scale_rows` asserts it), where a
    row's sum of squares falls to 1e-25 and below: an absolute threshold on the spread in the standalone RTPS passes
    (`k_row_spread`, `k_relax_rows`) shows here and not in [-30, 30].  The routes that take those passes: the sweeps, the GC
    sweeps, and the transform above 136 members."""
    L = _lib()
    for M, gc, path in ((20, False, L.PATH_SWEEP), (7, False, L.PATH_SWEEP), (20, True, L.PATH_AUTO), (7, True, L.PATH_AUTO),
                        (138, False, L.PATH_TRANSFORM)):
        pb, ps, k = _scaled_pair(M, lo=-45, hi=30)
        assert (k <= -40).sum() >= 5 and float(np.sum(ps.X64[6].astype(F64) ** 2)) < 1e-22
        with _settings(relax=(L.RELAX_RTPS, 0.5), path=path):
            ref = _assert_entries_scale(pb, ps, k, gc, "RTPS, exponents to -45, M=%d gc=%r path=%d" % (M, gc, path))
            assert _ctx().last_timing()["path"] == (L.PATH_TRANSFORM if M == 138 else L.PATH_SWEEP)
        with _settings(path=path):
            assert not np.array_equal(ref[0], _run(pb, gc, "state_cycle")[0]), "the relaxation did nothing"


def test_scaling_with_the_outlier_check():
    for M, gc in ((20, False), (20, True), (7, True)):
        pb, ps, k = _scaled_pair(M, gross=(0, 5))
        with _settings(outlier=3.0):
            ref = _assert_entries_scale(pb, ps, k, gc, "outlier check M=%d gc=%r" % (M, gc))
        assert not ref[1]["assimilated"][[0, 5]].any() and ref[1]["assimilated"].sum() == 8


def test_scaling_with_adaptive_inflation_leaves_the_field_bits():
    """Anderson (2009): the inflation field is dimensionless, so the scaled run leaves its bits; the posterior scales."""
    from test_gpu_adaptive_inflation import _field
    L, ctx = _lib(), _ctx()
    for M in (20, 7):
        pb, ps, k = _scaled_pair(M)
        field = _field(ROWS, seed=M)
        res = []
        for p in (pb, ps):
            Xd, F = ctx.to_device(p.X64), ctx.to_device(field)
            ctx.inflate_rows(ROWS, M, Xd, F)
            prior = Xd.download()
            ym, Yp = ctx.empty((P,)), ctx.to_device(p.HX)
            ctx.form_perts(P, M, Yp, ym, Yp)
            ctx.set_adaptive_inflation(F, ROWS)
            try:
                diag = ctx.ensrf_cycle(ROWS, M, P, Xd, Xd, ym, Yp, p.value, p.error, ASSIM, loc_mode=L.LOC_GC, ob_lat=p.ob_lat,
                                       ob_lon=p.ob_lon, ob_halfwidth=p.hw, grid_lat=p.glat, grid_lon=p.glon, n_lead=N_LEAD)
            finally:
                ctx.set_adaptive_inflation(None)
            res.append((Xd.download(), diag, F.download(), prior))
        (post, diag, fld, prior), (s_post, s_diag, s_fld, s_prior) = res
        rp.assert_same_bits(s_prior, rp.scale_rows(prior, k), "M=%d: inflated prior" % M)
        rp.assert_same_bits(s_post, rp.scale_rows(post, k), "M=%d: posterior under adaptive inflation" % M)
        rp.assert_same_bits(s_fld, fld, "M=%d: inflation field" % M)
        rp.assert_diag_bits(s_diag, diag, "M=%d" % M)
        assert not np.array_equal(fld, field) and not np.array_equal(post, prior)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
def test_scaling_through_the_streamed_host_update(dtype):
    L, ctx = _lib(), _ctx()
    for M, gc in ((20, True), (7, True), (20, False), (138, False)):
        pb, ps, k = _scaled_pair(M)
        res = []
        for p in (pb, ps):
            kw = dict(loc_mode=L.LOC_GC, ob_lat=p.ob_lat, ob_lon=p.ob_lon, ob_halfwidth=p.hw, grid_lat=p.glat, grid_lon=p.glon) if gc else {}
            prior = [np.ascontiguousarray(p.X32.astype(dtype)[:NCOL].reshape(1, NCOL, M)),
                     np.ascontiguousarray(p.X32.astype(dtype)[NCOL:].reshape(2, NCOL, M))]
            post = [np.empty(a.shape, dtype=dtype) for a in prior]
            diag = ctx.ensrf_cycle_host(prior, post, NCOL, M, p.HX, 16, p.value, p.error, ASSIM, **kw)
            assert ctx.stream_stats()["chunks"] == 3
            res.append((np.concatenate([a.reshape(-1, M) for a in post]), diag))
        w = "streamed %s M=%d gc=%r" % (np.dtype(dtype).name, M, gc)
        rp.assert_same_bits(res[1][0], rp.scale_rows(res[0][0], k), w)
        rp.assert_diag_bits(res[1][1], res[0][1], w)
        assert not np.array_equal(res[0][0], pb.X32.astype(dtype))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
@pytest.mark.parametrize("loc", [False, "GC"])
def test_scaling_through_the_python_api(loc, dtype):
    """`EnSRF.update()` with an operator override (as tests/test_gpu_parity._make_api_objects): the obs see the clean state."""
    from efa_xray_amd import EnSRF, EnsembleState, Observation

    class FixedOb(Observation):
        def estimate(self, state):
            return self.hx.copy()

    for M in (20, 7):
        pb, ps, k = _scaled_pair(M)
        res = []
        for p in (pb, ps):
            state = EnsembleState.from_array(p.X32.astype(dtype).reshape(N_LEAD, 1, NY, NX, M), p.lat2d, p.lon2d, dtype=dtype)
            rp.assert_same_bits(state.to_vect(), p.X32.astype(dtype), "state layout")
            obs = []
            for j in range(P):
                ob = FixedOb(value=float(p.value[j]), error=float(p.error[j]), lat=float(p.ob_lat[j]), lon=float(p.ob_lon[j]),
                             assimilate_this=bool(ASSIM[j]), localize_radius=float(p.hw[j]))
                ob.hx = p.HX[j]
                obs.append(ob)
            post, _ = EnSRF(state, obs, verbose=False, loc=loc).update()
            assert post.to_vect().dtype == dtype
            res.append((post.to_vect().copy(), dict((key, np.array([np.nan if getattr(o, key) is None else float(getattr(o, key))
                                                                     for o in obs])) for key in rp.DIAG)))
        w = "EnSRF.update() %s M=%d loc=%r" % (np.dtype(dtype).name, M, loc)
        rp.assert_same_bits(res[1][0], rp.scale_rows(res[0][0], k), w)
        rp.assert_diag_bits(res[1][1], res[0][1], w)
        assert not np.array_equal(res[0][0], pb.X32.astype(dtype))


# ---------------------------------------------------------------------------
# relation 3: obs and rows of mixed magnitude against the oracle, per row and per ob
# ---------------------------------------------------------------------------
def _member_cycle(c):
    """Phase A and `state_cycle` in member form, route asserted ("auto": the transform unlocalised, above 136 members only
    beyond M/2 assimilated obs): (posterior members, diagnostics, final obs means, final obs perturbations)."""
    L, ctx = _lib(), _ctx()
    N, M, Pn = c["N"], c["M"], c["P"]
    ym, Yp = ctx.empty((Pn,)), ctx.to_device(c["HX"])
    ctx.form_perts(Pn, M, Yp, ym, Yp)
    kw, grid = {}, {}
    if c["loc"]:
        kw = dict(loc_mode=L.LOC_GC, ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"])
        grid = dict(grid_lat=c["lat"].reshape(-1), grid_lon=c["lon"].reshape(-1), n_lead=c["n_lead"])
    diag = ctx.obs_phase(M, Pn, ym, Yp, c["val"], c["err"], c["asm"], **kw)
    X, post = ctx.to_device(c["X"]), ctx.empty((N, M))
    ctx.state_cycle(N, M, X, post, **grid)
    n_active = int(np.asarray(diag["assimilated"], dtype=bool).sum())
    transform = not c["loc"] and n_active > 0 and (M <= 136 or n_active > M // 2)
    assert ctx.last_timing()["path"] == (L.PATH_TRANSFORM if transform else L.PATH_SWEEP), "member form: another path"
    return post.download(), diag, ym.download(), Yp.download()


# (name, path, obs_batch, pipeline of tests/test_gpu_parity._run_hip, phase_a_kind up to 128 members)
_RUNS = [("sweep batch 1", "sweep", 1, None, None), ("sweep batch 32", "sweep", 32, None, None),
         ("transform", "transform", 32, None, None), ("per-batch kernels", "sweep", 32, 0, 2),
         ("vector chain", "sweep", 32, 1, 1), ("Gram leader", "sweep", 32, 2, 3), ("band leader", "sweep", 32, 3, 4)]

_MIXED = [(s, None) for s in rp.MIXED_SHAPES] + [(s[:3], s[3]) for s in rp.MIXED_GC_SHAPES]


@pytest.mark.parametrize("shape,ncol", _MIXED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_mixed_magnitudes_per_row_and_per_ob(shape, ncol):
    from _phase_a_guard import expected_kind
    from test_gpu_parity import _run_hip
    N, M, Pn = shape
    c = rp.mixed_case(N, M, Pn, ncol)
    j = rp.ob_exponents(Pn, 40 + M)
    cs = rp.scale_obs(c, j)
    xam, Xap, diag, ratio = rp.run_oracle(c, guard=True)
    assert expected_kind(ratio, M) == (4 if M <= 128 else 2)
    assert diag["assimilated"].any()
    want_path = {"sweep": _lib().PATH_SWEEP, "transform": _lib().PATH_TRANSFORM}
    ref_post = xam[:N, None] + Xap[:N]
    worst = {}
    for name, path, batch, pipe, kind in _RUNS:
        if ncol and path == "transform":
            continue
        w = "%r %s" % (shape, name)
        g_xam, g_Xap, g_diag = _run_hip(c, path=path, batch=batch, pipeline=pipe)
        got_kind = _ctx().get_option("phase_a_kind")
        assert _ctx().last_timing()["path"] == want_path[path], w + ": another path"
        if kind is not None:
            assert got_kind == (kind if M <= 128 else 2), "%s: phase_a_kind %d (guard min ratio %.3e)" % (w, got_kind, ratio)
        a, b = rp.assert_augmented_close(g_xam, g_Xap, xam, Xap, w)
        worst[name] = (a, b, rp.assert_diag_close(g_diag, diag, w))
        # ob k times 2^j: the state rows keep their bits, the obs rows and the diagnostics scale
        s_xam, s_Xap, s_diag = _run_hip(cs, path=path, batch=batch, pipeline=pipe)
        assert _ctx().get_option("phase_a_kind") == got_kind, w + ": the scaled obs took another Phase-A kernel"
        assert _ctx().last_timing()["path"] == want_path[path], w + ": the scaled obs took another path"
        rp.assert_same_bits(s_xam[:N], g_xam[:N], w + ": state means under scaled obs")
        rp.assert_same_bits(s_Xap[:N], g_Xap[:N], w + ": state perturbations under scaled obs")
        rp.assert_same_bits(s_xam[N:], np.ldexp(g_xam[N:], j), w + ": obs means under scaled obs")
        rp.assert_same_bits(s_Xap[N:], rp.scale_rows(g_Xap[N:], j), w + ": obs perturbations under scaled obs")
        rp.assert_diag_bits(s_diag, rp.scaled_diag(g_diag, j), w + " under scaled obs")
    w = "%r member form" % (shape,)
    post, g_diag, ym, Yp = _member_cycle(c)
    worst["member form"] = (rp.assert_rows_close(post, ref_post, w),
                            rp.assert_rows_close(Yp, Xap[N:], w + " obs perturbations"), rp.assert_diag_close(g_diag, diag, w))
    rp.assert_rows_close(ym.reshape(-1, 1), xam[N:].reshape(-1, 1), w + " obs means", extra=np.max(np.abs(Xap[N:]), axis=1))
    s_post, s_diag, s_ym, s_Yp = _member_cycle(cs)
    rp.assert_same_bits(s_post, post, w + ": posterior under scaled obs")
    rp.assert_same_bits(s_Yp, rp.scale_rows(Yp, j), w + ": obs perturbations under scaled obs")
    rp.assert_same_bits(s_ym, np.ldexp(ym, j), w + ": obs means under scaled obs")
    rp.assert_diag_bits(s_diag, rp.scaled_diag(g_diag, j), w + " under scaled obs")
    print("%r ncol=%r: worst err/tol (xam or members, Xap, diagnostics): %s" % (
        shape, ncol, "; ".join("%s %s" % (n, " ".join("%.3g" % v for v in t)) for n, t in worst.items())))
