"""GPU tests of Phase A on poisoned, degenerate and guard-margin observations.  tests/test_gpu_rowprops.py keeps
its poison out of Phase A; here it goes in, through every Phase-A kernel (`pipeline` 0..3 of tests/test_gpu_parity._run_hip:
per-batch kernels, vector chain, Gram leader, band leader), without localisation and under Gaspari-Cohn, 96 state rows riding along
behind 150 obs (two full 64-row blocks and a partial one):

  A. value and error of an ob whose flag is 0 are not read: NaN, Inf, 0, negative and huge pairs leave every bit of every output;
  B. an ob the outlier check rejects for a NaN value, error or member is an ob whose flag is 0, bit for bit;
  C. a NaN, +Inf, zero or one-NaN-member row of an ob whose flag is 0 changes no other row, no state row and no other diagnostic;
  D. assimilated obs without spread (R > 0) have no gain: every output finite, every other row's bits those of the flags-off run;
  E. near-copy pairs tuned on the CPU to [SAFE, 2 SAFE] of the leaders' cancellation guard keep the leaders and the project's
     1e-10 per row and per ob; tuned to [FALLS_BACK / 2, FALLS_BACK] in one block they send both leaders to the vector chain;
  F. obs rows that are not centred: RTOL per ob against the oracle on the same arrays, the leaders up to a shift of 1e-12 of the
     row's spread and the vector chain from 1e-10 on.

The finite cases come first, the non-finite ones in functions of their own behind them.  tests/test_obsprops_host.py proves the
generators' conditions and the oracle's side of every relation on the CPU.

Seen on the MI355X (DESIGN.md 7n has the table).  A, B: bit for bit on every kernel and entry; the parent commit's persistent
kernels fail them (NaN means and rows), hence the neutral (0, 1) pair in the device pack.  C: bit for bit and 2.6e-4 of RTOL on the
other rows; both leader requests are served by the vector chain for NaN / +Inf / one-NaN rows and by the leaders themselves for zero
rows.  D: 2.4e-4; both leader requests are served by the vector chain (G_kk = 0 is not above a threshold of 0).  Worst err/RTOL of
E: per-batch 9.5e-4, vector chain 9.7e-4, Gram leader 7.7e-3, band leader 1.0e-2 (the leaders at [SAFE, 2 SAFE]; at
[FALLS_BACK / 2, FALLS_BACK] both report kind 1); of F: 2.2e-4, 4.2e-4, 2.7e-4, 2.1e-4, the leaders at c = 1e-12 and kind 1 from
1e-10 on."""
import numpy as np
import pytest

import _obsprops as op
import _outlier as qc
import _rowprops as rp
from _phase_a_guard import expected_kind
from _rowprops import F32, assert_same_bits
from test_gpu_f32_state import _ctx, _lib, _settings
from test_gpu_parity import GRAM_DEFAULT, _run_hip

pytestmark = pytest.mark.gpu

LOCS = [False, True]
N, P = op.N, op.P
_CACHE = {}


def _paths(loc):
    """State paths of the augmented-array entry: the sweeps, and without localisation "auto": the transform with its carried
    [T | w] rows behind the obs rows."""
    return ("sweep",) if loc else ("sweep", "auto")


def _hip(c, request, path="sweep"):
    """(xam, Xap, diag, phase_a_kind) of `_run_hip`."""
    xam, Xap, diag = _run_hip(c, path=path, batch=32, pipeline=request)
    return xam, Xap, diag, _ctx().get_option("phase_a_kind")


def _assert_bits(got, want, what, obs=None):
    """Two runs of `_hip`: every row of both arrays bit for bit, the diagnostics (of the obs in `obs` only), the kind."""
    assert_same_bits(got[0], want[0], what + ": means")
    assert_same_bits(got[1], want[1], what + ": perturbations")
    op.assert_diag_bits(got[2], want[2], what, obs=obs)
    assert got[3] == want[3], "%s: phase_a_kind %d against %d" % (what, got[3], want[3])


def _assert_oracle(got, ref, what):
    """A run of `_hip` within RTOL of the oracle's (xam, Xap, diag), per row and per ob: worst err/RTOL."""
    a, b = rp.assert_augmented_close(got[0], got[1], ref[0], ref[1], what)
    return max(a, b, rp.assert_diag_close(got[2], ref[2], what))


def _clean_oracle(M, loc, rows_key):
    key = ("oracle", M, loc, rows_key)
    if key not in _CACHE:
        rows = dict(special=op.SPECIAL, second=op.SPECIAL_SECOND)[rows_key]
        _CACHE[key] = (op.base_case(M, loc, False, rows=rows),) + op.oracle_case(op.base_case(M, loc, False, rows=rows))
    return _CACHE[key]


# ---------------------------------------------------------------------------
# Part A, finite pairs
# ---------------------------------------------------------------------------
def _ignored_inputs(M, loc, pairs):
    worst = 0.0
    for rows_key, rows in (("special", op.SPECIAL), ("second", op.SPECIAL_SECOND)):
        c, xam, Xap, diag, ratio = _clean_oracle(M, loc, rows_key)
        assert expected_kind(ratio, M) == (4 if M <= 128 else 2)
        for request in op.REQUESTS:
            for path in _paths(loc):
                w = "M=%d loc=%r request %d path=%s rows %s" % (M, loc, request, path, rows_key)
                clean = _hip(c, request, path)
                assert clean[3] == op.want_kind(request, M), "%s: phase_a_kind %d" % (w, clean[3])
                worst = max(worst, _assert_oracle(clean, (xam, Xap, diag), w))
                for pair in pairs:
                    _assert_bits(_hip(op.with_ignored(c, pair, rows), request, path), clean, "%s (value, error) = %r" % (w, pair))
    print("M=%d loc=%r: clean runs, worst err/RTOL %.3g" % (M, loc, worst))


@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [7, 24, 100, 130])
def test_finite_value_and_error_of_unassimilated_obs_are_not_read(M, loc):
    """Part A with (0, 0), (1, -1) and (1e300, 1e-300): bit for bit the clean run, which is within RTOL of the oracle."""
    _ignored_inputs(M, loc, op.IGNORED_FINITE)


# ---------------------------------------------------------------------------
# the obs_phase entry: the obs block exactly as the test writes it, the state through `state_cycle`
# ---------------------------------------------------------------------------
def _members(c, ym, Yp, request, outlier=None):
    """Phase A on (ym, Yp) as given, then the member-form state cycle on the sweeps: (obs means, obs perturbations, diag, kind,
    posterior members)."""
    L, ctx = _lib(), _ctx()
    M, Pn = c["M"], len(ym)
    kw, grid = {}, {}
    if c["loc"]:
        kw = dict(loc_mode=L.LOC_GC, ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"])
        grid = dict(grid_lat=c["lat"].reshape(-1), grid_lon=c["lon"].reshape(-1), n_lead=c["n_lead"])
    ctx.set_option("pipeline", 1 if request else 0)
    ctx.set_option("gram", 2 if request == 3 else 1 if request == 2 else 0)
    try:
        with _settings(path=L.PATH_SWEEP, **({} if outlier is None else dict(outlier=outlier))):
            ymd, Ypd = ctx.to_device(np.ascontiguousarray(ym)), ctx.to_device(np.ascontiguousarray(Yp))
            diag = ctx.obs_phase(M, Pn, ymd, Ypd, c["val"], c["err"], c["asm"], **kw)
            kind = ctx.get_option("phase_a_kind")
            X, post = ctx.to_device(c["X"]), ctx.empty((c["N"], M))
            ctx.state_cycle(c["N"], M, X, post, **grid)
            return ymd.download(), Ypd.download(), diag, kind, post.download()
    finally:
        ctx.set_option("pipeline", 1)
        ctx.set_option("gram", GRAM_DEFAULT)


def _assert_members_bits(got, want, what, keep=None, same_kind=True):
    assert_same_bits(got[0], want[0], what + ": obs means", rows=keep)
    assert_same_bits(got[1], want[1], what + ": obs perturbations", rows=keep)
    op.assert_diag_bits(got[2], want[2], what, obs=keep)
    assert_same_bits(got[4], want[4], what + ": posterior members")
    if same_kind:
        assert got[3] == want[3], "%s: phase_a_kind %d against %d" % (what, got[3], want[3])


def _assert_members_oracle(got, ref, c, what, keep=None):
    """Against the oracle's (xam, Xap, diag): state members, obs rows and diagnostics of the obs in `keep`; worst err/RTOL."""
    n = c["N"]
    a = op.assert_block_close((got[4], got[0], got[1]), (ref[0][:n, None] + ref[1][:n], ref[0][n:], ref[1][n:]), what, keep=keep)
    return max(a, op.assert_diag_close(got[2], ref[2], what, obs=keep))


def _leader_kind(kind, request, M, what):
    """Requests 2 and 3 on a block whose degenerate rows may trip a guard: the requested leader or the vector chain."""
    want = op.want_kind(request, M)
    if request in (2, 3) and M <= 128:
        assert kind in (want, 1), "%s: phase_a_kind %d" % (what, kind)
    else:
        assert kind == want, "%s: phase_a_kind %d" % (what, kind)
    return kind


# ---------------------------------------------------------------------------
# Part D: assimilated obs without spread
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [7, 24, 128, 130])
def test_zero_spread_obs_have_no_gain(M, loc):
    rows = op.zero_spread_rows()
    on, off = op.zero_spread_case(M, loc, True), op.zero_spread_case(M, loc, False)
    ref = op.oracle_case(on)
    keep = op.others(rows)
    served, worst = {}, 0.0
    for request in op.REQUESTS:
        for path in _paths(loc):
            w = "M=%d loc=%r request %d path=%s" % (M, loc, request, path)
            got = _hip(on, request, path)
            served[request, path] = _leader_kind(got[3], request, M, w)
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), w + ": not finite"
            for key in rp.DIAG[:4]:
                assert np.isfinite(np.asarray(got[2][key])[rows]).all(), "%s: %s of a zero-spread ob" % (w, key)
            worst = max(worst, rp.rows_err(got[1], ref[1]),
                        rp.rows_err(got[0].reshape(-1, 1), ref[0].reshape(-1, 1), extra=np.max(np.abs(ref[1]), axis=1)),
                        op.diag_err(got[2], ref[2]))
            assert worst <= 1.0, "%s: off by %.3g of the tolerance" % (w, worst)
            assert (np.asarray(got[2]["post_var"])[rows] == 0).all(), w + ": post_var of a zero-spread ob"
            assert_same_bits(np.asarray(got[2]["post_mean"])[rows], np.asarray(got[2]["prior_mean"])[rows], w + ": post_mean")
            if request in (0, 1):
                flags_off = _hip(off, request, path)
                _assert_bits(got, flags_off, w + " against the flags-off run", obs=keep)
                for key in ("prior_mean", "prior_var"):
                    assert_same_bits(np.asarray(got[2][key]), np.asarray(flags_off[2][key]), w + ": " + key)
    print("M=%d loc=%r: zero-spread obs, worst err/RTOL %.3g; leader requests served by %s" % (
        M, loc, worst, ", ".join("request %d: kind %s" % (r, sorted(set(k for (rr, p), k in served.items() if rr == r))) for r in (2, 3))))


# ---------------------------------------------------------------------------
# Part E: the cancellation guard's margin
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,loc", op.MARGIN_CASES)
def test_cancellation_guard_margins(name, M, loc):
    c = op.margin(name, M, loc)
    ref = rp.run_oracle(c)
    worst = {}
    for request in op.REQUESTS:
        w = "%s M=%d loc=%r request %d" % (name, M, loc, request)
        got = _hip(c, request)
        want = op.want_kind(request, M) if (name == "safe" or request < 2) else 1
        assert got[3] == want, "%s: phase_a_kind %d, expected %d (block min ratios %s)" % (
            w, got[3], want, " ".join("%.2e" % v for v in c["block_ratios"].values()))
        worst[got[3]] = max(worst.get(got[3], 0.0), _assert_oracle(got, ref, w))
    print("%s M=%d loc=%r: worst err/RTOL per kind: %s" % (name, M, loc, ", ".join("%d: %.3g" % kv for kv in sorted(worst.items()))))


# ---------------------------------------------------------------------------
# Part F: obs rows that are not centred
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [7, 100, 128])
def test_uncentred_obs_rows(M, loc):
    c = op.base_case(M, loc, True, rows=np.array(op.UNCENTRED_ROWS))
    c = dict(c, X=c["X"][:0], N=0)                      # the obs block alone, as the oracle takes it
    ym, Yp = op.priors(c)
    worst = {}
    for cfac in op.UNCENTRED_C:
        Ys = op.uncentred(Yp, cfac)
        r_ym, r_Yp, r_diag = op.oracle_obs_only(c, ym, Ys)
        for request in op.REQUESTS:
            w = "M=%d loc=%r c=%g request %d" % (M, loc, cfac, request)
            got = _obs_only(c, ym, Ys, request)
            want = op.want_kind(request, M) if (request < 2 or cfac < 1e-11) else 1
            assert got[3] == want, "%s: phase_a_kind %d, expected %d" % (w, got[3], want)
            a, b = rp.assert_augmented_close(got[0], got[1], r_ym, r_Yp, w)
            worst[got[3]] = max(worst.get(got[3], 0.0), a, b, rp.assert_diag_close(got[2], r_diag, w))
    print("M=%d loc=%r: uncentred rows, worst err/RTOL per kind: %s" % (M, loc, ", ".join("%d: %.3g" % kv for kv in sorted(worst.items()))))


def _obs_only(c, ym, Yp, request):
    """`obs_phase` alone: (obs means, obs perturbations, diag, kind)."""
    L, ctx = _lib(), _ctx()
    kw = dict(loc_mode=L.LOC_GC, ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"]) if c["loc"] else {}
    ctx.set_option("pipeline", 1 if request else 0)
    ctx.set_option("gram", 2 if request == 3 else 1 if request == 2 else 0)
    try:
        with _settings(path=L.PATH_SWEEP):
            ymd, Ypd = ctx.to_device(np.ascontiguousarray(ym)), ctx.to_device(np.ascontiguousarray(Yp))
            diag = ctx.obs_phase(c["M"], len(ym), ymd, Ypd, c["val"], c["err"], c["asm"], **kw)
            return ymd.download(), Ypd.download(), diag, ctx.get_option("phase_a_kind")
    finally:
        ctx.set_option("pipeline", 1)
        ctx.set_option("gram", GRAM_DEFAULT)


# ---------------------------------------------------------------------------
# Part C: rows of unassimilated obs -- zeros here, the non-finite ones below
# ---------------------------------------------------------------------------
def _poisoned_rows(M, loc, kinds):
    served, worst = {}, 0.0
    for rows in op.SPECIAL_SETS:
        c = op.base_case(M, loc, False, rows=rows)
        ym, Yp = op.priors(c)
        keep = op.others(rows)
        clean = dict((request, _members(c, ym, Yp, request)) for request in op.REQUESTS)
        for request in op.REQUESTS:
            assert clean[request][3] == op.want_kind(request, M)
        for kind in kinds:
            Ybad = op.poison_obs_rows(Yp, kind, rows)
            ref = op.oracle_block(c, ym, Ybad)
            for request in op.REQUESTS:
                w = "M=%d loc=%r %s rows %s, request %d" % (M, loc, kind, rows.tolist(), request)
                got = _members(c, ym, Ybad, request)
                served[kind, len(rows), request] = _leader_kind(got[3], request, M, w)
                worst = max(worst, _assert_members_oracle(got, ref, c, w, keep=keep))
                op.assert_own_priors(got[2], ref[2], rows, w)
                assert not np.asarray(got[2]["assimilated"])[rows].any(), w
                if request in (0, 1):
                    _assert_members_bits(got, clean[request], w + " against the clean run", keep=keep)
    print("M=%d loc=%r: poisoned rows %s, worst err/RTOL of the other rows %.3g; leader requests served by %s" % (
        M, loc, "/".join(kinds), worst, ", ".join("%s request %d: kind %s" % (kd, r, sorted(set(v for k, v in served.items() if k[0] == kd and k[2] == r)))
                                                   for kd in kinds for r in (2, 3))))


@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [7, 100, 128, 256])
def test_zero_rows_of_unassimilated_obs_change_no_other_row(M, loc):
    _poisoned_rows(M, loc, ("zero",))


# ===========================================================================
# the non-finite cases
# ===========================================================================
@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [7, 24, 100, 130])
def test_nonfinite_value_and_error_of_unassimilated_obs_are_not_read(M, loc):
    """Part A with (NaN, NaN), (+Inf, 1) and (-Inf, +Inf)."""
    _ignored_inputs(M, loc, op.IGNORED_NONFINITE)


def _entries(c, M, loc):
    """Every other entry point on the case, each as a flat list of arrays (kinds and paths as the library chooses them)."""
    L, ctx = _lib(), _ctx()
    n = c["N"]
    kw, grid = {}, {}
    if loc:
        kw = dict(loc_mode=L.LOC_GC, ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"])
        grid = dict(grid_lat=c["lat"].reshape(-1), grid_lon=c["lon"].reshape(-1), n_lead=c["n_lead"])
    out = {}

    def block():
        ym, Yp = ctx.empty((P,)), ctx.to_device(c["HX"])
        ctx.form_perts(P, M, Yp, ym, Yp)
        return ym, Yp

    def flat(diag, *arrays):
        return [np.asarray(diag[k]) for k in rp.DIAG] + [np.asarray(a) for a in arrays]

    ym, Yp = block()
    diag = ctx.obs_phase(M, P, ym, Yp, c["val"], c["err"], c["asm"], **kw)
    X, post = ctx.to_device(c["X"]), ctx.empty((n, M))
    ctx.state_cycle(n, M, X, post, **grid)
    out["obs_phase + state_cycle"] = flat(diag, ym.download(), Yp.download(), post.download(), ctx.get_option("phase_a_kind"))
    X32, post32 = ctx.to_device(c["X"].astype(F32), F32), ctx.empty((n, M), F32)
    ctx.state_cycle_f32(n, M, X32, post32, **grid)
    out["float32 state cycle"] = flat(diag, post32.download())
    ym, Yp = block()
    X, post = ctx.to_device(c["X"]), ctx.empty((n, M))
    diag = ctx.ensrf_cycle(n, M, P, X, post, ym, Yp, c["val"], c["err"], c["asm"], obs_block_out=True, **kw, **grid)
    out["ensrf_cycle"] = flat(diag, ym.download(), Yp.download(), post.download(), ctx.last_timing()["path"])
    if not loc:
        assert ctx.last_timing()["path"] == L.PATH_TRANSFORM, "the fused cycle did not take the transform"
    ncol = op.NCOL
    prior = [np.ascontiguousarray(c["X"].reshape(n // ncol, ncol, M))]
    host_post = [np.empty_like(prior[0])]
    diag = ctx.ensrf_cycle_host(prior, host_post, ncol, M, c["HX"], 16, c["val"], c["err"], c["asm"],
                                **dict(kw, **dict((k, grid[k]) for k in ("grid_lat", "grid_lon") if k in grid)))
    assert ctx.stream_stats()["chunks"] == 3
    out["ensrf_cycle_host"] = flat(diag, host_post[0])
    return out


def _api(c, M, loc, none_for_ignored):
    """`EnSRF(...).update()` with the special obs as `Observation(value=None, error=None, assimilate_this=False)`."""
    from efa_xray_amd import EnSRF, EnsembleState, Observation

    class FixedOb(Observation):
        def estimate(self, state):
            return self.hx.copy()

    ny, nx = (c["ny"], c["nx"]) if loc else (6, 8)
    lat, lon = (c["lat"], c["lon"]) if loc else np.meshgrid(np.linspace(-70, 70, ny), np.linspace(0, 357, nx), indexing="ij")
    state = EnsembleState.from_array(c["X"].reshape(N // op.NCOL, 1, ny, nx, M), lat, lon)
    assert_same_bits(state.to_vect(), c["X"], "state layout")
    obs = []
    for k in range(P):
        ignored = none_for_ignored and k in op.SPECIAL
        ob = FixedOb(value=None if ignored else float(c["val"][k]), error=None if ignored else float(c["err"][k]),
                     lat=float(c["ob_lat"][k]) if loc else 0.0, lon=float(c["ob_lon"][k]) if loc else 0.0,
                     assimilate_this=bool(c["asm"][k]), localize_radius=float(c["hw"][k]) if loc else None)
        ob.hx = c["HX"][k]
        obs.append(ob)
    post, _ = EnSRF(state, obs, verbose=False, loc="GC" if loc else False).update()
    return [post.to_vect().copy()] + [np.array([np.nan if getattr(o, key) is None else float(getattr(o, key)) for o in obs]) for key in rp.DIAG]


@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [24, 100])
def test_nan_value_and_error_through_every_other_entry_point(M, loc):
    """Part A, (NaN, NaN) only: obs_phase + state_cycle, the float32 state cycle, the fused ensrf_cycle (the speculative transform
    without localisation), the streamed host update in chunks of 16 columns and the Python front end, each against the bits of
    its own clean run."""
    c = _clean_oracle(M, loc, "special")[0]
    bad = op.with_ignored(c, (np.nan, np.nan))
    clean, got = _entries(c, M, loc), _entries(bad, M, loc)
    clean["EnSRF.update()"], got["EnSRF.update()"] = _api(c, M, loc, False), _api(bad, M, loc, True)
    for name in clean:
        assert len(clean[name]) == len(got[name])
        for i, (a, b) in enumerate(zip(got[name], clean[name])):
            assert_same_bits(np.asarray(a), np.asarray(b), "M=%d loc=%r %s, output %d" % (M, loc, name, i))


# ---------------------------------------------------------------------------
# Part B: the outlier check
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [24, 100])
@pytest.mark.parametrize("what", ["value", "error", "row"])
def test_outlier_check_rejects_nan_as_a_cleared_flag(what, M, loc):
    bad, ref, ym, Yp = op.outlier_case(M, loc, what)
    keep = op.others(op.SPECIAL)
    served = {}
    for request in op.REQUESTS:
        w = "NaN %s, M=%d loc=%r request %d" % (what, M, loc, request)
        got = _members(bad, ym, Yp, request, outlier=op.OUTLIER_T)
        want = _members(ref, ym, Yp, request, outlier=op.OUTLIER_T)
        assert not np.asarray(got[2]["assimilated"])[op.SPECIAL].any(), w + ": a poisoned ob was assimilated"
        assert np.asarray(want[2]["assimilated"])[keep].sum() >= 100
        if what == "row":      # Part C's rules: the other rows and obs against the oracle, and bit for bit for requests 0 and 1
            served[request] = _leader_kind(got[3], request, M, w)
            with np.errstate(invalid="ignore"):
                flags = ref["asm"] & ~qc.outlier_mask(ym, Yp, ref["val"], ref["err"], ref["asm"], op.OUTLIER_T)
            oracle = op.oracle_block(dict(ref, asm=flags), ym, Yp)
            _assert_members_oracle(got, oracle, ref, w, keep=keep)
            op.assert_own_priors(got[2], oracle[2], op.SPECIAL, w)
            if request in (0, 1):
                _assert_members_bits(got, want, w, keep=keep)
        else:
            assert got[3] == op.want_kind(request, M), "%s: phase_a_kind %d" % (w, got[3])
            _assert_members_bits(got, want, w)
            assert np.isfinite(got[4]).all() and np.isfinite(got[1]).all()
    if served:
        print("NaN member, M=%d loc=%r: leader requests served by %s" % (M, loc, served))


# ---------------------------------------------------------------------------
# Part C, non-finite rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [7, 100, 128, 256])
def test_nonfinite_rows_of_unassimilated_obs_change_no_other_row(M, loc):
    _poisoned_rows(M, loc, ("nan", "inf", "one_nan"))
