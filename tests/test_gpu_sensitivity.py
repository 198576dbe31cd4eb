"""Ensemble sensitivity and observation targeting on the MI355X: efa_sensitivity_dev / efa_sensitivity_f32_dev against
the NumPy model tests/_sensitivity.py.

Tolerances (set by the definition, not measured): |var - ref| <= 1e-10 var0_i and |cov - ref| <= 1e-10 sqrt(var0_i varJ0_k), the
project's float64 parity figure relative to the unconditioned statistics; sens / corr / dvar / score are recomputed on the host from
the device's own var, cov and metric_var by the formulas of the definition, to 1e-10 relative; picked_row equals the model's
exactly, picked_score and metric_var to 1e-9 relative.  Every pick case asserts on the model that the best candidate leads the
second by >= 1e-6 relative, so that device rounding at 1e-10 cannot flip a pick.

Picks are made at 3 members and more, 31 of them at 80 and at 256 members; the two shapes of 2 members check the fields only.
An ensemble of 2 members has rank 1: every row correlates +-1 with every metric, so score_i = w varJ var_i / (var_i + R) and the
leading rows (var / R ~ 1e6) differ by ~1e-6 relative -- the picks are not separated by the margin above by construction (six of
twelve seeds tried on the model fell below it) -- and after one pick every later score is the 1e-6 remainder of a cancellation, where
the model itself is only good to 2e-8 relative against the explicit covariance update: no yardstick for a bound of 1e-9."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import _sensitivity as sm
from conftest import ROOT

pytestmark = pytest.mark.gpu

FIELDS = ("var", "cov", "sens", "corr", "dvar", "score")
TOL, TOL_PICK, MARGIN = 1e-10, 1e-9, 1e-6
GUARD = 64           # doubles between the fields of one allocation
SENTINEL = -1234.5
_SRC = open(os.path.join(ROOT, "efa_xray_amd", "csrc", "efa_sensitivity.hip")).read()
# k_sens_pass: at most kSensBlocks workgroups of 4 waves, a tile of 16 rows per wave and trip
ROWS_PER_TRIP = int(re.search(r"constexpr int kSensBlocks = (\d+);", _SRC).group(1)) * 4 * 16
assert 4096 <= ROWS_PER_TRIP <= 1 << 17


def _ctx():
    from efa_xray_amd import _lib
    return _lib.get_context(0)


def _call(ctx, X, J, n_lead, R, w=None, cand=None, n=0, dtype=np.float64, want=FIELDS, over=None):
    """One raw library call.  Every field lives in ONE device allocation, GUARD doubles of SENTINEL around each; only the fields
    in `want` are passed (the others NULL).  `over`: arguments replaced for the refusal tests.  Returns (status, outputs dict)."""
    from efa_xray_amd import _lib
    rows, M = X.shape
    K = J.shape[0]
    sizes = dict(var=rows, score=rows, cov=K * rows, sens=K * rows, corr=K * rows, dvar=K * rows)
    off, total = {}, GUARD
    for name in FIELDS:
        off[name] = total
        total += sizes[name] + GUARD
    buf = ctx.to_device(np.full(total, SENTINEL))
    Xd = ctx.to_device(X, dtype)
    d_cand = None
    if cand is not None:
        d_cand = ctx.malloc_bytes(max(rows, 1))
        ctx.h2d(d_cand, np.ascontiguousarray(cand, dtype=np.uint8))
    prow = np.full(max(n, 1), -77, dtype=np.int64)
    psc = np.full(max(n, 1), SENTINEL)
    mv = np.full((max(n, 0) + 1, K), SENTINEL)
    a = dict(rows=rows, M=M, K=K, X=Xd.ptr, J=np.ascontiguousarray(J, dtype=np.float64), ncol=rows // max(n_lead, 1), n_lead=n_lead,
             R=np.ascontiguousarray(R, dtype=np.float64), w=None if w is None else np.ascontiguousarray(w, dtype=np.float64),
             n=n, prow=prow, psc=psc, mv=mv)
    a.update(over or {})
    ptr = dict((name, ctypes.c_void_p(buf.address + 8 * off[name]) if name in want else None) for name in FIELDS)
    fn = ctx.lib.efa_sensitivity_f32_dev if np.dtype(dtype) == np.float32 else ctx.lib.efa_sensitivity_dev
    st = fn(ctx.handle, a["rows"], a["M"], a["K"], a["X"], _lib._dp(a["J"]), a["ncol"], a["n_lead"], _lib._dp(a["R"]), _lib._dp(a["w"]),
            d_cand, a["n"], ptr["var"], ptr["cov"], ptr["sens"], ptr["corr"], ptr["dvar"], ptr["score"],
            None if a["prow"] is None else a["prow"].ctypes.data_as(ctypes.POINTER(ctypes.c_long)), _lib._dp(a["psc"]), _lib._dp(a["mv"]))
    flat = buf.download()
    out = dict(picked_row=prow[:n], picked_score=psc[:n], metric_var=mv, flat=flat, off=off, sizes=sizes,
               sens_us=ctx.get_option("sens_us") if st == 0 else None)
    for name in FIELDS:
        f = flat[off[name]:off[name] + sizes[name]]
        out[name] = f if name in ("var", "score") else f.reshape(K, rows)
    if d_cand is not None:
        ctx.free_bytes(d_cand)
    Xd.free()
    buf.free()
    return st, out


def _guards_intact(out, written):
    """The guard words, and every field that was not asked for, still hold SENTINEL."""
    keep = np.ones(out["flat"].size, dtype=bool)
    for name in written:
        keep[out["off"][name]:out["off"][name] + out["sizes"][name]] = False
    return bool(np.all(out["flat"][keep] == SENTINEL))


def _assert_fields(what, out, m, w, cand, finite_rows=None):
    """var / cov against the model at the definition's tolerances; the derived fields from the device's own var / cov."""
    var0, varJ0 = m["var0"], m["varJ0"]
    ok = np.isfinite(var0) if finite_rows is None else finite_rows
    e_var = np.abs(out["var"] - m["var"])[ok]
    e_cov = np.abs(out["cov"] - m["cov"])[:, ok]
    s_cov = np.sqrt(var0[None, ok] * varJ0[:, None])
    worst_v = float(np.max(e_var / np.where(var0[ok] > 0, var0[ok], 1.0), initial=0.0))
    worst_c = float(np.max(e_cov / np.where(s_cov > 0, s_cov, 1.0), initial=0.0))
    print("%s: max |var - ref| / var0 = %.2e, max |cov - ref| / sqrt(var0 varJ0) = %.2e" % (what, worst_v, worst_c))
    assert np.all(e_var <= TOL * var0[ok]), what
    assert np.all(e_cov <= TOL * s_cov), what
    K = out["cov"].shape[0]
    ww = np.ones(K) if w is None else w
    cc = np.ones(var0.size, dtype=bool) if cand is None else np.asarray(cand).astype(bool)
    sens, corr, dvar, score = sm.derived(out["var"], out["cov"], out["metric_var"][-1], m["R_rows"], ww, cc)
    for name, exp in (("sens", sens), ("corr", corr), ("dvar", dvar), ("score", score)):
        got = out[name]
        assert np.array_equal(np.isnan(got), np.isnan(exp)), (what, name)
        fin = ~np.isnan(exp)
        assert np.all(np.isfinite(got[fin])), (what, name)
        assert np.all(np.abs(got[fin] - exp[fin]) <= TOL * np.abs(exp[fin])), (what, name, float(np.max(np.abs(got[fin] - exp[fin]))))


def _assert_picks(what, out, m, n):
    if n == 0:
        return
    made = int(np.sum(m["picked_row"] >= 0))
    if made:
        print("%s: %d picks, model margins %.1e .. %.1e" % (what, made, m["margins"].min(), m["margins"].max()))
        assert m["margins"].min() >= MARGIN, (what, m["margins"])
    assert np.array_equal(out["picked_row"], m["picked_row"]), (what, out["picked_row"], m["picked_row"])
    assert np.all(np.abs(out["picked_score"] - m["picked_score"]) <= TOL_PICK * np.abs(m["picked_score"])), what
    assert np.all(np.abs(out["metric_var"] - m["metric_var"]) <= TOL_PICK * np.abs(m["metric_var"])), what


# (rows per slab, n_lead, M, K, n_targets, storage): every value of every axis at least once, the edge values combined
F64, F32 = np.float64, np.float32
CASES = [
    (1, 1, 2, 1, 0, F64), (1, 1, 256, 32, 0, F32), (63, 1, 3, 3, 1, F64), (64, 1, 4, 16, 5, F32), (65, 1, 7, 32, 0, F64),
    (65, 1, 2, 1, 0, F64), (143, 1, 50, 3, 5, F64), (143, 3, 80, 1, 31, F64), (143, 17, 100, 16, 5, F32), (143, 3, 104, 3, 1, F32),
    (143, 1, 105, 1, 5, F64), (143, 17, 137, 32, 0, F32), (143, 3, 255, 3, 5, F64), (143, 17, 256, 16, 1, F64),
    (143, 1, 256, 1, 31, F32), (2 * ROWS_PER_TRIP + 53, 1, 7, 3, 1, F64),
]


@functools.lru_cache(maxsize=None)
def _problem(ncol, n_lead, M, K, n, dtype, offset=None):
    rows = ncol * n_lead
    X, J, R, w = sm.make_case(7000 + 13 * M + K + n + rows % 1000, rows, M, K, n_lead, offset)
    X = X.astype(dtype)
    cand = None
    if rows >= 63:      # every seventh row is no candidate
        cand = (np.arange(rows) % 7 != 3)
    return X, J, R, w, cand, sm.model(X.astype(np.float64), J, n_lead, R, w, cand, n)


@pytest.mark.parametrize("ncol,n_lead,M,K,n,dtype", CASES)
def test_fields_and_picks(ncol, n_lead, M, K, n, dtype):
    X, J, R, w, cand, m = _problem(ncol, n_lead, M, K, n, dtype)
    what = "%d x %d rows, M=%d K=%d n=%d %s" % (ncol, n_lead, M, K, n, np.dtype(dtype).name)
    st, out = _call(_ctx(), X, J, n_lead, R, w, cand, n, dtype)
    assert st == 0, what
    _assert_fields(what, out, m, w, cand)
    _assert_picks(what, out, m, n)
    assert _guards_intact(out, FIELDS)
    if cand is not None:
        assert np.all(out["score"][~cand] == 0.0)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_large_mean_small_spread(dtype):
    """Row mean 280, spread 1: the mean is removed from the registers before any product is formed."""
    X, J, R, w, cand, m = _problem(143, 3, 80, 3, 5, dtype, 280.0)
    st, out = _call(_ctx(), X, J, 3, R, w, cand, 5, dtype)
    assert st == 0
    _assert_fields("mean 280 %s" % np.dtype(dtype).name, out, m, w, cand)
    _assert_picks("mean 280 %s" % np.dtype(dtype).name, out, m, 5)


def test_exact_rules():
    ncol, n_lead, M, K = 143, 3, 20, 3
    rows = ncol * n_lead
    X, J, R, w = sm.make_case(31, rows, M, K, n_lead)
    X[5] = 0.1                       # constant, and its sum / M does not round back to 0.1
    X[9, 4] = np.nan
    X[11, 0] = np.inf
    X[70] = np.nan
    z = np.random.default_rng(2).standard_normal(M)
    X[20] = 3.0 + 2.0 * z            # two rows with identical members, far ahead of every other row
    X[21] = X[20]
    J[0] = 5.0 * z + 0.01 * J[0]
    cand = np.ones(rows, dtype=bool)
    cand[300:] = False
    cand[9] = cand[5] = True
    m = sm.model(X, J, n_lead, R, w, cand, 2)
    st, out = _call(_ctx(), X, J, n_lead, R, w, cand, 2)
    assert st == 0
    for f in ("var", "score"):
        assert out[f][5] == 0.0 and all(np.isnan(out[f][i]) for i in (9, 11, 70)), f
    for f in ("cov", "sens", "corr", "dvar"):
        assert np.all(out[f][:, 5] == 0.0) and all(np.all(np.isnan(out[f][:, i])) for i in (9, 11, 70)), f
    assert np.all(out["score"][300:] == 0.0) and np.count_nonzero(out["score"][:300]) > 250
    assert out["picked_row"][0] == 20 == m["picked_row"][0]          # the tie goes to the lower row
    assert not np.isin(out["picked_row"], [5, 9, 11, 70]).any() and np.all(out["picked_row"] < 300)
    if m["margins"][1] >= MARGIN:
        assert out["picked_row"][1] == m["picked_row"][1]
    fin = np.isfinite(m["var0"])
    _assert_fields("exact rules", out, m, w, cand, fin)
    # nothing to pick: no candidate at all, and every score 0 (metrics that do not vary)
    for c2, J2 in ((np.zeros(rows, dtype=bool), J), (cand, np.ones((K, M)) * np.array([[1.0], [2.0], [-3.0]]))):
        st, o = _call(_ctx(), X, J2, n_lead, R, w, c2, 3)
        ref = sm.model(X, J2, n_lead, R, w, c2, 3)
        assert st == 0 and np.all(o["picked_row"] == -1) and np.all(o["picked_score"] == 0.0)
        assert np.array_equal(o["metric_var"], np.tile(o["metric_var"][0], (4, 1)))
        assert np.allclose(o["metric_var"], ref["metric_var"], rtol=TOL_PICK, atol=0.0)
        assert np.all((o["score"] == 0.0) | np.isnan(o["score"])) and np.count_nonzero(np.isnan(o["score"])) <= 3


def test_null_fields_are_not_written():
    X, J, R, w, cand, m = _problem(143, 3, 104, 3, 1, F32)
    for want in (("cov",), ("var", "dvar"), ("score",), ()):
        st, out = _call(_ctx(), X, J, 3, R, w, cand, 1, F32, want=want)
        assert st == 0 and _guards_intact(out, want), want
        for name in want:
            assert not np.any(out[name] == SENTINEL), name
        _assert_picks("want=%r" % (want,), out, m, 1)
    # no field and no pick: no pass at all, metric_var alone
    st, out = _call(_ctx(), X, J, 3, R, w, cand, 0, F32, want=())
    assert st == 0 and _guards_intact(out, ()) and out["sens_us"] == 0
    assert np.allclose(out["metric_var"][0], m["varJ0"], rtol=TOL_PICK, atol=0.0)


@pytest.mark.parametrize("M,dtype", [(80, F64), (137, F32)])
def test_two_calls_agree_bit_for_bit(M, dtype):
    X, J, R, w = sm.make_case(77 + M, 143 * 17, M, 4, 17)
    X = X.astype(dtype)
    a = _call(_ctx(), X, J, 17, R, w, None, 5, dtype)[1]
    b = _call(_ctx(), X, J, 17, R, w, None, 5, dtype)[1]
    assert np.all(a["picked_row"] >= 0) and a["sens_us"] > 0
    for key in FIELDS + ("picked_row", "picked_score", "metric_var"):
        assert np.array_equal(a[key], b[key]), key


def test_refusals_leave_the_outputs_untouched():
    from efa_xray_amd import _lib
    ctx = _ctx()
    X, J, R, w = sm.make_case(3, 143 * 2, 7, 3, 2)

    def spoiled(a, value, at=1):
        a = np.array(a)
        a.reshape(-1)[at] = value
        return a

    overs = [dict(M=1), dict(M=257), dict(K=0), dict(n=-1), dict(n=30), dict(rows=285), dict(n_lead=3), dict(X=None), dict(J=None),
             dict(R=None), dict(J=spoiled(J, np.nan)), dict(J=spoiled(J, np.inf)), dict(R=spoiled(R, 0.0)), dict(R=spoiled(R, -1.0)),
             dict(R=spoiled(R, np.nan)), dict(R=spoiled(R, np.inf)), dict(w=spoiled(w, -1.0)), dict(w=spoiled(w, np.nan)),
             dict(w=spoiled(w, np.inf)), dict(prow=None), dict(psc=None), dict(mv=None)]
    for over in overs:
        st, out = _call(ctx, X, J, 2, R, w, None, 2, over=over)
        assert st == _lib.EFA_ERR_INVALID, over
        assert _guards_intact(out, ()), over
        assert np.all(out["picked_row"] == -77) and np.all(out["picked_score"] == SENTINEL) and np.all(out["metric_var"] == SENTINEL), over
    assert _call(ctx, X, J, 2, R, w, None, 2)[0] == 0
    assert _call(ctx, X, J, 2, R, spoiled(w, 0.0), None, 2)[0] == 0      # a weight of 0 is allowed


def test_a_cycle_after_a_sensitivity_call_returns_the_same_bits():
    """A GC cycle, a sensitivity call, the same cycle again: the second cycle's posterior and diagnostics are bit for bit those of
    a context that never made the call; gc_active_pairs and phase_a_kind too."""
    from efa_xray_amd import _lib
    glat, glon = np.meshgrid(np.linspace(25, 55, 13), np.linspace(240, 290, 11), indexing="ij")
    glat, glon = glat.reshape(-1), glon.reshape(-1)
    ncol, n_lead, M, P = glat.size, 5, 20, 60
    rng = np.random.default_rng(11)
    N = n_lead * ncol
    X = 2.0 * rng.standard_normal((N, M)) + rng.standard_normal((N, 1))
    pick = rng.choice(N, P, replace=False)
    HX = X[pick] + 0.05 * rng.standard_normal((P, M))
    ob = dict(value=HX.mean(axis=1) + rng.standard_normal(P), error=rng.uniform(0.5, 2.0, P), assim=rng.random(P) < 0.9,
              lat=glat[pick % ncol] + rng.uniform(-0.5, 0.5, P), lon=glon[pick % ncol] + rng.uniform(-0.5, 0.5, P),
              hw=rng.uniform(600, 1500, P))
    Xs, Js, Rs, ws, cs, ms = _problem(143, 3, 50, 3, 2, F64)

    def cycle(ctx):
        Xd, post, Yp, ym = ctx.to_device(X), ctx.empty((N, M)), ctx.to_device(HX), ctx.empty((P,))
        ctx.form_perts(P, M, Yp, ym, Yp)
        diag = ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, ob["value"], ob["error"], ob["assim"], _lib.LOC_GC, ob["lat"], ob["lon"],
                               ob["hw"], glat, glon, n_lead)
        return post.download(), diag, ctx.get_option("gc_active_pairs"), ctx.get_option("phase_a_kind")

    results = []
    for with_call in (True, False):
        ctx = _lib.Context(0)
        try:
            first = cycle(ctx)
            if with_call:
                st, out = _call(ctx, Xs, Js, 3, Rs, ws, cs, 2)
                assert st == 0
                _assert_fields("between two cycles", out, ms, ws, cs)
                _assert_picks("between two cycles", out, ms, 2)
            results.append((first, cycle(ctx)))
        finally:
            ctx.close()
    (a1, a2), (b1, b2) = results
    for got, want in ((a1, b1), (a2, b2)):
        assert np.array_equal(got[0], want[0])
        for key in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
            assert np.array_equal(got[1][key], want[1][key], equal_nan=True), key
        assert got[2:] == want[2:]
    assert a2[2] > 0


@pytest.mark.parametrize("dtype", [F64, F32])
def test_end_to_end(dtype):
    """observation_targets and ensemble_sensitivity on 2 variables x 2 times x 9 x 11 x 20 members; candidates: one variable at the
    first time only."""
    from efa_xray_amd import EnsembleState, ensemble_sensitivity, observation_targets
    nvar, nt, ny, nx, M, K, n = 2, 2, 9, 11, 20, 2, 3
    rows = nvar * nt * ny * nx
    X, J, R, w = sm.make_case(41, rows, M, K, nvar * nt)
    lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(230, 260, nx), indexing="ij")
    times = np.array([0.0, 3600.0])
    st = EnsembleState.from_array(X.reshape(nvar, nt, ny, nx, M), lat, lon, varnames=["t", "q"], validtime=times, dtype=dtype)
    Xw = st.to_vect().astype(np.float64)
    err = dict(t=0.8, q=1.7)
    Rs = np.repeat([0.8, 1.7], nt)
    cand = np.zeros((nvar, nt, ny, nx), dtype=bool)
    cand[1, 0] = True
    m = sm.model(Xw, J, nvar * nt, Rs, w, cand.reshape(-1), n)
    assert m["margins"].size == n and m["margins"].min() >= MARGIN
    res = observation_targets(st, dict(a=J[0], b=J[1]), n, err, candidates=dict(q=np.array([True, False])[:, None, None]),
                              weights=dict(a=w[0], b=w[1]))
    assert [tg["row"] for tg in res["targets"]] == list(m["picked_row"])
    for tg, row, sc in zip(res["targets"], m["picked_row"], m["picked_score"]):
        iv, it, iy, ix = np.unravel_index(row, (nvar, nt, ny, nx))
        assert (tg["var"], tg["time"], tg["y"], tg["x"]) == ("q", times[it], iy, ix) and iv == 1 and it == 0
        assert tg["lat"] == lat[iy, ix] and tg["lon"] == lon[iy, ix]
        assert abs(tg["score"] - sc) <= TOL_PICK * sc
    assert res["metric_var"].shape == (n + 1, K) and res["names"] == ["a", "b"]
    assert np.all(np.abs(res["metric_var"] - m["metric_var"]) <= TOL_PICK * np.abs(m["metric_var"]))
    assert res["score"].shape == (nvar, nt, ny, nx) and res["dvar"].shape == (K, nvar, nt, ny, nx)
    assert np.all(res["score"][~cand] == 0.0)
    assert np.allclose(res["score"].reshape(-1), m["score"], rtol=1e-8, atol=0.0)
    assert np.allclose(res["dvar"].reshape(K, -1), m["dvar"], rtol=1e-6, atol=1e-10 * np.max(np.abs(m["dvar"])))

    m0 = sm.model(Xw, J, nvar * nt, np.ones(nvar * nt), None, None, 0)
    ens = ensemble_sensitivity(st, J)
    assert ens["var"].shape == (nvar, nt, ny, nx) and all(ens[f].shape == (K, nvar, nt, ny, nx) for f in ("cov", "sens", "corr"))
    assert np.all(np.abs(ens["var"].reshape(-1) - m0["var"]) <= TOL * m0["var0"])
    assert np.all(np.abs(ens["cov"].reshape(K, -1) - m0["cov"]) <= TOL * np.sqrt(m0["var0"][None, :] * m0["varJ0"][:, None]))
    assert np.allclose(ens["sens"].reshape(K, -1), m0["sens"], rtol=1e-6, atol=1e-9 * np.max(np.abs(m0["sens"])))
    assert np.allclose(ens["corr"].reshape(K, -1), m0["corr"], rtol=1e-6, atol=1e-9)
    assert np.allclose(ens["metric_var"], m0["varJ0"], rtol=TOL_PICK, atol=0.0)
