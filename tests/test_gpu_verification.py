"""Ensemble verification on the MI355X: efa_verify_dev / efa_verify_f32_dev against the NumPy model
tests/_verification.py.

Integers (below, equal, rank, hist, n, n_bad) are compared exactly.  Tolerances of the floats, u = 2^-53, mad = mean |d| of the row,
from the forward bound of an M-term sum of once-rounded terms (DESIGN.md 7o has the derivation):
  crps  (2M + 8) u mad                      the two M-term sums plus the rounding of d (the issue's bound)
  err   (M + 4) u mad                       one M-term sum, a division
  var   (4M + 16) u (var + err^2 M/(M-1))   M squares of differences from a rounded mean, sum (d - err)^2 <= sum d^2
  sums  (n + 4) u sum |w t|  +  sum of w times the row's bound above (for err^2: (2 |err| + b) b with b the bound of err);
        n - 1 roundings of the n-term sum, up to two in each term (w t; err^2), the rest for the terms of second order."""
import ctypes

import numpy as np
import pytest

import _verification as vm

pytestmark = pytest.mark.gpu

U = vm.U
MEMBERS = [2, 3, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256]
N_LEAD, NCOL = 4, 39          # nvar = 2, nt = 2, ny = 3, nx = 13
INT_FIELDS = ("below", "equal", "rank")
FLT_FIELDS = ("crps", "err", "var")
SENT_I, SENT_F = -77, -1234.5


def _ctx():
    from efa_xray_amd import _lib
    return _lib.get_context(0)


def _call(X, y, slab_group, n_lead, w=None, fair=False, seed=0, col_offset=0, ncol_total=None, want=INT_FIELDS + FLT_FIELDS,
          groups=True, over=None):
    """One raw library call.  Returns (status, dict): the wanted fields, hist, n, n_bad, sums (pre-filled with sentinels)."""
    from efa_xray_amd import _lib
    ctx = _ctx()
    X = np.ascontiguousarray(X)
    rows, M = X.shape
    ncol = rows // max(n_lead, 1)
    sg = np.ascontiguousarray(slab_group, dtype=np.int32)
    G = max(int(sg.max()) + 1, 0) if sg.size else 0
    Xd = ctx.to_device(X, X.dtype)
    yd = ctx.to_device(np.ascontiguousarray(y, dtype=np.float64))
    wd = None if w is None else ctx.to_device(np.ascontiguousarray(w, dtype=np.float64))
    ibuf = dict((f, ctx.malloc_bytes(4 * max(rows, 1))) for f in INT_FIELDS)
    fbuf = dict((f, ctx.to_device(np.full(max(rows, 1), SENT_F))) for f in FLT_FIELDS)
    for f in INT_FIELDS:
        ctx.h2d(ibuf[f], np.full(max(rows, 1), SENT_I, dtype=np.int32))
    hist = np.full((max(G, 1), M + 1), SENT_I, dtype=np.int64)
    n = np.full(max(G, 1), SENT_I, dtype=np.int64)
    n_bad = np.full(max(G, 1), SENT_I, dtype=np.int64)
    sums = np.full((max(G, 1), 5), SENT_F)
    llp = ctypes.POINTER(ctypes.c_longlong)
    a = dict(ctx=ctx.handle, rows=rows, M=M, X=Xd.ptr, y=yd.ptr, ncol=ncol, n_lead=n_lead, col_offset=col_offset,
             ncol_total=ncol if ncol_total is None else ncol_total, sg=sg.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
             hist=hist.ctypes.data_as(llp) if groups else None, n=n.ctypes.data_as(llp) if groups else None,
             n_bad=n_bad.ctypes.data_as(llp) if groups else None, sums=_lib._dp(sums) if groups else None)
    a.update(over or {})
    fn = ctx.lib.efa_verify_f32_dev if X.dtype == np.float32 else ctx.lib.efa_verify_dev
    st = fn(a["ctx"], a["rows"], a["M"], a["X"], a["y"], a["ncol"], a["n_lead"], a["col_offset"], a["ncol_total"], a["sg"],
            None if wd is None else wd.ptr, 1 if fair else 0, ctypes.c_uint64(seed),
            *[ibuf[f] if f in want else None for f in INT_FIELDS], *[fbuf[f].ptr if f in want else None for f in FLT_FIELDS],
            a["hist"], a["n"], a["n_bad"], a["sums"])
    out = dict(hist=hist[:G], n=n[:G], n_bad=n_bad[:G], sums=sums[:G], raw=(hist, n, n_bad, sums))
    for f in INT_FIELDS:
        host = np.empty(max(rows, 1), dtype=np.int32)
        ctx.d2h(host, ibuf[f])
        out[f] = host[:rows]
        ctx.free_bytes(ibuf[f])
    for f in FLT_FIELDS:
        out[f] = fbuf[f].download()[:rows]
        fbuf[f].free()
    for d in (Xd, yd, wd):
        if d is not None:
            d.free()
    return st, out


def _same_bits(a, b, names=INT_FIELDS + FLT_FIELDS + ("hist", "n", "n_bad", "sums"), rows=None):
    for f in names:
        x, y = a[f], b[f]
        if rows is not None and f in INT_FIELDS + FLT_FIELDS:
            x, y = x[rows], y[rows]
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), f


def _check_ints(out, m):
    for f in INT_FIELDS + ("hist", "n", "n_bad"):
        assert np.array_equal(out[f], m[f]), f


def _row_bounds(m, M):
    mad = m["mean_abs_d"]
    b_crps = (2 * M + 8) * U * mad
    b_err = (M + 4) * U * mad
    b_var = (4 * M + 16) * U * (m["var"] + m["err"] ** 2 * M / (M - 1.0))
    return b_crps, b_err, b_var


def _check_floats(out, m, M, n_lead, w=None, label="", underflow=()):
    """Fields and group sums within the bounds of the module docstring; returns the largest ratio to each bound.  `underflow`:
    rows of subnormal d, where a relative bound says nothing (their integers are checked, their floats are not)."""
    good = m["rank"] >= 0
    bc, be, bv = _row_bounds(m, M)
    ratios = {}
    cmp = good.copy()
    cmp[list(underflow)] = False
    for f, b in (("crps", bc), ("err", be), ("var", bv)):
        assert np.array_equal(np.isnan(out[f]), ~good), f
        diff = np.abs(out[f][cmp] - m[f][cmp])
        tiny = b[cmp] == 0.0
        assert np.all(diff[tiny] == 0.0), f
        r = np.max(diff[~tiny] / b[cmp][~tiny]) if np.any(~tiny) else 0.0
        ratios[f] = r
        assert r <= 1.0, (f, r)
    ncol = good.size // n_lead
    wr = np.ones(good.size) if w is None else np.tile(w, n_lead)
    sg = np.repeat(np.asarray(m["slab_group"]), ncol)
    for g in range(m["sums"].shape[0]):
        sel = good & (sg == g)
        rowb = np.array([0.0, np.sum(wr[sel] * bc[sel]), np.sum(wr[sel] * be[sel]),
                         np.sum(wr[sel] * (2.0 * np.abs(m["err"][sel]) + be[sel]) * be[sel]), np.sum(wr[sel] * bv[sel])])
        bound = (m["n"][g] + 4) * U * m["abs_sums"][g] + rowb
        diff = np.abs(out["sums"][g] - m["sums"][g])
        assert np.all(diff <= bound), (g, diff, bound)
        ratios["sums"] = max(ratios.get("sums", 0.0), float(np.max(diff[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0)
    print("%s M=%d ratios to the bounds: %s" % (label, M, ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    return ratios


def _model(X, y, n_lead, sg, **kw):
    m = vm.model(X, y, n_lead, sg, **kw)
    m["slab_group"] = list(sg)
    return m


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", MEMBERS)
def test_against_the_model(M, dtype):
    """Cases 1 and 2: every M, both element types; integers exact, floats within their forward bounds."""
    X, y = vm.make_case(1000 + M, N_LEAD, NCOL, M, dtype)
    sg = [0, 0, 1, 1]
    for fair in (False, True):
        st, out = _call(X, y, sg, N_LEAD, fair=fair, seed=M)
        assert st == 0
        m = _model(X, y, N_LEAD, sg, fair=fair, seed=M)
        assert m["equal"].max() >= 1        # the case has ties
        _check_ints(out, m)
        _check_floats(out, m, M, N_LEAD, label="%s fair=%d" % (np.dtype(dtype).name, fair))


@pytest.mark.parametrize("M", [2, 9, 100, 256])
def test_one_row_and_many_tiles(M):
    """rows = 1, and a slab of 133 columns: nine tiles, so the waves of a workgroup take two and three trips."""
    X, y = vm.make_case(7, 1, 1, M)
    st, out = _call(X, y, [0], 1)
    assert st == 0
    m = _model(X, y, 1, [0])
    _check_ints(out, m)
    _check_floats(out, m, M, 1)
    X, y = vm.make_case(8, 2, 133, M)
    st, out = _call(X, y, [1, 0], 2, seed=5)
    assert st == 0
    m = _model(X, y, 2, [1, 0], seed=5)
    _check_ints(out, m)
    _check_floats(out, m, M, 2)


@pytest.mark.parametrize("M", [3, 8])
def test_several_chunks_per_slab(M):
    """A slab of 1100 columns is 69 tiles: two chunks, the second of five tiles with a last tile of 12 rows, so the reduce adds
    several partials per slab; with the grid capped at one workgroup the bits are the same."""
    ncol = 1100
    X, y = vm.make_case(40 + M, 3, ncol, M)
    sg = [1, 0, 1]
    w = np.random.default_rng(M).uniform(0.5, 1.5, ncol)
    st, out = _call(X, y, sg, 3, w=w, seed=2)
    assert st == 0
    m = _model(X, y, 3, sg, col_weight=w, seed=2)
    _check_ints(out, m)
    _check_floats(out, m, M, 3, w=w, label="1100 columns")
    ctx = _ctx()
    ctx.set_option("verify_blocks", 1)
    try:
        st, capped = _call(X, y, sg, 3, w=w, seed=2)
    finally:
        ctx.set_option("verify_blocks", 0)
    assert st == 0
    _same_bits(out, capped)


def _edge_rows(M, rng):
    base = np.sort(rng.standard_normal(M)) + np.arange(M) * 1e-3
    rows, ys = [], []

    def add(x, y):
        rows.append(np.asarray(x, dtype=np.float64))
        ys.append(y)
    add(base, base[0] - 1.0)                      # y below all
    add(base, base[-1] + 1.0)                     # above all
    add(base, base[0])                            # equal to the minimum
    add(base, base[-1])                           # equal to the maximum
    add(np.full(M, 0.1), 0.1)                     # all equal to y
    add(np.full(M, 0.1), 0.3)                     # all equal, not y
    z = np.where(np.arange(M) % 2 == 0, 0.0, -0.0)
    add(z, -0.0)                                  # +-0.0 mixtures
    add(np.where(np.arange(M) % 3 == 0, 1.0, z), 0.0)
    add(np.arange(M) * 5e-324 - 3 * 5e-324, 5e-324)       # subnormals
    add(np.round(rng.standard_normal(M), 1), 0.1)          # quantised, many ties
    add(np.round(rng.standard_normal(M) * 0.3, 1), 0.0)
    add(base, 0.05)                               # ascending
    add(base[::-1], 0.05)                         # descending
    add(np.concatenate([base[::2], base[1::2][::-1]]), 0.05)   # already bitonic
    return np.array(rows), np.array(ys)


@pytest.mark.parametrize("M", [2, 3, 8, 17, 33, 100, 256])
def test_edge_rows(M):
    """Case 3: exact on the integers; the all-equal rows have crps 0 and var 0.0 exactly."""
    X, y = _edge_rows(M, np.random.default_rng(M))
    st, out = _call(X, y, [0], 1, seed=11)
    assert st == 0
    m = _model(X, y, 1, [0], seed=11)
    _check_ints(out, m)
    _check_floats(out, m, M, 1, underflow=(8,))
    assert out["equal"][4] == M and out["crps"][4] == 0.0 and out["var"][4] == 0.0 and out["err"][4] == 0.0
    assert out["equal"][5] == 0 and out["var"][5] == 0.0
    assert out["below"][0] == 0 and out["rank"][0] == 0 and out["rank"][1] == M
    assert out["equal"][6] == M


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [7, 32, 33, 100, 256])
def test_poisoned_rows(M, dtype):
    """Case 4: a NaN / inf member at the first, the last and the last real slot, an overflowing d, a NaN y: -1 and NaN in exactly
    that row, n_bad (or nothing) goes up, every other row and group output keeps its bits."""
    X, y = vm.make_case(2000 + M, N_LEAD, NCOL, M, dtype)
    sg = [0, 1, 1, 0]
    st, clean = _call(X, y, sg, N_LEAD, seed=3)
    assert st == 0
    big = np.finfo(dtype).max
    poisons = [(5, 0, np.nan), (40, M - 1, np.inf), (77, M - 1, -np.inf), (100, (M - 1) // 8 * 8, np.nan), (130, M // 2, np.inf)]
    Xp, yp = X.copy(), y.copy()
    for r, s, v in poisons:
        Xp[r, s] = v
    over = [20] if dtype == np.float64 else []   # (a float32 member cannot make x - y overflow in float64)
    for r in over:
        Xp[r, 1] = big
        yp[r] = -big                             # d overflows
    yp[60] = np.nan                              # not verified
    st, out = _call(Xp, yp, sg, N_LEAD, seed=3)
    assert st == 0
    hit = np.array([r for r, _, _ in poisons] + over + [60])
    for f in INT_FIELDS:
        assert np.all(out[f][hit] == -1)
    for f in FLT_FIELDS:
        assert np.all(np.isnan(out[f][hit]))
    keep = np.ones(X.shape[0], dtype=bool)
    keep[hit] = False
    _same_bits(out, clean, INT_FIELDS + FLT_FIELDS, rows=keep)
    m = _model(Xp, yp, N_LEAD, sg, seed=3)
    _check_ints(out, m)
    assert out["n_bad"].sum() == hit.size - 1 and out["n"].sum() == clean["n"].sum() - hit.size
    # the group sums: those of the run in which the same rows are simply not verified
    y2 = y.copy()
    y2[hit] = np.nan
    st, ref = _call(X, y2, sg, N_LEAD, seed=3)
    assert st == 0
    _same_bits(out, ref, ("hist", "n", "sums"))


@pytest.mark.parametrize("M", [9, 64, 100])
def test_member_permutation(M):
    """Case 5."""
    X, y = vm.make_case(31 + M, N_LEAD, NCOL, M)
    sg = [0] * N_LEAD
    st, a = _call(X, y, sg, N_LEAD, seed=2)
    perm = np.random.default_rng(M).permutation(M)
    st2, b = _call(X[:, perm], y, sg, N_LEAD, seed=2)
    assert st == 0 and st2 == 0
    _same_bits(a, b, INT_FIELDS + ("hist", "n", "n_bad"))
    m = _model(X, y, N_LEAD, sg, seed=2)
    _check_floats(b, m, M, N_LEAD, label="permuted")


@pytest.mark.parametrize("k", [-40, 7, 100])
@pytest.mark.parametrize("M", [8, 33, 100])
def test_scaling_by_a_power_of_two(M, k):
    """Case 6: crps and err scale exactly, var by 4^k; the integers do not move."""
    rng = np.random.default_rng(1000 + M + k)
    X = 3.0 + rng.standard_normal((N_LEAD * NCOL, M))
    y = 3.0 + rng.standard_normal(N_LEAD * NCOL)
    sg = [0] * N_LEAD
    st, a = _call(X, y, sg, N_LEAD)
    st2, b = _call(np.ldexp(X, k), np.ldexp(y, k), sg, N_LEAD)
    assert st == 0 and st2 == 0
    _same_bits(a, b, INT_FIELDS + ("hist", "n", "n_bad"))
    assert np.array_equal(np.ldexp(a["crps"], k), b["crps"]) and np.array_equal(np.ldexp(a["err"], k), b["err"])
    assert np.array_equal(np.ldexp(a["var"], 2 * k), b["var"])


@pytest.mark.parametrize("M", [9, 100])
def test_column_shards(M):
    """Case 7."""
    X, y = vm.make_case(400 + M, N_LEAD, NCOL, M)
    sg = [0, 1, 0, 1]
    st, whole = _call(X, y, sg, N_LEAD, seed=77)
    assert st == 0
    X3, y2 = X.reshape(N_LEAD, NCOL, M), y.reshape(N_LEAD, NCOL)
    parts = []
    for c0, c1 in ((0, 20), (20, 39)):
        st, p = _call(X3[:, c0:c1].reshape(-1, M), y2[:, c0:c1].reshape(-1), sg, N_LEAD, seed=77, col_offset=c0, ncol_total=NCOL)
        assert st == 0
        parts.append((c0, c1, p))
    for f in INT_FIELDS + FLT_FIELDS:
        glued = np.concatenate([p[f].reshape(N_LEAD, c1 - c0) for c0, c1, p in parts], axis=1).reshape(-1)
        assert np.array_equal(glued.view(np.uint8), whole[f].view(np.uint8)), f
    for f in ("hist", "n", "n_bad"):
        assert np.array_equal(parts[0][2][f] + parts[1][2][f], whole[f]), f


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_groups_and_weights(dtype):
    """Case 8: the three groupings, a slab of group -1, a zero-weight column; weighted sums against the model."""
    M = 20
    X, y = vm.make_case(55, N_LEAD, NCOL, M, dtype)
    w = np.cos(np.linspace(-1.2, 1.2, NCOL))
    w[4] = 0.0
    for sg in ([0, 0, 1, 1], [0, 1, 2, 3], [0, 0, 0, 0], [1, -1, 0, 1], [-1, -1, -1, -1]):
        st, out = _call(X, y, sg, N_LEAD, w=w, seed=9)
        assert st == 0
        m = _model(X, y, N_LEAD, sg, col_weight=w, seed=9)
        _check_ints(out, m)
        _check_floats(out, m, M, N_LEAD, w=w, label=str(sg))
        assert np.all(out["rank"].reshape(N_LEAD, NCOL)[:, 4] == -1)
        for lead, g in enumerate(sg):
            if g < 0:
                assert np.all(out["rank"].reshape(N_LEAD, NCOL)[lead] == -1)
                assert np.all(np.isnan(out["crps"].reshape(N_LEAD, NCOL)[lead]))


def test_grid_trips_repeats_and_state():
    """Case 9: a lowered grid cap and a repeated call give the same bits; the context's later cycles are not disturbed."""
    ctx = _ctx()
    M = 33
    X, y = vm.make_case(91, 6, 133, M)
    sg = [0, 1, 2, 0, 1, 2]
    st, a = _call(X, y, sg, 6, seed=4)
    st2, b = _call(X, y, sg, 6, seed=4)
    assert st == 0 and st2 == 0
    _same_bits(a, b)
    assert ctx.get_option("verify_us") >= 0
    for cap in (1, 2, 5):
        ctx.set_option("verify_blocks", cap)
        try:
            st, c = _call(X, y, sg, 6, seed=4)
        finally:
            ctx.set_option("verify_blocks", 0)
        assert st == 0
        _same_bits(a, c)
    _check_ints(a, _model(X, y, sg=sg, n_lead=6, seed=4))


def _toy(seed=0, M=20, n=16, nobs=40):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(seed)
    lat, lon = np.meshgrid(np.linspace(30, 45, n), np.linspace(250, 265, n), indexing="ij")
    yy, xx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    modes = np.array([np.sin(0.3 * (a * yy + b * xx) + c) for a, b, c in ((1, 0, 0), (0, 1, 1), (1, 1, 2), (1, -1, 3), (2, 1, 4))])
    coef = rng.standard_normal((modes.shape[0], M + 1))
    fields = np.tensordot(coef.T, modes, axes=1)           # (M + 1, n, n)
    truth = fields[0]
    members = np.moveaxis(fields[1:], 0, -1)[None, None]   # (1, 1, n, n, M)
    prior = EnsembleState.from_array(members, lat, lon, varnames=["t"])
    obs = []
    for k in range(nobs):
        iy, ix = rng.integers(0, n, size=2)
        obs.append(Observation(value=float(truth[iy, ix] + 0.05 * rng.standard_normal()), time=prior.ensemble_times()[0],
                               lat=float(lat[iy, ix]), lon=float(lon[iy, ix]), obtype="t", error=0.0025, assimilate_this=True))
    return prior, obs, truth


def test_end_to_end_and_posteriors_unchanged():
    """Cases 9 (third point) and 11: the update reduces the rmse of the mean against the truth the obs were drawn from, both
    through the public API; and an update after a verification call gives the bits of the update before it."""
    from efa_xray_amd import EnSRF, ensemble_verification
    prior, obs, truth = _toy()
    post1, _ = EnSRF(prior, obs, loc=False).update()
    ver = {"t": truth[None]}
    a = ensemble_verification(prior, ver, fields=("rank", "crps"))
    b = ensemble_verification(post1, ver, by=None, fair=True, weights=np.ones(truth.shape))
    assert b["rmse"][0] < a["rmse"][0]
    assert a["groups"] == ["t"] and b["groups"] == [None]
    assert a["hist"].shape == (1, 21) and a["hist"].sum() == a["n"][0] == 256 and a["n_bad"][0] == 0
    assert sorted(a["fields"]) == ["crps", "rank"] and b["fields"] == {}
    assert a["fields"]["rank"].shape == (1, 1, 16, 16) and a["fields"]["rank"].dtype == np.int32
    assert np.array_equal(np.bincount(a["fields"]["rank"].reshape(-1), minlength=21), a["hist"][0])
    assert abs(a["fields"]["crps"].mean() - a["crps"][0]) <= 1e-12 * a["crps"][0]
    for key in ("crps", "bias", "rmse", "spread", "spread_skill", "outlier_fraction"):
        assert a[key].shape == (1,) and np.isfinite(a[key][0]), key
    post2, _ = EnSRF(prior, obs, loc=False).update()
    assert np.array_equal(post1.to_vect(), post2.to_vect())


def test_invalid_arguments_leave_the_outputs_untouched():
    """Case 10."""
    M = 8
    X, y = vm.make_case(3, N_LEAD, NCOL, M)
    sg = [0, 0, 1, 1]
    rows = X.shape[0]
    bad_sg = (ctypes.c_int * 4)(0, -2, 1, 1)
    cases = [dict(ctx=None), dict(X=None), dict(y=None), dict(sg=None), dict(M=1), dict(M=257), dict(rows=rows - 1),
             dict(ncol=NCOL + 1), dict(col_offset=-1), dict(col_offset=1), dict(ncol_total=NCOL - 1), dict(sg=bad_sg),
             dict(hist=None), dict(n=None), dict(n_bad=None), dict(sums=None)]
    for over in cases:
        st, out = _call(X, y, sg, N_LEAD, over=over)
        assert st == -1, over               # EFA_ERR_INVALID
        for f in INT_FIELDS:
            assert np.all(out[f] == SENT_I), (over, f)
        for f in FLT_FIELDS:
            assert np.all(out[f] == SENT_F), (over, f)
        hist, n, n_bad, sums = out["raw"]
        assert np.all(hist == SENT_I) and np.all(n == SENT_I) and np.all(n_bad == SENT_I) and np.all(sums == SENT_F), over
    # all four group outputs NULL: fields only
    st, out = _call(X, y, sg, N_LEAD, groups=False)
    assert st == 0 and np.all(out["raw"][0] == SENT_I)
    _check_ints(dict(out, hist=vm.model(X, y, N_LEAD, sg)["hist"], n=vm.model(X, y, N_LEAD, sg)["n"],
                     n_bad=vm.model(X, y, N_LEAD, sg)["n_bad"]), vm.model(X, y, N_LEAD, sg))
    # a field that is not asked for is not written
    st, out = _call(X, y, sg, N_LEAD, want=("rank", "crps"))
    assert st == 0 and np.all(out["below"] == SENT_I) and np.all(out["var"] == SENT_F) and np.all(out["rank"] >= 0)
