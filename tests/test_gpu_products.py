"""Ensemble products and probability verification on the MI355X: efa_products_dev / efa_products_f32_dev against
the NumPy model tests/_products.py.

prob, table, n and n_bad are compared exactly (prob bit for bit: one division of two integers).  Tolerances of the floats,
u = 2^-53, from the forward bound of an M-term sum of exact terms (DESIGN.md 7p has the derivation):
  mean      (M + 4) u mean|x|                    one M-term sum, a division
  sd^2      (4M + 16) u (var + mean^2 M/(M-1))   7o's variance bound with x for d: M squares of differences from a rounded mean
  quantile  6 u max(|x_lo|, |x_hi|), and x_lo <= value <= x_hi
  sums      (n + 8) u sum |w t|                  n - 1 roundings of the n-term sum and up to four in a term w (p - o)^2 (the
                                                 model takes p = k/M as the field has it, rounded once)"""
import ctypes

import numpy as np
import pytest

import _products as pm

pytestmark = pytest.mark.gpu

U = pm.U
MEMBERS = [2, 3, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128, 129, 255, 256]
N_LEAD = 3
QS = (0.0, 0.1, 0.5, 0.9, 1.0)
SENT_I, SENT_F = -77, -1234.5
FIELDS = ("mean", "sd", "quant", "prob")
RATIOS = {}


def _ctx():
    from efa_xray_amd import _lib
    return _lib.get_context(0)


def _call(X, n_lead, q=(), thr=None, y=None, sg=None, w=None, want=FIELDS, offset=False, outputs=True, over=None):
    """One raw library call.  Returns (status, dict): the wanted fields and table, n, n_bad, sums (all pre-filled with sentinels).
    offset: the rows start one element into their allocation (the unaligned path)."""
    from efa_xray_amd import _lib
    ctx = _ctx()
    X = np.ascontiguousarray(X)
    rows, M = X.shape
    ncol = rows // max(n_lead, 1)
    q = np.ascontiguousarray(q, dtype=np.float64)
    thr = np.zeros((n_lead, 0)) if thr is None else np.ascontiguousarray(thr, dtype=np.float64).reshape(n_lead, -1)
    Q, T = q.size, thr.shape[1]
    flat = np.concatenate([np.zeros(1 if offset else 0, dtype=X.dtype), X.reshape(-1)])
    Xd = ctx.to_device(flat, X.dtype)
    xptr = ctypes.c_void_p(Xd.ptr.value + (X.dtype.itemsize if offset else 0))
    yd = None if y is None else ctx.to_device(np.ascontiguousarray(y, dtype=np.float64))
    wd = None if w is None else ctx.to_device(np.ascontiguousarray(w, dtype=np.float64))
    sg_a = None if sg is None else np.ascontiguousarray(sg, dtype=np.int32)
    G = max(int(sg_a.max()) + 1, 0) if sg_a is not None and sg_a.size else 0
    nr = max(rows, 1)
    shapes = dict(mean=(nr,), sd=(nr,), quant=(max(Q, 1), nr), prob=(max(T, 1), nr))
    buf = dict((f, ctx.to_device(np.full(shapes[f], SENT_F))) for f in FIELDS)
    table = np.full((max(G, 1), max(T, 1), M + 1, 2), SENT_I, dtype=np.int64)
    n_bad = np.full((max(G, 1), max(T, 1)), SENT_I, dtype=np.int64)
    sums = np.full((max(G, 1), max(T, 1), 4), SENT_F)
    llp = ctypes.POINTER(ctypes.c_longlong)
    a = dict(ctx=ctx.handle, rows=rows, M=M, X=xptr, ncol=ncol, n_lead=n_lead, nq=Q, q=_lib._dp(q), nt=T, thr=_lib._dp(thr),
             y=None if yd is None else yd.ptr, sg=None if sg_a is None else sg_a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
             w=None if wd is None else wd.ptr, table=table.ctypes.data_as(llp) if outputs else None,
             n_bad=n_bad.ctypes.data_as(llp) if outputs else None, sums=_lib._dp(sums) if outputs else None)
    for f in FIELDS:
        a[f] = buf[f].ptr if f in want else None
    a.update(over or {})
    fn = ctx.lib.efa_products_f32_dev if X.dtype == np.float32 else ctx.lib.efa_products_dev
    st = fn(a["ctx"], a["rows"], a["M"], a["X"], a["ncol"], a["n_lead"], a["nq"], a["q"], a["nt"], a["thr"], a["mean"], a["sd"],
            a["quant"], a["prob"], a["y"], a["sg"], a["w"], a["table"], a["n_bad"], a["sums"])
    out = dict(raw=(table, n_bad, sums), table=table[:G, :T], n_bad=n_bad[:G, :T], sums=sums[:G, :T])
    out["n"] = out["table"].sum(axis=(2, 3))
    for f in FIELDS:
        host = buf[f].download()
        out[f] = host[:rows] if host.ndim == 1 else host[:(Q if f == "quant" else T), :rows]
        out[f + "_raw"] = host
        buf[f].free()
    for d in (Xd, yd, wd):
        if d is not None:
            d.free()
    return st, out


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _same_bits(a, b, names=FIELDS + ("table", "n_bad", "sums"), rows=None):
    for f in names:
        x, y = a[f], b[f]
        if rows is not None and f in FIELDS:
            x, y = x[..., rows], y[..., rows]
        assert np.array_equal(_bits(x), _bits(y)), f


def _note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(r))


def _ratio(diff, bound, key):
    tiny = bound == 0.0
    assert np.all(diff[tiny] == 0.0), key
    r = float(np.max(diff[~tiny] / bound[~tiny])) if np.any(~tiny) else 0.0
    _note(key, r)
    assert r <= 1.0, (key, r)


def _check(out, m, M, qs, verified=True):
    """Everything of one call against the model: integers and prob exactly, floats within the bounds of the module docstring."""
    good = ~m["bad"]
    assert np.array_equal(_bits(out["prob"]), _bits(m["prob"]))
    for f in ("mean", "sd"):
        assert np.array_equal(np.isnan(out[f]), ~good), f
    _ratio(np.abs(out["mean"][good] - m["mean"][good]), (M + 4) * U * m["mean_abs"][good], "mean")
    bvar = (4 * M + 16) * U * (m["var"][good] + m["mean"][good] ** 2 * M / (M - 1.0))
    _ratio(np.abs(out["sd"][good] ** 2 - m["var"][good]), bvar, "sd^2")
    for i, q in enumerate(qs):
        v, lo, hi = out["quant"][i], m["qlo"][i], m["qhi"][i]
        assert np.array_equal(np.isnan(v), ~good), q
        assert np.all((lo[good] <= v[good]) & (v[good] <= hi[good])), q
        _ratio(np.abs(v[good] - m["quant"][i][good]), 6 * U * np.maximum(np.abs(lo[good]), np.abs(hi[good])), "quantile")
        l, h, f = pm.levels(q, M)
        if f == 0.0:                        # q = 0, q = 1, the median of an odd M, ...: a member, bit for bit
            assert np.array_equal(_bits(v[good]), _bits(lo[good])), q
    if verified:
        for f in ("table", "n", "n_bad"):
            assert np.array_equal(out[f], m[f]), f
        bound = (m["n"][:, :, None] + 8) * U * m["abs_sums"]
        _ratio(np.abs(out["sums"] - m["sums"]).reshape(-1), bound.reshape(-1), "sums")


_CASES = {}


def _case(M, dtype, ncol=37):
    """The shared inputs and their model, computed once per (M, dtype, ncol)."""
    key = (M, np.dtype(dtype).name, ncol)
    if key not in _CASES:
        X, y, thr = pm.make_case(100 + M, N_LEAD, ncol, M, dtype)
        sg = [0, 1, 0]
        w = np.linspace(0.5, 1.5, ncol)
        m = pm.model(X, N_LEAD, quantiles=QS, thr=thr, y=y, slab_group=sg, col_weight=w)
        for a in (X, y, thr, w):
            a.setflags(write=False)
        _CASES[key] = (X, y, thr, sg, w, m)
    return _CASES[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", MEMBERS)
def test_against_the_model(M, dtype):
    X, y, thr, sg, w, m = _case(M, dtype)
    st, out = _call(X, N_LEAD, QS, thr, y, sg, w)
    assert st == 0
    _check(out, m, M, QS)
    assert m["n"].sum() == 2 * X.shape[0]
    # the SORT = false kernel: the same call without quantiles gives the same bits, and the quantile buffer is left alone
    st, plain = _call(X, N_LEAD, (), thr, y, sg, w)
    assert st == 0 and np.all(plain["quant_raw"] == SENT_F)
    _same_bits(out, plain, names=("mean", "sd", "prob", "table", "n_bad", "sums"))
    print("M=%d %s ratios so far: %s" % (M, np.dtype(dtype).name, ", ".join("%s %.3f" % kv for kv in sorted(RATIOS.items()))))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("ncol", [1, 16, 1100])
@pytest.mark.parametrize("M", [9, 100])
def test_column_counts_one_tile_and_two_chunks(M, ncol, dtype):
    X, y, thr, sg, w, m = _case(M, dtype, ncol)
    st, out = _call(X, N_LEAD, QS, thr, y, sg, w)
    assert st == 0
    _check(out, m, M, QS)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [2, 8, 33, 100, 256])
def test_rows_offset_by_one_element(M, dtype):
    X, y, thr, sg, w, m = _case(M, dtype)
    st, out = _call(X, N_LEAD, QS, thr, y, sg, w, offset=True)
    assert st == 0
    _check(out, m, M, QS)
    st, aligned = _call(X, N_LEAD, QS, thr, y, sg, w)
    _same_bits(out, aligned)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_edge_rows(dtype):
    M = 9
    X = np.zeros((6, M))
    X[0] = 0.1                                             # all members equal
    X[1] = [3, 1, 2, 2, 2, 1, 3, 3, 2]                       # integers with many ties; thresholds 2 and 3 are members
    X[2] = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0]
    X[3] = [1e308, -1e308, 1e308, -1e308, 1e308, -1e308, 1e308, -1e308, 1e308]   # sorted: 4 x -1e308, 5 x 1e308
    X[4] = -0.0
    X[5] = [7, 7, 7, 7, 8, 7, 7, 7, 7]
    if dtype == np.float32:
        X[3] = np.where(np.abs(X[3]) > 1.0, np.sign(X[3]) * 3e38, X[3])
    X = X.astype(dtype)
    big = float(np.abs(X[3].astype(np.float64)).max())
    thr = np.array([[2.0, 3.0, 0.0, -0.0]])
    qs = (0.0, 0.5, 1.0, 0.45)           # 0.45: between sorted members 3 and 4, where x_hi - x_lo overflows in row 3
    y = np.array([0.1, 2.0, 0.0, 0.0, -0.0, 7.5])
    m = pm.model(X, 1, quantiles=qs, thr=thr, y=y, slab_group=[0])
    st, out = _call(X, 1, qs, thr, y, [0])
    assert st == 0
    assert np.array_equal(_bits(out["prob"]), _bits(m["prob"]))
    assert np.array_equal(out["table"], m["table"]) and np.array_equal(out["n_bad"], m["n_bad"])
    x0 = X[0, 0].astype(np.float64)
    assert out["mean"][0] == x0 and out["sd"][0] == 0.0 and np.all(out["quant"][:, 0] == x0)
    assert out["sd"][4] == 0.0 and out["mean"][4] == 0.0 and np.all(out["quant"][:, 4] == 0.0)
    assert list(out["prob"][:, 1]) == [3 / 9, 0.0, 1.0, 1.0]            # a member equal to t does not count
    assert list(out["prob"][2:, 2]) == [1 / 9, 1 / 9] and list(out["prob"][2:, 4]) == [0.0, 0.0]   # -0.0 > 0.0 is false, both ways
    assert list(out["quant"][:3, 1]) == [1.0, 2.0, 3.0] and list(out["quant"][:3, 5]) == [7.0, 7.0, 8.0]
    assert list(out["quant"][:3, 3]) == [-big, big, big]                # f == 0: x_lo, no 0 * inf
    assert (m["qlo"][3, 3], m["qhi"][3, 3]) == (-big, big) and -big <= out["quant"][3, 3] <= big
    assert out["quant"][3, 3] == m["quant"][3, 3]
    rest = [0, 1, 2, 4, 5]
    bq = 6 * U * np.maximum(np.abs(m["qlo"][:, rest]), np.abs(m["qhi"][:, rest]))
    assert np.all(np.abs(out["quant"][:, rest] - m["quant"][:, rest]) <= bq)
    assert np.all(np.abs(out["mean"][rest] - m["mean"][rest]) <= (M + 4) * U * m["mean_abs"][rest])
    assert np.all(np.abs(out["quant"][:, 2]) <= 1.0) and list(np.abs(out["quant"][:3, 2])) == [1.0, 0.0, 1.0]
    # 1e308 in float64: the sum overflows, so mean and sd are not finite there, but the row is not bad: its probabilities count
    assert out["n_bad"].sum() == 0 and np.all(out["n"] == 6)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [9, 100])
def test_poisoned_rows_stay_in_their_rows(M, dtype):
    X, y, thr, sg, w, m = _case(M, dtype)
    st, clean = _call(X, N_LEAD, QS, thr, y, sg, w)
    rows = X.shape[0]
    hit = [0, 15, 16, rows - 1]
    Xp = X.copy()
    for i, (r, v) in enumerate(zip(hit, (np.nan, np.inf, -np.inf, np.nan))):
        Xp[r, (i * 5 + M - 1) % M] = v
    mp = pm.model(Xp, N_LEAD, quantiles=QS, thr=thr, y=y, slab_group=sg, col_weight=w)
    st, out = _call(Xp, N_LEAD, QS, thr, y, sg, w)
    assert st == 0
    for f in FIELDS:
        assert np.all(np.isnan(out[f][..., hit])), f
    assert out["n_bad"].sum() == 2 * len(hit) and np.array_equal(out["n_bad"], mp["n_bad"])
    assert np.array_equal(out["table"], mp["table"])
    others = np.setdiff1d(np.arange(rows), hit)
    _same_bits(out, clean, names=FIELDS, rows=others)
    _check(out, mp, M, QS)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_thresholds_groups_weights_and_missing_verification(dtype):
    M, ncol = 17, 37
    X, y, thr, sg, w, _ = _case(M, dtype)
    thr = np.concatenate([thr, np.full((N_LEAD, 1), np.nan)], axis=1)        # threshold 2 exists nowhere
    thr[1, 0] = np.nan                                                       # slab 1 has no threshold 0
    y = y.copy()
    y[[3, 40, 41, 100]] = [np.nan, np.inf, -np.inf, np.nan]
    w = w.copy()
    w[[0, 5, 36]] = 0.0
    sg = [1, 0, -1]
    m = pm.model(X, N_LEAD, quantiles=QS, thr=thr, y=y, slab_group=sg, col_weight=w)
    st, out = _call(X, N_LEAD, QS, thr, y, sg, w)
    assert st == 0
    _check(out, m, M, QS)
    assert np.all(np.isnan(out["prob"][2])) and np.all(np.isnan(out["prob"][0, ncol:2 * ncol]))
    assert not np.any(np.isnan(out["prob"][1])) and not np.any(np.isnan(out["mean"]))       # the fields are written all the same
    assert np.all(out["n"][:, 2] == 0) and out["n"][0, 0] == 0 and out["n"][1, 0] == ncol - 3 - 1
    assert out["n"][0, 1] == ncol - 3 - 2 and np.all(out["sums"][:, 2] == 0.0)
    # every slab switched off: fields only, empty outputs
    st, off = _call(X, N_LEAD, QS, thr, y, [-1, -1, -1], w)
    assert st == 0 and off["table"].size == 0
    _same_bits(out, off, names=FIELDS)
    # no verification at all: the same fields, host outputs untouched
    st, nov = _call(X, N_LEAD, QS, thr)
    assert st == 0 and np.all(nov["raw"][0] == SENT_I) and np.all(nov["raw"][2] == SENT_F)
    _same_bits(out, nov, names=FIELDS)
    # only some fields wanted: the others keep their sentinels
    st, some = _call(X, N_LEAD, QS, None, want=("sd", "quant"))
    assert st == 0 and np.all(some["mean_raw"] == SENT_F) and np.all(some["prob_raw"] == SENT_F)
    _same_bits(out, some, names=("sd", "quant"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_same_bits_for_every_grid_and_every_call(dtype):
    ctx = _ctx()
    X, y, thr, sg, w, m = _case(100, dtype, 1100)
    assert ctx.get_option("products_blocks") == 0
    st, ref = _call(X, N_LEAD, QS, thr, y, sg, w)
    assert st == 0 and ctx.get_option("products_us") > 0
    try:
        for blocks in (1, 2, 5, 5):
            ctx.set_option("products_blocks", blocks)
            assert ctx.get_option("products_blocks") == blocks
            st, out = _call(X, N_LEAD, QS, thr, y, sg, w)
            assert st == 0
            _same_bits(out, ref)
    finally:
        ctx.set_option("products_blocks", 0)
    st, again = _call(X, N_LEAD, QS, thr, y, sg, w)
    _same_bits(again, ref)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [3, 33, 100, 256])
def test_member_permutation_changes_nothing_sorted_or_counted(M, dtype):
    X, y, thr, sg, w, m = _case(M, dtype)
    st, ref = _call(X, N_LEAD, QS, thr, y, sg, w)
    perm = np.random.default_rng(M).permutation(M)
    st, out = _call(X[:, perm], N_LEAD, QS, thr, y, sg, w)
    assert st == 0
    _same_bits(out, ref, names=("quant", "prob", "table", "n_bad"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_python_functions_end_to_end_and_the_update_is_undisturbed(dtype):
    from efa_xray_amd import EnsembleState, EnSRF, Observation, ensemble_products, probability_verification
    rng = np.random.default_rng(11)
    nvar, nt, ny, nx, M = 2, 2, 5, 7, 20
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    arr = 280.0 + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon, varnames=["t2m", "psfc"], dtype=dtype)
    Xv = state.to_vect()

    class RowOb(Observation):
        def estimate(self, st):
            return st.to_vect()[self.row].copy()

    obs = []
    for k in range(6):
        ob = RowOb(value=280.0 + float(rng.standard_normal()), error=1.0, lat=float(lat.reshape(-1)[5 * k]),
                   lon=float(lon.reshape(-1)[5 * k]), assimilate_this=True, localize_radius=800.0)
        ob.row = 5 * k
        obs.append(ob)
    before = EnSRF(state, obs, verbose=False, loc="GC").update()[0].to_vect().copy()

    thresholds = {"t2m": [279.0, 280.5, 281.0], "psfc": [280.0]}
    qs = (0.1, 0.5, 0.9)
    out = ensemble_products(state, quantiles=qs, thresholds=thresholds)
    thr = np.full((nvar * nt, 3), np.nan)
    thr[:nt] = thresholds["t2m"]
    thr[nt:, 0] = 280.0
    truth = 280.0 + 2.0 * rng.standard_normal((nvar, nt, ny, nx))
    truth[0, 0, 0, 0] = np.nan
    wts = np.cos(np.radians(lat))
    m = pm.model(Xv, nvar * nt, quantiles=qs, thr=thr, y=truth.reshape(-1), slab_group=[0, 0, 1, 1], col_weight=wts.reshape(-1))
    shape = (nvar, nt, ny, nx)
    assert out["mean"].shape == shape and out["sd"].shape == shape and out["quantiles"].shape == (3,) + shape
    assert np.all(np.abs(out["mean"].reshape(-1) - m["mean"]) <= (M + 4) * U * m["mean_abs"])
    assert np.all(np.abs(out["quantiles"].reshape(3, -1) - m["quant"]) <= 6 * U * np.maximum(np.abs(m["qlo"]), np.abs(m["qhi"])))
    assert sorted(out["probabilities"]) == ["psfc", "t2m"]
    assert out["probabilities"]["t2m"].shape == (3, nt, ny, nx) and out["probabilities"]["psfc"].shape == (1, nt, ny, nx)
    pr = m["prob"].reshape(3, nvar, nt, ny, nx)
    assert np.array_equal(out["probabilities"]["t2m"], pr[:, 0]) and np.array_equal(out["probabilities"]["psfc"], pr[:1, 1])
    only = ensemble_products(state, mean=False, sd=False, thresholds={"psfc": [280.0]})
    assert "mean" not in only and "sd" not in only and list(only["probabilities"]) == ["psfc"]
    assert np.array_equal(only["probabilities"]["psfc"], pr[:1, 1]) and only["quantiles"].shape == (0,) + shape

    ver = probability_verification(state, {"t2m": truth[0], "psfc": truth[1]}, thresholds, by="var", weights=wts)
    assert ver["groups"] == ["t2m", "psfc"] and ver["table"].shape == (2, 3, M + 1, 2)
    assert np.array_equal(ver["table"], m["table"]) and np.array_equal(ver["n"], m["n"]) and np.array_equal(ver["n_bad"], m["n_bad"])
    assert ver["n"][0, 0] == nt * ny * nx - 1 and np.all(ver["n"][1, 1:] == 0)
    assert np.array_equal(np.isnan(ver["thresholds"]), [[False] * 3, [False, True, True]])
    for g in range(2):
        for j in range(3):
            if m["n"][g, j] == 0:
                assert np.isnan(ver["brier"][g, j]) and np.isnan(ver["reliability"][g, j])
                continue
            s = pm.scores(m["table"][g, j], m["sums"][g, j])
            for key, v in s.items():
                assert np.isclose(ver[key][g, j], v, rtol=1e-12, atol=1e-14, equal_nan=True), (key, g, j)
    # without weights the decomposition adds up to the Brier score
    flat = probability_verification(state, {"t2m": truth[0]}, {"t2m": [280.0]}, by=None)
    assert flat["groups"] == [None] and flat["n"][0, 0] == nt * ny * nx - 1
    assert abs(flat["brier"][0, 0] - (flat["reliability"][0, 0] - flat["resolution"][0, 0] + flat["uncertainty"][0, 0])) <= 1e-12

    after = EnSRF(state, obs, verbose=False, loc="GC").update()[0].to_vect()
    assert np.array_equal(_bits(before), _bits(after))


def test_invalid_arguments_leave_every_output_untouched():
    from efa_xray_amd import _lib
    ctx = _ctx()
    X, y, thr, sg, w, _ = _case(9, np.float64)
    bad_q, inf_t, low_sg = np.array([0.5, 1.5]), thr.copy(), np.array([0, -2, 0], dtype=np.int32)
    inf_t[1, 1] = np.inf
    nan_q = np.array([np.nan])
    sgp = low_sg.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    cases = [
        (dict(over=dict(ctx=None)), "null context"),
        (dict(over=dict(X=None)), "null"),
        (dict(over=dict(M=1)), "M="),
        (dict(over=dict(M=257)), "M="),
        (dict(over=dict(rows=X.shape[0] - 1)), "rows="),
        (dict(over=dict(nq=9)), "nq="),
        (dict(over=dict(nq=-1)), "nq="),
        (dict(over=dict(nt=9)), "nt="),
        (dict(over=dict(nt=-1)), "nt="),
        (dict(over=dict(q=_lib._dp(bad_q), nq=2)), "q["),
        (dict(over=dict(q=_lib._dp(nan_q), nq=1)), "q["),
        (dict(over=dict(thr=_lib._dp(inf_t))), "infinite"),
        (dict(over=dict(quant=None)), "quant_dev"),
        (dict(over=dict(prob=None, y=None)), "both null"),
        (dict(over=dict(nt=0)), "nt=0"),
        (dict(over=dict(sg=None)), "slab_group"),
        (dict(over=dict(table=None)), "go together"),
        (dict(over=dict(n_bad=None, sums=None)), "go together"),
        (dict(over=dict(sg=sgp)), "must be >= -1"),
    ]
    for kw, word in cases:
        st, out = _call(X, N_LEAD, QS, thr, y, sg, w, **kw)
        assert st == _lib.EFA_ERR_INVALID, word
        assert word.encode() in ctx.lib.efa_last_error(), (word, ctx.lib.efa_last_error())
        for f in FIELDS:
            assert np.all(out[f + "_raw"] == SENT_F), (word, f)
        table, n_bad, sums = out["raw"]
        assert np.all(table == SENT_I) and np.all(n_bad == SENT_I) and np.all(sums == SENT_F), word
    # the Python wrapper turns the status into an exception
    Xd = ctx.to_device(X)
    with pytest.raises(_lib.EfaError):
        ctx.products(X.shape[0], 9, Xd, ncol=37, n_lead=N_LEAD, quantiles=(0.5,))
    Xd.free()
    st, out = _call(X, N_LEAD, QS, thr, y, sg, w)
    assert st == 0


def test_largest_ratios_to_the_bounds_are_reported():
    """Not a check of its own: prints what the tests above saw (DESIGN.md 7p quotes it).  Runs last in this file."""
    print("largest observed error / bound: %s" % ", ".join("%s %.3f" % kv for kv in sorted(RATIOS.items())))
    assert all(v <= 1.0 for v in RATIOS.values())
