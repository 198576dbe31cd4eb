"""The ensemble Gram matrix on the MI355X: efa_gram_dev / efa_gram_f32_dev against the longdouble model
tests/_gram.py.

n, n_bad and the symmetry are exact.  The tolerance of G is derived, not measured (DESIGN.md 7q has the derivation): with
u = 2^-53, S_ab = sum c |x'_a| |x'_b|, A_a = sum_i c_i mean_m |x_im| |x'_ia| and n used rows,

    |G_ab - model| <= u ((n + 8) S_ab + (M + 6) (A_a + A_b)) / (M - 1):

an n-term sum of products in any order, and the rounded row mean carried into both factors.  sums: (n + 4) u sum |terms|.

The kernel's chunk is 32 rows of one slab; the accumulation streams are min(chunks, cap), cap = 1024 for 1, 2 and 5 member tiles
of 16, 768 for the other sizes up to 128 members and 256 above."""
import ctypes

import numpy as np
import pytest

import _gram as gm

pytestmark = pytest.mark.gpu

U = gm.U
MEMBERS = [2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 100, 128, 129, 255, 256]
N_LEAD = 3
NCOLS = (1, 16, 37, 1100)
SCALE = np.array([1.0, 0.5, 2.0])
CHUNK = 32
SENT_I, SENT_F = -77, -1234.5
RATIOS = {}


def _ctx():
    from efa_xray_amd import _lib
    return _lib.get_context(0)


def _streams(M):
    T = (M + 15) // 16
    return 256 if T > 8 else 1024 if T in (1, 2, 5) else 768


def _weights(ncol, seed=0):
    """weights in eighths, 0.25 .. 2: their sums are exact in any order"""
    return np.random.default_rng(1000 + seed).integers(2, 17, ncol) / 8.0


def _call(X, n_lead, scale, w=None, offset=False, over=None, xbuf=None):
    """One raw library call.  Returns (status, dict G, n, n_bad, sums), the outputs pre-filled with sentinels.
    offset: the rows start one element into their allocation (the unaligned path)."""
    from efa_xray_amd import _lib
    ctx = _ctx()
    X = np.ascontiguousarray(X)
    rows, M = X.shape
    ncol = rows // max(n_lead, 1)
    sc = np.ascontiguousarray(scale, dtype=np.float64)
    flat = X.reshape(-1) if xbuf is None else np.ascontiguousarray(xbuf, dtype=X.dtype)
    flat = np.concatenate([np.zeros(1 if offset else 0, dtype=X.dtype), flat])
    Xd = ctx.to_device(flat if flat.size else np.zeros(1, dtype=X.dtype), X.dtype)
    xptr = ctypes.c_void_p(Xd.ptr.value + (X.dtype.itemsize if offset else 0))
    wd = None if w is None else ctx.to_device(np.ascontiguousarray(w, dtype=np.float64))
    G = np.full((M, M), SENT_F)
    n, n_bad = ctypes.c_longlong(SENT_I), ctypes.c_longlong(SENT_I)
    sums = np.full(2, SENT_F)
    a = dict(ctx=ctx.handle, rows=rows, M=M, X=xptr, ncol=ncol, n_lead=n_lead, scale=_lib._dp(sc),
             w=None if wd is None else wd.ptr, G=_lib._dp(G), n=ctypes.byref(n), n_bad=ctypes.byref(n_bad), sums=_lib._dp(sums))
    a.update(over or {})
    fn = ctx.lib.efa_gram_f32_dev if X.dtype == np.float32 else ctx.lib.efa_gram_dev
    st = fn(a["ctx"], a["rows"], a["M"], a["X"], a["ncol"], a["n_lead"], a["scale"], a["w"], a["G"], a["n"], a["n_bad"], a["sums"])
    Xd.free()
    if wd is not None:
        wd.free()
    return st, dict(G=G, n=int(n.value), n_bad=int(n_bad.value), sums=sums)


def _same_bits(a, b, names=("G", "n", "n_bad", "sums")):
    for f in names:
        assert np.array_equal(gm.bits(np.asarray(a[f])), gm.bits(np.asarray(b[f]))), f


def _check(out, m, label):
    """Counts exact, G symmetric bit for bit and within the derived bound, sums within theirs; returns the ratio of G."""
    assert out["n"] == m["n"] and out["n_bad"] == m["n_bad"], (label, out["n"], out["n_bad"], m["n"], m["n_bad"])
    assert np.array_equal(gm.bits(out["G"]), gm.bits(np.ascontiguousarray(out["G"].T))), label
    r = gm.ratio(out["G"], m)
    print("%s: n = %d, largest |G - model| / bound = %.4f" % (label, m["n"], r))
    RATIOS["gram"] = max(RATIOS.get("gram", 0.0), r)
    assert r <= 1.0, (label, r)
    sb = (m["n"] + 4) * U * np.abs(m["sums"]).astype(np.float64)
    assert np.all(np.abs(out["sums"] - m["sums"]).astype(np.float64) <= sb), (label, out["sums"], m["sums"])
    return r


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", MEMBERS)
def test_against_the_model(M, dtype):
    for ncol in NCOLS:
        X = gm.make_rows(M * 7 + ncol, N_LEAD * ncol, M, dtype)
        w = _weights(ncol, M)
        st, out = _call(X, N_LEAD, SCALE, w)
        assert st == 0
        _check(out, gm.model(X, N_LEAD, SCALE, w), "M=%d %s ncol=%d" % (M, np.dtype(dtype).name, ncol))
        assert out["n"] == N_LEAD * ncol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [5, 100, 130])
def test_row_counts_around_the_step_and_the_chunk(M, dtype):
    for rows in (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1):
        X = gm.make_rows(M + rows, rows, M, dtype)
        st, out = _call(X, 1, [1.5])
        assert st == 0
        _check(out, gm.model(X, 1, [1.5]), "M=%d %s rows=%d" % (M, np.dtype(dtype).name, rows))


@pytest.mark.parametrize("M", [17, 100, 129])
def test_every_stream_gets_two_chunks_and_the_last_fewer(M):
    S = _streams(M)
    rows = (2 * S + S // 2) * CHUNK - 7      # 2.5 S chunks, the last one short: streams >= S/2 get two chunks, the others three
    X = gm.make_rows(M, rows, M, np.float64)
    w = _weights(rows, 3)
    if M > 32:                               # (the longdouble model of every row would take too long: one row in 16 is used,
        w[np.random.default_rng(M).random(rows) > 1.0 / 16] = 0.0     # two of every chunk on average, and its first and last)
        w[[0, rows - 1]] = 1.0
    st, out = _call(X, 1, [1.0], w)
    assert st == 0
    _check(out, gm.model(X, 1, [1.0], w), "M=%d rows=%d (%d streams)" % (M, rows, S))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [100, 129])
def test_same_bits_for_every_grid_and_every_call(M, dtype):
    ctx = _ctx()
    X = gm.make_rows(M, N_LEAD * 1100, M, dtype)
    w = _weights(1100)
    assert ctx.get_option("gram_blocks") == 0
    st, ref = _call(X, N_LEAD, SCALE, w)
    assert st == 0 and ctx.get_option("gram_us") > 0
    try:
        for blocks in (1, 2, 5, 0):
            ctx.set_option("gram_blocks", blocks)
            assert ctx.get_option("gram_blocks") == blocks
            st, out = _call(X, N_LEAD, SCALE, w)
            assert st == 0
            _same_bits(out, ref)
    finally:
        ctx.set_option("gram_blocks", 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [2, 16, 100, 256])
def test_rows_offset_by_one_element(M, dtype):
    X = gm.make_rows(M + 1, N_LEAD * 37, M, dtype)
    w = _weights(37)
    m = gm.model(X, N_LEAD, SCALE, w)
    st, al = _call(X, N_LEAD, SCALE, w)
    st2, un = _call(X, N_LEAD, SCALE, w, offset=True)
    assert st == 0 and st2 == 0
    _check(al, m, "M=%d %s aligned" % (M, np.dtype(dtype).name))
    _check(un, m, "M=%d %s one element in" % (M, np.dtype(dtype).name))
    _same_bits(un, al)       # the same doubles are staged either way


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [17, 100])
def test_large_common_offset(M, dtype):
    rng = np.random.default_rng(M)
    off = 1e6 if dtype == np.float64 else 300.0
    X = np.ascontiguousarray((off + rng.standard_normal((N_LEAD * 200, M))).astype(dtype))
    w = _weights(200)
    m = gm.model(X, N_LEAD, SCALE, w)
    st, out = _call(X, N_LEAD, SCALE, w)
    assert st == 0
    _check(out, m, "M=%d %s offset %g" % (M, np.dtype(dtype).name, off))
    # G annihilates the vector of ones
    assert np.all(np.abs(out["G"].sum(axis=1)) <= m["bound"].sum(axis=1) + U * np.abs(out["G"]).sum(axis=1))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [3, 100, 200])
def test_exact_scaling_symmetry_and_equal_members(M, dtype):
    X = gm.make_rows(M + 2, N_LEAD * 37, M, dtype)
    w = _weights(37)
    st, ref = _call(X, N_LEAD, SCALE, w)
    assert st == 0
    assert np.array_equal(gm.bits(ref["G"]), gm.bits(np.ascontiguousarray(ref["G"].T)))
    for k in (3, -5):
        st, out = _call(X * dtype(2.0 ** k), N_LEAD, SCALE, w)
        assert st == 0
        assert np.array_equal(gm.bits(out["G"]), gm.bits(ref["G"] * 4.0 ** k)), k
        _same_bits(out, ref, names=("n", "n_bad", "sums"))
    # all members equal, at values whose sum / M does not give the member back
    rows = N_LEAD * 37
    same = np.ascontiguousarray(np.repeat((0.1 * (1 + np.arange(rows)))[:, None], M, axis=1).astype(dtype))
    st, out = _call(same, N_LEAD, SCALE, w)
    assert st == 0 and out["n"] == rows and out["n_bad"] == 0
    assert np.all(out["G"] == 0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nothing_used_gives_exact_zeros(dtype):
    M, ncol = 20, 50
    poison = np.full((N_LEAD * ncol, M), np.nan, dtype=dtype)
    # every scale 0: nothing is launched; X is one element long
    st, out = _call(poison, N_LEAD, np.zeros(N_LEAD), _weights(ncol), xbuf=np.zeros(1))
    assert st == 0 and out["n"] == 0 and out["n_bad"] == 0
    assert np.all(gm.bits(out["G"]) == 0) and np.all(out["sums"] == 0.0)
    # every weight 0 (and -1, NaN): no row is used
    for wv in (0.0, -1.0, np.nan):
        st, out = _call(poison, N_LEAD, SCALE, np.full(ncol, wv))
        assert st == 0 and out["n"] == 0 and out["n_bad"] == 0, wv
        assert np.all(gm.bits(out["G"]) == 0) and np.all(out["sums"] == 0.0), wv
    st, out = _call(np.zeros((0, M), dtype=dtype), 0, np.zeros(0), None)
    assert st == 0 and out["n"] == 0 and np.all(gm.bits(out["G"]) == 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [9, 130])
def test_selection_by_scale_and_weight(M, dtype):
    ncol = 70
    X = gm.make_rows(M + 3, N_LEAD * ncol, M, dtype)
    w = _weights(ncol)
    huge = 0.5 * float(np.finfo(dtype).max)           # 1e308 / 1.7e38: finite, and its square is not
    junk = np.array([np.nan, huge, -huge, np.inf]).astype(dtype)
    # a slab of scale 0 between two used slabs: whatever it holds changes no bit and is not counted
    sc = np.array([1.0, 0.0, 2.0])
    st, ref = _call(X, N_LEAD, sc, w)
    Xj = X.copy()
    Xj[ncol:2 * ncol] = junk[np.arange(ncol * M).reshape(ncol, M) % 4]
    st2, out = _call(Xj, N_LEAD, sc, w)
    assert st == 0 and st2 == 0 and ref["n"] == 2 * ncol
    _same_bits(out, ref)
    _check(ref, gm.model(X, N_LEAD, sc, w), "M=%d %s middle slab of scale 0" % (M, np.dtype(dtype).name))
    # columns of weight 0, negative or NaN weight: the same
    cols = np.array([0, 5, 31, 32, 33, 63, 64, 69])
    w0 = w.copy()
    w0[cols] = 0.0
    st, ref = _call(X, N_LEAD, SCALE, w0)
    assert st == 0 and ref["n"] == N_LEAD * (ncol - cols.size) and ref["n_bad"] == 0
    _check(ref, gm.model(X, N_LEAD, SCALE, w0), "M=%d %s columns of weight 0" % (M, np.dtype(dtype).name))
    Xj = X.copy().reshape(N_LEAD, ncol, M)
    Xj[:, cols] = junk[np.arange(M) % 4]
    Xj = Xj.reshape(-1, M)
    for wv in (0.0, -2.0, np.nan):
        wj = w.copy()
        wj[cols] = wv
        st, out = _call(Xj, N_LEAD, SCALE, wj)
        assert st == 0
        _same_bits(out, ref)
    # an infinite weight makes the rows of its column bad: counted, and nothing added
    wi = w.copy()
    wi[cols] = np.inf
    st, out = _call(X, N_LEAD, SCALE, wi)
    assert st == 0 and out["n_bad"] == N_LEAD * cols.size
    _same_bits(out, ref, names=("G", "n", "sums"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [7, 64, 255])
def test_poisoned_rows_are_counted_and_add_nothing(M, dtype):
    rows = 38                                  # the last chunk holds rows 32 .. 37: its last group of four is rows 36, 37 and two pads
    X = gm.make_rows(M + 4, rows, M, dtype)
    w = _weights(rows)
    hit = [0, 36, 37]
    w0 = w.copy()
    w0[hit] = 0.0
    st, ref = _call(X, 1, [2.0], w0)
    assert st == 0 and ref["n"] == rows - 3 and ref["n_bad"] == 0
    _check(ref, gm.model(X, 1, [2.0], w0), "M=%d %s three rows of weight 0" % (M, np.dtype(dtype).name))
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        Xb = X.copy()
        for r in hit:
            Xb[r, (r + k) % M] = bad
        st, out = _call(Xb, 1, [2.0], w)
        assert st == 0 and out["n_bad"] == 3, (bad, out["n_bad"])
        _same_bits(out, ref, names=("G", "n", "sums"))
        assert gm.model(Xb, 1, [2.0], w)["n_bad"] == 3


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_column_shards_add_up(dtype):
    M, ncol = 33, 75
    X = gm.make_rows(5, N_LEAD * ncol, M, dtype)
    X[ncol + 3, 4] = np.nan                    # a bad row
    w = _weights(ncol)
    w[10] = 0.0
    m = gm.model(X, N_LEAD, SCALE, w)
    st, whole = _call(X, N_LEAD, SCALE, w)
    assert st == 0
    _check(whole, m, "whole")
    X3 = X.reshape(N_LEAD, ncol, M)
    for cut in (1, ncol // 2, ncol - 1):
        parts = []
        for lo, hi in ((0, cut), (cut, ncol)):
            st, out = _call(X3[:, lo:hi].reshape(-1, M), N_LEAD, SCALE, w[lo:hi])
            assert st == 0
            parts.append(out)
        both = dict(G=parts[0]["G"] + parts[1]["G"], n=parts[0]["n"] + parts[1]["n"], n_bad=parts[0]["n_bad"] + parts[1]["n_bad"],
                    sums=parts[0]["sums"] + parts[1]["sums"])
        _check(both, m, "shards cut at %d" % cut)
        assert both["n"] == whole["n"] and both["n_bad"] == whole["n_bad"] == 1
        assert both["sums"][0] == whole["sums"][0]          # weights in eighths: exact


def test_invalid_arguments_leave_every_output_untouched():
    from efa_xray_amd import _lib
    ctx = _ctx()
    X = gm.make_rows(1, N_LEAD * 37, 9, np.float64)
    w = _weights(37)

    def dp(*v):
        return np.array(v, dtype=np.float64)
    bad_scales = [dp(1.0, np.nan, 1.0), dp(1.0, np.inf, 1.0), dp(1.0, 1.0, -0.5)]
    cases = [
        (dict(ctx=None), "null context"),
        (dict(X=None), "null device pointer"),
        (dict(scale=None), "null slab_scale"),
        (dict(G=None), "null output"),
        (dict(n=None), "null output"),
        (dict(n_bad=None), "null output"),
        (dict(sums=None), "null output"),
        (dict(M=1), "M="),
        (dict(M=257), "M="),
        (dict(rows=X.shape[0] - 1), "rows="),
        (dict(ncol=36), "rows="),
    ] + [(dict(scale=_lib._dp(s)), "slab_scale[") for s in bad_scales]
    for dtype in (np.float64, np.float32):
        for over, word in cases:
            st, out = _call(X.astype(dtype), N_LEAD, SCALE, w, over=over)
            assert st == _lib.EFA_ERR_INVALID, word
            assert word.encode() in ctx.lib.efa_last_error(), (word, ctx.lib.efa_last_error())
            assert np.all(out["G"] == SENT_F) and np.all(out["sums"] == SENT_F) and out["n"] == SENT_I and out["n_bad"] == SENT_I, word
    with pytest.raises(_lib.EfaError):
        ctx.set_option("gram_blocks", 2049)
    with pytest.raises(_lib.EfaError):
        ctx.set_option("gram_us", 1)
    # the Python wrapper turns the status into an exception, and returns what the raw call returns
    Xd = ctx.to_device(X)
    with pytest.raises(_lib.EfaError):
        ctx.gram(X.shape[0], 9, Xd, SCALE, ncol=36, n_lead=N_LEAD)
    wd = ctx.to_device(w)
    G, n, n_bad, sums = ctx.gram(X.shape[0], 9, Xd, SCALE, ncol=37, n_lead=N_LEAD, col_weight=wd)
    Xd.free()
    wd.free()
    st, out = _call(X, N_LEAD, SCALE, w)
    assert st == 0
    _same_bits(dict(G=G, n=n, n_bad=n_bad, sums=sums), out)


def test_a_cycle_before_and_after_a_gram_call_returns_the_same_bits():
    from efa_xray_amd import EnsembleState, EnSRF, Observation
    rng = np.random.default_rng(11)
    nvar, nt, ny, nx, M = 2, 2, 5, 7, 20
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    arr = 280.0 + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon, varnames=["t2m", "psfc"])

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
    X = np.ascontiguousarray(state.to_vect())
    st, out = _call(X, nvar * nt, np.ones(nvar * nt))
    assert st == 0
    _check(out, gm.model(X, nvar * nt, np.ones(nvar * nt)), "between two cycles")
    after = EnSRF(state, obs, verbose=False, loc="GC").update()[0].to_vect()
    assert np.array_equal(gm.bits(before), gm.bits(after))


def test_on_the_callers_stream():
    import torch
    ctx = _ctx()
    M, ncol = 100, 300
    X = gm.make_rows(8, N_LEAD * ncol, M, np.float64)
    w = _weights(ncol)
    st, ref = _call(X, N_LEAD, SCALE, w)
    assert st == 0
    dev = torch.device("cuda:0")
    src = torch.from_numpy(X).to(dev)
    Xd = torch.full_like(src, float("nan"))
    wd = torch.from_numpy(w).to(dev)
    busy = torch.randn(1024, 1024, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for _ in range(20):
            busy = torch.tanh(busy @ busy * 1e-3)
        Xd.copy_(src)                          # the rows arrive on the caller's stream, behind its work
    ctx.set_stream(stream.cuda_stream)
    try:
        G, n, n_bad, sums = ctx.gram(N_LEAD * ncol, M, Xd.data_ptr(), SCALE, ncol=ncol, n_lead=N_LEAD, col_weight=wd.data_ptr(),
                                     f32=False)
    finally:
        ctx.use_own_stream()
    torch.cuda.synchronize()
    assert torch.isfinite(busy).all()
    _same_bits(dict(G=G, n=n, n_bad=n_bad, sums=sums), ref)


def test_largest_ratio_to_the_bound_is_reported():
    """Not a check of its own: prints what the tests above saw (DESIGN.md 7q quotes it).  Runs last in this file."""
    print("largest observed |G - model| / bound: %s" % ", ".join("%s %.4f" % kv for kv in sorted(RATIOS.items())))
    assert all(v <= 1.0 for v in RATIOS.values())
