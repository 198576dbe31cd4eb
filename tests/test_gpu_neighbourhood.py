"""Neighbourhood probabilities and the fractions skill score on the MI355X: efa_neighbourhood_dev /
efa_neighbourhood_f32_dev against the NumPy model tests/_neighbourhood.py.

nep, nmep, n and n_bad are compared exactly (the fields bit for bit: one division of two integers).  The six sums are compared
within (n + 8) u sum |w t|, u = 2^-53, the bound of the products' sums: n - 1 roundings of the n-term sum and up to four in a term
such as w (P - O)^2 (the model takes P and O as the device has them, each rounded once).

The largest radius is 64 and a tile is 16 x 64 centres: radius 64 exceeds a tile's height and every grid here, and the (40, 70)
grid makes the kernel stage the full 64-point halo."""
import ctypes

import numpy as np
import pytest

import _neighbourhood as nm

pytestmark = pytest.mark.gpu

U = nm.U
N_LEAD = 3
SENT_I, SENT_F = -77, -1234.5
FIELDS = ("nep", "nmep")
RATIOS = {}


def _ctx():
    from efa_xray_amd import _lib
    return _lib.get_context(0)


def _call(X, n_lead, ny, nx, thr, radii, shape=0, wrap=0, y=None, sg=None, w=None, want=FIELDS, offset=False, outputs=True,
          over=None):
    """One raw library call.  Returns (status, dict): the wanted fields and sums, n, n_bad (all pre-filled with sentinels).
    offset: the rows start one element into their allocation (the unaligned path)."""
    from efa_xray_amd import _lib
    ctx = _ctx()
    X = np.ascontiguousarray(X)
    rows, M = X.shape
    thr = np.ascontiguousarray(thr, dtype=np.float64).reshape(n_lead, -1)
    rad = np.ascontiguousarray(radii, dtype=np.int32)
    T, R = thr.shape[1], rad.size
    flat = np.concatenate([np.zeros(1 if offset else 0, dtype=X.dtype), X.reshape(-1)])
    Xd = ctx.to_device(flat, X.dtype)
    xptr = ctypes.c_void_p(Xd.ptr.value + (X.dtype.itemsize if offset else 0))
    yd = None if y is None else ctx.to_device(np.ascontiguousarray(y, dtype=np.float64))
    wd = None if w is None else ctx.to_device(np.ascontiguousarray(w, dtype=np.float64))
    sg_a = None if sg is None else np.ascontiguousarray(sg, dtype=np.int32)
    G = max(int(sg_a.max()) + 1, 0) if sg_a is not None and sg_a.size and y is not None else 0
    buf = dict((f, ctx.to_device(np.full((R * T, max(rows, 1)), SENT_F))) for f in FIELDS)
    sums = np.full((max(G, 1), R, T, 6), SENT_F)
    n = np.full((max(G, 1), R, T), SENT_I, dtype=np.int64)
    n_bad = np.full((max(G, 1), R, T), SENT_I, dtype=np.int64)
    llp = ctypes.POINTER(ctypes.c_longlong)
    a = dict(ctx=ctx.handle, rows=rows, M=M, X=xptr, ny=ny, nx=nx, n_lead=n_lead, nt=T, thr=_lib._dp(thr), nr=R,
             radius=rad.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), shape=shape, wrap=wrap,
             y=None if yd is None else yd.ptr, sg=None if sg_a is None else sg_a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
             w=None if wd is None else wd.ptr, sums=_lib._dp(sums) if outputs else None,
             n=n.ctypes.data_as(llp) if outputs else None, n_bad=n_bad.ctypes.data_as(llp) if outputs else None)
    for f in FIELDS:
        a[f] = buf[f].ptr if f in want else None
    a.update(over or {})
    fn = ctx.lib.efa_neighbourhood_f32_dev if X.dtype == np.float32 else ctx.lib.efa_neighbourhood_dev
    st = fn(a["ctx"], a["rows"], a["M"], a["X"], a["ny"], a["nx"], a["n_lead"], a["nt"], a["thr"], a["nr"], a["radius"], a["shape"],
            a["wrap"], a["nep"], a["nmep"], a["y"], a["sg"], a["w"], a["sums"], a["n"], a["n_bad"])
    out = dict(raw=(sums, n, n_bad), sums=sums[:G], n=n[:G], n_bad=n_bad[:G])
    for f in FIELDS:
        host = buf[f].download()
        out[f] = host[:, :rows].reshape(R, T, rows)
        out[f + "_raw"] = host
        buf[f].free()
    for d in (Xd, yd, wd):
        if d is not None:
            d.free()
    return st, out


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _same_bits(a, b, names=FIELDS + ("sums", "n", "n_bad")):
    for f in names:
        assert np.array_equal(_bits(a[f]), _bits(b[f])), f


def _check(out, m, want=FIELDS, key="sums"):
    """Everything of one call against the model: the fields bit for bit, the counts exactly, the sums within the bound."""
    for f in want:
        assert np.array_equal(_bits(out[f]), _bits(m[f])), f
    if "sums" in m:
        assert np.array_equal(out["n"], m["cnt"]) and np.array_equal(out["n_bad"], m["n_bad"])
        bound = ((m["cnt"][..., None] + 8) * U * m["abs_sums"]).reshape(-1)
        diff = np.abs(out["sums"] - m["sums"]).reshape(-1)
        tiny = bound == 0.0
        assert np.all(diff[tiny] == 0.0)
        r = float(np.max(diff[~tiny] / bound[~tiny])) if np.any(~tiny) else 0.0
        RATIOS[key] = max(RATIOS.get(key, 0.0), r)
        print("%s: error / bound %.3f" % (key, r))
        assert r <= 1.0, (key, r)


def _thr(n_lead, T, nan_slab=None):
    """T thresholds per slab around the fields' median (280), one of them a value the rounded members tie with."""
    base = np.array([280.0, 280.5, 279.3, 281.1, 279.9, 280.2, 278.8, 280.8])[:T]
    thr = np.tile(base, (n_lead, 1)) + 0.05 * np.arange(n_lead)[:, None] * (np.arange(T) != 1)
    if nan_slab is not None:
        thr[nan_slab, T // 2] = np.nan
    return thr


_CASES = {}


def _case(M, dtype, ny=6, nx=9, T=2, radii=(0, 2), shape=1, wrap=0, nan_slab=None, sg=(0, 1, 0), seed=None):
    """The shared inputs and their model, computed once per key."""
    key = (M, np.dtype(dtype).name, ny, nx, T, tuple(radii), shape, wrap, nan_slab, tuple(sg), seed)
    if key not in _CASES:
        X, y = nm.make_case(100 + M + ny if seed is None else seed, N_LEAD, ny, nx, M, dtype)
        thr = _thr(N_LEAD, T, nan_slab)
        w = np.linspace(0.5, 1.5, ny * nx)
        m = nm.model(X, N_LEAD, ny, nx, thr, list(radii), shape, bool(wrap), y=y, slab_group=list(sg), col_weight=w)
        for a in (X, y, thr, w):
            a.setflags(write=False)
        _CASES[key] = (X, y, thr, list(sg), w, m)
    return _CASES[key]


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [2, 3, 63, 64, 65, 100, 128, 129, 255, 256])
def test_members_at_the_mask_word_borders(M, dtype, offset):
    X, y, thr, sg, w, m = _case(M, dtype)
    st, out = _call(X, N_LEAD, 6, 9, thr, [0, 2], 1, 0, y, sg, w, offset=offset)
    assert st == 0
    _check(out, m)
    assert np.any(m["union"] > m["k"][None]) and np.all(m["cnt"].sum(axis=0) == X.shape[0])
    # the count-only records (no NMEP wanted) give the same NEP and sums, and the NMEP buffer is left alone
    st, plain = _call(X, N_LEAD, 6, 9, thr, [0, 2], 1, 0, y, sg, w, want=("nep",), offset=offset)
    assert st == 0 and np.all(plain["nmep_raw"] == SENT_F)
    _same_bits(out, plain, names=("nep", "sums", "n", "n_bad"))


@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("grid", [(1, 1), (1, 17), (17, 1), (15, 16), (16, 17), (33, 31)])
def test_grids_radii_and_shapes(grid, shape):
    ny, nx = grid
    for radii in ((0, 1, 2, 5), (64,)):
        X, y, thr, sg, w, m = _case(9, np.float64, ny, nx, 2, radii, shape)
        st, out = _call(X, N_LEAD, ny, nx, thr, radii, shape, 0, y, sg, w)
        assert st == 0
        _check(out, m)
    if shape == 0:      # a square that covers the grid from every centre: one value per slab
        for l in range(N_LEAD):
            for j in range(2):
                assert len(np.unique(out["nep"][0, j, l * ny * nx:(l + 1) * ny * nx])) == 1
                assert len(np.unique(out["nmep"][0, j, l * ny * nx:(l + 1) * ny * nx])) == 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_full_halo_of_radius_64(dtype):
    ny, nx, M = 40, 70, 5
    X, y, thr, sg, w, m = _case(M, dtype, ny, nx, 1, (64, 3), 1)
    st, out = _call(X, N_LEAD, ny, nx, thr, [64, 3], 1, 0, y, sg, w)
    assert st == 0
    _check(out, m)
    assert m["n"][0].max() == ny * nx and m["n"][0].min() < ny * nx        # the disc covers the grid from its middle only


@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("grid,radii", [((1, 17), (0, 8)), ((15, 16), (1, 2, 5, 7)), ((16, 17), (8, 3)), ((33, 31), (15, 0, 5)),
                                        ((17, 1), (0,)), ((3, 70), (2, 34))])
def test_wrap_in_x(grid, radii, shape):
    ny, nx = grid
    X, y, thr, sg, w, m = _case(9, np.float64, ny, nx, 2, radii, shape, 1)
    st, out = _call(X, N_LEAD, ny, nx, thr, radii, shape, 1, y, sg, w)
    assert st == 0
    _check(out, m)
    if max(radii) > 0:
        open_ = _case(9, np.float64, ny, nx, 2, radii, shape, 0)[5]
        assert not np.array_equal(open_["n"], m["n"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", [1, 4, 5, 8])
def test_threshold_counts_with_a_missing_threshold(T, dtype):
    ny, nx = 7, 11
    X, y, thr, sg, w, m = _case(33, dtype, ny, nx, T, (1, 3), 0, 0, nan_slab=1)
    st, out = _call(X, N_LEAD, ny, nx, thr, [1, 3], 0, 0, y, sg, w)
    assert st == 0
    _check(out, m)
    j = T // 2
    assert np.all(np.isnan(out["nep"][:, j, ny * nx:2 * ny * nx])) and np.all(np.isnan(out["nmep"][:, j, ny * nx:2 * ny * nx]))
    assert np.all(out["n"][1, :, j] == 0) and np.all(out["sums"][1, :, j] == 0.0)
    assert not np.any(np.isnan(out["nep"][:, j, :ny * nx]))


def test_slabs_and_batches_do_not_leak():
    """A slab whose members all exceed the threshold beside one where none do: NEP exactly 1 and 0, whatever the batches."""
    ctx = _ctx()
    ny, nx, M = 9, 20, 65
    ncol = ny * nx
    X = np.empty((4 * ncol, M))
    for l in range(4):
        X[l * ncol:(l + 1) * ncol] = 5.0 if l % 2 == 0 else -5.0
    thr = np.zeros((4, 1))
    y = X[:, 0].copy()
    radii = [0, 3, 64]
    st, ref = _call(X, 4, ny, nx, thr, radii, 0, 0, y, [0, 1, 0, 1])
    assert st == 0
    for f in FIELDS:
        for l in range(4):
            assert np.all(ref[f][:, :, l * ncol:(l + 1) * ncol] == (1.0 if l % 2 == 0 else 0.0)), (f, l)
    assert np.all(ref["n"] == 2 * ncol) and np.all(ref["sums"][1, :, 0, 1:] == 0.0) and np.all(ref["sums"][:, :, 0, 0] == 2 * ncol)
    assert np.all(ref["sums"][0, :, 0, 2:] == 2 * ncol) and np.all(ref["sums"][0, :, 0, 1] == 0.0)
    assert ctx.get_option("neighbourhood_us") > 0 and ctx.get_option("nbr_ws_bytes") == 0
    try:
        for ws, blocks in ((1, 0), (1, 1), (3 * ncol * (4 + 16), 3), (0, 1)):
            ctx.set_option("nbr_ws_bytes", ws)
            ctx.set_option("neighbourhood_blocks", blocks)
            assert ctx.get_option("nbr_ws_bytes") == ws and ctx.get_option("neighbourhood_blocks") == blocks
            st, out = _call(X, 4, ny, nx, thr, radii, 0, 0, y, [0, 1, 0, 1])
            assert st == 0
            _same_bits(out, ref)
    finally:
        ctx.set_option("nbr_ws_bytes", 0)
        ctx.set_option("neighbourhood_blocks", 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_same_bits_for_every_grid_and_batch_on_a_random_case(dtype):
    ctx = _ctx()
    ny, nx = 33, 31
    X, y, thr, sg, w, m = _case(100, dtype, ny, nx, 2, (0, 1, 2, 5), 1)
    st, ref = _call(X, N_LEAD, ny, nx, thr, [0, 1, 2, 5], 1, 0, y, sg, w)
    assert st == 0
    _check(ref, m)
    try:
        for ws, blocks in ((1, 1), (1, 5), (0, 2)):
            ctx.set_option("nbr_ws_bytes", ws)
            ctx.set_option("neighbourhood_blocks", blocks)
            st, out = _call(X, N_LEAD, ny, nx, thr, [0, 1, 2, 5], 1, 0, y, sg, w)
            assert st == 0
            _same_bits(out, ref)
    finally:
        ctx.set_option("nbr_ws_bytes", 0)
        ctx.set_option("neighbourhood_blocks", 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [0, 1])
def test_invalid_rows_leave_their_neighbours_windows(shape, dtype):
    ny, nx, M = 16, 17, 9
    ncol = ny * nx
    X, y, thr, sg, w, clean = _case(M, dtype, ny, nx, 2, (0, 1, 2, 5), shape)
    Xp, yp = X.copy(), y.copy()
    hit = [0, nx - 1, 5 * nx, ncol - 3, 7 * nx + 8, ncol + 8 * nx + 9]        # corners, edges, the interior; slab 1 too
    for i, (r, v) in enumerate(zip(hit, (np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan))):
        Xp[r, (i * 5 + M - 1) % M] = v
    ynan = [3 * nx + 3, 2 * ncol + 40]
    yp[ynan] = np.nan
    m = nm.model(Xp, N_LEAD, ny, nx, thr, [0, 1, 2, 5], shape, False, y=yp, slab_group=sg, col_weight=w)
    st, out = _call(Xp, N_LEAD, ny, nx, thr, [0, 1, 2, 5], shape, 0, yp, sg, w)
    assert st == 0
    _check(out, m)
    for f in FIELDS:
        assert np.all(np.isnan(out[f][:, :, hit + ynan])), f
        assert np.count_nonzero(np.isnan(out[f])) == 4 * 2 * (len(hit) + len(ynan))
    # a neighbour's n drops by one: the window of radius 1 around the cell next to the interior hit
    assert m["n"][1, 0, 7 * nx + 9] == clean["n"][1, 0, 7 * nx + 9] - 1
    assert np.array_equal(out["n_bad"][:, 0, 0], [5, 1]) and np.all(out["n_bad"] == out["n_bad"][:, :1])
    assert out["n"][0, 0, 0] == 2 * ncol - 5 - 2 and out["n"][1, 0, 0] == ncol - 1
    # without verif the rows whose y is NaN are valid again
    st, nov = _call(Xp, N_LEAD, ny, nx, thr, [0, 1, 2, 5], shape)
    mn = nm.model(Xp, N_LEAD, ny, nx, thr, [0, 1, 2, 5], shape, False)
    assert st == 0 and np.all(nov["raw"][0] == SENT_F) and np.all(nov["raw"][1] == SENT_I)
    _check(nov, mn)
    assert not np.any(np.isnan(nov["nep"][:, :, ynan]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [9, 80, 256])
def test_radius_0_is_the_products_probability_and_nmep_bounds_nep(M, dtype):
    ctx = _ctx()
    ny, nx = 16, 17
    X, y, thr, sg, w, m = _case(M, dtype, ny, nx, 2, (0, 2), 0)
    st, out = _call(X, N_LEAD, ny, nx, thr, [0, 2], 0)
    assert st == 0
    Xd = ctx.to_device(X, X.dtype)
    prob = ctx.to_device(np.full((2, X.shape[0]), SENT_F))
    ctx.products(X.shape[0], M, Xd, ncol=ny * nx, n_lead=N_LEAD, thresholds=thr, prob=prob)
    p = prob.download()
    Xd.free()
    prob.free()
    assert np.array_equal(_bits(out["nep"][0]), _bits(p))
    assert np.array_equal(_bits(out["nmep"][0]), _bits(p))               # one element: the union is its own count
    assert np.all(out["nmep"] >= out["nep"]) and np.any(out["nmep"][1] > out["nep"][1])
    assert np.all((out["nep"] >= 0.0) & (out["nmep"] <= 1.0))


def _blob_state(ny, nx, M, shift):
    """Members with a blob of exceedance each, jittered around a centre; the verification's blob is `shift` points further in x."""
    rng = np.random.default_rng(2)
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    X = np.zeros((ny, nx, M))
    for k in range(M):
        cy, cx = ny // 2 + rng.integers(-1, 2), nx // 3 + rng.integers(-1, 2)
        X[:, :, k] = 3.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 8.0)
    yv = 3.0 * np.exp(-((yy - ny // 2) ** 2 + (xx - nx // 3 - shift) ** 2) / 8.0)
    return X, yv


def test_fss_groups_weights_and_known_answers():
    from efa_xray_amd import EnsembleState, fractions_skill_score
    ny, nx, M, nt = 20, 31, 10, 2
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    blob, yb = _blob_state(ny, nx, M, 5)
    arr = np.empty((2, nt, ny, nx, M))
    truth = np.empty((2, nt, ny, nx))
    arr[0, :], truth[0, :] = blob, yb                                        # a displaced blob
    truth[1, :] = yb
    arr[1, :] = yb[:, :, None]                                               # a perfect forecast: every member is the truth
    state = EnsembleState.from_array(arr, lat, lon, varnames=["rain", "gust"])
    ver = {"rain": truth[0], "gust": truth[1]}
    radii = [0, 1, 3, 7]
    out = fractions_skill_score(state, ver, {"rain": [1.0], "gust": [1.0, 2.0]}, radii, by="var")
    assert out["groups"] == ["rain", "gust"] and out["fss"].shape == (2, 4, 2) and np.all(out["n"][1] == nt * ny * nx)
    assert np.all(out["fss"][1] == 1.0) and np.all(out["mse"][1] == 0.0)    # perfect, exactly, at every radius and threshold
    assert np.all(np.isnan(out["fss"][0, :, 1])) and np.all(out["n"][0, :, 1] == 0) and np.isnan(out["thresholds"][0, 1])
    f = out["fss"][0, :, 0]
    assert np.all(np.diff(f) >= 0.0) and f[0] < 0.2 and f[-1] > 0.5, f      # the displacement is forgiven as the window grows
    assert np.array_equal(out["fss_useful"], 0.5 + out["base_rate"] / 2.0, equal_nan=True) and np.all(out["n_bad"] == 0)
    # against the model, with weights, one weight 0, a NaN in the truth, per variable and time, and in one group
    wts = np.cos(np.radians(lat))
    wts[3, 4] = 0.0
    truth2 = truth.copy()
    truth2[0, 1, 2, 2] = np.nan
    ver2 = {"rain": truth2[0], "gust": truth2[1]}
    thr = np.array([[1.0, np.nan]] * nt + [[1.0, 2.0]] * nt)
    X = state.to_vect()
    for by, sg in (("var", [0, 0, 1, 1]), ("var_time", [0, 1, 2, 3]), (None, [0, 0, 0, 0])):
        m = nm.model(X, 2 * nt, ny, nx, thr, radii, 1, False, y=truth2.reshape(-1), slab_group=sg, col_weight=wts.reshape(-1))
        got = fractions_skill_score(state, ver2, {"rain": [1.0], "gust": [1.0, 2.0]}, radii, by=by, weights=wts, shape="disc")
        _check(dict(sums=got["sums"], n=got["n"], n_bad=got["n_bad"]), m, want=(), key="fss sums by=%s" % (by,))
        assert got["n"][0, 0, 0] == (nt if by != "var_time" else 1) * (ny * nx - 1) - (1 if by != "var_time" else 0) + \
            (nt * (ny * nx - 1) if by is None else 0)
        for g in range(len(got["groups"])):
            for i in range(4):
                for j in range(2):
                    if m["cnt"][g, i, j] == 0:
                        assert np.isnan(got["fss"][g, i, j])
                        continue
                    fs, mse, base, frate = nm.fss(m["sums"][g, i, j])
                    assert np.isclose(got["fss"][g, i, j], fs, rtol=1e-12, atol=1e-14) and np.isclose(got["mse"][g, i, j], mse, rtol=1e-12, atol=1e-16)
                    assert np.isclose(got["base_rate"][g, i, j], base, rtol=1e-12) and np.isclose(got["forecast_rate"][g, i, j], frate, rtol=1e-12)


def test_fss_of_disjoint_events_is_0_and_a_switched_off_group_is_not_read():
    ny, nx, M = 8, 12, 7
    ncol = ny * nx
    X = np.zeros((3 * ncol, M))
    y = np.zeros(3 * ncol)
    X[:ncol][np.arange(ncol) % 3 == 0] = 2.0          # forecast events where x % 3 == 0 ...
    y[:ncol][np.arange(ncol) % 3 == 1] = 2.0          # ... observed ones where x % 3 == 1
    X[ncol:2 * ncol] = np.nan                          # a slab of group -1, full of NaN: it is never looked at
    X[2 * ncol:] = 2.0
    y[2 * ncol:] = 2.0
    thr = np.ones((3, 1))
    st, out = _call(X, 3, ny, nx, thr, [0, 1], 0, 0, y, [0, -1, 1], want=())
    assert st == 0
    assert np.all(out["nep_raw"] == SENT_F) and np.all(out["nmep_raw"] == SENT_F)
    fs0 = nm.fss(out["sums"][0, 0, 0])[0]
    assert fs0 == 0.0 and nm.fss(out["sums"][0, 1, 0])[0] > 0.0 and nm.fss(out["sums"][1, 1, 0])[0] == 1.0
    assert np.all(out["n"] == ncol) and np.all(out["n_bad"] == 0)
    m = nm.model(X, 3, ny, nx, thr, [0, 1], 0, False, y=y, slab_group=[0, -1, 1])
    _check(out, m, want=())
    # with the fields wanted the slab is read: NaN rows, and n_bad stays 0 because its group is -1
    st, out = _call(X, 3, ny, nx, thr, [0, 1], 0, 0, y, [0, -1, 1])
    assert st == 0 and np.all(np.isnan(out["nep"][:, :, ncol:2 * ncol])) and np.all(out["n_bad"] == 0)
    _check(out, m)
    # a slab without any threshold is not read either, and its fields are NaN
    thr2 = thr.copy()
    thr2[2] = np.nan
    st, out = _call(X, 3, ny, nx, thr2, [0, 1], 0, 0, y, [0, -1, 1])
    m2 = nm.model(X, 3, ny, nx, thr2, [0, 1], 0, False, y=y, slab_group=[0, -1, 1])
    assert st == 0 and np.all(np.isnan(out["nep"][:, :, 2 * ncol:])) and np.all(out["n"][1] == 0)
    _check(out, m2)


def test_python_functions_on_two_variables():
    from efa_xray_amd import EnsembleState, neighbourhood_probabilities
    nvar, nt, ny, nx, M = 2, 2, 9, 13, 20
    rng = np.random.default_rng(4)
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    X, _ = nm.make_case(77, nvar * nt, ny, nx, M)
    arr = X.reshape(nvar, nt, ny, nx, M).copy()
    arr[1, 0, 4, 6, 3] = np.nan
    for dtype in (np.float64, np.float32):
        state = EnsembleState.from_array(arr, lat, lon, varnames=["t2m", "psfc"], dtype=dtype)
        thresholds = {"t2m": [279.5, 280.0, 280.5], "psfc": [280.2]}
        thr = np.full((nvar * nt, 3), np.nan)
        thr[:nt] = thresholds["t2m"]
        thr[nt:, 0] = 280.2
        for shape, wrap in (("square", False), ("disc", True)):
            out = neighbourhood_probabilities(state, thresholds, [0, 2, 6], shape=shape, wrap_x=wrap, nmep=True)
            m = nm.model(state.to_vect(), nvar * nt, ny, nx, thr, [0, 2, 6], 0 if shape == "square" else 1, wrap)
            assert list(out["radii"]) == [0, 2, 6] and sorted(out["nep"]) == ["psfc", "t2m"]
            for f in FIELDS:
                ref = m[f].reshape(3, 3, nvar, nt, ny, nx)
                assert out[f]["t2m"].shape == (3, 3, nt, ny, nx) and out[f]["psfc"].shape == (3, 1, nt, ny, nx)
                assert np.array_equal(_bits(out[f]["t2m"]), _bits(ref[:, :, 0])), (f, shape)
                assert np.array_equal(_bits(out[f]["psfc"]), _bits(ref[:, :1, 1])), (f, shape)
            assert np.isnan(out["nep"]["psfc"][0, 0, 0, 4, 6]) and not np.isnan(out["nep"]["psfc"][1, 0, 0, 4, 7])
        only = neighbourhood_probabilities(state, {"psfc": [280.2]}, 1, nep=False, nmep=True)
        assert "nep" not in only and list(only["nmep"]) == ["psfc"] and only["nmep"]["psfc"].shape == (1, 1, nt, ny, nx)


def test_invalid_arguments_leave_every_output_untouched():
    from efa_xray_amd import _lib
    ctx = _ctx()
    ny, nx = 6, 9
    X, y, thr, sg, w, _ = _case(9, np.float64)
    inf_t, low_sg = thr.copy(), np.array([0, -2, 0], dtype=np.int32)
    inf_t[1, 1] = -np.inf
    ip = ctypes.POINTER(ctypes.c_int)
    sgp = low_sg.ctypes.data_as(ip)

    def rad(*r):
        a = np.array(r, dtype=np.int32)
        return a, a.ctypes.data_as(ip)
    r65, rneg, r5 = rad(0, 65), rad(-1, 2), rad(0, 5)
    cases = [
        (dict(over=dict(ctx=None)), "null context"),
        (dict(over=dict(X=None)), "null"),
        (dict(over=dict(thr=None)), "null"),
        (dict(over=dict(radius=None)), "null"),
        (dict(over=dict(M=1)), "M="),
        (dict(over=dict(M=257)), "M="),
        (dict(over=dict(rows=X.shape[0] - 1)), "rows="),
        (dict(over=dict(ny=5)), "rows="),
        (dict(over=dict(rows=-X.shape[0], n_lead=-N_LEAD)), "negative"),
        (dict(over=dict(nt=0)), "nt="),
        (dict(over=dict(nt=9)), "nt="),
        (dict(over=dict(nr=0)), "nr="),
        (dict(over=dict(nr=5)), "nr="),
        (dict(over=dict(radius=r65[1])), "radius[1]"),
        (dict(over=dict(radius=rneg[1])), "radius[0]"),
        (dict(over=dict(shape=2)), "shape="),
        (dict(over=dict(shape=-1)), "shape="),
        (dict(over=dict(wrap=2)), "wrap_x="),
        (dict(over=dict(wrap=-1)), "wrap_x="),
        (dict(over=dict(wrap=1, radius=r5[1])), "2*radius+1"),
        (dict(over=dict(thr=_lib._dp(inf_t))), "infinite"),
        (dict(over=dict(nep=None, nmep=None, sums=None, n=None, n_bad=None)), "no output"),
        (dict(over=dict(nep=None, nmep=None, y=None)), "no output"),
        (dict(over=dict(sg=None)), "slab_group"),
        (dict(over=dict(sums=None)), "go together"),
        (dict(over=dict(n=None, n_bad=None)), "go together"),
        (dict(over=dict(sg=sgp)), "must be >= -1"),
    ]
    for kw, word in cases:
        st, out = _call(X, N_LEAD, ny, nx, thr, [0, 2], 1, 0, y, sg, w, **kw)
        assert st == _lib.EFA_ERR_INVALID, word
        assert word.encode() in ctx.lib.efa_last_error(), (word, ctx.lib.efa_last_error())
        for f in FIELDS:
            assert np.all(out[f + "_raw"] == SENT_F), (word, f)
        sums, n, n_bad = out["raw"]
        assert np.all(sums == SENT_F) and np.all(n == SENT_I) and np.all(n_bad == SENT_I), word
    for key, bad in (("neighbourhood_blocks", 2049), ("neighbourhood_blocks", -1), ("nbr_ws_bytes", -1), ("nbr_ws_bytes", (256 << 20) + 1)):
        with pytest.raises(_lib.EfaError):
            ctx.set_option(key, bad)
    # the Python wrapper turns the status into an exception; wrap with 2r+1 == nx is fine
    Xd = ctx.to_device(X)
    with pytest.raises(_lib.EfaError):
        ctx.neighbourhood(X.shape[0], 9, Xd, ny, nx, N_LEAD, thr, [0, 5], wrap_x=True, nep=None)
    Xd.free()
    st, out = _call(X, N_LEAD, ny, nx, thr, [0, 4], 1, 1, y, sg, w)
    assert st == 0


def test_largest_ratios_to_the_bound_are_reported():
    """Not a check of its own: prints what the tests above saw (DESIGN.md 7r quotes it).  Runs last in this file."""
    print("largest observed error / bound: %s" % ", ".join("%s %.3f" % kv for kv in sorted(RATIOS.items())))
    assert all(v <= 1.0 for v in RATIOS.values())
