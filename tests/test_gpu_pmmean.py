"""The probability-matched mean on the MI355X: efa_pm_mean_dev / efa_pm_mean_f32_dev against the NumPy model
tests/_pmmean.py.  The result is a selection of input values, so every comparison is bit for bit (NaNs by position).

A sort block is EFA_PM_TILE_KEYS = 4096 keys and the scan takes EFA_PM_UNIT_BLOCKS = 32 blocks of one segment as a unit
(include/efa_hip.h; test_pmmean_host.py pins both): 37*41 rows of 17 members are 25 789 keys, six blocks and 1 213 keys of a
seventh; one slab of 361*720 rows of 8 members is 2 079 360 keys, 508 blocks in 16 units, and its 259 920 rank keys are 64
blocks in 2 units."""
import ctypes

import numpy as np
import pytest

import _pmmean as pmm

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -77, -1234.5
TILE, UNIT = 4096, 32
PICKS = ("min", "mid", "max", 1)


def _ctx():
    from efa_xray_amd import _lib
    return _lib.get_context(0)


def _g(pick, M):
    return {"min": 0, "mid": M // 2, "max": M - 1}.get(pick, pick)


def _call(X, f, n_lead, ny, nx, patch=None, g=None, slab_on=None, over=None):
    """One raw library call.  Returns (status, pm (rows,), n_bad (n_lead,), the state as the device holds it afterwards); pm and
    n_bad are pre-filled with sentinels."""
    ctx = _ctx()
    X = np.ascontiguousarray(X)
    rows, M = X.shape
    py, px = (ny, nx) if patch is None else patch
    Xd = ctx.to_device(X, X.dtype)
    fd = ctx.to_device(np.ascontiguousarray(f, dtype=np.float64))
    pmd = ctx.to_device(np.full(max(rows, 1), SENT_F))
    n_bad = np.full(max(n_lead, 1), SENT_I, dtype=np.int64)
    on = None if slab_on is None else np.ascontiguousarray(slab_on, dtype=np.int32)
    a = dict(ctx=ctx.handle, rows=rows, M=M, X=Xd.ptr, ny=ny, nx=nx, n_lead=n_lead, f=fd.ptr,
             on=None if on is None else on.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), py=py, px=px,
             g=M // 2 if g is None else g, pm=pmd.ptr, n_bad=n_bad.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
    a.update(over or {})
    fn = ctx.lib.efa_pm_mean_f32_dev if X.dtype == np.float32 else ctx.lib.efa_pm_mean_dev
    st = fn(a["ctx"], a["rows"], a["M"], a["X"], a["ny"], a["nx"], a["n_lead"], a["f"], a["on"], a["py"], a["px"], a["g"], a["pm"],
            a["n_bad"])
    pm = pmd.download()
    after = Xd.download()
    for d in (Xd, fd, pmd):
        d.free()
    return st, pm[:rows] if st == 0 else pm, n_bad[:n_lead] if st == 0 else n_bad, after


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _same(got, want):
    """Bit equality with NaNs matched by position."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))


def _check(X, f, n_lead, ny, nx, patch, g, slab_on=None, tag=None):
    st, pm, n_bad, after = _call(X, f, n_lead, ny, nx, patch, g, slab_on)
    assert st == 0, tag
    ref, ref_bad = pmm.model(X, f, n_lead, ny, nx, patch, g, slab_on)
    assert _same(pm, ref), tag
    assert np.array_equal(n_bad, ref_bad), tag
    assert np.array_equal(_bits(after), _bits(X)), tag                     # the state is only read
    return pm


_CASES = {}


def _case(family, n_lead, ny, nx, M, dtype, seed=0):
    key = (family, n_lead, ny, nx, M, np.dtype(dtype).name, seed)
    if key not in _CASES:
        X, f = pmm.make_case(family, 1000 + seed + 7 * M + ny, n_lead, ny, nx, M, dtype)
        X.setflags(write=False)
        f.setflags(write=False)
        _CASES[key] = (X, f)
    return _CASES[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("M", [2, 3, 17, 80, 256])
def test_parity_over_members_grids_slabs_and_patches(M, dtype):
    """Both grids with 1 and 3 slabs, the four patches each; the value families and the picks rotate through the calls."""
    i = 0
    for ny, nx in ((5, 7), (33, 17)):
        for n_lead in (1, 3):
            for patch in (None, (4, 3), (1, 1), (ny, nx)):
                family = pmm.FAMILIES[(i + M) % len(pmm.FAMILIES)]
                g = _g(PICKS[i % 4], M)
                X, f = _case(family, n_lead, ny, nx, M, dtype)
                pm = _check(X, f, n_lead, ny, nx, patch, g, tag=(ny, nx, n_lead, patch, family, g))
                if patch == (1, 1):     # a segment of one row: its sorted member g
                    assert np.array_equal(_bits(pm), _bits(np.sort(X + X.dtype.type(0), axis=1)[:, g].astype(np.float64)))
                i += 1


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", pmm.FAMILIES)
def test_every_value_family_with_every_patch_and_pick(family, dtype):
    ny, nx, n_lead, M = 33, 17, 3, 17
    X, f = _case(family, n_lead, ny, nx, M, dtype)
    ctx = _ctx()
    for patch in (None, (4, 3), (1, 1), (ny, nx)):
        for pick in PICKS:
            _check(X, f, n_lead, ny, nx, patch, _g(pick, M), tag=(family, patch, pick))
        if patch is None:
            passes = ctx.get_option("pm_passes")
            nbytes = np.dtype(dtype).itemsize
            want = {"const": 0, "lowbyte": 1, "highbyte": 1, "bits": nbytes}.get(family)
            assert want is None or passes == want, (family, passes)          # a byte with one digit costs no pass
            assert ctx.get_option("pm_us") > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_segment_of_several_blocks_and_a_part(dtype):
    ny, nx, M = 37, 41, 17
    assert TILE < ny * nx * M < UNIT * TILE and (ny * nx * M) % TILE != 0
    for family in ("bits", "precip"):
        X, f = _case(family, 1, ny, nx, M, dtype)
        _check(X, f, 1, ny, nx, None, M // 2, tag=family)
    # two slabs whose blocks do not start at a multiple of the tile, and patches of more than one block beside small ones
    X, f = _case("mixed", 2, ny, nx, M, dtype)
    _check(X, f, 2, ny, nx, None, M - 1)
    _check(X, f, 2, ny, nx, (20, 30), 0)


def test_a_segment_of_more_blocks_than_a_scan_unit():
    """One slab of 361 x 720 with 8 members: 508 blocks of pooled keys in 16 units, 64 blocks of rank keys in 2 units."""
    ny, nx, M = 361, 720, 8
    assert ny * nx * M > UNIT * TILE and ny * nx > UNIT * TILE
    rng = np.random.default_rng(5)
    X = np.round(rng.gamma(0.6, 4.0, size=(ny * nx, M)) * (rng.random((ny * nx, M)) < 0.4), 2) - 0.5 * (rng.random((ny * nx, M)) < 0.01)
    f = X.mean(axis=1)
    X[123456, 3] = np.nan
    f[7] = np.inf
    st, pm, n_bad, _ = _call(X, f, 1, ny, nx, None, M - 1)
    assert st == 0 and n_bad[0] == 2
    ref, _ = pmm.model(X, f, 1, ny, nx, None, M - 1)
    assert _same(pm, ref)
    assert np.nanmax(pm) == X[np.isfinite(X).all(axis=1) & np.isfinite(f)].max()     # Ebert's pick: the pooled maximum


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("patch", [None, (4, 3), (1, 1)])
def test_excluded_rows(patch, dtype):
    ny, nx, M, n_lead = 9, 11, 5, 3
    ncol = ny * nx
    X, f = _case("mixed", n_lead, ny, nx, M, dtype, seed=3)
    Xp, fp = X.copy(), f.copy()
    hit = [0, nx - 1, 4 * nx, ncol - 2, 5 * nx + 6, ncol + 3 * nx + 4]            # corners, edges, the interior; slab 1 too
    for i, (r, v) in enumerate(zip(hit, (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf))):
        Xp[r, (2 * i + 1) % M] = v
    fbad = [2 * nx + 2, ncol + 7, 2 * ncol + 5]
    fp[fbad] = [np.nan, np.inf, -np.inf]
    # a whole segment excluded: the patch (4, 3) at Y = 1, X = 2 of slab 2 (the whole slab would leave nothing to compare)
    whole = [2 * ncol + y * nx + x for y in range(4, 8) for x in range(6, 9)]
    Xp[whole, 0] = np.nan
    pm = _check(Xp, fp, n_lead, ny, nx, patch, 2)
    bad = sorted(set(hit + fbad + whole))
    assert np.all(np.isnan(pm[bad])) and np.count_nonzero(np.isnan(pm)) == len(bad)
    # every other element is what the model gives with those rows removed: per segment, from the rows that are left
    good = np.ones(n_lead * ncol, dtype=bool)
    good[bad] = False
    py, px = (ny, nx) if patch is None else patch
    for lead in range(n_lead):
        for cols in pmm.segments(ny, nx, py, px):
            r = lead * ncol + cols
            r = r[good[r]]
            if r.size:
                sub, _ = pmm.model(Xp[r], fp[r], 1, 1, r.size, None, 2)
                assert np.array_equal(_bits(pm[r]), _bits(sub))
    # a slab that is switched off is not read: NaN, n_bad 0, and its neighbours are what they were
    st, off, n_bad, _ = _call(Xp, fp, n_lead, ny, nx, patch, 2, slab_on=[1, 0, 1])
    assert st == 0 and np.all(np.isnan(off[ncol:2 * ncol])) and n_bad[1] == 0 and n_bad[0] == 6 and n_bad[2] == 1 + len(whole)
    assert _same(off[:ncol], pm[:ncol]) and _same(off[2 * ncol:], pm[2 * ncol:])
    st, off, n_bad, _ = _call(Xp, fp, n_lead, ny, nx, patch, 2, slab_on=[0, 0, 0])
    assert st == 0 and np.all(np.isnan(off)) and np.all(n_bad == 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ties_go_by_row_index_and_zeros_are_equal(dtype):
    ny, nx, M, n_lead = 33, 17, 3, 2
    rows = n_lead * ny * nx
    X, _ = _case("precip", n_lead, ny, nx, M, dtype)
    for patch in (None, (4, 3)):
        pm = _check(X, np.full(rows, 2.5), n_lead, ny, nx, patch, 1)
        zeros = np.where(np.arange(rows) % 2 == 0, -0.0, 0.0)
        assert np.array_equal(_bits(_check(X, zeros, n_lead, ny, nx, patch, 1)), _bits(pm))
        # a constant rank field: along the row index of a segment the result does not decrease
        for lead in range(n_lead):
            for cols in pmm.segments(ny, nx, *((ny, nx) if patch is None else patch)):
                assert np.all(np.diff(pm[lead * ny * nx + cols]) >= 0)
    # both zeros among other values: row 3 (-0.0) and row 9 (+0.0) keep their order, and so do 9 and 3 swapped
    f = np.linspace(-1.0, 1.0, rows)
    f[[3, 9]] = [-0.0, 0.0]
    a = _check(X, f, n_lead, ny, nx, None, 1)
    f[[3, 9]] = [0.0, -0.0]
    assert np.array_equal(_bits(_check(X, f, n_lead, ny, nx, None, 1)), _bits(a))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_properties_without_the_model(dtype):
    ny, nx, M, n_lead = 33, 17, 17, 2
    ncol = ny * nx
    X, f = _case("mixed", n_lead, ny, nx, M, dtype, seed=9)
    rng = np.random.default_rng(2)
    zero = X.dtype.type(0)
    for patch, g in ((None, 0), ((4, 3), 8), ((16, 16), 16)):
        st, pm, n_bad, _ = _call(X, f, n_lead, ny, nx, patch, g)
        assert st == 0 and np.all(n_bad == 0)
        for lead in range(n_lead):
            for cols in pmm.segments(ny, nx, *((ny, nx) if patch is None else patch)):
                r = lead * ncol + cols
                pool = np.sort((X[r] + zero).reshape(-1))
                assert np.array_equal(_bits(np.sort(pm[r])), _bits(pool[g::M].astype(np.float64)))
                order = r[np.argsort(f[r] + 0.0, kind="stable")]
                assert np.all(np.diff(pm[order]) >= 0)
        # the members of a row in another order: the pool is the same
        Xs = np.ascontiguousarray(np.take_along_axis(X, np.argsort(rng.random(X.shape), axis=1), axis=1))
        st, pm2, _, _ = _call(Xs, f, n_lead, ny, nx, patch, g)
        assert st == 0 and np.array_equal(_bits(pm2), _bits(pm))
        # a power of two scales every value exactly, and the order with it
        Xn = np.ascontiguousarray(rng.standard_normal(X.shape).astype(X.dtype))
        for k in (-7, 12):
            sc = X.dtype.type(2.0 ** k)
            st, a, _, _ = _call(Xn, f, n_lead, ny, nx, patch, g)
            st2, b, _, _ = _call(Xn * sc, f, n_lead, ny, nx, patch, g)
            assert st == 0 and st2 == 0 and np.array_equal(_bits(a * 2.0 ** k), _bits(b))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_same_bits_for_every_batch_and_grid(dtype):
    ctx = _ctx()
    ny, nx, M, n_lead = 37, 41, 17, 3
    X, f = _case("bits", n_lead, ny, nx, M, dtype)
    Xp = X.copy()
    Xp[50, 2] = np.nan
    assert ctx.get_option("pm_ws_bytes") == 0 and ctx.get_option("pm_blocks") == 0
    for patch in (None, (20, 30)):
        ref = _check(Xp, f, n_lead, ny, nx, patch, 5)
        try:
            for ws, blocks in ((1, 0), (1, 1), (0, 1), (0, 3), (2 * 2 * ny * nx * M * X.dtype.itemsize, 3)):
                ctx.set_option("pm_ws_bytes", ws)
                ctx.set_option("pm_blocks", blocks)
                assert ctx.get_option("pm_ws_bytes") == ws and ctx.get_option("pm_blocks") == blocks
                st, pm, n_bad, _ = _call(Xp, f, n_lead, ny, nx, patch, 5)
                assert st == 0 and np.array_equal(_bits(pm), _bits(ref)) and list(n_bad) == [1, 0, 0], (ws, blocks)
        finally:
            ctx.set_option("pm_ws_bytes", 0)
            ctx.set_option("pm_blocks", 0)


def test_python_function_on_two_variables():
    from efa_xray_amd import EnsembleState, ensemble_products, probability_matched_mean
    nvar, nt, ny, nx, M = 2, 2, 9, 13, 20
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    X, _ = pmm.make_case("precip", 77, nvar * nt, ny, nx, M)
    arr = X.reshape(nvar, nt, ny, nx, M).copy()
    arr[1, 0, 4, 6, 3] = np.nan
    for dtype in (np.float64, np.float32):
        state = EnsembleState.from_array(arr, lat, lon, varnames=["rain", "gust"], dtype=dtype)
        Xs = state.to_vect()
        mean = ensemble_products(state, sd=False)["mean"]
        for patch, pick in ((None, "mid"), ((4, 5), "max"), ((9, 13), 3)):
            out = probability_matched_mean(state, patch=patch, pick=pick)
            g = _g(pick, M)
            ref, ref_bad = pmm.model(Xs, mean.reshape(-1), nvar * nt, ny, nx, patch, g)
            ref = ref.reshape(nvar, nt, ny, nx)
            assert out["patch"] == ((ny, nx) if patch is None else patch) and out["pick"] == g
            assert sorted(out["pm_mean"]) == ["gust", "rain"]
            for iv, name in enumerate(("rain", "gust")):
                assert out["pm_mean"][name].shape == (nt, ny, nx) and _same(out["pm_mean"][name], ref[iv]), (name, patch)
                assert np.array_equal(_bits(out["rank_field"][name]), _bits(mean[iv]))
                assert np.array_equal(out["n_bad"][name], ref_bad.reshape(nvar, nt)[iv])
            assert np.isnan(out["pm_mean"]["gust"][0, 4, 6]) and list(out["n_bad"]["gust"]) == [1, 0]
        # one variable, ranked by a field of the caller's; the other is not read
        smooth = np.round(mean[0], 0)
        only = probability_matched_mean(state, variables=["rain"], patch=(4, 5), rank_field={"rain": smooth})
        fr = mean.copy()
        fr[0] = smooth
        ref, _ = pmm.model(Xs, fr.reshape(-1), nvar * nt, ny, nx, (4, 5), M // 2, slab_on=[1, 1, 0, 0])
        assert list(only["pm_mean"]) == ["rain"] and _same(only["pm_mean"]["rain"], ref.reshape(nvar, nt, ny, nx)[0])
        assert np.array_equal(only["rank_field"]["rain"], smooth)


def test_a_cycle_on_the_same_context_is_not_disturbed():
    from efa_xray_amd import EnsembleState, Observation, EnSRF, probability_matched_mean
    rng = np.random.default_rng(0)
    nvar, nt, ny, nx, M, P = 2, 1, 12, 16, 20, 24
    lat, lon = np.meshgrid(np.linspace(20, 60, ny), np.linspace(200, 280, nx), indexing="ij")
    arr = rng.standard_normal((nvar, nt, ny, nx, 1)) + 3.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon)
    Xv = state.to_vect().copy()
    pick = rng.choice(state.nstate(), P, replace=False)

    class RowOb(Observation):
        def estimate(self, st):
            return st.to_vect()[self.row].copy()

    def cycle():
        obs = []
        for k in range(P):
            col = pick[k] % (ny * nx)
            ob = RowOb(value=float(Xv[pick[k]].mean() + 0.3), error=1.0, lat=float(lat.reshape(-1)[col]),
                       lon=float(lon.reshape(-1)[col]), localize_radius=1500.0)
            ob.row = int(pick[k])
            obs.append(ob)
        post, _ = EnSRF(state, obs, verbose=False, loc="GC").update()
        return post.to_vect().copy()

    before = cycle()
    held = state.to_vect().copy()
    out = probability_matched_mean(state, patch=(5, 6), pick="max")
    assert np.all(np.isfinite(out["pm_mean"][state.vars()[0]]))
    assert np.array_equal(_bits(state.to_vect()), _bits(held))
    assert np.array_equal(_bits(cycle()), _bits(before))


def test_invalid_arguments_leave_every_output_untouched():
    from efa_xray_amd import _lib
    ctx = _ctx()
    ny, nx, n_lead, M = 5, 7, 3, 17
    X, f = _case("mixed", n_lead, ny, nx, M, np.float64)
    rows = X.shape[0]
    cases = [
        (dict(ctx=None), "null context"),
        (dict(X=None), "null"),
        (dict(f=None), "null"),
        (dict(pm=None), "null"),
        (dict(n_bad=None), "null"),
        (dict(M=1), "M="),
        (dict(M=257), "M="),
        (dict(rows=rows - 1), "rows="),
        (dict(ny=4), "rows="),
        (dict(rows=-rows, n_lead=-n_lead), "negative"),
        (dict(py=0), "py="),
        (dict(py=ny + 1), "py="),
        (dict(px=0), "px="),
        (dict(px=nx + 1), "px="),
        (dict(g=-1), "pick="),
        (dict(g=M), "pick="),
    ]
    for dtype in (np.float64, np.float32):
        for over, word in cases:
            st, pm, n_bad, _ = _call(X.astype(dtype), f, n_lead, ny, nx, (4, 3), 2, over=over)
            assert st == _lib.EFA_ERR_INVALID, word
            assert word.encode() in ctx.lib.efa_last_error(), (word, ctx.lib.efa_last_error())
            assert np.all(pm == SENT_F) and np.all(n_bad == SENT_I), word
    for key, bad in (("pm_blocks", 2049), ("pm_blocks", -1), ("pm_ws_bytes", -1), ("pm_ws_bytes", (1 << 30) + 1)):
        with pytest.raises(_lib.EfaError):
            ctx.set_option(key, bad)
    # the Python wrapper turns the status into an exception
    Xd, fd, pmd = ctx.to_device(X), ctx.to_device(f), ctx.empty((rows,))
    with pytest.raises(_lib.EfaError):
        ctx.pm_mean(rows, M, Xd, ny, nx, n_lead, fd, pmd, patch=(6, 3))
    for d in (Xd, fd, pmd):
        d.free()
