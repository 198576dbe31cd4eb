"""GPU tests of float32 state storage: efa_state_cycle_f32_dev, efa_ensrf_cycle_host_f32 and
`EnSRF.update()` on a float32 state.

The yardstick of every case is the FLOAT64 path in the same process on `X32.astype(np.float64)`, rounded once with
`.astype(np.float32)`: the posterior must have its bits (`np.array_equal`), and the obs block and the five diagnostics those of
the float64 run.  That holds by construction -- the float32 kernels keep the float64 kernels' lane mapping and summation order,
and every other route runs the float64 kernels themselves on a widened workspace -- so no case here is held to anything looser.
The float64 yardstick always runs out of place.  Against the reference (the oracle on the widened inputs) the bound is
|post32 - ref| <= 2^-24 |ref| + 1e-10 max|ref row|: half a float32 ulp of the one rounding plus the project's float64 tolerance."""
import ctypes
from copy import deepcopy

import numpy as np
import pytest

from conftest import load_golden, GOLDEN_CASES

pytestmark = pytest.mark.gpu

DIAG = ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated")
F32, F64 = np.float32, np.float64


def _lib():
    from efa_xray_amd import _lib
    return _lib


def _ctx():
    return _lib().get_context(0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------
# the C entry point on resident rows
# ---------------------------------------------------------------------------
class Problem(object):
    """rows = n_lead * ny * nx float32 state rows of M members and P obs of single rows; gc: Gaspari-Cohn localised."""

    def __init__(self, seed, M, P, n_lead=1, ny=1, nx=1, gc=False, assim=None, gross=()):
        rng = np.random.default_rng(seed)
        self.M, self.P, self.n_lead, self.gc = M, P, n_lead, gc
        self.ncol = ny * nx
        self.rows = rows = n_lead * self.ncol
        lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(230, 262, nx), indexing="ij")
        self.glat, self.glon = lat.reshape(-1).copy(), lon.reshape(-1).copy()
        self.X32 = (3.0 * rng.standard_normal((rows, 1)) + 2.0 * rng.standard_normal((rows, M))).astype(F32)
        self.X64 = self.X32.astype(F64)
        pick = rng.integers(0, rows, P)
        self.HX = self.X64[pick].copy()
        self.value = self.HX.mean(axis=1) + rng.standard_normal(P)
        for k in gross:
            self.value[k] += 40.0
        self.error = rng.uniform(0.5, 1.5, P)
        self.assim = (np.arange(P) % 5 != 2) if assim is None else np.asarray(assim, dtype=bool)
        self.ob_lat, self.ob_lon = self.glat[pick % self.ncol], self.glon[pick % self.ncol]
        self.hw = rng.uniform(600.0, 1500.0, P)


def _run(pb, f32, in_place=False, offset=0, ctx=None, form="member", exact=False):
    """Phase A and the state phase; returns (posterior, diagnostics, (ym, Yp), f32_native).  The posterior: float32 rows -- those
    of the float64 call rounded once, or with `exact` that call's float64 rows as they are.  form "perts" (float64 only) is the
    perturbation form on the means and perturbations that form_perts makes of the prior on the device: the posterior is then the
    pair (means, perturbations), float64, never rounded.  A float64 call too runs in place when asked to."""
    L = _lib()
    ctx = ctx or _ctx()
    M, P, rows, n = pb.M, pb.P, pb.rows, pb.rows * pb.M
    ym = ctx.empty((max(P, 1),))
    Yp = ctx.to_device(pb.HX) if P else ctx.empty((1, M))
    if P:
        ctx.form_perts(P, M, Yp, ym, Yp)
    kw = dict(loc_mode=L.LOC_GC, ob_lat=pb.ob_lat, ob_lon=pb.ob_lon, ob_halfwidth=pb.hw) if pb.gc else {}
    diag = ctx.obs_phase(M, P, ym, Yp, pb.value, pb.error, pb.assim, **kw)
    grid = dict(grid_lat=pb.glat, grid_lon=pb.glon, n_lead=pb.n_lead) if pb.gc else {}
    native = None
    if f32:
        host = np.full(n + 4, 7.0, dtype=F32)
        host[offset:offset + n] = pb.X32.reshape(-1)
        buf = ctx.empty((n + 4,), F32).upload(host)
        out = buf if in_place else ctx.empty((n + 4,), F32).upload(np.full(n + 4, 9.0, dtype=F32))
        xin = ctypes.c_void_p(buf.address + 4 * offset)
        xout = ctypes.c_void_p(out.address + 4 * offset)
        ctx.state_cycle_f32(rows, M, xin, xout, **grid)
        native = ctx.get_option("f32_native")
        got = out.download()
        post = got[offset:offset + n].reshape(rows, M).copy()
        guard = np.ones(n + 4, dtype=bool)
        guard[offset:offset + n] = False
        assert np.all(got[guard] == (7.0 if in_place else 9.0)), "written outside the rows"
        if not in_place:
            assert _same(buf.download(), host), "the prior was written"
    elif form == "perts":
        Xd = ctx.to_device(pb.X64)
        xm, Xp = ctx.empty((rows,)), ctx.empty((rows, M))
        ctx.form_perts(rows, M, Xd, xm, Xp)
        xo, Xo = (xm, Xp) if in_place else (ctx.empty((rows,)), ctx.empty((rows, M)))
        ctx.state_phase(rows, M, xm, Xp, xo, Xo, **grid)
        post = (xo.download(), Xo.download())
    else:
        Xd = ctx.to_device(pb.X64)
        out = Xd if in_place else ctx.empty((rows, M))
        ctx.state_cycle(rows, M, Xd, out, **grid)
        post = out.download() if exact else out.download().astype(F32)
    obs_block = (ym.download(), Yp.download())
    return post, diag, obs_block, native


def _check(pb, what, native=None, variants=((False, 0), (True, 0)), ref=None):
    """float32 runs (in place / out of place, offsets) against the float64 yardstick; returns the yardstick."""
    ref = ref or _run(pb, False)
    for in_place, offset in variants:
        got = _run(pb, True, in_place, offset)
        w = "%s in_place=%r offset=%d" % (what, in_place, offset)
        bad = int(np.sum(_bits(got[0]) != _bits(ref[0])))
        assert bad == 0, "%s: %d of %d posterior values differ from fl32(float64 path)" % (w, bad, ref[0].size)
        for key in DIAG:
            assert _same(got[1][key], ref[1][key]), "%s: %s" % (w, key)
        assert _same(got[2][0], ref[2][0]) and _same(got[2][1], ref[2][1]), w + ": obs block"
        if native is not None:
            assert got[3] == native, "%s: f32_native %d, expected %d" % (w, got[3], native)
    return ref


class _settings(object):
    """Context settings for the block, back to the defaults after it."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        L, ctx, kw = _lib(), _ctx(), self.kw
        if "relax" in kw:
            ctx.set_relaxation(*kw["relax"])
        if "path" in kw:
            ctx.set_option("path", kw["path"])
        if "gc_onepass" in kw:
            ctx.set_option("gc_onepass", kw["gc_onepass"])
        if "outlier" in kw:
            ctx.set_outlier_threshold(kw["outlier"])
        if "vloc" in kw:
            ctx.set_vertical_localization(*kw["vloc"])
        return ctx

    def __exit__(self, *exc):
        L, ctx = _lib(), _ctx()
        ctx.set_relaxation(L.RELAX_NONE, 0.0)
        ctx.set_option("path", L.PATH_AUTO)
        ctx.set_option("gc_onepass", 1)
        ctx.set_outlier_threshold(None)
        ctx.set_vertical_localization(None)
        return False


TRANSFORM_M = [2, 4, 7, 20, 50, 100, 137, 256]   # AL / odd, HALF, NARROW, RTPS-fused up to 136, wide
ROWS = [5, 16, 16 * 37 + 5]


def _transform_path(M):
    return dict(path=_lib().PATH_TRANSFORM) if M > 136 else {}


@pytest.mark.parametrize("M", TRANSFORM_M)
def test_transform(M):
    """Unlocalised, member form: the transform, always on the float32 rows themselves.  (Above 136 members "auto" takes the
    transform only beyond M/2 assimilated obs: there the path is asked for.)"""
    with _settings(**_transform_path(M)):
        for rows in ROWS:
            pb = Problem(1000 + M + rows, M, 24, ny=rows)
            variants = [(False, 0), (True, 0)]
            if M % 2 == 0:   # base not 8-byte aligned with an even M: the narrower loads, not the workspace
                variants += [(False, 1), (True, 1)]
            ref = _check(pb, "transform M=%d rows=%d" % (M, rows), native=1, variants=variants)
            assert _ctx().last_timing()["path"] == _lib().PATH_TRANSFORM
            assert not _same(ref[0], pb.X32)


@pytest.mark.parametrize("M", [4, 7, 50, 100, 136, 137, 256])
@pytest.mark.parametrize("kind", ["rtps", "rtpp"])
def test_transform_relaxation(M, kind):
    """RTPP is folded into T at every size; RTPS is fused up to 136 members and takes the workspace above."""
    L = _lib()
    relax = (L.RELAX_RTPS, 0.7) if kind == "rtps" else (L.RELAX_RTPP, 0.4)
    native = 1 if (kind == "rtpp" or M <= 136) else 0
    with _settings(relax=relax, **_transform_path(M)):
        for rows in (5, 16 * 37 + 5):
            pb = Problem(2000 + M + rows, M, 24, ny=rows)
            _check(pb, "%s M=%d rows=%d" % (kind, M, rows), native=native, variants=[(False, 0), (True, 0), (True, 1)])
            assert _ctx().last_timing()["path"] == L.PATH_TRANSFORM
    # ... and it is the relaxed posterior that was compared
    plain = _run(pb, False)
    with _settings(relax=relax, **_transform_path(M)):
        assert not _same(_run(pb, False)[0], plain[0])


GRIDS = [(3, 5, 7), (1, 3, 5), (5, 9, 13), (17, 5, 7), (33, 2, 9)]   # (n_lead, ny, nx): ncol and n_lead no multiples of 16


@pytest.mark.parametrize("n_lead,ny,nx", GRIDS)
@pytest.mark.parametrize("vloc", [False, True])
def test_gc_onepass(n_lead, ny, nx, vloc):
    """One-pass GC sweep: the row-per-lane kernel on the float32 rows for an even M up to 104, the quad kernel through the workspace
    for an odd M or more members; plain and with vertical localisation."""
    for M, native in ((20, 1), (50, 1), (104, 1), (2, 1), (7, 0), (21, 0), (106, 0)):
        pb = Problem(3000 + M + n_lead, M, 40, n_lead=n_lead, ny=ny, nx=nx, gc=True)
        kw = {}
        if vloc:
            rng = np.random.default_rng(5)
            z = np.linspace(1000.0, 200.0, n_lead)
            z[n_lead // 2] = np.nan
            ov = rng.uniform(200.0, 1000.0, pb.P)
            ov[::7] = np.nan
            kw["vloc"] = (z, ov, rng.uniform(150.0, 600.0, pb.P))
        with _settings(**kw):
            ref = _check(pb, "GC M=%d grid=%r vloc=%r" % (M, (n_lead, ny, nx), vloc), native=native,
                         variants=[(False, 0), (True, 0), (True, 1)])
            assert _ctx().last_timing()["path"] == _lib().PATH_SWEEP
            assert not _same(ref[0], pb.X32)


def test_gc_onepass_long_lists_on_a_larger_ragged_grid():
    """A G8-sized ragged grid (19 x 31 = 589 columns: 36 blocks of 16 and a rest of 13; 19 slabs: one group of 16 and a rest of 3)
    with 300 obs of 600-1500 km on a 2200 x 2700 km domain: every block's active list is several times the 32 obs the kernels
    stage at a time (asserted), so the chunked list loop runs many turns.  With vertical localisation and without; M = 20 (16-byte
    loads), 50 (8-byte), an odd M and more than 104 members (quad kernel through the workspace)."""
    n_lead, ny, nx, P = 19, 19, 31, 300
    for vloc in (True, False):
        for M, native in ((20, 1), (50, 1), (21, 0), (106, 0)):
            pb = Problem(3500 + M, M, P, n_lead=n_lead, ny=ny, nx=nx, gc=True)
            cnt, _, _ = _ctx().gc_block_counts(pb.glat, pb.glon, pb.ob_lat, pb.ob_lon, pb.hw, pb.assim)
            assert cnt.min() > 2 * 32, cnt.min()
            kw = {}
            if vloc:
                rng = np.random.default_rng(6)
                z = np.linspace(1000.0, 100.0, n_lead)
                z[7] = np.nan
                ov = rng.uniform(100.0, 1000.0, P)
                ov[::9] = np.nan
                kw["vloc"] = (z, ov, rng.uniform(150.0, 500.0, P))
            with _settings(**kw):
                variants = [(True, 0)] if (vloc and M != 20) else [(False, 0), (True, 0), (True, 1)]
                ref = _check(pb, "large GC M=%d vloc=%r" % (M, vloc), native=native, variants=variants)
                assert not _same(ref[0], pb.X32)


@pytest.mark.parametrize("kind", ["rtps", "rtpp"])
def test_gc_relaxation_takes_the_workspace(kind):
    L = _lib()
    relax = (L.RELAX_RTPS, 0.7) if kind == "rtps" else (L.RELAX_RTPP, 0.4)
    for M in (20, 7):
        pb = Problem(4000 + M, M, 40, n_lead=3, ny=5, nx=7, gc=True)
        with _settings(relax=relax):
            _check(pb, "GC %s M=%d" % (kind, M), native=0)


def test_per_batch_paths_take_the_workspace():
    L = _lib()
    for M in (20, 7, 137):
        pb = Problem(5000 + M, M, 70, n_lead=3, ny=5, nx=7, gc=True)
        with _settings(gc_onepass=0):
            _check(pb, "gc_onepass=0 M=%d" % M, native=0)
        pu = Problem(5100 + M, M, 70, ny=16 * 9 + 3)
        with _settings(path=L.PATH_SWEEP):
            _check(pu, "path=sweep M=%d" % M, native=0)
            assert _ctx().last_timing()["path"] == L.PATH_SWEEP
        with _settings(path=L.PATH_SWEEP, relax=(L.RELAX_RTPP, 0.3)):
            _check(pu, "path=sweep rtpp M=%d" % M, native=0)


def test_outlier_threshold():
    """Injected gross errors are rejected alike, and the posterior is that of the obs that are left."""
    for gc in (False, True):
        kw = dict(n_lead=3, ny=5, nx=7, gc=True) if gc else dict(ny=16 * 5 + 3)
        pb = Problem(6000 + gc, 20, 40, gross=(0, 11, 23), **kw)
        with _settings(outlier=3.0):
            ref = _check(pb, "outlier gc=%r" % gc, native=1)
        assert not ref[1]["assimilated"][[0, 11, 23]].any() and ref[1]["assimilated"].sum() > 20
        assert not _same(ref[0], _run(pb, False)[0])


def test_no_assimilated_ob_leaves_the_prior_bits():
    for gc in (False, True):
        kw = dict(n_lead=3, ny=5, nx=7, gc=True) if gc else dict(ny=16 * 5 + 3)
        for M in (20, 7):
            pb = Problem(7000 + M + gc, M, 12, assim=np.zeros(12, dtype=bool), **kw)
            ref = _check(pb, "nothing assimilated gc=%r M=%d" % (gc, M), variants=[(False, 0), (True, 0), (True, 1)])
            assert _same(ref[0], pb.X32)
            p0 = Problem(7100 + M + gc, M, 0, **kw)
            assert _same(_check(p0, "no obs gc=%r M=%d" % (gc, M))[0], p0.X32)


def test_argument_checks():
    L = _lib()
    ctx = _ctx()
    pb = Problem(8000, 20, 10, n_lead=3, ny=5, nx=7, gc=True)
    _run(pb, True)
    X = ctx.empty((pb.rows * pb.M + 4,), F32)
    with pytest.raises(L.EfaError) as ei:   # an odd address
        ctx.state_cycle_f32(pb.rows, pb.M, ctypes.c_void_p(X.address + 2), X, grid_lat=pb.glat, grid_lon=pb.glon, n_lead=pb.n_lead)
    assert ei.value.status == L.EFA_ERR_INVALID
    with pytest.raises(L.EfaError) as ei:   # another M than Phase A's
        ctx.state_cycle_f32(pb.rows, pb.M + 2, X, X, grid_lat=pb.glat, grid_lon=pb.glon, n_lead=pb.n_lead)
    assert ei.value.status == L.EFA_ERR_INVALID
    field = ctx.to_device(np.tile([1.0, 0.6], (pb.rows, 1)))
    ctx.set_adaptive_inflation(field, pb.rows)
    try:
        with pytest.raises(L.EfaError) as ei:
            ctx.state_cycle_f32(pb.rows, pb.M, X, X, grid_lat=pb.glat, grid_lon=pb.glon, n_lead=pb.n_lead)
        assert ei.value.status == L.EFA_ERR_INVALID and "adaptive" in str(ei.value)
        seg = np.zeros((3, 35, 20), dtype=F32)
        with pytest.raises(L.EfaError) as ei:
            ctx.ensrf_cycle_host([seg], [seg.copy()], 35, 20, pb.HX, 16, pb.value, pb.error, pb.assim)
        assert ei.value.status == L.EFA_ERR_INVALID and "efa_ensrf_cycle_host_f32:" in str(ei.value)   # names the entry point called
        with pytest.raises(L.EfaError) as ei:
            ctx.ensrf_cycle_host([seg.astype(F64)], [seg.astype(F64)], 35, 20, pb.HX, 16, pb.value, pb.error, pb.assim)
        assert "efa_ensrf_cycle_host:" in str(ei.value)
    finally:
        ctx.set_adaptive_inflation(None)
    fresh = L.Context(0)
    try:
        with pytest.raises(L.EfaError) as ei:   # before any obs phase
            fresh.state_cycle_f32(pb.rows, pb.M, X, X)
        assert ei.value.status == L.EFA_ERR_INVALID
    finally:
        fresh.close()


# ---------------------------------------------------------------------------
# EnSRF.update() on a float32 state
# ---------------------------------------------------------------------------
def _state(seed, M, nvar=2, nt=3, ny=9, nx=13, dtype=F32):
    """ncol = 117 by default: seven blocks of 16 and a ragged rest of 5."""
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(seed)
    lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(230, 262, nx), indexing="ij")
    arr = rng.standard_normal((nvar, nt, ny, nx, 1)) + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    return EnsembleState.from_array(arr, lat, lon, validtime=np.array([0.0, 3600.0, 7200.0, 10800.0])[:nt], dtype=dtype)


def _point_obs(state, seed, P, cls=None):
    from efa_xray_amd import Observation
    rng = np.random.default_rng(seed)
    names = state.vars()
    times = [0.0, 1800.0, 3600.0, 5000.0, 7200.0] if state.ntimes() >= 3 else [0.0]
    return [(cls or Observation)(value=float(rng.standard_normal()), obtype=names[k % len(names)], time=float(times[k % len(times)]),
                                 error=float(rng.uniform(0.5, 1.5)), lat=float(rng.uniform(31, 49)), lon=float(rng.uniform(231, 261)),
                                 assimilate_this=(k % 6 != 1), localize_radius=float(rng.uniform(600.0, 1500.0))) for k in range(P)]


def _diag(obs):
    return dict((key, np.array([np.nan if getattr(o, key) is None else float(getattr(o, key)) for o in obs])) for key in DIAG)


def _update(state, obs, **kw):
    from efa_xray_amd import EnSRF
    obs = deepcopy(obs)
    flt = EnSRF(state, obs, verbose=False, **kw)
    post, _ = flt.update()
    return post, post.to_vect(), _diag(obs), flt


def _assert_f32_update(state32, obs, what, streamed=(), **kw):
    """update() on the float32 state against the float64 update() on the widened state, rounded once; then every streamed chunk
    setting against the unstreamed float32 update.  Returns the float32 run."""
    X0 = state32.to_vect().copy()
    ref = _update(state32.astype(F64), obs, **kw)
    got = _update(state32, obs, **kw)
    assert got[0].dtype == F32 and got[1].dtype == F32 and got[0] is not state32
    bad = int(np.sum(_bits(got[1]) != _bits(ref[1].astype(F32))))
    assert bad == 0, "%s: %d of %d posterior values differ from fl32(float64 update)" % (what, bad, got[1].size)
    for key in DIAG:
        assert _same(got[2][key], ref[2][key]), "%s: %s" % (what, key)
    assert _same(state32.to_vect(), X0), what + ": the prior was written"
    L = _lib()
    ncol, M, n_lead = state32.ny() * state32.nx(), state32.nmems(), state32.nvars() * state32.ntimes()
    for cc in streamed:
        s = _update(state32, obs, streamed=True, stream_chunk_cols=cc, **kw)
        w = "%s streamed chunk_cols=%r" % (what, cc)
        assert s[0].dtype == F32 and _same(s[1], got[1]), w + ": differs from the unstreamed float32 update"
        for key in DIAG:
            assert _same(s[2][key], got[2][key]), "%s: %s" % (w, key)
        cols = cc if cc is not None else L.default_chunk_cols(n_lead, M, itemsize=4)
        plan = L.plan_chunks(ncol, cols, itemsize=4)
        assert s[3].last_stream["chunks"] == len(plan)
        chunk_rows = n_lead * (plan[0][1] - plan[0][0])
        assert s[3].last_stream["peak_bytes"] == 3 * chunk_rows * M * 4, w   # three chunks of 4-byte elements: nothing is widened on the host
        assert _same(state32.to_vect(), X0), w + ": the prior was written"
    return got


def _chunk_settings(ncol):
    """16, a value giving a ragged last chunk, one chunk for everything, and the default."""
    ragged = next((c for c in (32, 48, 16, 64, 80, 96) if c < ncol and ncol % c), 16)
    return [16, ragged, ncol + 16, None]


@pytest.mark.parametrize("M", [7, 20, 50, 100])
@pytest.mark.parametrize("loc", [False, "GC"])
def test_update_and_streamed_update(M, loc):
    state = _state(100 + M, M)
    obs = _point_obs(state, 200 + M, 30)
    got = _assert_f32_update(state, obs, "M=%d loc=%r" % (M, loc), streamed=_chunk_settings(117), loc=loc)
    assert got[3]._default_forward_operator()
    assert _ctx().get_option("f32_native") == (0 if (loc == "GC" and M % 2) else 1)


@pytest.mark.parametrize("kw", [dict(rtps=0.6), dict(rtpp=0.3), dict(rtps=0.6, loc="GC"), dict(path="sweep"), dict(outlier_threshold=1.5),
                                dict(loc="GC", vert_coord=True)], ids=lambda kw: "-".join(sorted(kw)))
def test_update_options(kw):
    kw = dict(kw)
    state = _state(300, 20)
    obs = _point_obs(state, 301, 30)
    if kw.get("vert_coord") is True:
        kw["vert_coord"] = np.array([[900.0, 700.0, np.nan], [500.0, 300.0, 200.0]])
        for k, ob in enumerate(obs):
            if k % 4:
                ob.vert, ob.vert_localize_radius = 200.0 + 30.0 * k, 400.0
    _assert_f32_update(state, obs, "options %r" % sorted(kw), streamed=[16, 48], **kw)


@pytest.mark.parametrize("default_op", [True, False])
def test_format_and_ob_prior_helpers_on_a_float32_state(default_op):
    """`format_prior_state`, `compute_ob_estimates`, `compute_ob_priors` and `format_posterior_state` run float64 kernels: on a
    float32 prior they widen (exactly) and return what they return for `prior.astype(float64)`; the state that comes back is float32,
    rounded once.  A float32 resident copy handed to them is refused before any kernel sees it."""
    from efa_xray_amd import EnSRF, Observation

    class RowOb(Observation):
        def estimate(self, st):
            return st.to_vect()[self.row].astype(F64)

    state = _state(450, 20)
    obs = _point_obs(state, 451, 25, cls=None if default_op else RowOb)
    for k, ob in enumerate(obs):
        ob.row = 27 * k
    f32 = EnSRF(state, deepcopy(obs), verbose=False, loc="GC")
    f64 = EnSRF(state.astype(F64), deepcopy(obs), verbose=False, loc="GC")
    assert f32._default_forward_operator() == default_op
    assert _same(f32.compute_ob_estimates(), f64.compute_ob_estimates())
    for a, b in zip(f32.compute_ob_priors(), f64.compute_ob_priors()):
        assert _same(a, b)
    xbm, Xbp = f32.format_prior_state()
    rbm, Rbp = f64.format_prior_state()
    assert xbm.dtype == F64 and Xbp.dtype == F64 and _same(xbm, rbm) and _same(Xbp, Rbp)
    xam, Xap = xbm + 0.25, Xbp * 1.5
    p32, _ = f32.format_posterior_state(xam, Xap)
    p64, _ = f64.format_posterior_state(xam, Xap)
    assert p32.dtype == F32 and p64.dtype == F64 and _same(p32.to_vect(), p64.to_vect().astype(F32))
    ctx = f32._context()
    X32 = f32._upload_prior(ctx)
    assert X32.dtype == F32 and f32._upload_prior(ctx, F64).dtype == F64
    if default_op:
        with pytest.raises(ValueError, match="float32 DeviceArray"):
            f32.compute_ob_estimates(X32)
    with pytest.raises(ValueError, match="float32 DeviceArray"):
        ctx.form_perts(state.nstate(), state.nmems(), X32, ctx.empty((state.nstate(),)), X32)


def test_inflation_rounds_the_inflated_prior_once():
    """inflation=1.1: the perturbations are scaled in float64 and the inflated prior rounded to float32 once; the update is then
    that of the inflated float32 prior."""
    from efa_xray_amd import EnSRF
    state = _state(400, 20)
    obs = _point_obs(state, 401, 30)
    want_prior = EnSRF(state.astype(F64), [], verbose=False, inflation=1.1)
    want_prior.inflate_state()
    s32 = deepcopy(state)
    got = _update(s32, obs, inflation=1.1, loc="GC")
    assert s32.dtype == F32 and _same(s32.to_vect(), want_prior.prior.to_vect().astype(F32))   # in place, as the float64 hook
    assert not _same(s32.to_vect(), state.to_vect())
    ref = _update(s32.astype(F64), obs, loc="GC")
    assert _same(got[1], ref[1].astype(F32))
    for key in DIAG:
        assert _same(got[2][key], ref[2][key]), key
    s32b = deepcopy(state)
    st = _update(s32b, obs, inflation=1.1, loc="GC", streamed=True, stream_chunk_cols=32)
    assert _same(st[1], got[1])


def test_user_defined_operator_sees_the_float32_state():
    from efa_xray_amd import Observation
    seen = []

    class RowOb(Observation):
        def estimate(self, st):
            seen.append(st.dtype)
            v = st.to_vect()
            return 0.5 * (v[self.row].astype(F64) + v[self.row + 1].astype(F64))

    state = _state(500, 50)
    obs = _point_obs(state, 501, 20, cls=RowOb)
    for k, ob in enumerate(obs):
        ob.row = 35 * k
    got = _assert_f32_update(state, obs, "user-defined operator", streamed=[16, None], loc="GC")
    assert not got[3]._default_forward_operator()
    assert F32 in seen and F64 in seen


def test_two_cycles_with_the_posterior_fed_back():
    """Streamed, float32: the page-locked posterior of cycle 1 is the prior of cycle 2; a pinned and a plain first prior."""
    ctx = _ctx()
    state = _state(600, 50)
    obs1, obs2 = _point_obs(state, 601, 30), _point_obs(state, 602, 25)
    u1 = _update(state, obs1, loc="GC")
    u2 = _update(u1[0], obs2, loc="GC")
    for first in (state, state.pinned_copy(ctx)):
        assert first.dtype == F32
        s1 = _update(first, obs1, loc="GC", streamed=True, stream_chunk_cols=48)
        assert s1[0].dtype == F32 and _same(s1[1], u1[1])
        s2 = _update(s1[0], obs2, loc="GC", streamed=True, stream_chunk_cols=48)
        assert _same(s2[1], u2[1])
        for key in DIAG:
            assert _same(s2[2][key], u2[2][key]), key
    r1 = _update(state.astype(F64), obs1, loc="GC")
    assert _same(u1[1], r1[1].astype(F32))
    r2 = _update(u1[0].astype(F64), obs2, loc="GC")
    assert _same(u2[1], r2[1].astype(F32))


def test_cycle_host_f32_entry_point():
    """efa_ensrf_cycle_host_f32 itself: pinned and plain segments, every chunk setting, against the resident float32 call."""
    L = _lib()
    ctx = _ctx()
    for M, gc in ((20, True), (50, False), (7, True)):
        n_lead, ny, nx = 5, 9, 13
        pb = Problem(9000 + M, M, 40, n_lead=n_lead, ny=ny, nx=nx, gc=gc)
        ref = _run(pb, True, in_place=True)
        slabs = (2, 3)
        prior = [np.ascontiguousarray(pb.X32[:2 * pb.ncol].reshape(2, pb.ncol, M)), np.ascontiguousarray(pb.X32[2 * pb.ncol:].reshape(3, pb.ncol, M))]
        kw = dict(loc_mode=L.LOC_GC, ob_lat=pb.ob_lat, ob_lon=pb.ob_lon, ob_halfwidth=pb.hw, grid_lat=pb.glat, grid_lon=pb.glon) if gc else {}
        for pinned in (False, True):
            if pinned:
                segs = [ctx.pinned_empty(a.shape, F32) for a in prior]
                for a, b in zip(segs, prior):
                    a[...] = b
            else:
                segs = prior
            for cc in _chunk_settings(pb.ncol)[:3]:
                post = [ctx.pinned_empty(a.shape, F32) if pinned else np.empty(a.shape, dtype=F32) for a in prior]
                assert all(p.dtype == F32 for p in post)
                diag = ctx.ensrf_cycle_host(segs, post, pb.ncol, M, pb.HX, cc, pb.value, pb.error, pb.assim, **kw)
                w = "M=%d gc=%r pinned=%r chunk_cols=%d" % (M, gc, pinned, cc)
                got = np.concatenate([p.reshape(-1, M) for p in post])
                assert _same(got, ref[0]), w
                for key in DIAG:
                    assert _same(diag[key], ref[1][key]), "%s: %s" % (w, key)
                stats = ctx.stream_stats()
                plan = L.plan_chunks(pb.ncol, cc, 4)
                assert stats["chunks"] == len(plan)
                assert stats["peak_bytes"] == 3 * sum(slabs) * (plan[0][1] - plan[0][0]) * M * 4, w
                assert all(_same(a, b) for a, b in zip(segs, prior)), w + ": the prior was written"
    with pytest.raises(ValueError):
        ctx.ensrf_cycle_host([prior[0]], [np.empty(prior[0].shape)], pb.ncol, M, pb.HX, 16, pb.value, pb.error, pb.assim)


def test_one_context_through_mixed_dtypes():
    """float64 -> float32 -> streamed float32 -> float64 on one context, each against a fresh context."""
    L = _lib()
    state = _state(700, 20)
    s64 = state.astype(F64)
    obs = _point_obs(state, 701, 30)
    steps = [(s64, dict(loc="GC")), (state, dict(loc="GC")), (state, dict(loc="GC", streamed=True, stream_chunk_cols=32)),
             (state, dict(rtps=0.5)), (s64, dict(loc="GC")), (s64, dict())]
    shared = [_update(st, obs, **kw) for st, kw in steps]
    saved = L._contexts.pop(0, None)
    try:
        for (st, kw), got in zip(steps, shared):
            L._contexts.pop(0, None)
            fresh = _update(st, obs, **kw)
            assert fresh[1].dtype == got[1].dtype and _same(fresh[1], got[1]), "step %r" % (sorted(kw),)
            for key in DIAG:
                assert _same(fresh[2][key], got[2][key]), key
            L._contexts.pop(0).close()
    finally:
        if saved is not None:
            L._contexts[0] = saved
    assert _same(shared[1][1], shared[0][1].astype(F32)) and _same(shared[2][1], shared[1][1]) and _same(shared[4][1], shared[0][1])


# ---------------------------------------------------------------------------
# against the reference: the oracle, float64, on the widened float32 inputs
# ---------------------------------------------------------------------------
def _assert_reference_bound(post32, ref, what):
    post = np.asarray(post32, dtype=F64)
    bound = 2.0 ** -24 * np.abs(ref) + 1e-10 * np.max(np.abs(ref), axis=1, keepdims=True)
    err = np.abs(post - ref)
    worst = float(np.max(err / bound))
    print("%s: max |post32 - ref| / bound = %.4f" % (what, worst))
    assert np.all(err <= bound), "%s: %d values beyond 2^-24 |ref| + 1e-10 max|ref row| (worst %.4f of the bound)" % (
        what, int(np.sum(err > bound)), worst)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_goldens_rounded_to_float32_against_the_oracle(name):
    from oracle import ensrf_oracle as orc
    from test_gpu_parity import _make_api_objects, oracle_kwargs
    g = load_golden(name)
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    state, obs = _make_api_objects(g)
    s32 = state.astype(F32)
    Xw = s32.to_vect().astype(F64)
    HXw = np.zeros((len(obs), M))
    for k in range(len(obs)):
        nz = g["sten_wts"][k] != 0
        rows, wts = Xw[g["sten_idx"][k][nz]], g["sten_wts"][k][nz]
        HXw[k] = rows[0] if (len(wts) == 1 and wts[0] == 1.0) else (wts[:, None] * rows).sum(axis=0)
    ref_post, _, _, diag = orc.ensrf_cycle(Xw.reshape(N, M), HXw, g["ob_value"], g["ob_error"], g["ob_assim"], **oracle_kwargs(g))
    loc = g["loc"] or False
    got = _assert_f32_update(s32, obs, name, streamed=[16], loc=loc)
    _assert_reference_bound(got[1], ref_post, name)
    done = np.asarray(diag["assimilated"], dtype=bool)
    assert np.array_equal(got[2]["assimilated"].astype(bool), done)
    for key in ("prior_mean", "prior_var"):
        np.testing.assert_allclose(got[2][key], diag[key], rtol=1e-10, atol=1e-10 * np.max(np.abs(diag[key])))


def test_g11_rounded_to_float32_against_the_oracle():
    """G11 (plain Observations, the default forward operator through the host gather) with the state rounded to float32."""
    from oracle import ensrf_oracle as orc
    from efa_xray_amd import EnsembleState, Observation
    g = load_golden("G11")
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    names = [str(n) for n in g["var_names"]]
    s32 = EnsembleState.from_array(g["X"], g["grid_lat"], g["grid_lon"], varnames=names, validtime=g["validtime"], dtype=F32)
    obs = [Observation(value=float(g["ob_value"][k]), obtype=names[g["ob_var"][k]], time=g["ob_time"][k],
                       error=float(g["ob_error"][k]), lat=float(g["ob_lat"][k]), lon=float(g["ob_lon"][k]),
                       assimilate_this=bool(g["ob_assim"][k]), localize_radius=float(g["ob_radius"][k]))
           for k in range(len(g["ob_value"]))]
    Xw = s32.to_vect().astype(F64)
    Xs = Xw.reshape(nvar, nt, ny, nx, M)
    HXw = np.stack([np.asarray(orc.interpolate(Xs[g["ob_var"][k]], g["grid_lat"], g["grid_lon"], g["validtime"], g["ob_time"][k],
                                               g["ob_lat"][k], g["ob_lon"][k])).reshape(M) for k in range(len(obs))])
    ref_post, _, _, diag = orc.ensrf_cycle(Xw, HXw, g["ob_value"], g["ob_error"], g["ob_assim"], loc="GC", ob_lat=g["ob_lat"],
                                           ob_lon=g["ob_lon"], ob_halfwidth=g["ob_radius"], grid_lat=g["grid_lat"],
                                           grid_lon=g["grid_lon"], state_shape=(nvar, nt, ny, nx))
    got = _assert_f32_update(s32, obs, "G11", streamed=[16, None], loc="GC")
    assert got[3]._default_forward_operator()
    _assert_reference_bound(got[1], ref_post, "G11")
    assert np.array_equal(got[2]["assimilated"].astype(bool), np.asarray(diag["assimilated"], dtype=bool))
