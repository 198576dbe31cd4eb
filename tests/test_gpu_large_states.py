"""GPU tests of the state-phase kernels BEYOND their grid caps.

Every state-phase kernel is a grid-stride loop behind a capped grid.  Each case here runs on `2 * cap + 53` rows, `cap` being the
rows one full grid covers in one trip: some waves then make three trips and others two, the prefetch of the transform sees both a
real next tile and none, and the last tile holds 5 rows and falls in a third trip.  The caps are spelled below from the launchers'
constants.

The yardsticks; none of them is the code under test at the same shape and mode:
(a)  `oracle.ensrf_oracle.ensrf_cycle`, float64, on the whole state, held by `assert_parity` at the project's RTOL (with relaxation:
     the closed forms of tests/test_relaxation_host.py applied to the oracle's posterior);
(a') for float32 rows the bound of DESIGN 7g against the same reference, |post32 - ref| <= 2^-24 |ref| + 1e-10 max|ref row|;
(b)  row independence, bit for bit: a row's posterior depends only on that row and [T | w], and neither the lane mapping nor the
     summation order depends on the tile index, the row count or the grid -- so rows [a, b) of the large posterior have the bits
     of a separate out-of-place call on just those rows behind the same obs phase and settings (blocks at the start, across each
     cap, across twice each cap up to the ragged end, and a 16-aligned and an unaligned block in the middle);
(c)  in place is out of place, bit for bit: float64, float32, and float32 with the base offset by one float.

24 obs of single rows, 19 of them assimilated; the transform is asked for above 136 members, as elsewhere in the suite."""
import copy
import ctypes

import numpy as np
import pytest

import _anderson2009 as a09
from test_gpu_f32_state import DIAG, F32, F64, Problem, _assert_reference_bound, _bits, _check, _ctx, _lib, _run, _same, _settings
from test_gpu_parity import assert_parity
from test_relaxation_host import relax

pytestmark = pytest.mark.gpu

P_OBS = 24

# ---- the caps, from the launchers ---------------------------------------------------------------------------------------------
CUS, T_WAVES, TILE_ROWS = 256, 8, 16   # efa_transform.hip: EFA_T_WAVES waves per workgroup, one 16-row tile per wave and trip


def transform_image_bytes(M, member=True):
    """The LDS image of [T | w] (TShape in efa_transform.hip): 2 NU K-steps x NT 16-column tiles x 64 doubles, and the narrow tile."""
    nu = (M + 7) // 8
    half = M % 8 in (1, 2, 3, 4)
    narrow = member and half and nu % 2 == 1
    nt = (nu // 2 + 1) if not member else (nu // 2 if narrow else (nu + 1) // 2)
    return 8 * (2 * nu * nt * 64 + (2 * nu * 64 if narrow else 0))


def transform_cap(M, member=True):
    if M > 136:   # transform_wide_nu: at most 256 workgroups per column group
        return CUS * T_WAVES * TILE_ROWS
    per_cu = 2 if transform_image_bytes(M, member) <= 80 * 1024 else 1   # transform_launch / transform_rtps_launch
    return CUS * per_cu * T_WAVES * TILE_ROWS


ROW_WAVE_CAP = 256 * 8 * (256 // 64)   # grid_for(rows, 4) / rows_grid / launch_inflate_rows: 2048 blocks of 4 waves, a row per wave
FLAT_CAP = 256 * 8 * 256               # grid_for(n, kThreads): k_posterior, k_widen_f32, k_narrow_f32, elements
SWEEP_CAP = 256 * 8 * (256 // 4)       # sweep_launch<4, NC>: 2048 blocks of kRowsPerBlock = kThreads / 4 rows

assert [transform_cap(M) for M in (7, 20, 100, 136, 137, 256)] == [65536, 65536, 32768, 32768, 32768, 32768]
assert [transform_cap(M, False) for M in (20, 100)] == [65536, 32768]
assert (ROW_WAVE_CAP, FLAT_CAP, SWEEP_CAP) == (8192, 524288, 131072)


def big(cap):
    return 2 * cap + 53


def _blocks(rows, caps):
    """The row blocks of yardstick (b) for a state of `rows` rows whose kernels have the row caps `caps` (the first: the main one)."""
    out = [(0, 64)]
    for cap in caps:
        out += [(cap - 24, cap + 40), (2 * cap - 24, min(2 * cap + 53, rows))]
    mid = caps[0] + caps[0] // 2
    out += [(mid // 16 * 16, mid // 16 * 16 + 64), (caps[0] // 2 + 7, caps[0] // 2 + 7 + 61)]
    out.append((rows - 53 - 24, rows))
    return sorted(set((a, b) for a, b in out if 0 <= a < b <= rows))


# ---- the problems: built once per (M, rows), with the oracle and the float64 out-of-place posteriors they are compared with ----
class Case(object):
    def __init__(self, M, rows):
        self.pb = Problem(9100 + M, M, P_OBS, ny=rows)
        assert self.pb.rows == rows and int(self.pb.assim.sum()) == 19
        self._oracle = None
        self._ref, self.yards = {}, {}

    def oracle(self):
        """(posterior members, posterior means, posterior perturbations) of the reference, float64, computed once."""
        if self._oracle is None:
            from oracle import ensrf_oracle as orc
            pb = self.pb
            post, xam, Xap, _ = orc.ensrf_cycle(pb.X64, pb.HX, pb.value, pb.error, pb.assim)
            self._oracle = (post, xam[:pb.rows], Xap[:pb.rows])
            for a in self._oracle:
                a.flags.writeable = False
        return self._oracle

    def ref(self, key, settings, form="member"):
        """The float64 out-of-place call of these settings on the whole state, run once: (posterior, diag, obs block, None)."""
        if key not in self._ref:
            with _settings(**settings):
                self._ref[key] = _run(self.pb, False, form=form, exact=True)
            for a in _parts(self._ref[key][0]):
                a.flags.writeable = False
        return self._ref[key]


_CASES = {}


def _case(M, rows):
    if (M, rows) not in _CASES:
        _CASES[(M, rows)] = Case(M, rows)
    return _CASES[(M, rows)]


def _rows_of(pb, a, b):
    """The problem of rows [a, b) alone: the same obs, so the same obs phase."""
    q = copy.copy(pb)
    q.rows, q.X32, q.X64 = b - a, pb.X32[a:b], pb.X64[a:b]
    return q


def _transform(M, **kw):
    return dict(kw, path=_lib().PATH_TRANSFORM) if M > 136 else kw


def _parts(post):
    return post if isinstance(post, tuple) else (post,)


def _differing(got, ref):
    return sum(int(np.sum(_bits(g) != _bits(r))) for g, r in zip(_parts(got), _parts(ref)))


def _assert_f64(case, key, settings, what, caps, yard, path, form="member", launches=None):
    """Yardsticks (a), (b), (c) on the float64 calls of one setting.  yard: what (a) compares with, one array per output."""
    pb = case.pb
    ref = case.ref(key, settings, form)
    for got, want, name in zip(_parts(ref[0]), yard, ("posterior", "posterior perturbations") if form == "member" else
                               ("posterior means", "posterior perturbations")):
        assert_parity(got, want, "%s: %s against the reference" % (what, name))
    with _settings(**settings):
        for a, b in _blocks(pb.rows, caps):
            sub = _run(_rows_of(pb, a, b), False, form=form, exact=True)
            bad = _differing(sub[0], tuple(p[a:b] for p in _parts(ref[0])))
            assert bad == 0, "%s: rows [%d, %d) of the large call differ from a call on those rows alone in %d values" % (what, a, b, bad)
        t = _ctx().last_timing()
        assert t["path"] == path, what
        got = _run(pb, False, in_place=True, form=form, exact=True)
        t = _ctx().last_timing()
        assert t["path"] == path, what
        if launches is not None:
            assert t["state_launches"] == launches, "%s: %d launches in place, expected %d" % (what, t["state_launches"], launches)
    bad = _differing(got[0], ref[0])
    assert bad == 0, "%s: in place differs from out of place in %d of %d values" % (what, bad, sum(p.size for p in _parts(ref[0])))
    for key_ in DIAG:
        assert _same(got[1][key_], ref[1][key_]), "%s: %s" % (what, key_)


def _assert_f32(case, key, settings, what, yard, native):
    """Yardsticks (a') and (c) on the float32 calls: out of place, in place and in place off an 8-byte boundary, each to the bits
    of the float64 out-of-place posterior rounded once (which yardstick (b) holds row by row)."""
    ref = case.ref(key, settings)
    ref32 = (ref[0].astype(F32),) + tuple(ref[1:])
    with _settings(**settings):
        _check(case.pb, what, native=native, variants=[(False, 0), (True, 0), (True, 1)], ref=ref32)
    _assert_reference_bound(ref32[0], yard, what)   # (the bits every float32 call above returned)


# ---- the transform, member form -----------------------------------------------------------------------------------------------
MEMBER_M = [7, 20, 100, 136, 137, 160, 256]   # odd; HALF + NARROW; the headline shape; the largest single image; wide: odd, 3, 4 groups


@pytest.mark.parametrize("M", MEMBER_M)
def test_transform_member_form_float64(M):
    cap = transform_cap(M)
    case = _case(M, big(cap))
    _assert_f64(case, "plain", _transform(M), "transform M=%d rows=%d float64" % (M, big(cap)), [cap], (case.oracle()[0],),
                _lib().PATH_TRANSFORM, launches=1)
    assert not _same(case.ref("plain", _transform(M))[0], case.pb.X64)


@pytest.mark.parametrize("M", MEMBER_M)
def test_transform_member_form_float32(M):
    cap = transform_cap(M)
    case = _case(M, big(cap))
    _assert_f32(case, "plain", _transform(M), "transform M=%d rows=%d float32" % (M, big(cap)), case.oracle()[0], native=1)


# ---- the transform, perturbation form (efa_state_phase_dev) ---------------------------------------------------------------------
@pytest.mark.parametrize("M", [20, 100, 137, 256])   # at 256 the mean-increment column is a fifth group of one tile
def test_transform_perturbation_form(M):
    """Means and perturbations, both outputs: against the oracle's, row blocks against calls on those rows, in place against out of
    place.  The prior means and perturbations are k_form_perts' (a row per wave, past 8192 rows)."""
    cap = transform_cap(M, member=False)
    case = _case(M, big(cap))
    _, xam, Xap = case.oracle()
    _assert_f64(case, "perts", _transform(M), "perturbation form M=%d rows=%d" % (M, big(cap)), [cap, ROW_WAVE_CAP], (xam, Xap),
                _lib().PATH_TRANSFORM, form="perts", launches=1)


# ---- relaxation on the transform ----------------------------------------------------------------------------------------------
RTPS, RTPP = 0.7, 0.4


def _relaxed(case, kind):
    """Yardstick (a) with relaxation: its closed form, float64 numpy, on the prior and the oracle's posterior."""
    if kind not in case.yards:
        alpha = dict(rtps=RTPS) if kind == "rtps" else dict(rtpp=RTPP)
        case.yards[kind] = relax(case.pb.X64, case.oracle()[0], **alpha)
    return case.yards[kind]


def _relax(kind):
    L = _lib()
    return (L.RELAX_RTPS, RTPS) if kind == "rtps" else (L.RELAX_RTPP, RTPP)


@pytest.mark.parametrize("M", [20, 100, 136])
@pytest.mark.parametrize("elem", ["float64", "float32"])
def test_rtps_fused_into_the_transform(M, elem):
    cap = transform_cap(M)
    case = _case(M, big(cap))
    settings = dict(relax=_relax("rtps"))
    what = "RTPS fused M=%d rows=%d %s" % (M, big(cap), elem)
    if elem == "float64":
        _assert_f64(case, "rtps", settings, what, [cap], (_relaxed(case, "rtps"),), _lib().PATH_TRANSFORM, launches=1)
    else:
        _assert_f32(case, "rtps", settings, what, _relaxed(case, "rtps"), native=1)


@pytest.mark.parametrize("M", [100, 256])
@pytest.mark.parametrize("elem", ["float64", "float32"])
def test_rtpp_folded_into_the_transform(M, elem):
    cap = transform_cap(M)
    case = _case(M, big(cap))
    settings = _transform(M, relax=_relax("rtpp"))
    what = "RTPP folded M=%d rows=%d %s" % (M, big(cap), elem)
    if elem == "float64":
        _assert_f64(case, "rtpp", settings, what, [cap], (_relaxed(case, "rtpp"),), _lib().PATH_TRANSFORM, launches=2)
    else:
        _assert_f32(case, "rtpp", settings, what, _relaxed(case, "rtpp"), native=1)


@pytest.mark.parametrize("elem", ["float64", "float32"])
def test_rtps_standalone_around_the_wide_transform(elem):
    """M = 160: k_row_spread, the column-group transform and k_relax_rows, each past its cap; float32 rows take the workspace, so
    k_widen_f32 / k_narrow_f32 cross theirs."""
    M = 160
    cap = transform_cap(M)
    case = _case(M, big(cap))
    settings = _transform(M, relax=_relax("rtps"))
    what = "RTPS standalone M=%d rows=%d %s" % (M, big(cap), elem)
    if elem == "float64":
        _assert_f64(case, "rtps", settings, what, [cap, ROW_WAVE_CAP], (_relaxed(case, "rtps"),), _lib().PATH_TRANSFORM, launches=3)
    else:
        _assert_f32(case, "rtps", settings, what, _relaxed(case, "rtps"), native=0)


# ---- the per-batch sweeps, member form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rtps", "rtpp"])
@pytest.mark.parametrize("elem", ["float64", "float32"])
def test_per_batch_sweeps_member_form(kind, elem):
    """path "sweep": k_form_perts, k_sweep, k_posterior and the standalone relaxation passes, each past its cap (k_sweep's is the
    largest: 2048 blocks of 64 rows); float32 rows through the workspace (f32_native 0)."""
    M, rows = 20, big(SWEEP_CAP)
    assert rows >= big(ROW_WAVE_CAP) and rows * M > 2 * FLAT_CAP
    case = _case(M, rows)
    settings = dict(path=_lib().PATH_SWEEP, relax=_relax(kind))
    what = "sweeps %s M=%d rows=%d %s" % (kind, M, rows, elem)
    if elem == "float64":
        caps = [SWEEP_CAP, ROW_WAVE_CAP, -(-FLAT_CAP // M)]
        _assert_f64(case, "sweep_" + kind, settings, what, caps, (_relaxed(case, kind),), _lib().PATH_SWEEP)
    else:
        _assert_f32(case, "sweep_" + kind, settings, what, _relaxed(case, kind), native=0)


# ---- efa_inflate_rows_dev -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [7, 100])
def test_inflate_rows_past_the_cap(M):
    ctx = _ctx()
    rows = big(ROW_WAVE_CAP)
    rng = np.random.default_rng(9300 + M)
    X = rng.standard_normal((rows, 1)) + 3.0 * rng.standard_normal((rows, M))
    field = np.stack([rng.uniform(0.6, 2.5, rows), rng.uniform(0.1, 0.6, rows)], axis=1)
    ones = np.array([0, 5, ROW_WAVE_CAP - 2, ROW_WAVE_CAP, ROW_WAVE_CAP + 3, 2 * ROW_WAVE_CAP - 1, 2 * ROW_WAVE_CAP + 1, rows - 1])
    field[ones, 0] = 1.0
    field[11::37, 0] = 1.0
    skipped = field[:, 0] == 1.0
    Xd, Fd = ctx.to_device(X), ctx.to_device(field)
    ctx.inflate_rows(rows, M, Xd, Fd)
    got = Xd.download()
    assert_parity(got, a09.inflate(X, field[:, 0]), "inflate_rows M=%d rows=%d" % (M, rows))
    assert _same(got[skipped], X[skipped]), "rows of inflation 1 must keep their bits"
    assert not np.any(np.all(got[~skipped] == X[~skipped], axis=1)), "a row of inflation other than 1 was left as it was"
    assert _same(Fd.download(), field), "the field was written"
    for a, b in _blocks(rows, [ROW_WAVE_CAP]):   # (b): a row's result depends on that row alone
        xs, fs = ctx.to_device(X[a:b]), ctx.to_device(field[a:b])
        ctx.inflate_rows(b - a, M, xs, fs)
        assert _same(xs.download(), got[a:b]), "rows [%d, %d)" % (a, b)


# ---- one streamed float64 update: every chunk runs in place ---------------------------------------------------------------------
def test_streamed_update_wide_transform_chunks_in_place():
    """`EnSRF.update(streamed=True)` at M = 160 in two chunks of 16 512 rows, each transformed in place in its ring buffer by the
    column groups: the bits of the unstreamed out-of-place posterior, and the oracle.  Then the unstreamed `update()`, in place."""
    from efa_xray_amd import EnSRF, EnsembleState, Observation
    from oracle import ensrf_oracle as orc
    L = _lib()
    M, nvar, ny, nx = 160, 2, 129, 128
    ncol, cc = ny * nx, ny * nx // 2
    rows = nvar * ncol
    assert cc % 16 == 0 and nvar * cc >= 16384 and L.plan_chunks(ncol, cc) == [(0, cc), (cc, ncol)]
    pb = Problem(9400, M, P_OBS, ny=rows)
    lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(230, 262, nx), indexing="ij")
    state = EnsembleState.from_array(pb.X64.reshape(nvar, 1, ny, nx, M), lat, lon)
    assert _same(state.to_vect(), pb.X64)

    class RowOb(Observation):
        def estimate(self, st):
            return pb.HX[self.k].copy()

    obs = []
    for k in range(P_OBS):
        ob = RowOb(value=float(pb.value[k]), error=float(pb.error[k]), lat=40.0, lon=250.0, assimilate_this=bool(pb.assim[k]))
        ob.k = k
        obs.append(ob)
    flt = EnSRF(state, obs, verbose=False, loc=False, path="transform", streamed=True, stream_chunk_cols=cc)
    post, _ = flt.update()
    got = post.to_vect()
    assert flt.last_stream["chunks"] == 2 and flt.last_timing["path"] == L.PATH_TRANSFORM
    assert _same(state.to_vect(), pb.X64), "the prior was written"
    with _settings(path=L.PATH_TRANSFORM):
        ref = _run(pb, False, exact=True)
    bad = _differing(got, ref[0])
    assert bad == 0, "streamed: %d of %d values differ from the unstreamed out-of-place posterior" % (bad, got.size)
    diag = dict((key, np.array([np.nan if getattr(o, key) is None else float(getattr(o, key)) for o in obs])) for key in DIAG)
    done = ref[1]["assimilated"].astype(bool)
    assert np.array_equal(diag["assimilated"].astype(bool), done)
    for key in ("prior_mean", "prior_var"):
        assert _same(diag[key], ref[1][key]), key
    for key in ("post_mean", "post_var"):
        assert _same(diag[key][done], ref[1][key][done]), key
    want, _, _, _ = orc.ensrf_cycle(pb.X64, pb.HX, pb.value, pb.error, pb.assim)
    assert_parity(got, want, "streamed M=160 against the reference")
    # ... and the unstreamed update(), which runs efa_ensrf_cycle_dev in place on all 33 024 rows
    whole, _ = EnSRF(state, copy.deepcopy(obs), verbose=False, loc=False, path="transform").update()
    bad = _differing(whole.to_vect(), ref[0])
    assert bad == 0, "unstreamed update(): %d of %d values differ from the out-of-place posterior" % (bad, got.size)


# ---- a posterior range that overlaps the prior without coinciding with it ---------------------------------------------------------
def test_partial_overlap_is_refused():
    """Pointer arithmetic on one allocation: either way round, both forms, both element types -- EFA_ERR_INVALID before any launch
    (nothing is written); the same rows exactly (in place) and adjacent ranges (disjoint) are served."""
    L, ctx = _lib(), _ctx()
    M, rows = 20, 64
    pb = Problem(9500, M, 10, ny=rows)
    ref = _run(pb, False, exact=True)      # (the obs phase the calls below stand behind)
    n = rows * M

    def invalid(call):
        with pytest.raises(L.EfaError) as ei:
            call()
        assert ei.value.status == L.EFA_ERR_INVALID and "overlap" in str(ei.value), str(ei.value)

    def at(buf, elems):
        return ctypes.c_void_p(buf.address + elems * buf.itemsize)

    for dtype, cycle, X in ((F64, ctx.state_cycle, pb.X64), (F32, ctx.state_cycle_f32, pb.X32)):
        host = np.full(2 * n, 7.0, dtype=dtype)
        host[:n] = X.reshape(-1)
        buf = ctx.empty((2 * n,), dtype).upload(host)
        for shift in (1, M, n - 1):
            invalid(lambda: cycle(rows, M, buf, at(buf, shift)))
            invalid(lambda: cycle(rows, M, at(buf, shift), buf))
        assert _same(buf.download(), host), "a refused call wrote"
        cycle(rows, M, buf, at(buf, n))    # adjacent: disjoint
        got = buf.download()
        assert _same(got[:n], host[:n]) and _same(got[n:].reshape(rows, M), ref[0].astype(dtype))
        cycle(rows, M, buf, buf)           # the same rows: in place
        assert _same(buf.download()[:n].reshape(rows, M), ref[0].astype(dtype))

    xm, Xp = pb.X64.mean(axis=1), pb.X64 - pb.X64.mean(axis=1, keepdims=True)
    host = np.full(2 * n, 7.0)
    host[:n] = Xp.reshape(-1)
    buf = ctx.empty((2 * n,)).upload(host)
    mhost = np.full(2 * rows, 7.0)
    mhost[:rows] = xm
    mbuf = ctx.empty((2 * rows,)).upload(mhost)
    for shift in (1, M, n - 1):
        invalid(lambda: ctx.state_phase(rows, M, mbuf, buf, at(mbuf, rows), at(buf, shift)))
        invalid(lambda: ctx.state_phase(rows, M, mbuf, at(buf, shift), at(mbuf, rows), buf))
    for shift in (1, rows - 1):            # the means alone
        invalid(lambda: ctx.state_phase(rows, M, mbuf, buf, at(mbuf, shift), at(buf, n)))
        invalid(lambda: ctx.state_phase(rows, M, at(mbuf, shift), buf, mbuf, at(buf, n)))
    assert _same(buf.download(), host) and _same(mbuf.download(), mhost), "a refused call wrote"
    ctx.state_phase(rows, M, mbuf, buf, at(mbuf, rows), at(buf, n))
    got, gm = buf.download(), mbuf.download()
    assert _same(got[:n], host[:n]) and _same(gm[:rows], mhost[:rows])
    assert_parity(gm[rows:, None] + got[n:].reshape(rows, M), ref[0], "perturbation form on adjacent ranges")
