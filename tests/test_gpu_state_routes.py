"""GPU test that pins the ROUTE of every state-phase call: which of transform / one-pass GC sweep / per-batch
sweeps runs, in which relaxation form, on the float32 rows themselves or through the float64 workspace, and how many launches that
takes -- for every combination of path, relaxation, localisation and entry point at three ensemble sizes.

The expectation is spelled HERE, in `expected()`, from the rules of the design and not read back from the library: it is the
second, independent statement of what `plan_state` (efa_phase_b.hip) decides.  Beside the route every case holds the float32
posterior to the bits of the float64 posterior of the same settings rounded once, and the single-call cycle to the bits of the
two-call one, in place to the bits of out of place at every size.  Only the perturbation form, which sums differently, is held to
the member form by `assert_parity` instead of bit for bit.

The problem: 3 slabs of 5 x 7 columns (35 columns: no multiple of the 16-column block), 105 rows; 12 obs of single rows of which
10 are assimilated (one sweep batch; fewer than M/2 at 138 members, more than M/8 at 6 and 7).  M = 6: even, the row-per-lane GC
kernel; 7: odd, the quad kernel; 138: above 136 the transform runs as column groups and RTPS is not fused."""
import itertools

import numpy as np
import pytest

from test_gpu_f32_state import DIAG, F32, F64, _bits, _ctx, _lib, _same, _settings
from test_gpu_parity import assert_parity

N_LEAD, NY, NX, P = 3, 5, 7, 12
NCOL, ROWS = NY * NX, N_LEAD * NY * NX
ASSIM = np.arange(P) % 5 != 2
N_ACTIVE = int(ASSIM.sum())

SIZES = [6, 7, 138]
PATHS = ["auto", "transform", "sweep"]
RELAX = ["none", "rtpp", "rtps"]
LOCS = ["none", "gc_onepass", "gc_batches"]
ENTRIES = ["state_phase", "state_cycle", "f32_out", "f32_in", "ensrf_cycle"]


def expected(M, loc, path, relax, entry):
    """(path taken, state launches, f32_native or None) by the rules of DESIGN.md 7h."""
    member = entry != "state_phase"
    f32 = entry in ("f32_out", "f32_in")
    # Phase A leaves [T | w] only unlocalised and unless the sweeps were asked for
    have_T = loc == "none" and path != "sweep"
    if path == "transform":
        want = True
    elif path == "sweep":
        want = False
    elif M > 136:
        want = N_ACTIVE > M // 2
    else:
        want = member or N_ACTIVE > M // 8
    transform = have_T and want and N_ACTIVE > 0
    onepass = not transform and loc == "gc_onepass" and N_ACTIVE > 0
    if transform:
        if relax == "none":
            form, launches = "none", 1
        elif relax == "rtpp":
            form, launches = "folded", 2            # fold + transform
        elif member and M <= 136:
            form, launches = "fused", 1
        else:
            form, launches = "standalone", 3        # spread + transform + relax
    else:
        form = "none" if relax == "none" else "standalone"
        launches = 1 + {"none": 0, "rtpp": 1, "rtps": 2}[relax]   # one pass, or one batch of obs
    native = None
    if f32:
        # (the recorded ye rows are the library's own: an even stride for an even M, 16-byte aligned)
        native = (transform and form != "standalone") or (onepass and form == "none" and M % 2 == 0 and M <= 104)
        if not native:
            launches += 2                           # widen + narrow
        native = int(native)
    return ("transform" if transform else "sweep"), launches, native


def test_expected_anchors():
    """The table of `expected` against values worked out by hand (needs no GPU)."""
    for relax, n in (("none", 1), ("rtpp", 2), ("rtps", 1)):
        assert expected(6, "none", "auto", relax, "state_cycle") == ("transform", n, None)
        assert expected(6, "none", "auto", relax, "f32_in") == ("transform", n, 1)
    assert expected(138, "none", "transform", "rtps", "state_cycle") == ("transform", 3, None)
    assert expected(138, "none", "transform", "rtps", "f32_out") == ("transform", 5, 0)
    assert expected(138, "none", "auto", "none", "state_cycle") == ("sweep", 1, None)
    assert expected(138, "none", "auto", "none", "f32_out") == ("sweep", 3, 0)
    for path in PATHS:
        assert expected(6, "gc_onepass", path, "none", "state_cycle") == ("sweep", 1, None)
        assert expected(6, "gc_onepass", path, "none", "f32_in") == ("sweep", 1, 1)
        assert expected(6, "gc_onepass", path, "rtps", "state_cycle") == ("sweep", 3, None)
        assert expected(6, "gc_onepass", path, "rtps", "f32_out") == ("sweep", 5, 0)
        assert expected(7, "gc_onepass", path, "none", "state_cycle") == ("sweep", 1, None)
        assert expected(7, "gc_onepass", path, "none", "f32_out") == ("sweep", 3, 0)


class Problem(object):
    def __init__(self, M):
        rng = np.random.default_rng(7000 + M)
        self.M = M
        lat, lon = np.meshgrid(np.linspace(30, 50, NY), np.linspace(230, 262, NX), indexing="ij")
        self.glat, self.glon = lat.reshape(-1).copy(), lon.reshape(-1).copy()
        self.X32 = (3.0 * rng.standard_normal((ROWS, 1)) + 2.0 * rng.standard_normal((ROWS, M))).astype(F32)
        self.X64 = self.X32.astype(F64)
        pick = rng.integers(0, ROWS, P)
        self.HX = self.X64[pick].copy()
        self.value = self.HX.mean(axis=1) + rng.standard_normal(P)
        self.error = rng.uniform(0.5, 1.5, P)
        self.ob_lat, self.ob_lon = self.glat[pick % NCOL], self.glon[pick % NCOL]
        self.hw = rng.uniform(600.0, 1500.0, P)


_PROBLEMS = {}


def _problem(M):
    if M not in _PROBLEMS:
        _PROBLEMS[M] = Problem(M)
    return _PROBLEMS[M]


def _run(pb, gc, entry, in_place=False):
    """One call of `entry` behind its own obs phase; returns (posterior, diagnostics, obs block, path, launches, native).  The
    perturbation form runs in place and its posterior is rebuilt on the host, means + perturbations."""
    L, ctx, M = _lib(), _ctx(), pb.M
    ym = ctx.empty((P,))
    Yp = ctx.to_device(pb.HX)
    ctx.form_perts(P, M, Yp, ym, Yp)
    obs_kw = dict(loc_mode=L.LOC_GC, ob_lat=pb.ob_lat, ob_lon=pb.ob_lon, ob_halfwidth=pb.hw) if gc else {}
    grid = dict(grid_lat=pb.glat, grid_lon=pb.glon, n_lead=N_LEAD) if gc else {}
    native = post = None
    if entry == "ensrf_cycle":
        X, out = ctx.to_device(pb.X64), ctx.empty((ROWS, M))
        diag = ctx.ensrf_cycle(ROWS, M, P, X, out, ym, Yp, pb.value, pb.error, ASSIM, obs_block_out=True, **obs_kw, **grid)
        post = out.download()
    else:
        diag = ctx.obs_phase(M, P, ym, Yp, pb.value, pb.error, ASSIM, **obs_kw)
        if entry == "state_phase":
            X = ctx.to_device(pb.X64)
            xm, Xp = ctx.empty((ROWS,)), ctx.empty((ROWS, M))
            ctx.form_perts(ROWS, M, X, xm, Xp)
            ctx.state_phase(ROWS, M, xm, Xp, xm, Xp, **grid)
            post = xm.download()[:, None] + Xp.download()
        elif entry == "state_cycle":
            X = ctx.to_device(pb.X64)
            out = X if in_place else ctx.empty((ROWS, M))
            ctx.state_cycle(ROWS, M, X, out, **grid)
            post = out.download()
        else:
            X = ctx.to_device(pb.X32, F32)
            out = X if entry == "f32_in" else ctx.empty((ROWS, M), F32)
            ctx.state_cycle_f32(ROWS, M, X, out, **grid)
            native = ctx.get_option("f32_native")
            post = out.download()
    t = ctx.last_timing()
    return post, diag, (ym.download(), Yp.download()), t["path"], t["state_launches"], native


@pytest.mark.gpu
@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", SIZES)
def test_routes(M, loc):
    L = _lib()
    pb = _problem(M)
    gc = loc != "none"
    path_opt = {"auto": L.PATH_AUTO, "transform": L.PATH_TRANSFORM, "sweep": L.PATH_SWEEP}
    relax_opt = {"none": (L.RELAX_NONE, 0.0), "rtpp": (L.RELAX_RTPP, 0.5), "rtps": (L.RELAX_RTPS, 0.5)}
    for path, relax in itertools.product(PATHS, RELAX):
        with _settings(path=path_opt[path], relax=relax_opt[relax], gc_onepass=0 if loc == "gc_batches" else 1):
            runs = {e: _run(pb, gc, e) for e in ENTRIES}
            ref = runs["state_cycle"]          # the float64 yardstick: the member form out of place
            for e in ENTRIES:
                w = "M=%d loc=%s path=%s relax=%s entry=%s" % (M, loc, path, relax, e)
                want_path, want_launches, want_native = expected(M, loc, path, relax, e)
                post, diag, obs_block, got_path, got_launches, got_native = runs[e]
                assert got_path == path_opt[want_path], w
                assert got_launches == want_launches, "%s: %d launches, expected %d" % (w, got_launches, want_launches)
                assert got_native == want_native, "%s: f32_native %r, expected %r" % (w, got_native, want_native)
                for key in DIAG:
                    assert _same(diag[key], ref[1][key]), "%s: %s" % (w, key)
                assert _same(obs_block[0], ref[2][0]) and _same(obs_block[1], ref[2][1]), w + ": obs block"
                if e in ("f32_out", "f32_in"):
                    bad = int(np.sum(_bits(post) != _bits(ref[0].astype(F32))))
                    assert bad == 0, "%s: %d of %d posterior values differ from fl32(float64 path)" % (w, bad, post.size)
                elif e == "ensrf_cycle":
                    assert _same(post, ref[0]), w + ": the single-call cycle differs from obs phase + state cycle"
                elif e == "state_phase":   # (the forms sum differently: no bit comparison)
                    assert_parity(post, ref[0], w + ": the perturbation form against the member form")
            assert np.all(np.isfinite(ref[0])) and not _same(ref[0], pb.X64)
            w = "M=%d loc=%s path=%s relax=%s float64 in place" % (M, loc, path, relax)
            got = _run(pb, gc, "state_cycle", in_place=True)
            assert (got[3], got[4]) == (ref[3], ref[4]), w
            assert _same(got[0], ref[0]), w + ": differs from out of place"
