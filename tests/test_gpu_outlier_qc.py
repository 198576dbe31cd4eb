"""Outlier check on the MI355X: the goldens with injected gross errors through EnSRF against the oracle run on
the flags the NumPy mask leaves (tests/_outlier.py), and every library path bit for bit against the same call with those flags
cleared on the host -- each Phase-A kind, windows, the speculative transform, geometry reuse, adaptive inflation, vertical
localisation, relaxation, shards.  Every test turns the check off again: the per-device context is shared."""
import numpy as np
import pytest

import _anderson2009 as a09
import _outlier as qc
import _vertloc as vl
from conftest import GOLDEN_CASES, load_golden
from oracle import ensrf_oracle as orc
from test_gpu_parity import _make_api_objects, assert_parity, golden_kwargs, oracle_kwargs
from test_relaxation_host import relax

pytestmark = pytest.mark.gpu

T = 3.0


def _ctx():
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    ctx.set_outlier_threshold(None)
    ctx.set_vertical_localization(None)
    ctx.set_adaptive_inflation(None)
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    for key, v in (("path", 0), ("gram", 2), ("pipeline", 1), ("gc_onepass", 1), ("geometry_reuse", 1)):
        ctx.set_option(key, v)
    return ctx


def _golden(name, n_bad=2, seed=0):
    """Golden case with n_bad requested obs moved to +-(T + 5) sigma; X (N, M), HX, the new values, the masked flags."""
    g = dict(load_golden(name))
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    X = g["X"].reshape(N, M)
    HX = (g["sten_wts"][:, :, None] * X[g["sten_idx"]]).sum(axis=1)
    value, bad = qc.inject(HX, g["ob_value"], g["ob_error"], g["ob_assim"], T, n_bad, seed=seed)
    g["ob_value"] = value
    ym, Yp = orc.compute_ob_priors(HX)
    assert qc.clear_of_threshold(ym, Yp, value, g["ob_error"], T), name + ": an ob sits within 1e-6 of the threshold"
    flags = qc.masked_flags(HX, value, g["ob_error"], g["ob_assim"], T)
    assert not flags[bad].any()
    return g, X, HX, flags


def _diag_check(what, diag, ref):
    assert_parity(np.asarray(diag["prior_mean"], float), ref["prior_mean"], what + " prior_mean")
    assert_parity(np.asarray(diag["prior_var"], float), ref["prior_var"], what + " prior_var")
    a = np.asarray(diag["assimilated"], bool)
    assert np.array_equal(a, ref["assimilated"]), what + " assimilated"
    for key in ("post_mean", "post_var"):
        assert_parity(np.asarray(diag[key], float)[a], ref[key][a], what + " " + key)


# ---- 1, 8: EnSRF.update / update_arrays on the goldens ----------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_CASES)
@pytest.mark.parametrize("path", ["transform", "sweep"])
def test_goldens_with_gross_errors_match_the_masked_oracle(name, path):
    from efa_xray_amd import EnSRF
    _ctx()
    g, X, HX, flags = _golden(name, seed=len(name))
    post, xam, Xap, rdiag = orc.ensrf_cycle(X, HX, g["ob_value"], g["ob_error"], flags, **oracle_kwargs(g))
    state, obs = _make_api_objects(g)
    requested = [o.assimilate_this for o in obs]
    try:
        got, obs = EnSRF(state, obs, verbose=False, loc=(g["loc"] or False), path=path, outlier_threshold=T).update()
        assert_parity(got.to_vect(), post, "%s %s posterior" % (name, path))
        diag = {k: np.array([getattr(o, k) if getattr(o, k) is not None else np.nan for o in obs], float)
                for k in ("prior_mean", "prior_var", "post_mean", "post_var")}
        diag["assimilated"] = np.array([o.assimilated for o in obs])
        _diag_check("%s %s" % (name, path), diag, rdiag)
        rejected = np.array(requested) & ~diag["assimilated"]
        assert np.array_equal(rejected, np.asarray(g["ob_assim"], bool) & ~flags), name + ": rejected set"
        assert [o.assimilate_this for o in obs] == requested, "assimilate_this must not be modified"
        if path == "sweep":  # 8: the host-array entry (efa_ensrf_update), perturbation form
            state, obs = _make_api_objects(g)
            xbm, Xbp = orc.format_prior_state(X, HX)
            gx, gX = EnSRF(state, obs, verbose=False, loc=(g["loc"] or False), outlier_threshold=T).update_arrays(xbm, Xbp)
            assert_parity(gx, xam, name + " update_arrays mean")
            assert_parity(gX, Xap, name + " update_arrays perturbations")
            assert np.array_equal(np.array([o.assimilated for o in obs]), rdiag["assimilated"])
    finally:
        _ctx()


# ---- 2: every Phase-A kind, bit for bit against the host-cleared flags ------------------------------------------------
def _seeded(M, P, loc, seed, N=None, n_bad=None):
    rng = np.random.default_rng(seed)
    ny, nx, nvar, nt = 8, 10, 2, 3
    N = N or nvar * nt * ny * nx
    X = rng.standard_normal((N, M)) * 2.0 + rng.standard_normal((N, 1))
    rows = rng.choice(N, P, replace=P > N)
    HX = X[rows] + 0.1 * rng.standard_normal((P, M))
    err = rng.uniform(0.5, 2.0, P)
    assim = rng.random(P) < 0.9
    value = HX.mean(axis=1) + rng.standard_normal(P)
    value, bad = qc.inject(HX, value, err, assim, T, n_bad if n_bad is not None else max(2, P // 100), seed=seed)
    kw = dict(loc_mode=0)
    if loc:
        glat, glon = np.meshgrid(np.linspace(25, 55, ny), np.linspace(240, 290, nx), indexing="ij")
        col = rows % (ny * nx)
        kw = dict(loc_mode=1, ob_lat=glat.reshape(-1)[col] + rng.uniform(-0.5, 0.5, P),
                  ob_lon=glon.reshape(-1)[col] + rng.uniform(-0.5, 0.5, P), ob_halfwidth=rng.uniform(600, 1500, P),
                  grid_lat=glat.reshape(-1), grid_lon=glon.reshape(-1), n_lead=N // (ny * nx))
    ym, Yp = orc.compute_ob_priors(HX)
    assert qc.clear_of_threshold(ym, Yp, value, err, T)
    return X, HX, value, err, assim, kw


def _okw(kw):
    """The oracle's localisation arguments for a _seeded case (an empty dict without localisation)."""
    if kw["loc_mode"] == 0:
        return {}
    return dict(loc="GC", ob_lat=kw["ob_lat"], ob_lon=kw["ob_lon"], ob_halfwidth=kw["ob_halfwidth"],
                grid_lat=kw["grid_lat"].reshape(8, 10), grid_lon=kw["grid_lon"].reshape(8, 10), state_shape=(2, 3, 8, 10))


def _cycle(ctx, X, HX, value, err, assim, kw, t=None, in_place=False):
    """efa_ensrf_cycle_dev with the obs block copied back: (posterior, ym, Yp, diagnostics)."""
    N, M = X.shape
    P = HX.shape[0]
    ctx.set_outlier_threshold(t)
    try:
        Xd = ctx.to_device(X)
        post = Xd if in_place else ctx.empty((N, M))
        Yp = ctx.to_device(HX)
        ym = ctx.empty((P,))
        ctx.form_perts(P, M, Yp, ym, Yp)
        diag = ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, value, err, assim, obs_block_out=True, **kw)
        return post.download(), ym.download(), Yp.download(), diag
    finally:
        ctx.set_outlier_threshold(None)


def _bit_equal(a, b, what):
    assert np.array_equal(a[0], b[0]), what + ": posterior"
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), what + ": obs block"
    for key in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
        assert np.array_equal(a[3][key], b[3][key], equal_nan=True), what + ": " + key


@pytest.mark.parametrize("loc", [False, True], ids=["none", "GC"])
@pytest.mark.parametrize("kind", [("band", 2, 1, 4), ("gram", 1, 1, 3), ("chain", 0, 1, 1), ("batch", 2, 0, 2)])
def test_every_phase_a_kind_bit_for_bit_as_host_cleared(kind, loc):
    from efa_xray_amd import _lib
    name, gram, pipe, want = kind
    ctx = _ctx()
    ctx.set_option("gram", gram)
    ctx.set_option("pipeline", pipe)
    ctx.set_option("path", _lib.PATH_SWEEP if loc else _lib.PATH_TRANSFORM)
    try:
        X, HX, value, err, assim, kw = _seeded(40, 400, loc, seed=17)
        flags = qc.masked_flags(HX, value, err, assim, T)
        assert flags.sum() < assim.sum()
        on = _cycle(ctx, X, HX, value, err, assim, kw, t=T)
        assert ctx.get_option("phase_a_kind") == want, "%s: phase_a_kind %d" % (name, ctx.get_option("phase_a_kind"))
        off = _cycle(ctx, X, HX, value, err, flags, kw)
        assert ctx.get_option("phase_a_kind") == want
        _bit_equal(on, off, "Phase A %s loc=%s" % (name, loc))
        post, _, _, rdiag = orc.ensrf_cycle(X, HX, value, err, flags, **_okw(kw))
        assert_parity(on[0], post, "Phase A %s vs oracle" % name)
        _diag_check("Phase A " + name, on[3], rdiag)
    finally:
        _ctx()


# ---- 3: windows --------------------------------------------------------------------------------------------------------
def test_windows_decide_once_against_the_prior():
    """20 000 obs x 20 members: several persistent windows; the flags come from the caller's block, not from rows earlier
    windows updated -- bit for bit as the host-cleared run."""
    ctx = _ctx()
    try:
        X, HX, value, err, assim, kw = _seeded(20, 20000, False, seed=23, N=64, n_bad=200)
        flags = qc.masked_flags(HX, value, err, assim, T)
        on = _cycle(ctx, X, HX, value, err, assim, kw, t=T)
        assert ctx.get_option("phase_a_kind") != 2
        off = _cycle(ctx, X, HX, value, err, flags, kw)
        _bit_equal(on, off, "windows")
        assert np.array_equal(on[3]["assimilated"], flags)
    finally:
        _ctx()


# ---- 4, 5: nothing left, nothing rejected ----------------------------------------------------------------------------
@pytest.mark.parametrize("M", [20, 200])
def test_every_ob_rejected_returns_the_prior_as_with_no_ob_assimilated(M):
    from efa_xray_amd import _lib
    ctx = _ctx()
    try:
        X, HX, value, err, assim, kw = _seeded(M, 150, False, seed=M, N=300, n_bad=0)
        ym, Yp = orc.compute_ob_priors(HX)
        value = ym + 1e3 * np.sqrt(np.var(Yp, axis=1) + err)   # every ob far out
        none = np.zeros_like(assim)
        for relax_kw in ((_lib.RELAX_NONE, 0.0), (_lib.RELAX_RTPS, 0.9)):
            ctx.set_relaxation(*relax_kw)
            for in_place in (False, True):
                on = _cycle(ctx, X, HX, value, err, assim, kw, t=T, in_place=in_place)
                off = _cycle(ctx, X, HX, value, err, none, kw, in_place=in_place)
                _bit_equal(on, off, "all rejected M=%d in_place=%s relax=%r" % (M, in_place, relax_kw))
                assert not on[3]["assimilated"].any()
                np.testing.assert_allclose(on[0], X, rtol=0, atol=1e-13 * np.abs(X).max())
        # the speculative transform guessed on the caller's flags: with M > 136 "auto" takes it above M/2 obs only, so a check
        # that leaves fewer must hand the state phase back to the sweep path
        ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
        value2, _ = qc.inject(HX, ym + 0.1 * np.sqrt(err), err, assim, T, int(0.4 * assim.sum()), seed=5)
        flags = qc.masked_flags(HX, value2, err, assim, T)
        on = _cycle(ctx, X, HX, value2, err, assim, kw, t=T)
        off = _cycle(ctx, X, HX, value2, err, flags, kw)
        _bit_equal(on, off, "partly rejected M=%d" % M)
    finally:
        _ctx()


@pytest.mark.parametrize("loc", [False, True], ids=["none", "GC"])
def test_a_threshold_that_rejects_nothing_is_bit_for_bit_off(loc):
    ctx = _ctx()
    try:
        X, HX, value, err, assim, kw = _seeded(30, 200, loc, seed=31)
        on = _cycle(ctx, X, HX, value, err, assim, kw, t=1e6)
        off = _cycle(ctx, X, HX, value, err, assim, kw)
        _bit_equal(on, off, "threshold 1e6")
        assert np.array_equal(on[3]["assimilated"], assim)
    finally:
        _ctx()


# ---- 6: geometry reuse ------------------------------------------------------------------------------------------------
def test_gc_geometry_reuse_with_a_different_rejected_set_each_cycle():
    ctx = _ctx()
    try:
        X, HX, value, err, assim, kw = _seeded(24, 300, True, seed=41, n_bad=0)
        okw = _okw(kw)
        vals = [qc.inject(HX, value, err, assim, T, 6, seed=s)[0] for s in (1, 2)]
        masks = [qc.masked_flags(HX, v, err, assim, T) for v in vals]
        assert not np.array_equal(masks[0], masks[1])
        runs = {}
        for reuse in (1, 0):
            ctx.set_option("geometry_reuse", reuse)
            runs[reuse] = [_cycle(ctx, X, HX, v, err, assim, kw, t=T) for v in vals]
        for c in range(2):
            _bit_equal(runs[1][c], runs[0][c], "cycle %d reuse 1 vs 0" % c)
            post, _, _, rdiag = orc.ensrf_cycle(X, HX, vals[c], err, masks[c], **okw)
            assert_parity(runs[1][c][0], post, "cycle %d vs oracle" % c)
            _diag_check("cycle %d" % c, runs[1][c][3], rdiag)
    finally:
        _ctx()


# ---- 7: adaptive inflation, vertical localisation, relaxation -------------------------------------------------------
def test_adaptive_inflation_learns_from_the_kept_obs_only():
    ctx = _ctx()
    g = dict(load_golden("G6"))
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    X = g["X"].reshape(N, M).copy()
    idx, wts = g["sten_idx"], g["sten_wts"]

    def H(Xi):
        return (wts[:, :, None] * Xi[idx]).sum(axis=1)
    rng = np.random.default_rng(2)
    field = np.stack([1.0 + rng.uniform(0, 1, N), np.full(N, 0.6)], axis=1)
    HXi = H(a09.inflate(X, field[:, 0]))                 # the check sees the inflated prior's obs block
    value, bad = qc.inject(HXi, g["ob_value"], g["ob_error"], g["ob_assim"], T, 3, seed=9)
    ymi, Ypi = orc.compute_ob_priors(HXi)
    assert qc.clear_of_threshold(ymi, Ypi, value, g["ob_error"], T)
    flags = qc.masked_flags(HXi, value, g["ob_error"], g["ob_assim"], T)
    post, F, rdiag, _ = a09.cycle(X, H, value, g["ob_error"], flags, g["ob_lat"], g["ob_lon"], g["ob_radius"], g["grid_lat"],
                                  g["grid_lon"], (nvar, nt, ny, nx), field)
    Xd = ctx.to_device(X)
    Fd = ctx.to_device(field)
    ctx.inflate_rows(N, M, Xd, Fd)
    Yp = ctx.to_device(H(Xd.download()))
    ym = ctx.empty((len(value),))
    ctx.form_perts(len(value), M, Yp, ym, Yp)
    ctx.set_adaptive_inflation(Fd, N)
    ctx.set_outlier_threshold(T)
    try:
        diag = ctx.ensrf_cycle(N, M, len(value), Xd, Xd, ym, Yp, value, g["ob_error"], g["ob_assim"], **golden_kwargs(g))
    finally:
        _ctx()
    assert_parity(Xd.download(), post, "adaptive posterior")
    got = Fd.download()
    assert np.max(np.abs(got - F) / np.abs(F)) <= 1e-10
    _diag_check("adaptive", diag, rdiag)


def test_vertical_localisation_and_relaxation_with_the_check():
    from efa_xray_amd import _lib
    ctx = _ctx()
    X, HX, value, err, assim, kw = _seeded(20, 150, True, seed=51)
    flags = qc.masked_flags(HX, value, err, assim, T)
    n_lead = kw["n_lead"]
    rng = np.random.default_rng(52)
    lead = np.linspace(0.0, 3.0, n_lead)
    ov, oh = rng.uniform(-0.3, 3.3, len(value)), rng.uniform(0.6, 1.2, len(value))
    N = X.shape[0]
    xbm, Xbp = orc.format_prior_state(X, HX)
    xam, Xap, rdiag = vl.ensrf_update_vert(xbm, Xbp, N, value, err, flags, kw["ob_lat"], kw["ob_lon"], kw["ob_halfwidth"],
                                           kw["grid_lat"].reshape(8, 10), kw["grid_lon"].reshape(8, 10), (2, 3, 8, 10),
                                           lead_vert=lead, ob_vert=ov, ob_vert_halfwidth=oh)
    ref = orc.format_posterior_state(xam, Xap, N)
    try:
        ctx.set_vertical_localization(lead, ov, oh)
        got = _cycle(ctx, X, HX, value, err, assim, kw, t=T)
        assert_parity(got[0], ref, "vertical posterior")
        _diag_check("vertical", got[3], rdiag)
    finally:
        _ctx()
    plain, _, _, _ = orc.ensrf_cycle(X, HX, value, err, flags, **_okw(kw))
    for name, kind, a in (("rtps", _lib.RELAX_RTPS, 0.8), ("rtpp", _lib.RELAX_RTPP, 0.5)):
        try:
            ctx.set_relaxation(kind, a)
            got = _cycle(ctx, X, HX, value, err, assim, kw, t=T)
        finally:
            _ctx()
        assert_parity(got[0], relax(X, plain, **{name: a}), name + " with the check")


# ---- 9: shards ---------------------------------------------------------------------------------------------------------
def test_two_column_shards_equal_the_unsharded_run():
    from efa_xray_amd.distributed import HipEngine, ShardedEnSRF
    _ctx()
    X, HX, value, err, assim, kw = _seeded(20, 120, True, seed=61)
    flags = qc.masked_flags(HX, value, err, assim, T)
    n_lead, ncol, M = kw["n_lead"], 80, 20
    eng = HipEngine(0)
    torch = eng.torch
    ob = dict(value=value, error=err, assim=assim, loc="GC", lat=kw["ob_lat"], lon=kw["ob_lon"], halfwidth=kw["ob_halfwidth"])
    Xl = X.reshape(n_lead, ncol, M)
    outs = []
    try:
        for bounds in ([(0, ncol)], [(0, 37), (37, ncol)]):
            parts = []
            for lo, hi in bounds:
                sh = ShardedEnSRF(eng, n_lead, ncol, M, rank=0, world_size=1, bounds=[(0, ncol)])
                sh.lo, sh.hi, sh.rows_local = lo, hi, n_lead * (hi - lo)
                Xd = torch.from_numpy(np.ascontiguousarray(Xl[:, lo:hi].reshape(-1, M))).to(eng.device)
                post = torch.empty_like(Xd)
                HXd = torch.from_numpy(HX.copy()).to(eng.device)
                diag = sh.assimilate(Xd, post, HXd, ob, kw["grid_lat"], kw["grid_lon"], outlier_threshold=T)
                torch.cuda.synchronize()
                assert np.array_equal(np.asarray(diag["assimilated"], bool), flags)
                parts.append(post.cpu().numpy().reshape(n_lead, hi - lo, M))
            outs.append(np.concatenate(parts, axis=1).reshape(-1, M))
    finally:
        eng.ctx.set_outlier_threshold(None)
        _ctx()
    assert np.array_equal(outs[0], outs[1])
    post, _, _, _ = orc.ensrf_cycle(X, HX, value, err, flags, **_okw(kw))
    assert_parity(outs[0], post, "sharded posterior")


# ---- 10: resources ----------------------------------------------------------------------------------------------------
def test_qc_prep_kernel_uses_no_scratch():
    from efa_xray_amd import _lib
    from _codeobj import kernel_table
    hits = [k for n, k in kernel_table(_lib.LIB_PATH).items() if "k_phase_a_prep_qc" in n]
    assert len(hits) == 1
    k = hits[0]
    assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0
