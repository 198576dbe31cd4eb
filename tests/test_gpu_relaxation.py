"""Posterior relaxation (RTPP / RTPS) on the MI355X: the Python surface against the closed forms applied to the oracle's
posterior (goldens G1-G8, both state paths, with and without localisation), the fused transform kernels against the
standalone passes over ensemble sizes, the resident-cycle entries (speculative transform, Phase-A windows), the cases that
must stay bit for bit as without relaxation, and the sharded path."""
import numpy as np
import pytest

from conftest import load_golden, GOLDEN_CASES
from test_gpu_parity import assert_parity, _make_api_objects
from test_relaxation_host import relax, golden_oracle

pytestmark = pytest.mark.gpu


def _ctx():
    from efa_xray_amd import _lib
    return _lib.get_context(0)


def _reset(ctx):
    from efa_xray_amd import _lib
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    ctx.set_option("path", 0)


@pytest.mark.parametrize("name", GOLDEN_CASES)
@pytest.mark.parametrize("path", ["transform", "sweep"])
@pytest.mark.parametrize("kind", ["rtps", "rtpp"])
@pytest.mark.parametrize("alpha", [0.5, 0.9])
def test_update_matches_relaxed_oracle_on_goldens(name, path, kind, alpha):
    from efa_xray_amd import EnSRF
    g = load_golden(name)
    X, post = golden_oracle(g)
    state, obs = _make_api_objects(g)
    got, _ = EnSRF(state, obs, verbose=False, loc=(g["loc"] or False), path=path, **{kind: alpha}).update()
    assert_parity(got.to_vect(), relax(X, post, **{kind: alpha}), "%s %s %s=%g" % (name, path, kind, alpha))
    # the per-ob diagnostics still describe the serial loop
    assert_parity([o.prior_var for o in obs], g["prior_var"], name + " prior_var")
    for k, o in enumerate(obs):
        if o.assimilated:
            assert abs(o.post_var - g["post_var"][k]) <= 1e-10 * max(1.0, abs(g["post_var"][k]))


@pytest.mark.parametrize("kind", ["rtps", "rtpp"])
def test_update_arrays_relaxes_the_state_rows_only(kind):
    from efa_xray_amd import EnSRF
    from oracle import ensrf_oracle as orc
    g = load_golden("G4")
    X, post = golden_oracle(g)
    N, M = X.shape
    xbm, Xbp = orc.format_prior_state(X, g["HX"])
    state, obs = _make_api_objects(g)
    xam0, Xap0 = EnSRF(state, obs, verbose=False).update_arrays(xbm, Xbp)
    xam, Xap = EnSRF(state, obs, verbose=False, **{kind: 0.7}).update_arrays(xbm, Xbp)
    assert np.array_equal(xam[N:], xam0[N:]) and np.array_equal(Xap[N:], Xap0[N:]), "obs block must not be relaxed"
    assert np.array_equal(xam[:N], xam0[:N]), "the posterior mean row is not changed"
    assert_parity(xam[:N, None] + Xap[:N], relax(X, post, **{kind: 0.7}), "update_arrays " + kind)


def _seeded(N, M, P, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, 1)) + 2.0 * rng.standard_normal((N, M))
    rows = rng.choice(N, P, replace=False)
    val = X[rows].mean(axis=1) + rng.standard_normal(P)
    err = rng.uniform(0.5, 1.5, P)
    asm = rng.random(P) > 0.1
    return X, rows, val, err, asm


@pytest.mark.parametrize("M", [2, 7, 50, 99, 100, 136, 160, 256])
def test_fused_kernels_equal_standalone_passes(M):
    """One Phase A, then the state phase with each relaxation on the same trajectory: the member-form transform (RTPS fused
    up to 136 members, RTPP folded into T) against the perturbation-form transform (RTPS by the standalone passes) and the
    sweep path (both by the standalone passes), and all against the closed form of the unrelaxed posterior."""
    from efa_xray_amd import _lib
    ctx = _ctx()
    N, P = 1237, 60                                        # rows not a multiple of 16
    X, rows, val, err, asm = _seeded(N, M, P, 100 + M)
    try:
        ctx.set_option("path", 2)
        Yp = ctx.to_device(X[rows])
        ym = ctx.empty((P,))
        ctx.form_perts(P, M, Yp, ym, Yp)
        ctx.obs_phase(M, P, ym, Yp, val, err, asm)
        Xd = ctx.to_device(X)
        out = ctx.empty((N, M))

        def member(kind, alpha, path=2):
            ctx.set_option("path", path)
            ctx.set_relaxation(kind, alpha)
            ctx.state_cycle(N, M, Xd, out)
            return out.download()

        def perts(kind, alpha, path=2):
            ctx.set_option("path", path)
            ctx.set_relaxation(kind, alpha)
            xm = ctx.to_device(X.mean(axis=1))
            Xp = ctx.to_device(X - X.mean(axis=1, keepdims=True))
            xo, Xo = ctx.empty((N,)), ctx.empty((N, M))
            ctx.state_phase(N, M, xm, Xp, xo, Xo)
            return xo.download()[:, None] + Xo.download()

        base_t = member(_lib.RELAX_NONE, 0.0)
        base_s = member(_lib.RELAX_NONE, 0.0, path=1)
        for alpha in (0.5, 0.9):
            for kind, kw in ((_lib.RELAX_RTPS, dict(rtps=alpha)), (_lib.RELAX_RTPP, dict(rtpp=alpha))):
                what = "M=%d kind=%d alpha=%g" % (M, kind, alpha)
                fused = member(kind, alpha)
                assert_parity(fused, relax(X, base_t, **kw), what + " member-form transform")
                assert_parity(perts(kind, alpha), fused, what + " perturbation-form transform")
                assert_parity(member(kind, alpha, path=1), relax(X, base_s, **kw), what + " member-form sweep")
                assert_parity(perts(kind, alpha, path=1), relax(X, base_s, **kw), what + " perturbation-form sweep")
        # alpha 0 and no relaxation: bit for bit
        assert np.array_equal(member(_lib.RELAX_RTPS, 0.0), base_t)
        assert np.array_equal(member(_lib.RELAX_RTPP, 0.0), base_t)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("in_place", [False, True])
def test_resident_cycle_entry(in_place):
    """efa_ensrf_cycle_dev: out of place the transform is enqueued behind Phase A before its status is known (the fold and
    the fused RTPS kernel must go with it); in place it runs after.  Obs block and diagnostics as without relaxation."""
    from efa_xray_amd import _lib
    ctx = _ctx()
    N, M, P = 5003, 100, 300
    X, rows, val, err, asm = _seeded(N, M, P, 7)
    try:
        ctx.set_option("path", 2)
        res = {}
        for tag, kind, alpha in (("none", _lib.RELAX_NONE, 0.0), ("rtps", _lib.RELAX_RTPS, 0.8), ("rtpp", _lib.RELAX_RTPP, 0.6)):
            ctx.set_relaxation(kind, alpha)
            Xd = ctx.to_device(X)
            post = Xd if in_place else ctx.empty((N, M))
            Yp = ctx.to_device(X[rows])
            ym = ctx.empty((P,))
            ctx.form_perts(P, M, Yp, ym, Yp)
            d = ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, val, err, asm, obs_block_out=True)
            res[tag] = (post.download(), Yp.download(), ym.download(), d)
            if not in_place:
                assert np.array_equal(Xd.download(), X), "the prior must not change"
        ref = res["none"]
        for tag, kw in (("rtps", dict(rtps=0.8)), ("rtpp", dict(rtpp=0.6))):
            got = res[tag]
            assert_parity(got[0], relax(X, ref[0], **kw), tag + " posterior")
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), tag + ": obs block"
            for key in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
                assert np.array_equal(got[3][key], ref[3][key], equal_nan=True), key
    finally:
        _reset(ctx)


def test_phase_a_windows_leave_obs_block_and_diagnostics_untouched():
    """More obs than one persistent Phase-A launch (unlocalised): the windows' internal transforms of the obs rows are not
    relaxed; only the state rows are."""
    from efa_xray_amd import _lib
    ctx = _ctx()
    N, M, P = 2000, 20, 17000
    rng = np.random.default_rng(3)
    X = rng.standard_normal((N, 1)) + 2.0 * rng.standard_normal((N, M))
    HX = rng.standard_normal((P, 1)) + 2.0 * rng.standard_normal((P, M))
    val = HX.mean(axis=1) + rng.standard_normal(P)
    err = rng.uniform(0.5, 2.0, P)
    asm = rng.random(P) < 0.95
    try:
        ctx.set_option("path", 2)
        res = {}
        for tag, kind, alpha in (("none", _lib.RELAX_NONE, 0.0), ("rtps", _lib.RELAX_RTPS, 0.9), ("rtpp", _lib.RELAX_RTPP, 0.5)):
            ctx.set_relaxation(kind, alpha)
            Xd = ctx.to_device(X)
            post = ctx.empty((N, M))
            Yp = ctx.to_device(HX)
            ym = ctx.empty((P,))
            ctx.form_perts(P, M, Yp, ym, Yp)
            d = ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, val, err, asm, obs_block_out=True)
            res[tag] = (post.download(), Yp.download(), ym.download(), d)
        ref = res["none"]
        for tag, kw in (("rtps", dict(rtps=0.9)), ("rtpp", dict(rtpp=0.5))):
            got = res[tag]
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), tag + ": obs block"
            for key in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
                assert np.array_equal(got[3][key], ref[3][key], equal_nan=True), key
            assert_parity(got[0], relax(X, ref[0], **kw), tag + " posterior")
    finally:
        _reset(ctx)


def test_bit_identical_cases_and_no_context_leak():
    """alpha 0, a cycle with no assimilated ob, and a plain EnSRF after a relaxed one on the same device's context."""
    from efa_xray_amd import EnSRF
    for name in ("G4", "G5"):
        g = load_golden(name)
        loc = g["loc"] or False
        plain, _ = EnSRF(*_make_api_objects(g), verbose=False, loc=loc).update()
        for kw in (dict(rtps=0.0), dict(rtpp=0.0)):
            got, _ = EnSRF(*_make_api_objects(g), verbose=False, loc=loc, **kw).update()
            assert np.array_equal(got.to_vect(), plain.to_vect()), (name, kw)
        relaxed, _ = EnSRF(*_make_api_objects(g), verbose=False, loc=loc, rtps=0.9).update()
        assert not np.array_equal(relaxed.to_vect(), plain.to_vect())
        again, _ = EnSRF(*_make_api_objects(g), verbose=False, loc=loc).update()
        assert np.array_equal(again.to_vect(), plain.to_vect()), name + ": relaxation leaked into a later plain EnSRF"
        # nothing assimilated: the posterior exactly as without relaxation
        def unassimilated():
            state, obs = _make_api_objects(g)
            for o in obs:
                o.assimilate_this = False
            return state, obs
        none, _ = EnSRF(*unassimilated(), verbose=False, loc=loc).update()
        for kw in (dict(rtps=0.9), dict(rtpp=0.9)):
            got, _ = EnSRF(*unassimilated(), verbose=False, loc=loc, **kw).update()
            assert np.array_equal(got.to_vect(), none.to_vect()), (name, kw)


@pytest.mark.parametrize("path", ["transform", "sweep"])
def test_zero_spread_row_stays_finite_and_unchanged(path):
    from efa_xray_amd import EnSRF
    g = load_golden("G7")
    loc = g["loc"] or False
    g = dict(g)
    X = g["X"].copy()
    X.reshape(-1, X.shape[-1])[5] = 1.5                   # one state row without spread
    g["X"] = X
    plain, _ = EnSRF(*_make_api_objects(g), verbose=False, loc=loc, path=path).update()
    assert np.all(plain.to_vect()[5] == 1.5)
    for kw in (dict(rtps=0.9), dict(rtpp=0.9), dict(rtps=3.0)):
        got, _ = EnSRF(*_make_api_objects(g), verbose=False, loc=loc, path=path, **kw).update()
        v = got.to_vect()
        assert np.all(np.isfinite(v)), kw
        assert np.array_equal(v[5], plain.to_vect()[5]), kw


@pytest.mark.parametrize("loc", [False, True])
def test_two_logical_column_shards_with_rtps_equal_unsharded_bit_for_bit(loc):
    import torch
    from efa_xray_amd.distributed import ShardedEnSRF, HipEngine
    from test_gpu_sharded import _problem, _oracle
    pr = _problem(loc, row_pick=True, seed=6)
    glat, glon = pr["lat"].reshape(-1), pr["lon"].reshape(-1)
    e0 = HipEngine(0)
    s0 = ShardedEnSRF(e0, pr["n_lead"], pr["ncol"], pr["M"])
    X0 = torch.from_numpy(pr["X"]).to(e0.device)
    P0 = torch.empty_like(X0)
    s0.update(X0, P0, pr["idx"], pr["wts"], pr["ob"], glat, glon, rtps=0.9)
    torch.cuda.synchronize()
    full = P0.cpu().numpy()
    engines = [HipEngine(0), HipEngine(0)]
    shards = [ShardedEnSRF(engines[r], pr["n_lead"], pr["ncol"], pr["M"], rank=r, world_size=2) for r in range(2)]
    Xl = [torch.from_numpy(np.ascontiguousarray(pr["X"][sh.local_rows()])).to(engines[0].device) for sh in shards]
    Pl = [torch.empty_like(x) for x in Xl]
    parts = [sh.partial_estimates(x, pr["idx"], pr["wts"]) for sh, x in zip(shards, Xl)]
    torch.cuda.synchronize()
    total = parts[0] + parts[1]
    torch.cuda.synchronize()
    out = np.empty_like(full)
    for sh, x, p in zip(shards, Xl, Pl):
        sh.assimilate(x, p, total.clone(), pr["ob"], glat, glon, rtps=0.9)
        torch.cuda.synchronize()
        out[sh.local_rows()] = p.cpu().numpy()
    assert np.array_equal(out, full)
    ref_post, _ = _oracle(pr)
    assert_parity(out, relax(pr["X"], ref_post, rtps=0.9), "sharded rtps vs oracle")
    # a plain cycle on the same engine afterwards is not relaxed
    s0.update(X0, P0, pr["idx"], pr["wts"], pr["ob"], glat, glon)
    torch.cuda.synchronize()
    assert_parity(P0.cpu().numpy(), ref_post, "plain cycle after a relaxed one")
    for e in engines + [e0]:
        e.ctx.close()


def test_fused_rtps_kernel_fits_its_register_budget():
    from efa_xray_amd import _lib
    from _codeobj import kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    for part in ("k_transform_rtpsILi13ELb1ELb1E", "k_transform_rtpsILi7ELb1ELb1E", "k_transform_rtpsILi7ELb0ELb1E"):
        hits = [k for n, k in tab.items() if part in n]
        assert len(hits) == 1, part
        assert hits[0].get(".vgpr_spill_count", 0) == 0, (part, hits[0][".vgpr_count"], hits[0].get(".vgpr_spill_count"))
