"""GPU parity on BASELINE.json's own workloads at their own sizes.

configs[0] is golden G1 and the headline (1e7 x 100 x 1e4) is
`test_gpu_parity.py::test_headline_size_properties`; this file covers
configs[1] (512x512 x 50 x 1000, no localisation), configs[2] (361x720x37x4 x
80 x 5000, Gaspari-Cohn) and configs[4] (1e6 x 128 x 4096, fp32 dense
contraction) and configs[3]'s WORKLOAD (the same 3-D state x 100 members x
10 000 obs, Gaspari-Cohn) on one GPU -- 30.8 GB prior + 30.8 GB posterior of the
288 GB; its sharding over 8 GPUs is host logic, covered by
tests/test_distributed_gloo.py and the logical-shard tests in tests/test_gpu_sharded.py.

An oracle run at these sizes would take hours, so each test
combines (i) the oracle on the obs block alone (Phase A is independent of the
state rows: DESIGN.md F1), (ii) the oracle on a slice of state rows carried with
the full obs block, and (iii) size-independent properties.  With localisation
the oracle uses its vector obs-obs taper (`obs_taper="vector"`), so it follows
all P obs.
Tolerance: float64 1e-10 relative (BASELINE.json north_star); fp32 contraction
|C - ref| <= 1e-4 |ref| + 2e-6 sum|a||b| against a float64 evaluation.
"""
import numpy as np
import pytest

from oracle import ensrf_oracle as orc
from test_gpu_parity import assert_parity, _ctx

pytestmark = pytest.mark.gpu


def _synthetic_state(ctx, rows, M, seed):
    X = ctx.empty((rows, M))
    ctx.fill_synthetic(rows, 0, M, seed, 3.0, X)
    return X


def test_config1_512x512_50_members_1000_obs_full_size():
    """configs[1]: single-variable 512 x 512 grid x 50 members x 1 000 obs, float64, no localisation."""
    ctx = _ctx()
    rows, M, P = 512 * 512, 50, 1000
    rng = np.random.default_rng(101)
    X = _synthetic_state(ctx, rows, M, 1001)
    pick = rng.choice(rows, P, replace=False).astype(np.int64)
    HX = ctx.empty((P, M))
    ctx.forward_stencil(rows, 0, M, X, pick[:, None], np.ones((P, 1)), HX)
    hx = HX.download()
    val = hx.mean(axis=1) + rng.standard_normal(P)
    err = rng.uniform(0.5, 2.0, P)
    asm = rng.random(P) < 0.97
    # (i) Phase A against the oracle on the obs block alone (nstate = 0)
    ym0, Yp0 = orc.compute_ob_priors(hx)
    o_ym, o_Yp, o_diag = orc.ensrf_update(ym0, Yp0, 0, val, err, asm)
    outs = {}
    try:
        for path in (2, 1):
            ctx.set_option("path", path)
            ym = ctx.empty((P,))
            Yp = ctx.to_device(hx)
            ctx.form_perts(P, M, Yp, ym, Yp)
            d = ctx.obs_phase(M, P, ym, Yp, val, err, asm)
            for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
                assert_parity(d[key], o_diag[key], "cfg1 path %d %s" % (path, key))
            assert np.array_equal(d["assimilated"], o_diag["assimilated"])
            assert_parity(Yp.download(), o_Yp, "cfg1 final obs perturbations")
            assert_parity(ym.download(), o_ym, "cfg1 final obs means")
            post = ctx.empty((rows, M))
            ctx.state_cycle(rows, M, X, post)
            assert ctx.last_timing()["path"] == path
            outs[path] = post.download()
            post.free()
    finally:
        ctx.set_option("path", 0)
    # (ii) the oracle on 2 000 state rows + the observed rows, carried with the full obs block
    sl = np.unique(np.concatenate([rng.choice(rows, 2000, replace=False), pick]))
    Xh = X.download()
    ref_post, _, _, _ = orc.ensrf_cycle(Xh[sl], hx, val, err, asm)
    for path in (2, 1):
        assert_parity(outs[path][sl], ref_post, "cfg1 path %d slice vs oracle" % path)
    # (iii) properties over the whole state: both Phase-B paths agree, no variance grows, and the
    # last assimilated ob's row reproduces its diagnostics
    a, b = outs[2], outs[1]
    assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max()
    assert (a.var(axis=1) <= Xh.var(axis=1) * (1.0 + 1e-9)).all()
    k = int(np.nonzero(asm)[0][-1])
    if not asm[k + 1:].any():
        assert abs(a[pick[k]].mean() - o_diag["post_mean"][k]) <= 1e-10 * max(1.0, abs(o_diag["post_mean"][k]))
    X.free()


def _cfg2_grid():
    ny, nx = 361, 720
    lat2, lon2 = np.meshgrid(np.linspace(-90, 90, ny), np.linspace(0, 360 - 360.0 / nx, nx), indexing="ij")
    return ny, nx, lat2, lon2


@pytest.mark.parametrize("cfg,M,P", [("cfg2", 80, 5000), ("cfg3", 100, 10000)])
def test_3d_atmosphere_gaspari_cohn_full_size(cfg, M, P):
    """configs[2]: (lat=361, lon=720, lev=37, vars=4) x 80 members x 5 000 obs, Gaspari-Cohn 1 000 km
    (state 38 468 160 rows x 80 = 24.6 GB, generated on the device), and configs[3]'s global problem on ONE GPU:
    the same state x 100 members (30.8 GB) x 10 000 obs.
      - Phase A (all obs, with the obs-obs taper, band leader) against the oracle on the obs block alone;
      - configs[2]: the one-pass active-list sweep against the per-batch taper-table sweep on sampled column slabs;
      - rows whose taper is zero for every assimilated ob come back as the prior;
      - the last ob's row reproduces its post_mean / post_var;
      - ALL P obs against the oracle (vector obs-obs taper), carrying a slab of 48 columns x 8 of the 148 variable x level
        slabs -- state rows are independent of one another, so a few slabs cost the oracle little beside the obs block --:
        all four diagnostics of every ob and the slab's posterior of the same full run; the oracle runs on a host thread
        while the GPU works;
      - a 300-ob prefix against the oracle on a slab of columns (all 148 variable x level slabs of them)."""
    from concurrent.futures import ThreadPoolExecutor
    from _phase_a_guard import GuardProbe, expected_kind
    ctx = _ctx()
    ny, nx, lat2, lon2 = _cfg2_grid()
    ncol, n_lead = ny * nx, 148
    rows = ncol * n_lead
    glat, glon = lat2.reshape(-1), lon2.reshape(-1)
    rng = np.random.default_rng(202 if cfg == "cfg2" else 303)
    X = _synthetic_state(ctx, rows, M, 1002 if cfg == "cfg2" else 1003)
    # obs between 55S and 55N so that the caps beyond 55 + 18 degrees are outside every footprint
    band = np.nonzero(np.abs(glat) <= 55.0)[0]
    ocol = rng.choice(band, P, replace=False)
    pick = (rng.integers(0, n_lead, P) * ncol + ocol).astype(np.int64)
    HX = ctx.empty((P, M))
    ctx.forward_stencil(rows, 0, M, X, pick[:, None], np.ones((P, 1)), HX)
    hx = HX.download()
    val = hx.mean(axis=1) + rng.standard_normal(P)
    err = np.ones(P)
    asm = np.ones(P, dtype=bool)
    ob_lat, ob_lon, hw = glat[ocol], glon[ocol], np.full(P, 1000.0)
    # the full-length slab: the 48 columns around the column that the most footprints (of all P obs) cover, of 200
    # candidate ob columns; the first, the last and six more of the variable x level slabs
    cand = ocol[::P // 200]
    cover = [int((orc.localize_obs_vec(ob_lat, ob_lon, glat[cc], glon[cc], hw) > 0).sum()) for cc in cand]
    cf = int(cand[int(np.argmax(cover))])
    cf = min(max(cf - 24, 0), ncol - 48)
    leads_f = [0, 21, 42, 63, 84, 105, 126, n_lead - 1]
    Xf = np.concatenate([X.download_rows(l * ncol + cf, l * ncol + cf + 48) for l in leads_f])

    def full_oracle():
        probe = GuardProbe(len(Xf), asm)
        post_f, _, _, rdf = orc.ensrf_cycle(Xf, hx, val, err, asm, loc="GC", ob_lat=ob_lat, ob_lon=ob_lon, ob_halfwidth=hw,
                                            grid_lat=glat[cf:cf + 48].reshape(1, 48), grid_lon=glon[cf:cf + 48].reshape(1, 48),
                                            state_shape=(len(leads_f), 1, 1, 48), obs_taper="vector", step_hook=probe)
        return post_f, rdf, probe.min_ratio()

    pool = ThreadPoolExecutor(1)
    fut = pool.submit(full_oracle)

    def run(n_obs, onepass, post):
        ctx.set_option("gc_onepass", onepass)
        ym = ctx.empty((n_obs,))
        Yp = ctx.to_device(hx[:n_obs])
        ctx.form_perts(n_obs, M, Yp, ym, Yp)
        d = ctx.obs_phase(M, n_obs, ym, Yp, val[:n_obs], err[:n_obs], asm[:n_obs], 1, ob_lat[:n_obs], ob_lon[:n_obs],
                          hw[:n_obs])
        ctx.state_cycle(rows, M, X, post, glat, glon, n_lead)
        return d

    def slab(arr, c0, c1):
        """rows of columns [c0, c1) for every lead, lead-major: (n_lead * (c1-c0), M)"""
        return np.concatenate([arr.download_rows(l * ncol + c0, l * ncol + c1) for l in range(n_lead)])

    post = ctx.empty((rows, M))
    try:
        # ---- full 5 000 obs, one pass -------------------------------------------------------
        d = run(P, 1, post)
        assert d["assimilated"].all()
        assert ctx.get_option("phase_a_kind") == 4, "Phase A did not run as the persistent band-leader launch"
        # Phase A vs the oracle on the obs block alone (obs-obs taper included): first 400 obs
        # (the oracle's obs-obs haversines are a Python loop, O(P^2))
        n_a = 400
        ym0, Yp0 = orc.compute_ob_priors(hx)
        sub = slice(0, n_a)
        _, _, od = orc.ensrf_update(ym0[sub], Yp0[sub], 0, val[sub], err[sub], asm[sub], loc="GC", ob_lat=ob_lat[sub],
                                    ob_lon=ob_lon[sub], ob_halfwidth=hw[sub], grid_lat=np.zeros((1, 0)),
                                    grid_lon=np.zeros((1, 0)), state_shape=(1, 1, 1, 0))
        # obs k < n_a are only influenced by earlier obs, so the prefix run's diagnostics are the full run's
        for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
            assert_parity(d[key][sub], od[key], "%s Phase A %s (first %d obs)" % (cfg, key, n_a))
        # last ob's row: taper of an ob at its own column is 1, nothing comes after it
        last = post.download_rows(int(pick[-1]), int(pick[-1]) + 1)[0]
        assert abs(last.mean() - d["post_mean"][-1]) <= 1e-10 * max(1.0, abs(d["post_mean"][-1]))
        assert abs(last.var() - d["post_var"][-1]) <= 1e-9 * max(1.0, d["post_var"][-1])
        # polar caps: |lat| > 55 + degrees(2000 km / 6371 km) = 73 -> untouched by every footprint
        for c0 in (0, 3 * nx, ncol - 5 * nx):
            pr, po = slab(X, c0, c0 + 64), slab(post, c0, c0 + 64)
            assert np.abs(po - pr).max() <= 4e-15 * np.abs(pr).max(), "zero-taper rows changed (cols %d..)" % c0
        got_f = {"one-pass": np.concatenate([post.download_rows(l * ncol + cf, l * ncol + cf + 48) for l in leads_f])}
        # sampled slabs, kept for the comparison with the per-batch taper-table path
        samples = [int(c) for c in rng.choice(ncol - 48, 5, replace=False)] + [int(ocol[-1]) - int(ocol[-1]) % 16]
        onepass = [slab(post, c0, c0 + 48) for c0 in samples]
        assert all(np.isfinite(s).all() for s in onepass)
        changed = sum(float(np.abs(s - slab(X, c0, c0 + 48)).max()) > 1e-6 for s, c0 in zip(onepass, samples))
        assert changed >= 3, "sampled slabs were not updated"
        # ---- the per-batch taper-table path (79 read+write passes) gives the same posterior ----
        if cfg == "cfg2":
            d2 = run(P, 0, post)
            assert_parity(d2["post_var"], d["post_var"], "cfg2 post_var, table path vs one-pass")
            for s, c0 in zip(onepass, samples):
                t = slab(post, c0, c0 + 48)
                assert np.abs(t - s).max() <= 1e-10 * np.abs(s).max(), "one-pass vs table path, cols %d.." % c0
            got_f["table"] = np.concatenate([post.download_rows(l * ncol + cf, l * ncol + cf + 48) for l in leads_f])
        # ---- 300-ob prefix vs the oracle on a slab of 48 columns x 148 slabs --------------------
        n_p = 300
        dp = run(n_p, 1, post)
        c0 = int(ocol[:n_p][np.argmax(np.abs(ob_lat[:n_p]))])        # around the most poleward ob: many footprints
        c0 = min(max(c0 - 24, 0), ncol - 48)
        Xs = slab(X, c0, c0 + 48)
        kw = dict(loc="GC", ob_lat=ob_lat[:n_p], ob_lon=ob_lon[:n_p], ob_halfwidth=hw[:n_p],
                  grid_lat=glat[c0:c0 + 48].reshape(1, 48), grid_lon=glon[c0:c0 + 48].reshape(1, 48),
                  state_shape=(n_lead, 1, 1, 48))
        ref_post, _, _, rd = orc.ensrf_cycle(Xs, hx[:n_p], val[:n_p], err[:n_p], asm[:n_p], **kw)
        assert_parity(slab(post, c0, c0 + 48), ref_post, cfg + " 300-ob prefix, slab vs oracle")
        assert float(np.abs(ref_post - Xs).max()) > 1e-3, "the oracle slab saw no update: test is vacuous"
        for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
            assert_parity(dp[key], rd[key], cfg + " prefix " + key)
        # ---- all P obs vs the oracle: every ob's diagnostics and the slab's posterior -------------------------
        post_f, rdf, ratio = fut.result()
        print("%s: oracle over all %d obs, slab columns %d..%d, guard min ratio %.3e" % (cfg, P, cf, cf + 47, ratio))
        assert expected_kind(ratio, M) == 4
        for key in ("prior_mean", "prior_var", "post_mean", "post_var"):
            rel = assert_parity(d[key], rdf[key], "%s Phase A %s, all %d obs" % (cfg, key, P))
            print("%s all %d obs vs oracle, %s: max rel err %.3e" % (cfg, P, key, rel))
        assert np.array_equal(d["assimilated"], rdf["assimilated"])
        for how, got in got_f.items():
            rel = assert_parity(got, post_f, "%s all %d obs, %s sweep: slab vs oracle" % (cfg, P, how))
            print("%s all %d obs vs oracle, slab posterior (%s sweep): max rel err %.3e" % (cfg, P, how, rel))
        assert float(np.abs(post_f - Xf).max()) > 1e-3, "the full-length oracle slab saw no update: test is vacuous"
    finally:
        ctx.set_option("gc_onepass", 1)
        post.free()
        X.free()
        pool.shutdown(wait=True)


def test_config4_dense_contraction_1e6_x_128_x_4096_fp32_full_size():
    """configs[4]: 1e6 state x 128 members x 4 096 obs as one (state x member).(member x obs) MFMA contraction,
    fp32; 64 random rows (and the first/last tiles) against a float64 evaluation."""
    ctx = _ctx()
    N, M, P = 1_000_000, 128, 4096
    rng = np.random.default_rng(404)
    X = rng.standard_normal((N, M), dtype=np.float32)
    Ye = rng.standard_normal((P, M), dtype=np.float32)
    dX, dY, dC = ctx.malloc_bytes(X.nbytes), ctx.malloc_bytes(Ye.nbytes), ctx.malloc_bytes(N * P * 4)
    try:
        ctx.h2d(dX, X)
        ctx.h2d(dY, Ye)
        ctx.cov_contract_f32(N, M, P, dX, dY, dC)
        ctx.synchronize()
        pick = np.unique(np.concatenate([rng.choice(N, 64, replace=False), [0, 1, 255, 256, N - 257, N - 1]]))
        import ctypes
        Ye64 = Ye.astype(np.float64)
        for r in pick:
            row = np.empty(P, dtype=np.float32)
            ctx.d2h(row, ctypes.c_void_p(dC.value + int(r) * P * 4))
            ref = Ye64 @ X[r].astype(np.float64)
            scale = np.abs(Ye64) @ np.abs(X[r].astype(np.float64))
            assert np.all(np.abs(row - ref) <= 1e-4 * np.abs(ref) + 2e-6 * scale), "row %d" % r
    finally:
        for p in (dX, dY, dC):
            ctx.free_bytes(p)
