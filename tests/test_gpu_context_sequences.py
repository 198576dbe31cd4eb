"""One efa_ctx through long mixed sequences of cycles, and on caller streams (MI355X).

Everything the context keeps from one call to the next -- the obs-geometry cache, the obs-obs taper table, the active lists and
the pointers they are keyed by, the grid mirror, the stencil image, the grow-only workspaces, deferred timing, the speculated
transform, the per-feature settings -- is exercised by plans of steps (tests/_sequences.py) run on ONE context.  Every step is
checked two ways: against `model(step)` to the suite's tolerance (assert_parity, 1e-10 of the array's scale; 1e-10 relative for
the inflation field), and bit for bit against the same step on a fresh context that is created for it and closed after it.

The second generation of plans (S.plans2) adds the slab setting, float32 rows, the streamed host cycle and calls of the impact,
diagnostic and helper entry points between the steps.  A float32 step is held to the model under the bound of
test_gpu_f32_state (one rounding) and to its fresh context bit for bit; a streamed step also to the resident cycle of the same
step on the fresh context, bit for bit; after a GC step that ran the one-pass sweep, option "gc_family" must be the
family the step's arrays imply; the calls between the steps are compared with the fresh context's bit for bit, the impact calls
and the factor table with their NumPy helpers as well.

Replay of a failing step: run_plan(seed, length, only=range(i - 3, i + 1)); run_steps(S.plans2()[k], only=...) for the second
generation."""
import numpy as np
import pytest

import _sequences as S
from oracle import ensrf_oracle as orc
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

FIELD_RTOL = 1e-10            # the inflation field, relative (test_gpu_outlier_qc.py)
KIND_DIFF_MAX = 0.02          # share of a plan's steps whose used and fresh context may differ in phase_a_kind (spin fall-back)
DEFAULTS = dict(relax=None, qc=None, ai=None, vl=None, sl=None, path=0, obs_batch=64, phase_a="band", gc_onepass=1, geometry_reuse=1,
                timing=0, stream="own")
DIAG_KEYS = ("prior_mean", "prior_var", "post_mean", "post_var")


def _lib():
    from efa_xray_amd import _lib
    return _lib


def _torch():
    import torch
    return torch


def dev(a):
    """A float64 device tensor holding `a` (at least one row is allocated: an empty tensor has no address)."""
    torch = _torch()
    a = np.ascontiguousarray(a, dtype=np.float64)
    t = torch.zeros((max(a.shape[0], 1),) + a.shape[1:], dtype=torch.float64, device="cuda:0")
    if a.shape[0]:
        t[:a.shape[0]].copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    return t


def dev32(a):
    """The same for float32 rows."""
    torch = _torch()
    a = np.ascontiguousarray(a, dtype=np.float32)
    t = torch.zeros((max(a.shape[0], 1),) + a.shape[1:], dtype=torch.float32, device="cuda:0")
    if a.shape[0]:
        t[:a.shape[0]].copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    return t


def host(ctx, t, n):
    """The first n rows of a device tensor, once the context's stream is done."""
    ctx.synchronize()
    return t[:n].cpu().numpy()


def ctx_array(made, ctx, a):
    """A device array of the context holding `a`, added to the list its caller frees."""
    made.append(ctx.to_device(np.ascontiguousarray(a, dtype=np.float64)))
    return made[-1]


def same_value(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b, equal_nan=True)
    return a == b


class Runner(object):
    """Drives one context through steps.  Settings are sent to the context only when they differ from what it holds (a setting
    that leaks into the next cycle then shows), except the vertical arrays, the slab arrays and the inflation field, which are
    handed over again whenever they are on (keep "sl_off_on": cleared first)."""

    def __init__(self, ctx, caller_stream=None, read_timing=True):
        self.ctx = ctx
        self.caller = caller_stream or _torch().cuda.Stream()
        self.have = dict(DEFAULTS)
        self.field = None          # the device inflation field the context points to: alive while it is set
        self.read_timing = read_timing

    def settings(self, s):
        lib, ctx, have = _lib(), self.ctx, self.have
        if s["stream"] != have["stream"]:
            if s["stream"] == "own":
                ctx.use_own_stream()
            else:
                ctx.set_stream(self.caller.cuda_stream if s["stream"] == "caller" else 0)
        for key in ("path", "obs_batch", "gc_onepass", "geometry_reuse", "timing"):
            if s[key] != have[key]:
                ctx.set_option(key, s[key])
        if s["phase_a"] != have["phase_a"]:
            ctx.set_option("pipeline", S.PHASE_A[s["phase_a"]][0])
            ctx.set_option("gram", S.PHASE_A[s["phase_a"]][1])
        if s["relax"] != have["relax"]:
            if s["relax"] is None:
                ctx.set_relaxation(lib.RELAX_NONE, 0.0)
            else:
                ctx.set_relaxation(lib.RELAX_RTPS if s["relax"][0] == "rtps" else lib.RELAX_RTPP, s["relax"][1])
        if s["qc"] != have["qc"]:
            ctx.set_outlier_threshold(s["qc"])
        if s["ai"] is not None:
            a = s["ai"]
            self.field = dev(a["field"])
            ctx.set_adaptive_inflation(self.field.data_ptr(), a["field"].shape[0], a["lower"], a["upper"], a["sd_lower"])
        elif have["ai"] is not None:
            ctx.set_adaptive_inflation(None)
            self.field = None
        if s["vl"] is not None:
            ctx.set_vertical_localization(*s["vl"])
        elif have["vl"] is not None:
            ctx.set_vertical_localization(None)
        if s["sl"] is not None:
            if s.get("keep") == "sl_off_on":
                ctx.set_slab_localization(None)
            ctx.set_slab_localization(**s["sl"])
        elif have["sl"] is not None:
            ctx.set_slab_localization(None)
        for key in DEFAULTS:
            have[key] = s[key]

    def reset(self):
        """Everything back to the defaults of a new context."""
        self.settings(dict(DEFAULTS))

    def forget(self):
        """Someone else has used the context (the Python surface sets what it needs on every call and leaves it there): every
        setting is sent again with the next step."""
        self.have = dict.fromkeys(DEFAULTS, "unknown")

    @staticmethod
    def ob_kw(c):
        if not c["loc"]:
            return dict(loc_mode=0)
        return dict(loc_mode=1, ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"])

    @staticmethod
    def grid_kw(c):
        if not c["loc"]:
            return {}
        return dict(grid_lat=c["lat"].reshape(-1), grid_lon=c["lon"].reshape(-1), n_lead=c["n_lead"])

    def run(self, s):
        """One valid step.  Returns dict(post, ym, Yp (None where the entry point returns no obs block), diag, field, kind,
        path, launches)."""
        import _anderson2009 as a09
        ctx = self.ctx
        self.settings(s)
        c = s["case"]
        N, M, P = c["N"], c["M"], c["P"]
        okw, gkw = self.ob_kw(c), self.grid_kw(c)
        entry = s["entry"]
        out = dict(ym=None, Yp=None, field=None)
        if entry == "host":
            Xi, HX = S.prior_and_obs(s)          # (prior inflation on the host: a09.inflate)
            xbm, Xbp = orc.format_prior_state(Xi, HX)
            xbm, Xbp = np.ascontiguousarray(xbm), np.ascontiguousarray(Xbp)
            out["diag"] = ctx.ensrf_update_host(xbm, Xbp, N, c["val"], c["err"], c["asm"], **dict(okw, **gkw))
            out.update(post=orc.format_posterior_state(xbm, Xbp, N), ym=xbm[N:].copy(), Yp=Xbp[N:].copy())
        elif entry == "host_streamed":
            out.update(self.streamed(s))
        elif entry == "state_cycle_f32":
            X = dev32(c["X"])
            Yp, ym = dev(c["HX"]), dev(np.zeros(P))
            if P:
                ctx.form_perts(P, M, Yp.data_ptr(), ym.data_ptr(), Yp.data_ptr())
            post = X if s["in_place"] else dev32(np.full((N, M), 9.0))
            out["diag"] = ctx.obs_phase(M, P, ym.data_ptr(), Yp.data_ptr(), c["val"], c["err"], c["asm"], **okw)
            ctx.state_cycle_f32(N, M, X.data_ptr(), post.data_ptr(), **gkw)
            out.update(post=host(ctx, post, N), ym=host(ctx, ym, P), Yp=host(ctx, Yp, P))
            if not s["in_place"]:
                assert np.array_equal(host(ctx, X, N), c["X"].astype(np.float32)), "the float32 prior was written"
        else:
            X = dev(c["X"])
            if s["ai"] is not None:              # prior inflation on the device, the forward operator on the inflated prior
                ctx.inflate_rows(N, M, X.data_ptr(), self.field.data_ptr())
                Xi = host(ctx, X, N)
                assert_parity(Xi, a09.inflate(c["X"], s["ai"]["field"][:, 0]), "inflated prior")
                HX = S.forward(c)(Xi)
            else:
                HX = c["HX"]
            Yp = dev(HX)
            ym = dev(np.zeros(P))
            if P:
                ctx.form_perts(P, M, Yp.data_ptr(), ym.data_ptr(), Yp.data_ptr())
            ob = (c["val"], c["err"], c["asm"])
            if entry in ("update_dev", "phases_in", "phases_out"):
                xm = dev(np.zeros(N))
                Xp = dev(np.zeros((N, M)))
                if N:
                    ctx.form_perts(N, M, X.data_ptr(), xm.data_ptr(), Xp.data_ptr())
                prior = (host(ctx, xm, N), host(ctx, Xp, N))
                xo, Xo = (dev(np.zeros(N)), dev(np.zeros((N, M)))) if entry == "phases_out" else (xm, Xp)
                if entry == "update_dev":
                    out["diag"] = ctx.ensrf_update_dev(N, M, P, xm.data_ptr(), Xp.data_ptr(), ym.data_ptr(), Yp.data_ptr(), *ob,
                                                       **dict(okw, **gkw))
                else:
                    out["diag"] = ctx.obs_phase(M, P, ym.data_ptr(), Yp.data_ptr(), *ob, **okw)
                    ctx.state_phase(N, M, xm.data_ptr(), Xp.data_ptr(), xo.data_ptr(), Xo.data_ptr(), **gkw)
                out["post"] = host(ctx, xo, N)[:, None] + host(ctx, Xo, N)
                if entry == "phases_out":
                    assert np.array_equal(host(ctx, xm, N), prior[0]) and np.array_equal(host(ctx, Xp, N), prior[1]), \
                        "the out-of-place state phase wrote to its input"
            else:
                post = X if entry == "cycle_in" else dev(np.zeros((N, M)))
                if entry == "state_cycle":
                    out["diag"] = ctx.obs_phase(M, P, ym.data_ptr(), Yp.data_ptr(), *ob, **okw)
                    ctx.state_cycle(N, M, X.data_ptr(), post.data_ptr(), **gkw)
                else:
                    before = (host(ctx, ym, P), host(ctx, Yp, P))
                    out["diag"] = ctx.ensrf_cycle(N, M, P, X.data_ptr(), post.data_ptr(), ym.data_ptr(), Yp.data_ptr(), *ob,
                                                  obs_block_out=s["obs_block_out"], **dict(okw, **gkw))
                    if not s["obs_block_out"]:
                        assert np.array_equal(before[0], host(ctx, ym, P)) and np.array_equal(before[1], host(ctx, Yp, P)), \
                            "obs_block_out 0 must leave the obs block as it came"
                out["post"] = host(ctx, post, N)
                if entry != "cycle_in":
                    assert np.array_equal(host(ctx, X, N), Xi if s["ai"] is not None else c["X"]), "the prior was written"
            if entry not in ("cycle_in", "cycle_out") or s["obs_block_out"]:
                out.update(ym=host(ctx, ym, P), Yp=host(ctx, Yp, P))
        if s["ai"] is not None:
            out["field"] = host(ctx, self.field, N)
        ctx.synchronize()
        out["kind"] = int(ctx.get_option("phase_a_kind")) if P else 0
        if self.read_timing:
            t = ctx.last_timing()
            # (a call without obs or without rows returns before the state phase says which path it takes)
            out["path"], out["launches"] = (t["path"], t["state_launches"]) if N and P else (0, 0)
        else:
            out["path"], out["launches"] = None, None
        if c["loc"] and s["gc_onepass"] == 1 and N and np.any(out["diag"]["assimilated"]):
            # the state phase ran the one-pass sweep: the kernel family is the one the step's arrays imply
            fam = int(ctx.get_option("gc_family"))
            assert fam == S.gc_family(s), "gc_family %d, the step's settings imply %d" % (fam, S.gc_family(s))
            out["pairs"] = int(ctx.get_option("gc_active_pairs"))
        out["after"] = dict((b, self.bystander(b, s, out)) for b in s.get("after", ()))
        return out

    def streamed(self, s):
        """efa_ensrf_cycle_host(_f32): the state in host memory, one segment per variable, pinned and ordinary arrays in turn."""
        ctx, c = self.ctx, s["case"]
        N, M, P = c["N"], c["M"], c["P"]
        dt = np.float32 if s["elem"] == "f32" else np.float64
        nvar = c["state_shape"][0] if c["loc"] else 1
        nt = c["n_lead"] // nvar
        ncol = N // c["n_lead"]
        X3 = c["X"].astype(dt).reshape(c["n_lead"], ncol, M)
        prior, post = [], []
        for v in range(nvar):
            seg = X3[v * nt:(v + 1) * nt]
            a, b = (ctx.pinned_empty(seg.shape, dt), ctx.pinned_empty(seg.shape, dt)) if v % 2 == 0 else \
                (np.empty(seg.shape, dtype=dt), np.empty(seg.shape, dtype=dt))
            a[...] = seg
            b[...] = 9.0
            prior.append(a)
            post.append(b)
        chunk = ncol + 5 if s["chunk_cols"] == "all" else s["chunk_cols"]
        kw = self.ob_kw(c)
        if c["loc"]:
            kw.update(grid_lat=c["lat"].reshape(-1), grid_lon=c["lon"].reshape(-1))
        diag = ctx.ensrf_cycle_host(prior, post, ncol, M, c["HX"] if P else None, chunk, c["val"], c["err"], c["asm"], **kw)
        for v in range(nvar):
            assert np.array_equal(prior[v], X3[v * nt:(v + 1) * nt]), "the streamed cycle wrote to its prior"
        return dict(diag=diag, post=np.concatenate([b.reshape(-1, M) for b in post]).copy())

    def bystander(self, name, s, out):
        """One call between this step and the next.  The impact calls and the factor table work on the step's posterior and
        settings and are checked against their NumPy helpers here; the others on a small state of their own.  Returns what the
        call gave, for the comparison with the fresh context."""
        import _efso
        import _efso_slab
        import _slabloc
        ctx, c = self.ctx, s["case"]
        N, M, P = c["N"], c["M"], c["P"]
        rng = np.random.default_rng([s["index"], (S.BYSTANDERS + S.DIRECTED_BYSTANDERS).index(name)])
        if name in ("obs_impact", "obs_impact_slab"):
            Xf = np.asarray(out["post"], dtype=np.float64)
            Ya = S.forward(c)(Xf)
            werr = rng.standard_normal(N)
            werr[::7] = 0.0
            innov = c["val"] - c["HX"].mean(axis=1)
            used = np.asarray(out["diag"]["assimilated"], dtype=bool)
            Xd, wd, Yd = ctx.to_device(Xf), ctx.to_device(werr), ctx.to_device(Ya)
            try:
                J = getattr(ctx, name)(N, M, P, Xd, wd, Yd, innov, c["err"], used, **dict(self.ob_kw(c), **self.grid_kw(c)))
            finally:
                for d in (Xd, wd, Yd):
                    d.free()
            geo = dict(grid_lat=c["lat"], grid_lon=c["lon"], ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"],
                       n_lead=c["n_lead"]) if c["loc"] else {}
            if s["vl"] is not None:
                geo.update(lead_vert=s["vl"][0], ob_vert=s["vl"][1], ob_vert_halfwidth=s["vl"][2])
            if s["sl"] is not None:
                kw = S.slab_arrays(s["sl"])
                kw.pop("ob_var", None)
                ref, A = _efso_slab.efso_slab(Xf, Ya, werr, innov, c["err"], used, **dict(geo, **kw))
            else:
                ref, A = _efso.efso(Xf, Ya, werr, innov, c["err"], used, **geo)
            tol = _efso.tolerance(N, M)
            assert np.all(np.abs(J - ref) <= tol * A), "%s after the step: worst |J - ref| / A = %.3e (bound %.3e)" % (
                name, float(np.max(np.abs(J - ref) / np.where(A > 0, A, 1.0))), tol)
            assert np.all(J[~used] == 0.0)
            return J
        if name == "obs_impact_slab_other_vl":
            # the impact call under other vertical half-widths brings the factor table's cache to THAT pair of settings; the
            # original half-widths are set again behind it, and the next cycle must rebuild the table
            lead, ov, oh = s["vl"]
            other = dict(s, vl=(lead, ov, 0.5 * oh))
            ctx.set_vertical_localization(*other["vl"])
            try:
                return self.bystander("obs_impact_slab", other, out)
            finally:
                ctx.set_vertical_localization(*s["vl"])
        if name == "slab_factor_table":
            tab = ctx.slab_factor_table(P, c["n_lead"])
            ref = S.slab_table(s)
            assert tab.shape == ref.shape and np.array_equal(tab == 0.0, ref == 0.0), "factor table: zeros"
            nz = ref != 0.0
            assert not nz.any() or np.max(np.abs(tab[nz] - ref[nz]) / ref[nz]) <= 1e-15, "factor table"
            return tab
        if name == "gc_block_counts":
            o = S.new_case(4200 + s["index"], 2 * 150, 20, 77, True, ncol=150)
            cnt, bp, pairs = ctx.gc_block_counts(o["lat"], o["lon"], o["ob_lat"], o["ob_lon"], o["hw"], o["asm"])
            assert pairs == int(bp.sum())
            return cnt, bp
        n_lead, ny, nx, Mz = 2, 5, 7, 10
        rows = n_lead * ny * nx
        Z = 2.0 * rng.standard_normal((rows, Mz)) + rng.standard_normal((rows, 1))
        y = rng.standard_normal(rows)
        Zd = ctx.to_device(Z)
        made = [Zd]

        def field(*shape):
            made.append(ctx.to_device(np.full(shape, -7.0)))
            return made[-1]
        try:
            if name == "forward_stencil":
                idx, wts = rng.integers(0, rows, (30, 3)), rng.random((30, 3))
                HX = field(30, Mz)
                ctx.forward_stencil(rows, 0, Mz, Zd, idx, wts, HX)
                res = HX.download()
                assert_parity(res, _numpy_stencil(Z, idx, wts), "forward stencil after the step")
                return res
            if name == "gram":
                G, n, n_bad, sums = ctx.gram(rows, Mz, Zd, [1.0, 0.5], ncol=ny * nx, n_lead=n_lead)
                return G, n, n_bad, sums
            if name == "products":
                mean, sd, quant, prob = field(rows), field(rows), field(2, rows), field(1, rows)
                ctx.products(rows, Mz, Zd, ncol=ny * nx, n_lead=n_lead, quantiles=(0.1, 0.5), thresholds=np.zeros((n_lead, 1)),
                             mean=mean, sd=sd, quant=quant, prob=prob)
                return tuple(d.download() for d in (mean, sd, quant, prob))
            if name == "verify":
                crps = field(rows)
                res = ctx.verify(rows, Mz, Zd, ctx_array(made, ctx, y), [0, 1], ncol=ny * nx, n_lead=n_lead, crps=crps)
                return tuple(res) + (crps.download(),)
            if name == "neighbourhood":
                nep = field(1, rows)
                ctx.neighbourhood(rows, Mz, Zd, ny, nx, n_lead, np.zeros((n_lead, 1)), [1], nep=nep)
                return nep.download()
            if name == "pm_mean":
                pm = field(rows)
                n_bad = ctx.pm_mean(rows, Mz, Zd, ny, nx, n_lead, ctx_array(made, ctx, y), pm)
                return n_bad, pm.download()
            if name == "sensitivity":
                var, sens = field(rows), field(2, rows)
                res = ctx.sensitivity(rows, Mz, Zd, rng.standard_normal((2, Mz)), [1.0, 2.0], ncol=ny * nx, n_lead=n_lead, var=var,
                                      sens=sens)
                return tuple(res) + (var.download(), sens.download())
            raise KeyError(name)
        finally:
            for d in made:
                d.free()

    def refuse(self, s):
        """A refusal step: the call the header says must fail returns EFA_ERR_INVALID and leaves the caller's buffers alone."""
        lib, ctx = _lib(), self.ctx
        c = s["case"]
        N, M, P = c["N"], c["M"], c["P"]
        kind = s["refusal"]
        self.settings(s)
        Mx = M + 1 if kind == "state_cycle_m" else M
        rng = np.random.default_rng(P)
        Xh = c["X"] if Mx == M else rng.standard_normal((N, Mx))
        X, post = dev(Xh), dev(np.full((N, Mx), 7.0))
        Yp, ym = dev(c["HX"]), dev(np.zeros(P))
        ctx.form_perts(P, M, Yp.data_ptr(), ym.data_ptr(), Yp.data_ptr())
        ob = (c["val"], c["err"], c["asm"])
        okw, gkw = self.ob_kw(c), self.grid_kw(c)
        before = [host(ctx, t, t.shape[0]) for t in (X, post, Yp, ym)] + ([host(ctx, self.field, self.field.shape[0])]
                                                                          if self.field is not None else [])

        def must_fail(call, *a, **kw):
            with pytest.raises(lib.EfaError) as e:
                call(*a, **kw)
            assert e.value.status == lib.EFA_ERR_INVALID, str(e.value)

        if kind == "state_cycle_m":
            ctx.obs_phase(M, P, ym.data_ptr(), Yp.data_ptr(), *ob, **okw)          # valid, M members
            before[2], before[3] = host(ctx, Yp, P), host(ctx, ym, P)
            must_fail(ctx.state_cycle, N, Mx, X.data_ptr(), post.data_ptr(), **gkw)
        elif kind == "nan_hw":
            must_fail(ctx.obs_phase, M, P, ym.data_ptr(), Yp.data_ptr(), *ob, **okw)
            must_fail(ctx.state_cycle, N, M, X.data_ptr(), post.data_ptr(), **gkw)  # no trajectory
            xm = dev(np.zeros(N))
            must_fail(ctx.state_phase, N, M, xm.data_ptr(), X.data_ptr(), xm.data_ptr(), post.data_ptr(), **gkw)
        elif kind == "impact_plain_entry_under_sl":
            # efa_obs_impact_dev while the slab setting is on (efa_obs_impact_slab_dev is the impact under these tapers)
            werr = dev(np.ones(N))
            must_fail(ctx.obs_impact, N, M, P, X.data_ptr(), werr.data_ptr(), Yp.data_ptr(), np.zeros(P), c["err"], c["asm"],
                      **dict(okw, **gkw))
        elif kind == "f32_with_ai":
            # the obs phase is valid under the field; the float32 state cycle is float64 only there
            X32, post32 = dev32(c["X"]), dev32(np.full((N, M), 7.0))
            ctx.obs_phase(M, P, ym.data_ptr(), Yp.data_ptr(), *ob, **okw)
            before[2], before[3] = host(ctx, Yp, P), host(ctx, ym, P)
            must_fail(ctx.state_cycle_f32, N, M, X32.data_ptr(), post32.data_ptr(), **gkw)
            assert np.array_equal(host(ctx, X32, N), c["X"].astype(np.float32)) and np.all(host(ctx, post32, N) == 7.0), \
                "a refused call wrote to the caller's float32 rows"
        else:
            must_fail(ctx.ensrf_cycle, N, M, P, X.data_ptr(), post.data_ptr(), ym.data_ptr(), Yp.data_ptr(), *ob,
                      obs_block_out=True, **dict(okw, **gkw))
            # (the obs phase alone checks the vertical and the slab setting, but for the number of slabs; the adaptive one needs
            # the rows)
            if s["vl"] is not None or (s["sl"] is not None and kind != "sl_other_nlead"):
                must_fail(ctx.obs_phase, M, P, ym.data_ptr(), Yp.data_ptr(), *ob, **okw)
        after = [host(ctx, t, t.shape[0]) for t in (X, post, Yp, ym)] + ([host(ctx, self.field, self.field.shape[0])]
                                                                         if self.field is not None else [])
        for a, b in zip(before, after):
            assert np.array_equal(a, b), "a refused call wrote to the caller's buffers"


def parity(got, ref, what):
    """assert_parity; an array the reference leaves NaN throughout (post_mean when no ob is assimilated) has no scale to
    compare against: then the NaN pattern is the whole check."""
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size and np.all(np.isnan(ref)):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == ref.shape and np.all(np.isnan(got)), what + ": NaN pattern"
        return 0.0
    return assert_parity(got, ref, what)


def check_against_model(s, got, m, what):
    """Returns the worst relative error of the step.  A float32 step's posterior is held to the bound of test_gpu_f32_state: half
    a float32 ulp of the one rounding plus the float64 tolerance (its share of the worst error is not in the figure returned)."""
    if s.get("elem", "f64") == "f32":
        import test_gpu_f32_state as f32t
        assert got["post"].dtype == np.float32 and got["post"].shape == m["post"].shape, what + " posterior: float32 rows"
        if m["post"].size:
            f32t._assert_reference_bound(got["post"], m["post"], what + " posterior")
        worst = 0.0
    else:
        worst = assert_parity(got["post"], m["post"], what + " posterior")
    for key in DIAG_KEYS:
        worst = max(worst, parity(np.asarray(got["diag"][key], float), m["diag"][key], what + " " + key))
    assert np.array_equal(np.asarray(got["diag"]["assimilated"], bool), m["diag"]["assimilated"]), what + " assimilated"
    if got["ym"] is not None:
        worst = max(worst, assert_parity(got["ym"], m["ym"], what + " final obs means"))
        worst = max(worst, assert_parity(got["Yp"], m["Yp"], what + " final obs perturbations"))
    if m["field"] is not None:
        err = np.abs(got["field"] - m["field"]) / np.maximum(np.abs(m["field"]), 1e-300)
        e = float(err.max()) if err.size else 0.0
        assert e <= FIELD_RTOL, "%s: inflation field relative error %.3e" % (what, e)
        worst = max(worst, e)
    return worst


OWN_ARGUMENTS = ("gram", "products", "verify", "neighbourhood", "pm_mean", "sensitivity", "gc_block_counts", "forward_stencil",
                 "slab_factor_table")      # bystanders that do not read the step's posterior


def check_against_fresh(got, fresh, what, keys=("post", "ym", "Yp", "field")):
    """Bit for bit when both contexts ran the same kernels; returns 1 if they differ in kind (then: parity only, and none for
    float32 rows, whose one rounding the model's bound covers).  The calls after the step: bit for bit too."""
    same_kernels = got["kind"] == fresh["kind"] and got["path"] == fresh["path"]
    for b, v in got.get("after", {}).items():
        if same_kernels or b in OWN_ARGUMENTS:
            assert same_value(v, fresh["after"][b]), "%s: %s after the step differs from a fresh context's" % (what, b)
    if same_kernels:
        for key in keys:
            assert same_value(got[key], fresh[key]), "%s: %s differs from a fresh context's" % (what, key)
        for key in DIAG_KEYS + ("assimilated",):
            assert same_value(np.asarray(got["diag"][key]), np.asarray(fresh["diag"][key])), \
                "%s: %s differs from a fresh context's" % (what, key)
        return 0
    for key in keys:
        if got[key] is not None and got[key].dtype != np.float32:
            assert_parity(got[key], fresh[key], what + " " + key + " (other Phase-A kind than the fresh context)")
    return 1


def resident_form(s):
    """The resident step a streamed step must equal bit for bit: efa_ensrf_cycle_dev on disjoint buffers, or obs
    phase + efa_state_cycle_f32_dev for float32 rows."""
    return dict(s, entry="cycle_out" if s["elem"] == "f64" else "state_cycle_f32", in_place=False, chunk_cols=None, after=())


def run_steps(steps, ctx=None, only=None, stats=None, results=None):
    """The steps on one context (a new one unless given), each against the model and against a fresh context.
    only: indices to run (replay); stats: dict the counters are added to; results: list the used context's outputs are added to."""
    lib, torch = _lib(), _torch()
    own_ctx = ctx is None
    if own_ctx:
        ctx = lib.Context(0)
    stats = stats if stats is not None else {}
    for key in ("steps", "refusals", "kind_differs"):
        stats.setdefault(key, 0)
    stats.setdefault("worst", 0.0)
    caller = torch.cuda.Stream()
    used = Runner(ctx, caller)
    try:
        for i, s in enumerate(steps):
            if only is not None and i not in only:
                continue
            what = "seed %s %s" % (s["seed"], S.describe(s))
            try:
                if s["refusal"]:
                    used.refuse(s)
                    stats["refusals"] += 1
                    continue
                got = used.run(s)
                if results is not None:
                    results.append(got)
                stats["worst"] = max(stats["worst"], check_against_model(s, got, S.model(s), what))
                fctx = lib.Context(0)
                try:
                    fresh = Runner(fctx, caller).run(s)
                    resident = Runner(fctx, caller).run(resident_form(s)) if s["entry"] == "host_streamed" else None
                    fctx.synchronize()
                finally:
                    fctx.close()
                differs = check_against_fresh(got, fresh, what)
                if resident is not None:
                    differs = max(differs, check_against_fresh(dict(got, after={}), resident, what + " (resident)", keys=("post",)))
                stats["kind_differs"] += differs
                stats["steps"] += 1
            except lib.EfaError as e:
                raise AssertionError("%s: the library refused the step: %s" % (what, e))
    finally:
        ctx.synchronize()
        torch.cuda.synchronize()
        if own_ctx:
            used.field = None
            torch.cuda.empty_cache()
            before = torch.cuda.mem_get_info(0)[0]
            ctx.close()
            stats["given_back"] = torch.cuda.mem_get_info(0)[0] - before     # device memory the context held until close()
        else:
            used.reset()
    return stats


def workspace_floor(steps):
    """Bytes a context that ran these steps must hold at the end, from the sizes alone: its workspaces only grow, so it still has
    the largest recorded obs rows (Ye_rec, [P][M]) and the largest working obs block (Yw, at least [P][M]), the largest state
    copy of the host entry point (h_Xp, [N][M]) and, after a localised cycle of more obs than one persistent launch takes
    (256 workgroups x 64 rows), the obs-obs taper table of one full window (16384 x 16384 doubles)."""
    valid = [s["case"] for s in steps if not s["refusal"]]
    floor = 2 * 8 * max(c["P"] * c["M"] for c in valid)
    floor += 8 * max([c["N"] * c["M"] for s, c in ((s, s["case"]) for s in steps if not s["refusal"]) if s["entry"] == "host"] or [0])
    if any(c["loc"] and c["P"] > 16384 for c in valid):
        floor += 8 * 16384 * 16384
    return floor


def run_plan(seed, length, only=None):
    return run_steps(S.make_plan(seed, length), only=only)


# ---- a. random plans --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,length", S.PLANS)
def test_random_plan_on_one_context(seed, length):
    plan = S.make_plan(seed, length)
    stats = run_steps(plan)
    # close() gives the device back what the context held: at least what the plan's sizes say it must still hold (its workspaces
    # only grow).  Measured around close() itself, so that what the runtime allocates once per process (code objects, scratch,
    # signal pools: some 400 MiB over a first plan) stays out of it.
    floor = workspace_floor(plan)
    print("plan (%d, %d): %d steps, %d refusals, %d differed in phase_a_kind from the fresh context, worst relative error %.3e, "
          "close() gave back %.1f MiB (the sizes say at least %.1f)" % (seed, length, stats["steps"], stats["refusals"],
                                                                        stats["kind_differs"], stats["worst"],
                                                                        stats["given_back"] / 2**20, floor / 2**20))
    assert stats["steps"] == length and stats["refusals"] >= 1
    assert stats["kind_differs"] <= KIND_DIFF_MAX * length, "%d of %d steps ran another Phase-A kind than a fresh context" % (
        stats["kind_differs"], length)
    assert stats["given_back"] >= floor, "close() gave back %.1f MiB, the context held at least %.1f" % (
        stats["given_back"] / 2**20, floor / 2**20)


@pytest.mark.parametrize("k", range(len(S.PLANS2)), ids=["%d-%d-%d" % key for key in S.PLANS2])
def test_second_generation_plan_on_one_context(k):
    """The plans with the slab setting, float32 rows, the streamed cycle and the calls between the steps (S.plans2)."""
    plan = S.plans2()[k]
    seed, length, _ = S.PLANS2[k]
    stats = run_steps(plan)
    print("plan %r: %d steps, %d refusals, %d differed in phase_a_kind from the fresh context (at most %d may), worst relative "
          "error %.3e" % (S.PLANS2[k], stats["steps"], stats["refusals"], stats["kind_differs"], int(KIND_DIFF_MAX * length),
                          stats["worst"]))
    assert stats["steps"] == length and stats["refusals"] >= 3
    assert stats["kind_differs"] <= KIND_DIFF_MAX * length, "%d of %d steps ran another Phase-A kind than a fresh context" % (
        stats["kind_differs"], length)


# ---- b. directed transitions -------------------------------------------------------------------------------------------------
def _gc(seed=808, n_lead=4, ncol=600, M=40, P=150):
    return S.new_case(seed, n_lead * ncol, M, P, True, ncol=ncol)


def _seq(cases_and_kw):
    return [S.make_step(c, index=i, seed="directed", **kw) for i, (c, kw) in enumerate(cases_and_kw)]


_DIRECTED = {}


def directed_sequences():
    """name -> steps.  Each comes from reading which keys one cache compares."""
    if not _DIRECTED:
        _DIRECTED.update(_directed_sequences())
    return _DIRECTED


def _directed_sequences():
    rng = np.random.default_rng(99)
    seqs = {}
    base = _gc()
    moved = S.revalue(base, rng)
    moved["lat"] = base["lat"] + 0.5
    # 1. same obs, same ncol, grid VALUES changed, then the same again: grid_serial and the pinned mirror, through both grid paths
    for entry in ("cycle_out", "state_cycle"):
        seqs["grid values changed, %s" % entry] = _seq([(base, dict(entry=entry)), (moved, dict(entry=entry, keep="grid")),
                                                        (S.revalue(moved, rng), dict(entry=entry, keep="values")),
                                                        (base, dict(entry=entry, keep="grid"))])
    # 2. does the geometry cache survive a cycle that never looked at it
    other = S.new_case(5, 900, 64, 65, False)
    seqs["GC, unlocalised with other M and P, the GC cycle again"] = _seq([(base, {}), (other, {}), (base, dict(keep="values"))])
    # 3. who may reuse the taper table and the lists
    seqs["gc_onepass 1, 0, 1"] = _seq([(S.revalue(base, rng), dict(gc_onepass=g, keep="values")) for g in (1, 0, 1, 0, 1)])
    seqs["obs_batch 64, 7, 64 and each Phase-A kind"] = _seq(
        [(S.revalue(base, rng), dict(obs_batch=b, phase_a=k, keep="values"))
         for b, k in ((64, "band"), (7, "band"), (64, "band"), (64, "gram"), (64, "chain"), (64, "batch"), (32, "band"),
                      (1, "batch"), (64, "band"))])
    # 4. same geometry on more slabs, then fewer
    seqs["n_lead 4, 6, 1"] = _seq([(dict(S.revalue(base, rng, N=600 * n), n_lead=n), dict(keep="n_lead")) for n in (4, 6, 1)])
    # 5. ob_pack, tw_mat, gc_idx / gc_wts re-allocate; then the EARLIER, smaller geometry; then the larger one again
    small = _gc(seed=31, n_lead=2, ncol=80, M=20, P=30)
    large = _gc(seed=32, n_lead=2, ncol=2000, M=20, P=700)
    seqs["small, large, small, large geometry"] = _seq([(small, {}), (large, {}), (S.revalue(small, rng), {}),
                                                        (S.revalue(large, rng), {}), (small, {})])
    # 7. vertical localisation set, re-set to identical values, half-widths only, off; adaptive inflation set, other bounds, off
    vl = S.vertical(rng, base["n_lead"], base["P"])
    vl2 = (vl[0].copy(), vl[1].copy(), vl[2] * 0.6)
    seqs["vertical localisation set, identical, half-widths, off"] = _seq(
        [(S.revalue(base, rng), dict(vl=v, keep="values")) for v in (vl, tuple(a.copy() for a in vl), vl2, None, vl2, None)])
    f = S.inflation_field(rng, base["N"])
    seqs["adaptive inflation set, other bounds, off"] = _seq(
        [(S.revalue(base, rng), dict(ai=a, keep="values", entry=e))
         for a, e in ((dict(field=f, lower=1.0, upper=1e6, sd_lower=0.0), "cycle_in"),
                      (dict(field=f, lower=0.8, upper=1.3, sd_lower=0.2), "update_dev"), (None, "cycle_out"),
                      (dict(field=f, lower=1.0, upper=1e6, sd_lower=0.0), "phases_out"), (None, "state_cycle"))])
    # 8. RTPP in place on the sweeps (keeps a copy of the prior), more rows, RTPS, none
    u = S.new_case(8, 700, 40, 100, False)
    u2 = S.new_case(9, 2100, 40, 100, False)
    seqs["RTPP in place, more rows, RTPS, none"] = _seq(
        [(u, dict(relax=("rtpp", 0.5), entry="update_dev", path=1)), (u2, dict(relax=("rtpp", 0.5), entry="cycle_in", path=1)),
         (u, dict(relax=("rtpp", 0.5), entry="phases_in", path=1)), (u2, dict(relax=("rtps", 0.9), entry="cycle_in", path=1)),
         (u2, dict(relax=None, entry="cycle_in", path=1)), (u, dict(relax=("rtpp", 0.5), entry="cycle_out", path=2)),
         (u, dict(relax=None, entry="cycle_out", path=2))])
    # the outlier check on, another rejected set, off (qc_used, qc_act)
    g1 = S.revalue(base, rng)
    g1["val"], _ = S._outlier.inject(g1["HX"], g1["val"], g1["err"], g1["asm"], 3.0, 5, seed=1)
    g2 = S.revalue(base, rng)
    g2["val"], _ = S._outlier.inject(g2["HX"], g2["val"], g2["err"], g2["asm"], 3.0, 9, seed=2)
    seqs["outlier check on, another rejected set, off, on one geometry"] = _seq(
        [(g1, dict(qc=3.0, keep="values")), (g2, dict(qc=3.0, keep="values", entry="state_cycle")),
         (g2, dict(qc=None, keep="values")), (g1, dict(qc=3.0, keep="values", entry="update_dev")), (g1, dict(keep="values"))])
    seqs.update(_slab_sequences(rng))
    for steps in seqs.values():
        for s in steps:
            assert S.clear(s), S.describe(s)
    return seqs


def _gc_slab(seed=909, nvar=3, nt=2, ncol=600, M=40, P=150):
    c = S.new_case(seed, nvar * nt * ncol, M, P, True, ncol=ncol)
    c["state_shape"] = (nvar, nt, c["ny"], c["nx"])
    return c


def _first_ob(c, sl, test):
    """The first ob of the first third that is assimilated and passes `test`: the obs after it then see what changes with it."""
    return next(k for k in range(c["P"] // 3) if c["asm"][k] and test(k))


def _slab_sequences(rng):
    """One sequence per key the caches of the slab setting, the streamed cycle and the float32 rows are compared by."""
    seqs = {}
    base = _gc_slab()
    nvar, nt = base["state_shape"][:2]
    P, n_lead = base["P"], base["n_lead"]
    sl = S.slab_setting(rng, nvar, nt, P)
    vl = S.vertical(rng, n_lead, P)
    # geo_sl_serial (efa_obs_phase: the obs geometry counts as unchanged only under the same slab setting) and with it the tapered
    # obs-obs table and the active lists: the same case, one ob's tau three times as wide, the first setting again
    k = _first_ob(base, sl, lambda k: not np.isnan(sl["ob_time"][k]) and not np.isnan(sl["ob_time_halfwidth"][k]))
    wide = S.slab_copy(sl)
    wide["ob_time_halfwidth"][k] *= 3.0
    seqs["slab: one ob's tau changed on one geometry (geo_sl_serial)"] = _seq(
        [(base, dict(sl=sl)), (base, dict(sl=wide, keep="sl_tau")), (base, dict(sl=S.slab_copy(sl), keep="sl_tau")),
         (S.revalue(base, rng), dict(sl=wide, keep="sl_tau", entry="state_cycle"))])
    # the same key through the variable part: the impact of the obtype that names no state variable on variable 0
    other = S.slab_copy(sl)
    other["impact"][nvar - 1, 0] = 0.55 if sl["impact"][nvar - 1, 0] != 0.55 else 0.3
    seqs["slab: one impact entry changed on one geometry (geo_sl_serial)"] = _seq(
        [(base, dict(sl=sl)), (base, dict(sl=other, keep="sl_impact")), (base, dict(sl=S.slab_copy(sl), keep="sl_impact")),
         (S.revalue(base, rng), dict(sl=other, keep="sl_impact", entry="update_dev"))])
    # efa_ctx_set_slab_localization returns early on identical arrays: no serial moves, the lists and the table are reused
    seqs["slab: identical setting sent again (sl_serial stays)"] = _seq(
        [(base, dict(sl=sl, vl=vl))] + [(S.revalue(base, rng), dict(sl=S.slab_copy(sl), vl=tuple(a.copy() for a in vl), keep="sl_same",
                                                                    entry=e)) for e in ("cycle_out", "state_cycle", "cycle_in")])
    # sl_tab_vl_serial (ensure_slab_table: the table carries the vertical factor and must follow vl_serial)
    vl2 = (vl[0].copy(), vl[1].copy(), vl[2] * 0.5)
    seqs["slab: vertical half-widths alone changed (sl_tab_vl_serial)"] = _seq(
        [(base, dict(sl=sl, vl=vl)), (base, dict(sl=S.slab_copy(sl), vl=vl2, keep="vl_under_sl")),
         (base, dict(sl=S.slab_copy(sl), vl=tuple(a.copy() for a in vl), keep="vl_under_sl")),
         (S.revalue(base, rng), dict(sl=S.slab_copy(sl), vl=vl2, keep="vl_under_sl", entry="phases_out"))])
    # efa_obs_impact_slab_dev writes the table's cache from outside a cycle, here under other half-widths than the cycles'
    seqs["slab: obs_impact_slab under another vertical setting between two cycles (sl_tab cache)"] = _seq(
        [(base, dict(sl=sl, vl=vl, after=("obs_impact_slab_other_vl",))), (base, dict(sl=S.slab_copy(sl), vl=vl, keep="sl_same")),
         (S.revalue(base, rng), dict(sl=S.slab_copy(sl), vl=vl, keep="sl_same", after=("obs_impact_slab", "slab_factor_table"))),
         (S.revalue(base, rng), dict(sl=S.slab_copy(sl), vl=vl, keep="sl_same", entry="state_cycle"))])
    # cleared, a plain cycle on the same geometry, the identical setting again: both switches move sl_serial
    seqs["slab: on, off with a plain cycle, the identical setting on again (sl_serial moves)"] = _seq(
        [(base, dict(sl=sl)), (base, dict(keep="values")), (base, dict(sl=S.slab_copy(sl), keep="values")),
         (S.revalue(base, rng), dict(keep="values", entry="state_cycle")),
         (S.revalue(base, rng), dict(sl=S.slab_copy(sl), keep="sl_off_on", entry="cycle_in"))])
    # sl_any false between two settings with factors: the plain family serves the step, the table of the first must not
    sl_b = S.slab_setting(rng, nvar, nt, P)
    seqs["slab: a setting of ones between two real settings (sl_any)"] = _seq(
        [(base, dict(sl=sl)), (base, dict(sl=S.slab_ones(nvar, nt, P), keep="sl_ones")), (base, dict(sl=sl_b, keep="values")),
         (S.revalue(base, rng), dict(sl=S.slab_ones(nvar, nt, P), keep="sl_ones", vl=vl)),
         (S.revalue(base, rng), dict(sl=S.slab_copy(sl), keep="values", vl=vl))])
    # qc_used / qc_act feed the list builders: a slab step after a step whose outlier check rejected obs of the same geometry
    g1 = S.revalue(base, rng)
    g1["val"], _ = S._outlier.inject(g1["HX"], g1["val"], g1["err"], g1["asm"], 3.0, 3, seed=3)
    seqs["slab: after an outlier check that rejected three obs of the same geometry (qc_used, qc_act)"] = _seq(
        [(g1, dict(qc=3.0)), (S.revalue(base, rng), dict(sl=sl, keep="values")), (g1, dict(qc=3.0, sl=S.slab_copy(sl), keep="sl_same")),
         (S.revalue(base, rng), dict(sl=S.slab_copy(sl), keep="sl_same", entry="state_cycle"))])
    # ColumnGrid::take_slice: the streamed cycle cuts the grid mirror into chunks (mirror_ncol = -1, grid.serial moves); the
    # resident cycle on the same grid arrays must upload the whole grid again
    seqs["streamed in chunks of 16, resident on the same grid, streamed in chunks of 48 (take_slice, grid.serial)"] = _seq(
        [(base, dict(entry="host_streamed", chunk_cols=16)), (S.revalue(base, rng), dict(entry="cycle_in", keep="values")),
         (S.revalue(base, rng), dict(entry="host_streamed", chunk_cols=48, keep="values", sl=sl)),
         (S.revalue(base, rng), dict(entry="state_cycle", keep="values", sl=S.slab_copy(sl)))])
    # f32_ws, wide_prior, relax_prior, relax_ss only grow: rows of 4 and 8 bytes, above and below 136 members, standalone relaxation
    u = dict((M, S.new_case(1000 + M, 700, M, 100, False)) for M in (100, 137, 256))
    seqs["float32 and float64 rows in turn, above and below 136 members (f32_ws, wide_prior, relax_prior, relax_ss)"] = _seq(
        [(S.to_f32(u[137]), dict(entry="state_cycle_f32", elem="f32", in_place=True, path=2)), (u[137], dict(entry="cycle_in", path=2)),
         (S.to_f32(u[100]), dict(entry="state_cycle_f32", elem="f32", relax=("rtpp", 0.5), path=1)),
         (u[256], dict(entry="cycle_in", relax=("rtps", 0.9), path=2)),
         (S.to_f32(u[137]), dict(entry="state_cycle_f32", elem="f32", relax=("rtps", 0.9), path=2))])
    # the per-batch rows table against the whole obs-obs table (tw_serial, tw_Pw, tw_Rw, tw_ptr)
    seqs["slab: Phase A per batch, then the band leader, on one geometry (tw table)"] = _seq(
        [(S.revalue(base, rng), dict(sl=S.slab_copy(sl), vl=vl, keep="sl_same", phase_a=k, obs_batch=b))
         for k, b in (("batch", 64), ("band", 64), ("batch", 7), ("gram", 64))])
    # sl_tab is grow-only: one more ob may or may not move its pointer (sl_tab_ptr); then the first setting again
    more = _gc_slab(seed=910, P=P + 1)
    seqs["slab: P obs, P + 1 obs with their own setting, P obs again (sl_tab_ptr)"] = _seq(
        [(base, dict(sl=sl)), (more, dict(sl=S.slab_setting(rng, nvar, nt, P + 1))), (base, dict(sl=S.slab_copy(sl))),
         (S.revalue(more, rng), dict(sl=S.slab_setting(rng, nvar, nt, P + 1), keep="values"))])
    return seqs


def _taper_changed(results):
    """Steps 0..2 run one case under setting A, B, A: the obs block under B differs from A's, and A's comes back bit for bit."""
    assert not np.array_equal(results[1]["Yp"], results[0]["Yp"]), "the changed setting left the obs block as it was"
    if results[2]["kind"] == results[0]["kind"]:
        for key in ("post", "ym", "Yp"):
            assert np.array_equal(results[2][key], results[0][key]), "the first setting again: %s differs from the first step's" % key


def _state_taper_changed(results):
    """The same where only the state rows' factors change (the obs-obs table has its own key)."""
    assert not np.array_equal(results[1]["post"], results[0]["post"]), "the changed half-widths left the posterior as it was"
    if results[2]["kind"] == results[0]["kind"]:
        assert np.array_equal(results[2]["post"], results[0]["post"]), "the first half-widths again: another posterior"


def _lists_reused(results):
    """What the options show of work that hangs on geo_serial: the same active pairs and as many state launches in every step."""
    assert len(set(r["pairs"] for r in results)) == 1 and len(set(r["launches"] for r in results)) == 1, \
        [(r["pairs"], r["launches"]) for r in results]


DIRECTED_CHECKS = {"slab: one ob's tau changed on one geometry (geo_sl_serial)": _taper_changed,
                   "slab: one impact entry changed on one geometry (geo_sl_serial)": _taper_changed,
                   "slab: vertical half-widths alone changed (sl_tab_vl_serial)": _state_taper_changed,
                   "slab: identical setting sent again (sl_serial stays)": _lists_reused}


DIRECTED = ["grid values changed, cycle_out", "grid values changed, state_cycle",
            "GC, unlocalised with other M and P, the GC cycle again", "gc_onepass 1, 0, 1",
            "obs_batch 64, 7, 64 and each Phase-A kind", "n_lead 4, 6, 1", "small, large, small, large geometry",
            "vertical localisation set, identical, half-widths, off", "adaptive inflation set, other bounds, off",
            "RTPP in place, more rows, RTPS, none", "outlier check on, another rejected set, off, on one geometry",
            "slab: one ob's tau changed on one geometry (geo_sl_serial)",
            "slab: one impact entry changed on one geometry (geo_sl_serial)",
            "slab: identical setting sent again (sl_serial stays)",
            "slab: vertical half-widths alone changed (sl_tab_vl_serial)",
            "slab: obs_impact_slab under another vertical setting between two cycles (sl_tab cache)",
            "slab: on, off with a plain cycle, the identical setting on again (sl_serial moves)",
            "slab: a setting of ones between two real settings (sl_any)",
            "slab: after an outlier check that rejected three obs of the same geometry (qc_used, qc_act)",
            "streamed in chunks of 16, resident on the same grid, streamed in chunks of 48 (take_slice, grid.serial)",
            "float32 and float64 rows in turn, above and below 136 members (f32_ws, wide_prior, relax_prior, relax_ss)",
            "slab: Phase A per batch, then the band leader, on one geometry (tw table)",
            "slab: P obs, P + 1 obs with their own setting, P obs again (sl_tab_ptr)"]


def few_kind_differences(stats):
    """The plans' rule for a sequence of a few steps: a step whose persistent launch gave up on a busy device (spin fall-back) ran
    another Phase-A kind than the fresh context and was compared through assert_parity; 2 % of fewer than fifty steps is none,
    so one such step is let through, and a second one in so short a sequence is not a coincidence."""
    return stats["kind_differs"] <= max(1, int(KIND_DIFF_MAX * stats["steps"]))


@pytest.mark.parametrize("name", DIRECTED)
def test_directed_transition(name):
    seqs = directed_sequences()
    assert sorted(seqs) == sorted(DIRECTED)
    results = []
    stats = run_steps(seqs[name], results=results)
    assert stats["steps"] == len(seqs[name]) and few_kind_differences(stats)
    if name in DIRECTED_CHECKS:
        DIRECTED_CHECKS[name](results)


def _numpy_stencil(X, idx, wts):
    return (wts[:, :, None] * X[idx]).sum(axis=1)


def helper_calls(ctx, base, rng):
    """Every helper entry point once on the grid of the GC case `base`, each checked: efa_gc_block_counts of another ob set,
    efa_forward_stencil_dev (the same stencil twice, the same indices with other weights, a longer one, the first again),
    efa_interp_stencils + efa_forward_interp_dev."""
    ny, nx, N, M = base["ny"], base["nx"], base["N"], base["M"]
    X = dev(base["X"])
    # block counts of ANOTHER ob set on the same grid
    o = _gc(seed=42, n_lead=2, ncol=ny * nx, M=20, P=77)
    cnt, bp, pairs = ctx.gc_block_counts(base["lat"], base["lon"], o["ob_lat"], o["ob_lon"], o["hw"], o["asm"])
    assert pairs == int(bp.sum()) and cnt.shape == ((ny * nx + 15) // 16,)
    # forward stencils
    P1 = 50
    idx = rng.integers(0, N, (P1, 3))
    w1, w2 = rng.random((P1, 3)), rng.random((P1, 3))
    idx_long = rng.integers(0, N, (400, 5))
    w_long = rng.random((400, 5))
    HX = dev(np.zeros((400, M)))
    for ix, w in ((idx, w1), (idx, w1), (idx, w2), (idx_long, w_long), (idx, w1)):
        HX.zero_()
        _torch().cuda.synchronize()
        ctx.forward_stencil(N, 0, M, X.data_ptr(), ix, w, HX.data_ptr())
        assert_parity(host(ctx, HX, len(ix)), _numpy_stencil(base["X"], ix, w), "forward stencil")
    # interpolation stencils of point obs, and their estimates
    nvar, nt = 2, 1
    Pq = 40
    qlat = rng.uniform(base["lat"].min() + 1, base["lat"].max() - 1, Pq)
    qlon = rng.uniform(base["lon"].min() + 1, base["lon"].max() - 1, Pq)
    sidx, swts, st = ctx.interp_stencils(nvar, nt, ny, nx, base["lat"], base["lon"], [0.0], rng.integers(0, nvar, Pq),
                                         np.zeros(Pq), qlat, qlon)
    assert not st.any()
    ctx.forward_interp(ny * nx, 0, ny * nx, nvar * nt, M, X.data_ptr(), HX.data_ptr())
    ref = (np.where(sidx >= 0, swts, 0.0)[:, :, None] * base["X"][np.maximum(sidx, 0)]).sum(axis=1)
    assert_parity(host(ctx, HX, Pq), ref, "forward interp")


def test_helper_calls_between_two_cycles_on_one_geometry():
    """efa_gc_block_counts, efa_interp_stencils + efa_forward_interp_dev and efa_forward_stencil_dev (the same stencil twice, the
    same indices with other weights, a longer one, the first again) between cycles: they share the context's workspaces and the
    stencil image, and must neither disturb the cycles' caches nor serve a stale stencil."""
    lib = _lib()
    rng = np.random.default_rng(4)
    base = _gc(seed=41, n_lead=2, ncol=25 * 32, M=20, P=120)
    ctx = lib.Context(0)
    try:
        used = Runner(ctx)
        first = S.make_step(base, seed="helpers")
        got0 = used.run(first)
        check_against_model(first, got0, S.model(first), "before the helper calls")
        pairs0 = ctx.get_option("gc_active_pairs")
        helper_calls(ctx, base, rng)
        # the cycle's geometry again: the same bits as a fresh context, the same pairs
        second = S.make_step(S.revalue(base, rng), keep="values", seed="helpers", index=1)
        got = used.run(second)
        check_against_model(second, got, S.model(second), "after the helper calls")
        assert ctx.get_option("gc_active_pairs") == pairs0
        fctx = lib.Context(0)
        try:
            assert check_against_fresh(got, Runner(fctx).run(second), "after the helper calls") == 0
        finally:
            fctx.close()
    finally:
        ctx.close()


def test_deferred_timing_sums_over_the_directed_sequences():
    """timing 2 across ALL the directed sequences, one of the calls of S.BYSTANDERS after every step (the impact, diagnostic and
    helper entry points: none of them may add to either sum), the helper calls after each sequence, with efa_last_timing read only
    at the end:
    state_launches equals the sum of the per-step values read with timing 1 on a second pass (the times themselves are not
    asserted).  The per-batch sweeps (obs_batch 7 and 1, gc_onepass 0) are where the count of launches varies most."""
    lib = _lib()
    seqs = directed_sequences()
    helper_base = _gc(seed=41, n_lead=2, ncol=25 * 32, M=20, P=120)
    ctx = lib.Context(0)
    try:
        r = Runner(ctx, read_timing=False)

        def one_pass(timing):
            kinds, launches = [], 0
            for name in DIRECTED:
                for s in seqs[name]:
                    got = r.run(dict(s, timing=timing))
                    kinds.append(got["kind"])
                    launches += got["launches"] or 0
                    b = S.BYSTANDERS[len(kinds) % len(S.BYSTANDERS)]     # one call between this step and the next, in turn
                    if S.bystander_legal(s, b):
                        r.bystander(b, s, got)
                helper_calls(ctx, helper_base, np.random.default_rng(4))
            return kinds, launches

        kinds2, _ = one_pass(2)
        total = ctx.last_timing()
        r.read_timing = True
        kinds1, per_step = one_pass(1)
        steps = kinds1
        assert kinds1 == kinds2, "the two passes ran other Phase-A kinds (a spin fall-back): their launches cannot be compared"
        assert total["state_launches"] == per_step and per_step > len(steps) // 2
        assert total["state_ms"] > 0 and total["obs_ms"] > 0
    finally:
        ctx.close()


def test_raw_cycles_interleaved_with_the_python_surface_on_the_shared_context():
    """On get_context(0): raw GC cycle, EnSRF(..., rtps=, vert_coord=, outlier_threshold=).update(), raw unlocalised cycle with
    relaxation and the outlier check, EnSRF(..., adaptive_inflation=).update() (the two keywords exclude each other in one
    call), raw GC cycle, plain EnSRF.update().  The Python surface sets what it needs on every call, so the plain results equal
    a fresh context's bit for bit: nothing the raw cycles set is taken over.  The adaptive update() hands the shared context a
    raw device pointer to its field and must take it back: the raw cycle after it re-sends every setting but that one, so a
    field left behind (other rows than this cycle's) would make the library refuse it."""
    from conftest import load_golden
    from efa_xray_amd import AdaptiveInflation, EnSRF
    from test_gpu_parity import _make_api_objects
    lib = _lib()
    g = load_golden("G6")
    nvar, nt = int(g["shape"][0]), int(g["shape"][1])
    P = len(g["ob_value"])
    rng = np.random.default_rng(6)
    raw = S.make_step(_gc(seed=61, n_lead=2, ncol=300, M=20, P=90), seed="shared")
    raw_u = S.make_step(S.new_case(62, 500, 50, 70, False), seed="shared", relax=("rtps", 0.4), qc=3.0)
    assert S.clear(raw_u)

    def plain():
        state, obs = _make_api_objects(g)
        post, obs_out = EnSRF(state, obs, verbose=False, loc="GC").update()
        return post.to_vect().copy(), np.array([o.prior_var for o in obs_out]), np.array([bool(o.assimilated) for o in obs_out])

    shared = lib.get_context(0)
    used = Runner(shared)
    try:
        check_against_model(raw, used.run(raw), S.model(raw), "raw GC cycle")
        used.reset()
        state, obs = _make_api_objects(g)
        lead, ov, oh = S.vertical(rng, nvar * nt, P)
        for k, ob in enumerate(obs):
            ob.vert = None if np.isnan(ov[k]) else float(ov[k])
            ob.vert_localize_radius = float(oh[k])
        EnSRF(state, obs, verbose=False, loc="GC", rtps=0.7, vert_coord=lead.reshape(nvar, nt), outlier_threshold=3.0).update()
        used.forget()
        check_against_model(raw_u, used.run(raw_u), S.model(raw_u), "raw unlocalised cycle")
        used.reset()
        state, obs = _make_api_objects(g)
        ai = AdaptiveInflation(state, ("adaptive", "/nonexistent/prior_inflation.nc", (1.0, 0.6)))
        field = S.inflation_field(rng, state.nstate())
        ai.inflation.from_vect(field)
        EnSRF(state, obs, verbose=False, loc="GC", adaptive_inflation=ai).update()
        assert np.abs(ai.inflation.to_vect() - field).max() > 1e-6, "the field did not move"
        used.forget()
        used.have["ai"] = None           # not sent again: update() itself must have taken its field back
        raw2 = S.make_step(S.revalue(raw["case"], rng), keep="values", seed="shared", index=2, entry="state_cycle")
        check_against_model(raw2, used.run(raw2), S.model(raw2), "raw GC cycle after the adaptive update()")
        got = plain()
        used.forget()
        keep = lib._contexts[0]
        lib._contexts[0] = lib.Context(0)
        try:
            want = plain()
        finally:
            lib._contexts[0].close()
            lib._contexts[0] = keep
        for a, b, what in zip(got, want, ("posterior", "prior_var", "assimilated")):
            assert np.array_equal(a, b), "plain update() after the feature calls: %s differs from a fresh context's" % what
        assert_parity(got[0], g["post"], "plain update() vs the stored reference")
    finally:
        used.reset()
        shared.set_vertical_localization(None)
        shared.set_adaptive_inflation(None)
        shared.set_relaxation(lib.RELAX_NONE, 0.0)
        shared.set_outlier_threshold(None)
        shared.use_own_stream()


# ---- d. refusals in the middle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.REFUSALS + S.REFUSALS2)
def test_refusal_then_the_next_valid_step(kind):
    rng = np.random.default_rng(12)
    base = _gc(seed=71, n_lead=2, ncol=200, M=20, P=60)
    vl = S.vertical(rng, base["n_lead"], base["P"])
    refusal = (lambda i: S._refusal_step(rng, kind, None, "refusal", i)) if kind in S.REFUSALS else \
        (lambda i: S._refusal_step2(rng, kind, "refusal", i))
    steps = [S.make_step(base, seed="refusal", index=0, vl=vl, qc=3.0),
             refusal(1),
             S.make_step(S.revalue(base, rng), seed="refusal", index=2, keep="values", vl=vl, entry="state_cycle"),
             refusal(3),
             S.make_step(S.new_case(72, 400, 40, 50, False), seed="refusal", index=4),
             S.make_step(S.revalue(base, rng), seed="refusal", index=5, keep="values", entry="cycle_in")]
    assert all(S.clear(s) for s in steps if not s["refusal"])
    stats = run_steps(steps)
    assert stats["steps"] == 4 and stats["refusals"] == 2 and few_kind_differences(stats)


# ---- c. streams ----------------------------------------------------------------------------------------------------------------
BIG_ROWS = 10_000_000          # x 100 members: the transform of such a state runs for milliseconds
BIG_M, BIG_P = 100, 64


def _sample_rows(rng, N, n=3000):
    """Seeded rows over the whole state, and its first and last thousand (the transform's first and last workgroups)."""
    return np.unique(np.concatenate([rng.choice(N, n, replace=False), np.arange(1000), np.arange(N - 1000, N)]))


class BigCycle(object):
    """An unlocalised cycle on a resident synthetic state, disjoint buffers, transform path: efa_ensrf_cycle_dev returns with
    the transform still in the stream.  The model is the oracle on a sample of the rows (rows are independent given the obs)."""

    def __init__(self, ctx, rows=BIG_ROWS, seed=1):
        torch = _torch()
        self.rows, self.rng = rows, np.random.default_rng(seed)
        self.X = torch.empty((rows, BIG_M), dtype=torch.float64, device="cuda:0")
        self.post = torch.zeros((rows, BIG_M), dtype=torch.float64, device="cuda:0")
        ctx.fill_synthetic(rows, 0, BIG_M, seed, 1.0, self.X.data_ptr())
        ctx.synchronize()
        self.pick = self.rng.choice(rows, BIG_P, replace=False)
        self.sample = _sample_rows(self.rng, rows)
        self.Xs = self.X[torch.from_numpy(self.sample).to("cuda:0")].cpu().numpy()
        self.HX = self.X[torch.from_numpy(self.pick).to("cuda:0")].cpu().numpy()
        self.val = self.HX.mean(axis=1) + self.rng.standard_normal(BIG_P)
        self.err = self.rng.uniform(0.5, 2.0, BIG_P)
        self.asm = np.ones(BIG_P, dtype=bool)
        self.Yp, self.ym = dev(self.HX), dev(np.zeros(BIG_P))
        ctx.form_perts(BIG_P, BIG_M, self.Yp.data_ptr(), self.ym.data_ptr(), self.Yp.data_ptr())
        ctx.synchronize()
        torch.cuda.synchronize()

    def issue(self, ctx):
        """No synchronisation after it."""
        return ctx.ensrf_cycle(self.rows, BIG_M, BIG_P, self.X.data_ptr(), self.post.data_ptr(), self.ym.data_ptr(),
                               self.Yp.data_ptr(), self.val, self.err, self.asm)

    def check(self, what, post=None):
        """After the caller has synchronised."""
        torch = _torch()
        post = self.post if post is None else post
        got = post[torch.from_numpy(self.sample).to("cuda:0")].cpu().numpy()
        ref = orc.ensrf_cycle(self.Xs, self.HX, self.val, self.err, self.asm)[0]
        return assert_parity(got, ref, what)


def _set_stream(ctx, which, streams):
    if which == "own":
        ctx.use_own_stream()
    else:
        ctx.set_stream(0 if which == "null" else streams[which].cuda_stream)


@pytest.mark.parametrize("first,second", [("A", "B"), ("own", "A"), ("A", "own"), ("own", "null")])
def test_change_of_stream_with_a_cycle_in_flight(first, second):
    """Cycle 1 on one stream with its transform still running, then at once another stream and cycle 2 with other obs, another M
    and a tiny state: cycle 2's obs phase rewrites the context's workspaces cycle 1's transform reads ([T | w] behind the obs
    rows).  Work issued after a change of stream must be ordered behind everything the context issued before it."""
    torch, lib = _torch(), _lib()
    ctx = lib.Context(0)
    streams = dict(A=torch.cuda.Stream(), B=torch.cuda.Stream())
    try:
        ctx.set_option("path", lib.PATH_TRANSFORM)
        big = BigCycle(ctx)
        small = S.make_step(S.new_case(77, 500, 40, 200, False), seed="stream", path=2)
        c = small["case"]
        X2, post2 = dev(c["X"]), dev(np.zeros((c["N"], c["M"])))
        Yp2, ym2 = dev(c["HX"]), dev(np.zeros(c["P"]))
        ctx.form_perts(c["P"], c["M"], Yp2.data_ptr(), ym2.data_ptr(), Yp2.data_ptr())
        # cycle 2 once beforehand: its workspaces then exist at their size, and nothing is re-allocated while cycle 1 is in
        # flight (a hipFree waits for the whole device and would order the two cycles by accident)
        ctx.ensrf_cycle(c["N"], c["M"], c["P"], X2.data_ptr(), post2.data_ptr(), ym2.data_ptr(), Yp2.data_ptr(), c["val"],
                        c["err"], c["asm"])
        ctx.synchronize()
        post2.zero_()
        torch.cuda.synchronize()
        _set_stream(ctx, first, streams)
        big.issue(ctx)
        _set_stream(ctx, second, streams)
        d2 = ctx.ensrf_cycle(c["N"], c["M"], c["P"], X2.data_ptr(), post2.data_ptr(), ym2.data_ptr(), Yp2.data_ptr(), c["val"],
                             c["err"], c["asm"])
        ctx.synchronize()
        torch.cuda.synchronize()
        e1 = big.check("cycle 1 (%s), its stream changed to %s while its transform ran" % (first, second))
        m = S.model(small)
        e2 = assert_parity(post2.cpu().numpy(), m["post"], "cycle 2 on stream %s" % second)
        assert_parity(d2["post_var"], m["diag"]["post_var"], "cycle 2 post_var")
        print("stream %s -> %s: relative errors %.3e (cycle 1, sampled rows), %.3e (cycle 2)" % (first, second, e1, e2))
    finally:
        ctx.use_own_stream()
        ctx.synchronize()
        torch.cuda.synchronize()
        ctx.close()


def _big_gc():
    """A one-pass sweep of about a millisecond: 1.6 million rows, 1000 obs."""
    return S.new_case(81, 16 * 102400, 40, 1000, True, ncol=102400)


def test_change_of_stream_with_a_localised_cycle_in_flight():
    """The same with a GC cycle first: its one-pass sweep reads the recorded obs rows, the coefficients, the active lists and the
    grid from the context's workspaces for as long as it runs, and cycle 2 (other obs, another M, another grid) rewrites them
    all.  Cycle 1 is checked on a sample of its rows (tests/_vertloc.py, rows=).  Of the stream tests, this one and the next are the two that fail when a change of
    stream is not ordered behind the work issued before it; the unlocalised pairs above pass either way."""
    import _vertloc
    torch, lib = _torch(), _lib()
    c1 = _big_gc()
    small = S.make_step(S.new_case(82, 3 * 700, 64, 200, True, ncol=700), seed="stream")
    c2 = small["case"]
    ctx = lib.Context(0)
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        bufs = []
        for c in (c1, c2):
            Yp, ym = dev(c["HX"]), dev(np.zeros(c["P"]))
            ctx.form_perts(c["P"], c["M"], Yp.data_ptr(), ym.data_ptr(), Yp.data_ptr())
            bufs.append((dev(c["X"]), dev(np.zeros((c["N"], c["M"]))), Yp, ym))
        X, post, Yp, ym = bufs[1]     # cycle 2 once beforehand: nothing is re-allocated while cycle 1 is in flight (see above)
        ctx.ensrf_cycle(c2["N"], c2["M"], c2["P"], X.data_ptr(), post.data_ptr(), ym.data_ptr(), Yp.data_ptr(), c2["val"],
                        c2["err"], c2["asm"], **dict(Runner.ob_kw(c2), **Runner.grid_kw(c2)))
        ctx.synchronize()
        post.zero_()
        torch.cuda.synchronize()
        ctx.set_stream(A.cuda_stream)
        for k, c in enumerate((c1, c2)):
            X, post, Yp, ym = bufs[k]
            ctx.ensrf_cycle(c["N"], c["M"], c["P"], X.data_ptr(), post.data_ptr(), ym.data_ptr(), Yp.data_ptr(), c["val"], c["err"],
                            c["asm"], **dict(Runner.ob_kw(c), **Runner.grid_kw(c)))
            if k == 0:
                ctx.set_stream(B.cuda_stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        sample = _sample_rows(np.random.default_rng(5), c1["N"])
        xbm, Xbp = orc.format_prior_state(c1["X"][sample], c1["HX"])
        xam, Xap, _ = _vertloc.ensrf_update_vert(xbm, Xbp, len(sample), c1["val"], c1["err"], c1["asm"], c1["ob_lat"], c1["ob_lon"],
                                                 c1["hw"], c1["lat"], c1["lon"], (c1["n_lead"], 1, c1["ny"], c1["nx"]), rows=sample,
                                                 obs_taper="vector")
        got = bufs[0][1][torch.from_numpy(sample).to("cuda:0")].cpu().numpy()
        e1 = assert_parity(got, orc.format_posterior_state(xam, Xap, len(sample)), "GC cycle 1, its stream changed while its sweep ran")
        e2 = assert_parity(bufs[1][1].cpu().numpy(), S.model(small)["post"], "GC cycle 2 on the new stream")
        print("GC stream A -> B: relative errors %.3e (cycle 1, sampled rows), %.3e (cycle 2)" % (e1, e2))
    finally:
        ctx.use_own_stream()
        ctx.synchronize()
        torch.cuda.synchronize()
        ctx.close()


def test_change_of_stream_then_only_gc_active_pairs():
    """A GC cycle on stream A, then stream B and nothing but option gc_active_pairs: the counter is copied on the new stream while
    the sweep that writes it runs on the old one."""
    torch, lib = _torch(), _lib()
    c = _big_gc()
    kw = dict(Runner.ob_kw(c), **Runner.grid_kw(c))
    want = None
    for changed in (False, True):
        ctx = lib.Context(0)
        A, B = torch.cuda.Stream(), torch.cuda.Stream()
        try:
            X, post = dev(c["X"]), dev(np.zeros((c["N"], c["M"])))
            Yp, ym = dev(c["HX"]), dev(np.zeros(c["P"]))
            ctx.set_stream(A.cuda_stream)
            ctx.form_perts(c["P"], c["M"], Yp.data_ptr(), ym.data_ptr(), Yp.data_ptr())
            ctx.ensrf_cycle(c["N"], c["M"], c["P"], X.data_ptr(), post.data_ptr(), ym.data_ptr(), Yp.data_ptr(), c["val"], c["err"],
                            c["asm"], **kw)
            if changed:
                ctx.set_stream(B.cuda_stream)
            else:
                ctx.synchronize()
            pairs = ctx.get_option("gc_active_pairs")
            torch.cuda.synchronize()
            if not changed:
                want = pairs
                _, bp, total = ctx.gc_block_counts(c["lat"], c["lon"], c["ob_lat"], c["ob_lon"], c["hw"], c["asm"])
                assert want == total > 0
            else:
                assert pairs == want, "gc_active_pairs read on a new stream while the sweep ran on the old one: %d, not %d" % (
                    pairs, want)
        finally:
            ctx.use_own_stream()
            ctx.synchronize()
            torch.cuda.synchronize()
            ctx.close()


def test_inputs_written_on_a_caller_stream_are_seen_in_order():
    """On stream s without any host synchronisation: X filled with NaN, a large transform cycle on unrelated buffers as the delay,
    X copied in from pinned memory, forward_stencil -> form_perts -> ensrf_cycle.  A read issued on any other stream sees NaN."""
    torch, lib = _torch(), _lib()
    ctx = lib.Context(0)
    s = torch.cuda.Stream()
    try:
        ctx.set_option("path", lib.PATH_TRANSFORM)
        big = BigCycle(ctx)
        step = S.make_step(S.new_case(91, 4000, 40, 120, False), seed="stream")
        c = step["case"]
        N, M, P = c["N"], c["M"], c["P"]
        pinned = torch.from_numpy(c["X"]).pin_memory()
        X = torch.empty((N, M), dtype=torch.float64, device="cuda:0")
        post = torch.zeros((N, M), dtype=torch.float64, device="cuda:0")
        Yp, ym = torch.zeros((P, M), dtype=torch.float64, device="cuda:0"), torch.zeros(P, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            X.fill_(float("nan"))
            big.issue(ctx)                                   # the delay: milliseconds of transform in front of the copy
            X.copy_(pinned, non_blocking=True)
            ctx.forward_stencil(N, 0, M, X.data_ptr(), c["rows"][:, None], np.ones((P, 1)), Yp.data_ptr())
            ctx.form_perts(P, M, Yp.data_ptr(), ym.data_ptr(), Yp.data_ptr())
            d = ctx.ensrf_cycle(N, M, P, X.data_ptr(), post.data_ptr(), ym.data_ptr(), Yp.data_ptr(), c["val"], c["err"], c["asm"])
        s.synchronize()
        m = S.model(step)
        assert_parity(post.cpu().numpy(), m["post"], "cycle behind an asynchronous copy on the caller's stream")
        assert_parity(d["prior_mean"], m["diag"]["prior_mean"], "prior_mean")
        big.check("the delay cycle")
    finally:
        ctx.use_own_stream()
        ctx.synchronize()
        torch.cuda.synchronize()
        ctx.close()


@pytest.mark.parametrize("entry", ["cycle_out", "state_cycle", "phases_out"])
def test_outputs_are_ordered_on_the_caller_stream(entry):
    """Directly after the call returns on s (no efa_ctx_synchronize): a clone on s, and one on a second stream that waits for an
    event recorded on s; both are the posterior."""
    torch, lib = _torch(), _lib()
    ctx = lib.Context(0)
    s, t = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        ctx.set_option("path", lib.PATH_TRANSFORM)
        big = BigCycle(ctx, rows=4_000_000)
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            if entry == "cycle_out":
                big.issue(ctx)
                out = big.post
            else:
                ctx.obs_phase(BIG_M, BIG_P, big.ym.data_ptr(), big.Yp.data_ptr(), big.val, big.err, big.asm)
                if entry == "state_cycle":
                    ctx.state_cycle(big.rows, BIG_M, big.X.data_ptr(), big.post.data_ptr())
                    out = big.post
                else:
                    xm = torch.empty(big.rows, dtype=torch.float64, device="cuda:0")
                    xo = torch.empty(big.rows, dtype=torch.float64, device="cuda:0")
                    Xo = torch.empty((big.rows, BIG_M), dtype=torch.float64, device="cuda:0")
                    # (members -> perturbations in big.post, the state phase out of place into Xo, members again in Xo)
                    ctx.form_perts(big.rows, BIG_M, big.X.data_ptr(), xm.data_ptr(), big.post.data_ptr())
                    ctx.state_phase(big.rows, BIG_M, xm.data_ptr(), big.post.data_ptr(), xo.data_ptr(), Xo.data_ptr())
                    ctx.posterior(big.rows, BIG_M, xo.data_ptr(), Xo.data_ptr(), Xo.data_ptr())
                    out = Xo
            on_s = out.clone()
            ev = torch.cuda.Event()
            ev.record(s)
        with torch.cuda.stream(t):
            t.wait_event(ev)
            on_t = out.clone()
        s.synchronize()
        t.synchronize()
        big.check("%s: clone on the caller's stream" % entry, on_s)
        big.check("%s: clone on a stream that waited for an event on the caller's" % entry, on_t)
    finally:
        ctx.use_own_stream()
        ctx.synchronize()
        torch.cuda.synchronize()
        ctx.close()


def test_two_contexts_on_two_streams_alternately():
    """Two contexts, two caller streams, one device; cycles issued alternately without synchronising in between: each equals its
    own fresh-context result bit for bit."""
    torch, lib = _torch(), _lib()
    rng = np.random.default_rng(3)
    geo = [_gc(seed=101, n_lead=3, ncol=500, M=40, P=130), S.new_case(102, 60000, 64, 100, False)]
    rounds = [[S.revalue(g, rng) for g in geo] for _ in range(4)]
    ctxs = [lib.Context(0), lib.Context(0)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        bufs = []
        for r in rounds:
            for c in r:
                Yp, ym = dev(c["HX"]), dev(np.zeros(c["P"]))
                bufs.append((dev(c["X"]), dev(np.zeros((c["N"], c["M"]))), Yp, ym))
        for k in (0, 1):
            ctxs[k].set_stream(streams[k].cuda_stream)
        for i, r in enumerate(rounds):
            for k, c in enumerate(r):
                X, post, Yp, ym = bufs[2 * i + k]
                ctxs[k].form_perts(c["P"], c["M"], Yp.data_ptr(), ym.data_ptr(), Yp.data_ptr())
                ctxs[k].ensrf_cycle(c["N"], c["M"], c["P"], X.data_ptr(), post.data_ptr(), ym.data_ptr(), Yp.data_ptr(), c["val"],
                                    c["err"], c["asm"], **dict(Runner.ob_kw(c), **Runner.grid_kw(c)))
        for k in (0, 1):
            ctxs[k].synchronize()
        torch.cuda.synchronize()
        for i, r in enumerate(rounds):
            for k, c in enumerate(r):
                step = S.make_step(c, seed="two contexts", index=2 * i + k)
                got = bufs[2 * i + k][1].cpu().numpy()
                assert_parity(got, S.model(step)["post"], "context %d round %d" % (k, i))
                f = lib.Context(0)
                try:
                    fresh = Runner(f).run(step)
                finally:
                    f.close()
                assert np.array_equal(got, fresh["post"]), "context %d round %d differs from a fresh context's" % (k, i)
    finally:
        for k in (0, 1):
            ctxs[k].use_own_stream()
            ctxs[k].synchronize()
        torch.cuda.synchronize()
        for k in (0, 1):
            ctxs[k].close()
