"""What the GPU tests of the LETKF family (test_gpu_letkf.py, test_gpu_letkf_interp.py, test_gpu_letkf_slab.py) share: the bounds,
the shared context's reset, the prior obs block on the device, and the comparisons."""
import numpy as np

TOL = 1e-10
SWEEP_CAP = 30
COND_CAP = 1e4


def _reset(ctx):
    from efa_xray_amd import _lib
    ctx.set_outlier_threshold(None)
    ctx.set_vertical_localization(None)
    ctx.set_slab_localization(None)
    ctx.set_sampling_error_correction(None)
    ctx.set_adaptive_inflation(None)
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    for key, v in (("path", 0), ("gram", 2), ("pipeline", 1), ("gc_onepass", 1), ("obs_solver", 0)):
        ctx.set_option(key, v)
    return ctx


def _obs_block(ctx, HX, M):
    P = HX.shape[0]
    if P == 0:
        return ctx.empty((1,)), ctx.empty((1, M)), np.zeros(0), np.zeros((0, M))
    Yp = ctx.to_device(np.ascontiguousarray(HX))
    ym = ctx.empty((P,))
    ctx.form_perts(P, M, Yp, ym, Yp)
    return ym, Yp, ym.download(), Yp.download()


def _close(got, want, what, tol=TOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.max(np.abs(want)) if want.size else 0.0
    err = np.max(np.abs(got - want)) if want.size else 0.0
    print("%s: max abs err %.3e, scale %.3e" % (what, err, scale))
    assert np.all(np.isfinite(got)), what + ": not finite"
    assert err <= tol * max(scale, np.finfo(float).tiny), "%s: %.3e > %g * %.3e" % (what, err, tol, scale)


def _check_diag(diag, ref, what):
    a = np.asarray(ref["assimilated"], bool)
    assert np.array_equal(np.asarray(diag["assimilated"], bool), a), what + ": assimilated"
    _close(diag["prior_mean"], ref["prior_mean"], what + " prior_mean")
    _close(diag["prior_var"], ref["prior_var"], what + " prior_var")
    if a.any():
        _close(np.asarray(diag["post_mean"])[a], ref["post_mean"][a], what + " post_mean")
        _close(np.asarray(diag["post_var"])[a], ref["post_var"][a], what + " post_var")
    assert np.all(np.isnan(np.asarray(diag["post_mean"])[~a])), what + ": post_mean written for an ob that is not assimilated"


def _same_bits(a, b, what, keys=("post", "ym", "Yp", "stats")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s differs" % (what, k)
    for k in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
        assert np.array_equal(np.asarray(a["diag"][k]), np.asarray(b["diag"][k]), equal_nan=True), "%s: %s differs" % (what, k)
