"""Observation impact (EFSO; Kalnay et al. 2012, Ota et al. 2013): which observations helped.

Once a verifying state exists, `observation_impact` estimates for every assimilated ob how much it changed a forecast error norm

    J_k = (1/(M-1)) (d_k / r_k) sum_i rho_ik c_i (e^a_i + e^b_i) (Xf'_i . Ya'_k)

with e^b / e^a the errors of the prior / posterior ensemble mean against the verification, c the norm's weights, Xf' the posterior
perturbations, Ya' the posterior perturbations in observation space, d_k the innovation against the prior mean, r_k the ob's error
variance and rho the taper the update used: Gaspari-Cohn in the horizontal, times the vertical factor (`vert_coord`), times the
temporal and cross-variable factors (`time_localize`, `var_impact`).  The contraction runs on the device
(`efa_obs_impact_dev`, `efa_obs_impact_slab_dev` under the last two); there is no NumPy path.
"""
import numpy as np

from efa_xray_amd import _lib
from efa_xray_amd.assimilation.assimilation import Assimilation
from efa_xray_amd.assimilation.ensrf import ob_slab, ob_vertical, slab_setting, vertical_setting


def _error_terms(prior, post, verification, norm):
    """(v (nstate,) = c (e^a + e^b) in to_vect() row order, 0 where not verified; actual = sum c (e^a^2 - e^b^2))."""
    nvar, nt, ny, nx, _ = post.shape()
    want = (nt, ny, nx)
    if norm is not None and not hasattr(norm, "get"):
        raise ValueError("norm must be None or a mapping from variable name to weights, got %r" % type(norm).__name__)
    if not hasattr(verification, "get"):
        raise ValueError("verification must be a mapping from variable name to an array %r" % (want,))
    v = np.zeros((nvar,) + want)
    actual = 0.0
    for iv, name in enumerate(post.vars()):
        c = 1.0
        if norm is not None and norm.get(name) is not None:
            try:
                c = np.broadcast_to(np.asarray(norm[name], dtype=np.float64), want)
            except ValueError:
                raise ValueError("norm[%r] has shape %r, not broadcastable to (ntimes, ny, nx) = %r"
                                 % (name, np.shape(norm[name]), want))
            if not np.all(np.isfinite(c)) or np.any(c < 0.0):
                raise ValueError("norm[%r] must hold finite non-negative weights" % name)
        ver = verification.get(name)
        if ver is None:         # a variable that is not verified: weight 0
            continue
        ver = np.asarray(ver, dtype=np.float64)
        if ver.shape != want:
            raise ValueError("verification[%r] has shape %r but the state has (ntimes, ny, nx) = %r" % (name, ver.shape, want))
        ok = ~np.isnan(ver)
        truth = np.where(ok, ver, 0.0)
        eb = prior.variables[name].mean(axis=-1) - truth
        ea = post.variables[name].mean(axis=-1) - truth
        v[iv] = np.where(ok, c * (ea + eb), 0.0)
        actual += float(np.sum(np.where(ok, c * (ea * ea - eb * eb), 0.0)))
    return v.reshape(-1), actual


def observation_impact(prior, post, obs, verification, norm=None, loc=False, vert_coord=None, device=0, time_localize=False,
                       var_impact=None):
    """The forecast impact of every assimilated observation.

    prior, post  -- the `EnsembleState`s that went into and came out of `EnSRF(...).update()` (float64)
    obs          -- the observation list that came out of it (`ob.assimilated` says which obs were used)
    verification -- mapping variable name -> array (ntimes, ny, nx): the verifying state; NaN, or a variable that is missing,
                    means not verified (weight 0)
    norm         -- None (weight 1), or mapping variable name -> non-negative scalar or array broadcastable to (ntimes, ny, nx)
    loc, vert_coord, time_localize, var_impact -- as in `EnSRF`: pass what the update used (the taper is not advected)
    device       -- HIP device ordinal

    Returns a dict: `impact` (P,), NaN where the ob was not assimilated, negative where it reduced the error; `total`, the sum
    over the assimilated obs; `actual` = sum c (e^a^2 - e^b^2), which `total` approximates (not an identity here: the filter's
    gain mixes a ddof-0 variance with an (M-1) covariance, and localisation breaks it further).  Sets
    `ob.impact` on every ob (None where not assimilated)."""
    for what, st in (("prior", prior), ("post", post)):
        if st.dtype != np.float64:
            raise ValueError("observation_impact needs float64 states; %s is stored as %s (use state.astype(numpy.float64))"
                             % (what, np.dtype(st.dtype).name))
    if prior.shape() != post.shape() or prior.vars() != post.vars():
        raise ValueError("prior and post differ in shape or variables: %r %r and %r %r"
                         % (prior.shape(), prior.vars(), post.shape(), post.vars()))
    if loc in (None, False):
        loc_mode = _lib.LOC_NONE
    elif loc == 'GC':
        loc_mode = _lib.LOC_GC
    else:
        raise ValueError("loc=%r: supported values are None, False and 'GC'" % (loc,))
    z = vertical_setting(post, vert_coord, loc)
    ov = oh = None
    if z is not None:
        ov, oh = ob_vertical(obs)
    slab = slab_setting(post, loc, time_localize, var_impact)
    slab_kw = ob_slab(post, obs, slab) if slab is not None else None
    v, actual = _error_terms(prior, post, verification, norm)
    P = len(obs)
    used = np.array([bool(getattr(ob, "assimilated", False)) for ob in obs], dtype=bool)
    error = np.array([float(ob.error) if u else np.nan for ob, u in zip(obs, used)], dtype=np.float64)
    lat = lon = hw = None
    if loc_mode == _lib.LOC_GC:
        for k, ob in enumerate(obs):
            if used[k] and ob.localize_radius is None:
                raise ValueError("observation %d was assimilated but has localize_radius=None with loc='GC'" % k)
        lat = np.array([float(ob.lat) for ob in obs], dtype=np.float64)
        lon = np.array([float(ob.lon) for ob in obs], dtype=np.float64)
        hw = np.array([float(ob.localize_radius) if ob.localize_radius is not None else np.nan for ob in obs], dtype=np.float64)
    out = dict(impact=np.full(P, np.nan), total=0.0, actual=actual)
    if P == 0:
        return out

    nvar, nt, ny, nx, M = post.shape()
    N = post.nstate()
    # d_k = value - mean(estimate(prior)); Ya = estimates of post, which stays resident as Xf.  The default point operator runs on
    # the device through the stencil path, user-defined `estimate` through the objects
    fb = Assimilation(prior, obs, device=device)
    fa = Assimilation(post, obs, device=device)
    ctx = fa._context()
    if fa._default_forward_operator():
        yb = fb.device_ob_estimates(ctx, fb._upload_prior(ctx)).download().mean(axis=-1)
        X = fa._upload_prior(ctx)
        Ya = fa.device_ob_estimates(ctx, X)
    else:
        yb = fb.compute_ob_estimates().mean(axis=-1)
        Ya = ctx.to_device(fa.compute_ob_estimates())
        X = fa._upload_prior(ctx)
    innov = np.array([float(ob.value) - yb[k] if used[k] else np.nan for k, ob in enumerate(obs)], dtype=np.float64)
    grid_lat = grid_lon = None
    n_lead = 1
    if loc_mode == _lib.LOC_GC:
        grid_lat, grid_lon = post.column_latlon()
        n_lead = nvar * nt
    try:
        if slab_kw is None:                            # (an EnSRF on this device may have left it set)
            ctx.set_slab_localization(None)
        else:
            ctx.set_slab_localization(**slab_kw)
        if z is None:
            ctx.set_vertical_localization(None)
        else:
            ctx.set_vertical_localization(z.reshape(-1), ov, oh)
        impact = ctx.obs_impact if slab_kw is None else ctx.obs_impact_slab
        J = impact(N, M, P, X, ctx.to_device(v), Ya, innov, error, used, loc_mode, lat, lon, hw, grid_lat, grid_lon, n_lead)
    finally:
        ctx.set_slab_localization(None)
        ctx.set_vertical_localization(None)
    out["impact"] = np.where(used, J, np.nan)
    out["total"] = float(np.sum(J[used]))
    for k, ob in enumerate(obs):
        ob.impact = np.float64(J[k]) if used[k] else None
    return out
