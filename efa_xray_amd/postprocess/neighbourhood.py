"""Neighbourhood ensemble probabilities and the fractions skill score (Schwartz et al. 2010; Schwartz and Sobash 2017; Roberts
and Lean 2008).

The products that need the (y, x) structure of the state.  For every element and threshold, over the window of radius r around
it (a square or a disc, within its own (variable, time) slab), `neighbourhood_probabilities` forms on the device
(`efa_neighbourhood_dev` / `efa_neighbourhood_f32_dev`; there is no NumPy path) the neighbourhood ensemble probability NEP, the
mean over the window's elements of k/M, and the neighbourhood maximum ensemble probability NMEP, the share of members that exceed
the threshold somewhere in the window.  `fractions_skill_score` compares NEP with the observed fraction of a verifying state.

A window needs the whole (y, x) grid on one device: a column-sharded state is not supported, gather it first.
"""
import numpy as np

from efa_xray_amd import _lib
from efa_xray_amd.assimilation.assimilation import Assimilation
from efa_xray_amd.postprocess.products import _check_state, _check_thresholds
from efa_xray_amd.postprocess.verification import _check_args as _check_verification

MAX_RADII = 4
MAX_RADIUS = 64
SHAPES = {"square": 0, "disc": 1}


def _check_windows(state, radii, shape, wrap_x):
    """(radii as an int32 array (R,), the shape's number)."""
    if np.isscalar(radii):
        radii = (radii,)
    try:
        raw = np.asarray(tuple(radii))
    except TypeError:
        raise ValueError("radii must be a sequence of at most %d integers in [0, %d]" % (MAX_RADII, MAX_RADIUS))
    if raw.ndim != 1 or raw.size < 1 or raw.size > MAX_RADII:
        raise ValueError("radii must be a sequence of 1 to %d integers in [0, %d]" % (MAX_RADII, MAX_RADIUS))
    if raw.dtype.kind not in "iuf" or not np.all(np.isfinite(raw)) or np.any(raw != np.floor(raw)):
        raise ValueError("radii must be integers in [0, %d], got %r" % (MAX_RADIUS, raw.tolist()))
    if np.any(raw < 0) or np.any(raw > MAX_RADIUS):
        raise ValueError("radii must be integers in [0, %d], got %r" % (MAX_RADIUS, raw.tolist()))
    rad = raw.astype(np.int32)
    if not isinstance(shape, str) or shape not in SHAPES:
        raise ValueError("shape=%r must be 'square' or 'disc'" % (shape,))
    nx = state.shape()[3]
    if wrap_x and 2 * int(rad.max()) + 1 > nx:
        raise ValueError("wrap_x=True needs 2*radius+1 <= nx = %d, got the radius %d" % (nx, int(rad.max())))
    return rad, SHAPES[shape]


def neighbourhood_probabilities(state, thresholds, radii, shape="square", wrap_x=False, nep=True, nmep=False, device=0):
    """Neighbourhood ensemble probability (NEP) and neighbourhood maximum ensemble probability (NMEP) of every element.

    state      -- an `EnsembleState`, stored as float64 or float32, whole on one device (a column-sharded state is not supported)
    thresholds -- mapping variable name -> at most 8 finite numbers; the event at threshold t is x > t
    radii      -- at most 4 integers in [0, 64]: the windows' radii in grid points
    shape      -- 'square' (|dy| <= r and |dx| <= r) or 'disc' (dy^2 + dx^2 <= r^2); a window stays within its (variable, time)
                  slab and is cut at the grid's edges
    wrap_x     -- the grid is periodic in x: columns are taken modulo nx (needs 2r+1 <= nx)
    nep, nmep  -- which fields to bring back
    device     -- HIP device ordinal

    Returns a dict: `radii`, and `nep` and / or `nmep`, each a mapping variable name -> (R, T_var, ntimes, ny, nx).  Over the
    elements of the window whose members are all finite, NEP is the sum of their counts k = #{m: x_m > t} over M times their
    number (at r = 0 `ensemble_products`' probability, bit for bit), NMEP the number of members above t at one of them over M.
    An element with a member that is not finite is NaN and enters no window."""
    _check_state(state)
    per_var, thr = _check_thresholds(state, thresholds, required=True)
    rad, shp = _check_windows(state, radii, shape, wrap_x)
    if not nep and not nmep:
        raise ValueError("neither nep nor nmep is wanted")
    nvar, nt, ny, nx, M = state.shape()
    N, T, R = state.nstate(), thr.shape[1], rad.size
    out = {"radii": rad.copy()}
    wanted = [k for k, on in (("nep", nep), ("nmep", nmep)) if on]
    if T == 0:
        for k in wanted:
            out[k] = {}
        return out
    ctx = _lib.get_context(device)
    X = Assimilation(state, [], device=device)._upload_prior(ctx)
    dev = {}
    try:
        for k in wanted:
            dev[k] = ctx.empty((R * T, N))
        ctx.neighbourhood(N, M, X, ny, nx, nvar * nt, thr, rad, shape=shp, wrap_x=wrap_x, **dev)
        host = dict((k, a.download().reshape(R, T, nvar, nt, ny, nx)) for k, a in dev.items())
    finally:
        for a in dev.values():
            a.free()
        X.free()
    for k in wanted:
        out[k] = dict((name, host[k][:, :per_var[name].size, iv].copy()) for iv, name in enumerate(state.vars()) if name in per_var)
    return out


def fss_from_sums(sums):
    """The scores of one (group, radius, threshold) from its sums (sum w, sum w (P-O)^2, sum w P^2, sum w O^2, sum w P, sum w O):
    a dict of fss = 1 - sum w (P-O)^2 / (sum w P^2 + sum w O^2) (NaN when that denominator is 0), mse, base_rate, forecast_rate
    and Roberts and Lean's fss_useful = 0.5 + base_rate / 2 (all NaN when sum w is 0)."""
    s = [float(v) for v in sums]
    out = dict(fss=np.nan, mse=np.nan, base_rate=np.nan, forecast_rate=np.nan, fss_useful=np.nan)
    if not s[0] > 0.0:
        return out
    den = s[2] + s[3]
    if den != 0.0:
        out["fss"] = 1.0 - s[1] / den
    out["mse"] = s[1] / s[0]
    out["forecast_rate"] = s[4] / s[0]
    out["base_rate"] = s[5] / s[0]
    out["fss_useful"] = 0.5 + out["base_rate"] / 2.0
    return out


def fractions_skill_score(state, verification, thresholds, radii, by="var", weights=None, shape="square", wrap_x=False, device=0):
    """The fractions skill score (Roberts and Lean 2008) of the neighbourhood ensemble probability against a verifying state.

    state        -- an `EnsembleState`, stored as float64 or float32, whole on one device (a column-sharded state is not supported)
    verification -- mapping variable name -> array (ntimes, ny, nx): the verifying state; NaN, or a variable that is missing,
                    means not verified (such an element enters no window either); an infinite value raises ValueError
    thresholds   -- mapping variable name -> at most 8 finite numbers; the event at threshold t is x > t
    radii        -- at most 4 integers in [0, 64]
    by           -- 'var' (one group per variable), 'var_time' (one per variable and valid time) or None (one group)
    weights      -- None, or (ny, nx) finite weights >= 0; an element of weight 0 is not scored but counts in its neighbours' windows
    shape, wrap_x -- as in `neighbourhood_probabilities`
    device       -- HIP device ordinal

    With P the NEP and O the observed fraction (the share of the window's elements whose verifying value exceeds t), returns a
    dict of arrays (G, R, T): `fss` = 1 - sum w (P-O)^2 / (sum w P^2 + sum w O^2) (NaN when the denominator is 0 or n == 0),
    `mse`, `base_rate`, `forecast_rate`, `fss_useful` = 0.5 + base_rate / 2, `n` and `n_bad` (scored elements; elements that
    would be scored but have a member that is not finite), the raw `sums` (G, R, T, 6), and `groups` (labels), `radii` and
    `thresholds` (G, T), NaN where the group has no such threshold."""
    verif, groups, labels, w, _, _ = _check_verification(state, verification, by, weights, 0, ())
    per_var, thr = _check_thresholds(state, thresholds, required=True)
    rad, shp = _check_windows(state, radii, shape, wrap_x)
    nvar, nt, ny, nx, M = state.shape()
    N, T, R, G = state.nstate(), thr.shape[1], rad.size, len(labels)
    gthr = np.full((G, T), np.nan)
    if by is None:    # one group over variables whose thresholds may differ: each is scored at its own, the label is the first's
        for s in range(nvar * nt - 1, -1, -1):
            gthr[0] = np.where(np.isnan(thr[s]), gthr[0], thr[s])
    else:
        for s in range(nvar * nt):
            gthr[groups[s]] = thr[s]
    keys = ("fss", "mse", "base_rate", "forecast_rate", "fss_useful")
    out = dict((k, np.full((G, R, T), np.nan)) for k in keys)
    out.update(groups=labels, radii=rad.copy(), thresholds=gthr, n=np.zeros((G, R, T), dtype=np.int64),
               n_bad=np.zeros((G, R, T), dtype=np.int64), sums=np.zeros((G, R, T, 6)))
    if T == 0:
        return out
    ctx = _lib.get_context(device)
    X = Assimilation(state, [], device=device)._upload_prior(ctx)
    d_ver = d_w = None
    try:
        d_ver = ctx.to_device(verif.reshape(-1))
        if w is not None:
            d_w = ctx.to_device(w)
        sums, n, n_bad = ctx.neighbourhood(N, M, X, ny, nx, nvar * nt, thr, rad, shape=shp, wrap_x=wrap_x, verif=d_ver,
                                           slab_group=groups, col_weight=d_w)
    finally:
        for a in (d_ver, d_w):
            if a is not None:
                a.free()
        X.free()
    out.update(sums=sums, n=n, n_bad=n_bad)
    for g in range(G):
        for i in range(R):
            for j in range(T):
                if n[g, i, j] == 0:
                    continue
                sc = fss_from_sums(sums[g, i, j])
                for k in keys:
                    out[k][g, i, j] = sc[k]
    return out
