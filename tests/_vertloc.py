"""NumPy test oracle of vertical localisation: the serial loop of `oracle.ensrf_update` restated with the product
taper, built from the oracle's own `localize_state` / `localize_obs` / `localize_obs_vec` / `gaspari_cohn`.

State row i = s * ncol + column (slab s = variable-major, then valid time) tapers ob k by GC_h(column, k) * GC(|z_s - z_k|, c_k),
and obs row j by GC_h(j, k) * GC(|z_j - z_k|, c_k).  The vertical factor is 1 where z_s or z_j is NaN, and for an ob k whose
z_k or c_k is NaN (no vertical information); such an ob takes exactly the oracle's statements.  `rows` restricts the state to the
given global rows (they are independent given the obs trajectory, so this is exact for them)."""
import numpy as np

from oracle.ensrf_oracle import gaspari_cohn, localize_obs, localize_obs_vec, localize_state


def vertical_factor(z, z_k, c_k):
    """GC(|z - z_k|, c_k), 1 where z is NaN (z an array)."""
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        w = gaspari_cohn(np.abs(z - z_k), c_k)
    return np.where(np.isnan(z), 1.0, w)


def ensrf_update_vert(xbm, Xbp, nstate, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_halfwidth, grid_lat, grid_lon,
                      state_shape, lead_vert=None, ob_vert=None, ob_vert_halfwidth=None, rows=None, obs_taper="loop"):
    """xbm (A,), Xbp (A, M): augmented prior mean / perturbations, A = nstate + P (state rows first: all of them, or the
    global rows `rows` in that order).  lead_vert (nvar*nt,), ob_vert / ob_vert_halfwidth (P,): NaN where missing; None: none.
    Returns xam, Xap and the per-ob diagnostics as `oracle.ensrf_update` does."""
    xam = xbm
    Xap = Xbp
    A, M = Xap.shape
    P = len(ob_value)
    assert A == nstate + P
    loc_obs = {"loop": localize_obs, "vector": localize_obs_vec}[obs_taper]
    grid_lat = np.asarray(grid_lat, dtype=np.float64)
    grid_lon = np.asarray(grid_lon, dtype=np.float64)
    nvar, nt = state_shape[0], state_shape[1]
    dum_localize = np.ones(tuple(state_shape))
    ncol = int(np.prod(state_shape[2:]))
    gidx = np.arange(nvar * nt * ncol) if rows is None else np.asarray(rows, dtype=np.int64)
    assert len(gidx) == nstate
    lead_of = gidx // ncol
    if rows is not None:
        assert grid_lat.shape == tuple(state_shape[2:]), "rows= needs the 2-D (ny, nx) grid"
        col_lat = grid_lat.reshape(-1)[gidx % ncol]
        col_lon = grid_lon.reshape(-1)[gidx % ncol]
    lv = np.full(nvar * nt, np.nan) if lead_vert is None else np.asarray(lead_vert, dtype=np.float64).reshape(-1)
    ov = np.full(P, np.nan) if ob_vert is None else np.asarray(ob_vert, dtype=np.float64)
    oc = np.full(P, np.nan) if ob_vert_halfwidth is None else np.asarray(ob_vert_halfwidth, dtype=np.float64)
    has_v = ~np.isnan(ov) & ~np.isnan(oc)
    ovj = np.where(has_v, ov, np.nan)  # an ob without vertical information takes factor 1 as a target too

    prior_mean = np.full(P, np.nan)
    prior_var = np.full(P, np.nan)
    post_mean = np.full(P, np.nan)
    post_var = np.full(P, np.nan)
    assimilated = np.zeros(P, dtype=bool)
    for k in range(P):
        xb = xam
        Xb = Xap
        row = nstate + k
        mye = xb[row]
        ye = Xb[row]
        prior_mean[k] = mye
        varye = np.var(ye)
        prior_var[k] = varye
        if not ob_assim[k]:
            continue
        obs_err = ob_error[k]
        innov = ob_value[k] - mye
        kdenom = varye + obs_err
        kcov = np.dot(Xb, np.transpose(ye)) / (M - 1)
        if rows is None:
            sl = localize_state(grid_lat, grid_lon, ob_lat[k], ob_lon[k], ob_halfwidth[k])
            if sl.ndim == 2:
                sl = (sl[None, None, :, :] * dum_localize).flatten()
            else:
                sl = (sl[None, None, None, :] * dum_localize).flatten()
        else:  # the same element-wise arithmetic at the rows' columns only
            sl = localize_state(col_lat, col_lon, ob_lat[k], ob_lon[k], ob_halfwidth[k])
        ol = loc_obs(ob_lat, ob_lon, ob_lat[k], ob_lon[k], ob_halfwidth[k])
        taper = np.hstack((sl, ol))
        if has_v[k]:
            fs = vertical_factor(lv, ov[k], oc[k])[lead_of]
            fo = vertical_factor(ovj, ov[k], oc[k])
            taper = taper * np.hstack((fs, fo))
        kcov = np.multiply(taper, kcov)
        kmat = np.divide(kcov, kdenom)
        xam = xb + np.multiply(kmat, innov)
        beta = 1.0 / (1.0 + np.sqrt(obs_err / (varye + obs_err)))
        kmat = np.multiply(beta, kmat)
        ye2 = np.array(ye)[np.newaxis]
        kmat2 = np.array(kmat)[np.newaxis]
        Xap = Xb - np.dot(kmat2.T, ye2)
        post_mean[k] = xam[row]
        post_var[k] = np.var(Xap[row])
        assimilated[k] = True
    diag = dict(prior_mean=prior_mean, prior_var=prior_var, post_mean=post_mean, post_var=post_var, assimilated=assimilated)
    return xam, Xap, diag
