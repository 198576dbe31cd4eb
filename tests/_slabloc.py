"""NumPy test oracle of temporal and cross-variable localisation: the serial loop of `tests/_vertloc.py` restated
with the product taper, built from the oracle's own `localize_state` / `localize_obs` / `localize_obs_vec` and
`_vertloc.vertical_factor` (the oracle's `gaspari_cohn`, 1 where a coordinate is NaN).  (x * 1.0 is x: an ob with vertical
information only takes `_vertloc`'s statements bit for bit.)

State row i = s * ncol + column (slab s = variable-major, then valid time; variable v_s, time t_s) tapers ob k by
GC_h(column, k) * S(k, s) with S = (V * T) * C: V the vertical factor of 7d, T = GC(|t_s - t_k|, tau_k) and C = impact[group_k, v_s].
Obs row j takes GC_h(j, k) * ((V(j,k) * T(j,k)) * C[k, v_j]).  T is 1 where t_x is NaN (a row without a time) and for an ob k
whose t_k or tau_k is NaN; C is 1 for an ob without an impact row (group -1) and for an obs row without a target variable
(ob_var -1); V is 1 as in `_vertloc`.  `rows` restricts the state to the given global rows (exact for them)."""
import numpy as np

from oracle.ensrf_oracle import localize_obs, localize_obs_vec, localize_state

from _vertloc import vertical_factor


def temporal_factor(t, t_k, tau_k):
    """GC(|t - t_k|, tau_k) for the array t, 1 where t is NaN; all ones when t_k or tau_k is NaN."""
    t = np.asarray(t, dtype=np.float64)
    if np.isnan(t_k) or np.isnan(tau_k):
        return np.ones(t.shape)
    return vertical_factor(t, t_k, tau_k)


def impact_factor(impact, group_k, var):
    """impact[group_k, var] for the int array var, 1 where var is -1; all ones when group_k is -1 or there is no table."""
    var = np.asarray(var, dtype=np.int64)
    if impact is None or group_k < 0:
        return np.ones(var.shape)
    row = np.asarray(impact, dtype=np.float64)[group_k]
    return np.where(var >= 0, row[np.maximum(var, 0)], 1.0)


def slab_factor_table(n_lead, P, lead_vert=None, ob_vert=None, ob_vert_halfwidth=None, lead_time=None, ob_time=None,
                      ob_time_halfwidth=None, lead_var=None, ob_group=None, impact=None):
    """S[P][n_lead] = (V T) C, each product rounded once in that order."""
    S = np.ones((P, n_lead))
    for k in range(P):
        S[k] = _slab_row(k, np.arange(n_lead), n_lead, P, lead_vert, ob_vert, ob_vert_halfwidth, lead_time, ob_time,
                         ob_time_halfwidth, lead_var, ob_group, impact)
    return S


def _arrays(n_lead, P, lead_vert, ob_vert, ob_vert_halfwidth, lead_time, ob_time, ob_time_halfwidth, lead_var, ob_group, ob_var):
    nan_l, nan_p = np.full(n_lead, np.nan), np.full(P, np.nan)
    f = lambda a, d: d if a is None else np.asarray(a, dtype=np.float64).reshape(-1)
    i = lambda a, n: np.full(n, -1, dtype=np.int64) if a is None else np.asarray(a, dtype=np.int64).reshape(-1)
    return (f(lead_vert, nan_l), f(ob_vert, nan_p), f(ob_vert_halfwidth, nan_p), f(lead_time, nan_l), f(ob_time, nan_p),
            f(ob_time_halfwidth, nan_p), i(lead_var, n_lead), i(ob_group, P), i(ob_var, P))


def _slab_row(k, lead_of, n_lead, P, lead_vert, ob_vert, ob_vert_halfwidth, lead_time, ob_time, ob_time_halfwidth, lead_var,
              ob_group, impact):
    lv, ov, oc, lt, ot, oh, lvar, og, _ = _arrays(n_lead, P, lead_vert, ob_vert, ob_vert_halfwidth, lead_time, ob_time,
                                                  ob_time_halfwidth, lead_var, ob_group, None)
    has_v = not (np.isnan(ov[k]) or np.isnan(oc[k]))
    V = vertical_factor(lv, ov[k], oc[k])[lead_of] if has_v else np.ones(len(lead_of))
    T = temporal_factor(lt, ot[k], oh[k])[lead_of]
    C = impact_factor(impact, og[k], lvar)[lead_of]
    return (V * T) * C


def ensrf_update_slab(xbm, Xbp, nstate, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_halfwidth, grid_lat, grid_lon,
                      state_shape, lead_vert=None, ob_vert=None, ob_vert_halfwidth=None, lead_time=None, ob_time=None,
                      ob_time_halfwidth=None, lead_var=None, ob_group=None, ob_var=None, impact=None, rows=None, obs_taper="loop"):
    """xbm (A,), Xbp (A, M): augmented prior mean / perturbations, A = nstate + P (state rows first: all of them, or the global rows
    `rows` in that order).  lead_* (nvar*nt,), ob_* (P,): NaN (floats) / -1 (ints) where missing; None: none.  impact
    [n_group][n_var].  Returns xam, Xap and the per-ob diagnostics as `oracle.ensrf_update` does."""
    xam = xbm
    Xap = Xbp
    A, M = Xap.shape
    P = len(ob_value)
    assert A == nstate + P
    loc_obs = {"loop": localize_obs, "vector": localize_obs_vec}[obs_taper]
    grid_lat = np.asarray(grid_lat, dtype=np.float64)
    grid_lon = np.asarray(grid_lon, dtype=np.float64)
    nvar, nt = state_shape[0], state_shape[1]
    n_lead = nvar * nt
    dum_localize = np.ones(tuple(state_shape))
    ncol = int(np.prod(state_shape[2:]))
    gidx = np.arange(n_lead * ncol) if rows is None else np.asarray(rows, dtype=np.int64)
    assert len(gidx) == nstate
    lead_of = gidx // ncol
    if rows is not None:
        assert grid_lat.shape == tuple(state_shape[2:]), "rows= needs the 2-D (ny, nx) grid"
        col_lat = grid_lat.reshape(-1)[gidx % ncol]
        col_lon = grid_lon.reshape(-1)[gidx % ncol]
    lv, ov, oc, lt, ot, oh, lvar, og, ovar = _arrays(n_lead, P, lead_vert, ob_vert, ob_vert_halfwidth, lead_time, ob_time,
                                                     ob_time_halfwidth, lead_var, ob_group, ob_var)
    has_v = ~np.isnan(ov) & ~np.isnan(oc)
    ovj = np.where(has_v, ov, np.nan)  # an ob without vertical information takes factor 1 as a target too (7d)
    has_t = ~np.isnan(ot) & ~np.isnan(oh)
    any_factor = has_v.any() or has_t.any() or (impact is not None and (og >= 0).any())

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
        if any_factor and (has_v[k] or has_t[k] or og[k] >= 0):  # (an ob without any factor takes exactly the oracle's statements)
            Vs = vertical_factor(lv, ov[k], oc[k])[lead_of] if has_v[k] else np.ones(nstate)
            Vo = vertical_factor(ovj, ov[k], oc[k]) if has_v[k] else np.ones(P)
            fs = (Vs * temporal_factor(lt, ot[k], oh[k])[lead_of]) * impact_factor(impact, og[k], lvar)[lead_of]
            fo = (Vo * temporal_factor(ot, ot[k], oh[k])) * impact_factor(impact, og[k], ovar)
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
