"""NumPy model of the serial EnSRF with sampling error correction (Anderson 2012) -- TEST INFRASTRUCTURE ONLY.

`ensrf_update` is oracle/ensrf_oracle.py's loop (the reference's ensrf.py:50-149, statement for statement, in its operation
order) with ONE statement added: behind the taper, kcov is multiplied by alpha(|r|), r the sample correlation of every augmented
row with the observation, both as they are before the observation moves them; the observation's own row takes alpha = 1.  With a
table of ones that statement multiplies by exactly 1.0, so the model is then the oracle bit for bit.
"""
import numpy as np

from oracle import ensrf_oracle as orc


def lookup(alpha, r):
    """alpha(|r|), piecewise linear between the nodes j/(T-1); |r| > 1 reads the last node, a NaN r gives NaN (and no index
    outside the table)."""
    alpha = np.asarray(alpha, dtype=np.float64)
    T = alpha.size
    a = np.minimum(np.abs(np.asarray(r, dtype=np.float64)), 1.0)
    t = a * (T - 1)
    with np.errstate(invalid="ignore"):
        j = np.where(np.isnan(t), 0, np.minimum(np.floor(t), T - 2)).astype(np.int64)
    return alpha[j] + (t - j) * (alpha[j + 1] - alpha[j])


def correlation(dots, xx, yy):
    """r = x'.y' / sqrt(x'.x' y'.y') per row, 0 where either norm is 0."""
    nn = xx * yy
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(nn > 0, dots / np.sqrt(nn), np.where(np.isnan(nn), np.nan, 0.0))


def ensrf_update(xbm, Xbp, nstate, ob_value, ob_error, ob_assim, alpha, loc=None, ob_lat=None, ob_lon=None, ob_halfwidth=None,
                 grid_lat=None, grid_lon=None, state_shape=None):
    """oracle.ensrf_update with the correction; `alpha` the table.  Returns xam, Xap and the diagnostics dict."""
    xam = xbm
    Xap = Xbp
    A, M = Xap.shape
    P = len(ob_value)
    assert A == nstate + P
    use_loc = loc not in (None, False)
    if use_loc:
        grid_lat = np.asarray(grid_lat, dtype=np.float64)
        grid_lon = np.asarray(grid_lon, dtype=np.float64)
        dum_localize = np.ones(tuple(state_shape))

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
        dots = np.dot(Xb, np.transpose(ye))
        kcov = dots / (M - 1)
        if use_loc:
            sl = orc.localize_state(grid_lat, grid_lon, ob_lat[k], ob_lon[k], ob_halfwidth[k])
            if sl.ndim == 2:
                sl = (sl[None, None, :, :] * dum_localize).flatten()
            else:
                sl = (sl[None, None, None, :] * dum_localize).flatten()
            ol = orc.localize_obs(ob_lat, ob_lon, ob_lat[k], ob_lon[k], ob_halfwidth[k])
            kcov = np.multiply(np.hstack((sl, ol)), kcov)
        # ---- the correction
        xx = np.einsum("ij,ij->i", Xb, Xb)
        al = lookup(alpha, correlation(dots, xx, np.dot(ye, ye)))
        al[row] = 1.0                       # a variable with itself
        kcov = np.multiply(al, kcov)
        # ----
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


def ensrf_cycle(X, HX, ob_value, ob_error, ob_assim, alpha, **kw):
    """format_prior_state -> the loop above -> format_posterior_state, as oracle.ensrf_cycle."""
    N = X.shape[0]
    xbm, Xbp = orc.format_prior_state(X, HX)
    xam, Xap, diag = ensrf_update(xbm, Xbp, N, ob_value, ob_error, ob_assim, alpha, **kw)
    return orc.format_posterior_state(xam, Xap, N), xam, Xap, diag


def steep_table(T):
    """Nodes (j/(T-1))^2: a table that moves the result far from the uncorrected one."""
    return (np.arange(T) / (T - 1.0)) ** 2
