"""Per-point multiplicative inflation of the LETKF in NumPy, for the tests: written from the definition.

For a solve point x with prior factor lam_b > 0, over the obs with an effective flag and rho_k(x) != 0, w_k = rho_k/r_k:
    A_x = ((M-1)/lam_b) I + C_x = V diag(mu) V^T,  T = V diag(sqrt((M-1)/mu)) V^T,  w = V diag(1/mu) V^T g,
    dfs = sum_i (mu_i - (M-1)/lam_b)/mu_i,
    p1 = sum_k w_k d_k^2,  p2 = sum_k w_k |Yp_k|^2/(M-1),  p3 = sum_k rho_k,
    lam_o = (p1 - p3)/p2,  v_o = (2/p3) ((lam_b p2 + p3)/p2)^2,  v_b = sigma_b^2,
    lam_a = clip(lam_b + v_b/(v_o + v_b) (lam_o - lam_b), lower, upper).
The solve uses lam_b.  lam_a stays lam_b when sigma_b == 0, when no ob reaches the point, when p2 or p3 is not finite and positive,
and when the estimate is not finite.  Obs row j is solved at its own position under ob_infl[j], which is never updated."""
import numpy as np

import _etkf
import _letkf


def solve_point(rho_x, ym, Yp, value, error, assim, lam_b=1.0):
    """(T, w, extras) at one location: tests/_letkf.py's solve_point with the prior factor, and p1, p2, p3, lam_o."""
    Yp = np.asarray(Yp, dtype=np.float64)
    M = Yp.shape[1]
    use = np.asarray(assim, dtype=bool) & (rho_x != 0.0)
    if not use.any():
        return np.eye(M), np.zeros(M), dict(n_local=0, dfs=0.0, cond=1.0, p1=0.0, p2=0.0, p3=0.0, lam_o=np.nan, q=(0.0, 0.0, 0.0))
    rho = rho_x[use]
    wt = rho / np.asarray(error, dtype=np.float64)[use]
    Y = Yp[use]
    d = np.asarray(value, dtype=np.float64)[use] - np.asarray(ym, dtype=np.float64)[use]
    C = Y.T @ (wt[:, None] * Y)
    g = Y.T @ (wt * d)
    shift = (M - 1.0) / lam_b
    mu, V = np.linalg.eigh(shift * np.eye(M) + C)
    T = (V * np.sqrt((M - 1.0) / mu)) @ V.T
    w = (V / mu) @ (V.T @ g) if np.all(np.isfinite(g)) else np.full(M, np.nan)
    p1 = float(np.sum(wt * d * d))
    p2 = float(np.sum(wt * np.sum(Y * Y, axis=1))) / (M - 1.0)
    p3 = float(np.sum(rho))
    # q_i = sum_k |d p_i / d rho_k|: what an absolute error of the tapers does to the three sums
    q = (float(np.sum(d * d / np.asarray(error, dtype=np.float64)[use])),
         float(np.sum(np.sum(Y * Y, axis=1) / np.asarray(error, dtype=np.float64)[use])) / (M - 1.0), float(use.sum()))
    with np.errstate(divide="ignore", invalid="ignore"):
        lam_o = float((np.float64(p1) - p3) / np.float64(p2))
    return T, w, dict(n_local=int(use.sum()), dfs=float(np.sum((mu - shift) / mu)), cond=float(mu.max() / mu.min()), p1=p1, p2=p2,
                      p3=p3, lam_o=lam_o, q=q)


def estimate(lam_b, p1, p2, p3, sigma_b, lower, upper):
    """lam_a of one point."""
    if sigma_b == 0.0 or not (np.isfinite(p2) and p2 > 0.0 and np.isfinite(p3) and p3 > 0.0):
        return lam_b
    lam_o = (p1 - p3) / p2
    v_o = (2.0 / p3) * ((lam_b * p2 + p3) / p2) ** 2
    v_b = sigma_b * sigma_b
    la = lam_b + v_b / (v_o + v_b) * (lam_o - lam_b)
    if not np.isfinite(la):
        return lam_b
    return min(max(la, lower), upper)


def points(rho, lam, ym, Yp, value, error, assim, sigma_b=0.0, lower=1e-2, upper=1e2):
    """Every point of the taper rho (npts, P) under its factor lam (npts,): T, w, statistics (n_local, dfs, cond, p (npts, 4) =
    p1, p2, p3, lam_o, and q (npts, 3) = sum_k |d p_i / d rho_k|), and lam_a (npts,)."""
    n, M = rho.shape[0], np.asarray(Yp).shape[1]
    T, w = np.empty((n, M, M)), np.empty((n, M))
    st = dict(n_local=np.zeros(n, dtype=np.int64), dfs=np.zeros(n), cond=np.ones(n), p=np.zeros((n, 4)), q=np.zeros((n, 3)))
    lam_a = np.array(lam, dtype=np.float64)
    for i in range(n):
        T[i], w[i], ex = solve_point(rho[i], ym, Yp, value, error, assim, lam[i])
        for k in ("n_local", "dfs", "cond"):
            st[k][i] = ex[k]
        st["p"][i] = ex["p1"], ex["p2"], ex["p3"], ex["lam_o"]
        st["q"][i] = ex["q"]
        if ex["n_local"]:
            lam_a[i] = estimate(lam[i], ex["p1"], ex["p2"], ex["p3"], sigma_b, lower, upper)
    return T, w, st, lam_a


def obs_block(rho_o, ym, Yp, value, error, assim, ob_infl=None):
    """The posterior obs block (ym, Yp): ob j through the pair solved under rho_o[j] and ob_infl[j] (None: 1.0)."""
    P = len(ym)
    yam, Yap = np.array(ym), np.array(Yp)
    for j in range(P):
        To, wo, ex = solve_point(rho_o[j], ym, Yp, value, error, assim, 1.0 if ob_infl is None else ob_infl[j])
        if ex["n_local"]:
            a, b = _etkf.etkf_apply(ym[j:j + 1], Yp[j:j + 1], To, wo)
            yam[j], Yap[j] = a[0], b[0]
    return yam, Yap


def diagnostics(ym, Yp, yam, Yap, assim):
    a = np.asarray(assim, dtype=bool)
    P = len(ym)
    return dict(prior_mean=np.array(ym), prior_var=np.var(Yp, axis=1) if P else np.zeros(0), post_mean=np.where(a, yam, np.nan),
                post_var=np.where(a, np.var(Yap, axis=1), np.nan) if P else np.zeros(0), assimilated=a)


def letkf_cycle(X, HX, value, error, assim, ob_lat, ob_lon, ob_hw, grid_lat, grid_lon, n_lead, lam, ob_infl=None, sigma_b=0.0,
                lower=1e-2, upper=1e2):
    """tests/_letkf.py's letkf_cycle under the column field lam (ncol,) and the ob factors: posterior members, obs block,
    diagnostics, statistics, and lam_a."""
    X = np.asarray(X, dtype=np.float64)
    M = X.shape[1]
    ym, Yp = _etkf.ob_priors(HX) if len(HX) else (np.zeros(0), np.zeros((0, M)))
    glat = np.asarray(grid_lat, dtype=np.float64).reshape(-1)
    glon = np.asarray(grid_lon, dtype=np.float64).reshape(-1)
    ncol = glat.size
    rho = _letkf.taper(glat, glon, ob_lat, ob_lon, ob_hw, assim)
    Tc, wc, st, lam_a = points(rho, lam, ym, Yp, value, error, assim, sigma_b, lower, upper)
    post = np.array(X)
    for c in range(ncol):
        if st["n_local"][c]:
            rows = c + ncol * np.arange(n_lead)
            post[rows] = _etkf.etkf_members(X[rows], Tc[c], wc[c])
    rho_o = _letkf.taper(ob_lat, ob_lon, ob_lat, ob_lon, ob_hw, assim)
    yam, Yap = obs_block(rho_o, ym, Yp, value, error, assim, ob_infl)
    return dict(post=post, ym=yam, Yp=Yap, diag=diagnostics(ym, Yp, yam, Yap, assim), stats=st, T=Tc, w=wc, rho=rho, lam_a=lam_a,
                prior_ym=ym, prior_Yp=Yp)


def inflate_rows(X, lam):
    """Member rows with their perturbations scaled by sqrt(lam) (a scalar or one factor per row), the means kept."""
    X = np.asarray(X, dtype=np.float64)
    m = X.mean(axis=1, keepdims=True)
    return m + np.sqrt(np.asarray(lam, dtype=np.float64)).reshape(-1, 1) * (X - m)


def ob_factors(lam_rows, idx, wts):
    """lam_ob[j] = sum_e wts[j, e] lam_rows[idx[j, e]]: the ob's own point interpolation applied to the field expanded to state
    rows (an entry of weight 0 is not read)."""
    idx, wts = np.asarray(idx), np.asarray(wts, dtype=np.float64)
    out = np.zeros(idx.shape[0])
    for j in range(idx.shape[0]):
        for e in range(idx.shape[1]):
            if wts[j, e] != 0.0:
                out[j] += wts[j, e] * lam_rows[idx[j, e]]
    return out
