"""The LETKF's deterministic control analysis in NumPy, for the tests: written from the definition, on top of
tests/_letkf.py (the taper, the seeded case) and tests/_letkf_slab.py (the slab table, the groups, the obs-obs factors).

For a location x (a grid column, a (slab group, column), an ob position), over the obs with an effective flag a_k = 1 and
rho_k(x) != 0, with d^c_k = value_k - y_c[k] (R-localisation, the inflation shift (M-1)/lambda_b on the diagonal):
    A_x = (M-1)/lambda_b I + sum_k (rho_k/r_k) Yp_k^T Yp_k,   g^c_x = sum_k (rho_k/r_k) d^c_k Yp_k^T,   w^c_x = A_x^-1 g^c_x.
State rows: x_c^a[row] = x_c[row] + X'[row, :] . w^c of the row's (group, column), X' the row's prior perturbations.  Obs block:
y_c^a[j] = y_c[j] + Yp_j . w^c(ob j's position).  A point no ob reaches leaves its rows as they are.  Two routes to w^c:
numpy.linalg.eigh per point (V diag(1/mu) V^T g^c) and numpy.linalg.solve(A, g^c)."""
import numpy as np

import _etkf
import _letkf
import _letkf_slab


def control_weight(rho_x, Yp, value, yc, error, assim, lam_b=1.0, route="eigh"):
    """(w^c, cond(A)) at one location from its taper row; (None, 1.0) when no ob reaches it.  A NaN in g^c poisons all of w^c."""
    Yp = np.asarray(Yp, dtype=np.float64)
    M = Yp.shape[1]
    use = np.asarray(assim, dtype=bool) & (rho_x != 0.0)
    if not use.any():
        return None, 1.0
    wt = rho_x[use] / np.asarray(error, dtype=np.float64)[use]
    Y = Yp[use]
    dc = np.asarray(value, dtype=np.float64)[use] - np.asarray(yc, dtype=np.float64)[use]
    A = (M - 1.0) / lam_b * np.eye(M) + Y.T @ (wt[:, None] * Y)
    g = Y.T @ (wt * dc)
    mu, V = np.linalg.eigh(A)
    cond = float(mu.max() / mu.min())
    if not np.all(np.isfinite(g)):
        return np.full(M, np.nan), cond
    if route == "eigh":
        return (V / mu) @ (V.T @ g), cond
    return np.linalg.solve(A, g), cond


def plain_tapers(c, assim=None):
    """(rho_cols (1, ncol, P), group_of (n_lead,), rho_obs (P, P)) of a case of tests/_letkf.py under the flags `assim`."""
    a = c["assim"] if assim is None else assim
    rho = _letkf.taper(c["grid_lat"], c["grid_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], a)
    rho_o = _letkf.taper(c["ob_lat"], c["ob_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], a) if c["P"] else np.zeros((0, 0))
    return rho[None], np.zeros(c["n_lead"], dtype=np.int64), rho_o


def slab_tapers(c, assim=None):
    """... of a case of tests/_letkf_slab.py: rho_cols (ngroups, ncol, P) under the slab factors, the obs' under the obs-obs factors."""
    a = c["assim"] if assim is None else assim
    P, n_lead, loc = c["P"], c["n_lead"], c["loc"]
    S = _letkf_slab.slab_table(n_lead, P, loc)
    group_of, rep = _letkf_slab.groups(n_lead, P, loc)
    rho_h = _letkf.taper(c["grid_lat"], c["grid_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], a)
    rho = np.stack([rho_h * S[:, r][None, :] for r in rep])
    rho_o = _letkf.taper(c["ob_lat"], c["ob_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], a) * _letkf_slab.obs_factor(P, loc)
    return rho, group_of, rho_o


def control_cycle(X, HX, xc, yc, value, error, assim, rho_cols, group_of, rho_obs, lam=None, ob_infl=None, route="eigh"):
    """The control analysis of one cycle: xc_post (rows,), yc_post (P,), reached (ngroups, ncol), ob_reached (P,) and the largest
    cond(A) met.  assim: the EFFECTIVE flags.  lam (ngroups, ncol) / ob_infl (P,): the inflation factors of the solves, or None."""
    X = np.asarray(X, dtype=np.float64)
    M = X.shape[1]
    P = len(HX)
    ym, Yp = _etkf.ob_priors(HX) if P else (np.zeros(0), np.zeros((0, M)))
    ng, ncol = rho_cols.shape[:2]
    Xp = X - X.mean(axis=1, keepdims=True)
    xc = np.asarray(xc, dtype=np.float64)
    xc_post = np.array(xc)
    reached = np.zeros((ng, ncol), dtype=bool)
    cond = 1.0
    for g in range(ng):
        slabs = np.flatnonzero(group_of == g)
        for c in range(ncol):
            w, k = control_weight(rho_cols[g, c], Yp, value, yc, error, assim, 1.0 if lam is None else lam[g, c], route)
            if w is None:
                continue
            reached[g, c] = True
            cond = max(cond, k)
            rows = slabs * ncol + c
            xc_post[rows] = xc[rows] + Xp[rows] @ w
    yc = np.asarray(yc, dtype=np.float64)
    yc_post = np.array(yc)
    ob_reached = np.zeros(P, dtype=bool)
    for j in range(P):
        w, k = control_weight(rho_obs[j], Yp, value, yc, error, assim, 1.0 if ob_infl is None else ob_infl[j], route)
        if w is None:
            continue
        ob_reached[j] = True
        cond = max(cond, k)
        yc_post[j] = yc[j] + Yp[j] @ w
    return dict(xc_post=xc_post, yc_post=yc_post, reached=reached, ob_reached=ob_reached, cond=cond, ym=ym, Yp=Yp)


def control_inputs(c, seed=0):
    """The seeded control of a case: x_c = row mean + 0.5 normal, y_c = ym + sqrt(err) normal."""
    rng = np.random.default_rng(4241 * c["M"] + 7 * c["P"] + seed)
    X = np.asarray(c["X"], dtype=np.float64)
    xc = X.mean(axis=1) + 0.5 * rng.standard_normal(X.shape[0])
    ym = _etkf.ob_priors(c["HX"])[0] if c["P"] else np.zeros(0)
    yc = ym + np.sqrt(c["error"]) * rng.standard_normal(c["P"])
    return xc, yc
