"""The local ensemble transform Kalman filter (LETKF) in NumPy, for the tests: written from the definition.

For a location x (a grid column or an ob position), over the obs with an effective flag a_k = 1 and rho_k(x) =
gaspari_cohn(distance(x, ob k), halfwidth_k) != 0, with d_k = value_k - ym_k (R-localisation: the taper multiplies 1/r_k):
    C_x = sum_k (rho_k/r_k) Yp_k^T Yp_k,  g_x = sum_k (rho_k/r_k) d_k Yp_k^T,  A_x = (M-1) I + C_x = V diag(mu) V^T,
    T_x = V diag(sqrt((M-1)/mu)) V^T,     w_x = V diag(1/mu) V^T g_x.
State rows: the n_lead rows of column c (row lead*ncol + c) map with (T_c, w_c); obs block: ob j with the pair at its own position.
Every solve reads the prior obs block.  The effective flags are the caller's, or tests/_outlier.py's mask applied to them."""
import numpy as np

from oracle import ensrf_oracle as orc
import _etkf


def taper(pt_lat, pt_lon, ob_lat, ob_lon, ob_hw, assim):
    """rho (npts, P): the taper of ob k at every point; 0 for an ob with a flag of 0 (its half-width is never read)."""
    pt_lat = np.asarray(pt_lat, dtype=np.float64).reshape(-1)
    pt_lon = np.asarray(pt_lon, dtype=np.float64).reshape(-1)
    P = len(ob_lat)
    rho = np.zeros((pt_lat.size, P))
    for k in range(P):
        if assim[k]:
            rho[:, k] = orc.gaspari_cohn(orc.distance_to_point(pt_lat, pt_lon, ob_lat[k], ob_lon[k]), ob_hw[k])
    return rho


def solve_point(rho_x, ym, Yp, value, error, assim):
    """(T, w, extras) at one location from its taper row, through numpy.linalg.eigh."""
    Yp = np.asarray(Yp, dtype=np.float64)
    M = Yp.shape[1]
    use = np.asarray(assim, dtype=bool) & (rho_x != 0.0)
    wt = rho_x[use] / np.asarray(error, dtype=np.float64)[use]
    Y = Yp[use]
    d = np.asarray(value, dtype=np.float64)[use] - np.asarray(ym, dtype=np.float64)[use]
    C = Y.T @ (wt[:, None] * Y)
    g = Y.T @ (wt * d)
    A = (M - 1.0) * np.eye(M) + C
    if not use.any():
        return np.eye(M), np.zeros(M), dict(n_local=0, dfs=0.0, cond=1.0, A=A, g=g)
    mu, V = np.linalg.eigh(A)
    T = (V * np.sqrt((M - 1.0) / mu)) @ V.T
    w = (V / mu) @ (V.T @ g) if np.all(np.isfinite(g)) else np.full(M, np.nan)      # a NaN value poisons w, and w only
    return T, w, dict(n_local=int(use.sum()), dfs=float(np.sum((mu - (M - 1.0)) / mu)), cond=float(mu.max() / mu.min()), A=A, g=g)


def solve_point_svd(rho_x, ym, Yp, value, error, assim):
    """The same pair by another route: numpy.linalg.solve for w, the SVD of the weighted Y for T (as _etkf.etkf_solution_svd)."""
    Yp = np.asarray(Yp, dtype=np.float64)
    M = Yp.shape[1]
    use = np.asarray(assim, dtype=bool) & (rho_x != 0.0)
    if not use.any():
        return np.eye(M), np.zeros(M)
    s = np.sqrt(rho_x[use] / np.asarray(error, dtype=np.float64)[use])
    Yt = s[:, None] * Yp[use]
    dt = s * (np.asarray(value, dtype=np.float64)[use] - np.asarray(ym, dtype=np.float64)[use])
    _, sv, Vt = np.linalg.svd(Yt, full_matrices=True)
    lam = np.zeros(M)
    lam[:sv.size] = sv ** 2
    T = (Vt.T * np.sqrt((M - 1.0) / (M - 1.0 + lam))) @ Vt
    w = np.linalg.solve((M - 1.0) * np.eye(M) + Yt.T @ Yt, Yt.T @ dt)
    return T, w


def weights(pt_lat, pt_lon, ym, Yp, value, error, assim, ob_lat, ob_lon, ob_hw, route=solve_point):
    """T (npts, M, M), w (npts, M) and, for the eigh route, stats: n_local, dfs, cond per point."""
    rho = taper(pt_lat, pt_lon, ob_lat, ob_lon, ob_hw, assim)
    M = np.asarray(Yp).shape[1]
    n = rho.shape[0]
    T = np.empty((n, M, M))
    w = np.empty((n, M))
    st = dict(n_local=np.zeros(n, dtype=np.int64), dfs=np.zeros(n), cond=np.ones(n))
    for i in range(n):
        out = route(rho[i], ym, Yp, value, error, assim)
        T[i], w[i] = out[0], out[1]
        if len(out) > 2:
            for key in st:
                st[key][i] = out[2][key]
    return T, w, st, rho


def letkf_cycle(X, HX, value, error, assim, ob_lat, ob_lon, ob_hw, grid_lat, grid_lon, n_lead):
    """The whole cycle on member rows X (n_lead*ncol, M) and obs estimates HX (P, M): posterior members, the posterior obs block
    (ym, Yp), the diagnostics, and the per-column statistics."""
    X = np.asarray(X, dtype=np.float64)
    ym, Yp = _etkf.ob_priors(HX) if len(HX) else (np.zeros(0), np.zeros((0, X.shape[1])))
    glat = np.asarray(grid_lat, dtype=np.float64).reshape(-1)
    glon = np.asarray(grid_lon, dtype=np.float64).reshape(-1)
    ncol, M = glat.size, X.shape[1]
    Tc, wc, st, rho = weights(glat, glon, ym, Yp, value, error, assim, ob_lat, ob_lon, ob_hw)
    post = np.empty_like(X)
    for c in range(ncol):
        rows = c + ncol * np.arange(n_lead)
        if st["n_local"][c] == 0:
            post[rows] = X[rows]
        else:
            post[rows] = _etkf.etkf_members(X[rows], Tc[c], wc[c])
    To, wo, sto, _ = weights(ob_lat, ob_lon, ym, Yp, value, error, assim, ob_lat, ob_lon, ob_hw)
    P = len(ym)
    yam, Yap = np.array(ym), np.array(Yp)
    for j in range(P):
        if sto["n_local"][j]:
            a, b = _etkf.etkf_apply(ym[j:j + 1], Yp[j:j + 1], To[j], wo[j])
            yam[j], Yap[j] = a[0], b[0]
    a = np.asarray(assim, dtype=bool)
    diag = dict(prior_mean=np.array(ym), prior_var=np.var(Yp, axis=1) if P else np.zeros(0), post_mean=np.where(a, yam, np.nan),
                post_var=np.where(a, np.var(Yap, axis=1), np.nan) if P else np.zeros(0), assimilated=a)
    return dict(post=post, ym=yam, Yp=Yap, diag=diag, stats=st, T=Tc, w=wc, rho=rho, prior_ym=ym, prior_Yp=Yp)


def make_case(M, P, ny, nx, n_lead, seed=0, hw=(300.0, 3000.0), frac_off=0.1):
    """The seeded case of DESIGN.md 7y: columns on linspace(25, 55, ny) x linspace(230, 290, nx), obs uniform in lat 20..60,
    lon 225..295, half-widths uniform in hw km, r in 0.5..2, about frac_off of the obs unflagged, HX amplitude
    min(1, 20 sqrt(M/P))."""
    rng = np.random.default_rng(100000 * M + 100 * P + ny * nx + seed)
    lat, lon = np.meshgrid(np.linspace(25.0, 55.0, ny), np.linspace(230.0, 290.0, nx), indexing="ij")
    ncol = ny * nx
    X = rng.standard_normal((n_lead * ncol, M)) * 2.0 + rng.standard_normal((n_lead * ncol, 1))
    amp = min(1.0, 20.0 * np.sqrt(M / float(max(P, 1))))
    HX = amp * rng.standard_normal((P, M)) + rng.standard_normal((P, 1))
    err = rng.uniform(0.5, 2.0, P)
    assim = rng.random(P) >= frac_off
    if P and not assim.any():
        assim[0] = True
    value = HX.mean(axis=1) + np.sqrt(err) * rng.standard_normal(P) if P else np.zeros(0)
    return dict(X=X, HX=HX, value=value, error=err, assim=assim, M=M, P=P, ny=ny, nx=nx, n_lead=n_lead, ncol=ncol,
                grid_lat=lat, grid_lon=lon, ob_lat=rng.uniform(20.0, 60.0, P), ob_lon=rng.uniform(225.0, 295.0, P),
                ob_hw=rng.uniform(hw[0], hw[1], P))
