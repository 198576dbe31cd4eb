"""NumPy restatement of DESIGN.md 7c (Anderson 2009 spatially varying adaptive inflation): the test oracle.

Vectorised over state rows, serial over observations.  The serial ob records and the posterior come from
`oracle.ensrf_oracle` (obs_taper="vector"): a step hook sees the augmented arrays BEFORE each ob updates them and applies
the per-row update with them.  The formulas are written as DESIGN.md 7c states them; the kernels evaluate algebraically
equal forms with fewer square roots and divides (efa_gcsweep.hip, anderson_update), so the two agree to rounding.
"""
import numpy as np

from oracle import ensrf_oracle as orc

LOG_099 = np.log(0.99)


def inflate(X, lam):
    """x_im <- mean_i + sqrt(lam_i) (x_im - mean_i); rows with lam == 1 unchanged."""
    X = np.asarray(X, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    mean = X.mean(axis=1, keepdims=True)
    return np.where((lam == 1.0)[:, None], X, mean + np.sqrt(lam)[:, None] * (X - mean))


def update(lam, sd, w, dot, ss, yy, d2, sp2, so2, lower=1.0, upper=1e6, sd_lower=0.0):
    """One ob's update of the rows' (lam, sd): arrays over rows (w, dot, ss, lam, sd) and the ob's scalars."""
    lam = np.asarray(lam, dtype=np.float64)
    sd = np.asarray(sd, dtype=np.float64)
    nn = np.asarray(ss, dtype=np.float64) * yy
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(nn > 0.0, dot / np.sqrt(np.where(nn > 0.0, nn, 1.0)), 0.0)
        gamma = np.minimum(1.0, w * np.abs(r))
        act = (gamma > 0.0) & (sd > 0.0)
        lam_s = np.where(act, lam, 1.0)
        sd_s = np.where(act, sd, 1.0)
        rl = np.sqrt(lam_s)
        q = 1.0 + gamma * (rl - 1.0)
        th2 = q * q * sp2 + so2
        th = np.sqrt(th2)
        dth = sp2 * gamma * q / (2.0 * th * rl)
        g = (dth / th) * (d2 / th2 - 1.0)
        s2 = sd_s * sd_s
        ln = lam_s + 2.0 * s2 * g / (1.0 + np.sqrt(1.0 + 4.0 * s2 * (g * g)))
        ln = np.minimum(np.maximum(ln, lower), upper)
        q0 = 1.0 + gamma * (np.sqrt(ln) - 1.0)
        q1 = 1.0 + gamma * (np.sqrt(ln + sd_s) - 1.0)
        t0 = q0 * q0 * sp2 + so2
        t1 = q1 * q1 * sp2 + so2
        a0 = ln - lam_s
        a1 = (ln + sd_s) - lam_s
        e0 = -(a0 * a0) / (2.0 * s2) - d2 / (2.0 * t0)
        e1 = -(a1 * a1) / (2.0 * s2) - d2 / (2.0 * t1)
        ell = (e1 - e0) + 0.5 * np.log(t0 / t1)
        shrink = (sd_s > sd_lower) & (ell < LOG_099)
        sd_new = np.where(shrink, np.minimum(np.maximum(np.sqrt(-s2 / (2.0 * np.where(shrink, ell, -1.0))), sd_lower), sd_s), sd_s)
    return np.where(act, ln, lam), np.where(act, sd_new, sd)


def state_taper(grid_lat, grid_lon, state_shape, ob_lat, ob_lon, hw):
    """The GC taper of one ob on every state row (ensrf.py:108-111: per column, broadcast over variable x time)."""
    sl = orc.localize_state(np.asarray(grid_lat, dtype=np.float64), np.asarray(grid_lon, dtype=np.float64), ob_lat, ob_lon, hw)
    nvar, nt, ny, nx = state_shape
    return np.broadcast_to(sl.reshape(-1)[None, :], (nvar * nt, ny * nx)).reshape(-1) if sl.ndim == 2 else \
        np.broadcast_to(np.tile(sl, ny)[None, :], (nvar * nt, ny * nx)).reshape(-1)


def cycle(X, H, ob_value, ob_error, ob_assim, ob_lat, ob_lon, hw, grid_lat, grid_lon, state_shape, field,
          lower=1.0, upper=1e6, sd_lower=0.0, prior_inflated=False):
    """One adaptive cycle on prior members X (N, M) with the field (N, 2) and a linear forward operator H (P, N) (dense or
    a callable on member rows): the prior is inflated, HX taken from the inflated prior, the serial EnSRF run and the field
    updated ob by ob (prior_inflated: X is inflated already, the step is skipped).  Returns (posterior members, new field,
    diagnostics, inflated prior)."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    field = np.asarray(field, dtype=np.float64)
    Xi = X if prior_inflated else inflate(X, field[:, 0])
    HX = H(Xi) if callable(H) else np.asarray(H) @ Xi
    lam = field[:, 0].copy()
    sd = field[:, 1].copy()

    def hook(k, xam, Xap):
        nonlocal lam, sd
        if not ob_assim[k]:
            return
        ye = Xap[N + k]
        Xs = Xap[:N]
        w = state_taper(grid_lat, grid_lon, state_shape, ob_lat[k], ob_lon[k], hw[k])
        lam, sd = update(lam, sd, w, Xs @ ye, np.einsum("ij,ij->i", Xs, Xs), float(ye @ ye),
                         (ob_value[k] - xam[N + k]) ** 2, np.var(ye), ob_error[k], lower, upper, sd_lower)

    post, _, _, diag = orc.ensrf_cycle(Xi, HX, ob_value, ob_error, ob_assim, loc="GC", ob_lat=ob_lat, ob_lon=ob_lon,
                                       ob_halfwidth=hw, grid_lat=grid_lat, grid_lon=grid_lon, state_shape=state_shape,
                                       obs_taper="vector", step_hook=hook)
    return post, np.stack([lam, sd], axis=1), diag, Xi
