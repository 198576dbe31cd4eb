"""NumPy test oracle of the observation impact (EFSO).  For every ob k with used[k]

    J_k = (1/(M-1)) (d_k / r_k) sum_i rho_ik v_i (Xf'_i . Ya'_k)

Xf' / Ya' the row-mean-removed perturbations of Xf (rows, M) / Ya (P, M), and J_k = 0.0 for every other ob.  rho_ik is 1 without
localisation; with it, for state row i = slab * ncol + column, the oracle's `localize_state` taper of (column, ob k) times -- for
an ob with vertical information -- `_vertloc.vertical_factor` of (slab, ob k) (1 on a NaN slab).  The taper is not advected.
Also returned: A_k, the same sum with every one of its rows * M terms replaced by its absolute value -- the scale of the rounding
error of J_k, a sum with heavy cancellation."""
import numpy as np

from _vertloc import vertical_factor
from oracle.ensrf_oracle import localize_state


def efso(Xf, Ya, v, d, r, used, grid_lat=None, grid_lon=None, ob_lat=None, ob_lon=None, ob_halfwidth=None, n_lead=1,
         lead_vert=None, ob_vert=None, ob_vert_halfwidth=None):
    """grid_lat None: unlocalised.  Else grid_lat / grid_lon (ncol,) with rows == n_lead * ncol, and optionally lead_vert
    (n_lead,), ob_vert / ob_vert_halfwidth (P,), NaN where missing.  Returns (J, A), both (P,)."""
    Xf = np.asarray(Xf, dtype=np.float64)
    Ya = np.asarray(Ya, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    rows, M = Xf.shape
    P = Ya.shape[0]
    Xp = Xf - Xf.mean(axis=1, keepdims=True)
    Yp = Ya - Ya.mean(axis=1, keepdims=True)
    aXp = np.abs(Xp)
    J = np.zeros(P)
    A = np.zeros(P)
    if grid_lat is not None:
        grid_lat = np.asarray(grid_lat, dtype=np.float64).reshape(-1)
        grid_lon = np.asarray(grid_lon, dtype=np.float64).reshape(-1)
        assert rows == n_lead * grid_lat.size
        lv = np.full(n_lead, np.nan) if lead_vert is None else np.asarray(lead_vert, dtype=np.float64).reshape(-1)
        ov = np.full(P, np.nan) if ob_vert is None else np.asarray(ob_vert, dtype=np.float64)
        oc = np.full(P, np.nan) if ob_vert_halfwidth is None else np.asarray(ob_vert_halfwidth, dtype=np.float64)
    for k in range(P):
        if not used[k]:
            continue
        rho = 1.0
        if grid_lat is not None:
            sl = localize_state(grid_lat, grid_lon, ob_lat[k], ob_lon[k], ob_halfwidth[k])
            rho = np.tile(sl, n_lead)
            if not (np.isnan(ov[k]) or np.isnan(oc[k])):
                rho = rho * np.repeat(vertical_factor(lv, ov[k], oc[k]), grid_lat.size)
        pref = (1.0 / (M - 1)) * (d[k] / r[k])
        J[k] = pref * np.sum(rho * v * np.dot(Xp, Yp[k]))
        A[k] = abs(pref) * np.sum(rho * np.abs(v) * np.dot(aXp, np.abs(Yp[k])))
    return J, A


def tolerance(rows, M):
    """|J_k - ref_k| <= tolerance * A_k: the worst-case forward bound of a float64 sum of rows * M terms in any order."""
    return max(1e-9, 4.0 * rows * M * 2.0 ** -53)
