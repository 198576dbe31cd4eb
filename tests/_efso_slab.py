"""NumPy test oracle of the observation impact under the temporal and variable tapers (EFSO): `_efso.efso` with

    rho_ik = GC_h(column, k) * S(k, slab)        for state row i = slab * ncol + column

GC_h the oracle's `localize_state` and S = (V T) C the factor table of `_slabloc.slab_factor_table` -- the vertical factor of 7d, the
temporal taper and the impact of ob k's obtype on the slab's variable, each 1 where its inputs are missing, each product rounded
once in that order.  Returns (J, A) as `_efso.efso` does: A_k is the same sum with every term replaced by its absolute value."""
import numpy as np

from _slabloc import slab_factor_table
from oracle.ensrf_oracle import localize_state


def efso_slab(Xf, Ya, v, d, r, used, grid_lat, grid_lon, ob_lat, ob_lon, ob_halfwidth, n_lead, lead_vert=None, ob_vert=None,
              ob_vert_halfwidth=None, lead_time=None, ob_time=None, ob_time_halfwidth=None, lead_var=None, ob_group=None, impact=None):
    """grid_lat / grid_lon (ncol,) with rows == n_lead * ncol; lead_* (n_lead,), ob_* (P,), NaN (floats) / -1 (ints) where missing,
    None: none; impact [n_group][n_var].  Returns (J, A), both (P,)."""
    Xf = np.asarray(Xf, dtype=np.float64)
    Ya = np.asarray(Ya, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    rows, M = Xf.shape
    P = Ya.shape[0]
    grid_lat = np.asarray(grid_lat, dtype=np.float64).reshape(-1)
    grid_lon = np.asarray(grid_lon, dtype=np.float64).reshape(-1)
    ncol = grid_lat.size
    assert rows == n_lead * ncol
    S = slab_factor_table(n_lead, P, lead_vert, ob_vert, ob_vert_halfwidth, lead_time, ob_time, ob_time_halfwidth, lead_var,
                          ob_group, impact)
    Xp = Xf - Xf.mean(axis=1, keepdims=True)
    Yp = Ya - Ya.mean(axis=1, keepdims=True)
    aXp = np.abs(Xp)
    J = np.zeros(P)
    A = np.zeros(P)
    for k in range(P):
        if not used[k]:
            continue
        rho = np.tile(localize_state(grid_lat, grid_lon, ob_lat[k], ob_lon[k], ob_halfwidth[k]), n_lead) * np.repeat(S[k], ncol)
        pref = (1.0 / (M - 1)) * (d[k] / r[k])
        J[k] = pref * np.sum(rho * v * np.dot(Xp, Yp[k]))
        A[k] = abs(pref) * np.sum(rho * np.abs(v) * np.dot(aXp, np.abs(Yp[k])))
    return J, A
