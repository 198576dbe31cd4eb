"""The outlier (gross-error) check of DESIGN.md 7e in NumPy, for the tests: which requested observations a threshold rejects,
and the seeded gross errors the tests inject.  The filter itself is the oracle (oracle/ensrf_oracle.py) run on the flags this
mask leaves."""
import numpy as np
from oracle import ensrf_oracle as orc


def outlier_mask(ym, Yp, value, error, assim, t):
    """True where a requested ob is REJECTED by threshold t > 0: with d = value - ym, s2 = np.var(Yp[k]) (ddof 0, the
    reference's varye) and r = error (the variance), an ob is kept iff d^2 <= t^2 (s2 + r); a NaN anywhere rejects it.
    Obs not requested (assim 0) are never rejected.  ym, Yp as compute_ob_priors returns them (after any prior inflation)."""
    ym = np.asarray(ym, dtype=np.float64)
    Yp = np.asarray(Yp, dtype=np.float64)
    d = np.asarray(value, dtype=np.float64) - ym
    s2 = np.var(Yp, axis=1)
    r = np.asarray(error, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        keep = d ** 2 <= t ** 2 * (s2 + r)
    return np.asarray(assim, dtype=bool) & ~keep


def ratio(ym, Yp, value, error):
    """|d| / sqrt(s2 + r) of every ob: compared with t by the check."""
    d = np.asarray(value, dtype=np.float64) - np.asarray(ym, dtype=np.float64)
    return np.abs(d) / np.sqrt(np.var(np.asarray(Yp, dtype=np.float64), axis=1) + np.asarray(error, dtype=np.float64))


def masked_flags(HX, value, error, assim, t):
    """The flags the check leaves for obs estimates HX (P, M): requested and not rejected."""
    ym, Yp = orc.compute_ob_priors(HX)
    return np.asarray(assim, dtype=bool) & ~outlier_mask(ym, Yp, value, error, assim, t)


def inject(HX, value, error, assim, t, n, seed=0, margin=5.0):
    """value with n requested obs moved to ym +- (t + margin) sqrt(s2 + r) (a gross error each); returns (value, their index)."""
    rng = np.random.default_rng(seed)
    ym, Yp = orc.compute_ob_priors(HX)
    value = np.array(value, dtype=np.float64)
    req = np.flatnonzero(np.asarray(assim, dtype=bool))
    idx = np.sort(rng.choice(req, size=min(n, req.size), replace=False))
    sign = np.where(rng.random(idx.size) < 0.5, -1.0, 1.0)
    value[idx] = ym[idx] + sign * (t + margin) * np.sqrt(np.var(Yp[idx], axis=1) + np.asarray(error, dtype=np.float64)[idx])
    return value, idx


def clear_of_threshold(ym, Yp, value, error, t, rel=1e-6):
    """Every ob's ratio at least `rel` (relative) away from t: the device's variance may differ from NumPy's in the last bits."""
    q = ratio(ym, Yp, value, error)
    q = q[np.isfinite(q)]
    return bool(np.all(np.abs(q - t) >= rel * t))
