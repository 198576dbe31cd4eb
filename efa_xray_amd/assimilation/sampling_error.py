"""Sampling error correction of the EnSRF gain (Anderson 2012): the default table and the keyword's checks.

The gain of an observation on a state row is damped by a factor alpha(|r|; M) of the SAMPLE correlation r of the row and the
observation: a regression estimated from M members is, on average, too large where the true correlation is small.  The factor is
a table over |r| in [0, 1], node j at |r| = j/(T-1), read piecewise linearly on the device.
"""
import numpy as np

MAX_NODES = 512          # kSecMaxT of the library: the sweep stages the table in 4 KB of LDS
DEFAULT_NODES = 201

_cache = {}


def sampling_error_table(M, T=DEFAULT_NODES):
    """The default table for M members: float64 [T], node j at r_j = j/(T-1).

    For 0 < r_j < 1 the least-squares factor E[rho | r_j] / r_j under a uniform prior on the true correlation rho in (-1, 1),

        alpha_j = int rho f(r_j | rho) drho / (r_j int f(r_j | rho) drho),

    with Fisher's exact density of the sample correlation of M pairs,

        f(r | rho) ~ (1 - rho^2)^((M-1)/2) (1 - r^2)^((M-4)/2) int_0^inf dw (cosh w - rho r)^-(M-1);

    alpha_{T-1} = 1 and alpha_0 = alpha_1.  NumPy quadrature only, deterministic, cached per (M, T).

    The inner integral is taken in the variable theta with cosh w = 1 + (1 - c) tan^2(theta), c = rho r, in which it is

        (1 - c)^(3/2 - M) int_0^(pi/2) 2 cos^(2M-4)(theta) / sqrt(2 + (1 - c) tan^2(theta)) dtheta

    -- a smooth integrand on a finite interval for every c < 1 (Gauss-Legendre, 96 nodes) -- and the outer one in Fisher's
    z = artanh(rho), in which the weight is close to a normal of width (M - 3)^(-1/2) wherever its mode lies (midpoint rule,
    |z| <= 12); the weights are formed in logarithms, so 256 members neither overflow nor underflow.
    """
    if isinstance(M, bool) or int(M) != M or M < 2:
        raise ValueError("sampling_error_table: M=%r must be an integer >= 2" % (M,))
    if isinstance(T, bool) or int(T) != T or not 2 <= T <= MAX_NODES:
        raise ValueError("sampling_error_table: T=%r must be an integer in [2, %d]" % (T, MAX_NODES))
    M, T = int(M), int(T)
    key = (M, T)
    if key not in _cache:
        alpha = np.ones(T)
        if T > 2:
            xg, wg = np.polynomial.legendre.leggauss(96)
            theta = 0.25 * np.pi * (xg + 1.0)
            wth = 0.25 * np.pi * wg * 2.0 * np.cos(theta) ** (2 * M - 4)
            tan2 = np.tan(theta) ** 2
            nz = 2400
            z = (np.arange(nz) + 0.5) * (24.0 / nz) - 12.0
            rho = np.tanh(z)
            lcosh = np.logaddexp(z, -z) - np.log(2.0)                  # log cosh z
            lprior = -(M - 1) * lcosh - 2.0 * lcosh                    # (1 - rho^2)^((M-1)/2) drho/dz
            for j in range(1, T - 1):
                r = j / (T - 1.0)
                omc = 1.0 - rho * r                                     # 1 - c, > 0
                inner = (wth[None, :] / np.sqrt(2.0 + omc[:, None] * tan2[None, :])).sum(axis=1)
                lw = lprior + (1.5 - M) * np.log(omc) + np.log(inner)
                w = np.exp(lw - lw.max())
                alpha[j] = (rho * w).sum() / (r * w.sum())
            alpha[0] = alpha[1]
        alpha.setflags(write=False)
        _cache[key] = alpha
    return _cache[key].copy()


def check_table(alpha):
    """`alpha` as a float64 [T] table the library accepts; ValueError otherwise."""
    try:
        a = np.array(alpha, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("sampling_error_correction: expected True or a table of factors, got %r" % type(alpha).__name__)
    if a.ndim != 1 or not 2 <= a.size <= MAX_NODES:
        raise ValueError("sampling_error_correction: the table must be one-dimensional with 2 to %d nodes, got shape %r"
                         % (MAX_NODES, a.shape))
    if not (np.isfinite(a).all() and (a >= 0.0).all()):
        raise ValueError("sampling_error_correction: every factor must be a finite number >= 0")
    return np.ascontiguousarray(a)


def sec_setting(value, M, loc, adaptive=None, vert_coord=None, slab=None, streamed=False):
    """The table of the `sampling_error_correction` keyword as a float64 array, or None when off (None / False); True gives
    the default table for M members.  ValueError on a bad table and on a setting it cannot be combined with."""
    if value is None or value is False:
        return None
    if loc != 'GC':
        raise ValueError("sampling_error_correction needs loc='GC' (the factor multiplies the localised gain); got loc=%r" % (loc,))
    if adaptive is not None:
        raise ValueError("sampling_error_correction cannot be combined with adaptive_inflation (not supported, DESIGN.md 7w)")
    if vert_coord is not None:
        raise ValueError("sampling_error_correction cannot be combined with vert_coord (not supported, DESIGN.md 7w)")
    if slab is not None:
        raise ValueError("sampling_error_correction cannot be combined with time_localize / var_impact (not supported, DESIGN.md 7w)")
    if streamed:
        raise ValueError("sampling_error_correction cannot be combined with streamed=True (not supported, DESIGN.md 7w)")
    if value is True:
        return sampling_error_table(M)
    return check_table(value)
