"""The batch observation-space solver (ETKF) in NumPy, for the tests.

Over the obs with an effective flag a_k = 1: s_k = 1/sqrt(r_k), Y~_k = s_k Yp[k,:], d~_k = s_k (value_k - ym_k);
C = Y~^T Y~, g = Y~^T d~, q = d~^T d~; A = (M-1) I + C = V diag(mu) V^T; T = V diag(sqrt((M-1)/mu)) V^T (the symmetric square
root), w = V diag(1/mu) V^T g; every row, state and obs block alike: xam = xbm + Xbp w, Xap = Xbp T.
Yp is used as handed in (not re-centred).  The effective flags are the caller's, or tests/_outlier.py's mask applied to them."""
import numpy as np


def _scaled(ym, Yp, value, error, assim):
    a = np.asarray(assim, dtype=bool)
    ym = np.asarray(ym, dtype=np.float64)
    Yp = np.asarray(Yp, dtype=np.float64)
    s = 1.0 / np.sqrt(np.asarray(error, dtype=np.float64)[a])
    Yt = s[:, None] * Yp[a]
    dt = s * (np.asarray(value, dtype=np.float64)[a] - ym[a])
    return Yt, dt


def _stats(M, mu, g, w, q, n_active):
    lam = np.sort(mu - (M - 1.0))[::-1]
    return dict(eigenvalues=lam, mu=np.sort(mu)[::-1], n_active=int(n_active), q=float(q),
                dfs=float(np.sum(lam / (M - 1.0 + lam))), chi2=float(q - g @ w))


def etkf_solution(ym, Yp, value, error, assim):
    """T (M, M), w (M,) and the extras, through numpy.linalg.eigh of A."""
    Yt, dt = _scaled(ym, Yp, value, error, assim)
    M = np.asarray(Yp).shape[1]
    C = Yt.T @ Yt
    g = Yt.T @ dt
    q = dt @ dt
    A = (M - 1.0) * np.eye(M) + C
    mu, V = np.linalg.eigh(A)
    T = (V * np.sqrt((M - 1.0) / mu)) @ V.T
    w = (V / mu) @ (V.T @ g)
    out = dict(T=T, w=w, A=A, g=g, cond=float(mu.max() / mu.min()))
    out.update(_stats(M, mu, g, w, q, Yt.shape[0]))
    return out


def etkf_solution_svd(ym, Yp, value, error, assim):
    """The same T and w by another route: the SVD of Y~ for the spectrum of C, numpy.linalg.solve for w."""
    Yt, dt = _scaled(ym, Yp, value, error, assim)
    M = np.asarray(Yp).shape[1]
    if Yt.shape[0] == 0:
        return dict(T=np.eye(M), w=np.zeros(M))
    _, sv, Vt = np.linalg.svd(Yt, full_matrices=True)      # Vt (M, M): right singular vectors, the eigenvectors of C
    lam = np.zeros(M)
    lam[:sv.size] = sv ** 2
    T = (Vt.T * np.sqrt((M - 1.0) / (M - 1.0 + lam))) @ Vt
    w = np.linalg.solve((M - 1.0) * np.eye(M) + Yt.T @ Yt, Yt.T @ dt)
    return dict(T=T, w=w)


def etkf_apply(xm, Xp, T, w):
    """(xam, Xap) of perturbation rows Xp (rows, M) with means xm (rows,)."""
    Xp = np.asarray(Xp, dtype=np.float64)
    return np.asarray(xm, dtype=np.float64) + Xp @ w, Xp @ T


def etkf_members(X, T, w):
    """Posterior members of member rows X (rows, M): mean' + (X - mean) [T | w]."""
    X = np.asarray(X, dtype=np.float64)
    xm = X.mean(axis=1)
    xam, Xap = etkf_apply(xm, X - xm[:, None], T, w)
    return xam[:, None] + Xap


def etkf_diagnostics(ym, Yp, assim, T, w):
    """The five per-ob diagnostics: prior_mean / prior_var (ddof 0) of every ob from the prior, post_mean / post_var (ddof 0) of
    the mapped obs rows (NaN where the ob is not assimilated), assimilated."""
    a = np.asarray(assim, dtype=bool)
    yam, Yap = etkf_apply(ym, Yp, T, w)
    return dict(prior_mean=np.asarray(ym, dtype=np.float64).copy(), prior_var=np.var(np.asarray(Yp, dtype=np.float64), axis=1),
                post_mean=np.where(a, yam, np.nan), post_var=np.where(a, np.var(Yap, axis=1), np.nan), assimilated=a,
                post_ym=yam, post_Yp=Yap)


def serial_consistent(xbm, Xbp, nstate, value, error, assim):
    """The reference's serial loop (ensrf.py:50-149, no localisation) on the augmented arrays with /(M-1) THROUGHOUT -- in the
    gain's denominator (where the reference has np.var, /M) as in its numerator: an exact Kalman update, ob by ob."""
    xam = np.array(xbm, dtype=np.float64)
    Xap = np.array(Xbp, dtype=np.float64)
    M = Xap.shape[1]
    for k in range(len(value)):
        if not assim[k]:
            continue
        i = nstate + k
        ye = Xap[i].copy()
        mye = xam[i]
        varye = ye @ ye / (M - 1.0)
        innov = value[k] - mye
        kcov = Xap @ ye / (M - 1.0)
        kmat = kcov / (varye + error[k])
        beta = 1.0 / (1.0 + np.sqrt(error[k] / (varye + error[k])))
        xam = xam + kmat * innov
        Xap = Xap - beta * np.outer(kmat, ye)
    return xam, Xap


def make_case(M, P, N=5000, seed=0, frac_off=0.1):
    """A seeded case: state members X (N, M), obs estimates HX (P, M) -- so the obs rows of compute_ob_priors are centred --
    values, error variances r in [0.5, 2], and about frac_off of the obs unflagged.  The spread of HX is scaled down with P/M so
    that cond(A) stays <= 1e4 (asserted by the caller from the model)."""
    rng = np.random.default_rng(1000 * M + P + seed)
    X = rng.standard_normal((N, M)) * 2.0 + rng.standard_normal((N, 1))
    amp = min(1.0, 20.0 * np.sqrt(M / float(max(P, 1))))
    HX = amp * rng.standard_normal((P, M)) + rng.standard_normal((P, 1))
    err = rng.uniform(0.5, 2.0, P)
    assim = rng.random(P) >= frac_off
    if P and not assim.any():
        assim[0] = True
    value = HX.mean(axis=1) + np.sqrt(err) * rng.standard_normal(P)
    return dict(X=X, HX=HX, value=value, error=err, assim=assim, M=M, P=P, N=N)


def ob_priors(HX):
    """(ym, Yp) as assimilation.py:46-48 forms them."""
    HX = np.asarray(HX, dtype=np.float64)
    ym = HX.mean(axis=1)
    return ym, HX - ym[:, None]
