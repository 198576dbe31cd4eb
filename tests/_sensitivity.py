"""NumPy float64 model of ensemble sensitivity and greedy observation targeting: what efa_sensitivity_dev is compared
with.  Not a test file, and not importable from the product (there is no NumPy path there).

X (rows, M) state members in to_vect() order (rows = n_lead * ncol), J (K, M) metric members, R (n_lead,) the error variance of a
hypothetical observation of a row of each slab, w (K,) weights, cand (rows,) mask.  Every statistic uses 1/(M-1).

Picks t = 0 .. n-1, one after the other, host state G_0 = I (M x M).  For pick t of row i_t with raw deviations y_t = x'_{i_t}:
    u_t = G_t y_t,  d_t = y_t.u_t/(M-1) + R_slab(i_t),  b_tk = J'_k.u_t/(M-1),  G_{t+1} = G_t - u_t u_t^T/((M-1) d_t)
and with a_is = x'_i.u_s/(M-1) the statistics conditioned on picks 0 .. t-1 are
    var_i(t) = max(0, var0_i - sum_s a_is^2/d_s),  cov_ik(t) = cov0_ik - sum_s a_is b_sk/d_s,  varJ_k(t) = varJ0_k - sum_s b_sk^2/d_s
    score_i(t) = sum_k w_k cov_ik(t)^2 / (var_i(t) + R_slab(i)).
The pick is the candidate with the largest score, the lowest row among equals, never a NaN; no candidate with a score > 0: the picks
stop.  A denominator of 0 (or below) gives exactly 0.0.  A row whose members are all equal has deviations of exactly 0."""
import numpy as np


def deviations(X):
    X = np.asarray(X, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = X - X.mean(axis=1, keepdims=True)
    d[np.all(X == X[:, :1], axis=1)] = 0.0
    return d


def safe_div(num, den):
    """num / den where den > 0, NaN where either is NaN, exactly 0.0 elsewhere."""
    num, den = np.broadcast_arrays(np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64))
    out = np.zeros(num.shape)
    ok = den > 0.0
    out[ok] = num[ok] / den[ok]
    bad = np.isnan(den) | np.isnan(num)
    out[bad] = np.nan
    return out


def derived(var, cov, varJ, R_rows, w, cand):
    """sens, corr, dvar, score from var (rows,), cov (K, rows), varJ (K,) by the formulas of the definition."""
    with np.errstate(invalid="ignore", over="ignore"):
        sens = safe_div(cov, var[None, :])
        d2 = var[None, :] * varJ[:, None]      # (a varJ rounded below 0 counts as a zero denominator)
        corr = safe_div(cov, np.where(np.isnan(d2), np.nan, np.sqrt(np.where(d2 > 0.0, d2, 0.0))))
        dvar = -(cov * cov) / (var + R_rows)[None, :]
        score = np.sum(w[:, None] * cov * cov, axis=0) / (var + R_rows)
    score = np.where(cand, score, 0.0)
    return sens, corr, dvar, score


def model(X, J, n_lead, R, w=None, cand=None, n_targets=0):
    X = np.asarray(X, dtype=np.float64)
    J = np.asarray(J, dtype=np.float64)
    rows, M = X.shape
    K = J.shape[0]
    ncol = rows // n_lead
    assert ncol * n_lead == rows
    R = np.asarray(R, dtype=np.float64)
    R_rows = np.repeat(R, ncol)
    w = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    cand = np.ones(rows, dtype=bool) if cand is None else np.asarray(cand).astype(bool)
    Xp, Jp = deviations(X), deviations(J)
    with np.errstate(invalid="ignore", over="ignore"):
        var0 = np.sum(Xp * Xp, axis=1) / (M - 1)
        cov0 = (Jp @ Xp.T) / (M - 1)
    varJ0 = np.sum(Jp * Jp, axis=1) / (M - 1)
    var_raw, cov, varJ = var0.copy(), cov0.copy(), varJ0.copy()
    G = np.eye(M)
    picked_row = np.full(n_targets, -1, dtype=np.int64)
    picked_score = np.zeros(n_targets)
    metric_var = np.tile(varJ0, (n_targets + 1, 1))
    margins = []

    def clamp(v):
        return np.where(v < 0.0, 0.0, v)

    for t in range(n_targets):
        with np.errstate(invalid="ignore", over="ignore"):
            score = np.sum(w[:, None] * cov * cov, axis=0) / (clamp(var_raw) + R_rows)
        s = np.where(cand & ~np.isnan(score), score, -np.inf)
        i = int(np.argmax(s)) if rows else -1      # the first of equals
        if i < 0 or not s[i] > 0.0:
            break
        rest = np.delete(s, i)
        second = float(rest.max()) if rest.size else -np.inf
        margins.append((s[i] - max(second, 0.0)) / s[i])
        y = Xp[i]
        u = G @ y
        d = float(y @ u) / (M - 1) + R_rows[i]
        b = (Jp @ u) / (M - 1)
        G = G - np.outer(u, u) / ((M - 1) * d)
        with np.errstate(invalid="ignore", over="ignore"):
            a = (Xp @ u) / (M - 1)
            var_raw = var_raw - a * a / d
            cov = cov - np.outer(b, a) / d
        varJ = varJ - b * b / d
        picked_row[t], picked_score[t] = i, s[i]
        metric_var[t + 1:] = varJ
    var = clamp(var_raw)
    sens, corr, dvar, score = derived(var, cov, varJ, R_rows, w, cand)
    return dict(var=var, cov=cov, sens=sens, corr=corr, dvar=dvar, score=score, var0=var0, varJ0=varJ0, varJ=varJ, R_rows=R_rows,
                picked_row=picked_row, picked_score=picked_score, metric_var=metric_var, margins=np.array(margins))


def explicit(X, J, n_lead, R, picks):
    """The same conditioning by the explicit update P <- P - P[:, i] P[i, :] / (P_ii + R) of the covariance of the stacked [X; J].
    Returns (var (rows,), cov (K, rows), varJ trajectory (len(picks) + 1, K))."""
    X = np.asarray(X, dtype=np.float64)
    J = np.asarray(J, dtype=np.float64)
    rows, M = X.shape
    R_rows = np.repeat(np.asarray(R, dtype=np.float64), rows // n_lead)
    Z = np.vstack([X, J])
    Zp = Z - Z.mean(axis=1, keepdims=True)
    P = (Zp @ Zp.T) / (M - 1)
    traj = [np.diag(P)[rows:].copy()]
    for i in picks:
        P = P - np.outer(P[:, i], P[i, :]) / (P[i, i] + R_rows[i])
        traj.append(np.diag(P)[rows:].copy())
    return np.diag(P)[:rows].copy(), P[rows:, :rows].copy(), np.array(traj)


def make_case(seed, rows, M, K, n_lead, offset=None):
    """Rows mu_i + sigma_i z with |mu_i| <= 10 sigma_i and sigma from 1e-3 to 1e3 across the rows (offset: every row has mean
    `offset` and spread 1 instead); J partly correlated with a few rows; slab errors of the order of the median row variance."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((rows, M))
    if offset is None:
        sigma = 10.0 ** rng.uniform(-3.0, 3.0, rows)
        mu = rng.uniform(-10.0, 10.0, rows) * sigma
    else:
        sigma = np.ones(rows)
        mu = np.full(rows, float(offset))
    X = mu[:, None] + sigma[:, None] * z
    J = np.empty((K, M))
    for k in range(K):
        src = rng.choice(rows, min(3, rows), replace=False)
        J[k] = rng.uniform(0.5, 2.0, src.size) @ z[src] + 0.7 * rng.standard_normal(M) + rng.uniform(-5.0, 5.0)
    R = rng.uniform(0.5, 2.0, n_lead)
    w = rng.uniform(0.5, 2.0, K)
    return X, J, R, w
