"""The LETKF with cross validation (Buehner 2020) in NumPy, for the tests: written from the definition.

Per solve point x (a column, a node of the weight_stride mesh, an ob's own position), with C = sum_k (rho_k/r_k) Y_k^T Y_k and
g = sum_k (rho_k/r_k) d_k Y_k^T over tests/_letkf.py's tapers and flags, and a label group[m] in 0..K-1 per member:
  mean      w = ((M-1) I + C)^-1 g, as the plain filter's
  group k   I = members with another label (ascending), H = those with label k, m = |I|, a = m - 1, J = I_m - 1 1^T / m,
            a I + J C[I,I] J = V diag(mu) V^T,  G_k = V diag(1 / (mu (1 + sqrt(a/mu)))) V^T,
            T[I,H] = -J G_k J C[I,H],  T[H,H] = identity
  recentre  T <- T - (T 1 / M) 1^T: the rows of T sum to zero, so do the posterior perturbations X' T
  apply     mean += X' w, X' <- X' T
A point no ob reaches keeps the pair (I, 0).  `transform_by_subfilter` is the second route to T[I,H]: tests/_letkf.py's own model run
on the sub-ensemble I alone.  Every eigen-decomposition asserts cond <= COND_CAP, a condition on the inputs as in the family."""
import numpy as np

import _etkf
import _letkf
import _letkf_interp as li

COND_CAP = 1e4


def labels(spec, M):
    """The labels (M,) of cross_validation=spec: an int K >= 2 is m % K, an integer array (M,) the labels themselves.  ValueError
    for anything else and for labels that break the rules (every label 0..K-1 used, every independent set of >= 2 members)."""
    if isinstance(spec, (bool, np.bool_)):
        raise ValueError("cross_validation")
    if isinstance(spec, (int, np.integer)):
        if spec < 2 or spec > M:
            raise ValueError("cross_validation")
        g = np.arange(M, dtype=np.int64) % int(spec)
    else:
        g = np.asarray(spec)
        if g.ndim != 1 or g.shape[0] != M or not np.issubdtype(g.dtype, np.integer):
            raise ValueError("cross_validation")
        g = g.astype(np.int64)
    K = int(g.max()) + 1 if g.size else 0
    if g.size == 0 or g.min() < 0 or K < 2 or np.unique(g).size != K:
        raise ValueError("cross_validation")
    if M - np.bincount(g, minlength=K).max() < 2:
        raise ValueError("cross_validation")
    return g


def _sets(group):
    group = np.asarray(group)
    for k in range(int(group.max()) + 1):
        yield np.flatnonzero(group != k), np.flatnonzero(group == k)


def transform(C, group, info=None):
    """T (M, M) of step 2, not recentred.  info: a dict that receives cond (K,), the sub-solves' max mu / min mu."""
    M = C.shape[0]
    T = np.zeros((M, M))
    conds = []
    for I, H in _sets(group):
        m = I.size
        a = m - 1.0
        J = np.eye(m) - 1.0 / m
        B = J @ C[np.ix_(I, I)] @ J
        mu, V = np.linalg.eigh(a * np.eye(m) + 0.5 * (B + B.T))
        conds.append(mu.max() / mu.min())
        assert conds[-1] <= COND_CAP, "sub-solve cond %g" % conds[-1]
        G = (V / (mu * (1.0 + np.sqrt(a / mu)))) @ V.T
        T[np.ix_(I, H)] = -J @ G @ J @ C[np.ix_(I, H)]
        T[np.ix_(H, H)] = np.eye(H.size)
    if info is not None:
        info["cond"] = np.array(conds)
    return T


def transform_by_subfilter(rho_x, ym, Yp, value, error, assim, group, form="solve"):
    """The same T by the second route: for every group tests/_letkf.py's solve on the sub-ensemble I alone, its perturbations
    re-centred on their own mean, gives the symmetric transform W_I = V diag(sqrt(a/mu)) V^T, and
        T[I,H] = -J (I - W_I) (J C[I,I] J)^+ J C[I,H]                                     (form "pinv")
    wherever gamma = mu - a is not small.  On the range of B = J C[I,I] J, in which every column of J C[I,H] lies,
    (I - W_I) B^+ = W_I^2 (I + W_I)^-1 / a (per eigenvalue: (1 - w)/gamma = (w^2/a)/(1 + w), w^2 = a/mu), which needs no
    pseudo-inverse and holds for small gamma as well                                       (form "solve", the default)."""
    Yp = np.asarray(Yp, dtype=np.float64)
    M = Yp.shape[1]
    use = np.asarray(assim, dtype=bool) & (rho_x != 0.0)
    wt = rho_x[use] / np.asarray(error, dtype=np.float64)[use]
    C = Yp[use].T @ (wt[:, None] * Yp[use])
    T = np.zeros((M, M))
    for I, H in _sets(group):
        m = I.size
        J = np.eye(m) - 1.0 / m
        sub = Yp[:, I] @ J                                   # the independent members about their own mean
        W, _, ex = _letkf.solve_point(rho_x, ym, sub, value, error, assim)
        assert ex["cond"] <= COND_CAP
        if form == "pinv":
            B = ex["A"] - (m - 1.0) * np.eye(m)              # = J C[I,I] J
            G = (np.eye(m) - W) @ np.linalg.pinv(B, rcond=1e-12, hermitian=True)
        else:
            G = np.linalg.solve(np.eye(m) + W, W @ W) / (m - 1.0)
        T[np.ix_(I, H)] = -J @ G @ J @ C[np.ix_(I, H)]
        T[np.ix_(H, H)] = np.eye(H.size)
    return T


def recentre(T):
    return T - T.mean(axis=1, keepdims=True)


def solve_point(rho_x, ym, Yp, value, error, assim, group):
    """(T, w, extras) at one location: the plain model's w and statistics, the cross-validated and recentred T."""
    Tp, w, ex = _letkf.solve_point(rho_x, ym, Yp, value, error, assim)
    M = Tp.shape[0]
    ex = dict(ex, cv_cond=0.0, T_plain=Tp)
    if ex["n_local"] == 0:
        return np.eye(M), w, ex
    assert ex["cond"] <= COND_CAP, "cond(A) %g" % ex["cond"]
    info = {}
    T = recentre(transform(ex["A"] - (M - 1.0) * np.eye(M), group, info))
    ex["cv_cond"] = float(info["cond"].max())
    return T, w, ex


def weights(pt_lat, pt_lon, ym, Yp, value, error, assim, ob_lat, ob_lon, ob_hw, group):
    """T (npts, M, M), w (npts, M), stats (n_local, dfs, cond, cv_cond per point) and the tapers."""
    rho = _letkf.taper(pt_lat, pt_lon, ob_lat, ob_lon, ob_hw, assim)
    M = np.asarray(Yp).shape[1]
    n = rho.shape[0]
    T, w = np.empty((n, M, M)), np.empty((n, M))
    st = dict(n_local=np.zeros(n, dtype=np.int64), dfs=np.zeros(n), cond=np.ones(n), cv_cond=np.zeros(n))
    for i in range(n):
        T[i], w[i], ex = solve_point(rho[i], ym, Yp, value, error, assim, group)
        for key in st:
            st[key][i] = ex[key]
    return T, w, st, rho


def cv_cycle(c, group, stride=None, assim=None, rtpp=None):
    """The whole cycle of a seeded case c (tests/_letkf.py's make_case): posterior members, the posterior obs block, the diagnostics,
    the solve points' pairs and statistics (the columns', or with a stride the nodes')."""
    a = np.asarray(c["assim"] if assim is None else assim, dtype=bool)
    X = np.asarray(c["X"], dtype=np.float64)
    HX = np.asarray(c["HX"], dtype=np.float64)
    ym, Yp = _etkf.ob_priors(HX)
    ny, nx, n_lead = c["ny"], c["nx"], c["n_lead"]
    args = (ym, Yp, c["value"], c["error"], a, c["ob_lat"], c["ob_lon"], c["ob_hw"], group)
    glat, glon = np.asarray(c["grid_lat"], dtype=np.float64).reshape(-1), np.asarray(c["grid_lon"], dtype=np.float64).reshape(-1)
    m = li.mesh(ny, nx, (1, 1) if stride is None else stride)
    Tn, wn, st, rho = weights(glat[m["node_col"]], glon[m["node_col"]], *args)
    Tc, wc, reached = li.column_pairs(m, Tn, wn, st["n_local"])
    post = li.apply_pairs(X, ny * nx, n_lead, Tc, wc, reached, rtpp=rtpp)
    To, wo, sto, _ = weights(c["ob_lat"], c["ob_lon"], *args)
    yam, Yap = np.array(ym), np.array(Yp)
    for j in range(len(ym)):
        if sto["n_local"][j]:
            yam[j], Yap[j] = ym[j] + Yp[j] @ wo[j], Yp[j] @ To[j]
    diag = dict(prior_mean=np.array(ym), prior_var=np.var(Yp, axis=1), post_mean=np.where(a, yam, np.nan),
                post_var=np.where(a, np.var(Yap, axis=1), np.nan), assimilated=a)
    return dict(post=post, ym=yam, Yp=Yap, diag=diag, stats=st, T=Tn, w=wn, rho=rho, reached=reached, ob_stats=sto, mesh=m)


def permuted_labels(M, K, seed):
    """Labels from a seeded permutation: group sizes as m % K has them, members scattered."""
    return np.random.default_rng(seed).permutation(np.arange(M, dtype=np.int64) % K)


# the parity cases of DESIGN.md 7y-9: (M, K, P, ny, nx, n_lead); the last one takes its labels from permuted_labels(M, K, 5)
CASES = [
    (4, 2, 3, 3, 5, 2),
    (6, 3, 5, 3, 5, 2),
    (16, 4, 64, 5, 7, 3),
    (17, 4, 33, 5, 7, 17),
    (31, 5, 64, 4, 5, 2),
    (40, 8, 400, 6, 7, 3),
    (80, 4, 700, 6, 7, 2),
    (136, 2, 300, 3, 6, 1),
    (136, 4, 300, 3, 6, 1),
    (12, 12, 20, 3, 4, 1),
]
PERMUTED = (20, 3, 48, 4, 5, 2)


def make_case(M, K, P, ny, nx, n_lead, permuted=False):
    c = _letkf.make_case(M, P, ny, nx, n_lead, seed=0)
    return c, (permuted_labels(M, K, 5) if permuted else np.arange(M, dtype=np.int64) % K)
