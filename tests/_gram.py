"""NumPy model of efa_gram_dev: the definitions evaluated in numpy.longdouble, and the derived bound of the
float64 result

    |G_ab - model| <= u ((n + 8) S_ab + (M + 6) (A_a + A_b)) / (M - 1),    u = 2^-53,
    S_ab = sum_i c_i |x'_ia| |x'_ib|,    A_a = sum_i c_i mean_m |x_im| |x'_ia|,    n the used, good rows:

an n-term sum of products in any order, and the rounded row mean carried into both factors."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def classes(X, n_lead, scale, w=None):
    """(used, bad, c) per row of X (rows, M), rows = n_lead * ncol, row = lead * ncol + col."""
    rows, M = X.shape
    ncol = rows // n_lead if n_lead else 0
    s = np.repeat(np.asarray(scale, dtype=np.float64), ncol)
    wc = np.ones(ncol) if w is None else np.asarray(w, dtype=np.float64)
    wr = np.tile(wc, n_lead)
    with np.errstate(invalid="ignore"):
        used = (s > 0.0) & (wr > 0.0)
    bad = used & ~(np.all(np.isfinite(X), axis=1) & np.isfinite(wr))
    return used, bad, wr, s


def model(X, n_lead, scale, w=None):
    """dict: G (M, M) longdouble, n, n_bad, sums (2,) longdouble, bound (M, M) float64."""
    X = np.asarray(X)
    rows, M = X.shape
    used, bad, wr, s = classes(X, n_lead, scale, w)
    good = used & ~bad
    Xg = X[good].astype(LD)
    wg, sg = wr[good].astype(LD), s[good].astype(LD)
    c = wg * sg * sg
    n = int(good.sum())
    if n:
        mean = Xg.sum(axis=1) / LD(M)
        xp = Xg - mean[:, None]
        G = (xp * c[:, None]).T @ xp / LD(M - 1)
        ax = np.abs(xp).astype(np.float64)
        cf = c.astype(np.float64)
        S = (ax * cf[:, None]).T @ ax
        mabs = np.mean(np.abs(Xg.astype(np.float64)), axis=1)
        A = (ax * (cf * mabs)[:, None]).sum(axis=0)
    else:
        G = np.zeros((M, M), dtype=LD)
        S = np.zeros((M, M))
        A = np.zeros(M)
    bound = U * ((n + 8) * S + (M + 6) * (A[:, None] + A[None, :])) / (M - 1.0)
    return dict(G=G, n=n, n_bad=int(bad.sum()), sums=np.array([wg.sum(), c.sum()], dtype=LD), bound=bound)


def ratio(G, m):
    """Largest |G - model| / bound; where the bound is 0 the difference must be 0."""
    diff = np.abs(np.asarray(G, dtype=LD) - m["G"]).astype(np.float64)
    b = m["bound"]
    zero = b == 0.0
    assert np.all(diff[zero] == 0.0), "a difference where the bound is 0"
    return float(np.max(diff[~zero] / b[~zero])) if np.any(~zero) else 0.0


def make_rows(seed, rows, M, dtype, offset=None):
    """rows x M members: a common offset (280; 1e6 and 300 test the cancellation) plus N(0, 3) and a per-row signal."""
    rng = np.random.default_rng(seed)
    off = 280.0 if offset is None else offset
    X = off + 3.0 * rng.standard_normal((rows, M)) + rng.standard_normal((rows, 1))
    return np.ascontiguousarray(X.astype(dtype))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)
