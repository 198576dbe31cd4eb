"""NumPy model of efa_verify_dev: the rows sorted one by one, every sum in numpy.longdouble over the once-rounded
d = x - y, the tie-break hash in uint64.  No GPU, no library."""
import numpy as np

U = 2.0 ** -53
MASK = (1 << 64) - 1


def pick(seed, R, equal):
    """The tie-break of global row R: splitmix64, scaled to [0, equal] (Python integers, mod 2^64)."""
    z = (int(seed) + (int(R) + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return ((z >> 32) * (int(equal) + 1)) >> 32


def pick_array(seed, R, equal):
    """The same on arrays, in numpy.uint64 (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        R = np.asarray(R, dtype=np.uint64)
        z = np.uint64(seed) + (R + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return (((z >> np.uint64(32)) * (np.asarray(equal, dtype=np.uint64) + np.uint64(1))) >> np.uint64(32)).astype(np.int64)


def crps_pairwise(d, fair=False):
    """mean|d| - sum_ij |d_i - d_j| / (2 D): the definition, O(M^2), in longdouble."""
    d = np.asarray(d, dtype=np.longdouble)
    M = d.size
    D = M * (M - 1) if fair else M * M
    return float(np.abs(d).sum() / M - np.abs(d[:, None] - d[None, :]).sum() / (2 * D))


def model(X, y, n_lead, slab_group, col_weight=None, fair=False, seed=0, col_offset=0, ncol_total=None):
    """X (rows, M) float64 or float32, y (rows,), slab_group (n_lead,), col_weight (ncol,) or None.  Returns the six fields, hist,
    n, n_bad, sums (G, 5) and, for the tolerances, mean_abs_d (rows,) and abs_sums (G, 5) = sum |w t|."""
    X = np.asarray(X)
    rows, M = X.shape
    ncol = rows // max(n_lead, 1)
    ncol_total = ncol if ncol_total is None else ncol_total
    sg = np.asarray(slab_group, dtype=np.int64)
    G = int(sg.max()) + 1 if sg.size and sg.max() >= 0 else 0
    Xd = X.astype(np.float64)
    y = np.asarray(y, dtype=np.float64)
    below = np.full(rows, -1, dtype=np.int32)
    equal = np.full(rows, -1, dtype=np.int32)
    rank = np.full(rows, -1, dtype=np.int32)
    crps = np.full(rows, np.nan)
    err = np.full(rows, np.nan)
    var = np.full(rows, np.nan)
    mad = np.full(rows, np.nan)
    hist = np.zeros((G, M + 1), dtype=np.int64)
    n = np.zeros(G, dtype=np.int64)
    n_bad = np.zeros(G, dtype=np.int64)
    sums = np.zeros((G, 5), dtype=np.longdouble)
    asums = np.zeros((G, 5), dtype=np.longdouble)
    D = M * (M - 1) if fair else M * M
    coef = (2 * np.arange(M) - M + 1).astype(np.longdouble)
    for i in range(rows):
        lead, col = divmod(i, ncol)
        w = 1.0 if col_weight is None else float(col_weight[col])
        g = int(sg[lead])
        if not (np.isfinite(y[i]) and w > 0.0 and g >= 0):
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            d = Xd[i] - y[i]
        if not (np.all(np.isfinite(Xd[i])) and np.all(np.isfinite(d))):
            n_bad[g] += 1
            continue
        below[i] = int(np.sum(Xd[i] < y[i]))
        equal[i] = int(np.sum(Xd[i] == y[i]))
        rank[i] = below[i] + pick(seed, lead * ncol_total + col_offset + col, equal[i])
        dl = d.astype(np.longdouble)
        e = dl.sum() / M
        err[i] = float(e)
        var[i] = 0.0 if np.all(d == d[0]) else float(((dl - e) ** 2).sum() / (M - 1))
        mad[i] = float(np.abs(dl).sum() / M)
        crps[i] = float(np.abs(dl).sum() / M - (coef * np.sort(dl)).sum() / D)
        hist[g, rank[i]] += 1
        n[g] += 1
        t = np.array([1.0, crps[i], err[i], err[i] * err[i], var[i]], dtype=np.longdouble) * w
        sums[g] += t
        asums[g] += np.abs(t)
    return dict(below=below, equal=equal, rank=rank, crps=crps, err=err, var=var, hist=hist, n=n, n_bad=n_bad,
                sums=sums.astype(np.float64), abs_sums=asums.astype(np.float64), mean_abs_d=mad)


def make_case(seed, n_lead, ncol, M, dtype=np.float64):
    """A state of mixed magnitudes with ties: slabs around 280 with spread 1, around 0 with spread 1e-3, quantised to 0.1."""
    rng = np.random.default_rng(seed)
    rows = n_lead * ncol
    centre = np.repeat(np.array([280.0, 0.0, -5.0, 1e4])[np.arange(n_lead) % 4], ncol)
    scale = np.repeat(np.array([1.0, 1e-3, 2.0, 30.0])[np.arange(n_lead) % 4], ncol)
    X = centre[:, None] + scale[:, None] * rng.standard_normal((rows, M))
    y = centre + scale * rng.standard_normal(rows)
    q = np.arange(rows) % 5 == 0          # every fifth row quantised: ties among the members and with y
    X[q] = np.round(X[q], 1)
    y[q] = np.round(y[q], 1)
    X = X.astype(dtype)
    if dtype == np.float32:
        y[q] = X[q, 0].astype(np.float64)  # a tie with y needs y on the float32 grid
    return X, y
