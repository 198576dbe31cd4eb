"""NumPy model of efa_pm_mean_dev: per segment a stable argsort of the rank field + 0.0 and a sort of the pooled
members + 0.0; a two-loop brute force of the same definition to check the model against; and the value families of the tests.
No GPU, no library."""
import numpy as np

FAMILIES = ("bits", "mixed", "precip", "const", "lowbyte", "highbyte")


def segments(ny, nx, py, px):
    """The column indices (y*nx + x, ascending) of every patch of a slab, patch (Y, X) at Y*ceil(nx/px) + X."""
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    npx = -(-nx // px)
    sid = ((yy // py) * npx + xx // px).reshape(-1)
    return [np.flatnonzero(sid == s) for s in range(int(sid.max()) + 1)]


def included(X, f):
    return np.isfinite(np.asarray(f, dtype=np.float64)) & np.all(np.isfinite(np.asarray(X, dtype=np.float64)), axis=1)


def model(X, f, n_lead, ny, nx, patch=None, g=None, slab_on=None):
    """X (rows, M) float64 or float32, f (rows,), rows = n_lead*ny*nx.  Returns (pm (rows,) float64, n_bad (n_lead,) int64)."""
    X = np.asarray(X)
    f = np.asarray(f, dtype=np.float64)
    rows, M = X.shape
    ncol = ny * nx
    assert rows == n_lead * ncol and f.shape == (rows,)
    py, px = (ny, nx) if patch is None else patch
    g = M // 2 if g is None else g
    inc = included(X, f)
    pm = np.full(rows, np.nan)
    n_bad = np.zeros(n_lead, dtype=np.int64)
    segs = segments(ny, nx, py, px)
    for lead in range(n_lead):
        if slab_on is not None and not slab_on[lead]:
            continue
        n_bad[lead] = np.count_nonzero(~inc[lead * ncol:(lead + 1) * ncol])
        for cols in segs:
            r = lead * ncol + cols
            r = r[inc[r]]
            if r.size == 0:
                continue
            order = r[np.argsort(f[r] + 0.0, kind="stable")]
            pool = np.sort((X[r] + X.dtype.type(0.0)).reshape(-1))
            pm[order] = pool[np.arange(r.size) * M + g].astype(np.float64)
    return pm, n_bad


def brute(X, f, n_lead, ny, nx, patch=None, g=None, slab_on=None):
    """The definition with two loops per segment: a row's rank is the number of rows before it, its value the pooled value with
    exactly rank*M + g values before it (smaller ones, and equal ones counted as sorting puts them)."""
    X = np.asarray(X)
    f = np.asarray(f, dtype=np.float64)
    rows, M = X.shape
    ncol = ny * nx
    py, px = (ny, nx) if patch is None else patch
    g = M // 2 if g is None else g
    pm = np.full(rows, np.nan)
    n_bad = np.zeros(n_lead, dtype=np.int64)
    for lead in range(n_lead):
        if slab_on is not None and not slab_on[lead]:
            continue
        for Y in range(-(-ny // py)):
            for Xp in range(-(-nx // px)):
                rws = [lead * ncol + y * nx + x for y in range(Y * py, min(ny, (Y + 1) * py))
                       for x in range(Xp * px, min(nx, (Xp + 1) * px))]
                ok = [i for i in rws if np.isfinite(f[i]) and np.all(np.isfinite(X[i].astype(np.float64)))]
                n_bad[lead] += len(rws) - len(ok)
                pool = [float(v) for i in ok for v in X[i]]
                for i in ok:
                    rank = 0
                    for j in ok:
                        if f[j] < f[i] or (f[j] == f[i] and j < i):
                            rank += 1
                    k = rank * M + g
                    for v in pool:
                        less = sum(1 for u in pool if u < v)
                        leq = sum(1 for u in pool if u <= v)
                        if less <= k < leq:
                            pm[i] = v + 0.0
                            break
    return pm, n_bad


def _finite_bits(rng, n, dtype):
    """Random bit patterns as floats, the ones that are not finite replaced: every digit of every key byte occurs."""
    if np.dtype(dtype) == np.float64:
        v = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64).view(np.float64)
    else:
        v = rng.integers(0, 2 ** 32, size=n, dtype=np.uint32).view(np.float32)
    v = v.copy()
    v[~np.isfinite(v)] = 1.0
    return v


def make_case(family, seed, n_lead, ny, nx, M, dtype=np.float64):
    """(X (rows, M) of `dtype`, f (rows,) float64): a state of one value family and a rank field with ties that shares its keys'
    digits (member 0, rounded in part)."""
    rng = np.random.default_rng(seed)
    rows = n_lead * ny * nx
    n = rows * M
    dt = np.dtype(dtype)
    wide = dt == np.float64
    if family == "bits":
        v = _finite_bits(rng, n, dt)
    elif family == "mixed":
        # both signs over many binades, denormals of both signs, and both zeros
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, size=n)).astype(dt)
        tiny = np.finfo(dt).smallest_subnormal
        k = rng.integers(0, 8, size=n)
        v[k == 0] = (rng.integers(-50, 50, size=np.count_nonzero(k == 0)) * tiny).astype(dt)
        v[k == 1] = 0.0
        v[k == 2] = -0.0
    elif family == "precip":
        v = np.where(rng.random(n) < 0.7, 0.0, np.round(rng.gamma(0.6, 4.0, size=n), 1)).astype(dt)
    elif family == "const":
        v = np.full(n, 3.25, dtype=dt)
    elif family == "lowbyte":
        if wide:
            v = (np.float64(1.5).view(np.uint64) | rng.integers(0, 256, size=n, dtype=np.uint64)).view(np.float64)
        else:
            v = (np.float32(1.5).view(np.uint32) | rng.integers(0, 256, size=n, dtype=np.uint32)).view(np.float32)
    elif family == "highbyte":
        # positive values (a negative one has every lower bit of its key flipped) whose bits differ in the highest byte only;
        # the exponent bits below that byte are 0, so no pattern is Inf or NaN
        if wide:
            v = ((rng.integers(0, 128, size=n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x000A5A5A5A5A5A5A)).view(np.float64)
        else:
            v = ((rng.integers(0, 128, size=n, dtype=np.uint32) << np.uint32(24)) | np.uint32(0x005A5A5A)).view(np.float32)
    else:
        raise ValueError(family)
    X = np.ascontiguousarray(v.reshape(rows, M))
    assert X.dtype == dt and np.all(np.isfinite(X))
    f = X[:, 0].astype(np.float64)
    q = np.arange(rows) % 3 == 0
    f[q] = f[(np.arange(rows)[q] // 6) * 6 % rows]        # ties between neighbours
    return X, f
