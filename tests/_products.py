"""NumPy model of efa_products_dev: the rows sorted by numpy.sort, every sum in numpy.longdouble, the counts by plain
comparison, the quantile by the definition's own three steps.  No GPU, no library."""
import numpy as np

U = 2.0 ** -53


def levels(q, M):
    """(lo, hi, f) of level q for M members: numpy's linear rule, h = q (M - 1) in float64."""
    h = np.float64(q) * np.float64(M - 1)
    lo = min(int(np.floor(h)), M - 1)
    hi = min(lo + 1, M - 1)
    return lo, hi, float(h - lo)


def quantile_rows(xs, q):
    """The quantile at level q of every row of xs (rows, M), sorted upwards: x_lo when f == 0, else min(x_hi, fma(f, x_hi - x_lo,
    x_lo)) with the difference rounded to float64 and the fma taken in longdouble before its rounding to float64.  Also x_lo and x_hi."""
    M = xs.shape[1]
    lo, hi, f = levels(q, M)
    xlo, xhi = xs[:, lo], xs[:, hi]
    if f == 0.0:
        return xlo.copy(), xlo, xhi
    with np.errstate(over="ignore", invalid="ignore"):
        diff = xhi - xlo                                         # float64, may overflow to inf as on the device
        v = (np.longdouble(f) * diff.astype(np.longdouble) + xlo.astype(np.longdouble)).astype(np.float64)
    return np.minimum(xhi, v), xlo, xhi


def model(X, n_lead, quantiles=(), thr=None, y=None, slab_group=None, col_weight=None):
    """X (rows, M) float64 or float32; thr (n_lead, T) or None; y (rows,) or None (no verification).  Returns mean, sd, var
    (longdouble-accurate, rounded once), mean_abs (rows,), quant / qlo / qhi (Q, rows), prob (T, rows), k (T, rows) int, bad
    (rows,), and with y: table (G, T, M+1, 2), n, n_bad (G, T), sums, abs_sums (G, T, 4)."""
    X = np.asarray(X)
    rows, M = X.shape
    ncol = rows // max(n_lead, 1)
    Xd = X.astype(np.float64)
    bad = ~np.all(np.isfinite(Xd), axis=1)
    Xl = np.where(bad[:, None], 0.0, Xd).astype(np.longdouble)
    mean_l = Xl.sum(axis=1) / M
    flat = np.all(Xd == Xd[:, :1], axis=1)
    mean = np.where(flat, Xd[:, 0], mean_l.astype(np.float64))
    var_l = ((Xl - mean_l[:, None]) ** 2).sum(axis=1) / (M - 1)
    with np.errstate(over="ignore"):                               # (members of 1e308: the variance is beyond float64)
        var = np.where(flat, 0.0, var_l.astype(np.float64))
        sd = np.where(flat, 0.0, np.sqrt(var_l).astype(np.float64))
    mean_abs = (np.abs(Xl).sum(axis=1) / M).astype(np.float64)
    for a in (mean, var, sd, mean_abs):
        a[bad] = np.nan
    out = dict(mean=mean, sd=sd, var=var, mean_abs=mean_abs, bad=bad)
    xs = np.sort(np.where(bad[:, None], 0.0, Xd), axis=1)
    Q = len(quantiles)
    quant, qlo, qhi = (np.full((Q, rows), np.nan) for _ in range(3))
    for i, q in enumerate(quantiles):
        quant[i], qlo[i], qhi[i] = quantile_rows(xs, q)
        for a in (quant, qlo, qhi):
            a[i, bad] = np.nan
    out.update(quant=quant, qlo=qlo, qhi=qhi)
    thr = np.zeros((n_lead, 0)) if thr is None else np.asarray(thr, dtype=np.float64).reshape(n_lead, -1)
    T = thr.shape[1]
    trow = np.repeat(thr, ncol, axis=0).T                          # (T, rows)
    with np.errstate(invalid="ignore"):
        k = np.sum(Xd[None, :, :] > trow[:, :, None], axis=2).astype(np.int64)
    prob = k / np.float64(M)
    prob[np.isnan(trow) | bad[None, :]] = np.nan
    out.update(prob=prob, k=k)
    if y is None:
        return out
    y = np.asarray(y, dtype=np.float64)
    sg = np.asarray(slab_group, dtype=np.int64)
    G = int(sg.max()) + 1 if sg.size and sg.max() >= 0 else 0
    w = np.ones(ncol) if col_weight is None else np.asarray(col_weight, dtype=np.float64)
    wrow = np.tile(w, n_lead)
    grow = np.repeat(sg, ncol)
    table = np.zeros((G, T, M + 1, 2), dtype=np.int64)
    n_bad = np.zeros((G, T), dtype=np.int64)
    sums = np.zeros((G, T, 4), dtype=np.longdouble)
    asums = np.zeros((G, T, 4), dtype=np.longdouble)
    for j in range(T):
        would = np.isfinite(y) & (wrow > 0.0) & (grow >= 0) & np.isfinite(trow[j])
        for i in np.nonzero(would)[0]:
            g = grow[i]
            if bad[i]:
                n_bad[g, j] += 1
                continue
            o = 1 if y[i] > trow[j, i] else 0
            table[g, j, k[j, i], o] += 1
            p = np.longdouble(prob[j, i])                          # the field: k / M rounded once
            t = np.array([1.0, (p - o) ** 2, p, o], dtype=np.longdouble) * np.longdouble(wrow[i])
            sums[g, j] += t
            asums[g, j] += np.abs(t)
    out.update(table=table, n=table.sum(axis=(2, 3)), n_bad=n_bad, sums=sums.astype(np.float64), abs_sums=asums.astype(np.float64))
    return out


def scores(table, sums):
    """Brier score and Murphy's (1973) decomposition of one (group, threshold): (brier, base_rate, forecast_rate, brier_skill) from
    the sums and (reliability, resolution, uncertainty) from the integer table with its M + 1 natural bins."""
    table = np.asarray(table, dtype=np.float64)
    M = table.shape[0] - 1
    nk = table.sum(axis=1)
    n = nk.sum()
    brier, base, frate = sums[1] / sums[0], sums[3] / sums[0], sums[2] / sums[0]
    den = base * (1.0 - base)
    skill = 1.0 - brier / den if den != 0.0 else np.nan
    p = np.arange(M + 1) / float(M)
    ok = np.divide(table[:, 1], nk, out=np.zeros(M + 1), where=nk > 0)
    obar = table[:, 1].sum() / n
    rel = np.sum(nk * (p - ok) ** 2) / n
    res = np.sum(nk * (ok - obar) ** 2) / n
    return dict(brier=brier, base_rate=base, forecast_rate=frate, brier_skill=skill, reliability=rel, resolution=res,
                uncertainty=obar * (1.0 - obar))


def make_case(seed, n_lead, ncol, M, dtype=np.float64):
    """A state of mixed magnitudes with ties (slabs around 280 with spread 1, around 0 with spread 1e-3, around -5 with spread 2;
    every fifth row quantised to 0.1), a verifying value per row, and two thresholds per slab near the slab's centre."""
    rng = np.random.default_rng(seed)
    rows = n_lead * ncol
    c_s = np.array([280.0, 0.0, -5.0, 1e4])[np.arange(n_lead) % 4]
    s_s = np.array([1.0, 1e-3, 2.0, 30.0])[np.arange(n_lead) % 4]
    centre, scale = np.repeat(c_s, ncol), np.repeat(s_s, ncol)
    X = centre[:, None] + scale[:, None] * rng.standard_normal((rows, M))
    y = centre + scale * rng.standard_normal(rows)
    q = np.arange(rows) % 5 == 0
    X[q] = np.round(X[q], 1) + 0.0                                  # (+ 0.0: no -0.0, whose place among zeros no sort defines)
    y[q] = np.round(y[q], 1)
    X = X.astype(dtype)
    thr = np.stack([c_s - 0.5 * s_s, np.round(c_s + 0.3 * s_s, 1)], axis=1)
    if dtype == np.float32:
        thr = thr.astype(np.float32).astype(np.float64)             # a tie with a member needs the threshold on the float32 grid
    return X, y, thr
