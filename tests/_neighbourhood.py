"""NumPy model of efa_neighbourhood_dev: the windows as sums and ORs of shifted arrays, every count an integer, a
field one division of two integers, the six sums in numpy.longdouble.  No GPU, no library."""
import numpy as np

U = 2.0 ** -53


def half_widths(r, shape):
    """h[|dy|] for |dy| <= r: r for the square (shape 0); the largest h with h*h + dy*dy <= r*r for the disc (shape 1)."""
    out = []
    for dy in range(r + 1):
        h = r
        if shape == 1:
            while h * h + dy * dy > r * r:
                h -= 1
        out.append(h)
    return out


def offsets(r, shape):
    hw = half_widths(r, shape)
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-hw[abs(dy)], hw[abs(dy)] + 1)]


def _shifted(A, dy, dx, wrap):
    """B[l, y, x, ...] = A[l, y + dy, x + dx, ...] where that lies in the slab (x + dx modulo nx with wrap), else 0."""
    ny, nx = A.shape[1:3]
    B = np.zeros_like(A)
    if abs(dy) >= ny:
        return B
    ys, yd = slice(max(dy, 0), ny + min(dy, 0)), slice(max(-dy, 0), ny + min(-dy, 0))
    if wrap:
        B[:, yd] = np.roll(A, -dx, axis=2)[:, ys]
    elif abs(dx) < nx:
        xs, xd = slice(max(dx, 0), nx + min(dx, 0)), slice(max(-dx, 0), nx + min(-dx, 0))
        B[:, yd, xd] = A[:, ys, xs]
    return B


def model(X, n_lead, ny, nx, thr, radii, shape=0, wrap=False, y=None, slab_group=None, col_weight=None):
    """X (rows, M) float64 or float32, rows = n_lead*ny*nx; thr (n_lead, T); radii a sequence.  Returns valid (rows,), k (T, rows),
    and per radius and threshold the integers S, n, union, osum (R, T, rows) and the fields nep, nmep (R, T, rows); with y also
    sums, abs_sums (G, R, T, 6) and cnt, n_bad (G, R, T)."""
    X = np.asarray(X)
    rows, M = X.shape
    ncol = ny * nx
    assert rows == n_lead * ncol
    Xd = X.astype(np.float64)
    thr = np.asarray(thr, dtype=np.float64).reshape(n_lead, -1)
    T, R = thr.shape[1], len(radii)
    members_ok = np.all(np.isfinite(Xd), axis=1)
    ver = y is not None
    yv = np.asarray(y, dtype=np.float64) if ver else np.zeros(rows)
    valid = members_ok & (np.isfinite(yv) if ver else True)
    trow = np.repeat(thr, ncol, axis=0).T                                   # (T, rows)
    with np.errstate(invalid="ignore"):
        E = (Xd[None, :, :] > trow[:, :, None]) & valid[None, :, None]    # (T, rows, M)
        o = ((yv[None, :] > trow) & valid[None, :]).astype(np.int64)       # (T, rows)
    k = E.sum(axis=2).astype(np.int64)
    S, n, un, osum = (np.zeros((R, T, rows), dtype=np.int64) for _ in range(4))
    V3 = valid.astype(np.int64).reshape(n_lead, ny, nx)
    for ri, r in enumerate(radii):
        offs = [(dy, dx) for dy, dx in offsets(int(r), shape) if abs(dy) < ny and (wrap or abs(dx) < nx)]
        nn = np.zeros((n_lead, ny, nx), dtype=np.int64)
        for dy, dx in offs:
            nn += _shifted(V3, dy, dx, wrap)
        for j in range(T):
            K3 = k[j].reshape(n_lead, ny, nx)
            O3 = o[j].reshape(n_lead, ny, nx)
            E3 = E[j].reshape(n_lead, ny, nx, M)
            sk, so = np.zeros_like(K3), np.zeros_like(O3)
            ue = np.zeros_like(E3)
            for dy, dx in offs:
                sk += _shifted(K3, dy, dx, wrap)
                so += _shifted(O3, dy, dx, wrap)
                ue |= _shifted(E3, dy, dx, wrap)
            S[ri, j], n[ri, j], osum[ri, j] = sk.reshape(-1), nn.reshape(-1), so.reshape(-1)
            un[ri, j] = ue.sum(axis=3).reshape(-1)
    tnan = np.isnan(trow)[None, :, :] | ~valid[None, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        nep = S.astype(np.float64) / (np.float64(M) * n.astype(np.float64))
        nmep = un.astype(np.float64) / np.float64(M)
        obs = osum.astype(np.float64) / n.astype(np.float64)
    nep[np.broadcast_to(tnan, nep.shape)] = np.nan
    nmep[np.broadcast_to(tnan, nmep.shape)] = np.nan
    out = dict(valid=valid, k=k, S=S, n=n, union=un, osum=osum, nep=nep, nmep=nmep)
    if not ver:
        return out
    sg = np.asarray(slab_group, dtype=np.int64)
    G = int(sg.max()) + 1 if sg.size and sg.max() >= 0 else 0
    w = np.ones(ncol) if col_weight is None else np.asarray(col_weight, dtype=np.float64)
    wrow, grow = np.tile(w, n_lead), np.repeat(sg, ncol)
    sums = np.zeros((G, R, T, 6), dtype=np.longdouble)
    asums = np.zeros((G, R, T, 6), dtype=np.longdouble)
    cnt = np.zeros((G, R, T), dtype=np.int64)
    n_bad = np.zeros((G, R, T), dtype=np.int64)
    for j in range(T):
        would = (wrow > 0.0) & (grow >= 0) & np.isfinite(trow[j]) & np.isfinite(yv)
        for g in range(G):
            ing = would & (grow == g)
            sc = ing & valid
            n_bad[g, :, j] = np.count_nonzero(ing & ~members_ok)
            cnt[g, :, j] = np.count_nonzero(sc)
            wl = wrow[sc].astype(np.longdouble)
            for ri in range(R):
                P, O = nep[ri, j, sc].astype(np.longdouble), obs[ri, j, sc].astype(np.longdouble)
                t = np.stack([np.ones_like(P), (P - O) ** 2, P * P, O * O, P, O], axis=1) * wl[:, None]
                sums[g, ri, j] = t.sum(axis=0)
                asums[g, ri, j] = np.abs(t).sum(axis=0)
    out.update(sums=sums.astype(np.float64), abs_sums=asums.astype(np.float64), cnt=cnt, n_bad=n_bad, obs=obs)
    return out


def brute(X, n_lead, ny, nx, thr, radii, shape=0, wrap=False, y=None):
    """The definitions with four loops: (S, n, union, osum) (R, T, rows) as integers."""
    X = np.asarray(X, dtype=np.float64)
    rows, M = X.shape
    thr = np.asarray(thr, dtype=np.float64).reshape(n_lead, -1)
    T, R = thr.shape[1], len(radii)
    S, n, un, osum = (np.zeros((R, T, rows), dtype=np.int64) for _ in range(4))
    ok = [bool(np.all(np.isfinite(X[i])) and (y is None or np.isfinite(y[i]))) for i in range(rows)]
    for ri, r in enumerate(radii):
        for j in range(T):
            for lead in range(n_lead):
                t = thr[lead, j]
                for yy in range(ny):
                    for xx in range(nx):
                        members = np.zeros(M, dtype=bool)
                        s = c = so = 0
                        for dy in range(-r, r + 1):
                            for dx in range(-r, r + 1):
                                if shape == 1 and dy * dy + dx * dx > r * r:
                                    continue
                                y2, x2 = yy + dy, xx + dx
                                if y2 < 0 or y2 >= ny:
                                    continue
                                if wrap:
                                    x2 %= nx
                                elif x2 < 0 or x2 >= nx:
                                    continue
                                i2 = (lead * ny + y2) * nx + x2
                                if not ok[i2]:
                                    continue
                                ex = X[i2] > t
                                members |= ex
                                s += int(ex.sum())
                                c += 1
                                if y is not None and y[i2] > t:
                                    so += 1
                        i = (lead * ny + yy) * nx + xx
                        S[ri, j, i], n[ri, j, i], un[ri, j, i], osum[ri, j, i] = s, c, int(members.sum()), so
    return S, n, un, osum


def fss(sums):
    """(fss, mse, base_rate, forecast_rate) of one (group, radius, threshold) by the direct formulas."""
    den = sums[2] + sums[3]
    return (1.0 - sums[1] / den if den != 0.0 else np.nan, sums[1] / sums[0], sums[5] / sums[0], sums[4] / sums[0])


def make_case(seed, n_lead, ny, nx, M, dtype=np.float64, smooth=True):
    """A state with spatial structure (a smooth field per slab plus member noise), a verifying value per row and thresholds near
    the field's median, so that events are neither rare nor universal."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    X = np.empty((n_lead, ny, nx, M))
    yv = np.empty((n_lead, ny, nx))
    for l in range(n_lead):
        base = np.sin(0.7 * yy + l) + np.cos(0.5 * xx - l) if smooth else np.zeros((ny, nx))
        X[l] = 280.0 + base[:, :, None] + 0.8 * rng.standard_normal((ny, nx, M))
        yv[l] = 280.0 + base + 0.8 * rng.standard_normal((ny, nx))
    X = X.reshape(-1, M)
    q = np.arange(X.shape[0]) % 5 == 0
    X[q] = np.round(X[q], 1)                       # ties with the rounded thresholds
    X = X.astype(dtype)
    return X, yv.reshape(-1)
