"""Row independence: helpers of tests/test_rowprops_host.py and tests/test_gpu_rowprops.py.

Three relations, none of which an error scaled by the ARRAY's maximum can see:
  1. scaling state row i by 2^k_i scales its posterior by 2^k_i, bit for bit (`row_exponents`, `scale_rows`);
  2. a row of NaN, +Inf, zeros or one constant changes no other row's bits (`POISON_*`, `poison`, `assert_poisoned`);
  3. with obs (and state rows) of mixed magnitude every row and every ob stays within 1e-10 of ITS OWN scale of the oracle
     (`mixed_case`, `assert_rows_close`, `assert_diag_close`), and scaling ob k by 2^j_k leaves the state posterior's bits
     (`scale_obs`, `scaled_diag`).
Nothing here needs a GPU."""
import numpy as np

from oracle import ensrf_oracle as orc
from test_gpu_state_routes import ASSIM, N_LEAD, NCOL, NX, NY, P, ROWS

F32, F64 = np.float32, np.float64
DIAG = ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated")
RTOL = 1e-10            # BASELINE.json north_star, here per row and per ob
CONDITION = 1e-12       # the generators keep the oracle's own error below a hundredth of RTOL

SIZES = [2, 4, 6, 7, 20, 100, 104, 106, 136, 138, 256]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_bits(got, want, what, rows=None):
    """Bit for bit (NaN payloads and the sign of zero included); `rows` restricts the comparison to those rows."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if rows is not None:
        got, want = got[rows], want[rows]
    bad = bits(got) != bits(want)
    if bad.any():
        first = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d values differ in their bits, first at %r: %r against %r" % (
            what, int(bad.sum()), bad.size, first, got[first], want[first]))


# ---------------------------------------------------------------------------
# relation 1: powers of two on the state rows
# ---------------------------------------------------------------------------
def row_exponents(rows, seed, lo=-30, hi=30):
    """k_i in [lo, hi] from a seeded stream, with the neighbours hi / lo (both orders), a run of 16 equal exponents that
    starts off a multiple of 16 and an exponent 0 next to it."""
    rng = np.random.default_rng(seed)
    k = rng.integers(lo, hi + 1, rows)
    assert rows >= 48
    k[5], k[6], k[7] = hi, lo, hi
    k[20:36] = 11
    k[36] = 0
    k[rows - 2], k[rows - 1] = lo, hi
    return k.astype(np.int64)


def scale_rows(X, k):
    """diag(2^k) X, exactly: asserts that no value leaves the normal range of X's type (and of float32 when X holds float32
    values widened) and that every square stays normal in float64, so that no mantissa changes anywhere downstream."""
    X = np.asarray(X)
    k = np.asarray(k)
    kk = k.reshape((-1,) + (1,) * (X.ndim - 1))
    out = np.ldexp(X, kk).astype(X.dtype)
    fin = np.isfinite(X) & (X != 0)
    if fin.any():
        info = np.finfo(X.dtype)
        mag = np.abs(out[fin].astype(np.longdouble))
        assert mag.min() >= info.tiny and mag.max() <= info.max, "a scaled value left the normal range"
        sq = mag * mag
        assert sq.min() >= np.finfo(F64).tiny * 2.0 ** 60 and sq.max() <= np.finfo(F64).max * 2.0 ** -60, "a square is not normal"
        assert np.array_equal(np.ldexp(out, -kk)[fin], X[fin]), "the scaling is not exact"
    return out


# ---------------------------------------------------------------------------
# the problem of parts 1 and 2: the grid of tests/test_gpu_state_routes.py with a caller-supplied state
# ---------------------------------------------------------------------------
# rows that hold the poison: row 0; 15 | 16 (an MFMA tile edge); the last row and one more of the partial last tile (96..104);
# two adjacent rows; rows 3 and 79: columns 3 and 9 of the first 16-column block in slabs 0 and 2; row 69: the north-east corner
# column in slab 1, which no ob's taper reaches (as row 104, the same column in slab 2)
POISON_ROWS = np.array([0, 3, 15, 16, 50, 51, 69, 79, 100, 104])
# ... and only the second row of each pair (tile edge, adjacent rows, partial last tile), so that a leak from one poisoned row
# into its neighbour is seen too
POISON_SECOND = np.array([16, 51, 104])
POISON_SETS = (POISON_ROWS, POISON_SECOND)
UNREACHED_ROWS = (69, 104)
POISON_KINDS = ("nan", "inf", "zero", "const")
POISON_CONST = 287.15


class RowProblem(object):
    """The attributes `_run` of tests/test_gpu_state_routes.py reads (3 slabs of 5 x 7 columns, 105 rows, 12 obs of single
    rows of which 10 are assimilated).  The obs sample rows of the south-west part of the grid that are not in POISON_ROWS,
    with half-widths of 350..650 km, so that the north-east corner column lies beyond every taper (asserted).  `state`:
    float32 rows that replace the state AFTER the obs block was built from the seeded one."""

    def __init__(self, M, state=None, gross=()):
        rng = np.random.default_rng(7100 + M)
        self.M, self.gross = M, tuple(gross)
        lat, lon = np.meshgrid(np.linspace(30, 50, NY), np.linspace(230, 262, NX), indexing="ij")
        self.lat2d, self.lon2d = lat, lon
        self.glat, self.glon = lat.reshape(-1).copy(), lon.reshape(-1).copy()
        clean = (3.0 * rng.standard_normal((ROWS, 1)) + 2.0 * rng.standard_normal((ROWS, M))).astype(F32)
        iy, ix = np.divmod(np.arange(ROWS) % NCOL, NX)
        ok = (iy <= 2) & (ix <= 4) & ~np.isin(np.arange(ROWS), POISON_ROWS)
        self.pick = pick = rng.choice(np.flatnonzero(ok), P, replace=False)
        self.clean32 = clean
        self.HX = clean.astype(F64)[pick].copy()
        self.value = self.HX.mean(axis=1) + rng.standard_normal(P)
        for k in gross:
            self.value[k] += 40.0
        self.error = rng.uniform(0.5, 1.5, P)
        self.ob_lat, self.ob_lon = self.glat[pick % NCOL], self.glon[pick % NCOL]
        self.hw = rng.uniform(350.0, 650.0, P)
        self.X32 = clean if state is None else np.ascontiguousarray(state, dtype=F32)
        assert self.X32.shape == (ROWS, M)
        self.X64 = self.X32.astype(F64)
        reach = np.zeros(NCOL, dtype=bool)
        for k in np.flatnonzero(ASSIM):
            reach |= orc.localize_state(lat, lon, self.ob_lat[k], self.ob_lon[k], self.hw[k]).reshape(-1) != 0
        self.reached = np.tile(reach, N_LEAD)
        assert not self.reached[list(UNREACHED_ROWS)].any() and self.reached[[3, 79]].all()

    def with_state(self, state):
        return RowProblem(self.M, state=state, gross=self.gross)

    def oracle_kw(self, gc):
        if not gc:
            return {}
        return dict(loc="GC", ob_lat=self.ob_lat, ob_lon=self.ob_lon, ob_halfwidth=self.hw, grid_lat=self.lat2d,
                    grid_lon=self.lon2d, state_shape=(N_LEAD, 1, NY, NX))


def poison(X, kind, rows=POISON_ROWS):
    """X with `rows` replaced (a copy)."""
    X = np.array(X)
    X[rows] = {"nan": np.nan, "inf": np.inf, "zero": 0.0, "const": POISON_CONST}[kind]
    return X


def oracle_members(pb, gc, relax="none", alpha=0.5):
    """The oracle's posterior members and diagnostics of the problem (obs block as built, state as it is now), relaxed by the
    closed forms of tests/test_relaxation_host.py."""
    from test_relaxation_host import relax as closed_form
    with np.errstate(invalid="ignore", over="ignore"):
        post, _, _, diag = orc.ensrf_cycle(pb.X64, pb.HX, pb.value, pb.error, ASSIM, **pb.oracle_kw(gc))
        if relax == "rtpp":
            post = closed_form(pb.X64, post, rtpp=alpha)
        elif relax == "rtps":
            post = closed_form(pb.X64, post, rtps=alpha)
    return post, diag


def assert_poisoned(kind, got, clean, what, ref_rows=None, f32=False, poisoned=POISON_ROWS):
    """The posterior of the poisoned state against that of the clean one: every other row bit for bit, and the poisoned rows
    as the kind demands (`ref_rows`: the oracle's posterior of the constant rows)."""
    keep = np.ones(ROWS, dtype=bool)
    keep[poisoned] = False
    assert_same_bits(got, clean, what + ": rows that hold no poison", rows=keep)
    rows = got[poisoned]
    if kind == "nan":
        assert np.isnan(rows).all(), "%s: a NaN row came back with %d numbers" % (what, int((~np.isnan(rows)).sum()))
    elif kind == "inf":
        assert not np.isfinite(rows).any(), "%s: an Inf row came back with %d finite values" % (what, int(np.isfinite(rows).sum()))
    elif kind == "zero":
        assert (rows == 0).all(), "%s: a zero row came back with %d non-zero values" % (what, int((rows != 0).sum()))
    else:
        assert_rows_close(rows, ref_rows, what + ": constant rows", f32=f32)


# ---------------------------------------------------------------------------
# relation 3: the project's 1e-10 per row and per ob
# ---------------------------------------------------------------------------
def rows_err(got, ref, extra=None, f32=False):
    """max over the rows of |got - ref| / tol with tol = RTOL * max|ref row| (+ `extra`, for a mean row: the row's largest
    perturbation).  f32: the values were rounded to float32 once, which adds half an ulp of the value, 2^-24 |ref|."""
    got = np.asarray(got, dtype=F64)
    ref = np.asarray(ref, dtype=F64)
    assert got.shape == ref.shape
    g2, r2 = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    assert np.array_equal(np.isnan(g2), np.isnan(r2)), "NaN pattern"
    scale = np.max(np.abs(r2), axis=1, keepdims=True)
    if extra is not None:
        scale = scale + np.asarray(extra, dtype=F64).reshape(-1, 1)
    tol = RTOL * scale + (2.0 ** -24 * np.abs(r2) if f32 else 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(np.abs(g2 - r2) == 0, 0.0, np.abs(g2 - r2) / tol)
    q = np.where(np.isnan(r2), 0.0, q)
    return float(q.max()) if q.size else 0.0


def assert_rows_close(got, ref, what, extra=None, f32=False, tol=1.0):
    """Returns the worst err/tol.  `tol` = 1: the bound of the issue's table; CONDITION / RTOL: the generators' condition."""
    worst = rows_err(got, ref, extra, f32)
    assert worst <= tol, "%s: a row is off by %.3g of its own tolerance (%.1e of its scale)" % (what, worst / tol, worst * RTOL)
    return worst


def diag_err(got, ref):
    """Worst err/tol of the four diagnostics: variances RTOL * ref, means RTOL * (|ref| + sqrt(var)); NaN patterns and
    `assimilated` exact."""
    assert np.array_equal(np.asarray(got["assimilated"], dtype=bool), np.asarray(ref["assimilated"], dtype=bool)), "assimilated"
    worst = 0.0
    for mean, var in (("prior_mean", "prior_var"), ("post_mean", "post_var")):
        gv, rv = np.asarray(got[var], dtype=F64), np.asarray(ref[var], dtype=F64)
        gm, rm = np.asarray(got[mean], dtype=F64), np.asarray(ref[mean], dtype=F64)
        assert np.array_equal(np.isnan(gv), np.isnan(rv)) and np.array_equal(np.isnan(gm), np.isnan(rm)), "NaN pattern of " + mean
        ok = ~np.isnan(rv)
        if ok.any():
            assert (rv[ok] > 0).all()
            worst = max(worst, float(np.max(np.abs(gv[ok] - rv[ok]) / (RTOL * rv[ok]))),
                        float(np.max(np.abs(gm[ok] - rm[ok]) / (RTOL * (np.abs(rm[ok]) + np.sqrt(rv[ok]))))))
    return worst


def assert_diag_close(got, ref, what, tol=1.0):
    worst = diag_err(got, ref)
    assert worst <= tol, "%s: a diagnostic is off by %.3g of its own tolerance" % (what, worst / tol)
    return worst


def assert_augmented_close(xam, Xap, ref_xam, ref_Xap, what, tol=1.0):
    """(xam, Xap) of the augmented arrays, state rows and obs rows alike; returns (worst xam, worst Xap)."""
    a = assert_rows_close(Xap, ref_Xap, what + " Xap", tol=tol)
    b = assert_rows_close(np.asarray(xam).reshape(-1, 1), np.asarray(ref_xam, dtype=F64).reshape(-1, 1), what + " xam",
                          extra=np.max(np.abs(np.asarray(ref_Xap, dtype=F64)), axis=1), tol=tol)
    return b, a


# the weight of the four shared modes beside the unit noise: tuned on the CPU (tests/test_rowprops_host.py) so that every shape
# without localisation keeps each ob's variance above 2e-3 of its value at its block's start, and the band leader serves it
MODE_WEIGHT = 0.35
OFFSET = 300.0

MIXED_SHAPES = [(300, 7, 40), (257, 50, 70), (400, 100, 150), (300, 128, 140), (130, 256, 30)]
MIXED_GC_SHAPES = [(1024, 20, 90, 256), (900, 33, 40, 900)]      # (N, M, P, ncol), geometry as tests/test_gpu_parity._random_case


def mixed_case(N, M, P, ncol=None, offset=OFFSET, mode_weight=MODE_WEIGHT):
    """A state whose rows have scales 10^e, e in -6..6 -- the first half in blocks ("variables"), the second interleaved --,
    share four modes beside unit noise and carry a mean within +-offset of their own spread; P obs of single rows that meet
    every scale, value = mean + s N(0,1), error = s^2 U(0.25, 4), about one in ten not assimilated.  The dict of
    tests/test_gpu_parity._random_case (with `s_row`, `s_ob`)."""
    rng = np.random.default_rng(31000 + N + M + P)
    half = N // 2
    e = np.empty(N, dtype=np.int64)
    e[:half] = (np.arange(half) * 13) // max(half, 1) - 6
    e[half:] = (np.arange(N - half) * 5) % 13 - 6
    s = 10.0 ** e
    Z = mode_weight * rng.standard_normal((N, 4)) @ rng.standard_normal((4, M)) + rng.standard_normal((N, M))
    Z += (rng.uniform(-offset, offset, N) * Z.std(axis=1) - Z.mean(axis=1))[:, None]
    X = s[:, None] * Z
    rows = rng.choice(N, P, replace=(P > N))
    for v in range(min(13, P)):                      # every scale is observed
        rows[v] = rng.choice(np.flatnonzero(e == v - 6))
    HX = X[rows].copy()
    val = HX.mean(axis=1) + s[rows] * rng.standard_normal(P)
    err = s[rows] ** 2 * rng.uniform(0.25, 4.0, P)
    asm = rng.random(P) < 0.9
    c = dict(X=X, HX=HX, val=val, err=err, asm=asm, N=N, M=M, P=P, loc=bool(ncol), s_row=s, s_ob=s[rows], rows=rows)
    if ncol:
        assert N % ncol == 0
        ny = int(np.sqrt(ncol))
        while ncol % ny:
            ny -= 1
        nx = ncol // ny
        lat, lon = np.meshgrid(np.linspace(-70, 70, ny), np.linspace(0, 357, nx), indexing="ij")
        c.update(lat=lat, lon=lon, n_lead=N // ncol, ny=ny, nx=nx,
                 ob_lat=lat.reshape(-1)[rows % ncol] + 0.2 * rng.standard_normal(P),
                 ob_lon=lon.reshape(-1)[rows % ncol] + 0.2 * rng.standard_normal(P), hw=rng.uniform(800, 4000, P))
    return c


def oracle_kw(c):
    if not c["loc"]:
        return {}
    return dict(loc="GC", ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"], grid_lat=c["lat"], grid_lon=c["lon"],
                state_shape=(c["n_lead"], 1, c["ny"], c["nx"]))


def run_oracle(c, dtype=F64, perm=None, guard=False):
    """(xam, Xap, diag[, guard min ratio]) of the oracle's loop on arrays of `dtype` (np.longdouble: the augmented arrays
    are formed in that type too), with the members in the order `perm` (undone in the result)."""
    from _phase_a_guard import GuardProbe
    if dtype == F64 and perm is None:
        xbm, Xbp = orc.format_prior_state(c["X"], c["HX"])
    else:
        X, HX = np.asarray(c["X"], dtype=dtype), np.asarray(c["HX"], dtype=dtype)
        if perm is not None:
            X, HX = X[:, perm], HX[:, perm]
        xm, ym = X.mean(axis=1), HX.mean(axis=1)
        xbm = np.hstack((xm, ym))
        Xbp = np.vstack((X - xm[:, None], HX - ym[:, None]))
    probe = GuardProbe(c["N"], c["asm"]) if guard else None
    xam, Xap, diag = orc.ensrf_update(xbm, Xbp, c["N"], np.asarray(c["val"], dtype=dtype), np.asarray(c["err"], dtype=dtype),
                                      c["asm"], step_hook=probe, **oracle_kw(c))
    if perm is not None:
        Xap = Xap[:, np.argsort(perm)]
    return (xam, Xap, diag, probe.min_ratio()) if guard else (xam, Xap, diag)


# ---------------------------------------------------------------------------
# relation 3b: powers of two on the obs
# ---------------------------------------------------------------------------
def ob_exponents(P, seed, lo=-20, hi=20):
    j = np.random.default_rng(seed).integers(lo, hi + 1, P)
    if P >= 3:
        j[0], j[1], j[2] = hi, lo, 0
    return j.astype(np.int64)


def scale_obs(c, j):
    """The case with ob k's (HX_k, value_k, error_k) times (2^j, 2^j, 2^2j): the same update of the state."""
    out = dict(c)
    out["HX"] = scale_rows(c["HX"], j)
    out["val"] = np.ldexp(c["val"], j)
    out["err"] = np.ldexp(c["err"], 2 * j)
    return out


def scaled_diag(diag, j):
    out = dict(diag)
    for key in ("prior_mean", "post_mean"):
        out[key] = np.ldexp(diag[key], j)
    for key in ("prior_var", "post_var"):
        out[key] = np.ldexp(diag[key], 2 * j)
    return out


def assert_diag_bits(got, want, what):
    for key in DIAG:
        assert_same_bits(np.asarray(got[key]), np.asarray(want[key]), "%s: %s" % (what, key))
