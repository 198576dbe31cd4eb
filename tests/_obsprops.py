"""Phase A on poisoned, degenerate and guard-margin observations: generators and assertions of
tests/test_obsprops_host.py and tests/test_gpu_obsprops.py.  Nothing here needs a GPU.

  A. value and error of an ob that is not assimilated are not read (`IGNORED_*`, `with_ignored`);
  B. an ob the outlier check rejects for a NaN is one whose flag is 0 (`outlier_case`);
  C. a NaN, +Inf or zero row of an ob that is not assimilated changes no other row (`ROW_POISONS`, `poison_obs_rows`);
  D. an assimilated ob without spread has no gain (`zero_spread_case`);
  E. near-copy pairs placed just above and just below the leaders' cancellation guard (`margin_case`);
  F. obs rows that are not centred (`uncentred`).
"""
import numpy as np

from oracle import ensrf_oracle as orc
from _phase_a_guard import FALLS_BACK, MAX_PIPELINE_M, ROWS_PER_BLOCK, SAFE, GuardProbe
from _rowprops import DIAG, F64, RTOL, assert_same_bits, oracle_kw, rows_err
from test_gpu_parity import _random_case

N, P, P_MARGIN, NCOL = 96, 150, 200, 48          # 96 state rows ride along; 150 obs: two full 64-row blocks and a partial one
SIZES = (7, 24, 100, 128, 130, 256)
REQUESTS = (0, 1, 2, 3)                          # `pipeline` of tests/test_gpu_parity._run_hip
KIND_OF_REQUEST = {0: 2, 1: 1, 2: 3, 3: 4}       # phase_a_kind up to 128 members; 2 above

# the special obs: 0; 3 | 4 (a band edge); 63 | 64 (a block edge, both sides); 90, 91 (adjacent, inside block 1); 120 (directly
# before an assimilated ob) and 123 (directly after one); 149 (the last ob) ...
SPECIAL = np.array([0, 3, 4, 63, 64, 90, 91, 120, 123, 149])
# ... and only the second of each pair, so that a leak from one special ob into its special neighbour shows too
SPECIAL_SECOND = np.array([4, 64, 91])
SPECIAL_SETS = (SPECIAL, SPECIAL_SECOND)
NEIGHBOURS_ON = np.array([1, 2, 5, 62, 65, 89, 92, 119, 121, 122, 124, 148])   # assimilated whatever the seed says

IGNORED_FINITE = ((0.0, 0.0), (1.0, -1.0), (1e300, 1e-300))
IGNORED_NONFINITE = ((np.nan, np.nan), (np.inf, 1.0), (-np.inf, np.inf))
ROW_POISONS = ("nan", "inf", "zero", "one_nan")
ZERO_RUN = np.array([100, 101, 102])             # Part D: three zero-spread obs in a row (row 64, a block's first, is in SPECIAL)
UNCENTRED_ROWS = (5, 70)
UNCENTRED_C = (1e-12, 1e-10, 1e-3, 1.0)          # the band leader's centring guard sits at 1e-11


def want_kind(request, M):
    return 2 if M > MAX_PIPELINE_M else KIND_OF_REQUEST[request]


def _seeded(M, loc, seed, special_flag, rows):
    c = _random_case(seed, N, M, P, bool(loc), ncol=NCOL if loc else None)
    c["asm"] = np.array(c["asm"], dtype=bool)
    c["asm"][NEIGHBOURS_ON] = True
    c["asm"][rows] = bool(special_flag)
    c["HX"] = np.array(c["HX"])
    return c


_SEEDS = {}


def base_case(M, loc, special_flag, rows=SPECIAL):
    """The dict of tests/test_gpu_parity._random_case at (N, M, P) -- GC: 2 slabs of 48 columns, the obs at their sampled
    columns -- with the flag of the obs in `rows` set to `special_flag` and their neighbours assimilated.  The seed is the
    first of 52000 + 10 M + loc + 1000 j whose obs, all special ones assimilated, stay 1.5 SAFE clear of the leaders'
    cancellation guard (64 obs of a block on 7 members leave little variance): the tests assert the leader's own kind."""
    key = (M, bool(loc))
    if key not in _SEEDS:
        for j in range(40):
            seed = 52000 + 10 * M + int(bool(loc)) + 1000 * j
            if M > MAX_PIPELINE_M or oracle_case(_seeded(M, loc, seed, True, SPECIAL))[3] >= 1.5 * SAFE:
                break
        else:
            raise AssertionError("base_case: no seed keeps M=%d loc=%r clear of the guard" % key)
        _SEEDS[key] = seed
    return _seeded(M, loc, _SEEDS[key], special_flag, rows)


def with_ignored(c, pair, rows=SPECIAL):
    out = dict(c)
    out["val"], out["err"] = np.array(c["val"]), np.array(c["err"])
    out["val"][rows], out["err"][rows] = pair
    return out


def priors(c):
    """(ym, Yp) as `efa_form_perts_dev` and assimilation.py:36-49 form them."""
    return orc.compute_ob_priors(c["HX"])


def poison_obs_rows(Yp, kind, rows=SPECIAL):
    """Yp with `rows` replaced (a copy): NumPy's default quiet NaN, +Inf, 0.0, or one member (another one in every row) NaN."""
    Yp = np.array(Yp)
    if kind == "one_nan":
        Yp[rows, np.asarray(rows) % Yp.shape[1]] = np.nan
    else:
        Yp[rows] = {"nan": np.nan, "inf": np.inf, "zero": 0.0}[kind]
    return Yp


def oracle_block(c, ym, Yp, dtype=F64):
    """The oracle's (xam, Xap, diag, guard min ratio) on the case's state rows and the obs block (ym, Yp) exactly as given."""
    X = np.asarray(c["X"], dtype=dtype)
    xm = X.mean(axis=1)
    xbm = np.hstack((xm, np.asarray(ym, dtype=dtype)))
    Xbp = np.vstack((X - xm[:, None], np.asarray(Yp, dtype=dtype)))
    probe = GuardProbe(c["N"], c["asm"])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xam, Xap, diag = orc.ensrf_update(xbm, Xbp, c["N"], np.asarray(c["val"], dtype=dtype), np.asarray(c["err"], dtype=dtype),
                                          c["asm"], step_hook=probe, obs_taper="vector", **oracle_kw(c))
        ratio = probe.min_ratio() if np.isfinite(probe.var_step[probe.asm]).all() else np.nan
    return xam, Xap, diag, ratio


def oracle_case(c, dtype=F64):
    ym, Yp = priors(c)
    return oracle_block(c, ym, Yp, dtype)


# ---------------------------------------------------------------------------
# assertions
# ---------------------------------------------------------------------------
def diag_err(got, ref, obs=None):
    """`_rowprops.diag_err` for diagnostics that may hold a variance of 0 and NaNs: variances RTOL * ref, means
    RTOL * (|ref| + sqrt(var)); where that tolerance is 0 the values must be equal; NaN patterns and `assimilated` exact."""
    sel = slice(None) if obs is None else obs
    assert np.array_equal(np.asarray(got["assimilated"], dtype=bool)[sel], np.asarray(ref["assimilated"], dtype=bool)[sel]), "assimilated"
    worst = 0.0
    for mean, var in (("prior_mean", "prior_var"), ("post_mean", "post_var")):
        gv, rv = np.asarray(got[var], dtype=F64)[sel], np.asarray(ref[var], dtype=F64)[sel]
        gm, rm = np.asarray(got[mean], dtype=F64)[sel], np.asarray(ref[mean], dtype=F64)[sel]
        assert np.array_equal(np.isnan(gv), np.isnan(rv)) and np.array_equal(np.isnan(gm), np.isnan(rm)), "NaN pattern of " + mean
        ok = ~np.isnan(rv) & ~np.isnan(rm)
        assert (rv[ok] >= 0).all()
        with np.errstate(invalid="ignore", divide="ignore"):
            for d, tol in ((np.abs(gv - rv)[ok], RTOL * rv[ok]), (np.abs(gm - rm)[ok], RTOL * (np.abs(rm[ok]) + np.sqrt(rv[ok])))):
                q = np.where(d == 0, 0.0, d / tol)
                worst = max(worst, float(q.max()) if q.size else 0.0)
    return worst


def assert_diag_close(got, ref, what, obs=None, tol=1.0):
    worst = diag_err(got, ref, obs)
    assert worst <= tol, "%s: a diagnostic is off by %.3g of its own tolerance" % (what, worst / tol)
    return worst


def assert_block_close(got, ref, what, keep=None, tol=1.0):
    """(state posterior members or perturbations, obs means, obs perturbations) against the oracle's, per row, on the obs rows
    in `keep` (all by default): returns the worst err/tol."""
    post, ym, Yp = got
    r_post, r_ym, r_Yp = ref
    k = slice(None) if keep is None else keep
    worst = [rows_err(post, r_post), rows_err(Yp[k], r_Yp[k]),
             rows_err(np.asarray(ym)[k].reshape(-1, 1), np.asarray(r_ym, dtype=F64)[k].reshape(-1, 1),
                      extra=np.max(np.abs(np.asarray(r_Yp, dtype=F64)[k]), axis=1))]
    assert max(worst) <= tol, "%s: a row is off by %.3g of its own tolerance (state, obs perturbations, obs means: %s)" % (
        what, max(worst) / tol, " ".join("%.3g" % w for w in worst))
    return max(worst)


def assert_diag_bits(got, want, what, obs=None):
    for key in DIAG:
        assert_same_bits(np.asarray(got[key]), np.asarray(want[key]), "%s: %s" % (what, key), rows=obs)


def others(rows, P=P):
    keep = np.ones(P, dtype=bool)
    keep[rows] = False
    return keep


def assert_own_priors(got, ref, rows, what):
    """The poisoned obs' own prior_mean and prior_var: the oracle's, NaN where it has NaN (and Inf where it has Inf)."""
    rv = np.asarray(ref["prior_var"], dtype=F64)[rows]
    spread = np.where(np.isfinite(rv), np.sqrt(np.abs(rv)), 0.0)
    for key, extra in (("prior_mean", spread), ("prior_var", 0.0)):
        g, r = np.asarray(got[key], dtype=F64)[rows], np.asarray(ref[key], dtype=F64)[rows]
        assert np.array_equal(np.isnan(g), np.isnan(r)), "%s: NaN pattern of the poisoned obs' %s: %r against %r" % (what, key, g, r)
        fin = np.isfinite(r)
        assert np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)]), "%s: the poisoned obs' %s" % (what, key)
        tol = RTOL * (np.abs(r) + extra)
        assert (np.abs(g[fin] - r[fin]) <= tol[fin]).all(), "%s: the poisoned obs' %s: %r against %r" % (what, key, g, r)


# ---------------------------------------------------------------------------
# Part D: zero spread
# ---------------------------------------------------------------------------
def zero_spread_rows():
    return np.unique(np.concatenate((SPECIAL, ZERO_RUN)))


def zero_spread_case(M, loc, flag=True):
    """Every member's estimate of the obs in `zero_spread_rows()` is 0.0 (no precipitation anywhere): Yp rows of exactly 0.0,
    R in [0.5, 2] as the case has it."""
    rows = zero_spread_rows()
    c = base_case(M, loc, flag, rows=rows)
    c["HX"][rows] = 0.0
    c["val"] = np.array(c["val"])
    c["val"][rows] = np.random.default_rng(77 + M).standard_normal(len(rows))
    assert (priors(c)[1][rows] == 0.0).all() and (c["err"][rows] >= 0.5).all()
    return c


# ---------------------------------------------------------------------------
# Part B: the outlier check
# ---------------------------------------------------------------------------
OUTLIER_T = 3.0


def outlier_case(M, loc, what):
    """(case with the special obs requested and poisoned, reference case with their flag 0 and clean values, ym, Yp of the
    poisoned case, ym, Yp of the reference).  what: "value", "error" (NaN there) or "row" (one NaN in the ob's Yp row: the
    reference has the same row)."""
    ref = base_case(M, loc, False)
    bad = dict(ref)
    bad["asm"] = np.array(ref["asm"])
    bad["asm"][SPECIAL] = True
    ym, Yp = priors(ref)
    if what == "row":
        Yp = poison_obs_rows(Yp, "one_nan")
    else:
        key = {"value": "val", "error": "err"}[what]
        bad[key] = np.array(ref[key])
        bad[key][SPECIAL] = np.nan
    return bad, ref, ym, Yp


# ---------------------------------------------------------------------------
# Part E: near-copy pairs at the cancellation guard's margin
# ---------------------------------------------------------------------------
# second obs of the pairs, by block: band positions 0..3 (rows 8, 13, 18, 23 of the block) and the block's row 63; one pair
# across 127 | 128, whose second ob starts block 2 -- the ratio restarts there, so it trips nothing
MARGIN_SECONDS = {0: (8, 13, 18, 23, 63), 1: (64 + 8, 64 + 13, 64 + 18, 64 + 23), 2: (128 + 13, 128 + 18, 128 + 23, 128 + 63)}
MARGIN_CROSS = (127, 128)
MARGIN_BANDS = {"safe": (SAFE, 2 * SAFE, (0, 1, 2)), "falls_back": (FALLS_BACK / 2, FALLS_BACK, (2,))}
MARGIN_M = (24, 100, 128)


def block_min_ratios(c, upto=None):
    """{block: min over its assimilated obs of var at the ob's step / var at block start} of the obs block alone."""
    n = c["P"] if upto is None else upto
    ym, Yp = orc.compute_ob_priors(c["HX"][:n])
    probe = GuardProbe(0, c["asm"][:n])
    kw = {}
    if c["loc"]:
        kw = dict(loc="GC", ob_lat=c["ob_lat"][:n], ob_lon=c["ob_lon"][:n], ob_halfwidth=c["hw"][:n], grid_lat=np.zeros((1, 0)),
                  grid_lon=np.zeros((1, 0)), state_shape=(1, 1, 1, 0), obs_taper="vector")
    orc.ensrf_update(ym, Yp, 0, c["val"][:n], c["err"][:n], c["asm"][:n], step_hook=probe, **kw)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(probe.var0 > 0, probe.var_step / probe.var0, 0.0)
    r = np.where(probe.asm, r, np.inf)
    return dict((b, float(r[b * ROWS_PER_BLOCK:(b + 1) * ROWS_PER_BLOCK].min())) for b in range((n + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK)), r


def margin_case(P, M, seed, lo, hi, blocks, loc=False):
    """Near-copy pairs HX[b+1] = HX[b] + 1e-3 noise, err[b] = q var(HX[b]), co-located under GC so that their taper is 1.  q is
    tuned pair by pair, in the obs' order, on the oracle of the obs block's prefix: the ratio of the pair's second ob is close to
    A (sqrt(q) - 1/(M-1))^2 (the reference divides the covariance by M-1 and the variance by M), A being what the block's
    earlier obs left of its variance (they also shrink the variance that q is relative to), so q is
    bracketed on the rising side and bisected; the pairs of `blocks` in [lo, hi], the others in [SAFE, 2 SAFE].  Returns the case with `q` (per pair) and `block_ratios`."""
    c = _random_case(seed, N, M, P, bool(loc), frac_assim=0.9, ncol=NCOL if loc else None)
    rng = np.random.default_rng(seed + 1)
    c["HX"], c["err"], c["asm"] = np.array(c["HX"]), np.array(c["err"]), np.array(c["asm"], dtype=bool)
    # fresh rows for the obs block: pairs must not also be copies of another ob through a shared state row
    c["HX"] = 3.0 * rng.standard_normal((P, M)) + rng.standard_normal((P, 1))
    c["val"] = c["HX"].mean(axis=1) + rng.standard_normal(P)
    pairs = sorted([(s - 1, s, s // ROWS_PER_BLOCK) for b in MARGIN_SECONDS for s in MARGIN_SECONDS[b]] +
                   [(MARGIN_CROSS[0], MARGIN_CROSS[1], None)])
    cm, q = 1.0 / (M - 1), {}
    for first, second, block in pairs:
        c["HX"][second] = c["HX"][first] + 1e-3 * rng.standard_normal(M)
        c["val"][second] = c["HX"][second].mean() + rng.standard_normal()
        c["asm"][[first, second]] = True
        if loc:
            for key in ("ob_lat", "ob_lon", "hw"):
                c[key] = np.array(c[key])
                c[key][second] = c[key][first]
        var = np.var(c["HX"][first])
        if block is None:                      # the pair across the block edge: as tight as the tightest, and harmless
            q[first] = (cm + np.sqrt(lo)) ** 2
            c["err"][first] = q[first] * var
            continue
        t_lo, t_hi = (lo, hi) if block in blocks else (SAFE, 2 * SAFE)
        # the ratio falls with q down to a minimum near 0 (where sqrt(q) meets 1/(M-1)) and rises again below it: walk q down
        # from the rising side's far end until the ratio is below the target, then bisect that bracket (geometrically)
        def ratio_at(qq):
            c["err"][first] = qq * var
            return block_min_ratios(c, upto=second + 1)[1][second]
        target = np.sqrt(t_lo * t_hi)
        q_hi = (cm + np.sqrt(target)) ** 2
        while ratio_at(q_hi) < target:
            q_hi *= 4.0
        q_lo = q_hi / 4.0
        while ratio_at(q_lo) > target:
            q_hi, q_lo = q_lo, q_lo / 4.0
        for _ in range(30):
            qq = np.sqrt(q_lo * q_hi)
            r = ratio_at(qq)
            if t_lo * 1.05 <= r <= t_hi / 1.05:
                break
            q_lo, q_hi = (qq, q_hi) if r < target else (q_lo, qq)
        else:
            raise AssertionError("margin_case: pair %d|%d did not reach [%g, %g]: %g" % (first, second, t_lo, t_hi, r))
        q[first] = qq
    c["q"], c["pairs"] = q, pairs
    c["block_ratios"], c["ratios"] = block_min_ratios(c)
    return c


MARGIN_CASES = [(name, M, loc) for name in MARGIN_BANDS for M in MARGIN_M for loc in (False, True)]
_MARGIN = {}


def margin(name, M, loc):
    """The case of Part E: generated once and shared."""
    if (name, M, loc) not in _MARGIN:
        lo, hi, blocks = MARGIN_BANDS[name]
        _MARGIN[name, M, loc] = margin_case(P_MARGIN, M, 61000 + M + 7 * int(loc) + len(name), lo, hi, blocks, loc)
    return _MARGIN[name, M, loc]


# ---------------------------------------------------------------------------
# Part F: rows that are not centred
# ---------------------------------------------------------------------------
def uncentred(Yp, cfac, rows=UNCENTRED_ROWS):
    Yp = np.array(Yp)
    for r in rows:
        Yp[r] = Yp[r] + cfac * np.std(Yp[r])
    return Yp


def oracle_obs_only(c, ym, Yp):
    """`orc.ensrf_update(ym, Yp, 0, ...)` on the arrays as given: np.var re-centres, np.dot does not."""
    kw = {}
    if c["loc"]:
        kw = dict(loc="GC", ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"], grid_lat=np.zeros((1, 0)),
                  grid_lon=np.zeros((1, 0)), state_shape=(1, 1, 1, 0), obs_taper="vector")
    return orc.ensrf_update(np.array(ym), np.array(Yp), 0, c["val"], c["err"], c["asm"], **kw)
