"""A taper probe: a synthetic Gaspari-Cohn cycle whose posterior gives back every (row, assimilated ob) taper weight separately.

The P probing obs (assimilate flag 1) have member perturbations y_k that are mutually orthogonal and zero-mean (the QR of a
centred random M x P matrix, P <= M - 1).  Every state row and every witness ob (flag 0) starts as mu + sum_k y_k.  Since
y_j . y_k = 0, ob k only ever changes the y_k component of a row, and no probing ob changes another probing ob's row.  With a the
posterior perturbations of a row,

    w(row, k) = (1 - (a . y_k) / (y_k . y_k)) / (beta_k K_k),      K_k = (y_k . y_k / (M - 1)) / (var_k + r_k),
    beta_k = 1 / (1 + sqrt(r_k / (var_k + r_k))),  var_k = y_k . y_k / M  (np.var, ensrf.py:135)

and the row's mean moves by sum_k w(row, k) K_k (value_k - mean_k): a second, independent reading of the same weights.

The yardstick is the reference's formulas (distance_to_point for state rows, haversine(ob k, witness) for the obs-obs taper, the
Gaspari-Cohn polynomial) evaluated in numpy.longdouble on the same float64 inputs; it takes nothing from the library or from the
float64 oracle.  Per pair, with a the haversine argument and R the Earth's radius,

    tol = 16 * 2^-52 * (M + (R / |hw_k|) / sqrt(1 - a))

M for the extraction's dot products, R/|hw| for a float64 `radians` difference in units of r, 1/sqrt(1 - a) for the conditioning
of atan2(sqrt(a), sqrt(1 - a)), 16 for a libm a few ulp from another.  The vertical factor adds nothing to it: r_v = |dz| / c is
two roundings from exact and the polynomial's slope is below 1, so its error is under 4 * 2^-52, inside the M term.
The mean increment of a row is held to sum_k tol(row, k) K_k |innov_k| + 16 * 2^-52 (|mu| + sum_k K_k |innov_k| + P), the last
term the rounding of a mean of M members of that size.

Pairs with 1 - a < 1e-6 (within 13 km of the antipode, where the reference's own formula is unstable and may return NaN) are left
out of the value comparison; they may be at most 0.1 % of a case's pairs.  Zero pattern, with tol_r = 1e-12 +
16 * 2^-52 (R / |hw|) / sqrt(1 - a): r >= 2 + tol_r must leave the pair exactly untouched, r <= 2 - 1e-2 must give w != 0.
"""
import functools

import numpy as np

R_KM = 6371.0
EPS = 2.0 ** -52
LD = np.longdouble
_PI180 = LD("3.14159265358979323846264338327950288") / LD(180)
NEAR_ANTIPODE = 1e-6
# 2 - 3e-3 and 2 - 8e-4: true weights 2.5e-11 and 3.4e-14.  A cheap rejection in sin^2(d/2R) that is too tight by 1e-3 drops the
# pairs beyond 2 - 1e-3 (the haversine argument goes with the square of the distance); the second point lies there and still
# carries a weight that float64 cannot lose (COUNTED below).
R_LIST = (0.0, 1e-9, 0.5, 1.0 - 1e-9, 1.0 + 1e-9, 1.5, 2.0 - 1e-2, 2.0 - 3e-3, 2.0 - 8e-4, 2.0 - 1e-9, 2.0 + 1e-9)
# A pair whose true horizontal weight is at least this must be COUNTED as non-zero by the list builder: the float64 polynomial's
# own rounding near r = 2 is about 1e-15 absolute (the outer branch sums terms of size 5), and an error tol_r of r moves the
# weight by 5 w tol_r / (2 - r), under 1e-17 here.  The extraction cannot see such a weight (it is below tol); the pair counts can.
COUNTED = 1e-14
FIXED_OBS = ((90.0, 0.0), (-90.0, 123.0), (0.0, 180.0), (10.0, 359.95))
# the wrap and antipode list of tests/test_oracle_golden.py::_taper_sets
WRAP_POINTS = ((10.0, 359.95), (10.0, 0.05), (10.0, -0.05), (-20.0, 179.9), (-20.0, -179.9), (-20.0, 540.1), (33.0, 0.0),
               (33.0, 360.0), (0.0, -180.0), (0.0, 180.0))
ANTIPODE_POINTS = ((45.0, 10.0), (-45.0, 190.0), (-45.0, 189.999999), (89.99, 0.0), (-89.99, 180.0))


def _rad(x):
    return np.asarray(x, dtype=LD) * _PI180


def gc_ld(r):
    """Gaspari-Cohn polynomial (observation.py:117-130) of r >= 0 in long double; 0 for r >= 2 and for NaN."""
    r = np.asarray(r, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        inner = ((((LD(-0.25) * r + LD(0.5)) * r + LD(0.625)) * r - LD(5) / LD(3)) * r * r + LD(1))
        outer = (((((r / LD(12) - LD(0.5)) * r + LD(0.625)) * r + LD(5) / LD(3)) * r - LD(5)) * r + LD(4) - LD(2) / (LD(3) * r))
    return np.where(r <= 1, inner, np.where(r < 2, outer, LD(0)))


def yardstick(row_lat, row_lon, ob_lat, ob_lon, ob_hw, kind):
    """(r, a, w) as long double (rows, P) arrays.  kind "state": EnsembleState.distance_to_point(row -> ob), ensemble.py:254-267;
    kind "obs": haversine(ob k, row), observation.py:135-146 (radians of the longitude DIFFERENCE)."""
    rla, rlo = np.asarray(row_lat, dtype=LD)[:, None], np.asarray(row_lon, dtype=LD)[:, None]
    ola, olo = np.asarray(ob_lat, dtype=LD)[None, :], np.asarray(ob_lon, dtype=LD)[None, :]
    if kind == "state":
        dlat = _rad(ola) - _rad(rla)
        dlon = _rad(olo) - _rad(rlo)
    else:
        dlat = _rad(rla) - _rad(ola)
        dlon = _rad(rlo - olo)
    a = np.sin(dlat / 2) ** 2 + np.cos(_rad(ola)) * np.cos(_rad(rla)) * np.sin(dlon / 2) ** 2
    a = np.minimum(a, LD(1))
    c = 2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a))
    r = LD(R_KM) * c / np.abs(np.asarray(ob_hw, dtype=LD))[None, :]
    return r, a, gc_ld(r)


def vertical_ld(z_row, z_ob, c_ob, c_row=None):
    """(rows, P) long double vertical factors: GC(|z_row - z_k| / c_k), 1 where a coordinate or ob k's half-width is NaN -- or,
    for a row that is itself an ob (c_row given), that ob's own half-width."""
    z_row, z_ob, c_ob = (np.asarray(v, dtype=np.float64) for v in (z_row, z_ob, c_ob))
    none = np.isnan(z_row)[:, None] | (np.isnan(z_ob) | np.isnan(c_ob))[None, :]
    if c_row is not None:
        none = none | np.isnan(np.asarray(c_row, dtype=np.float64))[:, None]
    with np.errstate(invalid="ignore"):
        v = gc_ld(np.abs(z_row.astype(LD)[:, None] - z_ob.astype(LD)[None, :]) / np.abs(c_ob.astype(LD))[None, :])
    return np.where(none, LD(1), v)


def _sphere(rng, n):
    return np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))), rng.uniform(-180.0, 180.0, n)


class Probe(object):
    """See the module docstring.  Obs block of PT = Q + P rows: Q // 2 witnesses, the P probing obs, the other witnesses.
    reach "regional": half-widths 200 .. 3000 km, one of 0.5 km and one of -800 km; "global": also 9000 km and 25 000 km.
    cluster: the random probing obs sit within a few degrees of each other, so that a column block near them lists nearly all.
    ncol: pad the columns with uniform points up to this number (None: the geometry's own points only).
    antipodes False: no column or witness within NEAR_ANTIPODE of a probing ob's antipode (cases under 10 000 pairs).
    n_lead > 1 adds vertical coordinates (some NaN): state row = lead * ncol + col, weight = horizontal x vertical."""

    def __init__(self, M, P, Q, reach="regional", seed=0, cluster=False, ncol=None, antipodes=True, n_lead=1):
        assert 5 <= P <= M - 1 and Q >= 8
        rng = np.random.default_rng(seed * 7919 + 1000003 * M + 1009 * P + Q)
        self.M, self.P, self.Q, self.n_lead, self.reach = M, P, Q, n_lead, reach
        # ---- probing obs
        nf = len(FIXED_OBS)
        if cluster:
            lat, lon = rng.uniform(40.0, 44.0, P), rng.uniform(250.0, 255.0, P)
        else:   # a sector 240 degrees wide across Greenwich and the dateline: the far side keeps rows that no regional ob reaches
            lat, lon = np.degrees(np.arcsin(rng.uniform(-0.95, 0.95, P))), rng.uniform(-40.0, 200.0, P)
        at = rng.permutation(P)
        for i, (la, lo) in enumerate(FIXED_OBS):
            lat[at[i]], lon[at[i]] = la, lo
        hw = rng.uniform(200.0, 3000.0, P)
        special = [0.5, -800.0] + ([9000.0, 25000.0] if reach == "global" else [])
        for i, h in enumerate(special):
            hw[at[(nf + i) % P]] = h
        # ---- points: per ob along its meridian towards the equator, the wrap / antipode list, the poles, uniform points
        plat, plon, forced = [], [], []
        for k in range(P):
            toward = -1.0 if lat[k] > 0 else 1.0
            for r in R_LIST:
                la = lat[k] + toward * np.degrees(r * abs(hw[k]) / R_KM)
                if abs(la) <= 90.0:
                    plat.append(la)
                    plon.append(lon[k] + (360.0 if k % 2 else 0.0))
                    # witnesses that do not depend on the draw: two obs' points just inside and just outside the cut-off
                    if len(forced) < 4 and abs(r - 2.0) < 2e-9 and 200.0 <= hw[k] <= 3000.0 and abs(la) < 80.0:
                        forced.append((la, lon[k]))
        assert len(forced) == 4
        for la, lo in WRAP_POINTS + ANTIPODE_POINTS + ((90.0, 17.0), (-90.0, 0.0), (90.0, 0.0), (-90.0, 200.0)):
            plat.append(la)
            plon.append(lo)
        ula, ulo = _sphere(rng, 120)
        plat, plon = np.concatenate([plat, ula]), np.concatenate([plon, ulo])
        if ncol is not None and ncol + Q > plat.size:     # (Q: four more than needed, the forced witnesses are extra)
            ela, elo = _sphere(rng, ncol + Q - plat.size)
            plat, plon = np.concatenate([plat, ela]), np.concatenate([plon, elo])
        if not antipodes:
            _, a, _ = yardstick(plat, plon, lat, lon, hw, "state")
            keep = ~np.any(1 - a < 2 * NEAR_ANTIPODE, axis=1)
            plat, plon = plat[keep], plon[keep]
        sh = rng.permutation(plat.size)
        plat, plon = plat[sh], plon[sh]
        # witnesses first in the shuffled order -- but a point near a probing ob's antipode becomes a column, except one where
        # the witnesses' pairs number 10 000 or more (the excluded pairs stay under 0.1 % whatever the draw)
        _, a, _ = yardstick(plat, plon, lat, lon, hw, "state")
        anti = np.any(1 - a < 2 * NEAR_ANTIPODE, axis=1)
        if Q * P >= 10000 and anti.any():
            anti[np.argmax(anti)] = False
        sh = np.concatenate([np.nonzero(~anti)[0], np.nonzero(anti)[0]])
        first = np.sort(sh[:Q - 4])
        sh = np.concatenate([first, np.setdiff1d(np.arange(plat.size), first)])
        plat, plon = plat[sh], plon[sh]
        # the forced witnesses: one ob's pair before the probing obs in the obs block, the other's after them
        fla, flo = np.array([f[0] for f in forced]), np.array([f[1] for f in forced])
        nq = Q - 4
        wlat, wlon = np.concatenate([fla[:2], plat[:nq], fla[2:]]), np.concatenate([flo[:2], plon[:nq], flo[2:]])
        self.grid_lat, self.grid_lon = np.ascontiguousarray(plat[nq:]), np.ascontiguousarray(plon[nq:])
        if ncol is not None:
            assert self.grid_lat.size >= ncol
            self.grid_lat, self.grid_lon = self.grid_lat[:ncol].copy(), self.grid_lon[:ncol].copy()
        self.ncol = self.grid_lat.size
        self.rows = n_lead * self.ncol
        # ---- the obs block
        Z = rng.standard_normal((M, P))
        Y, _ = np.linalg.qr(Z - Z.mean(axis=0))
        Y = (Y * (np.sqrt(M - 1.0) * rng.uniform(0.8, 1.25, P))).T.copy()          # (P, M), variance about 1
        Y -= Y.mean(axis=1, keepdims=True)
        self.Y = Y
        S = Y.sum(axis=0)
        S -= S.mean()
        q0 = Q // 2
        self.PT = PT = P + Q
        self.probe_idx = np.arange(q0, q0 + P)
        self.wit_idx = np.concatenate([np.arange(q0), np.arange(q0 + P, PT)])
        self.wit_before = np.arange(Q) < q0
        self.ob_lat, self.ob_lon, self.ob_hw = np.empty(PT), np.empty(PT), np.full(PT, 1234.5)
        self.ob_lat[self.probe_idx], self.ob_lon[self.probe_idx], self.ob_hw[self.probe_idx] = lat, lon, hw
        self.ob_lat[self.wit_idx], self.ob_lon[self.wit_idx] = wlat, wlon
        self.ob_assim = np.zeros(PT, dtype=np.uint8)
        self.ob_assim[self.probe_idx] = 1
        self.ym = rng.uniform(-5.0, 5.0, PT)
        self.Yp = np.empty((PT, M))
        self.Yp[self.probe_idx] = Y
        self.Yp[self.wit_idx] = S
        self.HX = self.ym[:, None] + self.Yp
        self.ob_value = self.ym + rng.uniform(-2.0, 2.0, PT)
        self.ob_error = rng.uniform(0.5, 2.0, PT)
        self.mu = rng.uniform(-5.0, 5.0, self.rows)
        self.X = self.mu[:, None] + S[None, :]
        # ---- vertical coordinates
        self.lead_vert = self.ob_vert = self.ob_vhw = None
        vs = vw = LD(1)
        if n_lead > 1:
            self.lead_vert = np.linspace(0.0, 2.0, n_lead)
            self.lead_vert[n_lead // 2] = np.nan
            self.ob_vert = rng.uniform(-0.3, 2.3, PT)
            self.ob_vhw = rng.uniform(0.6, 1.5, PT)
            self.ob_vert[self.probe_idx[0]] = np.nan
            self.ob_vhw[self.probe_idx[1]] = np.nan
            self.ob_vert[self.wit_idx[0]] = np.nan
            self.ob_vert[self.wit_idx[-1]] = np.nan
            self.ob_vhw[self.wit_idx[1]] = np.nan
            pk = self.probe_idx
            vs = np.repeat(vertical_ld(self.lead_vert, self.ob_vert[pk], self.ob_vhw[pk]), self.ncol, axis=0)
            vw = vertical_ld(self.ob_vert[self.wit_idx], self.ob_vert[pk], self.ob_vhw[pk], self.ob_vhw[self.wit_idx])
        # ---- the yardstick and the gains
        r, a, w = yardstick(self.grid_lat, self.grid_lon, lat, lon, hw, "state")
        self.state = dict(r=np.tile(r, (n_lead, 1)), a=np.tile(a, (n_lead, 1)), w=np.tile(w, (n_lead, 1)) * vs, v=vs,
                          wh=np.tile(w, (n_lead, 1)))
        r, a, w = yardstick(wlat, wlon, lat, lon, hw, "obs")
        self.obs = dict(r=r, a=a, w=w * vw, v=vw, wh=w)
        yy = (Y.astype(LD) ** 2).sum(axis=1)
        rk = self.ob_error[self.probe_idx].astype(LD)
        var = yy / M
        self.yy = yy
        self.K = (yy / (M - 1)) / (var + rk)
        self.beta = 1 / (1 + np.sqrt(rk / (var + rk)))
        self.innov = (self.ob_value[self.probe_idx] - self.ym[self.probe_idx]).astype(LD)
        self.hw = hw
        for v in self.__dict__.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)

    # ---- per-pair bounds --------------------------------------------------------------------------------------------
    def _geo(self, ref):
        a = ref["a"].astype(np.float64)
        with np.errstate(divide="ignore"):
            return (R_KM / np.abs(self.hw))[None, :] / np.sqrt(1.0 - a)

    def tol(self, ref):
        return 16 * EPS * (self.M + self._geo(ref))

    def tol_r(self, ref):
        return 1e-12 + 16 * EPS * self._geo(ref)

    def excluded(self, ref):
        return (1.0 - ref["a"].astype(np.float64)) < NEAR_ANTIPODE

    def far(self, ref):
        """Pairs that must be exactly untouched: r >= 2 + tol_r, or a vertical factor that is exactly 0."""
        far = ref["r"].astype(np.float64) >= 2.0 + self.tol_r(ref)
        if np.ndim(ref["v"]) == 2:
            far = far | np.asarray(ref["v"] == 0)
        return far

    def near(self, ref):
        """Pairs that must be touched: r <= 2 - 1e-2, away from the antipode (and, vertically, a factor that is not tiny)."""
        near = (ref["r"].astype(np.float64) <= 2.0 - 1e-2) & ~self.excluded(ref)
        if np.ndim(ref["v"]) == 2:
            near = near & np.asarray(ref["v"] > 1e-6)
        return near

    def counted(self, ref):
        """Pairs a count of non-zero weights must include: the issue's r <= 2 - 1e-2, and every true weight >= COUNTED."""
        return self.near(ref) | ((ref["wh"].astype(np.float64) >= COUNTED) & ~self.excluded(ref))

    def untouched_rows(self, ref):
        return np.all(self.far(ref), axis=1)

    def pair_count_bounds(self, cols=None):
        """(lo, hi) for a count of (column, ob) pairs with a non-zero horizontal taper over columns `cols` (default: all)."""
        ref = dict((k, v[:self.ncol] if np.ndim(v) == 2 else v) for k, v in self.state.items())
        ref["v"] = LD(1)
        near, far = self.counted(ref), self.far(ref)
        if cols is not None:
            near, far = near[cols], far[cols]
        return int(near.sum()), int((~far).sum())

    # ---- extraction -------------------------------------------------------------------------------------------------
    def extract(self, post_perts):
        """w (rows, P) from posterior perturbations (rows, M), in long double."""
        c = np.dot(np.asarray(post_perts, dtype=LD), self.Y.T.astype(LD))
        return (1 - c / self.yy[None, :]) / (self.beta * self.K)[None, :]

    def check(self, what, ref, post_mean, post_perts, prior_mean, cap=1.0, need_cut=False):
        """Assert the weights, the mean increments and the zero pattern of posterior rows against `ref` (self.state or
        self.obs); prints and returns the worst weight and mean err / tol, the excluded-pair count and the near-cut-off pair
        count (need_cut: the case must have such pairs).  A far pair in a row that other obs touch carries those updates' rounding in its y_k component, so per pair
        "untouched" is |w| <= tol here; exactness is asserted on whole rows (`assert_untouched`) and through the pair counts."""
        post_perts = np.asarray(post_perts, dtype=np.float64)
        post_perts = post_perts - post_perts.astype(LD).mean(axis=1, keepdims=True).astype(np.float64)
        assert np.all(np.isfinite(post_perts)) and np.all(np.isfinite(post_mean)), what + ": non-finite posterior"
        w = self.extract(post_perts)
        tol, excl, far, near = self.tol(ref), self.excluded(ref), self.far(ref), self.near(ref)
        n_pairs = excl.size
        n_excl = int(excl.sum())
        assert n_excl * 1000 <= n_pairs, "%s: %d of %d pairs near an antipode (over 0.1 %%)" % (what, n_excl, n_pairs)
        err = np.abs((w - ref["w"]).astype(np.float64))
        ratio = np.where(excl, 0.0, err / tol)
        worst = float(ratio.max())
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        # the mean increment, on rows without an excluded pair
        gain = (self.K * self.innov)[None, :]
        inc_ref = (ref["w"] * gain).sum(axis=1)
        inc_tol = (tol * np.abs(gain).astype(np.float64)).sum(axis=1) + 16 * EPS * (
            np.abs(prior_mean) + float(np.abs(gain).sum()) + self.P)
        inc = np.asarray(post_mean, dtype=LD) - np.asarray(prior_mean, dtype=LD)
        rows_ok = ~excl.any(axis=1)
        mratio = np.where(rows_ok, np.abs((inc - inc_ref).astype(np.float64)) / inc_tol, 0.0)
        mworst = float(mratio.max())
        cut = int(((np.abs(ref["r"].astype(np.float64) - 2.0) < 1e-2) & ~far & ~near).sum())
        still = self.untouched_rows(ref)
        print("%s: worst weight err/tol %.4f (row %d, ob %d: r %.12g, w %.6e), worst mean err/tol %.4f, %d of %d pairs excluded, "
              "%d pairs near the cut-off, %d of %d rows untouched" % (
                  what, worst, at[0], at[1], float(ref["r"][at]), float(ref["w"][at]), mworst, n_excl, n_pairs, cut,
                  int(still.sum()), still.size))
        assert cut > 0 or not need_cut, what + ": no pair between 2 - 1e-2 and 2 + tol_r half-widths (the meridian points are gone)"
        assert worst <= cap, "%s: weight of (row %d, ob %d) off by %.3f tol" % (what, at[0], at[1], worst)
        assert mworst <= cap, "%s: mean increment of row %d off by %.3f tol" % (what, int(mratio.argmax()), mworst)
        # zero pattern: the y_k component of a far pair keeps its coefficient 1 (exactly, when the whole row is untouched)
        wf = w.astype(np.float64)
        assert np.all(wf[near] != 0.0), "%s: %d pairs inside 2 - 1e-2 half-widths have weight 0" % (
            what, int((wf[near] == 0.0).sum()))
        assert np.all(np.abs(wf[far]) <= tol[far]), what + ": a pair beyond the cut-off was touched"
        return worst, mworst, n_excl, cut

    def assert_untouched(self, what, ref, *prior_post):
        """Rows whose every pair lies beyond the cut-off are bit-identical to the prior in every (prior, post) array pair given."""
        still = self.untouched_rows(ref)
        assert still.any(), what + ": the case has no untouched row"
        for prior, post in prior_post:
            prior, post = np.asarray(prior), np.asarray(post)
            assert prior.shape == post.shape and prior.shape[0] == still.size
            assert np.array_equal(prior[still], post[still]), "%s: %d untouched rows changed" % (
                what, int(np.any((prior[still] != post[still]).reshape(int(still.sum()), -1), axis=1).sum()))
        return int(still.sum())

    def block_bounds(self):
        """Per block of 16 columns: (pairs_lo, pairs_hi, obs_lo, obs_hi), the bounds of efa_gc_block_counts' block_pairs and
        block_count (the length of the block's active list).  The lower side counts `counted` pairs: at least the pairs with
        r <= 2 - 1e-2, so a count within these bounds is within the wider ones too."""
        ref = dict((k, v[:self.ncol] if np.ndim(v) == 2 else v) for k, v in self.state.items())
        ref["v"] = LD(1)
        near, live = self.counted(ref), ~self.far(ref)
        assert np.all(near >= self.near(ref)) and np.all(live >= near)
        nblk = (self.ncol + 15) // 16
        pad = nblk * 16 - self.ncol
        near = np.vstack([near, np.zeros((pad, self.P), bool)]).reshape(nblk, 16, self.P)
        live = np.vstack([live, np.zeros((pad, self.P), bool)]).reshape(nblk, 16, self.P)
        return (near.sum(axis=(1, 2)), live.sum(axis=(1, 2)), near.any(axis=1).sum(axis=1), live.any(axis=1).sum(axis=1))


# the geometries the GPU tests use (tests/test_gpu_taper_geometry.py); tests/test_taper_probe_host.py runs every one of them
# through the float64 oracle.  Cases under 10 000 pairs carry no near-antipodal point.
CASES = {
    "lane-regional": dict(M=64, P=40, Q=60, reach="regional"),
    "lane-global": dict(M=64, P=40, Q=60, reach="global"),
    "odd-regional": dict(M=21, P=20, Q=33, reach="regional", antipodes=False),
    "odd-global": dict(M=21, P=20, Q=33, reach="global", antipodes=False),
    "wide-regional": dict(M=256, P=200, Q=100, reach="regional"),
    "wide-global": dict(M=256, P=200, Q=100, reach="global"),
    "cluster": dict(M=256, P=200, Q=100, reach="regional", cluster=True),
    "obsobs": dict(M=100, P=64, Q=40, reach="global"),
    "cap": dict(M=64, P=40, Q=60, reach="global", ncol=16437),
    "vertical": dict(M=64, P=40, Q=60, reach="global", n_lead=3),
    "vertical-regional": dict(M=64, P=40, Q=60, reach="regional", n_lead=3),
    "tiny": dict(M=7, P=5, Q=20, reach="regional", antipodes=False),
}


@functools.lru_cache(maxsize=None)
def get_probe(name):
    return Probe(**CASES[name])
