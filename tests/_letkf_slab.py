"""The LETKF under vertical, temporal and cross-variable localisation in NumPy, for the tests: tests/_letkf.py's
eigh-per-point solve with the horizontal taper multiplied by tests/_slabloc.py's factors.  Written from the definition.

Slab s of column c (row s*ncol + c) is solved under rho_k(c, s) = GC_h(c, k) * S(k, s), S = (V T) C of _slabloc.slab_factor_table;
obs row j under GC_h(j, k) * F(j, k), F(j, k) = (V(j,k) T(j,k)) C[k, v_j].  Slabs with equal keys share one solve: the key of slab
s is the bit pattern (every NaN alike) of lead_vert[s] while some ob has a vertical coordinate and half-width, lead_time[s] while
some ob has a time and a temporal half-width, lead_var[s] while some ob's impact row has an entry other than 1; groups are
numbered by first appearance.  A `loc` dict holds the settings: lead_vert, ob_vert, ob_vert_halfwidth, lead_time, ob_time,
ob_time_halfwidth, lead_var, ob_group, ob_var, impact (None where a part is absent)."""
import numpy as np

import _etkf
import _letkf
import _letkf_interp
import _slabloc
from _vertloc import vertical_factor

KEYS = ("lead_vert", "ob_vert", "ob_vert_halfwidth", "lead_time", "ob_time", "ob_time_halfwidth", "lead_var", "ob_group", "ob_var",
        "impact")


def _loc(loc):
    return {k: (loc or {}).get(k) for k in KEYS}


def slab_table(n_lead, P, loc):
    """S (P, n_lead)."""
    l = _loc(loc)
    return _slabloc.slab_factor_table(n_lead, P, l["lead_vert"], l["ob_vert"], l["ob_vert_halfwidth"], l["lead_time"], l["ob_time"],
                                      l["ob_time_halfwidth"], l["lead_var"], l["ob_group"], l["impact"])


def obs_factor(P, loc):
    """F (P, P): F[j, k] the factor of ob k on obs row j."""
    l = _loc(loc)
    _, ov, oc, _, ot, oh, _, og, ovar = _slabloc._arrays(1, P, None, l["ob_vert"], l["ob_vert_halfwidth"], None, l["ob_time"],
                                                         l["ob_time_halfwidth"], None, l["ob_group"], l["ob_var"])
    has_v = ~np.isnan(ov) & ~np.isnan(oc)
    ovj = np.where(has_v, ov, np.nan)       # an ob without vertical information takes factor 1 as a target too (7d)
    F = np.ones((P, P))
    for k in range(P):
        V = vertical_factor(ovj, ov[k], oc[k]) if has_v[k] else np.ones(P)
        F[:, k] = (V * _slabloc.temporal_factor(ot, ot[k], oh[k])) * _slabloc.impact_factor(l["impact"], og[k], ovar)
    return F


def _bits(a):
    a = np.array(a, dtype=np.float64).reshape(-1)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return b


def groups(n_lead, P, loc):
    """(group_of (n_lead,), rep (ngroups,)): the grouping rule, from the inputs that determine S."""
    l = _loc(loc)
    lv, ov, oc, lt, ot, oh, lvar, og, _ = _slabloc._arrays(n_lead, P, l["lead_vert"], l["ob_vert"], l["ob_vert_halfwidth"], l["lead_time"],
                                                           l["ob_time"], l["ob_time_halfwidth"], l["lead_var"], l["ob_group"], None)
    vert = l["lead_vert"] is not None and bool(np.any(~np.isnan(ov) & ~np.isnan(oc)))
    temporal = l["lead_time"] is not None and bool(np.any(~np.isnan(ot) & ~np.isnan(oh)))
    variable = False
    if l["impact"] is not None:
        C = np.asarray(l["impact"], dtype=np.float64)
        variable = any(g >= 0 and np.any(C[g] != 1.0) for g in og)
    kv = _bits(lv) if vert else np.zeros(n_lead, dtype=np.uint64)
    kt = _bits(lt) if temporal else np.zeros(n_lead, dtype=np.uint64)
    kc = lvar if variable else np.zeros(n_lead, dtype=np.int64)
    seen, group_of, rep = {}, np.zeros(n_lead, dtype=np.int64), []
    for s in range(n_lead):
        key = (int(kv[s]), int(kt[s]), int(kc[s]))
        if key not in seen:
            seen[key] = len(rep)
            rep.append(s)
        group_of[s] = seen[key]
    return group_of, np.array(rep, dtype=np.int64)


def point_weights(rho_h, S, rep, ym, Yp, value, error, assim, route=_letkf.solve_point):
    """T (ng, npts, M, M), w (ng, npts, M), stats (n_local, dfs, cond: (ng, npts)) at points of horizontal taper rho_h (npts, P)."""
    M, npts, ng = np.asarray(Yp).shape[1], rho_h.shape[0], len(rep)
    T, w = np.empty((ng, npts, M, M)), np.empty((ng, npts, M))
    st = dict(n_local=np.zeros((ng, npts), dtype=np.int64), dfs=np.zeros((ng, npts)), cond=np.ones((ng, npts)))
    for g in range(ng):
        rho = rho_h * S[:, rep[g]][None, :]
        for i in range(npts):
            out = route(rho[i], ym, Yp, value, error, assim)
            T[g, i], w[g, i] = out[0], out[1]
            if len(out) > 2:
                for key in st:
                    st[key][g, i] = out[2][key]
    return T, w, st


def _apply(X, ncol, group_of, T, w, reached):
    """Rows of slab s of column c through the pair (group_of[s], c); a (group, column) that is not reached keeps its rows."""
    X = np.asarray(X, dtype=np.float64)
    post = np.array(X)
    for g in range(T.shape[0]):
        slabs = np.flatnonzero(group_of == g)
        for c in range(ncol):
            if reached[g, c]:
                rows = slabs * ncol + c
                post[rows] = _etkf.etkf_members(X[rows], T[g, c], w[g, c])
    return post


def slab_cycle(X, HX, value, error, assim, ob_lat, ob_lon, ob_hw, grid_lat, grid_lon, n_lead, loc, stride=None, shape=None):
    """The whole cycle: posterior members, the posterior obs block, the diagnostics, the statistics per (group, column).  With
    `stride` (and the grid's `shape`): the pairs are solved at the nodes of tests/_letkf_interp.py's mesh and interpolated per group;
    the statistics, T and w are then the nodes'."""
    X = np.asarray(X, dtype=np.float64)
    M = X.shape[1]
    P = len(HX)
    ym, Yp = _etkf.ob_priors(HX) if P else (np.zeros(0), np.zeros((0, M)))
    glat = np.asarray(grid_lat, dtype=np.float64).reshape(-1)
    glon = np.asarray(grid_lon, dtype=np.float64).reshape(-1)
    ncol = glat.size
    S = slab_table(n_lead, P, loc)
    group_of, rep = groups(n_lead, P, loc)
    out = dict(S=S, group_of=group_of, rep=rep, prior_ym=ym, prior_Yp=Yp)
    if stride is None or tuple(stride) == (1, 1):
        rho_h = _letkf.taper(glat, glon, ob_lat, ob_lon, ob_hw, assim)
        T, w, st = point_weights(rho_h, S, rep, ym, Yp, value, error, assim)
        post = _apply(X, ncol, group_of, T, w, st["n_local"] > 0)
    else:
        m = _letkf_interp.mesh(shape[0], shape[1], stride)
        rho_h = _letkf.taper(glat[m["node_col"]], glon[m["node_col"]], ob_lat, ob_lon, ob_hw, assim)
        T, w, st = point_weights(rho_h, S, rep, ym, Yp, value, error, assim)
        Tc, wc = np.empty((len(rep), ncol, M, M)), np.empty((len(rep), ncol, M))
        reached = np.zeros((len(rep), ncol), dtype=bool)
        for g in range(len(rep)):
            Tc[g], wc[g], reached[g] = _letkf_interp.column_pairs(m, T[g], w[g], st["n_local"][g])
        post = _apply(X, ncol, group_of, Tc, wc, reached)
        out.update(mesh=m, reached=reached)
    # the obs block: ob j at its own position under the obs-obs factors
    rho_o = _letkf.taper(ob_lat, ob_lon, ob_lat, ob_lon, ob_hw, assim) * obs_factor(P, loc) if P else np.zeros((0, 0))
    yam, Yap = np.array(ym), np.array(Yp)
    for j in range(P):
        To, wo, ex = _letkf.solve_point(rho_o[j], ym, Yp, value, error, assim)
        if ex["n_local"]:
            a, b = _etkf.etkf_apply(ym[j:j + 1], Yp[j:j + 1], To, wo)
            yam[j], Yap[j] = a[0], b[0]
    a = np.asarray(assim, dtype=bool)
    diag = dict(prior_mean=np.array(ym), prior_var=np.var(Yp, axis=1) if P else np.zeros(0), post_mean=np.where(a, yam, np.nan),
                post_var=np.where(a, np.var(Yap, axis=1), np.nan) if P else np.zeros(0), assimilated=a)
    out.update(post=post, ym=yam, Yp=Yap, diag=diag, stats=st, T=T, w=w, rho_h=rho_h, rho_o=rho_o)
    return out


def make_case(M, P, ny, nx, nvars, ntimes, seed=0, parts="vtc", hw=(300.0, 3000.0)):
    """tests/_letkf.py's seeded case on nvars x ntimes slabs, with the settings of `parts` (v vertical, t temporal, c variable):
    one level per variable, valid times 6 apart, obtype g observes variable g.  Ob 0 has no vertical coordinate, ob 1 no time, ob 2
    an obtype that names no state variable and has no impact row (where P allows)."""
    c = _letkf.make_case(M, P, ny, nx, nvars * ntimes, seed=seed, hw=hw)
    rng = np.random.default_rng(7919 * M + 31 * P + 1000 * nvars + ntimes + seed)
    n_lead = nvars * ntimes
    levels = np.array([850.0, 500.0, 250.0])[:nvars]
    loc = {}
    if "v" in parts:
        loc["lead_vert"] = np.repeat(levels, ntimes)
        loc["ob_vert"] = rng.choice(levels, P) + rng.uniform(-60.0, 60.0, P)
        loc["ob_vert_halfwidth"] = rng.uniform(120.0, 600.0, P)
        if P > 3:
            loc["ob_vert"][0] = np.nan
    if "t" in parts:
        loc["lead_time"] = np.tile(6.0 * np.arange(ntimes), nvars)
        loc["ob_time"] = rng.uniform(0.0, 6.0 * max(ntimes - 1, 1), P)
        loc["ob_time_halfwidth"] = rng.uniform(2.5, 12.0, P)
        if P > 3:
            loc["ob_time"][1] = np.nan
    if "c" in parts:
        C = np.ones((nvars, nvars))
        for g in range(nvars):
            for v in range(nvars):
                if g != v:
                    C[g, v] = (0.0, 0.5, 0.25)[(g + v) % 3]
        loc["impact"] = C
        loc["lead_var"] = np.repeat(np.arange(nvars), ntimes)
        loc["ob_group"] = rng.integers(0, nvars, P)
        loc["ob_var"] = loc["ob_group"].copy()
        if P > 3:
            loc["ob_group"][2] = -1
            loc["ob_var"][2] = -1
    c.update(loc=loc, nvars=nvars, ntimes=ntimes, n_lead=n_lead)
    return c
