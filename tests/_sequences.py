"""Plans of EnSRF cycles for ONE context, and the model every step is checked against (NumPy only, no GPU).

A plan is a list of steps made from (seed, length) with np.random.default_rng: the same arguments give the same plan on any
machine.  A step is a dict that holds everything one cycle needs -- the case (test_gpu_parity._random_case), what it keeps from
the step before it, the features of include/efa_hip.h that are on, the options, the entry point and the stream -- so that a
directed test can write its own steps with `make_step` and run them through the same executor
(tests/test_gpu_context_sequences.py).

`model(step)` composes what the suite already trusts and nothing else, in the order DESIGN.md 7b-7e gives: prior inflation
(_anderson2009.inflate), forward operator (the rows the obs were drawn from), outlier decision against the inflated obs block
(_outlier.masked_flags), the serial loop (oracle.ensrf_update unlocalised, _vertloc.ensrf_update_vert localised -- bit-identical
to the oracle without vertical information --, _anderson2009.cycle for the inflation field), relaxation of the state rows only
(test_relaxation_host.relax)."""
import hashlib

import numpy as np

import _anderson2009 as a09
import _outlier
import _vertloc
from oracle import ensrf_oracle as orc
from test_gpu_parity import _random_case
from test_relaxation_host import relax

M_VALUES = [2, 3, 4, 10, 20, 40, 64, 100, 104, 128, 129, 136, 137, 256]
P_VALUES = [0, 1, 2, 17, 63, 64, 65, 128, 129, 200, 300]
KEEP_KINDS = ["new", "values", "ob_moved", "flag", "radius", "grid", "n_lead"]
# entry points: efa_ensrf_update (augmented host arrays) / efa_ensrf_update_dev (perturbation form) / obs phase + state phase in
# place and out of place / obs phase + efa_state_cycle_dev / efa_ensrf_cycle_dev in place and on disjoint buffers (speculated)
ENTRIES = ["host", "update_dev", "phases_in", "phases_out", "state_cycle", "cycle_in", "cycle_out"]
# Phase-A kinds as the suite names them: (option "pipeline", option "gram")
PHASE_A = {"band": (1, 2), "gram": (1, 1), "chain": (1, 0), "batch": (0, 2)}
OBS_BATCH = [1, 7, 32, 64]
STREAMS = ["own", "caller", "null"]
RELAX = [None, ("rtps", 0.5), ("rtps", 0.0), ("rtps", 1.7), ("rtpp", 0.3), ("rtpp", 1.0), ("rtpp", 0.0)]
QC = [None, 3.0, 1e6]           # off, the usual threshold, one that rejects nothing
FEATURES = ["relax", "qc", "ai", "vl"]
# refusals (EFA_ERR_INVALID, decided on the host before anything is launched).  Before the context changes: vertical
# localisation set and an unlocalised cycle / another P; an adaptive field with other rows; state_cycle with another M than the
# obs phase; gc_onepass 0 with either.  After obs_phase began to change it: a requested GC ob with a NaN half-width.
REFUSALS = ["vl_unloc", "vl_other_p", "ai_rows", "state_cycle_m", "onepass0_vl", "onepass0_ai", "nan_hw"]
BIG_P = 16500                   # beyond one persistent Phase-A launch (256 workgroups x 64 rows)
REDRAW_MAX = 3


# ---- cases --------------------------------------------------------------------------------------------------------------------
def _rows_of(seed, N, M, P):
    """The state rows _random_case(seed, ...) drew its obs from (its first three draws), checked by the caller."""
    rng = np.random.default_rng(seed)
    rng.standard_normal((N, 1))
    rng.standard_normal((N, M))
    return rng.choice(N, P, replace=(P > N))


def new_case(seed, N, M, P, loc, frac_assim=0.9, ncol=None):
    c = _random_case(seed, N, M, P, loc, frac_assim=frac_assim, ncol=ncol)
    c["rows"] = _rows_of(seed, N, M, P)
    assert np.array_equal(c["X"][c["rows"]], c["HX"])
    c["asm"] = np.asarray(c["asm"], dtype=bool)
    if not loc:
        c["n_lead"] = 1
    return c


def revalue(c, rng, N=None):
    """The same geometry with a new state, new obs values and new error variances (N: on another number of rows)."""
    c = dict(c)
    N = c["N"] if N is None else N
    M, P = c["M"], c["P"]
    c["N"] = N
    c["X"] = rng.standard_normal((N, 1)) + 3.0 * rng.standard_normal((N, M))
    c["rows"] = rng.choice(N, P, replace=(P > N))
    c["HX"] = c["X"][c["rows"]]
    c["val"] = c["HX"].mean(axis=1) + rng.standard_normal(P)
    c["err"] = rng.uniform(0.5, 2.0, P)
    return c


def vertical(rng, n_lead, P, kind="full"):
    """(lead_vert, ob_vert, ob_vert_halfwidth): "nan" carries no vertical information at all (bit-identical to off)."""
    if kind == "nan":
        return np.full(n_lead, np.nan), np.full(P, np.nan), np.full(P, np.nan)
    lead = np.linspace(0.0, 3.0, n_lead)
    if n_lead > 2:
        lead[n_lead // 2] = np.nan
    ov = rng.uniform(-0.3, 3.3, P)
    if P:
        ov[0] = np.nan
    return lead, ov, 0.9 * rng.uniform(0.7, 1.3, P)


def inflation_field(rng, N):
    lam = 1.0 + 0.5 * (1.0 + np.sin(0.37 * np.arange(N) + rng.uniform(0, 6.28)))
    lam[::5] = 1.0
    return np.stack([lam, np.full(N, 0.6)], axis=1)


def make_step(case, keep="new", relax=None, qc=None, ai=None, vl=None, path=0, obs_batch=64, phase_a="band", gc_onepass=1,
              geometry_reuse=1, timing=0, entry="cycle_out", stream="own", obs_block_out=True, refusal=None, seed=0, index=0):
    """One step.  relax: None or ("rtps" | "rtpp", alpha); qc: None or the threshold; ai: None or dict(field (N, 2), lower,
    upper, sd_lower); vl: None or (lead_vert, ob_vert, ob_vert_halfwidth)."""
    s = dict(case=case, keep=keep, relax=relax, qc=qc, ai=ai, vl=vl, path=path, obs_batch=obs_batch, phase_a=phase_a,
             gc_onepass=gc_onepass, geometry_reuse=geometry_reuse, timing=timing, entry=entry, stream=stream,
             obs_block_out=obs_block_out, refusal=refusal, seed=seed, index=index, redraws=0)
    check_legal(s)
    return s


def describe(s):
    c = s["case"]
    f = []
    if s["relax"]:
        f.append("%s=%g" % s["relax"])
    if s["qc"]:
        f.append("qc=%g" % s["qc"])
    if s["ai"]:
        f.append("ai[%g,%g,%g]" % (s["ai"]["lower"], s["ai"]["upper"], s["ai"]["sd_lower"]))
    if s["vl"]:
        f.append("vl(nan)" if np.all(np.isnan(s["vl"][0])) else "vl")
    return "step %d %s%s loc=%d N=%d M=%d P=%d n_lead=%d entry=%s path=%d batch=%d %s onepass=%d reuse=%d timing=%d stream=%s [%s]" % (
        s["index"], s["keep"], " REFUSAL " + s["refusal"] if s["refusal"] else "", bool(c["loc"]), c["N"], c["M"], c["P"],
        c["n_lead"], s["entry"], s["path"], s["obs_batch"], s["phase_a"], s["gc_onepass"], s["geometry_reuse"], s["timing"],
        s["stream"], " ".join(f) or "plain")


def check_legal(s):
    """The rules of include/efa_hip.h a valid step obeys (a refusal step breaks exactly the one it names)."""
    c = s["case"]
    assert s["entry"] in ENTRIES and s["phase_a"] in PHASE_A and s["obs_batch"] in OBS_BATCH and s["stream"] in STREAMS
    assert s["path"] in (0, 1, 2) and s["timing"] in (0, 1, 2) and s["gc_onepass"] in (0, 1) and s["geometry_reuse"] in (0, 1)
    assert 2 <= c["M"] <= 256 and c["P"] >= 0 and c["N"] >= 0
    if s["relax"]:
        kind, alpha = s["relax"]
        # "alpha < 0 or (RTPP) alpha > 1 return EFA_ERR_INVALID"
        assert kind in ("rtps", "rtpp") and alpha >= 0 and (kind == "rtps" or alpha <= 1)
    if s["qc"] is not None:
        assert np.isfinite(s["qc"]) and s["qc"] > 0     # "a negative, NaN or infinite threshold fails"
    if s["refusal"]:
        assert s["refusal"] in REFUSALS
        return
    if c["loc"]:
        assert c["N"] == c["n_lead"] * c["lat"].size    # "i = lead*ncol + col"
        assert np.all(np.isfinite(c["hw"][c["asm"]])) and np.all(c["hw"][c["asm"]] != 0)
    else:
        assert s["gc_onepass"] == 1 and c["n_lead"] == 1
    if s["ai"]:
        # "The call fails unless the cycle is GC-localised, option gc_onepass is 1 and the state phase has `rows` rows"
        assert c["loc"] and s["gc_onepass"] == 1 and s["ai"]["field"].shape == (c["N"], 2)
        assert 0 < s["ai"]["lower"] <= s["ai"]["upper"] < np.inf and s["ai"]["sd_lower"] >= 0
        assert s["vl"] is None                          # "... and no adaptive-inflation field is set"
    if s["vl"]:
        # "a later call fails unless it is a GC cycle of exactly P observations (and n_lead slabs for the state phase),
        # option gc_onepass is 1"
        lead, ov, oh = s["vl"]
        assert c["loc"] and s["gc_onepass"] == 1 and lead.shape == (c["n_lead"],) and ov.shape == oh.shape == (c["P"],)
        assert np.all(np.isnan(oh) | ((oh > 0) & np.isfinite(oh))) and not np.any(np.isinf(lead)) and not np.any(np.isinf(ov))


def forward(c):
    """The linear forward operator of a case on member rows: the rows the obs were drawn from, or the case's own "H"."""
    rows = c["rows"]
    return c.get("H") or (lambda Z: Z[rows])


def golden_case(g):
    """A stored reference case (conftest.load_golden) as a case of this module: 2-D grid, its stencil as forward operator."""
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    idx, wts = g["sten_idx"], g["sten_wts"]
    c = dict(X=g["X"].reshape(N, M).copy(), HX=g["HX"].copy(), val=g["ob_value"].copy(), err=g["ob_error"].copy(),
             asm=np.asarray(g["ob_assim"], dtype=bool), N=N, M=M, P=len(g["ob_value"]), loc=g["loc"] == "GC", n_lead=nvar * nt,
             rows=idx[:, 0], H=lambda Z: (wts[:, :, None] * Z[idx]).sum(axis=1))
    if c["loc"]:
        c.update(lat=g["grid_lat"], lon=g["grid_lon"], ny=ny, nx=nx, ob_lat=g["ob_lat"], ob_lon=g["ob_lon"], hw=g["ob_radius"],
                 state_shape=(nvar, nt, ny, nx))
    else:
        c["n_lead"] = 1
    return c


# ---- the model ----------------------------------------------------------------------------------------------------------------
def prior_and_obs(s):
    """(the prior the cycle is given: inflated if an adaptive field is set, its obs estimates HX)."""
    c = s["case"]
    if not s["ai"]:
        return c["X"], c["HX"]
    Xi = a09.inflate(c["X"], s["ai"]["field"][:, 0])
    return Xi, forward(c)(Xi)


def flags(s, HX=None):
    """The assimilate flags the outlier check leaves."""
    c = s["case"]
    if s["qc"] is None or c["P"] == 0:
        return c["asm"]
    return _outlier.masked_flags(prior_and_obs(s)[1] if HX is None else HX, c["val"], c["err"], c["asm"], s["qc"])


def clear(s):
    """Every requested ob's outlier ratio at least 1e-6 (relative) away from the threshold."""
    c = s["case"]
    if s["qc"] is None or c["P"] == 0:
        return True
    ym, Yp = orc.compute_ob_priors(prior_and_obs(s)[1])
    a = c["asm"]
    return _outlier.clear_of_threshold(ym[a], Yp[a], c["val"][a], c["err"][a], s["qc"])


def model(s):
    """dict(post (N, M) posterior members, xam, Xap (augmented posterior mean / perturbations before relaxation; None with an
    adaptive field and relaxation does not touch them), ym, Yp (final obs block), diag, field (new inflation field or None),
    prior (what the cycle was given))."""
    c = s["case"]
    N, M, P = c["N"], c["M"], c["P"]
    Xi, HX = prior_and_obs(s)
    asm = flags(s, HX)
    taper = "loop" if P <= 128 else "vector"
    xbm, Xbp = orc.format_prior_state(Xi, HX)
    field = None
    if not c["loc"]:
        xam, Xap, diag = orc.ensrf_update(xbm, Xbp, N, c["val"], c["err"], asm)
        post = orc.format_posterior_state(xam, Xap, N)
    else:
        shape = c.get("state_shape", (c["n_lead"], 1, c["ny"], c["nx"]))
        vl = s["vl"] or (None, None, None)
        if s["ai"]:
            taper = "vector"     # (what _anderson2009.cycle runs its oracle with)
        xam, Xap, diag = _vertloc.ensrf_update_vert(xbm, Xbp, N, c["val"], c["err"], asm, c["ob_lat"], c["ob_lon"], c["hw"],
                                                    c["lat"], c["lon"], shape, lead_vert=vl[0], ob_vert=vl[1],
                                                    ob_vert_halfwidth=vl[2], obs_taper=taper)
        post = orc.format_posterior_state(xam, Xap, N)
        if s["ai"]:
            a = s["ai"]
            post2, field, diag2, _ = a09.cycle(Xi, forward(c), c["val"], c["err"], asm, c["ob_lat"], c["ob_lon"], c["hw"],
                                               c["lat"], c["lon"], shape, a["field"], lower=a["lower"], upper=a["upper"],
                                               sd_lower=a["sd_lower"], prior_inflated=True)
            assert np.array_equal(post2, post) and np.array_equal(diag2["assimilated"], diag["assimilated"])
    if s["relax"]:
        post = relax(Xi, post, **{s["relax"][0]: s["relax"][1]})
    return dict(post=post, xam=xam, Xap=Xap, ym=xam[N:], Yp=Xap[N:], diag=diag, field=field, prior=Xi)


# ---- plans --------------------------------------------------------------------------------------------------------------------
def _entry_cycle():
    """A cyclic order of the entry points in which every ordered pair (a, b), a == b included, is adjacent once: the Euler
    circuit of the complete directed graph with loops (Hierholzer)."""
    n = len(ENTRIES)
    nxt = [0] * n
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            out.append(stack.pop())
    return [ENTRIES[i] for i in out[::-1][:-1]]


ENTRY_CYCLE = _entry_cycle()


def _draw_shape(rng, loc, big):
    M = int(rng.choice(M_VALUES))
    P = int(rng.choice(P_VALUES))
    if big:          # sizes grow and shrink along a plan: a big case makes the workspaces re-allocate, small ones reuse them
        M = max(M, int(rng.choice([104, 128, 137, 256])))
        P = max(P, int(rng.choice([129, 200, 300])))
    if loc:
        n_lead = int(rng.integers(1, 5))
        ncol = int(rng.integers(150, 400)) if big else int(rng.integers(17, 150))
        return n_lead * ncol, M, P, n_lead, ncol
    return (int(rng.integers(800, 2000)) if big else int(rng.integers(1, 800))), M, P, 1, None


def _draw_features(rng, c, prev, only=None, none=False, keep="new"):
    """Features in the combinations the header allows.  only: exactly that feature on; none: all off."""
    f = dict(relax=None, qc=None, ai=None, vl=None, gc_onepass=1)
    if none:
        return f
    P, N = c["P"], c["N"]
    want = {k: (k == only if only else rng.random() < 0.4) for k in FEATURES}
    if not only and keep != "new" and prev is not None and prev["vl"] is not None and rng.random() < 0.7:
        want.update(vl=True, ai=False)       # stay on it: re-set to identical values, or only the half-widths changed
    if want["relax"]:
        f["relax"] = RELAX[1 + int(rng.integers(len(RELAX) - 1))]
    if want["qc"]:
        f["qc"] = QC[1 + int(rng.integers(len(QC) - 1))]
    if c["loc"]:
        if want["ai"] and (only == "ai" or not want["vl"] or rng.random() < 0.5):
            lo, up, sl = [(1.0, 1e6, 0.0), (0.8, 1.5, 0.0), (1.0, 3.0, 0.3)][int(rng.integers(3))]
            f["ai"] = dict(field=inflation_field(rng, N), lower=lo, upper=up, sd_lower=sl)
        elif want["vl"]:
            pv = prev["vl"] if prev is not None and prev["vl"] is not None else None
            same_geo = pv is not None and pv[0].shape == (c["n_lead"],) and pv[1].shape == (P,)
            r = rng.random()
            if same_geo and r < 0.3:
                f["vl"] = tuple(a.copy() for a in pv)                  # re-set to identical values
            elif same_geo and r < 0.6 and not np.all(np.isnan(pv[2])):
                f["vl"] = (pv[0].copy(), pv[1].copy(), pv[2] * rng.uniform(0.5, 1.5))  # half-widths only
            else:
                f["vl"] = vertical(rng, c["n_lead"], P, "nan" if r > 0.85 else "full")
        if f["ai"] is None and f["vl"] is None and rng.random() < 0.3:
            f["gc_onepass"] = 0
    return f


def _refusal_step(rng, kind, prev, seed, index):
    """A small case of its own with exactly the one rule broken that `kind` names."""
    loc = kind != "vl_unloc"
    n_lead, ncol = 2, 40
    N, M, P = (n_lead * ncol if loc else 90), 20, 30
    c = new_case(int(rng.integers(1 << 30)), N, M, P, loc, ncol=ncol if loc else None)
    kw = dict(keep="new", refusal=kind, entry="cycle_out", seed=seed, index=index)
    if kind in ("vl_unloc", "vl_other_p", "onepass0_vl"):
        # vl_unloc: set for 30 obs and 1 slab, then an unlocalised cycle; vl_other_p: set for P + 1 obs
        kw["vl"] = vertical(rng, c["n_lead"], P + (1 if kind == "vl_other_p" else 0))
    if kind in ("ai_rows", "onepass0_ai"):
        kw["ai"] = dict(field=inflation_field(rng, N + (ncol if kind == "ai_rows" else 0)), lower=1.0, upper=1e6, sd_lower=0.0)
    if kind in ("onepass0_vl", "onepass0_ai"):
        kw["gc_onepass"] = 0
    if kind == "state_cycle_m":
        kw["entry"] = "state_cycle"
    if kind == "nan_hw":
        c["hw"] = c["hw"].copy()
        c["asm"] = c["asm"].copy()
        c["asm"][P // 2] = True
        c["hw"][P // 2] = np.nan
        kw["entry"] = "state_cycle"
    return make_step(c, **kw)


def _plain_loc(i):
    """Whether the plain step at position i is localised: over 48 steps every feature is followed by both kinds."""
    return bool((i // 24 + i // 6) % 2 == 1)


def _choose_keep(sub, prev, i, only, plain, zero_at):
    """What step i keeps from the step before it: a draw, then brought down to what the previous case allows."""
    keep = KEEP_KINDS[int(sub.integers(len(KEEP_KINDS)))]
    if prev is None or i == zero_at:
        return "new"
    pc = prev["case"]
    if pc["P"] == BIG_P or pc["N"] == 0:                       # nothing to build on
        return "new"
    if only and (not pc["loc"] or pc["P"] == 0):               # a feature step is a GC cycle with obs
        return "new"
    if plain and pc["loc"] != _plain_loc(i):
        return "new"
    if keep != "new" and keep not in ("values", "flag") and not pc["loc"]:   # no positions, radii, grid or slabs without GC
        keep = "values"
    if keep in ("ob_moved", "flag", "radius") and pc["P"] == 0:
        keep = "values"
    return keep


def _fresh_case(sub, i, only, plain, zero_at):
    """Everything new: sizes that grow and shrink along the plan; at zero_at a shard that owns no row at all."""
    loc = True if only else _plain_loc(i) if plain else bool(sub.random() < 0.6) and i != zero_at
    N, M, P, n_lead, ncol = _draw_shape(sub, loc, big=bool(sub.random() < 0.35))
    if only and P == 0:
        P = 17
    fa = float(sub.choice([0.0, 0.5, 0.9, 1.0], p=[0.06, 0.24, 0.4, 0.3]))
    if i == zero_at:
        c = new_case(int(sub.integers(1 << 30)), 5, M, P, False, frac_assim=fa)
        c.update(X=c["X"][:0], N=0)
        return c
    return new_case(int(sub.integers(1 << 30)), N, M, P, loc, frac_assim=fa, ncol=ncol)


def _kept_case(sub, pc, keep):
    """The previous case with new values, errors and state, and the one thing `keep` names changed."""
    n_lead = pc["n_lead"]
    if keep == "n_lead":
        n_lead = int(sub.choice([v for v in (1, 2, 3, 4, 6) if v != pc["n_lead"]]))
    c = revalue(pc, sub, N=(pc["N"] // pc["n_lead"]) * n_lead if pc["loc"] else pc["N"])
    c["n_lead"] = n_lead
    k = int(sub.integers(max(c["P"], 1)))
    if keep == "ob_moved":
        c["ob_lat"] = c["ob_lat"].copy()
        c["ob_lat"][k] += sub.uniform(-5, 5)
    elif keep == "flag":
        c["asm"] = c["asm"].copy()
        c["asm"][k] = not c["asm"][k]
    elif keep == "radius":
        c["hw"] = c["hw"].copy()
        c["hw"][k] *= sub.uniform(0.2, 3.0)
    elif keep == "grid":
        c["lon"] = (c["lon"] + sub.uniform(-2, 2)) % 360.0
    return c


def _gross_errors(sub, c, f, i):
    """With the usual threshold on: sometimes every requested ob a gross error (all rejected), sometimes three of them."""
    if not (f["qc"] == 3.0 and c["P"] and c["asm"].any()):
        return
    n = int(c["asm"].sum()) if sub.random() < 0.2 else 3 if sub.random() < 0.5 else 0
    if n:
        c["val"], _ = _outlier.inject(prior_and_obs(dict(case=c, ai=f["ai"]))[1], c["val"], c["err"], c["asm"], 3.0, n, seed=i)


def _draw_options(sub, c):
    return dict(path=int(sub.choice([0, 0, 1, 2])) if not c["loc"] else 0, obs_batch=int(sub.choice(OBS_BATCH)),
                phase_a=["band", "band", "gram", "chain", "batch"][int(sub.integers(5))], geometry_reuse=int(sub.random() < 0.8),
                timing=int(sub.choice([0, 0, 1, 2])), stream=STREAMS[int(sub.choice([0, 0, 1, 2]))],
                obs_block_out=bool(sub.random() < 0.6))


def _draw_step(sub, seed, i, index, prev, only, plain, big, zero_at):
    """One attempt at step i from its own generator: case, features, gross errors, options -- in that order of draws."""
    if big:
        # (its model is 16 500 serial steps in NumPy, a few times the unlocalised one's: only one of the two plans is localised)
        loc = bool((seed // 7) % 2)
        c = new_case(int(sub.integers(1 << 30)), 300, 20, BIG_P, loc, ncol=100 if loc else None)
        keep = "new"
    else:
        keep = _choose_keep(sub, prev, i, only, plain, zero_at)
        c = _fresh_case(sub, i, only, plain, zero_at) if keep == "new" else _kept_case(sub, prev["case"], keep)
    f = _draw_features(sub, c, prev, only=only, none=plain or c["P"] == BIG_P, keep=keep)
    _gross_errors(sub, c, f, i)
    return make_step(c, keep=keep, relax=f["relax"], qc=f["qc"], ai=f["ai"], vl=f["vl"], gc_onepass=f["gc_onepass"],
                     entry=ENTRY_CYCLE[(i + seed) % len(ENTRY_CYCLE)], seed=seed, index=index, **_draw_options(sub, c))


def make_plan(seed, length, big_p=True):
    """`length` valid steps plus a few refusal steps.  Positions i % 6 == 4 hold exactly one feature (they rotate) on a GC case
    and i % 6 == 5 a plain cycle, unlocalised and GC in turn, so that every feature is followed by both; step length // 2 has
    more obs than one persistent Phase-A launch takes (big_p); the entry points follow ENTRY_CYCLE.  A step whose outlier ratios
    are not clear of the threshold is drawn again from the next sub-seed."""
    rng = np.random.default_rng(seed)
    plan, prev = [], None
    big_at = length // 2 if big_p else -1
    zero_at = (length // 3) // 6 * 6 + 1     # a shard that owns no row at all
    refuse_at = set(int(v) for v in rng.choice(np.arange(1, max(length, 2)), size=min(4, max(length - 1, 0)), replace=False))
    n_refused = 0
    for i in range(length):
        if i in refuse_at:
            plan.append(_refusal_step(rng, REFUSALS[(seed + n_refused) % len(REFUSALS)], prev, seed, len(plan)))
            n_refused += 1
        only = FEATURES[(i // 6) % 4] if i % 6 == 4 else None
        for attempt in range(REDRAW_MAX + 1):
            s = _draw_step(np.random.default_rng([seed, i, attempt]), seed, i, len(plan), prev, only, i % 6 == 5, i == big_at,
                           zero_at)
            s["redraws"] = attempt
            if clear(s):
                break
        else:
            s["redraws"] = REDRAW_MAX + 1    # (the host test fails on this)
        plan.append(s)
        prev = s
    return plan


def plan_hash(plan):
    """A digest of every array and setting of a plan."""
    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, dict):
            for k in sorted(v):
                h.update(k.encode())
                feed(v[k])
        elif isinstance(v, (tuple, list)):
            for x in v:
                feed(x)
        elif isinstance(v, np.ndarray):
            h.update(str(v.dtype).encode() + str(v.shape).encode())
            h.update(np.ascontiguousarray(v).tobytes())
        elif not callable(v):
            h.update(repr(v).encode())
    for s in plan:
        feed(s)
    return h.hexdigest()


# the two plans the suite runs (tests/test_gpu_context_sequences.py) and whose coverage the host test counts
PLANS = [(17, 54), (2023, 60)]
