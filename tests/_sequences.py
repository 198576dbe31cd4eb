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
(test_relaxation_host.relax).  Under the slab setting the serial loop is _slabloc.ensrf_update_slab, which takes the
vertical keywords too and is bit-identical to _vertloc.ensrf_update_vert where no factor differs from 1.

A second generation of plans (make_plan2, PLANS2, plans2) draws what came to efa_ctx after the first: the slab setting as a
fifth feature with keep kinds of its own, float32 rows (the case holds what the rows widen to), the streamed host cycle, the
float32 state cycle, and calls of the other entry points between the steps (BYSTANDERS).  The first generation, its plans and
their digests are unchanged: a step that uses none of this hashes and reads as before (NEW_DEFAULTS)."""
import hashlib

import numpy as np

import _anderson2009 as a09
import _outlier
import _slabloc
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
# ---- the second generation of plans (make_plan2): what came to efa_ctx after the first ----
# a fifth feature: the keywords of Context.set_slab_localization (temporal and cross-variable localisation)
FEATURES2 = FEATURES + ["sl"]
# a step that keeps the previous step's geometry AND its slab setting, with exactly one thing changed: the setting sent again with
# identical arrays / one ob's tau / one ob's time / one impact entry / one ob's impact row / a setting whose every factor is 1 /
# cleared and the identical setting again / the vertical half-widths alone under an unchanged slab setting
SL_KEEP_KINDS = ["sl_same", "sl_tau", "sl_time", "sl_impact", "sl_group", "sl_ones", "sl_off_on", "vl_under_sl"]
KEEP_KINDS2 = KEEP_KINDS + SL_KEEP_KINDS
# obs phase + efa_state_cycle_f32_dev on float32 rows (in place and out of place) / efa_ensrf_cycle_host(_f32): the state in host
# memory, one segment per variable, streamed through the device in chunks of columns
ENTRIES2 = ENTRIES + ["state_cycle_f32", "host_streamed"]
ELEMS = ["f64", "f32"]
CHUNK_COLS = [16, 48, "all"]    # "all": one chunk of at least ncol columns
# calls made on a step's posterior between that step and the next, each on small arguments of its own
BYSTANDERS = ["obs_impact", "obs_impact_slab", "gram", "products", "verify", "neighbourhood", "pm_mean", "sensitivity",
              "slab_factor_table", "gc_block_counts", "forward_stencil"]
# the slab setting on and: an unlocalised cycle / another P / another n_lead / gc_onepass 0 / an adaptive field /
# efa_obs_impact_dev; float32 rows with an adaptive field
DIRECTED_BYSTANDERS = ["obs_impact_slab_other_vl"]      # written into directed sequences only, never drawn
REFUSALS2 = ["sl_unloc", "sl_other_p", "sl_other_nlead", "onepass0_sl", "sl_with_ai", "impact_plain_entry_under_sl", "f32_with_ai"]
SL_STEP = 6.0                   # hours between the valid times of a variable's slabs
# the keys a step of the second generation adds, at the values a step of the first generation has: plan_hash skips them there
NEW_DEFAULTS = dict(sl=None, elem="f64", chunk_cols=None, in_place=False, after=())


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
              geometry_reuse=1, timing=0, entry="cycle_out", stream="own", obs_block_out=True, refusal=None, seed=0, index=0,
              sl=None, elem="f64", chunk_cols=None, in_place=False, after=()):
    """One step.  relax: None or ("rtps" | "rtpp", alpha); qc: None or the threshold; ai: None or dict(field (N, 2), lower,
    upper, sd_lower); vl: None or (lead_vert, ob_vert, ob_vert_halfwidth); sl: None or the keywords of
    Context.set_slab_localization; elem: the rows' element type ("f32": the case's X holds float32 values); chunk_cols: columns
    per chunk of the streamed entry; in_place: the float32 state cycle writes over its prior; after: names of BYSTANDERS."""
    s = dict(case=case, keep=keep, relax=relax, qc=qc, ai=ai, vl=vl, path=path, obs_batch=obs_batch, phase_a=phase_a,
             gc_onepass=gc_onepass, geometry_reuse=geometry_reuse, timing=timing, entry=entry, stream=stream,
             obs_block_out=obs_block_out, refusal=refusal, seed=seed, index=index, redraws=0, sl=sl, elem=elem,
             chunk_cols=chunk_cols, in_place=in_place, after=tuple(after))
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
    if s.get("sl"):
        f.append("sl(%s%s%s)" % ("t" if "lead_time" in s["sl"] else "", "v" if "impact" in s["sl"] else "",
                                 "" if slab_has_factors(s["sl"]) else ",ones"))
    tail = ""
    if s.get("elem", "f64") != "f64" or s.get("chunk_cols") or s.get("in_place") or s.get("after"):   # (second generation only)
        tail = " elem=%s chunk=%s in_place=%d after=%s" % (s["elem"], s["chunk_cols"], s["in_place"], ",".join(s["after"]) or "-")
    return _describe(s, c, f) + tail


def _describe(s, c, f):
    return "step %d %s%s loc=%d N=%d M=%d P=%d n_lead=%d entry=%s path=%d batch=%d %s onepass=%d reuse=%d timing=%d stream=%s [%s]" % (
        s["index"], s["keep"], " REFUSAL " + s["refusal"] if s["refusal"] else "", bool(c["loc"]), c["N"], c["M"], c["P"],
        c["n_lead"], s["entry"], s["path"], s["obs_batch"], s["phase_a"], s["gc_onepass"], s["geometry_reuse"], s["timing"],
        s["stream"], " ".join(f) or "plain")


def check_legal(s):
    """The rules of include/efa_hip.h a valid step obeys (a refusal step breaks exactly the one it names)."""
    c = s["case"]
    assert s["entry"] in ENTRIES2 and s["phase_a"] in PHASE_A and s["obs_batch"] in OBS_BATCH and s["stream"] in STREAMS
    assert s["path"] in (0, 1, 2) and s["timing"] in (0, 1, 2) and s["gc_onepass"] in (0, 1) and s["geometry_reuse"] in (0, 1)
    assert 2 <= c["M"] <= 256 and c["P"] >= 0 and c["N"] >= 0
    if s["relax"]:
        kind, alpha = s["relax"]
        # "alpha < 0 or (RTPP) alpha > 1 return EFA_ERR_INVALID"
        assert kind in ("rtps", "rtpp") and alpha >= 0 and (kind == "rtps" or alpha <= 1)
    if s["qc"] is not None:
        assert np.isfinite(s["qc"]) and s["qc"] > 0     # "a negative, NaN or infinite threshold fails"
    if s["refusal"]:
        assert s["refusal"] in REFUSALS + REFUSALS2
        return
    assert s["elem"] in ELEMS and all(b in BYSTANDERS + DIRECTED_BYSTANDERS for b in s["after"])
    assert (s["elem"] == "f32") == (s["entry"] == "state_cycle_f32") or s["entry"] == "host_streamed"
    if s["elem"] == "f32":
        # "while an adaptive-inflation field is set the call fails"; the case holds what the float32 rows widen to
        assert s["ai"] is None and np.array_equal(c["X"], c["X"].astype(np.float32).astype(np.float64))
    if s["entry"] == "host_streamed":
        assert s["ai"] is None and (s["chunk_cols"] == "all" or s["chunk_cols"] >= 1)
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
    if s["sl"]:
        # "while it is set a later call fails unless it is a GC cycle of exactly P observations (and n_lead slabs for the state
        # phase), option gc_onepass is 1 and no adaptive-inflation field is set"
        sl = s["sl"]
        assert c["loc"] and s["gc_onepass"] == 1 and s["ai"] is None and sl["n_lead"] == c["n_lead"] and sl["P"] == c["P"]
        assert "lead_time" in sl or "impact" in sl      # "both NULL turns the setting off"
        assert "state_shape" in c and c["state_shape"][0] * c["state_shape"][1] == c["n_lead"]
        if "lead_time" in sl:
            t, tau = sl["ob_time"], sl["ob_time_halfwidth"]
            assert sl["lead_time"].shape == (c["n_lead"],) and t.shape == tau.shape == (c["P"],)
            # "a half-width that is neither NaN nor finite and > 0; an infinite time"
            assert np.all(np.isnan(tau) | ((tau > 0) & np.isfinite(tau))) and not np.any(np.isinf(t))
            assert not np.any(np.isinf(sl["lead_time"]))
        if "impact" in sl:
            C, lv, og, ov = sl["impact"], sl["lead_var"], sl["ob_group"], sl["ob_var"]
            assert C.ndim == 2 and C.size and lv.shape == (c["n_lead"],) and og.shape == ov.shape == (c["P"],)
            assert np.all(np.isfinite(C) & (C >= 0) & (C <= 1))        # "an impact entry that is not a finite number in [0, 1]"
            assert np.all((lv >= 0) & (lv < C.shape[1])) and np.all((og >= -1) & (og < C.shape[0]))
            assert np.all((ov >= -1) & (ov < C.shape[1]))
            both = (og >= 0) & (ov >= 0)
            assert np.all(C[og[both], ov[both]] == 1.0)                # "impact[ob_group[k]][ob_var[k]] != 1"


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
        if s.get("sl"):
            xam, Xap, diag = _slabloc.ensrf_update_slab(xbm, Xbp, N, c["val"], c["err"], asm, c["ob_lat"], c["ob_lon"], c["hw"],
                                                        c["lat"], c["lon"], shape, lead_vert=vl[0], ob_vert=vl[1],
                                                        ob_vert_halfwidth=vl[2], obs_taper=taper, **slab_arrays(s["sl"]))
        else:
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
    for s in plan:    # (a step that uses nothing of the second generation hashes as it did before those keys existed)
        feed({k: v for k, v in s.items() if not (k in NEW_DEFAULTS and (v is None or v == NEW_DEFAULTS[k]))})
    return h.hexdigest()


# the two plans the suite runs (tests/test_gpu_context_sequences.py) and whose coverage the host test counts
PLANS = [(17, 54), (2023, 60)]


# ---- the slab setting ---------------------------------------------------------------------------------------------------------
def slab_arrays(sl):
    """The setting as the keywords of the NumPy helpers (_slabloc.ensrf_update_slab, _efso_slab.efso_slab take all of these)."""
    return {k: v for k, v in sl.items() if k not in ("n_lead", "P")}


def slab_has_factors(sl):
    """The header's rule: "When no ob has both a time and a half-width and no impact entry of a row in use differs from 1, every
    factor is 1 and the library runs the kernels it runs without the setting"."""
    if sl is None:
        return False
    if "lead_time" in sl and np.any(~np.isnan(sl["ob_time"]) & ~np.isnan(sl["ob_time_halfwidth"])):
        return True
    if "impact" in sl:
        used = np.unique(sl["ob_group"][sl["ob_group"] >= 0])
        return bool(np.any(sl["impact"][used] != 1.0))
    return False


def slab_table(s):
    """S[P][n_lead] of a step (with the vertical factor where the step has one)."""
    c, vl = s["case"], s["vl"] or (None, None, None)
    kw = slab_arrays(s["sl"])
    kw.pop("ob_var", None)
    return _slabloc.slab_factor_table(c["n_lead"], c["P"], lead_vert=vl[0], ob_vert=vl[1], ob_vert_halfwidth=vl[2], **kw)


def slab_times(nvar, nt):
    return np.tile(SL_STEP * np.arange(nt), nvar), np.repeat(np.arange(nvar), nt).astype(np.int32)


def slab_setting(rng, nvar, nt, P, time=True, var=True):
    """The draws of tests/test_gpu_slab_localization.py::_slab.  Ob times spread over (and beyond) the slabs', ob 0 without a time,
    every 11th ob without tau, tau 2 .. 14 h (many (ob, slab) pairs lie beyond 2 tau).  Obtypes: the first nvar - 1 variables (their
    own entry exactly 1) and one that names no state variable; about a tenth of the obs have no impact row.  The last variable has
    impact 0 from every obtype; one entry lies strictly between 0 and 1."""
    lead_time, lead_var = slab_times(nvar, nt)
    sl = dict(n_lead=nvar * nt, P=P)
    if time:
        ot = rng.uniform(-SL_STEP, SL_STEP * nt, P)
        tau = rng.uniform(2.0, 14.0, P)
        if P:
            ot[0] = np.nan
        tau[3::11] = np.nan
        sl.update(lead_time=lead_time, ob_time=ot, ob_time_halfwidth=tau)
    if var:
        named = max(nvar - 1, 1)
        og = rng.integers(0, named + 1, P)
        ov = np.where(og < named, og, -1)
        og = np.where(rng.random(P) < 0.1, -1, og)
        C = rng.choice([1.0, 0.7, 0.25], (named + 1, nvar))
        C[np.arange(named), np.arange(named)] = 1.0
        if nvar > 1:
            C[:, nvar - 1] = 0.0
            C[0, 1 % nvar] = 0.4 if nvar > 2 else 0.0
        else:
            C[named, 0] = 0.4        # (one variable: the obtype that names none is the only row that may differ from 1)
        sl.update(lead_var=lead_var, ob_group=og.astype(np.int32), ob_var=ov.astype(np.int32), impact=C)
    return sl


def slab_ones(nvar, nt, P):
    """A setting whose every factor is 1: times without a single tau, an impact table of ones."""
    lead_time, lead_var = slab_times(nvar, nt)
    return dict(n_lead=nvar * nt, P=P, lead_time=lead_time, ob_time=np.linspace(0.0, 30.0, P), ob_time_halfwidth=np.full(P, np.nan),
                lead_var=lead_var, ob_group=np.zeros(P, np.int32), ob_var=np.zeros(P, np.int32), impact=np.ones((1, nvar)))


def slab_copy(sl):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sl.items()}


def slab_same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def slab_changed(rng, sl, kind):
    """A copy of the setting with the one thing `kind` names changed, or None where the setting has no such thing."""
    sl = slab_copy(sl)
    P = sl["P"]
    if not P:
        return None
    k = int(rng.integers(P))
    if kind in ("sl_tau", "sl_time"):
        if "lead_time" not in sl:
            return None
        key = "ob_time_halfwidth" if kind == "sl_tau" else "ob_time"
        old = sl[key][k]
        sl[key][k] = rng.uniform(2.0, 14.0) if kind == "sl_tau" else rng.uniform(-SL_STEP, SL_STEP * 3)
        assert not sl[key][k] == old
    elif kind == "sl_impact":
        if "impact" not in sl:
            return None
        C, og, ov = sl["impact"], sl["ob_group"], sl["ob_var"]
        own = np.zeros(C.shape, dtype=bool)              # entries some ob's obtype has on its own variable: they stay 1
        both = (og >= 0) & (ov >= 0)
        own[og[both], ov[both]] = True
        free = np.argwhere(~own)
        if not len(free):
            return None
        g, v = free[int(rng.integers(len(free)))]
        C[g, v] = 0.55 if C[g, v] != 0.55 else 0.3
    elif kind == "sl_group":
        if "impact" not in sl:
            return None
        C, og, ov = sl["impact"], sl["ob_group"], sl["ob_var"]
        ok = [g for g in range(-1, C.shape[0]) if g != og[k] and (g < 0 or ov[k] < 0 or C[g, ov[k]] == 1.0)]
        if not ok:
            return None
        og[k] = ok[int(rng.integers(len(ok)))]
    return sl


def to_f32(c):
    """The case with its state rounded to float32 and widened again: what a float32 step's model sees."""
    c = dict(c)
    c["X"] = c["X"].astype(np.float32).astype(np.float64)
    c["HX"] = forward(c)(c["X"])
    return c


def gc_family(s):
    """Option "gc_family" after a GC step whose state phase ran the one-pass sweep: 3 the slab table, 2 vertical, 1 adaptive."""
    if s.get("sl") and slab_has_factors(s["sl"]):
        return 3
    if s["vl"] is not None and np.any(~np.isnan(s["vl"][1]) & ~np.isnan(s["vl"][2])):
        return 2
    return 1 if s["ai"] else 0


# ---- the second generation of plans ---------------------------------------------------------------------------------------
def _euler(names):
    n = len(names)
    nxt = [0] * n
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            out.append(stack.pop())
    return [names[i] for i in out[::-1][:-1]]


ENTRY_CYCLE2 = _euler(ENTRIES2)      # 81 entries, cyclic: every ordered pair of the nine adjacent once
SAME_GEOMETRY = ["values"] + SL_KEEP_KINDS
NVAR_NT = [(1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (2, 2), (1, 4), (1, 5), (2, 3), (3, 2), (1, 6)]


def _fresh_case2(sub, loc, want_sl):
    big = bool(sub.random() < 0.3)
    _, M, P, _, ncol = _draw_shape(sub, loc, big)
    if want_sl and P < 17:
        P = 17
    fa = float(sub.choice([0.5, 0.9, 1.0], p=[0.25, 0.45, 0.3]))
    if not loc:
        return new_case(int(sub.integers(1 << 30)), int(sub.integers(800, 2000)) if big else int(sub.integers(1, 800)), M, P, False,
                        frac_assim=fa)
    nvar, nt = NVAR_NT[int(sub.integers(len(NVAR_NT)))]
    if want_sl and nvar * nt == 1 and sub.random() < 0.7:
        nvar, nt = 2, 3
    c = new_case(int(sub.integers(1 << 30)), nvar * nt * ncol, M, P, True, frac_assim=fa, ncol=ncol)
    c["state_shape"] = (nvar, nt, c["ny"], c["nx"])
    return c


def _kept_case2(sub, pc, keep):
    """_kept_case; "n_lead" changes the number of valid times of every variable."""
    if keep != "n_lead":
        c = _kept_case(sub, pc, keep if keep in KEEP_KINDS else "values")
        return c
    nvar, nt = pc["state_shape"][:2]
    nt2 = int(sub.choice([v for v in (1, 2, 3) if v != nt and nvar * v <= 6] or [nt + 1]))
    c = revalue(pc, sub, N=(pc["N"] // pc["n_lead"]) * nvar * nt2)
    c["n_lead"] = nvar * nt2
    c["state_shape"] = (nvar, nt2) + tuple(pc["state_shape"][2:])
    return c


def _legal_keeps(prev):
    """The keep kinds a step after `prev` may have, and for each kind of the slab setting whether `prev` offers it."""
    if prev is None:
        return []
    pc = prev["case"]
    if pc["N"] == 0:
        return []
    if not pc["loc"]:
        return ["values", "flag"] if pc["P"] else ["values"]
    kinds = ["values", "grid", "n_lead"] + (["ob_moved", "flag", "radius"] if pc["P"] else [])
    sl = prev["sl"]
    if sl is not None and pc["P"]:
        kinds += ["sl_same", "sl_ones", "sl_off_on"]
        kinds += ["sl_tau", "sl_time"] if "lead_time" in sl else []
        kinds += ["sl_impact", "sl_group"] if "impact" in sl else []
        if prev["vl"] is not None and not np.all(np.isnan(prev["vl"][2])):
            kinds.append("vl_under_sl")
    return kinds


def _draw_step2(sub, seed, i, index, prev, entry, used_keeps, force, streak):
    """One attempt at step i of a second-generation plan."""
    f32_entry = entry == "state_cycle_f32"
    streamed = entry == "host_streamed"
    legal = _legal_keeps(prev)
    keep = "new"
    under = prev is not None and prev["sl"] is not None
    # (a case is kept for at most three steps, six under the slab setting, whose kinds need a setting to build on)
    if legal and force not in ("new", "plain_u", "plain_g") + tuple(FEATURES2) and streak < (6 if under else 3) and (force == "keep" or sub.random() < (0.9 if under else 0.4)):
        # the legal kind the plans have used least so far, counted apart under the slab setting (its own kinds first among equals)
        order = [k for k in SL_KEEP_KINDS + KEEP_KINDS if k in legal]
        keep = min(order, key=lambda k: (used_keeps.get((k, under), 0), order.index(k)))
    f = dict(relax=None, qc=None, ai=None, vl=None, sl=None, gc_onepass=1)
    if keep == "new":
        loc = bool(sub.random() < 0.75)
        want = {k: bool(sub.random() < p) for k, p in (("relax", 0.35), ("qc", 0.35), ("ai", 0.25), ("vl", 0.4), ("sl", 0.7))}
        if force in ("plain_u", "plain_g"):
            loc, want = force == "plain_g", dict.fromkeys(want, False)
        if force in FEATURES2:
            loc = loc or force in ("ai", "vl", "sl")
            want[force] = True
            if force == "ai":
                want.update(sl=False, vl=False)
        c = _fresh_case2(sub, loc, want["sl"] or force in ("ai", "vl", "sl"))
        P = c["P"]
        if c["loc"] and P:
            nvar, nt = c["state_shape"][:2]
            if want["ai"] and not (f32_entry or streamed) and (force == "ai" or not want["sl"]):
                lo, up, sd = [(1.0, 1e6, 0.0), (0.8, 1.5, 0.0), (1.0, 3.0, 0.3)][int(sub.integers(3))]
                f["ai"] = dict(field=inflation_field(sub, c["N"]), lower=lo, upper=up, sd_lower=sd)
            else:
                if want["sl"]:
                    r = sub.random()      # the whole setting, the time part only, the variable part only
                    f["sl"] = slab_setting(sub, nvar, nt, P, time=r < 0.7 or r >= 0.85, var=r < 0.85)
                if want["vl"]:
                    f["vl"] = vertical(sub, c["n_lead"], P, "nan" if sub.random() > 0.85 else "full")
            if f["ai"] is None and f["vl"] is None and f["sl"] is None and force is None and sub.random() < 0.2:
                f["gc_onepass"] = 0
    else:
        pc = prev["case"]
        c = _kept_case2(sub, pc, keep)
        want = {k: bool(sub.random() < 0.3) for k in ("relax", "qc")}
        if prev["ai"] is not None and not (f32_entry or streamed):      # the field of the step before, with this step's rows
            f["ai"] = dict(prev["ai"], field=inflation_field(sub, c["N"]))
        if prev["vl"] is not None and keep != "n_lead":
            f["vl"] = tuple(a.copy() for a in prev["vl"])
        elif prev["vl"] is not None:
            f["vl"] = vertical(sub, c["n_lead"], c["P"])
        if prev["sl"] is not None:
            nvar, nt = c["state_shape"][:2]
            if keep in ("sl_tau", "sl_time", "sl_impact", "sl_group"):
                f["sl"] = slab_changed(sub, prev["sl"], keep)
                assert f["sl"] is not None
            elif keep == "sl_ones":
                f["sl"] = slab_ones(nvar, nt, c["P"])
            elif keep == "n_lead":
                f["sl"] = slab_copy(prev["sl"])
                f["sl"]["n_lead"] = nvar * nt
                if "lead_time" in f["sl"]:
                    f["sl"]["lead_time"] = slab_times(nvar, nt)[0]
                if "impact" in f["sl"]:
                    f["sl"]["lead_var"] = slab_times(nvar, nt)[1]
            else:
                f["sl"] = slab_copy(prev["sl"])
            if keep == "vl_under_sl":
                f["vl"] = (prev["vl"][0].copy(), prev["vl"][1].copy(), prev["vl"][2] * sub.uniform(0.5, 1.5))
    if want["relax"]:
        f["relax"] = RELAX[1 + int(sub.integers(len(RELAX) - 1))]
    if want["qc"]:
        f["qc"] = QC[1 + int(sub.integers(len(QC) - 1))]
    elem = "f32" if f32_entry or (streamed and sub.random() < 0.5) else "f64"
    if elem == "f32":
        c = to_f32(c)
    _gross_errors(sub, c, f, i)
    opts = _draw_options(sub, c)
    chunk = CHUNK_COLS[int(sub.integers(3))] if streamed else None
    return make_step(c, keep=keep, relax=f["relax"], qc=f["qc"], ai=f["ai"], vl=f["vl"], sl=f["sl"], gc_onepass=f["gc_onepass"],
                     entry=entry, seed=seed, index=index, elem=elem, chunk_cols=chunk, in_place=bool(f32_entry and sub.random() < 0.5),
                     **opts)


def _refusal_step2(rng, kind, seed, index):
    """A small GC case of its own (2 variables x 2 times, 40 columns, 30 obs) with exactly the one rule broken that `kind` names."""
    nvar, nt, ncol, M, P = 2, 2, 40, 20, 30
    loc = kind != "sl_unloc"
    c = new_case(int(rng.integers(1 << 30)), nvar * nt * ncol if loc else 90, M, P, loc, ncol=ncol if loc else None)
    if loc:
        c["state_shape"] = (nvar, nt, c["ny"], c["nx"])
    kw = dict(keep="new", refusal=kind, entry="cycle_out", seed=seed, index=index)
    if kind == "f32_with_ai":
        c = to_f32(c)
        kw.update(entry="state_cycle_f32", elem="f32", ai=dict(field=inflation_field(rng, c["N"]), lower=1.0, upper=1e6, sd_lower=0.0))
        return make_step(c, **kw)
    kw["sl"] = slab_setting(rng, nvar, nt - (1 if kind == "sl_other_nlead" else 0), P + (1 if kind == "sl_other_p" else 0))
    if kind == "onepass0_sl":
        kw["gc_onepass"] = 0
    if kind == "sl_with_ai":
        kw["ai"] = dict(field=inflation_field(rng, c["N"]), lower=1.0, upper=1e6, sd_lower=0.0)
    return make_step(c, **kw)


def _bystander_positions(plan):
    """For every valid step the positions its bystanders stand in: "after sl" (the step ran under the slab setting; for obs_impact,
    which the setting refuses: the step before it did), "before sl" (the next step runs under it), "same geometry" (the next step
    keeps this step's obs positions, radii, flags and grid)."""
    valid = [s for s in plan if not s["refusal"]]
    out = []
    for j, s in enumerate(valid):
        nxt = valid[j + 1] if j + 1 < len(valid) else None
        pos = set()
        if s["sl"] is not None:
            pos.add("after sl")
        if j and valid[j - 1]["sl"] is not None and s["sl"] is None:
            pos.add("after sl, cleared")
        if nxt is not None and nxt["sl"] is not None:
            pos.add("before sl")
        if nxt is not None and nxt["keep"] in SAME_GEOMETRY:
            pos.add("same geometry")
        out.append(pos)
    return valid, out


def bystander_legal(s, b):
    c = s["case"]
    if b == "obs_impact":
        return s["sl"] is None and c["N"] > 0 and c["P"] > 0
    if b == "obs_impact_slab":
        return c["N"] > 0 and c["P"] > 0
    if b == "slab_factor_table":
        return s["sl"] is not None
    return True


def bystander_positions_of(b, pos):
    """The positions bystander b stands in on a step that offers `pos`."""
    p = set(pos) - {"after sl, cleared"}
    if b == "obs_impact" and "after sl, cleared" in pos:
        p.add("after sl")
    return p


def _assign_bystanders(plans):
    """Zero to two bystanders per step, given out in the order of the plans to the bystander that still lacks most of the three
    positions, then to the one used least (a function of the plans alone)."""
    have = {b: set() for b in BYSTANDERS}
    uses = dict.fromkeys(BYSTANDERS, 0)
    n = 0
    for plan in plans:
        valid, positions = _bystander_positions(plan)
        for s, pos in zip(valid, positions):
            n += 1
            chosen = []
            for _ in range(n % 3):
                cand = [b for b in BYSTANDERS if b not in chosen and bystander_legal(s, b)]
                if not cand:
                    break
                b = max(cand, key=lambda b: (len(bystander_positions_of(b, pos) - have[b]), -uses[b], -BYSTANDERS.index(b)))
                chosen.append(b)
                uses[b] += 1
                have[b] |= bystander_positions_of(b, pos)
            s["after"] = tuple(chosen)


def make_plan2(seed, length, start, refusals=True):
    """`length` valid steps whose entry points are ENTRY_CYCLE2[start:start + length] (cyclic), plus refusal steps.  Positions
    i % 10 == 2 and 3 hold new cases with one of the five features forced on (they rotate, so that each follows each other one),
    i % 10 == 4 keeps that case, i % 10 == 5 is a plain cycle, unlocalised or GC in turn, and i % 10 == 6 keeps it; what a step
    keeps is the legal kind used least so far.  The refusals of REFUSALS2 are shared out between the plan that starts the circuit
    and the one that ends it.  No step has more obs than one persistent Phase-A launch takes, and none a state without rows: the
    first generation has those.  The bystanders are given out over PLANS2 as a whole (plans2())."""
    rng = np.random.default_rng(seed)
    plan, prev = [], None
    kinds = REFUSALS2[:4] if start == 0 else REFUSALS2[3:]
    refuse_at = {}
    if refusals:
        at = sorted(int(v) for v in rng.choice(np.arange(1, max(length, 2)), size=min(len(kinds), max(length - 1, 0)), replace=False))
        refuse_at = dict(zip(at, kinds))
    used_keeps, streak = {}, 0
    for i in range(length):
        if i in refuse_at:
            plan.append(_refusal_step2(rng, refuse_at[i], seed, len(plan)))
        entry = ENTRY_CYCLE2[(start + i) % len(ENTRY_CYCLE2)]
        k = i // 10 + (2 if start else 0)
        force = {2: FEATURES2[(k + 1) % 5], 3: FEATURES2[k % 5], 4: "keep", 5: "plain_u" if (k + (start > 0)) % 2 == 0 else "plain_g",
                 6: "keep"}.get(i % 10, "new" if i == 0 else None)
        if force == "ai" and entry in ("state_cycle_f32", "host_streamed"):
            force = "sl"
        for attempt in range(REDRAW_MAX + 1):
            s = _draw_step2(np.random.default_rng([seed, i, attempt]), seed, i, len(plan), prev, entry, used_keeps, force, streak)
            s["redraws"] = attempt
            if clear(s):
                break
        else:
            s["redraws"] = REDRAW_MAX + 1
        key = (s["keep"], prev is not None and prev["sl"] is not None)
        used_keeps[key] = used_keeps.get(key, 0) + 1
        streak = 0 if s["keep"] == "new" else streak + 1
        plan.append(s)
        prev = s
    return plan


# the two plans of the second generation: together they walk ENTRY_CYCLE2 once (41 + 42 steps, the step at the seam in both)
PLANS2 = [(45, 41, 0), (48, 42, 40)]


def plans2():
    """The plans of PLANS2 with their bystanders."""
    plans = [make_plan2(*key) for key in PLANS2]
    _assign_bystanders(plans)
    return plans
