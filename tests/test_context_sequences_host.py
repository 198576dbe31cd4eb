"""The plans of tests/_sequences.py without a GPU: they are reproducible, every step obeys the rules of include/efa_hip.h, the
two plans the GPU suite runs contain every transition the context's caches and settings can get wrong (counted from the plans:
a zero fails, so an edit of the generator cannot silently lose one), and the model equals the helpers it is composed of."""
import itertools

import numpy as np
import pytest

import _anderson2009 as a09
import _outlier
import _sequences as S
import _vertloc
from conftest import load_golden
from oracle import ensrf_oracle as orc
from test_relaxation_host import relax


@pytest.fixture(scope="module")
def plans():
    return [S.make_plan(seed, length) for seed, length in S.PLANS]


def _valid(plan):
    return [s for s in plan if not s["refusal"]]


def test_a_plan_is_a_function_of_seed_and_length():
    a = S.make_plan(5, 14, big_p=False)
    b = S.make_plan(5, 14, big_p=False)
    assert S.plan_hash(a) == S.plan_hash(b)
    assert S.plan_hash(a) != S.plan_hash(S.make_plan(6, 14, big_p=False))
    assert S.plan_hash(a[:9]) == S.plan_hash(S.make_plan(5, 14, big_p=False)[:9])
    assert len(_valid(a)) == 14


# sha256 of the steps' one-line descriptions (sizes, what is kept, entry point, options, features): what the draws of
# np.random.default_rng decide, which NumPy keeps stable across versions and machines; the arrays' last bits are left out
PINNED = {(17, 54): "263088b59c8d2a3146d39e387442bf1ae2ac818ce48a925adebc00bbe77ea5fa",
          (2023, 60): "c583f08caac924a787fc6bb9d6219bcdc713401390caedc290be9cf08fa5079b"}


def test_the_committed_plans_are_the_same_on_any_machine(plans):
    import hashlib
    assert sorted(PINNED) == sorted(S.PLANS)
    for key, plan in zip(S.PLANS, plans):
        assert hashlib.sha256("\n".join(S.describe(s) for s in plan).encode()).hexdigest() == PINNED[key], \
            "plan %r changed: a step number quoted anywhere no longer names the same step" % (key,)
    first = plans[0][:4]
    assert [(s["case"]["M"], s["case"]["P"], s["entry"]) for s in first] == [
        (136, 129, "phases_out"), (136, 129, "update_dev"), (136, 129, "state_cycle"), (136, 129, "update_dev")]


def test_every_step_is_legal_and_clear_of_the_outlier_threshold(plans):
    for plan in plans:
        for i, s in enumerate(plan):
            assert s["index"] == i
            S.check_legal(s)
            assert s["redraws"] <= S.REDRAW_MAX, "%s needed more than %d redraws" % (S.describe(s), S.REDRAW_MAX)
            if not s["refusal"]:
                assert S.clear(s), S.describe(s)
                c = s["case"]
                assert c["X"].shape == (c["N"], c["M"]) and c["HX"].shape == (c["P"], c["M"])
                if c["N"]:
                    assert np.array_equal(c["X"][c["rows"]], c["HX"])


def _feature_value(s, f):
    v = s[f]
    if v is None:
        return None
    if f == "ai":
        return (v["field"].tobytes(), v["lower"], v["upper"], v["sd_lower"])
    if f == "vl":
        return tuple(a.tobytes() for a in v)
    return v


def _plain(s):
    return all(s[f] is None for f in S.FEATURES) and s["gc_onepass"] == 1


def coverage(plans):
    """Counts of what the plans contain, by name."""
    n = {}

    def hit(key):
        n[key] = n.get(key, 0) + 1
    for key in ["%s %s" % (f, t) for f in S.FEATURES for t in ("switched on", "changed while on", "switched off",
                                                               "then plain unlocalised", "then plain GC")]:
        n[key] = 0
    for a, b in itertools.product(S.ENTRIES, S.ENTRIES):
        n["entry %s -> %s" % (a, b)] = 0
    for dim in ("M", "P", "N", "ncol"):
        n[dim + " grows x3"] = n[dim + " shrinks x3"] = 0
    for key in ("same geometry after a larger P", "P = 0", "no ob requested", "every ob rejected", "rows = 0", "vl all NaN",
                "vl re-set identical", "vl half-widths only", "P beyond one persistent launch", "gc_onepass 0",
                "refused before the context changes", "refused after obs_phase began", "same obs on another n_lead"):
        n[key] = 0
    for k in S.KEEP_KINDS:
        n["keeps " + k] = 0
    for k in S.REFUSALS:
        n["refusal " + k] = 0
    for opt, values in (("path", (0, 1, 2)), ("obs_batch", S.OBS_BATCH), ("phase_a", list(S.PHASE_A)), ("geometry_reuse", (0, 1)),
                        ("timing", (0, 1, 2)), ("stream", S.STREAMS)):
        for v in values:
            n["%s %s" % (opt, v)] = 0
    for plan in plans:
        for s in plan:
            if s["refusal"]:
                hit("refusal " + s["refusal"])
                hit("refused after obs_phase began" if s["refusal"] == "nan_hw" else "refused before the context changes")
        steps = _valid(plan)
        grow = dict.fromkeys(("M", "P", "N", "ncol"), 0)
        shrink = dict(grow)
        last = {}
        for i, s in enumerate(steps):
            c = s["case"]
            hit("keeps " + s["keep"])
            for opt in ("path", "obs_batch", "phase_a", "geometry_reuse", "timing", "stream"):
                hit("%s %s" % (opt, s[opt]))
            if c["P"] == 0:
                hit("P = 0")
            elif not c["asm"].any():
                hit("no ob requested")
            elif not S.flags(s).any():
                hit("every ob rejected")
            if c["N"] == 0:
                hit("rows = 0")
            if c["P"] == S.BIG_P:
                hit("P beyond one persistent launch")
            if c["loc"] and s["gc_onepass"] == 0:
                hit("gc_onepass 0")
            if s["vl"] is not None and np.all(np.isnan(s["vl"][2])):
                hit("vl all NaN")
            if s["keep"] == "n_lead":
                hit("same obs on another n_lead")
            if i == 0:
                last = dict(M=c["M"], P=c["P"], N=c["N"])
                if c["loc"]:
                    last["ncol"] = c["lat"].size
                continue
            p = steps[i - 1]
            pc = p["case"]
            hit("entry %s -> %s" % (p["entry"], s["entry"]))
            for f in S.FEATURES:
                va, vb = _feature_value(p, f), _feature_value(s, f)
                if va is None and vb is not None:
                    hit(f + " switched on")
                elif va is not None and vb is None:
                    hit(f + " switched off")
                elif va is not None and va != vb:
                    hit(f + " changed while on")
                if va is not None and _plain(s):
                    hit(f + (" then plain GC" if c["loc"] else " then plain unlocalised"))
            if p["vl"] is not None and s["vl"] is not None and s["keep"] != "new":
                if _feature_value(p, "vl") == _feature_value(s, "vl"):
                    hit("vl re-set identical")
                elif all(np.array_equal(x, y, equal_nan=True) for x, y in zip(p["vl"][:2], s["vl"][:2])):
                    hit("vl half-widths only")
            # (ncol against the last GC step's: the grid mirror lives through the unlocalised cycles in between)
            for dim, v in dict(M=c["M"], P=c["P"], N=c["N"], ncol=c["lat"].size if c["loc"] else None).items():
                if v is not None:
                    if dim in last:
                        grow[dim] += v > last[dim]
                        shrink[dim] += v < last[dim]
                    last[dim] = v
            # a step on the previous step's geometry, directly after that step made the per-ob workspaces re-allocate
            if s["keep"] != "new" and pc["P"] > max(k["case"]["P"] for k in steps[:i - 1] + [dict(case=dict(P=-1))]):
                hit("same geometry after a larger P")
        for dim in grow:
            n[dim + " grows x3"] += grow[dim] >= 3
            n[dim + " shrinks x3"] += shrink[dim] >= 3
    return n


def test_the_committed_plans_cover_every_transition(plans):
    n = coverage(plans)
    missing = sorted(k for k, v in n.items() if v == 0)
    assert not missing, "the plans %r no longer contain: %s" % (S.PLANS, "; ".join(missing))


def test_coverage_counting_notices_a_missing_transition():
    """The counter itself: a short plan without refusals and big steps must report zeros."""
    n = coverage([[s for s in S.make_plan(3, 6, big_p=False) if not s["refusal"]]])
    assert n["P beyond one persistent launch"] == 0 and n["refused after obs_phase began"] == 0
    assert sum(v == 0 for k, v in n.items() if k.startswith("entry ")) >= 44


# ---- the model against the helpers it is made of ---------------------------------------------------------------------------
def _golden_step(name, **kw):
    g = load_golden(name)
    return g, S.make_step(S.golden_case(g), **kw)


def _oracle_kw(g):
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    if g["loc"] != "GC":
        return {}
    return dict(loc="GC", ob_lat=g["ob_lat"], ob_lon=g["ob_lon"], ob_halfwidth=g["ob_radius"], grid_lat=g["grid_lat"],
                grid_lon=g["grid_lon"], state_shape=(nvar, nt, ny, nx))


def _same(m, post, xam, Xap, diag):
    assert np.array_equal(m["post"], post)
    if xam is not None:
        assert np.array_equal(m["xam"], xam) and np.array_equal(m["Xap"], Xap)
    for k in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
        assert np.array_equal(m["diag"][k], diag[k], equal_nan=True), k


@pytest.mark.parametrize("name", ["G1", "G6"])
def test_model_with_every_feature_off_is_the_oracle_bit_for_bit(name):
    g, s = _golden_step(name)
    c = s["case"]
    post, xam, Xap, diag = orc.ensrf_cycle(c["X"], c["HX"], c["val"], c["err"], c["asm"], **_oracle_kw(g))
    m = S.model(s)
    _same(m, post, xam, Xap, diag)
    assert m["field"] is None
    assert np.array_equal(m["post"], g["post"]) or np.allclose(m["post"], g["post"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["G1", "G6"])
@pytest.mark.parametrize("kind,alpha", [("rtps", 0.5), ("rtpp", 0.3), ("rtps", 0.0)])
def test_model_with_relaxation_only(name, kind, alpha):
    g, s = _golden_step(name, relax=(kind, alpha))
    c = s["case"]
    post, xam, Xap, diag = orc.ensrf_cycle(c["X"], c["HX"], c["val"], c["err"], c["asm"], **_oracle_kw(g))
    _same(S.model(s), relax(c["X"], post, **{kind: alpha}), xam, Xap, diag)      # the obs block and diagnostics are not relaxed


@pytest.mark.parametrize("name", ["G1", "G6"])
def test_model_with_the_outlier_check_only(name):
    g = load_golden(name)
    c = S.golden_case(g)
    c["val"], idx = _outlier.inject(c["HX"], c["val"], c["err"], c["asm"], 3.0, 3, seed=1)
    s = S.make_step(c, qc=3.0)
    assert S.clear(s)
    asm = _outlier.masked_flags(c["HX"], c["val"], c["err"], c["asm"], 3.0)
    assert not asm[idx].any() and asm.sum() == c["asm"].sum() - len(idx)
    post, xam, Xap, diag = orc.ensrf_cycle(c["X"], c["HX"], c["val"], c["err"], asm, **_oracle_kw(g))
    _same(S.model(s), post, xam, Xap, diag)
    # a threshold that rejects nothing is the plain cycle
    post, xam, Xap, diag = orc.ensrf_cycle(c["X"], c["HX"], c["val"], c["err"], c["asm"], **_oracle_kw(g))
    _same(S.model(S.make_step(c, qc=1e6)), post, xam, Xap, diag)


def test_model_with_vertical_localisation_only():
    g = load_golden("G6")
    c = S.golden_case(g)
    vl = S.vertical(np.random.default_rng(0), c["n_lead"], c["P"])
    s = S.make_step(c, vl=vl)
    xbm, Xbp = orc.format_prior_state(c["X"], c["HX"])
    xam, Xap, diag = _vertloc.ensrf_update_vert(xbm, Xbp, c["N"], c["val"], c["err"], c["asm"], c["ob_lat"], c["ob_lon"], c["hw"],
                                                c["lat"], c["lon"], c["state_shape"], lead_vert=vl[0], ob_vert=vl[1],
                                                ob_vert_halfwidth=vl[2])
    m = S.model(s)
    _same(m, orc.format_posterior_state(xam, Xap, c["N"]), xam, Xap, diag)
    # no vertical information at all: the plain cycle, bit for bit
    plain = S.model(S.make_step(c))
    assert not np.array_equal(m["post"], plain["post"])
    nan = S.model(S.make_step(c, vl=S.vertical(None, c["n_lead"], c["P"], "nan")))
    _same(nan, plain["post"], plain["xam"], plain["Xap"], plain["diag"])


def test_model_with_adaptive_inflation_only():
    g = load_golden("G6")
    c = S.golden_case(g)
    field = S.inflation_field(np.random.default_rng(1), c["N"])
    s = S.make_step(c, ai=dict(field=field, lower=0.8, upper=1.5, sd_lower=0.0))
    post, fnew, diag, Xi = a09.cycle(c["X"], c["H"], c["val"], c["err"], c["asm"], c["ob_lat"], c["ob_lon"], c["hw"], c["lat"],
                                     c["lon"], c["state_shape"], field, lower=0.8, upper=1.5, sd_lower=0.0)
    m = S.model(s)
    _same(m, post, None, None, diag)
    assert np.array_equal(m["field"], fnew) and np.array_equal(m["prior"], Xi)
    assert np.abs(fnew - field).max() > 1e-6


def test_model_order_of_the_features():
    """Prior inflation, forward operator, outlier decision against the INFLATED obs block, serial loop, relaxation of the state
    rows only: composed by hand from the helpers."""
    g = load_golden("G6")
    c = S.golden_case(g)
    field = S.inflation_field(np.random.default_rng(2), c["N"])
    Xi = a09.inflate(c["X"], field[:, 0])
    HXi = c["H"](Xi)
    c["val"], idx = _outlier.inject(HXi, c["val"], c["err"], c["asm"], 3.0, 4, seed=2)
    s = S.make_step(c, ai=dict(field=field, lower=1.0, upper=1e6, sd_lower=0.0), qc=3.0, relax=("rtps", 0.5))
    asm = _outlier.masked_flags(HXi, c["val"], c["err"], c["asm"], 3.0)
    post, fnew, diag, _ = a09.cycle(Xi, c["H"], c["val"], c["err"], asm, c["ob_lat"], c["ob_lon"], c["hw"], c["lat"], c["lon"],
                                    c["state_shape"], field, prior_inflated=True)
    m = S.model(s)
    _same(m, relax(Xi, post, rtps=0.5), None, None, diag)
    assert np.array_equal(m["field"], fnew) and not m["diag"]["assimilated"][idx].any()
