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
    # the second generation: a few steps without refusals and bystanders; then the committed plans without the steps that
    # change one ob's tau
    n = coverage2([S.make_plan2(45, 4, 0, refusals=False)])
    assert n["keeps sl_off_on"] == 0 and n["refusal sl_unloc"] == 0 and n["gram between steps of one geometry"] == 0
    assert sum(v == 0 for k, v in n.items() if k.startswith("entry ")) >= 70
    full = S.plans2()
    cut = [[s for s in plan if s["keep"] != "sl_tau"] for plan in full]
    assert coverage2(full)["keeps sl_tau"] >= NEED["keeps sl_tau"] > coverage2(cut)["keeps sl_tau"] == 0


# ---- the second generation: the slab setting, float32 rows, the streamed cycle, the calls between the steps ------------------
@pytest.fixture(scope="module")
def plans2():
    return S.plans2()


PINNED2 = {(45, 41, 0): "ad26392af88c5f2a05f37e0e3cb93cf557a4071accbcd08661a91485cbe5d0f7",
           (48, 42, 40): "1ac238fdd57325337e30620c293255c2c4ee33276302bd44d47f2a5c77c4d858"}


def test_the_second_generation_is_the_same_on_any_machine(plans2):
    import hashlib
    assert sorted(PINNED2) == sorted(S.PLANS2)
    for key, plan in zip(S.PLANS2, plans2):
        assert hashlib.sha256("\n".join(S.describe(s) for s in plan).encode()).hexdigest() == PINNED2[key], \
            "plan %r changed: a step number quoted anywhere no longer names the same step" % (key,)
        assert len(_valid(plan)) == key[1]
        again = S.make_plan2(*key)
        assert S.plan_hash([dict(s, after=()) for s in plan]) == S.plan_hash(again)


def test_a_first_generation_step_hashes_as_before_the_new_keys():
    """plan_hash skips a second-generation key at its default: the digest of a plan is that of its steps without those keys."""
    plan = S.make_plan(5, 8, big_p=False)
    old = [{k: v for k, v in s.items() if k not in S.NEW_DEFAULTS} for s in plan]
    assert S.plan_hash(plan) == S.plan_hash(old)
    assert S.plan_hash([dict(plan[0], elem="f32")]) != S.plan_hash(plan[:1])


def test_every_step_of_the_second_generation_is_legal(plans2):
    for plan in plans2:
        for i, s in enumerate(plan):
            assert s["index"] == i
            S.check_legal(s)
            assert s["redraws"] <= S.REDRAW_MAX, "%s needed more than %d redraws" % (S.describe(s), S.REDRAW_MAX)
            assert len(s["after"]) <= 2
            if s["refusal"]:
                continue
            assert S.clear(s), S.describe(s)
            c = s["case"]
            assert c["X"].shape == (c["N"], c["M"]) and c["HX"].shape == (c["P"], c["M"]) and c["P"] < S.BIG_P
            assert np.array_equal(c["X"][c["rows"]], c["HX"])
            assert all(S.bystander_legal(s, b) for b in s["after"])
            if c["loc"]:
                nvar, nt = c["state_shape"][:2]
                assert 1 <= nvar * nt <= 6 and nvar * nt == c["n_lead"] and 17 <= c["lat"].size <= 400
            if s["sl"] is not None and "lead_time" in s["sl"]:
                assert np.array_equal(s["sl"]["lead_time"], np.tile(S.SL_STEP * np.arange(nt), nvar))
            if s["sl"] is not None and "impact" in s["sl"]:
                assert np.array_equal(s["sl"]["lead_var"], np.repeat(np.arange(nvar), nt))


def test_a_kept_slab_step_changes_exactly_what_it_names(plans2):
    for plan in plans2:
        steps = _valid(plan)
        for p, s in zip(steps, steps[1:]):
            if s["keep"] not in S.SL_KEEP_KINDS:
                continue
            a, b, c, pc = p["sl"], s["sl"], s["case"], p["case"]
            for key in ("ob_lat", "ob_lon", "hw", "asm", "lat", "lon"):
                assert np.array_equal(c[key], pc[key]), (S.describe(s), key)
            differ = [k for k in a if k in b and not np.array_equal(a[k], b[k], equal_nan=True)]
            want = dict(sl_same=[], sl_off_on=[], vl_under_sl=[], sl_tau=["ob_time_halfwidth"], sl_time=["ob_time"],
                        sl_impact=["impact"], sl_group=["ob_group"])
            if s["keep"] == "sl_ones":
                assert not S.slab_has_factors(b) and np.all(S.slab_table(dict(s, vl=None)) == 1.0)
                continue
            assert sorted(a) == sorted(b) and differ == want[s["keep"]], S.describe(s)
            for k in differ:
                assert int(np.sum(~((a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))))) == 1, S.describe(s)
            same_vl = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(p["vl"] or (), s["vl"] or ()))
            assert (p["vl"] is None) == (s["vl"] is None)
            if s["keep"] == "vl_under_sl":
                assert not same_vl and np.array_equal(p["vl"][0], s["vl"][0], equal_nan=True) and \
                    np.array_equal(p["vl"][1], s["vl"][1], equal_nan=True)
            else:
                assert same_vl


POSITIONS = ("after a slab step", "before a slab step", "between steps of one geometry")
NEED = {"keeps " + k: 2 for k in S.SL_KEEP_KINDS}      # counts that must reach more than 1


def coverage2(plans):
    """Counts of what the second-generation plans contain, by name."""
    n = {}

    def hit(key):
        n[key] = n.get(key, 0) + 1
    for a, b in itertools.product(S.FEATURES2, S.FEATURES2):
        if {a, b} != {"ai", "sl"}:
            n["%s then %s" % (a, b)] = 0
    for a, b in itertools.product(S.ENTRIES2, S.ENTRIES2):
        n["entry %s -> %s" % (a, b)] = 0
    for k in S.SL_KEEP_KINDS:
        n["keeps " + k] = 0
    for k in S.KEEP_KINDS[1:]:
        n["keeps %s under the slab setting" % k] = 0
    for b in S.BYSTANDERS:
        for pos in POSITIONS:
            n["%s %s" % (b, pos)] = 0
    for k in S.REFUSALS2:
        n["refusal " + k] = 0
    for key in ("sl with vl", "sl without vl", "sl time part only", "sl variable part only", "sl both parts", "sl without a factor",
                "sl switched on", "sl switched off", "sl then plain GC", "sl then unlocalised", "sl after the outlier check rejected",
                "state_cycle_f32 in place", "state_cycle_f32 out of place", "host_streamed f32", "host_streamed f64",
                "host_streamed GC", "host_streamed unlocalised", "host_streamed under sl", "f32 under sl", "f32 with relaxation",
                "f32 above 136 members", "f32 up to 104 members", "f32 then f64 on one geometry", "f64 then f32 on one geometry",
                "resident GC after host_streamed on one grid"):
        n[key] = 0
    for v in S.CHUNK_COLS:
        n["chunk_cols %s" % v] = 0
    names = dict(zip(("after sl", "before sl", "same geometry"), POSITIONS))
    for plan in plans:
        for s in plan:
            if s["refusal"]:
                hit("refusal " + s["refusal"])
        steps, positions = S._bystander_positions(plan)
        for i, (s, pos) in enumerate(zip(steps, positions)):
            c = s["case"]
            for b in s["after"]:
                for p in S.bystander_positions_of(b, pos):
                    hit("%s %s" % (b, names[p]))
            sl = s["sl"]
            if sl is not None:
                hit("sl with vl" if s["vl"] is not None else "sl without vl")
                hit("sl both parts" if "lead_time" in sl and "impact" in sl else
                    "sl time part only" if "lead_time" in sl else "sl variable part only")
                if not S.slab_has_factors(sl):
                    hit("sl without a factor")
                if s["entry"] == "host_streamed":
                    hit("host_streamed under sl")
                if s["elem"] == "f32":
                    hit("f32 under sl")
            if s["entry"] == "state_cycle_f32":
                hit("state_cycle_f32 in place" if s["in_place"] else "state_cycle_f32 out of place")
            if s["entry"] == "host_streamed":
                hit("host_streamed " + s["elem"])
                hit("host_streamed GC" if c["loc"] else "host_streamed unlocalised")
                hit("chunk_cols %s" % s["chunk_cols"])
            if s["elem"] == "f32":
                if s["relax"]:
                    hit("f32 with relaxation")
                hit("f32 above 136 members" if c["M"] > 136 else "f32 up to 104 members" if c["M"] <= 104 else "f32 other")
            if i == 0:
                continue
            p = steps[i - 1]
            hit("entry %s -> %s" % (p["entry"], s["entry"]))
            for a, b in itertools.product(S.FEATURES2, S.FEATURES2):
                if p[a] is not None and s[b] is not None:
                    hit("%s then %s" % (a, b))
            if s["keep"] in S.SL_KEEP_KINDS:
                hit("keeps " + s["keep"])
            elif s["keep"] != "new" and p["sl"] is not None and sl is not None:
                hit("keeps %s under the slab setting" % s["keep"])
            if p["sl"] is None and sl is not None:
                hit("sl switched on")
            if p["sl"] is not None and sl is None:
                hit("sl switched off")
                if all(s[f] is None for f in S.FEATURES2):
                    hit("sl then plain GC" if c["loc"] else "sl then unlocalised")
            if sl is not None and s["keep"] != "new" and p["qc"] is not None and not np.array_equal(S.flags(p), p["case"]["asm"]):
                hit("sl after the outlier check rejected")
            if s["keep"] in S.SAME_GEOMETRY and p["elem"] != s["elem"]:
                hit("%s then %s on one geometry" % (p["elem"], s["elem"]))
            if p["entry"] == "host_streamed" and s["entry"] != "host_streamed" and c["loc"] and s["keep"] in S.SAME_GEOMETRY + ["flag"]:
                hit("resident GC after host_streamed on one grid")
    n.pop("f32 other", None)
    return n


def test_the_second_generation_covers_every_transition(plans2):
    n = coverage2(plans2)
    missing = sorted("%s (%d)" % (k, v) for k, v in n.items() if v < NEED.get(k, 1))
    assert not missing, "the plans %r no longer contain: %s" % (S.PLANS2, "; ".join(missing))
    # together the two plans walk the Euler circuit of the nine entry points once
    assert all(v == 1 for k, v in n.items() if k.startswith("entry ")), "an ordered pair of entry points occurs twice"


def test_the_slab_factors_take_part_in_the_second_generation(plans2):
    """At least a third of the steps under the slab setting have a factor different from 1 on an ob that is assimilated (the table
    of _slabloc.slab_factor_table, the vertical factor left out), and at least one has none."""
    with_factor, without = 0, 0
    for plan in plans2:
        for s in _valid(plan):
            if s["sl"] is None:
                continue
            tab = S.slab_table(dict(s, vl=None))
            took = bool(np.any(tab[S.flags(s)] != 1.0))
            with_factor += took
            without += not took
            assert took or not S.slab_has_factors(s["sl"]) or not np.any(tab[S.flags(s)] != 1.0)
    assert without >= 1 and 3 * with_factor >= with_factor + without, (with_factor, without)


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


# ---- the model under the slab setting -------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_vl", [False, True], ids=["plain", "vl"])
def test_model_with_a_slab_setting_without_factors_is_the_model_without_it(with_vl):
    import _slabloc
    g = load_golden("G8")
    c = S.golden_case(g)
    nvar, nt = c["state_shape"][:2]
    vl = S.vertical(np.random.default_rng(3), c["n_lead"], c["P"]) if with_vl else None
    ones = S.slab_ones(nvar, nt, c["P"])
    assert not S.slab_has_factors(ones) and S.gc_family(S.make_step(c, vl=vl, sl=ones)) == (2 if with_vl else 0)
    off = S.model(S.make_step(c, vl=vl))
    _same(S.model(S.make_step(c, vl=vl, sl=ones)), off["post"], off["xam"], off["Xap"], off["diag"])
    if with_vl:
        xbm, Xbp = orc.format_prior_state(c["X"], c["HX"])
        xam, Xap, diag = _vertloc.ensrf_update_vert(xbm, Xbp, c["N"], c["val"], c["err"], c["asm"], c["ob_lat"], c["ob_lon"], c["hw"],
                                                    c["lat"], c["lon"], c["state_shape"], lead_vert=vl[0], ob_vert=vl[1],
                                                    ob_vert_halfwidth=vl[2], obs_taper="loop" if c["P"] <= 128 else "vector")
        _same(off, orc.format_posterior_state(xam, Xap, c["N"]), xam, Xap, diag)
    assert np.all(_slabloc.slab_factor_table(c["n_lead"], c["P"], **{k: v for k, v in S.slab_arrays(ones).items() if k != "ob_var"}) == 1.0)


@pytest.mark.parametrize("name", ["G5", "G8"])
def test_model_with_the_slab_setting_only(name):
    import _slabloc
    g = load_golden(name)
    c = S.golden_case(g)
    nvar, nt = c["state_shape"][:2]
    sl = S.slab_setting(np.random.default_rng(4), nvar, nt, c["P"])
    s = S.make_step(c, sl=sl)
    assert S.slab_has_factors(sl) and S.gc_family(s) == 3
    xbm, Xbp = orc.format_prior_state(c["X"], c["HX"])
    xam, Xap, diag = _slabloc.ensrf_update_slab(xbm, Xbp, c["N"], c["val"], c["err"], c["asm"], c["ob_lat"], c["ob_lon"], c["hw"], c["lat"],
                                                c["lon"], c["state_shape"], obs_taper="loop" if c["P"] <= 128 else "vector",
                                                **S.slab_arrays(sl))
    m = S.model(s)
    _same(m, orc.format_posterior_state(xam, Xap, c["N"]), xam, Xap, diag)
    assert not np.array_equal(m["post"], S.model(S.make_step(c))["post"])       # the factors took part
    # the outlier decision and relaxation compose around it as they do without it
    c2 = dict(c)
    c2["val"], idx = _outlier.inject(c["HX"], c["val"], c["err"], c["asm"], 3.0, 3, seed=1)
    s2 = S.make_step(c2, sl=sl, qc=3.0, relax=("rtps", 0.5))
    assert S.clear(s2)
    asm = _outlier.masked_flags(c["HX"], c2["val"], c["err"], c["asm"], 3.0)
    xam, Xap, diag = _slabloc.ensrf_update_slab(xbm, Xbp, c["N"], c2["val"], c["err"], asm, c["ob_lat"], c["ob_lon"], c["hw"], c["lat"],
                                                c["lon"], c["state_shape"], obs_taper="loop" if c["P"] <= 128 else "vector",
                                                **S.slab_arrays(sl))
    _same(S.model(s2), relax(c["X"], orc.format_posterior_state(xam, Xap, c["N"]), rtps=0.5), xam, Xap, diag)


def test_a_float32_case_holds_what_the_rows_widen_to():
    c = S.to_f32(S.new_case(7, 300, 20, 40, False))
    assert np.array_equal(c["X"], c["X"].astype(np.float32).astype(np.float64)) and np.array_equal(c["X"][c["rows"]], c["HX"])
    with pytest.raises(AssertionError):
        S.make_step(S.new_case(7, 300, 20, 40, False), entry="state_cycle_f32", elem="f32")     # not rounded
    with pytest.raises(AssertionError):
        S.make_step(c, entry="cycle_out", elem="f32")                                          # no float32 form of this entry
