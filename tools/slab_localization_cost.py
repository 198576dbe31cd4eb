"""Cost of temporal and cross-variable localisation on device-resident localised cycles.

Times efa_ensrf_cycle_dev in ONE process, alternating four variants round by round (warm-up + timed cycles per variant and
round), on the configs[2]-like cycle of tools/vertical_localization_cost.py: 4 variables x 37 levels x 361 x 720 rows x 80 members
x 5 000 obs, GC 1 000 km, the levels on the time slot with ln p as the slabs' vertical coordinate (one scale height as half-width):

  off        no per-slab factor: the plain one-pass sweep (k_sweep_gc_lane, family 0)
  vert       vertical localisation only: the vertical family (k_sweep_gc_lane, family 2), the factor evaluated while staging
  slab_vert  the slab-table family (k_sweep_gc_lane, family 3) fed the same vertical factors and nothing else: a temporal part whose
             every factor is exactly 1 (slabs without a time, all obs at one time) keeps the setting active
  slab_all   slab_vert plus a temporal factor (the slab index as time, tau a quarter of the span) and a variable factor (the last
             variable takes impact 0 from every other obtype)

Per variant: the state phase and Phase A (HIP events, "timing" 2), the family that ran (option "gc_family"), the share of
(group of 16 slabs, ob) pairs whose factors are all zero -- the (wave, ob) pairs of the lane form skipped on top of the horizontal
skipping -- and, for the slab variants, the time to build the table (host clock around efa_slab_factor_table after a change of
the setting, waited for).  "state_spread" is (max - min) / median of a variant's state phase over the rounds, "spread" the larger
of vert's and slab_vert's; the yardstick for slab_vert is vert: slab_vert <= vert * (1 + spread + 0.01).

    python tools/slab_localization_cost.py [--rounds 3] [--steps 10] [--warmup 2] [--sizes cfg2] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vertical_localization_cost import SIZES, cycle, setup  # noqa: E402  (the same cycle, state and obs)

VARIANTS = ("off", "vert", "slab_vert", "slab_all")
VERT_HALFWIDTH = 1.0  # one scale height in ln p ("tight" in tools/vertical_localization_cost.py)


def slab_setting(s, wl, variant):
    """The keywords of Context.set_slab_localization for a variant (None: the setting stays off)."""
    P, n_lead, nvar, nlev = s["P"], s["n_lead"], wl["nvar"], wl["nlev"]
    if variant == "slab_vert":
        return dict(n_lead=n_lead, P=P, lead_time=np.full(n_lead, np.nan), ob_time=np.zeros(P), ob_time_halfwidth=np.ones(P))
    if variant != "slab_all":
        return None
    lead_time = np.tile(np.arange(nlev, dtype=np.float64), nvar)
    impact = np.ones((nvar, nvar))
    impact[:, nvar - 1] = 0.0
    impact[nvar - 1, nvar - 1] = 1.0
    # each ob at the time of its own level (setup places it at a slab's ln p), its obtype one of the variables
    lnp = s["lead"][:nlev]
    ob_time = np.abs(s["ob_vert"][:, None] - lnp[None, :]).argmin(axis=1).astype(np.float64)
    ob_var = np.random.default_rng(5).integers(0, nvar, P).astype(np.int32)
    return dict(n_lead=n_lead, P=P, lead_time=lead_time, ob_time=ob_time, ob_time_halfwidth=np.full(P, (nlev - 1) / 4.0),
                lead_var=np.repeat(np.arange(nvar, dtype=np.int32), nlev), ob_group=ob_var, ob_var=ob_var, impact=impact)


def apply(ctx, s, wl, variant):
    ctx.set_slab_localization(None)
    ctx.set_vertical_localization(None)
    if variant != "off":
        ctx.set_vertical_localization(s["lead"], s["ob_vert"], np.full(s["P"], VERT_HALFWIDTH))
    kw = slab_setting(s, wl, variant)
    if kw is not None:
        ctx.set_slab_localization(**kw)


def skipped_pairs(S):
    """Share of (group of 16 slabs, ob) pairs whose factors are all zero; S [P][n_lead]."""
    groups = range(0, S.shape[1], 16)
    skip = sum(int((~(S[:, g:g + 16] != 0.0).any(axis=1)).sum()) for g in groups)
    return skip / float(len(groups) * S.shape[0])


def table_of(ctx, s, wl, variant):
    """The factors of a variant as the slab table gives them ("vert": the table of the same vertical factors)."""
    apply(ctx, s, wl, "slab_vert" if variant == "vert" else variant)
    try:
        return ctx.slab_factor_table(s["P"], s["n_lead"])
    finally:
        apply(ctx, s, wl, "off")


def table_build_ms(ctx, s, wl, variant, reps=5):
    out = []
    for _ in range(reps):
        apply(ctx, s, wl, variant)   # (turned off and on again: the serial moves, the table is rebuilt)
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.slab_factor_table(s["P"], s["n_lead"], download=False)
        out.append(1e3 * (time.perf_counter() - t0))
    apply(ctx, s, wl, "off")
    return float(np.median(out))


def run_variant(ctx, s, wl, v, warmup, steps):
    apply(ctx, s, wl, v)
    try:
        for _ in range(warmup):
            cycle(ctx, s)
        ctx.synchronize()
        ctx.last_timing()
        t0 = time.perf_counter()
        for _ in range(steps):
            cycle(ctx, s)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        family = ctx.get_option("gc_family")
    finally:
        apply(ctx, s, wl, "off")
    t = ctx.last_timing()
    return dict(state_ms=t["state_ms"] / steps, obs_ms=t["obs_ms"] / steps, wall_ms=1e3 * wall / steps, family=family)


def measure(ctx, name, wl, rounds, warmup, steps):
    s = setup(ctx, wl)
    res = {v: [] for v in VARIANTS}
    for r in range(rounds):
        for v in VARIANTS:
            res[v].append(run_variant(ctx, s, wl, v, warmup, steps))
            x = res[v][-1]
            print("%-6s round %d %-9s state %.3f ms  obs %.3f ms  wall %.3f ms  family %d" %
                  (name, r, v, x["state_ms"], x["obs_ms"], x["wall_ms"], x["family"]), flush=True)
    out = dict(workload=name, rows=s["rows"], M=s["M"], P=s["P"], n_lead=s["n_lead"], rounds=rounds, warmup=warmup, steps=steps,
               vert_halfwidth_lnp=VERT_HALFWIDTH, table_bytes=s["P"] * s["n_lead"] * 8, variants={})
    for v in VARIANTS:
        st = np.array([x["state_ms"] for x in res[v]])
        ob = np.array([x["obs_ms"] for x in res[v]])
        wa = np.array([x["wall_ms"] for x in res[v]])
        out["variants"][v] = dict(state_ms=[round(x, 4) for x in st], obs_ms=[round(x, 4) for x in ob], wall_ms=[round(x, 4) for x in wa],
                                  state_ms_median=float(np.median(st)), obs_ms_median=float(np.median(ob)),
                                  wall_ms_median=float(np.median(wa)), gc_family=res[v][0]["family"],
                                  state_spread=float((st.max() - st.min()) / np.median(st)))
        if v != "off":
            out["variants"][v]["state_over_off"] = float(np.median(st)) / out["variants"]["off"]["state_ms_median"]
            out["variants"][v]["skipped_pairs"] = skipped_pairs(table_of(ctx, s, wl, v))
        if v.startswith("slab"):
            out["variants"][v]["table_build_ms"] = table_build_ms(ctx, s, wl, v)
    b, c = out["variants"]["vert"]["state_ms_median"], out["variants"]["slab_vert"]["state_ms_median"]
    spread = max(out["variants"]["vert"]["state_spread"], out["variants"]["slab_vert"]["state_spread"])
    out["spread"] = spread
    out["slab_vert_over_vert"] = c / b
    out["slab_vert_within_yardstick"] = bool(c <= b * (1.0 + spread + 0.01))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="cfg2")
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    ctx.set_option("timing", 2)
    results = []
    for name in a.sizes.split(","):
        results.append(measure(ctx, name, SIZES[name], a.rounds, a.warmup, a.steps))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
