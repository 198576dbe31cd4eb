"""Cost of the observation-impact pass under the temporal and variable tapers (EFSO).

Times the contraction and its reduction (read-only option "impact_us") in ONE process, alternating four variants round by round
(warm-up + timed calls per variant and round), on the state and obs of tools/slab_localization_cost.py: 4 variables x 37 levels x
361 x 720 rows x 80 members x 5 000 obs, GC 1 000 km, ln p as the slabs' vertical coordinate, one scale height as half-width:

  plain      efa_obs_impact_dev, no per-slab factor (k_sweep_gc_lane_impact<., false, .>)
  vert       efa_obs_impact_dev under the vertical setting: the factor evaluated while staging (k_sweep_gc_lane_impact<., true, .>)
  slab_vert  efa_obs_impact_slab_dev with the table carrying those same vertical factors and nothing else (variant slab_vert of
             tools/slab_localization_cost.py: a temporal part whose every factor is exactly 1 keeps the setting on)
  slab_all   slab_vert plus the temporal factor (tau a quarter of the span) and one variable at impact 0, as slab_all there

A round's figure is the median of its timed calls' "impact_us", a variant's the median of its rounds; "spread" of a variant is
(max - min) / median of its rounds; the yardstick for slab_vert is vert of the same run:
slab_vert <= vert * (1 + the larger of the two spreads + 0.01) -- a 128-byte load replaces a polynomial.  slab_all has no target;
it is reported with the share of (group of 16 slabs, ob) pairs whose factors are all zero, the (wave, ob) pairs skipped on top of
the horizontal skipping.  The table is cached after a variant's first call (its build is in tools/slab_localization_cost.py).

    python tools/obs_impact_slab_cost.py [--rounds 3] [--steps 10] [--warmup 2] [--sizes cfg2] [--json out.json]
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

from slab_localization_cost import apply, skipped_pairs, table_of  # noqa: E402  (the same settings)
from vertical_localization_cost import SIZES, setup  # noqa: E402  (the same state and obs)

VARIANTS = ("plain", "vert", "slab_vert", "slab_all")
SETTING = dict(plain="off", vert="vert", slab_vert="slab_vert", slab_all="slab_all")   # slab_localization_cost.apply's names


def run_variant(ctx, s, wl, v, warmup, steps):
    apply(ctx, s, wl, SETTING[v])
    call = ctx.obs_impact_slab if v.startswith("slab") else ctx.obs_impact
    us = []
    t0 = 0.0
    try:
        for i in range(warmup + steps):
            if i == warmup:
                t0 = time.perf_counter()
            J = call(s["rows"], s["M"], s["P"], s["X"], s["werr"], s["Yp"], s["innov"], s["err"], s["assim"], 1, s["lat"], s["lon"],
                     s["hw"], s["glat"], s["glon"], s["n_lead"])
            if i >= warmup:
                us.append(ctx.get_option("impact_us"))
        wall = time.perf_counter() - t0
    finally:
        apply(ctx, s, wl, "off")
    return dict(ms=1e-3 * float(np.median(us)), wall_ms=1e3 * wall / steps, nonzero=int(np.count_nonzero(J)))


def measure(ctx, name, wl, rounds, warmup, steps):
    s = setup(ctx, wl)
    rng = np.random.default_rng(7)
    s["werr"] = ctx.to_device(rng.standard_normal(s["rows"]))
    s["innov"] = rng.standard_normal(s["P"])
    res = {v: [] for v in VARIANTS}
    for r in range(rounds):
        for v in VARIANTS:
            res[v].append(run_variant(ctx, s, wl, v, warmup, steps))
            x = res[v][-1]
            print("%-6s round %d %-9s impact %.3f ms  wall %.3f ms  non-zero impacts %d" % (name, r, v, x["ms"], x["wall_ms"], x["nonzero"]),
                  flush=True)
    out = dict(workload=name, rows=s["rows"], M=s["M"], P=s["P"], n_lead=s["n_lead"], rounds=rounds, warmup=warmup, steps=steps,
               table_bytes=s["P"] * s["n_lead"] * 8, variants={})
    for v in VARIANTS:
        ms = np.array([x["ms"] for x in res[v]])
        out["variants"][v] = dict(ms=[round(float(x), 4) for x in ms], ms_median=float(np.median(ms)),
                                  wall_ms=[round(x["wall_ms"], 4) for x in res[v]], spread=float((ms.max() - ms.min()) / np.median(ms)),
                                  nonzero_impacts=res[v][0]["nonzero"])
        if v != "plain":
            out["variants"][v]["over_plain"] = float(np.median(ms)) / out["variants"]["plain"]["ms_median"]
            out["variants"][v]["skipped_pairs"] = skipped_pairs(table_of(ctx, s, wl, SETTING[v]))
    b, c = out["variants"]["vert"]["ms_median"], out["variants"]["slab_vert"]["ms_median"]
    spread = max(out["variants"]["vert"]["spread"], out["variants"]["slab_vert"]["spread"])
    out["spread"] = spread
    out["slab_vert_over_vert"] = c / b
    out["slab_vert_within_yardstick"] = bool(c <= b * (1.0 + spread + 0.01))
    out["slab_all_over_vert"] = out["variants"]["slab_all"]["ms_median"] / b
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
    results = []
    for name in a.sizes.split(","):
        results.append(measure(ctx, name, SIZES[name], a.rounds, a.warmup, a.steps))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
