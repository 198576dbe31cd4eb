"""Cost of the LETKF (efa_letkf_cycle_dev) on device-resident cycles, beside EnSRF's GC cycle on the same inputs.

One MI355X, one process, 3 warm-up + 10 timed cycles per variant, medians.  Workloads: 64 x 64 columns x 8 leads x P = 1000 obs
with 1000 km half-widths for M = 20, 40, 80; and configs[2]'s geometry (361 x 720 columns x 148 leads, P = 5000, 1000 km) for
M = 40 when the cycle is estimated (from the 64 x 64 run's columns per second) to stay under --limit seconds -- otherwise the
measured columns per second and the extrapolation, labelled as such.  Per variant: wall ms per cycle, columns per second, and the
split of efa_last_timing (LETKF: list builds + obs block as obs_ms, the column launch as state_ms; EnSRF: Phase A, state phase).
The two are different filters: this compares their cost, not their results.  Run it under `rocprofv3 --kernel-trace --stats`
(a run of its own, --steps 3) for the kernels' own times.

    python tools/letkf_cost.py [--steps 10] [--warmup 3] [--members 20,40,80] [--limit 60] [--no-big] [--json profiles/letkf_cost.json]

--inflation measures the per-column inflation instead, on the three 64 x 64 workloads in the same process: the
LETKF cycle with the setting off (`letkf`), with a fixed field of 1.2 (`letkf_infl_fixed`, sigma_b = 0) and with the adaptive field
(`letkf_infl_adaptive`, sigma_b = 0.04, the field carried from cycle to cycle); random ob factors in both.  The call's check of the
field (a download of ncol + P doubles) is inside the timed call.

    python tools/letkf_cost.py --inflation --json profiles/letkf_inflation_cost.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(ctx, ny, nx, n_lead, M, P, hw_km, lat=(25.0, 55.0), lon=(230.0, 290.0), seed=1):
    rng = np.random.default_rng(7000 + seed + M)
    glat, glon = np.meshgrid(np.linspace(lat[0], lat[1], ny), np.linspace(lon[0], lon[1], nx), indexing="ij")
    rows = ny * nx * n_lead
    X = ctx.empty((rows, M))
    ctx.fill_synthetic(rows, 0, M, seed, 3.0, X)
    amp = min(1.0, 20.0 * np.sqrt(M / float(P)))
    HX = amp * rng.standard_normal((P, M)) + rng.standard_normal((P, 1))
    err = rng.uniform(0.5, 2.0, P)
    return dict(X=X, HX=HX, rows=rows, M=M, P=P, n_lead=n_lead, ncol=ny * nx, glat=glat, glon=glon, error=err,
                value=HX.mean(axis=1) + np.sqrt(err) * rng.standard_normal(P), assim=rng.random(P) >= 0.1,
                ob_lat=rng.uniform(lat[0] - 5, lat[1] + 5, P), ob_lon=rng.uniform(lon[0] - 5, lon[1] + 5, P), ob_hw=np.full(P, float(hw_km)))


def one_cycle(ctx, s, variant):
    from efa_xray_amd import _lib
    Yp = ctx.to_device(s["HX"])
    ym = ctx.empty((s["P"],))
    ctx.form_perts(s["P"], s["M"], Yp, ym, Yp)
    ctx.synchronize()
    if variant in ("letkf_infl_fixed", "letkf_infl_adaptive"):
        ctx.set_letkf_inflation(s["lam"], s["ob_infl"], s["P"], 0.04 if variant == "letkf_infl_adaptive" else 0.0, 1e-2, 1e2, s["lam_stats"])
    t0 = time.perf_counter()
    if variant.startswith("letkf"):
        try:
            ctx.letkf_cycle(s["rows"], s["M"], s["P"], s["X"], s["X"], ym, Yp, s["value"], s["error"], s["assim"], s["ob_lat"],
                            s["ob_lon"], s["ob_hw"], s["glat"], s["glon"], s["n_lead"])
        finally:
            ctx.set_letkf_inflation(None)
    else:
        ctx.ensrf_cycle(s["rows"], s["M"], s["P"], s["X"], s["X"], ym, Yp, s["value"], s["error"], s["assim"], _lib.LOC_GC, s["ob_lat"],
                        s["ob_lon"], s["ob_hw"], s["glat"], s["glon"], s["n_lead"])
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.last_timing()
    return wall, t["obs_ms"], t["state_ms"]


def measure(ctx, s, variant, warmup, steps):
    for _ in range(warmup):
        one_cycle(ctx, s, variant)
    runs = np.array([one_cycle(ctx, s, variant) for _ in range(steps)])
    wall, obs, state = [float(np.median(runs[:, i])) for i in range(3)]
    return dict(wall_ms=wall, obs_ms=obs, state_ms=state, columns_per_s=s["ncol"] / (wall * 1e-3),
                columns_per_s_state=s["ncol"] / (state * 1e-3) if state > 0 else None, wall_ms_min=float(runs[:, 0].min()),
                wall_ms_max=float(runs[:, 0].max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", default="20,40,80")
    ap.add_argument("--limit", type=float, default=60.0, help="seconds a configs[2] cycle may be estimated to take")
    ap.add_argument("--no-big", action="store_true")
    ap.add_argument("--inflation", action="store_true", help="the per-column inflation's three variants (DESIGN.md 7y-6)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from efa_xray_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_option("timing", 1)
    out = []
    rate40 = None
    for M in [int(m) for m in a.members.split(",")]:
        s = setup(ctx, 64, 64, 8, M, 1000, 1000.0)
        rec = dict(workload="64x64x8", M=M, P=1000, halfwidth_km=1000.0, ncol=s["ncol"], n_lead=8, warmup=a.warmup, steps=a.steps,
                   threads=None, variants={})
        if a.inflation:
            s.update(lam=ctx.to_device(np.full(s["ncol"], 1.2)), lam_stats=ctx.empty((s["ncol"], 4)),
                     ob_infl=ctx.to_device(np.random.default_rng(M).uniform(0.8, 1.6, s["P"])))
        for variant in ("letkf", "letkf_infl_fixed", "letkf_infl_adaptive") if a.inflation else ("letkf", "ensrf_gc"):
            ctx.fill_synthetic(s["rows"], 0, M, 1, 3.0, s["X"])      # (the cycles run in place: the same prior for both variants)
            rec["variants"][variant] = measure(ctx, s, variant, a.warmup, a.steps)
            print(json.dumps(dict(workload=rec["workload"], M=M, variant=variant, **rec["variants"][variant])), flush=True)
        if M == 40:
            rate40 = rec["variants"]["letkf"]
        out.append(rec)
        del s
    if rate40 is not None and not a.no_big and not a.inflation:
        ny, nx, n_lead, P = 361, 720, 148, 5000
        # per column: the solve (as measured at 8 leads, where it dominates) and 148 / 8 times the rows to apply
        est_s = ny * nx / rate40["columns_per_s_state"] * (148.0 / 8.0)
        rec = dict(workload="configs[2] geometry", M=40, P=P, halfwidth_km=1000.0, ncol=ny * nx, n_lead=n_lead,
                   upper_estimate_s=est_s, note="upper estimate: the 64x64x8 column rate scaled by 148/8 as if the apply were all of a column's time")
        if est_s <= a.limit:
            s = setup(ctx, ny, nx, n_lead, 40, P, 1000.0, lat=(-90.0, 90.0), lon=(0.0, 359.5))
            rec["variants"] = dict(letkf=measure(ctx, s, "letkf", 1, 3))
            ctx.fill_synthetic(s["rows"], 0, 40, 1, 3.0, s["X"])
            rec["variants"]["ensrf_gc"] = measure(ctx, s, "ensrf_gc", 1, 3)
            rec["measured"] = True
        else:
            rec["measured"] = False
            rec["extrapolated_wall_s"] = est_s
        print(json.dumps(rec), flush=True)
        out.append(rec)
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
