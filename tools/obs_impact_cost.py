"""Cost of the observation-impact pass (EFSO) against the plain one-pass GC sweep of the same geometry.

One process, alternating round by round (warm-up + timed calls per variant and round) on a configs[2]-like workload: 4 variables
x 37 levels x 361 x 720 rows x 80 members x 5 000 obs, GC 1 000 km.  "sweep" is efa_ensrf_cycle_dev's state phase (HIP events,
"timing" 2: k_sweep_gc_lane, lists cached after the first cycle); "impact" is efa_obs_impact_dev's read-only option "impact_us"
(k_sweep_gc_lane_impact and its reduction; the build of the call's own lists is outside it, as the cached lists are outside the
sweep's figure).  The impact pass reads the state once and writes nothing: its achieved bandwidth is (rows M + rows) 8 bytes over
its time.

    python tools/obs_impact_cost.py [--rounds 3] [--steps 10] [--warmup 2] [--sizes cfg2] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {
    "cfg2": dict(nvar=4, nlev=37, ny=361, nx=720, M=80, P=5_000, radius_km=1000.0),
    "small": dict(nvar=2, nlev=8, ny=90, nx=180, M=40, P=300, radius_km=1000.0),
}


def setup(ctx, wl, seed=1):
    M, P = wl["M"], wl["P"]
    n_lead = wl["nvar"] * wl["nlev"]
    ny, nx = wl["ny"], wl["nx"]
    lat2, lon2 = np.meshgrid(np.linspace(-90, 90, ny), np.linspace(0, 360 - 360.0 / nx, nx), indexing="ij")
    glat, glon = lat2.reshape(-1), lon2.reshape(-1)
    ncol = ny * nx
    rows = n_lead * ncol
    rng = np.random.default_rng(4000 + seed)
    pick = rng.choice(rows, P, replace=False).astype(np.int64)
    X = ctx.empty((rows, M))
    post = ctx.empty((rows, M))
    ctx.fill_synthetic(rows, 0, M, seed, 3.0, X)
    HX = np.stack([X.download_rows(int(r), int(r) + 1)[0] for r in pick])
    val = HX.mean(axis=1) + rng.standard_normal(P)
    Yp = ctx.to_device(HX)
    ym = ctx.empty((P,))
    ctx.form_perts(P, M, Yp, ym, Yp)
    col = pick % ncol
    return dict(X=X, post=post, Yp=Yp, ym=ym, Ya=ctx.to_device(HX), werr=ctx.to_device(rng.standard_normal(rows)), val=val,
                innov=rng.standard_normal(P), err=np.ones(P), assim=np.ones(P, dtype=bool), lat=glat[col], lon=glon[col],
                hw=np.full(P, wl["radius_km"]), glat=glat, glon=glon, rows=rows, M=M, P=P, n_lead=n_lead)


def run_sweep(ctx, s, warmup, steps):
    def cycle():
        ctx.ensrf_cycle(s["rows"], s["M"], s["P"], s["X"], s["post"], s["ym"], s["Yp"], s["val"], s["err"], s["assim"], 1,
                        s["lat"], s["lon"], s["hw"], s["glat"], s["glon"], s["n_lead"])
    for _ in range(warmup):
        cycle()
    ctx.synchronize()
    ctx.last_timing()
    t0 = time.perf_counter()
    for _ in range(steps):
        cycle()
    ctx.synchronize()
    wall = time.perf_counter() - t0
    t = ctx.last_timing()
    return dict(ms=t["state_ms"] / steps, wall_ms=1e3 * wall / steps)


def run_impact(ctx, s, warmup, steps):
    us = []
    t0 = 0.0
    for i in range(warmup + steps):
        if i == warmup:
            t0 = time.perf_counter()
        ctx.obs_impact(s["rows"], s["M"], s["P"], s["post"], s["werr"], s["Ya"], s["innov"], s["err"], s["assim"], 1, s["lat"],
                       s["lon"], s["hw"], s["glat"], s["glon"], s["n_lead"])
        if i >= warmup:
            us.append(ctx.get_option("impact_us"))
    wall = time.perf_counter() - t0
    return dict(ms=1e-3 * float(np.mean(us)), wall_ms=1e3 * wall / steps)


def measure(ctx, name, wl, rounds, warmup, steps):
    s = setup(ctx, wl)
    res = {"sweep": [], "impact": []}
    for r in range(rounds):
        for v, fn in (("sweep", run_sweep), ("impact", run_impact)):
            res[v].append(fn(ctx, s, warmup, steps))
            print("%-6s round %d %-6s %.3f ms  wall %.3f ms" % (name, r, v, res[v][-1]["ms"], res[v][-1]["wall_ms"]), flush=True)
    out = dict(workload=name, rows=s["rows"], M=s["M"], P=s["P"], n_lead=s["n_lead"], rounds=rounds, warmup=warmup, steps=steps)
    for v in res:
        ms = np.array([x["ms"] for x in res[v]])
        out[v] = dict(ms=[round(float(x), 4) for x in ms], ms_median=float(np.median(ms)),
                      wall_ms=[round(x["wall_ms"], 4) for x in res[v]])
    out["impact_over_sweep"] = out["impact"]["ms_median"] / out["sweep"]["ms_median"]
    nbytes = 8.0 * (s["rows"] * s["M"] + s["rows"])
    out["impact_read_bytes"] = nbytes
    out["impact_tb_per_s"] = nbytes / (1e-3 * out["impact"]["ms_median"]) / 1e12
    out["sweep_tb_per_s"] = 2.0 * 8.0 * s["rows"] * s["M"] / (1e-3 * out["sweep"]["ms_median"]) / 1e12   # one read + one write
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
