"""Cost of adaptive inflation (Anderson 2009) on device-resident localised cycles.

Times efa_ensrf_cycle_dev with adaptive inflation off and on in ONE process, alternating the two round by round (warm-up +
timed cycles per variant and round), on
  - cfg2: a configs[2]-like cycle, 4 x 37 x 361 x 720 rows x 80 members x 5 000 obs, GC 1 000 km;
  - cfg3: a configs[3]-sized cycle on one GPU, the same grid x 100 members x 10 000 obs.
The state phase (HIP events, "timing" 2) is reported per variant: off it is the plain one-pass sweep, on it is the sweep with
the fused field update and the per-ob record pass (k_adapt_obs).  k_inflate_rows, which runs before the forward operator and
outside the state phase, is timed on its own (host clock around synchronised batches) with the HBM bytes it moves.  Run it
under `rocprofv3 --kernel-trace --stats` for per-kernel times.

    python tools/adaptive_inflation_cost.py [--rounds 3] [--steps 10] [--warmup 2] [--sizes cfg2,cfg3] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0
SIZES = {
    "cfg2": dict(n_lead=148, ny=361, nx=720, M=80, P=5_000, radius_km=1000.0),
    "cfg3": dict(n_lead=148, ny=361, nx=720, M=100, P=10_000, radius_km=1000.0),
    "small": dict(n_lead=8, ny=90, nx=180, M=40, P=300, radius_km=1000.0),
}


def setup(ctx, wl, seed=1):
    M, P, n_lead = wl["M"], wl["P"], wl["n_lead"]
    ny, nx = wl["ny"], wl["nx"]
    lat2, lon2 = np.meshgrid(np.linspace(-90, 90, ny), np.linspace(0, 360 - 360.0 / nx, nx), indexing="ij")
    glat, glon = lat2.reshape(-1), lon2.reshape(-1)
    ncol = ny * nx
    rows = n_lead * ncol
    rng = np.random.default_rng(3000 + seed)
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
    lam = 1.0 + 0.5 * (1.0 + np.sin(np.radians(glat) * 3.0) * np.cos(np.radians(glon) * 2.0))
    field = np.stack([np.tile(lam, n_lead), np.full(rows, 0.6)], axis=1)
    return dict(X=X, post=post, Yp=Yp, ym=ym, val=val, err=np.ones(P), assim=np.ones(P, dtype=bool), lat=glat[col],
                lon=glon[col], hw=np.full(P, wl["radius_km"]), glat=glat, glon=glon, rows=rows, M=M, P=P, n_lead=n_lead,
                F=ctx.to_device(field), field=field)


def cycle(ctx, s):
    ctx.ensrf_cycle(s["rows"], s["M"], s["P"], s["X"], s["post"], s["ym"], s["Yp"], s["val"], s["err"], s["assim"], 1,
                    s["lat"], s["lon"], s["hw"], s["glat"], s["glon"], s["n_lead"])


def run_variant(ctx, s, on, warmup, steps):
    if on:
        ctx.set_adaptive_inflation(s["F"], s["rows"])
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
    finally:
        ctx.set_adaptive_inflation(None)
    t = ctx.last_timing()
    return dict(state_ms=t["state_ms"] / steps, obs_ms=t["obs_ms"] / steps, wall_ms=1e3 * wall / steps,
                launches=t["state_launches"] / steps)


def time_inflate(ctx, s, steps):
    """k_inflate_rows on the posterior buffer (a scratch copy of the state): a field of mild factors, so that every row is
    read and written and repeated passes stay finite."""
    rows, M = s["rows"], s["M"]
    mild = s["field"].copy()
    mild[:, 0] = 1.0 + 0.01 * (mild[:, 0] - 1.0) + 1e-6
    Fm = ctx.to_device(mild)
    ctx.fill_synthetic(rows, 0, M, 7, 3.0, s["post"])
    ctx.inflate_rows(rows, M, s["post"], Fm)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.inflate_rows(rows, M, s["post"], Fm)
    ctx.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    moved = rows * M * 8.0 * 2 + rows * 16.0
    del Fm
    return dict(inflate_ms=ms, bytes=moved, GBps=moved / (ms * 1e-3) / 1e9, hbm_peak_fraction=moved / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS)


def measure(ctx, name, wl, rounds, warmup, steps):
    s = setup(ctx, wl)
    res = {"off": [], "on": []}
    for r in range(rounds):
        for v in ("off", "on"):
            res[v].append(run_variant(ctx, s, v == "on", warmup, steps))
            x = res[v][-1]
            print("%-6s round %d %-3s state %.3f ms  obs %.3f ms  wall %.3f ms  launches %.1f" %
                  (name, r, v, x["state_ms"], x["obs_ms"], x["wall_ms"], x["launches"]), flush=True)
    out = dict(workload=name, rows=s["rows"], M=s["M"], P=s["P"], rounds=rounds, warmup=warmup, steps=steps, variants={})
    for v in ("off", "on"):
        st = np.array([x["state_ms"] for x in res[v]])
        wa = np.array([x["wall_ms"] for x in res[v]])
        out["variants"][v] = dict(state_ms=[round(x, 4) for x in st], wall_ms=[round(x, 4) for x in wa],
                                  state_ms_median=float(np.median(st)), wall_ms_median=float(np.median(wa)),
                                  launches=res[v][0]["launches"])
    out["state_on_over_off"] = out["variants"]["on"]["state_ms_median"] / out["variants"]["off"]["state_ms_median"]
    out["inflate_rows"] = time_inflate(ctx, s, steps)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="cfg2,cfg3")
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
