"""Cost of posterior relaxation (RTPP / RTPS) on device-resident cycles.

Times efa_ensrf_cycle_dev (ShardedEnSRF at world size 1, as bench.py drives it) with no relaxation, RTPP and RTPS in ONE
process, alternating the variants round by round (3 warm-up + 20 timed cycles per variant and round), on
  - the headline: 1e7 state rows x 100 members x 1e4 obs, loc=None, synthetic state (efa_fill_synthetic_dev) -- the
    transform path: RTPP folded into T, RTPS fused into k_transform_rtps;
  - a configs[2]-like localised size (--gc cfg3: 4 x 37 x 361 x 720 rows x 80 members x 5000 obs, GC 1000 km) -- the
    one-pass GC sweep with the standalone row-spread and relax passes around it.
Prints per variant the library's state-phase time per cycle (HIP events, "timing" 2) and the wall time per cycle, and for
the standalone passes the HBM bytes they move against the added time.  Run it under `rocprofv3 --kernel-trace --stats`
for per-kernel times.

    python tools/relax_cost.py [--rounds 3] [--steps 20] [--warmup 3] [--gc cfg3|small_gc|none] [--headline-rows N]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0

SIZES = {
    "headline": dict(n_lead=1, ncol=10_000_000, M=100, P=10_000, loc=None),
    "cfg3": dict(n_lead=148, ny=361, nx=720, M=80, P=5_000, loc="GC", radius_km=1000.0),
    "small_gc": dict(n_lead=8, ny=90, nx=180, M=40, P=300, loc="GC", radius_km=1000.0),
}
VARIANTS = (("none", {}), ("rtpp", dict(rtpp=0.5)), ("rtps", dict(rtps=0.9)))


def setup(eng, wl, seed=1):
    from efa_xray_amd.distributed import ShardedEnSRF
    torch = eng.torch
    M, P = wl["M"], wl["P"]
    glat = glon = None
    if wl["loc"] == "GC":
        ny, nx = wl["ny"], wl["nx"]
        lat2, lon2 = np.meshgrid(np.linspace(-90, 90, ny), np.linspace(0, 360 - 360.0 / nx, nx), indexing="ij")
        glat, glon = lat2.reshape(-1), lon2.reshape(-1)
        ncol = ny * nx
    else:
        ncol = wl["ncol"]
    n_lead = wl["n_lead"]
    rows = n_lead * ncol
    sh = ShardedEnSRF(eng, n_lead, ncol, M)
    rng = np.random.default_rng(3000 + seed)
    pick = rng.choice(rows, P, replace=False).astype(np.int64)
    idx, wts = pick[:, None].copy(), np.ones((P, 1))
    err = np.ones(P)
    ob = dict(value=None, error=err, assim=np.ones(P, dtype=bool))
    if wl["loc"] == "GC":
        col = pick % ncol
        ob.update(loc="GC", lat=glat[col], lon=glon[col], halfwidth=np.full(P, wl["radius_km"]))
    X = eng.empty((rows, M))
    post = eng.empty((rows, M))
    eng.ctx.fill_synthetic(rows, 0, M, seed, 3.0, X.data_ptr())
    HX = sh.partial_estimates(X, idx, wts)
    torch.cuda.synchronize()
    ob["value"] = HX.cpu().numpy().mean(axis=1) + np.random.default_rng(4000 + seed).standard_normal(P)
    return dict(sh=sh, X=X, post=post, idx=idx, wts=wts, ob=ob, glat=glat, glon=glon, rows=rows, M=M)


def run_variant(eng, s, kw, warmup, steps):
    torch, ctx = eng.torch, eng.ctx
    for _ in range(warmup):
        s["sh"].update(s["X"], s["post"], s["idx"], s["wts"], s["ob"], s["glat"], s["glon"], **kw)
    torch.cuda.synchronize()
    ctx.last_timing()
    gc.collect()
    gc.disable()
    try:
        t0 = time.perf_counter()
        for _ in range(steps):
            s["sh"].update(s["X"], s["post"], s["idx"], s["wts"], s["ob"], s["glat"], s["glon"], **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        gc.enable()
    t = ctx.last_timing()
    return dict(state_ms=t["state_ms"] / steps, obs_ms=t["obs_ms"] / steps, wall_ms=1e3 * wall / steps,
                launches=t["state_launches"] / steps, path=t["path"])


def measure(eng, name, wl, rounds, warmup, steps):
    s = setup(eng, wl)
    res = {v: [] for v, _ in VARIANTS}
    for r in range(rounds):
        for v, kw in VARIANTS:
            res[v].append(run_variant(eng, s, kw, warmup, steps))
            print("%-9s round %d %-5s state %.3f ms  obs %.3f ms  wall %.3f ms  launches %.1f" %
                  (name, r, v, res[v][-1]["state_ms"], res[v][-1]["obs_ms"], res[v][-1]["wall_ms"], res[v][-1]["launches"]),
                  flush=True)
    rows, M = s["rows"], s["M"]
    state_bytes = rows * M * 8.0
    out = dict(workload=name, rows=rows, M=M, P=wl["P"], loc=wl["loc"], rounds=rounds, warmup=warmup, steps=steps, variants={})
    base = np.array([x["state_ms"] for x in res["none"]])
    for v, _ in VARIANTS:
        st = np.array([x["state_ms"] for x in res[v]])
        wa = np.array([x["wall_ms"] for x in res[v]])
        e = dict(state_ms=[round(x, 4) for x in st], wall_ms=[round(x, 4) for x in wa],
                 state_ms_median=float(np.median(st)), wall_ms_median=float(np.median(wa)),
                 launches=res[v][0]["launches"], path=res[v][0]["path"],
                 state_vs_none_pct=float(100.0 * (np.median(st) / np.median(base) - 1.0)))
        if v != "none" and wl["loc"] == "GC":
            # standalone passes: row spread reads the prior; RTPS relax reads + writes the posterior, RTPP also reads the prior
            moved = state_bytes * (1 + 2) if v == "rtps" else state_bytes * 3
            added = float(np.median(st) - np.median(base))
            e["standalone_bytes"] = moved
            if added > 0:
                e["standalone_GBps"] = moved / (added * 1e-3) / 1e9
                e["standalone_hbm_peak_fraction"] = e["standalone_GBps"] / HBM_PEAK_GBPS
        out["variants"][v] = e
    del s
    eng.torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gc", default="cfg3", help="localised size for the standalone passes: cfg3 | small_gc | none")
    ap.add_argument("--headline-rows", type=int, default=None, help="override the headline's 1e7 rows (quick checks)")
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    from efa_xray_amd.distributed import HipEngine
    eng = HipEngine(0)
    eng.ctx.set_option("timing", 2)
    results = []
    hl = dict(SIZES["headline"])
    if a.headline_rows:
        hl["ncol"] = a.headline_rows
    results.append(measure(eng, "headline", hl, a.rounds, a.warmup, a.steps))
    if a.gc != "none":
        results.append(measure(eng, a.gc, SIZES[a.gc], a.rounds, a.warmup, a.steps))
    for r in results:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
