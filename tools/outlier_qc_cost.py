"""Cost of the outlier check on device-resident cycles.

Times efa_ensrf_cycle_dev (ShardedEnSRF at world size 1, as bench.py drives it) with the check off and on (threshold 3) in
ONE process, alternating the two round by round (3 warm-up + 20 timed cycles per variant and round), on
  - the headline: 1e7 state rows x 100 members x 1e4 obs, loc=None, synthetic state (efa_fill_synthetic_dev);
  - a configs[2]-like localised size (--gc cfg3: 4 x 37 x 361 x 720 rows x 80 members x 5000 obs, GC 1000 km).
About 1 % of the obs carry a gross error (+-8 prior-plus-ob standard deviations); the check rejects them, so "on" also
assimilates 1 % fewer obs.  Prints per variant the library's obs-phase (prep launch .. Phase A's results on the host) and
state-phase times per cycle (HIP events, "timing" 2) and the wall time per cycle.  Run it under
`rocprofv3 --kernel-trace --stats` for the prep kernels' own times.

    python tools/outlier_qc_cost.py [--rounds 3] [--steps 20] [--warmup 3] [--gc cfg3|small_gc|none] [--json out.json]
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

SIZES = {
    "headline": dict(n_lead=1, ncol=10_000_000, M=100, P=10_000, loc=None),
    "cfg3": dict(n_lead=148, ny=361, nx=720, M=80, P=5_000, loc="GC", radius_km=1000.0),
    "small_gc": dict(n_lead=8, ny=90, nx=180, M=40, P=300, loc="GC", radius_km=1000.0),
}
THRESHOLD = 3.0
VARIANTS = (("off", None), ("on", THRESHOLD))


def setup(eng, wl, seed=1, gross=0.01):
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
    hx = HX.cpu().numpy()
    ym, sd = hx.mean(axis=1), np.sqrt(hx.var(axis=1) + err)
    value = ym + np.random.default_rng(4000 + seed).standard_normal(P)
    bad = rng.choice(P, max(1, int(gross * P)), replace=False)
    value[bad] = ym[bad] + np.where(rng.random(bad.size) < 0.5, -8.0, 8.0) * sd[bad]
    ob["value"] = value
    kept = (value - ym) ** 2 <= THRESHOLD ** 2 * sd ** 2
    return dict(sh=sh, X=X, post=post, idx=idx, wts=wts, ob=ob, glat=glat, glon=glon, rows=rows, M=M,
                gross=int(bad.size), rejected_expected=int(P - kept.sum()))


def run_variant(eng, s, t, warmup, steps):
    torch, ctx = eng.torch, eng.ctx
    kw = dict(outlier_threshold=t)
    for _ in range(warmup):
        diag = s["sh"].update(s["X"], s["post"], s["idx"], s["wts"], s["ob"], s["glat"], s["glon"], **kw)
    torch.cuda.synchronize()
    ctx.last_timing()
    gc.collect()
    gc.disable()
    try:
        t0 = time.perf_counter()
        for _ in range(steps):
            diag = s["sh"].update(s["X"], s["post"], s["idx"], s["wts"], s["ob"], s["glat"], s["glon"], **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        gc.enable()
    tm = ctx.last_timing()
    rejected = int(np.sum(np.asarray(s["ob"]["assim"], bool) & ~np.asarray(diag["assimilated"], bool)))
    return dict(state_ms=tm["state_ms"] / steps, obs_ms=tm["obs_ms"] / steps, wall_ms=1e3 * wall / steps, path=tm["path"],
                rejected=rejected)


def measure(eng, name, wl, rounds, warmup, steps):
    s = setup(eng, wl)
    res = {v: [] for v, _ in VARIANTS}
    try:
        for r in range(rounds):
            for v, t in VARIANTS:
                res[v].append(run_variant(eng, s, t, warmup, steps))
                x = res[v][-1]
                print("%-9s round %d %-3s obs %.3f ms  state %.3f ms  wall %.3f ms  rejected %d" %
                      (name, r, v, x["obs_ms"], x["state_ms"], x["wall_ms"], x["rejected"]), flush=True)
    finally:
        eng.ctx.set_outlier_threshold(None)
    out = dict(workload=name, rows=s["rows"], M=s["M"], P=wl["P"], loc=wl["loc"], threshold=THRESHOLD, gross_errors=s["gross"],
               rejected_expected=s["rejected_expected"], rounds=rounds, warmup=warmup, steps=steps, variants={})
    for v, _ in VARIANTS:
        e = {}
        for key in ("obs_ms", "state_ms", "wall_ms"):
            a = np.array([x[key] for x in res[v]])
            e[key] = [round(float(x), 4) for x in a]
            e[key + "_median"] = float(np.median(a))
            e[key + "_spread"] = float(a.max() - a.min())
        e["rejected"] = res[v][0]["rejected"]
        e["path"] = res[v][0]["path"]
        out["variants"][v] = e
    for key in ("obs_ms", "wall_ms"):
        d = [b - a for a, b in zip(out["variants"]["off"][key], out["variants"]["on"][key])]
        out["on_minus_off_" + key] = [round(x, 4) for x in d]
        out["on_minus_off_%s_median_us" % key[:-3]] = float(1e3 * np.median(d))
    del s
    eng.torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gc", default="cfg3", help="localised size: cfg3 | small_gc | none")
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
