"""Cost of the batch observation-space solver (ETKF) against the serial Phase A on device-resident cycles.

Times efa_ensrf_cycle_dev (ShardedEnSRF at world size 1, as bench.py drives it) with option "obs_solver" 0 (serial) and 1
(batch) in ONE process, alternating the two round by round (3 warm-up + 20 timed cycles per variant and round), on resident
synthetic states (efa_fill_synthetic_dev), loc=None:
  - the headline: 1e7 state rows x 100 members x 1e4 obs;
  - configs[1]:   512^2 state rows x 50 members x 1000 obs;
  - wide:         1e6 state rows x 256 members x 1e4 obs (the eigen-solve in global memory, the transform in column groups).
Prints per variant the library's obs-phase time (prep launch .. results on the host) and state-phase time per cycle (HIP
events, "timing" 2), the wall time per cycle, each round's on-minus-off delta and the medians.  The two variants are different
filters: this compares their cost, not their results.  `--parent-phase-a a,b,c` records the parent commit's
Phase A times at the headline (bench.py's JSON, "phase_a" / "ms", three runs on the same machine) beside the batch obs phase,
with their ratio.  Run it under `rocprofv3 --kernel-trace --stats` (a run of its own, --rounds 1) for the kernels' own times.

    python tools/etkf_cost.py [--rounds 3] [--steps 20] [--warmup 3] [--sizes headline,cfg2,wide] [--parent-phase-a a,b,c] [--json out.json]
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
    "headline": dict(rows=10_000_000, M=100, P=10_000),
    "cfg2": dict(rows=512 * 512, M=50, P=1_000),
    "wide": dict(rows=1_000_000, M=256, P=10_000),
}
VARIANTS = (("serial", 0), ("batch", 1))


def setup(eng, wl, seed=1):
    from efa_xray_amd.distributed import ShardedEnSRF
    torch = eng.torch
    rows, M, P = wl["rows"], wl["M"], wl["P"]
    sh = ShardedEnSRF(eng, 1, rows, M)
    rng = np.random.default_rng(3000 + seed)
    pick = rng.choice(rows, P, replace=False).astype(np.int64)
    idx, wts = pick[:, None].copy(), np.ones((P, 1))
    X = eng.empty((rows, M))
    post = eng.empty((rows, M))
    eng.ctx.fill_synthetic(rows, 0, M, seed, 3.0, X.data_ptr())
    HX = sh.partial_estimates(X, idx, wts)
    torch.cuda.synchronize()
    ym = HX.cpu().numpy().mean(axis=1)
    ob = dict(value=ym + np.random.default_rng(4000 + seed).standard_normal(P), error=np.ones(P), assim=np.ones(P, dtype=bool))
    return dict(sh=sh, X=X, post=post, idx=idx, wts=wts, ob=ob, rows=rows, M=M)


def run_variant(eng, s, solver, warmup, steps):
    torch, ctx = eng.torch, eng.ctx
    ctx.set_option("obs_solver", solver)
    for _ in range(warmup):
        s["sh"].update(s["X"], s["post"], s["idx"], s["wts"], s["ob"])
    torch.cuda.synchronize()
    ctx.last_timing()
    gc.collect()
    gc.disable()
    try:
        t0 = time.perf_counter()
        for _ in range(steps):
            s["sh"].update(s["X"], s["post"], s["idx"], s["wts"], s["ob"])
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        gc.enable()
    tm = ctx.last_timing()
    out = dict(state_ms=tm["state_ms"] / steps, obs_ms=tm["obs_ms"] / steps, wall_ms=1e3 * wall / steps, path=tm["path"],
               phase_a_kind=ctx.get_option("phase_a_kind"))
    if solver:
        out["sweeps"] = ctx.etkf_solution(s["M"])["sweeps"]
    return out


def measure(eng, name, wl, rounds, warmup, steps):
    s = setup(eng, wl)
    res = {v: [] for v, _ in VARIANTS}
    try:
        for r in range(rounds):
            for v, solver in VARIANTS:
                res[v].append(run_variant(eng, s, solver, warmup, steps))
                x = res[v][-1]
                print("%-9s round %d %-6s obs %.3f ms  state %.3f ms  wall %.3f ms  kind %d" %
                      (name, r, v, x["obs_ms"], x["state_ms"], x["wall_ms"], x["phase_a_kind"]), flush=True)
    finally:
        eng.ctx.set_option("obs_solver", 0)
    out = dict(workload=name, rows=s["rows"], M=s["M"], P=wl["P"], loc=None, rounds=rounds, warmup=warmup, steps=steps, variants={})
    for v, _ in VARIANTS:
        e = {}
        for key in ("obs_ms", "state_ms", "wall_ms"):
            a = np.array([x[key] for x in res[v]])
            e[key] = [round(float(x), 4) for x in a]
            e[key + "_median"] = float(np.median(a))
            e[key + "_spread"] = float(a.max() - a.min())
        e["path"] = res[v][0]["path"]
        e["phase_a_kind"] = res[v][0]["phase_a_kind"]
        if "sweeps" in res[v][0]:
            e["jacobi_sweeps"] = res[v][0]["sweeps"]
        out["variants"][v] = e
    for key in ("obs_ms", "wall_ms"):
        d = [b - a for a, b in zip(out["variants"]["serial"][key], out["variants"]["batch"][key])]
        out["batch_minus_serial_" + key] = [round(x, 4) for x in d]
        out["batch_minus_serial_%s_median" % key] = float(np.median(d))
    del s
    eng.torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="headline,cfg2,wide")
    ap.add_argument("--headline-rows", type=int, default=None, help="override the headline's 1e7 rows (quick checks)")
    ap.add_argument("--parent-phase-a", default=None, help="the parent commit's phase_a ms at the headline (bench.py), comma separated")
    ap.add_argument("--json", default=None, help="also write the results here")
    a = ap.parse_args()
    from efa_xray_amd.distributed import HipEngine
    eng = HipEngine(0)
    eng.ctx.set_option("timing", 2)
    results = []
    for name in a.sizes.split(","):
        wl = dict(SIZES[name])
        if name == "headline" and a.headline_rows:
            wl["rows"] = a.headline_rows
        results.append(measure(eng, name, wl, a.rounds, a.warmup, a.steps))
    if a.parent_phase_a:
        parent = [float(x) for x in a.parent_phase_a.split(",")]
        for r in results:
            if r["workload"] == "headline":
                batch = r["variants"]["batch"]["obs_ms_median"]
                r["parent_phase_a_ms"] = parent
                r["parent_phase_a_spread_ms"] = max(parent) - min(parent)
                r["batch_obs_ms_over_parent_phase_a"] = batch / float(np.median(parent))
                r["batch_lower_by_more_than_parent_spread"] = bool(min(parent) - batch > max(parent) - min(parent))
    for r in results:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
