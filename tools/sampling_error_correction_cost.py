"""Cost of sampling error correction (Anderson 2012) on device-resident localised cycles.

Times efa_ensrf_cycle_dev with the correction off and on in ONE process, alternating the two round by round (warm-up + timed
cycles per variant and round), on
  - cfg2: a configs[2]-like cycle, 4 x 37 x 361 x 720 rows x 80 members x 5 000 obs, GC 1 000 km;
  - cfg3: a configs[3]-sized cycle on one GPU, the same grid x 100 members x 10 000 obs.
Off is the plain one-pass sweep behind the persistent Phase A -- the kernels every cycle ran before the correction existed, which
the code-object comparison of tests/_codeobj.py shows unchanged.  On, the state phase (HIP events, "timing" 2) is the kGcSec sweep
with the per-ob record pass (k_adapt_obs) and Phase A runs its per-batch kernels one ob at a time: the state-phase ratio on / off
and Phase A's time per ob on either route are reported, and (column, ob) pairs per second for the estimate of the extra
arithmetic.  Run it under `rocprofv3 --kernel-trace --stats` for per-kernel times.

    python tools/sampling_error_correction_cost.py [--rounds 3] [--steps 8] [--warmup 2] [--sizes cfg2,cfg3] [--json out.json]
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
    "cfg2": dict(n_lead=148, ny=361, nx=720, M=80, P=5_000, radius_km=1000.0),
    "cfg3": dict(n_lead=148, ny=361, nx=720, M=100, P=10_000, radius_km=1000.0),
    "small": dict(n_lead=8, ny=90, nx=180, M=40, P=300, radius_km=1000.0),
}


def setup(ctx, wl, seed=1):
    from efa_xray_amd import sampling_error_table
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
    col = pick % ncol
    return dict(X=X, post=post, HX=HX, Yp=ctx.empty((P, M)), ym=ctx.empty((P,)), val=val, err=np.ones(P), assim=np.ones(P, dtype=bool),
                lat=glat[col], lon=glon[col], hw=np.full(P, wl["radius_km"]), glat=glat, glon=glon, rows=rows, M=M, P=P,
                n_lead=n_lead, table=sampling_error_table(M))


def cycle(ctx, s):
    ctx.ensrf_cycle(s["rows"], s["M"], s["P"], s["X"], s["post"], s["ym"], s["Yp"], s["val"], s["err"], s["assim"], 1,
                    s["lat"], s["lon"], s["hw"], s["glat"], s["glon"], s["n_lead"])


def run_variant(ctx, s, on, warmup, steps):
    ctx.set_sampling_error_correction(s["table"] if on else None)
    try:
        s["Yp"].upload(s["HX"])
        ctx.form_perts(s["P"], s["M"], s["Yp"], s["ym"], s["Yp"])
        for _ in range(warmup):
            cycle(ctx, s)
        ctx.synchronize()
        ctx.last_timing()
        t0 = time.perf_counter()
        for _ in range(steps):
            cycle(ctx, s)
        ctx.synchronize()
        wall = time.perf_counter() - t0
        kind, fam, form = ctx.get_option("phase_a_kind"), ctx.get_option("gc_family"), ctx.get_option("gc_form")
        pairs = ctx.get_option("gc_active_pairs")
    finally:
        ctx.set_sampling_error_correction(None)
    assert (kind == 2 and fam == 4) if on else (kind != 2 and fam == 0), (on, kind, fam)
    t = ctx.last_timing()
    return dict(state_ms=t["state_ms"] / steps, obs_ms=t["obs_ms"] / steps, wall_ms=1e3 * wall / steps,
                launches=t["state_launches"] / steps, phase_a_kind=kind, gc_form=form, pairs=pairs)


def measure(ctx, name, wl, rounds, warmup, steps):
    s = setup(ctx, wl)
    res = {"off": [], "on": []}
    for r in range(rounds):
        for v in ("off", "on"):
            res[v].append(run_variant(ctx, s, v == "on", warmup, steps))
            x = res[v][-1]
            print("%-6s round %d %-3s state %.3f ms  obs %.3f ms  wall %.3f ms  launches %.1f  phase A kind %d" %
                  (name, r, v, x["state_ms"], x["obs_ms"], x["wall_ms"], x["launches"], x["phase_a_kind"]), flush=True)
    out = dict(workload=name, rows=s["rows"], M=s["M"], P=s["P"], rounds=rounds, warmup=warmup, steps=steps, table_nodes=int(s["table"].size),
               column_ob_pairs=res["on"][0]["pairs"], gc_form=res["on"][0]["gc_form"], variants={})
    for v in ("off", "on"):
        st = np.array([x["state_ms"] for x in res[v]])
        ob = np.array([x["obs_ms"] for x in res[v]])
        wa = np.array([x["wall_ms"] for x in res[v]])
        out["variants"][v] = dict(state_ms=[round(x, 4) for x in st], obs_ms=[round(x, 4) for x in ob], wall_ms=[round(x, 4) for x in wa],
                                  state_ms_median=float(np.median(st)), obs_ms_median=float(np.median(ob)),
                                  wall_ms_median=float(np.median(wa)), launches=res[v][0]["launches"],
                                  phase_a_kind=res[v][0]["phase_a_kind"],
                                  phase_a_us_per_ob=float(1e3 * np.median(ob) / s["P"]))
    on, off = out["variants"]["on"], out["variants"]["off"]
    out["state_on_over_off"] = on["state_ms_median"] / off["state_ms_median"]
    out["phase_a_on_over_off"] = on["obs_ms_median"] / off["obs_ms_median"]
    out["phase_a_share_of_cycle_on"] = on["obs_ms_median"] / (on["obs_ms_median"] + on["state_ms_median"])
    # (row, ob) pairs: every (column, ob) pair with a non-zero taper, on each slab
    out["row_ob_pairs_per_s_on"] = out["column_ob_pairs"] * s["n_lead"] / (on["state_ms_median"] * 1e-3)
    out["row_ob_pairs_per_s_off"] = out["column_ob_pairs"] * s["n_lead"] / (off["state_ms_median"] * 1e-3)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="cfg2,cfg3")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sampling_error_correction_cost.json"), help="where the results go")
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
