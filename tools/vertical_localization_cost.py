"""Cost of vertical localisation on device-resident localised cycles.

Times efa_ensrf_cycle_dev with vertical localisation off, on with a half-width so wide that no vertical factor is zero ("wide"),
and on with one scale height in ln p ("tight"), in ONE process, alternating the variants round by round (warm-up + timed cycles
per variant and round), on a configs[2]-like cycle: 4 variables x 37 levels x 361 x 720 rows x 80 members x 5 000 obs, GC
1 000 km, the levels on the time slot with ln p (1000 .. 10 hPa) as the slabs' coordinate and every fourth-variable surface
slab NaN.  The state phase (HIP events, "timing" 2) is reported per variant: off it is the plain one-pass sweep
(k_sweep_gc_lane, family 0), on it is family 2 of the same kernel.  "skipped_pairs" is the fraction of (group of 16 slabs, ob) pairs none of whose
slabs is within an ob's vertical reach: the share of (wave, ob) pairs of the lane form that the vertical factor removes on top of
the horizontal skipping (from the geometry, on the host).

    python tools/vertical_localization_cost.py [--rounds 3] [--steps 10] [--warmup 2] [--sizes cfg2] [--json out.json]
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
HALFWIDTH = {"wide": 100.0, "tight": 1.0}  # in ln p: the column spans ln(100) = 4.6, so 100 leaves every factor > 0


def setup(ctx, wl, seed=1):
    M, P, nvar, nlev = wl["M"], wl["P"], wl["nvar"], wl["nlev"]
    n_lead = nvar * nlev
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
    lnp = np.log(np.geomspace(1000.0, 10.0, nlev))
    lead = np.tile(lnp, nvar)
    lead[(nvar - 1) * nlev] = np.nan               # a surface field kept in the 3-D state
    ob_vert = lead[pick // ncol]                   # each ob at its own slab's level
    ob_vert = np.where(np.isnan(ob_vert), lnp[0], ob_vert)
    return dict(X=X, post=post, Yp=Yp, ym=ym, val=val, err=np.ones(P), assim=np.ones(P, dtype=bool), lat=glat[col],
                lon=glon[col], hw=np.full(P, wl["radius_km"]), glat=glat, glon=glon, rows=rows, M=M, P=P, n_lead=n_lead,
                lead=lead, ob_vert=ob_vert)


def cycle(ctx, s):
    ctx.ensrf_cycle(s["rows"], s["M"], s["P"], s["X"], s["post"], s["ym"], s["Yp"], s["val"], s["err"], s["assim"], 1,
                    s["lat"], s["lon"], s["hw"], s["glat"], s["glon"], s["n_lead"])


def skipped_pairs(s, c):
    lead, zk = s["lead"], s["ob_vert"]
    groups = [lead[g:g + 16] for g in range(0, len(lead), 16)]
    skip = 0
    for grp in groups:
        d = np.abs(grp[None, :] - zk[:, None])
        reach = (d < 2.0 * c) | np.isnan(grp)[None, :]
        skip += int((~reach.any(axis=1)).sum())
    return skip / float(len(groups) * len(zk))


def run_variant(ctx, s, v, warmup, steps):
    if v != "off":
        ctx.set_vertical_localization(s["lead"], s["ob_vert"], np.full(s["P"], HALFWIDTH[v]))
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
        ctx.set_vertical_localization(None)
    t = ctx.last_timing()
    return dict(state_ms=t["state_ms"] / steps, obs_ms=t["obs_ms"] / steps, wall_ms=1e3 * wall / steps,
                launches=t["state_launches"] / steps)


def measure(ctx, name, wl, rounds, warmup, steps):
    s = setup(ctx, wl)
    variants = ("off", "wide", "tight")
    res = {v: [] for v in variants}
    for r in range(rounds):
        for v in variants:
            res[v].append(run_variant(ctx, s, v, warmup, steps))
            x = res[v][-1]
            print("%-6s round %d %-5s state %.3f ms  obs %.3f ms  wall %.3f ms  launches %.1f" %
                  (name, r, v, x["state_ms"], x["obs_ms"], x["wall_ms"], x["launches"]), flush=True)
    out = dict(workload=name, rows=s["rows"], M=s["M"], P=s["P"], n_lead=s["n_lead"], rounds=rounds, warmup=warmup, steps=steps,
               halfwidth_lnp=HALFWIDTH, variants={})
    for v in variants:
        st = np.array([x["state_ms"] for x in res[v]])
        ob = np.array([x["obs_ms"] for x in res[v]])
        wa = np.array([x["wall_ms"] for x in res[v]])
        out["variants"][v] = dict(state_ms=[round(x, 4) for x in st], obs_ms=[round(x, 4) for x in ob], wall_ms=[round(x, 4) for x in wa],
                                  state_ms_median=float(np.median(st)), obs_ms_median=float(np.median(ob)),
                                  wall_ms_median=float(np.median(wa)), launches=res[v][0]["launches"])
        if v != "off":
            out["variants"][v]["state_over_off"] = float(np.median(st)) / out["variants"]["off"]["state_ms_median"]
            out["variants"][v]["skipped_pairs"] = skipped_pairs(s, HALFWIDTH[v])
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
