"""Cost of efa_neighbourhood_dev against efa_products_dev's probability pass and against a pass that reads the same
rows once.

One process, alternating round by round (warm-up + timed calls per variant and round):
  "sens"    the read yardstick: efa_sensitivity_dev with K = 1, n_targets = 0 and only `var` wanted, read-only option "sens_us" --
            one pass of k_sens_pass over the float64 rows;
  "probs"   "products_us" of efa_products_dev with the same four thresholds, probabilities only (the field prob, nothing else);
  "neighbourhood_us" of efa_neighbourhood_dev with four thresholds, for the radii {0}, {2}, {8} and {2, 8, 32}, both shapes, and
  three sets of outputs: "nep" (the field NEP), "nep_nmep" (NEP and NMEP) and "fss" (no field, the sums of the skill score).
Shapes: configs[2]'s state, 38 468 160 rows x 80 members as 148 slabs of 361 x 720, and 10^7 rows x 100 members as 100 slabs of
250 x 400 (float64).  Clocks are whatever the device runs at under this load (not pinned); medians of the rounds' medians are
reported with every round beside them.

    python tools/neighbourhood_cost.py [--rounds 3] [--steps 3] [--warmup 1] [--sizes cfg2,e7] [--json profiles/neighbourhood_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {
    "cfg2": dict(n_lead=148, ny=361, nx=720, M=80),
    "e7": dict(n_lead=100, ny=250, nx=400, M=100),
    "small": dict(n_lead=16, ny=90, nx=180, M=80),
}
THRESHOLDS = (-3.0, -1.0, 1.0, 3.0)
RADII = ((0,), (2,), (8,), (2, 8, 32))
SHAPES = ("square", "disc")
OUTPUTS = ("nep", "nep_nmep", "fss")


def setup(ctx, wl, seed=1):
    M, n_lead, ncol = wl["M"], wl["n_lead"], wl["ny"] * wl["nx"]
    rows = n_lead * ncol
    rng = np.random.default_rng(7000 + seed)
    X = ctx.empty((rows, M))
    ctx.fill_synthetic(rows, 0, M, seed, 3.0, X)
    y = ctx.to_device(3.0 * rng.standard_normal(rows))
    nf = max(len(r) for r in RADII) * len(THRESHOLDS)
    return dict(rows=rows, M=M, n_lead=n_lead, ncol=ncol, ny=wl["ny"], nx=wl["nx"], X=X, y=y, sg=(np.arange(n_lead) * 4) // n_lead,
                J=rng.standard_normal((1, M)), thr=np.tile(np.array(THRESHOLDS), (n_lead, 1)), var=ctx.empty((rows,)),
                nep=ctx.empty((nf, rows)), nmep=ctx.empty((nf, rows)))


def run_sens(ctx, s, warmup, steps):
    us = []
    for i in range(warmup + steps):
        ctx.sensitivity(s["rows"], s["M"], s["X"], s["J"], np.ones(s["n_lead"]), ncol=s["ncol"], n_lead=s["n_lead"], n_targets=0,
                        var=s["var"])
        if i >= warmup:
            us.append(ctx.get_option("sens_us"))
    return 1e-3 * float(np.median(us))


def run_probs(ctx, s, warmup, steps):
    us = []
    for i in range(warmup + steps):
        ctx.products(s["rows"], s["M"], s["X"], ncol=s["ncol"], n_lead=s["n_lead"], thresholds=s["thr"], prob=s["nep"])
        if i >= warmup:
            us.append(ctx.get_option("products_us"))
    return 1e-3 * float(np.median(us))


def run_neighbourhood(ctx, s, radii, shape, outputs, warmup, steps):
    kw = dict(shape=SHAPES.index(shape))
    if outputs in ("nep", "nep_nmep"):
        kw.update(nep=s["nep"])
    if outputs == "nep_nmep":
        kw.update(nmep=s["nmep"])
    if outputs == "fss":
        kw.update(verif=s["y"], slab_group=s["sg"])
    us = []
    for i in range(warmup + steps):
        res = ctx.neighbourhood(s["rows"], s["M"], s["X"], s["ny"], s["nx"], s["n_lead"], s["thr"], radii, **kw)
        if res is not None:
            sums, n, n_bad = res
            assert np.all(n.sum(axis=0) == s["rows"]) and n_bad.sum() == 0
        if i >= warmup:
            us.append(ctx.get_option("neighbourhood_us"))
    return 1e-3 * float(np.median(us))


def measure(ctx, name, wl, rounds, warmup, steps):
    s = setup(ctx, wl)
    res = {"sens": [], "probs": []}
    for r in range(rounds):
        res["sens"].append(run_sens(ctx, s, warmup, steps))
        res["probs"].append(run_probs(ctx, s, warmup, steps))
        for radii in RADII:
            for shape in SHAPES:
                for outputs in OUTPUTS:
                    key = "r%s_%s_%s" % ("+".join(str(x) for x in radii), shape, outputs)
                    res.setdefault(key, []).append(run_neighbourhood(ctx, s, radii, shape, outputs, warmup, steps))
        print("%-6s round %d: %s" % (name, r, " ".join("%s %.3f ms" % (k, v[-1]) for k, v in sorted(res.items()))), flush=True)
    med = dict((k, float(np.median(v))) for k, v in res.items())
    out = dict(workload=name, rows=s["rows"], M=s["M"], n_lead=s["n_lead"], ny=s["ny"], nx=s["nx"], rounds=rounds, warmup=warmup,
               steps=steps, clocks="not pinned", thresholds=THRESHOLDS, ms=dict((k, [round(x, 4) for x in v]) for k, v in res.items()),
               ms_median=med, sens_tb_per_s=8.0 * s["rows"] * s["M"] / (1e-3 * med["sens"]) / 1e12)
    for key, v in med.items():
        if key not in ("sens", "probs"):
            out[key] = dict(ms=v, over_sens=v / med["sens"], over_probs=v / med["probs"])
    print(json.dumps(out), flush=True)
    for a in (s["X"], s["y"], s["var"], s["nep"], s["nmep"]):
        a.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="cfg2,e7")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "neighbourhood_cost.json"))
    a = ap.parse_args()
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    results = [measure(ctx, name, SIZES[name], a.rounds, a.warmup, a.steps) for name in a.sizes.split(",")]
    with open(a.json, "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
