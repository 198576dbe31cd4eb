"""Cost of efa_products_dev against efa_verify_dev and against a pass that reads the same rows once.

One process, alternating round by round (warm-up + timed calls per variant and round):
  "sens"    the read yardstick: efa_sensitivity_dev with K = 1, n_targets = 0 and only `var` wanted, read-only option "sens_us" --
            one pass of k_sens_pass over the float64 rows;
  "verify"  "verify_us" of efa_verify_dev / efa_verify_f32_dev with every group output and no per-row field;
  "products_us" of efa_products_dev / efa_products_f32_dev in four variants:
    "moments"   mean + sd only
    "probs"     4 thresholds with verification (table, n_bad, sums; no per-row field), no quantile: the kernel without the sort
    "quantiles" quantiles (0.1, 0.5, 0.9)
    "all"       mean, sd, the three quantiles, the four probabilities and the verification at once
Shapes: 10^7 rows x 100 members (float64) and configs[2]'s state, 38 468 160 rows x 80 members (float64 and float32).  Clocks are
whatever the device runs at under this load (not pinned); medians of the rounds' medians are reported with every round beside them.

    python tools/products_cost.py [--rounds 3] [--steps 5] [--warmup 1] [--sizes e7,cfg2] [--json profiles/products_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {
    "e7": dict(n_lead=40, ncol=250000, M=100, dtypes=("float64",)),
    "cfg2": dict(n_lead=148, ncol=361 * 720, M=80, dtypes=("float64", "float32")),
    "small": dict(n_lead=16, ncol=90 * 180, M=80, dtypes=("float64", "float32")),
}
HBM_PEAK = 8.0e12
QS = (0.1, 0.5, 0.9)
THRESHOLDS = (-3.0, -1.0, 1.0, 3.0)
VARIANTS = ("moments", "probs", "quantiles", "all")


def setup(ctx, wl, seed=1):
    M, n_lead, ncol = wl["M"], wl["n_lead"], wl["ncol"]
    rows = n_lead * ncol
    rng = np.random.default_rng(7000 + seed)
    X = {}
    X["float64"] = ctx.empty((rows, M))
    ctx.fill_synthetic(rows, 0, M, seed, 3.0, X["float64"])
    if "float32" in wl["dtypes"]:
        X["float32"] = ctx.empty((rows, M), np.float32)
        blk = 1 << 20
        z = rng.standard_normal((min(blk, rows), M)).astype(np.float32)
        for i, r0 in enumerate(range(0, rows, blk)):
            X["float32"].upload_rows(r0, (z[:min(blk, rows - r0)] * np.float32(1.0 + 0.01 * i)))
    y = ctx.to_device(3.0 * rng.standard_normal(rows))
    s = dict(rows=rows, M=M, n_lead=n_lead, ncol=ncol, X=X, y=y, sg=(np.arange(n_lead) * 4) // n_lead, J=rng.standard_normal((1, M)),
             thr=np.tile(np.array(THRESHOLDS), (n_lead, 1)))
    # the fields of the widest variant, allocated once; `var` doubles as the yardstick's output
    s["mean"], s["sd"] = ctx.empty((rows,)), ctx.empty((rows,))
    s["quant"], s["prob"] = ctx.empty((len(QS), rows)), ctx.empty((len(THRESHOLDS), rows))
    return s


def run_sens(ctx, s, warmup, steps):
    us = []
    for i in range(warmup + steps):
        ctx.sensitivity(s["rows"], s["M"], s["X"]["float64"], s["J"], np.ones(s["n_lead"]), ncol=s["ncol"], n_lead=s["n_lead"],
                        n_targets=0, var=s["mean"])
        if i >= warmup:
            us.append(ctx.get_option("sens_us"))
    return 1e-3 * float(np.median(us))


def run_verify(ctx, s, dtype, warmup, steps):
    us = []
    for i in range(warmup + steps):
        hist, n, n_bad, _ = ctx.verify(s["rows"], s["M"], s["X"][dtype], s["y"], s["sg"], ncol=s["ncol"], n_lead=s["n_lead"], seed=i)
        assert hist.sum() == n.sum() == s["rows"] and n_bad.sum() == 0
        if i >= warmup:
            us.append(ctx.get_option("verify_us"))
    return 1e-3 * float(np.median(us))


def run_products(ctx, s, dtype, variant, warmup, steps):
    kw = dict(ncol=s["ncol"], n_lead=s["n_lead"])
    if variant in ("moments", "all"):
        kw.update(mean=s["mean"], sd=s["sd"])
    if variant in ("quantiles", "all"):
        kw.update(quantiles=QS, quant=s["quant"])
    if variant in ("probs", "all"):
        kw.update(thresholds=s["thr"], verif=s["y"], slab_group=s["sg"])
    if variant == "all":
        kw.update(prob=s["prob"])
    us = []
    for i in range(warmup + steps):
        res = ctx.products(s["rows"], s["M"], s["X"][dtype], **kw)
        if res is not None:
            table, n_bad, _ = res
            assert np.all(table.sum(axis=(0, 2, 3)) == s["rows"]) and n_bad.sum() == 0
        if i >= warmup:
            us.append(ctx.get_option("products_us"))
    return 1e-3 * float(np.median(us))


def measure(ctx, name, wl, rounds, warmup, steps):
    s = setup(ctx, wl)
    res = {"sens": []}
    for r in range(rounds):
        res["sens"].append(run_sens(ctx, s, warmup, steps))
        for dtype in wl["dtypes"]:
            res.setdefault("verify_" + dtype, []).append(run_verify(ctx, s, dtype, warmup, steps))
            for v in VARIANTS:
                res.setdefault("%s_%s" % (v, dtype), []).append(run_products(ctx, s, dtype, v, warmup, steps))
        print("%-6s round %d: %s" % (name, r, " ".join("%s %.3f ms" % (k, v[-1]) for k, v in sorted(res.items()))), flush=True)
    med = dict((k, float(np.median(v))) for k, v in res.items())
    out = dict(workload=name, rows=s["rows"], M=s["M"], n_lead=s["n_lead"], rounds=rounds, warmup=warmup, steps=steps,
               hbm_peak_tb_per_s=HBM_PEAK / 1e12, clocks="not pinned", quantiles=QS, thresholds=THRESHOLDS,
               ms=dict((k, [round(x, 4) for x in v]) for k, v in res.items()), ms_median=med,
               sens_tb_per_s=8.0 * s["rows"] * s["M"] / (1e-3 * med["sens"]) / 1e12)
    for dtype, size in (("float64", 8), ("float32", 4)):
        if "verify_" + dtype not in med:
            continue
        nbytes = float(size) * s["rows"] * s["M"]
        for v in VARIANTS:
            key = "%s_%s" % (v, dtype)
            out[key] = dict(ms=med[key], over_sens=med[key] / med["sens"], over_verify=med[key] / med["verify_" + dtype],
                            read_tb_per_s=nbytes / (1e-3 * med[key]) / 1e12)
    print(json.dumps(out), flush=True)
    for a in list(s["X"].values()) + [s["y"], s["mean"], s["sd"], s["quant"], s["prob"]]:
        a.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="e7,cfg2")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "products_cost.json"))
    a = ap.parse_args()
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    results = [measure(ctx, name, SIZES[name], a.rounds, a.warmup, a.steps) for name in a.sizes.split(",")]
    with open(a.json, "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
