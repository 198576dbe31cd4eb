"""Cost of efa_pm_mean_dev against a pass that reads the same rows once, against efa_products_dev's mean pass, and
against rocPRIM's device-wide radix sort of as many keys.

One process, alternating round by round (warm-up + timed calls per variant and round):
  "sens"   the read yardstick: efa_sensitivity_dev with K = 1, n_targets = 0 and only `var` wanted, read-only option "sens_us" --
           one pass of k_sens_pass over the float64 rows;
  "mean"   "products_us" of efa_products_dev with the mean only;
  "pm_us" of efa_pm_mean_dev / efa_pm_mean_f32_dev for the whole-slab pool and for patches of (32, 32), on two fields:
           "t2m"  285 + 8 z, z standard normal: the keys' high bytes are constant and their passes are skipped;
           "bits" finite random bit patterns: every byte of the key varies;
           ranked by member 0 (a field of the same kind as the members, known without a pass of its own).
State: one variable with 4 valid times on configs[2]'s grid, 4 slabs of 361 x 720 rows of 80 members, float64 and float32.
Per variant: the time, its ratio to "sens" and to "mean", pooled keys sorted per second, the radix passes run on the pool (per
batch), and the bytes per second of the paper count -- per key 2 K for the key kernel, K for the scan of the bytes that vary and
3 K per pass (K read by the histogram, K read and K written by the scatter), K the key's bytes -- against the bandwidth the read
yardstick achieves.  tools/rocprim_sort_probe (built from tools/rocprim_sort_probe.hip), when it is there, is run once as a child
process before the context opens the device, on as many keys as the pool holds.  Clocks are whatever the device runs at under
this load (not pinned); medians of the rounds' medians are reported with every round beside them.

    python tools/pm_mean_cost.py [--rounds 3] [--steps 2] [--warmup 1] [--size cfg2x4] [--json profiles/pm_mean_cost.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {
    "cfg2x4": dict(n_lead=4, ny=361, nx=720, M=80),
    "small": dict(n_lead=2, ny=90, nx=180, M=80),
}
PATCHES = {"slab": None, "p32": (32, 32)}
FIELDS = ("t2m", "bits")


def make_field(kind, rows, M, dtype, seed):
    rng = np.random.default_rng(seed)
    if kind == "t2m":
        X = rng.standard_normal((rows, M), dtype=dtype)     # (drawn in the state's own type: a float64 field has a full mantissa)
        X *= 8.0
        X += 285.0
        return X
    if np.dtype(dtype) == np.float64:
        X = rng.integers(0, 2 ** 64, size=(rows, M), dtype=np.uint64).view(np.float64)
    else:
        X = rng.integers(0, 2 ** 32, size=(rows, M), dtype=np.uint32).view(np.float32)
    X[~np.isfinite(X)] = 1.0
    return X


def timed(fn, read, warmup, steps):
    us = []
    for i in range(warmup + steps):
        fn()
        if i >= warmup:
            us.append(read())
    return 1e-3 * float(np.median(us))


def measure(ctx, name, wl, rounds, warmup, steps):
    M, n_lead, ny, nx = wl["M"], wl["n_lead"], wl["ny"], wl["nx"]
    ncol = ny * nx
    rows = n_lead * ncol
    res, passes, rank_passes = {}, {}, {}
    J = np.random.default_rng(1).standard_normal((1, M))
    out = dict(workload=name, rows=rows, M=M, n_lead=n_lead, ny=ny, nx=nx, rounds=rounds, warmup=warmup, steps=steps,
               clocks="not pinned", keys=rows * M, variants={})
    for dname, dtype in (("f64", np.float64), ("f32", np.float32)):
        for kind in FIELDS:
            Xh = make_field(kind, rows, M, dtype, 11)
            X = ctx.to_device(Xh, dtype)
            f = ctx.to_device(Xh[:, 0].astype(np.float64))
            del Xh
            pm, var, mean = ctx.empty((rows,)), ctx.empty((rows,)), ctx.empty((rows,))
            for r in range(rounds):
                if dtype == np.float64:
                    res.setdefault("sens_" + kind, []).append(timed(
                        lambda: ctx.sensitivity(rows, M, X, J, np.ones(n_lead), ncol=ncol, n_lead=n_lead, n_targets=0, var=var),
                        lambda: ctx.get_option("sens_us"), warmup, steps))
                res.setdefault("mean_%s_%s" % (dname, kind), []).append(timed(
                    lambda: ctx.products(rows, M, X, ncol=ncol, n_lead=n_lead, mean=mean),
                    lambda: ctx.get_option("products_us"), warmup, steps))
                for pname, patch in PATCHES.items():
                    key = "pm_%s_%s_%s" % (dname, kind, pname)

                    def call():
                        n_bad = ctx.pm_mean(rows, M, X, ny, nx, n_lead, f, pm, patch=patch)
                        assert n_bad.sum() == 0
                    res.setdefault(key, []).append(timed(call, lambda: ctx.get_option("pm_us"), warmup, steps))
                    passes[key] = ctx.get_option("pm_passes")
                    rank_passes[key] = ctx.get_option("pm_rank_passes")
                print("%s %s %s round %d: %s" % (name, dname, kind, r, " ".join(
                    "%s %.3f ms" % (k, v[-1]) for k, v in sorted(res.items()) if kind in k and (dname in k or k.startswith("sens")))),
                    flush=True)
            for a in (X, f, pm, var, mean):
                a.free()
    med = dict((k, float(np.median(v))) for k, v in res.items())
    out["ms"] = dict((k, [round(x, 4) for x in v]) for k, v in res.items())
    out["ms_median"] = med
    for kind in FIELDS:
        out["sens_tb_per_s_" + kind] = 8.0 * rows * M / (1e-3 * med["sens_" + kind]) / 1e12
    for key, v in med.items():
        if not key.startswith("pm_"):
            continue
        _, dname, kind, pname = key.split("_")
        K = 8 if dname == "f64" else 4
        # the batches of the call: the two pooled buffers of a batch fit 1 GiB (EFA_PM_WS_BYTES)
        per_batch = max(1, min(n_lead, (1 << 30) // (2 * K * M * ncol)))
        batches = -(-n_lead // per_batch)
        p = passes[key] / float(batches)
        nbytes = rows * M * K * (3.0 + 3.0 * p)
        out["variants"][key] = dict(ms=v, over_sens=v / med["sens_" + kind], over_mean=v / med["mean_%s_%s" % (dname, kind)],
                                    keys_per_s=rows * M / (1e-3 * v), pool_passes=p, rank_passes=rank_passes[key] / float(batches),
                                    batches=batches, paper_bytes=nbytes, paper_tb_per_s=nbytes / (1e-3 * v) / 1e12)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", default="cfg2x4")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "pm_mean_cost.json"))
    a = ap.parse_args()
    wl = SIZES[a.size]
    keys = wl["n_lead"] * wl["ny"] * wl["nx"] * wl["M"]
    rocprim = None
    probe = os.path.join(ROOT, "tools", "rocprim_sort_probe")
    if os.path.exists(probe):     # a child of its own, before this process opens the device
        line = subprocess.run([probe, str(keys), "5"], check=True, capture_output=True, text=True, timeout=300).stdout.strip()
        print("rocprim: " + line, flush=True)
        rocprim = json.loads(line.splitlines()[-1])
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    out = measure(ctx, a.size, wl, a.rounds, a.warmup, a.steps)
    out["rocprim"] = rocprim
    if rocprim:
        for key, v in out["variants"].items():
            v["over_rocprim"] = v["ms"] / rocprim["u64_ms" if "_f64_" in key else "u32_ms"]
    print(json.dumps(out), flush=True)
    with open(a.json, "w") as f:
        json.dump([out], f, indent=1)


if __name__ == "__main__":
    main()
