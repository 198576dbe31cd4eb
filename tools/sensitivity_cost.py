"""Cost of one pass of efa_sensitivity_dev against a kernel that reads the same rows once.

One process, alternating round by round (warm-up + timed calls per variant and round) on configs[2]'s state: 4 variables x 37
levels x 361 x 720 = 38 468 160 rows x 80 members, stored as float64 and as float32.
  "impact"  the yardstick: efa_obs_impact_dev with EFA_LOC_NONE, read-only option "impact_us" -- k_impact_z is one read pass over
            the float64 rows (plus two small kernels over P = 16 obs);
  "t0"      "sens_us" of a call with K = 4, n_targets = 1 and no field: exactly one pass at t = 0 and the reduction of the
            workgroups' bests;
  "t12"     one pass at K = 4, t = 12: "sens_us" with n_targets = 13 minus "sens_us" with n_targets = 12 (no field either).
A pass moves rows M elements in and next to nothing out, so its bytes are taken algorithmically: rows M itemsize.  HBM peak: 8.0 TB/s
(the data sheet); a float4 copy reaches 6.29 TB/s on this part.

    python tools/sensitivity_cost.py [--rounds 3] [--steps 5] [--warmup 1] [--sizes cfg2] [--json profiles/sensitivity_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {
    "cfg2": dict(nvar=4, nlev=37, ny=361, nx=720, M=80),
    "small": dict(nvar=2, nlev=8, ny=90, nx=180, M=80),
}
HBM_PEAK = 8.0e12
K, T_LATE, P_OBS = 4, 12, 16


def setup(ctx, wl, seed=1):
    M = wl["M"]
    n_lead, ncol = wl["nvar"] * wl["nlev"], wl["ny"] * wl["nx"]
    rows = n_lead * ncol
    rng = np.random.default_rng(5000 + seed)
    X64 = ctx.empty((rows, M))
    ctx.fill_synthetic(rows, 0, M, seed, 3.0, X64)
    # the float32 copy: one block of random rows, uploaded at a different scale to every position (the pass's time does not
    # depend on the values; a block of its own scale keeps the picks from tying across blocks)
    X32 = ctx.empty((rows, M), np.float32)
    blk = 1 << 20
    z = rng.standard_normal((min(blk, rows), M)).astype(np.float32)
    for i, r0 in enumerate(range(0, rows, blk)):
        X32.upload_rows(r0, (z[:min(blk, rows - r0)] * np.float32(1.0 + 0.01 * i)))
    J = rng.standard_normal((K, M))
    Ya = ctx.to_device(rng.standard_normal((P_OBS, M)))
    return dict(rows=rows, M=M, n_lead=n_lead, ncol=ncol, X={"float64": X64, "float32": X32}, J=J, R=np.ones(n_lead), Ya=Ya,
                werr=ctx.to_device(rng.standard_normal(rows)), innov=rng.standard_normal(P_OBS), err=np.ones(P_OBS),
                used=np.ones(P_OBS, dtype=bool))


def run_impact(ctx, s, warmup, steps):
    us = []
    for i in range(warmup + steps):
        ctx.obs_impact(s["rows"], s["M"], P_OBS, s["X"]["float64"], s["werr"], s["Ya"], s["innov"], s["err"], s["used"], 0)
        if i >= warmup:
            us.append(ctx.get_option("impact_us"))
    return 1e-3 * float(np.median(us))


def run_sens(ctx, s, dtype, n, warmup, steps):
    us = []
    for i in range(warmup + steps):
        prow, _, _ = ctx.sensitivity(s["rows"], s["M"], s["X"][dtype], s["J"], s["R"], ncol=s["ncol"], n_lead=s["n_lead"], n_targets=n)
        assert np.all(prow >= 0)
        if i >= warmup:
            us.append(ctx.get_option("sens_us"))
    return 1e-3 * float(np.median(us))


def measure(ctx, name, wl, rounds, warmup, steps):
    s = setup(ctx, wl)
    res = {"impact": []}
    for r in range(rounds):
        res["impact"].append(run_impact(ctx, s, warmup, steps))
        for dtype in ("float64", "float32"):
            t0 = run_sens(ctx, s, dtype, 1, warmup, steps)
            a = run_sens(ctx, s, dtype, T_LATE, warmup, steps)
            b = run_sens(ctx, s, dtype, T_LATE + 1, warmup, steps)
            res.setdefault(dtype + "_t0", []).append(t0)
            res.setdefault(dtype + "_t12", []).append(b - a)
            res.setdefault(dtype + "_13_passes", []).append(b)
        print("%-6s round %d: %s" % (name, r, " ".join("%s %.3f ms" % (k, v[-1]) for k, v in sorted(res.items()))), flush=True)
    out = dict(workload=name, rows=s["rows"], M=s["M"], n_lead=s["n_lead"], K=K, t_late=T_LATE, rounds=rounds, warmup=warmup, steps=steps,
               hbm_peak_tb_per_s=HBM_PEAK / 1e12)
    med = dict((k, float(np.median(v))) for k, v in res.items())
    out["ms"] = dict((k, [round(x, 4) for x in v]) for k, v in res.items())
    out["ms_median"] = med
    out["impact_tb_per_s"] = 8.0 * s["rows"] * (s["M"] + 1) / (1e-3 * med["impact"]) / 1e12
    for dtype, size in (("float64", 8), ("float32", 4)):
        for v in ("t0", "t12"):
            key = "%s_%s" % (dtype, v)
            nbytes = float(size) * s["rows"] * s["M"]
            out[key] = dict(ms=med[key], over_impact=med[key] / med["impact"], tb_per_s=nbytes / (1e-3 * med[key]) / 1e12,
                            fraction_of_hbm_peak=nbytes / (1e-3 * med[key]) / HBM_PEAK)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="cfg2")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sensitivity_cost.json"))
    a = ap.parse_args()
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    results = [measure(ctx, name, SIZES[name], a.rounds, a.warmup, a.steps) for name in a.sizes.split(",")]
    with open(a.json, "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
