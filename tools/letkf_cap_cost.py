"""Cost of the LETKF's cap on the local observations of a solve (efa_ctx_set_letkf_obs_cap) on device-resident cycles.

Workload: 64 x 64 columns x 8 leads, P = 1000 obs with 1000 km half-widths, M = 20, 40, 80 (tools/letkf_cost.py's).  A measurement
is one process on one MI355X: per M and variant 3 warm-up + 10 timed cycles of efa_letkf_cycle_dev, medians and min-max of the wall
time per cycle and of efa_last_timing's split (list builds + obs block as obs_ms, the column launch as state_ms).  Variants:
`off` (the setting off), `cap50` and `cap200` (one class, at most 50 / 200 obs per local analysis; every column of the workload
reaches more).

    python tools/letkf_cap_cost.py [--rounds 3] [--parent-root DIR] [--json profiles/letkf_cap_cost.json]

starts `--rounds` measurements of this tree, each a child process under its own `timeout`, and with --parent-root (a checkout of
the parent commit whose library is built) alternates them with measurements of that tree (`off` only: it has no cap), parent
first.  It stops at the first child that fails.  The summary compares, per M, this tree's `off` medians with the parent's own
min-max range over its timed cycles, and the capped variants with `off`.

    python tools/letkf_cap_cost.py --worker [--root DIR] [--variants cap50]    one measurement of the tree at DIR (default: this
                                                                              one), JSON lines; under a kernel trace this is the
                                                                              program that gives k_letkf_cap's time beside k_gc_build's
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def setup(ctx, ny, nx, n_lead, M, P, hw_km, lat=(25.0, 55.0), lon=(230.0, 290.0), seed=1):
    rng = np.random.default_rng(7000 + seed + M)
    glat, glon = np.meshgrid(np.linspace(lat[0], lat[1], ny), np.linspace(lon[0], lon[1], nx), indexing="ij")
    rows = ny * nx * n_lead
    X = ctx.empty((rows, M))
    ctx.fill_synthetic(rows, 0, M, seed, 3.0, X)
    amp = min(1.0, 20.0 * np.sqrt(M / float(P)))
    HX = amp * rng.standard_normal((P, M)) + rng.standard_normal((P, 1))
    err = rng.uniform(0.5, 2.0, P)
    s = dict(X=X, HX=HX, rows=rows, M=M, P=P, n_lead=n_lead, ncol=ny * nx, glat=glat, glon=glon, error=err,
             value=HX.mean(axis=1) + np.sqrt(err) * rng.standard_normal(P), assim=rng.random(P) >= 0.1,
             ob_lat=rng.uniform(lat[0] - 5, lat[1] + 5, P), ob_lon=rng.uniform(lon[0] - 5, lon[1] + 5, P), ob_hw=np.full(P, float(hw_km)))
    return s


def one_cycle(ctx, s, variant, col_stats=None):
    Yp = ctx.to_device(s["HX"])
    ym = ctx.empty((s["P"],))
    ctx.form_perts(s["P"], s["M"], Yp, ym, Yp)
    ctx.synchronize()
    if variant != "off":
        ctx.set_letkf_obs_cap(None, (int(variant[3:]),), s["reach"], P=s["P"])
    t0 = time.perf_counter()
    try:
        ctx.letkf_cycle(s["rows"], s["M"], s["P"], s["X"], s["X"], ym, Yp, s["value"], s["error"], s["assim"], s["ob_lat"],
                        s["ob_lon"], s["ob_hw"], s["glat"], s["glon"], s["n_lead"], col_stats=col_stats)
    finally:
        if variant != "off":
            ctx.set_letkf_obs_cap(None, None)
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.last_timing()
    return wall, t["obs_ms"], t["state_ms"]


def measure(ctx, s, variant, warmup, steps):
    for _ in range(warmup):
        one_cycle(ctx, s, variant)
    runs = np.array([one_cycle(ctx, s, variant) for _ in range(steps)])
    out = {}
    for i, key in enumerate(("wall_ms", "obs_ms", "state_ms")):
        out[key] = float(np.median(runs[:, i]))
        out[key + "_min"] = float(runs[:, i].min())
        out[key + "_max"] = float(runs[:, i].max())
    return out


def worker(a):
    root = os.path.abspath(a.root or ROOT)
    sys.path.insert(0, root)
    from efa_xray_amd import _lib
    assert os.path.abspath(_lib.__file__).startswith(root), "the package was imported from %s" % _lib.__file__
    ctx = _lib.Context(0)
    ctx.set_option("timing", 1)
    variants = tuple(a.variants.split(",")) if hasattr(ctx, "set_letkf_obs_cap") else ("off",)
    for M in [int(m) for m in a.members.split(",")]:
        s = setup(ctx, 64, 64, 8, M, 1000, 1000.0)
        s["reach"] = ctx.empty((s["ncol"],))
        for variant in variants:
            ctx.fill_synthetic(s["rows"], 0, M, 1, 3.0, s["X"])      # (the cycles run in place: the same prior for both variants)
            rec = dict(workload="64x64x8", M=M, P=1000, halfwidth_km=1000.0, variant=variant, warmup=a.warmup, steps=a.steps,
                       **measure(ctx, s, variant, a.warmup, a.steps))
            st = ctx.empty((s["ncol"], 3))                          # one more cycle for the columns' statistics
            one_cycle(ctx, s, variant, st)
            st = st.download()
            rec.update(n_local_median=float(np.median(st[:, 0])), dfs_median=float(np.median(st[:, 1])), sweeps_mean=float(st[:, 2].mean()))
            if variant != "off":
                reach = s["reach"].download()
                rec.update(reach_min=float(reach.min()), reach_median=float(np.median(reach)), reach_max=float(reach.max()))
            print(json.dumps(rec), flush=True)
        del s
    ctx.close()


def child(root, a, label):
    """One measurement in a process of its own, under its own time limit; its records, or None when it failed."""
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--root", root,
           "--members", a.members, "--variants", a.variants, "--steps", str(a.steps), "--warmup", str(a.warmup)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, cwd=root)
    if p.returncode != 0:
        print("%s: exit status %d -- nothing more is started" % (label, p.returncode), flush=True)
        return None
    recs = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    for r in recs:
        r["build"] = label
        print(json.dumps(r), flush=True)
    return recs


def summary(records, members, variants):
    out = []
    for M in members:
        def pick(build, variant):
            return [r for r in records if r["build"] == build and r["variant"] == variant and r["M"] == M]

        row = dict(M=M)
        par, off = pick("parent", "off"), pick("change", "off")
        for key in ("wall_ms", "obs_ms", "state_ms"):
            if par:
                lo, hi = min(r[key + "_min"] for r in par), max(r[key + "_max"] for r in par)
                row["parent_" + key] = dict(medians=[r[key] for r in par], min=lo, max=hi)
            if off:
                med = [r[key] for r in off]
                row["off_" + key] = dict(medians=med, min=min(r[key + "_min"] for r in off), max=max(r[key + "_max"] for r in off))
                if par:
                    row["off_" + key].update(inside_parent_range=all(lo <= m <= hi for m in med),
                                             ratio_to_parent=float(np.median(med) / np.median([r[key] for r in par])))
            for v in variants:
                on = pick("change", v)
                if not on or v == "off":
                    continue
                med = [r[key] for r in on]
                row[v + "_" + key] = dict(medians=med, min=min(r[key + "_min"] for r in on), max=max(r[key + "_max"] for r in on))
                if off:
                    row[v + "_" + key]["overhead_vs_off"] = float(np.median(med) / np.median([r[key] for r in off]) - 1.0)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", default="20,40,80")
    ap.add_argument("--variants", default="off,cap50,cap200")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one measurement (a child process) may take")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.worker:
        worker(a)
        return 0
    records, ok = [], True
    for _ in range(a.rounds):
        for label, root in (("parent", a.parent_root), ("change", ROOT)):
            if root is None:
                continue
            recs = child(os.path.abspath(root), a, label)
            if recs is None:
                ok = False
                break
            records += recs
        if not ok:
            break
    members = [int(m) for m in a.members.split(",")]
    out = dict(workload="64x64 columns x 8 leads, P=1000, 1000 km", rounds=a.rounds, warmup=a.warmup, steps=a.steps, complete=ok,
               summary=summary(records, members, a.variants.split(",")), records=records)
    print(json.dumps(out["summary"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
