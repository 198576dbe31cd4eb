"""Cost of the LETKF's cross validation over member groups (efa_ctx_set_letkf_cross_validation) on device-resident cycles.

Workload, protocol and record layout are tools/letkf_cap_cost.py's: 64 x 64 columns x 8 leads, P = 1000 obs with 1000 km half-widths,
M = 20, 40, 80; a measurement is one process on one MI355X, per M and variant 3 warm-up + 10 timed cycles, medians and min-max of the
wall time per cycle and of efa_last_timing's split.  Variants: `off` (the setting off, efa_letkf_cycle_dev), `cv2`, `cv4`, `cv8`
(K = 2, 4, 8 groups, member m in group m % K), and each of the four with `_s4` (weight_stride 4, efa_letkf_cycle_interp_dev).

    python tools/letkf_cv_cost.py [--rounds 3] [--parent-root DIR] [--json profiles/letkf_cv_cost.json]

alternates `--rounds` measurements of the parent tree (`off` and `off_s4` only: it has no cross validation), parent first, with
measurements of this tree, each a child process under its own `timeout`, and stops at the first child that fails.  The summary
compares, per M, this tree's `off` medians with the parent's own min-max range over its timed cycles, and every other variant with
the `off` of its stride.

    python tools/letkf_cv_cost.py --worker [--root DIR] [--variants cv4]    one measurement of the tree at DIR, JSON lines
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from letkf_cap_cost import setup  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = "off,cv2,cv4,cv8,off_s4,cv2_s4,cv4_s4,cv8_s4"


def parse(variant):
    """(K or 0, stride or None) of a variant's name."""
    head, _, tail = variant.partition("_s")
    return (0 if head == "off" else int(head[2:])), (int(tail) if tail else None)


def one_cycle(ctx, s, variant, col_stats=None, cv_stats=None):
    K, stride = parse(variant)
    Yp = ctx.to_device(s["HX"])
    ym = ctx.empty((s["P"],))
    ctx.form_perts(s["P"], s["M"], Yp, ym, Yp)
    ctx.synchronize()
    mesh = {} if stride is None else dict(shape=s["glat"].shape, stride=(stride, stride))
    if K:
        ctx.set_letkf_cross_validation(np.arange(s["M"]) % K, cv_stats)
    t0 = time.perf_counter()
    try:
        ctx.letkf_cycle(s["rows"], s["M"], s["P"], s["X"], s["X"], ym, Yp, s["value"], s["error"], s["assim"], s["ob_lat"],
                        s["ob_lon"], s["ob_hw"], s["glat"], s["glon"], s["n_lead"], col_stats=col_stats, **mesh)
    finally:
        if K:
            ctx.set_letkf_cross_validation(None)
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
    have = hasattr(ctx, "set_letkf_cross_validation")
    variants = [v for v in a.variants.split(",") if have or parse(v)[0] == 0]
    for M in [int(m) for m in a.members.split(",")]:
        s = setup(ctx, 64, 64, 8, M, 1000, 1000.0)
        for variant in variants:
            K, stride = parse(variant)
            ctx.fill_synthetic(s["rows"], 0, M, 1, 3.0, s["X"])      # (the cycles run in place: the same prior for every variant)
            rec = dict(workload="64x64x8", M=M, P=1000, halfwidth_km=1000.0, variant=variant, warmup=a.warmup, steps=a.steps,
                       **measure(ctx, s, variant, a.warmup, a.steps))
            npts = s["ncol"] if stride is None else _lib.letkf_mesh_nodes(64, stride).size ** 2
            st = ctx.empty((npts, 3))                               # one more cycle for the solve points' statistics
            cvs = ctx.empty((npts, 2)) if K else None
            one_cycle(ctx, s, variant, st, cvs)
            st = st.download()
            rec.update(solve_points=int(npts), n_local_median=float(np.median(st[:, 0])), sweeps_mean=float(st[:, 2].mean()))
            if K:
                cvs = cvs.download()
                rec.update(cv_sweeps_mean=float(cvs[:, 0].mean()), cv_cond_max=float(cvs[:, 1].max()))
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
        for v in variants:
            K, stride = parse(v)
            base = "off" if stride is None else "off_s%d" % stride
            on, off, par = pick("change", v), pick("change", base), pick("parent", v)
            if not on:
                continue
            for key in ("wall_ms", "obs_ms", "state_ms"):
                med = [r[key] for r in on]
                cell = dict(medians=med, min=min(r[key + "_min"] for r in on), max=max(r[key + "_max"] for r in on))
                if K == 0 and par:
                    lo, hi = min(r[key + "_min"] for r in par), max(r[key + "_max"] for r in par)
                    cell.update(parent_medians=[r[key] for r in par], parent_min=lo, parent_max=hi,
                                inside_parent_range=all(lo <= m <= hi for m in med),
                                ratio_to_parent=float(np.median(med) / np.median([r[key] for r in par])))
                if K and off:
                    cell["ratio_to_off"] = float(np.median(med) / np.median([r[key] for r in off]))
                row[v + "_" + key] = cell
            if K:
                row[v + "_cv_sweeps_mean"] = float(np.mean([r["cv_sweeps_mean"] for r in on]))
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", default="20,40,80")
    ap.add_argument("--variants", default=VARIANTS)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one measurement (a child process) may take")
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
