"""Cost and interpolation error of the LETKF with weight interpolation (efa_letkf_cycle_interp_dev) beside the
plain LETKF (efa_letkf_cycle_dev) on the same inputs, in the same run.

One MI355X, one process, 3 warm-up + 10 timed cycles per variant, medians with min and max.  Workloads: tools/letkf_cost.py's
(64 x 64 columns x 8 leads, P = 1000 obs, 1000 km half-widths, M = 20, 40, 80) and configs[2]'s geometry (361 x 720 columns x
148 leads, P = 5000, 1000 km, M = 40; 1 + 3 cycles).  Variants: plain, and strides (2,2), (4,4), (8,8).  Per variant: wall ms per
cycle, and efa_last_timing's obs_ms (list builds + obs block) and state_ms (plain: the column launch; interpolated: the node solve
plus the interpolate-and-apply launch).  On the 64 x 64 workload also the interpolation error: max and RMS difference of the
interpolated posterior from the plain one, relative to the RMS analysis increment of the plain one (reported, not bounded).

The two launches of state_ms are separated by a kernel trace, in a run of its own with nothing else traced:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/letkf_interp_cost.py --steps 3 --warmup 0 --no-error
    python tools/letkf_interp_cost.py --merge-trace DIR --json profiles/letkf_interp_cost.json

--merge-trace reads the trace's k_letkf (weights mode) and k_letkf_interp dispatches in order, three per variant in the order this
tool runs them, and adds solve_ms, apply_ms (medians), the apply's GB/s over the state's read plus write and its fp64 TFLOP/s
(2 M (M+1) per row + 7 M (M+1) per column) to the JSON written by a timing run.

    python tools/letkf_interp_cost.py [--steps 10] [--warmup 3] [--members 20,40,80] [--no-big] [--no-error] [--json profiles/letkf_interp_cost.json]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from letkf_cost import setup  # noqa: E402  (the workloads of DESIGN.md 7y, as that tool builds them)

STRIDES = [None, (2, 2), (4, 4), (8, 8)]


def label(stride):
    return "plain" if stride is None else "stride_%dx%d" % stride


def one_cycle(ctx, s, stride):
    Yp = ctx.to_device(s["HX"])
    ym = ctx.empty((s["P"],))
    ctx.form_perts(s["P"], s["M"], Yp, ym, Yp)
    ctx.synchronize()
    kw = {} if stride is None else dict(shape=s["glat"].shape, stride=stride)
    t0 = time.perf_counter()
    ctx.letkf_cycle(s["rows"], s["M"], s["P"], s["X"], s["X"], ym, Yp, s["value"], s["error"], s["assim"], s["ob_lat"], s["ob_lon"],
                    s["ob_hw"], s["glat"], s["glon"], s["n_lead"], **kw)
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.last_timing()
    return wall, t["obs_ms"], t["state_ms"]


def measure(ctx, s, stride, warmup, steps):
    for _ in range(warmup):
        one_cycle(ctx, s, stride)
    runs = np.array([one_cycle(ctx, s, stride) for _ in range(steps)])
    out = {}
    for i, key in enumerate(("wall_ms", "obs_ms", "state_ms")):
        out[key] = float(np.median(runs[:, i]))
        out[key + "_min"] = float(runs[:, i].min())
        out[key + "_max"] = float(runs[:, i].max())
    return out


def posterior(ctx, s, stride, seed=1):
    """One cycle from the seeded prior; the posterior members on the host."""
    ctx.fill_synthetic(s["rows"], 0, s["M"], seed, 3.0, s["X"])
    one_cycle(ctx, s, stride)
    return s["X"].download()


def counts(s):
    """Bytes the apply must move (the state, read and written) and its fp64 operations, from the shapes."""
    M = s["M"]
    return dict(state_bytes=2 * s["rows"] * M * 8, apply_flops=s["rows"] * 2 * M * (M + 1) + s["ncol"] * 7 * M * (M + 1))


def run(a):
    from efa_xray_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_option("timing", 1)
    out = []
    work = [dict(name="64x64x8", ny=64, nx=64, n_lead=8, M=int(m), P=1000, warmup=a.warmup, steps=a.steps, box={})
            for m in a.members.split(",")]
    if not a.no_big:
        work.append(dict(name="configs[2] geometry", ny=361, nx=720, n_lead=148, M=40, P=5000, warmup=min(a.warmup, 1), steps=min(a.steps, 3),
                         box=dict(lat=(-90.0, 90.0), lon=(0.0, 359.5))))
    for w in work:
        s = setup(ctx, w["ny"], w["nx"], w["n_lead"], w["M"], w["P"], 1000.0, **w["box"])
        rec = dict(workload=w["name"], M=w["M"], P=w["P"], halfwidth_km=1000.0, ncol=s["ncol"], n_lead=w["n_lead"], warmup=w["warmup"],
                   steps=w["steps"], variants={}, **counts(s))
        for stride in STRIDES:
            ctx.fill_synthetic(s["rows"], 0, w["M"], 1, 3.0, s["X"])      # (the cycles run in place: the same prior for every variant)
            rec["variants"][label(stride)] = measure(ctx, s, stride, w["warmup"], w["steps"])
            print(json.dumps(dict(workload=w["name"], M=w["M"], variant=label(stride), **rec["variants"][label(stride)])), flush=True)
        if w["name"] == "64x64x8" and not a.no_error:
            ctx.fill_synthetic(s["rows"], 0, w["M"], 1, 3.0, s["X"])
            prior = s["X"].download()
            plain = posterior(ctx, s, None)
            inc = float(np.sqrt(np.mean((plain - prior) ** 2)))
            rec["rms_increment"] = inc
            for stride in STRIDES[1:]:
                d = posterior(ctx, s, stride) - plain
                rec["variants"][label(stride)].update(err_max_over_rms_increment=float(np.abs(d).max() / inc),
                                                      err_rms_over_rms_increment=float(np.sqrt(np.mean(d * d)) / inc))
            print(json.dumps(dict(workload=w["name"], M=w["M"], rms_increment=inc,
                                  errors={k: (v.get("err_max_over_rms_increment"), v.get("err_rms_over_rms_increment"))
                                          for k, v in rec["variants"].items() if k != "plain"})), flush=True)
        out.append(rec)
        del s
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


def merge_trace(a):
    """Kernel times from a trace of `--steps 3 --warmup 0 --no-error [--no-big]` (the same --members) into the timing run's JSON."""
    paths = glob.glob(os.path.join(a.merge_trace, "**", "*kernel_trace.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_trace.csv under %s, found %d" % (a.merge_trace, len(paths)))
    solve, apply_, plain = [], [], []
    with open(paths[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name, ms = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        if "k_letkf_interp" in name:
            apply_.append(ms)
        elif "k_letkf<2" in name or "k_letkfILi2E" in name:
            solve.append(ms)
        elif "k_letkf<0" in name or "k_letkfILi0E" in name:
            plain.append(ms)
    with open(a.json) as f:
        out = json.load(f)
    if len(apply_) != 9 * len(out) or len(solve) != 9 * len(out) or len(plain) != 3 * len(out):
        raise SystemExit("the trace has %d / %d / %d dispatches of the apply / node solve / plain kernel: not 3 cycles per variant of %d "
                         "workloads" % (len(apply_), len(solve), len(plain), len(out)))
    for i, rec in enumerate(out):
        rec["variants"]["plain"]["kernel_ms"] = float(np.median(plain[3 * i:3 * i + 3]))
        for j, stride in enumerate(STRIDES[1:]):
            lo = 9 * i + 3 * j
            v = rec["variants"][label(stride)]
            v["solve_ms"] = float(np.median(solve[lo:lo + 3]))
            v["apply_ms"] = float(np.median(apply_[lo:lo + 3]))
            v["apply_ms_min"], v["apply_ms_max"] = float(min(apply_[lo:lo + 3])), float(max(apply_[lo:lo + 3]))
            v["apply_GBps"] = rec["state_bytes"] / (v["apply_ms"] * 1e-3) / 1e9
            v["apply_fp64_TFLOPs"] = rec["apply_flops"] / (v["apply_ms"] * 1e-3) / 1e12
            print(json.dumps(dict(workload=rec["workload"], M=rec["M"], variant=label(stride), solve_ms=v["solve_ms"], apply_ms=v["apply_ms"],
                                  apply_GBps=v["apply_GBps"], apply_fp64_TFLOPs=v["apply_fp64_TFLOPs"])), flush=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", default="20,40,80")
    ap.add_argument("--no-big", action="store_true")
    ap.add_argument("--no-error", action="store_true", help="skip the interpolation-error cycles (a traced run)")
    ap.add_argument("--merge-trace", default=None, help="directory of a rocprofv3 kernel trace of this tool to merge into --json")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.merge_trace:
        if not a.json:
            raise SystemExit("--merge-trace needs --json, the file a timing run wrote")
        merge_trace(a)
    else:
        run(a)


if __name__ == "__main__":
    main()
