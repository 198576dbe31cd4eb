"""Cost of the LETKF under vertical / slab localisation (efa_letkf_slab_cycle_dev and its interp call) beside the
plain LETKF (efa_letkf_cycle_dev / efa_letkf_cycle_interp_dev) on the same inputs, in the same run.

One MI355X, one process, 3 warm-up + 10 timed cycles per variant, medians with min and max.
  64 x 64 columns x 8 slabs, P = 1000 obs, 1000 km half-widths, M = 20, 40, 80: ngroups = 1 (the vertical setting on, no ob with a
    vertical coordinate: every S = 1), 2 and 8 (8 / ngroups slabs per level, levels one scale height apart, half-width 1), each
    plain and with stride (4, 4); the plain LETKF on the same inputs (no setting) is the yardstick.
  configs[2]'s geometry (361 x 720 columns x 148 slabs, P = 5000, 1000 km) at M = 40 with the vertical factors of 7t's cost run
    (37 levels in ln p x 4 variables, half-width 1: 37 groups), strides (4, 4) and (8, 8), 1 + 3 cycles; the plain stride-(4, 4)
    LETKF beside it.
Per variant: wall ms per cycle, efa_last_timing's obs_ms and state_ms, the number of (point, group) solves and how many of them the
zeros of S removed (n_local = 0 where the plain run's point is reached), and state_ms per solve beside the plain run's.

The node solve and the apply of state_ms are separated by a kernel trace, in a run of its own with nothing else traced:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/letkf_slab_cost.py --steps 3 --warmup 0 --no-small
    python tools/letkf_slab_cost.py --merge-trace DIR --json profiles/letkf_slab_cost.json

--merge-trace appends the dispatches of every k_letkf* instantiation, in time order (three per variant), to the timing run's JSON.

    python tools/letkf_slab_cost.py [--steps 10] [--warmup 3] [--members 20,40,80] [--no-big] [--no-small] [--json profiles/letkf_slab_cost.json]
"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from letkf_cost import setup  # noqa: E402  (the workloads of DESIGN.md 7y, as that tool builds them)


def vertical(s, ngroups, seed=3):
    """(lead_vert, ob_vert, ob_vert_halfwidth): ngroups levels one apart, the slabs dealt to them in turn; ngroups 1: no ob has a
    coordinate, every factor is 1."""
    rng = np.random.default_rng(seed)
    P, n_lead = s["P"], s["n_lead"]
    lead = (np.arange(n_lead) % ngroups).astype(np.float64)
    if ngroups == 1:
        return lead, np.full(P, np.nan), np.ones(P)
    return lead, rng.integers(0, ngroups, P).astype(np.float64), np.ones(P)


def vertical_cfg2(s, nvar=4, nlev=37, seed=3):
    """The vertical factors of 7t's cost run: 37 levels in ln p for each of 4 variables, each ob at a level, half-width 1."""
    rng = np.random.default_rng(seed)
    lnp = np.log(np.geomspace(1000.0, 10.0, nlev))
    return np.tile(lnp, nvar), lnp[rng.integers(0, nlev, s["P"])], np.ones(s["P"])


def one_cycle(ctx, s, slab, stride, stats):
    Yp = ctx.to_device(s["HX"])
    ym = ctx.empty((s["P"],))
    ctx.form_perts(s["P"], s["M"], Yp, ym, Yp)
    ctx.synchronize()
    kw = {} if stride is None else dict(shape=s["glat"].shape, stride=stride)
    call = ctx.letkf_slab_cycle if slab else ctx.letkf_cycle
    t0 = time.perf_counter()
    call(s["rows"], s["M"], s["P"], s["X"], s["X"], ym, Yp, s["value"], s["error"], s["assim"], s["ob_lat"], s["ob_lon"], s["ob_hw"],
         s["glat"], s["glon"], s["n_lead"], col_stats=stats, **kw)
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    t = ctx.last_timing()
    return wall, t["obs_ms"], t["state_ms"]


def npoints(s, stride):
    from efa_xray_amd import _lib
    if stride is None:
        return s["ncol"]
    ny, nx = s["glat"].shape
    return _lib.letkf_mesh_nodes(ny, stride[0]).size * _lib.letkf_mesh_nodes(nx, stride[1]).size


def measure(ctx, s, vert, stride, warmup, steps):
    """vert: None for the plain LETKF, else the three arrays of the vertical setting."""
    ctx.set_vertical_localization(None)
    ng = 1
    if vert is not None:
        ctx.set_vertical_localization(*vert)
        ng = ctx.letkf_slab_groups(s["n_lead"])[1]
    npts = npoints(s, stride)
    stats = ctx.empty((ng * npts, 3))
    ctx.fill_synthetic(s["rows"], 0, s["M"], 1, 3.0, s["X"])      # (the cycles run in place: the same prior for every variant)
    try:
        for _ in range(warmup):
            one_cycle(ctx, s, vert is not None, stride, stats)
        runs = np.array([one_cycle(ctx, s, vert is not None, stride, stats) for _ in range(steps)])
    finally:
        ctx.set_vertical_localization(None)
    out = dict(ngroups=ng, points=npts, solves=ng * npts)
    for i, key in enumerate(("wall_ms", "obs_ms", "state_ms")):
        out[key] = float(np.median(runs[:, i]))
        out[key + "_min"] = float(runs[:, i].min())
        out[key + "_max"] = float(runs[:, i].max())
    nl = stats.download().reshape(ng, npts, 3)[:, :, 0]
    out["solves_run"] = int((nl > 0).sum())
    out["reached_points"] = int((nl > 0).any(axis=0).sum())
    out["state_us_per_solve_run"] = 1e3 * out["state_ms"] / max(out["solves_run"], 1)
    return out


def label(ng, stride):
    return ("plain_letkf" if ng is None else "groups_%d" % ng) + ("" if stride is None else "_stride_%dx%d" % stride)


def finish(rec):
    """The two comparisons with a yardstick, from the variants of one workload."""
    v = rec["variants"]
    for stride in (None, (4, 4)):
        base, one = v.get(label(None, stride)), v.get(label(1, stride))
        if base and one:
            spread = (base["wall_ms_max"] - base["wall_ms_min"]) / base["wall_ms"]
            one["wall_over_plain"] = one["wall_ms"] / base["wall_ms"]
            one["state_over_plain"] = one["state_ms"] / base["state_ms"]
            one["within_plain_spread_plus_1pct"] = bool(one["wall_ms"] <= base["wall_ms_max"] + 0.01 * base["wall_ms"])
            one["plain_spread"] = spread
    for key, x in v.items():
        stride = None if "stride" not in key else tuple(int(t) for t in key.split("stride_")[1].split("x"))
        base = v.get(label(None, stride))
        if base and x is not base:
            x["cost_per_solve_over_plain_per_point"] = x["state_us_per_solve_run"] / base["state_us_per_solve_run"]
            x["solves_removed_by_zeros_of_S"] = int(x["ngroups"] * base["solves_run"] - x["solves_run"])


def run(a):
    from efa_xray_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_option("timing", 1)
    out = []
    if not a.no_small:
        for M in [int(m) for m in a.members.split(",")]:
            s = setup(ctx, 64, 64, 8, M, 1000, 1000.0)
            rec = dict(workload="64x64x8", M=M, P=1000, halfwidth_km=1000.0, ncol=s["ncol"], n_lead=8, warmup=a.warmup, steps=a.steps,
                       variants={})
            for stride in (None, (4, 4)):
                for ng in (None, 1, 2, 8):
                    r = measure(ctx, s, None if ng is None else vertical(s, ng), stride, a.warmup, a.steps)
                    rec["variants"][label(ng, stride)] = r
                    print(json.dumps(dict(workload=rec["workload"], M=M, variant=label(ng, stride), **r)), flush=True)
            finish(rec)
            out.append(rec)
            del s
    if not a.no_big:
        warm, steps = min(a.warmup, 1), min(a.steps, 3)
        s = setup(ctx, 361, 720, 148, 40, 5000, 1000.0, lat=(-90.0, 90.0), lon=(0.0, 359.5))
        rec = dict(workload="configs[2] geometry", M=40, P=5000, halfwidth_km=1000.0, ncol=s["ncol"], n_lead=148, warmup=warm, steps=steps,
                   vert_halfwidth_lnp=1.0, variants={})
        for ng, stride in ((None, (4, 4)), (37, (4, 4)), (37, (8, 8))):
            r = measure(ctx, s, None if ng is None else vertical_cfg2(s), stride, warm, steps)
            r["node_pair_buffer_bytes"] = r["solves"] * 40 * 41 * 8
            rec["variants"][label(ng, stride)] = r
            print(json.dumps(dict(workload=rec["workload"], M=40, variant=label(ng, stride), **r)), flush=True)
        finish(rec)
        out.append(rec)
        del s
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


def merge_trace(a):
    """Per-kernel times of a traced run into the timing run's JSON: one record per kernel name (node solve, apply, obs factor), its
    dispatches in time order (trace one workload at a time, --no-small or --no-big, --steps 3 --warmup 0: three per variant)."""
    paths = glob.glob(os.path.join(a.merge_trace, "**", "*kernel_trace.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_trace.csv under %s, found %d" % (a.merge_trace, len(paths)))
    times = {}
    with open(paths[0]) as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"])):
            name = r["Kernel_Name"]
            if "k_letkf" in name:
                key = re.search(r"k_letkf\w*(<[^>]*>)?", name).group(0)
                times.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    with open(a.json) as f:
        out = json.load(f)
    summary = {k: dict(calls=len(v), median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), total_ms=float(sum(v)),
                       ms_in_order=[round(x, 4) for x in v]) for k, v in times.items()}   # (in the order the variants ran)
    out.append(dict(kernel_trace=summary))
    print(json.dumps(summary, indent=1))
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", default="20,40,80")
    ap.add_argument("--no-big", action="store_true")
    ap.add_argument("--no-small", action="store_true")
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
