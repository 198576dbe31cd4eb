"""Cost of float32 state storage against float64, in the protocol of tools/streamed_update_cost.py: the variants
alternate in ONE process, round by round (3 rounds x (2 warm-up + 8 timed) by default); medians and round medians are kept.

Workloads:
  (a) 512 x 512 columns x 50 members x 1 000 obs, loc=None: `streamed_pinned` and `streamed_pinned_16mb`, float64 against float32;
  (b) 361 x 720 columns x 8 slabs x 80 members x 2 000 obs, Gaspari-Cohn 1 000 km: the same;
  (c) a resident state of --rows-c rows x 100 members, 10 000 obs, loc=None: state_ms of efa_state_cycle_dev against
      efa_state_cycle_f32_dev (out of place) and the transform's achieved GB/s (bytes read + written over state_ms).
Per streamed variant: wall time of update(), the library call (stream_wall_us), H2D / D2H GB/s (state bytes as stored over the
summed copy times of the chunks) and the device bytes held for state chunks (stream_peak_bytes).

The float64 BASELINE comes from a build of the parent commit run by this same tool: `--lib PATH` loads that library instead of
the product (only the float64 variants run when it lacks the float32 symbols) and `--json` keeps its figures; the product's run
takes them with `--baseline FILE`.  The gate, at (a) and (b): the float32 library-call median is below the baseline's float64
median by more than the baseline's own round-to-round spread (the rule of DESIGN.md 7f).  (c) is recorded only.

    python tools/f32_state_cost.py --lib parent/libefa_hip.so --json parent_f64.json
    python tools/f32_state_cost.py --baseline parent_f64.json [--json profiles/f32_state_cost.json]
"""
import argparse
import ctypes
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

F32_SYMBOLS = ("efa_state_cycle_f32_dev", "efa_ensrf_cycle_host_f32")


def load(lib_path):
    """The package on `lib_path` (None: the product).  True when the library has the float32 entry points."""
    from efa_xray_amd import _lib
    if lib_path is None:
        _lib.load_library()
        return True
    if "torch" not in sys.modules:   # as _lib.load_library: torch's copy of the HIP runtime first, so that both builds run on the same one
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    probe = ctypes.CDLL(os.path.abspath(lib_path))
    has = all(hasattr(probe, n) for n in F32_SYMBOLS)
    if not has:      # a parent build: bind what it exports
        for n in F32_SYMBOLS:
            _lib.SIGNATURES.pop(n, None)
    os.environ["EFA_HIP_LIB"] = os.path.abspath(lib_path)
    _lib.load_library()
    return has


def run_streamed(state, obs, kw, warmup, steps):
    from efa_xray_amd import EnSRF
    walls, stats = [], []
    post = None
    gc.collect()
    for i in range(warmup + steps):
        flt = EnSRF(state, obs, verbose=False, **kw)
        t0 = time.perf_counter()
        post, _ = flt.update()
        dt = time.perf_counter() - t0
        if i >= warmup:
            walls.append(1e3 * dt)
            stats.append(dict(flt.last_stream, state_ms=flt.last_timing["state_ms"], obs_ms=flt.last_timing["obs_ms"]))
    assert np.isfinite(post._first().reshape(-1)[:64]).all()
    return walls, stats, post


def summarise(rounds_data, nbytes):
    walls = [w for r in rounds_data for w in r[0]]
    st = [s for r in rounds_data for s in r[1]]
    lib_rounds = [float(np.median([s["wall_us"] for s in r[1]]) / 1e3) for r in rounds_data]
    h2d = np.array([s["h2d_us"] for s in st], dtype=float)
    d2h = np.array([s["d2h_us"] for s in st], dtype=float)
    return dict(wall_ms_median=float(np.median(walls)), wall_ms_min=float(min(walls)),
                wall_ms_round_medians=[round(float(np.median(r[0])), 3) for r in rounds_data],
                library_wall_ms_median=float(np.median([s["wall_us"] for s in st]) / 1e3),
                library_wall_ms_round_medians=[round(x, 3) for x in lib_rounds],
                library_wall_ms_round_spread=float(max(lib_rounds) - min(lib_rounds)),
                h2d_gb_s=float(np.median(nbytes / (h2d * 1e-6) / 1e9)), d2h_gb_s=float(np.median(nbytes / (d2h * 1e-6) / 1e9)),
                state_ms_median=float(np.median([s["state_ms"] for s in st])), obs_ms_median=float(np.median([s["obs_ms"] for s in st])),
                state_bytes=int(nbytes), chunks=int(st[0]["chunks"]), stream_peak_bytes=int(st[0]["peak_bytes"]))


def measure_streamed(name, make, rounds, warmup, steps, with_f32):
    from efa_xray_amd import _lib
    state, obs, base = make()
    nvar, nt, ny, nx, M = state.shape()
    ctx = _lib.get_context(0)
    variants = []
    for dt in ([np.float64, np.float32] if with_f32 else [np.float64]):
        st = state if dt == np.float64 else state.astype(np.float32)
        pinned = st.pinned_copy(ctx)
        del st
        item = np.dtype(dt).itemsize
        tag = "f64" if dt == np.float64 else "f32"
        cc16 = _lib.default_chunk_cols(nvar * nt, M, 16 << 20, itemsize=item)   # 16 MB chunks of this dtype
        # (both dtypes' pinned priors and posteriors are alive at once here: the limit is raised so that every posterior is pinned)
        kw = dict(base, streamed=True, stream_pinned_limit_mb=16384)
        variants.append(("streamed_pinned_" + tag, pinned, kw, state.nstate() * M * item))
        variants.append(("streamed_pinned_16mb_" + tag, pinned, dict(kw, stream_chunk_cols=cc16), state.nstate() * M * item))
    del state
    data = dict((v[0], []) for v in variants)
    vects = {}
    for r in range(rounds):
        for vname, st, kw, _ in variants:
            walls, stats, post = run_streamed(st, obs, kw, warmup, steps)
            data[vname].append((walls, stats))
            if r == 0:
                vects[vname] = post.to_vect()[:: max(1, post.nstate() // 4096)].copy()
            del post
            print("%s round %d %-28s wall median %.3f ms, library call %.3f ms" % (
                name, r, vname, np.median(walls), np.median([s["wall_us"] for s in stats]) / 1e3), flush=True)
    out = dict(workload=name, shape=[nvar, nt, ny, nx, M], P=len(obs), loc=base["loc"], rounds=rounds, warmup=warmup, steps=steps,
               variants=dict((v[0], summarise(data[v[0]], v[3])) for v in variants))
    # (the float64 variants run on the state as generated, the float32 ones on it rounded to float32: equal posteriors are the
    # tests' business; here the chunk sizes of one dtype must agree)
    for tag in ("f64", "f32") if with_f32 else ("f64",):
        assert np.array_equal(vects["streamed_pinned_" + tag], vects["streamed_pinned_16mb_" + tag]), name + ": " + tag
    return out


def measure_resident(rows, rounds, warmup, steps, with_f32, M=100, P=10000, block=100000, checked=True):
    """(c): the state phase alone, prior and posterior resident (out of place), a block of `block` random rows repeated."""
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    rng = np.random.default_rng(79)
    block = min(block, rows)
    B32 = (rng.standard_normal((block, 1)) + 3.0 * rng.standard_normal((block, M))).astype(np.float32)
    B64 = B32.astype(np.float64)
    pick = rng.integers(0, block, P)
    HX = B64[pick]
    value = HX.mean(axis=1) + rng.standard_normal(P)
    error = np.ones(P)
    assim = np.ones(P, dtype=bool)
    ctx.set_option("timing", 1)
    ctx.set_option("path", _lib.PATH_AUTO)
    ctx.set_relaxation(_lib.RELAX_NONE, 0.0)
    ctx.set_outlier_threshold(None)
    ctx.set_vertical_localization(None)
    bufs = {}
    for tag, B in ([("f64", B64), ("f32", B32)] if with_f32 else [("f64", B64)]):
        X = ctx.empty((rows, M), B.dtype)
        for r0 in range(0, rows, block):
            X.upload_rows(r0, B[: min(block, rows - r0)])
        bufs[tag] = (X, ctx.empty((rows, M), B.dtype))
    data = dict((tag, []) for tag in bufs)
    sample = {}
    for r in range(rounds):
        for tag, (X, post) in bufs.items():
            ms = []
            for i in range(warmup + steps):
                ym = ctx.empty((P,))
                Yp = ctx.to_device(HX)
                ctx.form_perts(P, M, Yp, ym, Yp)
                ctx.obs_phase(M, P, ym, Yp, value, error, assim)
                if tag == "f64":
                    ctx.state_cycle(rows, M, X, post)
                else:
                    ctx.state_cycle_f32(rows, M, X, post)
                t = ctx.last_timing()
                assert t["path"] == _lib.PATH_TRANSFORM
                if i >= warmup:
                    ms.append(t["state_ms"])
            data[tag].append(ms)
            if r == 0:
                sample[tag] = post.download_rows(0, min(block, 4096))
            print("c round %d %s state_ms median %.3f" % (r, tag, np.median(ms)), flush=True)
    out = dict(workload="c: resident %d x %d x %d obs, loc=None, state phase out of place" % (rows, M, P), rows=rows, M=M, P=P,
               rounds=rounds, warmup=warmup, steps=steps, variants={})
    for tag, d in data.items():
        item = 8 if tag == "f64" else 4
        med = float(np.median([x for r in d for x in r]))
        rm = [float(np.median(r)) for r in d]
        out["variants"]["state_cycle_" + tag] = dict(state_ms_median=med, state_ms_round_medians=[round(x, 4) for x in rm],
                                                     state_ms_round_spread=float(max(rm) - min(rm)), bytes_moved=2 * rows * M * item,
                                                     achieved_gb_s=2 * rows * M * item / (med * 1e-3) / 1e9)
    if with_f32:
        assert not checked or np.array_equal(sample["f32"], sample["f64"].astype(np.float32))
        out["f32_native"] = int(ctx.get_option("f32_native"))
    for X, post in bufs.values():
        X.free()
        post.free()
    return out


def gate(res, base):
    """float32 library call against the BASELINE's float64 one, beyond the baseline's round-to-round spread."""
    out = {}
    bv = dict((r["workload"], r) for r in base)[res["workload"]]["variants"]
    for tag in ("streamed_pinned", "streamed_pinned_16mb"):
        b, f = bv[tag + "_f64"], res["variants"][tag + "_f32"]
        gap = b["library_wall_ms_median"] - f["library_wall_ms_median"]
        out[tag] = dict(baseline_f64_library_ms=b["library_wall_ms_median"], baseline_round_spread_ms=b["library_wall_ms_round_spread"],
                        f32_library_ms=f["library_wall_ms_median"], gap_ms=gap, met=bool(gap > b["library_wall_ms_round_spread"]))
    return out


def main():
    from streamed_update_cost import workload_a, workload_b
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--rows-c", type=int, default=10 ** 7)
    ap.add_argument("--lib", default=None, help="measure this build of libefa_hip.so (the parent commit's: the float64 baseline)")
    ap.add_argument("--unchecked", action="store_true",
                    help="(c) on a diagnostic build whose posterior is meaningless (make nostore): time it, compare nothing")
    ap.add_argument("--baseline", default=None, help="JSON written by a --lib run: its float64 figures are the gate's baseline")
    ap.add_argument("--json", default=None, help="default: profiles/f32_state_cost.json (none with --lib)")
    a = ap.parse_args()
    with_f32 = load(a.lib)
    makers = {"a": ("a: 512x512 x 50 members x 1000 obs, loc=None", workload_a),
              "b": ("b: 361x720 x 8 slabs x 80 members x 2000 obs, GC 1000 km", workload_b)}
    base = json.load(open(a.baseline))["results"] if a.baseline else None
    results = []
    for w in a.workloads:
        if w == "c":
            res = measure_resident(a.rows_c, a.rounds, a.warmup, a.steps, with_f32, checked=not a.unchecked)
            res["results_checked"] = not a.unchecked
            if base:
                res["baseline_f64"] = dict((r["workload"], r) for r in base).get(res["workload"], {}).get("variants", {}).get("state_cycle_f64")
        else:
            res = measure_streamed(makers[w][0], makers[w][1], a.rounds, a.warmup, a.steps, with_f32)
            if base and with_f32:
                res["gate"] = gate(res, base)
                res["baseline_f64"] = dict((k, v) for k, v in dict((r["workload"], r) for r in base)[res["workload"]]["variants"].items())
        results.append(res)
        print(json.dumps(res), flush=True)
        gc.collect()
        from efa_xray_amd import _lib
        _lib.get_context(0).pinned_trim()
    path = a.json or (None if a.lib else os.path.join(ROOT, "profiles", "f32_state_cost.json"))
    if path:
        with open(path, "w") as f:
            json.dump(dict(library="parent build (--lib)" if a.lib else "product", float32=with_f32, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
