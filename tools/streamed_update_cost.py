"""Cost of `EnSRF.update()` from host memory: unstreamed against streamed.

Runs on one MI355X, the variants alternating in ONE process, round by round (3 rounds x (2 warm-up + 8 timed updates) by default):
  - unstreamed          `EnSRF(state, obs).update()`: upload everything, compute, download everything -- the yardstick;
  - streamed            `streamed=True` with a plain NumPy prior (staged through the pinned ring; the posterior is pinned);
  - streamed_pinned     `streamed=True` with a prior from `EnsembleState.pinned_copy()` (DMA both ways);
each streamed variant at every chunk size of --chunk-mb (the first one is the default of `stream_chunk_cols=None`).
Workloads:
  (a) bench.py's host_api_timing case: 512 x 512 columns x 50 members x 1 000 obs, loc=None;
  (b) a Gaspari-Cohn case of about 1.3 GB: 361 x 720 columns x 8 slabs x 80 members, 2 000 obs, 1 000 km.
Per variant: wall time per update (perf_counter around update()), H2D and D2H GB/s (state bytes over the summed copy times of
the chunks), the overlap (sum of the stage times -- copies, state phase, obs phase -- over the library call's wall time) and
`stream_peak_bytes`.  A streamed variant counts as faster when its median wall time is below the unstreamed one by more than
the round-to-round spread of the unstreamed variant in the same run.

    python tools/streamed_update_cost.py [--rounds 3] [--steps 8] [--warmup 2] [--workloads a b] [--chunk-mb 64 16]
                                         [--json profiles/streamed_update_cost.json]
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AIM_MS = 6.0   # VERDICT.md's aim for workload (a)


def workload_a():
    """bench.py host_api_timing: the same seed, grid, state and obs."""
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(77)
    ny = nx = 512
    M, P = 50, 1000
    lat, lon = np.meshgrid(np.linspace(20, 60, ny), np.linspace(200, 280, nx), indexing="ij")
    arr = rng.standard_normal((1, 1, ny, nx, 1)) + 3.0 * rng.standard_normal((1, 1, ny, nx, M))
    state = EnsembleState.from_array(arr, lat, lon)
    obs = [Observation(value=float(rng.standard_normal()), obtype="var0", time=0, error=1.0, lat=float(rng.uniform(21, 59)),
                       lon=float(rng.uniform(201, 279)), assimilate_this=True) for _ in range(P)]
    return state, obs, dict(loc=None)


def workload_b(ny=361, nx=720, nvar=4, nt=2, M=80, P=2000, radius_km=1000.0):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(78)
    lat, lon = np.meshgrid(np.linspace(-90, 90, ny), np.linspace(0, 360 - 360.0 / nx, nx), indexing="ij")
    arr = np.empty((nvar, nt, ny, nx, M))
    for v in range(nvar):
        for t in range(nt):
            arr[v, t] = rng.standard_normal((ny, nx, 1)) + 3.0 * rng.standard_normal((ny, nx, M), dtype=np.float32)
    state = EnsembleState.from_array(arr, lat, lon, validtime=np.arange(nt) * 3600.0)
    del arr
    obs = [Observation(value=float(rng.standard_normal()), obtype="var%d" % (k % nvar), time=float((k % nt) * 3600.0), error=1.0,
                       lat=float(rng.uniform(-80, 80)), lon=float(rng.uniform(1, 358)), assimilate_this=True,
                       localize_radius=radius_km) for k in range(P)]
    return state, obs, dict(loc="GC")


def run_variant(state, obs, kw, warmup, steps):
    from efa_xray_amd import EnSRF
    walls, stats, dev = [], [], []
    post = None
    gc.collect()
    for i in range(warmup + steps):
        flt = EnSRF(state, obs, verbose=False, **kw)
        t0 = time.perf_counter()
        post, _ = flt.update()
        dt = time.perf_counter() - t0
        if i >= warmup:
            walls.append(1e3 * dt)
            dev.append(dict(flt.last_timing))
            stats.append(flt.last_stream)
    assert np.isfinite(post._first().reshape(-1)[:64]).all()
    return walls, dev, stats, post


def summarise(name, rounds_data, nbytes):
    walls = [w for r in rounds_data for w in r[0]]
    per_round = [float(np.median(r[0])) for r in rounds_data]
    out = dict(wall_ms=[round(w, 3) for w in walls], wall_ms_median=float(np.median(walls)), wall_ms_min=float(min(walls)),
               wall_ms_round_medians=[round(x, 3) for x in per_round], wall_ms_round_spread=float(max(per_round) - min(per_round)),
               state_ms_median=float(np.median([d["state_ms"] for r in rounds_data for d in r[1]])),
               obs_ms_median=float(np.median([d["obs_ms"] for r in rounds_data for d in r[1]])))
    st = [s for r in rounds_data for s in r[2] if s is not None]
    dv = [d for r in rounds_data for d in r[1]]
    if st:
        h2d = np.array([s["h2d_us"] for s in st], dtype=float)
        d2h = np.array([s["d2h_us"] for s in st], dtype=float)
        wall = np.array([s["wall_us"] for s in st], dtype=float)
        stage = h2d + d2h + 1e3 * np.array([d["state_ms"] + d["obs_ms"] for d in dv])
        out.update(chunks=int(st[0]["chunks"]), stream_peak_bytes=int(st[0]["peak_bytes"]),
                   h2d_gb_s=float(np.median(nbytes / (h2d * 1e-6) / 1e9)), d2h_gb_s=float(np.median(nbytes / (d2h * 1e-6) / 1e9)),
                   h2d_ms_median=float(np.median(h2d) / 1e3), d2h_ms_median=float(np.median(d2h) / 1e3),
                   library_wall_ms_median=float(np.median(wall) / 1e3), overlap_median=float(np.median(stage / wall)))
    return out


def measure(name, make, rounds, warmup, steps, chunk_mb):
    from efa_xray_amd import _lib
    state, obs, base = make()
    nvar, nt, ny, nx, M = state.shape()
    nbytes = state.nstate() * M * 8
    ctx = _lib.get_context(0)
    pinned = state.pinned_copy(ctx)
    variants = [("unstreamed", state, dict(base))]
    for j, mb in enumerate(chunk_mb):
        cc = None if j == 0 else _lib.default_chunk_cols(nvar * nt, M, int(mb) << 20)
        tag = "" if j == 0 else "_%dmb" % mb
        variants.append(("streamed" + tag, state, dict(base, streamed=True, stream_chunk_cols=cc)))
        variants.append(("streamed_pinned" + tag, pinned, dict(base, streamed=True, stream_chunk_cols=cc)))
    data = dict((v[0], []) for v in variants)
    ref = None
    for r in range(rounds):
        for vname, st, kw in variants:
            walls, dev, stats, post = run_variant(st, obs, kw, warmup, steps)
            data[vname].append((walls, dev, stats))
            if r == 0:       # the same bits from every variant
                vect = post.to_vect()
                if ref is None:
                    ref = vect
                else:
                    assert np.array_equal(ref, vect), "%s: %s differs from the unstreamed posterior" % (name, vname)
                del vect
            del post
            print("%s round %d %-22s wall median %.3f ms (min %.3f)" % (name, r, vname, np.median(walls), min(walls)), flush=True)
    out = dict(workload=name, shape=[nvar, nt, ny, nx, M], P=len(obs), loc=base["loc"], state_bytes=nbytes, rounds=rounds,
               warmup=warmup, steps=steps, default_chunk_cols=_lib.default_chunk_cols(nvar * nt, M), variants={})
    for vname, _, _ in variants:
        out["variants"][vname] = summarise(vname, data[vname], nbytes)
    un = out["variants"]["unstreamed"]
    out["unstreamed_round_spread_ms"] = un["wall_ms_round_spread"]
    acc = {}
    for vname in out["variants"]:
        if vname == "unstreamed":
            continue
        gap = un["wall_ms_median"] - out["variants"][vname]["wall_ms_median"]
        acc[vname] = dict(gap_ms=gap, faster_beyond_spread=bool(gap > un["wall_ms_round_spread"]))
    out["acceptance"] = acc
    return out


def host_costs(nbytes=100 << 20):
    """What the pool of page-locked blocks and the staging threads rest on, measured here: page-locking and releasing a block of
    `nbytes` through the library, and one core's copy rate into a pinned block (best of 5 each)."""
    import ctypes
    from efa_xray_amd import _lib
    ctx = _lib.get_context(0)
    alloc, free, copy = [], [], []
    src = np.ones(nbytes // 8)
    for _ in range(5):
        p = ctypes.c_void_p()
        t0 = time.perf_counter()
        _lib._check(ctx.lib, ctx.lib.efa_pinned_alloc(ctx.handle, nbytes, ctypes.byref(p)))
        t1 = time.perf_counter()
        dst = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), shape=(nbytes // 8,))
        dst[...] = src                      # first touch
        t2 = time.perf_counter()
        dst[...] = src
        t3 = time.perf_counter()
        del dst
        _lib._check(ctx.lib, ctx.lib.efa_pinned_free(ctx.handle, p))
        t4 = time.perf_counter()
        alloc.append(t1 - t0)
        copy.append(t3 - t2)
        free.append(t4 - t3)
    return dict(block_bytes=nbytes, pinned_alloc_ms=1e3 * min(alloc), pinned_free_ms=1e3 * min(free),
                one_core_copy_gb_s=nbytes / min(copy) / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", nargs="+", default=["a", "b"], choices=["a", "b"])
    ap.add_argument("--chunk-mb", nargs="+", type=int, default=[64, 16],
                    help="chunk sizes of the streamed variants; the first is reported as the default (stream_chunk_cols=None)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "streamed_update_cost.json"))
    a = ap.parse_args()
    makers = {"a": ("a: 512x512 x 50 members x 1000 obs, loc=None (bench.py host_api_timing)", workload_a),
              "b": ("b: 361x720 x 8 slabs x 80 members x 2000 obs, GC 1000 km", workload_b)}
    results = []
    hc = host_costs()
    print(json.dumps(hc), flush=True)
    for w in a.workloads:
        name, make = makers[w]
        res = measure(name, make, a.rounds, a.warmup, a.steps, a.chunk_mb)
        if w == "a":
            best = min((v["wall_ms_median"], n) for n, v in res["variants"].items() if n != "unstreamed")
            res["aim_ms"] = AIM_MS
            res["aim_met"] = bool(best[0] <= AIM_MS)
            res["aim_best_variant"] = best[1]
            res["aim_best_ms"] = best[0]
        res["host_costs"] = hc
        results.append(res)
        print(json.dumps(res), flush=True)
        gc.collect()
        from efa_xray_amd import _lib
        _lib.get_context(0).pinned_trim()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
