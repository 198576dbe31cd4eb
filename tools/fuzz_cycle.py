"""Fuzz of SEQUENCES of cycles on one context: a long plan of tests/_sequences.py -- the generator the suite's own plans come from
(tests/test_gpu_context_sequences.py runs two short ones) -- on one context.  From one step to the next the geometry (obs positions,
radii, assimilate flags, grid, sizes, slabs) is kept or changed at random while values, error variances and the state always change,
and so do the entry point, the features (relaxation, outlier check, adaptive inflation, vertical localisation), the options and the
stream -- what the library keeps across cycles (obs-obs taper table, active lists, grid and stencil mirrors, the speculated
transform, deferred timing, the settings) must never leak from one cycle into a different one.  Every step is checked against the
model; a few steps are calls the library must refuse.
usage: python tools/fuzz_cycle.py [cycles] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import _sequences as S
import test_gpu_context_sequences as T
from efa_xray_amd import _lib

ncyc = int(sys.argv[1]) if len(sys.argv) > 1 else 300
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 17
plan = S.make_plan(seed, ncyc, big_p=False)
ctx = _lib.Context(0)
runner = T.Runner(ctx)
fails, worst, kept, it = [], 0.0, 0, 0
t0 = time.time()
try:
    for s in plan:
        c = s["case"]
        tag = ("refusal " + s["refusal"]) if s["refusal"] else {"new": "new case", "values": "same geometry"}.get(s["keep"], s["keep"])
        e, kind, ok = 0.0, 0, True
        try:
            if s["refusal"]:
                runner.refuse(s)
            else:
                got = runner.run(s)
                kind = got["kind"]
                e = T.check_against_model(s, got, S.model(s), S.describe(s))
                kept += s["keep"] == "values"
        except (AssertionError, _lib.EfaError) as err:
            ok = False
            e = float("nan")
            tag += " (%s)" % str(err).splitlines()[0][-120:]
        worst = max(worst, e) if ok else worst
        line = "cycle %3d %-15s loc=%d M=%3d P=%3d N=%4d inplace=%d kind=%d rel err %.2e" % (
            it, tag, c["loc"], c["M"], c["P"], c["N"], s["entry"] in ("cycle_in", "phases_in", "update_dev", "host"), kind, e)
        if not ok:
            fails.append(line + "  " + S.describe(s))
            line += " FAIL"
        print(line, flush=True)
        it += 1
finally:
    ctx.synchronize()
    runner.field = None
    ctx.close()
print("fuzz cycle: %d cycles (%d on the previous cycle's geometry), %d failures, worst rel err %.2e, %.0f s" % (it, kept, len(fails), worst, time.time() - t0))
for f in fails:
    print("  ", f)
sys.exit(1 if fails else 0)
