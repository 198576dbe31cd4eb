"""efa_cov_contract_f32_dev on the MI355X: every instantiation of k_contract_f32_ra, the general kernel with and
without a partial K chunk and beyond its grid cap, the edges of the obs split, and what lies around the output.

Every call writes into an allocation with GUARD floats of SENTINEL before and after C: the guards must be intact and the sentinel
must not be left in any element of C.  Bounds: the project's own against float64 on every element, and the existing
chain tolerance (rtol 2e-6, atol 1e-6) against the documented f32 FMA chain on every element; the exact relations need neither.
Shapes and helpers: tests/_contraction.py; the classes the shapes reach are proven on the CPU by tests/test_contraction_host.py."""
import ctypes
import time

import numpy as np
import pytest

import _contraction as ct

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GUARD = 64
SENTINEL = F32(-1234.5)
SENTINEL_BITS = int(np.array([SENTINEL]).view(np.uint32)[0])

_worst = {}      # kernel -> [worst err/bound, largest chain distance in ulps, largest chain distance in 2^-24 sum|a b|]


def _ctx():
    from efa_xray_amd import _lib
    return _lib.get_context(0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for kernel in sorted(_worst):
        w = _worst[kernel]
        print("\n%s: worst err/bound %.4f, largest distance to the chain %.2f ulp = %.3f * 2^-24 sum|a b|" % (kernel, w[0], w[1], w[2]))


def _addr(a, offset_bytes=0):
    if a is None:
        return None
    return ctypes.c_void_p((a.address if hasattr(a, "address") else int(a)) + offset_bytes)


def _contract(ctx, N, M, P, x, y, rows=None, cols=None, null_c=False):
    """One raw call into a guarded allocation of rows x cols floats (default N x P): (status, C, guards intact).  x, y: device
    addresses (ctypes.c_void_p or None)."""
    rows = N if rows is None else rows
    cols = P if cols is None else cols
    n = max(rows, 0) * max(cols, 0)
    buf = ctx.to_device(np.full(2 * GUARD + n, SENTINEL, dtype=F32), F32)
    try:
        st = ctx.lib.efa_cov_contract_f32_dev(ctx.handle, N, M, P, x, y, None if null_c else _addr(buf, 4 * GUARD))
        ctx.synchronize()
        flat = buf.download()
    finally:
        buf.free()
    b = ct.bits(flat)
    guards = bool(np.all(b[:GUARD] == SENTINEL_BITS) and np.all(b[GUARD + n:] == SENTINEL_BITS))
    C = flat[GUARD:GUARD + n].reshape(max(rows, 0), max(cols, 0))
    return st, C, guards


def _written(C):
    return not bool(np.any(ct.bits(C) == SENTINEL_BITS))


def _untouched(C):
    return bool(np.all(ct.bits(C) == SENTINEL_BITS))


class _Resident(object):
    """X and Ye of one problem on the device, for many calls."""

    def __init__(self, ctx, X, Ye):
        self.ctx, self.X, self.Ye = ctx, X, Ye
        (self.N, self.M), self.P = X.shape, Ye.shape[0]
        self.dX, self.dY = ctx.to_device(X, F32), ctx.to_device(Ye, F32)

    def run(self, r0=0, r1=None, c0=0, c1=None):
        """C of rows r0..r1 of X and obs c0..c1 of Ye: the operands are passed by a pointer offset of whole rows."""
        r1 = self.N if r1 is None else r1
        c1 = self.P if c1 is None else c1
        st, C, ok = _contract(self.ctx, r1 - r0, self.M, c1 - c0, _addr(self.dX, 4 * self.M * r0), _addr(self.dY, 4 * self.M * c0))
        assert st == 0 and ok and _written(C), (st, ok)
        return C

    def free(self):
        self.dX.free()
        self.dY.free()


def _label(N, M, P):
    p = ct.launch(N, M, P)
    return "k_contract_f32_ra<%d>" % p["KH"] if p["kernel"] == "ra" else "k_contract_f32"


# ---------------------------------------------------------------------------
# 1. parity and chain at every instantiation and edge
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,P", ct.SHAPES)
def test_parity_and_chain_on_every_element(N, M, P):
    ctx = _ctx()
    X, Ye = ct.problem(N, M, P)
    ref, scale, ch = ct.expected(N, M, P)
    r = _Resident(ctx, X, Ye)
    try:
        C = r.run()
    finally:
        r.free()
    what = "%s %d x %d x %d" % (_label(N, M, P), N, M, P)
    worst = ct.err_over_bound(C, ref, scale).max()
    dist = float(ct.ulps(C, ch).max())
    rel = float((np.abs(C.astype(F64) - ch.astype(F64)) / (2.0 ** -24 * scale)).max())
    plan = ct.launch(N, M, P)
    print("%s (split %s, per %s, idle %s): worst err/bound %.4f, chain distance %.2f ulp = %.3f * 2^-24 sum|a b|" % (
        what, plan["split"], plan["per"], plan["idle"], worst, dist, rel))
    w = _worst.setdefault("k_contract_f32_ra" if plan["kernel"] == "ra" else "k_contract_f32", [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], worst), max(w[1], dist), max(w[2], rel)
    ct.assert_within_bound(C, ref, scale, what)
    ct.assert_chain_close(C, ch, what)


# ---------------------------------------------------------------------------
# 2. beyond the grid cap
# ---------------------------------------------------------------------------
def test_second_trip_of_the_row_block_loop():
    """N = 128 * 65535 + 129 rows x 132 members x 3 obs: 65537 row blocks on a grid of 65535, so row blocks 65535 and 65536 (one
    row) are the second trip of k_contract_f32's blockIdx.y loop.  4.4 GB of X filled on the device, 100 MB of C; every row of
    row blocks 0, 65534, 65535 and 65536 against float64 and the chain, the guards, and no sentinel left anywhere in C (checked
    on the device).  Measured on the MI355X: fill 0.030 s, contraction 0.004 s, the whole test 0.21 s."""
    import torch
    ctx = _ctx()
    N, M, P = ct.BIG_SHAPE
    plan = ct.launch(N, M, P)
    assert plan["kernel"] == "general" and plan["trips"] == 2 and plan["grid_y"] == ct.GRID_Y_CAP
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    gen = torch.Generator(device=dev)
    gen.manual_seed(20)
    X = torch.empty((N, M), dtype=torch.float32, device=dev).normal_(generator=gen)
    Ye = torch.empty((P, M), dtype=torch.float32, device=dev).normal_(generator=gen)
    buf = torch.full((2 * GUARD + N * P,), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    try:
        ctx.cov_contract_f32(N, M, P, X.data_ptr(), Ye.data_ptr(), buf.data_ptr() + 4 * GUARD)
        ctx.synchronize()
        t2 = time.perf_counter()
        print("fill %.3f s, contraction %.3f s" % (t1 - t0, t2 - t1))
        assert bool((buf[:GUARD] == float(SENTINEL)).all()) and bool((buf[GUARD + N * P:] == float(SENTINEL)).all())
        C = buf[GUARD:GUARD + N * P].view(N, P)
        left = int((C == float(SENTINEL)).sum())        # no NaN in this C, and |C| stays far below the sentinel's magnitude
        assert left == 0, "%d elements of C were never written" % left
        Yh = Ye.cpu().numpy()
        for rb in (0, ct.GRID_Y_CAP - 1, ct.GRID_Y_CAP, plan["nrb"] - 1):
            lo, hi = rb * ct.kBM, min(rb * ct.kBM + ct.kBM, N)
            assert hi - lo == (1 if rb == plan["nrb"] - 1 else ct.kBM)
            Xh, Ch = X[lo:hi].cpu().numpy(), C[lo:hi].cpu().numpy()
            ref, scale = ct.reference(Xh, Yh)
            what = "row block %d" % rb
            print("%s: worst err/bound %.4f" % (what, ct.assert_within_bound(Ch, ref, scale, what)))
            ct.assert_chain_close(Ch, ct.chain(Xh, Yh), what)
    finally:
        X = buf = C = None
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# 3. exact relations: no tolerance, no reference
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=ct.EXACT_M)
def exact(request):
    M = request.param
    X, Ye = ct.problem(ct.EXACT_N, M, ct.EXACT_P)
    r = _Resident(_ctx(), X, Ye)
    r.clean = r.run()
    r.clean.setflags(write=False)
    yield r
    r.free()


def test_powers_of_two_on_rows_and_obs(exact):
    """C(D1 X, D2 Ye) == D1 C(X, Ye) D2 bit for bit, D = diag(2^k), k in [-20, 20]."""
    kx, ky = ct.exponents(exact.N, 100 + exact.M), ct.exponents(exact.P, 200 + exact.M)
    ct.assert_scaling_exact(exact.X, exact.Ye, kx, ky)
    r = _Resident(exact.ctx, ct.scale_pow2(exact.X, kx), ct.scale_pow2(exact.Ye, ky))
    try:
        got = r.run()
    finally:
        r.free()
    ct.assert_same_bits(got, ct.scaled_result(exact.clean, kx, ky), "M = %d: scaled operands" % exact.M)
    assert not np.array_equal(ct.bits(got), ct.bits(exact.clean))


@pytest.mark.parametrize("r0,r1,c0,c1", [(37, 291, 0, None), (0, None, 70, 230), (37, 291, 70, 230), (256, 300, 129, 300), (1, 2, 299, 300)])
def test_a_sub_block_has_the_bits_of_the_full_call(exact, r0, r1, c0, c1):
    """Rows r0..r1 of X and obs c0..c1 of Ye by a pointer offset of whole rows (16-byte aligned since M % 4 == 0): the rows land
    in other waves and lanes, the obs in another tile, half and share of the split."""
    r1 = exact.N if r1 is None else r1
    c1 = exact.P if c1 is None else c1
    got = exact.run(r0, r1, c0, c1)
    ct.assert_same_bits(got, np.ascontiguousarray(exact.clean[r0:r1, c0:c1]), "M = %d: rows %d..%d, obs %d..%d" % (exact.M, r0, r1, c0, c1))


@pytest.mark.parametrize("kind", ct.POISON_KINDS)
def test_a_poisoned_row_or_ob_changes_nothing_else(exact, kind):
    """One row of X (then one ob of Ye) all NaN, all +Inf, all zero, one at a time: only that row (column) of C changes."""
    value = {"nan": np.nan, "inf": np.inf, "zero": 0.0}[kind]
    general = ct.launch(exact.N, exact.M, exact.P)["kernel"] == "general"
    bad = np.full((1, exact.M), value, dtype=F32)
    for i in (ct.POISON_ROWS_GEN if general else ct.POISON_ROWS):
        exact.dX.upload_rows(i, bad)
        try:
            got = exact.run()
        finally:
            exact.dX.upload_rows(i, exact.X[i:i + 1])
        keep = np.ones(got.shape, dtype=bool)
        keep[i] = False
        ct.assert_same_bits(got, exact.clean, "M = %d: row %d of X %s" % (exact.M, i, kind), keep=keep)
        assert ct.poisoned_as(kind, got[i]), (exact.M, kind, i)
    for k in ct.POISON_OBS:
        exact.dY.upload_rows(k, bad)
        try:
            got = exact.run()
        finally:
            exact.dY.upload_rows(k, exact.Ye[k:k + 1])
        keep = np.ones(got.shape, dtype=bool)
        keep[:, k] = False
        ct.assert_same_bits(got, exact.clean, "M = %d: ob %d of Ye %s" % (exact.M, k, kind), keep=keep)
        assert ct.poisoned_as(kind, got[:, k]), (exact.M, kind, k)
    ct.assert_same_bits(exact.run(), exact.clean, "M = %d: the operands were restored" % exact.M)


# ---------------------------------------------------------------------------
# 4. API
# ---------------------------------------------------------------------------
def test_refusals_leave_c_untouched():
    from efa_xray_amd import _lib
    ctx = _ctx()
    N, M, P = 70, 132, 40
    X, Ye = ct.problem(N, M, P)
    r = _Resident(ctx, X, Ye)
    try:
        x, y = _addr(r.dX), _addr(r.dY)
        cases = [dict(M=0), dict(M=2), dict(M=6), dict(M=130 + 1), dict(N=-1), dict(P=-1), dict(N=-1, P=0), dict(x=None), dict(y=None),
                 dict(null_c=True), dict(x=_addr(r.dX, 4)), dict(y=_addr(r.dY, 4))]
        for over in cases:
            a = dict(N=N, M=M, P=P, x=x, y=y, null_c=False)
            a.update(over)
            st, C, ok = _contract(ctx, a["N"], a["M"], a["P"], a["x"], a["y"], rows=N, cols=P, null_c=a["null_c"])
            assert st == _lib.EFA_ERR_INVALID, (over, st)
            assert ok and _untouched(C), over
        # the same operands are served once the argument is put right (operands offset by 16 bytes included)
        st, C, ok = _contract(ctx, N - 1, M, P, _addr(r.dX, 16), y)
        assert st == 0 and ok and _written(C)
    finally:
        r.free()


@pytest.mark.parametrize("N,P", [(0, 40), (70, 0), (0, 0)])
def test_empty_calls_write_nothing(N, P):
    ctx = _ctx()
    X, Ye = ct.problem(70, 20, 40)
    r = _Resident(ctx, X, Ye)
    try:
        st, C, ok = _contract(ctx, N, 20, P, _addr(r.dX), _addr(r.dY), rows=70, cols=40)
        assert st == 0 and ok and _untouched(C)
        st, C, ok = _contract(ctx, N, 20, P, None, None, rows=70, cols=40, null_c=True)     # nothing to read, nothing to write
        assert st == 0 and ok
    finally:
        r.free()


def test_two_calls_agree_bit_for_bit(exact):
    ct.assert_same_bits(exact.run(), exact.clean, "M = %d: second call" % exact.M)
    ct.assert_same_bits(exact.run(), exact.clean, "M = %d: third call" % exact.M)


@pytest.mark.parametrize("M", [100, 132])
def test_on_a_caller_stream_behind_a_device_side_fill(M):
    """X is NaN until a copy on the caller's stream fills it, behind work that is still running when the call is made; the
    contraction follows on that stream without a host synchronisation and gives the default-stream result."""
    import torch
    ctx = _ctx()
    N, P = ct.EXACT_N, ct.EXACT_P
    X, Ye = ct.problem(N, M, P)
    r = _Resident(ctx, X, Ye)
    try:
        want = r.run()
    finally:
        r.free()
    dev = torch.device("cuda:0")
    src = torch.from_numpy(np.array(X)).to(dev)
    Xd = torch.full_like(src, float("nan"))
    Yd = torch.from_numpy(np.array(Ye)).to(dev)
    buf = torch.full((2 * GUARD + N * P,), float(SENTINEL), dtype=torch.float32, device=dev)
    busy = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for _ in range(20):
            busy = torch.tanh(busy @ busy * 1e-3)
        Xd.copy_(src)
    ctx.set_stream(stream.cuda_stream)
    try:
        ctx.cov_contract_f32(N, M, P, Xd.data_ptr(), Yd.data_ptr(), buf.data_ptr() + 4 * GUARD)
    finally:
        ctx.use_own_stream()
    torch.cuda.synchronize()
    assert torch.isfinite(busy).all()
    flat = buf.cpu().numpy()
    b = ct.bits(flat)
    assert np.all(b[:GUARD] == SENTINEL_BITS) and np.all(b[GUARD + N * P:] == SENTINEL_BITS)
    ct.assert_same_bits(flat[GUARD:GUARD + N * P].reshape(N, P), want, "M = %d on the caller's stream" % M)


def test_a_cycle_after_a_contraction_returns_the_same_bits():
    """An unlocalised cycle, a contraction by each kernel, the same cycle again: the second cycle's posterior and diagnostics are
    bit for bit those of a context that never made the calls."""
    from efa_xray_amd import _lib
    rng = np.random.default_rng(12)
    N, M, P = 715, 20, 60
    Xs = 2.0 * rng.standard_normal((N, M)) + rng.standard_normal((N, 1))
    pick = rng.choice(N, P, replace=False)
    HX = Xs[pick] + 0.05 * rng.standard_normal((P, M))
    value, error, assim = HX.mean(axis=1) + rng.standard_normal(P), rng.uniform(0.5, 2.0, P), rng.random(P) < 0.9

    def cycle(ctx):
        Xd, post, Yp, ym = ctx.to_device(Xs), ctx.empty((N, M)), ctx.to_device(HX), ctx.empty((P,))
        ctx.form_perts(P, M, Yp, ym, Yp)
        diag = ctx.ensrf_cycle(N, M, P, Xd, post, ym, Yp, value, error, assim)
        return post.download(), diag

    results = []
    for with_call in (True, False):
        ctx = _lib.Context(0)
        try:
            first = cycle(ctx)
            if with_call:
                for Mc in (100, 132):
                    X, Ye = ct.problem(ct.EXACT_N, Mc, ct.EXACT_P)
                    ref, scale, _ = ct.expected(ct.EXACT_N, Mc, ct.EXACT_P)
                    r = _Resident(ctx, X, Ye)
                    try:
                        ct.assert_within_bound(r.run(), ref, scale, "between two cycles, M = %d" % Mc)
                    finally:
                        r.free()
            results.append((first, cycle(ctx)))
        finally:
            ctx.close()
    (a1, a2), (b1, b2) = results
    for got, want in ((a1, b1), (a2, b2)):
        assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
        for key in ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated"):
            assert np.array_equal(got[1][key], want[1][key], equal_nan=True), key
    assert np.abs(a2[0] - Xs).max() > 1e-3, "the cycle saw no update: the test is vacuous"
