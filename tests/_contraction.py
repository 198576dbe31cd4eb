"""The fp32 contraction: helpers of tests/test_contraction_host.py and tests/test_gpu_contraction.py.

  1. `launch`: a Python restatement of `launch_contract_f32` / `contract_ra_launch` (efa_xray_amd/csrc/efa_contract.hip), its
     constants read from the source; the shape lists below are asserted against it, so that a retune of the kernel makes the
     tests say which class went missing;
  2. `reference`, `bound`, `err_over_bound`: float64 and the project's own bound;
  3. `chain`: the f32 FMA chain in the kernel's documented member order, over the whole N x P array;
  4. `exponents`, `scale_pow2`, `assert_scaling_exact`: exact powers of two on the rows of X and of Ye.
Nothing here needs a GPU."""
import functools
import os
import re

import numpy as np

from conftest import ROOT

F32, F64 = np.float32, np.float64
RTOL, ATOL_SCALE = 1e-4, 2e-6            # |C - ref| <= 1e-4 |ref| + 2e-6 sum|a b|  
CHAIN_RTOL, CHAIN_ATOL = 2e-6, 1e-6      # the existing chain tolerance of tests/test_gpu_parity.py

_SRC = open(os.path.join(ROOT, "efa_xray_amd", "csrc", "efa_contract.hip")).read()


def _const(pattern):
    m = re.search(pattern, _SRC)
    assert m, "efa_contract.hip no longer has %r: restate the launch mirror" % pattern
    return tuple(int(g) for g in m.groups()) if len(m.groups()) > 1 else int(m.group(1))


kBM, kBN, kBK = _const(r"constexpr int kBM = (\d+), kBN = (\d+), kBK = (\d+);")
kRaObs = _const(r"constexpr int kRaObs = (\d+);")
kRaThreads = _const(r"constexpr int kRaThreads = (\d+);")
assert re.search(r"constexpr int kRaRows = 32 \* \(kRaThreads / 64\);", _SRC)
kRaRows = 32 * (kRaThreads // 64)
# while (nrb * split < 4096 && split * 2 <= tiles && split < 16) split *= 2;
SPLIT_BLOCKS, SPLIT_MAX = _const(r"while \(nrb \* split < (\d+) && split \* 2 <= tiles && split < (\d+)\) split \*= 2;")
# grid.y of the general kernel: nrb < 65535 ? nrb : 65535
GRID_Y_CAP = _const(r"nrb < (\d+) \? nrb : \1\b")
RA_MAX_M = _const(r"if \(M <= (\d+) && N <=")
assert re.search(r"switch \(\(M \+ 15\) / 16\)", _SRC) and re.search(r"const long per = \(tiles \+ col_split - 1\) / col_split;", _SRC)
KH_ALL = tuple(int(k) for k in re.findall(r"case \d+: return contract_ra_launch<(\d+)>", _SRC)) + \
    (_const(r"default: return contract_ra_launch<(\d+)>"),)


def _cdiv(a, b):
    return -(-a // b)


def launch(N, M, P):
    """What `efa_cov_contract_f32_dev` launches for (N, M, P), or None for an empty call.  kernel "ra": `KH`, `split`, `tiles` (of
    kRaObs obs), `per`, `idle` (workgroups of one row block that get no tile), `one_tile` (those that get exactly one, and never
    prefetch), `nrb`; kernel "general": `tiles` (of kBN obs), `grid_y`, `trips` of the blockIdx.y loop, `kchunks`, `partial_k`."""
    assert N >= 0 and P >= 0 and M >= 4 and M % 4 == 0
    if N == 0 or P == 0:
        return None
    if M <= RA_MAX_M and N <= kRaRows * 2147483647 and P < 1 << 28:
        KH = 8 * _cdiv(M, 16)
        assert KH in KH_ALL
        nrb, tiles = _cdiv(N, kRaRows), _cdiv(P, kRaObs)
        split = 1
        while nrb * split < SPLIT_BLOCKS and split * 2 <= tiles and split < SPLIT_MAX:
            split *= 2
        per = _cdiv(tiles, split)
        got = [max(0, min(y * per + per, tiles) - y * per) for y in range(split)]
        assert sum(got) == tiles
        return dict(kernel="ra", KH=KH, nrb=nrb, split=split, tiles=tiles, per=per, idle=sum(1 for g in got if g == 0),
                    one_tile=sum(1 for g in got if g == 1), trips=1)
    nrb = _cdiv(N, kBM)
    grid_y = min(nrb, GRID_Y_CAP)
    return dict(kernel="general", KH=None, nrb=nrb, tiles=_cdiv(P, kBN), grid_y=grid_y, trips=_cdiv(nrb, grid_y),
                kchunks=_cdiv(M, kBK), partial_k=M % kBK != 0, split=1, per=None, idle=0)


def member_order(M):
    """The documented order of the sum: up to RA_MAX_M members step s adds members s and KH + s (the zero padding left out),
    larger ensembles run in k order."""
    if M <= RA_MAX_M:
        KH = 8 * _cdiv(M, 16)
        order = [k for s in range(KH) for k in (s, KH + s) if k < M]
    else:
        order = list(range(M))
    assert sorted(order) == list(range(M))
    return order


# ---------------------------------------------------------------------------
# shapes (N, M, P): the smallest that reach each class; tests/test_contraction_host.py proves the classes by `launch`
# ---------------------------------------------------------------------------
RA_M = (4, 12, 16, 20, 32, 36, 48, 52, 64, 68, 80, 84, 96, 100, 112, 116, 128)       # both ends of every KH
RA_N = (1, 31, 33, 255, 257, 513, 63, 65, 127, 129)
RA_P = (1, 63, 65, 127, 129, 257, 600, 2049, 31, 33, 255, 1100)                    # 1100: 9 tiles, split 8
GEN_M = (132, 160, 252, 256, 260, 512, 1000)
GEN_NP = (127, 128, 129, 300)


def _pairwise():
    """Every M with a walk through the N and P lists (each N and each P at least once per kernel, no full product)."""
    ra = [(RA_N[(3 * i) % len(RA_N)], M, RA_P[(5 * i) % len(RA_P)]) for i, M in enumerate(RA_M)]
    # the values the walk has not met, on the instantiations of the issue's first paragraph, and the named edges: the
    # interior | masked store paths meet at row0 + 32 <= N and colh + 64 <= P
    ra += [(513, 68, 600), (257, 20, 2049), (255, 52, 1100), (33, 84, 255), (129, 32, 33), (63, 96, 31), (65, 40, 129),
           (127, 128, 63), (31, 64, 65), (1, 100, 1), (256, 48, 128), (32, 116, 64), (288, 80, 192)]
    gen = [(GEN_NP[i % 4], M, GEN_NP[(i + 1 + i // 4) % 4]) for i, M in enumerate(GEN_M)]
    gen += [(300, 132, 300), (129, 260, 128), (128, 1000, 129), (127, 512, 127)]
    return ra, gen


RA_SHAPES, GEN_SHAPES = _pairwise()
SHAPES = RA_SHAPES + GEN_SHAPES
# the smallest N whose row blocks (full ones and a partial one) need a second trip of the blockIdx.y loop of k_contract_f32
BIG_SHAPE = (kBM * GRID_Y_CAP + kBM + 1, 132, 3)
# one shape per kernel and KH class with partial tiles in both directions, for the exact relations
EXACT_M = (20, 100, 128, 132, 260)
EXACT_N, EXACT_P = 300, 300
POISON_KINDS = ("nan", "inf", "zero")
POISON_ROWS = (0, 31, 32, 255, 290, 299)      # first; 31 | 32; the last row of a full block (ra: 256 rows); two of the partial last block
POISON_ROWS_GEN = (0, 31, 32, 127, 290, 299)  # ... the general kernel's blocks are kBM rows
POISON_OBS = (63, 64, 127, 128, 256, 299)     # the tile edges 63 | 64 and 127 | 128, two obs of the partial last tile


@functools.lru_cache(maxsize=None)
def problem(N, M, P):
    """Unit-normal float32 operands (read-only) of one shape."""
    rng = np.random.default_rng(9000 + 7 * N + 13 * M + P)
    X = rng.standard_normal((N, M)).astype(F32)
    Ye = rng.standard_normal((P, M)).astype(F32)
    X.setflags(write=False)
    Ye.setflags(write=False)
    return X, Ye


# ---------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------
def reference(X, Ye):
    """(ref, scale) = (X64 . Ye64^T, |X64| . |Ye64|^T)."""
    X64, Y64 = np.asarray(X, dtype=F64), np.asarray(Ye, dtype=F64)
    return X64 @ Y64.T, np.abs(X64) @ np.abs(Y64).T


def bound(ref, scale):
    return RTOL * np.abs(ref) + ATOL_SCALE * scale


def err_over_bound(C, ref, scale):
    """|C - ref| / bound per element (0 where both vanish)."""
    err = np.abs(np.asarray(C, dtype=F64) - ref)
    b = bound(ref, scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(err == 0, 0.0, err / b)


def assert_within_bound(C, ref, scale, what, fraction=1.0):
    """Every element within `fraction` of the bound; returns the worst err/bound."""
    C = np.asarray(C)
    assert C.shape == ref.shape, (what, C.shape, ref.shape)
    assert np.isfinite(C).all(), "%s: %d values are not finite" % (what, int((~np.isfinite(C)).sum()))
    q = err_over_bound(C, ref, scale)
    bad = ~(q <= fraction)
    assert not bad.any(), "%s: %d of %d elements are outside %.3g of the bound, worst %.3g at %r" % (
        what, int(bad.sum()), bad.size, fraction, float(np.nanmax(q)), tuple(int(v) for v in np.argwhere(bad)[0]))
    return float(q.max()) if q.size else 0.0


@functools.lru_cache(maxsize=None)
def expected(N, M, P):
    """(ref, scale, chain) of `problem(N, M, P)`, computed once and shared (read-only)."""
    X, Ye = problem(N, M, P)
    ref, scale = reference(X, Ye)
    ch = chain(X, Ye)
    for a in (ref, scale, ch):
        a.setflags(write=False)
    return ref, scale, ch


# ---------------------------------------------------------------------------
# the documented chain
# ---------------------------------------------------------------------------
def chain(X, Ye, order=None, dtype=F64):
    """acc <- f32(acc + x_m y_m) over the members in `order` (default: the documented one), for every element at once.  The
    product of two float32 values is exact in float64 and the sum is rounded to float64 and then to float32; `dtype`
    np.longdouble repeats it with a wider intermediate (tests/test_contraction_host.py: the same bits)."""
    X, Ye = np.asarray(X, dtype=F32), np.asarray(Ye, dtype=F32)
    N, M = X.shape
    order = member_order(M) if order is None else order
    Xw, Yw = X.astype(dtype), Ye.astype(dtype)
    acc = np.zeros((N, Ye.shape[0]), dtype=F32)
    for m in order:
        acc = (acc.astype(dtype) + Xw[:, m, None] * Yw[None, :, m]).astype(F32)
    return acc


def ulps(a, b):
    """Distance of two float32 arrays in units of the last place of the larger magnitude (both finite)."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    big = np.maximum(np.abs(a), np.abs(b)).astype(F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(big > 0, np.abs(a.astype(F64) - b.astype(F64)) / np.spacing(big.astype(F32)).astype(F64), 0.0)
    return u


def assert_chain_close(C, ch, what):
    bad = ~(np.abs(np.asarray(C, dtype=F64) - ch) <= CHAIN_ATOL + CHAIN_RTOL * np.abs(ch.astype(F64)))
    assert not bad.any(), "%s: %d of %d elements leave the documented chain, first at %r" % (
        what, int(bad.sum()), bad.size, tuple(int(v) for v in np.argwhere(bad)[0]))


# ---------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a, dtype=F32)
    return a.view(np.uint32)


def assert_same_bits(got, want, what, keep=None):
    """Bit for bit (NaN payloads and the sign of zero included); `keep`: a boolean mask of the elements compared."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F32, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if keep is not None:
        bad &= keep
    if bad.any():
        first = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d values differ in their bits, first at %r: %r against %r" % (
            what, int(bad.sum()), bad.size, first, got[first], want[first]))


def poisoned_as(kind, values):
    """What a poisoned row of X (or ob of Ye) leaves in its row (column) of C."""
    if kind == "nan":
        return bool(np.isnan(values).all())
    if kind == "inf":
        return not np.isfinite(values).any()
    return bool((values == 0).all())


# ---------------------------------------------------------------------------
# exact powers of two
# ---------------------------------------------------------------------------
def exponents(n, seed, lo=-20, hi=20):
    """k in [lo, hi] from a seeded stream, with the neighbours hi | lo (both orders), a run of equal exponents across the
    31 | 32 edge, an exponent 0, and lo | hi on the last two."""
    k = np.random.default_rng(seed).integers(lo, hi + 1, n)
    if n >= 48:
        k[5], k[6], k[7] = hi, lo, hi
        k[24:40] = 11
        k[40] = 0
        k[n - 2], k[n - 1] = lo, hi
    return k.astype(np.int64)


def scale_pow2(A, k):
    """diag(2^k) A in float32, exactly: every scaled value is normal and scales back to the bits of A."""
    A = np.asarray(A, dtype=F32)
    kk = np.asarray(k).reshape(-1, 1)
    out = np.ldexp(A, kk).astype(F32)
    nz = A != 0
    info = np.finfo(F32)
    mag = np.abs(out[nz].astype(F64))
    assert mag.min() >= info.tiny and mag.max() <= info.max, "a scaled input left the normal range of float32"
    assert np.array_equal(np.ldexp(out, -kk), A), "the scaling is not exact"
    return out


def assert_scaling_exact(X, Ye, kx, ky):
    """The condition under which C(D1 X, D2 Ye) == D1 C(X, Ye) D2 must hold bit for bit, for the plain and the scaled
    operands alike: every non-zero product x_m y_m and every sum|x y| is normal in float32, and so is what a complete
    cancellation can leave: an accumulator of 24 bits against an exact product of 48 leaves at least 2^-47 of the product
    (or exactly 0), so `min product * 2^-47 >= tiny` keeps every partial sum out of the subnormal range."""
    tiny, big = float(np.finfo(F32).tiny), float(np.finfo(F32).max)
    for A, B in ((np.asarray(X, dtype=F64), np.asarray(Ye, dtype=F64)),
                 (scale_pow2(X, kx).astype(F64), scale_pow2(Ye, ky).astype(F64))):
        lo, hi = np.inf, 0.0
        for m in range(A.shape[1]):
            p = np.abs(A[:, m, None] * B[None, :, m])
            hi = max(hi, float(p.max()))
            nz = p[p > 0]
            if nz.size:
                lo = min(lo, float(nz.min()))
        scale = np.abs(A) @ np.abs(B).T
        assert lo >= tiny and hi <= big, "a product left the normal range of float32 (%.3g .. %.3g)" % (lo, hi)
        assert lo * 2.0 ** -47 >= tiny, "a cancelled partial sum could be subnormal (smallest product %.3g)" % lo
        assert scale.min() >= tiny and scale.max() <= big, "a sum |x y| left the normal range of float32"


def scaled_result(C, kx, ky):
    """D1 C D2, exactly."""
    out = np.ldexp(np.asarray(C, dtype=F32), np.asarray(kx).reshape(-1, 1) + np.asarray(ky).reshape(1, -1)).astype(F32)
    fin = np.isfinite(out) & (out != 0)
    assert np.abs(out[fin].astype(F64)).min() >= np.finfo(F32).tiny
    return out
