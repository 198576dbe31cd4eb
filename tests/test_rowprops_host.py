"""Row independence without a GPU: the relations tests/test_gpu_rowprops.py holds the kernels to belong to the
algorithm -- the oracle obeys them bit for bit --, the mixed-magnitude generators keep the oracle's own error a hundredth of
the tolerance, the band leader is predicted to serve them, and the helpers fail when they should."""
import itertools

import numpy as np
import pytest

import _rowprops as rp
from _phase_a_guard import expected_kind
from test_gpu_parity import assert_parity
from test_gpu_state_routes import ASSIM, ROWS

RELAX = [("none", 0.0), ("rtpp", 0.5), ("rtps", 0.5)]


@pytest.mark.parametrize("M", [2, 7, 20, 138])
@pytest.mark.parametrize("gc", [False, True])
def test_oracle_scales_rows_exactly(M, gc):
    """Relation 1 on the oracle: update(D X) == D update(X) for D = diag(2^k), every relaxation; diagnostics unchanged."""
    pb = rp.RowProblem(M)
    k = rp.row_exponents(ROWS, 500 + M)
    assert {-30, 0, 30} <= set(k.tolist()) and (k[20:36] == k[20]).all()
    ps = pb.with_state(rp.scale_rows(pb.X32, k))
    rp.assert_same_bits(ps.HX, pb.HX, "obs block")
    for relax, alpha in RELAX:
        post, diag = rp.oracle_members(pb, gc, relax, alpha)
        got, gdiag = rp.oracle_members(ps, gc, relax, alpha)
        rp.assert_same_bits(got, rp.scale_rows(post, k), "M=%d gc=%r %s" % (M, gc, relax))
        rp.assert_diag_bits(gdiag, diag, "M=%d gc=%r %s" % (M, gc, relax))
        assert not np.array_equal(post, pb.X64)


@pytest.mark.parametrize("M", [2, 7, 20, 138])
@pytest.mark.parametrize("gc", [False, True])
def test_oracle_keeps_poison_in_its_row(M, gc):
    """Relation 2 on the oracle: NaN / Inf / zero / constant rows change no other row's bits and come back as they must."""
    pb = rp.RowProblem(M)
    for relax, alpha in RELAX:
        clean, diag = rp.oracle_members(pb, gc, relax, alpha)
        for kind, rows in itertools.product(rp.POISON_KINDS, rp.POISON_SETS):
            pp = pb.with_state(rp.poison(pb.X32, kind, rows))
            got, gdiag = rp.oracle_members(pp, gc, relax, alpha)
            rp.assert_poisoned(kind, got, clean, "M=%d gc=%r %s %s" % (M, gc, relax, kind), ref_rows=got[rows], poisoned=rows)
            rp.assert_diag_bits(gdiag, diag, kind)
            if kind == "inf":
                reached = pp.reached[rows] | (not gc)
                assert np.isnan(got[rows][reached]).all()     # Inf - mean(Inf)


CASES = [(s, None) for s in rp.MIXED_SHAPES] + [(s[:3], s[3]) for s in rp.MIXED_GC_SHAPES]


@pytest.mark.parametrize("shape,ncol", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_mixed_generator_condition_and_guard(shape, ncol):
    """The oracle in float64 against the oracle on np.longdouble arrays and against a member-permuted float64 run: within 1e-12
    of each row's and each ob's own scale, a hundredth of the tolerance.  The figures go into DESIGN.md 7l."""
    N, M, P = shape
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is no wider than float64 here: the condition is vacuous"
    c = rp.mixed_case(N, M, P, ncol)
    assert set(np.round(np.log10(c["s_ob"])).astype(int).tolist()) == set(range(-6, 7)), "an unobserved scale"
    assert 0 < (~c["asm"]).sum() < P // 4
    Z = c["X"] / c["s_row"][:, None]
    assert (np.abs(Z.mean(axis=1)) <= rp.OFFSET * Z.std(axis=1) * (1 + 1e-12)).all()
    xam, Xap, diag, ratio = rp.run_oracle(c, guard=True)
    tol = rp.CONDITION / rp.RTOL
    worst = {}
    for name, other in (("longdouble", rp.run_oracle(c, dtype=np.longdouble)),
                        ("permuted", rp.run_oracle(c, perm=np.random.default_rng(1).permutation(M)))):
        o_xam, o_Xap, o_diag = other
        a, b = rp.assert_augmented_close(xam, Xap, o_xam, o_Xap, "%r %s" % (shape, name), tol=tol)
        post = rp.assert_rows_close(xam[:N, None] + Xap[:N], np.asarray(o_xam[:N, None] + o_Xap[:N], dtype=np.float64),
                                    "%r %s members" % (shape, name), tol=tol)
        d = rp.assert_diag_close(diag, o_diag, "%r %s" % (shape, name), tol=tol)
        worst[name] = (a, b, post, d)
    print("%r ncol=%r: guard min ratio %.3e; err/1e-10 of (xam, Xap, members, diagnostics): %s" % (
        shape, ncol, ratio, ", ".join("%s %s" % (k, " ".join("%.2e" % v for v in w)) for k, w in worst.items())))
    if not ncol:
        assert expected_kind(ratio, M) == (4 if M <= 128 else 2), "guard min ratio %.3e: tune MODE_WEIGHT" % ratio
    else:
        assert expected_kind(ratio, M) == 4, "guard min ratio %.3e" % ratio


def test_obs_scaling_is_exact_on_the_oracle():
    """Relation 3b on the oracle: ob k times 2^j_k leaves the state rows' bits and scales the diagnostics exactly."""
    for shape, ncol in (CASES[0], CASES[-1]):
        c = rp.mixed_case(*shape, ncol=ncol)
        j = rp.ob_exponents(c["P"], 9)
        xam, Xap, diag = rp.run_oracle(c)
        s_xam, s_Xap, s_diag = rp.run_oracle(rp.scale_obs(c, j))
        N = c["N"]
        rp.assert_same_bits(s_xam[:N], xam[:N], "state means")
        rp.assert_same_bits(s_Xap[:N], Xap[:N], "state perturbations")
        rp.assert_same_bits(s_Xap[N:], rp.scale_rows(Xap[N:], j), "obs perturbations")
        rp.assert_diag_bits(s_diag, rp.scaled_diag(diag, j), "diagnostics")


def test_helpers_have_teeth():
    c = rp.mixed_case(*rp.MIXED_SHAPES[0])
    xam, Xap, diag = rp.run_oracle(c)
    N = c["N"]
    post = xam[:N, None] + Xap[:N]
    small = int(np.flatnonzero(c["s_row"] == 1e-6)[3])
    # one value of a 1e-6-scale row, off by 1e-9 of that row's scale: invisible to the array-wide metric
    bad = post.copy()
    bad[small, 2] += 1e-9 * np.max(np.abs(post[small]))
    assert_parity(bad, post, "array-wide")
    with pytest.raises(AssertionError, match="own tolerance"):
        rp.assert_rows_close(bad, post, "per row")
    bad = Xap.copy()
    bad[small, 1] += 1e-9 * np.max(np.abs(Xap[small]))
    assert_parity(bad, Xap, "array-wide")
    with pytest.raises(AssertionError, match="own tolerance"):
        rp.assert_augmented_close(xam, bad, xam, Xap, "per row")
    k = int(np.argmin(np.where(np.isnan(diag["post_var"]), np.inf, diag["post_var"])))
    worse = dict(diag, post_var=diag["post_var"].copy())
    worse["post_var"][k] *= 1.0 + 1e-9
    assert_parity(worse["post_var"], diag["post_var"], "array-wide")
    with pytest.raises(AssertionError, match="own tolerance"):
        rp.assert_diag_close(worse, diag, "per ob")
    flipped = dict(diag, assimilated=~diag["assimilated"])
    with pytest.raises(AssertionError):
        rp.assert_diag_close(flipped, diag, "flags")
    # one flipped low mantissa bit
    for dtype in (np.float64, np.float32):
        a = post.astype(dtype)
        b = a.copy()
        rp.assert_same_bits(b, a, "equal")
        rp.bits(b)[small, 1] ^= 1
        assert_parity(b, a, "array-wide")
        with pytest.raises(AssertionError, match="differ in their bits"):
            rp.assert_same_bits(b, a, "one bit")
        rp.assert_same_bits(b, a, "other rows", rows=np.arange(N) != small)
    pb = rp.RowProblem(7)
    clean, _ = rp.oracle_members(pb, False)
    for kind in rp.POISON_KINDS:
        got, _ = rp.oracle_members(pb.with_state(rp.poison(pb.X32, kind)), False)
        leak = got.copy()
        rp.bits(leak)[14, 0] ^= 1                      # the row before a poisoned one
        with pytest.raises(AssertionError, match="differ in their bits"):
            rp.assert_poisoned(kind, leak, clean, kind, ref_rows=got[rp.POISON_ROWS])
        wrong = got.copy()
        wrong[15, 3] = 1.0                             # a poisoned row that came back with a number in it
        with pytest.raises(AssertionError):
            rp.assert_poisoned(kind, wrong, clean, kind, ref_rows=got[rp.POISON_ROWS])
    with pytest.raises(AssertionError):                # a scaling that would leave float32's normal range
        rp.scale_rows(np.full((48, 2), 1e-30, dtype=np.float32), np.full(48, -30))
    with pytest.raises(AssertionError):
        rp.assert_same_bits(np.array([0.0]), np.array([-0.0]), "the sign of zero")
    assert -0.0 == 0.0 and ASSIM.sum() == 10
