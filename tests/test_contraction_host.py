"""The CPU side of tests/test_gpu_contraction.py: the shape lists reach every class of the launch by the launch
mirror, the reference alone stays well inside the bound, and the checks see a dropped member, two swapped obs and a KH-40 shape
served by the KH-32 kernel."""
import numpy as np
import pytest

import _contraction as ct

F32, F64 = np.float32, np.float64


def _plans(shapes):
    return [ct.launch(*s) for s in shapes]


def test_the_mirror_restates_the_launch():
    assert ct.KH_ALL == tuple(range(8, 8 * len(ct.KH_ALL) + 1, 8)) and ct.KH_ALL[-1] == ct.RA_MAX_M // 2
    assert ct.kRaRows == 32 * (ct.kRaThreads // 64) and ct.kBK % 4 == 0
    assert ct.launch(0, 8, 5) is None and ct.launch(5, 8, 0) is None
    # KH = 8 ceil(M / 16): both ends of every instantiation, then the general kernel
    for j, KH in enumerate(ct.KH_ALL):
        for M in (16 * j + 4, 16 * j + 16):
            assert ct.launch(300, M, 300) == dict(kernel="ra", KH=KH, nrb=2, split=2, tiles=3, per=2, idle=0, one_tile=1, trips=1)
    assert ct.launch(300, ct.RA_MAX_M + 4, 300)["kernel"] == "general"
    # the issue's example: 513..640 obs are 5 tiles in 4 shares of 2, the last share empty
    for P in (4 * ct.kRaObs + 1, 600, 5 * ct.kRaObs):
        p = ct.launch(257, 20, P)
        assert (p["tiles"], p["split"], p["per"], p["idle"], p["one_tile"]) == (5, 4, 2, 1, 1), (P, p)
    assert ct.launch(257, 20, 2049)["idle"] == 7
    # many row blocks: no split
    assert ct.launch(ct.kRaRows * ct.SPLIT_BLOCKS, 128, 4096)["split"] == 1
    assert ct.launch(ct.kRaRows * ct.SPLIT_BLOCKS // 2, 128, 4096)["split"] == 2
    # the member order of both kernels
    assert ct.member_order(20) == [0, 16, 1, 17, 2, 18, 3, 19, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
    assert ct.member_order(132) == list(range(132))


def test_shape_lists_reach_every_class():
    ra, gen = _plans(ct.RA_SHAPES), _plans(ct.GEN_SHAPES)
    assert all(p["kernel"] == "ra" for p in ra) and all(p["kernel"] == "general" for p in gen)
    # every instantiation, at both ends of its member range
    for j, KH in enumerate(ct.KH_ALL):
        ms = set(s[1] for s, p in zip(ct.RA_SHAPES, ra) if p["KH"] == KH)
        assert 16 * j + 4 in ms and 16 * j + 16 in ms, "KH %d is not run at both ends: %r" % (KH, sorted(ms))
    assert set(p["split"] for p in ra) == {1, 2, 4, 8, 16}
    assert any(p["idle"] > 0 for p in ra), "no shape leaves a workgroup without a tile"
    assert any(p["per"] == 1 and p["split"] > 1 for p in ra) and any(p["per"] > 1 and p["one_tile"] for p in ra)
    # the general kernel: with and without a partial last K chunk, beyond 256 members, one trip here and two at BIG_SHAPE
    assert any(p["partial_k"] for p in gen) and any(not p["partial_k"] for p in gen)
    for M in (132, 252, 260):
        assert ct.launch(128, M, 128)["partial_k"] and M in [s[1] for s in ct.GEN_SHAPES]
    assert any(s[1] > 256 and p["partial_k"] for s, p in zip(ct.GEN_SHAPES, gen))
    assert any(s[1] > 256 and not p["partial_k"] for s, p in zip(ct.GEN_SHAPES, gen))
    assert all(p["trips"] == 1 for p in ra + gen)
    # N and P on each side of 32, 64, 128, 256 (ra: wave rows, halves, tiles, row blocks; general: kBM, kBN)
    for edge in (32, 64, 128, 256):
        for axis in (0, 2):
            have = set(s[axis] for s in ct.RA_SHAPES)
            assert edge - 1 in have and edge + 1 in have, (edge, axis)
    for axis in (0, 2):
        have = set(s[axis] for s in ct.GEN_SHAPES)
        assert {ct.kBM - 1, ct.kBM, ct.kBM + 1} <= have and max(have) > 2 * ct.kBM
    # the two store paths of k_contract_f32_ra meet at row0 + 32 <= N and colh + 64 <= P: all four combinations within one call
    for N, M, P in ct.RA_SHAPES:
        if N > 32 and N % 32 and P > 64 and P % 64:
            break
    else:
        raise AssertionError("no shape has interior and masked stores in both directions")
    assert (32, 116, 64) in ct.RA_SHAPES and (256, 48, 128) in ct.RA_SHAPES      # nothing masked at all


def test_the_big_shape_is_the_first_with_two_trips():
    N, M, P = ct.BIG_SHAPE
    p = ct.launch(N, M, P)
    assert p["kernel"] == "general" and p["partial_k"] and p["grid_y"] == ct.GRID_Y_CAP
    assert p["trips"] == 2 and p["nrb"] == ct.GRID_Y_CAP + 2 and N % ct.kBM == 1
    assert ct.launch(ct.kBM * ct.GRID_Y_CAP, M, P)["trips"] == 1
    assert N == 128 * 65535 + 129
    # the exact relations run one shape per kernel and KH class, partial in both directions
    for M in ct.EXACT_M:
        q = ct.launch(ct.EXACT_N, M, ct.EXACT_P)
        assert ct.EXACT_N % (ct.kRaRows if q["kernel"] == "ra" else ct.kBM) and ct.EXACT_P % ct.kRaObs and ct.EXACT_P % ct.kBN
    assert [ct.launch(ct.EXACT_N, M, ct.EXACT_P)["KH"] for M in ct.EXACT_M] == [16, 56, 64, None, None]


@pytest.mark.parametrize("N,M,P", ct.SHAPES)
def test_the_chain_alone_stays_inside_a_quarter_of_the_bound(N, M, P):
    """The emulated f32 chain against float64: what an exact kernel is expected to give.  Measured at 24 member counts from 4 to
    1000 on 97 x 131 unit-normal operands: worst 0.046 of the bound, about 4.3 * 2^-24 * sum|a b|."""
    ref, scale, ch = ct.expected(N, M, P)
    worst = ct.assert_within_bound(ch, ref, scale, "chain %d x %d x %d" % (N, M, P), fraction=0.25)
    print("chain alone, %d x %d x %d: worst err/bound %.3f" % (N, M, P, worst))


@pytest.mark.parametrize("M", [4, 20, 100, 128, 132, 260, 1000])
def test_a_wider_intermediate_gives_the_same_chain(M):
    """acc + x y rounded to float64 and then to float32 against the same through np.longdouble: no element differs, so the
    double rounding of the emulation is no source of doubt at these sizes."""
    X, Ye = ct.problem(97, M, 131)
    wide = ct.chain(X, Ye, dtype=np.longdouble)
    ct.assert_same_bits(ct.chain(X, Ye), wide, "float64 against longdouble, M = %d" % M)
    ref, scale = ct.reference(X, Ye)
    ct.assert_within_bound(wide, ref, scale, "M = %d" % M, fraction=0.25)


def _violations(C, ref, scale):
    q = ct.err_over_bound(C, ref, scale)
    return ~(q <= 1.0)


@pytest.mark.parametrize("N,M,P", [(97, 4, 131), (97, 68, 131), (97, 128, 131), (97, 132, 131), (97, 1000, 131)])
def test_a_dropped_member_is_seen_almost_everywhere(N, M, P):
    X, Ye = ct.problem(N, M, P)
    ref, scale = ct.reference(X, Ye)
    for drop in (0, M // 2, M - 1):
        order = [m for m in ct.member_order(M) if m != drop]
        bad = _violations(ct.chain(X, Ye, order=order), ref, scale)
        assert bad.mean() >= 0.98, "member %d of %d dropped: only %.1f %% of the elements notice" % (drop, M, 100 * bad.mean())
        with pytest.raises(AssertionError):
            ct.assert_within_bound(ct.chain(X, Ye, order=order), ref, scale, "dropped")


def test_swapped_obs_and_a_wrong_instantiation_are_seen():
    # a KH-40 shape served by the KH-32 kernel: members 64.. are never read
    N, M, P = 65, 68, 129
    assert ct.launch(N, M, P)["KH"] == 40
    X, Ye = ct.problem(N, M, P)
    ref, scale = ct.reference(X, Ye)
    half = ct.chain(X, Ye, order=[m for m in ct.member_order(64) if m < 64])
    assert _violations(half, ref, scale).mean() >= 0.98
    # two obs swapped: exactly their two columns are wrong
    Ys = np.array(Ye)
    Ys[[63, 64]] = Ys[[64, 63]]
    bad = _violations(ct.chain(X, Ys), ref, scale)
    assert bad[:, [63, 64]].mean() >= 0.98 and not np.delete(bad, [63, 64], axis=1).any()
    with pytest.raises(AssertionError):
        ct.assert_chain_close(ct.chain(X, Ys), ct.chain(X, Ye), "swapped obs")
    # the chain check alone sees a dropped member too, and lets the honest chain through
    ct.assert_chain_close(ct.chain(X, Ye), ct.chain(X, Ye, dtype=np.longdouble), "honest")
    with pytest.raises(AssertionError):
        ct.assert_chain_close(half, ct.chain(X, Ye), "half the members")


@pytest.mark.parametrize("M", ct.EXACT_M)
def test_the_chain_obeys_the_exact_relations(M):
    """The relations tests/test_gpu_contraction.py asks of the kernels hold for the documented chain itself, bit for bit:
    powers of two on the rows of X and of Ye, a sub-block of rows and of obs, one poisoned row or ob."""
    N, P = 61, 70
    X, Ye = ct.problem(N, M, P)
    kx, ky = ct.exponents(N, 1), ct.exponents(P, 2)
    ct.assert_scaling_exact(X, Ye, kx, ky)
    C = ct.chain(X, Ye)
    ct.assert_same_bits(ct.chain(ct.scale_pow2(X, kx), ct.scale_pow2(Ye, ky)), ct.scaled_result(C, kx, ky), "scaling")
    ct.assert_same_bits(ct.chain(X[17:50], Ye[33:69]), np.ascontiguousarray(C[17:50, 33:69]), "position")
    for kind, value in (("nan", np.nan), ("inf", np.inf), ("zero", 0.0)):
        Xp = np.array(X)
        Xp[31] = value
        keep = np.ones((N, P), dtype=bool)
        keep[31] = False
        with np.errstate(invalid="ignore"):
            Cp = ct.chain(Xp, Ye)
        ct.assert_same_bits(Cp, C, kind, keep=keep)
        assert ct.poisoned_as(kind, Cp[31])


def test_scaling_helpers_refuse_what_is_not_exact():
    X, Ye = ct.problem(61, 20, 70)
    with pytest.raises(AssertionError):
        ct.scale_pow2(X, np.full(61, -140))          # subnormal inputs
    with pytest.raises(AssertionError):
        ct.assert_scaling_exact(X, Ye, np.full(61, -45), np.full(70, -45))     # subnormal products
    with pytest.raises(AssertionError):
        ct.assert_scaling_exact(X, Ye, np.full(61, 64), np.full(70, 64))       # overflowing products
