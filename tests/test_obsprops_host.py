"""The conditions tests/test_gpu_obsprops.py rests on, proven on the CPU: the oracle keeps its bits under every
ignored input of Parts A and C and under the zero-spread obs of Part D, the outlier model rejects what Part B poisons, every
margin band of Part E is hit and predicted, the float64 oracle is within CONDITION of an np.longdouble run of the same loop on
every margin case, and the uncentred rows of Part F sit on the side of the centring guard the GPU test expects."""
import numpy as np
import pytest

import _obsprops as op
import _outlier as qc
import _rowprops as rp
from _phase_a_guard import FALLS_BACK, SAFE, expected_kind, obs_block_min_ratio
from _rowprops import CONDITION, RTOL, assert_same_bits

LOCS = [False, True]


def _assert_oracle_bits(got, want, what, obs=None, rows=None):
    """(xam, Xap, diag) of two oracle runs: state rows and the obs rows in `rows` (a mask over the P obs), the diagnostics of `obs`."""
    keep = np.ones(len(got[0]), dtype=bool)
    if rows is not None:
        keep[op.N:] = rows
    assert_same_bits(got[0], want[0], what + ": xam", rows=keep)
    assert_same_bits(got[1], want[1], what + ": Xap", rows=keep)
    op.assert_diag_bits(got[2], want[2], what, obs=obs)


@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", op.SIZES)
def test_base_cases_keep_the_leaders(M, loc):
    """Parts A to D assert the leader's own kind on the clean problem: its guard ratio must predict it, whatever the flags."""
    for flag, rows in ((False, op.SPECIAL), (True, op.SPECIAL), (False, op.SPECIAL_SECOND), (False, op.zero_spread_rows()),
                       (True, np.array(op.UNCENTRED_ROWS))):
        c = op.base_case(M, loc, flag, rows=rows)
        assert c["asm"][op.NEIGHBOURS_ON[~np.isin(op.NEIGHBOURS_ON, rows)]].all() and (c["asm"][rows] == flag).all()
        assert c["asm"][121] and c["asm"][122]
        xam, Xap, diag, ratio = op.oracle_case(c)
        assert expected_kind(ratio, M) == (4 if M <= 128 else 2), "M=%d loc=%r: guard min ratio %.3e" % (M, loc, ratio)
        geo = dict(ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"]) if loc else {}
        alone, _ = obs_block_min_ratio(c["HX"], c["val"], c["err"], c["asm"], **geo)
        assert abs(alone - ratio) <= 1e-9 * ratio, "the obs block alone predicts another ratio"
        assert np.isfinite(xam).all() and np.isfinite(Xap).all()


@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [7, 100, 130])
def test_oracle_ignores_value_and_error_of_unassimilated_obs(M, loc):
    """Part A: ensrf.py:74-76 comes before the first read of either."""
    for rows in op.SPECIAL_SETS:
        c = op.base_case(M, loc, False, rows=rows)
        clean = op.oracle_case(c)
        for pair in op.IGNORED_FINITE + op.IGNORED_NONFINITE:
            _assert_oracle_bits(op.oracle_case(op.with_ignored(c, pair, rows)), clean, "M=%d loc=%r %r" % (M, loc, pair))


@pytest.mark.parametrize("what", ["value", "error", "row"])
def test_outlier_model_rejects_what_part_b_poisons(what):
    """Part B: the NumPy mask rejects every poisoned ob and leaves every other flag as the reference case has it."""
    for M, loc in ((24, False), (100, True)):
        bad, ref, ym, Yp = op.outlier_case(M, loc, what)
        with np.errstate(invalid="ignore"):
            rej = qc.outlier_mask(ym, Yp, bad["val"], bad["err"], bad["asm"], op.OUTLIER_T)
            rej_ref = qc.outlier_mask(ym, Yp, ref["val"], ref["err"], ref["asm"], op.OUTLIER_T)
        assert rej[op.SPECIAL].all() and not rej_ref[op.SPECIAL].any()
        assert np.array_equal(bad["asm"] & ~rej, ref["asm"] & ~rej_ref)
        keep = op.others(op.SPECIAL)
        assert qc.clear_of_threshold(ym[keep], Yp[keep], ref["val"][keep], ref["err"][keep], op.OUTLIER_T)


@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [7, 100, 256])
def test_oracle_keeps_poisoned_rows_of_unassimilated_obs_to_themselves(M, loc):
    """Part C: every other row and every other ob's diagnostics keep the bits of the clean run; a NaN row stays NaN."""
    for rows in op.SPECIAL_SETS:
        c = op.base_case(M, loc, False, rows=rows)
        ym, Yp = op.priors(c)
        clean = op.oracle_block(c, ym, Yp)
        keep = op.others(rows)
        for kind in op.ROW_POISONS:
            got = op.oracle_block(c, ym, op.poison_obs_rows(Yp, kind, rows))
            _assert_oracle_bits(got, clean, "M=%d loc=%r %s" % (M, loc, kind), obs=keep, rows=keep)
            own = got[1][op.N:][rows]
            if kind == "nan":
                assert np.isnan(own).all()
            elif kind == "zero":
                assert (own == 0).all() and (got[2]["prior_var"][rows] == 0).all()
            else:
                assert not np.isfinite(own).all()
            assert not got[2]["assimilated"][rows].any()
            assert np.isnan(got[3]) or got[3] == clean[3], "the guard ratio of the assimilated obs moved"


@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [7, 24, 128, 130])
def test_oracle_zero_spread_obs_change_nothing(M, loc):
    """Part D: kmat == 0.  Finite everywhere, post_var 0, post_mean = prior_mean, and every row and every other diagnostic
    keeps the bits of the run with these obs' flags off."""
    rows = op.zero_spread_rows()
    on, off = op.zero_spread_case(M, loc, True), op.zero_spread_case(M, loc, False)
    got, ref = op.oracle_case(on), op.oracle_case(off)
    assert all(np.isfinite(a).all() for a in got[:2])
    d = got[2]
    assert d["assimilated"][rows].all() and (d["post_var"][rows] == 0).all() and (d["prior_var"][rows] == 0).all()
    assert np.array_equal(d["post_mean"][rows], d["prior_mean"][rows])
    _assert_oracle_bits(got, ref, "M=%d loc=%r" % (M, loc), obs=op.others(rows))
    for key in ("prior_mean", "prior_var"):
        assert_same_bits(d[key], ref[2][key], key)
    # the guard: G_kk = 0 is not above its threshold of 0, so a leader may hand the block to the vector chain
    assert got[3] == 0.0 and expected_kind(ref[3], M) == (4 if M <= 128 else 2)


@pytest.mark.parametrize("name,M,loc", op.MARGIN_CASES)
def test_margin_cases_hit_their_bands_and_the_oracle_is_conditioned(name, M, loc):
    """Part E: the min ratio of every listed block in its band, the others in [SAFE, 2 SAFE]; the guard predictor says 4 or 1;
    the float64 oracle within CONDITION of the np.longdouble run, per row and per ob."""
    c = op.margin(name, M, loc)
    lo, hi, blocks = op.MARGIN_BANDS[name]
    w = "%s M=%d loc=%r" % (name, M, loc)
    for b in (0, 1, 2):
        t_lo, t_hi = (lo, hi) if b in blocks else (SAFE, 2 * SAFE)
        assert t_lo <= c["block_ratios"][b] <= t_hi, "%s: block %d has min ratio %.3e" % (w, b, c["block_ratios"][b])
    assert c["block_ratios"][3] > 2 * SAFE
    for first, second, block in c["pairs"]:
        if block is None:
            assert c["ratios"][second] == 1.0, w + ": the ratio does not restart at the block edge"
        else:
            t_lo, t_hi = (lo, hi) if block in blocks else (SAFE, 2 * SAFE)
            assert t_lo <= c["ratios"][second] <= t_hi, "%s: pair %d|%d at %.3e" % (w, first, second, c["ratios"][second])
        if loc:
            assert c["ob_lat"][first] == c["ob_lat"][second] and c["ob_lon"][first] == c["ob_lon"][second]
    geo = dict(ob_lat=c["ob_lat"], ob_lon=c["ob_lon"], ob_halfwidth=c["hw"]) if loc else {}
    ratio, _ = obs_block_min_ratio(c["HX"], c["val"], c["err"], c["asm"], **geo)
    assert ratio == min(c["block_ratios"].values())
    assert expected_kind(ratio, M) == (4 if name == "safe" else 1), "%s: %.3e" % (w, ratio)
    assert (lo, hi) == ((SAFE, 2 * SAFE) if name == "safe" else (FALLS_BACK / 2, FALLS_BACK))
    xam, Xap, diag, r2 = rp.run_oracle(c, guard=True)
    assert abs(r2 - ratio) <= 1e-9 * ratio
    xl, Xl, dl = rp.run_oracle(c, dtype=np.longdouble)
    dl = dict((k, np.asarray(v, dtype=np.float64) if k != "assimilated" else v) for k, v in dl.items())
    a, b = rp.assert_augmented_close(xam, Xap, np.asarray(xl, dtype=np.float64), np.asarray(Xl, dtype=np.float64), w, tol=CONDITION / RTOL)
    worst = max(a, b, rp.assert_diag_close(diag, dl, w, tol=CONDITION / RTOL)) * RTOL
    print("%s: q %.2e .. %.2e, block min ratios %s; float64 oracle against np.longdouble: %.2e" % (
        w, min(c["q"].values()), max(c["q"].values()), " ".join("%.2e" % c["block_ratios"][b] for b in range(4)), worst))


@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("M", [7, 100, 128])
def test_uncentred_rows_sit_where_the_centring_guard_is_expected(M, loc):
    """Part F: mean^2 against 1e-22 min(error, variance) -- below at c = 1e-12, above from 1e-10 on -- and the oracle on the
    shifted rows is the oracle on the centred ones to rounding at the small shifts."""
    c = op.base_case(M, loc, True, rows=np.array(op.UNCENTRED_ROWS))
    ym, Yp = op.priors(c)
    ref = op.oracle_obs_only(c, ym, Yp)
    for cfac in op.UNCENTRED_C:
        Ys = op.uncentred(Yp, cfac)
        for r in op.UNCENTRED_ROWS:
            pm, var = Ys[r].mean(), np.var(Ys[r])
            assert (pm * pm <= 1e-22 * min(c["err"][r], var)) == (cfac < 1e-11), "M=%d row %d c=%g" % (M, r, cfac)
        keep = op.others(np.array(op.UNCENTRED_ROWS))
        assert (np.abs(Ys[keep].mean(axis=1)) ** 2 <= 1e-24 * np.var(Ys[keep], axis=1)).all(), "a clean row is not centred"
        xam, Xap, diag = op.oracle_obs_only(c, ym, Ys)
        assert np.isfinite(Xap).all() and diag["assimilated"][list(op.UNCENTRED_ROWS)].all()
        if cfac <= 1e-10:
            rp.assert_diag_close(diag, ref[2], "c=%g" % cfac, tol=1e-3)
