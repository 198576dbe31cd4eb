"""The taper probe (tests/_taper_probe.py) through the float64 oracle, without a GPU: the extraction recovers the long-double
weights, the caps on excluded pairs hold for every geometry the GPU tests use, and the float64 zero pattern follows the probe's
rule.  This guards the helper, and makes "the reference alone stays within the cap" something that is checked.

The oracle's worst err / tol was 0.072 over the sizes tried when the probe was written; 0.25 leaves room for another NumPy build.
"""
import numpy as np
import pytest

import _taper_probe as tp
import _vertloc as vl
from oracle import ensrf_oracle as orc

ORACLE_CAP = 0.25


def _oracle_cycle(p):
    xbm, Xbp = orc.format_prior_state(p.X, p.HX)
    if p.n_lead > 1:
        # (rows= wants a 2-D grid: the probe's columns as one row of ncol points)
        return vl.ensrf_update_vert(xbm, Xbp, p.rows, p.ob_value, p.ob_error, p.ob_assim, p.ob_lat, p.ob_lon, p.ob_hw,
                                    p.grid_lat[None, :], p.grid_lon[None, :], (p.n_lead, 1, 1, p.ncol), lead_vert=p.lead_vert,
                                    ob_vert=p.ob_vert, ob_vert_halfwidth=p.ob_vhw, obs_taper="vector")
    return orc.ensrf_update(xbm, Xbp, p.rows, p.ob_value, p.ob_error, p.ob_assim, loc="GC", ob_lat=p.ob_lat, ob_lon=p.ob_lon,
                            ob_halfwidth=p.ob_hw, grid_lat=p.grid_lat, grid_lon=p.grid_lon, state_shape=(1, 1, 1, p.ncol),
                            obs_taper="vector")


@pytest.mark.parametrize("name", list(tp.CASES))
def test_extraction_recovers_the_long_double_weights_from_the_oracle(name):
    p = tp.get_probe(name)
    xam, Xap, diag = _oracle_cycle(p)
    N, w = p.rows, p.wit_idx
    s = p.check(name + " oracle state", p.state, xam[:N], Xap[:N], p.mu, cap=ORACLE_CAP, need_cut=True)
    o = p.check(name + " oracle obs-obs", p.obs, xam[N + w], Xap[N + w], p.ym[w], cap=ORACLE_CAP, need_cut=True)
    if p.state["r"].size < 10000:
        assert s[2] == 0 and o[2] == 0, "a case under 10 000 pairs carries no near-antipodal point"
    # the probing obs do not move one another: each sees its own prior when its turn comes
    k = p.probe_idx
    assert np.all(diag["assimilated"][k]) and not np.any(diag["assimilated"][w])
    np.testing.assert_allclose(diag["prior_mean"][k], p.ym[k], rtol=0, atol=16 * tp.EPS * p.M * 8)
    np.testing.assert_allclose(diag["post_mean"][k], (p.ym[k] + p.K * p.innov).astype(float), rtol=0, atol=16 * tp.EPS * p.M * 8)
    np.testing.assert_allclose(diag["post_var"][k], ((p.yy / p.M) * (1 - p.beta * p.K) ** 2).astype(float),
                               rtol=16 * tp.EPS * p.M)


@pytest.mark.parametrize("name", list(tp.CASES))
def test_float64_zero_pattern_follows_the_rule(name):
    """Beyond 2 + tol_r half-widths the float64 formulas give exactly 0 (or NaN -> 0 at an antipode), inside 2 - 1e-2 they give a
    non-zero weight; in between the pattern is not defined."""
    p = tp.get_probe(name)
    k = p.probe_idx
    hs = dict((key, v[:p.ncol] if np.ndim(v) == 2 else v) for key, v in p.state.items())
    hs["v"] = tp.LD(1)
    ho = dict(p.obs, v=tp.LD(1))
    w = p.wit_idx
    for j, kk in enumerate(k):
        ws = orc.localize_state(p.grid_lat, p.grid_lon, p.ob_lat[kk], p.ob_lon[kk], p.ob_hw[kk])
        wo = orc.localize_obs_vec(p.ob_lat[w], p.ob_lon[w], p.ob_lat[kk], p.ob_lon[kk], p.ob_hw[kk])
        for got, ref in ((ws, hs), (wo, ho)):
            assert np.all(got[p.far(ref)[:, j]] == 0.0), (name, j)
            assert np.all(got[p.near(ref)[:, j]] != 0.0), (name, j)
            assert np.all(got[p.counted(dict(ref, wh=ref["wh"]))[:, j]] != 0.0), (name, j)      # the tighter rule of the pair counts
            ok = ~p.excluded(ref)[:, j]
            assert np.all(np.abs(got - ref["wh"][:, j].astype(float))[ok] <= p.tol(ref)[:, j][ok]), (name, j)


def test_the_cases_hold_what_the_gpu_tests_rely_on():
    for name in ("lane-regional", "odd-regional", "wide-regional", "cluster", "vertical-regional"):
        p = tp.get_probe(name)
        assert p.untouched_rows(p.state).sum() >= 3, name          # rows to compare bit for bit
    for name in ("lane-global", "wide-global", "cap", "obsobs"):
        p = tp.get_probe(name)
        assert sorted(np.abs(p.hw))[-2:] == [9000.0, 25000.0] and 0.5 in p.hw and -800.0 in p.hw
        k = int(np.argmax(p.hw))
        ref = p.state
        assert np.all(ref["r"][:, k] < 2 - 1e-2)                   # the 25 000 km ob reaches every column
    p = tp.get_probe("cluster")
    lo = p.block_bounds()[2]
    assert lo.max() >= 150, "cluster: no 16-column block is reached by 150 obs (the builder's 128-entry queue must wrap)"
    p = tp.get_probe("cap")
    assert p.ncol == 16437 and p.ncol * 64 > 2 * 524288
    # points on both sides of each threshold, both poles as columns, both longitude frames
    p = tp.get_probe("lane-global")
    r = p.state["r"].astype(float)
    for lo_, hi_ in ((0.0, 0.0), (1 - 2e-9, 1.0), (1.0, 1 + 2e-9), (2 - 2e-9, 2.0), (2.0, 2 + 2e-9)):
        assert np.any((r >= lo_) & (r <= hi_) & (r != 1.0) | ((r == 0.0) & (lo_ == hi_))), (lo_, hi_)
    assert 90.0 in p.grid_lat and -90.0 in p.grid_lat
    assert p.grid_lon.min() < 0 and p.grid_lon.max() > 360
    # the point at 2 - 3e-3 half-widths of every ob: a weight far above the tolerance, in every case that builds lists
    for name in ("lane-global", "odd-global", "wide-global", "cluster", "vertical"):
        q = tp.get_probe(name)
        r, w, tol = q.state["r"].astype(float), q.state["wh"].astype(float), q.tol(q.state)     # (the horizontal weight)
        sel = np.abs(r - (2 - 3e-3)) < 1e-6
        assert sel.sum() >= q.P // 2 and np.all(w[sel] > 1e-11) and (w[sel] > 10 * tol[sel]).sum() >= q.P // 2, name
    # ... and the point at 2 - 8e-4: beyond 2 - 1e-3, counted, in every case that builds lists
    for name in ("lane-regional", "lane-global", "odd-regional", "odd-global", "wide-regional", "wide-global", "cluster"):
        q = tp.get_probe(name)
        r = q.state["r"].astype(float)
        sel = (np.abs(r - (2 - 8e-4)) < 1e-6) & q.counted(q.state) & ~q.near(q.state)
        assert sel.sum() >= q.P // 2, name
    q0 = p.Q // 2
    assert p.ob_assim[:q0].sum() == 0 and p.ob_assim[q0:q0 + p.P].all() and p.ob_assim[q0 + p.P:].sum() == 0
