"""Adaptive inflation (Anderson 2009) without a GPU: the closed forms of the oracle tests/_anderson2009.py, the
AdaptiveInflation class (the reference's surface, disk round trip, fallback) and the EnSRF / ShardedEnSRF argument checks."""
import numpy as np
import pytest

import _anderson2009 as a09
from conftest import load_golden


def _one(lam, sd, gamma, d2, sp2=1.0, so2=0.5, **kw):
    """The update for a row with |r| = 1 and taper gamma (dot^2 = ss yy)."""
    out = a09.update(np.array([lam]), np.array([sd]), np.array([gamma]), np.array([2.0]), np.array([4.0]), 1.0, d2, sp2, so2,
                     **kw)
    return float(out[0][0]), float(out[1][0])


def test_field_unchanged_when_gamma_or_sd_is_zero():
    assert _one(1.4, 0.6, 0.0, 9.0) == (1.4, 0.6)
    assert _one(1.4, 0.0, 1.0, 9.0) == (1.4, 0.0)
    # r = 0: a row uncorrelated with the ob, or a zero-spread row
    lam, sd = a09.update(np.array([1.4, 1.4]), np.array([0.6, 0.6]), np.ones(2), np.array([0.0, 0.0]), np.array([3.0, 0.0]),
                         1.0, 9.0, 1.0, 0.5)
    assert np.array_equal(lam, [1.4, 1.4]) and np.array_equal(sd, [0.6, 0.6])


def test_mean_unchanged_when_innovation_matches_theta():
    lam, sp2, so2 = 1.44, 1.0, 0.5
    theta2 = lam * sp2 + so2                    # gamma = 1: q = sqrt(lam)
    new_lam, new_sd = _one(lam, 0.6, 1.0, theta2, sp2, so2)
    assert new_lam == lam
    assert new_sd <= 0.6


def test_nearer_root_is_dart_linear_bayes():
    for lam, s, g in [(1.3, 0.6, 0.37), (1.0, 0.2, -2.5), (4.0, 1.5, 1e-7), (1.1, 0.6, 40.0)]:
        t = 1.0 / g
        roots = np.roots([1.0, t - 2.0 * lam, lam * lam - s * s - t * lam]).real
        near = roots[np.argmin(np.abs(roots - lam))]
        stable = lam + 2.0 * s * s * g / (1.0 + np.sqrt(1.0 + 4.0 * s * s * g * g))
        assert abs(stable - near) <= 1e-9 * max(1.0, abs(near))


def test_bounds_clamp_and_sd_never_grows():
    rng = np.random.default_rng(0)
    n = 2000
    lam = rng.uniform(1.0, 3.0, n)
    sd = rng.uniform(0.05, 1.0, n)
    w = rng.uniform(0.0, 1.0, n)
    ss = rng.uniform(0.5, 2.0, n)
    dot = rng.uniform(-1.0, 1.0, n) * np.sqrt(ss)
    for d2 in (0.0, 0.3, 5.0, 400.0):
        nl, ns = a09.update(lam, sd, w, dot, ss, 1.0, d2, 1.3, 0.4, lower=1.2, upper=2.5, sd_lower=0.1)
        moved = nl != lam
        assert np.all((nl[moved] >= 1.2) & (nl[moved] <= 2.5))
        assert np.all(ns <= sd) and np.all(ns[ns != sd] >= 0.1)
        assert np.all(np.isfinite(nl)) and np.all(np.isfinite(ns))
    # a large innovation pushes the mean up to the upper bound
    assert _one(2.0, 1.0, 1.0, 1e6, upper=2.5)[0] == 2.5
    # sd at or below sd_lower stays
    assert _one(1.5, 0.3, 1.0, 50.0, sd_lower=0.3)[1] == 0.3


def test_gamma_one_moves_mean_toward_the_innovation_estimate():
    """A row equal to the observed quantity (gamma = 1): the mean moves toward (D^2 - so2) / sp2."""
    sp2, so2 = 1.0, 0.5
    for d2, lam in [(4.0, 1.2), (0.6, 2.0), (2.5, 1.0), (1.0, 1.8)]:
        target = (d2 - so2) / sp2
        new, _ = _one(lam, 0.6, 1.0, d2, sp2, so2, lower=1e-3)
        assert abs(new - target) < abs(lam - target)
        assert (new - lam) * (target - lam) > 0


def test_inflate_closed_form():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((50, 9)) + 3.0
    lam = rng.uniform(1.0, 2.0, 50)
    lam[::4] = 1.0
    Y = a09.inflate(X, lam)
    assert np.array_equal(Y[::4], X[::4])
    np.testing.assert_allclose(Y.var(axis=1), lam * X.var(axis=1), rtol=1e-12)
    np.testing.assert_allclose(Y.mean(axis=1), X.mean(axis=1), rtol=1e-12)


def test_oracle_cycle_unit_field_is_the_plain_oracle():
    from oracle import ensrf_oracle as orc
    g = load_golden("G5")
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    X = g["X"].reshape(N, M)
    field = np.stack([np.ones(N), np.zeros(N)], axis=1)
    post, f, diag, _ = a09.cycle(X, lambda Xi: g["HX"], g["ob_value"], g["ob_error"], g["ob_assim"], g["ob_lat"], g["ob_lon"],
                                 g["ob_radius"], g["grid_lat"], g["grid_lon"], (nvar, nt, ny, nx), field)
    assert np.array_equal(f, field)
    np.testing.assert_allclose(post, g["post"], rtol=1e-12, atol=1e-12 * np.abs(g["post"]).max())


# ---- the Python class ----------------------------------------------------------------------------------------------------
def _state(nt=3, ny=4, nx=5, M=6, nvar=2, datetimes=True):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(2)
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(-100, -90, nx), indexing="ij")
    vt = np.datetime64("2026-01-01T00") + np.arange(nt) * np.timedelta64(6, "h") if datetimes else None
    return EnsembleState.from_array(rng.standard_normal((nvar, nt, ny, nx, M)), lat, lon, validtime=vt)


def test_initial_field_shape_and_coordinates(tmp_path):
    from efa_xray_amd import AdaptiveInflation
    st = _state()
    ai = AdaptiveInflation(st, ("spatial", str(tmp_path / "missing.nc"), (1.1, 0.6)))
    assert ai.inftype == "spatial"
    f = ai.inflation
    assert f.vars() == st.vars()
    for name in st.vars():
        assert f.variables[name].shape == (3, 4, 5, 2)
        assert np.all(f.variables[name][..., 0] == 1.1) and np.all(f.variables[name][..., 1] == 0.6)
    np.testing.assert_array_equal(f.coords["validtime"], [0.0, 6.0, 12.0])
    np.testing.assert_array_equal(f.coords["lat"], st.coords["lat"])
    np.testing.assert_array_equal(f.coords["lon"], st.coords["lon"])
    assert list(f.coords["moment"]) == ["mean", "std"]
    # row order of the state's to_vect
    v = f.to_vect()
    assert v.shape == (st.nstate(), 2)


def test_save_to_disk_round_trips(tmp_path):
    from efa_xray_amd import AdaptiveInflation
    st = _state()
    ai = AdaptiveInflation(st, ("spatial", None, (1.0, 0.6)))
    rng = np.random.default_rng(3)
    ai.inflation.from_vect(np.stack([rng.uniform(1, 2, st.nstate()), rng.uniform(0.1, 1, st.nstate())], axis=1))
    fn = str(tmp_path / "prior_inflation.nc")
    ai.save_to_disk(fn)
    back = AdaptiveInflation(st, ("spatial", fn, (5.0, 5.0)))
    np.testing.assert_array_equal(back.inflation.to_vect(), ai.inflation.to_vect())
    np.testing.assert_array_equal(back.inflation.coords["validtime"], ai.inflation.coords["validtime"])
    np.testing.assert_array_equal(back.inflation.coords["lat"], st.coords["lat"])


def test_missing_or_bad_file_falls_back_to_initvals(tmp_path):
    from efa_xray_amd import AdaptiveInflation
    st = _state()
    bad = tmp_path / "bad.nc"
    bad.write_text("not a netCDF file")
    for infile in (str(tmp_path / "none.nc"), str(bad), None):
        ai = AdaptiveInflation(st, ("x", infile, (1.3, 0.2)))
        assert np.all(ai.inflation.to_vect() == [1.3, 0.2])


def test_inflate_state_returns_a_new_state():
    from efa_xray_amd import AdaptiveInflation
    st = _state()
    before = st.to_vect().copy()
    ai = AdaptiveInflation(st, ("x", None, (1.0, 0.6)))
    lam = np.linspace(1.0, 2.0, st.nstate())
    ai.inflation.from_vect(np.stack([lam, np.full(st.nstate(), 0.6)], axis=1))
    out = ai.inflate_state(st)
    assert out is not st and np.array_equal(st.to_vect(), before)
    np.testing.assert_allclose(out.to_vect(), a09.inflate(before, lam), rtol=1e-14, atol=1e-14)
    assert np.array_equal(out.to_vect()[0], before[0])            # lambda 1: bit for bit


def test_bad_bounds_raise():
    from efa_xray_amd import AdaptiveInflation
    st = _state()
    for kw in (dict(lower=0.0), dict(lower=2.0, upper=1.5), dict(sd_lower=-1.0), dict(upper=np.inf)):
        with pytest.raises(ValueError):
            AdaptiveInflation(st, ("x", None, (1.0, 0.6)), **kw)


def test_ensrf_rejects_what_it_does_not_support():
    from efa_xray_amd import AdaptiveInflation, EnSRF
    from efa_xray_amd.distributed import ShardedEnSRF
    st = _state()
    ai = AdaptiveInflation(st, ("x", None, (1.0, 0.6)))
    with pytest.raises(ValueError, match="loc='GC'"):
        EnSRF(st, [], verbose=False, loc=None, adaptive_inflation=ai)
    with pytest.raises(ValueError, match="exclusive"):
        EnSRF(st, [], verbose=False, loc="GC", inflation=1.1, adaptive_inflation=ai)
    with pytest.raises(ValueError, match="AdaptiveInflation"):
        EnSRF(st, [], verbose=False, loc="GC", adaptive_inflation=(1.0, 0.6))
    other = _state(nx=6)
    with pytest.raises(ValueError, match="shape"):
        EnSRF(other, [], verbose=False, loc="GC", adaptive_inflation=ai)
    moved = _state()
    moved.coords["lat"] = moved.coords["lat"] + 1.0
    with pytest.raises(ValueError, match="grid"):
        EnSRF(moved, [], verbose=False, loc="GC", adaptive_inflation=ai)
    f = EnSRF(st, [], verbose=False, loc="GC", adaptive_inflation=ai, rtps=0.5)    # relaxation may be combined
    with pytest.raises(ValueError, match="out of scope"):
        f.update_arrays(np.zeros(st.nstate()), np.zeros((st.nstate(), st.nmems())))
    sh = ShardedEnSRF.__new__(ShardedEnSRF)
    with pytest.raises(ValueError, match="out of scope"):
        sh.assimilate(None, None, None, {}, adaptive_inflation=ai)
    with pytest.raises(ValueError, match="out of scope"):
        sh.update(None, None, None, None, {}, adaptive_inflation=ai)


def test_invalid_field_values_raise(tmp_path):
    from efa_xray_amd import AdaptiveInflation, EnSRF
    st = _state()
    for initvals, kw in (((0.5, 0.6), {}), ((-1.0, 0.6), dict(lower=1e-3)), ((1.0, -0.1), {}), ((np.nan, 0.6), {}),
                         ((2.0, 0.6), dict(upper=1.5))):
        with pytest.raises(ValueError, match="inflation field"):
            AdaptiveInflation(st, ("x", None, initvals), **kw)
    # a file whose values are out of bounds is an error, not a reason to start over from initvals
    ai = AdaptiveInflation(st, ("x", None, (1.0, 0.6)), lower=0.5)
    ai.inflation.from_vect(np.full((st.nstate(), 2), 0.7))
    fn = str(tmp_path / "low.nc")
    ai.save_to_disk(fn)
    with pytest.raises(ValueError, match="inflation field"):
        AdaptiveInflation(st, ("x", fn, (1.0, 0.6)))
    # values set later are checked before use
    ok = AdaptiveInflation(st, ("x", None, (1.0, 0.6)))
    ok.inflation.from_vect(np.full((st.nstate(), 2), np.nan))
    with pytest.raises(ValueError, match="inflation field"):
        EnSRF(st, [], verbose=False, loc="GC", adaptive_inflation=ok)
    with pytest.raises(ValueError, match="inflation field"):
        ok.inflate_state(st)
