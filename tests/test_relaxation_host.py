"""Posterior relaxation (RTPP / RTPS, Whitaker & Hamill 2012) without a GPU: the EnSRF keywords and their validation, the C
ABI entry, and the closed forms the GPU tests check the library against (`relax`), applied to the oracle's posteriors of the
reference goldens."""
import math

import numpy as np
import pytest

from conftest import load_golden, GOLDEN_CASES
from oracle import ensrf_oracle as orc


def relax(prior, post, rtps=None, rtpp=None):
    """Closed forms of the relaxation on member rows (state row x member).
    RTPP: mean(xa) + (1 - a) (xa - mean(xa)) + a (xb - mean(xb)).
    RTPS: mean(xa) + (xa - mean(xa)) ((1 - a) + a sigma_b / sigma_a); rows with sigma_a == 0 unchanged.
    a == 0 returns the posterior as it is."""
    prior = np.asarray(prior, dtype=np.float64)
    post = np.asarray(post, dtype=np.float64)
    alpha = rtpp if rtpp is not None else rtps
    if not alpha:                       # None or 0: no relaxation, bit for bit
        return post.copy()
    am = post.mean(axis=1, keepdims=True)
    a = post - am
    b = prior - prior.mean(axis=1, keepdims=True)
    if rtpp is not None:
        return am + (1.0 - rtpp) * a + rtpp * b
    sa = np.sqrt((a * a).sum(axis=1))
    sb = np.sqrt((b * b).sum(axis=1))
    out = post.copy()
    ok = sa > 0
    scale = (1.0 - rtps) + rtps * sb[ok] / sa[ok]
    out[ok] = am[ok] + a[ok] * scale[:, None]
    return out


def golden_oracle(g):
    """(prior members, oracle posterior members) of a golden case."""
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    N = nvar * nt * ny * nx
    kw = {}
    if g["loc"] == "GC":
        kw = dict(loc="GC", ob_lat=g["ob_lat"], ob_lon=g["ob_lon"], ob_halfwidth=g["ob_radius"],
                  grid_lat=g["grid_lat"], grid_lon=g["grid_lon"], state_shape=(nvar, nt, ny, nx))
    X = g["X"].reshape(N, M)
    post, _, _, _ = orc.ensrf_cycle(X, g["HX"], g["ob_value"], g["ob_error"], g["ob_assim"], **kw)
    return X, post


def _state():
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(20, 40, 3), np.linspace(250, 270, 4), indexing="ij")
    return EnsembleState.from_array(rng.standard_normal((1, 1, 3, 4, 6)), lat, lon)


def test_ensrf_accepts_the_relaxation_keywords():
    from efa_xray_amd import EnSRF, _lib
    st = _state()
    assert EnSRF(st, [], verbose=False).relaxation == (_lib.RELAX_NONE, 0.0)
    assert EnSRF(st, [], verbose=False, rtps=0.9).relaxation == (_lib.RELAX_RTPS, 0.9)
    assert EnSRF(st, [], verbose=False, rtps=1.7).relaxation == (_lib.RELAX_RTPS, 1.7)
    assert EnSRF(st, [], verbose=False, rtpp=0.5).relaxation == (_lib.RELAX_RTPP, 0.5)
    assert EnSRF(st, [], verbose=False, rtpp=1).relaxation == (_lib.RELAX_RTPP, 1.0)
    assert EnSRF(st, [], verbose=False, rtps=None, rtpp=0.0).relaxation == (_lib.RELAX_RTPP, 0.0)


@pytest.mark.parametrize("kw", [dict(rtps=-0.1), dict(rtpp=-1e-9), dict(rtps=float("nan")), dict(rtpp=float("nan")),
                                dict(rtps=math.inf), dict(rtpp=1.0000001), dict(rtpp=2.0), dict(rtps=0.5, rtpp=0.5),
                                dict(rtps=0.0, rtpp=0.0), dict(rtps="a lot")])
def test_ensrf_rejects_bad_relaxation_before_any_device_work(kw):
    from efa_xray_amd import EnSRF
    with pytest.raises(ValueError):
        EnSRF(_state(), [], verbose=False, **kw)


def test_relaxation_entry_is_declared_bound_and_exported():
    import re
    import subprocess
    from efa_xray_amd import _lib
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "efa_hip.h")).read()
    assert re.search(r"int efa_ctx_set_relaxation\(efa_ctx \*ctx, int kind, double alpha\);", hdr)
    for name, v in (("EFA_RELAX_NONE", 0), ("EFA_RELAX_RTPP", 1), ("EFA_RELAX_RTPS", 2)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr)
        assert getattr(_lib, name[4:]) == v
    assert "efa_ctx_set_relaxation" in _lib.SIGNATURES
    lib = _lib.load_library()
    assert lib.efa_ctx_set_relaxation(None, 1, 0.5) == _lib.EFA_ERR_INVALID
    assert b"null context" in lib.efa_last_error()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert " T efa_ctx_set_relaxation" in out


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_closed_forms_on_the_oracle_posteriors(name):
    g = load_golden(name)
    X, post = golden_oracle(g)
    moved = np.abs(post - X).max(axis=1) > 0
    assert moved.any()
    b = X - X.mean(axis=1, keepdims=True)
    for alpha in (0.5, 0.9, 1.0):
        for kw in (dict(rtps=alpha), dict(rtpp=alpha)):
            r = relax(X, post, **kw)
            # the posterior mean does not move
            np.testing.assert_allclose(r.mean(axis=1), post.mean(axis=1), rtol=0, atol=1e-12 * np.abs(post).max())
    # RTPP(1): the prior perturbations about the posterior mean
    r = relax(X, post, rtpp=1.0)
    np.testing.assert_allclose(r - r.mean(axis=1, keepdims=True), b, rtol=0, atol=1e-12 * np.abs(X).max())
    # RTPS(1): the posterior spread equals the prior spread, row by row
    r = relax(X, post, rtps=1.0)
    np.testing.assert_allclose(r.std(axis=1, ddof=1), X.std(axis=1, ddof=1), rtol=1e-12, atol=1e-300)
    # alpha 0 is the identity
    assert np.array_equal(relax(X, post, rtps=0.0), post)
    # a row with no posterior spread (a state row the obs never reach is unchanged and keeps its spread)
    Z = X.copy()
    Z[0] = 1.5
    pz = post.copy()
    pz[0] = 1.5
    for kw in (dict(rtps=0.9), dict(rtpp=0.9)):
        r = relax(Z, pz, **kw)
        assert np.all(np.isfinite(r)) and np.array_equal(r[0], pz[0])
