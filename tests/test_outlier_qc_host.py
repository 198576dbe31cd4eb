"""Outlier check without a GPU: known answers of the mask helper, EnSRF / ShardedEnSRF argument checks and the
C ABI entry (declared, bound, exported, refuses a null context first)."""
import math

import numpy as np
import pytest

import _outlier as qc


def _block(ratios, M=8, seed=0, error=None):
    """ym, Yp, value, error with |value - ym| / sqrt(var(Yp) + error) equal to `ratios` (signs alternate)."""
    rng = np.random.default_rng(seed)
    P = len(ratios)
    HX = rng.standard_normal((P, M)) * rng.uniform(0.5, 2.0, (P, 1)) + rng.standard_normal((P, 1))
    ym = HX.mean(axis=1)
    Yp = HX - ym[:, None]
    err = rng.uniform(0.2, 1.5, P) if error is None else np.asarray(error, dtype=float)
    sign = np.where(np.arange(P) % 2 == 0, 1.0, -1.0)
    value = ym + sign * np.asarray(ratios, dtype=float) * np.sqrt(np.var(Yp, axis=1) + err)
    return ym, Yp, value, err


def test_mask_known_answers_around_the_threshold():
    t = 3.0
    ratios = [0.5 * t, (1 - 1e-6) * t, (1 + 1e-6) * t, 10 * t, 0.0]
    ym, Yp, value, err = _block(ratios)
    assim = np.ones(len(ratios), dtype=bool)
    got = qc.outlier_mask(ym, Yp, value, err, assim, t)
    assert got.tolist() == [False, False, True, True, False]
    assert np.allclose(qc.ratio(ym, Yp, value, err), ratios, rtol=1e-12, atol=1e-15)
    assert qc.clear_of_threshold(ym, Yp, value, err, t, rel=5e-7)
    assert not qc.clear_of_threshold(ym, Yp, value, err, t, rel=2e-6)


def test_mask_uses_ddof_0_and_the_error_variance():
    # Yp row of +-1: var 1 (ddof 0; ddof 1 would give 8/7); error 3: s2 + r = 4, so |d| <= 2 t is kept
    M = 8
    Yp = np.tile(np.array([1.0, -1.0] * (M // 2)), (3, 1))
    ym = np.zeros(3)
    err = np.full(3, 3.0)
    t = 1.5
    value = np.array([2 * t, 2 * t * (1 + 1e-9), -2 * t * (1 - 1e-9)])
    assert qc.outlier_mask(ym, Yp, value, err, np.ones(3, bool), t).tolist() == [False, True, False]


def test_nan_rejects_and_unrequested_obs_are_never_rejected():
    t = 2.0
    ym, Yp, value, err = _block([0.1, 0.1, 0.1, 50.0, 50.0, 0.1])
    value[0] = np.nan
    Yp[1, 3] = np.nan
    err[2] = np.nan
    assim = np.array([1, 1, 1, 1, 0, 0], dtype=bool)
    value[5] = np.nan
    got = qc.outlier_mask(ym, Yp, value, err, assim, t)
    assert got.tolist() == [True, True, True, True, False, False]


def test_inject_moves_requested_obs_to_the_intended_ratio():
    rng = np.random.default_rng(3)
    HX = rng.standard_normal((40, 10))
    err = rng.uniform(0.5, 1.5, 40)
    assim = rng.random(40) < 0.8
    value = HX.mean(axis=1) + 0.1 * rng.standard_normal(40)
    v2, idx = qc.inject(HX, value, err, assim, 3.0, 5, seed=1)
    assert len(idx) == 5 and np.all(assim[idx])
    from oracle import ensrf_oracle as orc
    ym, Yp = orc.compute_ob_priors(HX)
    assert np.allclose(qc.ratio(ym, Yp, v2, err)[idx], 8.0, rtol=1e-12)
    flags = qc.masked_flags(HX, v2, err, assim, 3.0)
    assert not flags[idx].any() and np.array_equal(flags | ~assim, ~np.isin(np.arange(40), idx) | ~assim)


def _state():
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(20, 40, 3), np.linspace(250, 270, 4), indexing="ij")
    return EnsembleState.from_array(rng.standard_normal((1, 2, 3, 4, 6)), lat, lon)


def test_ensrf_accepts_the_threshold_and_its_combinations():
    from efa_xray_amd import AdaptiveInflation, EnSRF
    st = _state()
    assert EnSRF(st, [], verbose=False).outlier_threshold is None
    assert EnSRF(st, [], verbose=False, outlier_threshold=None).outlier_threshold is None
    assert EnSRF(st, [], verbose=False, outlier_threshold=3).outlier_threshold == 3.0
    assert EnSRF(st, [], verbose=False, outlier_threshold=np.float32(2.5)).outlier_threshold == 2.5
    assert EnSRF(st, [], verbose=False, outlier_threshold=1e6).outlier_threshold == 1e6
    for kw in (dict(inflation=1.1), dict(rtps=0.9), dict(rtpp=0.5), dict(loc="GC", vert_coord=np.zeros((1, 2))),
               dict(loc="GC", adaptive_inflation=AdaptiveInflation(st, ("spatial", None, (1.0, 0.6))))):
        e = EnSRF(st, [], verbose=False, outlier_threshold=4.0, **kw)
        assert e.outlier_threshold == 4.0, kw


@pytest.mark.parametrize("t", [0, 0.0, -1.0, -1e-300, float("nan"), math.inf, -math.inf, "3", True, [3.0], 1j])
def test_ensrf_rejects_a_bad_threshold_at_construction(t):
    from efa_xray_amd import EnSRF
    with pytest.raises(ValueError):
        EnSRF(_state(), [], verbose=False, outlier_threshold=t)


def test_sharded_update_refuses_a_bad_threshold_before_any_work():
    from efa_xray_amd.assimilation.ensrf import outlier_setting
    from efa_xray_amd.distributed import ShardedEnSRF

    class NoEngine(object):
        def __getattr__(self, name):
            raise AssertionError("engine used before the threshold was checked: %s" % name)

    sh = ShardedEnSRF.__new__(ShardedEnSRF)
    sh.engine = NoEngine()
    with pytest.raises(ValueError):
        sh.update(None, None, np.zeros((2, 1), dtype=np.int64), np.ones((2, 1)), dict(value=np.zeros(2)), outlier_threshold=-2.0)
    assert outlier_setting(None) is None and outlier_setting(2) == 2.0


def test_outlier_entry_is_declared_bound_and_exported():
    import re
    import subprocess
    from efa_xray_amd import _lib
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "efa_hip.h")).read()
    assert re.search(r"int efa_ctx_set_outlier_threshold\(efa_ctx \*ctx, double threshold\);", hdr)
    assert "efa_ctx_set_outlier_threshold" in _lib.SIGNATURES
    assert _lib.SIGNATURES["efa_ctx_set_outlier_threshold"][1][1] is _lib.ctypes.c_double
    lib = _lib.load_library()
    for t in (0.0, 3.0, -1.0, float("nan")):  # the null context is refused before the value is looked at
        assert lib.efa_ctx_set_outlier_threshold(None, t) == _lib.EFA_ERR_INVALID
        assert b"null context" in lib.efa_last_error()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert " T efa_ctx_set_outlier_threshold" in out
