"""The probability-matched mean, the part that needs no GPU: the NumPy model the GPU tests compare with against a
two-loop brute force, the exports and prototypes, the Python argument checks, and the registers and LDS of the new kernels."""
import os
import re

import numpy as np
import pytest

import _pmmean as pmm
from conftest import ROOT


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("patch", [None, (4, 3), (1, 1), (2, 7), (5, 1)])
def test_model_agrees_with_the_two_loop_brute_force(patch, dtype):
    n_lead, ny, nx, M = 2, 5, 7, 3
    ncol = ny * nx
    for fi, family in enumerate(pmm.FAMILIES):
        X, f = pmm.make_case(family, 10 + fi, n_lead, ny, nx, M, dtype)
        X[0, 1] = np.nan                     # a corner
        X[3 * nx, 0] = np.inf                # an edge
        X[ncol + 2 * nx + 3, 2] = -np.inf    # the interior of slab 1
        f[ncol - 1] = np.nan                 # a rank value that is not finite
        f[5], f[6] = -0.0, 0.0               # equal for the order: row 5 before row 6
        X[8, 0] = -0.0
        for g in (0, M // 2, M - 1):
            pm, n_bad = pmm.model(X, f, n_lead, ny, nx, patch, g)
            bpm, bn_bad = pmm.brute(X, f, n_lead, ny, nx, patch, g)
            assert np.array_equal(pm, bpm, equal_nan=True), (family, g)
            assert np.array_equal(np.signbit(pm), np.signbit(bpm))
            assert np.array_equal(n_bad, bn_bad) and list(n_bad) == [3, 1]
            assert np.all(np.isnan(pm[[0, 3 * nx, ncol - 1, ncol + 2 * nx + 3]])) and np.count_nonzero(np.isnan(pm)) == 4
    pm, n_bad = pmm.model(X, f, n_lead, ny, nx, patch, 1, slab_on=[0, 1])
    bpm, bn_bad = pmm.brute(X, f, n_lead, ny, nx, patch, 1, slab_on=[0, 1])
    assert np.array_equal(pm, bpm, equal_nan=True) and np.all(np.isnan(pm[:ncol])) and list(n_bad) == list(bn_bad) == [0, 1]


def test_segments_and_value_families():
    segs = pmm.segments(5, 7, 4, 3)
    assert [s.size for s in segs] == [12, 12, 4, 3, 3, 1] and list(segs[2]) == [6, 13, 20, 27] and list(segs[5]) == [34]
    assert sorted(np.concatenate(segs).tolist()) == list(range(35))
    assert len(pmm.segments(5, 7, 5, 7)) == 1 and len(pmm.segments(5, 7, 1, 1)) == 35
    for dtype, uint, nbytes in ((np.float64, np.uint64, 8), (np.float32, np.uint32, 4)):
        def key_bytes(X):
            b = (X + dtype(0.0)).view(uint).reshape(-1)
            top = uint(1) << uint(8 * nbytes - 1)
            k = np.where(b & top, ~b, b | top)
            return [np.unique((k >> uint(8 * p)) & uint(255)).size for p in range(nbytes)]
        X, _ = pmm.make_case("bits", 1, 1, 40, 40, 8, dtype)
        assert all(n == 256 for n in key_bytes(X)), key_bytes(X)         # every digit of every byte
        assert key_bytes(pmm.make_case("const", 1, 1, 5, 7, 3, dtype)[0]) == [1] * nbytes
        low = key_bytes(pmm.make_case("lowbyte", 1, 1, 33, 17, 17, dtype)[0])
        assert low[0] == 256 and low[1:] == [1] * (nbytes - 1)
        high = key_bytes(pmm.make_case("highbyte", 1, 1, 33, 17, 17, dtype)[0])
        assert high[-1] == 128 and high[:-1] == [1] * (nbytes - 1)
        X, _ = pmm.make_case("mixed", 1, 1, 33, 17, 17, dtype)
        tiny = np.finfo(dtype).tiny
        assert np.any(np.signbit(X) & (X == 0)) and np.any(~np.signbit(X) & (X == 0)) and np.any((X != 0) & (np.abs(X) < tiny))
        assert np.any(X < 0) and np.any(X > 0)
        X, _ = pmm.make_case("precip", 1, 1, 33, 17, 17, dtype)
        assert 0.6 < np.mean(X == 0) < 0.8 and np.unique(X).size < 400


def test_exports_and_prototypes():
    import efa_xray_amd
    from efa_xray_amd import _lib, postprocess
    name = "probability_matched_mean"
    assert name in efa_xray_amd.__all__ and callable(getattr(efa_xray_amd, name))
    assert name in postprocess.__all__ and getattr(postprocess, name) is getattr(efa_xray_amd, name)
    a, b = _lib.SIGNATURES["efa_pm_mean_dev"], _lib.SIGNATURES["efa_pm_mean_f32_dev"]
    assert len(a[1]) == len(b[1]) == 14 and a == b
    raw = open(os.path.join(ROOT, "include", "efa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for fn in ("efa_pm_mean_dev", "efa_pm_mean_f32_dev"):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % fn, text)
        assert proto is not None and len(proto.group(1).split(",")) == 14, fn
    for const, value in (("EFA_PM_WS_BYTES", r"\(1L << 30\)"), ("EFA_PM_TILE_KEYS", "4096"), ("EFA_PM_UNIT_BLOCKS", "32")):
        assert re.search(r"#define\s+%s\s+%s" % (const, value), text), const
    src = open(os.path.join(ROOT, "efa_xray_amd", "_lib.py")).read()
    assert src.index('"efa_pm_mean_f32_dev"') < src.index("def load_library")
    assert hasattr(_lib.Context, "pm_mean")
    assert "efa_pmmean.hip" in open(os.path.join(ROOT, "efa_xray_amd", "csrc", "Makefile")).read()
    lib = _lib.load_library()
    assert lib.efa_abi_version() == 1
    for fn in ("efa_pm_mean_dev", "efa_pm_mean_f32_dev"):
        assert hasattr(lib, fn)
        assert getattr(lib, fn)(None, 0, 0, None, 0, 0, 0, None, None, 0, 0, 0, None, None) == _lib.EFA_ERR_INVALID
        assert b"null context" in lib.efa_last_error()


def test_kernels_hold_their_keys_in_registers():
    """No kernel of the sort uses scratch.  k_pm_scatter keeps a thread's 16 keys, their places and (for the rank keys) their
    payloads in registers and stays at or below 168 of them, three waves per SIMD; its LDS is the four waves'
    counters and bases, 12 KiB, and k_pm_hist's the 256 counters."""
    from efa_xray_amd import _lib
    from _codeobj import kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    want = {
        "9k_pm_keysIdyE": (64, 3072), "9k_pm_keysIfjE": (64, 3072),
        "12k_pm_varbitsIyE": (64, 0), "12k_pm_varbitsIjE": (64, 0),
        "9k_pm_histIyE": (64, 1024), "9k_pm_histIjE": (64, 1024),
        "9k_pm_usumE": (64, 0), "12k_pm_segscanE": (64, 64),
        "12k_pm_scatterIyLb0EE": (168, 12288), "12k_pm_scatterIjLb0EE": (168, 12288), "12k_pm_scatterIyLb1EE": (168, 12288),
        "11k_pm_assignIyE": (64, 0), "11k_pm_assignIjE": (64, 0), "11k_pm_unreadE": (64, 0),
    }
    for key, (vgpr, lds) in want.items():
        hits = [k for n, k in tab.items() if key in n]
        assert len(hits) == 1, key
        k = hits[0]
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, (key, k)
        assert k.get(".sgpr_spill_count", 0) == 0, (key, k)
        assert k[".vgpr_count"] <= vgpr, (key, k[".vgpr_count"])
        assert k[".group_segment_fixed_size"] <= lds, (key, k[".group_segment_fixed_size"])
    assert len([n for n in tab if "k_pm_" in n]) == len(want)


def _state(M=4, dtype=None, nvar=2, nt=2, ny=3, nx=5):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    return EnsembleState.from_array(rng.standard_normal((nvar, nt, ny, nx, M)), lat, lon, varnames=["rain", "gust"][:nvar],
                                    dtype=dtype)


def test_argument_checks_raise_before_the_gpu_is_touched(monkeypatch):
    from efa_xray_amd import _lib, probability_matched_mean

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(_lib, "get_context", no_gpu)
    st = _state()
    bad = [
        (dict(variables=["rh"]), "no variable"),
        (dict(variables=["rain", "rain"]), "twice"),
        (dict(variables=3), "variables must be"),
        (dict(patch=(0, 1)), "patch="),
        (dict(patch=(4, 1)), "patch="),
        (dict(patch=(1, 6)), "patch="),
        (dict(patch=(1.5, 2)), "patch must be"),
        (dict(patch=(1, 2, 3)), "patch must be"),
        (dict(patch=3), "patch must be"),
        (dict(patch=("a", "b")), "patch must be"),
        (dict(pick="median"), "pick="),
        (dict(pick=4), "pick="),
        (dict(pick=-1), "pick="),
        (dict(pick=1.0), "pick="),
        (dict(pick=None), "pick="),
        (dict(pick=True), "pick="),
        (dict(rank_field=[1, 2]), "mapping"),
        (dict(rank_field={"rh": np.zeros((2, 3, 5))}), "no variable"),
        (dict(rank_field={"rain": np.zeros((2, 3, 4))}), "shape"),
        (dict(rank_field={"rain": "abc"}), "rank_field["),
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=re.escape(word)):
            probability_matched_mean(st, **kw)
    with pytest.raises(ValueError, match="members"):
        probability_matched_mean(_state(M=1))
    # no variable asked for: nothing to do, no library call
    out = probability_matched_mean(st, variables=[], patch=(2, 2), pick="max")
    assert out == {"pm_mean": {}, "rank_field": {}, "n_bad": {}, "patch": (2, 2), "pick": 3}
