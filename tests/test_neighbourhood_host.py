"""Neighbourhood probabilities and the fractions skill score, the part that needs no GPU: the NumPy model the GPU
tests compare with against a four-loop brute force, fss_from_sums against the direct formula, the exports and prototypes, the
Python argument checks, and the registers and LDS of the new kernels."""
import os
import re

import numpy as np
import pytest

import _neighbourhood as nm
from conftest import ROOT


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("shape", [0, 1])
def test_model_agrees_with_the_four_loop_brute_force(shape, wrap):
    n_lead, ny, nx, M = 2, 5, 7, 5
    X, y = nm.make_case(3 + shape, n_lead, ny, nx, M)
    X[0, 1] = np.nan                      # a corner
    X[3 * nx, 0] = np.inf                 # an edge
    X[ncol_mid(ny, nx), 2] = -np.inf      # the interior
    y[ny * nx + 9] = np.nan               # slab 1: a row that is not verified is not valid either
    thr = np.array([[280.0, 280.7, np.nan], [279.5, np.nan, np.nan]])
    radii = [0, 1, 2, 3] if wrap else [0, 1, 3, 9]      # 9 > ny, nx; with wrap 2*3+1 == nx
    for yv in (None, y):
        m = nm.model(X, n_lead, ny, nx, thr, radii, shape, wrap, y=yv, slab_group=[0, 1])
        S, n, un, osum = nm.brute(X, n_lead, ny, nx, thr, radii, shape, wrap, y=yv)
        for a, b, name in ((m["S"], S, "S"), (m["n"], n, "n"), (m["union"], un, "union"), (m["osum"], osum, "osum")):
            assert np.array_equal(a, b), (name, yv is None)
        ok = m["valid"]
        assert np.all(np.isnan(m["nep"][:, :, ~ok])) and np.all(np.isnan(m["nmep"][:, :, ~ok]))
        assert np.all(np.isnan(m["nep"][:, 2])) and np.all(np.isnan(m["nep"][:, 1, ny * nx:]))
        fin = ~np.isnan(m["nep"])
        assert np.all(m["nmep"][fin] >= m["nep"][fin]) and np.all(m["n"][:, :, ok] >= 1)
    assert not ok[0] and not ok[ny * nx + 9] and np.count_nonzero(~ok) == 4
    assert np.array_equal(m["n_bad"][:, 0, 0], [3, 0]) and m["cnt"][1, 0, 0] == ny * nx - 1 and np.all(m["cnt"][1, :, 1:] == 0)


def ncol_mid(ny, nx):
    return (ny // 2) * nx + nx // 2


def test_disc_half_widths_and_offsets():
    assert nm.half_widths(0, 1) == [0] and nm.half_widths(1, 1) == [1, 0] and nm.half_widths(2, 1) == [2, 1, 0]
    assert nm.half_widths(5, 1) == [5, 4, 4, 4, 3, 0] and nm.half_widths(5, 0) == [5] * 6
    assert len(nm.offsets(5, 1)) == 81 and len(nm.offsets(5, 0)) == 121
    for r in (0, 3, 10, 64):
        assert set(nm.offsets(r, 1)) == set((dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r)


def test_fss_from_sums_agrees_with_the_direct_formula():
    from efa_xray_amd import fss_from_sums
    rng = np.random.default_rng(5)
    P, O, w = rng.random(200), rng.random(200), rng.random(200) + 0.1
    sums = np.array([w.sum(), (w * (P - O) ** 2).sum(), (w * P * P).sum(), (w * O * O).sum(), (w * P).sum(), (w * O).sum()])
    sc = fss_from_sums(sums)
    direct = 1.0 - np.sum(w * (P - O) ** 2) / (np.sum(w * P ** 2) + np.sum(w * O ** 2))
    assert abs(sc["fss"] - direct) <= 1e-14 and 0.0 < sc["fss"] < 1.0
    f, mse, base, frate = nm.fss(sums)
    assert sc["fss"] == f and sc["mse"] == mse and sc["base_rate"] == base and sc["forecast_rate"] == frate
    assert sc["fss_useful"] == 0.5 + base / 2.0
    assert fss_from_sums([3.0, 0.0, 3.0, 3.0, 3.0, 3.0])["fss"] == 1.0           # P == O == 1 everywhere
    assert fss_from_sums([3.0, 2.0, 1.0, 1.0, 1.0, 1.0])["fss"] == 0.0           # disjoint events
    none = fss_from_sums([3.0, 0.0, 0.0, 0.0, 0.0, 0.0])                          # no event forecast or observed
    assert np.isnan(none["fss"]) and none["mse"] == 0.0 and none["base_rate"] == 0.0 and none["fss_useful"] == 0.5
    assert all(np.isnan(v) for v in fss_from_sums(np.zeros(6)).values())


def test_exports_and_prototypes():
    import efa_xray_amd
    from efa_xray_amd import _lib, postprocess
    for name in ("neighbourhood_probabilities", "fractions_skill_score", "fss_from_sums"):
        assert name in efa_xray_amd.__all__ and callable(getattr(efa_xray_amd, name))
        assert name in postprocess.__all__ and getattr(postprocess, name) is getattr(efa_xray_amd, name)
    a, b = _lib.SIGNATURES["efa_neighbourhood_dev"], _lib.SIGNATURES["efa_neighbourhood_f32_dev"]
    assert len(a[1]) == len(b[1]) == 21
    raw = open(os.path.join(ROOT, "include", "efa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ("efa_neighbourhood_dev", "efa_neighbourhood_f32_dev"):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert proto is not None and len(proto.group(1).split(",")) == 21, name
    for const, value in (("EFA_NBR_MAX_RADII", "4"), ("EFA_NBR_MAX_RADIUS", "64"), ("EFA_NBR_WS_BYTES", r"\(256L << 20\)")):
        assert re.search(r"#define\s+%s\s+%s" % (const, value), text), const
    src = open(os.path.join(ROOT, "efa_xray_amd", "_lib.py")).read()
    assert src.index('"efa_neighbourhood_f32_dev"') < src.index("def load_library")
    assert hasattr(_lib.Context, "neighbourhood")
    assert "efa_neighbourhood.hip" in open(os.path.join(ROOT, "efa_xray_amd", "csrc", "Makefile")).read()
    lib = _lib.load_library()
    assert lib.efa_abi_version() == 1
    for name in ("efa_neighbourhood_dev", "efa_neighbourhood_f32_dev"):
        assert hasattr(lib, name)
        assert getattr(lib, name)(*([None, 0, 0, None, 0, 0, 0, 0, None, 0, None, 0, 0] + [None] * 8)) == _lib.EFA_ERR_INVALID
        assert b"null context" in lib.efa_last_error()


def test_kernels_hold_their_rows_in_registers_and_their_tiles_in_lds():
    """k_nbr_records up to NU = 16 (128 members) runs without scratch, with and without the masks, for both element types.
    k_nbr_windows never spills; its LDS leaves room for the occupancy DESIGN.md 7r states: two workgroups per CU (160 KiB) up to a
    halo of 32, one at the largest radius."""
    from efa_xray_amd import _lib
    from _codeobj import kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    seen = 0
    for nu in (1, 2, 4, 8, 16, 32):
        for e in "df":
            for msk in (0, 1):
                hits = [k for n, k in tab.items() if "13k_nbr_recordsILi%dE%sLb%dE" % (nu, e, msk) in n]
                assert len(hits) == 1, (nu, e, msk)
                k = hits[0]
                seen += 1
                if nu <= 16:
                    assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, (k[".name"], k)
                    assert k[".vgpr_count"] <= 256, (k[".name"], k[".vgpr_count"])
    assert seen == 24
    lds = {}
    for halo in (8, 32, 64):
        hits = [k for n, k in tab.items() if "13k_nbr_windowsILi%dEE" % halo in n]
        assert len(hits) == 1, halo
        k = hits[0]
        assert k.get(".vgpr_spill_count", 0) == 0 and k[".private_segment_fixed_size"] == 0, (halo, k)
        assert k[".vgpr_count"] <= 168, (halo, k[".vgpr_count"])          # three waves per SIMD: three workgroups per CU
        lds[halo] = k[".group_segment_fixed_size"]
    assert lds[8] <= 16 * 1024 and lds[32] <= 80 * 1024 and lds[64] <= 160 * 1024, lds
    assert lds[64] >= (16 + 128) * (64 + 128) * 4                          # the tile and a 64-point halo do sit in LDS


# .vgpr_count of k_nbr_records<NU, E, MASK> before the row layout's helpers moved to efa_quadrow.h, (float64, float32) per (NU, MASK);
# every instantiation was free of scratch and spills
VGPRS_BEFORE = {(1, 0): (33, 33), (1, 1): (38, 38), (2, 0): (42, 39), (2, 1): (46, 46), (4, 0): (54, 55), (4, 1): (61, 61),
                (8, 0): (79, 75), (8, 1): (87, 86), (16, 0): (129, 146), (16, 1): (132, 132), (32, 0): (221, 221), (32, 1): (229, 229)}


def test_records_kernels_keep_their_occupancy_step():
    """No k_nbr_records instantiation falls to a lower occupancy step than it had with its private copy of the row layout, and
    none has scratch or spills."""
    from efa_xray_amd import _lib
    from _codeobj import assert_no_worse_than, kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    for (nu, msk), before in VGPRS_BEFORE.items():
        for e, v in zip("df", before):
            (k,) = [k for n, k in tab.items() if "13k_nbr_recordsILi%dE%sLb%dE" % (nu, e, msk) in n]
            assert_no_worse_than(k, v)


def _state(M=4, dtype=None, nvar=2, nt=2, ny=3, nx=5):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    return EnsembleState.from_array(rng.standard_normal((nvar, nt, ny, nx, M)), lat, lon, varnames=["t2m", "psfc"][:nvar],
                                    dtype=dtype)


def test_argument_checks_raise_before_the_gpu_is_touched(monkeypatch):
    from efa_xray_amd import _lib, neighbourhood_probabilities, fractions_skill_score

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(_lib, "get_context", no_gpu)
    st = _state()
    good_t, good_v = {"t2m": [0.0]}, {"t2m": np.zeros((2, 3, 5))}
    bad_windows = [
        (dict(radii=[1.5]), "radii must be integers"),
        (dict(radii=[-1]), "radii must be integers"),
        (dict(radii=[65]), "radii must be integers"),
        (dict(radii=[np.nan]), "radii must be integers"),
        (dict(radii=["a"]), "radii must be integers"),
        (dict(radii=[0, 1, 2, 3, 4]), "1 to 4"),
        (dict(radii=[]), "1 to 4"),
        (dict(radii=[[1, 2]]), "1 to 4"),
        (dict(shape="circle"), "shape="),
        (dict(shape=0), "shape="),
        (dict(radii=[3], wrap_x=True), "wrap_x=True needs"),
    ]
    for kw, word in bad_windows:
        for fn, args in ((neighbourhood_probabilities, (good_t,)), (fractions_skill_score, (good_v, good_t))):
            a = dict(radii=[1])
            a.update(kw)
            with pytest.raises(ValueError, match=re.escape(word)):
                fn(st, *args, **a)
    bad_common = [
        (dict(thresholds=[1.0]), "mapping"),
        (dict(thresholds=None), "mapping"),
        (dict(thresholds={"rh": [1.0]}), "no variable"),
        (dict(thresholds={"t2m": list(range(9))}), "at most 8"),
        (dict(thresholds={"t2m": [np.inf]}), "not finite"),
    ]
    for kw, word in bad_common:
        with pytest.raises(ValueError, match=re.escape(word)):
            neighbourhood_probabilities(st, kw["thresholds"], [1])
        with pytest.raises(ValueError, match=re.escape(word)):
            fractions_skill_score(st, good_v, kw["thresholds"], [1])
    bad_verif = [
        (dict(verification=[1, 2]), "mapping"),
        (dict(verification={"rh": np.zeros((2, 3, 5))}), "no variable"),
        (dict(verification={"t2m": np.zeros((2, 3, 4))}), "shape"),
        (dict(verification={"t2m": np.full((2, 3, 5), np.inf)}), "infinite"),
        (dict(by="time"), "by="),
        (dict(weights=np.ones((3, 4))), "weights has shape"),
        (dict(weights=-np.ones((3, 5))), "finite and >= 0"),
    ]
    for kw, word in bad_verif:
        args = dict(verification=good_v, thresholds=good_t, radii=[1])
        args.update(kw)
        with pytest.raises(ValueError, match=re.escape(word)):
            fractions_skill_score(st, **args)
    with pytest.raises(ValueError, match="neither"):
        neighbourhood_probabilities(st, good_t, [1], nep=False, nmep=False)
    with pytest.raises(ValueError, match="members"):
        neighbourhood_probabilities(_state(M=1), good_t, [1])
    # wrap_x with 2r+1 == nx is allowed (and a scalar radius is one radius); no threshold at all: nothing to do, no library call
    out = neighbourhood_probabilities(st, {}, 2, wrap_x=True, nmep=True)
    assert out["nep"] == {} and out["nmep"] == {} and list(out["radii"]) == [2]
    out = fractions_skill_score(st, good_v, {}, [0, 1])
    assert out["fss"].shape == (2, 2, 0) and out["n"].shape == (2, 2, 0) and out["groups"] == ["t2m", "psfc"]
