"""The LETKF's cap on the local observations of a solve without a device: the NumPy model of tests/_letkf_cap.py
(counts, tie rule, gap assertion, identity), the seeded cases' condition on their inputs, the front end's refusals, the symbol's
three declarations, and the scratch of k_letkf_cap."""
import os
import re

import numpy as np
import pytest

import _letkf as lk
import _letkf_cap as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _the_feature_exists():
    """The model below describes efa_ctx_set_letkf_obs_cap: without the entry point there is nothing for it to describe."""
    from efa_xray_amd import _lib
    assert "efa_ctx_set_letkf_obs_cap" in _lib.SIGNATURES, "the library has no cap on the local observations"


# ---- 1. select ------------------------------------------------------------------------------------------------------------------------
def test_select_keeps_the_largest_tapers_per_class():
    rng = np.random.default_rng(5)
    rho = rng.random((7, 40))
    rho[rng.random((7, 40)) < 0.3] = 0.0
    cls = np.arange(40) % 3
    caps = (4, 0, 6)
    info = {}
    out = cp.select(rho, cls, caps, info=info)
    assert np.array_equal(info["reach"], np.stack([((rho != 0) & (cls == c)).sum(axis=1) for c in range(3)], axis=1))
    assert np.array_equal((out != 0).sum(axis=1), cp.n_local(info["reach"], caps))
    assert np.all((out == rho) | (out == 0.0))
    for i in range(7):
        for c, cap in enumerate(caps):
            m = cls == c
            kept, lost = out[i, m][out[i, m] != 0], rho[i, m][(out[i, m] == 0) & (rho[i, m] != 0)]
            if cap == 0:
                assert lost.size == 0
            elif lost.size:
                assert kept.size == cap and kept.min() > lost.max()
    assert info["bites"].all() and info["gap"] >= cp.MIN_GAP


def test_select_orders_equal_tapers_by_lower_index_first():
    rho = np.array([[0.5, 0.7, 0.5, 0.0, 0.5, 0.9, 0.5]])
    for cap, want in ((1, [5]), (2, [1, 5]), (3, [0, 1, 5]), (4, [0, 1, 2, 5]), (5, [0, 1, 2, 4, 5]), (6, [0, 1, 2, 4, 5, 6]),
                      (7, [0, 1, 2, 4, 5, 6])):
        assert list(np.flatnonzero(cp.select(rho, None, (cap,))[0])) == want
    assert list(np.flatnonzero(cp.select(rho, None, (3,), last_first=True)[0])) == [1, 5, 6]
    # a flag of 0 is a taper of 0 (tests/_letkf.py's taper): the ob takes no place
    off = rho.copy()
    off[0, 0] = 0.0
    assert list(np.flatnonzero(cp.select(off, None, (3,))[0])) == [1, 2, 5]


def test_select_refuses_a_near_tie_at_the_cap():
    rho = np.array([[0.9, 0.5 + 1e-10, 0.5, 0.1]])
    with pytest.raises(AssertionError, match="near-tie"):
        cp.select(rho, None, (2,))
    assert list(np.flatnonzero(cp.select(rho, None, (1,))[0])) == [0]           # the near-tie is not at the cap
    assert list(np.flatnonzero(cp.select(rho, None, (3,))[0])) == [0, 1, 2]
    with pytest.raises(AssertionError):
        cp.select(rho, np.array([0, 0, 0, 5]), (2,))                            # a class outside the range


@pytest.mark.parametrize("shape", [(3, 5, 3, 5, 2), (16, 64, 5, 7, 3)])
def test_a_cap_at_or_above_the_reach_is_the_identity(shape):
    c = lk.make_case(*shape)
    rho = lk.taper(c["grid_lat"], c["grid_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"])
    reach = int((rho != 0).sum(axis=1).max())
    info = {}
    assert np.array_equal(cp.select(rho, None, (reach,), info=info), rho) and not info["bites"].any()
    assert np.array_equal(cp.select(rho, None, (c["P"],)), rho)
    assert np.array_equal(cp.select(rho, np.arange(c["P"]) % 3, (c["P"], 0, c["P"])), rho)
    assert not np.array_equal(cp.select(rho, None, (reach - 1,)), rho)
    plain = lk.letkf_cycle(c["X"], c["HX"], c["value"], c["error"], c["assim"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["grid_lat"],
                           c["grid_lon"], c["n_lead"])
    ref = cp.letkf_cycle(c, None, (c["P"],))
    for k in ("post", "ym", "Yp", "T", "w"):
        assert np.array_equal(plain[k], ref[k])
    assert lk.taper.__module__ == "_letkf", "capped() left its taper behind"


# ---- 2. the seeded cases hold the condition on their inputs, and the cap bites where DESIGN.md 7y-8 says ----------------------------
@pytest.mark.parametrize("shape,caps,hw", cp.CASES)
def test_the_seeded_cases_have_no_near_tie_at_the_cap(shape, caps, hw):
    c, ob_class = cp.make_case(shape, caps, hw)
    info_g, info_o = {}, {}
    rho = lk.taper(c["grid_lat"], c["grid_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"])
    rho_o = lk.taper(c["ob_lat"], c["ob_lon"], c["ob_lat"], c["ob_lon"], c["ob_hw"], c["assim"])
    cp.select(rho, ob_class, caps, info=info_g)
    cp.select(rho_o, ob_class, caps, info=info_o)
    print("%r caps %r: smallest gap grid %.2g / obs %.2g, bites at %d of %d columns and %d of %d ob positions"
          % (shape, caps, info_g["gap"], info_o["gap"], info_g["bites"].sum(), c["ncol"], info_o["bites"].sum(), c["P"]))
    assert min(info_g["gap"], info_o["gap"]) >= 5e-8
    if hw is not None:
        assert (info_g["bites"].sum(), info_o["bites"].sum()) == (73, 79)
    else:
        assert info_g["bites"].any() and info_o["bites"].any()


# ---- 3. the front end without a device ------------------------------------------------------------------------------------------------
def _tiny(M=6):
    from efa_xray_amd import EnsembleState, Observation
    rng = np.random.default_rng(3)
    lat, lon = np.meshgrid(np.linspace(20, 60, 4), np.linspace(200, 280, 5), indexing="ij")
    state = EnsembleState.from_array(rng.standard_normal((1, 1, 4, 5, M)), lat, lon)
    obs = [Observation(value=0.5, error=1.0, lat=40.0, lon=240.0, localize_radius=1000.0)]
    return state, obs


def test_the_keyword_is_validated_before_any_device_work(monkeypatch):
    from efa_xray_amd import LETKF, SlabLETKF, EnSRF, ETKF
    from efa_xray_amd.assimilation.assimilation import Assimilation

    def no_device(self):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(Assimilation, "_context", no_device)
    state, obs = _tiny()
    for cls in (LETKF, SlabLETKF):
        assert cls(state, obs, verbose=False).max_local_obs is None
        assert cls(state, obs, verbose=False, max_local_obs=5).max_local_obs == (None, (5,))
        assert cls(state, obs, verbose=False, max_local_obs=np.int64(1)).max_local_obs == (None, (1,))
        f = cls(state, obs, verbose=False, max_local_obs={"t2m": 3, "radar": 7}, weight_stride=2)
        assert f.max_local_obs == (["t2m", "radar"], (3, 7))
        for bad in (0, -1, True, False, 2.0, 2.5, "3", [3], (3,), {}, {"t2m": 0}, {"t2m": True}, {"t2m": 1.0}, {"t2m": None},
                    np.float64(2.0), float("nan")):
            with pytest.raises(ValueError, match="max_local_obs"):
                cls(state, obs, verbose=False, max_local_obs=bad)
        assert cls(state, obs, verbose=False, max_local_obs={"v%d" % i: 1 for i in range(31)}).max_local_obs[1] == (1,) * 31
        with pytest.raises(ValueError, match="more than 31"):
            cls(state, obs, verbose=False, max_local_obs={"v%d" % i: 1 for i in range(32)})
    for kw in (dict(vert_coord=np.zeros(1)), dict(time_localize=True), dict(var_impact={"var0": {"var0": 1.0}})):
        with pytest.raises(ValueError, match="a cap per group is the follow-up"):
            SlabLETKF(state, obs, verbose=False, max_local_obs=4, **kw)
        with pytest.raises(ValueError):
            LETKF(state, obs, verbose=False, max_local_obs=4, **kw)
    for cls, kw in ((EnSRF, dict(loc="GC")), (ETKF, {})):
        with pytest.raises((TypeError, ValueError)):
            cls(state, obs, verbose=False, max_local_obs=4, **kw)


def test_the_classes_of_the_dict_form():
    from efa_xray_amd import Observation
    from efa_xray_amd.assimilation import letkf
    obs = [Observation(value=0.0, obtype=t, error=1.0, lat=0.0, lon=0.0) for t in ("a", "b", "a", "c", None, "b")]
    assert letkf._cap_classes((None, (7,)), obs) == (None, [7])
    cls, caps = letkf._cap_classes((["b", "zz", "a"], (2, 9, 5)), obs)        # "zz": no ob has it; "c", None: not named
    assert list(cls) == [1, 0, 1, 2, 2, 0] and caps == [2, 5, 0] and cls.dtype == np.int32
    cls, caps = letkf._cap_classes((["zz"], (1,)), obs)
    assert list(cls) == [0] * 6 and caps == [0]


# ---- 4. the symbol: declared, bound, exported ---------------------------------------------------------------------------------------
def test_the_symbol_is_declared_bound_and_exported():
    from efa_xray_amd import _lib
    header = open(os.path.join(ROOT, "include", "efa_hip.h")).read()
    m = re.search(r"int\s+efa_ctx_set_letkf_obs_cap\s*\(([^;]*)\)\s*;", header)
    assert m, "include/efa_hip.h does not declare efa_ctx_set_letkf_obs_cap"
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == 7
    restype, argtypes = _lib.SIGNATURES["efa_ctx_set_letkf_obs_cap"]
    assert len(argtypes) == 7
    lib = _lib.load_library()
    assert lib.efa_ctx_set_letkf_obs_cap.argtypes == argtypes
    assert hasattr(_lib.Context, "set_letkf_obs_cap")


# ---- 5. k_letkf_cap uses no scratch ------------------------------------------------------------------------------------------------
def test_k_letkf_cap_uses_no_scratch():
    import _codeobj
    from efa_xray_amd import _lib
    table = _codeobj.kernel_table(_lib.LIB_PATH)
    ks = {n: k for n, k in table.items() if "k_letkf_cap" in n}
    assert len(ks) == 1, "one k_letkf_cap, not a template: %r" % sorted(ks)
    for n, k in ks.items():
        print(n, "vgpr", k[".vgpr_count"], "sgpr", k[".sgpr_count"], "lds", k[".group_segment_fixed_size"], "scratch",
              k[".private_segment_fixed_size"])
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0
        assert k[".group_segment_fixed_size"] <= 24 * 1024, "six workgroups of k_letkf_cap no longer fit a CU's LDS"
