"""Host-side tests of float32 state storage: the two C symbols, the `dtype=` plumbing of `EnsembleState`, the chunk
planners with a 4-byte item and every combination that is refused.  No GPU."""
import os
import re
import subprocess
from collections import OrderedDict
from copy import deepcopy

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("efa_state_cycle_f32_dev", "efa_ensrf_cycle_host_f32")


def _state(dtype=None, M=6, seed=0):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(seed)
    lat, lon = np.meshgrid(np.linspace(30, 40, 3), np.linspace(250, 260, 4), indexing="ij")
    arr = rng.standard_normal((2, 2, 3, 4, M))
    return EnsembleState.from_array(arr, lat, lon, validtime=np.array([0.0, 3600.0]), dtype=dtype), arr


def test_new_symbols_are_declared_bound_and_exported():
    from efa_xray_amd import _lib
    header = open(os.path.join(ROOT, "include", "efa_hip.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name + " is not declared in efa_hip.h"
        assert name in _lib.SIGNATURES, name + " has no ctypes prototype"
        assert re.search(r" T %s\b" % name, out), name + " is not exported"
        assert hasattr(_lib.load_library(), name)
    assert "EFA_ABI_VERSION 1" in header
    # float32 segments, float64 obs block
    assert re.search(r"efa_ensrf_cycle_host_f32\([^;]*const float \*const \*seg_prior,\s*float \*const \*seg_post[^;]*const double \*HX", header)
    assert re.search(r"efa_state_cycle_f32_dev\([^;]*const float \*X_dev,\s*float \*post_dev", header)
    assert len(_lib.SIGNATURES["efa_ensrf_cycle_host_f32"][1]) == len(_lib.SIGNATURES["efa_ensrf_cycle_host"][1])
    assert len(_lib.SIGNATURES["efa_state_cycle_f32_dev"][1]) == len(_lib.SIGNATURES["efa_state_cycle_dev"][1])


def test_default_dtype_is_still_float64():
    from efa_xray_amd import EnsembleState
    st, arr = _state()
    assert st.dtype == np.float64
    assert all(v.dtype == np.float64 for v in st.variables.values())
    # float32 input without the keyword is cast to float64, as it always was
    lat, lon = st.coords["lat"], st.coords["lon"]
    st2 = EnsembleState.from_array(arr.astype(np.float32), lat, lon)
    assert st2.dtype == np.float64
    assert np.array_equal(st2.to_vect(), arr.astype(np.float32).astype(np.float64).reshape(-1, arr.shape[-1]))
    vd = OrderedDict(a=(("validtime", "y", "x", "mem"), arr[0].astype(np.float32)))
    assert EnsembleState.from_vardict(vd, dict(lat=lat, lon=lon)).dtype == np.float64
    assert EnsembleState.from_vardict(vd, dict(lat=lat, lon=lon), dtype=None).dtype == np.float64
    assert EnsembleState.from_vardict(vd, dict(lat=lat, lon=lon), dtype=np.float64).dtype == np.float64


def test_float32_is_kept_through_the_state_methods(tmp_path):
    from efa_xray_amd import EnsembleState
    st, arr = _state(np.float32)
    a32 = arr.astype(np.float32)
    assert st.dtype == np.float32
    assert all(v.dtype == np.float32 and v.flags["C_CONTIGUOUS"] for v in st.variables.values())
    assert st.to_vect().dtype == np.float32
    assert np.array_equal(st.to_vect(), a32.reshape(-1, a32.shape[-1]))
    # from_vardict with permuted dims
    vd = OrderedDict(a=(("mem", "validtime", "y", "x"), np.moveaxis(arr[0], -1, 0)))
    sv = EnsembleState.from_vardict(vd, dict(lat=st.coords["lat"], lon=st.coords["lon"]), dtype=np.float32)
    assert sv.dtype == np.float32 and np.array_equal(sv.variables["a"], a32[0])
    # astype both ways: copies, the original untouched
    s64 = st.astype(np.float64)
    assert s64.dtype == np.float64 and st.dtype == np.float32 and s64 is not st
    assert np.array_equal(s64.to_vect(), a32.astype(np.float64).reshape(-1, a32.shape[-1]))
    back = s64.astype(np.float32)
    assert back.dtype == np.float32 and np.array_equal(back.to_vect(), st.to_vect())
    assert st.astype(None).dtype == np.float64
    back.variables["var0"][...] = 0
    assert np.array_equal(st.to_vect(), a32.reshape(-1, a32.shape[-1]))
    # from_vect rounds what it is given to the state's dtype
    c = deepcopy(st)
    assert c.dtype == np.float32 and np.array_equal(c.to_vect(), st.to_vect())
    v = st.to_vect().astype(np.float64) * (1.0 + 2.0 ** -30)
    c.from_vect(v)
    assert c.dtype == np.float32 and np.array_equal(c.to_vect(), v.astype(np.float32))
    assert st.ensemble_perts().dtype == np.float32
    # netCDF round trip: an 'f' variable on disk, float32 back when asked for, float64 by default
    fn = str(tmp_path / "s32.nc")
    st.save_to_disk(fn)
    try:
        import xarray  # noqa: F401
    except ImportError:
        from scipy.io import netcdf_file
        with netcdf_file(fn, "r", mmap=False) as f:
            assert f.variables["var0"].typecode() == "f"
    r32 = EnsembleState.from_netcdf(fn, dtype=np.float32)
    assert r32.dtype == np.float32 and np.array_equal(r32.to_vect(), st.to_vect())
    r64 = EnsembleState.from_netcdf(fn)
    assert r64.dtype == np.float64 and np.array_equal(r64.to_vect(), st.to_vect().astype(np.float64))
    # the host gather of the forward operator widens
    rows = np.array([0, 5, 17])
    g = st.gather_rows(rows, np.array([0.25, 0.5, 0.25]))
    assert g.dtype == np.float64
    assert np.array_equal(g, s64.gather_rows(rows, np.array([0.25, 0.5, 0.25])))


def test_bad_and_mixed_dtypes_are_rejected():
    from efa_xray_amd import EnsembleState, EnSRF, Observation
    st, arr = _state()
    lat, lon = st.coords["lat"], st.coords["lon"]
    for bad in (np.float16, np.int32, "int64", complex, "no-such-type"):
        with pytest.raises(ValueError):
            EnsembleState.from_array(arr, lat, lon, dtype=bad)
        with pytest.raises(ValueError):
            st.astype(bad)
    mixed = EnsembleState(OrderedDict(a=arr[0].astype(np.float32), b=arr[1].copy()), dict(lat=lat, lon=lon))
    with pytest.raises(ValueError, match="mix"):
        mixed.dtype
    ob = Observation(value=1.0, error=1.0, lat=35.0, lon=255.0, assimilate_this=True)
    ob.estimate = lambda s: s.to_vect()[0]
    with pytest.raises(ValueError, match="mix"):
        EnSRF(mixed, [ob], verbose=False).update()


def test_inflation_scales_in_float64_and_rounds_once():
    from efa_xray_amd import EnSRF
    st, arr = _state(np.float32, seed=3)
    s64 = st.astype(np.float64)
    f32 = EnSRF(st, [], verbose=False, inflation=1.1)
    f64 = EnSRF(s64, [], verbose=False, inflation=1.1)
    f32.inflate_state()
    f64.inflate_state()
    assert st.dtype == np.float32                      # in place, still float32
    assert np.array_equal(st.to_vect(), s64.to_vect().astype(np.float32))
    # per-dimension factors rebind the prior: float32 kept there too
    st2, _ = _state(np.float32, seed=4)
    g32 = EnSRF(st2, [], verbose=False, inflation={"y": np.array([1.0, 1.2, 1.4])})
    g64 = EnSRF(st2.astype(np.float64), [], verbose=False, inflation={"y": np.array([1.0, 1.2, 1.4])})
    g32.inflate_state()
    g64.inflate_state()
    assert g32.prior.dtype == np.float32
    assert np.array_equal(g32.prior.to_vect(), g64.prior.to_vect().astype(np.float32))


def test_chunk_planners_take_the_item_size():
    from efa_xray_amd import _lib
    assert _lib.default_chunk_cols(6, 50) == _lib.default_chunk_cols(6, 50, itemsize=8)
    for n_lead, M in ((6, 50), (64, 80), (1, 2), (3, 137)):
        c8, c4 = _lib.default_chunk_cols(n_lead, M), _lib.default_chunk_cols(n_lead, M, itemsize=4)
        assert c4 % 16 == 0 and c4 >= 16
        assert c4 == max(16, (64 << 20) // (n_lead * M * 4) // 16 * 16)
        assert c8 <= c4 <= 2 * c8 + 16               # about twice the columns in the same bytes
    assert _lib.default_chunk_cols(10 ** 6, 256, itemsize=4) == 16
    assert _lib.default_chunk_cols(4, 10, target_bytes=4 * 10 * 4 * 48, itemsize=4) == 48
    # the cuts are in columns: the same for either item size
    for ncol, cc in ((117, 16), (117, 48), (117, 1000), (5, 16), (0, 16), (160, 33)):
        assert _lib.plan_chunks(ncol, cc, itemsize=4) == _lib.plan_chunks(ncol, cc)
        plan = _lib.plan_chunks(ncol, cc, 4)
        assert [lo for lo, _ in plan] == list(range(0, ncol, max(16, cc // 16 * 16)))
        assert not plan or plan[-1][1] == ncol
    for bad in (2, 16, 0):
        with pytest.raises(ValueError):
            _lib.plan_chunks(100, 16, itemsize=bad)
        with pytest.raises(ValueError):
            _lib.default_chunk_cols(4, 10, itemsize=bad)


def test_refused_combinations_raise_value_error():
    from efa_xray_amd import EnSRF, Observation, AdaptiveInflation
    from efa_xray_amd.distributed import ShardedEnSRF
    st, _ = _state(np.float32)
    ob = Observation(value=1.0, error=1.0, lat=35.0, lon=255.0, assimilate_this=True, localize_radius=1000.0)
    ob.estimate = lambda s: s.to_vect()[0]
    ai = AdaptiveInflation(st.astype(np.float64), ("adaptive", None, (1.0, 0.6)))
    with pytest.raises(ValueError, match="float32"):
        EnSRF(st, [ob], verbose=False, loc="GC", adaptive_inflation=ai)
    # a float32 prior swapped in after construction is refused by update() as well
    flt = EnSRF(st.astype(np.float64), [ob], verbose=False, loc="GC", adaptive_inflation=ai)
    flt.prior = st
    with pytest.raises(ValueError, match="float32"):
        flt.update()
    with pytest.raises(ValueError, match="float32"):
        EnSRF(st, [ob], verbose=False).update_arrays(np.zeros(st.nstate() + 1), np.zeros((st.nstate() + 1, st.nmems())))
    sh = ShardedEnSRF(None, 4, 12, st.nmems())
    X = st.to_vect()
    obd = dict(value=np.zeros(1), error=np.ones(1), assim=np.ones(1, dtype=bool))
    idx, wts = np.zeros((1, 1), dtype=np.int64), np.ones((1, 1))
    with pytest.raises(ValueError, match="float32"):
        sh.update(X, X.copy(), idx, wts, obd)
    with pytest.raises(ValueError, match="float32"):
        sh.partial_estimates(X, idx, wts)
    with pytest.raises(ValueError, match="float32"):
        sh.assimilate(X, X.copy(), np.zeros((1, st.nmems())), obd)


def test_float64_wrappers_refuse_a_float32_device_array():
    """A float64 kernel on a float32 allocation would run past its end: the `Context` wrappers check the dtype of a DeviceArray."""
    from efa_xray_amd import _lib

    class Fake(_lib.DeviceArray):
        def __init__(self, dtype):
            self.dtype, self.ptr, self.ctx = np.dtype(dtype), None, None

        def free(self):
            pass

    a32, a64 = Fake(np.float32), Fake(np.float64)
    addr = _lib.Context._addr
    with pytest.raises(ValueError, match="float32 DeviceArray"):
        addr(a32)
    with pytest.raises(ValueError, match="float64 DeviceArray"):
        addr(a64, np.float32)
    assert addr(a64) is None and addr(a32, np.float32) is None and addr(a32, None) is None and addr(None) is None
    # every wrapper of a float64 kernel goes through the check before it reaches the library
    class NoLib(object):
        def __getattr__(self, name):
            return lambda *args: pytest.fail("%s was reached with a DeviceArray of the wrong dtype" % name)

    ctx = _lib.Context.__new__(_lib.Context)
    ctx.lib, ctx.handle = NoLib(), None
    for call in (lambda: ctx.form_perts(4, 6, a32, a64, a64), lambda: ctx.form_perts(4, 6, a64, a64, a32),
                 lambda: ctx.posterior(4, 6, a64, a32, a64), lambda: ctx.forward_interp(12, 0, 12, 4, 6, a32, a64),
                 lambda: ctx.forward_stencil(4, 0, 6, a32, np.zeros((1, 1), dtype=np.int64), np.ones((1, 1)), a64),
                 lambda: ctx.state_cycle(4, 6, a32, a32), lambda: ctx.state_phase(4, 6, a64, a32, a64, a64),
                 lambda: ctx.inflate_rows(4, 6, a32, a64), lambda: ctx.state_cycle_f32(4, 6, a64, a64),
                 lambda: ctx.ensrf_cycle(4, 6, 0, a32, a32, a64, a64, [], [], []),
                 lambda: ctx.obs_phase(6, 0, a32, a64, [], [], [])):
        with pytest.raises(ValueError, match="DeviceArray"):
            call()
    ctx.handle = None
