"""CPU-side tests (no GPU needed): the C-ABI library loads and exports every
symbol include/efa_hip.h declares, the product never touches the oracle, and
the host-side containers behave like the reference's."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from oracle import ensrf_oracle as orc


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "efa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(efa_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    from efa_xray_amd import _lib
    lib = _lib.load_library()
    declared = _declared_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), "libefa_hip.so does not export %s" % name
    # the ctypes table covers exactly the header
    assert sorted(_lib.SIGNATURES.keys()) == declared
    assert lib.efa_abi_version() == 1
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (efa_[a-z0-9_]+)", out))
    assert exported == set(declared)


def test_baseline_kernels_fit_their_register_budget():
    """The kernels BASELINE.json's configs run must not spill vector registers (a launch bound that asked for
    more waves than two rows of 100 members allow once made configs[3] six times slower without failing any
    parity test), and the persistent Phase-A kernels must fit one workgroup per CU."""
    from efa_xray_amd import _lib
    from _codeobj import gc_kernel_fragment, kernel_table
    tab = kernel_table(_lib.LIB_PATH)
    assert len(tab) > 100

    def find(*parts):
        hits = [k for n, k in tab.items() if all(p in n for p in parts)]
        assert len(hits) == 1, (parts, [h[".name"] for h in hits])
        return hits[0]

    no_spill = [
        ("k_transformILi13ELb1ELb1ELb1E",),          # headline, configs[1] (M = 100, 50 -> NU 13, 7: checked below)
        ("k_transformILi7ELb1ELb1ELb1E",),
        ("k_pipe_gramILi10E",), ("k_pipe_gramILi13E",),
        ("k_contract_f32_raILi64E",),                # configs[4]
        ("7k_sweepILi4ELi13ELb1E",),                 # the unlocalised batch sweep at M = 100
    ]
    for parts in no_spill:
        k = find(*parts)
        assert k.get(".vgpr_spill_count", 0) == 0, (k[".name"], k[".vgpr_count"], k[".vgpr_spill_count"])
    # configs[2] (80 members, four rows per quad) and configs[3] (100 members, three rows per quad) at two waves per SIMD: only the
    # per-row addresses and means spill, saved and reloaded once per group of slabs (no scratch access in the loop over the obs)
    assert find(gc_kernel_fragment("quad", "plain", "f64", 10, True, True, 4)).get(".vgpr_spill_count", 0) <= 32
    assert find(gc_kernel_fragment("quad", "plain", "f64", 13, True, True, 3)).get(".vgpr_spill_count", 0) <= 32
    # Phase A: 8 waves of up to 256 registers each; headline (100 members), configs[2] (80, tapered), configs[3] (100, tapered)
    for nm in ("k_pipe_bandILi13ELb0E", "k_pipe_bandILi10ELb1E", "k_pipe_bandILi13ELb1E"):
        band = find(nm)
        assert band.get(".vgpr_spill_count", 0) == 0 and band[".vgpr_count"] <= 256, (nm, band[".vgpr_count"])
    # occupancy the kernels are written for (512 VGPRs per SIMD lane on gfx950)
    assert find(gc_kernel_fragment("quad", "plain", "f64", 8, True, True, 2))[".vgpr_count"] <= 168      # three waves per SIMD
    assert find(gc_kernel_fragment("quad", "plain", "f64", 10, True, True, 4))[".vgpr_count"] <= 256     # two
    assert find(gc_kernel_fragment("quad", "plain", "f64", 13, True, True, 3))[".vgpr_count"] <= 256     # two
    assert find("k_contract_f32_raILi64E")[".vgpr_count"] <= 256
    # the row-per-lane GC sweep holds a whole row per lane: two waves per SIMD up to 104 members, no spills at configs[2] / configs[3]
    for mp in (80, 100):
        lane = find(gc_kernel_fragment("lane", "plain", "f64", mp, True))
        assert lane.get(".vgpr_spill_count", 0) == 0 and lane[".vgpr_count"] <= 256, (mp, lane[".vgpr_count"])
    # configs[4] at every member count: all eight instantiations of k_contract_f32_ra (KH = 8 .. 64; 196 .. 252 VGPRs when this was
    # written) and the general kernel (196 VGPRs + 64 AGPRs) keep everything in registers: no spill, no scratch
    contract = [find("k_contract_f32_raILi%dE" % kh) for kh in range(8, 65, 8)] + [find("k_contract_f32E")]
    assert len(set(k[".name"] for k in contract)) == 9
    for k in contract:
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (k[".name"], k[".vgpr_count"])
        assert k[".private_segment_fixed_size"] == 0, (k[".name"], k[".private_segment_fixed_size"])
    for k in contract[:8]:
        assert k[".vgpr_count"] <= 256, (k[".name"], k[".vgpr_count"])


def test_no_cpu_fallback_without_gpu():
    """Without a usable device the product fails loudly instead of computing on the CPU."""
    from efa_xray_amd import _lib, EnSRF, EnsembleState, Observation
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.EfaError) as ei:
        _lib.Context(0)
    assert ei.value.status == _lib.EFA_ERR_NO_DEVICE
    st = EnsembleState.from_array(np.random.default_rng(0).standard_normal((1, 1, 2, 3, 4)),
                                  np.zeros((2, 3)), np.zeros((2, 3)))
    ob = Observation(value=1.0, error=1.0, lat=0.0, lon=0.0, assimilate_this=True)
    ob.estimate = lambda s: s.to_vect()[0]
    with pytest.raises(_lib.EfaError):
        EnSRF(st, [ob], verbose=False).update()


def test_host_side_of_the_c_abi_under_address_and_ub_sanitizers():
    """SURVEY.md section 5's sanitizer row, on the CPU build only (no GPU sanitizers on this pool): the host side of the C ABI compiled
    with -fsanitize=address,undefined (make asan; device code as in the product), every entry point's argument checks walked in a
    child process under the preloaded clang ASan runtime.  A sanitizer report aborts the child.  Every GPU is hidden from the
    child, so it walks the same host-only path on a GPU box as on a CPU box (the GPU runtime never starts under the sanitizer)."""
    import glob
    csrc = os.path.join(ROOT, "efa_xray_amd", "csrc")
    lib = os.path.join(ROOT, "efa_xray_amd", "libefa_hip_asan.so")
    srcs = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(ROOT, "include", "efa_hip.h")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["make", "-C", csrc, "asan", "-j", str(min(8, os.cpu_count() or 1))], stdout=subprocess.DEVNULL)
    rt = glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so")
    if not rt:
        pytest.skip("clang ASan runtime not found")
    env = dict(os.environ, LD_PRELOAD=rt[0], ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0:protect_shadow_gap=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ROCR_VISIBLE_DEVICES="-1", HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_asan_abi_driver.py"), lib], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode("utf-8", "replace")
    assert out.returncode == 0 and "asan-abi-ok" in text, text[-3000:]
    assert "AddressSanitizer" not in text and "runtime error" not in text, text[-3000:]


def test_missing_library_fails_loudly(tmp_path):
    from efa_xray_amd import _lib
    with pytest.raises(RuntimeError, match="not built"):
        _lib.load_library(str(tmp_path / "libefa_hip.so"))


def test_product_never_imports_the_oracle():
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "efa_xray_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(base, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b|oracle/", src, flags=re.M):
                    bad.append(os.path.join(base, f))
    assert not bad, bad
    code = ("import sys; sys.path.insert(0, %r); import efa_xray_amd, efa_xray_amd._lib; "
            "assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


# ---------------------------------------------------------------------------
def _state(seed=0, shape=(2, 3, 4, 5, 6)):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(seed)
    nvar, nt, ny, nx, nm = shape
    lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(230, 260, nx), indexing="ij")
    arr = rng.standard_normal(shape)
    vd = dict(("v%d" % i, (("validtime", "y", "x", "mem"), arr[i])) for i in range(nvar))
    cd = dict(validtime=np.arange(nt) * 3600.0, lat=(("y", "x"), lat), lon=(("y", "x"), lon),
              mem=np.arange(1, nm + 1))
    return EnsembleState.from_vardict(vd, cd), arr, lat, lon


def test_ensemble_state_surface_matches_reference_semantics():
    st, arr, lat, lon = _state()
    nvar, nt, ny, nx, nm = arr.shape
    assert (st.nvars(), st.ntimes(), st.ny(), st.nx(), st.nmems()) == (nvar, nt, ny, nx, nm)
    assert st.nstate() == nvar * nt * ny * nx
    assert st.shape() == arr.shape
    assert st.vars() == ["v0", "v1"]
    v = st.to_vect()
    # state-vector order: variable, time, y, x; member last (ensemble.py:110-114)
    assert v.shape == (st.nstate(), nm) and np.array_equal(v, arr.reshape(-1, nm))
    st2 = __import__("copy").deepcopy(st)
    st2.from_vect(v * 2.0)
    assert np.array_equal(st2.to_vect(), v * 2.0) and np.array_equal(st.to_vect(), v)
    assert np.array_equal(st["lat"].values, lat) and st["lon"].shape == lon.shape
    # dims given in another order are transposed to (validtime, y, x, mem)
    from efa_xray_amd import EnsembleState
    st3 = EnsembleState.from_vardict({"a": (("mem", "x", "y", "validtime"), np.transpose(arr[0], (3, 2, 1, 0)))},
                                     dict(lat=lat, lon=lon))
    assert np.array_equal(st3.to_vect(), arr[0].reshape(-1, nm))
    pert = st.ensemble_perts()
    assert np.allclose(pert.to_vect().mean(axis=1), 0.0, atol=1e-15)
    assert np.allclose(st.ensemble_mean()["v1"], arr[1].mean(axis=-1))


def test_geometry_helpers_match_reference_known_answers():
    from efa_xray_amd import EnsembleState, Observation, gaspari_cohn, haversine
    k = load_golden("KAT")
    assert np.array_equal(gaspari_cohn(k["gc_d"], float(k["gc_c"])), k["gc_w"])
    hv = np.array([haversine(tuple(a), tuple(b)) for a, b in zip(k["hv_a"], k["hv_b"])])
    assert np.array_equal(hv, k["hv_km"])
    st = EnsembleState.from_array(np.zeros((1, 1, 9, 12, 2)), k["dp_lat"], k["dp_lon"])
    assert np.array_equal(st.distance_to_point(*k["dp_pt"]), k["dp_km"])
    ob = Observation(lat=k["dp_pt"][0], lon=k["dp_pt"][1], localize_radius=900.0)
    w = ob.localize(st)
    assert np.array_equal(w, orc.localize_state(k["dp_lat"], k["dp_lon"], k["dp_pt"][0], k["dp_pt"][1], 900.0))
    obs = [Observation(lat=a[0], lon=a[1]) for a in k["hv_a"][:8]]
    w2 = ob.localize(obs)
    assert np.array_equal(w2, orc.localize_obs(k["hv_a"][:8, 0], k["hv_a"][:8, 1], ob.lat, ob.lon, 900.0))
    # 1-D lat/lon columns broadcast over y
    st1 = EnsembleState.from_array(np.zeros((1, 1, 3, 4, 2)), np.arange(4.0), np.arange(4.0) * 2)
    cl, co = st1.column_latlon()
    assert np.array_equal(cl, np.tile(np.arange(4.0), 3)) and np.array_equal(co, np.tile(np.arange(4.0) * 2, 3))


def test_observation_defaults_and_interpolate_stencil():
    from efa_xray_amd import Observation
    ob = Observation()
    assert ob.assimilate_this is False and ob.assimilated is False and ob.localize_radius is None
    st, arr, lat, lon = _state(3)
    o = Observation(value=1.0, obtype="v1", time=4000.0, lat=41.3, lon=244.4, error=1.0)
    ye = o.estimate(st)
    rows, wts = o.stencil(st)
    assert ye.shape == (st.nmems(),)
    assert np.allclose(ye, (wts[:, None] * st.to_vect()[rows]).sum(axis=0))
    iy, ix, sw = orc.interp_space_weights(lat, lon, 41.3, 244.4)
    assert abs(wts.sum() - 1.0) < 1e-12 and abs(sw.sum() - 1.0) < 1e-12
    # time weights as coded in the reference (ensemble.py:218-224): weight of the
    # later time = |t - t_later| / dt
    w_later = abs(4000.0 - 7200.0) / 3600.0
    nt, ny, nx = st.ntimes(), st.ny(), st.nx()
    later = [(1 * nt + 2) * ny * nx + y * nx + x for y, x in zip(iy, ix)]
    got = dict(zip(rows.tolist(), wts.tolist()))
    assert np.allclose([got[r] for r in later], w_later * sw)
    assert o.estimate(st) is not None
    assert Observation(obtype="v0", time=1e9, lat=40, lon=240).estimate(st) is None


@pytest.mark.parametrize("name", ["G9", "G10"])
def test_host_interpolation_stencil_matches_the_reference(name):
    """`EnsembleState.interp_stencil` / `interpolate` / `nearest_points` and `Observation.estimate` against what the
    reference's own ensemble.py:152-239 / observation.py:40-50 returned on the same state (fixtures G9: 2-D lat/lon,
    datetime64 valid times; G10: the 1-D lat/lon branch incl. one ob within 1 km of a grid point)."""
    from conftest import load_golden
    from efa_xray_amd import EnsembleState, Observation
    g = load_golden(name)
    nvar, nt, ny, nx, M = [int(v) for v in g["shape"]]
    names = [str(n) for n in g["var_names"]]
    st = EnsembleState.from_array(g["X"], g["grid_lat"], g["grid_lon"], varnames=names, validtime=g["validtime"])
    for k in range(len(g["ob_lat"])):
        ob = Observation(obtype=names[g["ob_var"][k]], time=g["ob_time"][k], lat=float(g["ob_lat"][k]),
                         lon=float(g["ob_lon"][k]))
        near = st.nearest_points(ob.lat, ob.lon, npt=4)
        assert np.array_equal(np.stack(near, axis=-1), g["nearest"][k])
        rows, wts = ob.stencil(st)
        dense = np.zeros(nvar * nt * ny * nx)
        np.add.at(dense, rows, wts)
        iv = int(g["ob_var"][k])
        per_var = dense.reshape(nvar, -1)
        assert not per_var[np.arange(nvar) != iv].any()
        np.testing.assert_allclose(per_var[iv], g["weights"][k], rtol=1e-13, atol=0)
        np.testing.assert_allclose(ob.estimate(st), g["HX"][k], rtol=1e-12, atol=1e-14)
    late = Observation(obtype=names[0], time=g["validtime"][-1] + np.timedelta64(1, "s"), lat=float(g["ob_lat"][0]),
                       lon=float(g["ob_lon"][0]))
    assert late.estimate(st) is None


def test_obs_statistics_table_columns():
    from efa_xray_amd import Observation
    from efa_xray_amd.postprocess.postprocess import obs_assimilation_statistics
    st, arr, lat, lon = _state(5)
    obs = [Observation(value=1.0, obtype="v0", time=3600.0, lat=40.1, lon=240.2, error=0.5, description="a"),
           Observation(value=2.0, obtype="v1", time=3600.0, lat=45.0, lon=250.0, error=0.7, description="b")]
    df = obs_assimilation_statistics(st, st, obs)
    for col in ('validtime', 'flead', 'lat', 'lon', 'obtype', 'description', 'ob error', 'value', 'assimilated',
                'prior mean', 'post mean', 'prior variance', 'post variance'):
        assert col in df.columns
    ye = obs[0].estimate(st)
    assert abs(df['prior mean'][0] - ye.mean()) < 1e-15 and abs(df['post variance'][0] - ye.var()) < 1e-15
    obs[0].prior_mean, obs[0].prior_var = 1.5, 2.5
    obs[1].prior_mean, obs[1].prior_var, obs[1].post_mean, obs[1].post_var, obs[1].assimilated = 1.0, 2.0, 0.5, 1.0, True
    df2 = obs_assimilation_statistics(st, st, obs, from_diagnostics=True)
    assert df2['post mean'][1] == 0.5 and df2['post variance'][0] == 2.5


def test_inflate_state_float_dict_forms():
    """assimilation.py:52-118: float / per-variable / per-dimension forms of inflate_state().
    (No GPU needed: it is host logic on the NumPy-backed state.)  PARITY UNPINNED: the reference's
    inflation needs a real xarray Dataset, absent from the image; this follows its source text."""
    from efa_xray_amd.assimilation.assimilation import Assimilation
    st, arr, lat, lon = _state(7)
    nvar, nt, ny, nx, nm = arr.shape
    mine = __import__("copy").deepcopy(st)
    a = Assimilation(mine, [], inflation=1.3, verbose=False)
    assert a.is_inflated is False
    a.inflate_state()
    assert a.is_inflated is True
    assert a.prior is mine                  # the float form works in place on the caller's state (assimilation.py:67)
    for i in range(nvar):
        assert np.allclose(a.prior.variables["v%d" % i].reshape(-1, nm),
                           orc.inflate_constant(arr[i].reshape(-1, nm), 1.3), rtol=1e-14, atol=1e-14)
    before = a.prior.to_vect().copy()
    a.inflate_state()                      # second call is a no-op (assimilation.py:57-59)
    assert np.array_equal(a.prior.to_vect(), before)
    # per-variable factors; unknown names are skipped (assimilation.py:103-113)
    b = Assimilation(__import__("copy").deepcopy(st), [], inflation={"v1": 2.0, "nope": 3.0}, verbose=False)
    b.inflate_state()
    assert np.array_equal(b.prior.variables["v0"], arr[0])
    m1 = arr[1].mean(axis=-1, keepdims=True)
    assert np.allclose(b.prior.variables["v1"], (arr[1] - m1) * 2.0 + m1, rtol=1e-14, atol=1e-14)
    # per-time factors broadcast over y, x, members; the caller's state object is left alone (assimilation.py:82-96)
    mine = __import__("copy").deepcopy(st)
    f = np.linspace(1.0, 1.5, nt)
    c = Assimilation(mine, [], inflation={"validtime": f}, verbose=False)
    c.inflate_state()
    assert np.array_equal(mine.to_vect(), st.to_vect())
    for i in range(nvar):
        m = arr[i].mean(axis=-1, keepdims=True)
        assert np.allclose(c.prior.variables["v%d" % i], (arr[i] - m) * f[:, None, None, None] + m, rtol=1e-14, atol=1e-14)
    with pytest.raises((IOError, OSError)):   # the file form reads a netCDF file of factors: this one does not exist
        Assimilation(mine, [], inflation="no_such_factors.nc", verbose=False).inflate_state()


def test_inflation_hook_runs_inside_format_prior_state_and_update():
    """assimilation.py:131-134 (reached from ensrf.py:44): `format_prior_state()` -- and so `update()` --
    inflates the prior first whenever `inflation is not None`.  The GPU work after the hook is cut
    off here by a sentinel; tests/test_gpu_parity.py checks the numbers."""
    from efa_xray_amd import EnSRF
    from efa_xray_amd.assimilation.assimilation import Assimilation

    class Stop(Exception):
        pass

    def stop(self):
        raise Stop()

    st, arr, lat, lon = _state(9)
    nm = arr.shape[-1]
    for cls, call, kw in ((Assimilation, "format_prior_state", {}), (EnSRF, "update", {}), (EnSRF, "format_prior_state", {})):
        mine = __import__("copy").deepcopy(st)
        a = cls(mine, [], inflation=1.25, verbose=False, **kw)
        a._context = stop.__get__(a)
        with pytest.raises(Stop):
            getattr(a, call)()
        assert a.is_inflated is True
        assert np.allclose(mine.to_vect(), orc.inflate_constant(st.to_vect(), 1.25), rtol=1e-14, atol=1e-14)
        none = cls(__import__("copy").deepcopy(st), [], inflation=None, verbose=False)
        none._context = stop.__get__(none)
        with pytest.raises(Stop):
            getattr(none, call)()
        assert none.is_inflated is False and np.array_equal(none.prior.to_vect(), st.to_vect())


def _small_state(seed=0, nt=2, ny=3, nx=4, nm=5):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(seed)
    arr = rng.standard_normal((2, nt, ny, nx, nm))
    lat, lon = np.meshgrid(np.linspace(30, 40, ny), np.linspace(250, 260, nx), indexing="ij")
    vt = np.array(["2020-01-01T00", "2020-01-01T06"], dtype="datetime64[s]")[:nt]
    return EnsembleState.from_array(arr, lat, lon, varnames=["t2m", "psfc"], validtime=vt)


def test_state_round_trips_through_netcdf(tmp_path):
    """SURVEY.md 8(f4), ensemble.py:269-273: save_to_disk writes a netCDF file that reads back to the same state
    (classic netCDF-3 through scipy where xarray is absent).  PARITY UNPINNED: the reference's writer needs xarray."""
    from efa_xray_amd import EnsembleState
    st = _small_state()
    fn = str(tmp_path / "ens_state.nc")
    st.save_to_disk(fn)
    back = EnsembleState.from_netcdf(fn)
    assert back.vars() == st.vars()
    assert back.shape() == st.shape()
    for name in st.vars():
        assert np.array_equal(back.variables[name], st.variables[name])
    assert np.array_equal(back.coords["lat"], st.coords["lat"]) and np.array_equal(back.coords["lon"], st.coords["lon"])
    assert np.array_equal(np.asarray(back.coords["validtime"]).astype("datetime64[s]"),
                          np.asarray(st.coords["validtime"]).astype("datetime64[s]"))
    assert np.array_equal(back.to_vect(), st.to_vect())


def test_inflation_factors_from_a_netcdf_file(tmp_path):
    """assimilation.py:71-79: `inflation='file.nc'` multiplies the perturbations of each variable by the file's
    variable of the same name, broadcast by dimension name, and rebinds the prior (the caller's state is untouched).
    Checked against the closed form; a variable the file does not hold stays as it is."""
    from scipy.io import netcdf_file
    from efa_xray_amd.assimilation.assimilation import Assimilation
    st = _small_state(3)
    nt, ny, nx = 2, 3, 4
    rng = np.random.default_rng(5)
    f_yx = 1.0 + rng.random((ny, nx))
    fn = str(tmp_path / "inflation.nc")
    with netcdf_file(fn, "w", version=2) as f:
        f.createDimension("y", ny)
        f.createDimension("x", nx)
        f.createVariable("t2m", "d", ("x", "y"))[:] = f_yx.T          # dimension ORDER in the file is free
    before = {n: v.copy() for n, v in st.variables.items()}
    a = Assimilation(st, [], inflation=fn, verbose=False)
    a.inflate_state()
    assert a.is_inflated and a.prior is not st
    for n in st.vars():
        assert np.array_equal(st.variables[n], before[n])              # the caller's object is not touched
    m = before["t2m"].mean(axis=-1, keepdims=True)
    want = (before["t2m"] - m) * f_yx[None, :, :, None] + m
    assert np.allclose(a.prior.variables["t2m"], want, rtol=1e-15, atol=0)
    assert np.array_equal(a.prior.variables["psfc"], before["psfc"])   # no factors in the file
    a.inflate_state()                                                  # second call: no-op (assimilation.py:57-59)
    assert np.allclose(a.prior.variables["t2m"], want, rtol=1e-15, atol=0)
    with netcdf_file(fn, "w", version=2) as f:                        # a mismatching file must not broadcast silently
        f.createDimension("y", ny + 1)
        f.createVariable("t2m", "d", ("y",))[:] = np.ones(ny + 1)
    with pytest.raises(ValueError):
        Assimilation(_small_state(3), [], inflation=fn, verbose=False).inflate_state()


def test_lane_sweep_dpp_operands_are_not_written_by_the_vector_alu_just_before():
    """k_sweep_gc_lane's multiply-adds are inline assembly (v_fmac_f64_dpp row_newbcast), and the compiler's hazard
    recogniser does not see through inline assembly: a VALU write of a register that one of the next two instructions
    reads through DPP would need wait states nobody inserts.  The kernel is written so that the DPP operand (ye) only
    ever comes from LDS reads; this checks the generated code of every instantiation."""
    import os
    import re
    import subprocess
    import tempfile
    from efa_xray_amd import _lib
    from _codeobj import code_objects
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not in this image")
    reg = re.compile(r"v\[(\d+):(\d+)\]|v(\d+)")

    def regs(tok):
        m = reg.fullmatch(tok.strip().rstrip(","))
        if not m:
            return set()
        if m.group(3) is not None:
            return {int(m.group(3))}
        return set(range(int(m.group(1)), int(m.group(2)) + 1))

    seen = 0
    for co in code_objects(_lib.LIB_PATH):
        if b"k_sweep_gc_lane" not in co:
            continue
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(co)
            f.flush()
            asm = subprocess.run([objdump, "-d", "--mcpu=gfx950", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        inside = False
        recent = []   # destination registers of the last two VALU instructions
        for line in asm.splitlines():
            if line.endswith(">:"):
                inside = "k_sweep_gc_lane" in line
                recent = []
                continue
            if not inside or not line.startswith("\t"):
                continue
            ins = line.split("//")[0].split()
            if not ins or ins[0] == "s_nop":
                continue
            ops = " ".join(ins[1:]).split(",")
            if "row_newbcast" in line:
                seen += 1
                src = regs(ops[1].split()[0])
                assert src, line
                for written in recent:
                    assert not (src & written), "DPP operand written by the vector ALU within two instructions: " + line
            recent = (recent + [regs(ops[0]) if ins[0].startswith("v_") and ops else set()])[-2:]
    assert seen > 52 * 8
