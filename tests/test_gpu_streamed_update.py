"""GPU tests of the streamed update `EnSRF(..., streamed=True)`: the prior stays in host memory and crosses the
device in column chunks.  Every case is compared with the unstreamed `update()` of the same inputs in the same process, bit for
bit (`np.array_equal` on `to_vect()` and on all five diagnostics of every ob); the goldens also against their fixtures at the
project's 1e-10.

Bit equality holds on every path below: no ragged-tail path that makes a row's bits depend on its position in a chunk was found
(a chunk is a column shard, and tests/test_gpu_sharded.py pins the shards), so no path is held to the looser 1e-10 here."""
import ctypes
import gc
from copy import deepcopy

import numpy as np
import pytest

from conftest import load_golden, GOLDEN_CASES
from test_gpu_parity import assert_parity, _make_api_objects

pytestmark = pytest.mark.gpu

DIAG = ("prior_mean", "prior_var", "post_mean", "post_var", "assimilated")


def _lib():
    from efa_xray_amd import _lib
    return _lib


def _diag(obs):
    """The five diagnostics of every ob as comparable arrays (None, the constructor's value, as NaN)."""
    out = {}
    for key in DIAG:
        out[key] = np.array([np.nan if getattr(o, key) is None else float(getattr(o, key)) for o in obs])
    return out


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                                  b.view(np.uint64) if b.dtype == np.float64 else b)


def _run(state, obs, **kw):
    """update() on copies of the obs (the diagnostics are written onto them): (posterior state, to_vect(), diagnostics)."""
    from efa_xray_amd import EnSRF
    obs = deepcopy(obs)
    flt = EnSRF(state, obs, verbose=False, **kw)
    post, obs_out = flt.update()
    assert obs_out is obs
    return post, post.to_vect(), _diag(obs), flt


def _assert_equal_runs(ref, got, what):
    assert _same_bits(ref[1], got[1]), "%s: posterior differs from the unstreamed update (max abs %.3e)" % (
        what, np.max(np.abs(ref[1] - got[1])))
    for key in DIAG:
        assert _same_bits(ref[2][key], got[2][key]), "%s: %s differs from the unstreamed update" % (what, key)


def _chunk_settings(ncol):
    """16, a value giving a ragged last chunk, one chunk for everything, and the default."""
    ragged = next((c for c in (32, 48, 16, 64, 80, 96) if c < ncol and ncol % c), 16)
    return [16, ragged, ncol + 16, None]


def _compare(state, obs, what, chunks=None, **kw):
    """Unstreamed against streamed at every chunk setting; returns the unstreamed run."""
    X0 = state.to_vect().copy()
    ref = _run(state, obs, **kw)
    ncol = state.ny() * state.nx()
    for cc in (chunks if chunks is not None else _chunk_settings(ncol)):
        got = _run(state, obs, streamed=True, stream_chunk_cols=cc, **kw)
        _assert_equal_runs(ref, got, "%s, stream_chunk_cols=%r" % (what, cc))
        want = len(_lib().plan_chunks(ncol, cc if cc is not None else _lib().default_chunk_cols(state.nvars() * state.ntimes(),
                                                                                            state.nmems())))
        assert got[3].last_stream["chunks"] == want, what
        assert got[0] is not state
    assert _same_bits(state.to_vect(), X0), what + ": the prior was written"
    return ref


# ---------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------
def _state(seed, M, nvar=2, nt=3, ny=9, nx=13):
    """ncol = ny*nx = 117 by default: seven blocks of 16 and a ragged rest of 5."""
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(seed)
    lat, lon = np.meshgrid(np.linspace(30, 50, ny), np.linspace(230, 262, nx), indexing="ij")
    arr = rng.standard_normal((nvar, nt, ny, nx, 1)) + 2.0 * rng.standard_normal((nvar, nt, ny, nx, M))
    return EnsembleState.from_array(arr, lat, lon, validtime=np.array([0.0, 3600.0, 7200.0, 10800.0])[:nt])


def _point_obs(state, seed, P, cls=None, **extra):
    """Plain observations (the default forward operator: stencils of up to 8 rows, time brackets and exact valid times)."""
    from efa_xray_amd import Observation
    rng = np.random.default_rng(seed)
    names = state.vars()
    times = [0.0, 1800.0, 3600.0, 5000.0, 7200.0] if state.ntimes() >= 3 else [0.0]
    obs = []
    for k in range(P):
        obs.append((cls or Observation)(value=float(rng.standard_normal()), obtype=names[k % len(names)],
                                        time=float(times[k % len(times)]), error=float(rng.uniform(0.5, 1.5)),
                                        lat=float(rng.uniform(31, 49)), lon=float(rng.uniform(231, 261)),
                                        assimilate_this=(k % 6 != 1), localize_radius=float(rng.uniform(600.0, 1500.0)), **extra))
    return obs


@pytest.mark.parametrize("M", [2, 7, 50, 100, 137, 256])
@pytest.mark.parametrize("loc", [False, "GC"])
def test_ensemble_sizes(M, loc):
    state = _state(100 + M, M)
    obs = _point_obs(state, 200 + M, 30)
    _compare(state, obs, "M=%d loc=%r" % (M, loc), loc=loc)


# ---------------------------------------------------------------------------
# goldens: the fixtures at 1e-10, the unstreamed update bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_goldens(name):
    g = load_golden(name)
    state, obs = _make_api_objects(g)
    ncol = state.ny() * state.nx()
    ref = _compare(state, obs, name, loc=(g["loc"] or False))
    for cc in _chunk_settings(ncol):
        post, vect, diag, _ = _run(state, obs, streamed=True, stream_chunk_cols=cc, loc=(g["loc"] or False))
        assert_parity(vect, g["post"], "%s post, chunk %r" % (name, cc))
        for key in ("prior_mean", "prior_var"):
            assert_parity(diag[key], g[key], "%s %s" % (name, key))
        done = g["assimilated"].astype(bool)
        assert np.array_equal(diag["assimilated"].astype(bool), done)
        for key in ("post_mean", "post_var"):
            assert_parity(diag[key][done], g[key][done], "%s %s" % (name, key))
            assert np.isnan(diag[key][~done]).all()
    assert_parity(ref[1], g["post"], name + " unstreamed post")


def test_golden_g11_default_forward_operator():
    """G11: plain `Observation`s -- the forward operator runs on the compact gathered rows instead of the resident state."""
    from efa_xray_amd import EnsembleState, Observation
    g = load_golden("G11")
    names = [str(n) for n in g["var_names"]]
    state = EnsembleState.from_array(g["X"], g["grid_lat"], g["grid_lon"], varnames=names, validtime=g["validtime"])
    obs = [Observation(value=float(g["ob_value"][k]), obtype=names[g["ob_var"][k]], time=g["ob_time"][k],
                       error=float(g["ob_error"][k]), lat=float(g["ob_lat"][k]), lon=float(g["ob_lon"][k]),
                       assimilate_this=bool(g["ob_assim"][k]), localize_radius=float(g["ob_radius"][k]))
           for k in range(len(g["ob_value"]))]
    _compare(state, obs, "G11", loc="GC")
    for cc in _chunk_settings(state.ny() * state.nx()):
        post, vect, diag, flt = _run(state, obs, streamed=True, stream_chunk_cols=cc, loc="GC")
        assert flt._default_forward_operator()
        assert_parity(vect, g["post"], "G11 post, chunk %r" % (cc,))
        for key in ("prior_mean", "prior_var"):
            assert_parity(diag[key], g[key], "G11 " + key)
        done = g["assimilated"].astype(bool)
        assert np.array_equal(diag["assimilated"].astype(bool), done)
        for key in ("post_mean", "post_var"):
            assert_parity(diag[key][done], g[key][done], "G11 " + key)
    # the obs-space priors themselves: the compact route has the bits of the resident one
    from efa_xray_amd import EnSRF
    flt = EnSRF(state, obs, verbose=False)
    ctx = flt._context()
    assert _same_bits(flt.streamed_ob_estimates(ctx), flt.compute_ob_estimates())


# ---------------------------------------------------------------------------
# options
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["sweep", "transform"])
def test_paths(path):
    state = _state(1, 20)
    obs = _point_obs(state, 2, 40)
    try:
        for batch in (64, 7):
            ref = _compare(state, obs, "path=%s obs_batch=%r" % (path, batch), loc=False, path=path, obs_batch=batch)
            assert ref[3].last_timing["path"] == {"sweep": 1, "transform": 2}[path]
        _compare(state, obs, "GC path=%s" % path, loc="GC", path=path, obs_batch=7)
    finally:
        _lib().get_context(0).set_option("obs_batch", 64)     # (an option of the shared context: back to its default)


@pytest.mark.parametrize("loc", [False, "GC"])
@pytest.mark.parametrize("relax", [dict(rtps=0.6), dict(rtpp=0.4)])
@pytest.mark.parametrize("path", [None, "sweep"])
def test_relaxation(loc, relax, path):
    state = _state(3, 24)
    obs = _point_obs(state, 4, 40)
    ref = _compare(state, obs, "loc=%r %r path=%r" % (loc, relax, path), loc=loc, path=path, **relax)
    plain = _run(state, obs, loc=loc, path=path)
    assert not _same_bits(ref[1], plain[1]), "the relaxation did nothing"


@pytest.mark.parametrize("loc", [False, "GC"])
def test_outlier_threshold_with_injected_gross_errors(loc):
    state = _state(5, 30)
    obs = _point_obs(state, 6, 48)
    bad = [k for k in range(len(obs)) if k % 9 == 4]
    for k in bad:
        obs[k].value = float(obs[k].value) + 60.0           # far outside prior spread + error
        obs[k].assimilate_this = True
    ref = _compare(state, obs, "outlier loc=%r" % (loc,), loc=loc, outlier_threshold=3.0)
    assert not ref[2]["assimilated"][bad].any(), "the gross errors were not rejected"
    assert ref[2]["assimilated"].sum() > 20


def test_vertical_localisation():
    state = _state(7, 16)
    obs = _point_obs(state, 8, 36)
    rng = np.random.default_rng(9)
    for k, ob in enumerate(obs):
        if k % 5 != 2:                                       # some obs carry no vertical information
            ob.vert = float(rng.uniform(200.0, 1000.0))
            ob.vert_localize_radius = float(rng.uniform(150.0, 500.0))
    vert = rng.uniform(200.0, 1000.0, (state.nvars(), state.ntimes()))
    vert[1, 0] = np.nan                                      # a slab that is not localised vertically
    ref = _compare(state, obs, "vert_coord", loc="GC", vert_coord=vert)
    plain = _run(state, obs, loc="GC")
    assert not _same_bits(ref[1], plain[1]), "the vertical taper did nothing"
    _compare(state, obs, "vert_coord + rtps + outlier", chunks=[16, 48], loc="GC", vert_coord=vert, rtps=0.3, outlier_threshold=4.0)


@pytest.mark.parametrize("loc", [False, "GC"])
def test_float_inflation(loc):
    """`inflation=1.1` scales the caller's state in place (assimilation.py:62-69): each run gets its own copy."""
    from efa_xray_amd import EnSRF
    state = _state(10, 12)
    obs = _point_obs(state, 11, 30)
    ref_state, ref_obs = deepcopy(state), deepcopy(obs)
    ref_post, _ = EnSRF(ref_state, ref_obs, verbose=False, loc=loc, inflation=1.1).update()
    for cc in _chunk_settings(state.ny() * state.nx()):
        st, ob = deepcopy(state), deepcopy(obs)
        post, _ = EnSRF(st, ob, verbose=False, loc=loc, inflation=1.1, streamed=True, stream_chunk_cols=cc).update()
        assert _same_bits(post.to_vect(), ref_post.to_vect()), cc
        assert _same_bits(st.to_vect(), ref_state.to_vect()), "the inflated prior differs"
        for key in DIAG:
            assert _same_bits(_diag(ob)[key], _diag(ref_obs)[key]), key
    assert not _same_bits(ref_state.to_vect(), state.to_vect())


def test_user_defined_estimate_operator():
    from efa_xray_amd import Observation

    class MeanOfTwo(Observation):
        def estimate(self, state):
            x = state.to_vect()
            return 0.25 * x[self.r0] + 0.75 * x[self.r1]

    state = _state(12, 18)
    obs = _point_obs(state, 13, 30, cls=MeanOfTwo)
    rng = np.random.default_rng(14)
    for ob in obs:
        ob.r0, ob.r1 = (int(v) for v in rng.integers(0, state.nstate(), 2))
    for loc in (False, "GC"):
        ref = _compare(state, obs, "user-defined estimate loc=%r" % (loc,), loc=loc)
        assert not ref[3]._default_forward_operator()


# ---------------------------------------------------------------------------
# contract, cycling, memory, context hygiene
# ---------------------------------------------------------------------------
def _pinned(a):
    """True if the array is a view of a block of the context's page-locked memory."""
    while a is not None:
        if isinstance(a, _lib().PinnedBlock):
            return True
        a = getattr(a, "base", None)
    return False


def test_contract_of_the_posterior():
    from efa_xray_amd import EnSRF
    state = _state(20, 10)
    obs = _point_obs(state, 21, 24)
    X0 = state.to_vect().copy()
    ref = _run(state, obs, loc="GC")
    flt = EnSRF(state, deepcopy(obs), verbose=False, loc="GC", streamed=True, stream_chunk_cols=32)
    post, _ = flt.update()
    assert post is not state and _same_bits(state.to_vect(), X0)
    assert all(_pinned(v) for v in post.variables.values())
    for name, v in post.variables.items():
        assert v.flags["WRITEABLE"] and v.flags["C_CONTIGUOUS"] and v.shape == state.variables[name].shape
        assert v is not state.variables[name] and not np.shares_memory(v, state.variables[name])
    keep = post.to_vect().copy()
    assert _same_bits(keep, ref[1])
    del flt
    gc.collect()
    # a later cycle on the shared context (another shape, pooled and fresh blocks) leaves the arrays alone
    other = _state(22, 14, ny=7, nx=11)
    _run(other, _point_obs(other, 23, 12), loc=False, streamed=True, stream_chunk_cols=16)
    _run(state, obs, loc="GC", streamed=True, stream_chunk_cols=16)
    assert _same_bits(post.to_vect(), keep)
    first = post._first()
    first[...] = 1.5                                          # writable, and the write stays
    assert (post._first() == 1.5).all()
    # above the limit the posterior arrays are ordinary ones and the download is staged: the same bits
    post2, vect2, _, _ = _run(state, obs, loc="GC", streamed=True, stream_chunk_cols=32, stream_pinned_limit_mb=0)
    assert not any(_pinned(v) for v in post2.variables.values())
    assert _same_bits(vect2, ref[1])


@pytest.mark.parametrize("loc", [False, "GC"])
def test_two_cycles_with_the_posterior_fed_back(loc):
    """The posterior of a streamed update lies in page-locked memory: fed back as the next prior it takes the DMA path (and
    `pinned_copy` gives a first prior like that); two such cycles equal two unstreamed cycles bit for bit."""
    state = _state(30, 20)
    obs1, obs2 = _point_obs(state, 31, 30), _point_obs(state, 32, 30)
    ref1 = _run(state, obs1, loc=loc)
    ref2 = _run(ref1[0], obs2, loc=loc)
    for first in (state, state.pinned_copy()):
        assert _pinned(first._first()) == (first is not state)
        got1 = _run(first, obs1, loc=loc, streamed=True, stream_chunk_cols=32)
        assert all(_pinned(v) for v in got1[0].variables.values())
        got2 = _run(got1[0], obs2, loc=loc, streamed=True, stream_chunk_cols=32)
        _assert_equal_runs(ref1, got1, "cycle 1")
        _assert_equal_runs(ref2, got2, "cycle 2")
        assert _same_bits(got1[0].to_vect(), ref1[1]), "the fed-back prior was written"


def test_memory_bound_on_a_state_of_many_chunks():
    ny, nx, M = 13, 25, 24                                    # 325 columns: twenty blocks of 16 and a rest of 5
    state = _state(40, M, nvar=2, nt=3, ny=ny, nx=nx)
    obs = _point_obs(state, 41, 30)
    ref = _run(state, obs, loc="GC")
    got = _run(state, obs, loc="GC", streamed=True, stream_chunk_cols=16)
    _assert_equal_runs(ref, got, "21 chunks")
    plan = _lib().plan_chunks(ny * nx, 16)
    assert len(plan) >= 20
    stats = got[3].last_stream
    n_lead = state.nvars() * state.ntimes()
    largest = max(hi - lo for lo, hi in plan) * n_lead * M * 8
    state_bytes = state.nstate() * M * 8
    assert stats["chunks"] == len(plan)
    assert 0 < stats["peak_bytes"] <= 3 * largest
    assert stats["peak_bytes"] < state_bytes / 4
    assert stats["h2d_us"] > 0 and stats["d2h_us"] > 0 and stats["wall_us"] > 0
    t = got[3].last_timing
    assert t["state_ms"] > 0 and t["state_launches"] >= len(plan)   # the sum over the chunks


def _on_fresh_context(fn):
    lib = _lib()
    keep = lib._contexts.get(0)
    lib._contexts[0] = lib.Context(0)
    try:
        out = fn()
        gc.collect()
        return out
    finally:
        lib._contexts[0].close()
        if keep is not None:
            lib._contexts[0] = keep
        else:
            del lib._contexts[0]


def test_context_hygiene_streamed_unstreamed_streamed():
    state = _state(50, 16)
    obs = _point_obs(state, 51, 30)
    other = _state(52, 40, nvar=1, nt=1, ny=8, nx=9)
    other_obs = _point_obs(other, 53, 20)
    steps = [(state, obs, dict(loc="GC", streamed=True, stream_chunk_cols=16, rtps=0.5)),
             (other, other_obs, dict(loc=False)),
             (state, obs, dict(loc="GC", streamed=True, stream_chunk_cols=48)),
             (state, obs, dict(loc="GC")),
             (other, other_obs, dict(loc=False, streamed=True, stream_chunk_cols=32, outlier_threshold=2.0))]

    def values(st, ob, kw):
        r = _run(st, ob, **kw)
        return r[1].copy(), r[2]                              # (copies only: the posterior's memory goes with its context)

    shared = [values(*s) for s in steps]
    for i, s in enumerate(steps):
        fresh = _on_fresh_context(lambda: values(*s))
        assert _same_bits(shared[i][0], fresh[0]), "step %d: posterior differs from a fresh context's" % i
        for key in DIAG:
            assert _same_bits(shared[i][1][key], fresh[1][key]), "step %d: %s differs from a fresh context's" % (i, key)


def test_c_level_call_on_a_caller_stream():
    """efa_ensrf_cycle_host after efa_ctx_set_stream on a torch stream that has the caller's own work on it."""
    import torch
    from efa_xray_amd import EnSRF
    lib = _lib()
    state = _state(60, 20)
    obs = _point_obs(state, 61, 30)
    ref = _run(state, obs, loc="GC")
    flt = EnSRF(state, deepcopy(obs), verbose=False, loc="GC")
    ctx = flt._context()
    flt._configure(ctx)
    HX = flt.compute_ob_estimates()
    P, value, error, assim, lat, lon, hw = flt._ob_arrays(lib.LOC_GC)
    glat, glon = state.column_latlon()
    seg_prior = [state.variables[n] for n in state.vars()]
    seg_post = [np.empty_like(a) for a in seg_prior]
    stream = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda:0")
    with torch.cuda.stream(stream):
        for _ in range(20):
            a = torch.tanh(a @ a * 1e-3)                      # the caller's work, still running when the call is made
    ctx.set_stream(stream.cuda_stream)
    try:
        diag = ctx.ensrf_cycle_host(seg_prior, seg_post, state.ny() * state.nx(), state.nmems(), HX, 32, value, error, assim,
                                    lib.LOC_GC, lat, lon, hw, glat, glon)
    finally:
        ctx.use_own_stream()
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    got = np.concatenate([p.reshape(-1, state.nmems()) for p in seg_post])
    assert _same_bits(got, ref[1])
    for key in ("prior_mean", "prior_var"):
        assert _same_bits(diag[key], ref[2][key])
    done = diag["assimilated"]
    assert np.array_equal(done, ref[2]["assimilated"].astype(bool))
    for key in ("post_mean", "post_var"):
        assert _same_bits(diag[key][done], ref[2][key][done])
    # the library refuses what it cannot do: an adaptive-inflation field, a posterior over the prior, a chunk size below 1
    field = ctx.to_device(np.ones((state.nstate(), 2)))
    ctx.set_adaptive_inflation(field, state.nstate())
    try:
        with pytest.raises(lib.EfaError) as e:
            ctx.ensrf_cycle_host(seg_prior, seg_post, state.ny() * state.nx(), state.nmems(), HX, 32, value, error, assim,
                                 lib.LOC_GC, lat, lon, hw, glat, glon)
        assert e.value.status == lib.EFA_ERR_INVALID
    finally:
        ctx.set_adaptive_inflation(None)
    # (a posterior segment over ANY prior segment, or over another posterior segment, is refused as well)
    for bad_post, cc in ((seg_prior, 32), (seg_post, 0), ([seg_post[0], seg_prior[0]], 32), ([seg_post[0], seg_post[0]], 32)):
        with pytest.raises(lib.EfaError) as e:
            ctx.ensrf_cycle_host(seg_prior, bad_post, state.ny() * state.nx(), state.nmems(), HX, cc, value, error, assim,
                                 lib.LOC_GC, lat, lon, hw, glat, glon)
        assert e.value.status == lib.EFA_ERR_INVALID
    assert _same_bits(np.concatenate([p.reshape(-1, state.nmems()) for p in seg_prior]), state.to_vect())
    ptr = ctypes.c_void_p(12345)
    assert ctx.lib.efa_pinned_free(ctx.handle, ptr) == lib.EFA_ERR_INVALID    # not a block of this context
