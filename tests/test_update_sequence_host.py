"""What every update path asks of its context, without a GPU: the ordered `Context` calls of `EnSRF.update` (unlocalised, GC,
adaptive inflation with the device forward operator and with a user `estimate`, a float32 state, streamed), `update_arrays`,
`ETKF`, `LETKF` (plain and with a weight_stride) and `SlabLETKF`, with their scalar arguments and the shapes and dtypes of their
arrays, interleaved with the verbose lines the filters print.  The context is a recording stand-in handed over by overriding
`_context`; it returns plausible arrays.  State: 2 vars x 2 times x 3 x 5, M = 4, P = 3 with one ob not assimilated."""
import numpy as np
import pytest

NVAR, NT, NY, NX, M, P = 2, 2, 3, 5, 4, 3
N = NVAR * NT * NY * NX


def _describe(v):
    if isinstance(v, _Dev):
        return "dev:" + _describe(np.empty(v.shape, v.dtype))
    if isinstance(v, np.ndarray):
        return "%s[%s]" % (v.dtype.str[1:], ",".join(str(s) for s in v.shape))
    if isinstance(v, np.generic):
        return repr(v.item())
    if isinstance(v, (np.dtype, type)):
        return np.dtype(v).name
    if isinstance(v, (list, tuple)):
        return "[%s]" % ", ".join(_describe(x) for x in v)
    if isinstance(v, dict):
        return "{%s}" % ", ".join("%s=%s" % (k, _describe(v[k])) for k in sorted(v))
    return repr(v)


class _Dev(object):
    """What `Context.empty` / `to_device` hand back: a shape and a dtype; downloads give zeros."""

    def __init__(self, shape, dtype):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(np.float64 if dtype is None else dtype)

    def upload_rows(self, r0, host):
        assert np.asarray(host).dtype == self.dtype

    def download_rows_into(self, r0, out):
        assert out.dtype == self.dtype
        out[...] = 0
        return out

    def download(self):
        return np.zeros(self.shape, self.dtype)


class _Context(object):
    """Records every call made on it as one line of `log`; `say` takes the filters' print calls into the same list."""

    def __init__(self):
        self.log = []

    def say(self, *words):
        self.log.append("print " + " ".join(str(w) for w in words))

    def _diag(self):
        return dict(prior_mean=np.arange(P, dtype=np.float64), prior_var=np.ones(P), post_mean=np.full(P, 0.5),
                    post_var=np.full(P, 0.25), assimilated=np.array([True, True, False]))

    def _answer(self, name, a, k):
        if name == "empty":
            return _Dev(a[0], a[1] if len(a) > 1 else k.get("dtype"))
        if name == "to_device":
            return _Dev(np.shape(a[0]), a[1] if len(a) > 1 else k.get("dtype"))
        if name == "interp_stencils":      # every ob reads the first eight rows of its variable, equally weighted
            return np.tile(np.arange(8, dtype=np.int64), (P, 1)), np.full((P, 8), 0.125), np.zeros(P, dtype=np.uint8)
        if name == "pinned_reserve":
            return True
        if name == "pinned_empty":
            return np.empty(a[0], a[1])
        if name == "letkf_slab_groups":
            return np.arange(a[0], dtype=np.int32) % 2, 2
        if name in ("ensrf_cycle", "ensrf_cycle_host", "obs_phase", "ensrf_update_host", "letkf_cycle"):
            return self._diag()
        if name == "last_timing":
            return dict(obs_ms=1.0)
        if name == "stream_stats":
            return dict(chunks=1)
        if name == "etkf_solution":
            return dict(T=None, w=None, eigenvalues=np.zeros(M), n_active=2, q=0.0, dfs=1.0, chi2=2.0, sweeps=3)
        return None

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*a, **k):
            words = [_describe(x) for x in a] + ["%s=%s" % (key, _describe(k[key])) for key in sorted(k)]
            self.log.append("%s(%s)" % (name, ", ".join(words)))
            return self._answer(name, a, k)
        return call


def _state(dtype=None):
    from efa_xray_amd import EnsembleState
    rng = np.random.default_rng(0)
    lat, lon = np.meshgrid(np.linspace(30, 40, NY), np.linspace(250, 260, NX), indexing="ij")
    return EnsembleState.from_array(rng.standard_normal((NVAR, NT, NY, NX, M)), lat, lon, dtype=dtype)


def _obs(cls=None, **extra):
    from efa_xray_amd import Observation
    cls = cls or Observation
    return [cls(value=0.1 * k, obtype="var%d" % (k % 2), time=k % 2, error=1.0 + k, lat=33.0 + k, lon=252.0 + k,
                assimilate_this=k != 2, localize_radius=500.0 + k, **extra) for k in range(P)]


def _run(monkeypatch, cls, state, obs, call=None, **kw):
    """The log of one update on a filter of class `cls`; checks what the update hands back on the way."""
    import efa_xray_amd.assimilation.ensrf as ensrf_mod
    import efa_xray_amd.assimilation.letkf as letkf_mod
    ctx = _Context()
    for mod in (ensrf_mod, letkf_mod):
        monkeypatch.setattr(mod, "print", ctx.say, raising=False)
    f = cls(state, obs, verbose=True, **kw)
    monkeypatch.setattr(f, "_context", lambda: ctx, raising=False)
    if call is not None:
        call(f)
    else:
        post, out = f.update()
        assert out is obs and post is not state and type(post) is type(state)
        assert post.shape() == f.prior.shape() and post.dtype == f.prior.dtype
        assert f.last_timing == dict(obs_ms=1.0)
    assert [ob.assimilated for ob in obs] == [True, True, False]
    assert [ob.prior_mean for ob in obs] == [0.0, 1.0, 2.0] and [ob.prior_var for ob in obs] == [1.0] * 3
    assert [ob.post_mean for ob in obs] == [0.5, 0.5, None] and [ob.post_var for ob in obs] == [0.25, 0.25, None]
    assert all(type(ob.prior_mean) is np.float64 for ob in obs)
    return f, ctx.log


def _configure(solver=(), vertical="None", slab="None", outlier="None", relax="0, 0.0"):
    return ["set_option('path', 0)", "set_option('obs_solver', 0)", "set_relaxation(%s)" % relax, "set_adaptive_inflation(None)",
            "set_outlier_threshold(%s)" % outlier, "set_sampling_error_correction(None)",
            "set_vertical_localization(%s)" % vertical, "set_slab_localization(%s)" % slab] + list(solver)


OB_NONE = "f8[3], f8[3], b1[3], 0, None, None, None"
OB_GC = "f8[3], f8[3], b1[3], 1, f8[3], f8[3], f8[3]"
DEVICE_FO = ["interp_stencils(2, 2, 3, 5, f8[3,5], f8[3,5], f8[2], [0, 1, 0], f8[3], [33.0, 34.0, 35.0], [252.0, 253.0, 254.0], "
             "want_host=False)", "empty([3, 4])", "forward_interp(15, 0, 15, 4, 4, dev:f8[60,4], dev:f8[3,4])"]
HOST_FO = ["interp_stencils(2, 2, 3, 5, f8[3,5], f8[3,5], f8[2], [0, 1, 0], f8[3], [33.0, 34.0, 35.0], [252.0, 253.0, 254.0], "
           "want_host=True)", "to_device(f8[8,4])", "empty([3, 4])",
           "forward_stencil(8, 0, 4, dev:f8[8,4], i8[3,8], f8[3,8], dev:f8[3,4])"]
PERTS = ["form_perts(3, 4, dev:f8[3,4], dev:f8[3], dev:f8[3,4])"]
HEAD = ["print Beginning update sequence"]
UPLOAD = ["set_option('timing', 1)", "print Converting state to vector", "empty([60, 4], float64)",
          "print Computing observation priors", "empty([3])"]
UPLOAD_F32 = [UPLOAD[0], UPLOAD[1], "empty([60, 4], float32)"] + UPLOAD[3:]
TAIL = ["last_timing()", "print Formatting posterior"]


def test_ensrf_unlocalised(monkeypatch):
    _, log = _run(monkeypatch, __import__("efa_xray_amd").EnSRF, _state(), _obs())
    assert log == HEAD + _configure() + UPLOAD + DEVICE_FO + PERTS + [
        "print Beginning observation loop",
        "ensrf_cycle(60, 4, 3, dev:f8[60,4], dev:f8[60,4], dev:f8[3], dev:f8[3,4], %s, None, None, 1)" % OB_NONE] + TAIL


def test_ensrf_gc_with_every_setting(monkeypatch):
    """loc='GC' with obs_batch, path, rtps, an outlier threshold, vert_coord and time_localize: each reaches its setter."""
    from efa_xray_amd import EnSRF
    obs = _obs(vert=500.0, vert_localize_radius=100.0)
    _, log = _run(monkeypatch, EnSRF, _state(), obs, loc="GC", obs_batch=8, path="sweep", rtps=0.9, outlier_threshold=3.0,
                  vert_coord=np.full((NVAR, NT), 500.0), time_localize=True)
    conf = _configure(relax="2, 0.9", outlier="3.0", vertical="f8[4], f8[3], f8[3]",
                      slab="P=3, lead_time=f8[4], n_lead=4, ob_time=f8[3], ob_time_halfwidth=f8[3]")
    conf[0] = "set_option('path', 1)"
    assert log == HEAD + ["set_option('obs_batch', 8)"] + conf + UPLOAD + DEVICE_FO + PERTS + [
        "print Beginning observation loop",
        "ensrf_cycle(60, 4, 3, dev:f8[60,4], dev:f8[60,4], dev:f8[3], dev:f8[3,4], %s, f8[15], f8[15], 4)" % OB_GC] + TAIL


def _adaptive(state):
    from efa_xray_amd.assimilation.adaptive_inflation import AdaptiveInflation
    return AdaptiveInflation(state, ("adaptive", None, (1.1, 0.6)))


ADAPTIVE_CYCLE = [
    "print Beginning observation loop", "set_adaptive_inflation(dev:f8[60,2], 60, 1.0, 1000000.0, 0.0)",
    "ensrf_cycle(60, 4, 3, dev:f8[60,4], dev:f8[60,4], dev:f8[3], dev:f8[3,4], %s, f8[15], f8[15], 4)" % OB_GC,
    "set_adaptive_inflation(None)"] + TAIL


def test_ensrf_adaptive_with_the_device_forward_operator(monkeypatch):
    from efa_xray_amd import EnSRF
    state = _state()
    f, log = _run(monkeypatch, EnSRF, state, _obs(), loc="GC", adaptive_inflation=_adaptive(state))
    assert log == HEAD + _configure() + UPLOAD[:2] + [
        "to_device(f8[60,2])", "empty([60, 4], float64)", "inflate_rows(60, 4, dev:f8[60,4], dev:f8[60,2])"
    ] + UPLOAD[3:] + DEVICE_FO + PERTS + ADAPTIVE_CYCLE
    assert not f.adaptive_inflation.inflation.to_vect().any()       # the field the stand-in "downloaded"


def test_ensrf_adaptive_with_a_user_estimate(monkeypatch):
    """A user operator reads the inflated state object, which is also what is uploaded; self.prior is put back."""
    from efa_xray_amd import EnSRF, Observation
    seen = []

    class Mine(Observation):
        def estimate(self, state):
            seen.append(state)
            return state.variables[self.obtype][0, 0, 0]

    state = _state()
    f, log = _run(monkeypatch, EnSRF, state, _obs(Mine), loc="GC", adaptive_inflation=_adaptive(state))
    assert log == HEAD + _configure() + UPLOAD[:2] + ["to_device(f8[60,2])"] + UPLOAD[2:] + ["to_device(f8[3,4])"] + PERTS \
        + ADAPTIVE_CYCLE
    assert len(seen) == P and all(s is not state for s in seen) and f.prior is state


def test_float32_state_with_inflation(monkeypatch):
    from efa_xray_amd import EnSRF
    _, log = _run(monkeypatch, EnSRF, _state(np.float32), _obs(), loc="GC", inflation=1.5)
    assert log == HEAD + ["print Inflating Prior State"] + _configure() + UPLOAD_F32 + HOST_FO + ["to_device(f8[3,4])"] + PERTS + [
        "print Beginning observation loop", "obs_phase(4, 3, dev:f8[3], dev:f8[3,4], %s)" % OB_GC,
        "state_cycle_f32(60, 4, dev:f4[60,4], dev:f4[60,4], f8[15], f8[15], 4)", "synchronize()"] + TAIL


@pytest.mark.parametrize("dtype,chunk", [(None, None), (np.float32, 16)])
def test_streamed(monkeypatch, dtype, chunk):
    from efa_xray_amd import EnSRF
    state = _state(dtype)
    el = "f4" if dtype else "f8"
    f, log = _run(monkeypatch, EnSRF, state, _obs(), loc="GC", streamed=True, stream_chunk_cols=chunk, inflation=1.5)
    cols = 16 if chunk else (64 << 20) // (NVAR * NT * M * 8) // 16 * 16
    assert log == HEAD + ["print Inflating Prior State"] + _configure() + [
        "set_option('timing', 1)", "print Computing observation priors"] + HOST_FO + [
        "pinned_reserve([%d, %d], 4294967296)" % ((N // NVAR * M * (4 if dtype else 8),) * 2),
        "pinned_empty([2, 3, 5, 4], float%d)" % (32 if dtype else 64),
        "pinned_empty([2, 3, 5, 4], float%d)" % (32 if dtype else 64), "print Beginning observation loop",
        "ensrf_cycle_host([{0}[2,3,5,4], {0}[2,3,5,4]], [{0}[2,3,5,4], {0}[2,3,5,4]], 15, 4, f8[3,4], {1}, {2}, f8[15], f8[15])"
        .format(el, cols, OB_GC), "last_timing()", "stream_stats()", "print Formatting posterior"]
    assert f.last_stream == dict(chunks=1)


def test_update_arrays(monkeypatch):
    from efa_xray_amd import EnSRF
    xbm, Xbp = np.zeros(N + P), np.ones((N + P, M))
    got = []
    _, log = _run(monkeypatch, EnSRF, _state(), _obs(), call=lambda f: got.extend(f.update_arrays(xbm, Xbp)), loc="GC")
    assert log == _configure() + ["ensrf_update_host(f8[63], f8[63,4], 60, %s, f8[15], f8[15], 4)" % OB_GC]
    assert got[0] is not xbm and got[0].shape == xbm.shape and got[1] is not Xbp and got[1].shape == Xbp.shape


def test_etkf(monkeypatch):
    from efa_xray_amd import ETKF
    f, log = _run(monkeypatch, ETKF, _state(), _obs())
    assert log == HEAD + _configure(solver=["set_option('obs_solver', 1)"]) + UPLOAD + DEVICE_FO + PERTS + [
        "print Beginning observation loop",
        "ensrf_cycle(60, 4, 3, dev:f8[60,4], dev:f8[60,4], dev:f8[3], dev:f8[3,4], %s, None, None, 1)" % OB_NONE] + TAIL + [
        "etkf_solution(4)"]
    assert sorted(f.last_solve) == ["chi2", "dfs", "eigenvalues", "n_active", "sweeps"]


LETKF_OB = "f8[3], f8[3], b1[3], f8[3], f8[3], f8[3]"


@pytest.mark.parametrize("dtype", [None, np.float32])
def test_letkf(monkeypatch, dtype):
    from efa_xray_amd import LETKF
    el = "f4" if dtype else "f8"
    f, log = _run(monkeypatch, LETKF, _state(dtype), _obs(), rtpp=0.5)
    assert log == HEAD + _configure(relax="1, 0.5") + (UPLOAD_F32 + HOST_FO + ["to_device(f8[3,4])"] if dtype else UPLOAD + DEVICE_FO) \
        + PERTS + ["print Beginning the column solves", "empty([15, 3])",
                   "letkf_cycle(60, 4, 3, dev:{0}[60,4], dev:{0}[60,4], dev:f8[3], dev:f8[3,4], {1}, f8[15], f8[15], 4, _slab=False, "
                   "col_stats=dev:f8[15,3], f32={2})".format(el, LETKF_OB, bool(dtype))] + TAIL
    assert sorted(f.last_solve) == ["dfs", "n_local", "sweeps"] and f.last_solve["dfs"].shape == (NY, NX)


def test_letkf_with_a_weight_stride(monkeypatch):
    from efa_xray_amd import LETKF
    f, log = _run(monkeypatch, LETKF, _state(), _obs(), weight_stride=2)
    assert log == HEAD + _configure() + UPLOAD + DEVICE_FO + PERTS + [
        "print Beginning the column solves", "empty([6, 3])",
        "letkf_cycle(60, 4, 3, dev:f8[60,4], dev:f8[60,4], dev:f8[3], dev:f8[3,4], %s, f8[15], f8[15], 4, _slab=False, "
        "col_stats=dev:f8[6,3], f32=False, shape=[3, 5], stride=[2, 2])" % LETKF_OB] + TAIL
    assert f.last_solve["n_local"].shape == (2, 3)
    assert list(f.last_solve["node_y"]) == [0, 2] and list(f.last_solve["node_x"]) == [0, 2, 4]


def _slab_run(monkeypatch, fail=False):
    from efa_xray_amd import SlabLETKF
    obs = _obs(vert=500.0, vert_localize_radius=100.0)
    if fail:
        monkeypatch.setattr(_Context, "_diag", lambda self: 1 / 0)
    return _run(monkeypatch, SlabLETKF, _state(), obs, vert_coord=np.full((NVAR, NT), 500.0), var_impact={"var0": {"var1": 0.5}})


SLAB = _configure(vertical="f8[4], f8[3], f8[3]", slab="P=3, impact=f8[1,2], lead_var=i4[4], n_lead=4, ob_group=i4[3], ob_var=i4[3]") \
    + UPLOAD + DEVICE_FO + PERTS + [
        "print Beginning the column solves", "letkf_slab_groups(4)", "empty([30, 3])",
        "letkf_cycle(60, 4, 3, dev:f8[60,4], dev:f8[60,4], dev:f8[3], dev:f8[3,4], %s, f8[15], f8[15], 4, _slab=True, "
        "col_stats=dev:f8[30,3], f32=False)" % LETKF_OB, "set_vertical_localization(None)", "set_slab_localization(None)"]


def test_slab_letkf(monkeypatch):
    f, log = _slab_run(monkeypatch)
    assert log == HEAD + SLAB + TAIL
    assert f.last_solve["sweeps"].shape == (2, NY, NX) and f.last_solve["group_of_slab"].tolist() == [[0, 1], [0, 1]]


def test_slab_letkf_resets_its_settings_when_the_cycle_fails(monkeypatch):
    log = []
    monkeypatch.setattr(_Context, "__init__", lambda self: setattr(self, "log", log))
    with pytest.raises(ZeroDivisionError):
        _slab_run(monkeypatch, fail=True)
    assert log == HEAD + SLAB
