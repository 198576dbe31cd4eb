"""The probability-matched ensemble mean (Ebert 2001) and its patch-wise, "localised" form (Clark 2017; Snook et al. 2019;
DESIGN.md 7s).

The plain ensemble mean of a precipitation-like field smears the maxima and inflates the area of light amounts.  The
probability-matched mean keeps the mean's spatial pattern and takes its amplitudes from the members: within a patch of one
(variable, time) slab the n elements are ranked by a rank field (the ensemble mean unless another is given), the n*M member
values are pooled and sorted, and the element at rank r gets pooled value r*M + g.  `probability_matched_mean` does that on the
device (`efa_pm_mean_dev` / `efa_pm_mean_f32_dev`, a segmented radix sort; there is no NumPy path).  The result is a selection of
member values: no arithmetic is done on them.

A patch needs the whole (y, x) grid on one device: a column-sharded state is not supported, gather it first.
"""
import numpy as np

from efa_xray_amd import _lib
from efa_xray_amd.assimilation.assimilation import Assimilation
from efa_xray_amd.postprocess.products import _check_state

PICKS = ("min", "mid", "max")


def _check_args(state, variables, patch, pick, rank_field):
    """(names, slab_on (nvar*nt,) int32, (py, px), g, {name: float64 (nt, ny, nx)})."""
    _check_state(state)
    nvar, nt, ny, nx, M = state.shape()
    if variables is None:
        names = list(state.vars())
    else:
        if isinstance(variables, str):
            variables = (variables,)
        try:
            names = list(variables)
        except TypeError:
            raise ValueError("variables must be None or a sequence of variable names")
        for name in names:
            if name not in state.variables:
                raise ValueError("variables names %r, which is no variable of the state %r" % (name, state.vars()))
        if len(set(names)) != len(names):
            raise ValueError("variables names a variable twice: %r" % (names,))
        names = [name for name in state.vars() if name in names]
    on = np.zeros((nvar, nt), dtype=np.int32)
    for iv, name in enumerate(state.vars()):
        if name in names:
            on[iv] = 1
    if patch is None:
        py, px = ny, nx
    else:
        try:
            raw = np.asarray(tuple(patch))
        except TypeError:
            raise ValueError("patch must be None or (py, px)")
        if raw.shape != (2,) or raw.dtype.kind not in "iuf" or not np.all(np.isfinite(raw)) or np.any(raw != np.floor(raw)):
            raise ValueError("patch must be None or two integers (py, px), got %r" % (patch,))
        py, px = int(raw[0]), int(raw[1])
        if py < 1 or py > ny or px < 1 or px > nx:
            raise ValueError("patch=(%d, %d) must lie in [1, ny = %d] x [1, nx = %d]" % (py, px, ny, nx))
    if isinstance(pick, str):
        if pick not in PICKS:
            raise ValueError("pick=%r must be 'min', 'mid', 'max' or an integer in [0, M)" % (pick,))
        g = {"min": 0, "mid": M // 2, "max": M - 1}[pick]
    else:
        if isinstance(pick, bool) or not isinstance(pick, (int, np.integer)):
            raise ValueError("pick=%r must be 'min', 'mid', 'max' or an integer in [0, M)" % (pick,))
        g = int(pick)
        if g < 0 or g >= M:
            raise ValueError("pick=%d must lie in [0, M = %d)" % (g, M))
    fields = {}
    if rank_field is not None:
        if not hasattr(rank_field, "get"):
            raise ValueError("rank_field must be None or a mapping from variable name to an array (ntimes, ny, nx)")
        for name in rank_field.keys():
            if name not in state.variables:
                raise ValueError("rank_field names %r, which is no variable of the state %r" % (name, state.vars()))
            try:
                f = np.asarray(rank_field.get(name), dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("rank_field[%r] is not an array of numbers" % name)
            if f.shape != (nt, ny, nx):
                raise ValueError("rank_field[%r] has shape %r, expected %r" % (name, f.shape, (nt, ny, nx)))
            fields[name] = f
    return names, on.reshape(-1), (py, px), g, fields


def probability_matched_mean(state, variables=None, patch=None, pick="mid", rank_field=None, device=0):
    """The probability-matched mean of the variables of an ensemble state.

    state      -- an `EnsembleState`, stored as float64 or float32, whole on one device (a column-sharded state is not supported)
    variables  -- the names to process (None: all); the other variables are not read and are left out of the result
    patch      -- None (one pool per (variable, time) slab: the classic PM mean) or (py, px): the grid is cut into patches of
                  py x px points (smaller at the upper edges), each with a pool of its own
    pick       -- which of the M pooled values of a rank: 'mid' (M // 2), 'max' (M - 1, Ebert's: the PM maximum is the pooled
                  maximum), 'min' (0) or an integer in [0, M)
    rank_field -- None: the elements are ranked by the ensemble mean (`ensemble_products`' mean, from the same upload); or a
                  mapping variable name -> (ntimes, ny, nx), e.g. a smoothed mean; a variable that is missing falls back to
                  the mean
    device     -- HIP device ordinal

    Returns a dict: `pm_mean` and `rank_field`, mappings variable name -> (ntimes, ny, nx) float64; `n_bad`, variable name ->
    (ntimes,) int64; `patch` (py, px) and `pick` g.  Within a patch, ties of the rank field go by grid index and -0.0 ranks as
    +0.0.  An element whose rank value or one of whose members is not finite is NaN, enters no pool and is counted in n_bad.
    For a float32 state the result is the selected float32 member, widened."""
    names, on, (py, px), g, fields = _check_args(state, variables, patch, pick, rank_field)
    nvar, nt, ny, nx, M = state.shape()
    N = state.nstate()
    out = {"pm_mean": {}, "rank_field": {}, "n_bad": {}, "patch": (py, px), "pick": g}
    if not names:
        return out
    ctx = _lib.get_context(device)
    X = Assimilation(state, [], device=device)._upload_prior(ctx)
    d_f = d_pm = None
    try:
        d_f = ctx.empty((N,))
        if any(name not in fields for name in names):
            ctx.products(N, M, X, ncol=ny * nx, n_lead=nvar * nt, mean=d_f)
        if fields:
            f = d_f.download().reshape(nvar, nt, ny, nx)
            for iv, name in enumerate(state.vars()):
                if name in fields:
                    f[iv] = fields[name]
            d_f.free()
            d_f = None
            d_f = ctx.to_device(f.reshape(-1))
        d_pm = ctx.empty((N,))
        n_bad = ctx.pm_mean(N, M, X, ny, nx, nvar * nt, d_f, d_pm, slab_on=on, patch=(py, px), pick=g).reshape(nvar, nt)
        pm = d_pm.download().reshape(nvar, nt, ny, nx)
        f = d_f.download().reshape(nvar, nt, ny, nx)
    finally:
        for a in (d_f, d_pm):
            if a is not None:
                a.free()
        X.free()
    for iv, name in enumerate(state.vars()):
        if name in names:
            out["pm_mean"][name] = pm[iv].copy()
            out["rank_field"][name] = f[iv].copy()
            out["n_bad"][name] = n_bad[iv].copy()
    return out
