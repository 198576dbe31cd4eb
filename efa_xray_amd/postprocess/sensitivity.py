"""Ensemble sensitivity and greedy observation targeting (Ancell & Hakim 2007, Torn & Hakim 2008).

Asked before observations are taken.  Given a forecast ensemble (an `EnsembleState` carries every valid time) and the members'
values of K forecast metrics J_k, `ensemble_sensitivity` returns for every state element i

    var_i = x'_i.x'_i/(M-1)    cov_ik = x'_i.J'_k/(M-1)    sens_ik = cov_ik/var_i    corr_ik = cov_ik/sqrt(var_i var(J_k))

(primes: deviations from the ensemble mean), and `observation_targets` picks, one after the other, the elements whose observation
would reduce sum_k w_k var(J_k) most, each pick conditioning every statistic on the ones before by the exact, unlocalised Kalman
update.  Every statistic uses 1/(M-1): this is a product of its own, not the mixed convention of the reference's EnSRF loop.  The
contraction over the state runs on the device (`efa_sensitivity_dev` / `efa_sensitivity_f32_dev`); there is no NumPy path.
"""
import numpy as np

from efa_xray_amd import _lib
from efa_xray_amd.assimilation.assimilation import Assimilation

MAX_VECTORS = 32   # K + n_targets at most (two matrix-core tiles of 16 vectors)
MAX_MEMBERS = 256


def _metrics(state, metrics):
    """(names or None, J (K, M) float64) from an array (K, M) / (M,) or a mapping name -> (M,)."""
    M = state.nmems()
    names = None
    if hasattr(metrics, "items"):
        names = list(metrics.keys())
        rows = []
        for name in names:
            v = np.asarray(metrics[name], dtype=np.float64)
            if v.shape != (M,):
                raise ValueError("metrics[%r] has shape %r, expected (%d,): one value per member" % (name, v.shape, M))
            rows.append(v)
        J = np.array(rows, dtype=np.float64).reshape(len(rows), M)
    else:
        try:
            J = np.asarray(metrics, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("metrics must be an array (K, nmems) or a mapping from a name to an array (nmems,)")
        if J.ndim == 1:
            J = J[None, :]
        if J.ndim != 2 or J.shape[1] != M:
            raise ValueError("metrics has shape %r, expected (K, %d): one row per metric, one value per member" % (J.shape, M))
    if J.shape[0] < 1:
        raise ValueError("at least one metric is needed")
    if not np.all(np.isfinite(J)):
        raise ValueError("metrics must be finite")
    return names, np.ascontiguousarray(J)


def _check_state(state, K, n_targets):
    dt = state.dtype     # (raises ValueError when the variables mix dtypes)
    if state.nvars() < 1:
        raise ValueError("the state has no variables")
    M = state.nmems()
    if M < 2 or M > MAX_MEMBERS:
        raise ValueError("the state has %d members, supported are 2 to %d" % (M, MAX_MEMBERS))
    if K + n_targets > MAX_VECTORS:
        raise ValueError("%d metrics and %d targets: K + n_targets may be %d at most" % (K, n_targets, MAX_VECTORS))
    return dt


def _run(state, J, slab_error, weights, cand, n_targets, want, device):
    """One library call; `want`: the names of the fields to bring back.  Returns (fields dict, picked_row, picked_score, metric_var)."""
    nvar, nt, ny, nx, M = state.shape()
    K = J.shape[0]
    N, ncol = state.nstate(), ny * nx
    ctx = _lib.get_context(device)
    X = Assimilation(state, [], device=device)._upload_prior(ctx)
    shapes = dict(var=(N,), score=(N,), cov=(K, N), sens=(K, N), corr=(K, N), dvar=(K, N))
    dev = dict((name, ctx.empty(shapes[name])) for name in want)
    d_cand = None
    try:
        if cand is not None:
            d_cand = ctx.malloc_bytes(max(N, 1))
            ctx.h2d(d_cand, np.ascontiguousarray(cand, dtype=np.uint8))
        prow, psc, mv = ctx.sensitivity(N, M, X, J, slab_error, ncol=ncol, n_lead=nvar * nt, weights=weights, cand=d_cand,
                                        n_targets=n_targets, **dev)
        out = {}
        for name in want:
            lead = (K,) if len(shapes[name]) == 2 else ()
            out[name] = dev[name].download().reshape(lead + (nvar, nt, ny, nx))
    finally:
        if d_cand is not None:
            ctx.free_bytes(d_cand)
        for a in dev.values():
            a.free()
        X.free()
    return out, prow, psc, mv


def ensemble_sensitivity(state, metrics, device=0):
    """The classical ensemble-sensitivity fields of K forecast metrics to every state element.

    state   -- an `EnsembleState`, stored as float64 or float32 (every number is computed in float64)
    metrics -- array (K, nmems) (or (nmems,) for one metric), or a mapping name -> (nmems,): the members' values of the metrics
    device  -- HIP device ordinal

    Returns a dict: `var` (nvar, ntimes, ny, nx), the ensemble variance; `cov`, `sens` (the regression slope dJ_k/dx_i) and
    `corr`, each (K, nvar, ntimes, ny, nx); `metric_var` (K,); `names` (the mapping's keys, or None).  Where a denominator is 0
    the value is exactly 0.0; an element with a non-finite member has NaN fields."""
    names, J = _metrics(state, metrics)
    _check_state(state, J.shape[0], 0)
    slab_error = np.ones(state.nvars() * state.ntimes())     # (the error enters no field asked for here)
    out, _, _, mv = _run(state, J, slab_error, None, None, 0, ("var", "cov", "sens", "corr"), device)
    out["metric_var"] = mv[0].copy()
    out["names"] = names
    return out


def observation_targets(state, metrics, n_targets, ob_error, candidates=None, weights=None, device=0):
    """Greedy observation targeting: where would the next `n_targets` observations reduce the metrics' variance most.

    state      -- an `EnsembleState` (float64 or float32)
    metrics    -- as in `ensemble_sensitivity`
    n_targets  -- picks to make, >= 0, with K + n_targets <= 32
    ob_error   -- mapping variable name -> error variance (finite, > 0) of a hypothetical observation of that variable; every
                  variable of the state must be named
    candidates -- None (every element), or mapping variable name -> boolean array broadcastable to (ntimes, ny, nx): where an
                  observation could be taken.  A variable that is not named is no candidate
    weights    -- None (all 1), or (K,) finite non-negative weights of the metrics (a mapping name -> weight when `metrics` is one)
    device     -- HIP device ordinal

    Returns a dict: `targets`, a list of dicts (row, var, time, y, x, lat, lon, score) in pick order -- `time` the valid time,
    `score` the expected reduction of sum_k w_k var(J_k) by that observation, given the picks before it; the list is shorter
    than `n_targets` when no candidate is left with a score > 0; `metric_var` (n_targets + 1, K), var(J_k) after 0 ..
    n_targets picks; and, conditioned on all picks, the fields `score` (nvar, ntimes, ny, nx) (0.0 where no candidate) and
    `dvar` (K, nvar, ntimes, ny, nx) = -cov^2/(var + error), what one more observation there would do to each var(J_k)."""
    names, J = _metrics(state, metrics)
    K = J.shape[0]
    try:
        n = int(n_targets)
    except (TypeError, ValueError):
        raise ValueError("n_targets=%r is not an integer" % (n_targets,))
    if n != n_targets or n < 0:
        raise ValueError("n_targets=%r must be an integer >= 0" % (n_targets,))
    _check_state(state, K, n)
    nvar, nt, ny, nx, M = state.shape()
    want = (nt, ny, nx)
    if not hasattr(ob_error, "get"):
        raise ValueError("ob_error must be a mapping from variable name to an error variance")
    slab_error = np.empty(nvar * nt)
    for iv, name in enumerate(state.vars()):
        if ob_error.get(name) is None:
            raise ValueError("ob_error names no error variance for variable %r" % name)
        try:
            r = float(ob_error[name])
        except (TypeError, ValueError):
            raise ValueError("ob_error[%r]=%r is not a number" % (name, ob_error[name]))
        if not (np.isfinite(r) and r > 0.0):
            raise ValueError("ob_error[%r]=%r must be finite and > 0" % (name, r))
        slab_error[iv * nt:(iv + 1) * nt] = r
    for name in ob_error.keys():
        if name not in state.variables:
            raise ValueError("ob_error names %r, which is no variable of the state %r" % (name, state.vars()))
    w = None
    if weights is not None:
        if hasattr(weights, "get"):
            if names is None:
                raise ValueError("weights is a mapping but metrics is not: give weights as an array (K,)")
            for name in weights.keys():
                if name not in names:
                    raise ValueError("weights names %r, which is no metric %r" % (name, names))
            w = np.array([float(weights.get(name, 1.0)) for name in names], dtype=np.float64)
        else:
            w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.shape != (K,):
            raise ValueError("weights has %d entries for %d metrics" % (w.size, K))
        if not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError("weights must be finite and >= 0")
    cand = None
    if candidates is not None:
        if not hasattr(candidates, "get"):
            raise ValueError("candidates must be None or a mapping from variable name to a boolean array")
        for name in candidates.keys():
            if name not in state.variables:
                raise ValueError("candidates names %r, which is no variable of the state %r" % (name, state.vars()))
        cand = np.zeros((nvar,) + want, dtype=np.uint8)
        for iv, name in enumerate(state.vars()):
            if candidates.get(name) is None:
                continue
            try:
                cand[iv] = np.broadcast_to(np.asarray(candidates[name]).astype(bool), want)
            except ValueError:
                raise ValueError("candidates[%r] has shape %r, not broadcastable to (ntimes, ny, nx) = %r"
                                 % (name, np.shape(candidates[name]), want))
        cand = cand.reshape(-1)

    out, prow, psc, mv = _run(state, J, slab_error, w, cand, n, ("score", "dvar"), device)
    lat, lon = state.column_latlon()
    times = np.asarray(state.ensemble_times())
    vars_ = state.vars()
    targets = []
    for row, sc in zip(prow, psc):
        if row < 0:
            break
        iv, it, iy, ix = np.unravel_index(int(row), (nvar, nt, ny, nx))
        targets.append(dict(row=int(row), var=vars_[iv], time=times[it], y=int(iy), x=int(ix), lat=float(lat[iy * nx + ix]),
                            lon=float(lon[iy * nx + ix]), score=float(sc)))
    out["targets"] = targets
    out["metric_var"] = mv
    out["names"] = names
    return out
