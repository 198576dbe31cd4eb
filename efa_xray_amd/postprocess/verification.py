"""Ensemble verification against a gridded verifying state (Hamill 2001, Hersbach 2000, Ferro 2014).

Asked once a verifying analysis exists: is the ensemble calibrated, and did the update make it better?  For every verified state
element with members x_1..x_M and verifying value y, `ensemble_verification` forms on the device (`efa_verify_dev` /
`efa_verify_f32_dev`; there is no NumPy path) the rank of y among the members (ties broken by a hash of (seed, element)), the
CRPS of the ensemble, the error of its mean and its variance, and returns per group of elements the rank histogram and the
weighted means of the three.
"""
import numpy as np

from efa_xray_amd import _lib
from efa_xray_amd.assimilation.assimilation import Assimilation

MAX_MEMBERS = 256
FIELDS = ("below", "equal", "rank", "crps", "err", "var")
_INT_FIELDS = ("below", "equal", "rank")


def _check_args(state, verification, by, weights, seed, fields):
    """(verif (nvar, nt, ny, nx) with NaN where not verified, slab groups (nvar*nt,), labels, weights (ny*nx,) or None, seed,
    fields as a tuple)."""
    state.dtype     # (raises ValueError when the variables mix dtypes)
    if state.nvars() < 1:
        raise ValueError("the state has no variables")
    nvar, nt, ny, nx, M = state.shape()
    if M < 2 or M > MAX_MEMBERS:
        raise ValueError("the state has %d members, supported are 2 to %d" % (M, MAX_MEMBERS))
    want = (nt, ny, nx)
    if not hasattr(verification, "get"):
        raise ValueError("verification must be a mapping from variable name to an array %r" % (want,))
    for name in verification.keys():
        if name not in state.variables:
            raise ValueError("verification names %r, which is no variable of the state %r" % (name, state.vars()))
    verif = np.full((nvar,) + want, np.nan)
    for iv, name in enumerate(state.vars()):
        ver = verification.get(name)
        if ver is None:         # a variable that is not verified
            continue
        try:
            ver = np.asarray(ver, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("verification[%r] is not an array of numbers" % name)
        if ver.shape != want:
            raise ValueError("verification[%r] has shape %r but the state has (ntimes, ny, nx) = %r" % (name, ver.shape, want))
        if np.any(np.isinf(ver)):
            raise ValueError("verification[%r] holds an infinite value (NaN means not verified)" % name)
        verif[iv] = ver
    vars_ = state.vars()
    if by == "var":
        groups = np.repeat(np.arange(nvar, dtype=np.int32), nt)
        labels = list(vars_)
    elif by == "var_time":
        groups = np.arange(nvar * nt, dtype=np.int32)
        times = list(state.ensemble_times())
        labels = [(v, t) for v in vars_ for t in times]
    elif by is None:
        groups = np.zeros(nvar * nt, dtype=np.int32)
        labels = [None]
    else:
        raise ValueError("by=%r must be 'var', 'var_time' or None" % (by,))
    w = None
    if weights is not None:
        try:
            w = np.asarray(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("weights must be None or an array (ny, nx) = %r" % ((ny, nx),))
        if w.shape != (ny, nx):
            raise ValueError("weights has shape %r but the state has (ny, nx) = %r" % (w.shape, (ny, nx)))
        if not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError("weights must be finite and >= 0")
        w = np.ascontiguousarray(w).reshape(-1)
    try:
        s = int(seed)
    except (TypeError, ValueError):
        raise ValueError("seed=%r is not an integer" % (seed,))
    if s != seed or s < 0 or s >= 2 ** 64:
        raise ValueError("seed=%r must be an integer in [0, 2**64)" % (seed,))
    if isinstance(fields, str):
        fields = (fields,)
    try:
        fields = tuple(fields)
    except TypeError:
        raise ValueError("fields must be a sequence of names out of %r" % (FIELDS,))
    for name in fields:
        if name not in FIELDS:
            raise ValueError("fields names %r, known are %r" % (name, FIELDS))
    if len(set(fields)) != len(fields):
        raise ValueError("fields names a field twice: %r" % (fields,))
    return verif, groups, labels, w, s, fields


def ensemble_verification(state, verification, by="var", weights=None, fair=False, seed=0, fields=(), device=0):
    """Rank histogram, CRPS and spread-skill of an ensemble against a verifying state.

    state        -- an `EnsembleState`, stored as float64 or float32 (every number is computed in float64)
    verification -- mapping variable name -> array (ntimes, ny, nx): the verifying state; NaN, or a variable that is missing,
                    means not verified; an infinite value raises ValueError
    by           -- 'var' (one group per variable), 'var_time' (one per variable and valid time) or None (one group)
    weights      -- None, or (ny, nx) finite weights >= 0 (cos(lat), a region mask); an element of weight 0 is not verified
    fair         -- the fair CRPS of Ferro (2014): the members' mutual distances over M(M-1) instead of M^2
    seed         -- of the tie-break: the rank of y among `equal` members equal to it is below + a hash of (seed, element)
    fields       -- names out of ('below', 'equal', 'rank', 'crps', 'err', 'var'): per-element fields to bring back
    device       -- HIP device ordinal

    Returns a dict of per-group arrays -- `groups` (labels: the variable, (variable, time) or None), `hist` (G, M+1), `n` and
    `n_bad` (verified elements without / with a non-finite member or difference; the latter enter no score), `crps`, `bias` and
    `rmse` of the ensemble mean, `spread` = sqrt(mean variance), `spread_skill` = sqrt((M+1)/M mean variance / mean squared
    error), `outlier_fraction` = (hist[0] + hist[M])/n, every mean weighted -- and `fields`, a dict of the requested per-element
    fields (nvar, ntimes, ny, nx) (kept apart: `crps` names a group score as well): integers -1, floats NaN where the element is
    not verified or bad.  A group with n == 0 has NaN scores."""
    verif, groups, labels, w, seed, fields = _check_args(state, verification, by, weights, seed, fields)
    nvar, nt, ny, nx, M = state.shape()
    N, ncol = state.nstate(), ny * nx
    ctx = _lib.get_context(device)
    X = Assimilation(state, [], device=device)._upload_prior(ctx)
    dev, raw = {}, {}
    d_ver = d_w = None
    try:
        d_ver = ctx.to_device(verif.reshape(-1))
        if w is not None:
            d_w = ctx.to_device(w)
        for name in fields:
            if name in _INT_FIELDS:
                raw[name] = ctx.malloc_bytes(max(N, 1) * 4)
            else:
                dev[name] = ctx.empty((N,))
        args = dict(dev)
        args.update(raw)
        hist, n, n_bad, sums = ctx.verify(N, M, X, d_ver, groups, ncol=ncol, n_lead=nvar * nt, col_weight=d_w, fair=fair,
                                          seed=seed, **args)
        per_row = {}
        for name in fields:
            if name in raw:
                host = np.empty(N, dtype=np.int32)
                if N:
                    ctx.d2h(host, raw[name])
            else:
                host = dev[name].download()
            per_row[name] = host.reshape(nvar, nt, ny, nx)
    finally:
        for p in raw.values():
            ctx.free_bytes(p)
        for a in dev.values():
            a.free()
        for a in (d_ver, d_w):
            if a is not None:
                a.free()
        X.free()
    with np.errstate(divide="ignore", invalid="ignore"):
        sw = np.where(n > 0, sums[:, 0], np.nan)
        out = {"fields": per_row}
        out["groups"] = labels
        out["hist"] = hist
        out["n"] = n
        out["n_bad"] = n_bad
        out["crps"] = sums[:, 1] / sw
        out["bias"] = sums[:, 2] / sw
        out["rmse"] = np.sqrt(sums[:, 3] / sw)
        out["spread"] = np.sqrt(sums[:, 4] / sw)
        out["spread_skill"] = np.where(n > 0, np.sqrt((M + 1.0) / M * sums[:, 4] / sums[:, 3]), np.nan)
        out["outlier_fraction"] = np.where(n > 0, (hist[:, 0] + hist[:, M]) / np.maximum(n, 1).astype(np.float64), np.nan)
    return out
