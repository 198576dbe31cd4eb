"""Ensemble products and the verification of their probabilities (Murphy 1973).

What is read from an adjusted ensemble: for every state element with members x_1..x_M, `ensemble_products` forms on the device
(`efa_products_dev` / `efa_products_f32_dev`; there is no NumPy path) the mean, the standard deviation, quantiles by numpy's
linear rule and the probabilities k/M of exceeding thresholds, k = #{m: x_m > t}.  `probability_verification` scores those
probabilities against a verifying state: per group of elements and threshold the reliability table, the Brier score, its skill
and Murphy's decomposition.
"""
import numpy as np

from efa_xray_amd import _lib
from efa_xray_amd.assimilation.assimilation import Assimilation
from efa_xray_amd.postprocess.verification import _check_args as _check_verification

MAX_MEMBERS = 256
MAX_LEVELS = 8


def _check_state(state):
    state.dtype     # (raises ValueError when the variables mix dtypes)
    if state.nvars() < 1:
        raise ValueError("the state has no variables")
    M = state.shape()[4]
    if M < 2 or M > MAX_MEMBERS:
        raise ValueError("the state has %d members, supported are 2 to %d" % (M, MAX_MEMBERS))


def _check_quantiles(quantiles):
    """The levels as a float64 array (Q,)."""
    if np.isscalar(quantiles):
        quantiles = (quantiles,)
    try:
        q = np.asarray(tuple(quantiles), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("quantiles must be a sequence of numbers in [0, 1]")
    if q.ndim != 1:
        raise ValueError("quantiles must be a sequence of numbers in [0, 1]")
    if q.size > MAX_LEVELS:
        raise ValueError("%d quantiles were asked for, supported are at most %d per call" % (q.size, MAX_LEVELS))
    if not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError("quantiles must lie in [0, 1], got %r" % (q.tolist(),))
    return q


def _check_thresholds(state, thresholds, required):
    """({variable: float64 array (T_var,)}, thr (nvar*nt, T) with NaN where a slab has no threshold)."""
    nvar, nt = state.shape()[:2]
    if thresholds is None and not required:
        return {}, np.zeros((nvar * nt, 0))
    if not hasattr(thresholds, "get"):
        raise ValueError("thresholds must be a mapping from variable name to a sequence of at most %d numbers" % MAX_LEVELS)
    per_var = {}
    for name in thresholds.keys():
        if name not in state.variables:
            raise ValueError("thresholds names %r, which is no variable of the state %r" % (name, state.vars()))
        t = thresholds.get(name)
        if np.isscalar(t):
            t = (t,)
        try:
            t = np.asarray(tuple(t), dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("thresholds[%r] is not a sequence of numbers" % name)
        if t.ndim != 1:
            raise ValueError("thresholds[%r] is not a sequence of numbers" % name)
        if t.size > MAX_LEVELS:
            raise ValueError("thresholds[%r] holds %d numbers, supported are at most %d per call" % (name, t.size, MAX_LEVELS))
        if not np.all(np.isfinite(t)):
            raise ValueError("thresholds[%r] holds a value that is not finite" % name)
        per_var[name] = t
    T = max([t.size for t in per_var.values()] + [0])
    thr = np.full((nvar, nt, T), np.nan)
    for iv, name in enumerate(state.vars()):
        t = per_var.get(name)
        if t is not None:
            thr[iv, :, :t.size] = t
    return per_var, thr.reshape(nvar * nt, T)


def ensemble_products(state, quantiles=(), thresholds=None, mean=True, sd=True, device=0):
    """Mean, standard deviation, quantiles and exceedance probabilities of every element of an ensemble state.

    state      -- an `EnsembleState`, stored as float64 or float32 (every number is computed in float64)
    quantiles  -- at most 8 levels in [0, 1]; numpy's default linear rule on the sorted members
    thresholds -- None, or a mapping variable name -> at most 8 finite numbers; the variables may differ in count or be absent
    mean, sd   -- whether to bring those fields back
    device     -- HIP device ordinal

    Returns a dict: `mean` and `sd` (nvar, ntimes, ny, nx) (when wanted), `quantiles` (Q, nvar, ntimes, ny, nx) and
    `probabilities`, a mapping variable name -> (T_var, ntimes, ny, nx) of k/M, k the number of members above the threshold.
    An element with a member that is not finite is NaN in every field."""
    _check_state(state)
    q = _check_quantiles(quantiles)
    per_var, thr = _check_thresholds(state, thresholds, required=False)
    nvar, nt, ny, nx, M = state.shape()
    N, ncol = state.nstate(), ny * nx
    T = thr.shape[1]
    ctx = _lib.get_context(device)
    X = Assimilation(state, [], device=device)._upload_prior(ctx)
    dev = {}
    try:
        if mean:
            dev["mean"] = ctx.empty((N,))
        if sd:
            dev["sd"] = ctx.empty((N,))
        if q.size:
            dev["quant"] = ctx.empty((q.size, N))
        if T:
            dev["prob"] = ctx.empty((T, N))
        ctx.products(N, M, X, ncol=ncol, n_lead=nvar * nt, quantiles=q, thresholds=thr, **dev)
        host = dict((k, a.download()) for k, a in dev.items())
    finally:
        for a in dev.values():
            a.free()
        X.free()
    out = {}
    if mean:
        out["mean"] = host["mean"].reshape(nvar, nt, ny, nx)
    if sd:
        out["sd"] = host["sd"].reshape(nvar, nt, ny, nx)
    out["quantiles"] = host["quant"].reshape(q.size, nvar, nt, ny, nx) if q.size else np.zeros((0, nvar, nt, ny, nx))
    probs = {}
    for iv, name in enumerate(state.vars()):
        t = per_var.get(name)
        if t is not None:
            probs[name] = host["prob"].reshape(T, nvar, nt, ny, nx)[:t.size, iv].copy() if T else np.zeros((0, nt, ny, nx))
    out["probabilities"] = probs
    return out


def scores_from_table(table, sums):
    """The scores of one (group, threshold) from its table (M+1, 2) of counts and its sums (sum w, sum w (p-o)^2, sum w p, sum w o):
    a dict of brier, base_rate, forecast_rate, brier_skill (weighted, from the sums) and reliability, resolution, uncertainty,
    observed_frequency (M+1,), n_forecasts (M+1,) (unweighted, from the table with its M+1 natural bins)."""
    table = np.asarray(table, dtype=np.int64)
    M = table.shape[0] - 1
    nk = table.sum(axis=1)
    n = int(nk.sum())
    out = {"n_forecasts": nk}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["observed_frequency"] = np.where(nk > 0, table[:, 1] / np.maximum(nk, 1).astype(np.float64), np.nan)
        if n == 0:
            for key in ("brier", "base_rate", "forecast_rate", "brier_skill", "reliability", "resolution", "uncertainty"):
                out[key] = np.nan
            return out
        sw = float(sums[0])
        out["brier"] = float(sums[1]) / sw
        out["forecast_rate"] = float(sums[2]) / sw
        base = float(sums[3]) / sw
        out["base_rate"] = base
        den = base * (1.0 - base)
        out["brier_skill"] = 1.0 - out["brier"] / den if den != 0.0 else np.nan
        p = np.arange(M + 1) / float(M)
        obar = table[:, 1].sum() / float(n)
        ok = np.where(nk > 0, table[:, 1] / np.maximum(nk, 1).astype(np.float64), 0.0)
        out["reliability"] = float(np.sum(nk * (p - ok) ** 2) / n)
        out["resolution"] = float(np.sum(nk * (ok - obar) ** 2) / n)
        out["uncertainty"] = float(obar * (1.0 - obar))
    return out


def probability_verification(state, verification, thresholds, by="var", weights=None, device=0):
    """Brier score, its skill, Murphy's decomposition and the reliability table of the ensemble's exceedance probabilities.

    state        -- an `EnsembleState`, stored as float64 or float32
    verification -- mapping variable name -> array (ntimes, ny, nx): the verifying state; NaN, or a variable that is missing,
                    means not verified; an infinite value raises ValueError
    thresholds   -- mapping variable name -> at most 8 finite numbers; the event at threshold t is x > t
    by           -- 'var' (one group per variable), 'var_time' (one per variable and valid time) or None (one group)
    weights      -- None, or (ny, nx) finite weights >= 0; an element of weight 0 is not scored
    device       -- HIP device ordinal

    Returns a dict of arrays per group and threshold: `brier`, `base_rate`, `forecast_rate`, `brier_skill` (G, T), weighted;
    `reliability`, `resolution`, `uncertainty` (G, T) and `observed_frequency`, `n_forecasts` (G, T, M+1) from the unweighted
    integer `table` (G, T, M+1, 2) of scored elements by forecast count k and outcome; `n` and `n_bad` (G, T) (scored elements
    without / with a member that is not finite; the latter enter nothing); `groups` (labels) and `thresholds` (G, T), NaN where
    the group has no such threshold.  A group and threshold with n == 0 has NaN scores."""
    verif, groups, labels, w, _, _ = _check_verification(state, verification, by, weights, 0, ())
    per_var, thr = _check_thresholds(state, thresholds, required=True)
    nvar, nt, ny, nx, M = state.shape()
    N, ncol = state.nstate(), ny * nx
    T = thr.shape[1]
    G = len(labels)
    gthr = np.full((G, T), np.nan)
    if by is None:    # one group over variables whose thresholds may differ: each is scored at its own, the label is the first's
        for s in range(nvar * nt - 1, -1, -1):
            gthr[0] = np.where(np.isnan(thr[s]), gthr[0], thr[s])
    else:
        for s in range(nvar * nt):
            gthr[groups[s]] = thr[s]
    keys2 = ("brier", "base_rate", "forecast_rate", "brier_skill", "reliability", "resolution", "uncertainty")
    out = dict((k, np.full((G, T), np.nan)) for k in keys2)
    out["observed_frequency"] = np.full((G, T, M + 1), np.nan)
    out["n_forecasts"] = np.zeros((G, T, M + 1), dtype=np.int64)
    out["groups"] = labels
    out["thresholds"] = gthr
    if T == 0:
        out["table"] = np.zeros((G, 0, M + 1, 2), dtype=np.int64)
        out["n"] = np.zeros((G, 0), dtype=np.int64)
        out["n_bad"] = np.zeros((G, 0), dtype=np.int64)
        return out
    ctx = _lib.get_context(device)
    X = Assimilation(state, [], device=device)._upload_prior(ctx)
    d_ver = d_w = None
    try:
        d_ver = ctx.to_device(verif.reshape(-1))
        if w is not None:
            d_w = ctx.to_device(w)
        table, n_bad, sums = ctx.products(N, M, X, ncol=ncol, n_lead=nvar * nt, thresholds=thr, verif=d_ver, slab_group=groups,
                                          col_weight=d_w)
    finally:
        for a in (d_ver, d_w):
            if a is not None:
                a.free()
        X.free()
    out["table"] = table
    out["n"] = table.sum(axis=(2, 3))
    out["n_bad"] = n_bad
    for g in range(G):
        for j in range(T):
            sc = scores_from_table(table[g, j], sums[g, j])
            for k in keys2:
                out[k][g, j] = sc[k]
            out["observed_frequency"][g, j] = sc["observed_frequency"]
            out["n_forecasts"][g, j] = sc["n_forecasts"]
    return out
