"""The ensemble Gram matrix, EOFs / principal components and clusters of members.

The per-element products treat a state element on its own.  The questions between members -- how do the members differ from one
another over the whole field, which few patterns carry the spread, which members belong together as scenarios and which member
represents each -- all come from one object, the M x M Gram matrix of the perturbations in a weighted norm

    G = X'^T C X' / (M-1),    c_i = w_col * s_lead^2

(primes: deviations from the ensemble mean; w the weight of the grid point, s the scale of the element's variable and valid time).
The contraction over the state runs on the device (`efa_gram_dev` / `efa_gram_f32_dev`); there is no NumPy path.  What follows
from G is M x M work on the host, numpy only: `distances_from_gram`, `eofs_from_gram`, `clusters_from_gram`.

The principal components `ensemble_eofs(state, ...)['pcs']` are a valid `metrics` argument of `ensemble_sensitivity` and
`observation_targets`: EOF-based ensemble sensitivity (Zheng et al. 2013, Chang et al. 2013).
"""
import warnings

import numpy as np

from efa_xray_amd import _lib

MAX_MEMBERS = 256
U = 2.0 ** -53
PATTERN_BATCH = 32   # modes per efa_sensitivity_dev call


# ---- pure host functions -------------------------------------------------------------------------------------------------------
def _check_gram(G):
    try:
        G = np.asarray(G, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("the Gram matrix must be a square array of numbers")
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError("the Gram matrix has shape %r, expected (M, M)" % (G.shape,))
    M = G.shape[0]
    if M < 2 or M > MAX_MEMBERS:
        raise ValueError("the Gram matrix has %d members, supported are 2 to %d" % (M, MAX_MEMBERS))
    if not np.all(np.isfinite(G)):
        raise ValueError("the Gram matrix must be finite")
    return G, M


def _check_count(value, name, lo, hi, what):
    try:
        n = int(value)
    except (TypeError, ValueError):
        raise ValueError("%s=%r is not an integer" % (name, value))
    if n != value or n < lo or n > hi:
        raise ValueError("%s=%r must be an integer in [%d, %d] (%s)" % (name, value, lo, hi, what))
    return n


def distances_from_gram(G):
    """Squared distances between the members in the norm of G: d2[a][b] = (M-1)(G_aa + G_bb - 2 G_ab), clamped at 0, which is
    sum_i c_i (x_ia - x_ib)^2 because the means cancel.  The diagonal is exactly 0."""
    G, M = _check_gram(G)
    d = np.diag(G)
    d2 = (M - 1) * (d[:, None] + d[None, :] - 2.0 * G)
    d2 = np.maximum(d2, 0.0)
    np.fill_diagonal(d2, 0.0)
    return d2


def eofs_from_gram(G, n_modes):
    """The leading `n_modes` <= M-1 modes of G (numpy.linalg.eigh).  Returns a dict:

    variance  -- (n_modes,) eigenvalues, descending, clamped at 0
    explained -- variance / trace(G); NaN when the trace is 0
    pcs       -- (n_modes, M) principal components sqrt(M-1) v_k: mean 0 and unit sample variance (with 1/(M-1)); the sign makes
                 the component of largest magnitude positive, the lowest member among equals

    A mode whose eigenvalue is <= 64 M u trace(G) (u = 2^-53) is null: its `pcs` row is 0.0 and its `explained` is 0.0."""
    G, M = _check_gram(G)
    n_modes = _check_count(n_modes, "n_modes", 1, M - 1, "at most M-1 modes carry variance")
    lam, V = np.linalg.eigh(0.5 * (G + G.T))
    order = np.argsort(-lam, kind="stable")[:n_modes]
    lam, V = lam[order], V[:, order]
    tr = float(np.trace(G))
    variance = np.maximum(lam, 0.0)
    null = ~(lam > 64.0 * M * U * tr)
    pcs = np.zeros((n_modes, M))
    for k in range(n_modes):
        if null[k]:
            continue
        v = V[:, k]
        if v[int(np.argmax(np.abs(v)))] < 0.0:
            v = -v
        pcs[k] = np.sqrt(M - 1.0) * v
    if tr > 0.0:
        explained = np.where(null, 0.0, variance / tr)
    else:
        explained = np.full(n_modes, np.nan)
    return dict(variance=variance, explained=explained, pcs=pcs)


def clusters_from_gram(G, n_clusters):
    """Ward's agglomeration of the members on d2 = `distances_from_gram(G)` by the Lance-Williams update

        d2(k, i u j) = ((n_i + n_k) d2_ik + (n_j + n_k) d2_jk - n_k d2_ij) / (n_i + n_j + n_k).

    Every step merges the pair of smallest d2 -- among equals the lowest (i, j), a cluster being named by its lowest member --
    until `n_clusters` are left.  Returns a dict: `labels` (M,), the clusters numbered in the order of their lowest members;
    `sizes`; `medoids`, the member of each cluster with the smallest sum of d2 to the others (the lowest among equals); and
    `within`, each cluster's sum of d2 to its medoid."""
    G, M = _check_gram(G)
    n_clusters = _check_count(n_clusters, "n_clusters", 1, M, "between one cluster and one per member")
    d2 = distances_from_gram(G)
    D = d2.copy()
    D[np.tril_indices(M)] = np.inf           # the pairs (i < j) of live clusters; everything else is +inf
    size = np.ones(M)
    members = [[m] for m in range(M)]
    live = np.ones(M, dtype=bool)
    for _ in range(M - n_clusters):
        i, j = divmod(int(np.argmin(D)), M)  # the first minimum in row-major order: the lowest (i, j)
        dij = D[i, j]
        ks = np.nonzero(live)[0]
        ks = ks[(ks != i) & (ks != j)]
        dik = np.where(ks < i, D[ks, i], D[i, ks])
        djk = np.where(ks < j, D[ks, j], D[j, ks])
        nk = size[ks]
        new = ((size[i] + nk) * dik + (size[j] + nk) * djk - nk * dij) / (size[i] + size[j] + nk)
        lo = ks < i
        D[ks[lo], i] = new[lo]
        D[i, ks[~lo]] = new[~lo]
        D[j, :] = np.inf
        D[:, j] = np.inf
        live[j] = False
        size[i] += size[j]
        members[i] = sorted(members[i] + members[j])
        members[j] = []
    labels = np.empty(M, dtype=np.int64)
    sizes, medoids, within = [], [], []
    for c, i in enumerate(np.nonzero(live)[0]):
        mem = np.array(members[i], dtype=np.int64)
        labels[mem] = c
        s = d2[np.ix_(mem, mem)].sum(axis=1)
        k = int(np.argmin(s))
        sizes.append(mem.size)
        medoids.append(int(mem[k]))
        within.append(float(s[k]))
    return dict(labels=labels, sizes=np.array(sizes, dtype=np.int64), medoids=np.array(medoids, dtype=np.int64),
                within=np.array(within))


# ---- the arguments -------------------------------------------------------------------------------------------------------------
def _check_state(state):
    dt = state.dtype     # (raises ValueError when the variables mix dtypes)
    if state.nvars() < 1:
        raise ValueError("the state has no variables")
    M = state.nmems()
    if M < 2 or M > MAX_MEMBERS:
        raise ValueError("the state has %d members, supported are 2 to %d" % (M, MAX_MEMBERS))
    return dt


def _resolve_norm(state, norm):
    """The scale of every (variable, valid time) slab, (nvar * ntimes,), from `norm`; None for norm='std' (the scales are then
    measured on the device, one variable at a time)."""
    nvar, nt = state.nvars(), state.ntimes()
    if norm is None:
        return np.ones(nvar * nt)
    if isinstance(norm, str):
        if norm != "std":
            raise ValueError("norm=%r: expected None, 'std' or a mapping from variable name to a scale" % (norm,))
        return None
    if not hasattr(norm, "keys"):
        raise ValueError("norm=%r: expected None, 'std' or a mapping from variable name to a scale" % (norm,))
    for name in norm.keys():
        if name not in state.variables:
            raise ValueError("norm names %r, which is no variable of the state %r" % (name, state.vars()))
    scales = np.zeros((nvar, nt))
    for iv, name in enumerate(state.vars()):
        if name not in norm:
            continue                          # a variable that is not named takes no part
        try:
            s = np.asarray(norm[name], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("norm[%r]=%r is not a number or an array (ntimes,)" % (name, norm[name]))
        if s.shape not in ((), (nt,)):
            raise ValueError("norm[%r] has shape %r, expected a number or (ntimes,) = (%d,)" % (name, s.shape, nt))
        if not np.all(np.isfinite(s)) or np.any(s < 0.0):
            raise ValueError("norm[%r] must be finite and >= 0" % name)
        scales[iv] = s
    return scales.reshape(-1)


def _check_weights(state, weights):
    if weights is None:
        return None
    ny, nx = state.ny(), state.nx()
    try:
        w = np.asarray(weights, dtype=np.float64)
        w = np.broadcast_to(w, (ny, nx))
    except (TypeError, ValueError):
        raise ValueError("weights has shape %r, not broadcastable to (ny, nx) = %r" % (np.shape(weights), (ny, nx)))
    if not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError("weights must be finite and >= 0")
    return np.ascontiguousarray(w).reshape(-1)


def _uploaded_gram(ctx, X, shape, scales, d_w):
    """The Gram matrix of an uploaded state X (device array (N, M)) of shape (nvar, nt, ny, nx, M); `scales` as `_resolve_norm`
    returns them, `d_w` the device weights (ny*nx,) or None.  Returns the dict `ensemble_gram` documents."""
    nvar, nt, ny, nx, M = shape
    N, ncol, n_lead = nvar * nt * ny * nx, ny * nx, nvar * nt
    if scales is None:     # 'std': every variable by the inverse root of its own weighted mean variance
        scales = np.zeros(n_lead)
        for iv in range(nvar):
            one = np.zeros(n_lead)
            one[iv * nt:(iv + 1) * nt] = 1.0
            Gv, _, _, sv = ctx.gram(N, M, X, one, ncol=ncol, n_lead=n_lead, col_weight=d_w)
            mean_var = np.trace(Gv) / sv[0] if sv[0] > 0.0 else 0.0
            if mean_var > 0.0 and np.isfinite(mean_var):
                scales[iv * nt:(iv + 1) * nt] = 1.0 / np.sqrt(mean_var)
            else:
                warnings.warn("norm='std': variable %d has no variance (or no usable element); it gets scale 0" % iv,
                              RuntimeWarning, stacklevel=3)
    G, n, n_bad, sums = ctx.gram(N, M, X, scales, ncol=ncol, n_lead=n_lead, col_weight=d_w)
    return dict(gram=G, n=n, n_bad=n_bad, weight_sum=float(sums[0]), scales=np.array(scales, dtype=np.float64).reshape(nvar, nt))


def _run(state, norm, weights, device, after=None):
    """Checks, upload, the Gram matrix; `after(ctx, X, out)` runs while the state is still on the device."""
    from efa_xray_amd.assimilation.assimilation import Assimilation
    _check_state(state)
    scales = _resolve_norm(state, norm)
    w = _check_weights(state, weights)
    ctx = _lib.get_context(device)
    X = Assimilation(state, [], device=device)._upload_prior(ctx)
    d_w = None
    try:
        if w is not None:
            d_w = ctx.to_device(w)
        out = _uploaded_gram(ctx, X, state.shape(), scales, d_w)
        if after is not None:
            after(ctx, X, out)
    finally:
        if d_w is not None:
            d_w.free()
        X.free()
    return out


# ---- device-backed functions ---------------------------------------------------------------------------------------------------
def ensemble_gram(state, norm=None, weights=None, device=0):
    """The Gram matrix of the members' perturbations, G = X'^T C X'/(M-1), c_i = w s^2.

    state   -- an `EnsembleState`, stored as float64 or float32 (every number is computed in float64)
    norm    -- None: every variable has scale 1.  'std': each variable is scaled by 1/sqrt(its own weighted mean variance), so
               variables of different units weigh alike; a variable without variance gets scale 0 and a warning.  Or a mapping
               variable name -> scale (a number, or an array (ntimes,) to pick valid times; finite, >= 0); a variable that is not
               named gets 0
    weights -- None, or an array broadcastable to (ny, nx) of finite weights >= 0 (cos(lat), a region mask)
    device  -- HIP device ordinal

    Returns a dict: `gram` (M, M), bit-for-bit symmetric; `n`, the elements that entered (scale > 0, weight > 0, every member
    finite); `n_bad`, those left out for a member that is not finite; `weight_sum`, the sum of w over the n; `scales`
    (nvar, ntimes).  The Gram matrices, n and weight sums of column shards of a state add up to the whole state's."""
    return _run(state, norm, weights, device)


def ensemble_eofs(state, n_modes, norm=None, weights=None, patterns=True, device=0):
    """EOFs of the ensemble spread: the leading `n_modes` <= M-1 modes of `ensemble_gram(state, norm, weights)`.

    Returns the outputs of `ensemble_gram` and of `eofs_from_gram` (`variance`, `explained`, `pcs` (n_modes, M)) and, with
    `patterns`, `patterns` (n_modes, nvar, ntimes, ny, nx): the regression map cov(x_i, pc_k) of every element on the
    standardised component, in the variable's own units (the same contraction as `ensemble_sensitivity(state, pcs)['cov']`, on
    the same uploaded state).  With e_k the unit-length EOF in the norm of G and lambda_k its variance,

        sqrt(c_i) * patterns[k][i] = sqrt(lambda_k) * e_k[i].

    `pcs` is a valid `metrics` argument of `ensemble_sensitivity` and `observation_targets`."""
    _check_state(state)
    n_modes = _check_count(n_modes, "n_modes", 1, state.nmems() - 1, "at most M-1 modes carry variance")
    nvar, nt, ny, nx, M = state.shape()
    N = state.nstate()

    def after(ctx, X, out):
        out.update(eofs_from_gram(out["gram"], n_modes))
        if not patterns:
            return
        pat = np.empty((n_modes, N))
        ones = np.ones(nvar * nt)
        for k0 in range(0, n_modes, PATTERN_BATCH):
            J = out["pcs"][k0:k0 + PATTERN_BATCH]
            cov = ctx.empty((J.shape[0], N))
            try:
                ctx.sensitivity(N, M, X, J, ones, ncol=ny * nx, n_lead=nvar * nt, cov=cov)
                pat[k0:k0 + J.shape[0]] = cov.download().reshape(J.shape[0], N)
            finally:
                cov.free()
        out["patterns"] = pat.reshape(n_modes, nvar, nt, ny, nx)

    return _run(state, norm, weights, device, after)


def ensemble_clusters(state, n_clusters, norm=None, weights=None, device=0):
    """Scenarios: Ward clusters of the members in the norm of `ensemble_gram(state, norm, weights)`.

    Returns the outputs of `ensemble_gram` and of `clusters_from_gram` (`labels`, `sizes`, `medoids` -- the member that
    represents each cluster -- and `within`)."""
    _check_state(state)
    n_clusters = _check_count(n_clusters, "n_clusters", 1, state.nmems(), "between one cluster and one per member")
    out = _run(state, norm, weights, device)
    out.update(clusters_from_gram(out["gram"], n_clusters))
    return out
