"""LETKF: local ensemble transform Kalman filter, computed on an MI355X.

Hunt, Kostelich & Szunyogh (2007): the textbook ensemble-space update of `ETKF`, solved once per (y, x) column with every
observation's error variance divided by its Gaspari-Cohn taper at that column (R-localisation):

    A_c = (M-1) I + sum_k (rho_k(c)/r_k) Y_k^T Y_k = V diag(mu) V^T,  T_c = V diag(sqrt((M-1)/mu)) V^T,
    w_c = V diag(1/mu) V^T sum_k (rho_k(c)/r_k) d_k Y_k^T;   every row of column c: mean += X' w_c, X' <- X' T_c

over the observations that are assimilated and within reach of the column, Y_k and d_k the PRIOR observation-space perturbations
and innovations.  The obs block maps likewise, ob j with the pair solved at its own position.  This is the localised filter for
the states `ETKF` cannot serve; it is not the reference's serial loop, which `EnSRF(loc='GC')` reproduces.

Same surface as `EnSRF`: `LETKF(state, obs, ...).update() -> (post_state, obs)` with the five diagnostics written onto each
`Observation` as `ETKF` writes them.  After an update `last_solve` holds three (ny, nx) arrays: `n_local` (the observations
that reach the column), `dfs` (trace(HK) of the column's solve) and `sweeps` (Jacobi sweeps of its eigen-solve; 0 where no
observation reaches the column: there is nothing to solve and the column's rows come back bit for bit).

`weight_stride=s` or `(s_y, s_x)` turns on weight interpolation (Yang, Kalnay, Hunt & Bowler 2009): the pair
(T, w) is solved at every s_y x s_x-th column only (and at the last row and column of the grid), interpolated bilinearly in
grid-index space to the columns in between and applied there, which divides the number of eigen-solves by about s_y s_x.  The
observation block and the diagnostics are unchanged, bit for bit.  `last_solve` then holds `n_local`, `dfs` and `sweeps` of the
NODES, of shape (nyn, nxn), and their grid indices `node_y` and `node_x`.  A column all of whose nodes are out of every
observation's reach keeps its rows bit for bit -- also when an observation of short radius reaches the column itself: that
observation is lost to it.  Keep the stride, in km, well below the smallest localize_radius.  `None`, `1` and `(1, 1)` are the
plain filter.

`SlabLETKF` is the LETKF with the vertical, temporal and cross-variable factors of `EnSRF(loc='GC')`:
`vert_coord`, `time_localize` and `var_impact` as documented there.  The (nvars x ntimes) slabs of a column no longer share one
pair: slabs whose factors agree for every observation form a group, and every (group, column) runs its own solve under the
product taper.  `last_solve` then holds `n_local`, `dfs` and `sweeps` of shape (ngroups, ny, nx) -- (ngroups, nyn, nxn) with a
weight_stride -- and `group_of_slab` of shape (nvars, ntimes).  With none of the three options it is `LETKF`, bit for bit.

`column_inflation=ColumnInflation(...)` (letkf_inflation.py) gives every solve point a multiplicative inflation
factor that enters its solve as Hunt's rho and is re-estimated from the innovations after Miyoshi (2011).  Its `values` have the
shape of `last_solve`'s arrays -- (ny, nx), (nyn, nxn) with a weight_stride, a leading ngroups axis under `SlabLETKF`'s options --
and hold the factors for the NEXT update once this one returns; `last_solve` gains `inflation` (the factors this update used),
`inflation_post` and `inflation_stats` (..., 4) = (p1, p2, p3, lambda_o).  Observations with the default point interpolation are
solved under that interpolation of the field, observations with a user-defined forward operator under 1.0.  This is the LETKF's
adaptive inflation; `adaptive_inflation` (Anderson 2009, tied to the serial filter's order) stays refused.

`control=ctrl` carries a single deterministic forecast beside the ensemble and adjusts it by the same observations
through the ensemble's covariances (the deterministic analysis of Schraff et al. 2016; the control member of Hunt et al. 2007):

    x_c^a = x_c + X' w^c,   w^c = A_c^-1 sum_k (rho_k(c)/r_k) (value_k - H(x_c)_k) Y_k^T

per column (per (slab group, column) under `SlabLETKF`), and H(x_c)^a likewise at every observation's own position.  `ctrl` is an
`EnsembleState` with the state's variables, coordinates and grid and exactly ONE member; H(x_c) is the default point interpolation
applied to it, or `ob.estimate(ctrl)` for user-defined operators.  After `update()`, `last_control` is a dict: `state` (a NEW
one-member `EnsembleState`, the control analysis), `ob_prior` (P,) = H(x_c) and `ob_post` (P,), NaN where the observation was not
assimilated.  The ensemble's results -- the return value and the five diagnostics -- do not change by a bit; the outlier check is
decided on the ensemble mean alone; relaxation and the constant `inflation=` hook act on the ensemble's perturbations only.
`control` with `weight_stride` raises ValueError: weight interpolation of w^c is the follow-up.

`max_local_obs=N` caps the observations one local analysis may use, as Miyoshi's `nobsl`, SCALE-LETKF's
`MAX_NOBS_PER_GRID` and JEDI's `max nobs` do: at every solve point (a column, a node of the `weight_stride` mesh, an observation's
own position) only the N assimilated observations with the LARGEST taper keep it, equal tapers ordered by position in `obs`.  An int
>= 1 caps all observations together; `{obtype: N}` caps each named `obtype` on its own (an obtype that is not named has no limit, a
named obtype no observation has is ignored, at most 31 may be named), so that a dense network does not swamp the sparse one around
it.  An observation that is not assimilated (not requested, or rejected by `outlier_threshold`) takes no place.  `last_solve` gains
`n_reach`, the count before the cap, beside `n_local` = sum over the classes of min(N, reach).  It combines with every other option
of `LETKF`; `SlabLETKF` takes it only without its three keywords (a cap per slab group is the follow-up).

`cross_validation=K` is the LETKF with cross validation of Buehner (2020): the members are split into K groups
(an int K >= 2: member m has the label m % K; an integer array (M,): the labels 0..K-1 themselves, every label used), and at every
solve point the perturbations of each group are updated with the perturbation gain of an LETKF formed from the OTHER groups'
members alone, which takes the inbreeding out of the posterior spread; the mean keeps the full-ensemble gain, and the posterior
mean is the plain filter's.  Every group must leave at least 2 members outside it (so M >= 4).  K sub-solves of size M - M/K per
solve point share the point's one Gram matrix.  `last_solve` gains `cv_sweeps` (the sub-solves' Jacobi sweeps, summed) and
`cv_cond` (their largest condition number), in the shape of `n_local`.  It combines with weight_stride, max_local_obs, rtps /
rtpp, outlier_threshold and float32 states; with column_inflation or control it raises ValueError, as it does under `SlabLETKF`
together with any of its three keywords.
"""
from collections import OrderedDict
from copy import deepcopy

import numpy as np

from efa_xray_amd import _lib
from efa_xray_amd.assimilation.ensrf import EnSRF
from efa_xray_amd.assimilation.letkf_inflation import ColumnInflation, expand_nodes, ob_factors
from efa_xray_amd.state.ensemble import EnsembleState

MAX_MEMBERS = 136

# keywords of EnSRF that the per-column batch solve does not serve, with the reason given to the caller
_REFUSED = (
    ("adaptive_inflation", "adaptive inflation follows the serial order of the observations, which a column's batch solve does not have"),
    ("vert_coord", "vertical localisation needs a solve per (slab group, column): use SlabLETKF (DESIGN.md 7y-3)"),
    ("time_localize", "temporal localisation needs a solve per (slab group, column): use SlabLETKF (DESIGN.md 7y-3)"),
    ("var_impact", "cross-variable localisation needs a solve per (slab group, column): use SlabLETKF (DESIGN.md 7y-3)"),
    ("sampling_error_correction", "the sampling error correction acts on the serial gain of one observation at a time"),
    ("streamed", "the streamed host path is out of scope for the LETKF (DESIGN.md 7y): the state must be resident"),
    ("path", "there is no sweep or transform route to choose: every column runs its own solve and apply in one kernel"),
    ("obs_batch", "there is no per-batch sweep under the per-column solve"),
)


def _weight_stride(stride):
    """None for the plain filter (None, 1, (1, 1)), else (s_y, s_x); ValueError for anything but integers >= 1."""
    if stride is None:
        return None
    pair = tuple(stride) if isinstance(stride, (tuple, list)) else (stride, stride)
    ok = len(pair) == 2 and all(isinstance(s, (int, np.integer)) and not isinstance(s, bool) and s >= 1 for s in pair)
    if not ok:
        raise ValueError("LETKF: weight_stride=%r must be an integer >= 1 or a pair (s_y, s_x) of them" % (stride,))
    pair = (int(pair[0]), int(pair[1]))
    return None if pair == (1, 1) else pair


MAX_CAP_OBTYPES = 31     # named obtypes of max_local_obs: the library has 32 classes, one is "not named"


def _count(n, what):
    """n as an int >= 1; ValueError for anything else, booleans and floats included."""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("%s must be an integer >= 1, got %r" % (what, n))
    return int(n)


def _max_local_obs(cap):
    """None, or (names, caps): names None and caps (N,) for the int form, else the named obtypes and their caps."""
    if cap is None:
        return None
    if isinstance(cap, dict):
        if not cap:
            raise ValueError("max_local_obs: the dict names no obtype; use None for no cap")
        if len(cap) > MAX_CAP_OBTYPES:
            raise ValueError("max_local_obs names %d obtypes, more than %d" % (len(cap), MAX_CAP_OBTYPES))
        names = list(cap)
        return names, tuple(_count(cap[name], "max_local_obs[%r]" % (name,)) for name in names)
    return None, (_count(cap, "max_local_obs"),)


def _cap_classes(cap, obs):
    """(ob_class or None, caps) as Context.set_letkf_obs_cap takes them: the named obtypes some ob has are the classes 0.., the
    class behind them (cap 0: no limit) takes every other ob."""
    names, caps = cap
    if names is None:
        return None, list(caps)
    have = set(ob.obtype for ob in obs)
    keep = [i for i, name in enumerate(names) if name in have]
    cls = {names[i]: j for j, i in enumerate(keep)}
    ob_class = np.array([cls.get(ob.obtype, len(keep)) for ob in obs], dtype=np.int32)
    return ob_class, [caps[i] for i in keep] + [0]


def _cross_validation(spec, M):
    """None, or the labels (M,) int32 of cross_validation=spec; ValueError for anything but an int K >= 2 or an integer array (M,) of
    labels 0..K-1 with K >= 2, every label used and at least 2 members outside every group."""
    if spec is None:
        return None
    what = "cross_validation=%r" % (spec,)
    if isinstance(spec, (bool, np.bool_)):
        raise ValueError("%s must be an int K >= 2 or an integer array of M labels" % what)
    if isinstance(spec, (int, np.integer)):
        if spec < 2:
            raise ValueError("%s: the number of groups must be >= 2" % what)
        if spec > M:
            raise ValueError("%s: more groups than the ensemble's %d members, a label would be unused" % (what, M))
        g = np.arange(M, dtype=np.int64) % int(spec)
    else:
        try:
            g = np.asarray(spec)
        except Exception:
            g = None
        if g is None or g.ndim != 1 or g.dtype == np.bool_ or not np.issubdtype(g.dtype, np.integer):
            raise ValueError("%s must be an int K >= 2 or an integer array of M labels" % what)
        if g.shape[0] != M:
            raise ValueError("cross_validation has %d labels, the ensemble %d members" % (g.shape[0], M))
        g = g.astype(np.int64)
    if g.size == 0 or g.min() < 0:
        raise ValueError("cross_validation: the labels must be >= 0")
    K = int(g.max()) + 1
    size = np.bincount(g, minlength=K)
    if K < 2:
        raise ValueError("cross_validation: at least 2 groups are needed")
    if np.any(size == 0):
        raise ValueError("cross_validation: the label %d is unused (every label 0..%d must be)" % (int(np.flatnonzero(size == 0)[0]), K - 1))
    if M - int(size.max()) < 2:
        raise ValueError("cross_validation: group %d leaves %d members outside it (at least 2 are needed to form a gain)"
                         % (int(np.argmax(size)), M - int(size.max())))
    return g.astype(np.int32)


def _check_control(state, ctrl):
    """ValueError unless `ctrl` is a one-member EnsembleState on the state's variables, coordinates and grid."""
    if not isinstance(ctrl, EnsembleState):
        raise ValueError("control must be an EnsembleState with exactly one member, got %r" % type(ctrl).__name__)
    if ctrl.nvars() == 0 or ctrl.nmems() != 1:
        raise ValueError("control must have exactly one member, got %d" % (ctrl.nmems() if ctrl.nvars() else 0))
    if ctrl.vars() != state.vars():
        raise ValueError("control has the variables %r, the state has %r" % (ctrl.vars(), state.vars()))
    if ctrl.shape()[:4] != state.shape()[:4]:
        raise ValueError("control has (nvars, ntimes, ny, nx) = %r, the state has %r" % (ctrl.shape()[:4], state.shape()[:4]))
    for key in ("validtime", "lat", "lon"):
        a, b = np.asarray(ctrl.coords.get(key)), np.asarray(state.coords.get(key))
        if a.shape != b.shape or not np.all(a == b):
            raise ValueError("control and state differ in the coordinate %r" % key)


class LETKF(EnSRF):
    _served = ()        # the keywords of _REFUSED a subclass serves: handed on to EnSRF, which validates them

    def __init__(self, state, obs, nproc=1, inflation=None, verbose=True, **kw):
        """Keyword-only options, as `EnSRF` has them: loc ('GC', the default and the only value), device, rtps / rtpp,
        outlier_threshold; float32 states work as they do there; weight_stride (None, an int >= 1 or a pair of them: the module's
        docstring); column_inflation (None or a `ColumnInflation`).  ValueError, before any device work, for loc other than 'GC'
        (use `ETKF` for the unlocalised filter), adaptive_inflation, vert_coord, time_localize, var_impact,
        sampling_error_correction, streamed, path, obs_batch, a weight_stride that is not an integer >= 1, and for more than 136 members (the eigen-solve of a column keeps
        its M x M array in LDS).  control (None, or a one-member `EnsembleState` on the state's variables, coordinates and grid:
        the module's docstring): ValueError for anything else and for control with a weight_stride.  max_local_obs (None, an
        int >= 1 or {obtype: int >= 1} with at most 31 names: the module's docstring): ValueError for anything else, and under
        `SlabLETKF` together with any of its three keywords.  cross_validation (None, an int K >= 2 or an integer array (M,) of
        labels: the module's docstring): ValueError for anything else, for groups that break its rules, together with
        column_inflation or control, and under `SlabLETKF` together with any of its three keywords.  `update_arrays` is not
        offered."""
        stride = _weight_stride(kw.pop("weight_stride", None))
        cap = _max_local_obs(kw.pop("max_local_obs", None))
        if cap is not None:
            for name in self._served:
                if kw.get(name) is not None and kw.get(name) is not False:
                    raise ValueError("%s: max_local_obs and %s do not combine: under the vertical / temporal / variable factors "
                                     "the taper of a solve is a product per (slab group, column) while the cap ranks the per-column "
                                     "tapers of the lists (a cap per group is the follow-up, DESIGN.md 7y-8)"
                                     % (type(self).__name__, name))
        ctrl = kw.pop("control", None)
        if ctrl is not None:
            _check_control(state, ctrl)
            if stride is not None:
                raise ValueError("%s: control and weight_stride do not combine: the interpolated pairs [T | w] have no place for "
                                 "the control's weight vector (weight interpolation of w^c is the follow-up, DESIGN.md 7y-7)"
                                 % type(self).__name__)
        ci = kw.pop("column_inflation", None)
        if ci is not None and not isinstance(ci, ColumnInflation):
            raise ValueError("column_inflation must be a ColumnInflation, got %r" % type(ci).__name__)
        cv = _cross_validation(kw.pop("cross_validation", None), state.nmems())
        if cv is not None:
            for name, given in (("column_inflation", ci), ("control", ctrl)):
                if given is not None:
                    raise ValueError("%s: cross_validation and %s do not combine (out of scope, DESIGN.md 7y-9)"
                                     % (type(self).__name__, name))
            for name in self._served:
                if kw.get(name) is not None and kw.get(name) is not False:
                    raise ValueError("%s: cross_validation and %s do not combine: the sub-solves per (slab group, column) are out "
                                     "of scope (DESIGN.md 7y-9)" % (type(self).__name__, name))
        loc = kw.pop("loc", "GC")
        if not (isinstance(loc, str) and loc == "GC"):
            raise ValueError("LETKF: loc=%r is not supported: the LETKF is the localised filter and takes loc='GC' only; "
                             "use ETKF for the unlocalised ensemble transform filter" % (loc,))
        for name, why in _REFUSED:
            if name in self._served:
                continue
            if name in kw and kw[name] is not None and kw[name] is not False:
                raise ValueError("%s does not take %s: %s" % (type(self).__name__, name, why))
            kw.pop(name, None)
        if state.nmems() > MAX_MEMBERS:
            raise ValueError("LETKF: %d members exceed %d, the range in which the eigen-solve's M x M array of a column fits in "
                             "LDS (DESIGN.md 7y)" % (state.nmems(), MAX_MEMBERS))
        EnSRF.__init__(self, state, obs, nproc, inflation, verbose, "GC", **kw)
        self.last_solve = None
        self.weight_stride = stride
        self.column_inflation = ci
        self.control = ctrl
        self.last_control = None
        self.max_local_obs = cap
        self.cross_validation = cv

    _cycle_line = "Beginning the column solves"

    def _check_prior(self):
        M = self.prior.nmems()
        if M > MAX_MEMBERS:
            raise ValueError("LETKF: %d members exceed %d (DESIGN.md 7y)" % (M, MAX_MEMBERS))

    def update(self):
        self.last_solve = None
        self.last_control = None
        return EnSRF.update(self)       # the resident sequence (streamed is refused), with the cycle below

    def _run_cycle(self, ctx, X, P, ym, Yp, ob, geometry, field):
        """The column solves in place on X (float64 or float32 rows); returns the diagnostics and leaves `last_solve`."""
        prior = self.prior
        N, M = prior.nstate(), prior.nmems()
        ny, nx = prior.shape()[2:4]
        n_lead = geometry[2]
        slab = self.vert_coord is not None or self.slab is not None     # (SlabLETKF only: LETKF refuses the three keywords)
        mesh = {}
        sy, sx = ny, nx                         # the statistics' shape: the grid's, or the node mesh's
        if self.weight_stride is not None:
            node_y = _lib.letkf_mesh_nodes(ny, self.weight_stride[0])
            node_x = _lib.letkf_mesh_nodes(nx, self.weight_stride[1])
            sy, sx = node_y.size, node_x.size
            mesh = dict(shape=(ny, nx), stride=self.weight_stride)
        ng = 1                                  # solves per column or node
        ci = self.column_inflation
        ctrl = self.control
        if ctrl is not None:                    # host work first: the setting goes on only around the cycle
            _check_control(prior, ctrl)
            xc = np.ascontiguousarray(ctrl.to_vect()[:, 0], dtype=np.float64)
            yc = self._control_estimates(ctx, ctrl, xc) if P else None
        cap = self.max_local_obs
        if cap is not None:
            if slab:
                raise ValueError("%s: max_local_obs does not combine with vertical / temporal / variable localisation "
                                 "(DESIGN.md 7y-8)" % type(self).__name__)
            ob_class, caps = _cap_classes(cap, self.obs)
        cv = self.cross_validation
        if cv is not None:
            cv = _cross_validation(cv, M)
            if slab or ci is not None or ctrl is not None:
                raise ValueError("%s: cross_validation does not combine with vertical / temporal / variable localisation, "
                                 "column_inflation or control (DESIGN.md 7y-9)" % type(self).__name__)
        try:
            if cv is not None:
                cv_stats = ctx.empty((sy * sx, 2))
                ctx.set_letkf_cross_validation(cv, cv_stats)
            if cap is not None:
                reach = ctx.empty((sy * sx,))
                ctx.set_letkf_obs_cap(ob_class, caps, reach, P=P)
            if ctrl is not None:
                xc_dev, xc_post = ctx.to_device(xc), ctx.empty((max(N, 1),))
                yc_dev = yc_post = None
                if P:
                    yc_dev, yc_post = ctx.to_device(yc), ctx.empty((P,))
                ctx.set_letkf_control(xc_dev, xc_post, yc_dev, yc_post)
            if slab:
                group_of, ng = ctx.letkf_slab_groups(n_lead)
            stats = ctx.empty((ng * sy * sx, 3))
            if ci is not None:                  # one factor per solve point, in the statistics' layout
                lam_shape = ((ng,) if slab else ()) + (sy, sx)
                lam_b = ci.field(lam_shape).copy()
                lam_dev = ctx.to_device(lam_b.reshape(-1))
                lam_stats = ctx.empty((ng * sy * sx, 4))
                cols = lam_b.reshape(ng, sy, sx)
                if mesh:
                    cols = expand_nodes(cols, node_y, node_x, ny, nx)
                lam_ob = self._ob_inflation(ctx, P, cols.reshape(ng, ny * nx), group_of if slab else np.zeros(n_lead, dtype=np.int64))
                lam_ob_dev = None if lam_ob is None else ctx.to_device(np.clip(lam_ob, ci.lower, ci.upper))   # (held: an address)
                ctx.set_letkf_inflation(lam_dev, lam_ob_dev, P, ci.sigma_b, ci.lower, ci.upper, lam_stats)
            diag = ctx.letkf_cycle(N, M, P, X, X, ym, Yp, *(ob[:3] + ob[4:] + geometry), col_stats=stats,
                                   f32=prior.dtype == np.float32, _slab=slab, **mesh)
        finally:
            if slab:                            # the context is shared per device: the settings do not outlive the update
                ctx.set_vertical_localization(None)
                ctx.set_slab_localization(None)
            if ci is not None:
                ctx.set_letkf_inflation(None)
            if ctrl is not None:
                ctx.set_letkf_control(None)
            if cap is not None:
                ctx.set_letkf_obs_cap(None, None)
            if cv is not None:
                ctx.set_letkf_cross_validation(None)
        st = stats.download().reshape(ng, sy, sx, 3)
        if not slab:                            # the plain filter documents (ny, nx) / (nyn, nxn)
            st = st[0]
        self.last_solve = dict(n_local=st[..., 0].astype(np.int64), dfs=st[..., 1].copy(), sweeps=st[..., 2].astype(np.int64))
        if slab:
            self.last_solve.update(group_of_slab=group_of.astype(np.int64).reshape(prior.nvars(), prior.ntimes()))
        if mesh:
            self.last_solve.update(node_y=node_y, node_x=node_x)
        if cap is not None:
            self.last_solve.update(n_reach=reach.download().reshape(sy, sx).astype(np.int64))
        if cv is not None:
            cvs = cv_stats.download().reshape(sy, sx, 2)
            self.last_solve.update(cv_sweeps=cvs[..., 0].astype(np.int64), cv_cond=cvs[..., 1].copy())
        if ci is not None:
            ci.values = lam_dev.download().reshape(lam_shape)       # the next update's prior factors
            self.last_solve.update(inflation=lam_b, inflation_post=ci.values.copy(),
                                   inflation_stats=lam_stats.download().reshape(lam_shape + (4,)))
        if ctrl is not None:
            post = type(ctrl)(OrderedDict((n, v.copy()) for n, v in ctrl.variables.items()), deepcopy(ctrl.coords))
            post.from_vect(xc_post.download()[:N].reshape(N, 1))
            ob_post = np.where(diag["assimilated"], yc_post.download(), np.nan) if P else np.zeros(0)
            self.last_control = dict(state=post, ob_prior=yc if P else np.zeros(0), ob_post=ob_post)
        return diag

    def _control_estimates(self, ctx, ctrl, xc):
        """H(x_c) (P,): the default point interpolation's stencils on the control's rows, or the obs' own `estimate`."""
        if self._default_forward_operator():
            idx, wts = self._interp_stencils_host(ctx)
            yc = np.zeros(idx.shape[0])
            for j in range(idx.shape[1]):           # entry by entry, as the forward kernel sums them
                on = (idx[:, j] >= 0) & (wts[:, j] != 0.0)
                yc[on] += wts[on, j] * xc[idx[on, j]]
            return yc
        return np.array([np.asarray(ob.estimate(ctrl), dtype=np.float64).reshape(-1)[0] for ob in self.obs], dtype=np.float64)

    def _ob_inflation(self, ctx, P, field_cols, group_of):
        """The factor of every ob's own solve: its point interpolation applied to the field (ngroups, ncol); None (1.0 for all)
        without obs and for user-defined forward operators."""
        if not P or not self._default_forward_operator():
            return None
        idx, wts = self._interp_stencils_host(ctx)
        return ob_factors(field_cols, group_of, idx, wts)

    def update_arrays(self, xbm, Xbp):
        raise ValueError("LETKF does not offer update_arrays (out of scope, DESIGN.md 7y); use update()")


class SlabLETKF(LETKF):
    """The LETKF under vertical, temporal and cross-variable localisation: `LETKF` plus the keywords
    vert_coord, time_localize and var_impact of `EnSRF`, validated as there and read from the observations' `vert`,
    `vert_localize_radius`, `time` and `time_localize_radius`.  One solve per (slab group, column); everything else `LETKF`
    refuses is refused here.  With none of the three given it is `LETKF` bit for bit (the plain entry point is called)."""
    _served = ("vert_coord", "time_localize", "var_impact")
