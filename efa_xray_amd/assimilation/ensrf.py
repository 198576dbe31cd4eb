"""EnSRF: serial ensemble square-root filter, computed on an MI355X.

Drop-in for the reference's `EnSRF(Assimilation)`
(efa_xray/assimilation/ensrf.py:8-151): same constructor
`EnSRF(state, obs, nproc=1, inflation=None, verbose=True, loc=False)`, same
`.update() -> (post_state, obs)` with `post_state` a new object and the five
diagnostics (`prior_mean, prior_var, post_mean, post_var, assimilated`,
ensrf.py:66,70,75,146-149) written onto each `Observation` in place.

The per-observation loop (ensrf.py:50-149) does not exist in Python here:
`update()` marshals the state vector and the per-ob scalars into flat arrays
and calls libefa_hip (`efa_obs_phase_dev` + `efa_state_cycle_dev`).  If the
library or a gfx950 GPU is missing the call raises -- there is no NumPy path.
"""
import numbers

import numpy as np

from efa_xray_amd import _lib
from efa_xray_amd.assimilation.adaptive_inflation import AdaptiveInflation
from efa_xray_amd.assimilation.assimilation import Assimilation
from efa_xray_amd.assimilation.sampling_error import sec_setting
from efa_xray_amd.observation.observation import check_vert_halfwidth


def relaxation_setting(rtps=None, rtpp=None):
    """(kind, alpha) for efa_ctx_set_relaxation from the `rtps` / `rtpp` keywords; ValueError on a bad pair."""
    if rtps is not None and rtpp is not None:
        raise ValueError("rtps and rtpp are exclusive: set at most one of them")
    for name, val, top in (("rtps", rtps, None), ("rtpp", rtpp, 1.0)):
        if val is None:
            continue
        try:
            a = float(val)
        except (TypeError, ValueError):
            raise ValueError("%s=%r: expected a number" % (name, val))
        if not np.isfinite(a) or a < 0.0 or (top is not None and a > top):
            raise ValueError("%s=%r: expected a finite number in [0, %s]" % (name, val, "inf)" if top is None else "1]"))
        return (_lib.RELAX_RTPS if name == "rtps" else _lib.RELAX_RTPP), a
    return _lib.RELAX_NONE, 0.0


def vertical_setting(state, vert_coord, loc, adaptive=None):
    """vert_coord as a float64 (nvars, ntimes) array, or None; ValueError on a setting that is not supported."""
    if vert_coord is None:
        return None
    if loc != 'GC':
        raise ValueError("vert_coord needs loc='GC' (the vertical factor multiplies the Gaspari-Cohn taper); got loc=%r" % (loc,))
    if adaptive is not None:
        raise ValueError("vert_coord cannot be combined with adaptive_inflation (not supported, DESIGN.md 7d)")
    try:
        z = np.array(vert_coord, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("vert_coord must be a float array of shape (nvars, ntimes)")
    want = (state.nvars(), state.ntimes())
    if z.shape != want:
        raise ValueError("vert_coord has shape %r but the state has (nvars, ntimes) = %r" % (z.shape, want))
    if np.isinf(z).any():
        raise ValueError("vert_coord holds an infinite value (NaN marks a slab that is not localised vertically)")
    return z


def ob_vertical(obs):
    """(vert, vert half-width) of every ob as float64 arrays, NaN where missing; ValueError on a bad half-width."""
    ov = np.full(len(obs), np.nan)
    oh = np.full(len(obs), np.nan)
    for k, ob in enumerate(obs):
        c = getattr(ob, "vert_localize_radius", None)
        if c is not None:
            oh[k] = check_vert_halfwidth(c, "observation %d: vert_localize_radius" % k)
        z = getattr(ob, "vert", None)
        if z is not None:
            z = float(z)
            if np.isinf(z):
                raise ValueError("observation %d: vert=%r is infinite" % (k, ob.vert))
            ov[k] = z
    return ov, oh


def time_lags(validtime, times):
    """float64 lags of `times` relative to validtime[0]: hours when validtime is datetime64 (times are then anything
    numpy.datetime64 accepts), else in validtime's own unit (times are numbers).  None gives NaN; ValueError on a time that
    is not finite (NaT included)."""
    vt = np.asarray(validtime)
    if vt.size == 0:
        raise ValueError("the state has no valid times")
    out = np.full(len(times), np.nan)
    for i, t in enumerate(times):
        if t is None:
            continue
        try:
            if vt.dtype.kind == "M":
                lag = (np.datetime64(t) - vt.reshape(-1)[0]) / np.timedelta64(1, "h")
            else:
                lag = float(t) - float(vt.reshape(-1)[0])
        except (TypeError, ValueError):
            raise ValueError("time %r cannot be compared with the state's validtime (dtype %s)" % (t, vt.dtype))
        lag = float(lag)
        if not np.isfinite(lag):
            raise ValueError("time %r is not finite" % (t,))
        out[i] = lag
    return out


def slab_setting(state, loc, time_localize, var_impact, adaptive=None):
    """(time_localize, impact) from the `time_localize` / `var_impact` keywords, or None when both are off:
    impact is None or (obtypes, table) with one row of the float64 table [len(obtypes)][nvars] per obtype var_impact names.
    ValueError on a setting that is not supported."""
    time_localize = bool(time_localize)
    if not time_localize and not var_impact:
        return None
    what = "time_localize" if time_localize else "var_impact"
    if loc != 'GC':
        raise ValueError("%s needs loc='GC' (the factor multiplies the Gaspari-Cohn taper); got loc=%r" % (what, loc))
    if adaptive is not None:
        raise ValueError("%s cannot be combined with adaptive_inflation (not supported, DESIGN.md 7t)" % what)
    if time_localize:
        time_lags(state.coords["validtime"], list(np.asarray(state.coords["validtime"]).reshape(-1)))
    impact = None
    if var_impact:
        names = state.vars()
        if not isinstance(var_impact, dict):
            raise ValueError("var_impact must be a dict {obtype: {state variable: impact in [0, 1]}}, got %r" % type(var_impact).__name__)
        obtypes = list(var_impact)
        table = np.ones((len(obtypes), len(names)))
        for g, obtype in enumerate(obtypes):
            row = var_impact[obtype]
            if not isinstance(row, dict):
                raise ValueError("var_impact[%r] must be a dict {state variable: impact}, got %r" % (obtype, type(row).__name__))
            for name, val in row.items():
                if name not in names:
                    raise ValueError("var_impact[%r] names %r, which is not a state variable (%r)" % (obtype, name, names))
                try:
                    c = float(val)
                except (TypeError, ValueError):
                    raise ValueError("var_impact[%r][%r]=%r: expected a number" % (obtype, name, val))
                if not (np.isfinite(c) and 0.0 <= c <= 1.0):
                    raise ValueError("var_impact[%r][%r]=%r: expected a finite number in [0, 1]" % (obtype, name, val))
                table[g, names.index(name)] = c
            if obtype in names and table[g, names.index(obtype)] != 1.0:
                raise ValueError("var_impact[%r][%r] must be 1: an observation's taper against itself stays 1" % (obtype, obtype))
        impact = (obtypes, table)
    return time_localize, impact


def ob_slab(state, obs, setting):
    """The arrays of Context.set_slab_localization for these obs, as a dict of its keywords; ValueError on a bad half-width or time."""
    time_localize, impact = setting
    nvar, nt, P = state.nvars(), state.ntimes(), len(obs)
    kw = dict(n_lead=nvar * nt, P=P)
    if time_localize:
        vt = state.coords["validtime"]
        kw["lead_time"] = np.tile(time_lags(vt, list(np.asarray(vt).reshape(-1))), nvar)
        oh = np.full(P, np.nan)
        for k, ob in enumerate(obs):
            c = getattr(ob, "time_localize_radius", None)
            if c is not None:
                oh[k] = check_vert_halfwidth(c, "observation %d: time_localize_radius" % k)
        try:
            kw["ob_time"] = time_lags(vt, [getattr(ob, "time", None) for ob in obs])
        except ValueError as e:
            raise ValueError("observation times: %s" % e)
        kw["ob_time_halfwidth"] = oh
    if impact is not None:
        names = state.vars()
        obtypes, table = impact
        kw["lead_var"] = np.repeat(np.arange(nvar, dtype=np.int32), nt)
        kw["ob_group"] = np.array([obtypes.index(ob.obtype) if ob.obtype in obtypes else -1 for ob in obs], dtype=np.int32)
        kw["ob_var"] = np.array([names.index(ob.obtype) if ob.obtype in names else -1 for ob in obs], dtype=np.int32)
        kw["impact"] = table
    return kw


def stream_setting(streamed, chunk_cols, pinned_limit_mb, adaptive=None):
    """(streamed, chunk_cols or None, pinned limit in bytes) from the `streamed` / `stream_chunk_cols` /
    `stream_pinned_limit_mb` keywords; ValueError on a setting that is not supported."""
    streamed = bool(streamed)
    if chunk_cols is not None:
        if isinstance(chunk_cols, bool) or not isinstance(chunk_cols, numbers.Integral) or chunk_cols < 1:
            raise ValueError("stream_chunk_cols must be a positive integer or None, got %r" % (chunk_cols,))
        chunk_cols = int(chunk_cols)
    if isinstance(pinned_limit_mb, bool) or not isinstance(pinned_limit_mb, numbers.Real) or not pinned_limit_mb >= 0:
        raise ValueError("stream_pinned_limit_mb must be a number >= 0, got %r" % (pinned_limit_mb,))
    if streamed and adaptive is not None:
        raise ValueError("streamed=True cannot be combined with adaptive_inflation (its field update needs the whole state "
                         "resident, DESIGN.md 7f)")
    return streamed, chunk_cols, int(float(pinned_limit_mb) * (1 << 20))


def outlier_setting(threshold):
    """The outlier threshold as a float, or None when off; ValueError unless a finite number > 0."""
    if threshold is None:
        return None
    if isinstance(threshold, bool) or not isinstance(threshold, numbers.Real):
        raise ValueError("outlier_threshold must be a number > 0 or None, got %r" % (threshold,))
    t = float(threshold)
    if not (np.isfinite(t) and t > 0.0):
        raise ValueError("outlier_threshold must be a finite number > 0 (None: off), got %r" % (threshold,))
    return t


class EnSRF(Assimilation):
    def __init__(self, state, obs, nproc=1, inflation=None, verbose=True, loc=False, **kw):
        """Extra keyword-only options (all default to reference behaviour):
        device   -- HIP device ordinal (default 0)
        obs_batch-- observations fused per sweep launch (1..64)
        path     -- 'auto' | 'sweep' | 'transform' (how the state sweep runs)
        rtps     -- posterior relaxation to prior spread, factor >= 0 (Whitaker & Hamill 2012)
        rtpp     -- posterior relaxation to prior perturbations, factor in [0, 1]
                    (at most one of the two; None: no relaxation)
        adaptive_inflation -- an AdaptiveInflation: its field inflates the prior and is updated
                    from the innovations by every update() (Anderson 2009); needs
                    loc='GC' and excludes inflation=
        vert_coord -- vertical localisation: float array (nvars, ntimes) in
                    state.vars() order, the vertical coordinate of each 2-D slab (NaN: not
                    localised vertically); obs taper with their `vert` and `vert_localize_radius`.
                    Needs loc='GC'; excludes adaptive_inflation.  None: off
        time_localize -- temporal localisation: True multiplies the taper of ob k on a
                    slab valid at t_s (and on an ob at t_j) by GC(|t_s - t_k|, tau_k), tau_k the ob's
                    attribute `time_localize_radius` (set it after construction); times are lags from validtime[0], in hours when validtime is
                    datetime64, else in validtime's unit, and tau is in the same unit.  An ob without
                    `time` or `time_localize_radius` tapers nothing in time.  Default False
        var_impact -- cross-variable localisation: {obtype: {state variable: c}} with
                    0 <= c <= 1, the factor an ob of that obtype takes on that variable's slabs (and
                    on obs of that variable); pairs left out are 1, and an obtype's impact on the
                    variable of its own name must be 1.  None or {}: off.
                    Both need loc='GC', exclude adaptive_inflation and combine freely with vert_coord,
                    rtps / rtpp, outlier_threshold, streamed and float32 states
        outlier_threshold -- gross-error check, a number t > 0: an ob asked to be
                    assimilated is rejected (assimilated False, nothing updated by it) when
                    (value - prior mean)^2 > t^2 (prior variance + error), checked once per
                    update against the prior.  None: off
        sampling_error_correction -- Anderson's (2012) correction of the gain for sampling error
                    (DESIGN.md 7w): True damps the gain of every (row, ob) pair by the factor
                    alpha(|r|; M) of `sampling_error_table(M)` at the pair's sample correlation r; an
                    array of 2..512 factors >= 0 is used in its place (node j at |r| = j/(T-1), read
                    piecewise linearly).  Needs loc='GC'; excludes adaptive_inflation, vert_coord,
                    time_localize / var_impact, streamed and update_arrays; combines with rtps / rtpp,
                    outlier_threshold, inflation= and float32 states.  None or False: off
        streamed -- True: the prior stays in host memory and crosses the device in chunks of (y, x)
                    columns, upload, state phase and download overlapping; device
                    memory for the state is three chunks.  Same results bit for bit.  The posterior's
                    member arrays then lie in page-locked memory of the context (fed back as the next
                    prior they move by DMA; `EnsembleState.pinned_copy` makes a first prior like
                    that).  Excludes adaptive_inflation and update_arrays.  Default False
        stream_chunk_cols -- columns per chunk, a positive integer (cut to a multiple of 16); None:
                    about 64 MB per chunk
        stream_pinned_limit_mb -- page-locked posterior memory allowed in use at once (default 4096);
                    above it the posterior arrays are ordinary ones and the download is staged

        A state stored as float32 (`EnsembleState.from_vardict(..., dtype=numpy.float32)`, `state.astype`)
        stays float32 from end to end -- upload, device memory, download, posterior -- while every number
        is computed in float64: the posterior is the float64 result rounded once.  The
        obs-space estimates come from the host gather of the stencil rows (`streamed_ob_estimates`),
        user-defined `estimate` operators see the float32 state object, and `inflation=` scales in
        float64 and rounds once.  With a float32 state `adaptive_inflation` raises ValueError (its
        field update is float64 only), and so do `update_arrays` and `ShardedEnSRF`.
        """
        device = kw.pop("device", 0)
        self.obs_batch = kw.pop("obs_batch", None)
        self.path = kw.pop("path", None)
        rtps = kw.pop("rtps", None)
        rtpp = kw.pop("rtpp", None)
        adaptive = kw.pop("adaptive_inflation", None)
        vert_coord = kw.pop("vert_coord", None)
        outlier_threshold = kw.pop("outlier_threshold", None)
        time_localize = kw.pop("time_localize", False)
        var_impact = kw.pop("var_impact", None)
        streamed = kw.pop("streamed", False)
        sec = kw.pop("sampling_error_correction", None)
        stream_chunk_cols = kw.pop("stream_chunk_cols", None)
        stream_pinned_limit_mb = kw.pop("stream_pinned_limit_mb", 4096)
        if kw:
            raise TypeError("unexpected keyword arguments %r" % sorted(kw))
        self.relaxation = relaxation_setting(rtps, rtpp)
        self.outlier_threshold = outlier_setting(outlier_threshold)
        if adaptive is not None:
            if not isinstance(adaptive, AdaptiveInflation):
                raise ValueError("adaptive_inflation must be an AdaptiveInflation, got %r" % type(adaptive).__name__)
            if loc != 'GC':
                raise ValueError("adaptive_inflation needs loc='GC' (Anderson 2009 is defined per state element, "
                                 "weighted by localisation); got loc=%r" % (loc,))
            if inflation is not None:
                raise ValueError("adaptive_inflation and inflation= are exclusive: the adaptive field is the prior inflation")
            adaptive.check_state(state)
        if adaptive is not None and state.dtype == np.float32:
            raise ValueError("adaptive_inflation does not support a float32 state (its field update is float64 only, "
                             "DESIGN.md 7g); use state.astype(numpy.float64)")
        self.adaptive_inflation = adaptive
        self.streamed, self.stream_chunk_cols, self.stream_pinned_limit = stream_setting(
            streamed, stream_chunk_cols, stream_pinned_limit_mb, adaptive)
        self.last_stream = None
        self.vert_coord = vertical_setting(state, vert_coord, loc, adaptive)
        if self.vert_coord is not None:
            ob_vertical(obs)
        self.slab = slab_setting(state, loc, time_localize, var_impact, adaptive)
        if self.slab is not None:
            ob_slab(state, obs, self.slab)
        self.sec_table = sec_setting(sec, state.nmems(), loc, adaptive, self.vert_coord, self.slab, self.streamed)
        Assimilation.__init__(self, state, obs, nproc, inflation, verbose, device=device)
        self.loc = loc
        self.last_timing = None

    # ------------------------------------------------------------------
    def _loc_mode(self):
        if self.loc in (None, False):
            return _lib.LOC_NONE
        if self.loc == 'GC':
            return _lib.LOC_GC
        # ensrf.py:99-101 passes any other truthy value to Observation.localize,
        # which then hits an unbound local (observation.py:77-87)
        raise ValueError("loc=%r: supported values are None, False and 'GC'" % (self.loc,))

    def _ob_arrays(self, loc_mode):
        obs = self.obs
        P = len(obs)
        value = np.array([float(ob.value) if ob.assimilate_this else
                          (np.nan if ob.value is None else float(ob.value)) for ob in obs], dtype=np.float64)
        error = np.array([float(ob.error) if ob.assimilate_this else
                          (np.nan if ob.error is None else float(ob.error)) for ob in obs], dtype=np.float64)
        assim = np.array([bool(ob.assimilate_this) for ob in obs], dtype=bool)
        lat = lon = hw = None
        if loc_mode == _lib.LOC_GC:
            # the reference reads localize_radius only for obs it assimilates (ensrf.py:74-76 precedes :101)
            for k, ob in enumerate(obs):
                if ob.assimilate_this and ob.localize_radius is None:
                    raise ValueError("observation %d has localize_radius=None but loc='GC' "
                                     "(the reference raises TypeError in abs(None), observation.py:120)" % k)

            # lat/lon of EVERY ob enter the obs-obs taper (ensrf.py:113), assimilated or not
            lat = np.array([float(ob.lat) for ob in obs], dtype=np.float64)
            lon = np.array([float(ob.lon) for ob in obs], dtype=np.float64)
            hw = np.array([float(ob.localize_radius) if ob.localize_radius is not None else np.nan
                           for ob in obs], dtype=np.float64)
        return P, value, error, assim, lat, lon, hw

    def _configure(self, ctx):
        if self.obs_batch is not None:
            ctx.set_option("obs_batch", int(self.obs_batch))
        path = {None: _lib.PATH_AUTO, "auto": _lib.PATH_AUTO, "sweep": _lib.PATH_SWEEP,
                "transform": _lib.PATH_TRANSFORM}[self.path]
        ctx.set_option("path", path)
        ctx.set_option("obs_solver", 0)        # the serial loop (ETKF sets 1 behind this): every call, the context is shared per device
        ctx.set_relaxation(*self.relaxation)   # every call: the context is shared per device
        ctx.set_adaptive_inflation(None)        # set by update() around its own cycle only
        ctx.set_outlier_threshold(self.outlier_threshold)  # every call, "off" included
        ctx.set_sampling_error_correction(self.sec_table)  # likewise
        if self.vert_coord is None:             # every call as well, "off" included
            ctx.set_vertical_localization(None)
        else:
            if self.vert_coord.shape != (self.prior.nvars(), self.prior.ntimes()):
                raise ValueError("vert_coord has shape %r but the state has (nvars, ntimes) = %r"
                                 % (self.vert_coord.shape, (self.prior.nvars(), self.prior.ntimes())))
            ov, oh = ob_vertical(self.obs)
            ctx.set_vertical_localization(self.vert_coord.reshape(-1), ov, oh)
        if self.slab is None:                   # and the temporal / variable setting, "off" included
            ctx.set_slab_localization(None)
        else:
            ctx.set_slab_localization(**ob_slab(self.prior, self.obs, self.slab))

    def _write_diagnostics(self, diag):
        """The five diagnostics onto the observations, as ensrf.py:66,70,75,146-149."""
        for k, ob in enumerate(self.obs):
            ob.prior_mean = np.float64(diag["prior_mean"][k])
            ob.prior_var = np.float64(diag["prior_var"][k])
            if diag["assimilated"][k]:
                ob.post_mean = np.float64(diag["post_mean"][k])
                ob.post_var = np.float64(diag["post_var"][k])
                ob.assimilated = True
            else:
                ob.assimilated = False

    def _say(self, line):
        if self.verbose:
            print(line)

    def _column_geometry(self, loc_mode):
        """(grid_lat, grid_lon, n_lead) of a call: the columns' positions and the slabs on each under the 2-D taper
        (ensrf.py:108-111); (None, None, 1) without localisation."""
        if loc_mode != _lib.LOC_GC:
            return None, None, 1
        grid_lat, grid_lon = self.prior.column_latlon()
        return grid_lat, grid_lon, self.prior.nvars() * self.prior.ntimes()

    def _host_estimates(self, ctx):
        """(P, M) estimates without a resident float64 state: the host gather of the stencil rows, or the obs' own `estimate`."""
        return self.streamed_ob_estimates(ctx) if self._default_forward_operator() else self.compute_ob_estimates()

    def _obs_block(self, ctx, X, P, HX=None):
        """(ym, Yp) on the device: the forward operator, once per ob from the prior, and its mean and perturbations
        (assimilation.py:45-48).  On the device from the resident float64 rows X for the reference's point interpolation, from
        the host for a float32 state and for user-defined operators; HX: estimates the upload step made already."""
        M = self.prior.nmems()
        ym = ctx.empty((max(P, 1),))
        if not P:
            return ym, ctx.empty((1, M))
        if HX is not None:
            Yp = ctx.to_device(HX)
        elif self.prior.dtype == np.float32:
            Yp = ctx.to_device(self._host_estimates(ctx))
        elif self._default_forward_operator():
            Yp = self.device_ob_estimates(ctx, X)
        else:
            Yp = ctx.to_device(self.compute_ob_estimates())
        ctx.form_perts(P, M, Yp, ym, Yp)
        return ym, Yp

    def _check_prior(self):
        """What is checked of the prior the inflation hook left, before any device work."""
        if self.adaptive_inflation is not None:
            self.adaptive_inflation.check_state(self.prior)

    def _upload(self, ctx, P):
        """(X, HX, field): the prior on the device, slab by slab from the variables (no stacked host copy).  Under adaptive
        inflation the field goes up too and inflates the prior ahead of the forward operator: on the device for
        the reference's point interpolation, on the host for user-defined operators (they read the state object), which is
        then the state that is uploaded and whose estimates HX are made here."""
        ai = self.adaptive_inflation
        if ai is None:
            return self._upload_prior(ctx), None, None
        prior = self.prior
        field = ctx.to_device(ai.inflation.to_vect())
        if P and not self._default_forward_operator():
            self.prior = ai.inflate_state(prior)           # for the operators and the upload only
            try:
                return self._upload_prior(ctx), self.compute_ob_estimates(), field
            finally:
                self.prior = prior
        X = self._upload_prior(ctx)
        ctx.inflate_rows(prior.nstate(), prior.nmems(), X, field)
        return X, None, field

    _cycle_line = "Beginning observation loop"

    def _run_cycle(self, ctx, X, P, ym, Yp, ob, geometry, field):
        """Phase A (ensrf.py:50-149 on the obs block) and the state phase, in place on X; returns the diagnostics.  float64: one
        library call, so nothing is enqueued ahead of Phase A's status (efa_ensrf_cycle_dev speculates only into a separate
        posterior buffer).  float32: Phase A in float64, the state phase on the float32 rows."""
        N, M = self.prior.nstate(), self.prior.nmems()
        if self.prior.dtype == np.float32:
            diag = ctx.obs_phase(M, P, ym, Yp, *ob)
            ctx.state_cycle_f32(N, M, X, X, *geometry)
            ctx.synchronize()
            return diag
        ai = self.adaptive_inflation
        if ai is None:
            return ctx.ensrf_cycle(N, M, P, X, X, ym, Yp, *(ob + geometry))
        ctx.set_adaptive_inflation(field, N, ai.lower, ai.upper, ai.sd_lower)
        try:
            diag = ctx.ensrf_cycle(N, M, P, X, X, ym, Yp, *(ob + geometry))
        finally:
            ctx.set_adaptive_inflation(None)
        ai.inflation.from_vect(field.download())           # next cycle's prior inflation
        return diag

    def _update_resident(self, P, ob):
        """update() on a state that fits the device: up, the obs block, the cycle in place, down."""
        self._check_prior()
        ctx = self._context()
        self._configure(ctx)
        ctx.set_option("timing", 1)
        self._say("Converting state to vector")
        X, HX, field = self._upload(ctx, P)
        self._say("Computing observation priors")
        ym, Yp = self._obs_block(ctx, X, P, HX)
        geometry = self._column_geometry(ob[3])
        self._say(self._cycle_line)
        diag = self._run_cycle(ctx, X, P, ym, Yp, ob, geometry, field)
        self.last_timing = ctx.last_timing()
        self._write_diagnostics(diag)
        self._say("Formatting posterior")
        # a NEW state object (assimilation.py:165 deep-copies the prior): coordinates copied, member arrays downloaded
        # straight into their own fresh arrays -- the prior's members are not copied only to be overwritten
        return self._download_posterior(X), self.obs

    def _update_streamed(self, P, ob):
        """update() with the prior left in host memory (efa_ensrf_cycle_host)."""
        from collections import OrderedDict
        from copy import deepcopy
        prior = self.prior
        nvar, nt, ny, nx, M = prior.shape()
        ctx = self._context()
        self._configure(ctx)
        ctx.set_option("timing", 1)
        self._say("Computing observation priors")
        HX = self._host_estimates(ctx) if P else None
        grid_lat, grid_lon, _ = self._column_geometry(ob[3])
        names = prior.vars()
        dt = prior.dtype                          # float32 states stream as float32 (efa_ensrf_cycle_host_f32)
        seg_prior = [np.ascontiguousarray(prior.variables[n], dtype=dt) for n in names]
        # the posterior is a NEW state: member arrays in page-locked memory of the context while the limit allows
        if ctx.pinned_reserve([a.nbytes for a in seg_prior], self.stream_pinned_limit):
            seg_post = [ctx.pinned_empty(a.shape, dt) for a in seg_prior]
        else:
            seg_post = [np.empty(a.shape, dtype=dt) for a in seg_prior]
        chunk_cols = self.stream_chunk_cols
        if chunk_cols is None:
            chunk_cols = _lib.default_chunk_cols(nvar * nt, M, itemsize=dt.itemsize)
        self._say("Beginning observation loop")
        diag = ctx.ensrf_cycle_host(seg_prior, seg_post, ny * nx, M, HX, chunk_cols, *(ob + (grid_lat, grid_lon)))
        self.last_timing = ctx.last_timing()
        self.last_stream = ctx.stream_stats()
        self._write_diagnostics(diag)
        self._say("Formatting posterior")
        post_state = type(prior)(OrderedDict(zip(names, seg_post)), deepcopy(prior.coords))
        return post_state, self.obs

    # ------------------------------------------------------------------
    def update(self):
        self._say("Beginning update sequence")
        loc_mode = self._loc_mode()
        P, value, error, assim, lat, lon, hw = self._ob_arrays(loc_mode)
        if self.prior.dtype == np.float32 and self.adaptive_inflation is not None:
            raise ValueError("adaptive_inflation does not support a float32 state (DESIGN.md 7g)")
        # ensrf.py:44 -> format_prior_state: the inflation hook comes first (assimilation.py:131-134);
        # it may rebind self.prior (per-dimension factors, assimilation.py:96)
        if self.inflation is not None:
            self._say("Inflating Prior State")
            self.inflate_state()
        ob = (value, error, assim, loc_mode, lat, lon, hw)      # as every Context call takes them
        return self._update_streamed(P, ob) if self.streamed else self._update_resident(P, ob)

    # ------------------------------------------------------------------
    def update_arrays(self, xbm, Xbp):
        """Run the loop on the reference's augmented arrays (as returned by
        `format_prior_state`) and return `(xam, Xap)` as handed to
        `format_posterior_state` (ensrf.py:44,151).  Diagnostics are written
        onto the observations."""
        if self.streamed:
            raise ValueError("update_arrays is not available on a streamed filter (it takes the augmented arrays whole); "
                             "use update()")
        if self.prior.dtype == np.float32:
            raise ValueError("update_arrays does not support a float32 state (the augmented arrays are float64, DESIGN.md 7g); "
                             "use update()")
        if self.sec_table is not None:
            raise ValueError("update_arrays does not support sampling_error_correction (out of scope, DESIGN.md 7w); use update()")
        if self.adaptive_inflation is not None:
            raise ValueError("update_arrays does not support adaptive_inflation (out of scope: it runs on the augmented "
                             "arrays without the prior inflation step); use update()")
        loc_mode = self._loc_mode()
        P, value, error, assim, lat, lon, hw = self._ob_arrays(loc_mode)
        N = self.prior.nstate()
        xam = np.array(xbm, dtype=np.float64, order="C")
        Xap = np.array(Xbp, dtype=np.float64, order="C")
        geometry = self._column_geometry(loc_mode)
        ctx = self._context()
        self._configure(ctx)
        self._write_diagnostics(ctx.ensrf_update_host(xam, Xap, N, value, error, assim, loc_mode, lat, lon, hw, *geometry))
        return xam, Xap
