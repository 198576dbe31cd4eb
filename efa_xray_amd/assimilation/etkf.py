"""ETKF: ensemble transform Kalman filter, computed on an MI355X.

All observations are solved at once in ensemble space (Bishop et al. 2001; Hunt et al. 2007, global form): one M x M Gram
contraction over the observations, one symmetric eigenproblem of size M, and the transform pass `EnSRF` already ends with.

    A = (M-1) I + Y~^T Y~ = V diag(mu) V^T,   T = V diag(sqrt((M-1)/mu)) V^T,   w = V diag(1/mu) V^T Y~^T d~
    posterior mean = prior mean + X' w,        posterior perturbations = X' T

with Y~ the prior observation-space perturbations and d~ the innovations, each scaled by 1/sqrt(error).  This is the textbook
Kalman update.  It is NOT interchangeable with `EnSRF`: the reference's serial loop, which `EnSRF` reproduces, divides the gain's
denominator by M (`np.var`) and its numerator by M-1, so it is not an exact Kalman update and no batch filter reproduces it; the
two differ by 1 % to 78 % of the mean increment, most with many accurate observations.  `EnSRF` stays the drop-in for the reference.

Same surface as `EnSRF`: `ETKF(state, obs, ...).update() -> (post_state, obs)` with the five diagnostics written onto each
`Observation` (prior_mean / prior_var of every ob from the prior, not "at its turn in a loop"; post_mean / post_var and
`assimilated` as ever).  After an update `last_solve` holds `eigenvalues` (of Y~^T Y~, descending), `dfs` (trace(HK)), `chi2`
(d^T (H P H^T + R)^-1 d), `n_active` and `sweeps` (Jacobi sweeps of the eigen-solve), or None when there were no observations.
"""
from efa_xray_amd.assimilation.ensrf import EnSRF

# keywords of EnSRF that have no meaning for the batch solver, with the reason given to the caller
_REFUSED = (
    ("adaptive_inflation", "adaptive inflation follows the serial order of the observations, which the batch solve does not have"),
    ("vert_coord", "vertical localisation needs loc='GC'; a localised ETKF is out of scope"),
    ("time_localize", "temporal localisation needs loc='GC'; a localised ETKF is out of scope"),
    ("var_impact", "cross-variable localisation needs loc='GC'; a localised ETKF is out of scope"),
    ("sampling_error_correction", "the sampling error correction acts on the serial gain of one observation at a time"),
    ("path", "the batch solve leaves a transform and nothing for a sweep: the state phase always takes the transform"),
    ("obs_batch", "there is no per-batch sweep under the batch solve"),
)


class ETKF(EnSRF):
    def __init__(self, state, obs, nproc=1, inflation=None, verbose=True, **kw):
        """Keyword-only options, as `EnSRF` has them: device, rtps / rtpp, outlier_threshold, streamed, stream_chunk_cols,
        stream_pinned_limit_mb; float32 states work as they do there.  ValueError, before any device work, for loc other than
        None / False (a localised ETKF is out of scope), adaptive_inflation, vert_coord, time_localize, var_impact,
        sampling_error_correction, path and obs_batch.  `update_arrays` is not offered."""
        loc = kw.pop("loc", False)
        if loc not in (None, False):
            raise ValueError("ETKF: loc=%r is not supported: a localised ETKF is out of scope here; use LETKF (or EnSRF(loc='GC'))" % (loc,))
        for name, why in _REFUSED:
            if name in kw:
                raise ValueError("ETKF does not take %s: %s" % (name, why))
        EnSRF.__init__(self, state, obs, nproc, inflation, verbose, False, **kw)
        self.last_solve = None

    def _configure(self, ctx):
        EnSRF._configure(self, ctx)
        ctx.set_option("obs_solver", 1)

    def update(self):
        self.last_solve = None
        out = EnSRF.update(self)
        if len(self.obs):
            sol = self._context().etkf_solution(self.prior.nmems())
            self.last_solve = {k: sol[k] for k in ("eigenvalues", "dfs", "chi2", "n_active", "sweeps")}
        return out

    def update_arrays(self, xbm, Xbp):
        raise ValueError("ETKF does not offer update_arrays (out of scope, DESIGN.md 7x); use update()")
