"""Host-side predictor of the Phase-A leaders' cancellation guard (test infrastructure).

The band leader (`k_pipe_band`) and the Gram leader (`k_pipe_gram`) abandon their launch -- and the host hands
Phase A to the vector-chain kernel (`phase_a_kind` 1) -- when an assimilated ob's `G_kk` at its own step is at most
1e-3 of its value at the start of its 64-row block (efa_pipeline_band.hip, the "Cancellation" guard;
efa_pipeline_gram.hip, `thr_ld`).  The rows are centred, so `G_kk = M np.var(row)`: the guard's quantity is
np.var of ob k's row at its step (the oracle's `prior_var[k]`) over np.var of the same row at the step that starts
its block.  Blocks are 64 launch rows counted from the start of the persistent launch's window; a launch holds at
most 256 x 64 rows, less the carried transform rows (efa_phase_a.hip, the Phase-A window loop).

Use: pass a `GuardProbe` as `step_hook` to `oracle.ensrf_update` (any state rows may ride along: the obs rows do
not depend on them), then `probe.min_ratio()`; `expected_kind` maps it onto the kernel the library should report.
"""
import numpy as np

from oracle import ensrf_oracle as orc

ROWS_PER_BLOCK = 64
MAX_LAUNCH_ROWS = 256 * 64
MAX_PIPELINE_M = 128   # no persistent Phase-A kernel takes more members: the per-batch kernels (kind 2) serve them
TRIPS_AT = 1e-3        # the kernels' threshold
SAFE = 2e-3            # a test that expects the band leader keeps its obs at least this far from the threshold
FALLS_BACK = 5e-4      # ... and one that expects the fallback at least this far below it


def window_starts(P, extra=0):
    """First ob of every Phase-A window (efa_phase_a.hip: Wone / Wmax); `extra` = carried transform rows
    (M without localisation on the transform / auto paths, else 0)."""
    wone = MAX_LAUNCH_ROWS - extra
    wmax = wone if P <= wone else wone - extra
    return list(range(0, P, wmax))


class GuardProbe:
    """`step_hook` for `orc.ensrf_update`: records np.var of each ob row at the start of its 64-row block."""

    def __init__(self, nstate, ob_assim, extra=0):
        self.nstate = int(nstate)
        self.asm = np.asarray(ob_assim, dtype=bool)
        P = len(self.asm)
        self.var0 = np.full(P, np.nan)
        self.var_step = np.full(P, np.nan)
        ws = window_starts(P, extra) + [P]
        self.block_end = {}
        for w0, w1 in zip(ws[:-1], ws[1:]):
            for b0 in range(w0, w1, ROWS_PER_BLOCK):
                self.block_end[b0] = min(b0 + ROWS_PER_BLOCK, w1)

    def __call__(self, k, xam, Xap):
        r = self.nstate + k
        e = self.block_end.get(k)
        if e is not None:
            self.var0[k:e] = np.var(Xap[r:self.nstate + e], axis=1)
        self.var_step[k] = np.var(Xap[r])

    def ratios(self):
        """var at the ob's step / var at its block's start, assimilated obs only (0 where the row had no variance
        at block start: G_kk = 0 is not above its threshold either)."""
        v0, v = self.var0[self.asm], self.var_step[self.asm]
        assert np.isfinite(v0).all(), "the oracle run did not visit every block start"
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(v0 > 0, v / v0, 0.0)

    def min_ratio(self):
        r = self.ratios()
        return float(r.min()) if r.size else np.inf


def expected_kind(min_ratio, M=100):
    """Kind the band leader's request must end in: 4 (band leader), 1 (guard tripped: vector chain), 2 (more members
    than any persistent kernel takes) -- or None when the obs sit too close to the threshold to say."""
    if M > MAX_PIPELINE_M:
        return 2
    if min_ratio >= SAFE:
        return 4
    if min_ratio <= FALLS_BACK:
        return 1
    return None


def obs_block_min_ratio(HX, ob_value, ob_error, ob_assim, extra=0, ob_lat=None, ob_lon=None, ob_halfwidth=None):
    """The guard's min ratio for an obs block given as its (P, M) ensemble estimates: the oracle on the obs rows alone
    (vector obs-obs taper when localised).  Returns (min ratio, the oracle's diagnostics)."""
    ym0, Yp0 = orc.compute_ob_priors(HX)
    probe = GuardProbe(0, ob_assim, extra)
    kw = {}
    if ob_lat is not None:
        kw = dict(loc="GC", ob_lat=ob_lat, ob_lon=ob_lon, ob_halfwidth=ob_halfwidth, grid_lat=np.zeros((1, 0)),
                  grid_lon=np.zeros((1, 0)), state_shape=(1, 1, 1, 0), obs_taper="vector")
    _, _, diag = orc.ensrf_update(ym0, Yp0, 0, ob_value, ob_error, ob_assim, step_hook=probe, **kw)
    return probe.min_ratio(), diag
