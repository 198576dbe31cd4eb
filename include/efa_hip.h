/*
 * efa_hip.h -- C ABI of libefa_hip.so: the MI355X (gfx950) implementation of
 * efa_xray's serial EnSRF assimilation update.
 *
 * Boundary.  The reference (lmadaus/efa_xray) has no FFI; its seam is the
 * `Assimilation` subclass contract
 *     EnSRF(state, obs, nproc=1, inflation=None, verbose=True, loc=False).update()
 * (efa_xray/assimilation/ensrf.py:28-33,151).  This library sits exactly
 * between `format_prior_state` (assimilation.py:120-154) and
 * `format_posterior_state` (assimilation.py:157-171): it replaces the
 * per-observation loop ensrf.py:50-149.  The Python host
 * (efa_xray_amd.assimilation.ensrf.EnSRF) binds these symbols with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions.
 *  - extern "C", plain pointers and sizes.  `double` is IEEE binary64.
 *  - Matrices are row-major with the ensemble member as the fastest axis:
 *    `Xp[row * M + mem]` -- the layout of `EnsembleState.to_vect()`
 *    (efa_xray/state/ensemble.py:110-114).
 *  - Pointers named *_dev are device (HBM) addresses on the context's GPU;
 *    every other pointer is host memory.  Per-observation arrays (length P)
 *    are always host memory.
 *  - The caller owns every buffer.  The library never frees or retains a
 *    caller pointer after the call returns.
 *  - Every function returns 0 on success and a negative efa_status on
 *    failure; efa_last_error() returns a thread-local message.  No C++
 *    exception crosses the ABI.
 *  - One context per GPU.  Calls on one context must be serialised by the
 *    caller.  All work is issued on the context's stream; functions that
 *    return results to host memory synchronise that stream before returning.
 *  - There is NO CPU fallback: without a usable gfx950 device
 *    efa_ctx_create() fails with EFA_ERR_NO_DEVICE.
 */
#ifndef EFA_HIP_H
#define EFA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EFA_ABI_VERSION 1

typedef enum efa_status {
  EFA_OK = 0,
  EFA_ERR_INVALID = -1,    /* bad argument (shape, NULL pointer, option) */
  EFA_ERR_NO_DEVICE = -2,  /* no HIP device / wrong architecture */
  EFA_ERR_HIP = -3,        /* a HIP runtime call failed */
  EFA_ERR_UNSUPPORTED = -4, /* valid request this build cannot serve */
  EFA_ERR_ALLOC = -5        /* a device buffer a call sizes itself could not be allocated (the LETKF's node-pair buffer) */
} efa_status;

/* localisation modes: `loc` of EnSRF (ensrf.py:28,99) */
#define EFA_LOC_NONE 0 /* loc in (None, False) */
#define EFA_LOC_GC 1   /* loc == 'GC': Gaspari-Cohn, observation.py:117-130 */

/* how the state sweep (Phase B) is executed; results agree to ~1e-14 */
#define EFA_PATH_AUTO 0      /* transform when unlocalised and worth it */
#define EFA_PATH_SWEEP 1     /* per-batch fused covariance/gain/update sweep */
#define EFA_PATH_TRANSFORM 2 /* one pass: Xap = Xbp*T, xam = xbm + Xbp*w */

typedef struct efa_ctx efa_ctx;

/* ---- library / context --------------------------------------------------*/
int efa_abi_version(void);
const char *efa_last_error(void);
/* number of visible HIP devices (0 without a GPU; never fails the process) */
int efa_device_count(int *count);
/* create a context on HIP device `device_id` (must be gfx950) */
int efa_ctx_create(int device_id, efa_ctx **out);
int efa_ctx_destroy(efa_ctx *ctx);
/* issue all work on the caller's hipStream_t (e.g. torch's current stream).
 * NULL is the device's legacy default stream.  A new context uses a private
 * non-blocking stream; efa_ctx_set_option(ctx, "own_stream", 1) returns to it.
 * Several calls return with work still in the stream, and that work reads the
 * context's own workspaces: work issued after a change of stream is ordered
 * behind everything the context issued before it (an event on the stream that
 * is left, waited for on the device by the one that takes over; the host does
 * not wait; the stream that is left must still exist at that moment).  The
 * caller's own work on either stream is not ordered by this. */
int efa_ctx_set_stream(efa_ctx *ctx, void *hip_stream);
/* options: "obs_batch" (obs fused per sweep launch, 1..64, default 64),
 *          "path" (EFA_PATH_*), "timing" (0/1/2, see efa_last_timing), "pipeline" (1: run Phase A as
 *          one persistent launch when it applies, 0: per-batch kernels),
 *          "gram" (how the persistent launch leads a 64-ob block: 2 (default) in Gram space in
 *          bands of 4 obs, with or without localisation; 1 in Gram space step by step;
 *          0 on the vectors; the Gram-space leaders fall back to 0 if their cancellation guard trips),
 *          "spin_limit" (bound of the pipeline's in-kernel polls), "spin_ms" (its wall-time
 *          bound: the persistent launch gives up, and the per-batch kernels take over, when a
 *          wave has waited that long -- e.g. because another kernel keeps part of the grid from
 *          becoming resident; -1 = 100 ms + P/100 ms),
 *          "gc_onepass" (1: localised state sweep in one pass with per-column-block
 *          active lists, 0: per-batch taper tables),
 *          "own_stream" (see above),
 *          "obs_solver" (how the obs phase is solved: 0 (default) the serial EnSRF loop, 1 the batch
 *          ensemble-space solve, an ETKF -- a different filter, see efa_etkf_solution);
 *          read-only: "phase_a_kind" (1 pipeline / 2 per-batch / 3 Gram pipeline / 4 band pipeline /
 *          5 batch solver, last call),
 *          "gc_active_pairs"
 *          ((column, ob) pairs with a non-zero taper in the last one-pass sweep),
 *          "gc_family" (the kernel family of the last one-pass sweep: 0 plain, 1 adaptive inflation, 2 vertical factor,
 *          3 slab table, 4 sampling error correction; -1: none ran yet),
 *          "gc_form" (its kernel form: 1 quad per row, 2 row per lane; 0: none ran yet),
 *          "sec_on" (see efa_ctx_set_sampling_error_correction),
 *          "f32_native" (see efa_state_cycle_f32_dev), "impact_us" (see efa_obs_impact_dev),
 *          "sens_us" (see efa_sensitivity_dev), "verify_us" (see efa_verify_dev),
 *          "products_us" (see efa_products_dev), "gram_us" (see efa_gram_dev);
 *          "verify_blocks" (grid cap of efa_verify_dev's pass, 0 = the default of 2048; results do not depend on it),
 *          "products_blocks" (the same for efa_products_dev's pass),
 *          "gram_blocks" (the same for efa_gram_dev's pass);
 *          "neighbourhood_blocks" (the same for efa_neighbourhood_dev's kernels), "nbr_ws_bytes" (a lower cap
 *          of the records that call holds at a time, 0 = EFA_NBR_WS_BYTES; results do not depend on it),
 *          read-only "neighbourhood_us" (see efa_neighbourhood_dev);
 *          "pm_blocks" (the same grid cap for efa_pm_mean_dev's kernels), "pm_ws_bytes" (a lower cap of the
 *          pooled key buffers that call holds at a time, 0 = EFA_PM_WS_BYTES; results do not depend on it),
 *          read-only "pm_us", "pm_passes", "pm_rank_passes" (see efa_pm_mean_dev) */
int efa_ctx_set_option(efa_ctx *ctx, const char *key, long value);
int efa_ctx_get_option(efa_ctx *ctx, const char *key, long *value);

/* ---- posterior inflation by relaxation (Whitaker & Hamill 2012) ----------
 * Context state like "path": every later state phase that writes the caller's
 * state rows (efa_state_phase_dev, efa_state_cycle_dev, efa_ensrf_cycle_dev,
 * efa_ensrf_update_dev, efa_ensrf_update) relaxes each row i of M members,
 * with prior perturbations b_i and posterior perturbations a_i (deviations
 * from the row's member mean):
 *   EFA_RELAX_RTPP: xa_i <- mean(xa_i) + (1-alpha) a_i + alpha b_i, 0 <= alpha <= 1
 *   EFA_RELAX_RTPS: xa_i <- mean(xa_i) + a_i ((1-alpha) + alpha sigma_b/sigma_a),
 *                   alpha >= 0; a row with sigma_a == 0 is left as it is.
 * The prior is the ensemble the call is given.  The obs block and the
 * per-ob diagnostics are not relaxed; alpha == 0, EFA_RELAX_NONE and a cycle
 * with no assimilated ob leave the results bit for bit as without it.
 * Cost: on the unlocalised transform path RTPP is folded into T and RTPS
 * (up to 136 members, member form) is fused into the transform; every other
 * path adds a row-spread pass over the prior and a relaxation pass over the
 * posterior.  RTPP on those paths with the posterior written over the prior
 * keeps a copy of the prior in a context workspace: rows*M*8 bytes more
 * device memory.  Bad kind, NaN or infinite alpha, alpha < 0 or (RTPP)
 * alpha > 1 return EFA_ERR_INVALID. */
#define EFA_RELAX_NONE 0
#define EFA_RELAX_RTPP 1
#define EFA_RELAX_RTPS 2
int efa_ctx_set_relaxation(efa_ctx *ctx, int kind, double alpha);

/* ---- spatially varying adaptive inflation (Anderson 2009) --
 * field_dev: [rows][2] doubles on the device, (mean lambda, sd s) of each
 * state row's VARIANCE inflation factor, in the state's row order.
 * efa_inflate_rows_dev inflates the prior in place, before the forward
 * operator: x_im <- mean_i + sqrt(lambda_i) (x_im - mean_i); rows with
 * lambda == 1 are left bit for bit as they are.
 * efa_ctx_set_adaptive_inflation is context state like the relaxation: while
 * a field is set, every later state phase (efa_state_phase_dev,
 * efa_state_cycle_dev, efa_ensrf_cycle_dev, efa_ensrf_update_dev,
 * efa_ensrf_update) updates it in place, ob by ob in serial order, from the
 * innovations, fused into the one-pass GC sweep; the posterior is the one of
 * the prior it is given.  The call fails (EFA_ERR_INVALID) unless the cycle is
 * GC-localised, option "gc_onepass" is 1 and the state phase has `rows` rows.
 * Bounds: 0 < lower <= upper (finite), sd_lower >= 0 (DART: 1, 1e6, 0).
 * field_dev NULL turns it off.  The field must stay allocated while set. */
int efa_inflate_rows_dev(efa_ctx *ctx, long rows, int M, double *X_dev, const double *field_dev);
int efa_ctx_set_adaptive_inflation(efa_ctx *ctx, double *field_dev, long rows, double lower, double upper,
                                   double sd_lower);

/* ---- vertical localisation of the GC taper --------------
 * Host arrays, copied into the context: lead_vert[n_lead] is the vertical
 * coordinate of each slab (slab s = rows s*ncol .. s*ncol + ncol - 1, the
 * variable-major, then valid-time order), ob_vert[P] and
 * ob_vert_halfwidth[P] those of the observations, in any unit as long as it
 * is the same for all three.  With it every taper weight of a GC cycle --
 * state rows and the obs-obs taper -- is the horizontal one times
 * GC(|z_row - z_k|, c_k), the same Gaspari-Cohn polynomial with ob k's
 * vertical half-width c_k.  A NaN slab coordinate, or an ob whose coordinate
 * or half-width is NaN, takes factor 1 in every pair it is part of.  A
 * half-width that is not NaN must be finite and > 0; coordinates may not be
 * infinite.  lead_vert NULL turns it off.  Context state like the
 * relaxation: while it is set, a later call fails (EFA_ERR_INVALID) unless
 * it is a GC cycle of exactly P observations (and n_lead slabs for the state
 * phase), option "gc_onepass" is 1 and no adaptive-inflation field is set. */
int efa_ctx_set_vertical_localization(efa_ctx *ctx, long n_lead, const double *lead_vert, long P, const double *ob_vert,
                                      const double *ob_vert_halfwidth);

/* ---- temporal and cross-variable localisation of the GC taper
 * Slab s (variable-major, then valid time) has a variable index
 * lead_var[s] in [0, n_var) and a time lead_time[s]; ob k a time ob_time[k],
 * a temporal half-width ob_time_halfwidth[k] (same unit as the times), an
 * impact row ob_group[k] in [0, n_group) (-1: a row of ones) and a target
 * variable ob_var[k] in [0, n_var), the state variable its obtype names
 * (-1: none).  With it every taper weight of a GC cycle is
 *   state row i in slab s:  GC_h(col_i, k) * V(s,k) * T(s,k) * C[k, v_s]
 *   obs row j:              GC_h(j, k)     * V(j,k) * T(j,k) * C[k, v_j]
 * with T(x,k) = GC(|t_x - t_k|, tau_k), the same Gaspari-Cohn polynomial (0
 * from 2 tau_k on) with ob k's half-width, and 1 when t_x, t_k or tau_k is
 * NaN; C[k,v] = impact[ob_group[k]][v] (1 for ob_group[k] = -1 and for an
 * obs row j with ob_var[j] = -1); V the vertical factor of
 * efa_ctx_set_vertical_localization, exactly as without this setting (1 when
 * that is off).  The factor of a slab is formed as (V T) C, each product
 * rounded once.
 * Host arrays, copied into the context.  lead_time NULL: no temporal part
 * (ob_time and ob_time_halfwidth are not read); impact NULL: no variable part
 * (lead_var, ob_group, ob_var, n_var and n_group are not read); both NULL
 * turns the setting off.  Refused (EFA_ERR_INVALID): an impact entry that is
 * not a finite number in [0, 1]; impact[ob_group[k]][ob_var[k]] != 1 (an
 * ob's taper against itself stays 1); a half-width that is neither NaN nor
 * finite and > 0; an infinite time; an index out of range.
 * Context state like the vertical setting, with the same rules: while it is
 * set a later call fails (EFA_ERR_INVALID) unless it is a GC cycle of exactly
 * P observations (and n_lead slabs for the state phase), option "gc_onepass"
 * is 1 and no adaptive-inflation field is set; efa_obs_impact_dev fails while
 * it is set (efa_obs_impact_slab_dev is the impact under these tapers).
 * When no ob has both a time and a half-width and no impact entry of a row
 * in use differs from 1, every factor is 1 and the library runs the kernels
 * it runs without the setting.
 * Setting the same values again is a no-op (cached geometry stays valid).
 *
 * efa_slab_factor_table copies the table S[P][n_lead] of the factors (V T) C
 * the state sweep reads (row k = ob k) to the host array `table` (NULL: the
 * table is only brought up to date on the device); it waits. */
int efa_ctx_set_slab_localization(efa_ctx *ctx, long n_lead, const double *lead_time, const int *lead_var, long n_var, long P,
                                  const double *ob_time, const double *ob_time_halfwidth, const int *ob_group, const int *ob_var,
                                  long n_group, const double *impact /* [n_group][n_var] */);
int efa_slab_factor_table(efa_ctx *ctx, long P, long n_lead, double *table);

/* ---- outlier (gross-error) check ---------------------------
 * Context state like the relaxation, for every later obs phase
 * (efa_obs_phase_dev, efa_ensrf_update_dev, efa_ensrf_cycle_dev,
 * efa_ensrf_update).  With threshold t > 0 each ob the caller asks to
 * assimilate is checked ONCE per call against the obs block it is handed,
 * before any ob of the call is assimilated: with d = value - ym[k],
 * s2 = the variance of Yp[k][0..M-1] (divided by M) and r = error[k], the ob
 * is kept iff d*d <= t*t*(s2 + r) (a NaN rejects it).  A rejected ob is
 * treated exactly as one whose assimilate flag is 0; it comes back with
 * assimilated[k] = 0.  0 turns it off (the default); a negative, NaN or
 * infinite threshold fails with EFA_ERR_INVALID. */
int efa_ctx_set_outlier_threshold(efa_ctx *ctx, double threshold);

/* ---- sampling error correction (Anderson 2012) --------------
 * Context state like the relaxation, for every later GC cycle
 * (efa_obs_phase_dev, efa_state_phase_dev, efa_state_cycle_dev,
 * efa_state_cycle_f32_dev, efa_ensrf_update_dev, efa_ensrf_cycle_dev,
 * efa_ensrf_update).  alpha: a host table of T nodes, 2 <= T <= 512, node j
 * at |r| = j/(T-1), every value finite and >= 0; it is copied.  The gain of
 * ob k on row i (state rows and the rows of the obs block alike) becomes
 *   alpha(|r|) * taper * cov(x_i, y_k) / (var(y_k) + error_k),
 * r the sample correlation of the row and the ob as they are when ob k is
 * reached in serial order (0 if either has no spread), alpha read from the
 * table piecewise linearly (|r| > 1 reads the last node); ob k's own row takes
 * alpha = 1.  A pair with a zero taper leaves the row bit for bit as it is,
 * and a table of ones gives the results of the call without the setting.
 * While it is set a call must use EFA_LOC_GC with "gc_onepass" 1 and none of
 * adaptive inflation, vertical or slab localisation: any other call fails
 * with EFA_ERR_INVALID before it launches anything.  Phase A then runs its
 * per-batch kernels one ob at a time ("phase_a_kind" reads 2).  The
 * relaxation, the outlier check and float32 rows combine with it; the
 * streamed update (efa_ensrf_cycle_host, _f32) refuses it likewise.
 * efa_obs_impact_dev is not changed by it: the impact assumes the
 * uncorrected gain.  NULL or T == 0 turns it off (the default); a bad T or a
 * negative, NaN or infinite value fails with EFA_ERR_INVALID and leaves the
 * setting as it was.  Read-only option "sec_on": 1 while a table is set. */
int efa_ctx_set_sampling_error_correction(efa_ctx *ctx, const double *alpha, int T);
int efa_ctx_synchronize(efa_ctx *ctx);

/* ---- the batch observation-space solver: an ETKF (Bishop et al. 2001; Hunt et al. 2007, global form) ----
 * Option "obs_solver" 1 is context state like "path": every later obs phase
 * (efa_obs_phase_dev, efa_ensrf_cycle_dev, efa_ensrf_update_dev,
 * efa_ensrf_update, efa_ensrf_cycle_host, _f32) solves all observations at
 * once in ensemble space instead of walking them one after another.  With
 * a_k the effective flag of ob k (ob_assim[k], and the outlier check's
 * verdict when a threshold is set), over the obs with a_k = 1:
 *   s_k = 1/sqrt(ob_error[k]), Y~_k = s_k Yp[k,:], d~_k = s_k (ob_value[k] - ym[k]),
 *   C = Y~^T Y~, g = Y~^T d~, q = d~^T d~,
 *   A = (M-1) I + C = V diag(mu) V^T,
 *   T = V diag(sqrt((M-1)/mu)) V^T (the symmetric square root), w = V diag(1/mu) V^T g,
 * and every row, of the state and of the obs block alike (all P obs rows,
 * assimilated or not): xam = xbm + Xbp w, Xap = Xbp T.  The state phase takes
 * the transform whatever "path" says (there are no records for a sweep);
 * relaxation, float32 rows, in-place and out-of-place calls work as ever.
 * Diagnostics: prior_mean = ym and prior_var = the variance (ddof 0) of
 * Yp[k,:] for every ob, from the prior the call is handed; post_mean and
 * post_var (ddof 0) from the mapped obs rows where a_k = 1; assimilated = a.
 * This is the textbook Kalman update.  It is NOT the serial loop: that one
 * (as the reference does) divides the gain's denominator by M and its
 * numerator by M-1, so the two filters differ by 1 % to 78 % of the mean
 * increment, most with many accurate observations.  T 1 = 1 (member means
 * preserved) holds as far as the rows of Yp sum to zero; it is not enforced.
 * An ob with a_k = 0 is never read for value or error.  With no ob assimilated
 * the state calls return what they return under "obs_solver" 0, bit for bit.
 * The same inputs give the same bits (fixed reduction orders, no atomics).
 * Refused with EFA_ERR_INVALID before anything is launched (the context stays
 * usable): EFA_LOC_GC, an adaptive-inflation field, option "path"
 * EFA_PATH_SWEEP, an assimilated ob whose error variance is not finite and
 * > 0 (the batch form divides by it).  "phase_a_kind" reads 5.
 *
 * efa_etkf_solution returns the solution of the last obs phase, which must
 * have run with "obs_solver" 1 for M members (else EFA_ERR_INVALID): T, w,
 * eig = the eigenvalues lambda_i = mu_i - (M-1) of C in descending order,
 * stats = {n_active, q, dfs = sum lambda_i/(M-1+lambda_i) = trace(HK),
 * chi2 = q - g^T w = d^T (H P^b H^T + R)^-1 d}, and the Jacobi sweeps the
 * eigen-solve took (at most 30).  Any output may be NULL; it waits. */
int efa_etkf_solution(efa_ctx *ctx, int M, double *T /*[M*M]*/, double *w /*[M]*/, double *eig /*[M], descending*/,
                      double *stats /*[4]: n_active, q, dfs, chi2*/, long *sweeps);

/* ---- the local ensemble transform Kalman filter (LETKF) -----
 * Hunt, Kostelich & Szunyogh (2007): one ensemble-space solve per column
 * under the Gaspari-Cohn taper, the taper multiplying R^-1 (R-localisation).
 * The inputs are those of efa_ensrf_cycle_dev with EFA_LOC_GC.  With a_k the
 * effective flag as under "obs_solver" 1 (ob_assim[k], and the outlier
 * check's verdict when a threshold is set), rho_k(x) = gaspari_cohn(
 * distance(x, ob k), halfwidth_k) and d_k = value_k - ym_k, for a location x
 * (a grid column or an ob position), over the obs with a_k = 1, rho_k(x) != 0:
 *   C_x = sum_k (rho_k/r_k) Yp_k^T Yp_k,  g_x = sum_k (rho_k/r_k) d_k Yp_k^T,
 *   A_x = (M-1) I + C_x = V diag(mu) V^T,
 *   T_x = V diag(sqrt((M-1)/mu)) V^T,  w_x = V diag(1/mu) V^T g_x.
 * State rows: all n_lead rows of column c (row lead*ncol + c) map with that
 * column's pair, xam = xbm + Xbp w_c, Xap = Xbp T_c.  Obs block: all P rows map,
 * assimilated or not, ob j with the pair solved at (ob_lat[j], ob_lon[j]).
 * Every solve reads the PRIOR obs block; the posterior obs block is written
 * elsewhere and copied into ym_dev / Yp_dev afterwards when obs_block_out is 1
 * (0: both are left untouched).  Diagnostics as under "obs_solver" 1.
 * A column no ob reaches keeps its rows bit for bit, with relaxation too.  An
 * ob with a_k = 0 is never read for value or error.  A NaN value of an
 * assimilated ob poisons w of exactly the columns it reaches.  The same inputs
 * give the same bits.  post_dev == X_dev is allowed (a column's rows are read
 * and written by its own workgroup only); any other overlap is refused.
 * These are entry points of their own: option "obs_solver" is not read.  They
 * honour the context's relaxation (state rows only; RTPP folded into the
 * transform, RTPS per row) and outlier threshold.  Refused with
 * EFA_ERR_INVALID before anything is launched (the context stays usable):
 *   M > 136 (the eigen-solve's M x M array of a column must fit in LDS);
 *   an adaptive-inflation field (its update follows the serial order of the
 *   obs, which a batch solve does not have); vertical or slab (temporal /
 *   cross-variable) localisation (each needs a solve per (slab group, column));
 *   a sampling-error-correction table (it acts on the serial gain of one ob);
 *   an assimilated ob whose error variance is not finite and > 0, or whose
 *   half-width is NaN or 0.
 * col_stats_dev (device, may be NULL) receives per column {n_local = the obs
 * with a_k = 1 and rho != 0, dfs = sum lambda_i/(M-1+lambda_i), Jacobi sweeps
 * (at most 30)}; a column no ob reaches runs no solve and reports (0, 0, 0).
 * Afterwards "phase_a_kind" reads 6, and efa_last_timing gives the list builds
 * and the obs block as obs_ms, the column launch as state_ms.  They wait.
 *
 * efa_letkf_weights_dev solves at npts caller-given points (host arrays
 * pt_lat / pt_lon) and writes [T | w] of each to Tw_dev (device,
 * [npts][M][M+1]: row a = T[a][0..M) then w[a]; never relaxed) and the
 * statistics to stats_dev ([3*npts] or NULL): the probe the tests use, and the
 * solve the weight-interpolation entries below run at the nodes of their mesh. */
int efa_letkf_cycle_dev(efa_ctx *ctx, long rows, int M, long P, const double *X_dev, double *post_dev, double *ym_dev,
                        double *Yp_dev, int obs_block_out, const double *ob_value, const double *ob_error,
                        const uint8_t *ob_assim, const double *ob_lat, const double *ob_lon, const double *ob_halfwidth_km,
                        const double *grid_lat, const double *grid_lon, long ncol, long n_lead, double *prior_mean,
                        double *prior_var, double *post_mean, double *post_var, uint8_t *assimilated,
                        double *col_stats_dev /* [3*ncol] or NULL */);
int efa_letkf_cycle_f32_dev(efa_ctx *ctx, long rows, int M, long P, const float *X_dev, float *post_dev, double *ym_dev,
                            double *Yp_dev, int obs_block_out, const double *ob_value, const double *ob_error,
                            const uint8_t *ob_assim, const double *ob_lat, const double *ob_lon, const double *ob_halfwidth_km,
                            const double *grid_lat, const double *grid_lon, long ncol, long n_lead, double *prior_mean,
                            double *prior_var, double *post_mean, double *post_var, uint8_t *assimilated,
                            double *col_stats_dev /* [3*ncol] or NULL */);
int efa_letkf_weights_dev(efa_ctx *ctx, int M, long P, const double *ym_dev, const double *Yp_dev, const double *ob_value,
                          const double *ob_error, const uint8_t *ob_assim, const double *ob_lat, const double *ob_lon,
                          const double *ob_halfwidth_km, long npts, const double *pt_lat, const double *pt_lon,
                          double *Tw_dev /* [npts][M][M+1] */, double *stats_dev /* [3*npts] or NULL */);

/* ---- LETKF weight interpolation (Yang, Kalnay, Hunt & Bowler 2009)
 * The pair [T | w] varies smoothly in space (it depends on the taper and the
 * obs, not on the state rows), so it is solved at every (stride_y, stride_x)-th
 * column only and interpolated bilinearly, in grid-index space, to the columns
 * in between.  The grid has shape (ny, nx), column c = iy*nx + ix.  Nodes on an
 * axis of n points with stride s >= 1: the indices 0, s, 2s, .. below n-1, and
 * n-1 itself (1 node if n == 1, else ceil((n-1)/s) + 1; the last cell may be
 * shorter); node (jy, jx) has index jy*nxn + jx and the position of its grid
 * column.  Node pairs and statistics are exactly what efa_letkf_weights_dev
 * writes for that position.  Column (iy, ix) lies in the cell [y0,y1] x [x0,x1]
 * of consecutive nodes (on a node line: the cell with y0 < iy); with
 * ty = (iy-y0)/(y1-y0), tx likewise (0 on an axis with one node),
 *   [T_c | w_c] = sum beta_n [T_n | w_n],
 *   beta = (1-ty)(1-tx), (1-ty)tx, ty(1-tx), ty tx on (y0,x0) (y0,x1) (y1,x0) (y1,x1),
 * summed in that order over the corners with beta != 0; a corner with beta == 0
 * is not read (a node column maps with its own pair alone).  Every row of
 * column c maps as xam = xbm + X' w_c, Xap = X' T_c.  RTPP acts on the
 * interpolated T_c, RTPS per row.  The obs block and the diagnostics are those
 * of efa_letkf_cycle_dev bit for bit: ob j is solved at its own position.
 * If every corner in use has n_local = 0 the column's rows come back bit for
 * bit -- also when an ob of short radius reaches the column but none of its
 * nodes: that ob is lost to the column.  Keep the stride (in km) well below
 * the smallest half-width.  A NaN value of an assimilated ob poisons exactly
 * the columns that use a node it reaches.  Same inputs, same bits.  Stride
 * (1, 1) is efa_letkf_cycle_dev itself (node_stats_dev is then col_stats_dev).
 * Refused with EFA_ERR_INVALID before any launch: all that efa_letkf_cycle_dev
 * refuses, a stride < 1, rows != ny*nx*n_lead, a partial overlap of post_dev
 * and X_dev (post_dev == X_dev is allowed).  node_stats_dev ([3*nnodes] or
 * NULL) receives {n_local, dfs, sweeps} of every node.  Afterwards
 * "phase_a_kind" reads 7; efa_last_timing: obs_ms as efa_letkf_cycle_dev (the
 * nodes' lists in the place of the columns'), state_ms the node solve plus the
 * interpolate-and-apply launch, state_launches 2.  They wait.
 *
 * efa_letkf_interp_apply_dev is the second launch alone, on caller-given node
 * pairs Tw_nodes_dev ([nnodes][M][M+1], rows [T[a][0..M) | w[a]]) and
 * node_stats_dev ([3*nnodes], only n_local is read; NULL: every node counts as
 * reached), under the context's relaxation: for pairs solved elsewhere. */
int efa_letkf_cycle_interp_dev(efa_ctx *ctx, long rows, int M, long P, const double *X_dev, double *post_dev, double *ym_dev,
                               double *Yp_dev, int obs_block_out, const double *ob_value, const double *ob_error,
                               const uint8_t *ob_assim, const double *ob_lat, const double *ob_lon, const double *ob_halfwidth_km,
                               const double *grid_lat, const double *grid_lon, long ny, long nx, long stride_y, long stride_x,
                               long n_lead, double *prior_mean, double *prior_var, double *post_mean, double *post_var,
                               uint8_t *assimilated, double *node_stats_dev /* [3*nnodes] or NULL */);
int efa_letkf_cycle_interp_f32_dev(efa_ctx *ctx, long rows, int M, long P, const float *X_dev, float *post_dev, double *ym_dev,
                                   double *Yp_dev, int obs_block_out, const double *ob_value, const double *ob_error,
                                   const uint8_t *ob_assim, const double *ob_lat, const double *ob_lon,
                                   const double *ob_halfwidth_km, const double *grid_lat, const double *grid_lon, long ny, long nx,
                                   long stride_y, long stride_x, long n_lead, double *prior_mean, double *prior_var,
                                   double *post_mean, double *post_var, uint8_t *assimilated,
                                   double *node_stats_dev /* [3*nnodes] or NULL */);
int efa_letkf_interp_apply_dev(efa_ctx *ctx, long rows, int M, const double *X_dev, double *post_dev, long ny, long nx,
                               long stride_y, long stride_x, long n_lead, const double *Tw_nodes_dev,
                               const double *node_stats_dev /* [3*nnodes] or NULL */);
int efa_letkf_interp_apply_f32_dev(efa_ctx *ctx, long rows, int M, const float *X_dev, float *post_dev, long ny, long nx,
                                   long stride_y, long stride_x, long n_lead, const double *Tw_nodes_dev,
                                   const double *node_stats_dev /* [3*nnodes] or NULL */);

/* ---- vertical, temporal and variable localisation of the LETKF
 * The calls above map all n_lead rows of a column with one pair.  These solve
 * once per (slab group, column) under the product taper of 7d / 7t.  Inputs:
 * those of the call of the same name without "_slab", with the context's
 * vertical setting (efa_ctx_set_vertical_localization) and / or slab setting
 * (efa_ctx_set_slab_localization) on, sized for this call's P and n_lead.
 * S(k, s) is the slab factor (V T) C of ob k on slab s, exactly what
 * efa_slab_factor_table returns (V included while the vertical setting is on;
 * under the vertical setting alone S = V).  F(j, k) = (V(j,k) T(j,k)) C[k, v_j] is
 * the factor of ob k on obs row j, each product rounded once in that order.
 * For column c and slab s, over the obs with a_k = 1 and rho_k(c, s) != 0:
 *   rho_k(c, s) = fl(GC_h(c, k) * S(k, s)),  weight_k = fl(rho_k(c, s) / r_k),
 *   A_{c,s} = (M-1) I + sum_k weight_k Yp_k^T Yp_k,  g_{c,s} = sum_k weight_k d_k Yp_k^T,
 * and T, w follow as above; row s*ncol + c maps with the pair of (c, s).  Obs
 * row j maps with the pair solved at ob j's position under fl(GC_h(j,k) F(j,k)).
 * Slabs whose factors agree for every ob form a GROUP and share one solve.  The
 * key of slab s is the bit pattern (every NaN alike) of lead_vert[s] while some
 * ob carries vertical information, lead_time[s] while some ob has a time and a
 * temporal half-width, and lead_var[s] while some ob's impact row has an entry
 * other than 1.  Groups are numbered by first appearance;
 * efa_letkf_slab_groups writes the group of every slab (host, [n_lead]) and
 * their number.  A (column, group) no ob reaches (n_local = 0: every product is
 * 0) runs no solve, keeps that group's rows bit for bit and reports (0, 0, 0).
 * Statistics are laid out [ngroups][ncol][3] (col_stats_dev) or
 * [ngroups][nnodes][3] (node_stats_dev); efa_letkf_slab_weights_dev writes
 * Tw_dev [ngroups][npts][M][M+1] and stats_dev [ngroups][npts][3].  The interp
 * call interpolates per group, node pairs in a buffer of the context of
 * ngroups * nnodes * M * (M+1) doubles (EFA_ERR_ALLOC if it cannot be had); a
 * unit stride is the plain slab call.  Diagnostics, relaxation, the outlier
 * check, float32 rows and every other rule are those of the calls above.  With
 * every S = 1 the results equal the calls above bit for bit.
 * Refused with EFA_ERR_INVALID before any launch: neither setting on (use the
 * plain call); a setting sized for another P or n_lead; and all that the plain
 * call refuses but the two settings.  "phase_a_kind" reads 8 (9 for the interp
 * call); efa_last_timing as for the plain calls.  They wait. */
int efa_letkf_slab_cycle_dev(efa_ctx *ctx, long rows, int M, long P, const double *X_dev, double *post_dev, double *ym_dev,
                             double *Yp_dev, int obs_block_out, const double *ob_value, const double *ob_error,
                             const uint8_t *ob_assim, const double *ob_lat, const double *ob_lon, const double *ob_halfwidth_km,
                             const double *grid_lat, const double *grid_lon, long ncol, long n_lead, double *prior_mean,
                             double *prior_var, double *post_mean, double *post_var, uint8_t *assimilated,
                             double *col_stats_dev /* [ngroups][ncol][3] or NULL */);
int efa_letkf_slab_cycle_f32_dev(efa_ctx *ctx, long rows, int M, long P, const float *X_dev, float *post_dev, double *ym_dev,
                                 double *Yp_dev, int obs_block_out, const double *ob_value, const double *ob_error,
                                 const uint8_t *ob_assim, const double *ob_lat, const double *ob_lon, const double *ob_halfwidth_km,
                                 const double *grid_lat, const double *grid_lon, long ncol, long n_lead, double *prior_mean,
                                 double *prior_var, double *post_mean, double *post_var, uint8_t *assimilated,
                                 double *col_stats_dev /* [ngroups][ncol][3] or NULL */);
int efa_letkf_slab_cycle_interp_dev(efa_ctx *ctx, long rows, int M, long P, const double *X_dev, double *post_dev, double *ym_dev,
                                    double *Yp_dev, int obs_block_out, const double *ob_value, const double *ob_error,
                                    const uint8_t *ob_assim, const double *ob_lat, const double *ob_lon,
                                    const double *ob_halfwidth_km, const double *grid_lat, const double *grid_lon, long ny, long nx,
                                    long stride_y, long stride_x, long n_lead, double *prior_mean, double *prior_var,
                                    double *post_mean, double *post_var, uint8_t *assimilated,
                                    double *node_stats_dev /* [ngroups][nnodes][3] or NULL */);
int efa_letkf_slab_cycle_interp_f32_dev(efa_ctx *ctx, long rows, int M, long P, const float *X_dev, float *post_dev, double *ym_dev,
                                        double *Yp_dev, int obs_block_out, const double *ob_value, const double *ob_error,
                                        const uint8_t *ob_assim, const double *ob_lat, const double *ob_lon,
                                        const double *ob_halfwidth_km, const double *grid_lat, const double *grid_lon, long ny,
                                        long nx, long stride_y, long stride_x, long n_lead, double *prior_mean, double *prior_var,
                                        double *post_mean, double *post_var, uint8_t *assimilated,
                                        double *node_stats_dev /* [ngroups][nnodes][3] or NULL */);
int efa_letkf_slab_weights_dev(efa_ctx *ctx, int M, long P, const double *ym_dev, const double *Yp_dev, const double *ob_value,
                               const double *ob_error, const uint8_t *ob_assim, const double *ob_lat, const double *ob_lon,
                               const double *ob_halfwidth_km, long npts, const double *pt_lat, const double *pt_lon,
                               double *Tw_dev /* [ngroups][npts][M][M+1] */, double *stats_dev /* [ngroups][npts][3] or NULL */);
int efa_letkf_slab_groups(efa_ctx *ctx, long n_lead, int *group_of /* [n_lead] or NULL */, int *ngroups);

/* ---- LETKF: per-point multiplicative inflation, adaptive after Miyoshi
 * (2011, MWR 139) -------------------------------------------
 * Context state like the relaxation, read by every LETKF entry above
 * (cycle, f32, interp, slab and their combinations, efa_letkf_weights_dev,
 * efa_letkf_slab_weights_dev) and ignored by every other entry.  A solve
 * point x (a column, a node of the mesh, a probe point; with slab groups a
 * (group, point) pair, laid out [ngroups][points] as the statistics are) has a
 * prior factor lambda_b(x) = field_dev[x] > 0 that enters its solve as Hunt's
 * rho.  With w_k = rho_k(x)/r_k over the listed obs with rho_k(x) != 0, the
 * taper exactly as the solve uses it (slab factor included):
 *   A_x = ((M-1)/lambda_b) I + C_x,  T and w from its eigenpairs as above,
 *   dfs = sum_i (mu_i - (M-1)/lambda_b) / mu_i,
 *   p1 = sum_k w_k d_k^2,  p2 = trace(C_x)/(M-1),  p3 = sum_k rho_k,
 *   lambda_o = (p1 - p3)/p2,  v_o = (2/p3) ((lambda_b p2 + p3)/p2)^2,  v_b = sigma_b^2,
 *   lambda_a = clip(lambda_b + v_b/(v_o + v_b) (lambda_o - lambda_b), lower, upper).
 * The solve of this call uses lambda_b; lambda_a is written over field_dev[x]
 * for the next call.  sigma_b == 0: the field is fixed and keeps its bits.  A
 * point no ob reaches keeps its rows and its factor bit for bit (its pair stays
 * (I, 0)); so does the factor where p2 or p3 is not finite and positive or the
 * estimate is not finite (a NaN innovation reaching the point).
 * infl_stats_dev, [nsolve][4] or NULL, takes {p1, p2, p3, lambda_o} as
 * computed, NaN included ({0, 0, 0, NaN} for a point no ob reaches).  With a
 * mesh the nodes are the solve points; k_letkf_interp interpolates pairs that
 * carry the inflation.  The obs block: ob j is solved under ob_infl_dev[j]
 * ([P], NULL: 1.0 for all), which is never updated.  A field of 1.0
 * everywhere gives the bits of the call without the setting.
 * nsolve must equal ngroups * (columns, nodes or probe points) of the call and
 * P the call's; before any launch the call downloads the field (and
 * ob_infl_dev) and refuses values that are not finite or outside
 * [lower, upper].  The setter refuses sigma_b < 0 or not finite and anything
 * but 0 < lower <= upper, finite.  Every refusal is EFA_ERR_INVALID, writes
 * nothing and leaves the context usable.  field_dev == NULL turns it off. */
int efa_ctx_set_letkf_inflation(efa_ctx *ctx, double *field_dev, long nsolve, const double *ob_infl_dev, long P, double sigma_b,
                                double lower, double upper, double *infl_stats_dev);

/* ---- LETKF: the deterministic control analysis (Schraff et al. 2016, QJRMS
 * 142; the control member of Hunt et al. 2007, section 4) ----
 * Context state like the inflation.  A single forecast x_c carried beside the
 * ensemble is adjusted by the same observations through the ensemble's
 * covariances:
 *   x_c^a = x_c + X' [ (M-1)/lambda I + Y^T (rho o R^-1) Y ]^-1 Y^T (rho o R^-1) (y - H(x_c)).
 * xc_dev [rows] is the control, one float64 value per state row in the state's
 * row order lead*ncol + col (float64 also beside float32 member rows); yc_dev
 * [P] its observation estimates H(x_c).  At every solve point x (a column, a
 * (slab group, column), an ob position), over the listed obs with an effective
 * flag a_k = 1 and rho_k(x) != 0, with V, mu, rho_k, r_k those of the
 * ensemble's solve at that point (slab factor and inflation shift included):
 *   d^c_k = value_k - yc[k],  g^c = sum_k (rho_k/r_k) d^c_k Yp_k^T,  w^c = V diag(1/mu) V^T g^c,
 *   xc_post[row] = xc[row] + X'[row,:] . w^c      for every row the point maps,
 *   yc_post[j]   = yc[j] + Yp_j . w^c(ob j's position)   for all P obs,
 * X' the row's PRIOR perturbations in float64.  The effective flag is decided
 * on the ENSEMBLE mean's innovation: the control never votes in the outlier
 * check, and value, error and yc of an ob with a_k = 0 are never read.
 * The ensemble is untouched: with the control set every ensemble output
 * (posterior members, obs block, diagnostics, col_stats, the inflation field
 * and its statistics) has the bits it has without it, whatever xc and yc hold.
 * Relaxation (RTPS, RTPP) acts on perturbations and does not reach the control.
 * A point no ob reaches copies its control rows bit for bit (leaves them alone
 * when xc_post_dev == xc_dev), and yc_post[j] = yc[j] bit for bit for an ob
 * position no ob reaches.  A NaN yc[k] of an assimilated ob makes NaN the
 * control rows of exactly the columns with rho_k != 0.  Same inputs, same bits:
 * a row's control value is read and written by the wave that owns the row.
 * Served by efa_letkf_cycle_dev / _f32_dev and efa_letkf_slab_cycle_dev /
 * _f32_dev; these refuse, with EFA_ERR_INVALID before any launch, rows or P
 * that differ from the call's.  While the setting is on the four interp cycles,
 * efa_letkf_weights_dev and efa_letkf_slab_weights_dev are refused likewise:
 * their [M][M+1] pair layout has no place for w^c.  efa_letkf_interp_apply_dev
 * / _f32_dev take no obs and IGNORE the setting; so do the EnSRF and ETKF
 * entries.  The setter refuses (the setting stays as it was) negative counts,
 * null or misaligned arrays, xc_post_dev overlapping xc_dev without coinciding
 * with it, and yc_post_dev overlapping yc_dev; the control's arrays must be
 * clear of every other array of the call.  xc_dev == NULL turns it off. */
int efa_ctx_set_letkf_control(efa_ctx *ctx, const double *xc_dev, double *xc_post_dev, long rows, const double *yc_dev,
                              double *yc_post_dev, long P);

/* ---- LETKF: a cap on the local observations of a solve, by taper rank and
 * class (Miyoshi's nobsl, SCALE-LETKF's MAX_NOBS_PER_GRID, JEDI's max nobs)
 *  ----
 * Context state like the control.  ob_class [P] (host) gives every ob a class
 * in 0..nclass-1 (NULL: all of class 0), cap [nclass] (host) the most obs of
 * that class one local analysis may use, 0 meaning no limit.  At a solve point
 * x (a grid column, a mesh node, an ob position, a probe point), of the obs of
 * class c with an effective flag a_k = 1 and rho_k(x) != 0: if there are more
 * than cap[c], exactly the cap[c] with the LARGEST rho_k(x) keep their taper
 * and the others get rho_k(x) = 0; equal tapers (the same bits) are ordered by
 * lower ob index first.  Everything downstream is the LETKF's definition on
 * the tapers that remain: n_local (= sum_c min(cap[c], reach_c) exactly), dfs,
 * the inflation's p1..p3, the node pairs of a weight stride.  An ob with
 * a_k = 0 (not requested, or rejected by the outlier check) takes no place.
 * The obs block is capped at every ob's own position; with a mesh the nodes
 * are capped.  A point at which no class is over its cap is not touched: caps
 * >= P give the call without the setting bit for bit.  The NaN value of an ob
 * that loses at a point does not reach that point.  Same inputs, same bits.
 * reach_dev [nsolve] (device, or NULL) receives, for the STATE's solve points
 * (columns, nodes, probe points) only, the count of non-zero tapers before the
 * cap, as a double; nsolve is read with reach_dev only.
 * Served by efa_letkf_cycle_dev / _f32_dev, efa_letkf_cycle_interp_dev /
 * _f32_dev and efa_letkf_weights_dev; these refuse, with EFA_ERR_INVALID before
 * any launch, a P (and with reach_dev an nsolve) that differs from the call's.
 * While the setting is on the four slab cycles and efa_letkf_slab_weights_dev
 * are refused likewise: their taper is a product per (slab group, column), the
 * lists' tapers are per column, and a cap per group is a follow-up.
 * efa_letkf_interp_apply_dev / _f32_dev, the EnSRF, ETKF and impact entries
 * IGNORE it.  The setter refuses (the setting stays as it was) nclass outside
 * 1..32, a negative cap, a class outside 0..nclass-1, negative counts and a
 * misaligned reach_dev.  cap == NULL turns it off.  The cap's launch counts
 * towards obs_ms of efa_last_timing. */
int efa_ctx_set_letkf_obs_cap(efa_ctx *ctx, const int *ob_class /* host [P], NULL: all class 0 */, long P,
                              const long *cap /* host [nclass], NULL: off */, int nclass, double *reach_dev /* [nsolve] or NULL */,
                              long nsolve);

/* ---- LETKF: cross-validated perturbation update over member groups -----
 * (Buehner 2020, Mon. Wea. Rev. 148, 2265-2282)  Context
 * state in the style of the cap above.  Member m carries the label
 * group_of_member[m] in 0..ngroups-1.  At every solve point (a column, a node
 * of a mesh, an ob's own position, a probe point), on exactly the tapers and
 * flags of the plain solve, with C = sum_k (rho_k/r_k) Yp_k^T Yp_k:
 *   mean      w = ((M-1) I + C)^-1 g: the full-ensemble solve, unchanged, as
 *             are n_local, dfs and sweeps of the statistics;
 *   group k   I = the members with another label (ascending), H = those with
 *             label k, m = |I|, a = m - 1, J = I_m - 1 1^T / m,
 *             a I + J C[I,I] J = V diag(mu) V^T (the same Jacobi),
 *             G = V diag(1 / (mu (1 + sqrt(a / mu)))) V^T,
 *             T[I,H] = -J G J C[I,H], T[H,H] = identity;
 *   recentre  T <- T - (T 1 / M) 1^T;
 *   apply     mean += X' w, X' <- X' T, so that a held-out member's
 *             perturbation is updated with the gain of the other groups alone
 *             and the posterior perturbations sum to zero.
 * T is not symmetric.  The state is always applied by the interpolate-and-
 * apply launch, without a mesh on a unit mesh whose nodes are the columns: two
 * state launches, a node-pair buffer of nsolve M (M+1) doubles and a scratch
 * of nsolve M M doubles (P of each for the obs block), held by the context.
 * cv_stats_dev [nsolve][2] (device, or NULL) receives for the STATE's solve
 * points the sum of the ngroups sub-solves' sweeps and their largest
 * max mu / min mu ((0, 0) where no ob reaches the point); nsolve is read with
 * cv_stats_dev only.
 * Served by efa_letkf_cycle_dev / _f32_dev, efa_letkf_cycle_interp_dev /
 * _f32_dev and efa_letkf_weights_dev (whose T is then the recentred one); these
 * refuse, with EFA_ERR_INVALID before any launch, an M (and with cv_stats_dev
 * an nsolve) that differs from the call's.  While the setting is on, the slab
 * entries, any call with a LETKF inflation field set and any call with a
 * control set are refused likewise.  efa_letkf_interp_apply_dev / _f32_dev,
 * the EnSRF, ETKF and impact entries IGNORE it.  The setter refuses (the
 * setting stays as it was) M outside 4..136, ngroups < 2, a label outside
 * 0..ngroups-1, an unused label, a group that leaves fewer than 2 members
 * outside it, a negative nsolve and a misaligned cv_stats_dev.
 * group_of_member == NULL turns it off. */
int efa_ctx_set_letkf_cross_validation(efa_ctx *ctx, const int *group_of_member /* host [M], NULL: off */, int M, int ngroups,
                                       double *cv_stats_dev /* [nsolve][2] or NULL */, long nsolve);

/* ---- device memory for callers without their own allocator -------------*/
int efa_malloc(efa_ctx *ctx, size_t bytes, void **dev_out);
int efa_free(efa_ctx *ctx, void *dev);
int efa_memcpy_h2d(efa_ctx *ctx, void *dst_dev, const void *src, size_t bytes);
int efa_memcpy_d2h(efa_ctx *ctx, void *dst, const void *src_dev, size_t bytes);
int efa_memcpy_d2d(efa_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);

/* ---- a3: mean-removed perturbation matrix --------------------------------
 * Replaces `xbm = prior.mean(axis=1); Xbp = prior - xbm[:,None]`
 * (assimilation.py:146-147) for `rows` rows of M members.  Also used for the
 * obs-space priors of compute_ob_priors (assimilation.py:46-48).
 * `scale` multiplies the perturbations (constant inflation,
 * assimilation.py:62-68); pass 1.0 for none.  X_dev may equal Xp_dev. */
int efa_form_perts_dev(efa_ctx *ctx, long rows, int M, const double *X_dev,
                       double scale, double *xm_dev, double *Xp_dev);

/* ---- a15: posterior member values ----------------------------------------
 * Replaces `post = (xam[:,None] + Xap)[:Nstate]` (assimilation.py:168).
 * post_dev may equal Xp_dev. */
int efa_posterior_dev(efa_ctx *ctx, long rows, int M, const double *xm_dev,
                      const double *Xp_dev, double *post_dev);

/* ---- f1 (linear part): forward operator as a sparse row stencil ---------
 * HX[k,:] = sum_j wts[k*npt+j] * X[idx[k*npt+j] - row_offset, :] over the
 * stencil points owned by this shard (row_offset <= idx < row_offset+rows);
 * points owned elsewhere contribute 0 so that a sum all-reduce across shards
 * gives the full estimate (the payload of the multi-GPU exchange).
 * Stands in for Observation.estimate -> EnsembleState.interpolate
 * (observation.py:40-50, ensemble.py:170-239) once the stencil is known.
 * idx/wts are host arrays of length P*npt. */
int efa_forward_stencil_dev(efa_ctx *ctx, long rows, long row_offset, int M,
                            const double *X_dev, long P, int npt,
                            const int64_t *idx, const double *wts,
                            double *HX_dev);

/* ---- f1 (search + weights): the reference's default forward operator on the device ------
 * Observation.estimate -> EnsembleState.interpolate (observation.py:40-50,
 * ensemble.py:170-239) for P point observations at once, as a linear stencil of up
 * to 8 (state row, weight) entries per ob:
 *   space: the 4 grid points nearest in the reference's sin/cos pseudo-distance
 *          (ensemble.py:152-168; one workgroup scans the grid per ob instead of a
 *          full argsort; ties go to the lower flat index), weights = inverse
 *          great-circle distance, normalised; if a point lies within 1 km the
 *          nearest takes weight 1 (ensemble.py:178-200 -- the reference's own
 *          exact-match branch raises IndexError as written);
 *   time:  linear between the two valid times that bracket the ob, with the
 *          weights AS CODED in ensemble.py:201-224.
 * Inputs (host arrays): grid_lat/grid_lon [n_grid] degrees, n_grid = ny*nx for
 *   2-D lat/lon (latlon_1d = 0) or the length of a 1-D coordinate (latlon_1d = 1:
 *   the reference then uses one index for y and x, ensemble.py:186-190);
 *   valid_times [nt] ascending on any numeric axis; per ob: ob_var (index of
 *   Observation.obtype in EnsembleState.vars()), ob_time (same axis), ob_lat, ob_lon.
 * Outputs: the stencil stays in the context for efa_forward_interp_dev; optional
 *   host copies sten_idx [P*8] (global state rows in to_vect() order, -1 unused),
 *   sten_wts [P*8], ob_status [P]: 0 ok, 1 time outside the state's range (the
 *   reference prints a message and returns None), 2 grid index out of range (1-D
 *   lat/lon), 3 bad variable index.  Entries 0-3: the earlier valid time, 4-7: the
 *   later one (or the exact match).  Pinned to the reference by fixtures
 *   tests/golden/G9 (2-D lat/lon), G10 (1-D lat/lon) and G11 (EnSRF.update() end to
 *   end): its nearest_points / interpolate / estimate run verbatim in the build
 *   container on a duck-typed state (tests/golden/make_goldens.py). */
int efa_interp_stencils(efa_ctx *ctx, int nvar, int nt, int ny, int nx,
                        int latlon_1d, long n_grid, const double *grid_lat,
                        const double *grid_lon, const double *valid_times, long P,
                        const int32_t *ob_var, const double *ob_time,
                        const double *ob_lat, const double *ob_lon,
                        int64_t *sten_idx, double *sten_wts, uint8_t *ob_status);
/* HX[k,:] = sum of the context's stencil over the entries whose (y,x) column lies in
 * this shard's [col_lo, col_hi) of the ncol = ny*nx global columns; the shard holds
 * row lead*(col_hi-col_lo) + (col-col_lo) for lead in [0,n_lead).  A sum all-reduce
 * over the shards gives the full estimate (compute_ob_priors, assimilation.py:45-46). */
int efa_forward_interp_dev(efa_ctx *ctx, long ncol, long col_lo, long col_hi,
                           long n_lead, int M, const double *X_dev, double *HX_dev);

/* ---- a5-a14: the serial EnSRF loop, data resident in HBM -----------------
 * Replaces ensrf.py:50-149 for all P observations.
 *
 * State block (this GPU's shard):  xm_dev[rows], Xp_dev[rows*M], in/out.
 *   Row i of the shard is state element (lead, col) with
 *   i = lead*ncol + col, lead in [0,n_lead), col in [0,ncol): n_lead =
 *   nvar*ntimes, ncol = the shard's (y,x) columns -- the order of to_vect().
 *   With EFA_LOC_NONE pass n_lead=1, ncol=rows.
 * Obs block (replicated on every shard): ym_dev[P], Yp_dev[P*M], in/out:
 *   the obs-space prior means/perturbations that the reference appends to
 *   the state (assimilation.py:149-150); on return they hold the reference's
 *   final values of those augmented rows.
 * Per observation k (host arrays, length P):
 *   ob_value, ob_error (error VARIANCE, ensrf.py:79,91), ob_assim (0/1:
 *   Observation.assimilate_this, ensrf.py:74), and for EFA_LOC_GC ob_lat,
 *   ob_lon (degrees) and ob_halfwidth_km (Observation.localize_radius).
 *   ob_value and ob_error of an ob with ob_assim 0 are not read (the
 *   reference skips it before it reads either, ensrf.py:74-76): they may
 *   hold anything, NaN and Inf included, and change no bit of any output.
 *   The same holds in every entry point that takes these three arrays, and
 *   for an ob the outlier check rejects.
 * Grid (host arrays, length ncol, degrees; EFA_LOC_GC only): lat/lon of each
 *   local column (ensemble.py:254-267 distance_to_point).
 * Diagnostics (host arrays, length P; written for every ob as the reference
 *   does, ensrf.py:66,70,75,146-149): prior_mean, prior_var for all obs;
 *   post_mean, post_var only where assimilated[k]==1 (left untouched
 *   otherwise).
 */
int efa_ensrf_update_dev(efa_ctx *ctx, long rows, int M, long P,
                         double *xm_dev, double *Xp_dev,
                         double *ym_dev, double *Yp_dev,
                         const double *ob_value, const double *ob_error,
                         const uint8_t *ob_assim, int loc_mode,
                         const double *ob_lat, const double *ob_lon,
                         const double *ob_halfwidth_km,
                         const double *grid_lat, const double *grid_lon,
                         long ncol, long n_lead,
                         double *prior_mean, double *prior_var,
                         double *post_mean, double *post_var,
                         uint8_t *assimilated);

/* The two phases of efa_ensrf_update_dev, separately callable.
 * Phase A (obs space, serial in k, identical on every shard): consumes the
 * obs block, records the trajectory the state sweep needs and returns the
 * diagnostics.  Phase B (state space): applies the recorded trajectory to
 * `rows` state rows; independent per row, so shards never communicate.
 * efa_obs_phase_dev must precede efa_state_phase_dev on the same context. */
int efa_obs_phase_dev(efa_ctx *ctx, int M, long P, double *ym_dev,
                      double *Yp_dev, const double *ob_value,
                      const double *ob_error, const uint8_t *ob_assim,
                      int loc_mode, const double *ob_lat, const double *ob_lon,
                      const double *ob_halfwidth_km, double *prior_mean,
                      double *prior_var, double *post_mean, double *post_var,
                      uint8_t *assimilated);
/* out-of-place allowed: (xm_in, Xp_in) -> (xm_out, Xp_out); pass the same
 * pointers for in-place.  An output range that overlaps its input range
 * without coinciding with it is refused with EFA_ERR_INVALID (here, in
 * efa_state_cycle_dev and in efa_state_cycle_f32_dev). */
int efa_state_phase_dev(efa_ctx *ctx, long rows, int M, const double *xm_in_dev,
                        const double *Xp_in_dev, double *xm_out_dev,
                        double *Xp_out_dev, const double *grid_lat,
                        const double *grid_lon, long ncol, long n_lead);

/* ---- a3+a5-a15 fused for resident full-member states ---------------------
 * prior members X_dev[rows*M] -> posterior members post_dev[rows*M] using the
 * trajectory recorded by efa_obs_phase_dev.  Equivalent to
 * efa_form_perts_dev + efa_state_phase_dev + efa_posterior_dev with one read
 * and one write of the state when the transform path applies.
 * post_dev may equal X_dev (the transform above 136 members then reads a copy
 * of the prior, rows*M*8 bytes of device memory more: its column groups
 * re-read whole rows); any other overlap of the two ranges is EFA_ERR_INVALID.
 * Under EFA_LOC_GC with option "gc_onepass" 1 and no relaxation a row that no assimilated ob
 * reaches (every taper weight 0) comes back bit for bit as it went in, as its xm
 * and Xp rows do from efa_state_phase_dev. */
int efa_state_cycle_dev(efa_ctx *ctx, long rows, int M, const double *X_dev,
                        double *post_dev, const double *grid_lat,
                        const double *grid_lon, long ncol, long n_lead);

/* ---- the state stored as float32, every number still computed in float64 ----
 * efa_state_cycle_dev on float32 member rows X[row*M + mem]: for a float32 prior
 * X32 the posterior is fl32(F(widen(X32))) -- widen the exact float32 -> float64
 * conversion, F the float64 state phase of efa_state_cycle_dev (the same kernels'
 * arithmetic in the same order) and fl32 ONE round-to-nearest-even at the final
 * store -- on every path and with every option.  Like efa_state_cycle_dev it
 * follows efa_obs_phase_dev; the obs block, the trajectory and the diagnostics
 * are float64 as ever.  post_dev may equal X_dev; both need 4-byte alignment
 * only (rows whose base is 8-byte aligned, M even, are loaded two members at a
 * time).  Relaxation, vertical localisation and the options "path" and
 * "gc_onepass" apply as they do to efa_state_cycle_dev; while an adaptive-
 * inflation field is set the call fails with EFA_ERR_INVALID (that update is
 * float64 only).
 * The transform (up to 256 members; RTPP folded in, RTPS fused in up to 136
 * members) and the one-pass GC sweep for an even number of up to 104 members
 * without relaxation read and write the float32 rows themselves.  Every other
 * route -- the per-batch sweeps, "gc_onepass" 0, the one-pass sweep for odd or
 * more than 104 members, a relaxation that is not folded or fused, a cycle
 * without an assimilated ob -- widens the rows into a float64 workspace of the
 * context, runs the float64 kernels there and rounds the posterior members once
 * on the way out: rows*M*8 bytes more device memory (twice that for the
 * transform above 136 members, whose column groups cannot run in place; the
 * float32 transform above 136 members with post_dev == X_dev keeps a copy of the
 * prior instead, rows*M*4 bytes, as the float64 one does at 8 bytes a value).  Read-only option "f32_native" says which it
 * was for the last float32 state call: 1 on the float32 rows, 0 through the
 * workspace. */
int efa_state_cycle_f32_dev(efa_ctx *ctx, long rows, int M, const float *X_dev,
                            float *post_dev, const double *grid_lat,
                            const double *grid_lon, long ncol, long n_lead);

/* ---- one whole cycle on resident prior members, ONE call ------------------
 * efa_obs_phase_dev followed by efa_state_cycle_dev (ensrf.py:50-149 on the obs
 * block, then on every state row; same arguments, same results bit for bit),
 * with one difference in how the device is driven: when the cycle is
 * unlocalised, takes the transform path, fits one persistent Phase-A launch and
 * X_dev / post_dev do not overlap, the state transform is put into the stream
 * BEHIND the Phase-A launch before the host has seen that launch's status, so
 * the device goes from Phase A to Phase B without a host round trip.  A launch
 * that then reports a fallback (bounded spin expired, cancellation guard) is
 * redone by the other Phase-A kernels and the transform enqueued again: a
 * wrong guess costs one wasted pass, never a result (the prior is only read).
 * obs_block_out 0 leaves ym_dev / Yp_dev as they came (the reference discards
 * the augmented obs rows: format_posterior_state keeps [:N], assimilation.py:168);
 * 1 returns the final obs block in them like efa_obs_phase_dev. */
int efa_ensrf_cycle_dev(efa_ctx *ctx, long rows, int M, long P,
                        const double *X_dev, double *post_dev, double *ym_dev,
                        double *Yp_dev, int obs_block_out,
                        const double *ob_value, const double *ob_error,
                        const uint8_t *ob_assim, int loc_mode,
                        const double *ob_lat, const double *ob_lon,
                        const double *ob_halfwidth_km, const double *grid_lat,
                        const double *grid_lon, long ncol, long n_lead,
                        double *prior_mean, double *prior_var,
                        double *post_mean, double *post_var,
                        uint8_t *assimilated);

/* ---- host-memory convenience: the augmented arrays of the reference ------
 * xbm[A], Xbp[A*M] (A = N + P) exactly as format_prior_state returns them
 * (assimilation.py:154), updated in place to the (xam, Xap) handed to
 * format_posterior_state (ensrf.py:151).  Copies to the GPU, runs
 * efa_ensrf_update_dev, copies back.  grid_lat/grid_lon have ncol entries,
 * N = n_lead*ncol. */
int efa_ensrf_update(efa_ctx *ctx, long A, long N, int M, long P, double *xbm,
                     double *Xbp, const double *ob_value,
                     const double *ob_error, const uint8_t *ob_assim,
                     int loc_mode, const double *ob_lat, const double *ob_lon,
                     const double *ob_halfwidth_km, const double *grid_lat,
                     const double *grid_lon, long ncol, long n_lead,
                     double *prior_mean, double *prior_var, double *post_mean,
                     double *post_var, uint8_t *assimilated);

/* ---- one whole cycle on a prior in HOST memory, streamed in column chunks ----
 * The state never has to fit the device: it crosses it in chunks of (y,x)
 * columns, upload of chunk i+1, state phase of chunk i and download of chunk
 * i-1 overlapping on two copy streams beside the context's stream.  Phase A
 * starts as soon as the obs block is on the device, while the first chunks
 * upload.  Device memory for the state is a ring of three chunk buffers.
 *
 * State: n_seg segments (one per variable); segment v is a C-contiguous
 *   [seg_slabs[v]][ncol][M] float64 array at seg_prior[v], read only, and its
 *   posterior goes to seg_post[v] (same shape; must not overlap the prior).
 *   n_lead = sum of seg_slabs; state row (lead, col) is lead*ncol + col, the
 *   order of to_vect().  ncol is the number of (y,x) columns, with and without
 *   localisation.
 * HX[P*M]: the member estimates of the P observations (host), row k =
 *   ob_k.estimate(prior); means and perturbations are formed on the device
 *   (assimilation.py:46-48).  Not written.
 * chunk_cols (>= 1): columns per chunk, rounded down to a multiple of 16 (the
 *   one-pass sweep's block; at least 16); the last chunk takes the ragged
 *   rest.  Chunk [lo, hi) is on the device as the column shard
 *   row = lead*(hi-lo) + (col-lo).
 * Per-ob arrays, grid (ncol entries, EFA_LOC_GC only) and diagnostics exactly
 *   as efa_ensrf_cycle_dev has them.
 * Relaxation, outlier threshold and vertical localisation are context state
 * and apply per chunk as they do to a resident state; while an adaptive-
 * inflation field is set the call fails with EFA_ERR_INVALID.  Results equal
 * efa_ensrf_cycle_dev on the resident state bit for bit.
 *
 * A segment that lies inside a block of efa_pinned_alloc (looked up in the
 * context's registry; caller memory is never registered) is transferred
 * directly by DMA, strided pieces as 2-D copies; any other pointer is staged
 * through a bounded ring of pinned chunk images by the call itself.
 * The call returns with everything done: the posterior and the diagnostics
 * are in host memory.  With efa_ctx_set_stream the work is ordered behind
 * what the context issued on the caller's stream before, like a change of
 * stream.  The one-pass GC sweep's active lists are rebuilt per chunk (the
 * 8-byte capacity read-back is the only host wait between chunks besides the
 * staging ring's).
 * efa_last_timing keeps its meaning (state_ms: the sum over the chunks).
 * Read-only options about the last call: "stream_chunks",
 * "stream_peak_bytes" (device bytes held for state chunks), "stream_h2d_us",
 * "stream_d2h_us" (sums of the chunks' copy times on the device),
 * "stream_wall_us" (host wall time of the call). */
int efa_ensrf_cycle_host(efa_ctx *ctx, int n_seg, const double *const *seg_prior,
                         double *const *seg_post, const long *seg_slabs, long ncol,
                         int M, long P, const double *HX, long chunk_cols,
                         const double *ob_value, const double *ob_error,
                         const uint8_t *ob_assim, int loc_mode,
                         const double *ob_lat, const double *ob_lon,
                         const double *ob_halfwidth_km, const double *grid_lat,
                         const double *grid_lon, double *prior_mean,
                         double *prior_var, double *post_mean, double *post_var,
                         uint8_t *assimilated);
/* efa_ensrf_cycle_host on a state stored as float32: the segments are
 * [seg_slabs[v]][ncol][M] float32 arrays, every chunk runs
 * efa_state_cycle_f32_dev (above: posterior = fl32(F(widen(prior)))), and the
 * ring, the staging images and the copies move 4-byte elements -- half the
 * bytes over the link and "stream_peak_bytes" three chunks of rows*M*4.  HX,
 * the per-ob arrays, the grid and the diagnostics are float64 as above, and
 * bit for bit those of efa_ensrf_cycle_host on the widened prior.  Equal to
 * efa_state_cycle_f32_dev on the resident float32 state bit for bit. */
int efa_ensrf_cycle_host_f32(efa_ctx *ctx, int n_seg, const float *const *seg_prior,
                             float *const *seg_post, const long *seg_slabs, long ncol,
                             int M, long P, const double *HX, long chunk_cols,
                             const double *ob_value, const double *ob_error,
                             const uint8_t *ob_assim, int loc_mode,
                             const double *ob_lat, const double *ob_lon,
                             const double *ob_halfwidth_km, const double *grid_lat,
                             const double *grid_lon, double *prior_mean,
                             double *prior_var, double *post_mean, double *post_var,
                             uint8_t *assimilated);
/* Page-locked host memory owned by the context (hipHostMalloc), for states
 * that efa_ensrf_cycle_host moves by DMA without staging.  Blocks still
 * allocated when the context is destroyed are freed with it. */
int efa_pinned_alloc(efa_ctx *ctx, size_t bytes, void **host_out);
int efa_pinned_free(efa_ctx *ctx, void *host);

/* ---- configs[4]: batched-obs dense contraction, float32 --------------------
 * C[i*P + k] = sum_m Xbp[i*M + m] * Ye[k*M + m]: the covariance numerators
 * `np.dot(Xbp, ye.T)` of ensrf.py:95 for P recorded obs-space rows at once, as
 * one (state x member).(member x obs) contraction on the matrix cores
 * (v_mfma_f32_32x32x2_f32: exact f32 FMA chains).  All pointers are device
 * memory; M must be a multiple of 4; divide by (M-1) for covariances. */
int efa_cov_contract_f32_dev(efa_ctx *ctx, long N, int M, long P,
                             const float *Xbp_f32_dev, const float *Ye_f32_dev,
                             float *C_f32_dev);

/* ---- observation impact (EFSO; Kalnay et al. 2012, Ota et al. 2013) ----
 * How much each assimilated observation changed a forecast error norm, once a
 * verifying state exists.  For every ob k with ob_used[k] != 0
 *   impact[k] = (1/(M-1)) (innov[k] / ob_error[k])
 *               * sum_i rho_ik werr[i] (Xf'_i . Ya'_k)
 * and impact[k] = 0.0 for every other ob.  Negative: the ob reduced the error.
 *   Xf_dev   [rows][M] forecast members (Xf' their deviations from the row mean)
 *   werr_dev [rows]    the weighted error sum c_i (e^a_i + e^b_i) of every row;
 *                      0 for a row that is not verified
 *   Ya_dev   [P][M]    analysis members in observation space (Ya' their deviations)
 *   innov, ob_error, ob_used [P] (host): innovation against the background
 *                      mean, error variance, and whether the ob was assimilated
 *   rho_ik: 1 with EFA_LOC_NONE (pass n_lead = 1, ncol = rows).  With
 *     EFA_LOC_GC the taper the assimilation itself uses for state row
 *     i = lead*ncol + col and ob k: Gaspari-Cohn of the column's distance to the
 *     ob with ob_halfwidth_km[k], times -- while vertical localisation is set
 *     on the context -- the vertical factor of (slab lead, ob k) by the rules of
 *     efa_ctx_set_vertical_localization.  The taper is not advected.
 * Xf_dev, werr_dev and Ya_dev are read only.  The call needs no preceding obs
 * phase and leaves everything a later cycle reads -- cached active lists and
 * taper tables, the trajectory, options, the sums of efa_last_timing -- as it
 * found it: a cycle after it returns the bits it returns without it.  It
 * synchronises the stream before returning impact[P] (host).  The sums are
 * added in a fixed order without atomics: the same inputs give the same bits.
 * Relaxation, outlier threshold, adaptive-inflation field and "path" do not
 * apply and are ignored.
 * The rows may be a column shard (grid_lat/grid_lon its ncol columns): the
 * impact arrays of the shards add up to the whole state's, so one
 * efa_allreduce_sum_dev over a device copy of them finishes a sharded call.
 * EFA_ERR_INVALID: a NULL pointer, M < 2 or M > 256, rows != n_lead*ncol, a
 * used ob whose innov is not finite or whose ob_error is not finite and > 0,
 * a used ob with a NaN half-width under EFA_LOC_GC, or vertical localisation
 * set while the call is not an EFA_LOC_GC call of exactly its P and n_lead.
 * Read-only option "impact_us": device time (microseconds, HIP events) of the
 * last call's contraction and reduction kernels; the build of the call's
 * active lists and the copies around them are not in it. */
int efa_obs_impact_dev(efa_ctx *ctx, long rows, int M, long P,
                       const double *Xf_dev, const double *werr_dev,
                       const double *Ya_dev, const double *innov,
                       const double *ob_error, const uint8_t *ob_used,
                       int loc_mode, const double *ob_lat, const double *ob_lon,
                       const double *ob_halfwidth_km, const double *grid_lat,
                       const double *grid_lon, long ncol, long n_lead,
                       double *impact);

/* ---- observation impact under the temporal and variable tapers ----
 * efa_obs_impact_dev for a context on which efa_ctx_set_slab_localization is
 * set: the same parameters, the same formula, and
 *   rho_ik = GC(column, ob k; ob_halfwidth_km[k]) * S(k, slab)
 * for state row i = lead*ncol + col, S = (V T) C the slab factor of
 * efa_slab_factor_table: the vertical factor (1 unless vertical localisation
 * is set too), the temporal taper and the impact of ob k's obtype on the
 * slab's variable -- the taper the one-pass sweep used for that row, each
 * product rounded once as it rounds it.  The table is brought up to date on
 * the context's stream ahead of the contraction.
 * While the slab setting is on, the call must be an EFA_LOC_GC call of exactly
 * the P and n_lead the setting was made for (and the vertical setting, if on,
 * for the same P and n_lead); anything else is EFA_ERR_INVALID with a message
 * that names slab localisation.  While it is off, the call is
 * efa_obs_impact_dev, bit for bit: it is handed on to that entry, so the
 * message of an argument error then names efa_obs_impact_dev.
 * Everything else is as efa_obs_impact_dev has it: no preceding obs phase, a
 * column shard's rows (the table does not depend on the columns, so the
 * shards' impacts still add up), "impact_us", the stream synchronised before
 * returning, exactly 0.0 for an ob that is not used and for a used ob whose
 * taper or factor is zero on every row, sums in a fixed order without atomics.
 * Of the context it writes the cached factor table alone (keyed by the two
 * settings): a cycle after it returns the bits it returns without it.
 * Sensitivity and targeting stay unlocalised. */
int efa_obs_impact_slab_dev(efa_ctx *ctx, long rows, int M, long P,
                            const double *Xf_dev, const double *werr_dev,
                            const double *Ya_dev, const double *innov,
                            const double *ob_error, const uint8_t *ob_used,
                            int loc_mode, const double *ob_lat,
                            const double *ob_lon, const double *ob_halfwidth_km,
                            const double *grid_lat, const double *grid_lon,
                            long ncol, long n_lead, double *impact);

/* ---- ensemble sensitivity and greedy observation targeting (Ancell & Hakim 2007, Torn & Hakim 2008) ----
 * Asked BEFORE observations are taken: which state rows drive K forecast
 * metrics, and where would the next observation reduce their variance most.
 *   X_dev [rows][M]  state members (float64; float32 for the _f32 twin, every
 *                    number computed in float64 as DESIGN.md 7g has it), row
 *                    i = lead*ncol + col, rows = n_lead*ncol (to_vect() order)
 *   J [K][M] (host)  the members' values of the K metrics
 *   slab_error [n_lead] (host) error VARIANCE R of a hypothetical observation
 *                    of a row of that slab, finite and > 0
 *   weights [K] (host, NULL: all 1) finite, >= 0
 *   cand_dev [rows] (NULL: every row) non-zero: the row may be picked
 * With x'_i, J'_k the deviations from the member means, every statistic with
 * 1/(M-1) (a product of its own: not ensrf.py's mixed convention):
 *   var_i = x'_i.x'_i/(M-1)   cov_ik = x'_i.J'_k/(M-1)   varJ_k = J'_k.J'_k/(M-1)
 * Picks t = 0 .. n_targets-1 are made one after the other, each conditioning
 * every statistic on the ones before by the exact, unlocalised Kalman update
 * of observing row i_t with error R_slab(i_t):
 *   score_i(t) = sum_k w_k cov_ik(t)^2 / (var_i(t) + R_slab(i)),
 * the expected reduction of sum_k w_k var(J_k); i_t is the candidate with the
 * largest score, the lowest row among equals, never a NaN; when no candidate
 * scores > 0 the picks stop (picked_row -1, picked_score 0.0, metric_var
 * repeats its last row).  A row may be picked twice.
 * Fields at the final pass (device, each may be NULL = not wanted and not
 * written; n_targets = 0: the classical ensemble-sensitivity fields):
 *   var [rows], cov [K][rows], sens = cov/var, corr = cov/sqrt(var varJ_k),
 *   dvar = -cov^2/(var + R) (each [K][rows]), score [rows] (0.0 for a row that
 *   is no candidate).  A zero denominator gives exactly 0.0; a row with a
 *   non-finite member gives NaN fields and is never picked; a constant row
 *   gives 0.0 everywhere.
 * Host outputs: picked_row [n_targets], picked_score [n_targets], metric_var
 * [n_targets+1][K] = varJ after 0 .. n_targets picks (required when
 * n_targets > 0; metric_var may be given alone with n_targets = 0).
 * One pass over the state per pick plus one for the fields (skipped when no
 * field is wanted); between passes the picked row's M members come to the host
 * for an M x M update.  The best row is found without atomics, in a fixed
 * order: the same inputs give the same bits and the same picks.  The call
 * uses workspaces of its own and leaves everything a later cycle reads as it
 * found it, like efa_obs_impact_dev; it synchronises before returning.
 * The rows may be a column shard: the fields of the shards are the fields of
 * the whole state (picks across shards are the caller's business).
 * EFA_ERR_INVALID, before any launch and with no output written: a NULL
 * required pointer, M < 2 or M > 256, K < 1, n_targets < 0, K + n_targets >
 * 32, rows != n_lead*ncol, a non-finite J, a slab_error that is not finite
 * and > 0, a weight that is not finite and >= 0, n_targets > 0 with a NULL
 * picked_row / picked_score / metric_var.
 * Read-only option "sens_us": device time (microseconds, HIP events) of the
 * last call's passes, summed. */
int efa_sensitivity_dev(efa_ctx *ctx, long rows, int M, int K, const double *X_dev,
                        const double *J, long ncol, long n_lead,
                        const double *slab_error, const double *weights,
                        const uint8_t *cand_dev, int n_targets, double *var_dev,
                        double *cov_dev, double *sens_dev, double *corr_dev,
                        double *dvar_dev, double *score_dev, long *picked_row,
                        double *picked_score, double *metric_var);
int efa_sensitivity_f32_dev(efa_ctx *ctx, long rows, int M, int K, const float *X_dev,
                            const double *J, long ncol, long n_lead,
                            const double *slab_error, const double *weights,
                            const uint8_t *cand_dev, int n_targets, double *var_dev,
                            double *cov_dev, double *sens_dev, double *corr_dev,
                            double *dvar_dev, double *score_dev, long *picked_row,
                            double *picked_score, double *metric_var);

/* ---- ensemble verification: rank histogram, CRPS, spread and skill per row (Hamill 2001, Hersbach 2000, Ferro 2014) ----
 * Asked once a verifying state exists: is the ensemble calibrated?
 *   X_dev [rows][M]   state members (float64; float32 for the _f32 twin, every
 *                     number computed in float64 as DESIGN.md 7g has it), row
 *                     i = lead*ncol + col, rows = n_lead*ncol (to_vect() order)
 *   verif_dev [rows]  the verifying value y_i of every row; not finite: the row
 *                     is not verified
 *   slab_group [n_lead] (host) the group g >= 0 whose statistics slab `lead`
 *                     adds to, or -1: the slab is not verified.  G = 1 + max
 *   col_weight_dev [ncol] (NULL: all 1) the weight w of every row of a column;
 *                     a row counts only where w > 0
 *   col_offset, ncol_total  the columns are columns col_offset .. col_offset +
 *                     ncol - 1 of a state of ncol_total columns (a whole state:
 *                     0, ncol): the tie-break below then agrees across shards
 * A row is VERIFIED when y_i is finite, w > 0 and its slab's group is >= 0.  A
 * verified row is BAD when a member, or a d_m = x_im - y_i (rounded once, in
 * float64), is not finite: bad rows are counted, never summed.  For a good row:
 *   below = #{m: x_im < y_i}, equal = #{m: x_im == y_i} (IEEE: -0.0 == 0.0)
 *   rank  = below + pick, pick in [0, equal] from (seed, R = lead*ncol_total +
 *           col_offset + col) alone: z = seed + (R+1) 0x9E3779B97F4A7C15;
 *           z = (z ^ z>>30) 0xBF58476D1CE4E5B9; z = (z ^ z>>27) 0x94D049BB133111EB;
 *           z ^= z>>31 (mod 2^64); pick = ((z>>32) (equal+1)) >> 32
 *   err   = (sum d_m)/M, the error of the ensemble mean
 *   var   = sum (d_m - err)^2/(M-1); exactly 0.0 when all members are equal
 *   crps  = (sum |d_m|)/M - (sum_j (2j - M + 1) d_(j))/D with d_(0) <= .. <=
 *           d_(M-1) the sorted d and D = M^2, or M(M-1) when `fair` is set
 * Fields (device, [rows], each may be NULL = not wanted; written for EVERY
 * row): below, equal, rank (int, -1 where the row is not verified or bad),
 * crps, err, var (double, NaN there).
 * Group outputs (host): hist [G][M+1] counts of rank, n [G] good rows, n_bad
 * [G] bad rows, sums [G][5] = sum w, sum w crps, sum w err, sum w err^2,
 * sum w var over the good rows.  All four NULL: fields only.
 * One pass reads every row once and sorts it in registers; per-chunk partial
 * sums are reduced in a fixed order by a second small kernel, and there are no
 * floating-point atomics: the same inputs give the same bits, whatever the
 * grid.  The call uses a workspace of its own and leaves everything a later
 * cycle reads as it found it, like efa_obs_impact_dev; it synchronises before
 * returning.
 * EFA_ERR_INVALID, before any launch and with no output written: a NULL ctx,
 * X_dev, verif_dev or slab_group, M < 2 or M > 256, rows != n_lead*ncol,
 * col_offset < 0 or col_offset + ncol > ncol_total, a slab_group entry < -1,
 * some but not all of hist / n / n_bad / sums NULL while a group exists.
 * Read-only option "verify_us": device time (microseconds, HIP events) of the
 * last call. */
int efa_verify_dev(efa_ctx *ctx, long rows, int M, const double *X_dev,
                   const double *verif_dev, long ncol, long n_lead,
                   long col_offset, long ncol_total, const int *slab_group,
                   const double *col_weight_dev, int fair, uint64_t seed,
                   int *below_dev, int *equal_dev, int *rank_dev,
                   double *crps_dev, double *err_dev, double *var_dev,
                   long long *hist, long long *n, long long *n_bad, double *sums);
int efa_verify_f32_dev(efa_ctx *ctx, long rows, int M, const float *X_dev,
                       const double *verif_dev, long ncol, long n_lead,
                       long col_offset, long ncol_total, const int *slab_group,
                       const double *col_weight_dev, int fair, uint64_t seed,
                       int *below_dev, int *equal_dev, int *rank_dev,
                       double *crps_dev, double *err_dev, double *var_dev,
                       long long *hist, long long *n, long long *n_bad, double *sums);

/* ---- ensemble products and probability verification: mean, sd, quantiles, exceedance probabilities, Brier / reliability (Murphy 1973) ----
 * What is read from an adjusted ensemble, and how good its probabilities are.
 *   X_dev [rows][M]   state members (float64; float32 for the _f32 twin, every
 *                     number computed in float64), row i = lead*ncol + col,
 *                     rows = n_lead*ncol, 2 <= M <= 256
 *   q [nq] (host)     quantile levels in [0, 1], nq <= 8
 *   thr [n_lead][nt] (host) thresholds of every slab, nt <= 8; NaN: slab `lead`
 *                     has no threshold j; an infinite one is refused
 * A row is BAD when a member is not finite: every float field of it is NaN, it
 * enters no table and no sum, and it is counted.  Otherwise
 *   mean  = (sum x_m)/M; exactly the common value when all members are equal
 *   sd    = sqrt(sum (x_m - mean)^2/(M-1)); exactly 0.0 when all are equal
 *   quantile at q: numpy's default linear rule on the sorted members x_(0) <=
 *           .. <= x_(M-1): h = q (M-1), lo = min(floor(h), M-1), hi = min(lo+1,
 *           M-1), f = h - lo (the host computes them, in float64); the value is
 *           x_(lo) when f == 0, else min(x_(hi), fma(f, x_(hi) - x_(lo), x_(lo)))
 *   prob at t: k/M, k = #{m: x_m > t} (strict IEEE comparison, one division);
 *           NaN where the slab's threshold is NaN
 * Fields (device, each may be NULL = not wanted; written for EVERY row):
 * mean_dev [rows], sd_dev [rows], quant_dev [nq][rows], prob_dev [nt][rows].
 * Probability verification runs when verif_dev [rows] is given: row i is SCORED
 * at threshold j when y_i is finite, the column weight w > 0 (col_weight_dev
 * [ncol], NULL: all 1), slab_group[lead] = g >= 0 (host, G = 1 + max), thr[lead][j]
 * is finite and the row is not bad; the event is o = (y_i > t).  Host outputs:
 *   table [G][nt][M+1][2]  count of scored rows with forecast count k and
 *                     outcome o (unweighted: the reliability diagram, exact)
 *   n_bad [G][nt]     rows that would be scored but are bad
 *   sums  [G][nt][4]  sum w, sum w (k/M - o)^2, sum w k/M, sum w o
 * One pass reads every row once; the quantiles come from a sort in registers
 * that is compiled only into the kernels a call with nq > 0 runs.  Per-chunk
 * partial sums are reduced in a fixed order by a second small kernel, the
 * table is integer adds, and there are no floating-point atomics: the same
 * inputs give the same bits, whatever the grid.  The call uses a workspace of
 * its own and leaves everything a later cycle reads as it found it; it
 * synchronises before returning.
 * EFA_ERR_INVALID, before any launch and with no output written: a NULL ctx or
 * X_dev, M < 2 or M > 256, rows != n_lead*ncol, nq or nt outside [0, 8], a q
 * outside [0, 1] or NaN, an infinite threshold, nq > 0 with quant_dev NULL,
 * nt > 0 with prob_dev and verif_dev both NULL, verif_dev with nt == 0, with
 * slab_group NULL or with some but not all of table / n_bad / sums NULL, a
 * slab_group entry < -1.
 * Read-only option "products_us": device time (microseconds, HIP events) of
 * the last call. */
int efa_products_dev(efa_ctx *ctx, long rows, int M, const double *X_dev,
                     long ncol, long n_lead, int nq, const double *q, int nt,
                     const double *thr, double *mean_dev, double *sd_dev,
                     double *quant_dev, double *prob_dev,
                     const double *verif_dev, const int *slab_group,
                     const double *col_weight_dev, long long *table,
                     long long *n_bad, double *sums);
int efa_products_f32_dev(efa_ctx *ctx, long rows, int M, const float *X_dev,
                         long ncol, long n_lead, int nq, const double *q, int nt,
                         const double *thr, double *mean_dev, double *sd_dev,
                         double *quant_dev, double *prob_dev,
                         const double *verif_dev, const int *slab_group,
                         const double *col_weight_dev, long long *table,
                         long long *n_bad, double *sums);

/* ---- ensemble Gram matrix in a weighted norm: member distances, EOFs / principal components, clusters ----
 * How the members differ from one another over the whole field:
 *   G = X'^T C X' / (M-1), M x M, X' the rows with their means removed.
 *   X_dev [rows][M]   state members (float64; float32 for the _f32 twin, each
 *                     member converted once, every number computed in float64),
 *                     row i = lead*ncol + col, rows = n_lead*ncol, 2 <= M <= 256
 *   slab_scale [n_lead] (host) the scale s of every slab, finite and >= 0; a slab
 *                     of scale 0 is not read
 *   col_weight_dev [ncol] (NULL: all 1) the weight w of every row of a column
 * The coefficient of row i is c_i = w_col s_lead^2.  A row is USED when s_lead >
 * 0 and w_col > 0 (a negative or NaN weight: not used, and not read).  A used
 * row is BAD when a member or w_col is not finite: bad rows are counted in
 * n_bad and add nothing.  With mean_i = (sum_m x_im)/M, x'_im = x_im - mean_i
 * (exactly 0 when all members are equal), over the used, good rows:
 *   gram [M][M] (host) G_ab = (sum_i c_i x'_ia x'_ib)/(M-1), bit-for-bit symmetric
 *   n                 their number;  n_bad: the used rows that are bad
 *   sums [2]          sum w_col, sum c_i
 * With no used row G is exactly 0.0 everywhere and n = 0.  Scaling the whole
 * state by 2^k scales G by 4^k exactly.  The rows may be a column shard of a
 * larger state: the shards' gram, n, n_bad and sums add up to the whole
 * state's (gram up to rounding).
 * One pass reads every used row once: chunks of 32 rows are centred in LDS and
 * contracted on the fp64 matrix cores, upper-triangle tiles only, into a number
 * of accumulation streams that depends on the sizes alone; a second small
 * kernel adds the streams in a fixed order, mirrors the matrix and divides by
 * M-1.  No floating-point atomics: the same inputs give the same bits,
 * whatever the grid.  The call uses a workspace of its own (at most 134 MB)
 * and leaves everything a later cycle reads as it found it; it runs on the
 * context's stream and synchronises before returning.
 * EFA_ERR_INVALID, before any launch and with no output written: a NULL ctx,
 * X_dev, slab_scale, gram, n, n_bad or sums, M < 2 or M > 256, rows !=
 * n_lead*ncol, a slab_scale that is not finite or < 0.
 * Read-only option "gram_us": device time (microseconds, HIP events) of the
 * last call; "gram_blocks" caps the grid. */
int efa_gram_dev(efa_ctx *ctx, long rows, int M, const double *X_dev,
                 long ncol, long n_lead, const double *slab_scale,
                 const double *col_weight_dev, double *gram,
                 long long *n, long long *n_bad, double *sums);
int efa_gram_f32_dev(efa_ctx *ctx, long rows, int M, const float *X_dev,
                     long ncol, long n_lead, const double *slab_scale,
                     const double *col_weight_dev, double *gram,
                     long long *n, long long *n_bad, double *sums);

/* ---- neighbourhood ensemble probabilities and the fractions skill score (Schwartz et al. 2010; Schwartz and Sobash 2017; Roberts and Lean 2008) ----
 * The products that need the (y, x) structure of the state.
 *   X_dev [rows][M]   state members (float64; float32 for the _f32 twin, each
 *                     member converted once, compared in float64), row
 *                     i = lead*ncol + y*nx + x, ncol = ny*nx, rows = n_lead*ncol,
 *                     2 <= M <= 256
 *   thr [n_lead][nt] (host) thresholds of every slab, 1 <= nt <= 8; NaN: slab
 *                     `lead` has no threshold j; an infinite one is refused
 *   radius [nr] (host) radii in grid points, 1 <= nr <= EFA_NBR_MAX_RADII,
 *                     0 <= r <= EFA_NBR_MAX_RADIUS
 * A row is VALID when every member is finite and, in a call with verif_dev,
 * its y_i is finite.  An invalid row adds nothing to any window, and every
 * field is NaN at an invalid centre.  The window W_r(y, x) lies within one
 * slab: shape 0 (square) |dy| <= r and |dx| <= r; shape 1 (disc) dy*dy + dx*dx
 * <= r*r, in integers.  Rows outside 0 <= y+dy < ny are left out; columns
 * outside 0 <= x+dx < nx are left out when wrap_x = 0 and taken modulo nx when
 * wrap_x = 1 (which needs 2r+1 <= nx for every radius).  With k_i = #{m: x_im >
 * t} (strict IEEE comparison), over the valid rows i' of the window:
 *   n    = their number,  S = sum k_i'
 *   NEP  = (double)S / ((double)M * (double)n), one division; at r = 0 bit for
 *          bit efa_products_dev's prob
 *   NMEP = (double)#{m: some i' has x_i'm > t} / (double)M
 * Fields (device, each may be NULL = not wanted; written for EVERY row; NaN
 * where the centre is invalid or the slab's threshold is NaN):
 * nep_dev [nr][nt][rows], nmep_dev [nr][nt][rows].
 * With verif_dev [rows]: o_i = (y_i > t) on valid rows, O = (double)(sum of o
 * over the valid rows of the window) / (double)n.  Centre i is SCORED when it is
 * valid, its column weight w > 0 (col_weight_dev [ncol], NULL: all 1; a centre
 * of weight 0 still counts in its neighbours' windows), slab_group[lead] = g >=
 * 0 (host, G = 1 + max) and thr[lead][j] is finite.  Host outputs, with P = NEP:
 *   sums  [G][nr][nt][6]  sum w, sum w (P-O)^2, sum w P^2, sum w O^2, sum w P,
 *                     sum w O
 *   n     [G][nr][nt]     scored centres
 *   n_bad [G][nr][nt]     centres that would be scored but have a member that
 *                     is not finite
 * One pass reads every row of the slabs that are needed once (a slab whose
 * thresholds are all NaN, or which no field and no group wants, is not read)
 * and leaves a compact record per row in the call's workspace; a second kernel
 * forms the windows over the records in LDS.  The records of the slabs held at
 * a time take at most EFA_NBR_WS_BYTES (option "nbr_ws_bytes" lowers that; a
 * batch is at least one slab), the slabs are processed in batches, and the
 * per-tile partial sums (64 nr nt bytes per tile of 1024 rows when scoring) and
 * small tables come on top.  The partials are added in a fixed order by a third
 * small kernel; there are no floating-point atomics: the same inputs give the
 * same bits, whatever the grid and the batches.  The call leaves everything a
 * later cycle reads as it found it and synchronises before returning.
 * EFA_ERR_INVALID, before any launch and with no output written: a NULL ctx,
 * X_dev, thr or radius, M < 2 or M > 256, a negative size or rows !=
 * n_lead*ny*nx, nt outside [1, 8], nr outside [1, 4], a radius outside [0, 64],
 * shape or wrap_x not 0 or 1, wrap_x with 2r+1 > nx, an infinite threshold,
 * some but not all of sums / n / n_bad NULL, no output wanted (nep_dev and
 * nmep_dev NULL and nothing to score), verif_dev without slab_group, a
 * slab_group entry < -1.
 * Read-only option "neighbourhood_us": device time (microseconds, HIP events)
 * of the last call; "neighbourhood_blocks" caps the grids. */
#define EFA_NBR_MAX_THRESHOLDS 8
#define EFA_NBR_MAX_RADII 4
#define EFA_NBR_MAX_RADIUS 64
#define EFA_NBR_WS_BYTES (256L << 20) /* cap of the records held at a time */
int efa_neighbourhood_dev(efa_ctx *ctx, long rows, int M, const double *X_dev,
                          long ny, long nx, long n_lead, int nt,
                          const double *thr, int nr, const int *radius,
                          int shape, int wrap_x, double *nep_dev,
                          double *nmep_dev, const double *verif_dev,
                          const int *slab_group, const double *col_weight_dev,
                          double *sums, long long *n, long long *n_bad);
int efa_neighbourhood_f32_dev(efa_ctx *ctx, long rows, int M, const float *X_dev,
                              long ny, long nx, long n_lead, int nt,
                              const double *thr, int nr, const int *radius,
                              int shape, int wrap_x, double *nep_dev,
                              double *nmep_dev, const double *verif_dev,
                              const int *slab_group,
                              const double *col_weight_dev, double *sums,
                              long long *n, long long *n_bad);

/* ---- the probability-matched ensemble mean (Ebert 2001) and its patch-wise form (Clark 2017; Snook et al. 2019) ----
 * The pattern of a rank field with the amplitude distribution of all members
 * pooled.
 *   X_dev [rows][M]   state members (float64; float32 for the _f32 twin), row
 *                     i = lead*ny*nx + y*nx + x, rows = n_lead*ny*nx,
 *                     2 <= M <= 256
 *   rank_dev [rows]   the rank field f (float64), usually efa_products_dev's
 *                     mean or a smoothed form of it
 *   slab_on [n_lead] (host) 0: the slab is not read, its output is NaN and its
 *                     n_bad 0; NULL: every slab is on
 *   py, px            the patch, 1 <= py <= ny and 1 <= px <= nx
 *   pick              g in [0, M): M/2 is the usual choice, M-1 Ebert's (the PM
 *                     maximum is the pooled maximum), 0 its mirror image
 * A SEGMENT is one patch of one slab: patch (Y, X) holds the elements with
 * y/py == Y and x/px == X; the patches at the upper edges are smaller.
 * (py, px) = (ny, nx) is one segment per slab, the classic PM mean.
 * A row is EXCLUDED when f_i is not finite or a member is not finite: its
 * output is NaN, it enters no pool, and it is counted in n_bad [n_lead] (host).
 * Within a segment with n included rows:
 *   order = the included rows by f ascending, ties by row index ascending;
 *           -0.0 and +0.0 are the same value for this comparison
 *   pool  = the n*M members of the included rows ascending, -0.0 stored as +0.0
 *   the row at position r of order gets pool[r*M + g]
 * pm_dev [rows] (device, float64) is written for EVERY row; for a float32 state
 * it is the selected member widened, which is exact.  No arithmetic is done on
 * the values: everything is integer work on order-preserving keys (the bits of
 * v + 0.0, the sign bit flipped for v >= 0, every bit for v < 0), so the same
 * inputs give the same bits whatever the grid, the batches and the options.
 * One kernel reads the rows of a batch of slabs once and writes the keys at the
 * row's place in its segment (an excluded row writes all-ones keys, which no
 * finite value has and which sort to the end); a segmented LSD radix sort, 8
 * bits a pass, stable, sorts the pooled keys and (with the row as payload) the
 * rank keys; a last kernel assigns.  A pass is four launches (histograms of
 * tiles of EFA_PM_TILE_KEYS keys, their sums per unit of EFA_PM_UNIT_BLOCKS
 * tiles, the scan per segment, the stable scatter) ordered by the kernel
 * boundaries alone; a pass whose byte holds one digit in every segment is
 * skipped.  No floating-point atomics.  The call owns its workspace: the two
 * pooled key buffers of the slabs held at a time take at most EFA_PM_WS_BYTES
 * (option "pm_ws_bytes" lowers that; a batch is at least one slab), the rank
 * keys, 1 KiB of histograms per tile, 3 KiB of scans per unit and the tables
 * come on top.  It
 * runs on the context's stream, leaves everything a later cycle reads as it
 * found it and synchronises before returning.
 * EFA_ERR_INVALID, before any launch and with nothing written: a NULL ctx,
 * X_dev, rank_dev, pm_dev or n_bad, M < 2 or M > 256, a negative size or rows
 * != n_lead*ny*nx, py outside [1, ny], px outside [1, nx], pick outside [0, M),
 * a slab of 2^32 rows or more.
 * Read-only options: "pm_us", device time (microseconds, HIP events) of the
 * last call; "pm_passes" and "pm_rank_passes", the radix passes it ran on the
 * pool and on the rank keys, summed over its batches.  "pm_blocks" caps the
 * grids. */
#define EFA_PM_WS_BYTES (1L << 30) /* cap of the two pooled key buffers held at a time */
#define EFA_PM_TILE_KEYS 4096      /* keys of a sort block */
#define EFA_PM_UNIT_BLOCKS 32      /* sort blocks of a scan unit */
int efa_pm_mean_dev(efa_ctx *ctx, long rows, int M, const double *X_dev,
                    long ny, long nx, long n_lead, const double *rank_dev,
                    const int *slab_on, long py, long px, int pick,
                    double *pm_dev, long long *n_bad);
int efa_pm_mean_f32_dev(efa_ctx *ctx, long rows, int M, const float *X_dev,
                        long ny, long nx, long n_lead, const double *rank_dev,
                        const int *slab_on, long py, long px, int pick,
                        double *pm_dev, long long *n_bad);

/* ---- measurement support --------------------------------------------------
 * Device time (ms) spent in the state-sweep kernels and in the obs-space
 * kernels during the most recent efa_ensrf_update_dev / efa_obs_phase_dev /
 * efa_state_phase_dev / efa_state_cycle_dev / efa_ensrf_cycle_dev call, measured with HIP events on
 * the context's stream, plus the number of state-sweep launches and the path
 * taken (EFA_PATH_SWEEP / EFA_PATH_TRANSFORM).  Timing is off by default;
 * enable with efa_ctx_set_option(ctx, "timing", 1): every state-phase call
 * then ends in a wait for its own end event.  "timing" 2 is the deferred
 * form for back-to-back cycles: no call waits for its events (an interval is
 * read when its events are next re-recorded, or here), and efa_last_timing
 * returns the SUMS of state_ms, obs_ms and state_launches over the calls since
 * the previous efa_last_timing (which it clears); it waits for the last
 * recorded events, so call it after the cycles of interest. */
int efa_last_timing(efa_ctx *ctx, double *state_ms, double *obs_ms,
                    long *state_launches, int *path_taken);

/* Fill rows of a resident state with the bench's synthetic ensemble
 * (SURVEY.md 8d): X[i,m] = mu_i + sigma*z_im with counter-based normal
 * deviates keyed by (seed, global row, member), so any sharding of the rows
 * produces identical data. */
int efa_fill_synthetic_dev(efa_ctx *ctx, long rows, long row_offset, int M,
                           uint64_t seed, double sigma, double *X_dev);

/* ---- multi-GPU, one process per GPU ----------------------------
 * The reference has no working multi-process path; its sketch (assimilation.py:186-193,
 * ensemble.py:98-106) computes the obs priors once and hands them to every
 * worker.  Here the state is sharded by (y,x) column; each rank calls
 * efa_forward_interp_dev / efa_forward_stencil_dev on its own columns and the
 * P x M partial sums are added over the ranks by ONE all-reduce
 * (ncclAllReduce, sum, float64, over xGMI) issued on the context's stream.
 * Afterwards every rank runs efa_obs_phase_dev on the identical obs block and
 * efa_state_cycle_dev on its own rows: no per-observation communication.
 *
 * The communicator lives inside the context.  librccl is opened with dlopen by
 * efa_comm_unique_id / efa_comm_init, so single-GPU callers never load it.
 * Rank 0 obtains an id and hands the EFA_COMM_ID_BYTES bytes to the other
 * ranks by any means (MPI, a file, torch.distributed); then every rank calls
 * efa_comm_init collectively. */
#define EFA_COMM_ID_BYTES 128
int efa_comm_unique_id(uint8_t *id_out /* [EFA_COMM_ID_BYTES] */);
int efa_comm_init(efa_ctx *ctx, const uint8_t *id, int rank, int world);
int efa_comm_destroy(efa_ctx *ctx);
/* buf_dev[count] <- sum over ranks, in place, on the context's stream (asynchronous:
 * ordered before whatever is issued on the context afterwards) */
int efa_allreduce_sum_dev(efa_ctx *ctx, double *buf_dev, long count);

/* Cost of the localised state sweep per block of 16 consecutive (y,x) columns
 * of a grid: block_count[b] = number of assimilated observations whose
 * Gaspari-Cohn weight (observation.py:117-130 on ensemble.py:254-267 distances) is
 * non-zero on at least one of columns 16b..16b+15 -- the length of the block's
 * active list in the one-pass sweep; block_pairs[b] (optional) = (column,
 * observation) pairs with a non-zero weight inside the block (the sweep's waves
 * skip an observation that is zero on their four columns, so its work follows the
 * pairs); *active_pairs = their total.  Host arrays of (ncol+15)/16 entries.
 * Used to cut the columns into contiguous shards of equal cost
 * (the reference's sketch cuts equal chunks, ensemble.py:98-106, which leaves
 * polar shards of a lat/lon grid with several times the work). */
int efa_gc_block_counts(efa_ctx *ctx, long ncol, const double *grid_lat,
                        const double *grid_lon, long P, const double *ob_lat,
                        const double *ob_lon, const double *ob_halfwidth_km,
                        const uint8_t *ob_assim, int32_t *block_count,
                        int32_t *block_pairs, uint64_t *active_pairs);

#ifdef __cplusplus
}
#endif
#endif /* EFA_HIP_H */
