// What the host-side translation units of libefa_hip.so share.  Not exported.
//   efa_capi.hip     the extern "C" shell: contexts, options, memory helpers, the public wrappers, efa_last_timing
//   efa_phase_a.hip  the obs phase (Phase A): staging, the window driver, the speculative transform
//   efa_phase_b.hip  the state phase (Phase B): the column grid, the plan of a state call, its executor and the state calls
//   efa_stream.hip   the streamed host-memory update
//   efa_impact.hip   observation impact: its kernels and the driver of efa_obs_impact_dev
//   efa_sensitivity.hip  ensemble sensitivity and observation targeting: its kernels and the driver of efa_sensitivity_dev
//   efa_verify.hip   ensemble verification: its kernels and the driver of efa_verify_dev
//   efa_products.hip ensemble products and probability verification: its kernels and the driver of efa_products_dev
//   efa_neighbourhood.hip neighbourhood probabilities and the fractions skill score: its kernels and the driver of efa_neighbourhood_dev
//   efa_pmmean.hip   the probability-matched mean and the segmented radix sort under it: its kernels and the driver of efa_pm_mean_dev
//   efa_gram.hip     the ensemble Gram matrix: its kernels and the driver of efa_gram_dev
//   efa_etkf.hip     the batch observation-space solver's kernels (option "obs_solver" 1; driven from efa_phase_a.hip)
//   efa_letkf.hip    the local ensemble transform Kalman filter: its kernels and their launcher (plain, or per slab group)
//   efa_letkf_interp.hip  the interpolate-and-apply kernel of the weight-interpolation entries and its launcher
//   efa_letkf_driver.hip  the driver of every efa_letkf_* entry: the cycles (plain / interp / slab), the weights, efa_letkf_interp_apply_dev
//   efa_comm.hip    RCCL
// Headers the diagnostics share: efa_quadrow.h (the four-lane row layout of k_sens_pass, k_verify, k_products and k_nbr_records),
// efa_sortnet.h (the bitonic network on it), efa_quadreduce.h (table flush, chunk partial, k_group_reduce) and efa_diag.h (their
// drivers' host scaffolding: the interval helper, WsLayout, check_slab_groups, pad_thresholds, pairs_aligned, clamp_blocks, launch_quad).
// One call's arguments and results travel as arguments and return values; the context (efa_ctx.h) holds settings, caches,
// workspaces and what the last obs phase left for the state phase.  A state call's rows travel with their element type (StateRows);
// its route is decided once, by plan_state, and every caller issues the launches through run_state_plan.  The host per-observation
// arrays of a call travel as one ObsIn and its host diagnostics as one DiagOut, from the extern "C" wrappers (which fill them by
// name, obs_in / diag_out) down to the obs phase, the streamed update, the impact call and the LETKF; the device obs block
// (ym_dev, Yp_dev) stays beside them -- the EnSRF writes it in place, the LETKF only reads it.
#pragma once
#include "efa_ctx.h"
#include "efa_internal.h"

namespace efa_host {

// ---- efa_capi.hip -------------------------------------------------------------------------------------------------------------
int use(efa_ctx* c);  // null check, hipSetDevice
int h2d(efa_ctx* c, DevBuf& b, const void* src, size_t bytes);
int form_perts(efa_ctx* c, long rows, int M, const double* X_dev, double scale, double* xm_dev, double* Xp_dev);
// "timing": a pending interval is waited for and read into obs_ms / state_ms and the running sums
void harvest_obs_ms(efa_ctx* c);
void harvest_state_interval(efa_ctx* c, Interval& iv);
void harvest_state_ms(efa_ctx* c);  // both state intervals

// The per-observation inputs of a call, [P] each on the host: lat / lon / hw (the half-width, km) are read under EFA_LOC_GC only.
// The impact call carries the innovations in `value` and ob_used in `assim`; the LETKF sets loc_mode EFA_LOC_GC.
struct ObsIn {
  const double *value = nullptr, *error = nullptr;
  const uint8_t* assim = nullptr;
  int loc_mode = EFA_LOC_NONE;
  const double *lat = nullptr, *lon = nullptr, *hw = nullptr;
};
// the five host diagnostics of a call, [P] each or null
struct DiagOut {
  double *prior_mean = nullptr, *prior_var = nullptr, *post_mean = nullptr, *post_var = nullptr;
  uint8_t* assimilated = nullptr;
};
// how the extern "C" wrappers fill them: every field by name, so that no positional list of look-alike pointers is left to swap
inline ObsIn obs_in(const double* value, const double* error, const uint8_t* assim, int loc_mode, const double* lat, const double* lon,
                    const double* hw) {
  ObsIn o;
  o.value = value;
  o.error = error;
  o.assim = assim;
  o.loc_mode = loc_mode;
  o.lat = lat;
  o.lon = lon;
  o.hw = hw;
  return o;
}
inline DiagOut diag_out(double* prior_mean, double* prior_var, double* post_mean, double* post_var, uint8_t* assimilated) {
  DiagOut d;
  d.prior_mean = prior_mean;
  d.prior_var = prior_var;
  d.post_mean = post_mean;
  d.post_var = post_var;
  d.assimilated = assimilated;
  return d;
}

// ---- efa_comm.hip -------------------------------------------------------------------------------------------------------------
void release_comm(efa_ctx* c);  // efa_ctx_destroy: the communicator goes, errors ignored

// ---- efa_phase_a.hip ----------------------------------------------------------------------------------------------------------
int check_common(int M, long P);
long effective_batch(const efa_ctx* c, int M);
// efa_ensrf_cycle_dev asks the obs phase to put the member-form transform of `rows` state rows (prior X, posterior post, disjoint)
// into the stream behind the persistent launch, before that launch's status is known; rows 0: no speculation.  obs_out 0: the
// caller's obs block is not written back.
struct SpecRequest {
  const double* X = nullptr;
  double* post = nullptr;
  long rows = 0;
  bool obs_out = true;
};
// ... and what came of it: the transform is in the stream behind the launch that did Phase A, timed by *interval
struct SpecResult {
  bool launched = false;
  Interval* interval = nullptr;
  long launches = 0;  // state-phase launches it took (the transform, and the relaxation's)
};
int obs_phase(efa_ctx* c, int M, long P, double* ym_dev, double* Yp_dev, const ObsIn& ob, const DiagOut& diag,
              const SpecRequest& spec = SpecRequest{}, SpecResult* spec_out = nullptr);

// ---- efa_phase_b.hip ----------------------------------------------------------------------------------------------------------
int check_adaptive(const efa_ctx* c, int loc_mode, long rows);
int check_vloc(const efa_ctx* c, int loc_mode, long P, long n_lead);
inline bool vl_active(const efa_ctx* c) { return c->vl_on && c->vl_any; }
inline const double* vl_lead(const efa_ctx* c) { return c->vl_dev.as<double>(); }
inline const double* vl_obvert(const efa_ctx* c) { return c->vl_dev.as<double>() + c->vl_nlead; }
inline const double* vl_obvhw(const efa_ctx* c) { return c->vl_dev.as<double>() + c->vl_nlead + c->vl_P; }
// temporal and cross-variable localisation: as check_vloc for that setting, and its arrays on the device
int check_slab(const efa_ctx* c, int loc_mode, long P, long n_lead);
inline bool sl_active(const efa_ctx* c) { return c->sl_on && c->sl_any; }
inline const double* sl_lead_time(const efa_ctx* c) { return c->sl_dev.as<double>(); }
inline const int* sl_ints(const efa_ctx* c) {
  return reinterpret_cast<const int*>(c->sl_dev.as<double>() + c->sl_nlead + 2 * c->sl_P + c->sl_ngroup * c->sl_nvar);
}
inline const int* sl_lead_var(const efa_ctx* c) { return sl_ints(c); }
inline efa::SlabObs sl_obs(const efa_ctx* c, long w0) {  // the obs' side from ob w0 on
  const double* d = c->sl_dev.as<double>();
  const int* i = sl_ints(c);
  return efa::SlabObs{d + c->sl_nlead + w0, d + c->sl_nlead + c->sl_P + w0, i + c->sl_nlead + w0, i + c->sl_nlead + c->sl_P + w0,
                      d + c->sl_nlead + 2 * c->sl_P, c->sl_nvar};
}
// sampling error correction: while it is set every call must be a GC cycle on the one-pass sweep, without adaptive
// inflation, vertical or slab localisation (no combined kernel; Phase A then runs its one-ob batches)
int check_sec(const efa_ctx* c, int loc_mode);
inline bool sec_active(const efa_ctx* c) { return c->sec_T > 0; }
// the batch solver (option "obs_solver" 1): refused with GC localisation, an adaptive-inflation field or path sweep;
// and an assimilated ob's error variance must be finite and > 0 (efa_phase_a.hip; null arrays are left to the obs phase's own check)
int check_batch_solver(const efa_ctx* c, int loc_mode);
int check_batch_obs(const efa_ctx* c, long P, const double* ob_error, const uint8_t* ob_assim);
// the slab table S[P][n_lead] on the device, rebuilt when the slab or the vertical setting changed since it was written
int ensure_slab_table(efa_ctx* c);
using efa::Elem;
// The rows of one state call, prior and posterior: [rows][M] members of type elem, or the perturbation form's float64 perturbations
struct StateRows {
  const void* prior = nullptr;
  void* post = nullptr;
  Elem elem = Elem::f64;
  long rows = 0;
  int M = 0;
  size_t count() const { return (size_t)(rows > 0 ? rows : 0) * (size_t)(M > 0 ? M : 0); }
  size_t bytes() const { return count() * efa::elem_size(elem); }
  bool disjoint() const {  // the posterior is written clear of the prior
    const char *a = static_cast<const char*>(prior), *b = static_cast<const char*>(post);
    return a + bytes() <= b || b + bytes() <= a;
  }
  bool in_place() const { return !disjoint(); }
  // in place means over the prior exactly: a posterior that overlaps the prior without coinciding with it is served by no kernel
  bool partial_overlap() const { return in_place() && prior != post; }
  // As the kernel argument structs carry rows of either type: the launchers that take `elem` (launch_transform, launch_transform_rtps,
  // launch_sweep_gc) pick the kernels that read them.  Every other pass is float64 only, and no plan sends float32 rows there.
  const double* in() const { return static_cast<const double*>(prior); }
  double* out() const { return static_cast<double*>(post); }
};
// What a state call will do: plan_state decides it from the context's settings, what the last obs phase left (M, P, n_active,
// loc_mode, the records) and its arguments -- have_transform: c->have_transform, or ahead of Phase A's end what it will be -- and
// launches and writes nothing.  run_state_plan issues a plan's launches on the context's stream (xm_in / xm_out: the means of the
// perturbation form) and counts them; report_state_call sets what the call reports (efa_last_timing, "f32_native") from both.
enum class Route { transform, gc_onepass, sweeps };      // through [T | w] | the one-pass GC sweep | the per-batch sweeps
enum class Relax { none, folded, fused, standalone };    // RTPP folded into T | RTPS fused into the transform | passes around the route
struct StatePlan {
  Route route = Route::sweeps;
  Relax relax = Relax::none;
  bool member_form = true;
  int ws_copies = 0;        // float32 rows: 0 the kernels read and write the float rows; else copies of the state in the float64 workspace
  bool copy_prior = false;  // in place, transform above 136 members, no workspace: it reads a copy of the prior
};
StatePlan plan_state(const efa_ctx* c, bool member_form, Elem elem, bool in_place, bool have_transform);
int run_state_plan(efa_ctx* c, const StatePlan& p, const StateRows& r, const double* xm_in, double* xm_out, long ncol, long n_lead,
                   long* launches);
void report_state_call(efa_ctx* c, const StatePlan& p, Elem elem, long launches);
int read_gc_pairs(efa_ctx* c);
// the one check of a localised call's grid arguments (no-op without localisation)
int check_grid(int loc_mode, const double* grid_lat, const double* grid_lon, long ncol, long n_lead, long rows);
// How one state call differs from the plain public one.
struct StateCall {
  bool grid_current = false;  // the caller brought c->grid up to date already (ahead of Phase A, or from a device slice)
  bool timed = true;          // false: record no events whatever "timing" says (the streamed chunks keep their own)
};
int state_phase(efa_ctx* c, long rows, int M, const double* xm_in, const double* Xp_in, double* xm_out, double* Xp_out,
                const double* grid_lat, const double* grid_lon, long ncol, long n_lead, const StateCall& o = StateCall{});
// the member form, on float64 or float32 rows
int state_cycle(efa_ctx* c, const StateRows& r, const double* grid_lat, const double* grid_lon, long ncol, long n_lead,
                const StateCall& o = StateCall{});
// end of a state call: the launch count into the sum; "timing" 1 waits and reads the interval, 2 leaves it pending.
// end_recorded: iv.end is in the stream already (a speculative transform that turned out right)
int end_state_call(efa_ctx* c, Interval& iv, bool timed = true, bool end_recorded = false);

// ---- efa_letkf_driver.hip -----------------------------------------------------------------------------------------------------
// efa_letkf_cycle_dev / _f32_dev: checks, the obs' effective flags and prior diagnostics, the lists and the solve at every ob
// position (the obs block), the lists and the solve of every grid column (the state); waits before it returns the diagnostics.
// ym_dev / Yp_dev: the prior obs block, only read; ym_out / Yp_out: where the posterior obs block goes (obs_block_out: the caller's
// block), both null: nowhere
int letkf_cycle(efa_ctx* c, const StateRows& r, long P, const double* ym_dev, const double* Yp_dev, const ObsIn& ob, double* ym_out,
                double* Yp_out, const double* grid_lat, const double* grid_lon, long ncol, long n_lead, const DiagOut& diag,
                double* col_stats_dev, const efa::LetkfMesh* mesh, bool slab);
// (mesh: efa_letkf_cycle_interp_dev / _f32_dev, DESIGN.md §7y-2 -- ncol is taken from it, the solve runs at its nodes only into a
// buffer of the context, col_stats_dev receives the NODE statistics, and efa_letkf_interp.hip's kernel interpolates the pairs to
// every column and applies them; a unit stride is the call without a mesh)
// (slab: efa_letkf_slab_cycle_dev and its kin, DESIGN.md §7y-3 -- one solve per (slab group, column) under the vertical and / or slab
// setting; col_stats_dev is then [ngroups][ncol or nnodes][3])
// (the context's control, efa_ctx_set_letkf_control, DESIGN.md §7y-7: served without a mesh, sized for this call's rows and P;
// with a mesh, and by letkf_weights, the call is refused while it is set; letkf_interp_apply ignores it)
// (the context's obs cap, efa_ctx_set_letkf_obs_cap, DESIGN.md §7y-8: served by the plain and the interp cycle and by letkf_weights,
// sized for this call's P and solve points; the slab calls are refused while it is set; letkf_interp_apply ignores it)
// (the context's cross validation, efa_ctx_set_letkf_cross_validation, DESIGN.md §7y-9: served by the plain and the interp cycle and by
// letkf_weights, sized for this call's M and solve points, without an inflation field and without a control; the state then always
// goes "solve the points, apply their pairs", without a mesh on the unit mesh; the slab calls are refused while it is set;
// letkf_interp_apply ignores it)
// efa_letkf_interp_apply_dev / _f32_dev: that kernel alone on caller-given node pairs, under the context's relaxation; waits
int letkf_interp_apply(efa_ctx* c, const StateRows& r, const efa::LetkfMesh& mesh, long n_lead, const double* Tw_nodes_dev,
                       const double* node_stats_dev);
// efa_letkf_weights_dev: the same solve at caller-given points, [T | w] of each to Tw_dev; waits
int letkf_weights(efa_ctx* c, int M, long P, const double* ym_dev, const double* Yp_dev, const ObsIn& ob, long npts, const double* pt_lat,
                  const double* pt_lon, double* Tw_dev, double* stats_dev, bool slab);
// (slab: efa_letkf_slab_weights_dev -- Tw_dev [ngroups][npts][M][M + 1], stats_dev [ngroups][npts][3])
// efa_letkf_slab_groups: the group of every slab under the context's settings, numbered by first appearance
int letkf_slab_group_table(efa_ctx* c, long n_lead, int* group_of, int* ngroups);

// ---- efa_impact.hip -----------------------------------------------------------------------------------------------------------
// efa_obs_impact_dev: checks, the call's own active lists, the contraction and its reduction; waits before it returns impact[P].
// ob.value: the innovations, ob.assim: ob_used.
// slab_entry: efa_obs_impact_slab_dev -- the same call under the temporal and variable tapers while the slab setting is on (the
// contraction reads the slab table, brought up to date first); the plain call while it is off
int obs_impact(efa_ctx* c, long rows, int M, long P, const double* Xf_dev, const double* werr_dev, const double* Ya_dev, const ObsIn& ob,
               const double* grid_lat, const double* grid_lon, long ncol, long n_lead, double* impact, bool slab_entry);

// ---- efa_sensitivity.hip ------------------------------------------------------------------------------------------------------
// efa_sensitivity_dev / _f32_dev: checks, the passes and the host algebra between them; waits before it returns
int sensitivity(efa_ctx* c, Elem elem, long rows, int M, int K, const void* X_dev, const double* J, long ncol, long n_lead,
                const double* slab_error, const double* weights, const uint8_t* cand_dev, int n_targets, double* var_dev,
                double* cov_dev, double* sens_dev, double* corr_dev, double* dvar_dev, double* score_dev, long* picked_row,
                double* picked_score, double* metric_var);

// ---- efa_verify.hip -----------------------------------------------------------------------------------------------------------
// efa_verify_dev / _f32_dev: checks, the pass and the reduction of its partials; waits before it returns
int verify(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, const double* verif_dev, long ncol, long n_lead,
           long col_offset, long ncol_total, const int* slab_group, const double* col_weight_dev, int fair, uint64_t seed,
           int* below_dev, int* equal_dev, int* rank_dev, double* crps_dev, double* err_dev, double* var_dev, long long* hist,
           long long* n, long long* n_bad, double* sums);

// ---- efa_products.hip ---------------------------------------------------------------------------------------------------------
// efa_products_dev / _f32_dev: checks, the pass and the reduction of its partials; waits before it returns
int products(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, long ncol, long n_lead, int nq, const double* q, int nt,
             const double* thr, double* mean_dev, double* sd_dev, double* quant_dev, double* prob_dev, const double* verif_dev,
             const int* slab_group, const double* col_weight_dev, long long* table, long long* n_bad, double* sums);

// ---- efa_gram.hip -------------------------------------------------------------------------------------------------------------
// efa_gram_dev / _f32_dev: checks, the pass and the reduction of its partials; waits before it returns
int gram(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, long ncol, long n_lead, const double* slab_scale,
         const double* col_weight_dev, double* gram_out, long long* n, long long* n_bad, double* sums);

// ---- efa_neighbourhood.hip ----------------------------------------------------------------------------------------------------
// efa_neighbourhood_dev / _f32_dev: checks, the records and the windows batch by batch, the reduction; waits before it returns
int neighbourhood(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, long ny, long nx, long n_lead, int nt, const double* thr,
                  int nr, const int* radius, int shape, int wrap_x, double* nep_dev, double* nmep_dev, const double* verif_dev,
                  const int* slab_group, const double* col_weight_dev, double* sums, long long* n, long long* n_bad);

// ---- efa_pmmean.hip -----------------------------------------------------------------------------------------------------------
// efa_pm_mean_dev / _f32_dev: checks, then batch by batch the keys, the two sorts and the assignment; waits before it returns
int pm_mean(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, long ny, long nx, long n_lead, const double* rank_dev,
            const int* slab_on, long py, long px, int pick, double* pm_dev, long long* n_bad);

}  // namespace efa_host
