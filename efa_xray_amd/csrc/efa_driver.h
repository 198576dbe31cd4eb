// What the host-side translation units of libefa_hip.so share.  Not exported.
//   efa_capi.hip     the extern "C" shell: contexts, options, memory helpers, the public wrappers, efa_last_timing
//   efa_phase_a.hip  the obs phase (Phase A): staging, the window driver, the speculative transform
//   efa_phase_b.hip  the state phase (Phase B): relaxation glue, the column grid, the sweeps and the two state calls
//   efa_stream.hip   the streamed host-memory update
//   efa_comm.hip     RCCL
// One call's arguments and results travel as arguments and return values; the context (efa_ctx.h) holds settings, caches,
// workspaces and what the last obs phase left for the state phase.
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
int obs_phase(efa_ctx* c, int M, long P, double* ym_dev, double* Yp_dev, const double* ob_value, const double* ob_error,
              const uint8_t* ob_assim, int loc_mode, const double* ob_lat, const double* ob_lon, const double* ob_hw,
              double* prior_mean, double* prior_var, double* post_mean, double* post_var, uint8_t* assimilated,
              const SpecRequest& spec = SpecRequest{}, SpecResult* spec_out = nullptr);

// ---- efa_phase_b.hip ----------------------------------------------------------------------------------------------------------
int check_adaptive(const efa_ctx* c, int loc_mode, long rows);
int check_vloc(const efa_ctx* c, int loc_mode, long P, long n_lead);
inline bool vl_active(const efa_ctx* c) { return c->vl_on && c->vl_any; }
inline const double* vl_lead(const efa_ctx* c) { return c->vl_dev.as<double>(); }
inline const double* vl_obvert(const efa_ctx* c) { return c->vl_dev.as<double>() + c->vl_nlead; }
inline const double* vl_obvhw(const efa_ctx* c) { return c->vl_dev.as<double>() + c->vl_nlead + c->vl_P; }
bool auto_transform(int M, long n_active, bool member_form);
bool want_transform(const efa_ctx* c, bool member_form);
int transform_with_relaxation(efa_ctx* c, efa::TransformArgs t, long* nl, bool f32 = false);
efa::TransformArgs carried_transform(const efa_ctx* c, const double* Xin, const double* xin, double* Xout, double* xout, long rows,
                                     int fused_members);
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
int state_cycle(efa_ctx* c, long rows, int M, const double* X_dev, double* post_dev, const double* grid_lat,
                const double* grid_lon, long ncol, long n_lead, const StateCall& o = StateCall{});
// the member form on float32 rows: natively where a float32 kernel exists, through the float64 workspace otherwise (c->f32_native)
int state_cycle_f32(efa_ctx* c, long rows, int M, const float* X_dev, float* post_dev, const double* grid_lat,
                    const double* grid_lon, long ncol, long n_lead, const StateCall& o = StateCall{});
// end of a state call: the launch count into the sum; "timing" 1 waits and reads the interval, 2 leaves it pending.
// end_recorded: iv.end is in the stream already (a speculative transform that turned out right)
int end_state_call(efa_ctx* c, Interval& iv, bool timed = true, bool end_recorded = false);

}  // namespace efa_host
