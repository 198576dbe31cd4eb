// Phase B, the state phase (efa_driver.h): the checks of the settings that bind a state phase, the column grid, the plan of a state
// call (plan_state), its launches (run_state_plan: relaxation glue, sweeps) and the state calls (perturbation and member form).
#include "efa_driver.h"

#include <cstring>

namespace efa_host {

using namespace efa;

// ---- posterior relaxation (RTPP / RTPS, efa_relax.hip): the standalone passes -------------------------------------------------
// Applied only where a state phase writes the caller's state rows, and only when an ob was assimilated (otherwise the posterior
// is returned exactly as without it).  Float64 rows only: the plan sends float32 rows that need them through the workspace.
namespace {
// core(), the state phase's pass(es) from prior rows to posterior rows, between the plan's standalone passes: before it what the
// relaxation needs of the prior rows (members or perturbations) -- RTPS their spread, RTPP the rows themselves, copied when the
// state phase writes over them -- and after it the relaxation, in place on the posterior rows
template <class Core>
int with_relaxation(efa_ctx* c, const StatePlan& p, const StateRows& r, long* nl, Core&& core) {
  if (p.relax != Relax::standalone) return core();
  const bool rtpp = c->relax_kind == EFA_RELAX_RTPP;
  const double* prior = nullptr;
  if (!rtpp) {
    EFA_TRY(c->relax_ss.reserve((size_t)r.rows * sizeof(double)));
    EFA_HIP(launch_row_spread(r.rows, r.M, r.in(), c->relax_ss.as<double>(), c->stream));
    ++*nl;
  } else if (r.disjoint()) {
    prior = r.in();
  } else {
    EFA_TRY(c->relax_prior.reserve(r.bytes()));
    EFA_HIP(hipMemcpyAsync(c->relax_prior.p, r.prior, r.bytes(), hipMemcpyDeviceToDevice, c->stream));
    prior = c->relax_prior.as<double>();
  }
  EFA_TRY(core());
  EFA_HIP(launch_relax_rows(r.rows, r.M, rtpp ? 1 : 0, c->relax_alpha, r.out(), c->relax_ss.as<double>(), prior, c->stream));
  ++*nl;
  return EFA_OK;
}
}  // namespace

// ---- adaptive inflation (efa_adapt.hip, the update fused into the one-pass GC sweep) ----------------------------------------
// While a field is set, only the one-pass GC state sweep may run the state phase: it is the one that updates the field.
int check_adaptive(const efa_ctx* c, int loc_mode, long rows) {
  if (!c->ai_field) return EFA_OK;
  if (loc_mode != EFA_LOC_GC)
    return fail(EFA_ERR_INVALID, "adaptive inflation is set: it needs GC localisation (loc_mode %d is not EFA_LOC_GC)", loc_mode);
  if (!c->gc_onepass) return fail(EFA_ERR_INVALID, "adaptive inflation is set: it needs the one-pass GC sweep (option gc_onepass is 0)");
  if (rows != c->ai_rows)
    return fail(EFA_ERR_INVALID, "adaptive inflation field has %ld rows but the state phase has %ld", c->ai_rows, rows);
  return EFA_OK;
}

// ---- vertical localisation (efa_vloc.hip and the _vloc sweep kernels) -------------------------------------------------------
// While it is set, every call must be a GC cycle of the P obs and n_lead slabs it was set for, on the one-pass state sweep (the
// per-batch state sweep has no vertical factor) and without adaptive inflation (no combined kernel).  n_lead < 0: not checked.
int check_vloc(const efa_ctx* c, int loc_mode, long P, long n_lead) {
  if (!c->vl_on) return EFA_OK;
  if (loc_mode != EFA_LOC_GC)
    return fail(EFA_ERR_INVALID, "vertical localisation is set: it needs GC localisation (loc_mode %d is not EFA_LOC_GC)", loc_mode);
  if (!c->gc_onepass)
    return fail(EFA_ERR_INVALID, "vertical localisation is set: it needs the one-pass GC sweep (option gc_onepass is 0)");
  if (c->ai_field) return fail(EFA_ERR_INVALID, "vertical localisation is set: adaptive inflation cannot be combined with it");
  if (P != c->vl_P) return fail(EFA_ERR_INVALID, "vertical localisation was set for %ld observations, the call has %ld", c->vl_P, P);
  if (n_lead >= 0 && n_lead != c->vl_nlead)
    return fail(EFA_ERR_INVALID, "vertical localisation was set for %ld slabs, the call has n_lead=%ld", c->vl_nlead, n_lead);
  return EFA_OK;
}

// ---- temporal and cross-variable localisation (efa_slabloc.hip and the _slab sweep kernels) -------------------
// The same rules as check_vloc, for the same reasons: the factors live in the obs-obs table and in the one-pass sweep only.
int check_slab(const efa_ctx* c, int loc_mode, long P, long n_lead) {
  if (!c->sl_on) return EFA_OK;
  if (loc_mode != EFA_LOC_GC)
    return fail(EFA_ERR_INVALID, "slab localisation is set: it needs GC localisation (loc_mode %d is not EFA_LOC_GC)", loc_mode);
  if (!c->gc_onepass) return fail(EFA_ERR_INVALID, "slab localisation is set: it needs the one-pass GC sweep (option gc_onepass is 0)");
  if (c->ai_field) return fail(EFA_ERR_INVALID, "slab localisation is set: adaptive inflation cannot be combined with it");
  if (P != c->sl_P) return fail(EFA_ERR_INVALID, "slab localisation was set for %ld observations, the call has %ld", c->sl_P, P);
  if (n_lead >= 0 && n_lead != c->sl_nlead)
    return fail(EFA_ERR_INVALID, "slab localisation was set for %ld slabs, the call has n_lead=%ld", c->sl_nlead, n_lead);
  return EFA_OK;
}

// ---- sampling error correction (the kGcSec sweep kernels and k_sweep_sec) -----------------------------------
// The factor depends on the row's current correlation: only the kernels that hold a row while they walk its obs in order apply it.
int check_sec(const efa_ctx* c, int loc_mode) {
  if (!sec_active(c)) return EFA_OK;
  if (loc_mode != EFA_LOC_GC)
    return fail(EFA_ERR_INVALID, "sampling error correction is set: it needs GC localisation (loc_mode %d is not EFA_LOC_GC)", loc_mode);
  if (!c->gc_onepass)
    return fail(EFA_ERR_INVALID, "sampling error correction is set: it needs the one-pass GC sweep (option gc_onepass is 0)");
  if (c->ai_field) return fail(EFA_ERR_INVALID, "sampling error correction is set: adaptive inflation cannot be combined with it");
  if (c->vl_on) return fail(EFA_ERR_INVALID, "sampling error correction is set: vertical localisation cannot be combined with it");
  if (c->sl_on) return fail(EFA_ERR_INVALID, "sampling error correction is set: slab localisation cannot be combined with it");
  return EFA_OK;
}

// ---- the batch observation-space solver (option "obs_solver" 1, efa_etkf.hip) --------------------------------
// It solves all obs at once in ensemble space, which has no localised form here, leaves no records for a sweep, and no serial
// order for the inflation update to follow.
int check_batch_solver(const efa_ctx* c, int loc_mode) {
  if (!c->obs_solver) return EFA_OK;
  if (loc_mode == EFA_LOC_GC)
    return fail(EFA_ERR_INVALID, "option obs_solver is 1: the batch solver is unlocalised (a localised ETKF is out of scope)");
  if (c->ai_field) return fail(EFA_ERR_INVALID, "option obs_solver is 1: adaptive inflation cannot be combined with the batch solver");
  if (c->path == EFA_PATH_SWEEP)
    return fail(EFA_ERR_INVALID, "option obs_solver is 1: the batch solver leaves a transform and no records (option path is sweep)");
  return EFA_OK;
}

// The table depends on the two settings alone (not on the obs' positions): it is written once per change of either, on the
// context's stream, in front of the sweep that reads it.
// Without the slab setting (the LETKF under the vertical setting alone) the table is sized by the vertical setting
// and holds its factor alone; the slab setting's serial moves whenever it is turned on or off, so the cache tells the two apart.
int ensure_slab_table(efa_ctx* c) {
  const bool slab = c->sl_on;
  const long P = slab ? c->sl_P : c->vl_P, n_lead = slab ? c->sl_nlead : c->vl_nlead;
  EFA_TRY(c->sl_tab.reserve((size_t)(P * n_lead ? P * n_lead : 1) * sizeof(double)));
  if (c->sl_tab_serial == c->sl_serial && c->sl_tab_vl_serial == c->vl_serial && c->sl_tab_ptr == c->sl_tab.p) return EFA_OK;
  const bool vert = vl_active(c);  // (check_vloc: set for the same P and n_lead)
  EFA_HIP(launch_slab_factor(P, n_lead, vert ? vl_lead(c) : nullptr, vert ? vl_obvert(c) : nullptr, vert ? vl_obvhw(c) : nullptr,
                             slab ? sl_lead_time(c) : nullptr, slab ? sl_lead_var(c) : nullptr, slab ? sl_obs(c, 0) : efa::SlabObs{},
                             c->sl_tab.as<double>(), c->stream));
  c->sl_tab_serial = c->sl_serial;
  c->sl_tab_vl_serial = c->vl_serial;
  c->sl_tab_ptr = c->sl_tab.p;
  return EFA_OK;
}

// path "auto": one transform pass or sweep passes?  By FLOPS one transform pass is M/2 observations of sweep arithmetic (the rule of
// rounds 1-2), but the transform runs on the matrix cores at 49 TFLOP/s and the sweep on the vector ALUs at 10-20, and in MEMBER form
// (prior members in, posterior members out) the sweep path is three passes over the state -- form the perturbations, sweep, rebuild
// the members -- where the transform is one.  Measured at 1e7 x 100 (profiles/r03_auto_path.txt): member form 8 obs 10.6 ms by
// sweeps, 4.1 by the transform (48 obs: 16.9 vs 4.1); perturbation form 8 / 16 obs per sweep launch 3.4 / 4.5 ms vs 4.5.
// Above 136 members the transform re-reads the state once per group of 64 output columns: the flops rule stays.
static bool auto_transform(int M, long n_active, bool member_form) {
  if (n_active <= 0) return false;
  if (M > 136) return n_active > M / 2;
  if (member_form) return true;
  return n_active > M / 8;
}
// Do float32 kernels serve the cycle (route and relaxation decided)?  The transform does, but for the standalone relaxation
// passes; the one-pass GC sweep where its row-per-lane kernel applies and nothing is relaxed.
static bool f32_kernels_serve(const efa_ctx* c, const StatePlan& p) {
  if (p.route == Route::transform) return p.relax != Relax::standalone;
  return p.route == Route::gc_onepass && p.relax == Relax::none && sweep_gc_serves(Elem::f32, c->M, c->ye_stride, c->ye_ptr);
}

// ---- the plan of a state phase (StatePlan, efa_driver.h) ----------------------------------------------------------------------
// Every decision of a state call, from the settings and what the obs phase left; nothing is launched or written here.
StatePlan plan_state(const efa_ctx* c, bool member_form, Elem elem, bool in_place, bool have_transform) {
  StatePlan p;
  p.member_form = member_form;
  const bool any = c->P > 0 && c->n_active > 0;  // an ob was assimilated
  const bool wide = c->M > 136;                  // the transform runs as column groups (k_transform_wide)
  if (any && have_transform &&  // (behind the batch solver there are no records for any other route)
      (c->batch_solved || c->path == EFA_PATH_TRANSFORM || (c->path == EFA_PATH_AUTO && auto_transform(c->M, c->n_active, member_form))))
    p.route = Route::transform;
  else if (c->loc_mode == EFA_LOC_GC && c->gc_onepass && c->n_active > 0)  // every ensemble size the library accepts (2..256)
    p.route = Route::gc_onepass;
  if (c->relax_kind != EFA_RELAX_NONE && c->relax_alpha != 0.0 && any) {
    if (p.route != Route::transform) p.relax = Relax::standalone;
    else if (c->relax_kind == EFA_RELAX_RTPP) p.relax = Relax::folded;
    else p.relax = (member_form && transform_rtps_supported(c->M)) ? Relax::fused : Relax::standalone;
  }
  if (elem == Elem::f32 && !f32_kernels_serve(c, p)) p.ws_copies = (p.route == Route::transform && wide) ? 2 : 1;
  // in place the column groups would re-read rows that other groups have written: they read a copy of the prior;
  // either element type, either form (the workspace never runs that transform in place)
  p.copy_prior = p.ws_copies == 0 && p.route == Route::transform && wide && in_place;
  return p;
}

// ---- the column grid of a localised state phase (ColumnGrid, efa_ctx.h) -------------------------------------------------------
int check_grid(int loc_mode, const double* grid_lat, const double* grid_lon, long ncol, long n_lead, long rows) {
  if (loc_mode != EFA_LOC_GC) return EFA_OK;
  if (!grid_lat || !grid_lon) return fail(EFA_ERR_INVALID, "GC localisation needs grid_lat/grid_lon");
  if (ncol <= 0 || n_lead <= 0 || ncol * n_lead != rows)
    return fail(EFA_ERR_INVALID, "rows=%ld must equal n_lead*ncol = %ld*%ld", rows, n_lead, ncol);
  return EFA_OK;
}

int ColumnGrid::reserve(long ncol) {
  EFA_TRY(lat.reserve((size_t)ncol * sizeof(double)));
  EFA_TRY(lon.reserve((size_t)ncol * sizeof(double)));
  return EFA_OK;
}

int ColumnGrid::upload(hipStream_t s, const double* grid_lat, const double* grid_lon, long ncol) {
  const size_t nb = (size_t)ncol * sizeof(double);
  EFA_TRY(reserve(ncol));
  EFA_HIP(hipMemcpyAsync(lat.p, grid_lat, nb, hipMemcpyHostToDevice, s));
  EFA_HIP(hipMemcpyAsync(lon.p, grid_lon, nb, hipMemcpyHostToDevice, s));
  mirror_ncol = -1;
  serial++;
  EFA_HIP(hipStreamSynchronize(s));  // caller may reuse grid_lat/grid_lon on return
  return EFA_OK;
}

// Cycle after cycle on one grid nothing is copied; the comparison (4 MB at configs[3]) is host time spent while the device still
// works on the previous cycle.
int ColumnGrid::refresh(hipStream_t s, const double* grid_lat, const double* grid_lon, long ncol) {
  const size_t nb = (size_t)ncol * sizeof(double);
  const void* pin_before = mirror.p;
  EFA_TRY(mirror.reserve(2 * nb));
  char* pin = static_cast<char*>(mirror.p);
  const void *dl = lat.p, *dn = lon.p;
  EFA_TRY(reserve(ncol));
  const bool same = mirror_ncol == ncol && pin_before == mirror.p && dl == lat.p && dn == lon.p &&
                    std::memcmp(pin, grid_lat, nb) == 0 && std::memcmp(pin + nb, grid_lon, nb) == 0;
  if (!same) {
    EFA_HIP(hipStreamSynchronize(s));  // (an earlier copy out of the mirror may be in flight; a new grid is the rare case)
    std::memcpy(pin, grid_lat, nb);
    std::memcpy(pin + nb, grid_lon, nb);
    EFA_HIP(hipMemcpyAsync(lat.p, pin, nb, hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemcpyAsync(lon.p, pin + nb, nb, hipMemcpyHostToDevice, s));
    mirror_ncol = ncol;
    serial++;
  }
  return EFA_OK;
}

// (the one-pass sweep's lists are rebuilt: the grid changed)
int ColumnGrid::take_slice(hipStream_t s, const double* dev_grid, long pitch, long lo, long ncol) {
  EFA_HIP(hipMemcpyAsync(lat.p, dev_grid + lo, (size_t)ncol * sizeof(double), hipMemcpyDeviceToDevice, s));
  EFA_HIP(hipMemcpyAsync(lon.p, dev_grid + pitch + lo, (size_t)ncol * sizeof(double), hipMemcpyDeviceToDevice, s));
  mirror_ncol = -1;
  serial++;
  return EFA_OK;
}

int read_gc_pairs(efa_ctx* c) {
  if (!c->gc_pairs_pending) return EFA_OK;
  c->gc_pairs_pending = false;
  unsigned long long h_pairs = 0;
  EFA_HIP(hipMemcpyAsync(&h_pairs, c->gc_pairs.p, sizeof(h_pairs), hipMemcpyDeviceToHost, c->stream));
  EFA_HIP(hipStreamSynchronize(c->stream));
  c->gc_active_pairs = (long)h_pairs;
  return EFA_OK;
}

namespace {
// ---- Phase B, localised, one pass (efa_gcsweep.hip) --------------------------------------
// r: perturbation rows with their means xm_in / xm_out, or member rows (fused_members) of either element type
int state_gc_onepass(efa_ctx* c, const StateRows& r, const double* xm_in, double* xm_out, long ncol, long n_lead, int fused_members,
                     long* nl) {
  const int M = c->M;
  const long P = c->P;
  hipStream_t s = c->stream;
  const long nblk = gc_num_blocks(ncol);
  EFA_TRY(c->gc_cnt.reserve((size_t)nblk * sizeof(int)));
  EFA_TRY(c->gc_ub.reserve((size_t)nblk * sizeof(int)));
  EFA_TRY(c->gc_order.reserve((size_t)nblk * sizeof(int)));
  EFA_TRY(c->gc_obtrig.reserve((size_t)P * 6 * sizeof(double)));
  EFA_TRY(c->gc_off.reserve((size_t)(nblk + 1) * sizeof(long)));
  EFA_TRY(c->gc_pairs.reserve(sizeof(unsigned long long)));
  const void* ptrs[5] = {c->gc_off.p, c->gc_cnt.p, c->gc_order.p, c->gc_idx.p, c->gc_wts.p};
  const bool lists_ok = c->geometry_reuse && c->gc_list_valid && c->gc_list_geo == c->geo_serial && c->gc_list_grid == c->grid.serial &&
                        c->gc_list_ncol == ncol && c->gc_list_P == P && std::memcmp(ptrs, c->gc_list_ptrs, sizeof(ptrs)) == 0;
  if (!lists_ok) {
  c->gc_list_valid = false;
  EFA_TRY(read_gc_pairs(c));  // (the previous sweep's count, before the counter is cleared: that sweep is long done)
  EFA_HIP(hipMemsetAsync(c->gc_pairs.p, 0, sizeof(unsigned long long), s));
  // the lists hold the obs the CALLER asked to assimilate, as the geometry they are cached by: an ob the outlier check rejected
  // stays in them with its inactive record (zero gains), so a later cycle that keeps it finds it there
  const double* act = c->qc_used ? c->qc_act.as<double>() : c->coef.as<double>();
  EFA_HIP(launch_gc_bound(ncol, P, c->grid.lat.as<double>(), c->ob_lat, c->ob_hw, act, c->gc_ub.as<int>(), c->gc_off.as<long>(), s));
  long cap = 0;  // the only host round trip of the build: 8 bytes, the capacity the lists need
  EFA_HIP(hipMemcpyAsync(&cap, c->gc_off.as<long>() + nblk, sizeof(long), hipMemcpyDeviceToHost, s));
  EFA_HIP(hipStreamSynchronize(s));
  EFA_TRY(c->gc_idx.reserve((size_t)(cap ? cap : 1) * sizeof(int)));
  EFA_TRY(c->gc_wts.reserve((size_t)(cap ? cap : 1) * 16 * sizeof(double)));
  EFA_HIP(launch_gc_fill(ncol, P, c->grid.lat.as<double>(), c->grid.lon.as<double>(), c->ob_lat, c->ob_lon, c->ob_hw, act,
                         c->gc_obtrig.as<double>(), c->gc_off.as<long>(), c->gc_cnt.as<int>(), c->gc_idx.as<int>(),
                         c->gc_wts.as<double>(), c->gc_order.as<int>(), c->gc_pairs.as<unsigned long long>(), s));
  c->gc_list_valid = true;
  c->gc_list_geo = c->geo_serial;
  c->gc_list_grid = c->grid.serial;
  c->gc_list_ncol = ncol;
  c->gc_list_P = P;
  c->gc_list_ptrs[0] = c->gc_off.p;
  c->gc_list_ptrs[1] = c->gc_cnt.p;
  c->gc_list_ptrs[2] = c->gc_order.p;
  c->gc_list_ptrs[3] = c->gc_idx.p;
  c->gc_list_ptrs[4] = c->gc_wts.p;
  c->gc_pairs_pending = true;  // read by read_gc_pairs when somebody asks (option "gc_active_pairs") or before the next build
  }
  GcSweepArgs g{};
  g.ncol = ncol;
  g.n_lead = n_lead;
  g.M = M;
  g.nblk = nblk;
  g.off = c->gc_off.as<long>();
  g.cnt = c->gc_cnt.as<int>();
  g.order = c->gc_order.as<int>();
  g.idx = c->gc_idx.as<int>();
  g.wts = c->gc_wts.as<double>();
  g.coef = c->coef.as<double>();
  g.Ye = c->ye_ptr;
  g.ye_stride = c->ye_stride;
  g.Xin = r.in();
  g.xin = xm_in;
  g.Xout = r.out();
  g.xout = xm_out;
  g.fused_members = fused_members;
  if (c->ai_field) {  // the per-ob scalars of the inflation update, from Phase A's records and diagnostics
    EFA_TRY(c->ai_ob.reserve((size_t)(P ? P : 1) * 4 * sizeof(double)));
    EFA_HIP(launch_adapt_obs(P, M, c->coef.as<double>(), c->d_prior_var, c->ob_err, c->ye_ptr, c->ye_stride,
                             c->ai_ob.as<double>(), s));
    ++*nl;
    g.infl = c->ai_field;
    g.adapt_ob = c->ai_ob.as<double>();
    g.infl_lower = c->ai_lower;
    g.infl_upper = c->ai_upper;
    g.infl_sd_lower = c->ai_sd_lower;
  }
  if (vl_active(c)) {
    g.lead_vert = vl_lead(c);
    g.ob_vert = vl_obvert(c);
    g.ob_vhw = vl_obvhw(c);
  }
  if (sl_active(c)) {  // the slab table carries the vertical factor too: its family serves the call
    EFA_TRY(ensure_slab_table(c));
    g.slab_tab = c->sl_tab.as<double>();
  }
  if (sec_active(c)) {  // y'.y' of every ob, in the record of the inflation update (check_sec: that one is off)
    EFA_TRY(c->sec_ob.reserve((size_t)(P ? P : 1) * 4 * sizeof(double)));
    EFA_HIP(launch_adapt_obs(P, M, c->coef.as<double>(), c->d_prior_var, c->ob_err, c->ye_ptr, c->ye_stride, c->sec_ob.as<double>(), s));
    ++*nl;
    g.adapt_ob = c->sec_ob.as<double>();
    g.sec_tab = c->sec_dev.as<double>();
    g.sec_T = c->sec_T;
  }
  c->gc_family_used = g.infl ? 1 : g.sec_tab ? 4 : g.slab_tab ? 3 : g.lead_vert ? 2 : 0;
  c->gc_form_used = sweep_gc_form(g, r.elem);
  EFA_HIP(launch_sweep_gc(g, r.elem, s));
  ++*nl;
  return EFA_OK;
}

// ---- Phase B per batch of obs (perturbation form, float64) ------------------------------------------
int state_sweeps(efa_ctx* c, long rows, const double* xm_in, const double* Xp_in, double* xm_out, double* Xp_out, long ncol,
                 long* nl) {
  const int M = c->M;
  const long P = c->P;
  hipStream_t s = c->stream;
  const long B = effective_batch(c, M);
  bool first = true;
  for (long b0 = 0; b0 < P; b0 += B) {
    const int nb = (int)((P - b0 < B) ? (P - b0) : B);
    long act = 0;
    for (int k = 0; k < nb; ++k) act += c->h_assim[b0 + k] ? 1 : 0;
    if (act == 0) continue;
    SweepArgs a{};
    a.Xin = first ? Xp_in : Xp_out;
    a.xin = first ? xm_in : xm_out;
    a.Xout = Xp_out;
    a.xout = xm_out;
    a.nrows = rows;
    a.M = M;
    a.Ye = c->ye_ptr + (size_t)b0 * c->ye_stride;
    a.ye_stride = c->ye_stride;
    a.coef = c->coef.as<double>() + (size_t)b0 * kCoefStride;
    a.nb = nb;
    a.skip_lo = a.skip_hi = -1;
    if (c->loc_mode == EFA_LOC_GC) {
      EFA_TRY(c->W.reserve((size_t)B * ncol * sizeof(double)));
      EFA_HIP(launch_taper_table(ncol, nb, c->grid.lat.as<double>(), c->grid.lon.as<double>(), c->ob_lat + b0, c->ob_lon + b0, c->ob_hw + b0,
                                 c->W.as<double>(), s));
      a.taper_mode = kTaperTable;
      a.W = c->W.as<double>();
      a.ncol = ncol;
    } else {
      a.taper_mode = kTaperNone;
    }
    EFA_HIP(launch_sweep(a, s));
    ++*nl;
    first = false;
  }
  if (first && Xp_out != Xp_in) {  // nothing assimilated: posterior == prior
    EFA_HIP(hipMemcpyAsync(Xp_out, Xp_in, (size_t)rows * M * sizeof(double), hipMemcpyDeviceToDevice, s));
    EFA_HIP(hipMemcpyAsync(xm_out, xm_in, (size_t)rows * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  return EFA_OK;
}

}  // namespace

// ---- the executor: the launches of a plan ---------------------------------------------------------------------------------------
// xm_in / xm_out: the means of the perturbation form (null in member form).  *launches: the state-phase launches it issued.
int run_state_plan(efa_ctx* c, const StatePlan& p, const StateRows& r, const double* xm_in, double* xm_out, long ncol, long n_lead,
                   long* launches) {
  hipStream_t s = c->stream;
  long& nl = *launches;
  nl = 0;
  if (p.ws_copies) {  // float32 rows without a float32 kernel: widened, the same plan on the float64 workspace, rounded once
    const size_t n = r.count();
    EFA_TRY(c->f32_ws.reserve((size_t)p.ws_copies * n * sizeof(double)));
    double* ws = c->f32_ws.as<double>();
    const StateRows w{ws, p.ws_copies == 2 ? ws + n : ws, Elem::f64, r.rows, r.M};
    StatePlan q = p;
    q.ws_copies = 0;
    EFA_HIP(launch_widen_f32(n, static_cast<const float*>(r.prior), ws, s));
    EFA_TRY(run_state_plan(c, q, w, xm_in, xm_out, ncol, n_lead, launches));
    EFA_HIP(launch_narrow_f32(n, w.out(), static_cast<float*>(r.post), s));
    nl += 2;
    return EFA_OK;
  }
  if (p.route == Route::transform) {
    // through [T | w]; RTPP folded into T: Xb' ((1-alpha) T + alpha I), xam as without it
    StateRows in = r;
    if (p.copy_prior) {
      EFA_TRY(c->wide_prior.reserve(r.bytes()));
      EFA_HIP(hipMemcpyAsync(c->wide_prior.p, r.prior, r.bytes(), hipMemcpyDeviceToDevice, s));
      in.prior = c->wide_prior.p;
    }
    // [T | w] as Phase A left them: the carried identity rows behind the P obs rows of the working block
    TransformArgs t{in.in(), xm_in, in.out(), xm_out, in.rows, c->M, c->Yw.as<double>() + (size_t)c->P * c->M,
                    c->ymw.as<double>() + c->P, p.member_form ? 1 : 0};
    if (p.relax == Relax::fused) {
      EFA_HIP(launch_transform_rtps(t, c->relax_alpha, r.elem, s));
      ++nl;
    } else {
      if (p.relax == Relax::folded) {
        EFA_TRY(c->relax_T.reserve((size_t)t.M * t.M * sizeof(double)));
        EFA_HIP(launch_relax_fold(t.M, c->relax_alpha, t.T, c->relax_T.as<double>(), s));
        t.T = c->relax_T.as<double>();
        ++nl;
      }
      EFA_TRY(with_relaxation(c, p, r, &nl, [&]() -> int {  // (r: with the standalone passes no copy of the prior stands in)
        EFA_HIP(launch_transform(t, r.elem, s));
        ++nl;
        return EFA_OK;
      }));
    }
  } else {
    EFA_TRY(with_relaxation(c, p, r, &nl, [&]() -> int {
      if (p.route == Route::gc_onepass)  // localised: prior -> posterior in one read + one write of the state
        return state_gc_onepass(c, r, xm_in, xm_out, ncol, n_lead, p.member_form ? 1 : 0, &nl);
      if (!p.member_form) return state_sweeps(c, r.rows, xm_in, r.in(), xm_out, r.out(), ncol, &nl);
      // member form: form the perturbations in the posterior rows, sweep them in place, rebuild the members
      EFA_TRY(c->xm_ws.reserve((size_t)r.rows * sizeof(double)));
      double* xm = c->xm_ws.as<double>();
      EFA_HIP(launch_form_perts(r.rows, r.M, r.in(), 1.0, xm, r.out(), s));
      EFA_TRY(state_sweeps(c, r.rows, xm, r.out(), xm, r.out(), ncol, &nl));
      EFA_HIP(launch_posterior(r.rows, r.M, xm, r.out(), r.out(), s));
      return EFA_OK;
    }));
  }
  return EFA_OK;
}

// what a state call reports (efa_last_timing, option "f32_native"), from its plan and the launches it took
void report_state_call(efa_ctx* c, const StatePlan& p, Elem elem, long launches) {
  c->state_launches = launches;
  c->path_taken = p.route == Route::transform ? EFA_PATH_TRANSFORM : EFA_PATH_SWEEP;
  if (elem == Elem::f32) c->f32_native = p.ws_copies == 0 ? 1 : 0;
}

namespace {
// ---- the state calls ------------------------------------------------------------------------------------------------------------
// What both forms do before their first launch: the checks, the counters, and -- once there is work to do (rows > 0) -- the grid of
// a localised call on the device and the begin of the state interval.  ptrs_ok: no state pointer of the form is null; partial_overlap:
// an output range of the form overlaps its input range without coinciding with it.
int begin_state_call(efa_ctx* c, const char* who, long rows, int M, bool ptrs_ok, bool partial_overlap, const double* grid_lat,
                     const double* grid_lon, long ncol, long n_lead, const StateCall& o) {
  if (!c->have_traj) return fail(EFA_ERR_INVALID, "%s called before efa_obs_phase_dev", who);
  if (M != c->M) return fail(EFA_ERR_INVALID, "M=%d differs from the obs phase's M=%d", M, c->M);
  if (rows < 0) return fail(EFA_ERR_INVALID, "negative row count");
  EFA_TRY(check_adaptive(c, c->loc_mode, rows));
  EFA_TRY(check_vloc(c, c->loc_mode, c->P, n_lead));
  EFA_TRY(check_slab(c, c->loc_mode, c->P, n_lead));
  EFA_TRY(check_sec(c, c->loc_mode));
  harvest_state_ms(c);  // the arguments are checked: the previous interval is read, the counters cleared
  c->state_ms = 0.0;
  c->state_launches = 0;
  c->path_taken = EFA_PATH_SWEEP;
  if (rows == 0) return EFA_OK;
  if (!ptrs_ok) return fail(EFA_ERR_INVALID, "null state pointer");
  if (partial_overlap)
    return fail(EFA_ERR_INVALID, "%s: the posterior rows overlap the prior rows without coinciding with them (in place means the same address)", who);
  EFA_TRY(check_grid(c->loc_mode, grid_lat, grid_lon, ncol, n_lead, rows));
  if (c->loc_mode == EFA_LOC_GC && !o.grid_current) EFA_TRY(c->grid.upload(c->stream, grid_lat, grid_lon, ncol));
  if (c->timing && o.timed) EFA_HIP(hipEventRecord(c->state_iv[0].begin, c->stream));
  return EFA_OK;
}

// ... and after it: plan, launches, report
int plan_and_run(efa_ctx* c, bool member_form, const StateRows& r, const double* xm_in, double* xm_out, long ncol, long n_lead,
                 const StateCall& o) {
  const StatePlan plan = plan_state(c, member_form, r.elem, r.in_place(), c->have_transform);
  long launches = 0;
  EFA_TRY(run_state_plan(c, plan, r, xm_in, xm_out, ncol, n_lead, &launches));
  report_state_call(c, plan, r.elem, launches);
  return end_state_call(c, c->state_iv[0], o.timed);
}

}  // namespace

int end_state_call(efa_ctx* c, Interval& iv, bool timed, bool end_recorded) {
  c->state_launches_sum += c->state_launches;
  if (!c->timing || !timed) return EFA_OK;
  if (!end_recorded) EFA_HIP(hipEventRecord(iv.end, c->stream));
  iv.pending = true;
  if (c->timing == 1) harvest_state_ms(c);
  return EFA_OK;
}

// perturbation form (efa_state_phase_dev)
int state_phase(efa_ctx* c, long rows, int M, const double* xm_in, const double* Xp_in, double* xm_out, double* Xp_out,
                const double* grid_lat, const double* grid_lon, long ncol, long n_lead, const StateCall& o) {
  const StateRows r{Xp_in, Xp_out, Elem::f64, rows, M}, means{xm_in, xm_out, Elem::f64, rows, 1};
  EFA_TRY(begin_state_call(c, "efa_state_phase_dev", rows, M, xm_in && Xp_in && xm_out && Xp_out,
                           r.partial_overlap() || means.partial_overlap(), grid_lat, grid_lon, ncol, n_lead, o));
  if (rows == 0) return EFA_OK;
  return plan_and_run(c, false, r, xm_in, xm_out, ncol, n_lead, o);
}

// member form (efa_state_cycle_dev, efa_state_cycle_f32_dev).  On a state stored as float32 posterior =
// fl32(F(widen(prior))), F the float64 member form: by the float32 kernels where the plan finds them, else through the workspace.
int state_cycle(efa_ctx* c, const StateRows& r, const double* grid_lat, const double* grid_lon, long ncol, long n_lead,
                const StateCall& o) {
  const bool f32 = r.elem == Elem::f32;
  if (f32 && c->ai_field)
    return fail(EFA_ERR_INVALID, "efa_state_cycle_f32_dev: an adaptive-inflation field is set (its update is float64 only)");
  if (f32 && ((reinterpret_cast<uintptr_t>(r.prior) | reinterpret_cast<uintptr_t>(r.post)) & 3u) != 0)
    return fail(EFA_ERR_INVALID, "efa_state_cycle_f32_dev: state pointers must be 4-byte aligned");
  EFA_TRY(begin_state_call(c, f32 ? "efa_state_cycle_f32_dev" : "efa_state_cycle_dev", r.rows, r.M, r.prior && r.post,
                           r.partial_overlap(), grid_lat, grid_lon, ncol, n_lead, o));
  if (r.rows == 0) return EFA_OK;
  return plan_and_run(c, true, r, nullptr, nullptr, ncol, n_lead, o);
}

}  // namespace efa_host
