// C-ABI layer of libefa_hip.so (see include/efa_hip.h): contexts, workspaces,
// the Phase A / Phase B drivers and the host-memory convenience entry point.
#include "efa_ctx.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and enums only: librccl is opened with dlopen when a communicator is asked for

#include <dlfcn.h>

#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "efa_internal.h"

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace efa_host {
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}
}  // namespace efa_host

namespace {

using namespace efa;

// "timing" 2 (deferred): no phase call waits for its own events -- the host may run ahead of the device from one cycle into the
// next.  An interval is read when its events are about to be recorded again (the calls in between have synchronised the stream
// since: the wait returns at once) or in efa_last_timing, and added to running sums.
void harvest_obs_ms(efa_ctx* c) {
  if (!c->obs_ms_pending) return;
  float ms = 0.f;
  if (hipEventSynchronize(c->ev[c->obs_end_ev]) == hipSuccess && hipEventElapsedTime(&ms, c->ev[0], c->ev[c->obs_end_ev]) == hipSuccess) {
    c->obs_ms = ms;
    c->obs_ms_sum += ms;
  } else {
    (void)hipGetLastError();
  }
  c->obs_ms_pending = false;
}
void harvest_state_pair(efa_ctx* c, int pair) {
  bool& pending = pair ? c->state_ms_pending2 : c->state_ms_pending;
  if (!pending) return;
  float ms = 0.f;
  if (hipEventSynchronize(c->ev[3 + 2 * pair]) == hipSuccess &&
      hipEventElapsedTime(&ms, c->ev[2 + 2 * pair], c->ev[3 + 2 * pair]) == hipSuccess) {
    c->state_ms = ms;
    c->state_ms_sum += ms;
  } else {
    (void)hipGetLastError();
  }
  pending = false;
}
void harvest_state_ms(efa_ctx* c) {
  harvest_state_pair(c, 0);
  harvest_state_pair(c, 1);
}
// end of a state-phase call: timing 1 waits and reads, timing 2 leaves the interval pending
int finish_state_timing(efa_ctx* c, hipStream_t s) {
  c->state_launches_sum += c->state_launches;
  if (!c->timing) return EFA_OK;
  EFA_HIP(hipEventRecord(c->ev[3], s));
  c->state_ms_pending = true;
  if (c->timing == 1) harvest_state_ms(c);
  return EFA_OK;
}

// start of a state-phase call, once its arguments are checked: the previous interval is read, the counters cleared
void reset_state_phase(efa_ctx* c) {
  harvest_state_ms(c);
  c->state_ms = 0.0;
  c->state_launches = 0;
  c->path_taken = EFA_PATH_SWEEP;
}

int use(efa_ctx* c) {
  if (!c) return fail(EFA_ERR_INVALID, "null context");
  EFA_HIP(hipSetDevice(c->device));
  return EFA_OK;
}

long effective_batch(const efa_ctx* c, int M) {
  long b = c->obs_batch;
  if (b < 1) b = 1;
  if (b > kMaxBatch) b = kMaxBatch;
  // LDS budgets: the sweep's image of the batch (ye rows + coefs, either lane layout) and the
  // diag kernel's ring (ye rows + scalars + the GC taper matrix) must fit one CU's 160 KiB.
  const long s4 = sweep_slots(M), s16 = 32L * ((M + 31) / 32);
  const long per_ob = ((s4 > s16 ? s4 : s16) + kCoefStride) * (long)sizeof(double);
  while (b > 1 && (b * per_ob + 64L * kMaxBatch * 8 > 150L * 1024 || (long)diag_lds_bytes((int)s4, (int)b, 1) > 150L * 1024)) --b;
  return b;
}

int h2d(efa_ctx* c, DevBuf& b, const void* src, size_t bytes) {
  EFA_TRY(b.reserve(bytes ? bytes : 8));
  if (bytes) EFA_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
  return EFA_OK;
}

int check_common(int M, long P) {
  if (M < 2) return fail(EFA_ERR_INVALID, "ensemble size M=%d must be >= 2 (covariance divides by M-1)", M);
  if (M > kMaxMembers) return fail(EFA_ERR_UNSUPPORTED, "ensemble size M=%d exceeds the built maximum %d", M, kMaxMembers);
  if (P < 0) return fail(EFA_ERR_INVALID, "negative observation count");
  return EFA_OK;
}

bool auto_transform(int M, long n_active, bool member_form);  // (with Phase B's path choice, below)

// ---- posterior relaxation (RTPP / RTPS, efa_relax.hip) ----------------------------------------------------------
// Applied only where a state phase writes the caller's state rows, and only when an ob was assimilated (otherwise the posterior
// is returned exactly as without it).
bool relax_on(const efa_ctx* c) {
  return c->relax_kind != EFA_RELAX_NONE && c->relax_alpha != 0.0 && c->P > 0 && c->n_active > 0;
}
// standalone passes, before the state phase: what the relaxation needs of the prior rows Xin (members or perturbations) -- RTPS
// their spread, RTPP the rows themselves (copied when the state phase writes over them)
int relax_prepare(efa_ctx* c, long rows, int M, const double* Xin, const double* Xout, const double** prior, long* nl) {
  *prior = nullptr;
  if (c->relax_kind == EFA_RELAX_RTPS) {
    EFA_TRY(c->relax_ss.reserve((size_t)rows * sizeof(double)));
    EFA_HIP(launch_row_spread(rows, M, Xin, c->relax_ss.as<double>(), c->stream));
    ++*nl;
    return EFA_OK;
  }
  const size_t bytes = (size_t)rows * M * sizeof(double);
  const char *a = reinterpret_cast<const char*>(Xin), *b = reinterpret_cast<const char*>(Xout);
  if (a + bytes <= b || b + bytes <= a) {
    *prior = Xin;
  } else {
    EFA_TRY(c->relax_prior.reserve(bytes));
    EFA_HIP(hipMemcpyAsync(c->relax_prior.p, Xin, bytes, hipMemcpyDeviceToDevice, c->stream));
    *prior = c->relax_prior.as<double>();
  }
  return EFA_OK;
}
// ... and after it, in place on the posterior rows
int relax_apply(efa_ctx* c, long rows, int M, double* Xout, const double* prior, long* nl) {
  EFA_HIP(launch_relax_rows(rows, M, c->relax_kind == EFA_RELAX_RTPP ? 1 : 0, c->relax_alpha, Xout, c->relax_ss.as<double>(), prior,
                            c->stream));
  ++*nl;
  return EFA_OK;
}
// core(), the state phase's pass(es) from prior rows Xin to posterior rows Xout, between the standalone relaxation passes
template <class Core>
int with_relaxation(efa_ctx* c, long rows, int M, const double* Xin, double* Xout, long* nl, Core&& core) {
  const bool relax = relax_on(c);
  const double* prior = nullptr;
  if (relax) EFA_TRY(relax_prepare(c, rows, M, Xin, Xout, &prior, nl));
  EFA_TRY(core());
  if (relax) EFA_TRY(relax_apply(c, rows, M, Xout, prior, nl));
  return EFA_OK;
}
// The state transform through [T | w] (member or perturbation form, t.fused_members) with the relaxation: RTPP folded into T
// (Xb' ((1-alpha) T + alpha I); xam as without it), RTPS fused into the member-form transform up to 136 members, the standalone
// passes otherwise.  *nl = the launches it took.
int transform_with_relaxation(efa_ctx* c, TransformArgs t, long* nl) {
  hipStream_t s = c->stream;
  const bool relax = relax_on(c);
  *nl = 1;
  if (relax && c->relax_kind == EFA_RELAX_RTPP) {
    EFA_TRY(c->relax_T.reserve((size_t)t.M * t.M * sizeof(double)));
    EFA_HIP(launch_relax_fold(t.M, c->relax_alpha, t.T, c->relax_T.as<double>(), s));
    t.T = c->relax_T.as<double>();
    *nl = 2;
  } else if (relax && t.fused_members && transform_rtps_supported(t.M)) {
    EFA_HIP(launch_transform_rtps(t, c->relax_alpha, s));
    return EFA_OK;
  } else if (relax) {
    return with_relaxation(c, t.nrows, t.M, t.Xin, t.Xout, nl, [&]() -> int {
      EFA_HIP(launch_transform(t, s));
      return EFA_OK;
    });
  }
  EFA_HIP(launch_transform(t, s));
  return EFA_OK;
}
// [T | w] as Phase A left them: the carried identity rows behind the P obs rows of the working block
TransformArgs carried_transform(const efa_ctx* c, const double* Xin, const double* xin, double* Xout, double* xout, long rows,
                                int fused_members) {
  return TransformArgs{Xin, xin, Xout, xout, rows, c->M, c->Yw.as<double>() + (size_t)c->P * c->M, c->ymw.as<double>() + c->P,
                       fused_members};
}

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
bool vl_active(const efa_ctx* c) { return c->vl_on && c->vl_any; }
const double* vl_lead(const efa_ctx* c) { return c->vl_dev.as<double>(); }
const double* vl_obvert(const efa_ctx* c) { return c->vl_dev.as<double>() + c->vl_nlead; }
const double* vl_obvhw(const efa_ctx* c) { return c->vl_dev.as<double>() + c->vl_nlead + c->vl_P; }

// ---- Phase A ---------------------------------------------------------------
// One obs_phase call: its arguments and the workspace layout that the steps below share.
struct ObsCall {
  int M = 0, loc_mode = EFA_LOC_NONE;
  long P = 0;
  double *ym_dev = nullptr, *Yp_dev = nullptr;  // the caller's obs block
  const uint8_t* ob_assim = nullptr;            // host
  bool carry_T = false;  // M identity rows ride along behind the obs rows: Phase A leaves the transform [T | w] in them
  long extra = 0, R = 0;  // those rows (M or 0); rows of the working block, P + extra
  double *Yw = nullptr, *ymw = nullptr;  // the working block [R][M], [R]
  size_t oslot = 0;      // bytes of one diagnostics array in out_pack / pin_out
  size_t pack_bytes = 0; // of the input pack, which goes to the device inside the prep launch
  size_t islot = 0;      // bytes of one slot of that pack
  long B = 0;            // obs per pass of the per-batch kernels
  bool pipe_ok = false;  // the persistent kernels apply
  long Wmax = 0, nwin = 1;  // obs per window, windows
  long TS_std = 0, TS_band = 0, TS = 0;  // record strides of the two layouts, and the larger (the allocation's)
};
// The layout of the records Phase B reads.  All windows of a call leave ONE layout: Phase B reads them with one stride.
enum class Records { kNone /* dense ye rows in Ye_rec: the per-batch kernels */, kStandard /* k_pipe, k_pipe_gram */, kBand /* k_pipe_band */ };
long record_stride(const ObsCall& a, Records r) { return r == Records::kBand ? a.TS_band : a.TS_std; }

// Obs [w0, w1) and the rows their persistent launch works on: the block itself when one window covers it (direct), else a
// workspace [window rows | transform rows].
struct Window {
  long w, w0, w1, Pw, Rw;
  bool direct;
  double *Wy, *Wm;
};
Window make_window(const ObsCall& a, long w) {
  const long w0 = a.pipe_ok ? w * a.Wmax : 0, w1 = a.pipe_ok ? ((w0 + a.Wmax < a.P) ? w0 + a.Wmax : a.P) : a.P;
  return Window{w, w0, w1, w1 - w0, w1 - w0 + ((a.nwin == 1) ? a.extra : 2 * a.extra), a.nwin == 1, a.Yw, a.ymw};
}

// Argument and radius checks, the host copies of the assimilate flags and the geometry, the per-ob inputs in one pinned pack,
// the diagnostics pack and the workspaces.  ob_hw comes back sanitised.
int stage_obs_inputs(efa_ctx* c, ObsCall& a, const double* ob_value, const double* ob_error, const double* ob_lat,
                     const double* ob_lon, const double*& ob_hw) {
  const int M = a.M;
  const long P = a.P;
  const uint8_t* ob_assim = a.ob_assim;
  if (!a.ym_dev || !a.Yp_dev || !ob_value || !ob_error || !ob_assim)
    return fail(EFA_ERR_INVALID, "null observation array");
  if (a.loc_mode == EFA_LOC_GC) {
    if (!ob_lat || !ob_lon || !ob_hw) return fail(EFA_ERR_INVALID, "GC localisation needs ob_lat/ob_lon/ob_halfwidth_km");
    // the reference reads localize_radius only for obs it assimilates (ensrf.py:74-76 comes before :101):
    // an unassimilated ob may carry any radius; it is replaced by a harmless one before it goes to the device
    c->h_hw.assign(ob_hw, ob_hw + P);
    for (long k = 0; k < P; ++k) {
      if (!ob_assim[k]) {
        c->h_hw[k] = 1.0;
        continue;
      }
      if (!(ob_hw[k] == ob_hw[k]) || ob_hw[k] == 0.0)
        return fail(EFA_ERR_INVALID, "observation %ld: localize_radius must be a non-zero number for loc='GC' "
                    "(the reference raises in abs(None), observation.py:120)", k);
    }
    ob_hw = c->h_hw.data();
  }
  c->h_assim.assign(ob_assim, ob_assim + P);
  for (long k = 0; k < P; ++k) c->n_active += ob_assim[k] ? 1 : 0;
  if (a.loc_mode == EFA_LOC_GC) {
    const size_t nb8 = (size_t)P * sizeof(double);
    const bool same = (long)c->geo_lat.size() == P && std::memcmp(c->geo_lat.data(), ob_lat, nb8) == 0 &&
                      std::memcmp(c->geo_lon.data(), ob_lon, nb8) == 0 && std::memcmp(c->geo_hw.data(), ob_hw, nb8) == 0 &&
                      std::memcmp(c->geo_assim.data(), ob_assim, (size_t)P) == 0 && c->geo_vl_serial == c->vl_serial;
    if (!same) {
      c->geo_vl_serial = c->vl_serial;  // (the vertical setting is part of the geometry: the obs-obs table carries its factor)
      c->geo_lat.assign(ob_lat, ob_lat + P);
      c->geo_lon.assign(ob_lon, ob_lon + P);
      c->geo_hw.assign(ob_hw, ob_hw + P);     // (sanitised above)
      c->geo_assim.assign(ob_assim, ob_assim + P);
      c->geo_serial++;
    }
  }

  a.carry_T = (a.loc_mode == EFA_LOC_NONE) && transform_supported(M) && (c->path != EFA_PATH_SWEEP);
  a.extra = a.carry_T ? M : 0;
  a.R = P + a.extra;
  const size_t dP = (size_t)P * sizeof(double);

  // per-ob inputs: [value | error | assim bytes | {error, sqrt(error), assimilate (1.0 / 0.0), 0} x P | lat | lon | halfwidth] in one
  // allocation, ONE H2D from pinned memory (the last three slots only with localisation); the four-double records are the band
  // leader's per-ob constants, fetched with wave-uniform loads
  {
    const bool gc = a.loc_mode == EFA_LOC_GC;
    const size_t slot = ((size_t)P * sizeof(double) + 255) & ~(size_t)255;
    const size_t total = 10 * slot;
    EFA_TRY(c->ob_pack.reserve(total));
    EFA_TRY(c->pin_in.reserve(total));
    char* hb = static_cast<char*>(c->pin_in.p);
    char* db = static_cast<char*>(c->ob_pack.p);
    std::memcpy(hb, ob_value, dP);
    std::memcpy(hb + slot, ob_error, dP);
    std::memcpy(hb + 2 * slot, ob_assim, (size_t)P);
    {
      double* ec = reinterpret_cast<double*>(hb + 3 * slot);
      for (long k = 0; k < P; ++k) {
        ec[4 * k] = ob_error[k];
        ec[4 * k + 1] = std::sqrt(ob_error[k]);
        ec[4 * k + 2] = ob_assim[k] ? 1.0 : 0.0;
        ec[4 * k + 3] = 0.0;
      }
    }
    if (gc) {
      std::memcpy(hb + 7 * slot, ob_lat, dP);
      std::memcpy(hb + 8 * slot, ob_lon, dP);
      std::memcpy(hb + 9 * slot, ob_hw, dP);
    }
    c->ob_val = reinterpret_cast<double*>(db);
    c->ob_err = reinterpret_cast<double*>(db + slot);
    c->ob_asm = reinterpret_cast<uint8_t*>(db + 2 * slot);
    c->ob_errsq = reinterpret_cast<double*>(db + 3 * slot);
    c->ob_lat = reinterpret_cast<double*>(db + 7 * slot);
    c->ob_lon = reinterpret_cast<double*>(db + 8 * slot);
    c->ob_hw = reinterpret_cast<double*>(db + 9 * slot);
    a.pack_bytes = gc ? total : 7 * slot;  // goes to the device inside the prep launch (read from the mapped pinned buffer)
    a.islot = slot;
  }
  EFA_TRY(c->Ye_rec.reserve((size_t)P * M * sizeof(double)));
  EFA_TRY(c->coef.reserve((size_t)P * kCoefStride * sizeof(double)));
  // per-ob diagnostics: [prior_mean | prior_var | post_mean | post_var | assimilated bytes], one D2H at the end
  a.oslot = ((size_t)P * sizeof(double) + 255) & ~(size_t)255;
  {
    EFA_TRY(c->out_pack.reserve(5 * a.oslot));
    EFA_TRY(c->pin_out.reserve(5 * a.oslot));
    char* db = static_cast<char*>(c->out_pack.p);
    c->d_prior_mean = reinterpret_cast<double*>(db);
    c->d_prior_var = reinterpret_cast<double*>(db + a.oslot);
    c->d_post_mean = reinterpret_cast<double*>(db + 2 * a.oslot);
    c->d_post_var = reinterpret_cast<double*>(db + 3 * a.oslot);
    c->d_assimilated = reinterpret_cast<uint8_t*>(db + 4 * a.oslot);
  }
  EFA_TRY(c->Yw.reserve((size_t)a.R * M * sizeof(double)));
  EFA_TRY(c->ymw.reserve((size_t)a.R * sizeof(double)));
  a.Yw = c->Yw.as<double>();
  a.ymw = c->ymw.as<double>();
  return EFA_OK;
}

// ---- Phase A in WINDOWS of observations -----------------------------------------------------------------
// A persistent launch keeps 64 obs rows per workgroup and needs its whole grid resident: at most kPipeMaxWGs * 64
// rows (the window's obs + the M carried transform rows).  More observations are taken window by window: the
// window's rows and the transform rows go through one persistent launch (in a workspace when the window is not the
// whole block), and the rows of all OTHER observations -- earlier windows' (the reference keeps updating them,
// ensrf.py:141 acts on every augmented row) and later ones' -- take the window's trajectory through the per-batch
// sweep kernel, 64 obs per pass.  A window whose launch gives up (bounded spin, cancellation guard twice) is redone,
// for its own observations only, by the per-batch kernels.
// Without localisation a window that is not the whole block carries a SECOND set of identity rows: they come out as the
// window's own transform (T_w, w_w), which then updates all other rows of the block in one k_transform pass instead of
// one sweep pass per 64 obs.
//
// The window plan, and ONE launch that copies the caller's block into the working rows, writes the identity rows, fills the
// records with the sentinel and clears the status words.
int start_phase_a(efa_ctx* c, ObsCall& a) {
  const int M = a.M;
  const long P = a.P;
  hipStream_t s = c->stream;
  if (c->timing) EFA_HIP(hipEventRecord(c->ev[0], s));
  const long Wone = (long)kPipeMaxWGs * kPipeRowsPerWG - a.extra;           // one window covers the block up to here
  a.Wmax = (P <= Wone) ? Wone : Wone - a.extra;                              // else: two sets of extra rows per window
  a.pipe_ok = c->use_pipeline && a.Wmax > 0 && pipeline_supported(M, (P <= Wone ? P + a.extra : a.Wmax + 2 * a.extra));
  a.TS_std = traj_stride(M);
  a.TS_band = band_traj_stride(M);
  a.TS = a.TS_std > a.TS_band ? a.TS_std : a.TS_band;
  a.B = effective_batch(c, M);
  if (a.pipe_ok) {
    EFA_TRY(c->traj.reserve((size_t)P * a.TS * sizeof(unsigned long long)));
    EFA_TRY(c->status.reserve(3 * sizeof(int)));
  }
  unsigned long long* traj = a.pipe_ok ? c->traj.as<unsigned long long>() : nullptr;
  int* status = a.pipe_ok ? c->status.as<int>() : nullptr;
  c->qc_used = c->qc_threshold > 0.0;
  if (c->qc_used) {  // the outlier check decides every ob's flag here, ONCE, against the caller's block: windows and redone launches
                     // read the flags it wrote
    double* host_act = nullptr;
    if (a.loc_mode == EFA_LOC_GC) {
      EFA_TRY(c->qc_act.reserve((size_t)P * kCoefStride * sizeof(double)));
      host_act = c->qc_act.as<double>();
    }
    EFA_HIP(launch_phase_a_prep_qc(P, M, a.Yp_dev, a.ym_dev, a.Yw, a.ymw, a.carry_T ? 1 : 0, traj, a.pipe_ok ? (size_t)P * a.TS : 0,
                                   kTrajSentinel, status, c->pin_in.p, c->ob_pack.p, a.pack_bytes, a.islot, c->qc_threshold, host_act, s));
  } else {
    EFA_HIP(launch_phase_a_prep(P, M, a.Yp_dev, a.ym_dev, a.Yw, a.ymw, a.carry_T ? 1 : 0, traj, a.pipe_ok ? (size_t)P * a.TS : 0,
                                kTrajSentinel, status, c->pin_in.p, c->ob_pack.p, a.pack_bytes, s));
  }
  a.nwin = a.pipe_ok ? (P + a.Wmax - 1) / a.Wmax : 1;
  return EFA_OK;
}

// rows [0, nrows) of the working block but [skip_lo, skip_hi) take obs [b0, b0 + nb) from (Ye, ye_stride): the per-batch sweep
int sweep_rows(efa_ctx* c, const ObsCall& a, long b0, int nb, const double* Ye, long ye_stride, long skip_lo, long skip_hi,
               long nrows) {
  SweepArgs sw{};
  sw.Xin = a.Yw;
  sw.xin = a.ymw;
  sw.Xout = a.Yw;
  sw.xout = a.ymw;
  sw.nrows = nrows;
  sw.M = a.M;
  sw.Ye = Ye;
  sw.ye_stride = ye_stride;
  sw.coef = c->coef.as<double>() + (size_t)b0 * kCoefStride;
  sw.nb = nb;
  sw.taper_mode = (a.loc_mode == EFA_LOC_GC) ? kTaperObs : kTaperNone;
  if (a.loc_mode == EFA_LOC_GC && vl_active(c)) {  // horizontal x vertical taper of the batch against every row, in table mode
    EFA_TRY(c->vl_W.reserve((size_t)nb * a.R * sizeof(double)));
    EFA_HIP(launch_obs_taper_rows(b0, nb, a.R, a.P, c->ob_lat, c->ob_lon, c->ob_hw, vl_obvert(c), vl_obvhw(c), c->vl_W.as<double>(),
                                  c->stream));
    sw.taper_mode = kTaperTable;
    sw.W = c->vl_W.as<double>();
    sw.ncol = a.R;  // (row j of the block reads column j of the table)
  }
  sw.row_lat = c->ob_lat;
  sw.row_lon = c->ob_lon;
  sw.ob_lat = c->ob_lat + b0;
  sw.ob_lon = c->ob_lon + b0;
  sw.ob_hw = c->ob_hw + b0;
  sw.skip_lo = skip_lo;
  sw.skip_hi = skip_hi;
  sw.taper_rows = a.P;
  EFA_HIP(launch_sweep(sw, c->stream));
  return EFA_OK;
}

long active_in(const ObsCall& a, long b0, int nb) {
  long act = 0;
  for (int k = 0; k < nb; ++k) act += a.ob_assim[b0 + k] ? 1 : 0;
  return act;
}

// obs [w0, w1) by the per-batch kernels (k_diag on the batch's own rows, k_sweep on every other row of the block)
// (With vertical localisation one ob per batch: k_diag's in-batch taper is horizontal only, and an ob's taper against itself is 1.)
int batch_window(efa_ctx* c, const ObsCall& a, long w0, long w1) {
  const long B = (a.loc_mode == EFA_LOC_GC && vl_active(c)) ? 1 : a.B;
  for (long b0 = w0; b0 < w1; b0 += B) {
    const int nb = (int)((w1 - b0 < B) ? (w1 - b0) : B);
    DiagArgs d{};
    d.Yp = a.Yw;
    d.ym = a.ymw;
    d.M = a.M;
    d.b0 = b0;
    d.nb = nb;
    d.ob_value = c->ob_val;
    d.ob_error = c->ob_err;
    d.ob_assim = c->ob_asm;
    d.loc_mode = a.loc_mode;
    d.ob_lat = c->ob_lat;
    d.ob_lon = c->ob_lon;
    d.ob_hw = c->ob_hw;
    d.Ye_rec = c->Ye_rec.as<double>();
    d.coef = c->coef.as<double>();
    d.prior_mean = c->d_prior_mean;
    d.prior_var = c->d_prior_var;
    d.post_mean = c->d_post_mean;
    d.post_var = c->d_post_var;
    d.assimilated = c->d_assimilated;
    EFA_HIP(launch_diag(d, c->stream));
    if (active_in(a, b0, nb) == 0 || a.R == nb) continue;
    EFA_TRY(sweep_rows(c, a, b0, nb, c->Ye_rec.as<double>() + (size_t)b0 * a.M, a.M, b0, b0 + nb, a.R));
  }
  return EFA_OK;
}

// ... and for a window inside a call whose records are laid out already: the dense ye rows into that layout, zero-filled first
int batch_window_into_records(efa_ctx* c, const ObsCall& a, const Window& win, Records layout) {
  EFA_TRY(batch_window(c, a, win.w0, win.w1));
  const long TSk = record_stride(a, layout);
  double* rec = reinterpret_cast<double*>(c->traj.p) + (size_t)win.w0 * TSk;
  EFA_HIP(hipMemsetAsync(rec, 0, (size_t)win.Pw * TSk * sizeof(double), c->stream));
  EFA_HIP(hipMemcpy2DAsync(rec, (size_t)TSk * sizeof(double), c->Ye_rec.as<double>() + (size_t)win.w0 * a.M, (size_t)a.M * sizeof(double),
                           (size_t)a.M * sizeof(double), (size_t)win.Pw, hipMemcpyDeviceToDevice, c->stream));
  return EFA_OK;
}

// A windowed launch's rows, [window rows | transform rows | the window's own identity rows], copied out of the block.  Also the
// restore after a failed attempt: the block keeps the pre-launch rows.
int stage_window(efa_ctx* c, const ObsCall& a, const Window& win) {
  if (win.direct) return EFA_OK;
  hipStream_t s = c->stream;
  const int M = a.M;
  EFA_HIP(hipMemcpyAsync(win.Wy, a.Yw + (size_t)win.w0 * M, (size_t)win.Pw * M * sizeof(double), hipMemcpyDeviceToDevice, s));
  EFA_HIP(hipMemcpyAsync(win.Wm, a.ymw + win.w0, (size_t)win.Pw * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (a.extra) {
    EFA_HIP(hipMemcpyAsync(win.Wy + (size_t)win.Pw * M, a.Yw + (size_t)a.P * M, (size_t)a.extra * M * sizeof(double),
                           hipMemcpyDeviceToDevice, s));
    EFA_HIP(hipMemcpyAsync(win.Wm + win.Pw, a.ymw + a.P, (size_t)a.extra * sizeof(double), hipMemcpyDeviceToDevice, s));
    EFA_HIP(launch_set_identity(M, win.Wy + (size_t)(win.Pw + a.extra) * M, win.Wm + win.Pw + a.extra, s));  // the window's own transform
  }
  return EFA_OK;
}

// the rows of a failed attempt as they were before it: a direct launch from the caller's block and the identity rows
int restore_window(efa_ctx* c, const ObsCall& a, const Window& win) {
  if (!win.direct) return stage_window(c, a, win);
  hipStream_t s = c->stream;
  EFA_HIP(hipMemcpyAsync(a.Yw, a.Yp_dev, (size_t)a.P * a.M * sizeof(double), hipMemcpyDeviceToDevice, s));
  EFA_HIP(hipMemcpyAsync(a.ymw, a.ym_dev, (size_t)a.P * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (a.carry_T) EFA_HIP(launch_set_identity(a.M, a.Yw + (size_t)a.P * a.M, a.ymw + a.P, s));
  return EFA_OK;
}

// The persistent launch's arguments but the records; with localisation the window's obs-obs taper table, which a direct
// window reuses while the geometry, its shape and its allocation are unchanged.
int window_pipe_args(efa_ctx* c, const ObsCall& a, const Window& win, PipeArgs* out) {
  hipStream_t s = c->stream;
  const long w0 = win.w0, Pw = win.Pw, Rw = win.Rw;
  PipeArgs pa{};
  pa.Yp = win.Wy;
  pa.ym = win.Wm;
  pa.R = Rw;
  pa.P = Pw;
  pa.M = a.M;
  pa.ob_value = c->ob_val + w0;
  pa.ob_error = c->ob_err + w0;
  pa.ob_assim = c->ob_asm + w0;
  pa.ob_errsq = c->ob_errsq + 4 * w0;
  pa.loc_mode = a.loc_mode;
  pa.tw = nullptr;
  if (a.loc_mode == EFA_LOC_GC) {
    EFA_TRY(c->tw_mat.reserve((size_t)Pw * Rw * sizeof(double)));
    EFA_TRY(c->gc_obtrig.reserve((size_t)Pw * 6 * sizeof(double)));
    const bool tw_ok = c->geometry_reuse && win.direct && c->tw_serial == c->geo_serial && c->tw_Pw == Pw && c->tw_Rw == Rw &&
                       c->tw_ptr == c->tw_mat.p;
    if (!tw_ok) {
      EFA_HIP(launch_obs_taper_matrix(Pw, Rw, c->ob_lat + w0, c->ob_lon + w0, c->ob_hw + w0, c->gc_obtrig.as<double>(),
                                      c->tw_mat.as<double>(), s));
      if (vl_active(c)) EFA_HIP(launch_obs_taper_vert(Pw, Rw, vl_obvert(c) + w0, vl_obvhw(c) + w0, c->tw_mat.as<double>(), s));
      c->tw_serial = win.direct ? c->geo_serial : -1;  // (a window's table is not the whole block's)
      c->tw_Pw = Pw;
      c->tw_Rw = Rw;
      c->tw_ptr = c->tw_mat.p;
    }
    pa.tw = c->tw_mat.as<double>();
  }
  pa.coef = c->coef.as<double>() + (size_t)w0 * kCoefStride;
  pa.prior_mean = c->d_prior_mean + w0;
  pa.prior_var = c->d_prior_var + w0;
  pa.post_mean = c->d_post_mean + w0;
  pa.post_var = c->d_post_var + w0;
  pa.assimilated = c->d_assimilated + w0;
  pa.status = c->status.as<int>();
  pa.spin_limit = c->spin_limit;
  pa.spin_ticks = (c->spin_ms >= 0 ? c->spin_ms : 100 + Pw / 100) * 100000L;  // s_memrealtime runs at 100 MHz
  pa.cu_count = c->cu_count;
  pa.debug = (int)c->pipe_debug;
  pa.dbg = nullptr;
  if (c->pipe_debug & 4) {
    EFA_TRY(c->dbg.reserve((size_t)a.P * 8 * sizeof(unsigned long long)));
    if (win.w == 0) EFA_HIP(hipMemsetAsync(c->dbg.p, 0, (size_t)a.P * 8 * sizeof(unsigned long long), s));
    pa.dbg = c->dbg.as<unsigned long long>() + (size_t)w0 * 8;
  }
  *out = pa;
  return EFA_OK;
}

// The persistent kinds to try for a window, in order: 4 band leader (option "gram" 2), 3 Gram leader (1), 1 vector chain, the
// first whose kernel supports the window, then kind 1 if that was not it.  All windows of a call must leave records of ONE layout:
// after standard records a later window does not start with the band leader, and after band records it tries nothing but the band
// leader (it goes to the per-batch kernels instead).  A 0 ends the list.
std::array<int, 2> window_kinds(const efa_ctx* c, const ObsCall& a, long Rw, Records layout) {
  const bool band = c->use_gram >= 2 && pipeline_band_supported(a.M, Rw, a.loc_mode);
  const bool gram = c->use_gram >= 1 && pipeline_gram_supported(a.M, Rw, a.loc_mode);
  const int first = (band && layout != Records::kStandard) ? 4 : gram ? 3 : 1;
  if (layout == Records::kBand) return {first == 4 ? 4 : 0, 0};
  return {first, first == 1 ? 0 : 1};
}

// efa_ensrf_cycle_dev: the state transform goes into the stream behind the launch whose status is not known yet -- it reads
// [T | w] from the launch's working rows and writes only the caller's posterior; a launch that reports a fallback is redone
// and the transform enqueued again (by the caller), so a wrong guess costs time, never a result.  The device then runs
// Phase A -> Phase B with no host round trip in between.
int speculative_transform(efa_ctx* c, const ObsCall& a, const Window& win, bool* placed) {
  *placed = false;
  if (!(c->spec.armed && c->spec.rows > 0 && win.direct && a.carry_T && c->n_active > 0 &&
        (c->path == EFA_PATH_TRANSFORM || (c->path == EFA_PATH_AUTO && auto_transform(a.M, c->n_active, true)))))
    return EFA_OK;
  hipStream_t s = c->stream;
  const int pr = c->state_ms_pending ? 1 : 0;
  if (c->timing) harvest_state_pair(c, pr);  // (both pairs unread cannot happen across the wait below; kept correct anyway)
  // ONE event between Phase A and the transform (each record idles the stream ~6 us): the status words and diagnostics are on
  // the host -- what the host waits for -- the obs interval ends and the state interval of this pair begins
  EFA_HIP(hipEventRecord(c->ev[2 + 2 * pr], s));
  c->obs_end_ev = 2 + 2 * pr;
  EFA_TRY(transform_with_relaxation(c, carried_transform(c, c->spec.X, nullptr, c->spec.post, nullptr, c->spec.rows, 1),
                                    &c->spec.launches));
  if (c->timing) EFA_HIP(hipEventRecord(c->ev[3 + 2 * pr], s));
  c->spec.pair = pr;
  *placed = true;
  return EFA_OK;
}

// ONE host round trip per launch: the status words and -- when this launch is the whole Phase A -- the diagnostics it wrote come
// back together, into pinned memory (a second copy + synchronise after the status was known left the device idle for ~40 us
// before Phase B; a pageable destination made the status copy itself a staged one).  *st: the status words on the host.
int launch_round_trip(efa_ctx* c, const ObsCall& a, const Window& win, const int** st_out, bool* spec_now) {
  hipStream_t s = c->stream;
  int* st = reinterpret_cast<int*>(static_cast<char*>(c->pin_out.p) + 5 * a.oslot - 64);
  if (win.direct) EFA_HIP(launch_results_to_host(c->out_pack.p, c->pin_out.p, 4 * a.oslot + (size_t)a.P, c->status.as<int>(), st, s));
  else EFA_HIP(hipMemcpyAsync(st, c->status.p, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
  EFA_TRY(speculative_transform(c, a, win, spec_now));
  if (*spec_now) EFA_HIP(hipEventSynchronize(c->ev[2 + 2 * c->spec.pair]));  // (not the stream: the transform behind it is to run while the host goes on)
  else EFA_HIP(hipStreamSynchronize(s));
  c->spec.launched = false;
  if (*spec_now && c->timing) harvest_state_pair(c, 1 - c->spec.pair);  // the previous cycle's interval: complete by now
  *st_out = st;
  return EFA_OK;
}

// One window through the persistent kernels.  *kind_out: the kind that did it, or 0 -- fall back to the per-batch kernels.
// A failed attempt (bounded spin expired, or the Gram downdate's cancellation guard) may have let finished workgroups write
// their rows back, so the launch's rows are restored before anything else runs on them.  An attempt is skipped when its grid
// cannot be co-resident (occupancy query in the launcher), and after an attempt whose bounded spins EXPIRED (some workgroups
// never became resident, e.g. another kernel holds CUs) no other persistent kernel is tried: they have the same residency need.
int try_persistent_window(efa_ctx* c, const ObsCall& a, Window& win, Records layout, bool& status_clear, int* kind_out) {
  hipStream_t s = c->stream;
  *kind_out = 0;
  if (!win.direct) {
    EFA_TRY(c->win_Y.reserve((size_t)win.Rw * a.M * sizeof(double)));
    EFA_TRY(c->win_m.reserve((size_t)win.Rw * sizeof(double)));
    win.Wy = c->win_Y.as<double>();
    win.Wm = c->win_m.as<double>();
  }
  EFA_TRY(stage_window(c, a, win));
  if (!status_clear) EFA_HIP(hipMemsetAsync(c->status.p, 0, 3 * sizeof(int), s));  // (the prep launch cleared it for the first)
  status_clear = false;
  PipeArgs pa;
  EFA_TRY(window_pipe_args(c, a, win, &pa));
  for (const int kind : window_kinds(c, a, win.Rw, layout)) {
    if (kind == 0) break;
    pa.traj = c->traj.as<unsigned long long>() + (size_t)win.w0 * (kind == 4 ? a.TS_band : a.TS_std);
    const hipError_t le = kind == 4 ? launch_pipeline_band(pa, s) : kind == 3 ? launch_pipeline_gram(pa, s) : launch_pipeline(pa, s);
    if (le == hipErrorCooperativeLaunchTooLarge) {
      (void)hipGetLastError();
      continue;
    }
    EFA_HIP(le);
    const int* st = nullptr;
    bool spec_now = false;
    EFA_TRY(launch_round_trip(c, a, win, &st, &spec_now));
    if (st[0] == 0 && st[1] == 0) {
      *kind_out = kind;
      c->spec.launched = spec_now;
      return EFA_OK;
    }
    EFA_TRY(restore_window(c, a, win));
    if (st[2] == 0) break;  // not the Gram guard, so a spin expired: straight to the per-batch kernels
    if (kind != 1) {        // a failed first attempt (kind 1 only ever comes last): fresh records and status for the next
      EFA_HIP(launch_fill_u64(c->traj.as<unsigned long long>() + (size_t)win.w0 * a.TS, (size_t)win.Pw * a.TS, kTrajSentinel, s));
      EFA_HIP(hipMemsetAsync(c->status.p, 0, 3 * sizeof(int), s));
    }
  }
  return EFA_OK;
}

// A windowed launch that succeeded: window rows and transform rows back into the block, then every other row of the block takes
// the window's records -- through the window's own transform without localisation, else the per-batch sweep
int merge_window_into_block(efa_ctx* c, const ObsCall& a, const Window& win, Records layout) {
  hipStream_t s = c->stream;
  const int M = a.M;
  const long P = a.P, w0 = win.w0, w1 = win.w1, Pw = win.Pw, extra = a.extra;
  EFA_HIP(hipMemcpyAsync(a.Yw + (size_t)w0 * M, win.Wy, (size_t)Pw * M * sizeof(double), hipMemcpyDeviceToDevice, s));
  EFA_HIP(hipMemcpyAsync(a.ymw + w0, win.Wm, (size_t)Pw * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (extra) {
    EFA_HIP(hipMemcpyAsync(a.Yw + (size_t)P * M, win.Wy + (size_t)Pw * M, (size_t)extra * M * sizeof(double), hipMemcpyDeviceToDevice, s));
    EFA_HIP(hipMemcpyAsync(a.ymw + P, win.Wm + Pw, (size_t)extra * sizeof(double), hipMemcpyDeviceToDevice, s));
    for (int part = 0; part < 2; ++part) {  // unlocalised: rows [0, w0) and [w1, P) through the window's transform, in place
      const long lo = part ? w1 : 0, hi = part ? P : w0;
      if (hi <= lo) continue;
      const TransformArgs t{a.Yw + (size_t)lo * M, a.ymw + lo, a.Yw + (size_t)lo * M, a.ymw + lo, hi - lo, M,
                            win.Wy + (size_t)(Pw + extra) * M, win.Wm + Pw + extra, 0};
      EFA_HIP(launch_transform(t, s));
    }
    return EFA_OK;
  }
  const long TSk = record_stride(a, layout);
  const double* yebase = reinterpret_cast<const double*>(c->traj.p);
  for (long b0 = w0; b0 < w1; b0 += a.B) {
    const int nb = (int)((w1 - b0 < a.B) ? (w1 - b0) : a.B);
    if (active_in(a, b0, nb) == 0) continue;
    EFA_TRY(sweep_rows(c, a, b0, nb, yebase + (size_t)b0 * TSk, TSk, w0, w1, P));  // rows [0, P) but the window's own
  }
  return EFA_OK;
}

// Where Phase B finds the records, the obs block and the diagnostics back to the caller (ensrf.py:66,70,75,146-149)
int finish_obs_phase(efa_ctx* c, const ObsCall& a, Records layout, bool diag_on_host, double* prior_mean, double* prior_var,
                     double* post_mean, double* post_var, uint8_t* assimilated) {
  hipStream_t s = c->stream;
  const long P = a.P;
  const size_t dP = (size_t)P * sizeof(double), oslot = a.oslot;
  if (layout == Records::kNone) {
    c->ye_ptr = c->Ye_rec.as<double>();
    c->ye_stride = a.M;
    c->phase_a_kind = 2;
  } else {
    c->ye_ptr = reinterpret_cast<const double*>(c->traj.p);
    c->ye_stride = record_stride(a, layout);
  }
  if (!c->spec.armed || c->spec.obs_out) {
    EFA_HIP(hipMemcpyAsync(a.Yp_dev, a.Yw, (size_t)P * a.M * sizeof(double), hipMemcpyDeviceToDevice, s));
    EFA_HIP(hipMemcpyAsync(a.ym_dev, a.ymw, dP, hipMemcpyDeviceToDevice, s));
  }
  if (c->timing && !c->spec.launched) {  // (behind a speculative transform the interval ended at the event in front of it)
    EFA_HIP(hipEventRecord(c->ev[1], s));
    c->obs_end_ev = 1;
  }
  if (!diag_on_host) {
    EFA_HIP(hipMemcpyAsync(c->pin_out.p, c->out_pack.p, 4 * oslot + (size_t)P, hipMemcpyDeviceToHost, s));
    EFA_HIP(hipStreamSynchronize(s));
  }
  const char* hb = static_cast<const char*>(c->pin_out.p);
  if (prior_mean) std::memcpy(prior_mean, hb, dP);
  if (prior_var) std::memcpy(prior_var, hb + oslot, dP);
  const double* pm = reinterpret_cast<const double*>(hb + 2 * oslot);
  const double* pv = reinterpret_cast<const double*>(hb + 3 * oslot);
  const uint8_t* as = reinterpret_cast<const uint8_t*>(hb + 4 * oslot);
  for (long k = 0; k < P; ++k) {
    if (assimilated) assimilated[k] = as[k];
    if (as[k]) {
      if (post_mean) post_mean[k] = pm[k];
      if (post_var) post_var[k] = pv[k];
    }
  }
  if (c->qc_used) {  // the outlier check may have rejected obs: the state phase goes by the flags Phase A went by
    c->n_active = 0;
    for (long k = 0; k < P; ++k) {
      c->h_assim[k] = as[k] ? 1 : 0;
      c->n_active += as[k] ? 1 : 0;
    }
  }
  if (c->timing) c->obs_ms_pending = true;  // read in efa_last_timing: the copies back to the caller's block may still be in flight
  c->have_transform = a.carry_T;
  c->have_traj = true;
  return EFA_OK;
}

int obs_phase(efa_ctx* c, int M, long P, double* ym_dev, double* Yp_dev, const double* ob_value,
              const double* ob_error, const uint8_t* ob_assim, int loc_mode, const double* ob_lat,
              const double* ob_lon, const double* ob_hw, double* prior_mean, double* prior_var,
              double* post_mean, double* post_var, uint8_t* assimilated) {
  EFA_TRY(check_common(M, P));
  if (loc_mode != EFA_LOC_NONE && loc_mode != EFA_LOC_GC) return fail(EFA_ERR_INVALID, "loc_mode %d", loc_mode);
  EFA_TRY(check_vloc(c, loc_mode, P, -1));
  c->have_traj = false;
  c->M = M;
  c->P = P;
  c->loc_mode = loc_mode;
  c->n_active = 0;
  c->have_transform = false;
  c->spec.launched = false;
  c->qc_used = false;
  harvest_obs_ms(c);
  c->obs_ms = 0.0;
  if (P == 0) {
    c->have_traj = true;
    c->h_assim.clear();
    return EFA_OK;
  }
  ObsCall a;
  a.M = M;
  a.P = P;
  a.loc_mode = loc_mode;
  a.ym_dev = ym_dev;
  a.Yp_dev = Yp_dev;
  a.ob_assim = ob_assim;
  EFA_TRY(stage_obs_inputs(c, a, ob_value, ob_error, ob_lat, ob_lon, ob_hw));
  EFA_TRY(start_phase_a(c, a));
  Records layout = Records::kNone;
  bool diag_on_host = false;    // the diagnostics are already in pin_out (copied with the status words of the one launch that did it all)
  bool status_clear = a.pipe_ok;  // (cleared by the prep launch: the first window's launch needs no memset of its own)
  for (long w = 0; w < a.nwin; ++w) {
    Window win = make_window(a, w);
    const bool tw_fits = (loc_mode != EFA_LOC_GC) || ((size_t)win.Pw * (size_t)win.Rw * sizeof(double) <= ((size_t)3 << 30));
    int kind = 0;
    if (a.pipe_ok && tw_fits) EFA_TRY(try_persistent_window(c, a, win, layout, status_clear, &kind));
    if (kind != 0) {
      layout = (kind == 4) ? Records::kBand : Records::kStandard;
      c->phase_a_kind = kind;
      diag_on_host = win.direct;
      if (!win.direct) EFA_TRY(merge_window_into_block(c, a, win, layout));
    } else if (layout != Records::kNone) {
      EFA_TRY(batch_window_into_records(c, a, win, layout));
    } else if (w == 0) {
      EFA_TRY(batch_window(c, a, 0, P));  // nothing has run as a pipeline: the whole call goes to the per-batch kernels
      break;
    } else {
      return fail(EFA_ERR_UNSUPPORTED, "internal: mixed Phase-A layouts");
    }
  }
  return finish_obs_phase(c, a, layout, diag_on_host, prior_mean, prior_var, post_mean, post_var, assimilated);
}

// path "auto": one transform pass or sweep passes?  By FLOPS one transform pass is M/2 observations of sweep arithmetic (the rule of
// rounds 1-2), but the transform runs on the matrix cores at 49 TFLOP/s and the sweep on the vector ALUs at 10-20, and in MEMBER form
// (prior members in, posterior members out) the sweep path is three passes over the state -- form the perturbations, sweep, rebuild
// the members -- where the transform is one.  Measured at 1e7 x 100 (profiles/r03_auto_path.txt): member form 8 obs 10.6 ms by
// sweeps, 4.1 by the transform (48 obs: 16.9 vs 4.1); perturbation form 8 / 16 obs per sweep launch 3.4 / 4.5 ms vs 4.5.
// Above 136 members the transform re-reads the state once per group of 64 output columns: the flops rule stays.
bool auto_transform(int M, long n_active, bool member_form) {
  if (n_active <= 0) return false;
  if (M > 136) return n_active > M / 2;
  if (member_form) return true;
  return n_active > M / 8;
}
bool want_transform(const efa_ctx* c, bool member_form) {
  if (!c->have_transform) return false;
  if (c->path == EFA_PATH_TRANSFORM) return true;
  if (c->path == EFA_PATH_SWEEP) return false;
  return auto_transform(c->M, c->n_active, member_form);
}

int prepare_grid(efa_ctx* c, const double* grid_lat, const double* grid_lon, long ncol, long n_lead, long rows) {
  if (c->loc_mode != EFA_LOC_GC) return EFA_OK;
  if (!grid_lat || !grid_lon) return fail(EFA_ERR_INVALID, "GC localisation needs grid_lat/grid_lon");
  if (ncol <= 0 || n_lead <= 0 || ncol * n_lead != rows)
    return fail(EFA_ERR_INVALID, "rows=%ld must equal n_lead*ncol = %ld*%ld", rows, n_lead, ncol);
  if (c->grid_ready) {  // (the fused cycle did this before Phase A, while the device was still busy with the previous cycle)
    c->grid_ready = false;
    return EFA_OK;
  }
  EFA_TRY(h2d(c, c->glat, grid_lat, (size_t)ncol * sizeof(double)));
  EFA_TRY(h2d(c, c->glon, grid_lon, (size_t)ncol * sizeof(double)));
  c->grid_ncol = -1;
  c->grid_serial++;
  EFA_HIP(hipStreamSynchronize(c->stream));  // caller may reuse grid_lat/grid_lon on return
  return EFA_OK;
}

// The same grid ahead of Phase A (efa_ensrf_cycle_dev): compared with a pinned mirror of what the device holds and copied -- from
// the mirror, asynchronously -- only if it differs.  Cycle after cycle on one grid nothing is copied; the comparison (4 MB at
// configs[3]) is host time spent while the device still works on the previous cycle.
int prepare_grid_early(efa_ctx* c, int loc_mode, const double* grid_lat, const double* grid_lon, long ncol, long n_lead, long rows) {
  c->grid_ready = false;
  if (loc_mode != EFA_LOC_GC || rows <= 0) return EFA_OK;
  if (!grid_lat || !grid_lon) return fail(EFA_ERR_INVALID, "GC localisation needs grid_lat/grid_lon");
  if (ncol <= 0 || n_lead <= 0 || ncol * n_lead != rows)
    return fail(EFA_ERR_INVALID, "rows=%ld must equal n_lead*ncol = %ld*%ld", rows, n_lead, ncol);
  const size_t nb = (size_t)ncol * sizeof(double);
  const void* pin_before = c->pin_grid.p;
  EFA_TRY(c->pin_grid.reserve(2 * nb));
  char* pin = static_cast<char*>(c->pin_grid.p);
  const void *dl = c->glat.p, *dn = c->glon.p;
  EFA_TRY(c->glat.reserve(nb));
  EFA_TRY(c->glon.reserve(nb));
  const bool same = c->grid_ncol == ncol && pin_before == c->pin_grid.p && dl == c->glat.p && dn == c->glon.p &&
                    std::memcmp(pin, grid_lat, nb) == 0 && std::memcmp(pin + nb, grid_lon, nb) == 0;
  if (!same) {
    EFA_HIP(hipStreamSynchronize(c->stream));  // (an earlier copy out of the mirror may be in flight; a new grid is the rare case)
    std::memcpy(pin, grid_lat, nb);
    std::memcpy(pin + nb, grid_lon, nb);
    EFA_HIP(hipMemcpyAsync(c->glat.p, pin, nb, hipMemcpyHostToDevice, c->stream));
    EFA_HIP(hipMemcpyAsync(c->glon.p, pin + nb, nb, hipMemcpyHostToDevice, c->stream));
    c->grid_ncol = ncol;
    c->grid_serial++;
  }
  c->grid_ready = true;
  return EFA_OK;
}

// ... and once it has work to do: the grid of a localised call on the device, the state interval begins
int begin_state_work(efa_ctx* c, const double* grid_lat, const double* grid_lon, long ncol, long n_lead, long rows) {
  EFA_TRY(prepare_grid(c, grid_lat, grid_lon, ncol, n_lead, rows));
  if (c->timing) EFA_HIP(hipEventRecord(c->ev[2], c->stream));
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

// ---- Phase B, localised, one pass (efa_gcsweep.hip) --------------------------------------
int state_gc_onepass(efa_ctx* c, const double* xm_in, const double* Xp_in, double* xm_out, double* Xp_out, long ncol, long n_lead,
                     int fused_members) {
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
  const bool lists_ok = c->geometry_reuse && c->gc_list_valid && c->gc_list_geo == c->geo_serial && c->gc_list_grid == c->grid_serial &&
                        c->gc_list_ncol == ncol && c->gc_list_P == P && std::memcmp(ptrs, c->gc_list_ptrs, sizeof(ptrs)) == 0;
  if (!lists_ok) {
  c->gc_list_valid = false;
  EFA_TRY(read_gc_pairs(c));  // (the previous sweep's count, before the counter is cleared: that sweep is long done)
  EFA_HIP(hipMemsetAsync(c->gc_pairs.p, 0, sizeof(unsigned long long), s));
  // the lists hold the obs the CALLER asked to assimilate, as the geometry they are cached by: an ob the outlier check rejected
  // stays in them with its inactive record (zero gains), so a later cycle that keeps it finds it there
  const double* act = c->qc_used ? c->qc_act.as<double>() : c->coef.as<double>();
  EFA_HIP(launch_gc_bound(ncol, P, c->glat.as<double>(), c->ob_lat, c->ob_hw, act, c->gc_ub.as<int>(), c->gc_off.as<long>(), s));
  long cap = 0;  // the only host round trip of the build: 8 bytes, the capacity the lists need
  EFA_HIP(hipMemcpyAsync(&cap, c->gc_off.as<long>() + nblk, sizeof(long), hipMemcpyDeviceToHost, s));
  EFA_HIP(hipStreamSynchronize(s));
  EFA_TRY(c->gc_idx.reserve((size_t)(cap ? cap : 1) * sizeof(int)));
  EFA_TRY(c->gc_wts.reserve((size_t)(cap ? cap : 1) * 16 * sizeof(double)));
  EFA_HIP(launch_gc_fill(ncol, P, c->glat.as<double>(), c->glon.as<double>(), c->ob_lat, c->ob_lon, c->ob_hw, act,
                         c->gc_obtrig.as<double>(), c->gc_off.as<long>(), c->gc_cnt.as<int>(), c->gc_idx.as<int>(),
                         c->gc_wts.as<double>(), c->gc_order.as<int>(), c->gc_pairs.as<unsigned long long>(), s));
  c->gc_list_valid = true;
  c->gc_list_geo = c->geo_serial;
  c->gc_list_grid = c->grid_serial;
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
  g.Xin = Xp_in;
  g.xin = xm_in;
  g.Xout = Xp_out;
  g.xout = xm_out;
  g.fused_members = fused_members;
  if (c->ai_field) {  // the per-ob scalars of the inflation update, from Phase A's records and diagnostics
    EFA_TRY(c->ai_ob.reserve((size_t)(P ? P : 1) * 4 * sizeof(double)));
    EFA_HIP(launch_adapt_obs(P, M, c->coef.as<double>(), c->d_prior_var, c->ob_err, c->ye_ptr, c->ye_stride,
                             c->ai_ob.as<double>(), s));
    c->state_launches++;
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
  EFA_HIP(launch_sweep_gc(g, s));
  c->state_launches++;
  return EFA_OK;
}

// ---- Phase B (perturbation form) ------------------------------------------
int state_sweeps(efa_ctx* c, long rows, const double* xm_in, const double* Xp_in, double* xm_out, double* Xp_out,
                 long ncol) {
  const int M = c->M;
  const long P = c->P;
  hipStream_t s = c->stream;
  if (c->loc_mode == EFA_LOC_GC && c->gc_onepass && c->n_active > 0)  // every ensemble size the library accepts (2..256)
    return state_gc_onepass(c, xm_in, Xp_in, xm_out, Xp_out, ncol, rows / ncol, 0);
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
      EFA_HIP(launch_taper_table(ncol, nb, c->glat.as<double>(), c->glon.as<double>(), c->ob_lat + b0, c->ob_lon + b0, c->ob_hw + b0,
                                 c->W.as<double>(), s));
      a.taper_mode = kTaperTable;
      a.W = c->W.as<double>();
      a.ncol = ncol;
    } else {
      a.taper_mode = kTaperNone;
    }
    EFA_HIP(launch_sweep(a, s));
    c->state_launches++;
    first = false;
  }
  if (first && Xp_out != Xp_in) {  // nothing assimilated: posterior == prior
    EFA_HIP(hipMemcpyAsync(Xp_out, Xp_in, (size_t)rows * M * sizeof(double), hipMemcpyDeviceToDevice, s));
    EFA_HIP(hipMemcpyAsync(xm_out, xm_in, (size_t)rows * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  return EFA_OK;
}

int state_phase(efa_ctx* c, long rows, int M, const double* xm_in, const double* Xp_in, double* xm_out,
                double* Xp_out, const double* grid_lat, const double* grid_lon, long ncol, long n_lead) {
  if (!c->have_traj) return fail(EFA_ERR_INVALID, "efa_state_phase_dev called before efa_obs_phase_dev");
  if (M != c->M) return fail(EFA_ERR_INVALID, "M=%d differs from the obs phase's M=%d", M, c->M);
  if (rows < 0) return fail(EFA_ERR_INVALID, "negative row count");
  EFA_TRY(check_adaptive(c, c->loc_mode, rows));
  EFA_TRY(check_vloc(c, c->loc_mode, c->P, n_lead));
  reset_state_phase(c);
  if (rows == 0) return EFA_OK;
  if (!xm_in || !Xp_in || !xm_out || !Xp_out) return fail(EFA_ERR_INVALID, "null state pointer");
  EFA_TRY(begin_state_work(c, grid_lat, grid_lon, ncol, n_lead, rows));
  if (c->P > 0 && c->n_active > 0 && want_transform(c, false)) {
    EFA_TRY(transform_with_relaxation(c, carried_transform(c, Xp_in, xm_in, Xp_out, xm_out, rows, 0), &c->state_launches));
    c->path_taken = EFA_PATH_TRANSFORM;
  } else {
    EFA_TRY(with_relaxation(c, rows, M, Xp_in, Xp_out, &c->state_launches,
                            [&] { return state_sweeps(c, rows, xm_in, Xp_in, xm_out, Xp_out, ncol); }));
  }
  return finish_state_timing(c, c->stream);
}

}  // namespace

// ===========================================================================
// ---- RCCL, bound at run time: a single-GPU caller never loads it ---------------------------------------
namespace {
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;

int rccl_load() {
  if (g_rccl.lib) return EFA_OK;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;
  for (const char* n : names) {
    h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (h) break;
  }
  if (!h) return fail(EFA_ERR_UNSUPPORTED, "librccl could not be opened: %s", dlerror());
  RcclApi a;
  a.lib = h;
  a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
  a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
  a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(h, "ncclAllReduce"));
  a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
  a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
  if (!a.GetUniqueId || !a.CommInitRank || !a.AllReduce || !a.CommDestroy || !a.GetErrorString) {
    dlclose(h);
    return fail(EFA_ERR_UNSUPPORTED, "librccl lacks an expected symbol");
  }
  g_rccl = a;
  return EFA_OK;
}
#define EFA_RCCL(expr)                                                                                       \
  do {                                                                                                       \
    ncclResult_t _r = (expr);                                                                                \
    if (_r != ncclSuccess) return fail(EFA_ERR_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(_r));      \
  } while (0)
}  // namespace

extern "C" {

int efa_abi_version(void) { return EFA_ABI_VERSION; }

const char* efa_last_error(void) { return g_last_error.c_str(); }

int efa_device_count(int* count) {
  if (!count) return fail(EFA_ERR_INVALID, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  *count = n;
  return EFA_OK;
}

int efa_ctx_create(int device_id, efa_ctx** out) {
  if (!out) return fail(EFA_ERR_INVALID, "null out pointer");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return fail(EFA_ERR_NO_DEVICE,
                "no HIP device visible (%s): libefa_hip has no CPU fallback and needs an MI355X (gfx950)",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  }
  if (device_id < 0 || device_id >= n) return fail(EFA_ERR_INVALID, "device_id %d out of range [0,%d)", device_id, n);
  hipDeviceProp_t prop;
  EFA_HIP(hipGetDeviceProperties(&prop, device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(EFA_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", device_id,
                prop.gcnArchName);
  EFA_HIP(hipSetDevice(device_id));
  efa_ctx* c = new (std::nothrow) efa_ctx();
  if (!c) return fail(EFA_ERR_INVALID, "out of host memory");
  c->device = device_id;
  c->cu_count = prop.multiProcessorCount;
  hipError_t es = hipStreamCreateWithFlags(&c->own_stream.h, hipStreamNonBlocking);
  if (es != hipSuccess) {
    delete c;
    return fail(EFA_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(es));
  }
  c->stream = c->own_stream;
  for (int i = 0; i < 7; ++i) {
    hipError_t ee = hipEventCreate(&c->ev[i].h);
    if (ee != hipSuccess) {
      delete c;
      return fail(EFA_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(ee));
    }
  }
  {
    hipError_t ee = hipEventCreateWithFlags(&c->ev_order.h, hipEventDisableTiming);
    if (ee != hipSuccess) {
      delete c;
      return fail(EFA_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(ee));
    }
  }
  *out = c;
  return EFA_OK;
}

int efa_ctx_destroy(efa_ctx* c) {
  if (!c) return EFA_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
  delete c;
  return EFA_OK;
}

namespace {
// The calls return with work still in the stream, and that work reads the context's own workspaces (the transform [T | w] behind
// the obs rows, the recorded trajectory, the active lists, the grid, the pair counter).  What is issued after a change of stream
// is therefore ordered behind everything issued before it: an event on the stream that is left, waited for on the device by the
// one that takes over.  No host wait; NULL (the legacy default stream) is a stream like any other here.
int change_stream(efa_ctx* c, hipStream_t to) {
  if (to == c->stream) return EFA_OK;
  EFA_HIP(hipEventRecord(c->ev_order, c->stream));
  EFA_HIP(hipStreamWaitEvent(to, c->ev_order, 0));
  c->stream = to;
  return EFA_OK;
}
}  // namespace

int efa_ctx_set_stream(efa_ctx* c, void* hip_stream) {
  EFA_TRY(use(c));
  // NULL is a valid handle: the device's legacy default stream (what torch uses unless told otherwise)
  return change_stream(c, reinterpret_cast<hipStream_t>(hip_stream));
}

int efa_ctx_set_option(efa_ctx* c, const char* key, long value) {
  EFA_TRY(use(c));
  if (!key) return fail(EFA_ERR_INVALID, "null option key");
  if (!strcmp(key, "obs_batch")) {
    if (value < 1 || value > efa::kMaxBatch) return fail(EFA_ERR_INVALID, "obs_batch must be in [1,%d]", efa::kMaxBatch);
    c->obs_batch = value;
  } else if (!strcmp(key, "path")) {
    if (value < EFA_PATH_AUTO || value > EFA_PATH_TRANSFORM) return fail(EFA_ERR_INVALID, "path must be 0,1,2");
    c->path = value;
  } else if (!strcmp(key, "timing")) {
    if (value < 0 || value > 2) return fail(EFA_ERR_INVALID, "timing must be 0, 1 or 2");
    harvest_obs_ms(c);
    harvest_state_ms(c);
    c->timing = value;
    c->state_ms_sum = c->obs_ms_sum = 0.0;
    c->state_launches_sum = 0;
  } else if (!strcmp(key, "gram")) {
    if (value < 0 || value > 2) return fail(EFA_ERR_INVALID, "gram must be 0, 1 or 2");
    c->use_gram = value;
  } else if (!strcmp(key, "pipeline")) {
    c->use_pipeline = value ? 1 : 0;
  } else if (!strcmp(key, "gc_onepass")) {
    c->gc_onepass = value ? 1 : 0;
  } else if (!strcmp(key, "geometry_reuse")) {
    c->geometry_reuse = value ? 1 : 0;
  } else if (!strcmp(key, "own_stream")) {
    EFA_TRY(change_stream(c, c->own_stream));  // back to the context's private non-blocking stream
  } else if (!strcmp(key, "pipe_debug")) {
    c->pipe_debug = value;
  } else if (!strcmp(key, "spin_limit")) {
    if (value < 1) return fail(EFA_ERR_INVALID, "spin_limit must be positive");
    c->spin_limit = value;
  } else if (!strcmp(key, "spin_ms")) {
    c->spin_ms = value;
  } else if (!strcmp(key, "debug_occupy_blocks")) {
    c->dbg_occupy_blocks = value;
  } else if (!strcmp(key, "debug_occupy_ms")) {
    // diagnostic: on a stream of its own, debug_occupy_blocks workgroups hold 120 KB of LDS each (one per CU, and no
    // persistent Phase-A workgroup fits beside one) for `value` ms; value 0 waits for them to finish
    if (!c->dbg_stream) {
      // On a stream of the highest priority: the runtime keeps the hardware queues of each priority apart, so the occupier never
      // lands in the queue the context's own (default-priority) stream was given -- which, with few hardware queues and many
      // streams created in the process before, it otherwise can, and then it runs in front of Phase A instead of beside it.
      int least = 0, greatest = 0;
      EFA_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
      EFA_HIP(hipStreamCreateWithPriority(&c->dbg_stream.h, hipStreamNonBlocking, greatest));
    }
    if (value > 0) EFA_HIP(efa::launch_occupy((int)c->dbg_occupy_blocks, 120 * 1024, (double)value, c->dbg_stream));
    else EFA_HIP(hipStreamSynchronize(c->dbg_stream));
  } else if (!strcmp(key, "threads_hint")) {
  } else {
    return fail(EFA_ERR_INVALID, "unknown option '%s'", key);
  }
  return EFA_OK;
}

int efa_ctx_set_relaxation(efa_ctx* c, int kind, double alpha) {
  EFA_TRY(use(c));
  if (kind != EFA_RELAX_NONE && kind != EFA_RELAX_RTPP && kind != EFA_RELAX_RTPS)
    return fail(EFA_ERR_INVALID, "relaxation kind %d: expected EFA_RELAX_NONE (0), EFA_RELAX_RTPP (1) or EFA_RELAX_RTPS (2)", kind);
  if (kind != EFA_RELAX_NONE) {
    if (!std::isfinite(alpha)) return fail(EFA_ERR_INVALID, "relaxation factor must be a finite number");
    if (alpha < 0.0) return fail(EFA_ERR_INVALID, "relaxation factor %g must be >= 0", alpha);
    if (kind == EFA_RELAX_RTPP && alpha > 1.0) return fail(EFA_ERR_INVALID, "RTPP factor %g must be <= 1", alpha);
  }
  c->relax_kind = kind;
  c->relax_alpha = kind == EFA_RELAX_NONE ? 0.0 : alpha;
  return EFA_OK;
}

int efa_ctx_set_adaptive_inflation(efa_ctx* c, double* field_dev, long rows, double lower, double upper, double sd_lower) {
  EFA_TRY(use(c));
  if (!field_dev) {
    c->ai_field = nullptr;
    c->ai_rows = 0;
    return EFA_OK;
  }
  if (rows < 0) return fail(EFA_ERR_INVALID, "adaptive inflation: negative row count");
  if ((reinterpret_cast<uintptr_t>(field_dev) & 7u) != 0) return fail(EFA_ERR_INVALID, "adaptive inflation: field must be 8-byte aligned");
  if (!std::isfinite(lower) || !(lower > 0.0)) return fail(EFA_ERR_INVALID, "adaptive inflation: lower bound %g must be finite and > 0", lower);
  if (!std::isfinite(upper) || upper < lower)
    return fail(EFA_ERR_INVALID, "adaptive inflation: upper bound %g must be finite and >= the lower bound %g", upper, lower);
  if (!std::isfinite(sd_lower) || sd_lower < 0.0)
    return fail(EFA_ERR_INVALID, "adaptive inflation: sd lower bound %g must be finite and >= 0", sd_lower);
  c->ai_field = field_dev;
  c->ai_rows = rows;
  c->ai_lower = lower;
  c->ai_upper = upper;
  c->ai_sd_lower = sd_lower;
  return EFA_OK;
}

int efa_ctx_set_vertical_localization(efa_ctx* c, long n_lead, const double* lead_vert, long P, const double* ob_vert,
                                      const double* ob_vert_halfwidth) {
  EFA_TRY(use(c));
  if (!lead_vert) {
    if (c->vl_on) c->vl_serial++;
    c->vl_on = false;
    return EFA_OK;
  }
  if (n_lead <= 0) return fail(EFA_ERR_INVALID, "vertical localisation: n_lead=%ld must be > 0", n_lead);
  if (P < 0) return fail(EFA_ERR_INVALID, "vertical localisation: negative observation count");
  if (P > 0 && (!ob_vert || !ob_vert_halfwidth)) return fail(EFA_ERR_INVALID, "vertical localisation: null ob_vert/ob_vert_halfwidth");
  std::vector<double> v((size_t)(n_lead + 2 * P));
  bool any = false;
  for (long i = 0; i < n_lead; ++i) {
    if (std::isinf(lead_vert[i])) return fail(EFA_ERR_INVALID, "vertical localisation: slab %ld has an infinite coordinate", i);
    v[i] = lead_vert[i];
  }
  for (long k = 0; k < P; ++k) {
    const double z = ob_vert[k], h = ob_vert_halfwidth[k];
    if (std::isinf(z)) return fail(EFA_ERR_INVALID, "vertical localisation: observation %ld has an infinite coordinate", k);
    const bool none = std::isnan(z) || std::isnan(h);  // either missing: no vertical taper for this ob
    if (!none && !(std::isfinite(h) && h > 0.0))
      return fail(EFA_ERR_INVALID, "vertical localisation: observation %ld has half-width %g (must be finite and > 0, or NaN)", k, h);
    any = any || !none;
    v[n_lead + k] = none ? std::nan("") : z;
    v[n_lead + P + k] = none ? 1.0 : h;
  }
  if (c->vl_on && c->vl_nlead == n_lead && c->vl_P == P && std::memcmp(c->vl_host.data(), v.data(), v.size() * sizeof(double)) == 0)
    return EFA_OK;  // unchanged: nothing to copy, the geometry cache stays valid
  EFA_TRY(h2d(c, c->vl_dev, v.data(), v.size() * sizeof(double)));
  EFA_HIP(hipStreamSynchronize(c->stream));  // (v is gone on return)
  c->vl_host.swap(v);
  c->vl_nlead = n_lead;
  c->vl_P = P;
  c->vl_on = true;
  c->vl_any = any;
  c->vl_serial++;
  return EFA_OK;
}

int efa_ctx_set_outlier_threshold(efa_ctx* c, double threshold) {
  EFA_TRY(use(c));
  if (!std::isfinite(threshold) || threshold < 0.0)
    return fail(EFA_ERR_INVALID, "outlier threshold %g must be a finite number >= 0 (0: off)", threshold);
  c->qc_threshold = threshold;
  return EFA_OK;
}

int efa_inflate_rows_dev(efa_ctx* c, long rows, int M, double* X_dev, const double* field_dev) {
  EFA_TRY(use(c));
  if (rows < 0 || M < 1 || M > efa::kMaxMembers) return fail(EFA_ERR_INVALID, "efa_inflate_rows_dev: bad shape rows=%ld M=%d", rows, M);
  if (rows && (!X_dev || !field_dev)) return fail(EFA_ERR_INVALID, "null pointer");
  EFA_HIP(efa::launch_inflate_rows(rows, M, X_dev, field_dev, c->stream));
  return EFA_OK;
}

int efa_ctx_get_option(efa_ctx* c, const char* key, long* value) {
  EFA_TRY(use(c));
  if (!key || !value) return fail(EFA_ERR_INVALID, "null argument");
  if (!strcmp(key, "obs_batch")) *value = c->obs_batch;
  else if (!strcmp(key, "path")) *value = c->path;
  else if (!strcmp(key, "timing")) *value = c->timing;
  else if (!strcmp(key, "gram")) *value = c->use_gram;
  else if (!strcmp(key, "pipeline")) *value = c->use_pipeline;
  else if (!strcmp(key, "gc_onepass")) *value = c->gc_onepass;
  else if (!strcmp(key, "geometry_reuse")) *value = c->geometry_reuse;
  else if (!strcmp(key, "gc_active_pairs")) {
    EFA_TRY(read_gc_pairs(c));
    *value = c->gc_active_pairs;
  }
  else if (!strcmp(key, "spin_limit")) *value = c->spin_limit;
  else if (!strcmp(key, "spin_ms")) *value = c->spin_ms;
  else if (!strcmp(key, "cu_count")) *value = c->cu_count;
  else if (!strcmp(key, "phase_a_kind")) *value = c->phase_a_kind;
  else if (!strcmp(key, "pipe_dbg_addr")) *value = (long)reinterpret_cast<uintptr_t>(c->dbg.p);
  else if (!strcmp(key, "traj_addr")) *value = (long)reinterpret_cast<uintptr_t>(c->traj.p);  // (diagnostic tools only)
  else if (!strcmp(key, "device")) *value = c->device;
  else if (!strcmp(key, "stream_chunks")) *value = c->st.chunks;  // the last efa_ensrf_cycle_host (efa_stream.hip)
  else if (!strcmp(key, "stream_peak_bytes")) *value = c->st.peak_bytes;
  else if (!strcmp(key, "stream_h2d_us")) *value = c->st.h2d_us;
  else if (!strcmp(key, "stream_d2h_us")) *value = c->st.d2h_us;
  else if (!strcmp(key, "stream_wall_us")) *value = c->st.wall_us;
  else return fail(EFA_ERR_INVALID, "unknown option '%s'", key);
  return EFA_OK;
}

int efa_ctx_synchronize(efa_ctx* c) {
  EFA_TRY(use(c));
  EFA_HIP(hipStreamSynchronize(c->stream));
  return EFA_OK;
}

int efa_malloc(efa_ctx* c, size_t bytes, void** dev_out) {
  EFA_TRY(use(c));
  if (!dev_out) return fail(EFA_ERR_INVALID, "null out pointer");
  *dev_out = nullptr;
  EFA_HIP(hipMalloc(dev_out, bytes ? bytes : 8));
  return EFA_OK;
}

int efa_free(efa_ctx* c, void* dev) {
  EFA_TRY(use(c));
  if (dev) EFA_HIP(hipFree(dev));
  return EFA_OK;
}

int efa_memcpy_h2d(efa_ctx* c, void* dst_dev, const void* src, size_t bytes) {
  EFA_TRY(use(c));
  if (bytes) {
    EFA_HIP(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, c->stream));
    EFA_HIP(hipStreamSynchronize(c->stream));
  }
  return EFA_OK;
}

int efa_memcpy_d2h(efa_ctx* c, void* dst, const void* src_dev, size_t bytes) {
  EFA_TRY(use(c));
  if (bytes) {
    EFA_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    EFA_HIP(hipStreamSynchronize(c->stream));
  }
  return EFA_OK;
}

int efa_memcpy_d2d(efa_ctx* c, void* dst_dev, const void* src_dev, size_t bytes) {
  EFA_TRY(use(c));
  if (bytes) EFA_HIP(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, c->stream));
  return EFA_OK;
}

int efa_form_perts_dev(efa_ctx* c, long rows, int M, const double* X_dev, double scale, double* xm_dev,
                       double* Xp_dev) {
  EFA_TRY(use(c));
  if (rows < 0 || M < 1 || M > efa::kMaxMembers) return fail(EFA_ERR_INVALID, "bad shape rows=%ld M=%d", rows, M);
  if (rows && (!X_dev || !xm_dev || !Xp_dev)) return fail(EFA_ERR_INVALID, "null pointer");
  EFA_HIP(efa::launch_form_perts(rows, M, X_dev, scale, xm_dev, Xp_dev, c->stream));
  return EFA_OK;
}

int efa_posterior_dev(efa_ctx* c, long rows, int M, const double* xm_dev, const double* Xp_dev, double* post_dev) {
  EFA_TRY(use(c));
  if (rows < 0 || M < 1) return fail(EFA_ERR_INVALID, "bad shape rows=%ld M=%d", rows, M);
  if (rows && (!xm_dev || !Xp_dev || !post_dev)) return fail(EFA_ERR_INVALID, "null pointer");
  EFA_HIP(efa::launch_posterior(rows, M, xm_dev, Xp_dev, post_dev, c->stream));
  return EFA_OK;
}

int efa_forward_stencil_dev(efa_ctx* c, long rows, long row_offset, int M, const double* X_dev, long P, int npt,
                            const int64_t* idx, const double* wts, double* HX_dev) {
  EFA_TRY(use(c));
  if (rows < 0 || M < 1 || P < 0 || npt < 1) return fail(EFA_ERR_INVALID, "bad shape");
  if (P == 0) return EFA_OK;
  if (!X_dev || !idx || !wts || !HX_dev) return fail(EFA_ERR_INVALID, "null pointer");
  // staging of the stencil in grow-only context buffers (a hipMalloc/hipFree pair per call costs more than the kernel)
  // The caller's arrays are copied into pinned memory (free to be reused on return) and go to the device as ONE
  // asynchronous copy: no stream synchronisation here.  The pinned image is reused by the next call, which first waits
  // for this copy's event (long complete by then).
  const size_t n = (size_t)P * npt;
  const size_t half = (n * sizeof(int64_t) + 255) & ~(size_t)255;
  EFA_TRY(c->fs_idx.reserve(2 * half));
  EFA_TRY(c->pin_fs.reserve(2 * half));
  if (!c->ev_fs) EFA_HIP(hipEventCreateWithFlags(&c->ev_fs.h, hipEventDisableTiming));
  else EFA_HIP(hipEventSynchronize(c->ev_fs));
  // A fixed observing network hands over the same stencil cycle after cycle: when the pinned image still holds exactly these
  // indices and weights, the device copy made from it is current and nothing is copied (the copy itself is 8 us at 1e4 obs, but
  // a copy between two kernels idles the stream for ~10 us on either side).
  char* pin = static_cast<char*>(c->pin_fs.p);
  const bool same = c->fs_valid_n == n && c->fs_valid_dev == c->fs_idx.p && c->fs_valid_pin == c->pin_fs.p && std::memcmp(pin, idx, n * sizeof(int64_t)) == 0 &&
                    std::memcmp(pin + half, wts, n * sizeof(double)) == 0;
  if (!same) {
    std::memcpy(pin, idx, n * sizeof(int64_t));
    std::memcpy(pin + half, wts, n * sizeof(double));
    EFA_HIP(hipMemcpyAsync(c->fs_idx.p, c->pin_fs.p, half + n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    EFA_HIP(hipEventRecord(c->ev_fs, c->stream));
    c->fs_valid_n = n;
    c->fs_valid_dev = c->fs_idx.p;
    c->fs_valid_pin = c->pin_fs.p;
  }
  EFA_HIP(efa::launch_forward_stencil(rows, row_offset, M, X_dev, P, npt, c->fs_idx.as<int64_t>(),
                                      reinterpret_cast<const double*>(static_cast<const char*>(c->fs_idx.p) + half), HX_dev,
                                      c->stream));
  return EFA_OK;
}

int efa_interp_stencils(efa_ctx* c, int nvar, int nt, int ny, int nx, int latlon_1d, long n_grid, const double* grid_lat,
                        const double* grid_lon, const double* valid_times, long P, const int32_t* ob_var,
                        const double* ob_time, const double* ob_lat, const double* ob_lon, int64_t* sten_idx,
                        double* sten_wts, uint8_t* ob_status) {
  EFA_TRY(use(c));
  c->f_P = 0;
  if (nvar < 1 || nt < 1 || ny < 1 || nx < 1 || n_grid < 1 || P < 0)
    return fail(EFA_ERR_INVALID, "efa_interp_stencils: bad shape nvar=%d nt=%d ny=%d nx=%d n_grid=%ld P=%ld", nvar, nt, ny, nx, n_grid, P);
  if (!latlon_1d && n_grid != (long)ny * nx)
    return fail(EFA_ERR_INVALID, "efa_interp_stencils: 2-D lat/lon need n_grid = ny*nx = %ld, got %ld", (long)ny * nx, n_grid);
  if (P == 0) return EFA_OK;
  if (!grid_lat || !grid_lon || !valid_times || !ob_var || !ob_time || !ob_lat || !ob_lon)
    return fail(EFA_ERR_INVALID, "efa_interp_stencils: null input array");
  for (int i = 1; i < nt; ++i)
    if (!(valid_times[i] > valid_times[i - 1])) return fail(EFA_ERR_INVALID, "efa_interp_stencils: valid_times must ascend");
  const size_t dG = (size_t)n_grid * sizeof(double), dP = (size_t)P * sizeof(double);
  EFA_TRY(h2d(c, c->f_glat, grid_lat, dG));
  EFA_TRY(h2d(c, c->f_glon, grid_lon, dG));
  EFA_TRY(h2d(c, c->f_valids, valid_times, (size_t)nt * sizeof(double)));
  EFA_TRY(h2d(c, c->f_var, ob_var, (size_t)P * sizeof(int32_t)));
  EFA_TRY(h2d(c, c->f_time, ob_time, dP));
  EFA_TRY(h2d(c, c->f_lat, ob_lat, dP));
  EFA_TRY(h2d(c, c->f_lon, ob_lon, dP));
  EFA_TRY(c->f_sl.reserve(dG));
  EFA_TRY(c->f_cl.reserve(dG));
  EFA_TRY(c->f_near.reserve((size_t)P * 4 * sizeof(long)));
  EFA_TRY(c->f_idx.reserve((size_t)P * 8 * sizeof(long)));
  EFA_TRY(c->f_wts.reserve((size_t)P * 8 * sizeof(double)));
  EFA_TRY(c->f_status.reserve((size_t)P));
  efa::InterpArgs a{};
  a.P = P;
  a.nvar = nvar;
  a.nt = nt;
  a.ny = ny;
  a.nx = nx;
  a.latlon_1d = latlon_1d ? 1 : 0;
  a.n_grid = n_grid;
  a.glat = c->f_glat.as<double>();
  a.glon = c->f_glon.as<double>();
  a.sl = c->f_sl.as<double>();
  a.cl = c->f_cl.as<double>();
  a.valids = c->f_valids.as<double>();
  a.ob_var = c->f_var.as<int>();
  a.ob_time = c->f_time.as<double>();
  a.ob_lat = c->f_lat.as<double>();
  a.ob_lon = c->f_lon.as<double>();
  a.nearest = c->f_near.as<long>();
  a.sten_idx = c->f_idx.as<long>();
  a.sten_wts = c->f_wts.as<double>();
  a.status = c->f_status.as<unsigned char>();
  hipStream_t s = c->stream;
  EFA_HIP(efa::launch_interp_stencils(a, s));
  if (sten_idx) EFA_HIP(hipMemcpyAsync(sten_idx, c->f_idx.p, (size_t)P * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  if (sten_wts) EFA_HIP(hipMemcpyAsync(sten_wts, c->f_wts.p, (size_t)P * 8 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (ob_status) EFA_HIP(hipMemcpyAsync(ob_status, c->f_status.p, (size_t)P, hipMemcpyDeviceToHost, s));
  EFA_HIP(hipStreamSynchronize(s));  // the caller may reuse its input arrays on return
  c->f_P = P;
  return EFA_OK;
}

int efa_forward_interp_dev(efa_ctx* c, long ncol, long col_lo, long col_hi, long n_lead, int M, const double* X_dev,
                           double* HX_dev) {
  EFA_TRY(use(c));
  if (c->f_P <= 0) return fail(EFA_ERR_INVALID, "efa_forward_interp_dev called before efa_interp_stencils");
  if (ncol < 1 || col_lo < 0 || col_hi > ncol || col_lo > col_hi || n_lead < 1 || M < 1)
    return fail(EFA_ERR_INVALID, "efa_forward_interp_dev: bad shard [%ld,%ld) of %ld columns, n_lead=%ld, M=%d", col_lo, col_hi, ncol, n_lead, M);
  if (!X_dev || !HX_dev) return fail(EFA_ERR_INVALID, "null pointer");
  EFA_HIP(efa::launch_forward_cols(ncol, col_lo, col_hi, n_lead, M, X_dev, c->f_P, 8, c->f_idx.as<long>(), c->f_wts.as<double>(),
                                   HX_dev, c->stream));
  return EFA_OK;
}

int efa_obs_phase_dev(efa_ctx* c, int M, long P, double* ym_dev, double* Yp_dev, const double* ob_value,
                      const double* ob_error, const uint8_t* ob_assim, int loc_mode, const double* ob_lat,
                      const double* ob_lon, const double* ob_halfwidth_km, double* prior_mean, double* prior_var,
                      double* post_mean, double* post_var, uint8_t* assimilated) {
  EFA_TRY(use(c));
  return obs_phase(c, M, P, ym_dev, Yp_dev, ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon, ob_halfwidth_km,
                   prior_mean, prior_var, post_mean, post_var, assimilated);
}

int efa_state_phase_dev(efa_ctx* c, long rows, int M, const double* xm_in_dev, const double* Xp_in_dev,
                        double* xm_out_dev, double* Xp_out_dev, const double* grid_lat, const double* grid_lon,
                        long ncol, long n_lead) {
  EFA_TRY(use(c));
  return state_phase(c, rows, M, xm_in_dev, Xp_in_dev, xm_out_dev, Xp_out_dev, grid_lat, grid_lon, ncol, n_lead);
}

int efa_state_cycle_dev(efa_ctx* c, long rows, int M, const double* X_dev, double* post_dev, const double* grid_lat,
                        const double* grid_lon, long ncol, long n_lead) {
  EFA_TRY(use(c));
  if (!c->have_traj) return fail(EFA_ERR_INVALID, "efa_state_cycle_dev called before efa_obs_phase_dev");
  if (M != c->M) return fail(EFA_ERR_INVALID, "M=%d differs from the obs phase's M=%d", M, c->M);
  EFA_TRY(check_adaptive(c, c->loc_mode, rows));
  EFA_TRY(check_vloc(c, c->loc_mode, c->P, n_lead));
  reset_state_phase(c);
  if (rows <= 0) return rows == 0 ? EFA_OK : fail(EFA_ERR_INVALID, "negative row count");
  if (!X_dev || !post_dev) return fail(EFA_ERR_INVALID, "null state pointer");
  EFA_TRY(begin_state_work(c, grid_lat, grid_lon, ncol, n_lead, rows));
  hipStream_t s = c->stream;
  if (c->P > 0 && c->n_active > 0 && want_transform(c, true)) {
    EFA_TRY(transform_with_relaxation(c, carried_transform(c, X_dev, nullptr, post_dev, nullptr, rows, 1), &c->state_launches));
    c->path_taken = EFA_PATH_TRANSFORM;
  } else if (c->loc_mode == EFA_LOC_GC && c->gc_onepass && c->n_active > 0) {
    // localised: prior members -> posterior members in one read + one write of the state
    EFA_TRY(with_relaxation(c, rows, M, X_dev, post_dev, &c->state_launches,
                            [&] { return state_gc_onepass(c, nullptr, X_dev, nullptr, post_dev, ncol, n_lead, 1); }));
  } else {
    EFA_TRY(with_relaxation(c, rows, M, X_dev, post_dev, &c->state_launches, [&]() -> int {
      EFA_TRY(c->xm_ws.reserve((size_t)rows * sizeof(double)));
      double* xm = c->xm_ws.as<double>();
      EFA_HIP(efa::launch_form_perts(rows, M, X_dev, 1.0, xm, post_dev, s));
      EFA_TRY(state_sweeps(c, rows, xm, post_dev, xm, post_dev, ncol));
      EFA_HIP(efa::launch_posterior(rows, M, xm, post_dev, post_dev, s));
      return EFA_OK;
    }));
  }
  return finish_state_timing(c, s);
}

int efa_ensrf_update_dev(efa_ctx* c, long rows, int M, long P, double* xm_dev, double* Xp_dev, double* ym_dev,
                         double* Yp_dev, const double* ob_value, const double* ob_error, const uint8_t* ob_assim,
                         int loc_mode, const double* ob_lat, const double* ob_lon, const double* ob_halfwidth_km,
                         const double* grid_lat, const double* grid_lon, long ncol, long n_lead, double* prior_mean,
                         double* prior_var, double* post_mean, double* post_var, uint8_t* assimilated) {
  EFA_TRY(use(c));
  EFA_TRY(check_adaptive(c, loc_mode, rows));
  EFA_TRY(check_vloc(c, loc_mode, P, n_lead));
  EFA_TRY(obs_phase(c, M, P, ym_dev, Yp_dev, ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon,
                    ob_halfwidth_km, prior_mean, prior_var, post_mean, post_var, assimilated));
  EFA_TRY(state_phase(c, rows, M, xm_dev, Xp_dev, xm_dev, Xp_dev, grid_lat, grid_lon, ncol, n_lead));
  EFA_HIP(hipStreamSynchronize(c->stream));
  return EFA_OK;
}

int efa_ensrf_cycle_dev(efa_ctx* c, long rows, int M, long P, const double* X_dev, double* post_dev, double* ym_dev,
                        double* Yp_dev, int obs_block_out, const double* ob_value, const double* ob_error,
                        const uint8_t* ob_assim, int loc_mode, const double* ob_lat, const double* ob_lon,
                        const double* ob_halfwidth_km, const double* grid_lat, const double* grid_lon, long ncol, long n_lead,
                        double* prior_mean, double* prior_var, double* post_mean, double* post_var, uint8_t* assimilated) {
  EFA_TRY(use(c));
  if (rows < 0) return fail(EFA_ERR_INVALID, "negative row count");
  if (rows > 0 && (!X_dev || !post_dev)) return fail(EFA_ERR_INVALID, "null state pointer");
  EFA_TRY(check_adaptive(c, loc_mode, rows));
  EFA_TRY(check_vloc(c, loc_mode, P, n_lead));
  // Phase B may go into the stream before Phase A's status is known only if a wrong guess cannot cost the prior:
  // separate prior and posterior buffers (a redone Phase A needs the transform run again on the untouched prior)
  const char* xb = reinterpret_cast<const char*>(X_dev);
  const char* pb = reinterpret_cast<const char*>(post_dev);
  const size_t bytes = (size_t)rows * (size_t)(M > 0 ? M : 0) * sizeof(double);
  const bool disjoint = rows > 0 && (xb + bytes <= pb || pb + bytes <= xb);
  c->spec = efa_ctx::Spec{};
  c->spec.armed = true;
  c->spec.obs_out = obs_block_out != 0;
  c->spec.X = X_dev;
  c->spec.post = post_dev;
  c->spec.rows = (disjoint && loc_mode == EFA_LOC_NONE) ? rows : 0;  // 0: armed only for the optional obs-block copy
  {
    const int rg = prepare_grid_early(c, loc_mode, grid_lat, grid_lon, ncol, n_lead, rows);
    if (rg != EFA_OK) {
      c->spec = efa_ctx::Spec{};
      return rg;
    }
  }
  const int rc = obs_phase(c, M, P, ym_dev, Yp_dev, ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon, ob_halfwidth_km,
                           prior_mean, prior_var, post_mean, post_var, assimilated);
  const bool launched = c->spec.launched;
  const int pair = c->spec.pair;
  const long spec_launches = c->spec.launches;
  c->spec = efa_ctx::Spec{};
  if (rc != EFA_OK) {
    c->grid_ready = false;
    return rc;
  }
  // Phase B is in the stream already, behind the launch that turned out fine -- unless the outlier check rejected so many obs
  // that the state phase would not take the transform (none left, or "auto" with fewer): then it runs as it would have, over the
  // speculative posterior (the prior is untouched)
  if (launched && c->n_active > 0 && want_transform(c, true)) {
    c->state_ms = 0.0;
    c->state_launches = spec_launches;
    c->state_launches_sum += spec_launches;
    c->path_taken = EFA_PATH_TRANSFORM;
    if (c->timing) {
      (pair ? c->state_ms_pending2 : c->state_ms_pending) = true;
      if (c->timing == 1) harvest_state_pair(c, pair);
    }
    return EFA_OK;
  }
  return efa_state_cycle_dev(c, rows, M, X_dev, post_dev, grid_lat, grid_lon, ncol, n_lead);
}

int efa_ensrf_update(efa_ctx* c, long A, long N, int M, long P, double* xbm, double* Xbp, const double* ob_value,
                     const double* ob_error, const uint8_t* ob_assim, int loc_mode, const double* ob_lat,
                     const double* ob_lon, const double* ob_halfwidth_km, const double* grid_lat,
                     const double* grid_lon, long ncol, long n_lead, double* prior_mean, double* prior_var,
                     double* post_mean, double* post_var, uint8_t* assimilated) {
  EFA_TRY(use(c));
  if (N < 0 || P < 0 || A != N + P) return fail(EFA_ERR_INVALID, "A=%ld must equal N+P=%ld+%ld", A, N, P);
  EFA_TRY(check_common(M, P));
  if (A && (!xbm || !Xbp)) return fail(EFA_ERR_INVALID, "null xbm/Xbp");
  const size_t rowb = (size_t)M * sizeof(double);
  EFA_TRY(c->h_xm.reserve((size_t)(N ? N : 1) * sizeof(double)));
  EFA_TRY(c->h_Xp.reserve((size_t)(N ? N : 1) * rowb));
  EFA_TRY(c->h_ym.reserve((size_t)(P ? P : 1) * sizeof(double)));
  EFA_TRY(c->h_Yp.reserve((size_t)(P ? P : 1) * rowb));
  hipStream_t s = c->stream;
  if (N) {
    EFA_HIP(hipMemcpyAsync(c->h_xm.p, xbm, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemcpyAsync(c->h_Xp.p, Xbp, (size_t)N * rowb, hipMemcpyHostToDevice, s));
  }
  if (P) {
    EFA_HIP(hipMemcpyAsync(c->h_ym.p, xbm + N, (size_t)P * sizeof(double), hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemcpyAsync(c->h_Yp.p, Xbp + (size_t)N * M, (size_t)P * rowb, hipMemcpyHostToDevice, s));
  }
  EFA_TRY(efa_ensrf_update_dev(c, N, M, P, c->h_xm.as<double>(), c->h_Xp.as<double>(), c->h_ym.as<double>(),
                               c->h_Yp.as<double>(), ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon,
                               ob_halfwidth_km, grid_lat, grid_lon, ncol, n_lead, prior_mean, prior_var, post_mean,
                               post_var, assimilated));
  if (N) {
    EFA_HIP(hipMemcpyAsync(xbm, c->h_xm.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
    EFA_HIP(hipMemcpyAsync(Xbp, c->h_Xp.p, (size_t)N * rowb, hipMemcpyDeviceToHost, s));
  }
  if (P) {
    EFA_HIP(hipMemcpyAsync(xbm + N, c->h_ym.p, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, s));
    EFA_HIP(hipMemcpyAsync(Xbp + (size_t)N * M, c->h_Yp.p, (size_t)P * rowb, hipMemcpyDeviceToHost, s));
  }
  EFA_HIP(hipStreamSynchronize(s));
  return EFA_OK;
}

int efa_cov_contract_f32_dev(efa_ctx* c, long N, int M, long P, const float* Xbp_f32_dev, const float* Ye_f32_dev,
                             float* C_f32_dev) {
  EFA_TRY(use(c));
  if (N < 0 || P < 0 || M < 4 || (M & 3) != 0)
    return fail(EFA_ERR_INVALID, "efa_cov_contract_f32_dev: need N,P >= 0 and M a positive multiple of 4 (M=%d)", M);
  if (N == 0 || P == 0) return EFA_OK;
  if (!Xbp_f32_dev || !Ye_f32_dev || !C_f32_dev) return fail(EFA_ERR_INVALID, "null pointer");
  if ((reinterpret_cast<uintptr_t>(Xbp_f32_dev) & 15u) || (reinterpret_cast<uintptr_t>(Ye_f32_dev) & 15u))
    return fail(EFA_ERR_INVALID, "operands must be 16-byte aligned");
  EFA_HIP(efa::launch_contract_f32(N, M, P, Xbp_f32_dev, Ye_f32_dev, C_f32_dev, c->stream));
  return EFA_OK;
}

int efa_last_timing(efa_ctx* c, double* state_ms, double* obs_ms, long* state_launches, int* path_taken) {
  if (!c) return fail(EFA_ERR_INVALID, "null context");
  harvest_obs_ms(c);
  harvest_state_ms(c);
  if (c->timing == 2) {  // deferred: the sums over the calls since the previous efa_last_timing
    if (state_ms) *state_ms = c->state_ms_sum;
    if (obs_ms) *obs_ms = c->obs_ms_sum;
    if (state_launches) *state_launches = c->state_launches_sum;
    c->state_ms_sum = c->obs_ms_sum = 0.0;
    c->state_launches_sum = 0;
  } else {
    if (state_ms) *state_ms = c->state_ms;
    if (obs_ms) *obs_ms = c->obs_ms;
    if (state_launches) *state_launches = c->state_launches;
  }
  if (path_taken) *path_taken = c->path_taken;
  return EFA_OK;
}

int efa_fill_synthetic_dev(efa_ctx* c, long rows, long row_offset, int M, uint64_t seed, double sigma,
                           double* X_dev) {
  EFA_TRY(use(c));
  if (rows < 0 || M < 1) return fail(EFA_ERR_INVALID, "bad shape");
  if (rows && !X_dev) return fail(EFA_ERR_INVALID, "null pointer");
  EFA_HIP(efa::launch_fill_synthetic(rows, row_offset, M, seed, sigma, X_dev, c->stream));
  return EFA_OK;
}

// ---- the one exchange step, owned by the library ------------------------------------------
int efa_comm_unique_id(uint8_t* id_out) {
  if (!id_out) return fail(EFA_ERR_INVALID, "null id");
  EFA_TRY(rccl_load());
  static_assert(sizeof(ncclUniqueId) == EFA_COMM_ID_BYTES, "EFA_COMM_ID_BYTES must be sizeof(ncclUniqueId)");
  ncclUniqueId id;
  EFA_RCCL(g_rccl.GetUniqueId(&id));
  std::memcpy(id_out, &id, sizeof(id));
  return EFA_OK;
}

int efa_comm_init(efa_ctx* c, const uint8_t* id, int rank, int world) {
  EFA_TRY(use(c));
  if (!id || world < 1 || rank < 0 || rank >= world) return fail(EFA_ERR_INVALID, "bad communicator arguments (rank %d of %d)", rank, world);
  if (c->comm) return fail(EFA_ERR_INVALID, "the context already owns a communicator (efa_comm_destroy first)");
  EFA_TRY(rccl_load());
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  EFA_RCCL(g_rccl.CommInitRank(&c->comm, world, uid, rank));
  c->comm_rank = rank;
  c->comm_world = world;
  return EFA_OK;
}

int efa_comm_destroy(efa_ctx* c) {
  EFA_TRY(use(c));
  if (!c->comm) return EFA_OK;
  EFA_HIP(hipStreamSynchronize(c->stream));
  EFA_RCCL(g_rccl.CommDestroy(c->comm));
  c->comm = nullptr;
  c->comm_rank = 0;
  c->comm_world = 1;
  return EFA_OK;
}

int efa_allreduce_sum_dev(efa_ctx* c, double* buf_dev, long count) {
  EFA_TRY(use(c));
  if (count < 0 || (count && !buf_dev)) return fail(EFA_ERR_INVALID, "bad buffer");
  if (!c->comm) return fail(EFA_ERR_INVALID, "no communicator: call efa_comm_init first");
  if (count == 0) return EFA_OK;
  EFA_RCCL(g_rccl.AllReduce(buf_dev, buf_dev, (size_t)count, ncclDouble, ncclSum, c->comm, c->stream));
  return EFA_OK;
}

// ---- cost of a column block under Gaspari-Cohn localisation (the sharding plan of SURVEY.md 8e) ------------
int efa_gc_block_counts(efa_ctx* c, long ncol, const double* grid_lat, const double* grid_lon, long P, const double* ob_lat,
                        const double* ob_lon, const double* ob_halfwidth_km, const uint8_t* ob_assim, int32_t* block_count,
                        int32_t* block_pairs, uint64_t* active_pairs) {
  EFA_TRY(use(c));
  if (ncol <= 0 || P < 0) return fail(EFA_ERR_INVALID, "bad shape");
  if (!grid_lat || !grid_lon || !block_count || (P && (!ob_lat || !ob_lon || !ob_halfwidth_km || !ob_assim)))
    return fail(EFA_ERR_INVALID, "null pointer");
  const long nblk = efa::gc_num_blocks(ncol);
  hipStream_t s = c->stream;
  std::vector<double> coef((size_t)(P ? P : 1) * efa::kCoefStride, 0.0), hw((size_t)(P ? P : 1), 1.0);
  for (long k = 0; k < P; ++k) {
    const bool on = ob_assim[k] != 0;
    coef[(size_t)k * efa::kCoefStride + 3] = on ? 1.0 : 0.0;
    if (on) {
      if (!(ob_halfwidth_km[k] == ob_halfwidth_km[k]) || ob_halfwidth_km[k] == 0.0)
        return fail(EFA_ERR_INVALID, "observation %ld: localize_radius must be a non-zero number", k);
      hw[k] = ob_halfwidth_km[k];
    }
  }
  EFA_TRY(h2d(c, c->gcc_lat, grid_lat, (size_t)ncol * sizeof(double)));
  EFA_TRY(h2d(c, c->gcc_lon, grid_lon, (size_t)ncol * sizeof(double)));
  EFA_TRY(h2d(c, c->gcc_oblat, ob_lat, (size_t)P * sizeof(double)));
  EFA_TRY(h2d(c, c->gcc_oblon, ob_lon, (size_t)P * sizeof(double)));
  EFA_TRY(h2d(c, c->gcc_obhw, hw.data(), (size_t)P * sizeof(double)));
  EFA_TRY(h2d(c, c->gcc_coef, coef.data(), (size_t)P * efa::kCoefStride * sizeof(double)));
  EFA_TRY(c->gcc_trig.reserve((size_t)(P ? P : 1) * 6 * sizeof(double)));
  EFA_TRY(c->gcc_cnt.reserve((size_t)2 * nblk * sizeof(int)));  // [counts | pairs]
  EFA_TRY(c->gcc_pairs.reserve(sizeof(unsigned long long)));
  EFA_HIP(hipMemsetAsync(c->gcc_pairs.p, 0, sizeof(unsigned long long), s));
  EFA_HIP(hipMemsetAsync(c->gcc_cnt.p, 0, (size_t)2 * nblk * sizeof(int), s));
  if (P > 0)
    EFA_HIP(efa::launch_gc_count(ncol, P, c->gcc_lat.as<double>(), c->gcc_lon.as<double>(), c->gcc_oblat.as<double>(),
                                 c->gcc_oblon.as<double>(), c->gcc_obhw.as<double>(), c->gcc_coef.as<double>(),
                                 c->gcc_trig.as<double>(), c->gcc_cnt.as<int>(), c->gcc_cnt.as<int>() + nblk,
                                 c->gcc_pairs.as<unsigned long long>(), s));
  unsigned long long pairs = 0;
  EFA_HIP(hipMemcpyAsync(block_count, c->gcc_cnt.p, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost, s));
  if (block_pairs)
    EFA_HIP(hipMemcpyAsync(block_pairs, c->gcc_cnt.as<int>() + nblk, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost, s));
  EFA_HIP(hipMemcpyAsync(&pairs, c->gcc_pairs.p, sizeof(pairs), hipMemcpyDeviceToHost, s));
  EFA_HIP(hipStreamSynchronize(s));
  if (active_pairs) *active_pairs = pairs;
  return EFA_OK;
}

}  // extern "C"
