// Phase A, the obs phase (efa_driver.h): the per-ob inputs staged, the block taken through the persistent kernels window by window
// (the per-batch kernels where those do not apply or give up), the records and diagnostics left for Phase B and the caller.
#include "efa_driver.h"

#include <array>
#include <cmath>
#include <cstring>

namespace efa_host {

using namespace efa;

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

int check_common(int M, long P) {
  if (M < 2) return fail(EFA_ERR_INVALID, "ensemble size M=%d must be >= 2 (covariance divides by M-1)", M);
  if (M > kMaxMembers) return fail(EFA_ERR_UNSUPPORTED, "ensemble size M=%d exceeds the built maximum %d", M, kMaxMembers);
  if (P < 0) return fail(EFA_ERR_INVALID, "negative observation count");
  return EFA_OK;
}

namespace {

// ---- Phase A ---------------------------------------------------------------
// One obs_phase call: its arguments and the workspace layout that the steps below share.
struct ObsCall {
  int M = 0;
  long P = 0;
  double *ym_dev = nullptr, *Yp_dev = nullptr;  // the caller's obs block
  ObsIn ob;      // the caller's per-ob arrays (host); stage_obs_inputs points ob.hw at the sanitised copy
  DiagOut diag;  // where the diagnostics go (host)
  SpecRequest spec;      // efa_ensrf_cycle_dev: the transform to put behind the launch (none by default)
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
// the diagnostics pack and the workspaces.  a.ob.hw comes back sanitised.
int stage_obs_inputs(efa_ctx* c, ObsCall& a) {
  const int M = a.M;
  const long P = a.P;
  const double *ob_value = a.ob.value, *ob_error = a.ob.error, *ob_lat = a.ob.lat, *ob_lon = a.ob.lon;
  const double*& ob_hw = a.ob.hw;
  const uint8_t* ob_assim = a.ob.assim;
  if (!a.ym_dev || !a.Yp_dev || !ob_value || !ob_error || !ob_assim)
    return fail(EFA_ERR_INVALID, "null observation array");
  if (a.ob.loc_mode == EFA_LOC_GC) {
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
  if (a.ob.loc_mode == EFA_LOC_GC) {
    const size_t nb8 = (size_t)P * sizeof(double);
    const bool same = (long)c->geo_lat.size() == P && std::memcmp(c->geo_lat.data(), ob_lat, nb8) == 0 &&
                      std::memcmp(c->geo_lon.data(), ob_lon, nb8) == 0 && std::memcmp(c->geo_hw.data(), ob_hw, nb8) == 0 &&
                      std::memcmp(c->geo_assim.data(), ob_assim, (size_t)P) == 0 && c->geo_vl_serial == c->vl_serial &&
                      c->geo_sl_serial == c->sl_serial;
    if (!same) {
      c->geo_vl_serial = c->vl_serial;  // (the vertical setting is part of the geometry: the obs-obs table carries its factor)
      c->geo_sl_serial = c->sl_serial;  // (and so is the slab setting)
      c->geo_lat.assign(ob_lat, ob_lat + P);
      c->geo_lon.assign(ob_lon, ob_lon + P);
      c->geo_hw.assign(ob_hw, ob_hw + P);     // (sanitised above)
      c->geo_assim.assign(ob_assim, ob_assim + P);
      c->geo_serial++;
    }
  }

  a.carry_T = (a.ob.loc_mode == EFA_LOC_NONE) && transform_supported(M) && (c->path != EFA_PATH_SWEEP);
  a.extra = a.carry_T ? M : 0;
  a.R = P + a.extra;
  const size_t dP = (size_t)P * sizeof(double);

  // per-ob inputs: [value | error | assim bytes | {error, sqrt(error), assimilate (1.0 / 0.0), 0} x P | lat | lon | halfwidth] in one
  // allocation, ONE H2D from pinned memory (the last three slots only with localisation); the four-double records are the band
  // leader's per-ob constants, fetched with wave-uniform loads
  {
    const bool gc = a.ob.loc_mode == EFA_LOC_GC;
    const size_t slot = ((size_t)P * sizeof(double) + 255) & ~(size_t)255;
    const size_t total = 10 * slot;
    EFA_TRY(c->ob_pack.reserve(total));
    EFA_TRY(c->pin_in.reserve(total));
    char* hb = static_cast<char*>(c->pin_in.p);
    char* db = static_cast<char*>(c->ob_pack.p);
    std::memcpy(hb + 2 * slot, ob_assim, (size_t)P);
    {
      // value and error of an ob that is not assimilated are not read (the reference skips it before it reads either,
      // ensrf.py:74-76; the Python front end passes NaN for a None): the device gets the neutral pair (0, 1) in their place, so
      // a kernel that gates the ob's gain with a zero factor never multiplies that zero by a NaN or an Inf
      double* hv = reinterpret_cast<double*>(hb);
      double* he = reinterpret_cast<double*>(hb + slot);
      double* ec = reinterpret_cast<double*>(hb + 3 * slot);
      for (long k = 0; k < P; ++k) {
        const bool on = ob_assim[k] != 0;
        hv[k] = on ? ob_value[k] : 0.0;
        he[k] = on ? ob_error[k] : 1.0;
        ec[4 * k] = he[k];
        ec[4 * k + 1] = on ? std::sqrt(he[k]) : 1.0;
        ec[4 * k + 2] = on ? 1.0 : 0.0;
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
  if (c->timing) EFA_HIP(hipEventRecord(c->obs_iv.begin, s));
  const long Wone = (long)kPipeMaxWGs * kPipeRowsPerWG - a.extra;           // one window covers the block up to here
  a.Wmax = (P <= Wone) ? Wone : Wone - a.extra;                              // else: two sets of extra rows per window
  // (the persistent leaders rest on a gain that is linear in the row, which the sampling error correction's is not: per-batch kernels)
  // (... and the batch solver walks no chain at all: no records, no status words)
  a.pipe_ok = c->use_pipeline && !c->obs_solver && !sec_active(c) && a.Wmax > 0 && pipeline_supported(M, (P <= Wone ? P + a.extra : a.Wmax + 2 * a.extra));
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
    if (a.ob.loc_mode == EFA_LOC_GC) {
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
  sw.taper_mode = (a.ob.loc_mode == EFA_LOC_GC) ? kTaperObs : kTaperNone;
  if (a.ob.loc_mode == EFA_LOC_GC && sl_active(c)) {  // ... times the temporal and variable factors, likewise
    const bool vert = vl_active(c);
    EFA_TRY(c->vl_W.reserve((size_t)nb * a.R * sizeof(double)));
    EFA_HIP(launch_obs_taper_rows_slab(b0, nb, a.R, a.P, c->ob_lat, c->ob_lon, c->ob_hw, vert ? vl_obvert(c) : nullptr,
                                       vert ? vl_obvhw(c) : nullptr, sl_obs(c, 0), c->vl_W.as<double>(), c->stream));
    sw.taper_mode = kTaperTable;
    sw.W = c->vl_W.as<double>();
    sw.ncol = a.R;
  } else if (a.ob.loc_mode == EFA_LOC_GC && vl_active(c)) {  // horizontal x vertical taper of the batch against every row, in table mode
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
  if (sec_active(c)) {  // (batch_window: one ob per batch)
    sw.sec_tab = c->sec_dev.as<double>();
    sw.sec_T = c->sec_T;
  }
  EFA_HIP(launch_sweep(sw, c->stream));
  return EFA_OK;
}

long active_in(const ObsCall& a, long b0, int nb) {
  long act = 0;
  for (int k = 0; k < nb; ++k) act += a.ob.assim[b0 + k] ? 1 : 0;
  return act;
}

// obs [w0, w1) by the per-batch kernels (k_diag on the batch's own rows, k_sweep on every other row of the block)
// (With vertical or slab localisation one ob per batch: k_diag's in-batch taper is horizontal only, and an ob's taper against itself
// is 1.  With the sampling error correction likewise: k_diag applies none, and an ob's factor against itself is 1)
int batch_window(efa_ctx* c, const ObsCall& a, long w0, long w1) {
  const long B = (a.ob.loc_mode == EFA_LOC_GC && (vl_active(c) || sl_active(c) || sec_active(c))) ? 1 : a.B;
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
    d.loc_mode = a.ob.loc_mode;
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
  pa.loc_mode = a.ob.loc_mode;
  pa.tw = nullptr;
  if (a.ob.loc_mode == EFA_LOC_GC) {
    EFA_TRY(c->tw_mat.reserve((size_t)Pw * Rw * sizeof(double)));
    EFA_TRY(c->gc_obtrig.reserve((size_t)Pw * 6 * sizeof(double)));
    const bool tw_ok = c->geometry_reuse && win.direct && c->tw_serial == c->geo_serial && c->tw_Pw == Pw && c->tw_Rw == Rw &&
                       c->tw_ptr == c->tw_mat.p;
    if (!tw_ok) {
      EFA_HIP(launch_obs_taper_matrix(Pw, Rw, c->ob_lat + w0, c->ob_lon + w0, c->ob_hw + w0, c->gc_obtrig.as<double>(),
                                      c->tw_mat.as<double>(), s));
      if (vl_active(c)) EFA_HIP(launch_obs_taper_vert(Pw, Rw, vl_obvert(c) + w0, vl_obvhw(c) + w0, c->tw_mat.as<double>(), s));
      if (sl_active(c)) EFA_HIP(launch_obs_taper_slab(Pw, Rw, sl_obs(c, w0), c->tw_mat.as<double>(), s));
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
  const bool band = c->use_gram >= 2 && pipeline_band_supported(a.M, Rw, a.ob.loc_mode);
  const bool gram = c->use_gram >= 1 && pipeline_gram_supported(a.M, Rw, a.ob.loc_mode);
  const int first = (band && layout != Records::kStandard) ? 4 : gram ? 3 : 1;
  if (layout == Records::kBand) return {first == 4 ? 4 : 0, 0};
  return {first, first == 1 ? 0 : 1};
}

// efa_ensrf_cycle_dev: the state transform goes into the stream behind the launch whose status is not known yet -- it reads
// [T | w] from the launch's working rows and writes only the caller's posterior; a launch that reports a fallback is redone
// and the transform enqueued again (by the caller), so a wrong guess costs time, never a result.  The device then runs
// Phase A -> Phase B with no host round trip in between.
int speculative_transform(efa_ctx* c, const ObsCall& a, const Window& win, SpecResult* out) {
  *out = SpecResult{};
  // the member form's plan as the state call will make it, with the transform this launch is about to leave
  const StateRows r{a.spec.X, a.spec.post, Elem::f64, a.spec.rows, a.M};
  const StatePlan plan = plan_state(c, true, r.elem, false, a.carry_T);
  if (!(a.spec.rows > 0 && win.direct && plan.route == Route::transform)) return EFA_OK;
  hipStream_t s = c->stream;
  Interval& iv = c->state_iv[c->state_iv[0].pending ? 1 : 0];
  if (c->timing) harvest_state_interval(c, iv);  // (both intervals unread cannot happen across the wait below; kept correct anyway)
  // ONE event between Phase A and the transform (each record idles the stream ~6 us): the status words and diagnostics are on
  // the host -- what the host waits for -- the obs interval ends and this state interval begins
  EFA_HIP(hipEventRecord(iv.begin, s));
  c->obs_ends_at = iv.begin;
  EFA_TRY(run_state_plan(c, plan, r, nullptr, nullptr, 0, 0, &out->launches));
  if (c->timing) EFA_HIP(hipEventRecord(iv.end, s));
  out->interval = &iv;
  out->launched = true;
  return EFA_OK;
}

// ONE host round trip per launch: the status words and -- when this launch is the whole Phase A -- the diagnostics it wrote come
// back together, into pinned memory (a second copy + synchronise after the status was known left the device idle for ~40 us
// before Phase B; a pageable destination made the status copy itself a staged one).  *st: the status words on the host.
int launch_round_trip(efa_ctx* c, const ObsCall& a, const Window& win, const int** st_out, SpecResult* spec) {
  hipStream_t s = c->stream;
  int* st = reinterpret_cast<int*>(static_cast<char*>(c->pin_out.p) + 5 * a.oslot - 64);
  if (win.direct) EFA_HIP(launch_results_to_host(c->out_pack.p, c->pin_out.p, 4 * a.oslot + (size_t)a.P, c->status.as<int>(), st, s));
  else EFA_HIP(hipMemcpyAsync(st, c->status.p, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
  EFA_TRY(speculative_transform(c, a, win, spec));
  if (spec->launched) EFA_HIP(hipEventSynchronize(spec->interval->begin));  // (not the stream: the transform behind it is to run while the host goes on)
  else EFA_HIP(hipStreamSynchronize(s));
  if (spec->launched && c->timing) harvest_state_ms(c);  // the previous cycle's interval: complete by now (this one is not pending yet)
  *st_out = st;
  return EFA_OK;
}

// One window through the persistent kernels.  *kind_out: the kind that did it, or 0 -- fall back to the per-batch kernels;
// *spec_out: the speculative transform behind that launch, if one was placed.
// A failed attempt (bounded spin expired, or the Gram downdate's cancellation guard) may have let finished workgroups write
// their rows back, so the launch's rows are restored before anything else runs on them.  An attempt is skipped when its grid
// cannot be co-resident (occupancy query in the launcher), and after an attempt whose bounded spins EXPIRED (some workgroups
// never became resident, e.g. another kernel holds CUs) no other persistent kernel is tried: they have the same residency need.
int try_persistent_window(efa_ctx* c, const ObsCall& a, Window& win, Records layout, bool& status_clear, int* kind_out,
                          SpecResult* spec_out) {
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
    SpecResult spec;
    EFA_TRY(launch_round_trip(c, a, win, &st, &spec));
    if (st[0] == 0 && st[1] == 0) {
      *kind_out = kind;
      *spec_out = spec;
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
      EFA_HIP(launch_transform(t, Elem::f64, s));
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
int finish_obs_phase(efa_ctx* c, const ObsCall& a, Records layout, bool diag_on_host, const SpecResult& spec) {
  hipStream_t s = c->stream;
  const DiagOut& o = a.diag;
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
  if (a.spec.obs_out) {
    EFA_HIP(hipMemcpyAsync(a.Yp_dev, a.Yw, (size_t)P * a.M * sizeof(double), hipMemcpyDeviceToDevice, s));
    EFA_HIP(hipMemcpyAsync(a.ym_dev, a.ymw, dP, hipMemcpyDeviceToDevice, s));
  }
  if (c->timing && !spec.launched) {  // (behind a speculative transform the interval ended at the event in front of it)
    EFA_HIP(hipEventRecord(c->obs_iv.end, s));
    c->obs_ends_at = c->obs_iv.end;
  }
  if (!diag_on_host) {
    EFA_HIP(hipMemcpyAsync(c->pin_out.p, c->out_pack.p, 4 * oslot + (size_t)P, hipMemcpyDeviceToHost, s));
    EFA_HIP(hipStreamSynchronize(s));
  }
  const char* hb = static_cast<const char*>(c->pin_out.p);
  if (o.prior_mean) std::memcpy(o.prior_mean, hb, dP);
  if (o.prior_var) std::memcpy(o.prior_var, hb + oslot, dP);
  const double* pm = reinterpret_cast<const double*>(hb + 2 * oslot);
  const double* pv = reinterpret_cast<const double*>(hb + 3 * oslot);
  const uint8_t* as = reinterpret_cast<const uint8_t*>(hb + 4 * oslot);
  for (long k = 0; k < P; ++k) {
    if (o.assimilated) o.assimilated[k] = as[k];
    if (as[k]) {
      if (o.post_mean) o.post_mean[k] = pm[k];
      if (o.post_var) o.post_var[k] = pv[k];
    }
  }
  if (c->qc_used) {  // the outlier check may have rejected obs: the state phase goes by the flags Phase A went by
    c->n_active = 0;
    for (long k = 0; k < P; ++k) {
      c->h_assim[k] = as[k] ? 1 : 0;
      c->n_active += as[k] ? 1 : 0;
    }
  }
  if (c->timing) c->obs_iv.pending = true;  // read in efa_last_timing: the copies back to the caller's block may still be in flight
  c->have_transform = a.carry_T;
  c->have_traj = true;
  return EFA_OK;
}

// ---- the batch solver (option "obs_solver" 1, efa_etkf.hip) -------------------------------------------------------
// Behind the prep launch, which left the effective flags and the neutral (0, 1) of every ob that is not assimilated on the device:
// the prior diagnostics and the obs' scales, the Gram contraction and the eigen-solve that leave [T | w] where the carried identity
// rows stand, every obs row through them (perturbation form, from the caller's block into the working rows), the posterior
// diagnostics, and ONE round trip.  efa_ensrf_cycle_dev's state transform goes into the stream behind all that before the host
// waits -- nothing is speculated, the solver has no fallback -- unless the outlier check ran: the plan then needs its count.
int batch_solve(efa_ctx* c, const ObsCall& a, SpecResult* spec) {
  hipStream_t s = c->stream;
  const int M = a.M;
  const long P = a.P;
  EFA_TRY(c->etkf_buf.reserve(etkf_ws_doubles(M, P) * sizeof(double)));
  EFA_TRY(c->status.reserve(3 * sizeof(int)));
  const EtkfWs w = etkf_ws(c->etkf_buf.as<double>(), M, P);
  double *T = a.Yw + (size_t)P * M, *wv = a.ymw + P;
  EFA_HIP(launch_etkf_prior(P, M, a.Yp_dev, a.ym_dev, c->ob_val, c->ob_err, c->ob_asm, c->d_prior_mean, c->d_prior_var,
                            c->d_assimilated, w, s));
  EFA_HIP(launch_etkf_solve(P, M, a.Yp_dev, w, T, wv, s));
  const TransformArgs t{a.Yp_dev, a.ym_dev, a.Yw, a.ymw, P, M, T, wv, 0};
  EFA_HIP(launch_transform(t, Elem::f64, s));
  EFA_HIP(launch_etkf_post(P, M, a.Yw, a.ymw, c->d_post_mean, c->d_post_var, s));
  int* st = reinterpret_cast<int*>(static_cast<char*>(c->pin_out.p) + 5 * a.oslot - 64);
  EFA_HIP(launch_results_to_host(c->out_pack.p, c->pin_out.p, 4 * a.oslot + (size_t)P, c->status.as<int>(), st, s));  // (the status words: not read)
  *spec = SpecResult{};
  if (!c->qc_used) EFA_TRY(speculative_transform(c, a, make_window(a, 0), spec));
  if (spec->launched) EFA_HIP(hipEventSynchronize(spec->interval->begin));
  else EFA_HIP(hipStreamSynchronize(s));
  if (spec->launched && c->timing) harvest_state_ms(c);
  return EFA_OK;
}

}  // namespace

// option "obs_solver" 1: an assimilated ob's error variance divides (the serial loop only adds it)
int check_batch_obs(const efa_ctx* c, long P, const double* ob_error, const uint8_t* ob_assim) {
  if (!c->obs_solver || !ob_error || !ob_assim) return EFA_OK;
  for (long k = 0; k < P; ++k)
    if (ob_assim[k] && !(std::isfinite(ob_error[k]) && ob_error[k] > 0.0))
      return fail(EFA_ERR_INVALID, "observation %ld: error variance %g must be finite and > 0 for the batch solver (option obs_solver 1)", k,
                  ob_error[k]);
  return EFA_OK;
}

int obs_phase(efa_ctx* c, int M, long P, double* ym_dev, double* Yp_dev, const ObsIn& ob, const DiagOut& diag, const SpecRequest& spec,
              SpecResult* spec_out) {
  const int loc_mode = ob.loc_mode;
  EFA_TRY(check_common(M, P));
  if (loc_mode != EFA_LOC_NONE && loc_mode != EFA_LOC_GC) return fail(EFA_ERR_INVALID, "loc_mode %d", loc_mode);
  EFA_TRY(check_vloc(c, loc_mode, P, -1));
  EFA_TRY(check_slab(c, loc_mode, P, -1));
  EFA_TRY(check_sec(c, loc_mode));
  EFA_TRY(check_batch_solver(c, loc_mode));
  EFA_TRY(check_batch_obs(c, P, ob.error, ob.assim));
  c->have_traj = false;
  c->batch_solved = false;
  c->M = M;
  c->P = P;
  c->loc_mode = loc_mode;
  c->n_active = 0;
  c->have_transform = false;
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
  a.ym_dev = ym_dev;
  a.Yp_dev = Yp_dev;
  a.ob = ob;
  a.diag = diag;
  a.spec = spec;
  EFA_TRY(stage_obs_inputs(c, a));
  EFA_TRY(start_phase_a(c, a));
  if (c->obs_solver) {
    SpecResult done;
    c->batch_solved = true;  // (the plan of the transform behind the solver reads it)
    EFA_TRY(batch_solve(c, a, &done));
    EFA_TRY(finish_obs_phase(c, a, Records::kNone, true, done));
    c->phase_a_kind = 5;
    if (spec_out) *spec_out = done;
    return EFA_OK;
  }
  Records layout = Records::kNone;
  SpecResult done;
  bool diag_on_host = false;    // the diagnostics are already in pin_out (copied with the status words of the one launch that did it all)
  bool status_clear = a.pipe_ok;  // (cleared by the prep launch: the first window's launch needs no memset of its own)
  for (long w = 0; w < a.nwin; ++w) {
    Window win = make_window(a, w);
    const bool tw_fits = (loc_mode != EFA_LOC_GC) || ((size_t)win.Pw * (size_t)win.Rw * sizeof(double) <= ((size_t)3 << 30));
    int kind = 0;
    if (a.pipe_ok && tw_fits) EFA_TRY(try_persistent_window(c, a, win, layout, status_clear, &kind, &done));
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
  EFA_TRY(finish_obs_phase(c, a, layout, diag_on_host, done));
  if (spec_out) *spec_out = done;
  return EFA_OK;
}

}  // namespace efa_host
