// The context behind the C ABI (include/efa_hip.h) and the small owning types it is made of, shared by the translation units that
// drive it (efa_driver.h lists them).  Not exported.
#pragma once
#include "../../include/efa_hip.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and enums only: librccl is opened with dlopen when a communicator is asked for

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace efa_host {

// sets the thread's efa_last_error() message and returns `code` (efa_capi.hip)
int fail(int code, const char* fmt, ...);

#define EFA_HIP(expr)                                                                       \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return fail(EFA_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                  __LINE__);                                                                \
  } while (0)

#define EFA_TRY(expr)          \
  do {                         \
    int _s = (expr);           \
    if (_s != EFA_OK) return _s; \
  } while (0)

// grow-only device buffer, freed with its owner
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int reserve(size_t bytes) {
    if (bytes <= cap) return EFA_OK;
    if (p) {
      hipError_t e = hipFree(p);
      p = nullptr;
      cap = 0;
      if (e != hipSuccess) return fail(EFA_ERR_HIP, "hipFree failed: %s", hipGetErrorString(e));
    }
    size_t want = bytes + (bytes >> 3) + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      return fail(EFA_ERR_HIP, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    cap = want;
    return EFA_OK;
  }
  template <typename T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// grow-only pinned host staging: one asynchronous copy each way instead of one (synchronous, staged by the
// runtime) copy per pageable caller array
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() {
    if (p) (void)hipHostFree(p);
  }
  int reserve(size_t bytes) {
    if (bytes <= cap) return EFA_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = bytes + (bytes >> 2) + 256;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
      p = nullptr;
      return fail(EFA_ERR_HIP, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    cap = want;
    return EFA_OK;
  }
};

// a stream or event the context created, destroyed with it
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
  H h = nullptr;
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() {
    if (h) (void)Destroy(h);
  }
  operator H() const { return h; }
};
// a stream finishes its work first (the diagnostic occupier may still hold CUs)
inline hipError_t sync_and_destroy(hipStream_t s) {
  (void)hipStreamSynchronize(s);
  return hipStreamDestroy(s);
}
using OwnedStream = Owned<hipStream_t, sync_and_destroy>;
using OwnedEvent = Owned<hipEvent_t, hipEventDestroy>;

// A timed stretch of the context's stream.  "timing" 2 (deferred) leaves it pending: it is read when its events are about to be
// recorded again, or in efa_last_timing.
struct Interval {
  OwnedEvent begin, end;
  bool pending = false;  // recorded, not read yet
};

// The column grid (lat | lon) of a localised state phase on the device.  Only its own functions (efa_phase_b.hip) write it: one
// per way the grid arrives.  Each leaves the device copy current for the state phase that follows.
struct ColumnGrid {
  DevBuf lat, lon;        // [ncol]
  PinBuf mirror;          // pinned image (lat | lon) of what the device holds
  long mirror_ncol = -1;  // columns the mirror and the device copies hold (-1: the mirror is not current)
  long serial = 0;        // bumped whenever the device copy is rewritten
  // from the caller's arrays; waits, so the caller may reuse them on return
  int upload(hipStream_t s, const double* grid_lat, const double* grid_lon, long ncol);
  // the same arrays ahead of Phase A: compared with the mirror, copied from it -- asynchronously -- only if they differ
  int refresh(hipStream_t s, const double* grid_lat, const double* grid_lon, long ncol);
  // columns [lo, lo + ncol) of a whole grid (lat | lon, `pitch` columns each) already on the device: in stream order, no host wait
  // (room for the widest slice is reserved first, so that no slice reallocates under work in flight)
  int reserve(long ncol);
  int take_slice(hipStream_t s, const double* dev_grid, long pitch, long lo, long ncol);
};

// one block of efa_pinned_alloc
struct PinnedBlock {
  void* p = nullptr;
  size_t bytes = 0;
};

// What the streamed host-memory update (efa_ensrf_cycle_host, efa_stream.hip) keeps from call to call.  Declared last in the
// context, so it is destroyed first: its events and host blocks go while the device is still set up.
struct StreamState {
  static constexpr int kRing = 3;     // device chunk buffers: one uploading, one in the state phase, one downloading
  static constexpr int kStage = 2;    // pinned staging images each way for caller memory that is not pinned
  std::vector<hipEvent_t> events;     // six per chunk (upload, state phase, download: start and end), grow-only
  std::vector<PinnedBlock> blocks;    // registry of efa_pinned_alloc: a host segment inside one of them goes by DMA directly
  void* ring = nullptr;               // kRing chunk buffers, allocated to the byte
  size_t ring_bytes = 0;
  PinBuf stage_up[kStage], stage_dn[kStage];
  PinBuf pin_obs, pin_grid;           // pinned images of the obs block and of the column grid
  DevBuf HX, ym, grid;                // obs block [P][M], its means [P], the whole column grid [lat | lon] on the device
  long chunks = 0, peak_bytes = 0, h2d_us = 0, d2h_us = 0, wall_us = 0;  // read-only options stream_*: the last call
  StreamState() = default;
  StreamState(const StreamState&) = delete;
  StreamState& operator=(const StreamState&) = delete;
  ~StreamState() {
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    if (ring) (void)hipFree(ring);
    for (const PinnedBlock& b : blocks) (void)hipHostFree(b.p);
  }
};

}  // namespace efa_host

using efa_host::ColumnGrid;
using efa_host::DevBuf;
using efa_host::fail;
using efa_host::Interval;
using efa_host::OwnedEvent;
using efa_host::OwnedStream;
using efa_host::PinBuf;

struct efa_ctx {
  // Members are destroyed in reverse order of declaration: the streams and events come first, so every buffer below is
  // freed before they go away.
  OwnedStream own_stream;
  OwnedStream dbg_stream;  // diagnostic occupier (options debug_occupy_*)
  OwnedStream up_stream, dn_stream;  // the streamed update's copy streams (efa_stream.hip), created when first used
  Interval obs_iv;       // the obs phase; it ends at obs_ends_at
  Interval state_iv[2];  // the state phase; efa_ensrf_cycle_dev alternates the two: it records a state phase's events BEFORE the
                         // stream is synchronised, while the previous cycle's may still be unread
  Interval imp_iv;       // efa_obs_impact_dev's contraction (its events are created by the first call)
  Interval sens_iv;      // one pass of efa_sensitivity_dev (likewise)
  Interval ver_iv;       // efa_verify_dev's pass and its reduction (likewise)
  Interval prod_iv;      // efa_products_dev's pass and its reduction (likewise)
  Interval gram_iv;      // efa_gram_dev's pass and its reduction (likewise)
  Interval nbr_iv;       // efa_neighbourhood_dev's records, windows and reduction (likewise)
  Interval pm_iv;        // efa_pm_mean_dev's keys, sorts and assignment (likewise)
  OwnedEvent ev_fs;  // the last host-to-device copy of the forward-operator stencil (pin_fs)
  OwnedEvent ev_order;  // a change of stream: recorded on the stream that is left, waited for by the one that takes over
  int device = 0;
  hipStream_t stream = nullptr;
  long obs_batch = 64;
  long path = EFA_PATH_AUTO;
  long timing = 0;
  long use_gram = 2;       // persistent kernel's leader: 2 band leader (with and without localisation), 1 Gram leader step by step, 0 vector chain
  long use_pipeline = 1;   // persistent Phase-A kernel when it applies (else per-batch kernels)
  long spin_limit = 4000000;
  long spin_ms = -1;       // wall-time bound of the persistent Phase-A launch; -1: 100 ms + P/100 ms
  int cu_count = 0;
  long dbg_occupy_blocks = 0;
  long pipe_debug = 0;
  long gc_onepass = 1;     // localised state sweep in one pass with per-column-block active lists

  // --- trajectory recorded by the last obs phase --------------------------
  bool have_traj = false;
  int M = 0;
  long P = 0;
  int loc_mode = EFA_LOC_NONE;
  long n_active = 0;
  bool have_transform = false;   // identity rows were carried: (T, w) valid
  std::vector<uint8_t> h_assim;  // host copy of ob_assim
  std::vector<double> h_hw;      // host copy of ob_halfwidth_km, sanitised for unassimilated obs
  DevBuf Ye_rec, coef;           // [P][M], [P][4]
  DevBuf traj, tw_mat, status, dbg;  // pipeline: trajectory records, GC obs-obs taper, status words, stamps
  const double* ye_ptr = nullptr;  // where Phase B reads the recorded ye rows
  long ye_stride = 0;
  int phase_a_kind = 0;          // 1 vector-chain pipeline, 2 per-batch kernels, 3 Gram leader, 4 band leader, 5 batch solver, 6 LETKF (efa_letkf_cycle_dev), 7 LETKF with weight interpolation (efa_letkf_cycle_interp_dev), 8 / 9 the two under vertical / slab localisation (efa_letkf_slab_cycle_dev / _interp_dev)
  DevBuf ob_pack, out_pack;  // the per-ob inputs / diagnostics below are slices of these two allocations (stage_obs_inputs)
  PinBuf pin_in, pin_out;    // their pinned host images: one H2D and one D2H per call
  PinBuf pin_fs;             // pinned image of the forward-operator stencil
  size_t fs_valid_n = 0;       // the device copy fs_idx holds the pinned image's first fs_valid_n stencil entries ...
  const void* fs_valid_dev = nullptr;  // ... if fs_idx and pin_fs are still these allocations
  const void* fs_valid_pin = nullptr;
  // in ob_pack: device copies [P] ([P][4] ob_errsq)
  double *ob_val = nullptr, *ob_err = nullptr, *ob_errsq = nullptr, *ob_lat = nullptr, *ob_lon = nullptr, *ob_hw = nullptr;
  uint8_t* ob_asm = nullptr;
  // in out_pack: [P]
  double *d_prior_mean = nullptr, *d_prior_var = nullptr, *d_post_mean = nullptr, *d_post_var = nullptr;
  uint8_t* d_assimilated = nullptr;
  DevBuf Yw, ymw;  // obs block workspace [(P+M)][M], [(P+M)]
  DevBuf win_Y, win_m;  // rows of one Phase-A window + the transform rows (only when P exceeds one persistent launch)
  // --- state phase workspaces ---------------------------------------------
  DevBuf W;           // taper table [nb][ncol]
  DevBuf gc_cnt, gc_ub, gc_order, gc_obtrig, gc_off, gc_idx, gc_wts, gc_pairs;  // one-pass GC sweep: CSR active lists
  long gc_active_pairs = 0;  // (column, ob) pairs with a non-zero taper in the last one-pass sweep
  // What depends on the GEOMETRY of a localised cycle only -- the obs' positions, radii and assimilate flags, the column grid --
  // is kept from one cycle to the next while that geometry is unchanged (a fixed observing network on a fixed grid): the obs-obs
  // taper table of Phase A and the per-block active lists of the one-pass sweep (indices, tapers, hand-out order; the gains are
  // folded in by the sweep itself, cycle by cycle).  Compared by content on the host, never by pointer.
  std::vector<double> geo_lat, geo_lon, geo_hw;
  std::vector<uint8_t> geo_assim;
  long geo_serial = 0;       // bumped whenever the obs geometry of a call differs from the previous call's
  long tw_serial = -1, tw_Pw = -1, tw_Rw = -1;  // what the obs-obs taper table on the device was built from
  const void* tw_ptr = nullptr;
  bool gc_list_valid = false;
  long gc_list_geo = -1, gc_list_grid = -1, gc_list_ncol = -1, gc_list_P = -1;
  const void* gc_list_ptrs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  long geometry_reuse = 1;   // option "geometry_reuse" (0: rebuild every cycle)
  bool gc_pairs_pending = false;  // ... still on the device (read when asked for, or before the counter is cleared again: a read
                                  // behind the sweep would hold the host until the sweep is done, cycle after cycle)
  ColumnGrid grid;
  DevBuf xm_ws;       // means for efa_state_cycle_dev
  DevBuf wide_prior;  // a copy of the prior rows for the in-place transform above 136 members [rows][M] of the rows' element type
  // --- float32 state storage (efa_state_cycle_f32_dev) ---------------------------------------
  DevBuf f32_ws;      // the float64 workspace of the routes without a float32 kernel [rows][M] (twice that above 136 members)
  long f32_native = 0;  // read-only option "f32_native": the last float32 state call ran on the float rows themselves
  // --- posterior relaxation (efa_ctx_set_relaxation) ------------------------------------------------------
  int relax_kind = EFA_RELAX_NONE;
  double relax_alpha = 0.0;
  DevBuf relax_T;      // RTPP: (1-alpha) T + alpha I [M][M]
  DevBuf relax_ss;     // standalone passes: sum of squared prior deviations per row [rows]
  DevBuf relax_prior;  // standalone RTPP with the posterior written over the prior: a copy of the prior [rows][M]
  // --- adaptive inflation (efa_ctx_set_adaptive_inflation) -------------------------------------
  double* ai_field = nullptr;  // the caller's [ai_rows][2] (mean, sd), updated by every GC state phase; null: off
  long ai_rows = 0;
  double ai_lower = 1.0, ai_upper = 1e6, ai_sd_lower = 0.0;
  DevBuf ai_ob;               // [P][4] what the sweep's update reads of each ob (launch_adapt_obs)
  // --- vertical localisation (efa_ctx_set_vertical_localization) -----------------------------------
  bool vl_on = false;
  bool vl_any = false;          // some ob carries vertical information (else every factor is 1 and the plain kernels run)
  long vl_nlead = 0, vl_P = 0;
  std::vector<double> vl_host;  // [n_lead slab coordinates | P ob coordinates | P half-widths] as on the device (NaN: 1 as half-width)
  long vl_serial = 0;           // bumped whenever the setting changes: part of the obs geometry (geo_serial)
  long geo_vl_serial = 0;       // ... the value the current geometry was compared with
  DevBuf vl_dev;                // device copy of vl_host
  DevBuf vl_W;                  // the per-batch sweep's taper table [nb][R] (launch_obs_taper_rows)
  // --- temporal and cross-variable localisation (efa_ctx_set_slab_localization) -----------------------
  bool sl_on = false;
  bool sl_any = false;          // some ob carries a temporal taper or some impact entry is not 1 (else every factor is 1: today's kernels)
  long sl_nlead = 0, sl_P = 0, sl_nvar = 0, sl_ngroup = 0;
  std::vector<double> sl_host;  // as on the device: doubles [lead_time n_lead | ob_time P | ob half-width P | impact n_group*n_var],
                                // then ints [lead_var n_lead | ob_group P | ob_var P]; NaN / -1 where a part or a value is absent
  long sl_serial = 0;           // bumped whenever the setting changes: part of the obs geometry (geo_serial), as vl_serial
  long geo_sl_serial = 0;       // ... the value the current geometry was compared with
  DevBuf sl_dev;                // device copy of sl_host
  DevBuf sl_tab;                // S[P][n_lead]: the slab factor (V T) C of every (ob, slab) pair (launch_slab_factor)
  long sl_tab_serial = -1, sl_tab_vl_serial = -1;  // the settings the table was built from
  const void* sl_tab_ptr = nullptr;
  long gc_family_used = -1;     // read-only option "gc_family": the kernel family of the last one-pass sweep (0 plain, 1 adaptive,
                                // 2 vertical, 3 slab table, 4 sampling error correction; -1: none ran)
  long gc_form_used = 0;        // read-only option "gc_form": the form of the last one-pass sweep (1 quad kernel, 2 row-per-lane kernel; 0: none ran)
  // --- sampling error correction (efa_ctx_set_sampling_error_correction) --------------------------------
  int sec_T = 0;                // nodes of the table; 0: off
  std::vector<double> sec_host; // the table as on the device
  DevBuf sec_dev;               // device copy of sec_host
  DevBuf sec_ob;                // [P][4] the record the sweep reads y'.y' of each ob from (launch_adapt_obs)
  // --- outlier check (efa_ctx_set_outlier_threshold) ----------------------------------------------
  double qc_threshold = 0.0;    // 0: off
  bool qc_used = false;         // the last obs phase ran it: its flags on the device may be fewer than the caller's
  DevBuf qc_act;                // [P][kCoefStride], GC: the caller's flags where the one-pass sweep's list builders read coef[3]
  // --- batch observation-space solver (option "obs_solver", efa_etkf.hip) ------------------------------------------
  long obs_solver = 0;          // 0 serial (Phase A's kernels), 1 batch (ETKF)
  bool batch_solved = false;    // the last obs phase ran the batch solver: the state phase goes through [T | w], there are no records
  DevBuf etkf_buf;              // its workspace (EtkfWs): scales, A, g, q, sweeps, mu, partial tiles
  // --- local ensemble transform Kalman filter (efa_letkf_cycle_dev): buffers of its own as well ------------------------
  DevBuf letkf_ob;    // per ob: value | error | lat | lon | half-width | requested flag | act [4] | dr [2] | obtrig [6] | dc | diagnostics
  DevBuf letkf_pts;   // the points of a list build (lat | lon): the grid's columns, or the probe points of efa_letkf_weights_dev
  DevBuf letkf_blk, letkf_idx, letkf_wts;  // the call's lists: off | cnt | ub | order, entries, tapers (the obs' then the grid's)
  DevBuf letkf_Yw;    // the mapped obs block [P][M] | its means [P]
  DevBuf letkf_pairs; // the list builders' pair counter
  DevBuf letkf_Tw;    // weight interpolation (efa_letkf_cycle_interp_dev, §7y-2): the node pairs [nnodes][M][M+1] ...
  DevBuf letkf_nst;   // ... and the node statistics [nnodes][3] when the caller takes none
  // --- the LETKF's per-point multiplicative inflation (efa_ctx_set_letkf_inflation): the caller's device arrays
  double* li_field = nullptr;        // [nsolve] lambda of every solve point, updated in place when li_sigma_b > 0; null: off
  long li_nsolve = 0, li_P = 0;
  const double* li_ob = nullptr;     // [P] the factor of every ob's own solve, or null (1.0)
  double li_sigma_b = 0.0, li_lower = 0.0, li_upper = 0.0;
  double* li_stats = nullptr;        // [nsolve][4] {p1, p2, p3, lambda_o}, or null
  // --- the LETKF's deterministic control analysis (efa_ctx_set_letkf_control): the caller's device arrays
  const double* lc_xc = nullptr;     // [rows] the control, one value per state row; null: off
  double* lc_xc_post = nullptr;      // [rows] its analysis (lc_xc itself, or clear of it)
  const double* lc_yc = nullptr;     // [P] H(x_c)
  double* lc_yc_post = nullptr;      // [P] the analysis' ob estimates (clear of lc_yc)
  long lc_rows = 0, lc_P = 0;
  // --- the LETKF's cap on the local obs of a solve (efa_ctx_set_letkf_obs_cap)
  bool oc_on = false;
  int oc_nclass = 0;
  int oc_cap[32] = {};               // per class, 0: no limit (a cap beyond INT_MAX is none: a list has fewer entries)
  long oc_P = 0;
  bool oc_has_class = false;         // false: every ob is of class 0
  DevBuf oc_class;                   // [P] ints, the class of every ob
  double* oc_reach = nullptr;        // [nsolve] the caller's device array, or null
  long oc_nsolve = 0;
  // --- the LETKF's cross validation over member groups (efa_ctx_set_letkf_cross_validation)
  bool cv_on = false;
  int cv_M = 0, cv_ngroups = 0;
  DevBuf cv_lists;                   // ints: perm [ngroups][M] (per group: the other groups' members ascending, then its own) | nind [ngroups]
  double* cv_stats = nullptr;        // [nsolve][2] the caller's device array, or null
  long cv_nsolve = 0;
  DevBuf cv_C;                       // the Gram matrix C of every solve point of a launch [npts][M][M] (the sub-solves re-read it)
  DevBuf cv_Tw;                      // the obs block's pairs [P][M][M+1]
  // --- the LETKF's slab groups (efa_letkf_slab_cycle_dev): slabs whose factors agree for every ob share one solve
  std::vector<int> lg_group_of;                   // [n_lead] the group of every slab, numbered by first appearance
  int lg_ngroups = 0;
  long lg_vl_serial = -1, lg_sl_serial = -1;      // the settings the groups were computed from
  const void* lg_ptr = nullptr;
  DevBuf lg_dev;      // ints: rep [ngroups] | grp_off [ngroups + 1] | grp_leads [n_lead]
  // --- observation impact (efa_obs_impact_dev): buffers of its own, nothing above is touched by it ---------------
  //     (efa_obs_impact_slab_dev, §7u, brings sl_tab up to date as well: the table's cache, keyed by the two settings' serials)
  DevBuf imp_ob;    // per ob: used flags (coefficient-shaped) | scale | lat | lon | half-width | obtrig scratch | impact
  DevBuf imp_Yp;    // analysis perturbations in observation space [P][M] | their means [P]
  DevBuf imp_grid;  // the call's column grid (lat | lon)
  DevBuf imp_blk, imp_idx, imp_wts;  // the call's active lists: off | cnt | ub | order, entries, tapers
  DevBuf imp_part;  // GC: partial sums [groups of slabs][entries] | per-range sums [ranges][P]; unlocalised: per-wave z | z
  long impact_us = 0;  // read-only option "impact_us": device time of the last call's contraction and reduction
  // --- ensemble sensitivity and targeting (efa_sensitivity_dev): buffers of its own as well -------------------------
  DevBuf sens_pack;  // what a pass stages in LDS: vectors [K + t][M] | b/d [t][K] | 1/d [t] | weights [K] | varJ [K]; slab errors [n_lead]
  DevBuf sens_best;  // per workgroup: best score | its row; then the grid's
  long sens_us = 0;  // read-only option "sens_us": device time of the last call's passes
  // --- ensemble verification (efa_verify_dev): a buffer of its own as well ------------------------------------------
  DevBuf ver_ws;     // per chunk: partial sums | counts; per group: sums | histogram | n | n_bad; the slab groups
  long verify_us = 0;      // read-only option "verify_us": device time of the last call
  long verify_blocks = 0;  // option "verify_blocks": grid cap of k_verify (0: the default)
  // --- ensemble products and probability verification (efa_products_dev): a buffer of its own as well -----------------
  DevBuf prod_ws;    // per chunk: partial sums | bad counts; per group: sums | n_bad | table; thresholds; the slab groups
  long products_us = 0;      // read-only option "products_us": device time of the last call
  long products_blocks = 0;  // option "products_blocks": grid cap of k_products (0: the default)
  // --- ensemble Gram matrix (efa_gram_dev): a buffer of its own as well ------------------------------------------------
  DevBuf gram_ws;    // per stream: partial tiles | row statistics | counts; G, sums, counts; the slab scales
  long gram_us = 0;      // read-only option "gram_us": device time of the last call
  long gram_blocks = 0;  // option "gram_blocks": grid cap of k_gram (0: the default)
  // --- neighbourhood probabilities and the fractions skill score (efa_neighbourhood_dev): a buffer of its own as well ---
  DevBuf nbr_ws;     // per batch of slabs: mask words | counts | flags; per tile: partial sums | counts; per group: sums | n | n_bad; tables
  long neighbourhood_us = 0;      // read-only option "neighbourhood_us": device time of the last call
  long neighbourhood_blocks = 0;  // option "neighbourhood_blocks": grid cap of its kernels (0: the default)
  long nbr_ws_bytes = 0;          // option "nbr_ws_bytes": a lower cap of the records of a batch (0: EFA_NBR_WS_BYTES)
  // --- probability-matched mean (efa_pm_mean_dev): a buffer of its own as well -------------------------------------------
  DevBuf pm_ws;      // per batch of slabs: pooled keys a | b, rank keys and payloads a | b; histograms and scans; the tables; n_bad
  long pm_us = 0;           // read-only option "pm_us": device time of the last call
  long pm_passes = 0;       // read-only option "pm_passes": radix passes the last call ran on the pool, summed over its batches
  long pm_rank_passes = 0;  // read-only option "pm_rank_passes": the same on the rank keys
  long pm_blocks = 0;       // option "pm_blocks": grid cap of its kernels (0: the default)
  long pm_ws_bytes = 0;     // option "pm_ws_bytes": a lower cap of the pooled buffers of a batch (0: EFA_PM_WS_BYTES)
  // --- f1: interpolation stencils -------------------------------------------------
  DevBuf fs_idx;  // efa_forward_stencil_dev staging
  DevBuf f_glat, f_glon, f_sl, f_cl, f_valids, f_var, f_time, f_lat, f_lon, f_near, f_idx, f_wts, f_status;
  long f_P = 0;       // observations of the stencil held in f_idx / f_wts (0: none)
  // --- host-memory API buffers ----------------------------------------------
  DevBuf h_xm, h_Xp, h_ym, h_Yp;
  // --- multi-GPU exchange step: an RCCL communicator owned by the context (efa_comm_init) -------------
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  DevBuf gcc_lat, gcc_lon, gcc_oblat, gcc_oblon, gcc_obhw, gcc_coef, gcc_trig, gcc_cnt, gcc_pairs;  // efa_gc_block_counts
  // --- timing -----------------------------------------------------------------
  double state_ms = 0.0, obs_ms = 0.0;
  hipEvent_t obs_ends_at = nullptr;  // obs_iv.end, or the begin event of the state interval a speculative transform was put behind
  double state_ms_sum = 0.0, obs_ms_sum = 0.0;  // timing 2: sums since the previous efa_last_timing
  long state_launches_sum = 0;
  long state_launches = 0;
  int path_taken = 0;
  efa_host::StreamState st;  // efa_ensrf_cycle_host, efa_pinned_alloc
};
