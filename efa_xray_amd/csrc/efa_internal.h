// Internal interfaces between the C-ABI layer (efa_capi.hip) and the kernel
// translation units.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

namespace efa {

// ---- runtime width -> template argument ------------------------------------------------
// dispatch_width(w, Widths{}, f) returns f(std::integral_constant<int, W>{}) for the W of Widths equal to w, and
// hipErrorInvalidValue when there is none.  Only the listed widths are instantiated.
template <class F>
hipError_t dispatch_width(int, std::integer_sequence<int>, F&&) { return hipErrorInvalidValue; }
template <int W0, int... W, class F>
hipError_t dispatch_width(int w, std::integer_sequence<int, W0, W...>, F&& f) {
  if (w == W0) return f(std::integral_constant<int, W0>{});
  return dispatch_width(w, std::integer_sequence<int, W...>{}, f);
}
template <int Lo, int... I>
constexpr std::integer_sequence<int, (Lo + I)...> offset_widths(std::integer_sequence<int, I...>) { return {}; }
// Lo, Lo+1, ..., Hi
template <int Lo, int Hi>
using WidthRange = decltype(offset_widths<Lo>(std::make_integer_sequence<int, Hi - Lo + 1>{}));
// chunks of 8 members the quad-layout sweeps are instantiated for (sweep_slots(M) / 8)
using SweepChunks = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 20, 24, 32>;

// The element type of state rows in memory.  The kernel argument structs below carry rows of either type as
// double pointers: the launch, not the pointer, says which kernels read them.
enum class Elem { f64, f32 };
inline size_t elem_size(Elem e) { return e == Elem::f32 ? sizeof(float) : sizeof(double); }

// Largest ensemble the register-resident kernels are instantiated for.
constexpr int kMaxMembers = 256;
// Rows (observations) handled by one obs-space diag workgroup == max obs_batch.
constexpr int kMaxBatch = 64;
// Nodes of the largest sampling-error-correction table: the one-pass sweep stages it in 4 KB of LDS.
constexpr int kSecMaxT = 512;

// Per-observation coefficients recorded by Phase A (4 doubles per ob):
//   [0] innov   = ob.value - mye                     (ensrf.py:85)
//   [1] rden    = 1 / (varye + ob.error)             (ensrf.py:91,119)
//   [2] beta    = 1/(1+sqrt(err/(varye+err)))        (ensrf.py:135)
//   [3] active  = 1.0 if ob.assimilate_this else 0.0 (ensrf.py:74)
constexpr int kCoefStride = 4;

enum TaperMode : int {
  kTaperNone = 0,   // loc in (None, False)
  kTaperTable = 1,  // state rows: W[k][col] precomputed per batch (2-D taper, ensrf.py:108-111)
  kTaperObs = 2     // obs rows: haversine between observations, in-kernel (ensrf.py:113)
};

struct SweepArgs {
  const double* Xin;   // [nrows][M] perturbation rows (may alias Xout)
  const double* xin;   // [nrows]   means
  double* Xout;
  double* xout;
  long nrows;
  int M;
  const double* Ye;    // [nb][ye_stride] recorded obs-space perturbations of the batch
  long ye_stride;      // doubles between consecutive ye rows (>= M)
  const double* coef;  // [nb][kCoefStride]
  int nb;
  int taper_mode;
  const double* W;     // kTaperTable: [nb][ncol]
  long ncol;
  const double* row_lat;  // kTaperObs: lat/lon of the ob each swept row belongs to [nrows]
  const double* row_lon;
  const double* ob_lat;   // kTaperObs: lat/lon/halfwidth of the batch obs [nb]
  const double* ob_lon;
  const double* ob_hw;
  long skip_lo, skip_hi;  // rows in [skip_lo, skip_hi) are not touched
  long taper_rows;        // kTaperObs applies to rows < taper_rows (extra rows: weight 1)
  // sampling error correction; sec_tab == null: off.  Phase A's one-ob batches only (nb == 1)
  const double* sec_tab;  // [sec_T] the factor at |r| = j / (sec_T - 1), device
  int sec_T;
};

struct DiagArgs {
  double* Yp;  // [P(+extra)][M] obs block perturbations (in/out)
  double* ym;  // [P(+extra)]    obs block means (in/out)
  int M;
  long b0;  // first ob of the batch
  int nb;   // obs in the batch (<= kMaxBatch)
  const double* ob_value;  // device [P]
  const double* ob_error;
  const uint8_t* ob_assim;
  int loc_mode;
  const double* ob_lat;
  const double* ob_lon;
  const double* ob_hw;
  double* Ye_rec;  // [P][M] out: ye of ob k at the moment it is assimilated
  double* coef;    // [P][kCoefStride] out
  double* prior_mean;  // device [P] out
  double* prior_var;
  double* post_mean;
  double* post_var;
  uint8_t* assimilated;
};

// ---- persistent Phase-A pipeline (efa_pipeline.hip) --------------------------------
// Trajectory record of ob k in global memory: kTrajPad doubles of ye (zero padded) followed
// by 8 scalars.  Every 8-byte element is written once with an agent-scope store and is
// pre-filled with kTrajSentinel, so a reader validates each element on its own: no flag,
// no ordering between the elements (MI355X_MICROARCH.md, "R2 granule").
constexpr unsigned long long kTrajSentinel = 0x7FF8DEADBEEF0001ull;  // a NaN payload no arithmetic produces
constexpr int kTrajScalars = 8;  // mye, mean(ye), innov, rden, beta, active, prior_var, (unused)
constexpr int kPipeLanes = 4;    // lanes per row in the pipeline kernel (== its compute waves per workgroup)
inline int traj_pad(int M) { return 2 * kPipeLanes * ((M + 2 * kPipeLanes - 1) / (2 * kPipeLanes)); }
inline long traj_stride(int M) { return traj_pad(M) + kTrajScalars; }
constexpr int kPipeRowsPerWG = 64;
constexpr int kPipeMaxWGs = 256;  // one workgroup per CU (320 threads k_pipe, 512 threads k_pipe_gram): all co-resident

struct PipeArgs {
  double* Yp;   // [R][M] obs block (+ extra identity rows), in/out
  double* ym;   // [R]
  long R;       // rows swept (P + extra)
  long P;       // observations
  int M;
  const double* ob_value;  // device [P]
  const double* ob_error;
  const uint8_t* ob_assim;
  const double* ob_errsq;  // device [P][4]: {error, sqrt(error), assimilate (1.0 / 0.0), 0} (the band leader reads them with wave-uniform loads)
  int loc_mode;
  const double* tw;  // GC: dense obs-obs taper [P][R] (row k = ob k against every row); else null
  unsigned long long* traj;  // [P][traj_stride(M)] sentinel-filled
  double* coef;         // [P][kCoefStride] out
  double* prior_mean;   // [P] out
  double* prior_var;
  double* post_mean;
  double* post_var;
  uint8_t* assimilated;
  int* status;          // [3]: [0] abort flag (in-kernel), [1] 1 = given up, [2] 1 = because of the Gram cancellation guard
  long spin_limit;      // bound of the in-kernel polls (count)
  long spin_ticks;      // ... and in wall time: s_memrealtime ticks (100 MHz) since the kernel started; 0 = none
  int cu_count;         // compute units of the device: the launch is refused unless the grid is co-resident
  unsigned long long* dbg;  // diagnostic (debug & 4): [P][8] cycle stamps of the leader chain, else null
  int debug;  // diagnostic bits (single-workgroup timing runs only): 1 no global publication, 2 no prefetch
};

hipError_t launch_pipeline(const PipeArgs& a, hipStream_t s);
bool pipeline_supported(int M, long R);
hipError_t launch_pipeline_gram(const PipeArgs& a, hipStream_t s);  // efa_pipeline_gram.hip
bool pipeline_gram_supported(int M, long R, int loc_mode);
hipError_t launch_pipeline_band(const PipeArgs& a, hipStream_t s);  // efa_pipeline_band.hip (unlocalised cycles)
bool pipeline_band_supported(int M, long R, int loc_mode);
long band_traj_stride(int M);  // doubles per trajectory record as k_pipe_band lays them out (its rows are padded to its own lane layout)
hipError_t launch_fill_u64(unsigned long long* p, size_t n, unsigned long long v, hipStream_t s);
hipError_t launch_obs_taper_matrix(long P, long R, const double* ob_lat, const double* ob_lon, const double* ob_hw,
                                   double* trig_scratch /* [P][6] */, double* tw, hipStream_t s);
// vertical localisation of the obs-obs taper (efa_vloc.hip): tw[k][j] *= the vertical factor of obs (j, k) for
// j < P (the table launch_obs_taper_matrix wrote); and the per-batch sweep's table W[k][j] = horizontal x vertical taper of
// ob b0 + k against row j of the obs block (1 for rows j >= P), for the table mode of k_sweep
hipError_t launch_obs_taper_vert(long P, long R, const double* ob_vert, const double* ob_vhw, double* tw, hipStream_t s);
hipError_t launch_obs_taper_rows(long b0, int nb, long R, long P, const double* ob_lat, const double* ob_lon, const double* ob_hw,
                                 const double* ob_vert, const double* ob_vhw, double* W, hipStream_t s);
// temporal and cross-variable localisation (efa_slabloc.hip).  The obs' side of the setting on the device, every
// pointer at the first ob of the block or window it is used for
struct SlabObs {
  const double* ob_time;  // [P] lag of each ob, NaN: no time (factor 1 in every pair it is part of)
  const double* ob_thw;   // [P] temporal half-width, NaN: ob k tapers nothing in time
  const int* ob_group;    // [P] row of the impact table, -1: a row of ones
  const int* ob_var;      // [P] the state variable the ob's obtype names, -1: none
  const double* impact;   // [n_group][n_var]
  long n_var;
};
// S[k][s] = (V T) C of ob k and slab s (lead_vert null: V = 1), the table the slab family of the one-pass sweep stages from
hipError_t launch_slab_factor(long P, long n_lead, const double* lead_vert, const double* ob_vert, const double* ob_vhw,
                              const double* lead_time, const int* lead_var, const SlabObs& o, double* S, hipStream_t s);
// tw[k][j] = (tw[k][j] T(j,k)) C[k, v_j] for j < P, behind launch_obs_taper_matrix (and launch_obs_taper_vert); and
// launch_obs_taper_rows with both factors (ob_vert null: no vertical factor)
hipError_t launch_obs_taper_slab(long P, long R, const SlabObs& o, double* tw, hipStream_t s);
hipError_t launch_obs_taper_rows_slab(long b0, int nb, long R, long P, const double* ob_lat, const double* ob_lon, const double* ob_hw,
                                      const double* ob_vert, const double* ob_vhw, const SlabObs& o, double* W, hipStream_t s);

// ---- one-pass localised sweep (efa_gcsweep.hip) ---------------------------------------
struct GcSweepArgs {
  long ncol, n_lead;
  int M;
  long nblk;            // column blocks of 16
  const long* off;      // [nblk+1] offsets into idx / wts (a block's entries start at off[b])
  const int* cnt;       // [nblk] entries of block b
  const int* order;     // [nblk] blocks by descending list length: workgroup i takes block order[i]
  const int* idx;       // [nnz] observation index, ascending within a block
  const double* wts;    // [nnz][16] taper of the block's 16 columns
  const double* coef;   // [P][kCoefStride]
  const double* Ye;     // recorded ye rows
  long ye_stride;
  const double* Xin;    // [n_lead*ncol][M] perturbations (or prior members when fused_members)
  const double* xin;    // [n_lead*ncol] means (unused when fused_members)
  double* Xout;
  double* xout;
  int fused_members;
  int lead_split;       // set by the launcher: groups of slabs a column block is cut into (one workgroup each)
  long lead_chunk;      // slabs per group
  // adaptive inflation (Anderson 2009); infl == null: off
  double* infl;             // [n_lead*ncol][2] (mean, sd) of every state row, updated in place
  const double* adapt_ob;   // [P][4] {D^2, prior var, ob error variance, y'.y'} (launch_adapt_obs)
  double infl_lower, infl_upper, infl_sd_lower;
  // vertical localisation; lead_vert == null: off (exclusive with infl)
  const double* lead_vert;  // [n_lead] vertical coordinate of each slab, NaN: not localised vertically
  const double* ob_vert;    // [P] the obs' vertical coordinates, NaN: no vertical taper
  const double* ob_vhw;     // [P] their vertical half-widths (1 where ob_vert is NaN)
  // slab table; null: off.  It carries the vertical factor as well: the slab family serves the call
  const double* slab_tab;   // [P][n_lead] the factor of every (ob, slab) pair (launch_slab_factor)
  // sampling error correction; sec_tab == null: off (exclusive with the three above).  It reads y'.y' of each ob
  // from adapt_ob, the record of the adaptive-inflation family
  const double* sec_tab;    // [sec_T] the factor at |r| = j / (sec_T - 1), device
  int sec_T;                // 2 .. kSecMaxT
};
long gc_num_blocks(long ncol);
// list build in one pass: upper bounds + device prefix sum (off[nblk] = capacity needed), then the entries
hipError_t launch_gc_bound(long ncol, long P, const double* glat, const double* ob_lat, const double* ob_hw,
                           const double* coef, int* ub, long* off, hipStream_t s);
hipError_t launch_gc_fill(long ncol, long P, const double* glat, const double* glon, const double* ob_lat,
                          const double* ob_lon, const double* ob_hw, const double* coef, double* obtrig /* [P][6] scratch */,
                          const long* off, int* cnt, int* idx, double* wts, int* order, unsigned long long* npairs,
                          hipStream_t s);
// the counting half of the list build alone: cnt[b] = observations with a non-zero taper on any of block b's 16 columns
hipError_t launch_gc_count(long ncol, long P, const double* glat, const double* glon, const double* ob_lat,
                           const double* ob_lon, const double* ob_hw, const double* coef, double* obtrig /* [P][6] scratch */,
                           int* cnt, int* blk_pairs /* [nblk] (column, ob) pairs of each block, or null */,
                           unsigned long long* npairs, hipStream_t s);
// elem: the element type a.Xin / a.Xout point at.  float32 is the member form on the row-per-lane kernel:
// sweep_gc_serves says which cycles that is (an even M up to 104), whatever the alignment of the rows; float64 serves every cycle
bool sweep_gc_serves(Elem elem, int M, long ye_stride, const double* Ye);
// the form launch_sweep_gc runs the call in: 2 the row-per-lane kernel, 1 the quad kernel (the option "gc_form")
int sweep_gc_form(const GcSweepArgs& a, Elem elem);
hipError_t launch_sweep_gc(const GcSweepArgs& a, Elem elem, hipStream_t s);

// ---- observation impact (EFSO, efa_impact.hip) ----------------------------------
// The localised contraction: a sibling of the one-pass sweep's row-per-lane kernel that reads the state once and writes none of
// it.  It walks the same per-block active lists (built by launch_gc_bound / launch_gc_fill into buffers of the call's own).
struct ImpactGcArgs {
  long ncol, n_lead;
  int M;
  long nblk;
  const long* off;      // the active lists, as GcSweepArgs has them
  const int* cnt;
  const int* order;
  const int* idx;
  const double* wts;
  const double* Yp;     // [P][M] analysis perturbations in observation space
  const double* X;      // [n_lead*ncol][M] forecast members
  const double* v;      // [n_lead*ncol] weighted error sum of every state row
  const double* lead_vert;  // vertical localisation as in GcSweepArgs; null: off
  const double* ob_vert;
  const double* ob_vhw;
  double* partial;      // [lead_split][cap] out: one sum per (group of 16 slabs, list entry)
  long cap;             // off[nblk]
  int lead_split;       // groups of 16 slabs (set by the launcher)
  const double* slab_tab;   // slab table as in GcSweepArgs; null: off.  It carries the vertical factor as well
};
int impact_lead_split(long n_lead);
hipError_t launch_impact_gc(const ImpactGcArgs& a, hipStream_t s);
// partial -> impact[k] = scale[k] * (sum of ob k's partials), in a fixed order: `ranges` workgroups each add the entries of a
// contiguous range of column blocks into a row of acc [ranges][P], then one thread per ob adds the rows
int impact_reduce_ranges(long nblk, long P);
hipError_t launch_impact_reduce(long nblk, long P, const long* off, const int* cnt, const int* idx, const double* partial, long cap,
                                int lead_split, const double* scale, double* acc, double* impact, hipStream_t s);
// unlocalised: z[m] = sum_i v[i] X'[i][m] (grid-stride over a capped grid, per-wave partial sums in zpart [impact_z_waves()][256],
// added in a fixed order), then impact[k] = scale[k] * (Yp[k] . z)
long impact_z_waves();
hipError_t launch_impact_none(long rows, int M, long P, const double* X, const double* v, const double* Yp, const double* scale,
                              double* zpart, double* z /* [256] */, double* impact, hipStream_t s);

struct TransformArgs {
  const double* Xin;  // [rows][M] perturbations, or full members when fused_members
  const double* xin;  // [rows] means (unused when fused_members)
  double* Xout;       // [rows][M]
  double* xout;       // [rows] (unused when fused_members)
  long nrows;
  int M;
  const double* T;  // [M][M] row-major: Xap = Xbp * T
  const double* w;  // [M]:             xam = xbm + Xbp * w
  int fused_members;  // 1: Xin holds prior members, Xout receives posterior members
};

int sweep_slots(int M);                                  // padded row length of the quad layout
size_t diag_lds_bytes(int slots, int nb, int loc_mode);  // dynamic LDS of the diag kernel

hipError_t launch_sweep(const SweepArgs& a, hipStream_t s);
hipError_t launch_diag(const DiagArgs& a, hipStream_t s);
// elem: the element type a.Xin / a.Xout point at; float32 rows (the kernels of efa_transform_f32.hip) in member form only
hipError_t launch_transform(const TransformArgs& a, Elem elem, hipStream_t s);
bool transform_supported(int M);
// RTPS fused into the member-form transform (k_transform_rtps): M <= 136, one launch with [T | w] in LDS
hipError_t launch_transform_rtps(const TransformArgs& a, double alpha, Elem elem, hipStream_t s);
bool transform_rtps_supported(int M);
// float32 rows <-> the float64 workspace (efa_misc.hip): an exact widening copy, and posterior members rounded once
hipError_t launch_widen_f32(size_t n, const float* X, double* out, hipStream_t s);
hipError_t launch_narrow_f32(size_t n, const double* X, float* out, hipStream_t s);
// posterior relaxation (efa_relax.hip): Tout = (1-alpha) T + alpha I; per-row sum of squared deviations; in-place relaxation of
// rows (rtpp 0: RTPS from ss, 1: RTPP against the prior rows)
hipError_t launch_relax_fold(int M, double alpha, const double* T, double* Tout, hipStream_t s);
hipError_t launch_row_spread(long rows, int M, const double* X, double* ss, hipStream_t s);
hipError_t launch_relax_rows(long rows, int M, int rtpp, double alpha, double* X, const double* ss, const double* prior,
                             hipStream_t s);

// adaptive inflation (efa_adapt.hip): X[row] <- mean + sqrt(field[row][0]) (X[row] - mean) (rows with field 1 untouched);
// the per-ob scalars the sweep's update reads, from Phase A's records and diagnostics
hipError_t launch_inflate_rows(long rows, int M, double* X, const double* field, hipStream_t s);
hipError_t launch_adapt_obs(long P, int M, const double* coef, const double* prior_var, const double* ob_error, const double* Ye,
                            long ye_stride, double* out /* [P][4] */, hipStream_t s);

hipError_t launch_form_perts(long rows, int M, const double* X, double scale, double* xm,
                             double* Xp, hipStream_t s);
hipError_t launch_posterior(long rows, int M, const double* xm, const double* Xp, double* post,
                            hipStream_t s);
hipError_t launch_taper_table(long ncol, int nb, const double* grid_lat, const double* grid_lon,
                              const double* ob_lat, const double* ob_lon, const double* ob_hw,
                              double* W, hipStream_t s);
hipError_t launch_forward_stencil(long rows, long row_offset, int M, const double* X, long P,
                                  int npt, const int64_t* idx, const double* wts, double* HX,
                                  hipStream_t s);
// ---- f1: interpolation stencils on the device (efa_forward.hip) -----------------------------
struct InterpArgs {
  long P;
  int nvar, nt, ny, nx, latlon_1d;
  long n_grid;
  const double *glat, *glon;   // device [n_grid]
  double *sl, *cl;             // device workspace [n_grid]
  const double* valids;        // device [nt]
  const int* ob_var;           // device [P]
  const double *ob_time, *ob_lat, *ob_lon;  // device [P]
  long* nearest;               // device workspace [P][4]
  long* sten_idx;              // device out [P][8]
  double* sten_wts;            // device out [P][8]
  unsigned char* status;       // device out [P]
};
hipError_t launch_interp_stencils(const InterpArgs& a, hipStream_t s);
hipError_t launch_forward_cols(long ncol, long col_lo, long col_hi, long n_lead, int M, const double* X, long P, int npt,
                               const long* idx, const double* wts, double* HX, hipStream_t s);
hipError_t launch_fill_synthetic(long rows, long row_offset, int M, uint64_t seed, double sigma,
                                 double* X, hipStream_t s);
hipError_t launch_set_identity(int M, double* T, double* w, hipStream_t s);
hipError_t launch_phase_a_prep(long P, int M, const double* Yp, const double* ym, double* Yw, double* ymw, int carry_T,
                               unsigned long long* traj, size_t traj_words, unsigned long long sentinel, int* status,
                               const void* pack_host, void* pack_dev, size_t pack_bytes, hipStream_t s);
// ... with the outlier check: `slot` is the pack's slot size (value | error | assim bytes | 4 slots of records ...),
// `threshold` > 0; host_act [P][kCoefStride] (or null) receives the requested flags for the one-pass sweep's list builders
hipError_t launch_phase_a_prep_qc(long P, int M, const double* Yp, const double* ym, double* Yw, double* ymw, int carry_T,
                                  unsigned long long* traj, size_t traj_words, unsigned long long sentinel, int* status,
                                  const void* pack_host, void* pack_dev, size_t pack_bytes, size_t slot, double threshold,
                                  double* host_act, hipStream_t s);
// ---- the batch observation-space solver (ETKF, efa_etkf.hip) ----------------------------------------------------
constexpr int kEtkfLdsMaxM = 136;   // the eigen-solve keeps its M x M array in LDS up to here (148 KB), in global memory above
constexpr int kEtkfSweepCap = 30;   // Jacobi sweeps at most (convergence leaves the counted loop early)
// the solver's workspace, slices of one allocation of etkf_ws_doubles(M, P) doubles
struct EtkfWs {
  double* sc;      // [P] 1/sqrt(error) of an assimilated ob, 0 otherwise
  double* dt;      // [P] the scaled innovation, 0 for an ob that is not assimilated
  double* A;       // [M][M] (M-1) I + C; the eigen-solve works in it above kEtkfLdsMaxM members
  double* g;       // [M]
  double* q;       // [1]
  double* sweeps;  // [1] Jacobi sweeps taken
  double* mu;      // [M] eigenvalues of A, in the order of the columns
  double* part;    // [streams][tiles][256] partial Gram tiles
};
size_t etkf_ws_doubles(int M, long P);
EtkfWs etkf_ws(double* base, int M, long P);
int etkf_tiles(int M);
int etkf_streams(int M, long P);
// prior diagnostics of every ob and the obs' scales, from the caller's block and the effective flags the prep launch wrote
hipError_t launch_etkf_prior(long P, int M, const double* Yp, const double* ym, const double* ob_value, const double* ob_error,
                             const uint8_t* ob_assim, double* prior_mean, double* prior_var, uint8_t* assimilated, const EtkfWs& w,
                             hipStream_t s);
// Gram contraction, its reduction and the eigen-solve: [T | w] to Tout [M][M], wout [M]; mu, g, q, sweeps stay in the workspace
hipError_t launch_etkf_solve(long P, int M, const double* Yp, const EtkfWs& w, double* Tout, double* wout, hipStream_t s);
// posterior diagnostics of the mapped obs rows
hipError_t launch_etkf_post(long P, int M, const double* Yw, const double* ymw, double* post_mean, double* post_var, hipStream_t s);

// ---- the local ensemble transform Kalman filter (LETKF, efa_letkf.hip) ------------------------------------------
constexpr int kLetkfMaxM = kEtkfLdsMaxM;  // the eigen-solve's array of every column lives in LDS: no form above
enum LetkfMode : int {
  kLetkfMembers = 0,  // member rows of the state: n_lead rows per column, float64 or float32
  kLetkfPerts = 1,    // rows in perturbation form (the obs block: one row per point, its mean beside it), not relaxed
  kLetkfWeights = 2   // no rows: [T | w] of every point to Tw
};
struct LetkfArgs {
  long npts;          // columns of the grid, ob positions, or probe points: one workgroup each
  long n_lead;        // rows per column (kLetkfMembers), row lead * npts + col
  int M;
  // the per-block lists of launch_gc_bound / launch_gc_fill (all null: every list is empty)
  const long* off;
  const int* cnt;
  const int* order;
  const int* idx;
  const double* wts;
  const double* Yp;   // [P][M] the PRIOR obs perturbations
  const double* dr;   // [P][2] {value - ym, error variance} of every ob with an effective flag of 1
  const void* Xin;    // kLetkfMembers: [n_lead * npts][M] prior members ...
  void* Xout;         // ... and posterior members (the same address, or clear of Xin)
  const double* ym_in;   // kLetkfPerts: [npts] means, [npts][M] perturbations ...
  const double* Yp_in;
  double* ym_out;        // ... and where the mapped rows go (clear of the inputs)
  double* Yp_out;
  double* Tw;         // kLetkfWeights: [npts][M][M + 1], row a of a point = T[a][0..M) | w[a]
  double* stats;      // [npts][3] {n_local, dfs, sweeps} or null
  int relax_kind;     // kLetkfMembers: EFA_RELAX_* and its factor (RTPP folded into f, RTPS fused per row)
  double relax_alpha;
  // per-point multiplicative inflation: A = (M-1)/lambda I + C; null: lambda = 1 everywhere, no statistics
  double* infl;         // [ngroups][npts] lambda_b, indexed as stats; read and (infl_sigma2 > 0) written by the point's own workgroup
  double infl_sigma2;   // the prior variance sigma_b^2 of Miyoshi's (2011) estimate; 0: the field is fixed and never written
  double infl_lo, infl_hi;  // lambda_a is clipped to [lo, hi]
  double* infl_stats;   // [ngroups][npts][4] {p1, p2, p3, lambda_o} or null
  // the deterministic control analysis: a second right-hand side g^c = sum_k (rho_k/r_k) d^c_k Yp_k^T in every solve,
  // w^c = V diag(1/mu) V^T g^c, and per row ctl_out = ctl_in + x' . w^c; null: off (kLetkfMembers and kLetkfPerts only)
  const double* dc;     // [P] value - H(x_c) of every ob with an effective flag of 1, 0 for the others
  const double* ctl_in; // kLetkfMembers: [n_lead * npts] the control's rows; kLetkfPerts: [npts] its ob estimates ...
  double* ctl_out;      // ... and their analysis (kLetkfMembers: the same address, or clear of ctl_in; read and written by the row's wave)
};
int letkf_threads(int M, bool ctl = false);       // the workgroup size chosen for M members (ctl: with the control's column in the Gram)
size_t letkf_lds_bytes(int M, bool ctl = false);  // and its dynamic LDS (ctl: the stage of M + 2 columns and one more M-vector)
// a wave per ob: prior_mean, prior_var (ddof 0), the effective flag (the requested one, and with t2 > 0 the outlier check's verdict
// d^2 <= t2 (s2 + error), exactly as the prep launch decides it) as a byte and as the coefficient-shaped act [P][4] the list
// builders read, and dr [P][2]; an ob with an effective flag of 0 leaves the neutral (0, 1) there, whatever its value and error
hipError_t launch_letkf_prior(long P, int M, const double* Yp, const double* ym, const double* ob_value, const double* ob_error,
                              const double* ob_req, double t2, double* prior_mean, double* prior_var, uint8_t* assimilated, double* act,
                              double* dr, hipStream_t s);
// a thread per ob: dc[k] = value[k] - yc[k] where assimilated[k] (k_letkf_prior's verdict), else the neutral 0 (value and yc not read)
hipError_t launch_letkf_control_prior(long P, const double* ob_value, const double* yc, const uint8_t* assimilated, double* dc,
                                      hipStream_t s);
// The cap on the local obs of a solve, between launch_gc_fill and the solve: per point and class, of the listed obs
// with a non-zero taper the cap[c] with the largest taper keep it (equal bits: list order), the others' tapers become 0.0, which every
// reader of the lists takes as "not listed".  A point at which no class is over its cap is not written.
constexpr int kLetkfCapClasses = 32;
struct LetkfCapArgs {
  long npts;
  const long* off;      // the lists of launch_gc_fill over these points
  const int* cnt;
  const int* idx;
  double* wts;
  const int* ob_class;  // [P] 0..nclass-1, or null: every ob is of class 0
  int nclass;
  int cap[kLetkfCapClasses];  // 0: no limit for the class
  double* reach;        // [npts] the non-zero tapers of the point before the cap, as a double; or null
};
hipError_t launch_letkf_cap(const LetkfCapArgs& a, hipStream_t s);
// ---- weight interpolation (efa_letkf_interp.hip): [T | w] solved at the nodes of a coarse mesh of grid columns,
// interpolated bilinearly in grid-index space to every column and applied to its rows
struct LetkfMesh {
  long ny, nx;        // the grid: column c = iy * nx + ix
  long sy, sx;        // the node stride on each axis, 1 <= s <= max(n - 1, 1) (a longer stride gives the nodes of n - 1: the two ends)
  // nodes of an axis: 0, s, 2 s, .. below n - 1, and n - 1 itself (the last cell may be shorter)
  __host__ __device__ static long axis_nodes(long n, long s) { return n <= 1 ? 1 : (n - 1 + s - 1) / s + 1; }
  __host__ __device__ static long axis_node(long j, long n, long s) { return j * s < n - 1 ? j * s : n - 1; }
  __host__ __device__ long nyn() const { return axis_nodes(ny, sy); }
  __host__ __device__ long nxn() const { return axis_nodes(nx, sx); }
  __host__ __device__ long nnodes() const { return nyn() * nxn(); }
  __host__ __device__ long ncol() const { return ny * nx; }
  bool unit() const { return sy == 1 && sx == 1; }
};
struct LetkfInterpArgs {
  LetkfMesh mesh;
  long n_lead;         // rows per column, row lead * ncol + col
  int M;
  const void* Xin;     // [n_lead * ncol][M] prior members ...
  void* Xout;          // ... and posterior members (the same address, or clear of Xin)
  const double* Tw;    // [nnodes][M][M + 1] the node pairs, as kLetkfWeights writes them
  const double* stats; // [nnodes][3] of the node solves, n_local first; null: every node counts as reached
  int relax_kind;      // EFA_RELAX_*: RTPP on the interpolated T, RTPS per row
  double relax_alpha;
};
size_t letkf_interp_lds_bytes(int M);

// ---- vertical, temporal and variable localisation of the LETKF: one solve per (slab group, column) -------------
// Slabs whose factors agree for every ob form a group; group g is solved under rho_k(c) * S[k][rep[g]] and maps the rows of its
// slabs grp_leads[grp_off[g] .. grp_off[g + 1]) only.
struct LetkfGroups {
  int ngroups;
  long s_pitch;          // slabs of the table
  const double* S;       // [P][s_pitch] the slab factor table (launch_slab_factor)
  const int* rep;        // [ngroups] the first slab of every group
  const int* grp_off;    // [ngroups + 1]
  const int* grp_leads;  // [n_lead] the slabs, group by group, ascending within a group
};
// k_letkf: one workgroup per point; a.Xin / a.Xout are rows of `elem` (kLetkfMembers; the other modes are float64 only).
// grp (the SLAB switch): npts * ngroups solves, the group the fastest index of the launch; stats [ngroups][npts][3], Tw
// [ngroups][npts][M][M + 1].  kLetkfMembers and kLetkfWeights only (the obs block runs the plain kLetkfPerts launch on lists that
// launch_letkf_obs_factor scaled).
hipError_t launch_letkf(const LetkfArgs& a, const LetkfGroups* grp, int mode, Elem elem, hipStream_t s);
// ---- cross validation over member groups (Buehner 2020): the perturbations of a group are updated with the gain of the
// other groups' members; the mean keeps the full solve
struct LetkfCv {
  int ngroups;        // K >= 2
  const int* perm;    // [K][M] per group k: the members with another label ascending (the independent set I), then those with label k (H)
  const int* nind;    // [K] |I| >= 2 of every group
  double* C;          // [npts][M][M] scratch: the Gram matrix C of every point, written and re-read by the point's own workgroup
  double* stats;      // [npts][2] {the sub-solves' sweeps summed, their largest max mu / min mu} or null
};
// k_letkf_cv: kLetkfWeights under cross validation, a.Tw [npts][M][M + 1] = the recentred T | w of every point (T is not symmetric:
// row a holds what member a's prior perturbation contributes to every posterior one); a.stats as launch_letkf writes them.  With
// a.Yp_in (and ym_in, ym_out, Yp_out, clear of the inputs) point j's row of the obs block is mapped by its own pair as well.
hipError_t launch_letkf_cv(const LetkfArgs& a, const LetkfCv& cv, hipStream_t s);
// k_letkf_interp: one workgroup per column; a.Xin / a.Xout are rows of `elem`.  grp (the SLAB switch): one per (column, group), node
// pairs Tw [ngroups][nnodes][M][M + 1] and node statistics [ngroups][nnodes][3]; the table and rep are not read.
hipError_t launch_letkf_interp(const LetkfInterpArgs& a, const LetkfGroups* grp, Elem elem, hipStream_t s);
// the lists built at the P ob positions (blocks of 16 points): wts[e * 16 + cb] *= F(j, idx[e]), j = blk * 16 + cb, with
// F(j, k) = (V(j,k) T(j,k)) C[k, v_j] of §7t (ob_vert null: V = 1; slab null: T = C = 1); a zero stays zero
hipError_t launch_letkf_obs_factor(long P, const long* off, const int* cnt, const int* idx, double* wts, const double* ob_vert,
                                   const double* ob_vhw, const SlabObs* slab, hipStream_t s);

hipError_t launch_results_to_host(const void* src_dev, void* dst_host, size_t bytes, const int* st_dev, int* st_host, hipStream_t s);
// diagnostic: `blocks` workgroups that hold `lds_bytes` of LDS each and spin for `ms` milliseconds
hipError_t launch_occupy(int blocks, size_t lds_bytes, double ms, hipStream_t s);
hipError_t launch_contract_f32(long N, int M, long P, const float* X, const float* Ye, float* C, hipStream_t s);

}  // namespace efa
