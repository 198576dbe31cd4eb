// Observation impact (EFSO; Kalnay et al. 2012, Ota et al. 2013): for every assimilated ob k
//   J_k = (1/(M-1)) (d_k / r_k) sum_i rho_ik v_i (Xf'_i . Ya'_k),
// Xf' the forecast perturbations (rows x M), Ya' the analysis perturbations in observation space (P x M), v the weighted error sum
// of every state row, rho the taper the assimilation itself uses (1 without localisation).
//
// Localised: k_sweep_gc_lane_impact, a sibling of the one-pass sweep's row-per-lane kernel (efa_gcsweep_kernels.h) -- the same
// workgroup per (column block of 16, group of 16 slabs), lane per row, active list staged 32 obs at a time, wave-level skipping of
// zero tapers -- that writes no state: per staged ob the lanes' contributions are added across the workgroup in a fixed order and
// one partial sum per (group of slabs, list entry) is written.  k_impact_gather / k_impact_finish add the partials per ob, again in
// a fixed order: no floating-point atomics anywhere, two calls on the same inputs agree bit for bit.
// Its template parameter FAC adds the factor of every (staged ob, slab) pair: the vertical one, or under the temporal and variable
// tapers the entry of the context's slab table.
// Unlocalised: z = Xf'^T v by a grid-stride two-stage reduction, then J_k = scale_k (Ya'_k . z).
#include "efa_device.h"
#include "efa_driver.h"
#include "efa_lane_dot.h"

#include <cmath>
#include <vector>

namespace efa {
namespace {

constexpr int kBlkCols = 16;       // columns per block of the active lists (efa_gcsweep.hip builds them)
constexpr int kImpChunk = 32;      // list entries staged at a time (a 64-bit mask of them per wave)
constexpr int kImpLaneMax = 104;   // a lane holds a whole row up to here; above, the row goes through in pieces of kImpPiece members
constexpr int kImpPiece = 64;      // (the contraction is linear in the dot product, so the pieces' contributions simply add)
constexpr int kCS = 65;            // doubles per staged ob in cs: 4 waves x 16 quads, padded against bank conflicts

// members [m0, m0 + MP) of the row at p (zeros beyond M); vec: M even and the row 16-byte aligned
template <int MP>
__device__ __forceinline__ void load_piece(const double* __restrict__ p, int M, int m0, bool vec, double (&x)[MP]) {
  if (vec) {
    const double2* p2 = reinterpret_cast<const double2*>(p + m0);
#pragma unroll
    for (int i = 0; i < MP / 2; ++i) {
      const double2 t = (m0 + 2 * i < M) ? p2[i] : make_double2(0.0, 0.0);
      x[2 * i] = t.x;
      x[2 * i + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < MP; ++i) x[i] = (m0 + i < M) ? p[m0 + i] : 0.0;
  }
}

// The factor of a (staged ob, slab of the group) pair on top of the horizontal taper: none, the vertical factor evaluated while
// staging, or the context's slab table S[P][n_lead] = (V T) C, which carries the vertical factor
// too: 16 consecutive doubles per staged ob are loaded from a.slab_tab where the vertical form evaluates vert_factor
enum ImpactFactor { kFacNone = 0, kFacVert = 1, kFacTable = 2 };

// MP: members a lane holds at a time, a multiple of 4.  FAC: the factor on top of the horizontal taper (ImpactFactor).
// WIDE false: MP is M padded (M <= 104), the row mean comes from the registers as in the sweep's member form.  WIDE true: pieces
// of MP members, the mean from a first pass over the row.
// Two waves per SIMD while the row, the two ye register sets and the accumulators fit 256 registers (up to 96 members, no spills); one above.
// One kernel body and no helper function around it: a __forceinline__ function handed the arguments compiles to other code
// (DESIGN.md 7u).
template <int MP, int FAC, bool WIDE>
__global__ __launch_bounds__(256, (MP > 96 ? 1 : 2)) void k_sweep_gc_lane_impact(const ImpactGcArgs a) {
  constexpr int NG = (MP + 15) / 16;  // ye registers per lane
  constexpr int YS = 16 * NG;         // padded ye row in LDS (doubles)
  __shared__ __align__(16) double ye_s[kImpChunk * YS];
  __shared__ __align__(16) double w_s[kImpChunk * kBlkCols];         // the taper per (staged ob, column)
  __shared__ __align__(16) double vf_s[FAC != kFacNone ? kImpChunk * 16 : 1];   // the factor per (staged ob, slab of the group)
  __shared__ double cs[kImpChunk * kCS];                             // per (staged ob, wave, quad): the quad's contribution
  __shared__ unsigned long long todo_s[4];                           // per wave: the staged obs it did not skip
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  // the hand-out order of k_sweep_gc_lane: blocks longest list first, a block's groups of slabs next to each other
  const long pos = blockIdx.x / a.lead_split;
  const long b = a.order[pos];
  const int grp = (int)((blockIdx.x % a.lead_split + pos) % a.lead_split);
  const int lead0 = 16 * grp;
  const int lead_hi = (lead0 + 16 < (int)a.n_lead) ? lead0 + 16 : (int)a.n_lead;
  const int M = a.M;
  const long e0 = a.off[b], e1 = e0 + a.cnt[b];
  const auto seq = std::make_integer_sequence<int, MP>{};
  // 16 slabs x 4 columns per wave; a group of fewer slabs: the next power of two, more columns per wave (as the sweep folds it)
  const int rem = lead_hi - lead0;
  const int lg_cols = (rem > 8) ? 2 : (rem > 4) ? 3 : (rem > 2) ? 4 : (rem > 1) ? 5 : 6;
  const int ncw = 1 << lg_cols;
  const int cq = (lane & (ncw - 1)) + ncw * wave;
  const int lead = lead0 + (lane >> lg_cols);
  const long col = b * kBlkCols + cq;
  const bool live = cq < kBlkCols && col < a.ncol && lead < lead_hi;
  const bool any_live = __ballot(live) != 0ull;
  const long row = live ? (long)lead * a.ncol + col : 0;
  const double* xrow = a.X + (size_t)row * M;
  const bool vec = (M % 2 == 0) && ((reinterpret_cast<uintptr_t>(a.X) & 15u) == 0);
  const double vi = live ? a.v[row] : 0.0;
  double xm = 0.0;
  if (WIDE && live) {  // the row mean, ahead of the pieces
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int i = 0;
    for (; i + 4 <= M; i += 4) {
      s0 += xrow[i];
      s1 += xrow[i + 1];
      s2 += xrow[i + 2];
      s3 += xrow[i + 3];
    }
    for (; i < M; ++i) s0 += xrow[i];
    xm = ((s0 + s1) + (s2 + s3)) / (double)M;
  }
  const double* wq = w_s + (cq & (kBlkCols - 1));  // (a lane beyond the block's 16 columns holds a zero row: whatever it reads is multiplied by 0)
  const double* yq = ye_s + (lane & 15);
  const double* vq = vf_s + (FAC != kFacNone ? (lane >> lg_cols) : 0);  // the lane's slab slot (< 16 in every layout)

  for (int m0 = 0; m0 < (WIDE ? M : 1); m0 += MP) {
    double x[MP];
    if (live) {
      load_piece<MP>(xrow, M, m0, vec, x);
      if (!WIDE) {  // remove the ensemble mean as the sweep's member form does
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
        for (int i = 0; i < MP; i += 4) {
          s0 += x[i];
          s1 += x[i + 1];
          s2 += x[i + 2];
          s3 += x[i + 3];
        }
        xm = ((s0 + s1) + (s2 + s3)) / (double)M;
      }
#pragma unroll
      for (int i = 0; i < MP; ++i) x[i] = (m0 + i < M) ? (x[i] - xm) * vi : 0.0;  // v_i Xf'_i
    } else {
#pragma unroll
      for (int i = 0; i < MP; ++i) x[i] = 0.0;
    }
    for (long c0 = e0; c0 < e1; c0 += kImpChunk) {
      const int ne = (int)((e1 - c0 < kImpChunk) ? (e1 - c0) : kImpChunk);
      __syncthreads();  // previous chunk fully consumed
      for (int i = tid; i < ne * YS; i += 256) {
        const int ee = i / YS, m = i - ee * YS;
        const int k = a.idx[c0 + ee];
        ye_s[i] = (m < MP && m0 + m < M) ? a.Yp[(size_t)k * M + m0 + m] : 0.0;
      }
      for (int i = tid; i < ne * kBlkCols; i += 256) w_s[i] = a.wts[(size_t)c0 * kBlkCols + i];
      if (FAC == kFacVert)
        for (int i = tid; i < ne * 16; i += 256) {
          const int lead_i = lead0 + (i & 15);
          const int k = a.idx[c0 + (i >> 4)];
          vf_s[i] = (lead_i < lead_hi) ? vert_factor(a.lead_vert[lead_i], a.ob_vert[k], a.ob_vhw[k]) : 0.0;
        }
      if (FAC == kFacTable)
        for (int i = tid; i < ne * 16; i += 256) {
          const int lead_i = lead0 + (i & 15);
          const int k = a.idx[c0 + (i >> 4)];
          vf_s[i] = (lead_i < lead_hi) ? a.slab_tab[(size_t)k * a.n_lead + lead_i] : 0.0;  // 16 consecutive doubles per staged ob
        }
      __syncthreads();
      // the staged obs with a non-zero taper on any of this wave's columns (and, with a factor, any of its slabs): wave-uniform mask
      bool mine = false;
      if (lane < ne && any_live) {
        const int c_lo = ncw * wave, c_hi = (c_lo + ncw < kBlkCols) ? c_lo + ncw : kBlkCols;
        for (int c = c_lo; c < c_hi; ++c) mine = mine || (w_s[lane * kBlkCols + c] != 0.0);
        if (FAC != kFacNone && mine) {
          bool vz = false;
          for (int t = 0; t < (64 >> lg_cols) && t < 16; ++t) vz = vz || (vf_s[lane * 16 + t] != 0.0);
          mine = vz;
        }
      }
      unsigned long long todo = __ballot(mine);
      if (lane == 0) todo_s[wave] = todo;
      if (todo != 0ull) {
        // Two ye register sets taken in turn: the LDS reads of the next ob's members are issued ahead of this ob's dot, and each
        // set is written by LDS reads only (no register copy between the sets: a VALU write ahead of a DPP read is the hazard
        // efa_lane_dot.h describes)
        auto one_ob = [&](int ee, const double (&y)[NG]) {
          double w = wq[ee * kBlkCols];
          if (FAC != kFacNone) w = w * vq[ee * 16];  // horizontal taper times the slab's factor, rounded once as the sweep does
          const double dot = lane_dot<MP>(x, y, seq);
          const double q = quad_sum(w * dot);
          if ((lane & 3) == 0) cs[ee * kCS + 16 * wave + (lane >> 2)] = q;
        };
        double ya[NG], yb[NG];
        int ea = __builtin_ctzll(todo), eb = 0;
        todo &= todo - 1;
#pragma unroll
        for (int c = 0; c < NG; ++c) ya[c] = yq[ea * YS + 16 * c];
        while (true) {
          const bool more_b = todo != 0ull;
          if (more_b) {
            eb = __builtin_ctzll(todo);
            todo &= todo - 1;
#pragma unroll
            for (int c = 0; c < NG; ++c) yb[c] = yq[eb * YS + 16 * c];
          }
          one_ob(ea, ya);
          if (!more_b) break;
          const bool more_a = todo != 0ull;
          if (more_a) {
            ea = __builtin_ctzll(todo);
            todo &= todo - 1;
#pragma unroll
            for (int c = 0; c < NG; ++c) ya[c] = yq[ea * YS + 16 * c];
          }
          one_ob(eb, yb);
          if (!more_a) break;
        }
      }
      __syncthreads();
      // per staged ob: its 4 x 16 quad sums in a fixed order (thread 4e + w adds wave w's sixteen, the four are added by quad_sum)
      {
        const int e = tid >> 2, wv = tid & 3;
        double s = 0.0;
        if (e < ne && ((todo_s[wv] >> e) & 1ull)) {
          const double* p = cs + e * kCS + 16 * wv;
#pragma unroll
          for (int i = 0; i < 16; ++i) s += p[i];
        }
        s = quad_sum(s);
        if (e < ne && wv == 0) {
          double* out = a.partial + (size_t)grp * a.cap + (c0 + e);
          *out = (m0 == 0) ? s : *out + s;  // (a later piece: the same thread wrote the earlier ones)
        }
      }
    }
  }
}

// ---- the partials per ob, in a fixed order -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_impact_gather(long nblk, long per, long P, const long* __restrict__ off,
                                                       const int* __restrict__ cnt, const int* __restrict__ idx,
                                                       const double* __restrict__ partial, long cap, int lead_split, double* acc2) {
  double* acc = acc2 + (size_t)blockIdx.x * P;
  for (long k = threadIdx.x; k < P; k += 256) acc[k] = 0.0;
  __syncthreads();
  const long b_lo = (long)blockIdx.x * per, b_hi = (b_lo + per < nblk) ? b_lo + per : nblk;
  for (long b = b_lo; b < b_hi; ++b) {  // an ob appears once in a block's list: the threads of one step never meet
    const long e0 = off[b];
    const int n = cnt[b];
    for (int e = threadIdx.x; e < n; e += 256) {
      double s = 0.0;
      for (int g = 0; g < lead_split; ++g) s += partial[(size_t)g * cap + e0 + e];
      acc[idx[e0 + e]] += s;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_impact_finish(long P, int ranges, const double* __restrict__ acc2,
                                                       const double* __restrict__ scale, double* __restrict__ impact) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= P) return;
  double s = 0.0;
  for (int r = 0; r < ranges; ++r) s += acc2[(size_t)r * P + k];
  const double sc = scale[k];
  impact[k] = (sc == 0.0 || s == 0.0) ? 0.0 : sc * s;  // an ob not used, or out of reach of every row: exactly 0
}

// ---- unlocalised ---------------------------------------------------------------------------------------------------------------
constexpr int kZBlocks = 1024;  // grid cap of k_impact_z: workgroups of 4 waves, a row per wave and trip

__global__ __launch_bounds__(256) void k_impact_z(long rows, int M, const double* __restrict__ X, const double* __restrict__ v,
                                                  double* __restrict__ zpart) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * 4;
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  for (long row = wave; row < rows; row += nwaves) {
    const double vi = v[row];
    if (vi == 0.0) continue;  // (wave-uniform) a row that is not verified adds nothing
    const double* p = X + (size_t)row * M;
    double x[4];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = lane + 64 * j;
      x[j] = (m < M) ? p[m] : 0.0;
      s += x[j];
    }
    const double mean = wave_sum(s) / (double)M;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lane + 64 * j < M) z[j] = __builtin_fma(vi, x[j] - mean, z[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) zpart[(size_t)wave * 256 + lane + 64 * j] = z[j];
}

__global__ __launch_bounds__(256) void k_impact_zsum(long nwaves, const double* __restrict__ zpart, double* __restrict__ z) {
  double s = 0.0;
  for (long w = 0; w < nwaves; ++w) s += zpart[(size_t)w * 256 + threadIdx.x];
  z[threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_impact_none(long P, int M, const double* __restrict__ Yp, const double* __restrict__ z,
                                                     const double* __restrict__ scale, double* __restrict__ impact) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= P) return;
  const double sc = scale[k];
  double s = 0.0;
  if (sc != 0.0)
    for (int m = 0; m < M; ++m) s = __builtin_fma(Yp[(size_t)k * M + m], z[m], s);
  impact[k] = (sc == 0.0 || s == 0.0) ? 0.0 : sc * s;
}

template <int MP, bool WIDE>
hipError_t impact_launch_one(const ImpactGcArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)(a.nblk * a.lead_split)), block(256);
  if (a.slab_tab) hipLaunchKernelGGL((k_sweep_gc_lane_impact<MP, kFacTable, WIDE>), grid, block, 0, s, a);
  else if (a.lead_vert) hipLaunchKernelGGL((k_sweep_gc_lane_impact<MP, kFacVert, WIDE>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_sweep_gc_lane_impact<MP, kFacNone, WIDE>), grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace

int impact_lead_split(long n_lead) { return (int)((n_lead + 15) / 16); }

hipError_t launch_impact_gc(const ImpactGcArgs& a0, hipStream_t s) {
  if (a0.M < 2 || a0.M > kMaxMembers) return hipErrorInvalidValue;
  if (a0.nblk <= 0 || a0.n_lead <= 0 || a0.cap <= 0) return hipSuccess;
  ImpactGcArgs a = a0;
  a.lead_split = impact_lead_split(a.n_lead);
  if (a.M > kImpLaneMax) return impact_launch_one<kImpPiece, true>(a, s);
  return dispatch_width((a.M + 3) / 4, WidthRange<1, kImpLaneMax / 4>{}, [&](auto q) { return impact_launch_one<4 * q, false>(a, s); });
}

int impact_reduce_ranges(long nblk, long P) {
  long r = nblk < 1024 ? nblk : 1024;
  const long fit = (8L << 20) / (P > 0 ? P : 1);  // acc [ranges][P] within 64 MiB
  if (r > fit) r = fit;
  return (int)(r < 1 ? 1 : r);
}

hipError_t launch_impact_reduce(long nblk, long P, const long* off, const int* cnt, const int* idx, const double* partial, long cap,
                                int lead_split, const double* scale, double* acc, double* impact, hipStream_t s) {
  if (P <= 0) return hipSuccess;
  const int ranges = impact_reduce_ranges(nblk, P);
  const long per = (nblk + ranges - 1) / ranges;
  hipLaunchKernelGGL(k_impact_gather, dim3((unsigned)ranges), dim3(256), 0, s, nblk, per, P, off, cnt, idx, partial, cap, lead_split, acc);
  hipLaunchKernelGGL(k_impact_finish, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, ranges, acc, scale, impact);
  return hipGetLastError();
}

long impact_z_waves() { return 4L * kZBlocks; }

hipError_t launch_impact_none(long rows, int M, long P, const double* X, const double* v, const double* Yp, const double* scale,
                              double* zpart, double* z, double* impact, hipStream_t s) {
  if (M < 2 || M > kMaxMembers) return hipErrorInvalidValue;
  if (P <= 0) return hipSuccess;
  long blocks = (rows + 3) / 4;
  if (blocks > kZBlocks) blocks = kZBlocks;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_impact_z, dim3((unsigned)blocks), dim3(256), 0, s, rows, M, X, v, zpart);
  hipLaunchKernelGGL(k_impact_zsum, dim3(1), dim3(256), 0, s, blocks * 4, zpart, z);
  hipLaunchKernelGGL(k_impact_none, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, M, Yp, z, scale, impact);
  return hipGetLastError();
}

}  // namespace efa

// ---- the host side of efa_obs_impact_dev ----------------------------------------------------------------------------------------
namespace efa_host {

using namespace efa;

namespace {
int make_event(OwnedEvent& e) {
  if (!e.h) EFA_HIP(hipEventCreate(&e.h));
  return EFA_OK;
}
}  // namespace

// Everything the call needs lives in buffers of its own (imp_*): the context's cached lists, obs-obs taper table, geometry serial,
// trajectory, column grid, options and timing sums are neither read (but for the vertical and the slab setting) nor written.
// slab: the call is efa_obs_impact_slab_dev with the slab setting on -- the contraction runs under GC_h(col, k) S(k, slab), S the
// context's factor table, whose cache (keyed by the two settings' serials) is the one thing of the context it writes.
// slab_entry: the call came through efa_obs_impact_slab_dev, which with the slab setting off IS efa_obs_impact_dev.
int obs_impact(efa_ctx* c, long rows, int M, long P, const double* Xf_dev, const double* werr_dev, const double* Ya_dev, const ObsIn& ob,
               const double* grid_lat, const double* grid_lon, long ncol, long n_lead, double* impact, bool slab_entry) {
  const bool slab = slab_entry && c->sl_on;
  const char* me = slab ? "efa_obs_impact_slab_dev" : "efa_obs_impact_dev";
  const double *innov = ob.value, *ob_error = ob.error, *ob_lat = ob.lat, *ob_lon = ob.lon, *ob_hw = ob.hw;
  const uint8_t* ob_used = ob.assim;
  const int loc_mode = ob.loc_mode;
  const bool gc = loc_mode == EFA_LOC_GC;
  if (loc_mode != EFA_LOC_NONE && !gc) return fail(EFA_ERR_INVALID, "%s: loc_mode %d is neither EFA_LOC_NONE nor EFA_LOC_GC", me, loc_mode);
  if (M < 2 || M > kMaxMembers) return fail(EFA_ERR_INVALID, "%s: M=%d must be in [2,%d]", me, M, kMaxMembers);
  if (rows < 0 || P < 0 || ncol < 0 || n_lead < 0) return fail(EFA_ERR_INVALID, "%s: negative size", me);
  if (ncol * n_lead != rows) return fail(EFA_ERR_INVALID, "%s: rows=%ld must equal n_lead*ncol = %ld*%ld", me, rows, n_lead, ncol);
  if (c->sl_on && !slab)  // (its kernels have no temporal or variable factor: refused rather than computed under another taper)
    return fail(EFA_ERR_INVALID, "slab localisation is set: efa_obs_impact_dev does not support the temporal and variable tapers");
  if (slab) {
    if (!gc) return fail(EFA_ERR_INVALID, "slab localisation is set: the impact call needs GC localisation (loc_mode %d)", loc_mode);
    if (P != c->sl_P) return fail(EFA_ERR_INVALID, "slab localisation was set for %ld observations, the impact call has %ld", c->sl_P, P);
    if (n_lead != c->sl_nlead) return fail(EFA_ERR_INVALID, "slab localisation was set for %ld slabs, the impact call has n_lead=%ld", c->sl_nlead, n_lead);
    if (c->vl_on && (P != c->vl_P || n_lead != c->vl_nlead))  // (the table takes its vertical factors from that setting)
      return fail(EFA_ERR_INVALID, "slab localisation is set with vertical localisation, which was set for %ld observations and %ld slabs; the impact call has %ld and %ld",
                  c->vl_P, c->vl_nlead, P, n_lead);
  }
  if (c->vl_on) {
    if (!gc) return fail(EFA_ERR_INVALID, "vertical localisation is set: the impact call needs GC localisation (loc_mode %d)", loc_mode);
    if (P != c->vl_P) return fail(EFA_ERR_INVALID, "vertical localisation was set for %ld observations, the impact call has %ld", c->vl_P, P);
    if (n_lead != c->vl_nlead) return fail(EFA_ERR_INVALID, "vertical localisation was set for %ld slabs, the impact call has n_lead=%ld", c->vl_nlead, n_lead);
  }
  if (P == 0) {
    c->impact_us = 0;
    return EFA_OK;
  }
  if (!innov || !ob_error || !ob_used || !impact) return fail(EFA_ERR_INVALID, "%s: null per-observation array", me);
  if (!Ya_dev || (rows > 0 && (!Xf_dev || !werr_dev))) return fail(EFA_ERR_INVALID, "%s: null device pointer", me);
  if (gc && (!ob_lat || !ob_lon || !ob_hw || (rows > 0 && (!grid_lat || !grid_lon))))
    return fail(EFA_ERR_INVALID, "%s: GC localisation needs ob_lat/ob_lon/ob_halfwidth_km and grid_lat/grid_lon", me);
  // the per-ob pack: [used (coefficient-shaped: the list builders read [3]) | scale | lat | lon | half-width]
  std::vector<double> pack((size_t)P * (kCoefStride + 4), 0.0);
  double *h_used = pack.data(), *h_scale = h_used + (size_t)P * kCoefStride, *h_lat = h_scale + P, *h_lon = h_lat + P, *h_hw = h_lon + P;
  long n_used = 0;
  for (long k = 0; k < P; ++k) {
    h_hw[k] = 1.0;  // (an ob that is not used is never looked at; its half-width may be anything)
    if (!ob_used[k]) continue;
    if (!std::isfinite(innov[k])) return fail(EFA_ERR_INVALID, "%s: observation %ld is used but its innovation is not finite", me, k);
    if (!(std::isfinite(ob_error[k]) && ob_error[k] > 0.0))
      return fail(EFA_ERR_INVALID, "%s: observation %ld is used but its error variance %g is not finite and > 0", me, k, ob_error[k]);
    if (gc) {
      if (std::isnan(ob_hw[k])) return fail(EFA_ERR_INVALID, "%s: observation %ld is used but its half-width is NaN", me, k);
      h_lat[k] = ob_lat[k];
      h_lon[k] = ob_lon[k];
      h_hw[k] = ob_hw[k];
    }
    h_used[(size_t)k * kCoefStride + 3] = 1.0;
    h_scale[k] = (1.0 / (double)(M - 1)) * (innov[k] / ob_error[k]);
    ++n_used;
  }
  c->impact_us = 0;
  for (long k = 0; k < P; ++k) impact[k] = 0.0;
  if (n_used == 0 || rows == 0) return EFA_OK;

  hipStream_t s = c->stream;
  const size_t dP = (size_t)P * sizeof(double);
  // device: the pack | obtrig [P][6] | impact [P]
  EFA_TRY(c->imp_ob.reserve(pack.size() * sizeof(double) + 7 * dP));
  double* d_used = c->imp_ob.as<double>();
  double *d_scale = d_used + (size_t)P * kCoefStride, *d_lat = d_scale + P, *d_lon = d_lat + P, *d_hw = d_lon + P;
  double *d_trig = d_hw + P, *d_out = d_trig + 6 * P;
  EFA_HIP(hipMemcpyAsync(d_used, pack.data(), pack.size() * sizeof(double), hipMemcpyHostToDevice, s));
  // Ya' with the existing perturbation kernel; the caller's Ya_dev is read only
  EFA_TRY(c->imp_Yp.reserve((size_t)P * M * sizeof(double) + dP));
  double* Yp = c->imp_Yp.as<double>();
  EFA_HIP(launch_form_perts(P, M, Ya_dev, 1.0, Yp + (size_t)P * M, Yp, s));
  EFA_TRY(make_event(c->imp_iv.begin));
  EFA_TRY(make_event(c->imp_iv.end));
  if (!gc) {
    EFA_TRY(c->imp_part.reserve((size_t)(impact_z_waves() + 1) * 256 * sizeof(double)));
    double* zpart = c->imp_part.as<double>();
    EFA_HIP(hipEventRecord(c->imp_iv.begin, s));
    EFA_HIP(launch_impact_none(rows, M, P, Xf_dev, werr_dev, Yp, d_scale, zpart, zpart + (size_t)impact_z_waves() * 256, d_out, s));
    EFA_HIP(hipEventRecord(c->imp_iv.end, s));
  } else {
    // the active lists of the call's own geometry, built by the sweep's builders from the used flags
    const long nblk = gc_num_blocks(ncol);
    const size_t dC = (size_t)ncol * sizeof(double);
    EFA_TRY(c->imp_grid.reserve(2 * dC));
    double *g_lat = c->imp_grid.as<double>(), *g_lon = g_lat + ncol;
    EFA_HIP(hipMemcpyAsync(g_lat, grid_lat, dC, hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemcpyAsync(g_lon, grid_lon, dC, hipMemcpyHostToDevice, s));
    // [off (nblk + 1 longs) | cnt | ub | order (nblk ints each)]
    EFA_TRY(c->imp_blk.reserve((size_t)(nblk + 1) * sizeof(long) + (size_t)3 * nblk * sizeof(int)));
    long* off = c->imp_blk.as<long>();
    int *cnt = reinterpret_cast<int*>(off + nblk + 1), *ub = cnt + nblk, *order = ub + nblk;
    EFA_HIP(launch_gc_bound(ncol, P, g_lat, d_lat, d_hw, d_used, ub, off, s));
    long cap = 0;
    EFA_HIP(hipMemcpyAsync(&cap, off + nblk, sizeof(long), hipMemcpyDeviceToHost, s));
    EFA_HIP(hipStreamSynchronize(s));
    if (cap > 0) {
      const int split = impact_lead_split(n_lead);
      const int ranges = impact_reduce_ranges(nblk, P);
      EFA_TRY(c->imp_idx.reserve((size_t)cap * sizeof(int)));
      EFA_TRY(c->imp_wts.reserve((size_t)cap * 16 * sizeof(double)));  // the taper of a block's 16 columns per entry
      EFA_TRY(c->imp_part.reserve(((size_t)split * cap + (size_t)ranges * P) * sizeof(double)));
      double *partial = c->imp_part.as<double>(), *acc = partial + (size_t)split * cap;
      EFA_HIP(launch_gc_fill(ncol, P, g_lat, g_lon, d_lat, d_lon, d_hw, d_used, d_trig, off, cnt, c->imp_idx.as<int>(),
                             c->imp_wts.as<double>(), order, nullptr, s));
      ImpactGcArgs g{};
      g.ncol = ncol;
      g.n_lead = n_lead;
      g.M = M;
      g.nblk = nblk;
      g.off = off;
      g.cnt = cnt;
      g.order = order;
      g.idx = c->imp_idx.as<int>();
      g.wts = c->imp_wts.as<double>();
      g.Yp = Yp;
      g.X = Xf_dev;
      g.v = werr_dev;
      if (slab) {  // S = (V T) C: the vertical factor is in the table
        EFA_TRY(ensure_slab_table(c));
        g.slab_tab = c->sl_tab.as<double>();
      } else if (vl_active(c)) {
        g.lead_vert = vl_lead(c);
        g.ob_vert = vl_obvert(c);
        g.ob_vhw = vl_obvhw(c);
      }
      g.partial = partial;
      g.cap = cap;
      EFA_HIP(hipEventRecord(c->imp_iv.begin, s));
      EFA_HIP(launch_impact_gc(g, s));
      EFA_HIP(launch_impact_reduce(nblk, P, off, cnt, g.idx, partial, cap, split, d_scale, acc, d_out, s));
      EFA_HIP(hipEventRecord(c->imp_iv.end, s));
    } else {  // no used ob reaches a column
      EFA_HIP(hipEventRecord(c->imp_iv.begin, s));
      EFA_HIP(hipMemsetAsync(d_out, 0, dP, s));
      EFA_HIP(hipEventRecord(c->imp_iv.end, s));
    }
  }
  EFA_HIP(hipMemcpyAsync(impact, d_out, dP, hipMemcpyDeviceToHost, s));
  EFA_HIP(hipStreamSynchronize(s));
  float ms = 0.f;
  EFA_HIP(hipEventElapsedTime(&ms, c->imp_iv.begin, c->imp_iv.end));
  c->impact_us = (long)std::llround((double)ms * 1000.0);
  return EFA_OK;
}

}  // namespace efa_host
