// The local ensemble transform Kalman filter (LETKF, Hunt, Kostelich & Szunyogh 2007): one ensemble-space solve per
// column under the Gaspari-Cohn taper, the taper multiplying R^-1 (R-localisation).
//   For a location x (a grid column or an ob position), over the obs with an effective flag a_k = 1 (ob_assim[k], and the outlier
//   check's verdict when a threshold is set) and rho_k(x) = gaspari_cohn(distance(x, ob k), halfwidth_k) != 0, d_k = value_k - ym_k:
//     C_x = sum_k (rho_k/r_k) Yp_k^T Yp_k,  g_x = sum_k (rho_k/r_k) d_k Yp_k^T,  A_x = (M-1) I + C_x = V diag(mu) V^T,
//     T_x = V diag(sqrt((M-1)/mu)) V^T (the symmetric root),  w_x = V diag(1/mu) V^T g_x.
//   State rows: all n_lead rows of column c map with that column's pair, xam = xbm + Xbp w_c, Xap = Xbp T_c.  Obs block: all P rows
//   map, ob j with the pair solved at its own position.  Every solve reads the PRIOR obs block.
//
// k_letkf_prior   a wave per ob: prior_mean, prior_var, the effective flag, and {d_k, r_k} (the neutral (0, 1) for a flag of 0).
// k_letkf         ONE launch, one workgroup per column, in the block order k_gc_order leaves (longest list first, 16 columns per
//                 block: workgroup i takes column i & 15 of block order[i >> 4]).  Nothing of a column but its rows and its three
//                 statistics touches global memory.
//   1. Gram.      The block's listed obs rows [Yp_k | d_k], 32 at a time in ascending list order, staged in LDS (rows 16 (T | 1)
//                 doubles apart: consecutive rows half the banks apart); ONE MFMA operand scaled by rho_kc / r_k (no square root; a
//                 zero weight feeds exact zeros to both operands, so an ob that reaches a neighbour column only cannot bring its NaN);
//                 the upper 16 x 16 tiles of the (M+1)^2 product on v_mfma_f64_16x16x4_f64, up to three tiles per wave in registers,
//                 in k_gram / k_etkf_gram's lane layout.  Then A (mirrored, M-1 on the diagonal) and g to LDS, over the stage.
//   2. Eigen-solve: etkf_jacobi / etkf_factors (efa_etkf_eig.h) on the LDS array: V, mu, f = sqrt((M-1)/mu), h = (V^T g)/mu.
//   3. [T | w]    stay FACTORED in LDS, T = V diag(f) V^T, w = V h: at 136 members the array alone takes 148 of the 160 KB, a second
//                 M x M array does not fit, and the factored apply costs 4 M^2 flops per row where forming T costs 2 M^3 per column --
//                 less up to n_lead = M.  RTPP folds into f: (1-alpha) T + alpha I = V diag((1-alpha) f + alpha) V^T.
//   4. Apply.     Four rows at a time: members (or perturbations) to LDS, row mean and perturbations, z = V^T x' (16 lanes per
//                 (row, j)), xam = mean + h . z, x'_a = V (f z); RTPS per row from the two spreads at hand (§7b's formula).  Rows of
//                 float32 are widened on load and rounded once at the store.
//   kLetkfWeights skips 4 and writes T (as k_etkf_eig forms it: upper triangle, mirrored) and w of the point.
//   A column no ob reaches (n_local = 0) runs no solve: its rows are copied bit for bit, its statistics are (0, 0, 0), its pair (I, 0).
// Same inputs, same bits: every reduction has a fixed order, there are no floating-point atomics.
// Weight interpolation: the driver below also runs kLetkfWeights at the nodes of a coarse mesh of grid columns and
// hands the node pairs to k_letkf_interp (efa_letkf_interp.hip), which interpolates them to every column and applies them.
// Vertical, temporal and variable localisation (efa_letkf_slab_cycle_dev and its kin): k_letkf with the SLAB switch
// solves once per (slab group, column) under rho_k(c) * S[k][rep[g]], S the slab factor table of §7t; k_letkf_obs_factor scales the
// tapers of the lists built at the ob positions by the obs-obs factor F(j, k), after which the obs block runs as above.  The driver
// computes the groups from the host copies of the two settings (letkf_groups).
#include "efa_driver.h"
#include "efa_device.h"
#include "efa_etkf_eig.h"
#include "efa_rows.h"
#include "efa_slabfactor.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

namespace efa {
namespace {

typedef double letkf_v4 __attribute__((ext_vector_type(4)));

constexpr int kLetkfChunk = 32;  // obs per stage: 8 MFMA steps of 4
constexpr int kLetkfRows = 4;    // rows per apply batch (one wave each for the row reductions)
constexpr int kLetkfTiles = 3;   // tiles a wave may own
constexpr int kLetkfSmall = 16;  // doubles of per-row scalars: mean [4] | xam [4] | ssb [4] | (unused) [4]

__host__ __device__ inline int letkf_tiles_side(int M) { return (M + 1 + 15) / 16; }
__host__ __device__ inline int letkf_stage_pitch(int M) { return 16 * (letkf_tiles_side(M) | 1); }
// doubles of the region the stage and the M x M array share
__host__ __device__ inline int letkf_region(int M) {
  const int st = kLetkfChunk * letkf_stage_pitch(M) + kLetkfChunk, mm = M * M;
  return st > mm ? st : mm;
}

__global__ __launch_bounds__(256) void k_letkf_prior(long P, int M, const double* __restrict__ Yp, const double* __restrict__ ym,
                                                     const double* __restrict__ ob_value, const double* __restrict__ ob_error,
                                                     const double* __restrict__ ob_req, double t2, double* __restrict__ prior_mean,
                                                     double* __restrict__ prior_var, uint8_t* __restrict__ assimilated,
                                                     double* __restrict__ act, double* __restrict__ dr) {
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  for (long k = wave; k < P; k += nwaves) {
    const double* row = Yp + (size_t)k * M;
    double v[4];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = lane + 64 * j;
      v[j] = (m < M) ? row[m] : 0.0;
      s += v[j];
    }
    const double mean = wave_sum(s) / (double)M;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double e = (lane + 64 * j < M) ? v[j] - mean : 0.0;
      q += e * e;
    }
    const double s2 = wave_sum(q) / (double)M;
    if (lane == 0) {
      const double y = ym[k];
      bool on = ob_req[k] != 0.0;
      double d = 0.0, r = 1.0;
      if (on) {  // (value and error of an ob that is not requested are never read)
        r = ob_error[k];
        d = ob_value[k] - y;
        if (t2 > 0.0) on = d * d <= t2 * (s2 + r);  // a NaN rejects it
      }
      prior_mean[k] = y;
      prior_var[k] = s2;
      assimilated[k] = on ? 1 : 0;
      act[4 * k] = 0.0;
      act[4 * k + 1] = 0.0;
      act[4 * k + 2] = 0.0;
      act[4 * k + 3] = on ? 1.0 : 0.0;
      dr[2 * k] = on ? d : 0.0;
      dr[2 * k + 1] = on ? r : 1.0;
    }
  }
}

// upper tile ti of a T x T tile grid, row by row: (0,0) (0,1) .. (0,T-1) (1,1) ..
__device__ __forceinline__ void letkf_tile(int ti, int T, int* ta, int* tb) {
  int a = 0;
  while (ti >= T - a) {
    ti -= T - a;
    ++a;
  }
  *ta = a;
  *tb = a + ti;
}

template <typename E>
__device__ __forceinline__ E letkf_round(double v);
template <>
__device__ __forceinline__ double letkf_round<double>(double v) { return v; }
template <>
__device__ __forceinline__ float letkf_round<float>(double v) { return (float)v; }

// SLAB: one workgroup per (column, slab group), the group the fastest index of the launch so that the
// workgroups of a column run together and find its list and Yp rows in L2; the staged weight is fl(fl(rho S[k][rep[g]]) / r), the
// apply walks the group's slabs, the statistics and the pairs are laid out [group][point].
template <bool SLAB>
struct LetkfArgsOf { typedef LetkfArgs type; };
template <>
struct LetkfArgsOf<true> { typedef LetkfSlabArgs type; };

template <int MODE, typename E, int NTMAX, bool SLAB = false>
__global__ __launch_bounds__(NTMAX) void k_letkf(const typename LetkfArgsOf<SLAB>::type a) {
  extern __shared__ __align__(16) double letkf_smem[];
  const int M = a.M;
  const int tid = (int)threadIdx.x, nth = (int)blockDim.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nW = nth >> 6;
  const int T = letkf_tiles_side(M), Sp = letkf_stage_pitch(M), ntiles = T * (T + 1) / 2;
  double* G = letkf_smem;                     // the M x M array; before it the stage [32][Sp] | weights [32]
  double* wgt = G + kLetkfChunk * Sp;
  double* g_s = G + letkf_region(M);
  double* f_s = g_s + M;
  double* h_s = f_s + M;
  double* n_s = h_s + M;
  double* mu_s = n_s + M;
  double* x_s = mu_s + M;                     // [4][M] rows of a batch: members, perturbations, then posterior perturbations
  double* z_s = x_s + kLetkfRows * M;         // [4][M] V^T x'
  double* mean_s = z_s + kLetkfRows * M;
  double* xam_s = mean_s + kLetkfRows;
  double* ssb_s = xam_s + kLetkfRows;
  int* rot_s = reinterpret_cast<int*>(mean_s + kLetkfSmall);
  int* nloc_s = rot_s + 2;

  long bid = (long)blockIdx.x, grp = 0, lead0 = 0, nlead_g = a.n_lead;  // the group, its first entry in grp_leads, its slabs
  const double* Sg = nullptr;                                            // S[.][rep[grp]], pitch sp
  long sp = 0;
  const int* leads = nullptr;
  if constexpr (SLAB) {
    grp = bid % a.grp.ngroups;
    bid = bid / a.grp.ngroups;
    lead0 = a.grp.grp_off[grp];
    nlead_g = a.grp.grp_off[grp + 1] - lead0;
    sp = a.grp.s_pitch;
    Sg = a.grp.S + a.grp.rep[grp];
    leads = a.grp.grp_leads + lead0;
  }
  const long bi = bid >> 4;
  const int cb = (int)(bid & 15);
  const long blk = a.order ? (long)a.order[bi] : bi;
  const long col = blk * 16 + cb;
  if (col >= a.npts) return;  // (uniform)
  const long off = a.off ? a.off[blk] : 0;
  const int n = a.cnt ? a.cnt[blk] : 0;

  // n_local: the listed obs whose taper on THIS column is not zero
  if (wave == 0) {
    int cl = 0;
    for (int e = lane; e < n; e += 64) {
      double w = a.wts[(size_t)(off + e) * 16 + cb];
      if constexpr (SLAB) w = w * Sg[(size_t)a.idx[off + e] * sp];
      cl += (w != 0.0) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cl += __shfl_xor(cl, o, 64);
    if (lane == 0) *nloc_s = cl;
  }
  __syncthreads();
  const int nloc = *nloc_s;

  if (nloc == 0) {  // (uniform) no ob reaches the column: A = (M-1) I, no rotation, T = I, w = 0 -- the rows keep their bits
    if (MODE == kLetkfMembers) {
      const E* in = static_cast<const E*>(a.Xin);
      E* out = static_cast<E*>(a.Xout);
      if (in != out)
        for (long li = 0; li < nlead_g; ++li) {
          long l = li;
          if constexpr (SLAB) l = leads[li];
          const size_t base = (size_t)(l * a.npts + col) * M;
          for (int m = tid; m < M; m += nth) out[base + m] = in[base + m];
        }
    } else if (MODE == kLetkfPerts) {
      for (int m = tid; m < M; m += nth) a.Yp_out[(size_t)col * M + m] = a.Yp_in[(size_t)col * M + m];
      if (tid == 0) a.ym_out[col] = a.ym_in[col];
    } else {
      double* tw = a.Tw + (size_t)(grp * a.npts + col) * M * (M + 1);
      for (int e = tid; e < M * (M + 1); e += nth) {
        const int r = e / (M + 1), c = e - r * (M + 1);
        tw[e] = (r == c) ? 1.0 : 0.0;
      }
    }
    if (a.stats && tid < 3) a.stats[3 * (grp * a.npts + col) + tid] = 0.0;
    return;
  }

  // ---- 1. Gram ----------------------------------------------------------------------------------------------------------------
  {
    const int g = lane >> 4, nn = lane & 15;
    int ca[kLetkfTiles], cbt[kLetkfTiles];
    letkf_v4 acc[kLetkfTiles];
#pragma unroll
    for (int t = 0; t < kLetkfTiles; ++t) {
      const int ti = wave + t * nW;
      int ta = 0, tb = 0;
      if (ti < ntiles) letkf_tile(ti, T, &ta, &tb);
      ca[t] = 16 * ta + nn;
      cbt[t] = 16 * tb + nn;
      acc[t] = letkf_v4{0.0, 0.0, 0.0, 0.0};
    }
    const int nchunks = (n + kLetkfChunk - 1) / kLetkfChunk;
#pragma unroll 1
    for (int ch = 0; ch < nchunks; ++ch) {
      __syncthreads();  // the previous chunk is consumed
      for (int e = tid; e < kLetkfChunk * Sp; e += nth) {
        const int r = e / Sp, c = e - r * Sp;
        const int en = ch * kLetkfChunk + r;
        double v = 0.0;
        if (en < n && c <= M) {
          const long k = a.idx[off + en];
          v = (c < M) ? a.Yp[(size_t)k * M + c] : a.dr[2 * k];
        }
        G[e] = v;
      }
      if (tid < kLetkfChunk) {
        const int en = ch * kLetkfChunk + tid;
        double w = 0.0;
        if (en < n) {
          const long k = a.idx[off + en];
          w = a.wts[(size_t)(off + en) * 16 + cb];
          if constexpr (SLAB) w = w * Sg[(size_t)k * sp];
          w = w / a.dr[2 * k + 1];
        }
        wgt[tid] = w;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < kLetkfTiles; ++t) {
        if (wave + t * nW < ntiles) {  // (wave-uniform)
#pragma unroll
          for (int k = 0; k < kLetkfChunk / 4; ++k) {
            const int row = 4 * k + g;
            const double wv = wgt[row];
            const double ya = G[row * Sp + ca[t]], yb = G[row * Sp + cbt[t]];
            const double oa = (wv != 0.0) ? wv * ya : 0.0;  // a zero weight: exact zeros, whatever the row holds
            const double ob = (wv != 0.0) ? yb : 0.0;
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(oa, ob, acc[t], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();  // the stage is consumed: A goes over it
#pragma unroll
    for (int t = 0; t < kLetkfTiles; ++t) {
      const int ti = wave + t * nW;
      if (ti < ntiles) {
        int ta, tb;
        letkf_tile(ti, T, &ta, &tb);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int i = g + 4 * v, j = nn;
          const int I = 16 * ta + i, J = 16 * tb + j;
          if (ta == tb && i > j) continue;  // a diagonal tile holds each pair twice: the upper one is mirrored
          const double s = acc[t][v];
          if (I < M && J < M) {
            const double val = (I == J) ? s + (double)(M - 1) : s;
            G[I * M + J] = val;
            G[J * M + I] = val;
          } else if (I < M && J == M) {
            g_s[I] = s;
          }
        }
      }
    }
    __syncthreads();
  }

  // ---- 2. eigen-solve ---------------------------------------------------------------------------------------------------------
  const int sweeps = etkf_jacobi(M, G, n_s, rot_s, tid, nth);
  etkf_factors(M, G, g_s, mu_s, f_s, h_s, tid, nth);
  if (a.stats && wave == 0) {
    double s = 0.0;
    for (int j = lane; j < M; j += 64) s += (mu_s[j] - (double)(M - 1)) / mu_s[j];
    s = wave_sum(s);
    if (lane == 0) {
      a.stats[3 * (grp * a.npts + col)] = (double)nloc;
      a.stats[3 * (grp * a.npts + col) + 1] = s;
      a.stats[3 * (grp * a.npts + col) + 2] = (double)sweeps;
    }
  }

  // ---- 3. [T | w], factored ---------------------------------------------------------------------------------------------------
  if (MODE == kLetkfWeights) {
    double* tw = a.Tw + (size_t)(grp * a.npts + col) * M * (M + 1);
    etkf_assemble(M, G, f_s, h_s, tw, (size_t)(M + 1), tw + M, (size_t)(M + 1), tid, nth);
    return;
  }
  const bool rtps = MODE == kLetkfMembers && a.relax_kind == EFA_RELAX_RTPS && a.relax_alpha != 0.0;
  if (MODE == kLetkfMembers && a.relax_kind == EFA_RELAX_RTPP && a.relax_alpha != 0.0) {  // (uniform)
    for (int j = tid; j < M; j += nth) f_s[j] = (1.0 - a.relax_alpha) * f_s[j] + a.relax_alpha;
    __syncthreads();
  }

  // ---- 4. apply ---------------------------------------------------------------------------------------------------------------
  const int nslots = nth >> 4, slot = tid >> 4, sl = tid & 15;
  const long nrows = (MODE == kLetkfMembers) ? nlead_g : 1;
#pragma unroll 1
  for (long r0 = 0; r0 < nrows; r0 += kLetkfRows) {
    const int nr = (int)((nrows - r0 < kLetkfRows) ? nrows - r0 : kLetkfRows);
    for (int e = tid; e < nr * M; e += nth) {
      const int r = e / M, m = e - r * M;
      if (MODE == kLetkfMembers) {
        long l = r0 + r;
        if constexpr (SLAB) l = leads[l];
        x_s[e] = (double)static_cast<const E*>(a.Xin)[(size_t)(l * a.npts + col) * M + m];
      }
      else x_s[e] = a.Yp_in[(size_t)col * M + m];
    }
    __syncthreads();
    if (wave < nr) {  // the row's mean, its perturbations in place, the prior spread
      double* xr = x_s + wave * M;
      if (MODE == kLetkfMembers) {
        double s = 0.0;
        for (int m = lane; m < M; m += 64) s += xr[m];
        const double mean = wave_sum(s) / (double)M;
        double q = 0.0;
        for (int m = lane; m < M; m += 64) {
          const double p = xr[m] - mean;
          xr[m] = p;
          q = fma(p, p, q);
        }
        q = wave_sum(q);
        if (lane == 0) {
          mean_s[wave] = mean;
          ssb_s[wave] = q;
        }
      } else if (lane == 0) {
        mean_s[wave] = a.ym_in[col];
      }
    }
    __syncthreads();
    // z[r][j] = V_j . x'_r
#pragma unroll 1
    for (int pr = slot; pr < nr * M; pr += nslots) {
      const int r = pr / M, j = pr - r * M;
      const double* cj = G + (size_t)j * M;
      const double* xr = x_s + r * M;
      double d = 0.0;
      for (int i = sl; i < M; i += 16) d = fma(cj[i], xr[i], d);
      d = group_sum<16>(d);
      if (sl == 0) z_s[pr] = d;
    }
    __syncthreads();
    if (wave < nr) {  // xam = mean + x' w = mean + h . z
      const double* zr = z_s + wave * M;
      double s = 0.0;
      for (int j = lane; j < M; j += 64) s = fma(h_s[j], zr[j], s);
      s = wave_sum(s);
      if (lane == 0) xam_s[wave] = mean_s[wave] + s;
    }
    // x'_a[r][b] = sum_j (f_j z[r][j]) V[b][j], over the prior perturbations (z holds all that is needed of them)
    for (int e = tid; e < nr * M; e += nth) {
      const int r = e / M, b = e - r * M;
      const double* zr = z_s + r * M;
      double acc = 0.0;
      for (int j = 0; j < M; ++j) acc = fma(f_s[j] * zr[j], G[(size_t)j * M + b], acc);
      x_s[e] = acc;
    }
    __syncthreads();
    if (wave < nr) {
      const double* pa = x_s + wave * M;
      const double xam = xam_s[wave];
      if (MODE == kLetkfMembers) {
        long l = r0 + wave;
        if constexpr (SLAB) l = leads[l];
        E* out = static_cast<E*>(a.Xout) + (size_t)(l * a.npts + col) * M;
        if (rtps) {  // the posterior members' own mean and spread, as the standalone pass takes them (§7b)
          double s = 0.0;
          for (int m = lane; m < M; m += 64) s += pa[m];
          const double pm = wave_sum(s) / (double)M;
          double q = 0.0;
          for (int m = lane; m < M; m += 64) {
            const double dv = pa[m] - pm;
            q = fma(dv, dv, q);
          }
          q = wave_sum(q);
          if (q > 0.0) {  // (wave-uniform) sigma_a == 0: the row stays as it is
            const double sc = (1.0 - a.relax_alpha) + a.relax_alpha * sqrt(ssb_s[wave] / q);
            const double base = xam + pm;
            for (int m = lane; m < M; m += 64) out[m] = letkf_round<E>(base + sc * (pa[m] - pm));
          } else {
            for (int m = lane; m < M; m += 64) out[m] = letkf_round<E>(xam + pa[m]);
          }
        } else {
          for (int m = lane; m < M; m += 64) out[m] = letkf_round<E>(xam + pa[m]);
        }
      } else {
        for (int m = lane; m < M; m += 64) a.Yp_out[(size_t)col * M + m] = pa[m];
        if (lane == 0) a.ym_out[col] = xam;
      }
    }
    __syncthreads();  // the batch's rows are stored: the next batch takes x_s
  }
}

template <int MODE, typename E, int NTMAX>
hipError_t letkf_launch_as(const LetkfArgs& a, int nth, size_t lds, hipStream_t s) {
  auto kern = k_letkf<MODE, E, NTMAX>;
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const long nblk = (a.npts + 15) / 16;
  hipLaunchKernelGGL(kern, dim3((unsigned)(nblk * 16)), dim3((unsigned)nth), lds, s, a);
  return hipGetLastError();
}

template <int MODE, typename E>
hipError_t letkf_launch_mode(const LetkfArgs& a, hipStream_t s) {
  const int nth = letkf_threads(a.M);
  const size_t lds = letkf_lds_bytes(a.M);
  if (nth <= 256) return letkf_launch_as<MODE, E, 256>(a, nth, lds, s);
  if (nth <= 512) return letkf_launch_as<MODE, E, 512>(a, nth, lds, s);
  return letkf_launch_as<MODE, E, 1024>(a, nth, lds, s);
}

template <int MODE, typename E, int NTMAX>
hipError_t letkf_slab_launch_as(const LetkfSlabArgs& a, int nth, size_t lds, hipStream_t s) {
  auto kern = k_letkf<MODE, E, NTMAX, true>;
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const long nblk = (a.npts + 15) / 16;
  hipLaunchKernelGGL(kern, dim3((unsigned)(nblk * 16 * a.grp.ngroups)), dim3((unsigned)nth), lds, s, a);
  return hipGetLastError();
}

template <int MODE, typename E>
hipError_t letkf_slab_launch_mode(const LetkfSlabArgs& a, hipStream_t s) {
  const int nth = letkf_threads(a.M);
  const size_t lds = letkf_lds_bytes(a.M);
  if (nth <= 256) return letkf_slab_launch_as<MODE, E, 256>(a, nth, lds, s);
  if (nth <= 512) return letkf_slab_launch_as<MODE, E, 512>(a, nth, lds, s);
  return letkf_slab_launch_as<MODE, E, 1024>(a, nth, lds, s);
}

// The obs block under the obs-obs factors: the lists built at the ob positions take F(j, k) of §7t, the factors
// of k_obs_taper_vert / k_obs_taper_slab by the same device functions, F = (V T) C rounded in that order, then one product with the
// horizontal taper.  One workgroup per block of 16 ob positions.
__global__ __launch_bounds__(256) void k_letkf_obs_factor(long P, const long* __restrict__ off, const int* __restrict__ cnt,
                                                          const int* __restrict__ idx, double* __restrict__ wts,
                                                          const double* __restrict__ ob_vert, const double* __restrict__ ob_vhw,
                                                          const bool has_slab, const SlabObs o) {
  const long blk = (long)blockIdx.x;
  const long base = off[blk];
  const int n = cnt[blk];
  for (int i = (int)threadIdx.x; i < n * 16; i += (int)blockDim.x) {
    const int e = i >> 4, cb = i & 15;
    const long j = blk * 16 + cb;
    if (j >= P) continue;
    double* p = wts + (size_t)(base + e) * 16 + cb;
    const double w = *p;
    if (w == 0.0) continue;  // a zero stays zero, whatever the factors hold
    const long k = idx[base + e];
    double f = ob_vert ? vert_factor(ob_vert[j], ob_vert[k], ob_vhw[k]) : 1.0;
    if (has_slab) {
      f = f * time_factor(o.ob_time[j], o.ob_time[k], o.ob_thw[k]);
      f = f * impact_factor(o, k, o.ob_var[j]);
    }
    *p = w * f;
  }
}

}  // namespace

// The workgroup size, from M: the eigen-solve (where a column spends its time) plays ceil(M/2) column pairs per round on 16 lanes
// each, so 16 ceil(M/2) threads keep every lane of it busy and more would idle there; rounded up to whole waves, at least four (one
// per row of an apply batch) and at most 1024, and enough waves for the Gram's upper tiles at three per wave.  At 40 members that is
// 320 threads and 17 KB of LDS: nine workgroups fit a CU's LDS and four its registers, where 1024 threads would leave room for one.
int letkf_threads(int M) {
  const int npairs = (M + 1) / 2;
  int nth = 64 * ((16 * npairs + 63) / 64);
  if (nth < 64 * kLetkfRows) nth = 64 * kLetkfRows;
  if (nth > 1024) nth = 1024;
  const int T = letkf_tiles_side(M), ntiles = T * (T + 1) / 2;
  while (nth < 1024 && kLetkfTiles * (nth / 64) < ntiles) nth += 64;
  return nth;
}

size_t letkf_lds_bytes(int M) {
  // region | g, f, h, n, mu [M] each | x, z [4][M] each | per-row scalars | rot [2], n_local (ints)
  return ((size_t)letkf_region(M) + (size_t)(5 + 2 * kLetkfRows) * M + kLetkfSmall + 2) * sizeof(double);
}

hipError_t launch_letkf(const LetkfArgs& a, int mode, Elem elem, hipStream_t s) {
  if (a.M < 2 || a.M > kLetkfMaxM || a.npts < 0) return hipErrorInvalidValue;
  const int T = letkf_tiles_side(a.M);
  if (kLetkfTiles * (letkf_threads(a.M) / 64) < T * (T + 1) / 2 || letkf_lds_bytes(a.M) > 160 * 1024) return hipErrorInvalidValue;
  if (a.npts == 0) return hipSuccess;
  if ((a.npts + 15) / 16 * 16 > 0x7FFFFFF0L) return hipErrorInvalidValue;
  if (mode == kLetkfMembers) {
    if (!a.Xin || !a.Xout || a.n_lead < 1) return hipErrorInvalidValue;
    return elem == Elem::f32 ? letkf_launch_mode<kLetkfMembers, float>(a, s) : letkf_launch_mode<kLetkfMembers, double>(a, s);
  }
  if (elem != Elem::f64) return hipErrorInvalidValue;
  if (mode == kLetkfPerts) {
    if (!a.ym_in || !a.Yp_in || !a.ym_out || !a.Yp_out) return hipErrorInvalidValue;
    return letkf_launch_mode<kLetkfPerts, double>(a, s);
  }
  if (mode == kLetkfWeights) {
    if (!a.Tw) return hipErrorInvalidValue;
    return letkf_launch_mode<kLetkfWeights, double>(a, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_letkf_slab(const LetkfSlabArgs& a, int mode, Elem elem, hipStream_t s) {
  const LetkfGroups& g = a.grp;
  if (a.M < 2 || a.M > kLetkfMaxM || a.npts < 0) return hipErrorInvalidValue;
  const int T = letkf_tiles_side(a.M);
  if (kLetkfTiles * (letkf_threads(a.M) / 64) < T * (T + 1) / 2 || letkf_lds_bytes(a.M) > 160 * 1024) return hipErrorInvalidValue;
  if (g.ngroups < 1 || !g.rep || !g.grp_off || !g.grp_leads || g.s_pitch < 1) return hipErrorInvalidValue;
  if (a.idx && !g.S) return hipErrorInvalidValue;  // (no lists: the table is never read)
  if (a.npts == 0) return hipSuccess;
  if ((a.npts + 15) / 16 * 16 > 0x7FFFFFF0L / g.ngroups) return hipErrorInvalidValue;
  if (mode == kLetkfMembers) {
    if (!a.Xin || !a.Xout || a.n_lead < 1) return hipErrorInvalidValue;
    return elem == Elem::f32 ? letkf_slab_launch_mode<kLetkfMembers, float>(a, s) : letkf_slab_launch_mode<kLetkfMembers, double>(a, s);
  }
  if (elem != Elem::f64 || mode != kLetkfWeights || !a.Tw) return hipErrorInvalidValue;
  return letkf_slab_launch_mode<kLetkfWeights, double>(a, s);
}

hipError_t launch_letkf_obs_factor(long P, const long* off, const int* cnt, const int* idx, double* wts, const double* ob_vert,
                                   const double* ob_vhw, const SlabObs* slab, hipStream_t s) {
  if (P <= 0) return hipSuccess;
  if (!off || !cnt || !idx || !wts || (ob_vert && !ob_vhw)) return hipErrorInvalidValue;
  if (!ob_vert && !slab) return hipSuccess;
  const long nblk = (P + 15) / 16;
  if (nblk > 0x7FFFFFF0L) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_letkf_obs_factor, dim3((unsigned)nblk), dim3(256), 0, s, P, off, cnt, idx, wts, ob_vert, ob_vhw, slab != nullptr,
                     slab ? *slab : SlabObs{});
  return hipGetLastError();
}

hipError_t launch_letkf_prior(long P, int M, const double* Yp, const double* ym, const double* ob_value, const double* ob_error,
                              const double* ob_req, double t2, double* prior_mean, double* prior_var, uint8_t* assimilated, double* act,
                              double* dr, hipStream_t s) {
  if (M < 2 || M > kMaxMembers || P < 1) return hipErrorInvalidValue;
  const long b = (P + 3) / 4;
  hipLaunchKernelGGL(k_letkf_prior, dim3((unsigned)(b > 4096 ? 4096 : b)), dim3(256), 0, s, P, M, Yp, ym, ob_value, ob_error, ob_req, t2,
                     prior_mean, prior_var, assimilated, act, dr);
  return hipGetLastError();
}

}  // namespace efa

// ---- the driver (efa_letkf_driver) ----------------------------------------------------------------------------------------------
namespace efa_host {

using namespace efa;

namespace {

// the per-ob arrays of a call on the device, slices of c->letkf_ob
struct LetkfObs {
  long P = 0;
  double *value = nullptr, *error = nullptr, *lat = nullptr, *lon = nullptr, *hw = nullptr, *req = nullptr;
  double *act = nullptr, *dr = nullptr, *obtrig = nullptr;
  double *prior_mean = nullptr, *prior_var = nullptr, *post_mean = nullptr, *post_var = nullptr;
  uint8_t* assimilated = nullptr;
  size_t diag_bytes() const { return 4 * (size_t)P * sizeof(double) + (size_t)P; }
};

// the lists of one set of points, slices of c->letkf_blk and the two entry buffers
struct LetkfLists {
  const long* off = nullptr;
  const int *cnt = nullptr, *order = nullptr, *idx = nullptr;
  const double* wts = nullptr;
};

// What no LETKF call serves, refused before anything is launched (include/efa_hip.h gives the reasons)
// slab: the calls of DESIGN.md §7y-3, which need the vertical and/or the slab setting, sized for this call (n_lead < 0: not checked)
int letkf_check_settings(const efa_ctx* c, const char* who, int M, long P, bool slab = false, long n_lead = -1) {
  if (M < 2) return fail(EFA_ERR_INVALID, "%s: ensemble size M=%d must be >= 2", who, M);
  if (M > kLetkfMaxM)
    return fail(EFA_ERR_INVALID, "%s: M=%d exceeds %d members, the range in which the eigen-solve's M x M array of a column fits in LDS",
                who, M, kLetkfMaxM);
  if (P < 0) return fail(EFA_ERR_INVALID, "%s: negative observation count", who);
  if (c->ai_field)
    return fail(EFA_ERR_INVALID, "%s: an adaptive-inflation field is set (its update follows the serial order of the obs, which a "
                "column's batch solve does not have)", who);
  if (!slab && c->vl_on)
    return fail(EFA_ERR_INVALID, "%s: vertical localisation is set (it needs a solve per (slab group, column): out of scope here, "
                "use efa_letkf_slab_cycle_dev / SlabLETKF)", who);
  if (!slab && c->sl_on)
    return fail(EFA_ERR_INVALID, "%s: slab (temporal / cross-variable) localisation is set (it needs a solve per (slab group, column): "
                "out of scope here, use efa_letkf_slab_cycle_dev / SlabLETKF)", who);
  if (slab) {
    if (!c->vl_on && !c->sl_on)
      return fail(EFA_ERR_INVALID, "%s: neither vertical nor slab (temporal / cross-variable) localisation is set: use the plain call "
                  "(efa_letkf_cycle_dev and its kin)", who);
    if (c->vl_on && (c->vl_P != P || (n_lead >= 0 && c->vl_nlead != n_lead)))
      return fail(EFA_ERR_INVALID, "%s: vertical localisation was set for %ld observations and %ld slabs, the call has %ld and n_lead=%ld",
                  who, c->vl_P, c->vl_nlead, P, n_lead);
    if (c->sl_on && (c->sl_P != P || (n_lead >= 0 && c->sl_nlead != n_lead)))
      return fail(EFA_ERR_INVALID, "%s: slab localisation was set for %ld observations and %ld slabs, the call has %ld and n_lead=%ld", who,
                  c->sl_P, c->sl_nlead, P, n_lead);
  }
  if (sec_active(c))
    return fail(EFA_ERR_INVALID, "%s: a sampling-error-correction table is set (it acts on the serial gain of one observation at a time)",
                who);
  return EFA_OK;
}

int letkf_check_obs(const char* who, long P, const double* ym_dev, const double* Yp_dev, const double* ob_value, const double* ob_error,
                    const uint8_t* ob_assim, const double* ob_lat, const double* ob_lon, const double* ob_hw) {
  if (P == 0) return EFA_OK;
  if (!ym_dev || !Yp_dev || !ob_value || !ob_error || !ob_assim) return fail(EFA_ERR_INVALID, "%s: null observation array", who);
  if (!ob_lat || !ob_lon || !ob_hw) return fail(EFA_ERR_INVALID, "%s: the taper needs ob_lat/ob_lon/ob_halfwidth_km", who);
  for (long k = 0; k < P; ++k) {
    if (!ob_assim[k]) continue;
    if (!(std::isfinite(ob_error[k]) && ob_error[k] > 0.0))
      return fail(EFA_ERR_INVALID, "%s: observation %ld: error variance %g must be finite and > 0 (R-localisation divides by it)", who, k,
                  ob_error[k]);
    if (!(ob_hw[k] == ob_hw[k]) || ob_hw[k] == 0.0)
      return fail(EFA_ERR_INVALID, "%s: observation %ld: localize_radius must be a non-zero number", who, k);
  }
  return EFA_OK;
}

// the obs on the device, then their prior diagnostics, effective flags and {d, r}
int letkf_stage_obs(efa_ctx* c, int M, long P, const double* ym_dev, const double* Yp_dev, const double* ob_value, const double* ob_error,
                    const uint8_t* ob_assim, const double* ob_lat, const double* ob_lon, const double* ob_hw, LetkfObs* out) {
  hipStream_t s = c->stream;
  const size_t n = (size_t)P;
  // value | error | lat | lon | hw | requested [n each] | act [4n] | dr [2n] | obtrig [6n] | four diagnostics [n each] | assimilated bytes
  EFA_TRY(c->letkf_ob.reserve((22 * n + 1) * sizeof(double) + n));
  double* d = c->letkf_ob.as<double>();
  LetkfObs o;
  o.P = P;
  o.value = d;
  o.error = d + n;
  o.lat = d + 2 * n;
  o.lon = d + 3 * n;
  o.hw = d + 4 * n;
  o.req = d + 5 * n;
  o.act = d + 6 * n;
  o.dr = d + 10 * n;
  o.obtrig = d + 12 * n;
  o.prior_mean = d + 18 * n;
  o.prior_var = d + 19 * n;
  o.post_mean = d + 20 * n;
  o.post_var = d + 21 * n;
  o.assimilated = reinterpret_cast<uint8_t*>(d + 22 * n);
  // value and error of an ob that is not requested are not read: the device gets the neutral pair (0, 1), its radius a harmless 1
  std::vector<double> h(6 * n);
  for (size_t k = 0; k < n; ++k) {
    const bool on = ob_assim[k] != 0;
    h[k] = on ? ob_value[k] : 0.0;
    h[n + k] = on ? ob_error[k] : 1.0;
    h[2 * n + k] = ob_lat[k];
    h[3 * n + k] = ob_lon[k];
    h[4 * n + k] = on ? ob_hw[k] : 1.0;
    h[5 * n + k] = on ? 1.0 : 0.0;
  }
  EFA_HIP(hipMemcpyAsync(d, h.data(), 6 * n * sizeof(double), hipMemcpyHostToDevice, s));
  EFA_HIP(hipStreamSynchronize(s));  // (h goes out of scope)
  EFA_HIP(launch_letkf_prior(P, M, Yp_dev, ym_dev, o.value, o.error, o.req, c->qc_threshold * c->qc_threshold, o.prior_mean, o.prior_var,
                             o.assimilated, o.act, o.dr, s));
  *out = o;
  return EFA_OK;
}

// The lists of `npts` points (device lat / lon) against the obs, by the one-pass sweep's builders as they are; the flag entry of the
// coefficient table they read is the effective a_k.  One host round trip: the capacity.
int letkf_build_lists(efa_ctx* c, long npts, const double* plat, const double* plon, const LetkfObs& o, LetkfLists* out) {
  hipStream_t s = c->stream;
  const long nblk = gc_num_blocks(npts);
  const size_t b8 = ((size_t)(nblk + 1) * sizeof(long) + 15) & ~(size_t)15, b4 = ((size_t)nblk * sizeof(int) + 15) & ~(size_t)15;
  EFA_TRY(c->letkf_blk.reserve(b8 + 3 * b4));
  EFA_TRY(c->letkf_pairs.reserve(sizeof(unsigned long long)));
  char* b = static_cast<char*>(c->letkf_blk.p);
  long* off = reinterpret_cast<long*>(b);
  int* cnt = reinterpret_cast<int*>(b + b8);
  int* ub = reinterpret_cast<int*>(b + b8 + b4);
  int* order = reinterpret_cast<int*>(b + b8 + 2 * b4);
  EFA_HIP(hipMemsetAsync(c->letkf_pairs.p, 0, sizeof(unsigned long long), s));
  EFA_HIP(launch_gc_bound(npts, o.P, plat, o.lat, o.hw, o.act, ub, off, s));
  long cap = 0;
  EFA_HIP(hipMemcpyAsync(&cap, off + nblk, sizeof(long), hipMemcpyDeviceToHost, s));
  EFA_HIP(hipStreamSynchronize(s));
  EFA_TRY(c->letkf_idx.reserve((size_t)(cap ? cap : 1) * sizeof(int)));
  EFA_TRY(c->letkf_wts.reserve((size_t)(cap ? cap : 1) * 16 * sizeof(double)));
  EFA_HIP(launch_gc_fill(npts, o.P, plat, plon, o.lat, o.lon, o.hw, o.act, o.obtrig, off, cnt, c->letkf_idx.as<int>(),
                         c->letkf_wts.as<double>(), order, c->letkf_pairs.as<unsigned long long>(), s));
  out->off = off;
  out->cnt = cnt;
  out->order = order;
  out->idx = c->letkf_idx.as<int>();
  out->wts = c->letkf_wts.as<double>();
  return EFA_OK;
}

int letkf_upload_points(efa_ctx* c, long npts, const double* lat, const double* lon, const double** dlat, const double** dlon) {
  const size_t nb = (size_t)npts * sizeof(double);
  EFA_TRY(c->letkf_pts.reserve(2 * nb));
  double* d = c->letkf_pts.as<double>();
  EFA_HIP(hipMemcpyAsync(d, lat, nb, hipMemcpyHostToDevice, c->stream));
  EFA_HIP(hipMemcpyAsync(d + npts, lon, nb, hipMemcpyHostToDevice, c->stream));
  EFA_HIP(hipStreamSynchronize(c->stream));  // the caller may reuse its arrays on return
  *dlat = d;
  *dlon = d + npts;
  return EFA_OK;
}

LetkfArgs letkf_args(int M, long npts, const LetkfLists& l, const double* Yp, const LetkfObs& o) {
  LetkfArgs a{};
  a.npts = npts;
  a.n_lead = 1;
  a.M = M;
  a.off = l.off;
  a.cnt = l.cnt;
  a.order = l.order;
  a.idx = l.idx;
  a.wts = l.wts;
  a.Yp = Yp;
  a.dr = o.dr;
  a.relax_kind = EFA_RELAX_NONE;
  return a;
}

// the solve at `npts` points whose lists are built: [T | w] of each to Tw, the statistics to stats (or null); does not wait
int letkf_solve_points(efa_ctx* c, int M, long npts, const LetkfLists& lists, const double* Yp_dev, const LetkfObs& o, double* Tw,
                       double* stats) {
  LetkfArgs a = letkf_args(M, npts, lists, Yp_dev, o);
  a.Tw = Tw;
  a.stats = stats;
  EFA_HIP(launch_letkf(a, kLetkfWeights, Elem::f64, c->stream));
  return EFA_OK;
}

// the mesh of a weight-interpolation call; *out has the strides cut to the axis (a stride beyond it gives the same nodes: the two ends)
int letkf_check_mesh(const char* who, const LetkfMesh& m, LetkfMesh* out) {
  if (m.ny < 1 || m.nx < 1) return fail(EFA_ERR_INVALID, "%s: the grid's shape (%ld, %ld) must be positive", who, m.ny, m.nx);
  if (m.ny > 0x7FFFFFF0L / m.nx) return fail(EFA_ERR_INVALID, "%s: %ld x %ld columns exceed the launch grid", who, m.ny, m.nx);
  if (m.sy < 1 || m.sx < 1) return fail(EFA_ERR_INVALID, "%s: the weight stride (%ld, %ld) must be >= 1 on both axes", who, m.sy, m.sx);
  *out = m;
  const long cy = m.ny > 2 ? m.ny - 1 : 1, cx = m.nx > 2 ? m.nx - 1 : 1;
  if (out->sy > cy) out->sy = cy;
  if (out->sx > cx) out->sx = cx;
  return EFA_OK;
}

// the member rows of a state call: pointers, alignment, overlap, and rows == n_lead * ncol
int letkf_check_rows(const char* who, const StateRows& r, long ncol, long n_lead) {
  if (r.rows < 0) return fail(EFA_ERR_INVALID, "%s: negative row count", who);
  if (r.rows == 0) return EFA_OK;
  if (!r.prior || !r.post) return fail(EFA_ERR_INVALID, "%s: null state pointer", who);
  if (r.elem == Elem::f32 && ((reinterpret_cast<uintptr_t>(r.prior) | reinterpret_cast<uintptr_t>(r.post)) & 3u) != 0)
    return fail(EFA_ERR_INVALID, "%s: state pointers must be 4-byte aligned", who);
  if (r.partial_overlap())
    return fail(EFA_ERR_INVALID, "%s: the posterior rows overlap the prior rows without coinciding with them (in place means the same "
                "address: a column's rows are read and written by its own workgroup only)", who);
  if (n_lead < 1 || ncol < 1 || r.rows != n_lead * ncol)
    return fail(EFA_ERR_INVALID, "%s: rows=%ld is not n_lead=%ld times the grid's %ld columns", who, r.rows, n_lead, ncol);
  return EFA_OK;
}

// the interpolate-and-apply launch of the cycle and of efa_letkf_interp_apply_dev, under the context's relaxation; does not wait
int letkf_interp_launch(efa_ctx* c, const char* who, Elem elem, int M, const void* X_dev, void* post_dev, const LetkfMesh& nodes,
                        long n_lead, const double* Tw, const double* stats, const LetkfGroups* grp = nullptr) {
  LetkfInterpSlabArgs a{};
  a.mesh = nodes;
  a.n_lead = n_lead;
  a.M = M;
  a.Xin = X_dev;
  a.Xout = post_dev;
  a.Tw = Tw;
  a.stats = stats;
  a.relax_kind = c->relax_kind;
  a.relax_alpha = c->relax_alpha;
  if (grp) {
    a.ngroups = grp->ngroups;
    a.grp_off = grp->grp_off;
    a.grp_leads = grp->grp_leads;
    EFA_HIP(launch_letkf_interp_slab(a, elem, c->stream));
    return EFA_OK;
  }
  EFA_HIP(launch_letkf_interp(static_cast<const LetkfInterpArgs&>(a), elem, c->stream));
  return EFA_OK;
}

// ---- the slab groups --------------------------------------------------------------------------------------------
// Slabs whose factors agree for every ob share one solve.  Decided here from the host copies of the two settings, without the
// table: the key of slab s is the bit pattern of lead_vert[s], lead_time[s] and lead_var[s], each only while that part can give a
// factor other than 1 (some ob carries vertical information; some ob has a time and a temporal half-width; some ob's impact row
// has an entry other than 1).  Equal keys imply equal columns of S.  Groups are numbered by first appearance; cached on the
// settings' serials, the device copy uploaded once per change.
uint64_t letkf_key_bits(double v) {
  if (v != v) return ~(uint64_t)0;  // every NaN is "no coordinate"
  uint64_t b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}

int letkf_groups(efa_ctx* c, long n_lead) {
  if (c->lg_vl_serial == c->vl_serial && c->lg_sl_serial == c->sl_serial && (long)c->lg_group_of.size() == n_lead &&
      c->lg_ptr == c->lg_dev.p && c->lg_dev.p)
    return EFA_OK;
  const bool vert = vl_active(c);
  bool temporal = false, variable = false;
  const double* lt = nullptr;
  const int* lvar = nullptr;
  if (c->sl_on) {
    const long P = c->sl_P, nv = c->sl_nvar, ng = c->sl_ngroup;
    const double* d = c->sl_host.data();
    const int* iv = reinterpret_cast<const int*>(d + c->sl_nlead + 2 * P + ng * nv);
    lt = d;
    lvar = iv;
    for (long k = 0; k < P && !temporal; ++k) temporal = d[c->sl_nlead + k] == d[c->sl_nlead + k] && d[c->sl_nlead + P + k] == d[c->sl_nlead + P + k];
    for (long k = 0; k < P && !variable; ++k) {
      const int g = iv[c->sl_nlead + k];
      if (g < 0) continue;
      for (long u = 0; u < nv && !variable; ++u) variable = d[c->sl_nlead + 2 * P + g * nv + u] != 1.0;
    }
  }
  std::map<std::tuple<uint64_t, uint64_t, int>, int> seen;
  std::vector<int> group_of((size_t)n_lead), rep;
  for (long sidx = 0; sidx < n_lead; ++sidx) {
    const auto key = std::make_tuple(vert ? letkf_key_bits(c->vl_host[sidx]) : (uint64_t)0, temporal ? letkf_key_bits(lt[sidx]) : (uint64_t)0,
                                     variable ? lvar[sidx] : 0);
    auto it = seen.find(key);
    if (it == seen.end()) {
      it = seen.emplace(key, (int)rep.size()).first;
      rep.push_back((int)sidx);
    }
    group_of[sidx] = it->second;
  }
  const int ng = (int)rep.size();
  std::vector<int> h((size_t)(2 * ng + 1 + n_lead));  // rep | grp_off | grp_leads
  std::vector<int> count((size_t)ng, 0);
  for (long sidx = 0; sidx < n_lead; ++sidx) count[group_of[sidx]]++;
  for (int g = 0; g < ng; ++g) {
    h[g] = rep[g];
    h[ng + g + 1] = h[ng + g] + count[g];
  }
  std::vector<int> fill((size_t)ng, 0);
  for (long sidx = 0; sidx < n_lead; ++sidx) {
    const int g = group_of[sidx];
    h[2 * ng + 1 + h[ng + g] + fill[g]++] = (int)sidx;
  }
  EFA_TRY(c->lg_dev.reserve(h.size() * sizeof(int)));
  EFA_HIP(hipMemcpyAsync(c->lg_dev.p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  EFA_HIP(hipStreamSynchronize(c->stream));  // (h goes out of scope)
  c->lg_group_of.swap(group_of);
  c->lg_ngroups = ng;
  c->lg_vl_serial = c->vl_serial;
  c->lg_sl_serial = c->sl_serial;
  c->lg_ptr = c->lg_dev.p;
  return EFA_OK;
}

// the table and the groups of a slab call, as the kernels take them (the settings were checked for this P and n_lead)
int letkf_slab_groups(efa_ctx* c, long n_lead, LetkfGroups* out) {
  EFA_TRY(ensure_slab_table(c));
  EFA_TRY(letkf_groups(c, n_lead));
  const int* d = c->lg_dev.as<int>();
  const int ng = c->lg_ngroups;
  *out = LetkfGroups{ng, n_lead, c->sl_tab.as<double>(), d, d + ng, d + 2 * ng + 1};
  return EFA_OK;
}

// the node solve of the slab calls: [T | w] of every (group, point) to Tw, the statistics [group][point][3]; does not wait
int letkf_solve_points_slab(efa_ctx* c, int M, long npts, const LetkfLists& lists, const double* Yp_dev, const LetkfObs& o,
                            const LetkfGroups& grp, double* Tw, double* stats) {
  LetkfSlabArgs a{};
  static_cast<LetkfArgs&>(a) = letkf_args(M, npts, lists, Yp_dev, o);
  a.grp = grp;
  a.Tw = Tw;
  a.stats = stats;
  EFA_HIP(launch_letkf_slab(a, kLetkfWeights, Elem::f64, c->stream));
  return EFA_OK;
}

}  // namespace

int letkf_cycle(efa_ctx* c, Elem elem, long rows, int M, long P, const void* X_dev, void* post_dev, double* ym_dev, double* Yp_dev,
                int obs_block_out, const double* ob_value, const double* ob_error, const uint8_t* ob_assim, const double* ob_lat,
                const double* ob_lon, const double* ob_hw, const double* grid_lat, const double* grid_lon, long ncol, long n_lead,
                double* prior_mean, double* prior_var, double* post_mean, double* post_var, uint8_t* assimilated, double* col_stats_dev,
                const LetkfMesh* mesh, bool slab) {
  const bool f32 = elem == Elem::f32;
  const char* who = slab ? (mesh ? (f32 ? "efa_letkf_slab_cycle_interp_f32_dev" : "efa_letkf_slab_cycle_interp_dev")
                                 : (f32 ? "efa_letkf_slab_cycle_f32_dev" : "efa_letkf_slab_cycle_dev"))
                         : (mesh ? (f32 ? "efa_letkf_cycle_interp_f32_dev" : "efa_letkf_cycle_interp_dev")
                                 : (f32 ? "efa_letkf_cycle_f32_dev" : "efa_letkf_cycle_dev"));
  EFA_TRY(letkf_check_settings(c, who, M, P, slab, n_lead));
  LetkfMesh nodes{};
  if (mesh) {
    EFA_TRY(letkf_check_mesh(who, *mesh, &nodes));
    ncol = nodes.ncol();
    if (mesh->unit()) mesh = nullptr;  // every column is a node: the plain call, bit for bit (col_stats_dev: the nodes are the columns)
  }
  if (rows < 0) return fail(EFA_ERR_INVALID, "%s: negative row count", who);
  const StateRows r{X_dev, post_dev, elem, rows, M};
  if (rows > 0) {
    if (!X_dev || !post_dev) return fail(EFA_ERR_INVALID, "%s: null state pointer", who);
    if (f32 && ((reinterpret_cast<uintptr_t>(X_dev) | reinterpret_cast<uintptr_t>(post_dev)) & 3u) != 0)
      return fail(EFA_ERR_INVALID, "%s: state pointers must be 4-byte aligned", who);
    if (r.partial_overlap())
      return fail(EFA_ERR_INVALID, "%s: the posterior rows overlap the prior rows without coinciding with them (in place means the same "
                  "address: a column's rows are read and written by its own workgroup only)", who);
    EFA_TRY(check_grid(EFA_LOC_GC, grid_lat, grid_lon, ncol, n_lead, rows));
  }
  EFA_TRY(letkf_check_obs(who, P, ym_dev, Yp_dev, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_hw));
  hipStream_t s = c->stream;
  harvest_obs_ms(c);
  harvest_state_ms(c);
  c->obs_ms = c->state_ms = 0.0;
  c->state_launches = 0;
  c->phase_a_kind = slab ? (mesh ? 9 : 8) : (mesh ? 7 : 6);
  c->path_taken = EFA_PATH_TRANSFORM;
  if (c->timing) EFA_HIP(hipEventRecord(c->obs_iv.begin, s));

  // ---- the obs: flags and prior diagnostics, then the obs block as P more one-row columns, each solved at its own position ------
  LetkfObs o;
  LetkfLists lists;
  double *Yw = nullptr, *ymw = nullptr;
  if (P > 0) {
    EFA_TRY(letkf_stage_obs(c, M, P, ym_dev, Yp_dev, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_hw, &o));
    EFA_TRY(c->letkf_Yw.reserve(((size_t)P * M + (size_t)P) * sizeof(double)));
    Yw = c->letkf_Yw.as<double>();
    ymw = Yw + (size_t)P * M;
    EFA_TRY(letkf_build_lists(c, P, o.lat, o.lon, o, &lists));
    if (slab) {  // the obs-obs factors F(j, k) into the lists' tapers; the perturbation-form launch then runs as it is, one group
      const bool vert = vl_active(c);
      const SlabObs so = sl_active(c) ? sl_obs(c, 0) : SlabObs{};
      EFA_HIP(launch_letkf_obs_factor(P, lists.off, lists.cnt, lists.idx, c->letkf_wts.as<double>(), vert ? vl_obvert(c) : nullptr,
                                      vert ? vl_obvhw(c) : nullptr, sl_active(c) ? &so : nullptr, s));
    }
    LetkfArgs a = letkf_args(M, P, lists, Yp_dev, o);
    a.ym_in = ym_dev;
    a.Yp_in = Yp_dev;
    a.ym_out = ymw;
    a.Yp_out = Yw;
    EFA_HIP(launch_letkf(a, kLetkfPerts, Elem::f64, s));
    EFA_HIP(launch_etkf_post(P, M, Yw, ymw, o.post_mean, o.post_var, s));
  }
  // ---- the state: the grid's lists (the obs' are consumed: the stream is in order), then ONE launch -----------------------------
  //      (with a mesh: the nodes' lists, then the node solve and the interpolate-and-apply launch)
  LetkfLists glists;
  const long nnodes = mesh ? nodes.nnodes() : 0;
  double* node_stats = col_stats_dev;
  LetkfGroups grp{};
  if (rows > 0 && slab) EFA_TRY(letkf_slab_groups(c, n_lead, &grp));
  const size_t ngr = slab ? (size_t)grp.ngroups : 1;  // solves per column or node
  if (rows > 0 && mesh) {
    if (c->letkf_Tw.reserve(ngr * (size_t)nnodes * M * (M + 1) * sizeof(double)) != EFA_OK)
      return fail(EFA_ERR_ALLOC, "%s: the node-pair buffer of %zu groups x %ld nodes x %d x %d doubles could not be allocated", who, ngr,
                  nnodes, M, M + 1);
    if (!node_stats) {  // the apply reads n_local of every node
      EFA_TRY(c->letkf_nst.reserve(3 * ngr * (size_t)nnodes * sizeof(double)));
      node_stats = c->letkf_nst.as<double>();
    }
  }
  if (rows > 0 && P > 0) {
    if (mesh) {  // a node is a grid column: its position is that column's
      std::vector<double> h(2 * (size_t)nnodes);
      const long nyn = nodes.nyn(), nxn = nodes.nxn();
      for (long jy = 0; jy < nyn; ++jy)
        for (long jx = 0; jx < nxn; ++jx) {
          const long col = LetkfMesh::axis_node(jy, nodes.ny, nodes.sy) * nodes.nx + LetkfMesh::axis_node(jx, nodes.nx, nodes.sx);
          h[jy * nxn + jx] = grid_lat[col];
          h[nnodes + jy * nxn + jx] = grid_lon[col];
        }
      const double *dlat = nullptr, *dlon = nullptr;
      EFA_TRY(letkf_upload_points(c, nnodes, h.data(), h.data() + nnodes, &dlat, &dlon));
      EFA_TRY(letkf_build_lists(c, nnodes, dlat, dlon, o, &glists));
    } else {
      EFA_TRY(c->grid.upload(s, grid_lat, grid_lon, ncol));
      EFA_TRY(letkf_build_lists(c, ncol, c->grid.lat.as<double>(), c->grid.lon.as<double>(), o, &glists));
    }
  }
  if (c->timing) {
    EFA_HIP(hipEventRecord(c->obs_iv.end, s));
    c->obs_ends_at = c->obs_iv.end;
    c->obs_iv.pending = true;
    EFA_HIP(hipEventRecord(c->state_iv[0].begin, s));
  }
  if (rows > 0 && mesh && slab) {
    EFA_TRY(letkf_solve_points_slab(c, M, nnodes, glists, Yp_dev, o, grp, c->letkf_Tw.as<double>(), node_stats));
    EFA_TRY(letkf_interp_launch(c, who, elem, M, X_dev, post_dev, nodes, n_lead, c->letkf_Tw.as<double>(), node_stats, &grp));
    c->state_launches = 2;
  } else if (rows > 0 && slab) {
    LetkfSlabArgs a{};
    static_cast<LetkfArgs&>(a) = letkf_args(M, ncol, glists, Yp_dev, o);
    a.grp = grp;
    a.n_lead = n_lead;
    a.Xin = X_dev;
    a.Xout = post_dev;
    a.stats = col_stats_dev;
    a.relax_kind = c->relax_kind;
    a.relax_alpha = c->relax_alpha;
    EFA_HIP(launch_letkf_slab(a, kLetkfMembers, elem, s));
    c->state_launches = 1;
  } else if (rows > 0 && mesh) {  // (P == 0: no lists, every node has the pair (I, 0) and no column changes)
    EFA_TRY(letkf_solve_points(c, M, nnodes, glists, Yp_dev, o, c->letkf_Tw.as<double>(), node_stats));
    EFA_TRY(letkf_interp_launch(c, who, elem, M, X_dev, post_dev, nodes, n_lead, c->letkf_Tw.as<double>(), node_stats));
    c->state_launches = 2;
  } else if (rows > 0) {
    LetkfArgs a = letkf_args(M, ncol, glists, Yp_dev, o);  // (P == 0: no lists, every column keeps its rows)
    a.n_lead = n_lead;
    a.Xin = X_dev;
    a.Xout = post_dev;
    a.stats = col_stats_dev;
    a.relax_kind = c->relax_kind;
    a.relax_alpha = c->relax_alpha;
    EFA_HIP(launch_letkf(a, kLetkfMembers, elem, s));
    c->state_launches = 1;
  }
  if (c->timing) {
    EFA_HIP(hipEventRecord(c->state_iv[0].end, s));
    c->state_iv[0].pending = true;
  }
  c->state_launches_sum += c->state_launches;
  // ---- the posterior obs block to the caller, behind every solve that read the prior one; the diagnostics ----------------------
  std::vector<char> hd;
  if (P > 0) {
    if (obs_block_out) {
      EFA_HIP(hipMemcpyAsync(Yp_dev, Yw, (size_t)P * M * sizeof(double), hipMemcpyDeviceToDevice, s));
      EFA_HIP(hipMemcpyAsync(ym_dev, ymw, (size_t)P * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    hd.resize(o.diag_bytes());
    EFA_HIP(hipMemcpyAsync(hd.data(), o.prior_mean, hd.size(), hipMemcpyDeviceToHost, s));
  }
  EFA_HIP(hipStreamSynchronize(s));
  if (P > 0) {
    const size_t dP = (size_t)P * sizeof(double);
    const double* pm = reinterpret_cast<const double*>(hd.data() + 2 * dP);
    const double* pv = reinterpret_cast<const double*>(hd.data() + 3 * dP);
    const uint8_t* as = reinterpret_cast<const uint8_t*>(hd.data() + 4 * dP);
    if (prior_mean) std::memcpy(prior_mean, hd.data(), dP);
    if (prior_var) std::memcpy(prior_var, hd.data() + dP, dP);
    for (long k = 0; k < P; ++k) {
      if (assimilated) assimilated[k] = as[k];
      if (as[k]) {
        if (post_mean) post_mean[k] = pm[k];
        if (post_var) post_var[k] = pv[k];
      }
    }
  }
  if (c->timing == 1) {
    harvest_obs_ms(c);
    harvest_state_ms(c);
  }
  return EFA_OK;
}

int letkf_weights(efa_ctx* c, int M, long P, const double* ym_dev, const double* Yp_dev, const double* ob_value, const double* ob_error,
                  const uint8_t* ob_assim, const double* ob_lat, const double* ob_lon, const double* ob_hw, long npts,
                  const double* pt_lat, const double* pt_lon, double* Tw_dev, double* stats_dev, bool slab) {
  const char* who = slab ? "efa_letkf_slab_weights_dev" : "efa_letkf_weights_dev";
  const long n_lead = c->sl_on ? c->sl_nlead : c->vl_nlead;  // (slab: the slabs are the settings' own)
  EFA_TRY(letkf_check_settings(c, who, M, P, slab, slab ? n_lead : -1));
  if (npts < 0) return fail(EFA_ERR_INVALID, "%s: negative point count", who);
  if (npts > 0 && (!pt_lat || !pt_lon || !Tw_dev)) return fail(EFA_ERR_INVALID, "%s: null point or output array", who);
  EFA_TRY(letkf_check_obs(who, P, ym_dev, Yp_dev, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_hw));
  if (npts == 0) return EFA_OK;
  hipStream_t s = c->stream;
  LetkfObs o;
  LetkfLists lists;
  if (P > 0) {
    const double *dlat = nullptr, *dlon = nullptr;
    EFA_TRY(letkf_stage_obs(c, M, P, ym_dev, Yp_dev, ob_value, ob_error, ob_assim, ob_lat, ob_lon, ob_hw, &o));
    EFA_TRY(letkf_upload_points(c, npts, pt_lat, pt_lon, &dlat, &dlon));
    EFA_TRY(letkf_build_lists(c, npts, dlat, dlon, o, &lists));
  }
  if (slab) {
    LetkfGroups grp{};
    EFA_TRY(letkf_slab_groups(c, n_lead, &grp));
    EFA_TRY(letkf_solve_points_slab(c, M, npts, lists, Yp_dev, o, grp, Tw_dev, stats_dev));
  } else {
    EFA_TRY(letkf_solve_points(c, M, npts, lists, Yp_dev, o, Tw_dev, stats_dev));
  }
  EFA_HIP(hipStreamSynchronize(s));
  return EFA_OK;
}

int letkf_slab_group_table(efa_ctx* c, long n_lead, int* group_of, int* ngroups) {
  const char* who = "efa_letkf_slab_groups";
  if (!c->vl_on && !c->sl_on) return fail(EFA_ERR_INVALID, "%s: neither vertical nor slab localisation is set", who);
  if ((c->vl_on && c->vl_nlead != n_lead) || (c->sl_on && c->sl_nlead != n_lead))
    return fail(EFA_ERR_INVALID, "%s: the settings are not sized for n_lead=%ld", who, n_lead);
  if (c->vl_on && c->sl_on && c->vl_P != c->sl_P)
    return fail(EFA_ERR_INVALID, "%s: the vertical and the slab setting are sized for %ld and %ld observations", who, c->vl_P, c->sl_P);
  EFA_TRY(letkf_groups(c, n_lead));
  if (group_of) std::memcpy(group_of, c->lg_group_of.data(), (size_t)n_lead * sizeof(int));
  if (ngroups) *ngroups = c->lg_ngroups;
  return EFA_OK;
}

int letkf_interp_apply(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, void* post_dev, long ny, long nx, long stride_y,
                       long stride_x, long n_lead, const double* Tw_nodes_dev, const double* node_stats_dev) {
  const bool f32 = elem == Elem::f32;
  const char* who = f32 ? "efa_letkf_interp_apply_f32_dev" : "efa_letkf_interp_apply_dev";
  EFA_TRY(letkf_check_settings(c, who, M, 0));
  LetkfMesh nodes{};
  EFA_TRY(letkf_check_mesh(who, LetkfMesh{ny, nx, stride_y, stride_x}, &nodes));
  EFA_TRY(letkf_check_rows(who, StateRows{X_dev, post_dev, elem, rows, M}, nodes.ncol(), n_lead));
  if (rows == 0) return EFA_OK;
  if (!Tw_nodes_dev) return fail(EFA_ERR_INVALID, "%s: null node pairs", who);
  EFA_TRY(letkf_interp_launch(c, who, elem, M, X_dev, post_dev, nodes, n_lead, Tw_nodes_dev, node_stats_dev));
  EFA_HIP(hipStreamSynchronize(c->stream));
  return EFA_OK;
}

}  // namespace efa_host
