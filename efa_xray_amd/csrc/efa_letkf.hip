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
// Weight interpolation: the driver (efa_letkf_driver.hip) also runs kLetkfWeights at the nodes of a coarse mesh of
// grid columns and hands the node pairs to k_letkf_interp (efa_letkf_interp.hip), which interpolates them to every column and
// applies them.
// Vertical, temporal and variable localisation (efa_letkf_slab_cycle_dev and its kin): k_letkf with the SLAB switch
// solves once per (slab group, column) under rho_k(c) * S[k][rep[g]], S the slab factor table of §7t; k_letkf_obs_factor scales the
// tapers of the lists built at the ob positions by the obs-obs factor F(j, k), after which the obs block runs as above.  The driver
// computes the groups from the host copies of the two settings (letkf_groups).
// Per-point multiplicative inflation (efa_ctx_set_letkf_inflation): with a.infl the point's prior factor lambda_b
// enters the solve as Hunt's rho, A_x = (M-1)/lambda_b I + C_x, and with infl_sigma2 > 0 one lane writes back Miyoshi's (2011)
// estimate lambda_a from p1 = sum_k w_k d_k^2 (entry (M, M) of the Gram product), p2 = trace(C_x)/(M-1) (its diagonal before the
// shift) and p3 = sum_k rho_k (the n_local loop).  A uniform run-time branch: a.infl == nullptr is the kernel without it.
// The deterministic control analysis (efa_ctx_set_letkf_control): with a.dc the staged row is [Yp_k | d_k | d^c_k],
// d^c_k = value_k - H(x_c)_k from k_letkf_control_prior, column M+1 of the (M+2)^2 product is g^c, h^c = (V^T g^c)/mu goes over n_s
// behind the sweeps, and the wave that owns a row adds h^c . z to the control's value of that row (the obs block: to y_c[j]).  A
// template switch (CTRL): without a.dc the kernels are the ones without it.
// The cap on the local obs of a solve (efa_ctx_set_letkf_obs_cap): k_letkf_cap runs between the list build and
// the solve and zeroes, per point and class, the tapers of all but the cap[c] largest; a zero taper is "not listed" to every kernel
// above (the select of the Gram, the n_local loop, p3), so none of them changes.
// This file holds the kernels and their launchers only.
#include "efa_driver.h"
#include "efa_device.h"
#include "efa_etkf_eig.h"
#include "efa_rows.h"
#include "efa_slabfactor.h"

#include <cstdint>

namespace efa {
namespace {

typedef double letkf_v4 __attribute__((ext_vector_type(4)));

constexpr int kLetkfChunk = 32;  // obs per stage: 8 MFMA steps of 4
constexpr int kLetkfRows = 4;    // rows per apply batch (one wave each for the row reductions)
constexpr int kLetkfTiles = 3;   // tiles a wave may own
constexpr int kLetkfSmall = 16;  // doubles of per-row scalars: mean [4] | xam [4] | ssb [4] | inflation scalars [4]

// ctl (the control analysis): the staged row is [Yp_k | d_k | d^c_k], the product (M+2)^2
__host__ __device__ inline int letkf_tiles_side(int M, bool ctl = false) { return (M + (ctl ? 2 : 1) + 15) / 16; }
__host__ __device__ inline int letkf_stage_pitch(int M, bool ctl = false) { return 16 * (letkf_tiles_side(M, ctl) | 1); }
// doubles of the region the stage and the M x M array share
__host__ __device__ inline int letkf_region(int M, bool ctl = false) {
  const int st = kLetkfChunk * letkf_stage_pitch(M, ctl) + kLetkfChunk, mm = M * M;
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

// The control's innovations beside dr, under the flag k_letkf_prior decided on the ENSEMBLE mean: the control never
// votes, and neither value nor yc of an ob with a flag of 0 is read.
__global__ __launch_bounds__(256) void k_letkf_control_prior(long P, const double* __restrict__ ob_value, const double* __restrict__ yc,
                                                             const uint8_t* __restrict__ assimilated, double* __restrict__ dc) {
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= P) return;
  dc[k] = assimilated[k] ? ob_value[k] - yc[k] : 0.0;
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

// SLAB: one workgroup per (column, slab group), the group the fastest index of the launch so that the
// workgroups of a column run together and find its list and Yp rows in L2; the staged weight is fl(fl(rho S[k][rep[g]]) / r), the
// apply walks the group's slabs, the statistics and the pairs are laid out [group][point].
struct LetkfSlabArgs : LetkfArgs {
  LetkfGroups grp;
};
template <bool SLAB>
struct LetkfArgsOf { typedef LetkfArgs type; };
template <>
struct LetkfArgsOf<true> { typedef LetkfSlabArgs type; };

// k_letkf's argument block where it is needed and not before (k_letkf's only parameter is a LetkfArgs or begins with one,
// LetkfSlabArgs' base: the kernel's argument block is one).  What is read through it is not held in scalar registers from the entry
// on: the slab launch has none to spare, and what does not fit goes to vector registers and costs it a wave per SIMD.
typedef const __attribute__((address_space(4))) LetkfArgs* letkf_kernarg_ptr;
__device__ __forceinline__ letkf_kernarg_ptr letkf_kernarg() { return (letkf_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr(); }

// The inflation estimate of a point (Miyoshi 2011), by one lane, from the sums the solve left in sc = lambda_b | p3 |
// p1 | trace(C): the statistics as computed, and lambda_a over the field unless p2, p3 or the estimate rule it out.  The solve used
// lambda_b.  Called at the kernel's exits, where nothing else is live.
__device__ __forceinline__ void letkf_inflation_estimate(size_t pt, int M, const double* sc) {
  // its four parameters are read HERE from the kernel's argument block (letkf_kernarg)
  const auto& a = *letkf_kernarg();
  if (!a.infl_stats && !(a.infl_sigma2 > 0.0)) return;
  const double lb = sc[0], p3 = sc[1], p1 = sc[2], p2 = sc[3] / (double)(M - 1);
  const double lo = (p1 - p3) / p2;
  if (a.infl_stats) {
    double* st = a.infl_stats + 4 * pt;
    st[0] = p1;
    st[1] = p2;
    st[2] = p3;
    st[3] = lo;
  }
  if (a.infl_sigma2 > 0.0 && p2 > 0.0 && p3 > 0.0 && p2 < __builtin_inf() && p3 < __builtin_inf()) {
    const double q = (lb * p2 + p3) / p2;
    const double vo = (2.0 / p3) * (q * q);
    const double la = lb + a.infl_sigma2 / (vo + a.infl_sigma2) * (lo - lb);
    if (la - la == 0.0) a.infl[pt] = fmin(fmax(la, a.infl_lo), a.infl_hi);  // a non-finite estimate leaves the field as it is
  }
}

// CTRL: the deterministic control analysis beside the ensemble's.  A template switch, so that the instantiations
// without it are today's instruction for instruction; with it the Gram carries one more B-operand column (g^c), h^c = (V_j . g^c)/mu_j
// goes over n_s behind the sweeps, and the row's wave adds h^c . z to the control's value of its row.  Nothing of the ensemble's
// arithmetic changes: the tiles are independent accumulators, and every reduction keeps its order whatever the tile side is.
template <int MODE, typename E, int NTMAX, bool SLAB = false, bool CTRL = false>
__global__ __launch_bounds__(NTMAX) void k_letkf(const typename LetkfArgsOf<SLAB>::type a) {
  static_assert(!CTRL || MODE != kLetkfWeights, "the pair layout [M][M+1] has no place for w^c");
  extern __shared__ __align__(16) double letkf_smem[];
  const int M = a.M;
  const int tid = (int)threadIdx.x, nth = (int)blockDim.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nW = nth >> 6;
  const int T = letkf_tiles_side(M, CTRL), Sp = letkf_stage_pitch(M, CTRL), ntiles = T * (T + 1) / 2;
  double* G = letkf_smem;                     // the M x M array; before it the stage [32][Sp] | weights [32]
  double* wgt = G + kLetkfChunk * Sp;
  double* g_s = G + letkf_region(M, CTRL);
  double* f_s = g_s + M;
  double* h_s = f_s + M;
  double* n_s = h_s + M;
  double* mu_s = n_s + M;
  double* x_s = mu_s + M;                     // [4][M] rows of a batch: members, perturbations, then posterior perturbations
  double* z_s = x_s + kLetkfRows * M;         // [4][M] V^T x'
  double* mean_s = z_s + kLetkfRows * M;
  double* xam_s = mean_s + kLetkfRows;
  double* ssb_s = xam_s + kLetkfRows;
  double* infl_s = ssb_s + kLetkfRows;         // inflation (§7y-6): lambda_b | p3 | p1 | trace(C)
  int* rot_s = reinterpret_cast<int*>(mean_s + kLetkfSmall);
  int* nloc_s = rot_s + 2;
  double* gc_s = mean_s + kLetkfSmall + 2;    // CTRL: g^c [M] behind the ints (16-byte aligned); h^c takes n_s behind the sweeps

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

  // n_local: the listed obs whose taper on THIS column is not zero; under inflation p3, the sum of those tapers (each lane its
  // entries in list order, then the butterfly)
  const bool infl = a.infl != nullptr;  // (uniform)
  if (wave == 0) {
    int cl = 0;
    double p3 = 0.0;
    for (int e = lane; e < n; e += 64) {
      double w = a.wts[(size_t)(off + e) * 16 + cb];
      if constexpr (SLAB) w = w * Sg[(size_t)a.idx[off + e] * sp];
      cl += (w != 0.0) ? 1 : 0;
      if (infl && w != 0.0) p3 += w;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cl += __shfl_xor(cl, o, 64);
    if (infl) p3 = wave_sum(p3);
    if (lane == 0) {
      *nloc_s = cl;
      infl_s[0] = infl ? a.infl[grp * a.npts + col] : 1.0;
      infl_s[1] = p3;
    }
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
      if constexpr (CTRL) {  // the control's rows likewise: copied bit for bit, or left alone in place
        const double* cin = letkf_kernarg()->ctl_in;
        double* cout = letkf_kernarg()->ctl_out;
        if (cin != cout)
          for (long li = tid; li < nlead_g; li += nth) {
            long l = li;
            if constexpr (SLAB) l = leads[li];
            cout[l * a.npts + col] = cin[l * a.npts + col];
          }
      }
    } else if (MODE == kLetkfPerts) {
      for (int m = tid; m < M; m += nth) a.Yp_out[(size_t)col * M + m] = a.Yp_in[(size_t)col * M + m];
      if (tid == 0) a.ym_out[col] = a.ym_in[col];
      if constexpr (CTRL) {
        if (tid == 0) letkf_kernarg()->ctl_out[col] = letkf_kernarg()->ctl_in[col];
      }
    } else {
      double* tw = a.Tw + (size_t)(grp * a.npts + col) * M * (M + 1);
      for (int e = tid; e < M * (M + 1); e += nth) {
        const int r = e / (M + 1), c = e - r * (M + 1);
        tw[e] = (r == c) ? 1.0 : 0.0;
      }
    }
    if (a.stats && tid < 3) a.stats[3 * (grp * a.npts + col) + tid] = 0.0;
    if (infl && a.infl_stats && tid < 4) a.infl_stats[4 * (grp * a.npts + col) + tid] = (tid < 3) ? 0.0 : __builtin_nan("");  // lambda keeps its bits
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
        if (en < n && c <= M + (CTRL ? 1 : 0)) {
          const long k = a.idx[off + en];
          if constexpr (CTRL) v = (c < M) ? a.Yp[(size_t)k * M + c] : (c == M) ? a.dr[2 * k] : letkf_kernarg()->dc[k];
          else v = (c < M) ? a.Yp[(size_t)k * M + c] : a.dr[2 * k];
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
    const double shift = (double)(M - 1) / infl_s[0];  // the diagonal of A; (M-1)/1.0 is exact: no field, the bits without one
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
            const double val = (I == J) ? s + shift : s;
            G[I * M + J] = val;
            G[J * M + I] = val;
            if (infl && I == J) n_s[I] = s;  // the diagonal of C, for its trace (n_s is free until the sweeps)
          } else if (I < M && J == M) {
            g_s[I] = s;
          } else if (CTRL && I < M && J == M + 1) {
            gc_s[I] = s;  // g^c; entries (M, M+1) and (M+1, M+1) are dropped
          } else if (infl && I == M && J == M) {
            infl_s[2] = s;  // p1 = sum_k w_k d_k^2
          }
        }
      }
    }
    __syncthreads();
    if (infl) {  // (uniform) trace(C) in a fixed order before the sweeps take n_s
      if (wave == 0) {
        double tr = 0.0;
        for (int j = lane; j < M; j += 64) tr += n_s[j];
        tr = wave_sum(tr);
        if (lane == 0) infl_s[3] = tr;
      }
      __syncthreads();
    }
  }

  // ---- 2. eigen-solve ---------------------------------------------------------------------------------------------------------
  const int sweeps = etkf_jacobi(M, G, n_s, rot_s, tid, nth);
  etkf_factors(M, G, g_s, mu_s, f_s, h_s, tid, nth);
  if constexpr (CTRL) {  // h^c_j = (V_j . g^c) / mu_j over n_s, which the sweeps have left; read behind the apply's first barrier
    const int nslots_c = nth >> 4, slot_c = tid >> 4, sl_c = tid & 15;
#pragma unroll 1
    for (int j = slot_c; j < M; j += nslots_c) {
      const double* cj = G + (size_t)j * M;
      double hg = 0.0;
      for (int i = sl_c; i < M; i += 16) hg = fma(cj[i], gc_s[i], hg);
      hg = group_sum<16>(hg);
      if (sl_c == 0) n_s[j] = hg / mu_s[j];
    }
  }
  if (a.stats && wave == 0) {
    const double shift = (double)(M - 1) / infl_s[0];
    double s = 0.0;
    for (int j = lane; j < M; j += 64) s += (mu_s[j] - shift) / mu_s[j];
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
    if (infl && tid == 0) letkf_inflation_estimate((size_t)(grp * a.npts + col), M, infl_s);
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
      if constexpr (CTRL) {  // x_c^a = x_c + x' . w^c = x_c + h^c . z, by the wave that owns the row
        double sc = 0.0;
        for (int j = lane; j < M; j += 64) {
          s = fma(h_s[j], zr[j], s);
          sc = fma(n_s[j], zr[j], sc);
        }
        s = wave_sum(s);
        sc = wave_sum(sc);
        if (lane == 0) {
          xam_s[wave] = mean_s[wave] + s;
          long row = col;
          if (MODE == kLetkfMembers) {
            long l = r0 + wave;
            if constexpr (SLAB) l = leads[l];
            row = l * a.npts + col;
          }
          letkf_kernarg()->ctl_out[row] = letkf_kernarg()->ctl_in[row] + sc;  // (the pointers from the argument block, here)
        }
      } else {
        for (int j = lane; j < M; j += 64) s = fma(h_s[j], zr[j], s);
        s = wave_sum(s);
        if (lane == 0) xam_s[wave] = mean_s[wave] + s;
      }
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
  if (infl && tid == 0) letkf_inflation_estimate((size_t)(grp * a.npts + col), M, infl_s);
}

template <int MODE, typename E, int NTMAX, bool SLAB, bool CTRL>
hipError_t letkf_launch_as(const typename LetkfArgsOf<SLAB>::type& a, int nth, size_t lds, hipStream_t s) {
  auto kern = k_letkf<MODE, E, NTMAX, SLAB, CTRL>;
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  long nwg = (a.npts + 15) / 16 * 16;
  if constexpr (SLAB) nwg *= a.grp.ngroups;
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3((unsigned)nth), lds, s, a);
  return hipGetLastError();
}

template <int MODE, typename E, bool SLAB, bool CTRL>
hipError_t letkf_launch_ctl(const typename LetkfArgsOf<SLAB>::type& a, hipStream_t s) {
  const int nth = letkf_threads(a.M, CTRL);
  const size_t lds = letkf_lds_bytes(a.M, CTRL);
  if (nth <= 256) return letkf_launch_as<MODE, E, 256, SLAB, CTRL>(a, nth, lds, s);
  if (nth <= 512) return letkf_launch_as<MODE, E, 512, SLAB, CTRL>(a, nth, lds, s);
  return letkf_launch_as<MODE, E, 1024, SLAB, CTRL>(a, nth, lds, s);
}

// ... with the control analysis when its innovations are given (launch_letkf refuses them for kLetkfWeights)
template <int MODE, typename E, bool SLAB>
hipError_t letkf_launch_mode(const typename LetkfArgsOf<SLAB>::type& a, hipStream_t s) {
  if constexpr (MODE != kLetkfWeights) {
    if (a.dc) return letkf_launch_ctl<MODE, E, SLAB, true>(a, s);
  }
  return letkf_launch_ctl<MODE, E, SLAB, false>(a, s);
}

// the plain launch, or with groups the SLAB one on (a, *grp)
template <int MODE, typename E>
hipError_t letkf_launch(const LetkfArgs& a, const LetkfGroups* grp, hipStream_t s) {
  if (!grp) return letkf_launch_mode<MODE, E, false>(a, s);
  LetkfSlabArgs sa{};
  static_cast<LetkfArgs&>(sa) = a;
  sa.grp = *grp;
  return letkf_launch_mode<MODE, E, true>(sa, s);
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

// ---- the cap on the local obs of a solve -------------------------------------------------------------------------
// One workgroup per block of 16 points, between the list build and the solve.  Thread t = (column t & 15, entry slot t >> 4): a wave
// reads four whole 128-byte entries of wts per step.  Per class that is over its cap at some column of the block, a radix select on
// the taper's 64-bit pattern, most significant byte first: the counts of the byte's 256 values per column in LDS (integer atomics),
// then per column the value at which the places run out; a column stops as soon as the candidates that remain equal the places that
// remain.  The keys are re-read through L2 in every pass (a list is up to P long).  One more pass in list order, each wave a
// contiguous quarter of the list, zeroes the losers; at a threshold shared by more candidates than places (equal bits) the first in
// list order win, their ranks from ballots within the wave and, across the waves, from a counting pass that runs only then.
constexpr int kCapThreads = 256;
constexpr int kCapBins = 256;
// the count of byte value d on column c.  Rows of 16 columns: the 16 columns of an entry never share a bank, whatever their bytes are
// (neighbouring columns have nearly the same taper, so [column][value] would put them on one bank).  One row of padding per 16 values:
// the runs of 16 values that the four slots of a wave sum start 16 banks apart.
__device__ __forceinline__ int cap_hist(int d, int c) { return (d + (d >> 4)) * 16 + c; }
// every double but NaN orders as this key; positive doubles as their bits
__device__ __forceinline__ unsigned long long cap_key(double w) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(w);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ __launch_bounds__(kCapThreads) void k_letkf_cap(const LetkfCapArgs a) {
  __shared__ unsigned hist[(kCapBins + kCapBins / 16) * 16];
  __shared__ unsigned part[16][16];                  // [slot][column] the sum of values 16 slot .. 16 slot + 15
  __shared__ int reach_s[kLetkfCapClasses][16];      // the non-zero tapers per (class, column)
  __shared__ unsigned long long pre_s[16];           // per column: the key's leading bytes decided so far,
  __shared__ int need_s[16], cand_s[16];             //   the places left for the candidates that have them, and how many those are,
  __shared__ int sel_s[16], bite_s[16], shift_s[16]; //   still selecting, over the cap at all, the shift at which it stopped
  __shared__ int tie_s[kCapThreads / 64][16];        // [wave][column] the candidates at the threshold in the wave's part of the list
  const int tid = (int)threadIdx.x, col = tid & 15, slot = tid >> 4, lane = tid & 63, wv = tid >> 6;
  const long blk = (long)blockIdx.x;
  const long off = a.off[blk];
  const int n = a.cnt[blk];
  double* wts = a.wts + (size_t)off * 16;
  const int* idx = a.idx + off;

  for (int i = tid; i < kLetkfCapClasses * 16; i += kCapThreads) (&reach_s[0][0])[i] = 0;
  __syncthreads();
  for (int e = slot; e < n; e += 16) {
    if (wts[(size_t)e * 16 + col] == 0.0) continue;
    const int cls = a.ob_class ? a.ob_class[idx[e]] : 0;
    atomicAdd(&reach_s[cls][col], 1);
  }
  __syncthreads();
  if (a.reach && tid < 16 && blk * 16 + tid < a.npts) {
    int r = 0;
    for (int c = 0; c < a.nclass; ++c) r += reach_s[c][tid];
    a.reach[blk * 16 + tid] = (double)r;
  }

#pragma unroll 1
  for (int c = 0; c < a.nclass; ++c) {
    const int cap = a.cap[c];
    if (cap <= 0) continue;  // (uniform) no limit
    const int reach = reach_s[c][col];
    if (!__syncthreads_or(reach > cap)) continue;  // no column of the block is over this class's cap: nothing is written
    if (tid < 16) {  // (col == tid)
      pre_s[tid] = 0ull;
      need_s[tid] = cap;
      cand_s[tid] = reach;
      sel_s[tid] = bite_s[tid] = reach > cap ? 1 : 0;
      shift_s[tid] = 0;
    }
    // ---- the select: one byte per pass, most significant first ------------------------------------------------------------------
#pragma unroll 1
    for (int shift = 56;; shift -= 8) {
      for (int i = tid; i < (kCapBins + kCapBins / 16) * 16; i += kCapThreads) hist[i] = 0u;
      __syncthreads();
      const bool sel = sel_s[col] != 0;
      const unsigned long long pre = pre_s[col];
      if (sel)
        for (int e = slot; e < n; e += 16) {
          const double w = wts[(size_t)e * 16 + col];
          if (w == 0.0) continue;
          if (a.ob_class && a.ob_class[idx[e]] != c) continue;
          const unsigned long long key = cap_key(w);
          if (shift < 56 && (key >> (shift + 8)) != pre) continue;
          atomicAdd(&hist[cap_hist((int)((key >> shift) & 255ull), col)], 1u);
        }
      __syncthreads();
      {
        unsigned s = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) s += hist[cap_hist(16 * slot + j, col)];
        part[slot][col] = s;
      }
      __syncthreads();
      if (tid < 16 && sel) {  // from the largest value down to the one at which the places run out (the candidates outnumber them)
        int need = need_s[tid];
        unsigned acc = 0u;
        int sl = 15;
        for (; sl > 0; --sl) {
          const unsigned p = part[sl][tid];
          if (acc + p >= (unsigned)need) break;
          acc += p;
        }
        int d = 16 * sl + 15;
        for (; d > 16 * sl; --d) {
          const unsigned h = hist[cap_hist(d, tid)];
          if (acc + h >= (unsigned)need) break;
          acc += h;
        }
        const int h = (int)hist[cap_hist(d, tid)];
        need -= (int)acc;
        pre_s[tid] = (pre << 8) | (unsigned long long)d;
        need_s[tid] = need;
        cand_s[tid] = h;
        if (h == need || shift == 0) {  // every candidate left has a place, or the bits are out: equal tapers, list order decides
          sel_s[tid] = 0;
          shift_s[tid] = shift;
        }
      }
      if (!__syncthreads_or(tid < 16 && sel_s[tid] != 0)) break;  // (shift == 0 ends every column)
    }
    // ---- the losers to zero, in list order ---------------------------------------------------------------------------------------
    const int ties = __syncthreads_or(tid < 16 && bite_s[tid] != 0 && need_s[tid] < cand_s[tid]);
    const bool bite = bite_s[col] != 0;
    const unsigned long long pre = pre_s[col];
    const int fs = shift_s[col], need = need_s[col];
    const int sub = lane >> 4;
    const int nstep = (n + 3) >> 2, per = (nstep + kCapThreads / 64 - 1) / (kCapThreads / 64);
    const int s0 = wv * per, s1 = (s0 + per < nstep) ? s0 + per : nstep;
    const unsigned long long colbits = 0x0001000100010001ull << col;  // this column's lanes of the wave
    int base = 0;
    if (ties) {  // (uniform)
      int cnt = 0;
      for (int st = s0; st < s1; ++st) {
        const int e = 4 * st + sub;
        const double w = (e < n) ? wts[(size_t)e * 16 + col] : 0.0;
        bool eq = bite && w != 0.0;
        if (eq && a.ob_class) eq = a.ob_class[idx[e]] == c;
        eq = eq && (cap_key(w) >> fs) == pre;
        cnt += __builtin_popcountll(__ballot(eq) & colbits);
      }
      if (lane < 16) tie_s[wv][lane] = cnt;
      __syncthreads();
      for (int v = 0; v < wv; ++v) base += tie_s[v][col];
    }
    int run = base;
    for (int st = s0; st < s1; ++st) {
      const int e = 4 * st + sub;
      const double w = (e < n) ? wts[(size_t)e * 16 + col] : 0.0;
      bool cnd = bite && w != 0.0;
      if (cnd && a.ob_class) cnd = a.ob_class[idx[e]] == c;
      const unsigned long long top = cap_key(w) >> fs;
      const bool eq = cnd && top == pre;
      const unsigned long long mine = __ballot(eq) & colbits;
      const int rank = run + __builtin_popcountll(mine & ((1ull << (16 * sub)) - 1ull));
      if (cnd && (top < pre || (eq && rank >= need))) wts[(size_t)e * 16 + col] = 0.0;
      run += __builtin_popcountll(mine);
    }
  }
}

}  // namespace

// The workgroup size, from M: the eigen-solve (where a column spends its time) plays ceil(M/2) column pairs per round on 16 lanes
// each, so 16 ceil(M/2) threads keep every lane of it busy and more would idle there; rounded up to whole waves, at least four (one
// per row of an apply batch) and at most 1024, and enough waves for the Gram's upper tiles at three per wave.  At 40 members that is
// 320 threads and 17 KB of LDS: nine workgroups fit a CU's LDS and four its registers, where 1024 threads would leave room for one.
int letkf_threads(int M, bool ctl) {
  const int npairs = (M + 1) / 2;
  int nth = 64 * ((16 * npairs + 63) / 64);
  if (nth < 64 * kLetkfRows) nth = 64 * kLetkfRows;
  if (nth > 1024) nth = 1024;
  const int T = letkf_tiles_side(M, ctl), ntiles = T * (T + 1) / 2;
  while (nth < 1024 && kLetkfTiles * (nth / 64) < ntiles) nth += 64;
  return nth;
}

size_t letkf_lds_bytes(int M, bool ctl) {
  // region | g, f, h, n, mu [M] each | x, z [4][M] each | per-row scalars | rot [2], n_local (ints) | ctl: g^c [M]
  return ((size_t)letkf_region(M, ctl) + (size_t)(5 + 2 * kLetkfRows) * M + kLetkfSmall + 2 + (ctl ? (size_t)M : 0)) * sizeof(double);
}

hipError_t launch_letkf(const LetkfArgs& a, const LetkfGroups* grp, int mode, Elem elem, hipStream_t s) {
  if (a.M < 2 || a.M > kLetkfMaxM || a.npts < 0) return hipErrorInvalidValue;
  const bool ctl = a.dc != nullptr;
  if (ctl && (mode == kLetkfWeights || !a.ctl_in || !a.ctl_out)) return hipErrorInvalidValue;
  const int T = letkf_tiles_side(a.M, ctl);
  if (kLetkfTiles * (letkf_threads(a.M, ctl) / 64) < T * (T + 1) / 2 || letkf_lds_bytes(a.M, ctl) > 160 * 1024) return hipErrorInvalidValue;
  if (grp) {
    if (grp->ngroups < 1 || !grp->rep || !grp->grp_off || !grp->grp_leads || grp->s_pitch < 1) return hipErrorInvalidValue;
    if (a.idx && !grp->S) return hipErrorInvalidValue;  // (no lists: the table is never read)
  }
  if (a.npts == 0) return hipSuccess;
  if ((a.npts + 15) / 16 * 16 > 0x7FFFFFF0L / (grp ? grp->ngroups : 1)) return hipErrorInvalidValue;
  if (mode == kLetkfMembers) {
    if (!a.Xin || !a.Xout || a.n_lead < 1) return hipErrorInvalidValue;
    return elem == Elem::f32 ? letkf_launch<kLetkfMembers, float>(a, grp, s) : letkf_launch<kLetkfMembers, double>(a, grp, s);
  }
  if (elem != Elem::f64) return hipErrorInvalidValue;
  if (mode == kLetkfPerts) {  // (no SLAB instantiation: the obs block runs on lists that carry the factors already)
    if (grp || !a.ym_in || !a.Yp_in || !a.ym_out || !a.Yp_out) return hipErrorInvalidValue;
    return letkf_launch_mode<kLetkfPerts, double, false>(a, s);
  }
  if (mode == kLetkfWeights) {
    if (!a.Tw) return hipErrorInvalidValue;
    return letkf_launch<kLetkfWeights, double>(a, grp, s);
  }
  return hipErrorInvalidValue;
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

hipError_t launch_letkf_cap(const LetkfCapArgs& a, hipStream_t s) {
  if (a.npts <= 0) return hipSuccess;
  if (!a.off || !a.cnt || !a.idx || !a.wts || a.nclass < 1 || a.nclass > kLetkfCapClasses) return hipErrorInvalidValue;
  bool any = a.reach != nullptr;
  for (int c = 0; c < a.nclass; ++c) {
    if (a.cap[c] < 0) return hipErrorInvalidValue;
    any = any || a.cap[c] > 0;
  }
  if (!any) return hipSuccess;
  const long nblk = (a.npts + 15) / 16;
  if (nblk > 0x7FFFFFF0L) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_letkf_cap, dim3((unsigned)nblk), dim3(kCapThreads), 0, s, a);
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

hipError_t launch_letkf_control_prior(long P, const double* ob_value, const double* yc, const uint8_t* assimilated, double* dc,
                                      hipStream_t s) {
  if (P < 1 || !ob_value || !yc || !assimilated || !dc) return hipErrorInvalidValue;
  const long b = (P + 255) / 256;
  if (b > 0x7FFFFFF0L) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_letkf_control_prior, dim3((unsigned)b), dim3(256), 0, s, P, ob_value, yc, assimilated, dc);
  return hipGetLastError();
}

}  // namespace efa
