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
// Cross validation over member groups (Buehner 2020; efa_ctx_set_letkf_cross_validation): k_letkf_cv is the weights
// mode with the switch CV.  The Gram also parks C in the point's M x M block of a context-owned global scratch, the mean's solve runs as
// above and leaves w, and then per group k (I: the members of the other groups, H: its own, m = |I|, a = m - 1, J = I - 11^T/m)
// J C[I,I] J + a I goes into the LDS array, etkf_jacobi runs on it, and T[I,H] = -J V diag(1/(mu (1 + sqrt(a/mu)))) V^T J C[I,H] and
// the identity block T[H,H] go to the point's [M][M+1] pair in global memory; one pass takes the row means off T; with Yp_in the
// point's row of the obs block is mapped by its own pair.  The state is applied by k_letkf_interp (efa_letkf_interp.hip), without a
// mesh on the unit mesh whose nodes are the columns.  The body of k_letkf and k_letkf_cv is one text, efa_letkf_point.inc: with CV off
// it is k_letkf as it was, instruction for instruction.
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
//
// CV: the cross-validated perturbation update (Buehner 2020) of kLetkfWeights, k_letkf_cv's switch.  The body of
// both kernels is one text, efa_letkf_point.inc: with CV off it is k_letkf instruction for instruction (a kernel of another name,
// because the instantiations of k_letkf are counted and named by the tests).  With it the Gram also parks C in the point's M x M
// block of the context's scratch (global, re-read through L2), the mean's solve runs as it is and leaves w, and letkf_cv_transform
// forms T group by group from C.
struct LetkfCvArgs : LetkfArgs {
  LetkfCv cv;
};

// The cross-validated T of one point, by the whole workgroup, behind the mean's solve: every LDS vector but the
// M x M array G is free.  Per group k, from the lists the host made (perm[k] = I ascending | H ascending, nind[k] = |I| = m):
//   B = J C[I,I] J + (m-1) I into G (pitch m) from the row means of C[I,I], etkf_jacobi on it, V and mu, d_j = 1/(mu_j (1 + sqrt(a/mu_j)));
//   four held-out members at a time, as k_letkf's apply takes four rows: x = J C[I,h], z = d . (V^T x), t = V z, T[I,h] = -(t - mean(t)),
//   T[H,h] = the identity's column.
// Then one pass per row of T: its sum over 16 lanes in a fixed order, the mean taken off.  With Yp_in the point's one row of the obs
// block is mapped by its own [T | w] at the end.  No atomics; C and T are written and re-read by this workgroup only.
template <typename A>
__device__ __forceinline__ void letkf_cv_transform(const A& a, int M, long col, double* G, double* il_s, double* rb_s, double* d_s,
                                                   double* n_s, double* mu_s, double* x_s, double* z_s, double* mean_s, int* rot_s,
                                                   int tid, int nth) {
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nslots = nth >> 4, slot = tid >> 4, sl = tid & 15;
  const double* Cg = a.cv.C + (size_t)col * M * M;
  double* tw = a.Tw + (size_t)col * M * (M + 1);
  int* il = reinterpret_cast<int*>(il_s);  // [M] the group's I, then its H
  int swsum = 0;
  double cmax = 0.0;  // (wave 0)
#pragma unroll 1
  for (int k = 0; k < a.cv.ngroups; ++k) {
    const int m = a.cv.nind[k], nh = M - m;
    const double am = (double)(m - 1);
    __syncthreads();  // the previous group's lists, vectors and G are consumed
    for (int e = tid; e < M; e += nth) il[e] = a.cv.perm[(size_t)k * M + e];
    __syncthreads();
    // the row means of C[I,I], then their mean
#pragma unroll 1
    for (int i = slot; i < m; i += nslots) {
      const double* cr = Cg + (size_t)il[i] * M;
      double s = 0.0;
      for (int j = sl; j < m; j += 16) s += cr[il[j]];
      s = group_sum<16>(s);
      if (sl == 0) rb_s[i] = s / (double)m;
    }
    __syncthreads();
    if (wave == 0) {
      double s = 0.0;
      for (int i = lane; i < m; i += 64) s += rb_s[i];
      s = wave_sum(s);
      if (lane == 0) mean_s[0] = s / (double)m;
    }
    __syncthreads();
    const double cbar = mean_s[0];
    for (int e = tid; e < m * m; e += nth) {  // (rb_i + rb_j commutes: B is symmetric to the bit, as C is)
      const int i = e / m, j = e - i * m;
      const double v = (Cg[(size_t)il[i] * M + il[j]] - (rb_s[i] + rb_s[j])) + cbar;
      G[e] = (i == j) ? v + am : v;
    }
    __syncthreads();
    swsum += etkf_jacobi(m, G, n_s, rot_s, tid, nth);
#pragma unroll 1
    for (int j = slot; j < m; j += nslots) {  // V in place, mu, d
      double* cj = G + (size_t)j * m;
      double al = 0.0;
      for (int i = sl; i < m; i += 16) al = fma(cj[i], cj[i], al);
      al = group_sum<16>(al);
      const double mu = sqrt(al);
      for (int i = sl; i < m; i += 16) cj[i] = cj[i] / mu;
      if (sl == 0) {
        mu_s[j] = mu;
        d_s[j] = 1.0 / (mu * (1.0 + sqrt(am / mu)));
      }
    }
    __syncthreads();
    if (wave == 0) {  // the sub-solve's condition number
      double hi = 0.0, lo = __builtin_inf();
      for (int j = lane; j < m; j += 64) {
        hi = fmax(hi, mu_s[j]);
        lo = fmin(lo, mu_s[j]);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        hi = fmax(hi, __shfl_xor(hi, o, 64));
        lo = fmin(lo, __shfl_xor(lo, o, 64));
      }
      cmax = fmax(cmax, hi / lo);
    }
#pragma unroll 1
    for (int h0 = 0; h0 < nh; h0 += kLetkfRows) {
      const int nr = (nh - h0 < kLetkfRows) ? nh - h0 : kLetkfRows;
      for (int e = tid; e < nr * m; e += nth) {
        const int r = e / m, i = e - r * m;
        x_s[e] = Cg[(size_t)il[i] * M + il[m + h0 + r]];
      }
      __syncthreads();
      if (wave < nr) {  // x = J C[I,h]
        double* xr = x_s + wave * m;
        double s = 0.0;
        for (int i = lane; i < m; i += 64) s += xr[i];
        const double mean = wave_sum(s) / (double)m;
        for (int i = lane; i < m; i += 64) xr[i] -= mean;
      }
      __syncthreads();
#pragma unroll 1
      for (int pr = slot; pr < nr * m; pr += nslots) {  // z[r][j] = d_j (V_j . x_r)
        const int r = pr / m, j = pr - r * m;
        const double* cj = G + (size_t)j * m;
        const double* xr = x_s + r * m;
        double d = 0.0;
        for (int i = sl; i < m; i += 16) d = fma(cj[i], xr[i], d);
        d = group_sum<16>(d);
        if (sl == 0) z_s[pr] = d_s[j] * d;
      }
      __syncthreads();
      for (int e = tid; e < nr * m; e += nth) {  // t[r][b] = sum_j z[r][j] V[b][j]
        const int r = e / m, b = e - r * m;
        const double* zr = z_s + r * m;
        double acc = 0.0;
        for (int j = 0; j < m; ++j) acc = fma(zr[j], G[(size_t)j * m + b], acc);
        x_s[e] = acc;
      }
      __syncthreads();
      if (wave < nr) {
        const double* tr = x_s + wave * m;
        const int hc = il[m + h0 + wave];
        double s = 0.0;
        for (int i = lane; i < m; i += 64) s += tr[i];
        const double mean = wave_sum(s) / (double)m;
        for (int i = lane; i < m; i += 64) tw[(size_t)il[i] * (M + 1) + hc] = mean - tr[i];
        for (int q = lane; q < nh; q += 64) tw[(size_t)il[m + q] * (M + 1) + hc] = (il[m + q] == hc) ? 1.0 : 0.0;
      }
      __syncthreads();  // the batch is stored: the next one takes x_s
    }
  }
  __syncthreads();  // every column of T is written (by this workgroup: visible behind the barrier)
#pragma unroll 1
  for (int r = slot; r < M; r += nslots) {  // recentre: the row's mean off its entries
    double* row = tw + (size_t)r * (M + 1);
    double s = 0.0;
    for (int b = sl; b < M; b += 16) s += row[b];
    const double mean = group_sum<16>(s) / (double)M;
    for (int b = sl; b < M; b += 16) row[b] -= mean;
  }
  if (a.cv.stats && tid == 0) {
    a.cv.stats[2 * col] = (double)swsum;
    a.cv.stats[2 * col + 1] = cmax;
  }
  if (a.Yp_in) {  // (uniform) the obs block: the point's own row through its own pair, column M of which is w
    for (int m2 = tid; m2 < M; m2 += nth) x_s[m2] = a.Yp_in[(size_t)col * M + m2];
    __syncthreads();
    for (int b = tid; b <= M; b += nth) {
      double acc = 0.0;
      for (int r = 0; r < M; ++r) acc = fma(x_s[r], tw[(size_t)r * (M + 1) + b], acc);
      if (b < M) a.Yp_out[(size_t)col * M + b] = acc;
      else a.ym_out[col] = a.ym_in[col] + acc;
    }
  }
}

template <int MODE, typename E, int NTMAX, bool SLAB = false, bool CTRL = false>
__global__ __launch_bounds__(NTMAX) void k_letkf(const typename LetkfArgsOf<SLAB>::type a) {
  constexpr bool CV = false;
#include "efa_letkf_point.inc"
}

// the solve points under cross validation: [T | w] of every point to Tw, with Yp_in the obs block's rows as well
// (A is LetkfCvArgs: a template parameter so that the body's SLAB and CTRL branches, which name members it lacks, stay dependent)
template <int NTMAX, typename A>
__global__ __launch_bounds__(NTMAX) void k_letkf_cv(const A a) {
  constexpr int MODE = kLetkfWeights;
  constexpr bool SLAB = false, CTRL = false, CV = true;
  typedef double E;
#include "efa_letkf_point.inc"
}

template <int NTMAX>
hipError_t letkf_cv_launch_as(const LetkfCvArgs& a, int nth, size_t lds, hipStream_t s) {
  auto kern = k_letkf_cv<NTMAX, LetkfCvArgs>;
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)((a.npts + 15) / 16 * 16)), dim3((unsigned)nth), lds, s, a);
  return hipGetLastError();
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

hipError_t launch_letkf_cv(const LetkfArgs& a, const LetkfCv& cv, hipStream_t s) {
  if (a.M < 4 || a.M > kLetkfMaxM || a.npts < 0 || letkf_lds_bytes(a.M) > 160 * 1024) return hipErrorInvalidValue;
  if (cv.ngroups < 2 || cv.ngroups > a.M || !cv.perm || !cv.nind || !cv.C || !a.Tw) return hipErrorInvalidValue;
  if (a.infl || a.dc) return hipErrorInvalidValue;  // (out of scope: the driver refuses both before any launch)
  if (a.Yp_in && (!a.ym_in || !a.ym_out || !a.Yp_out)) return hipErrorInvalidValue;
  if (a.npts == 0) return hipSuccess;
  if ((a.npts + 15) / 16 * 16 > 0x7FFFFFF0L) return hipErrorInvalidValue;
  LetkfCvArgs ca{};
  static_cast<LetkfArgs&>(ca) = a;
  ca.cv = cv;
  const int nth = letkf_threads(a.M);
  const size_t lds = letkf_lds_bytes(a.M);
  if (nth <= 256) return letkf_cv_launch_as<256>(ca, nth, lds, s);
  if (nth <= 512) return letkf_cv_launch_as<512>(ca, nth, lds, s);
  return letkf_cv_launch_as<1024>(ca, nth, lds, s);
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
