// LETKF weight interpolation (Yang, Kalnay, Hunt & Bowler 2009): [T | w] is solved at the nodes of a coarse mesh of
// grid columns only (k_letkf in kLetkfWeights mode, unchanged), and this file's kernel interpolates the node pairs bilinearly in
// grid-index space to every column and applies the column's pair to its rows.
//
// k_letkf_interp  one workgroup per column: two waves up to 64 members, four above.  A column is a chain of latencies (launch, node
//                 statistics, node pairs, rows, stores), so what sets the rate is the number of columns in flight and the share of
//                 a wave's time spent on rows: small workgroups, and registers held to three waves per SIMD where that is free.
//   1. Cell.      The column's cell of consecutive nodes on each axis (a column on a node line belongs to the cell below it), its
//                 two fractions and the four corner weights beta.  A corner with beta == 0 is not read: a select, not a product.
//                 If no corner in use is reached by an ob (n_local == 0 in the node statistics) the column's rows are copied bit
//                 for bit and the workgroup is done.
//   2. [T_c | w_c] = sum_n beta_n [T_n | w_n] over the corners in use, in the fixed order (y0,x0) (y0,x1) (y1,x0) (y1,x1), formed
//                 ONCE in LDS (M x (M+1) doubles: 149 KB at 136 members) from node pairs read through L2, two doubles per lane and
//                 load (M (M+1) is even) and four such loads in flight per corner; RTPP turns T_c into (1-alpha) T_c + alpha I there.
//   3. Apply.     A wave takes 16 rows (16 leads of the column) at a time and holds them in registers as the A operand of
//                 v_mfma_f64_16x16x4_f64 (lane (g = lane >> 4, nn = lane & 15) feeds row nn, summation index g of a k-step).  The
//                 summation index of a product is free, so k-steps 2q and 2q + 1 of lane g take members 8q + 2g and 8q + 2g + 1:
//                 the lane loads them as one pair, and the four lanes of a row read 64 contiguous bytes.  The four lanes share the
//                 row's mean and prior spread with two shuffles.  A wave's first 16 rows are on their way while [T_c | w_c] is
//                 formed.  X' [T_c | w_c] runs over the tiles of 16 columns, B from LDS (row 8q + 2g + r of the array), all tiles of the
//                 16 rows kept in registers (C/D layout: column nn, rows g + 4 v); the w column gives xam, RTPS takes the row's
//                 posterior mean and spread from the tiles at hand (§7b's formula), and the rows are stored, 16 lanes to 128
//                 contiguous bytes.  Rows of float32 are widened on load and rounded once at the store.  A wave has read all of a
//                 row before it stores any of it, and no other wave or workgroup touches its rows: post == X is safe.
// KMAX is the number of MFMA k-steps a row may take, 2 ceil(M/8) <= KMAX: the register class of the instantiation.
// Same inputs, same bits: every reduction has a fixed order, there are no atomics.
// This file holds the kernel and its launcher (plain, or per slab group with LetkfGroups); the driver that runs the node solve and
// then this launch is efa_letkf_driver.hip.
#include "efa_driver.h"
#include "efa_device.h"

namespace efa {
namespace {

typedef double interp_v4 __attribute__((ext_vector_type(4)));
typedef double interp_v2 __attribute__((ext_vector_type(2)));
typedef float interp_f2 __attribute__((ext_vector_type(2)));
// pairs at the alignment of their elements (a row of odd M starts on any element; the caller's node pairs on any double)
typedef interp_v2 interp_v2u __attribute__((aligned(8)));
typedef interp_f2 interp_f2u __attribute__((aligned(4)));

__device__ __forceinline__ interp_v2 interp_load2(const double* p) { return *reinterpret_cast<const interp_v2u*>(p); }
__device__ __forceinline__ interp_v2 interp_load2(const float* p) {
  const interp_f2 v = *reinterpret_cast<const interp_f2u*>(p);
  return interp_v2{(double)v.x, (double)v.y};
}

// the cell of index i on an axis of n points with node stride s: its lower node j0, and the fraction of the way to the upper one
// (32-bit arithmetic: the launcher keeps ny nx, hence every index and stride, below 2^31)
__device__ __forceinline__ void interp_axis(unsigned i, unsigned n, unsigned s, unsigned* j0, double* t) {
  if (n <= 1 || i == 0) {
    *j0 = 0;
    *t = 0.0;
    return;
  }
  const unsigned j = (i - 1) / s;  // a point on a node line takes the cell below it
  const unsigned p0 = j * s, p1 = (n - 1 - p0 > s) ? p0 + s : n - 1;
  *j0 = j;
  *t = (double)(i - p0) / (double)(p1 - p0);
}

// waves per SIMD the register allocation aims at: a column is a chain of latencies, so the columns in flight set the rate
// (three is what the 16-step class reaches without scratch; four spills in the 8-step class as well)
constexpr int interp_waves(int KMAX) { return KMAX <= 16 ? 3 : 1; }

// 16 rows of a column into registers: lane (g, nn) takes members 8q + 2g, 8q + 2g + 1 of row `first + nn` as k-steps 2q, 2q + 1;
// exact zeros past M and past the last row
// (leads: the slab of each of the n_lead rows, the SLAB kernel's group list; null: row i is slab i)
template <typename E, int KMAX>
__device__ __forceinline__ void interp_load_rows(const E* in, long first, long n_lead, long ncol, long col, int M, int g, int nn,
                                                 double (&x)[KMAX], const int* leads = nullptr) {
  long l = first + nn;
  const bool rowok = l < n_lead;
  if (leads && rowok) l = leads[l];
  const E* xin = in + (size_t)((rowok ? l : 0) * ncol + col) * M;
#pragma unroll
  for (int q = 0; q < KMAX / 2; ++q) {
    const int j = 8 * q + 2 * g;
    interp_v2 v = interp_v2{0.0, 0.0};
    if (rowok && j + 1 < M) v = interp_load2(xin + j);
    else if (rowok && j < M) v.x = (double)xin[j];
    x[2 * q] = v.x;
    x[2 * q + 1] = v.y;
  }
}

// SLAB: one workgroup per (column, slab group), the group the fastest index; node pairs from Tw[group][node], node
// statistics from [group][node], a wave's 16 rows gathered from the group's slab list.
struct LetkfInterpSlabArgs : LetkfInterpArgs {
  int ngroups;
  const int* grp_off;
  const int* grp_leads;
};
template <bool SLAB>
struct InterpArgsOf { typedef LetkfInterpArgs type; };
template <>
struct InterpArgsOf<true> { typedef LetkfInterpSlabArgs type; };

template <typename E, int KMAX, int NT, bool SLAB = false>
__global__ __launch_bounds__(NT, interp_waves(KMAX)) void k_letkf_interp(const typename InterpArgsOf<SLAB>::type a) {
  extern __shared__ __align__(16) double interp_smem[];
  static_assert(KMAX % 2 == 0, "k-steps come in pairs");
  constexpr int TMAX = (4 * KMAX + 1 + 15) / 16;
  const int M = a.M, Mp = M + 1;
  const int K = 2 * ((M + 7) >> 3), T = (Mp + 15) >> 4;
  const int tid = (int)threadIdx.x, lane = tid & 63, g = lane >> 4, nn = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned bidx = (unsigned)blockIdx.x;
  long nrows = a.n_lead;             // the rows this workgroup maps: the column's, or the group's
  const int* leads = nullptr;        // ... and their slabs
  const double* Tw_g = a.Tw;
  const double* stats_g = a.stats;
  if constexpr (SLAB) {
    const unsigned grp = bidx % (unsigned)a.ngroups;
    bidx = bidx / (unsigned)a.ngroups;
    const int o0 = a.grp_off[grp];
    nrows = a.grp_off[grp + 1] - o0;
    leads = a.grp_leads + o0;
    const size_t nn_ = (size_t)a.mesh.nnodes();
    Tw_g = a.Tw + (size_t)grp * nn_ * (size_t)M * Mp;
    if (a.stats) stats_g = a.stats + 3 * (size_t)grp * nn_;
  }
  const long ncol = a.mesh.ncol(), col = (long)bidx;
  const E* in = static_cast<const E*>(a.Xin);
  E* out = static_cast<E*>(a.Xout);
  double* Tw_s = interp_smem;  // [M][M + 1]

  // ---- 1. the cell (every thread computes the same scalars) --------------------------------------------------------------------
  const unsigned nx = (unsigned)a.mesh.nx, iy = bidx / nx, ix = bidx - iy * nx;
  unsigned jy, jx;
  double ty, tx;
  interp_axis(iy, (unsigned)a.mesh.ny, (unsigned)a.mesh.sy, &jy, &ty);
  interp_axis(ix, nx, (unsigned)a.mesh.sx, &jx, &tx);
  const long nxn = a.mesh.nxn(), n00 = (long)jy * nxn + jx;
  const double beta[4] = {(1.0 - ty) * (1.0 - tx), (1.0 - ty) * tx, ty * (1.0 - tx), ty * tx};
  const long node[4] = {n00, n00 + 1, n00 + nxn, n00 + nxn + 1};
  bool reached = !a.stats;
  if (a.stats) {  // n_local of the corners in use, the four loads in flight together (a corner of weight 0 reads a used one's)
    long used = node[0];
#pragma unroll
    for (int n = 3; n >= 0; --n)
      if (beta[n] != 0.0) used = node[n];
    double nl[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) nl[n] = stats_g[3 * (beta[n] != 0.0 ? node[n] : used)];
#pragma unroll
    for (int n = 0; n < 4; ++n)
      if (nl[n] != 0.0) reached = true;
  }
  if (!reached) {  // (uniform) T_c = I, w_c = 0: the rows keep their bits
    if (in != out)
      for (long li = 0; li < nrows; ++li) {
        long l = li;
        if constexpr (SLAB) l = leads[li];
        const size_t base = (size_t)(l * ncol + col) * M;
        for (int m = tid; m < M; m += NT) out[base + m] = in[base + m];
      }
    return;
  }

  // the first 16 rows of every wave are on their way while [T_c | w_c] is formed
  const long ntiles = (nrows + 15) >> 4;
  double x[KMAX];
  if constexpr (SLAB) interp_load_rows<E, KMAX>(in, 16 * (long)wave, nrows, ncol, col, M, g, nn, x, leads);
  else interp_load_rows<E, KMAX>(in, 16 * (long)wave, a.n_lead, ncol, col, M, g, nn, x);

  // ---- 2. [T_c | w_c] in LDS, two elements per lane and step -----------------------------------------------------------------------
  {
    const size_t pair = (size_t)M * Mp;
    const int npairs = (M * Mp) >> 1;
    const bool rtpp = a.relax_kind == EFA_RELAX_RTPP && a.relax_alpha != 0.0;
#pragma unroll 4
    for (int e = tid; e < npairs; e += NT) {
      interp_v2 acc = interp_v2{0.0, 0.0};
      bool first = true;
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (beta[n] != 0.0) {  // (uniform)
          const interp_v2 v = beta[n] * interp_load2(Tw_g + (size_t)node[n] * pair + 2 * e);
          acc = first ? v : acc + v;
          first = false;
        }
      if (rtpp) {
        const int r0 = (2 * e) / Mp, c0 = 2 * e - r0 * Mp;
        const int r1 = (2 * e + 1) / Mp, c1 = 2 * e + 1 - r1 * Mp;
        if (c0 < M) acc.x = (1.0 - a.relax_alpha) * acc.x + ((r0 == c0) ? a.relax_alpha : 0.0);
        if (c1 < M) acc.y = (1.0 - a.relax_alpha) * acc.y + ((r1 == c1) ? a.relax_alpha : 0.0);
      }
      *reinterpret_cast<interp_v2*>(Tw_s + 2 * e) = acc;
    }
  }
  __syncthreads();

  // ---- 3. apply: 16 rows per wave and step -----------------------------------------------------------------------------------------
  const bool rtps = a.relax_kind == EFA_RELAX_RTPS && a.relax_alpha != 0.0;
  const int tw = M >> 4, cw = M & 15;  // the tile and the lane column of w
#pragma unroll 1
  for (long tile = wave; tile < ntiles; tile += NT / 64) {
    double s = 0.0;
#pragma unroll
    for (int kk = 0; kk < KMAX; ++kk) s += x[kk];
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    const double mean = s / (double)M;
    double q = 0.0;
#pragma unroll
    for (int kk = 0; kk < KMAX; ++kk) {
      const double p = (8 * (kk >> 1) + 2 * g + (kk & 1) < M) ? x[kk] - mean : 0.0;
      x[kk] = p;
      q = fma(p, p, q);
    }
    q += __shfl_xor(q, 16, 64);
    q += __shfl_xor(q, 32, 64);  // the prior spread (sum of squares) of row nn

    // X' [T_c | w_c]: every tile of the 16 rows, the k-steps outermost so that consecutive MFMAs are independent
    interp_v4 acc[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) acc[t] = interp_v4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < KMAX; ++kk) {
      if (kk < K) {  // (uniform)
        const int j = 8 * (kk >> 1) + 2 * g + (kk & 1);
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
          if (t < T) {  // (uniform)
            const int c = 16 * t + nn;
            const double b = (j < M && c <= M) ? Tw_s[j * Mp + c] : 0.0;
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[kk], b, acc[t], 0, 0, 0);
          }
        }
      }
    }

    // to the C/D layout (column nn, rows g + 4 v): x' w from the w column, the row's mean and prior spread from the lane of its row
    interp_v4 wsel = acc[0];
#pragma unroll
    for (int t = 1; t < TMAX; ++t)
      if (t == tw) wsel = acc[t];  // (uniform)
    double xam[4], ssb[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const double xw = __shfl(wsel[v], (lane & 48) | cw, 64);
      xam[v] = __shfl(mean, g + 4 * v, 64) + xw;
      ssb[v] = __shfl(q, g + 4 * v, 64);
    }
    double base[4], sc[4], pm[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      base[v] = xam[v];
      sc[v] = 1.0;
      pm[v] = 0.0;
    }
    if (rtps) {  // (uniform) the posterior perturbations' own mean and spread, as the standalone pass takes them (§7b)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        double sa = 0.0;
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
          if (t < T && 16 * t + nn < M) sa += acc[t][v];
#pragma unroll
        for (int o = 1; o <= 8; o <<= 1) sa += __shfl_xor(sa, o, 64);
        const double m = sa / (double)M;
        double qa = 0.0;
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
          if (t < T && 16 * t + nn < M) {
            const double dv = acc[t][v] - m;
            qa = fma(dv, dv, qa);
          }
#pragma unroll
        for (int o = 1; o <= 8; o <<= 1) qa += __shfl_xor(qa, o, 64);
        if (qa > 0.0) {  // sigma_a == 0: the row stays as it is
          sc[v] = (1.0 - a.relax_alpha) + a.relax_alpha * sqrt(ssb[v] / qa);
          base[v] = xam[v] + m;
          pm[v] = m;
        }
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      long l = tile * 16 + g + 4 * v;
      if (l < nrows) {
        if constexpr (SLAB) l = leads[l];
        E* xo = out + (size_t)(l * ncol + col) * M;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
          const int b = 16 * t + nn;
          if (t < T && b < M) {
            const double val = rtps ? base[v] + sc[v] * (acc[t][v] - pm[v]) : xam[v] + acc[t][v];
            xo[b] = letkf_round<E>(val);
          }
        }
      }
    }
    if (tile + NT / 64 < ntiles) {  // (uniform) the wave's next 16 rows
      if constexpr (SLAB) interp_load_rows<E, KMAX>(in, 16 * (tile + NT / 64), nrows, ncol, col, M, g, nn, x, leads);
      else interp_load_rows<E, KMAX>(in, 16 * (tile + NT / 64), a.n_lead, ncol, col, M, g, nn, x);
    }
  }
}

template <typename E, int KMAX, int NT, bool SLAB>
hipError_t interp_launch_as(const typename InterpArgsOf<SLAB>::type& a, size_t lds, hipStream_t s) {
  auto kern = k_letkf_interp<E, KMAX, NT, SLAB>;
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  long nwg = a.mesh.ncol();
  if constexpr (SLAB) nwg *= a.ngroups;
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(NT), lds, s, a);
  return hipGetLastError();
}

template <typename E, bool SLAB>
hipError_t interp_launch_mode(const typename InterpArgsOf<SLAB>::type& a, hipStream_t s) {
  const size_t lds = letkf_interp_lds_bytes(a.M);
  if (a.M <= 32) return interp_launch_as<E, 8, 128, SLAB>(a, lds, s);
  if (a.M <= 64) return interp_launch_as<E, 16, 128, SLAB>(a, lds, s);
  return interp_launch_as<E, 34, 256, SLAB>(a, lds, s);
}

// the plain launch, or with groups the SLAB one on (a, *grp)
template <typename E>
hipError_t interp_launch(const LetkfInterpArgs& a, const LetkfGroups* grp, hipStream_t s) {
  if (!grp) return interp_launch_mode<E, false>(a, s);
  LetkfInterpSlabArgs sa{};
  static_cast<LetkfInterpArgs&>(sa) = a;
  sa.ngroups = grp->ngroups;
  sa.grp_off = grp->grp_off;
  sa.grp_leads = grp->grp_leads;
  return interp_launch_mode<E, true>(sa, s);
}

}  // namespace

size_t letkf_interp_lds_bytes(int M) { return (size_t)M * (M + 1) * sizeof(double); }

hipError_t launch_letkf_interp(const LetkfInterpArgs& a, const LetkfGroups* grp, Elem elem, hipStream_t s) {
  const LetkfMesh& m = a.mesh;
  if (a.M < 2 || a.M > kLetkfMaxM || letkf_interp_lds_bytes(a.M) > 160 * 1024) return hipErrorInvalidValue;
  if (grp && (grp->ngroups < 1 || !grp->grp_off || !grp->grp_leads)) return hipErrorInvalidValue;
  if (m.ny < 1 || m.nx < 1 || m.sy < 1 || m.sx < 1 || m.ny > 0x7FFFFFF0L / m.nx) return hipErrorInvalidValue;
  if (grp && m.ny * m.nx > 0x7FFFFFF0L / grp->ngroups) return hipErrorInvalidValue;
  if (m.sy > (m.ny > 2 ? m.ny - 1 : 1) || m.sx > (m.nx > 2 ? m.nx - 1 : 1)) return hipErrorInvalidValue;
  if (!a.Xin || !a.Xout || !a.Tw || a.n_lead < 1) return hipErrorInvalidValue;
  return elem == Elem::f32 ? interp_launch<float>(a, grp, s) : interp_launch<double>(a, grp, s);
}

}  // namespace efa
