// Unlocalised collapse of the serial EnSRF loop into one pass over the state.
//
// With loc in (None, False) every row of the reference's update
//   kcov_i = Xbp_i . ye_k/(Nens-1); xam_i += kcov_i/kdenom*innov;
//   Xap_i  = Xbp_i - beta*kcov_i/kdenom * ye_k          (ensrf.py:95-141)
// is the same linear map of that row for all i, so after P observations
//   Xap = Xbp * T        (T: M x M)      xam = xbm + Xbp * w    (w: M)
// where (T, w) are what the loop does to the rows of the identity matrix
// (carried through Phase A as M extra rows of the obs block).  This kernel
// applies [T | w] to every state row: one HBM read and one write of the state
// for the whole assimilation cycle.
//
// It is a (rows x M) . (M x (M+1)) float64 contraction, done on the matrix
// cores with v_mfma_f64_16x16x4_f64:
//   - a wave owns a tile of 16 consecutive rows (contiguous in memory);
//   - lane l = (g = l>>4, n = l&15) loads members {8u+2g, 8u+2g+1} of row n with
//     16-byte global loads (a quad of lane-groups covers 64 contiguous bytes);
//     the K order of the contraction is permuted to match, so the A operand
//     goes HBM -> VGPR -> MFMA with no LDS staging;
//   - [T | w] lives in LDS (once per workgroup), pre-arranged so each MFMA's B
//     operand is one conflict-free ds_read_b64 per lane;
//   - the next tile's rows are prefetched while the current tile is multiplied.
#include "efa_device.h"
#include "efa_internal.h"

namespace efa {
namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));

#ifndef EFA_T_WAVES
#define EFA_T_WAVES 8
#endif
#ifndef EFA_T_PREFETCH
#define EFA_T_PREFETCH 1
#endif
constexpr int kThreadsT = 64 * EFA_T_WAVES;  // waves per workgroup, sharing its LDS copy of [T|w]
constexpr bool kPrefetchT = EFA_T_PREFETCH != 0;

// Column tiling of the product.  Perturbation form (!FUSED): M member columns plus the column of w (the mean
// increment): NU/2 + 1 tiles of 16.  Member form (FUSED: prior members in, posterior members out) needs no
// separate w column -- posterior_j = mean + sum_k Xp_k (T_kj + w_k), so w is folded into the LDS image of T --
// and when the last 16-column tile would hold at most four members (M % 16 in 1..4, i.e. HALF with NU odd) those
// columns are done by ONE v_mfma_f64_4x4x4_4b_f64 per K step (17 cycles instead of 64) over the same A operand:
// its four 4 x 4 x 4 blocks are the tile's four row groups, A[blk][i][k] sits in lane 16 k + 4 blk + i = 16 k + row
// exactly as in the 16 x 16 x 4 instruction, B[blk][k][j] in lane 16 k + 4 blk + j, D[blk][i][j] in lane
// 16 i + 4 blk + j (tools/mfma44_layout_probe.hip).  M = 100: 6 x 64 + 17 cycles per K step instead of 7 x 64.
template <int NU, bool FUSED, bool HALF>
struct TShape {
  static constexpr bool NARROW = FUSED && HALF && (NU & 1);
  static constexpr int NT = !FUSED ? NU / 2 + 1 : (NARROW ? NU / 2 : (NU + 1) / 2);
  static constexpr int NTA = NT > 0 ? NT : 1;    // array extent (NT = 0: M <= 4 in member form)
  static constexpr int kSteps = 2 * NU;          // K steps of 4 members
  static constexpr size_t wide_doubles = (size_t)kSteps * NT * 64;
  static constexpr size_t lds_doubles = wide_doubles + (NARROW ? (size_t)kSteps * 64 : 0);
};

// Loads of one tile are branch-free (clamped addresses; the partial last chunk is zeroed
// by a select at the point of use) and the prefetch is unconditional, so the compiler can
// keep the next tile's 16-byte loads in flight behind counted vmcnt waits while the current
// tile is multiplied.  With conditional loads it falls back to vmcnt(0) and the overlap is lost.
// HALF: the last chunk holds at most four members (M % 8 in 1..4).  Lane-group g then loads member
// 8(NU-1)+g alone, so the chunk is ONE K step of the matrix core instead of two half-empty ones
// (M = 100: 25 steps instead of 26).
// AL: rows are 16-byte aligned (M even and an aligned base): 16-byte loads.  Otherwise (odd M) the two
// members of a pair are loaded separately -- half the load width, the price of an odd ensemble size only.
// E: the element type of the rows in memory.  double as above; float (efa_transform_f32.hip) for a state stored as float32: the
// same lanes take the same members, an AL pair with one 8-byte load (M even and an 8-byte aligned base), and every value is
// widened -- exactly -- as it arrives, so everything downstream is the float64 arithmetic unchanged.
template <typename E>
struct Pair;
template <>
struct Pair<double> { typedef double2 type; };
template <>
struct Pair<float> { typedef float2 type; };
template <int NU, bool HALF, bool AL, typename E = double>
__device__ __forceinline__ void load_tile(const double* __restrict__ X, long row_clamped, int M, int g,
                                          double (&a)[2 * NU]) {
  const E* p = reinterpret_cast<const E*>(X) + (size_t)row_clamped * M;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    if (HALF && u == NU - 1) {
      const int m = 8 * u + g;
      a[2 * u] = p[(m < M) ? m : M - 1];
      a[2 * u + 1] = 0.0;
    } else if (AL) {
      int m0 = 8 * u + 2 * g;
      if (u == NU - 1) m0 = (m0 < M) ? m0 : M - 2;  // last chunk may be partial: clamp the address
      const typename Pair<E>::type v = *reinterpret_cast<const typename Pair<E>::type*>(p + m0);
      a[2 * u] = v.x;
      a[2 * u + 1] = v.y;
    } else {
      const int m0 = 8 * u + 2 * g;
      a[2 * u] = p[(m0 < M) ? m0 : M - 1];          // clamped addresses; invalid slots are zeroed at the point of use
      a[2 * u + 1] = p[(m0 + 1 < M) ? m0 + 1 : M - 1];
    }
  }
}

template <int NU, bool FUSED, bool HALF, bool AL, typename E = double>
__global__ __launch_bounds__(kThreadsT) void k_transform(const TransformArgs p) {
  using Sh = TShape<NU, FUSED, HALF>;
  E* const Xout = reinterpret_cast<E*>(p.Xout);  // E float: each posterior value is rounded once, at its store
  constexpr int NT = Sh::NT;
  constexpr bool NARROW = Sh::NARROW;
  extern __shared__ __align__(16) double Bs[];  // [(u*2+h)*NT + t][64], then the narrow tile's [(u*2+h)][64]
  const int M = p.M;
  const int tid = threadIdx.x;

  // Stage [T | w] (member form: T + w 1^T) in MFMA-B order: Bs[step s=(u,h)][t][lane (g,n)] = Text[8u+2g+h][16t+n]
  for (int i = tid; i < (int)Sh::lds_doubles; i += kThreadsT) {
    const int l = i & 63;
    const int g = l >> 4, n = l & 15;
    int s, j;
    if (i < (int)Sh::wide_doubles) {
      const int st = i >> 6;
      s = st / Sh::NTA;
      j = 16 * (st % Sh::NTA) + n;
    } else {  // narrow tile: B[blk][k = g][j = l & 3] for every block
      s = (i - (int)Sh::wide_doubles) >> 6;
      j = 16 * NT + (l & 3);
    }
    const int u = s >> 1, h = s & 1;
    const int m = (HALF && u == NU - 1) ? (h == 0 ? 8 * u + g : M) : 8 * u + 2 * g + h;  // (row M: never used, stays 0)
    double v = 0.0;
    if (m < M) {
      if (j < M) v = FUSED ? p.T[(size_t)m * M + j] + p.w[m] : p.T[(size_t)m * M + j];
      else if (j == M && !FUSED) v = p.w[m];
    }
    Bs[i] = v;
  }
  __syncthreads();

  const int lane = tid & 63;
  const int g = lane >> 4, n = lane & 15;
#ifdef EFA_T_CLOCKSTAMP  /* tools/transform_clock.py: shader clock over the kernel (non-fused launches only) */
  const unsigned long long tm0 = __builtin_amdgcn_s_memtime(), tr0 = __builtin_amdgcn_s_memrealtime();
#endif
  const long ntiles = (p.nrows + 15) / 16;
  const long wave = (long)blockIdx.x * (kThreadsT / 64) + (tid >> 6);
  const long nwaves = (long)gridDim.x * (kThreadsT / 64);
  const int tM = M >> 4, nM = M & 15;  // tile / lane column holding the mean increment
  const long last_row = p.nrows - 1;
  // this lane's two slots of the last chunk are real members?  (the second only matters for an odd M)
  const bool last_ok = (HALF ? (8 * (NU - 1) + g) : (8 * (NU - 1) + 2 * g)) < M;
  const bool last_ok1 = !HALF && (8 * (NU - 1) + 2 * g + 1) < M;

  double a[2 * NU], an[2 * NU];
  long tile = wave;
  if (tile < ntiles) {
    const long r = tile * 16 + n;
    load_tile<NU, HALF, AL, E>(p.Xin, r < last_row ? r : last_row, M, g, a);
  }
  if (kPrefetchT) {  // the first tile has arrived before the loop is entered: its header then needs no vmcnt wait, which on
#pragma unroll      // the back edge would also wait for the previous tile's stores
    for (int c = 0; c < 2 * NU; ++c) asm volatile("" : "+v"(a[c]));
  }

  while (tile < ntiles) {
    const long next = tile + nwaves;
    const long r0 = tile * 16;
    double xm4[4] = {0.0, 0.0, 0.0, 0.0};  // prior means of rows 4v+g (perturbation form)
    if (!FUSED) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long rr = r0 + 4 * v + g;
        xm4[v] = p.xin[rr < last_row ? rr : last_row];
      }
    }
    if (kPrefetchT) {  // prefetch (the last iteration harmlessly re-reads its own tile)
      const long r = (next < ntiles ? next : tile) * 16 + n;
      load_tile<NU, HALF, AL, E>(p.Xin, r < last_row ? r : last_row, M, g, an);
    }
    if (!last_ok) a[2 * NU - 2] = 0.0;
    if (!last_ok1) a[2 * NU - 1] = 0.0;

    double rmean = 0.0;  // prior mean of row n (FUSED only)
    if (FUSED) {
      double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < 2 * NU; ++c) s4[c & 3] += a[c];
      double s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      rmean = s / (double)M;
#pragma unroll
      for (int c = 0; c < 2 * NU - 2; ++c) a[c] -= rmean;
      a[2 * NU - 2] = last_ok ? a[2 * NU - 2] - rmean : 0.0;
      a[2 * NU - 1] = last_ok1 ? a[2 * NU - 1] - rmean : 0.0;
    }

    v4f64 acc[Sh::NTA];
    double accn = 0.0;  // narrow tile: D[row 4 ((lane >> 2) & 3) + (lane >> 4)][col 16 NT + (lane & 3)]
#pragma unroll
    for (int t = 0; t < Sh::NTA; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < (HALF ? 2 * NU - 1 : 2 * NU); ++s) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const double b = Bs[((size_t)s * NT + t) * 64 + lane];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b, acc[t], 0, 0, 0);
      }
      if (NARROW) accn = __builtin_amdgcn_mfma_f64_4x4x4f64(a[s], Bs[Sh::wide_doubles + (size_t)s * 64 + lane], accn, 0, 0, 0);
      // keep the scheduler from hoisting all 2*NU*NT LDS reads (register blow-up)
      __builtin_amdgcn_sched_barrier(0);
    }

    // The next tile's rows are taken over HERE, before this tile's stores are issued: vmcnt counts loads and stores
    // in one queue on this architecture, so a wait for the prefetched loads placed AFTER the stores (the top of the
    // next iteration) is also a wait for the stores.  (Measured: the launch time is the same either way -- the stores
    // drain well within a tile's MFMA phase -- but this is the order that does not depend on it.)
    if (kPrefetchT) {
#pragma unroll
      for (int c = 0; c < 2 * NU; ++c) a[c] = an[c];
#pragma unroll
      for (int c = 0; c < 2 * NU; ++c) asm volatile("" : "+v"(a[c]));  // the wait for the loads belongs here
    }
    // acc[t][v] = D[row 4v+g][col 16t+n]  (layout probed on gfx950: tools/mfma_probe.hip)
    double base[4];  // posterior mean of rows 4v+g: prior mean + column M of the product
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (FUSED) {
        base[v] = __shfl(rmean, 4 * v + g, 64);  // w is folded into the image of T
      } else {
        double dm = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (t == tM) dm = __shfl(acc[t][v], (lane & 48) | nM, 64);
        base[v] = xm4[v] + dm;
      }
    }
    const int nrow = 4 * ((lane >> 2) & 3) + g;  // the narrow tile's row and column of this lane
    const int ncol = 16 * NT + (lane & 3);
    const double nval = NARROW ? __shfl(rmean, nrow, 64) + accn : 0.0;
#ifdef EFA_T_NOSTORE_PROBE  /* make nostore (tools/f32_state_cost.py --unchecked): the kernel with its stores never executed (p.w is never
                               null), to tell the stores' share of the launch time for either element type */
    if (p.w == nullptr) {
#endif
    if (r0 + 16 <= p.nrows) {  // full tile: no row checks (wave-uniform)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int col = 16 * t + n;
        if (col < M) {
#pragma unroll
          for (int v = 0; v < 4; ++v)
            Xout[(size_t)(r0 + 4 * v + g) * M + col] = (E)(FUSED ? (base[v] + acc[t][v]) : acc[t][v]);
        }
      }
      if (NARROW && ncol < M) Xout[(size_t)(r0 + nrow) * M + ncol] = (E)nval;
      if (!FUSED && n == 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v) p.xout[r0 + 4 * v + g] = base[v];
      }
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int col = 16 * t + n;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const long row = r0 + 4 * v + g;
          if (col < M && row < p.nrows)
            Xout[(size_t)row * M + col] = (E)(FUSED ? (base[v] + acc[t][v]) : acc[t][v]);
        }
      }
      if (NARROW && ncol < M && r0 + nrow < p.nrows) Xout[(size_t)(r0 + nrow) * M + ncol] = (E)nval;
      if (!FUSED && n == 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const long row = r0 + 4 * v + g;
          if (row < p.nrows) p.xout[row] = base[v];
        }
      }
    }
#ifdef EFA_T_NOSTORE_PROBE
    }
#endif

    if (!kPrefetchT && next < ntiles) {
      const long r = next * 16 + n;
      load_tile<NU, HALF, AL, E>(p.Xin, r < last_row ? r : last_row, M, g, a);
    }
    tile = next;
  }
#ifdef EFA_T_CLOCKSTAMP
  if (!FUSED && blockIdx.x == 0 && tid == 0) {
    p.xout[0] = (double)(__builtin_amdgcn_s_memtime() - tm0);
    p.xout[1] = (double)(__builtin_amdgcn_s_memrealtime() - tr0);
  }
#endif
}

template <int NU, bool FUSED, bool HALF, bool AL, typename E = double>
hipError_t transform_launch(const TransformArgs& a, hipStream_t s) {
  using Sh = TShape<NU, FUSED, HALF>;
  const size_t lds = (Sh::lds_doubles ? Sh::lds_doubles : 64) * sizeof(double);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_transform<NU, FUSED, HALF, AL, E>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const long ntiles = (a.nrows + 15) / 16;
  const int per_cu = (lds <= 80 * 1024) ? 2 : 1;
  long grid = (ntiles + EFA_T_WAVES - 1) / EFA_T_WAVES;
  if (grid > 256L * per_cu) grid = 256L * per_cu;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((k_transform<NU, FUSED, HALF, AL, E>), dim3((unsigned)grid), dim3(kThreadsT), lds, s, a);
  return hipGetLastError();
}

// the pair loads need M even and a base aligned to a pair of elements
template <typename E>
inline bool pair_aligned(const TransformArgs& a) {
  return (a.M % 2 == 0) && (reinterpret_cast<uintptr_t>(a.Xin) & (2 * sizeof(E) - 1)) == 0;
}

#ifndef EFA_TRANSFORM_F32
template <int NU>
hipError_t transform_nu(const TransformArgs& a, hipStream_t s) {
  const int rem = a.M % 8;
  const bool half = rem != 0 && rem <= 4;
  const bool al = pair_aligned<double>(a);
  if (al) {
    if (half) return a.fused_members ? transform_launch<NU, true, true, true>(a, s) : transform_launch<NU, false, true, true>(a, s);
    return a.fused_members ? transform_launch<NU, true, false, true>(a, s) : transform_launch<NU, false, false, true>(a, s);
  }
  if (half) return a.fused_members ? transform_launch<NU, true, true, false>(a, s) : transform_launch<NU, false, true, false>(a, s);
  return a.fused_members ? transform_launch<NU, true, false, false>(a, s) : transform_launch<NU, false, false, false>(a, s);
}
#else
// member form only: a float32 state has no perturbation form
template <int NU>
hipError_t transform_nu_f32(const TransformArgs& a, hipStream_t s) {
  const int rem = a.M % 8;
  const bool half = rem != 0 && rem <= 4;
  if (pair_aligned<float>(a)) return half ? transform_launch<NU, true, true, true, float>(a, s) : transform_launch<NU, true, false, true, float>(a, s);
  return half ? transform_launch<NU, true, true, false, float>(a, s) : transform_launch<NU, true, false, false, float>(a, s);
}
#endif


// ---- RTPS fused into the member-form transform (M <= 136) -------------------------------------------------
// k_transform's member form with the relaxation to prior spread (Whitaker & Hamill 2012) applied before the stores:
//   post_ij <- mean_j(post_i) + (post_ij - mean_j(post_i)) ((1 - alpha) + alpha sigma_b / sigma_a)
// Once the row mean is removed, a[] holds the prior perturbations of row n (lane (g, n): members {8u+2g, 8u+2g+1}), so
// sum_m b^2 reduces over g exactly as rmean does.  The posterior member columns of rows 4v+g are acc[t][v] (w folded in)
// plus, at M % 16 in 1..4, the narrow tile's accn: their row mean and sum of squared deviations reduce over the 16 lanes n
// of a row group (the narrow tile's over its 4 columns first).  The scale is applied in registers: no extra HBM traffic.
// Rows with sigma_a == 0 are stored as k_transform stores them.  A kernel of its own -- not a flag of k_transform -- so
// the shipped transform's code stays as it is.
template <int NU, bool HALF, bool AL, typename E = double>
__global__ __launch_bounds__(kThreadsT) void k_transform_rtps(const TransformArgs p, const double alpha) {
  using Sh = TShape<NU, true, HALF>;
  E* const Xout = reinterpret_cast<E*>(p.Xout);
  constexpr int NT = Sh::NT;
  constexpr bool NARROW = Sh::NARROW;
  extern __shared__ __align__(16) double Bs[];  // as k_transform (member form: T + w 1^T)
  const int M = p.M;
  const int tid = threadIdx.x;
  for (int i = tid; i < (int)Sh::lds_doubles; i += kThreadsT) {
    const int l = i & 63;
    const int g = l >> 4, n = l & 15;
    int s, j;
    if (i < (int)Sh::wide_doubles) {
      const int st = i >> 6;
      s = st / Sh::NTA;
      j = 16 * (st % Sh::NTA) + n;
    } else {
      s = (i - (int)Sh::wide_doubles) >> 6;
      j = 16 * NT + (l & 3);
    }
    const int u = s >> 1, h = s & 1;
    const int m = (HALF && u == NU - 1) ? (h == 0 ? 8 * u + g : M) : 8 * u + 2 * g + h;
    double v = 0.0;
    if (m < M && j < M) v = p.T[(size_t)m * M + j] + p.w[m];
    Bs[i] = v;
  }
  __syncthreads();

  const int lane = tid & 63;
  const int g = lane >> 4, n = lane & 15;
  const long ntiles = (p.nrows + 15) / 16;
  const long wave = (long)blockIdx.x * (kThreadsT / 64) + (tid >> 6);
  const long nwaves = (long)gridDim.x * (kThreadsT / 64);
  const long last_row = p.nrows - 1;
  const bool last_ok = (HALF ? (8 * (NU - 1) + g) : (8 * (NU - 1) + 2 * g)) < M;
  const bool last_ok1 = !HALF && (8 * (NU - 1) + 2 * g + 1) < M;
  const int nv = (lane >> 2) & 3;            // the narrow tile: this lane's row is 4 nv + g ...
  const int nrow = 4 * nv + g;
  const int ncol = 16 * NT + (lane & 3);     // ... and its column

  double a[2 * NU], an[2 * NU];
  long tile = wave;
  if (tile < ntiles) {
    const long r = tile * 16 + n;
    load_tile<NU, HALF, AL, E>(p.Xin, r < last_row ? r : last_row, M, g, a);
  }
  if (kPrefetchT) {
#pragma unroll
    for (int c = 0; c < 2 * NU; ++c) asm volatile("" : "+v"(a[c]));
  }

  while (tile < ntiles) {
    const long next = tile + nwaves;
    const long r0 = tile * 16;
    if (kPrefetchT) {
      const long r = (next < ntiles ? next : tile) * 16 + n;
      load_tile<NU, HALF, AL, E>(p.Xin, r < last_row ? r : last_row, M, g, an);
    }
    if (!last_ok) a[2 * NU - 2] = 0.0;
    if (!last_ok1) a[2 * NU - 1] = 0.0;

    double rmean, sb;  // prior mean of row n and sum of its squared perturbations
    {
      double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < 2 * NU; ++c) s4[c & 3] += a[c];
      double s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      rmean = s / (double)M;
#pragma unroll
      for (int c = 0; c < 2 * NU - 2; ++c) a[c] -= rmean;
      a[2 * NU - 2] = last_ok ? a[2 * NU - 2] - rmean : 0.0;
      a[2 * NU - 1] = last_ok1 ? a[2 * NU - 1] - rmean : 0.0;
      double q4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < 2 * NU; ++c) q4[c & 3] = fma(a[c], a[c], q4[c & 3]);
      sb = (q4[0] + q4[1]) + (q4[2] + q4[3]);
      sb += __shfl_xor(sb, 16, 64);
      sb += __shfl_xor(sb, 32, 64);
    }

    v4f64 acc[Sh::NTA];
    double accn = 0.0;
#pragma unroll
    for (int t = 0; t < Sh::NTA; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < (HALF ? 2 * NU - 1 : 2 * NU); ++s) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const double b = Bs[((size_t)s * NT + t) * 64 + lane];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b, acc[t], 0, 0, 0);
      }
      if (NARROW) accn = __builtin_amdgcn_mfma_f64_4x4x4f64(a[s], Bs[Sh::wide_doubles + (size_t)s * 64 + lane], accn, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (kPrefetchT) {
#pragma unroll
      for (int c = 0; c < 2 * NU; ++c) a[c] = an[c];
#pragma unroll
      for (int c = 0; c < 2 * NU; ++c) asm volatile("" : "+v"(a[c]));
    }

    // posterior row mean (of the product part) and sum of squared deviations of rows 4v+g
    const bool nok = NARROW && ncol < M;
    double nsum = nok ? accn : 0.0;
    if (NARROW) {
      nsum += __shfl_xor(nsum, 1, 64);
      nsum += __shfl_xor(nsum, 2, 64);
    }
    double mv[4], base[4], sc[4];  // a row with sigma_a == 0 gets mv 0, sc 1: (base + 0) + 1 (acc - 0) == base + acc exactly
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      double rs = 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (16 * t + n < M) rs += acc[t][v];
      rs += __shfl_xor(rs, 1, 64);
      rs += __shfl_xor(rs, 2, 64);
      rs += __shfl_xor(rs, 4, 64);
      rs += __shfl_xor(rs, 8, 64);
      if (NARROW) rs += __shfl(nsum, (lane & 48) | (4 * v), 64);
      mv[v] = rs / (double)M;
    }
    double ndev = 0.0;
    if (NARROW) {
      const double mn = nv == 0 ? mv[0] : nv == 1 ? mv[1] : nv == 2 ? mv[2] : mv[3];
      const double d = nok ? accn - mn : 0.0;
      ndev = d * d;
      ndev += __shfl_xor(ndev, 1, 64);
      ndev += __shfl_xor(ndev, 2, 64);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      double q = 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const double d = (16 * t + n < M) ? acc[t][v] - mv[v] : 0.0;
        q = fma(d, d, q);
      }
      q += __shfl_xor(q, 1, 64);
      q += __shfl_xor(q, 2, 64);
      q += __shfl_xor(q, 4, 64);
      q += __shfl_xor(q, 8, 64);
      if (NARROW) q += __shfl(ndev, (lane & 48) | (4 * v), 64);
      const double sbv = __shfl(sb, 4 * v + g, 64);
      const bool keep = !(q > 0.0);
      sc[v] = keep ? 1.0 : (1.0 - alpha) + alpha * sqrt(sbv / q);
      if (keep) mv[v] = 0.0;
      base[v] = __shfl(rmean, 4 * v + g, 64) + mv[v];
    }
    double nval = 0.0;
    if (NARROW) {
      const double nb = nv == 0 ? base[0] : nv == 1 ? base[1] : nv == 2 ? base[2] : base[3];
      const double mn = nv == 0 ? mv[0] : nv == 1 ? mv[1] : nv == 2 ? mv[2] : mv[3];
      const double sn = nv == 0 ? sc[0] : nv == 1 ? sc[1] : nv == 2 ? sc[2] : sc[3];
      nval = nb + sn * (accn - mn);
    }
    if (r0 + 16 <= p.nrows) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int col = 16 * t + n;
        if (col < M) {
#pragma unroll
          for (int v = 0; v < 4; ++v)
            Xout[(size_t)(r0 + 4 * v + g) * M + col] = (E)(base[v] + sc[v] * (acc[t][v] - mv[v]));
        }
      }
      if (nok) Xout[(size_t)(r0 + nrow) * M + ncol] = (E)nval;
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int col = 16 * t + n;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const long row = r0 + 4 * v + g;
          if (col < M && row < p.nrows)
            Xout[(size_t)row * M + col] = (E)(base[v] + sc[v] * (acc[t][v] - mv[v]));
        }
      }
      if (nok && r0 + nrow < p.nrows) Xout[(size_t)(r0 + nrow) * M + ncol] = (E)nval;
    }

    if (!kPrefetchT && next < ntiles) {
      const long r = next * 16 + n;
      load_tile<NU, HALF, AL, E>(p.Xin, r < last_row ? r : last_row, M, g, a);
    }
    tile = next;
  }
}

template <int NU, bool HALF, bool AL, typename E = double>
hipError_t transform_rtps_launch(const TransformArgs& a, double alpha, hipStream_t s) {
  using Sh = TShape<NU, true, HALF>;
  const size_t lds = (Sh::lds_doubles ? Sh::lds_doubles : 64) * sizeof(double);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_transform_rtps<NU, HALF, AL, E>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const long ntiles = (a.nrows + 15) / 16;
  const int per_cu = (lds <= 80 * 1024) ? 2 : 1;
  long grid = (ntiles + EFA_T_WAVES - 1) / EFA_T_WAVES;
  if (grid > 256L * per_cu) grid = 256L * per_cu;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((k_transform_rtps<NU, HALF, AL, E>), dim3((unsigned)grid), dim3(kThreadsT), lds, s, a, alpha);
  return hipGetLastError();
}

template <int NU, typename E = double>
hipError_t transform_rtps_nu(const TransformArgs& a, double alpha, hipStream_t s) {
  const int rem = a.M % 8;
  const bool half = rem != 0 && rem <= 4;
  if (pair_aligned<E>(a)) return half ? transform_rtps_launch<NU, true, true, E>(a, alpha, s) : transform_rtps_launch<NU, false, true, E>(a, alpha, s);
  return half ? transform_rtps_launch<NU, true, false, E>(a, alpha, s) : transform_rtps_launch<NU, false, false, E>(a, alpha, s);
}

// ---- ensembles of 137 .. 256 members ----------------------------------------------------------------------
// The LDS image of [T | w] no longer fits one CU (M^2 x 8 B > 160 KB), so the product is cut into column groups of
// kWideTiles 16-wide tiles: blockIdx.y takes one group, stages only that part of the image and re-reads the
// rows (2 .. 5 reads of the state instead of 1; still one write, and still ONE pass where the sweep path would
// make one read+write pass per 64 observations).  Same operand layouts as k_transform; no prefetch (the A
// operand of 256 members is 128 registers), no narrow last tile.
constexpr int kWideTiles = 4;
template <int NU, bool FUSED, bool AL, typename E = double>
__global__ __launch_bounds__(kThreadsT) void k_transform_wide(const TransformArgs p) {
  constexpr int NTG = kWideTiles;
  E* const Xout = reinterpret_cast<E*>(p.Xout);
  constexpr int kSteps = 2 * NU;
  extern __shared__ __align__(16) double Bs[];  // [(u*2+h)*NTG + t][64] for this group's tiles
  const int M = p.M;
  const int tid = threadIdx.x;
  const int t0 = (int)blockIdx.y * NTG;         // first 16-wide tile of this group
  for (int i = tid; i < kSteps * NTG * 64; i += kThreadsT) {
    const int l = i & 63, st = i >> 6;
    const int t = st % NTG, s = st / NTG;
    const int u = s >> 1, h = s & 1;
    const int g = l >> 4, n = l & 15;
    const int m = 8 * u + 2 * g + h;
    const int j = 16 * (t0 + t) + n;
    double v = 0.0;
    if (m < M) {
      if (j < M) v = FUSED ? p.T[(size_t)m * M + j] + p.w[m] : p.T[(size_t)m * M + j];
      else if (j == M && !FUSED) v = p.w[m];
    }
    Bs[i] = v;
  }
  __syncthreads();

  const int lane = tid & 63;
  const int g = lane >> 4, n = lane & 15;
  const long ntiles = (p.nrows + 15) / 16;
  const long nwaves = (long)gridDim.x * (kThreadsT / 64);
  const int tM = M >> 4, nM = M & 15;  // tile / lane column holding the mean increment (perturbation form)
  const long last_row = p.nrows - 1;
  for (long tile = (long)blockIdx.x * (kThreadsT / 64) + (tid >> 6); tile < ntiles; tile += nwaves) {
    const long r0 = tile * 16;
    const long r = r0 + n;
    double a[2 * NU];
    load_tile<NU, false, AL, E>(p.Xin, r < last_row ? r : last_row, M, g, a);
#pragma unroll
    for (int c = 0; c < 2 * NU; ++c) {  // slots beyond M (only in the last chunk) are zero
      const int m = 8 * (c >> 1) + 2 * g + (c & 1);
      if (m >= M) a[c] = 0.0;
    }
    double rmean = 0.0;
    if (FUSED) {
      double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < 2 * NU; ++c) s4[c & 3] += a[c];
      double sm = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      sm += __shfl_xor(sm, 16, 64);
      sm += __shfl_xor(sm, 32, 64);
      rmean = sm / (double)M;
#pragma unroll
      for (int c = 0; c < 2 * NU; ++c) {
        const int m = 8 * (c >> 1) + 2 * g + (c & 1);
        a[c] = (m < M) ? a[c] - rmean : 0.0;
      }
    }
    v4f64 acc[NTG];
#pragma unroll
    for (int t = 0; t < NTG; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
#pragma unroll
      for (int t = 0; t < NTG; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], Bs[((size_t)s * NTG + t) * 64 + lane], acc[t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    double base[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const long rr = r0 + 4 * v + g;
      if (FUSED) {
        base[v] = __shfl(rmean, 4 * v + g, 64);
      } else {
        double dm = 0.0;
#pragma unroll
        for (int t = 0; t < NTG; ++t)
          if (t0 + t == tM) dm = __shfl(acc[t][v], (lane & 48) | nM, 64);
        base[v] = p.xin[rr < last_row ? rr : last_row] + dm;
      }
    }
#pragma unroll
    for (int t = 0; t < NTG; ++t) {
      const int col = 16 * (t0 + t) + n;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long row = r0 + 4 * v + g;
        if (col < M && row < p.nrows) Xout[(size_t)row * M + col] = (E)(FUSED ? (base[v] + acc[t][v]) : acc[t][v]);
      }
    }
    if (!FUSED && n == 0 && tM >= t0 && tM < t0 + NTG) {  // the group that holds column M writes the means
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const long row = r0 + 4 * v + g;
        if (row < p.nrows) p.xout[row] = base[v];
      }
    }
  }
}

template <int NU, typename E = double>
hipError_t transform_wide_nu(const TransformArgs& a, hipStream_t s) {
  const size_t lds = (size_t)2 * NU * kWideTiles * 64 * sizeof(double);
  const bool al = pair_aligned<E>(a);
  const int ncols = a.fused_members ? a.M : a.M + 1;
  const int groups = ((ncols + 15) / 16 + kWideTiles - 1) / kWideTiles;
  const long ntiles = (a.nrows + 15) / 16;
  long gx = (ntiles + EFA_T_WAVES - 1) / EFA_T_WAVES;
  if (gx > 256) gx = 256;
  if (gx < 1) gx = 1;
  const dim3 grid((unsigned)gx, (unsigned)groups);
#define EFA_WIDE_LAUNCH(F, A)                                                                                       \
  do {                                                                                                              \
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_transform_wide<NU, F, A, E>),                  \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                       \
    if (e != hipSuccess) return e;                                                                                  \
    hipLaunchKernelGGL((k_transform_wide<NU, F, A, E>), grid, dim3(kThreadsT), lds, s, a);                              \
  } while (0)
  if (a.fused_members) {
    if (al) EFA_WIDE_LAUNCH(true, true);
    else EFA_WIDE_LAUNCH(true, false);
  } else if constexpr (sizeof(E) == sizeof(double)) {
    if (al) EFA_WIDE_LAUNCH(false, true);
    else EFA_WIDE_LAUNCH(false, false);
  } else {
    return hipErrorInvalidValue;
  }
#undef EFA_WIDE_LAUNCH
  return hipGetLastError();
}

}  // namespace

// the float32 kernels' dispatch, compiled in efa_transform_f32.hip
hipError_t transform_rows_f32(const TransformArgs& a, hipStream_t s);
hipError_t transform_rtps_rows_f32(const TransformArgs& a, double alpha, hipStream_t s);

#ifndef EFA_TRANSFORM_F32
// one launch with the whole [T | w] image in LDS up to M = 136; column groups above (k_transform_wide) up to 256
bool transform_supported(int M) { return M >= 2 && M <= 256; }

bool transform_rtps_supported(int M) { return M >= 2 && M <= 136; }

// what a launch asks of its rows: float64 rows 8-byte aligned; float32 rows 4-byte aligned and in member form (a float32 state
// has no perturbation form)
static bool rows_ok(const TransformArgs& a, Elem elem) {
  const uintptr_t in = reinterpret_cast<uintptr_t>(a.Xin), out = reinterpret_cast<uintptr_t>(a.Xout);
  return elem == Elem::f32 ? (a.fused_members && ((in | out) & 3u) == 0) : (in & 7u) == 0;
}

// The launchers are where a.Xin / a.Xout get their element type: elem picks the kernels that read them as float or as double rows.
// T, w and every number computed are float64 either way.  (RTPS: member form only, Xin prior members, Xout posterior members.)
hipError_t launch_transform_rtps(const TransformArgs& a, double alpha, Elem elem, hipStream_t s) {
  if (!transform_rtps_supported(a.M) || !a.fused_members || !rows_ok(a, elem)) return hipErrorInvalidValue;
  if (a.nrows <= 0) return hipSuccess;
  if (elem == Elem::f32) return transform_rtps_rows_f32(a, alpha, s);
  return dispatch_width((a.M + 7) / 8, WidthRange<1, 17>{}, [&](auto nu) { return transform_rtps_nu<nu>(a, alpha, s); });
}

hipError_t launch_transform(const TransformArgs& a, Elem elem, hipStream_t s) {
  if (!transform_supported(a.M) || !rows_ok(a, elem)) return hipErrorInvalidValue;
  if (a.nrows <= 0) return hipSuccess;
  if (elem == Elem::f32) return transform_rows_f32(a, s);
  const int nu = (a.M + 7) / 8;
  if (nu <= 17) return dispatch_width(nu, WidthRange<1, 17>{}, [&](auto n) { return transform_nu<n>(a, s); });
  return dispatch_width(nu, WidthRange<18, 32>{}, [&](auto n) { return transform_wide_nu<n>(a, s); });
}

#else
// ---- the same kernels on rows stored as float32 (efa_transform_f32.hip), behind the checks of the launchers -------
hipError_t transform_rtps_rows_f32(const TransformArgs& a, double alpha, hipStream_t s) {
  return dispatch_width((a.M + 7) / 8, WidthRange<1, 17>{}, [&](auto nu) { return transform_rtps_nu<nu, float>(a, alpha, s); });
}

hipError_t transform_rows_f32(const TransformArgs& a, hipStream_t s) {
  const int nu = (a.M + 7) / 8;
  if (nu <= 17) return dispatch_width(nu, WidthRange<1, 17>{}, [&](auto n) { return transform_nu_f32<n>(a, s); });
  return dispatch_width(nu, WidthRange<18, 32>{}, [&](auto n) { return transform_wide_nu<n, float>(a, s); });
}
#endif

}  // namespace efa
