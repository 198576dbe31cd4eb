// The four-lane row layout of the diagnostics, once: k_sens_pass (efa_sensitivity.hip), k_verify (efa_verify.hip),
// k_products (efa_products.hip) and k_nbr_records (efa_neighbourhood.hip).
//   A wave owns a tile of 16 consecutive rows.  Lane l = (g = l>>4, n = l&15) holds members {8u+2g, 8u+2g+1}, u = 0..NU-1, of row
//   n: one 16-byte load per u (8-byte for float32 rows, widened exactly as they arrive), so slot c = 2u + e of lane g is member
//   8u + 2g + e and the whole row sits in registers, 2 NU doubles per lane.  What a row needs from its four lanes is two
//   __shfl_xor steps (16, 32) or one __ballot.
//
// Two padding rules live on this layout:
//   - k_verify, k_products and k_nbr_records round NU up to a power of two (the sort network's size), so any slot may lie beyond M:
//     quad_load_row clamps every address, the slot holds a copy of a real member, and the kernel masks it with quad_slot_ok as it
//     runs (+inf for the sort, 0 for a sum).  Only k_verify calls every helper: k_products and k_nbr_records keep the text of some
//     of them in their tile loops, where the call compiled to slower code (DESIGN.md 7j2 has the measurements).
//   - k_sens_pass has NU = (M + 7) / 8 exactly and the alignment as a template parameter: only the last chunk can lie beyond M, it
//     is clamped and then ZEROED (the matrix cores read every slot), by predicates computed once per lane.  It keeps its own
//     loader for that and shares the pair type, the row reductions and the quad test.
//
// efa_gram.hip and efa_pmmean.hip take only ElemPair and finite64 from here.  What the same kernels share around their row loops
// (the table flush, the chunk partial, the group reduction) is in efa_quadreduce.h.
#pragma once
#include <hip/hip_runtime.h>

namespace efa {
namespace {

constexpr int kQuadThreads = 256;  // 4 waves, one 16-row tile per wave and trip

// two consecutive members of a row, as one load
template <typename E>
struct ElemPair;
template <>
struct ElemPair<double> { typedef double2 type; };
template <>
struct ElemPair<float> { typedef float2 type; };

__device__ __forceinline__ bool finite64(double v) { return __builtin_fabs(v) < __builtin_inf(); }

// The lane's quarter g of its row, opaque to the optimiser.  Taken inside the row loop: what depends only on g and on M (the slot
// predicates, k_verify's 2 NU weights 2j - M + 1) is otherwise hoisted out of the loop and held in registers across it, which sent
// NU = 32 to scratch.
__device__ __forceinline__ int quad_lane_quarter(int lane) {
  int gq = lane >> 4;
  asm volatile("" : "+v"(gq));
  return gq;
}

// slot c of lane quarter gq holds a real member
__device__ __forceinline__ bool quad_slot_ok(int c, int gq, int M) { return 8 * (c >> 1) + 2 * gq + (c & 1) < M; }

// Row `row` of X into the lane's slots: clamped addresses, no branches, so the loads of a tile are issued together.  A slot beyond
// M holds some real member of the row (quad_slot_ok tells).  al: the rows are aligned for the paired loads.
template <int NU, typename E>
__device__ __forceinline__ void quad_load_row(const void* X, long row, int M, int gq, int al, double (&d)[2 * NU]) {
  const E* p = reinterpret_cast<const E*>(X) + (size_t)row * M;
  if (al) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      int m0 = 8 * u + 2 * gq;
      m0 = (m0 < M) ? m0 : M - 2;
      const typename ElemPair<E>::type v = *reinterpret_cast<const typename ElemPair<E>::type*>(p + m0);
      d[2 * u] = v.x;
      d[2 * u + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int m0 = 8 * u + 2 * gq;
      d[2 * u] = p[(m0 < M) ? m0 : M - 1];
      d[2 * u + 1] = p[(m0 + 1 < M) ? m0 + 1 : M - 1];
    }
  }
}

// the sum over a row's four lanes, in every one of them
template <typename T>
__device__ __forceinline__ T quad_row_sum(T v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// some lane of row n's four says so
__device__ __forceinline__ bool quad_row_any(bool b, int n) { return ((__ballot(b) >> n) & 0x0001000100010001ull) != 0ull; }

// The mean of a row and the sum of its squared deviations, in three steps the kernels place among their other reductions (the
// order of the shuffles in the source decides the registers):
//   d0 = __shfl(d[0], n, 64) is member 0, quad_differs says whether one of the lane's members differs from it, and with
//   varies = quad_row_any(that, n) and the row sum of four lane-local chains (slot c in chain c & 3)
//     mean = varies ? sum / M : d0
//   a row whose members are all equal has member 0 as its mean and deviations of exactly 0: its sum / M need not give the member
//   back.  quad_centred_ss is the sum of the squared deviations from that mean, added up in the same four chains.
// d: the row's slots, whatever the slots beyond M hold.
template <int LP>
__device__ __forceinline__ bool quad_differs(const double (&d)[LP], double d0, int gq, int M) {
  bool diff = false;
#pragma unroll
  for (int c = 0; c < LP; ++c) {
    const bool ok = quad_slot_ok(c, gq, M);
    diff = diff || (ok && d[c] != d0);
  }
  return diff;
}

template <int LP>
__device__ __forceinline__ double quad_centred_ss(const double (&d)[LP], double mean, int gq, int M) {
  double q4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < LP; ++c) {
    const double e = quad_slot_ok(c, gq, M) ? d[c] - mean : 0.0;
    q4[c & 3] = __builtin_fma(e, e, q4[c & 3]);
  }
  return quad_row_sum((q4[0] + q4[1]) + (q4[2] + q4[3]));
}

}  // namespace
}  // namespace efa
