// The row-per-lane dot product shared by the one-pass GC sweep (efa_gcsweep.hip) and the observation-impact contraction
// (efa_impact.hip): a lane holds a whole row x, lane l of each 16-lane row holds ye members l, 16 + l, 32 + l, ..., and every
// multiply-add is v_fmac_f64 with a DPP row_newbcast source, which takes one multiplicand from lane l of the lane's own 16-lane row.
// The DPP instructions are inline assembly (the compiler has no 64-bit DPP intrinsic).  Their DPP operand, ye, must be written by
// LDS reads only, never by a VALU instruction, so the "VALU write -> DPP read" hazard (which the compiler does not track through
// inline assembly) cannot arise; tests/test_cpu_host.py checks the generated code of every k_sweep_gc_lane* kernel for exactly that.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace efa {

template <int L>
__device__ __forceinline__ void fmac_bcast(double& acc, double y, double x) {  // acc += (y of lane L of this 16-lane row) * x
  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(y), "v"(x), "n"(L));
}
template <int MP, int... I>
__device__ __forceinline__ double lane_dot(const double (&x)[MP], const double (&y)[(MP + 15) / 16], std::integer_sequence<int, I...>) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  (fmac_bcast<I % 16>(acc[I & 3], y[I / 16], x[I]), ...);
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

}  // namespace efa
