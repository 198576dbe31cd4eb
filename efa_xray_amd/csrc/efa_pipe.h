// Device primitives shared by the three persistent Phase-A kernels (k_pipe, k_pipe_gram, k_pipe_band).
#pragma once
#include <hip/hip_runtime.h>

namespace efa {

typedef unsigned long long u64;
typedef double v4f64 __attribute__((ext_vector_type(4)));

// Trajectory records in global memory: every 8-byte element is written once and read on its own (efa_internal.h, kTrajSentinel),
// agent scope because the per-XCD L2s are not coherent.
__device__ __forceinline__ u64 traj_load(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void traj_store(u64* p, double v) {
  __hip_atomic_store(p, (u64)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// LDS control words: plain in-order LDS accesses + a compiler barrier (efa_pipeline.hip, header comment)
__device__ __forceinline__ int ctl_load_lane(const int* p) {  // per-lane address
  const int v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  asm volatile("" ::: "memory");
  return v;
}
// every lane reads the same word: hand the compiler a wave-uniform (SGPR) value so that the
// spin / bail logic compiles to scalar branches instead of exec-mask bookkeeping
__device__ __forceinline__ int ctl_load(const int* p) { return __builtin_amdgcn_readfirstlane(ctl_load_lane(p)); }
__device__ __forceinline__ void ctl_store(int* p, int v) {
  asm volatile("" ::: "memory");
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// v_rsq_f64 / v_rcp_f64 are accurate to 2e-8 relative on gfx950 (measured, tools/latency_probe.hip):
// one Newton step squares that (rsq: 1.5 e^2, rcp: e^2) -- below double rounding; the second-order
// term of the rsq step is added so that both land within ~1 ulp.
__device__ __forceinline__ double fast_rsq(double a) {  // 1/sqrt(a)
  const double q = __builtin_amdgcn_rsq(a);
  const double e = __builtin_fma(-a * q, q, 1.0);           // 1 - a q^2
  const double p = __builtin_fma(0.375, e, 0.5);            // 1/2 + 3/8 e
  return __builtin_fma(q * e, p, q);                        // q (1 + e/2 + 3 e^2/8)
}
__device__ __forceinline__ double fast_rcp(double b) {  // 1/b
  const double r = __builtin_amdgcn_rcp(b);
  const double e = __builtin_fma(-b, r, 1.0);
  return __builtin_fma(r, __builtin_fma(e, e, e), r);        // r (1 + e + e^2)
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {  // value held by `lane` (wave-uniform index)
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

}  // namespace efa
