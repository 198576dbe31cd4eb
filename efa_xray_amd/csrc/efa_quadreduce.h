// What the diagnostics on the four-lane row layout (efa_quadrow.h) share around their row loops: the flush of a workgroup's LDS
// count table and the chunk partial (k_verify; k_products keeps its own text of both), and k_group_reduce, the one
// kernel that adds the partials of each group of slabs in a fixed order (efa_verify.hip, efa_products.hip,
// efa_neighbourhood.hip).  No floating-point atomics anywhere: the same inputs give the same bits whatever the grid.
#pragma once
#include "efa_quadrow.h"

namespace efa {
namespace {

// The workgroup's 32-bit count table in LDS goes to its 64-bit copy in memory: integer atomics, whose result no order can change.
// Callers put a __syncthreads() in front; `clear`: the LDS table starts again at 0 (the caller syncs before it counts on).
__device__ __forceinline__ void quad_flush_table(unsigned int* tab_s, int len, unsigned long long* dst, bool clear) {
  for (int i = threadIdx.x; i < len; i += kQuadThreads) {
    const unsigned int v = tab_s[i];
    if (v) atomicAdd(&dst[i], (unsigned long long)v);
    if (clear) tab_s[i] = 0u;
  }
}

// A chunk's partial: the 64 lane sums of a field, (wave w, row lane n) at index 16 w + n, added in index order -- so it depends on
// neither the grid nor the schedule.  at(i): where lane sum i of this field lies in LDS.
template <typename R, typename T, typename At>
__device__ __forceinline__ R quad_chunk_partial(const T* lds, At at) {
  R s = 0;
  for (int i = 0; i < 64; ++i) s += lds[at(i)];
  return s;
}

// ---- the group reduction ---------------------------------------------------------------------------------------------------------
// Workgroup (group grp, field f): adds the partials of the items (chunks, tiles) whose slab belongs to grp.  Item i belongs to slab
// i / per_slab of the call's list, which `slabs` (or null: the identity) maps to the slab whose group sgroup holds.  Thread tid
// takes items tid, tid + 256, ... in order, then a tree over the threads with off = 128 .. 1: the order is a function of the sizes
// alone.  nf = gridDim.y fields are reduced out of the fstride an item holds: part [items][fstride][NSUMS], cnt [items][fstride][NCNT]
// -> sums [G][nf][NSUMS], cnt0 [G][nf] from count column 0 and cnt1 [G][nf] from column 1 (NCNT = 1: cnt1 unused).
// (Sizes as template parameters and restrict-qualified pointers: the code the three reduce kernels it replaces compiled to.)
template <int NSUMS, int NCNT>
__global__ __launch_bounds__(kQuadThreads) void k_group_reduce(long items, long per_slab, int fstride, const int* __restrict__ slabs,
                                                               const int* __restrict__ sgroup, const double* __restrict__ part,
                                                               const long long* __restrict__ cnt, double* __restrict__ sums,
                                                               long long* __restrict__ cnt0, long long* __restrict__ cnt1) {
  __shared__ double s_s[kQuadThreads];
  __shared__ long long c_s[kQuadThreads];
  const int tid = threadIdx.x;
  const int grp = (int)blockIdx.x, f = (int)blockIdx.y, nf = (int)gridDim.y;
  for (int k = 0; k < NSUMS + NCNT; ++k) {
    double s = 0.0;
    long long c = 0;
    for (long i = tid; i < items; i += kQuadThreads) {
      const long sl = i / per_slab;
      if (sgroup[slabs ? slabs[sl] : sl] != grp) continue;
      if (k < NSUMS) s += part[((size_t)i * fstride + f) * NSUMS + k];
      else c += cnt[((size_t)i * fstride + f) * NCNT + (k - NSUMS)];
    }
    s_s[tid] = s;
    c_s[tid] = c;
    __syncthreads();
    for (int off = kQuadThreads / 2; off >= 1; off >>= 1) {
      if (tid < off) {
        s_s[tid] += s_s[tid + off];
        c_s[tid] += c_s[tid + off];
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (k < NSUMS) sums[((size_t)grp * nf + f) * NSUMS + k] = s_s[0];
      else (k == NSUMS ? cnt0 : cnt1)[(size_t)grp * nf + f] = c_s[0];
    }
    __syncthreads();
  }
}

// G groups times nf fields; the other arguments are the kernel's
template <int NSUMS, int NCNT>
hipError_t launch_group_reduce(int G, int nf, hipStream_t s, long items, long per_slab, int fstride, const int* slabs, const int* sgroup,
                               const double* part, const long long* cnt, double* sums, long long* cnt0, long long* cnt1) {
  hipLaunchKernelGGL((k_group_reduce<NSUMS, NCNT>), dim3((unsigned)G, (unsigned)nf), dim3(kQuadThreads), 0, s, items, per_slab, fstride,
                     slabs, sgroup, part, cnt, sums, cnt0, cnt1);
  return hipGetLastError();
}

}  // namespace
}  // namespace efa
