// The bitonic sorting network of a row held in registers in the four-lane layout (efa_quadrow.h), shared by k_verify
// (efa_verify.hip) and k_products (efa_products.hip).
//   A row's four lanes hold LP = 2 NU slots each (a power of two), padded with +inf.  Every lane sorts its slots with a network
//   whose comparators all point upwards (sortnet_local); the four lanes are merged by two bitonic stages (sortnet_split_rev,
//   sortnet_split_same across lanes, sortnet_merge inside one).  Every register index is a compile-time constant.  quad_sort is
//   the whole sequence.
#pragma once
#include <hip/hip_runtime.h>

namespace efa {
namespace {

#define SORTNET_CMPX(a, b)                   \
  {                                          \
    const double lo_ = __builtin_fmin(a, b); \
    const double hi_ = __builtin_fmax(a, b); \
    a = lo_;                                 \
    b = hi_;                                 \
  }

// sorts d[0..LP-1] upwards (LP a power of two)
template <int LP>
__device__ __forceinline__ void sortnet_local(double (&d)[LP]) {
#pragma unroll
  for (int k = 2; k <= LP; k <<= 1) {
#pragma unroll
    for (int i = 0; i < LP; ++i) {
      const int l = i ^ (k - 1);
      if (l > i) SORTNET_CMPX(d[i], d[l]);
    }
    __builtin_amdgcn_sched_barrier(0);  // (layer by layer: the scheduler otherwise spreads the network over every register)
#pragma unroll
    for (int j = k >> 2; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < LP; ++i) {
        const int l = i ^ j;
        if (l > i) SORTNET_CMPX(d[i], d[l]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// sorts a bitonic d[0..LP-1] upwards
template <int LP>
__device__ __forceinline__ void sortnet_merge(double (&d)[LP]) {
#pragma unroll
  for (int j = LP >> 1; j > 0; j >>= 1) {
#pragma unroll
    for (int i = 0; i < LP; ++i) {
      const int l = i ^ j;
      if (l > i) SORTNET_CMPX(d[i], d[l]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// two sorted lanes (this one and lane ^ mask) -> the lower keeps the LP smaller values, the upper the LP larger, each bitonic
template <int LP>
__device__ __forceinline__ void sortnet_split_rev(double (&d)[LP], int mask, bool upper) {
#pragma unroll
  for (int k = 0; k < LP / 2; ++k) {
    const int kk = LP - 1 - k;
    const double t1 = __shfl_xor(d[kk], mask, 64);
    const double t2 = __shfl_xor(d[k], mask, 64);
    d[k] = ((d[k] < t1) != upper) ? d[k] : t1;
    d[kk] = ((d[kk] < t2) != upper) ? d[kk] : t2;
    if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // (a few exchanges in flight, not all of them)
  }
}

// the first step of a bitonic merge over two lanes: same slot
template <int LP>
__device__ __forceinline__ void sortnet_split_same(double (&d)[LP], int mask, bool upper) {
#pragma unroll
  for (int k = 0; k < LP; ++k) {
    const double t = __shfl_xor(d[k], mask, 64);
    d[k] = ((d[k] < t) != upper) ? d[k] : t;
    if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);
  }
}

// the row's 4 LP slots, sorted: afterwards sorted position g LP + k is slot k of lane quarter g
template <int LP>
__device__ __forceinline__ void quad_sort(double (&d)[LP], int gq) {
  __builtin_amdgcn_sched_barrier(0);
  sortnet_local<LP>(d);
  sortnet_split_rev<LP>(d, 16, (gq & 1) != 0);
  sortnet_merge<LP>(d);
  sortnet_split_rev<LP>(d, 48, gq >= 2);
  sortnet_split_same<LP>(d, 16, (gq & 1) != 0);
  sortnet_merge<LP>(d);
}

}  // namespace
}  // namespace efa
