// The temporal and cross-variable factors of DESIGN.md §7t as device functions, shared by the table and obs-obs taper kernels of
// efa_slabloc.hip and by the LETKF's obs-block factor (efa_letkf.hip, §7y-3).  The vertical factor is vert_factor (efa_device.h).
#pragma once
#include "efa_device.h"
#include "efa_internal.h"

namespace efa {

// GC(|t_x - t_k|, tau_k); 1 when row x has no time, or ob k no time or no temporal half-width (NaN)
__device__ __forceinline__ double time_factor(double t_x, double t_k, double thw_k) {
  return (t_x == t_x && t_k == t_k && thw_k == thw_k) ? gaspari_cohn(fabs(t_x - t_k), thw_k) : 1.0;
}
// C[obtype of ob k, variable v]; 1 for an ob without an impact row (group -1) and for a row without a variable (v -1)
__device__ __forceinline__ double impact_factor(const SlabObs& o, long k, int v) {
  const int g = o.ob_group[k];
  return (g >= 0 && v >= 0) ? o.impact[(size_t)g * o.n_var + v] : 1.0;
}

}  // namespace efa
