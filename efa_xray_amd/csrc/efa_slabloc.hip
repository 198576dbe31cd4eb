// Temporal and cross-variable localisation: the slab-factor table of the one-pass GC sweep's "slab table" family
// (k_sweep_gc / k_sweep_gc_lane with FAM = kGcSlab, efa_gcsweep_kernels.h) and the obs-obs taper passes of Phase A.
//
// k_slab_factor writes S[k][s] = (V(s,k) T(s,k)) C[k, v_s] for every (ob k, slab s): V the vertical factor of §7d (1 when that
// setting is off), T = GC(|t_s - t_k|, tau_k) (1 when t_s, t_k or tau_k is NaN), C the impact of ob k's obtype on slab s's
// variable (1 for an ob without an impact row).  Each product is rounded once, in that order.
// k_obs_taper_slab multiplies T(j,k) C[k, v_j] into the dense obs-obs table behind k_obs_taper_matrix (and k_obs_taper_vert):
// tw[k][j] = (tw[k][j] T) C for j < P; zeros stay as they are and columns j >= P (carried identity rows) are left alone.
// k_obs_taper_rows_slab is k_obs_taper_rows (efa_vloc.hip) with the two factors: the per-batch sweep's table of one batch.
#include "efa_device.h"
#include "efa_internal.h"
#include "efa_slabfactor.h"

namespace efa {
namespace {

__global__ __launch_bounds__(256) void k_slab_factor(long P, long n_lead, const double* __restrict__ lead_vert,
                                                     const double* __restrict__ ob_vert, const double* __restrict__ ob_vhw,
                                                     const double* __restrict__ lead_time, const int* __restrict__ lead_var,
                                                     const SlabObs o, double* __restrict__ S) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * n_lead) return;
  const long k = i / n_lead;
  const long lead = i - k * n_lead;
  const double v = lead_vert ? vert_factor(lead_vert[lead], ob_vert[k], ob_vhw[k]) : 1.0;
  const double vt = v * time_factor(lead_time[lead], o.ob_time[k], o.ob_thw[k]);
  S[i] = vt * impact_factor(o, k, lead_var[lead]);
}

// the table without a slab setting (lead_time null: the LETKF under the vertical setting alone): S = V, or 1 when
// lead_vert is null as well -- what k_slab_factor writes when T and C are 1, (V * 1) * 1
__global__ __launch_bounds__(256) void k_slab_factor_vert(long P, long n_lead, const double* __restrict__ lead_vert,
                                                          const double* __restrict__ ob_vert, const double* __restrict__ ob_vhw,
                                                          double* __restrict__ S) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * n_lead) return;
  const long k = i / n_lead;
  const long lead = i - k * n_lead;
  S[i] = lead_vert ? vert_factor(lead_vert[lead], ob_vert[k], ob_vhw[k]) : 1.0;
}

__global__ __launch_bounds__(256) void k_obs_taper_slab(long P, long R, const SlabObs o, double* __restrict__ tw) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= P) return;
  const double tj = o.ob_time[j];
  const int vj = o.ob_var[j];
  for (long k = blockIdx.y; k < P; k += gridDim.y) {
    double* p = tw + (size_t)k * R + j;
    const double w = *p;
    if (w == 0.0) continue;
    const double wt = w * time_factor(tj, o.ob_time[k], o.ob_thw[k]);
    *p = wt * impact_factor(o, k, vj);
  }
}

__global__ __launch_bounds__(256) void k_obs_taper_rows_slab(long b0, int nb, long R, long P, const double* __restrict__ lat,
                                                             const double* __restrict__ lon, const double* __restrict__ hw,
                                                             const double* __restrict__ vert, const double* __restrict__ vhw,
                                                             const SlabObs o, double* __restrict__ W) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  if (j >= R || k >= nb) return;
  double w = 1.0;  // rows beyond the obs: weight 1, as kTaperObs gives rows >= taper_rows
  if (j < P) {
    const long kk = b0 + k;
    w = gaspari_cohn(haversine_km(lat[kk], lon[kk], lat[j], lon[j]), hw[kk]);
    if (vert) w = w * vert_factor(vert[j], vert[kk], vhw[kk]);
    w = w * time_factor(o.ob_time[j], o.ob_time[kk], o.ob_thw[kk]);
    w = w * impact_factor(o, kk, o.ob_var[j]);
  }
  W[(size_t)k * R + j] = w;
}

}  // namespace

hipError_t launch_slab_factor(long P, long n_lead, const double* lead_vert, const double* ob_vert, const double* ob_vhw,
                              const double* lead_time, const int* lead_var, const SlabObs& o, double* S, hipStream_t s) {
  if (P <= 0 || n_lead <= 0) return hipSuccess;
  if (lead_vert && (!ob_vert || !ob_vhw)) return hipErrorInvalidValue;
  const long n = P * n_lead;
  if (!lead_time) {  // no slab setting: the vertical factor alone (lead_var and o are not read)
    hipLaunchKernelGGL(k_slab_factor_vert, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, n_lead, lead_vert, ob_vert, ob_vhw, S);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_slab_factor, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, n_lead, lead_vert, ob_vert, ob_vhw, lead_time,
                     lead_var, o, S);
  return hipGetLastError();
}

hipError_t launch_obs_taper_slab(long P, long R, const SlabObs& o, double* tw, hipStream_t s) {
  if (P <= 0 || R < P) return P <= 0 ? hipSuccess : hipErrorInvalidValue;
  long gy = P < 1024 ? P : 1024;
  hipLaunchKernelGGL(k_obs_taper_slab, dim3((unsigned)((P + 255) / 256), (unsigned)gy), dim3(256), 0, s, P, R, o, tw);
  return hipGetLastError();
}

hipError_t launch_obs_taper_rows_slab(long b0, int nb, long R, long P, const double* ob_lat, const double* ob_lon, const double* ob_hw,
                                      const double* ob_vert, const double* ob_vhw, const SlabObs& o, double* W, hipStream_t s) {
  if (nb <= 0 || R <= 0) return hipSuccess;
  if (nb > kMaxBatch || b0 < 0 || b0 + nb > P || R < P) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_obs_taper_rows_slab, dim3((unsigned)((R + 255) / 256), (unsigned)nb), dim3(256), 0, s, b0, nb, R, P, ob_lat,
                     ob_lon, ob_hw, ob_vert, ob_vhw, o, W);
  return hipGetLastError();
}

}  // namespace efa
