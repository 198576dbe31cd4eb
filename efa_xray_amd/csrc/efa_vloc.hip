// Vertical localisation: the two obs-obs taper passes of Phase A.  The state rows' factor is fused into the
// one-pass GC sweep (k_sweep_gc / k_sweep_gc_lane with FAM = kGcVloc, efa_gcsweep_kernels.h).
//
// k_obs_taper_vert multiplies the vertical factor into the dense obs-obs table that k_obs_taper_matrix wrote, which the band,
// Gram and vector-chain Phase-A kernels read: tw[k][j] = GC_h(j, k) * GC(|z_j - z_k|, c_k).  The horizontal value is rounded
// first and the product once, as the NumPy definition does.  Columns j >= P (carried identity rows) are left as they are.
// k_obs_taper_rows writes the per-batch sweep's table of one batch, ob b0 + k against row j of the obs block, with the
// horizontal formula of k_sweep's in-kernel taper (kTaperObs) times the vertical factor; k_sweep then reads it in table mode.
#include "efa_device.h"
#include "efa_internal.h"

namespace efa {
namespace {

__global__ __launch_bounds__(256) void k_obs_taper_vert(long P, long R, const double* __restrict__ vert,
                                                        const double* __restrict__ vhw, double* __restrict__ tw) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= P) return;
  const double zj = vert[j];
  if (!(zj == zj)) return;  // no vertical information on row j: factor 1 against every ob
  for (long k = blockIdx.y; k < P; k += gridDim.y) {
    const double zk = vert[k];
    if (!(zk == zk)) continue;
    double* p = tw + (size_t)k * R + j;
    const double w = *p;
    if (w != 0.0) *p = w * gaspari_cohn(fabs(zj - zk), vhw[k]);
  }
}

__global__ __launch_bounds__(256) void k_obs_taper_rows(long b0, int nb, long R, long P, const double* __restrict__ lat,
                                                        const double* __restrict__ lon, const double* __restrict__ hw,
                                                        const double* __restrict__ vert, const double* __restrict__ vhw,
                                                        double* __restrict__ W) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  if (j >= R || k >= nb) return;
  double w = 1.0;  // rows beyond the obs: weight 1, as kTaperObs gives rows >= taper_rows
  if (j < P) {
    const long kk = b0 + k;
    w = gaspari_cohn(haversine_km(lat[kk], lon[kk], lat[j], lon[j]), hw[kk]);
    w = w * vert_factor(vert[j], vert[kk], vhw[kk]);
  }
  W[(size_t)k * R + j] = w;
}

}  // namespace

hipError_t launch_obs_taper_vert(long P, long R, const double* ob_vert, const double* ob_vhw, double* tw, hipStream_t s) {
  if (P <= 0 || R < P) return P <= 0 ? hipSuccess : hipErrorInvalidValue;
  long gy = P < 1024 ? P : 1024;
  hipLaunchKernelGGL(k_obs_taper_vert, dim3((unsigned)((P + 255) / 256), (unsigned)gy), dim3(256), 0, s, P, R, ob_vert, ob_vhw, tw);
  return hipGetLastError();
}

hipError_t launch_obs_taper_rows(long b0, int nb, long R, long P, const double* ob_lat, const double* ob_lon, const double* ob_hw,
                                 const double* ob_vert, const double* ob_vhw, double* W, hipStream_t s) {
  if (nb <= 0 || R <= 0) return hipSuccess;
  if (nb > kMaxBatch || b0 < 0 || b0 + nb > P || R < P) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_obs_taper_rows, dim3((unsigned)((R + 255) / 256), (unsigned)nb), dim3(256), 0, s, b0, nb, R, P, ob_lat, ob_lon,
                     ob_hw, ob_vert, ob_vhw, W);
  return hipGetLastError();
}

}  // namespace efa
