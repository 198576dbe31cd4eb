// Spatially varying adaptive inflation (Anderson 2009): the two passes outside the sweep.
//
// k_inflate_rows applies each state row's prior inflation in place, x_im <- mean_i + sqrt(lambda_i) (x_im - mean_i), before the
// forward operator.  It is memory-bound (one read and one write of the rows it changes); a row with lambda == 1 is neither
// recomputed nor written, since mean + (x - mean) is not x in floating point.
// k_adapt_obs folds, once per cycle, what the sweep's per-(row, ob) update needs of each observation into one 32-byte record:
// D^2 = innov^2 (innov from Phase A's coefficients), sigma_p^2 = prior var (ddof 0), sigma_o^2 = the ob's error variance, and
// y'.y' summed over the recorded ye row the sweep reads.  The update itself is fused into the one-pass GC sweep (efa_gcsweep.hip).
#include "efa_device.h"
#include "efa_internal.h"

namespace efa {
namespace {

constexpr int kThreadsA = 256;
constexpr int kPerA = kMaxMembers / 64;  // members per lane

// One wave per row (as k_relax_rows): lane l holds members l, l + 64, ...
__global__ __launch_bounds__(kThreadsA) void k_inflate_rows(long rows, int M, double* __restrict__ X,
                                                            const double* __restrict__ field) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (kThreadsA / 64) + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * (kThreadsA / 64);
  for (long row = wave; row < rows; row += nwaves) {
    const double lam = field[2 * row];
    if (lam == 1.0) continue;  // (wave-uniform) the row stays bit for bit as it is
    const double f = sqrt(lam);
    double* p = X + (size_t)row * M;
    double v[kPerA];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kPerA; ++j) {
      const int m = lane + 64 * j;
      v[j] = (m < M) ? p[m] : 0.0;
      s += v[j];
    }
    const double mean = wave_sum(s) / (double)M;
#pragma unroll
    for (int j = 0; j < kPerA; ++j) {
      const int m = lane + 64 * j;
      if (m < M) p[m] = mean + f * (v[j] - mean);
    }
  }
}

__global__ __launch_bounds__(kThreadsA) void k_adapt_obs(long P, int M, const double* __restrict__ coef,
                                                         const double* __restrict__ prior_var,
                                                         const double* __restrict__ ob_error, const double* __restrict__ Ye,
                                                         long ye_stride, double* __restrict__ out) {
  const long k = (long)blockIdx.x * kThreadsA + threadIdx.x;
  if (k >= P) return;
  const bool active = coef[k * kCoefStride + 3] != 0.0;  // (an ob not assimilated has no record to read: its taper is staged as 0)
  const double* y = Ye + (size_t)k * ye_stride;
  double q0 = 0.0, q1 = 0.0;
  int m = 0;
  for (; active && m + 1 < M; m += 2) {
    q0 = fma(y[m], y[m], q0);
    q1 = fma(y[m + 1], y[m + 1], q1);
  }
  if (active && m < M) q0 = fma(y[m], y[m], q0);
  const double innov = coef[k * kCoefStride + 0];
  double* o = out + (size_t)k * 4;
  o[0] = active ? innov * innov : 0.0;
  o[1] = active ? prior_var[k] : 0.0;
  o[2] = active ? ob_error[k] : 0.0;
  o[3] = active ? q0 + q1 : 0.0;
}

}  // namespace

hipError_t launch_inflate_rows(long rows, int M, double* X, const double* field, hipStream_t s) {
  if (M < 1 || M > kMaxMembers) return hipErrorInvalidValue;
  if (rows <= 0) return hipSuccess;
  long g = (rows + kThreadsA / 64 - 1) / (kThreadsA / 64);
  if (g > 256L * 8) g = 256L * 8;
  hipLaunchKernelGGL(k_inflate_rows, dim3((unsigned)g), dim3(kThreadsA), 0, s, rows, M, X, field);
  return hipGetLastError();
}

hipError_t launch_adapt_obs(long P, int M, const double* coef, const double* prior_var, const double* ob_error, const double* Ye,
                            long ye_stride, double* out, hipStream_t s) {
  if (P <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_adapt_obs, dim3((unsigned)((P + kThreadsA - 1) / kThreadsA)), dim3(kThreadsA), 0, s, P, M, coef, prior_var,
                     ob_error, Ye, ye_stride, out);
  return hipGetLastError();
}

}  // namespace efa
