// Posterior inflation by relaxation (Whitaker & Hamill 2012): the standalone passes and the RTPP fold.
//
// For state row i with prior perturbations b_i and posterior perturbations a_i (member deviations from the row mean):
//   RTPP(alpha): xa_i <- mean(xa_i) + (1 - alpha) a_i + alpha b_i
//   RTPS(alpha): xa_i <- mean(xa_i) + a_i ((1 - alpha) + alpha sigma_b / sigma_a)   (rows with sigma_a == 0 untouched)
// Rows are independent.  On the unlocalised transform path RTPP is folded into T (k_relax_fold: Xap = Xbp ((1-alpha) T +
// alpha I)) and RTPS is fused into the member-form transform (k_transform_rtps, efa_transform.hip) up to 136 members.  Every
// other path runs the two memory-bound passes below around its state phase: k_row_spread records sum_m b_im^2 of each row
// BEFORE the state phase (the posterior may overwrite the prior), k_relax_rows rescales the posterior rows in place after it.
// Both work on member rows and on perturbation rows alike (the row mean is removed in the kernel; in perturbation form the
// mean row xam is left as it is and the posterior perturbation row keeps its own mean).
#include "efa_device.h"
#include "efa_internal.h"

namespace efa {
namespace {

constexpr int kThreadsR = 256;
constexpr int kPer = kMaxMembers / 64;  // members per lane

// Tout = (1 - alpha) T + alpha I  (M x M, row-major)
__global__ __launch_bounds__(kThreadsR) void k_relax_fold(int M, double alpha, const double* __restrict__ T,
                                                          double* __restrict__ Tout) {
  const long n = (long)M * M;
  for (long i = (long)blockIdx.x * kThreadsR + threadIdx.x; i < n; i += (long)gridDim.x * kThreadsR) {
    const long r = i / M, c = i - r * M;
    Tout[i] = (1.0 - alpha) * T[i] + ((r == c) ? alpha : 0.0);
  }
}

// One wave per row (as k_form_perts): lane l holds members l, l+64, ...
__device__ __forceinline__ double load_row(const double* __restrict__ p, int M, int lane, double (&v)[kPer]) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int m = lane + 64 * j;
    v[j] = (m < M) ? p[m] : 0.0;
    s += v[j];
  }
  return wave_sum(s) / (double)M;
}

// ss[row] = sum_m (X[row][m] - mean)^2
__global__ __launch_bounds__(kThreadsR) void k_row_spread(long rows, int M, const double* __restrict__ X,
                                                          double* __restrict__ ss) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (kThreadsR / 64) + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * (kThreadsR / 64);
  for (long row = wave; row < rows; row += nwaves) {
    double v[kPer];
    const double mean = load_row(X + (size_t)row * M, M, lane, v);
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const double d = (lane + 64 * j < M) ? v[j] - mean : 0.0;
      q = fma(d, d, q);
    }
    q = wave_sum(q);
    if (lane == 0) ss[row] = q;
  }
}

// RTPS (prior == null): X[row] <- mean + s (X[row] - mean), s from ss[row];  RTPP: with the prior rows
template <bool RTPP>
__global__ __launch_bounds__(kThreadsR) void k_relax_rows(long rows, int M, double alpha, double* __restrict__ X,
                                                          const double* __restrict__ ss, const double* __restrict__ prior) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * (kThreadsR / 64) + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * (kThreadsR / 64);
  for (long row = wave; row < rows; row += nwaves) {
    double* p = X + (size_t)row * M;
    double v[kPer];
    const double mean = load_row(p, M, lane, v);
    if (RTPP) {
      double b[kPer];
      const double bmean = load_row(prior + (size_t)row * M, M, lane, b);
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int m = lane + 64 * j;
        if (m < M) p[m] = mean + ((1.0 - alpha) * (v[j] - mean) + alpha * (b[j] - bmean));
      }
    } else {
      double q = 0.0;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const double d = (lane + 64 * j < M) ? v[j] - mean : 0.0;
        q = fma(d, d, q);
      }
      q = wave_sum(q);
      if (!(q > 0.0)) continue;  // sigma_a == 0: the row stays as it is (wave-uniform)
      const double sc = (1.0 - alpha) + alpha * sqrt(ss[row] / q);
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int m = lane + 64 * j;
        if (m < M) p[m] = mean + sc * (v[j] - mean);
      }
    }
  }
}

unsigned rows_grid(long rows) {
  long g = (rows + kThreadsR / 64 - 1) / (kThreadsR / 64);
  if (g > 256L * 8) g = 256L * 8;
  if (g < 1) g = 1;
  return (unsigned)g;
}

}  // namespace

hipError_t launch_relax_fold(int M, double alpha, const double* T, double* Tout, hipStream_t s) {
  if (M < 1 || M > kMaxMembers) return hipErrorInvalidValue;
  const long n = (long)M * M;
  hipLaunchKernelGGL(k_relax_fold, dim3((unsigned)((n + kThreadsR - 1) / kThreadsR)), dim3(kThreadsR), 0, s, M, alpha, T, Tout);
  return hipGetLastError();
}

hipError_t launch_row_spread(long rows, int M, const double* X, double* ss, hipStream_t s) {
  if (M < 1 || M > kMaxMembers) return hipErrorInvalidValue;
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_row_spread, dim3(rows_grid(rows)), dim3(kThreadsR), 0, s, rows, M, X, ss);
  return hipGetLastError();
}

hipError_t launch_relax_rows(long rows, int M, int rtpp, double alpha, double* X, const double* ss, const double* prior,
                             hipStream_t s) {
  if (M < 1 || M > kMaxMembers) return hipErrorInvalidValue;
  if (rows <= 0) return hipSuccess;
  if (rtpp) hipLaunchKernelGGL(k_relax_rows<true>, dim3(rows_grid(rows)), dim3(kThreadsR), 0, s, rows, M, alpha, X, ss, prior);
  else hipLaunchKernelGGL(k_relax_rows<false>, dim3(rows_grid(rows)), dim3(kThreadsR), 0, s, rows, M, alpha, X, ss, prior);
  return hipGetLastError();
}

}  // namespace efa
