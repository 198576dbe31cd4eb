// The batch observation-space solver (ETKF): all assimilated obs at once in ensemble space.
//   Over the obs with an effective flag of 1: s_k = 1/sqrt(r_k), Y~_k = s_k Yp[k,:], d~_k = s_k (value_k - ym_k);
//   C = Y~^T Y~, g = Y~^T d~, q = d~^T d~;  A = (M-1) I + C = V diag(mu) V^T;
//   T = V diag(sqrt((M-1)/mu)) V^T (the symmetric square root), w = V diag(1/mu) V^T g.
// [T | w] go where Phase A's carried identity rows come out (the tail of the working block): k_transform reads them there.
//
// k_etkf_prior    a wave per ob: prior_mean, prior_var (ddof 0, two passes), the assimilated byte, and the ob's scale s_k (0 for an
//                 ob that is not assimilated: a select, never a product with its value or error) and scaled innovation d~_k.
// k_etkf_gram     [Y~ | d~]^T [Y~ | d~] (M+1 columns, tiles of 16) on v_mfma_f64_16x16x4_f64, the contraction index the ob.  A wave
//                 owns ONE upper tile (ta <= tb) of ONE accumulation stream and reads its two operand columns straight from the obs
//                 block (L2 resident; lane (g = l>>4, n = l&15) holds row 4k+g, column 16t+n, as k_gram does).  Stream s takes the
//                 chunks of 32 obs s, s+S, ... in order; S depends on (M, P) alone.  No LDS, no atomics.
// k_etkf_reduce   adds the streams' partial tiles in stream order, mirrors, adds (M-1) on the diagonal: A, g, q.
// k_etkf_eig      ONE workgroup.  Parallel cyclic one-sided (Hestenes) Jacobi on the columns of A (= its rows): round-robin rounds of
//                 M/2 disjoint column pairs, 16 lanes per pair, a rotation when |gamma| > 2^-50 sqrt(alpha beta) (the squared norms
//                 alpha, beta recomputed once per sweep and updated by every rotation; only gamma is a dot product per pair).  The sweep loop is a
//                 counted loop (kEtkfSweepCap) that a sweep without a rotation leaves early; a NaN never satisfies the test, so a NaN
//                 block ends after one sweep with NaNs.  Afterwards the column norms are mu and the normalised columns V.  The array
//                 lives in LDS up to kEtkfLdsMaxM members and in its (L2 resident) global workspace above: the same code.
// k_etkf_post     a wave per ob: post_mean, post_var (ddof 0) of the mapped obs rows.
#include "efa_device.h"
#include "efa_etkf_eig.h"
#include "efa_internal.h"
#include "efa_rows.h"

namespace efa {
namespace {

typedef double etkf_v4 __attribute__((ext_vector_type(4)));

constexpr int kEtkfRows = 32;       // obs per chunk: 8 MFMA steps of 4
constexpr int kEtkfStreamCap = 256; // accumulation streams at most ...
constexpr int kEtkfWaveCap = 8192;  // ... and tiles x streams at most (the partials stay a few MB)

__global__ __launch_bounds__(256) void k_etkf_prior(long P, int M, const double* __restrict__ Yp, const double* __restrict__ ym,
                                                    const double* __restrict__ ob_value, const double* __restrict__ ob_error,
                                                    const uint8_t* __restrict__ ob_assim, double* __restrict__ prior_mean,
                                                    double* __restrict__ prior_var, uint8_t* __restrict__ assimilated,
                                                    double* __restrict__ sc, double* __restrict__ dt) {
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  for (long k = wave; k < P; k += nwaves) {
    const double* row = Yp + (size_t)k * M;
    double v[4];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = lane + 64 * j;
      v[j] = (m < M) ? row[m] : 0.0;
      s += v[j];
    }
    const double mean = wave_sum(s) / (double)M;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double e = (lane + 64 * j < M) ? v[j] - mean : 0.0;
      q += e * e;
    }
    const double var = wave_sum(q) / (double)M;
    if (lane == 0) {
      const bool on = ob_assim[k] != 0;
      const double y = ym[k];
      prior_mean[k] = y;
      prior_var[k] = var;
      assimilated[k] = on ? 1 : 0;
      double s_k = 0.0, d_k = 0.0;
      if (on) {
        s_k = 1.0 / sqrt(ob_error[k]);
        d_k = s_k * (ob_value[k] - y);
      }
      sc[k] = s_k;
      dt[k] = d_k;
    }
  }
}

__global__ __launch_bounds__(256) void k_etkf_post(long P, int M, const double* __restrict__ Yw, const double* __restrict__ ymw,
                                                   double* __restrict__ post_mean, double* __restrict__ post_var) {
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  for (long k = wave; k < P; k += nwaves) {
    const double* row = Yw + (size_t)k * M;
    double v[4];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = lane + 64 * j;
      v[j] = (m < M) ? row[m] : 0.0;
      s += v[j];
    }
    const double mean = wave_sum(s) / (double)M;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double e = (lane + 64 * j < M) ? v[j] - mean : 0.0;
      q += e * e;
    }
    const double var = wave_sum(q) / (double)M;
    if (lane == 0) {
      post_mean[k] = ymw[k];
      post_var[k] = var;
    }
  }
}

// upper tile ti of a T x T tile grid, row by row: (0,0) (0,1) .. (0,T-1) (1,1) ..
__device__ __forceinline__ void etkf_tile(int ti, int T, int* ta, int* tb) {
  int a = 0;
  while (ti >= T - a) {
    ti -= T - a;
    ++a;
  }
  *ta = a;
  *tb = a + ti;
}

// grid (ceil(ntiles / 4), S), 4 waves: wave w of block (bx, st) owns tile 4 bx + w of stream st
__global__ __launch_bounds__(256) void k_etkf_gram(long P, int M, int T, int ntiles, int nstreams, const double* __restrict__ Yp,
                                                   const double* __restrict__ sc, const double* __restrict__ dt,
                                                   double* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int ti = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + ((int)threadIdx.x >> 6));
  const int st = (int)blockIdx.y;
  if (ti >= ntiles) return;  // (wave-uniform)
  int ta, tb;
  etkf_tile(ti, T, &ta, &tb);
  const int g = lane >> 4, n = lane & 15;
  const int ca = 16 * ta + n, cb = 16 * tb + n;
  const long nchunks = (P + kEtkfRows - 1) / kEtkfRows;
  etkf_v4 acc = etkf_v4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (long ch = st; ch < nchunks; ch += nstreams) {
#pragma unroll
    for (int k = 0; k < kEtkfRows / 4; ++k) {
      const long row = ch * kEtkfRows + 4 * k + g;
      double a = 0.0, b = 0.0;
      if (row < P) {
        const double s = sc[row];
        if (s != 0.0) {  // an ob that is not assimilated contributes exact zeros, whatever its row holds
          const double* yr = Yp + (size_t)row * M;
          const double d = dt[row];
          a = ca < M ? s * yr[ca] : (ca == M ? d : 0.0);
          b = cb < M ? s * yr[cb] : (cb == M ? d : 0.0);
        }
      }
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
  }
  double* out = part + ((size_t)st * ntiles + ti) * 256;
#pragma unroll
  for (int v = 0; v < 4; ++v) out[(g + 4 * v) * 16 + n] = acc[v];
}

// block ti, thread (i = tid >> 4, j = tid & 15): element (16 ta + i, 16 tb + j), the streams added in stream order
__global__ __launch_bounds__(256) void k_etkf_reduce(int M, int T, int ntiles, int nstreams, const double* __restrict__ part,
                                                     double* __restrict__ A, double* __restrict__ gvec, double* __restrict__ q) {
  const int ti = (int)blockIdx.x, tid = (int)threadIdx.x;
  int ta, tb;
  etkf_tile(ti, T, &ta, &tb);
  const int i = tid >> 4, j = tid & 15;
  const int I = 16 * ta + i, J = 16 * tb + j;
  const double* p = part + (size_t)ti * 256 + tid;
  double s = 0.0;
  for (int st = 0; st < nstreams; ++st) s += p[(size_t)st * ntiles * 256];
  if (ta == tb && i > j) return;  // a diagonal tile holds each pair twice: the upper one is mirrored
  if (I < M && J < M) {
    const double v = (I == J) ? s + (double)(M - 1) : s;
    A[(size_t)I * M + J] = v;
    A[(size_t)J * M + I] = v;
  } else if (I < M && J == M) {
    gvec[I] = s;
  } else if (I == M && J == M) {
    *q = s;
  }
}

// G: the array, column j at G + j M.  One workgroup of a multiple of 64 threads; 16 lanes per column pair.  The body is
// etkf_eig_solve (efa_etkf_eig.h), which k_letkf runs once per column on an array of its own.
__global__ __launch_bounds__(1024) void k_etkf_eig(int M, int use_lds, double* A, const double* __restrict__ gvec, double* mu_out,
                                                   double* Tout, double* wout, double* sweeps_out) {
  extern __shared__ __align__(16) double etkf_smem[];
  __shared__ double f_s[kMaxMembers];  // sqrt((M-1)/mu_j)
  __shared__ double h_s[kMaxMembers];  // (V_j . g) / mu_j
  __shared__ double n_s[kMaxMembers];  // squared column norms while the sweeps run
  __shared__ int rot_s[2];
  const int tid = (int)threadIdx.x, nth = (int)blockDim.x;
  double* G = use_lds ? etkf_smem : A;
  if (use_lds)
    for (int i = tid; i < M * M; i += nth) G[i] = A[i];
  __syncthreads();
  const int sweeps = etkf_eig_solve(M, G, gvec, mu_out, Tout, wout, f_s, h_s, n_s, rot_s, tid, nth);
  if (tid == 0) *sweeps_out = (double)sweeps;
}

int etkf_grid(long work_waves) {
  const long b = (work_waves + 3) / 4;
  return (int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

}  // namespace

int etkf_tiles(int M) {
  const int T = (M + 1 + 15) / 16;
  return T * (T + 1) / 2;
}

int etkf_streams(int M, long P) {
  const long nchunks = (P + kEtkfRows - 1) / kEtkfRows;
  long S = kEtkfWaveCap / etkf_tiles(M);
  if (S > kEtkfStreamCap) S = kEtkfStreamCap;
  if (S > nchunks) S = nchunks;
  return (int)(S < 1 ? 1 : S);
}

size_t etkf_ws_doubles(int M, long P) {
  // sc [P] | dt [P] | A [M][M] | g [M] | q, sweeps [2] | mu [M] | part [S][ntiles][256]
  return 2 * (size_t)P + (size_t)M * M + 2 * (size_t)M + 2 + (size_t)etkf_streams(M, P) * etkf_tiles(M) * 256;
}

EtkfWs etkf_ws(double* base, int M, long P) {
  EtkfWs w;
  w.sc = base;
  w.dt = w.sc + P;
  w.A = w.dt + P;
  w.g = w.A + (size_t)M * M;
  w.q = w.g + M;
  w.sweeps = w.q + 1;
  w.mu = w.sweeps + 1;
  w.part = w.mu + M;
  return w;
}

hipError_t launch_etkf_prior(long P, int M, const double* Yp, const double* ym, const double* ob_value, const double* ob_error,
                             const uint8_t* ob_assim, double* prior_mean, double* prior_var, uint8_t* assimilated, const EtkfWs& w,
                             hipStream_t s) {
  if (M < 2 || M > kMaxMembers || P < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_etkf_prior, dim3(etkf_grid(P)), dim3(256), 0, s, P, M, Yp, ym, ob_value, ob_error, ob_assim, prior_mean,
                     prior_var, assimilated, w.sc, w.dt);
  return hipGetLastError();
}

hipError_t launch_etkf_post(long P, int M, const double* Yw, const double* ymw, double* post_mean, double* post_var, hipStream_t s) {
  if (M < 2 || M > kMaxMembers || P < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_etkf_post, dim3(etkf_grid(P)), dim3(256), 0, s, P, M, Yw, ymw, post_mean, post_var);
  return hipGetLastError();
}

hipError_t launch_etkf_solve(long P, int M, const double* Yp, const EtkfWs& w, double* Tout, double* wout, hipStream_t s) {
  if (M < 2 || M > kMaxMembers || P < 1) return hipErrorInvalidValue;
  const int T = (M + 1 + 15) / 16, ntiles = etkf_tiles(M), S = etkf_streams(M, P);
  hipLaunchKernelGGL(k_etkf_gram, dim3((unsigned)((ntiles + 3) / 4), (unsigned)S), dim3(256), 0, s, P, M, T, ntiles, S, Yp, w.sc, w.dt,
                     w.part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_etkf_reduce, dim3((unsigned)ntiles), dim3(256), 0, s, M, T, ntiles, S, w.part, w.A, w.g, w.q);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int use_lds = M <= kEtkfLdsMaxM ? 1 : 0;
  const size_t lds = use_lds ? (size_t)M * M * sizeof(double) : 0;
  if (lds > 48 * 1024) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_etkf_eig), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const int npairs = (M + (M & 1)) / 2;
  int nth = 64 * ((16 * npairs + 63) / 64);
  if (nth > 1024) nth = 1024;
  hipLaunchKernelGGL(k_etkf_eig, dim3(1), dim3((unsigned)nth), lds, s, M, use_lds, w.A, w.g, w.mu, Tout, wout, w.sweeps);
  return hipGetLastError();
}

}  // namespace efa
