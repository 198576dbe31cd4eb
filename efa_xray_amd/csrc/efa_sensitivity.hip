// Ensemble sensitivity and greedy observation targeting (Ancell & Hakim 2007, Torn & Hakim 2008).
//   var_i = x'_i.x'_i/(M-1), cov_ik = x'_i.J'_k/(M-1) for every state row i and K forecast metrics, and -- one pick after the other,
//   each conditioning on the ones before by the exact, unlocalised Kalman update -- the row whose observation would reduce
//   sum_k w_k var(J_k) most.  Conditioning on picks 0..t-1 needs only the dots of the RAW row with u_0..u_{t-1} (u_s = G_s y_s, kept
//   on the host with the M x M matrix G), so a pass is stateless: it reads every row once, forms K + t dots and the row's sum of
//   squares, and keeps nothing of the size of the state between passes.
//
// k_sens_pass is a (rows x M) . (M x (K + t)) float64 contraction on the matrix cores, in the form of k_transform (efa_transform.hip):
//   - the rows are read in the four-lane row layout (efa_quadrow.h, with its zero padding of the last chunk): HBM -> VGPR -> MFMA,
//     the whole row in registers up to 256 members (2 NU doubles per lane), so the mean is removed from the registers and no row
//     is read twice;
//   - the vectors [J'_1..J'_K, u_0..u_{t-1}]/(M-1) live in LDS, once per workgroup, in MFMA-B order: one or two tiles of 16;
//   - v_mfma_f64_16x16x4_f64 leaves D[row (lane>>4) + 4 v][vector lane&15] in acc[v]; the wave turns that through LDS so that lane
//     (n, g) holds row n again and forms the conditioned var, the cov of metrics g, g+4, ... and the score, whose stores
//     [K][rows] run along the rows;
//   - the best (score, row) per workgroup is found by comparison only (larger score, then lower row: a total order, so the
//     result does not depend on how the comparisons are bracketed); k_sens_best reduces the workgroups' bests.  No atomics.
#include "efa_device.h"
#include "efa_diag.h"
#include "efa_quadrow.h"

#include <cmath>
#include <vector>

namespace efa {
namespace {

typedef double sens_v4 __attribute__((ext_vector_type(4)));

constexpr int kSensThreads = 256;  // 4 waves, one 16-row tile per wave and trip
constexpr int kSensBlocks = 1024;  // grid cap of k_sens_pass: 65536 rows per trip
constexpr int kSensVec = 32;       // K + n_targets at most: two MFMA tiles of 16 vectors
constexpr int kSensRLds = 256;     // slab errors staged in LDS up to here; beyond, read from memory
constexpr int kSensDS = 33;        // doubles per row of the turned D tile (padded against bank conflicts)
// the pack a pass stages (doubles): vectors [kSensVec][M] | b/d [kSensVec][kSensVec] | 1/d | weights | varJ (kSensVec each)
constexpr int kSensAux = kSensVec * kSensVec + 3 * kSensVec;

struct SensArgs {
  const void* X;
  long rows, ncol, n_lead;
  int M, K, t;
  const double* pack;
  const double* R;      // [n_lead]
  const uint8_t* cand;  // [rows] or null
  double *var, *cov, *sens, *corr, *dvar, *score;  // the final pass's fields (null: not wanted)
  double* best_score;   // per workgroup, or null: no pick wanted of this pass
  long* best_row;
};

// (a, ra) is a better pick than (b, rb): the larger score, the lower row among equals; a row of -1 is no pick (its score is 0)
__device__ __forceinline__ bool sens_better(double a, long ra, double b, long rb) {
  return a > b || (a == b && ra >= 0 && (rb < 0 || ra < rb));
}

// NU: chunks of 8 members ((M + 7) / 8).  AL: the rows are aligned for the paired loads (M even, base aligned to two elements).
template <int NU, bool AL, typename E>
__global__ __launch_bounds__(kSensThreads) void k_sens_pass(const SensArgs a) {
  extern __shared__ __align__(16) double sens_lds[];
  const int M = a.M, K = a.K, t = a.t, NV = K + t;
  const int NT = NV > 16 ? 2 : 1;
  const bool two = NT == 2;
  double* const Bs = sens_lds;                          // [2 NU steps][NT][64]
  double* const binv_s = Bs + (size_t)2 * NU * NT * 64;  // b_sk / d_s [s][kSensVec]
  double* const dinv_s = binv_s + kSensVec * kSensVec;
  double* const w_s = dinv_s + kSensVec;
  double* const vj_s = w_s + kSensVec;
  double* const R_s = vj_s + kSensVec;                  // [kSensRLds]
  double* const dots_s = R_s + kSensRLds;               // [4 waves][16 rows][kSensDS]; at the end the workgroup's (score, row)
  const int tid = threadIdx.x;
  const double Mm1 = (double)(M - 1);
  const double inv = 1.0 / Mm1;

  for (int i = tid; i < 2 * NU * NT * 64; i += kSensThreads) {
    const int l = i & 63, st = i >> 6;
    const int s = st / NT, j = 16 * (st % NT) + (l & 15);
    const int m = 8 * (s >> 1) + 2 * (l >> 4) + (s & 1);
    Bs[i] = (m < M && j < NV) ? a.pack[(size_t)j * M + m] * inv : 0.0;
  }
  for (int i = tid; i < kSensAux; i += kSensThreads) binv_s[i] = a.pack[(size_t)kSensVec * M + i];
  const bool r_lds = a.n_lead <= kSensRLds;
  if (r_lds)
    for (int i = tid; i < (int)a.n_lead; i += kSensThreads) R_s[i] = a.R[i];
  __syncthreads();
  const double* const Rp = r_lds ? R_s : a.R;

  const int lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const long ntiles = (a.rows + 15) / 16;
  const long nwaves = (long)gridDim.x * (kSensThreads / 64);
  const long last_row = a.rows - 1;
  const bool last_ok = 8 * (NU - 1) + 2 * g < M;  // this lane's two slots of the last chunk are real members?
  const bool last_ok1 = 8 * (NU - 1) + 2 * g + 1 < M;
  const bool final_pass = a.var || a.cov || a.sens || a.corr || a.dvar || a.score;
  double* const drow = dots_s + ((size_t)wv * 16 + n) * kSensDS;
  double best = 0.0;
  long brow = -1;

  for (long tile = (long)blockIdx.x * (kSensThreads / 64) + wv; tile < ntiles; tile += nwaves) {
    const long r = tile * 16 + n;
    double x[2 * NU];
    {  // clamped addresses, no branches: the loads of a tile are issued together
      const E* p = reinterpret_cast<const E*>(a.X) + (size_t)(r < last_row ? r : last_row) * M;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        int m0 = 8 * u + 2 * g;
        if (AL) {
          if (u == NU - 1) m0 = (m0 < M) ? m0 : M - 2;
          const typename ElemPair<E>::type v = *reinterpret_cast<const typename ElemPair<E>::type*>(p + m0);
          x[2 * u] = v.x;
          x[2 * u + 1] = v.y;
        } else {
          x[2 * u] = p[(m0 < M) ? m0 : M - 1];
          x[2 * u + 1] = p[(m0 + 1 < M) ? m0 + 1 : M - 1];
        }
      }
    }
    if (!last_ok) x[2 * NU - 2] = 0.0;
    if (!last_ok1) x[2 * NU - 1] = 0.0;
    // the row mean; a row whose members are all equal has deviations of exactly 0 (its sum / M need not give the member back)
    const double x0 = __shfl(x[0], n, 64);
    bool diff = false;
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 2 * NU; ++c) {
      s4[c & 3] += x[c];
      const bool ok = c < 2 * NU - 2 || ((c & 1) ? last_ok1 : last_ok);
      diff = diff || (ok && x[c] != x0);
    }
    const double sum = quad_row_sum((s4[0] + s4[1]) + (s4[2] + s4[3]));
    const double mean = quad_row_any(diff, n) ? sum / (double)M : x0;
    double q4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 2 * NU; ++c) {
      const bool ok = c < 2 * NU - 2 || ((c & 1) ? last_ok1 : last_ok);
      x[c] = ok ? x[c] - mean : 0.0;
      q4[c & 3] = __builtin_fma(x[c], x[c], q4[c & 3]);
    }
    const double ss = quad_row_sum((q4[0] + q4[1]) + (q4[2] + q4[3]));

    sens_v4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 2 * NU; ++s) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x[s], Bs[((size_t)s * NT) * 64 + lane], acc0, 0, 0, 0);
      if (two) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x[s], Bs[((size_t)s * NT + 1) * 64 + lane], acc1, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);  // (keeps the LDS reads from being hoisted together: registers)
    }
    // turn D: acc[v] is (row g + 4 v, vector n); afterwards lane (n, g) reads row n
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the previous tile's reads of this wave are done (one wave's LDS operations complete in order)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      double* d = dots_s + ((size_t)wv * 16 + g + 4 * v) * kSensDS;
      d[n] = acc0[v];
      if (two) d[16 + n] = acc1[v];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const bool live = r <= last_row;
    const double Ri = Rp[live ? r / a.ncol : 0];
    double var = ss / Mm1;
    for (int s = 0; s < t; ++s) {
      const double as = drow[K + s];
      var = __builtin_fma(-(as * as), dinv_s[s], var);
    }
    var = (var < 0.0) ? 0.0 : var;  // (a NaN stays)
    const double den = var + Ri;    // > 0, or NaN
    double num = 0.0;
    for (int k = g; k < K; k += 4) {
      double c = drow[k];
      for (int s = 0; s < t; ++s) c = __builtin_fma(-drow[K + s], binv_s[s * kSensVec + k], c);
      const double cc = c * c;
      num = __builtin_fma(w_s[k], cc, num);
      if (final_pass && live) {
        const size_t o = (size_t)k * a.rows + r;
        if (a.cov) a.cov[o] = c;
        if (a.sens) a.sens[o] = (var == 0.0) ? 0.0 : c / var;
        if (a.corr) {
          const double d2 = var * vj_s[k];
          a.corr[o] = (d2 > 0.0) ? c / sqrt(d2) : (d2 != d2 ? d2 : 0.0);
        }
        if (a.dvar) a.dvar[o] = -cc / den;
      }
    }
    num = quad_row_sum(num);
    if (g == 0 && live) {
      const bool cand = !a.cand || a.cand[r] != 0;
      const double sc = cand ? num / den : 0.0;
      if (a.var) a.var[r] = var;
      if (a.score) a.score[r] = sc;
      if (cand && sens_better(sc, r, best, brow) && sc > 0.0) {
        best = sc;
        brow = r;
      }
    }
  }

  if (!a.best_score) return;
  __syncthreads();  // every wave is done with dots_s
  double* const bs = dots_s;
  long* const br = reinterpret_cast<long*>(dots_s + kSensThreads);
  bs[tid] = best;
  br[tid] = brow;
  __syncthreads();
  for (int off = kSensThreads / 2; off >= 1; off >>= 1) {
    if (tid < off && sens_better(bs[tid + off], br[tid + off], bs[tid], br[tid])) {
      bs[tid] = bs[tid + off];
      br[tid] = br[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.best_score[blockIdx.x] = bs[0];
    a.best_row[blockIdx.x] = br[0];
  }
}

// the workgroups' bests -> entry nblk of the same arrays
__global__ __launch_bounds__(kSensThreads) void k_sens_best(int nblk, double* __restrict__ score, long* __restrict__ row) {
  __shared__ double bs[kSensThreads];
  __shared__ long br[kSensThreads];
  const int tid = threadIdx.x;
  double best = 0.0;
  long brow = -1;
  for (int i = tid; i < nblk; i += kSensThreads)
    if (sens_better(score[i], row[i], best, brow)) {
      best = score[i];
      brow = row[i];
    }
  bs[tid] = best;
  br[tid] = brow;
  __syncthreads();
  for (int off = kSensThreads / 2; off >= 1; off >>= 1) {
    if (tid < off && sens_better(bs[tid + off], br[tid + off], bs[tid], br[tid])) {
      bs[tid] = bs[tid + off];
      br[tid] = br[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    score[nblk] = bs[0];
    row[nblk] = br[0];
  }
}

size_t sens_lds_bytes(int NU, int NV) {
  const int NT = NV > 16 ? 2 : 1;
  return ((size_t)2 * NU * NT * 64 + kSensAux + kSensRLds + 4 * 16 * kSensDS) * sizeof(double);
}

int sens_grid(long rows) {
  long blocks = ((rows + 15) / 16 + 3) / 4;
  if (blocks > kSensBlocks) blocks = kSensBlocks;
  return (int)(blocks < 1 ? 1 : blocks);
}

template <int NU, bool AL, typename E>
hipError_t sens_launch(const SensArgs& a, hipStream_t s) {
  const size_t lds = sens_lds_bytes(NU, a.K + a.t);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sens_pass<NU, AL, E>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_sens_pass<NU, AL, E>), dim3((unsigned)sens_grid(a.rows)), dim3(kSensThreads), lds, s, a);
  return hipGetLastError();
}

// one pass over the state; with best_score the grid's best (score, row) ends up in entry sens_grid(rows) of best_score / best_row
hipError_t launch_sens_pass(const SensArgs& a, Elem elem, hipStream_t s) {
  if (a.M < 2 || a.M > kMaxMembers || a.K < 1 || a.t < 0 || a.K + a.t > kSensVec) return hipErrorInvalidValue;
  if (a.rows <= 0) return hipSuccess;
  const bool al = efa_host::pairs_aligned(a.X, a.M, elem);
  hipError_t e = dispatch_width((a.M + 7) / 8, WidthRange<1, kMaxMembers / 8>{}, [&](auto nu_c) {
    constexpr int nu = decltype(nu_c)::value;
    if (elem == Elem::f32) return al ? sens_launch<nu, true, float>(a, s) : sens_launch<nu, false, float>(a, s);
    return al ? sens_launch<nu, true, double>(a, s) : sens_launch<nu, false, double>(a, s);
  });
  if (e != hipSuccess) return e;
  if (a.best_score) {
    hipLaunchKernelGGL(k_sens_best, dim3(1), dim3(kSensThreads), 0, s, sens_grid(a.rows), a.best_score, a.best_row);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace
}  // namespace efa

// ---- the host side of efa_sensitivity_dev / efa_sensitivity_f32_dev ------------------------------------------------------------
namespace efa_host {

using namespace efa;

// Everything the call needs lives in buffers of its own (sens_*): like efa_obs_impact_dev it neither reads nor writes what a later
// cycle reads.  Between passes the host holds G (M x M, G_0 = I) and, for pick t of row i_t with raw deviations y_t:
//   u_t = G_t y_t, d_t = y_t.u_t/(M-1) + R, b_tk = J'_k.u_t/(M-1), G_{t+1} = G_t - u_t u_t^T/((M-1) d_t), varJ_k -= b_tk^2/d_t
// every sum in index order.
int sensitivity(efa_ctx* c, Elem elem, long rows, int M, int K, const void* X_dev, const double* J, long ncol, long n_lead,
                const double* slab_error, const double* weights, const uint8_t* cand_dev, int n_targets, double* var_dev,
                double* cov_dev, double* sens_dev, double* corr_dev, double* dvar_dev, double* score_dev, long* picked_row,
                double* picked_score, double* metric_var) {
  const char* me = elem == Elem::f32 ? "efa_sensitivity_f32_dev" : "efa_sensitivity_dev";
  if (M < 2 || M > kMaxMembers) return fail(EFA_ERR_INVALID, "%s: M=%d must be in [2,%d]", me, M, kMaxMembers);
  if (K < 1 || n_targets < 0 || K + n_targets > kSensVec)
    return fail(EFA_ERR_INVALID, "%s: K=%d metrics and n_targets=%d picks: need K >= 1, n_targets >= 0 and K + n_targets <= %d", me, K,
                n_targets, kSensVec);
  if (rows < 0 || ncol < 0 || n_lead < 0) return fail(EFA_ERR_INVALID, "%s: negative size", me);
  if (ncol * n_lead != rows) return fail(EFA_ERR_INVALID, "%s: rows=%ld must equal n_lead*ncol = %ld*%ld", me, rows, n_lead, ncol);
  if (!J) return fail(EFA_ERR_INVALID, "%s: null metrics J", me);
  if (n_lead > 0 && !slab_error) return fail(EFA_ERR_INVALID, "%s: null slab_error", me);
  if (rows > 0 && !X_dev) return fail(EFA_ERR_INVALID, "%s: null device pointer", me);
  if (n_targets > 0 && (!picked_row || !picked_score || !metric_var))
    return fail(EFA_ERR_INVALID, "%s: n_targets=%d needs picked_row, picked_score and metric_var", me, n_targets);
  for (long i = 0; i < (long)K * M; ++i)
    if (!std::isfinite(J[i])) return fail(EFA_ERR_INVALID, "%s: metric %ld, member %ld is not finite", me, i / M, i % M);
  for (long s = 0; s < n_lead; ++s)
    if (!(std::isfinite(slab_error[s]) && slab_error[s] > 0.0))
      return fail(EFA_ERR_INVALID, "%s: slab_error[%ld] = %g is not finite and > 0", me, s, slab_error[s]);
  if (weights)
    for (int k = 0; k < K; ++k)
      if (!(std::isfinite(weights[k]) && weights[k] >= 0.0))
        return fail(EFA_ERR_INVALID, "%s: weights[%d] = %g is not finite and >= 0", me, k, weights[k]);

  c->sens_us = 0;
  const double Mm1 = (double)(M - 1);
  // the pack of a pass, as k_sens_pass stages it
  std::vector<double> pack((size_t)kSensVec * M + kSensAux, 0.0);
  double *vec = pack.data(), *binv = vec + (size_t)kSensVec * M, *dinv = binv + kSensVec * kSensVec, *w = dinv + kSensVec,
         *varJ = w + kSensVec;
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
    for (int m = 0; m < M; ++m) s += J[(size_t)k * M + m];
    const double mean = s / (double)M;
    double q = 0.0;
    for (int m = 0; m < M; ++m) {
      const double d = J[(size_t)k * M + m] - mean;
      vec[(size_t)k * M + m] = d;
      q += d * d;
    }
    varJ[k] = q / Mm1;
    w[k] = weights ? weights[k] : 1.0;
  }
  if (metric_var)
    for (int k = 0; k < K; ++k) metric_var[k] = varJ[k];
  const bool fields = var_dev || cov_dev || sens_dev || corr_dev || dvar_dev || score_dev;
  int t = 0;
  if (rows > 0 && (n_targets > 0 || fields)) {
    hipStream_t s = c->stream;
    const int nblk = sens_grid(rows);
    const size_t pack_bytes = pack.size() * sizeof(double);
    EFA_TRY(c->sens_pack.reserve(pack_bytes + (size_t)n_lead * sizeof(double)));
    EFA_TRY(c->sens_best.reserve((size_t)(nblk + 1) * (sizeof(double) + sizeof(long))));
    double* d_pack = c->sens_pack.as<double>();
    double* d_R = d_pack + pack.size();
    double* d_bs = c->sens_best.as<double>();
    long* d_br = reinterpret_cast<long*>(d_bs + nblk + 1);
    EFA_HIP(hipMemcpyAsync(d_R, slab_error, (size_t)n_lead * sizeof(double), hipMemcpyHostToDevice, s));
    SensArgs a{};
    a.X = X_dev;
    a.rows = rows;
    a.ncol = ncol;
    a.n_lead = n_lead;
    a.M = M;
    a.K = K;
    a.pack = d_pack;
    a.R = d_R;
    a.cand = cand_dev;
    double ms_sum = 0.0;
    auto one_pass = [&]() -> int {  // uploads the pack, runs the pass between the two events, waits and adds its time
      EFA_HIP(hipMemcpyAsync(d_pack, pack.data(), pack_bytes, hipMemcpyHostToDevice, s));
      EFA_TRY(interval_begin(c->sens_iv, s));
      EFA_HIP(launch_sens_pass(a, elem, s));
      EFA_TRY(interval_end(c->sens_iv, s));
      return EFA_OK;
    };
    auto pass_time = [&]() -> int {
      float ms = 0.f;
      EFA_HIP(hipEventElapsedTime(&ms, c->sens_iv.begin, c->sens_iv.end));
      ms_sum += (double)ms;
      return EFA_OK;
    };
    std::vector<double> G, y(M), u(M);
    std::vector<char> rowbuf((size_t)M * elem_size(elem));
    if (n_targets > 0) {
      G.assign((size_t)M * M, 0.0);
      for (int m = 0; m < M; ++m) G[(size_t)m * M + m] = 1.0;
    }
    for (; t < n_targets; ++t) {
      a.t = t;
      a.best_score = d_bs;
      a.best_row = d_br;
      EFA_TRY(one_pass());
      double sc = 0.0;
      long row = -1;
      EFA_HIP(hipMemcpyAsync(&sc, d_bs + nblk, sizeof(double), hipMemcpyDeviceToHost, s));
      EFA_HIP(hipMemcpyAsync(&row, d_br + nblk, sizeof(long), hipMemcpyDeviceToHost, s));
      EFA_HIP(hipStreamSynchronize(s));
      EFA_TRY(pass_time());
      if (row < 0 || row >= rows || !(sc > 0.0)) break;  // no candidate scores > 0: the picks stop
      EFA_HIP(hipMemcpyAsync(rowbuf.data(), static_cast<const char*>(X_dev) + (size_t)row * M * elem_size(elem), rowbuf.size(),
                             hipMemcpyDeviceToHost, s));
      EFA_HIP(hipStreamSynchronize(s));
      double sum = 0.0;
      for (int m = 0; m < M; ++m) {
        y[m] = elem == Elem::f32 ? (double)reinterpret_cast<const float*>(rowbuf.data())[m] : reinterpret_cast<const double*>(rowbuf.data())[m];
        sum += y[m];
      }
      const double mean = sum / (double)M;
      for (int m = 0; m < M; ++m) y[m] -= mean;
      double yu = 0.0;
      for (int i = 0; i < M; ++i) {
        double acc = 0.0;
        for (int m = 0; m < M; ++m) acc += G[(size_t)i * M + m] * y[m];
        u[i] = acc;
      }
      for (int m = 0; m < M; ++m) yu += y[m] * u[m];
      const double d = yu / Mm1 + slab_error[row / ncol];
      for (int k = 0; k < K; ++k) {
        double b = 0.0;
        for (int m = 0; m < M; ++m) b += vec[(size_t)k * M + m] * u[m];
        b /= Mm1;
        binv[t * kSensVec + k] = b / d;
        varJ[k] -= b * b / d;
      }
      dinv[t] = 1.0 / d;
      for (int i = 0; i < M; ++i)
        for (int m = 0; m < M; ++m) G[(size_t)i * M + m] -= u[i] * u[m] / (Mm1 * d);
      for (int m = 0; m < M; ++m) vec[(size_t)(K + t) * M + m] = u[m];
      picked_row[t] = row;
      picked_score[t] = sc;
      for (int k = 0; k < K; ++k) metric_var[(size_t)(t + 1) * K + k] = varJ[k];
    }
    if (fields) {  // the fields, conditioned on the t picks made
      a.t = t;
      a.best_score = nullptr;
      a.best_row = nullptr;
      a.var = var_dev;
      a.cov = cov_dev;
      a.sens = sens_dev;
      a.corr = corr_dev;
      a.dvar = dvar_dev;
      a.score = score_dev;
      EFA_TRY(one_pass());
      EFA_HIP(hipStreamSynchronize(s));
      EFA_TRY(pass_time());
    }
    c->sens_us = (long)std::llround(ms_sum * 1000.0);
  }
  for (int i = t; i < n_targets; ++i) {  // the picks that were not made: the trajectory repeats its last row
    picked_row[i] = -1;
    picked_score[i] = 0.0;
    for (int k = 0; k < K; ++k) metric_var[(size_t)(i + 1) * K + k] = varJ[k];
  }
  return EFA_OK;
}

}  // namespace efa_host
