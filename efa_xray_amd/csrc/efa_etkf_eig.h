// The ensemble-space eigen-solve shared by k_etkf_eig (efa_etkf.hip, one solve for all obs) and k_letkf (efa_letkf.hip, one solve per
// column): A = V diag(mu) V^T by parallel cyclic one-sided (Hestenes) Jacobi, then the factor vectors of T = V diag(f) V^T and
// w = V h.  One workgroup of `nth` threads (a multiple of 64; 16 lanes per column pair); G is the M x M array, column j at G + j M,
// in LDS or in global memory: the code is the same.  Every barrier below is reached by all `nth` threads.
#pragma once
#include "efa_device.h"
#include "efa_internal.h"
#include "efa_rows.h"

namespace efa {

constexpr double kEtkfRotTol = 8.8817841970012523e-16;  // 2^-50

// The sweeps: round-robin rounds of M/2 disjoint column pairs, a rotation when |gamma| > 2^-50 sqrt(alpha beta) (the squared norms
// alpha, beta recomputed once per sweep in n_s [M] and updated by every rotation; only gamma is a dot product per pair).  A counted
// loop (kEtkfSweepCap) that a sweep without a rotation leaves early; a NaN never satisfies the test, so a NaN block ends after one
// sweep with NaNs.  rot_s [2] and n_s are LDS scratch.  Returns the sweeps taken (uniform).
__device__ __forceinline__ int etkf_jacobi(int M, double* G, double* n_s, int* rot_s, int tid, int nth) {
  const int n = M + (M & 1), npairs = n / 2, nslots = nth >> 4, slot = tid >> 4, sl = tid & 15;
  int sweeps = 0;
#pragma unroll 1
  for (int sw = 0; sw < kEtkfSweepCap; ++sw) {
    if (tid == 0) rot_s[sw & 1] = 0;
    // the squared column norms, afresh once per sweep; a rotation then updates its two (alpha - t gamma, beta + t gamma)
#pragma unroll 1
    for (int j = slot; j < M; j += nslots) {
      const double* cj = G + (size_t)j * M;
      double al = 0.0;
      for (int i = sl; i < M; i += 16) al = fma(cj[i], cj[i], al);
      al = group_sum<16>(al);
      if (sl == 0) n_s[j] = al;
    }
    __syncthreads();
#pragma unroll 1
    for (int r = 0; r < n - 1; ++r) {
#pragma unroll 1
      for (int pi = slot; pi < npairs; pi += nslots) {
        int p = n - 1, q = r;
        if (pi != 0) {
          p = r + pi;
          if (p >= n - 1) p -= n - 1;
          q = r - pi;
          if (q < 0) q += n - 1;
        }
        if (p >= M || q >= M) continue;  // (an odd M plays against a bye)
        double* cp = G + (size_t)p * M;
        double* cq = G + (size_t)q * M;
        double ga = 0.0;
        for (int i = sl; i < M; i += 16) ga = fma(cp[i], cq[i], ga);
        ga = group_sum<16>(ga);  // a butterfly: the 16 lanes hold the same bits
        const double al = n_s[p], be = n_s[q];
        if (ga * ga > (kEtkfRotTol * kEtkfRotTol) * (al * be)) {  // |gamma| > 2^-50 sqrt(alpha beta); false for a NaN
          const double d = be - al;
          const double t = copysign(2.0, d) * ga / (fabs(d) + sqrt(fma(d, d, 4.0 * (ga * ga))));
          const double c = rsqrt(fma(t, t, 1.0));
          const double s = c * t;
          for (int i = sl; i < M; i += 16) {
            const double x = cp[i], y = cq[i];
            cp[i] = c * x - s * y;
            cq[i] = s * x + c * y;
          }
          if (sl == 0) {
            n_s[p] = al - t * ga;
            n_s[q] = be + t * ga;
            rot_s[sw & 1] = 1;
          }
        }
      }
      __syncthreads();
    }
    sweeps = sw + 1;
    if (rot_s[sw & 1] == 0) break;  // (uniform: read behind the round's barrier; the next sweep clears the other word)
  }
  return sweeps;
}

// Behind the sweeps: the column norms mu (to mu_out [M]), V in place of G, and the two factor vectors f_s [M] = sqrt((M-1)/mu_j),
// h_s [M] = (V_j . g) / mu_j.  Ends with a barrier.
__device__ __forceinline__ void etkf_factors(int M, double* G, const double* gvec, double* mu_out, double* f_s, double* h_s, int tid,
                                             int nth) {
  const int nslots = nth >> 4, slot = tid >> 4, sl = tid & 15;
#pragma unroll 1
  for (int j = slot; j < M; j += nslots) {
    double* cj = G + (size_t)j * M;
    double al = 0.0, hg = 0.0;
    for (int i = sl; i < M; i += 16) {
      const double x = cj[i];
      al = fma(x, x, al);
      hg = fma(x, gvec[i], hg);
    }
    al = group_sum<16>(al);
    hg = group_sum<16>(hg);
    const double mu = sqrt(al);
    for (int i = sl; i < M; i += 16) cj[i] = cj[i] / mu;
    if (sl == 0) {
      mu_out[j] = mu;
      f_s[j] = sqrt((double)(M - 1) / mu);
      h_s[j] = (hg / mu) / mu;
    }
  }
  __syncthreads();
}

// T[a][b] = sum_j f_j V[a][j] V[b][j] for a <= b, mirrored, to Tout (rows `ldt` doubles apart); w[a] = sum_j h_j V[a][j] to wout
// (elements `ldw` doubles apart)
__device__ __forceinline__ void etkf_assemble(int M, const double* G, const double* f_s, const double* h_s, double* Tout, size_t ldt,
                                              double* wout, size_t ldw, int tid, int nth) {
#pragma unroll 1
  for (int e = tid; e < M * M; e += nth) {
    const int a = e / M, b = e - a * M;
    if (a > b) continue;
    double acc = 0.0;
    for (int j = 0; j < M; ++j) acc = fma(f_s[j] * G[(size_t)j * M + a], G[(size_t)j * M + b], acc);
    Tout[(size_t)a * ldt + b] = acc;
    Tout[(size_t)b * ldt + a] = acc;
  }
  for (int a = tid; a < M; a += nth) {
    double acc = 0.0;
    for (int j = 0; j < M; ++j) acc = fma(h_s[j], G[(size_t)j * M + a], acc);
    wout[(size_t)a * ldw] = acc;
  }
}

// The whole solve as k_etkf_eig runs it.  Returns the sweeps taken.
__device__ __forceinline__ int etkf_eig_solve(int M, double* G, const double* gvec, double* mu_out, double* Tout, double* wout,
                                              double* f_s, double* h_s, double* n_s, int* rot_s, int tid, int nth) {
  const int sweeps = etkf_jacobi(M, G, n_s, rot_s, tid, nth);
  etkf_factors(M, G, gvec, mu_out, f_s, h_s, tid, nth);
  etkf_assemble(M, G, f_s, h_s, Tout, (size_t)M, wout, 1, tid, nth);
  return sweeps;
}

}  // namespace efa
