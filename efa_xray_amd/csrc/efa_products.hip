// Ensemble products and probability verification (Murphy 1973).
//   For every state row i = lead*ncol + col with members x_i1..x_iM: the mean, the standard deviation, up to 8 quantiles (numpy's
//   linear rule on the sorted members) and up to 8 exceedance probabilities k/M, k = #{m: x_im > t}, with thresholds per slab; and,
//   given a verifying value y_i, per group of slabs and threshold the reliability table table[k][o] of o = (y_i > t), the count of
//   bad rows and the weighted sums of 1, (k/M - o)^2, k/M and o.  Every number in float64.
//
// k_products reads every row once in the four-lane row layout (efa_quadrow.h): the whole row sits in registers, 2 NU doubles per
// lane.  Slots beyond M hold +inf.  Sum, sum of squared deviations and the counts are lane-local plus two __shfl_xor steps; the count is taken as
// M - #{slot <= t}, which the +inf slots never enter and which equals #{x > t} on a row without NaN (a row with one is bad).  The
// counts of a lane travel as 16-bit fields of two 64-bit words, so the 8 thresholds cost 4 shuffles, and lane g of a row then does
// the work of thresholds g and g + 4 (the division, the stores, the table, the sums).
//
// SORT = true (a call that wants quantiles) sorts the members with the network of efa_sortnet.h: afterwards sorted position j is
// slot j % LP of lane j / LP.  lo and hi of a level depend on q and M only and are wave-uniform: the slot is picked by an unrolled
// compare-and-select chain over compile-time register indices and fetched from the owning lane with __shfl.  SORT = false never
// instantiates the network.
//
// Sums: a chunk is kProdChunkTiles tiles of one slab, whatever the grid; wave w takes its tiles w, w+4, ... in order, every lane
// adds its rows up, and the 64 lane sums of the chunk are added in index order into the chunk's partial.  k_group_reduce (efa_quadreduce.h) adds
// the partials of each group in a fixed order.  The table is integer adds in LDS and integer atomics in memory.  No
// floating-point atomics: the same inputs give the same bits whatever the grid.
#include "efa_device.h"
#include "efa_diag.h"
#include "efa_quadreduce.h"
#include "efa_sortnet.h"

#include <cmath>
#include <vector>

namespace efa {
namespace {

constexpr int kProdBlocks = 2048;     // default grid cap of k_products (option "products_blocks" lowers it)
constexpr int kProdChunkTiles = 64;   // tiles per chunk: 1024 rows give one partial
constexpr int kProdMax = 8;           // quantile levels and thresholds per call
constexpr int kProdSums = 4;          // sum w, w (p - o)^2, w p, w o
constexpr long kProdFlushChunks = 1L << 20;  // the LDS table (32-bit) goes to memory at least this often: < 2^31 rows

struct ProdArgs {
  const void* X;
  const double* verif;   // [rows] or null: no verification
  const double* colw;    // [ncol] or null
  const int* sgroup;     // [n_lead], device copy (all -1 without verification)
  const double* thr;     // [n_lead][kProdMax], device copy, NaN beyond nt
  long ncol, n_lead, rows;
  long nchunks, cps;     // chunks in all, chunks per slab
  int M, al;             // al: the rows are aligned for the paired loads
  int nq, nt;
  int qlo[kProdMax], qhi[kProdMax];
  double qf[kProdMax];
  double *mean, *sd;     // [rows] each, or null
  double* quant;         // [nq][rows] or null
  double* prob;          // [nt][rows] or null
  double* part;          // [nchunks][kProdMax][kProdSums]
  long long* cnt;        // [nchunks][kProdMax]: bad rows that would be scored
  unsigned long long* table;  // [G][nt][M + 1][2]
};

// slot `slot` (wave-uniform) of d: a chain of selects over compile-time indices, never an indexed register array
template <int LP>
__device__ __forceinline__ double prod_pick(const double (&d)[LP], int slot) {
  double v = d[0];
#pragma unroll
  for (int k = 1; k < LP; ++k) {
    const double dk = d[k];  // (read first: a slot read only under the condition becomes an indexed read, and the row goes to scratch)
    v = (slot == k) ? dk : v;
  }
  return v;
}

// NU: chunks of 8 members the lanes hold, (M + 7) / 8 rounded up to a power of two, as in k_verify
template <int NU, typename E, bool SORT>
__global__ __launch_bounds__(kQuadThreads) void k_products(const ProdArgs a) {
  constexpr int LP = 2 * NU;
  static_assert((NU & (NU - 1)) == 0, "the bitonic network needs a power of two");
  __shared__ unsigned int tab_s[kProdMax * (kMaxMembers + 1) * 2];
  __shared__ double red_s[kQuadThreads * 2 * kProdSums];
  __shared__ int cnt_s[kQuadThreads * 2];
  const int M = a.M;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const double inf = __builtin_inf();
  const double nan = __builtin_nan("");
  const double dM = (double)M;
  const long tps = (a.ncol + 15) / 16;
  const bool ver = a.verif != nullptr;
  const int ntab = a.nt * (M + 1) * 2;

  if (ver) {
    for (int i = tid; i < ntab; i += kQuadThreads) tab_s[i] = 0u;
    __syncthreads();
  }
  int cur_g = -1;  // the group the LDS table belongs to
  long since = 0;

#pragma unroll 1
  for (long ch = blockIdx.x; ch < a.nchunks; ch += gridDim.x) {
    const long lead = ch / a.cps, cc = ch % a.cps;
    const int sg = ver ? a.sgroup[lead] : -1;
    if (ver && (sg != cur_g || since >= kProdFlushChunks)) {  // (uniform)
      __syncthreads();
      if (cur_g >= 0)
        for (int i = tid; i < ntab; i += kQuadThreads) {
          const unsigned int v = tab_s[i];
          if (v) atomicAdd(&a.table[(size_t)cur_g * ntab + i], (unsigned long long)v);
          tab_s[i] = 0u;
        }
      __syncthreads();
      cur_g = sg;
      since = 0;
    }
    ++since;
    const long t0 = cc * kProdChunkTiles;
    const long t1 = (t0 + kProdChunkTiles < tps) ? t0 + kProdChunkTiles : tps;
    const double* thr = a.thr + (size_t)lead * kProdMax;
    // the two thresholds this lane finishes: j = g and g + 4
    const double tj0 = thr[g], tj1 = thr[g + 4];
    double acc[2][kProdSums] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    int n_bad[2] = {0, 0};

#pragma unroll 1
    for (long tl = t0 + wv; tl < t1; tl += kQuadThreads / 64) {
      const long col = tl * 16 + n;
      const bool live = col < a.ncol;
      const long colc = live ? col : a.ncol - 1;
      const long r = lead * a.ncol + colc;
      const int gq = quad_lane_quarter(lane);
      // The loader, the slot predicate and the row reductions are written out here, not taken from efa_quadrow.h, and so are the
      // table flush and the chunk partial of efa_quadreduce.h below: with the former the quantile variants ran 6 % slower, with the
      // latter the float32 variants up to 0.9 %.  As it stands the kernel is its predecessor's code.
      double d[LP];
      {  // clamped addresses, no branches: the loads of a tile are issued together
        const E* p = reinterpret_cast<const E*>(a.X) + (size_t)r * M;
        if (a.al) {
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            int m0 = 8 * u + 2 * gq;
            m0 = (m0 < M) ? m0 : M - 2;
            const typename ElemPair<E>::type v = *reinterpret_cast<const typename ElemPair<E>::type*>(p + m0);
            d[2 * u] = v.x;
            d[2 * u + 1] = v.y;
          }
        } else {
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            const int m0 = 8 * u + 2 * gq;
            d[2 * u] = p[(m0 < M) ? m0 : M - 1];
            d[2 * u + 1] = p[(m0 + 1 < M) ? m0 + 1 : M - 1];
          }
        }
      }
      double y = nan, w = 1.0;
      if (ver) {
        y = a.verif[r];
        if (a.colw) w = a.colw[colc];
      }
      bool badl = false;
      double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < LP; ++c) {
        const bool ok = 8 * (c >> 1) + 2 * gq + (c & 1) < M;  // the slot holds a real member
        const double xv = d[c];
        badl = badl || (ok && !finite64(xv));
        s4[c & 3] += ok ? xv : 0.0;
        d[c] = ok ? xv : inf;
      }
      const double x0 = __shfl(d[0], n, 64);  // member 0
      bool diff = false;
#pragma unroll
      for (int c = 0; c < LP; ++c) {
        const bool ok = 8 * (c >> 1) + 2 * gq + (c & 1) < M;
        diff = diff || (ok && d[c] != x0);
      }
      double sum = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      const bool varies = quad_row_any(diff, n);
      const bool bad = quad_row_any(badl, n);
      // a row whose members are all equal has that value as its mean and deviations of exactly 0 (its sum / M need not give it back)
      const double mean = varies ? sum / dM : x0;
      double q4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < LP; ++c) {
        const bool ok = 8 * (c >> 1) + 2 * gq + (c & 1) < M;
        const double e = ok ? d[c] - mean : 0.0;
        q4[c & 3] = __builtin_fma(e, e, q4[c & 3]);
      }
      double ss = (q4[0] + q4[1]) + (q4[2] + q4[3]);
      ss += __shfl_xor(ss, 16, 64);
      ss += __shfl_xor(ss, 32, 64);
      const double sd = __builtin_sqrt(ss / (double)(M - 1));

      // #{slot <= t} of every threshold, 16 bits each: thresholds 0..3 in pk0, 4..7 in pk1
      unsigned long long pk0 = 0ull, pk1 = 0ull;
#pragma unroll 1
      for (int j = 0; j < a.nt; ++j) {
        const double t = thr[j];  // (uniform)
        int cle = 0;
#pragma unroll
        for (int c = 0; c < LP; ++c) cle += (d[c] <= t) ? 1 : 0;
        const unsigned long long v = (unsigned long long)cle << (16 * (j & 3));
        if (j < 4) pk0 += v;
        else pk1 += v;
      }
      pk0 += __shfl_xor(pk0, 16, 64);
      pk0 += __shfl_xor(pk0, 32, 64);
      pk1 += __shfl_xor(pk1, 16, 64);
      pk1 += __shfl_xor(pk1, 32, 64);

      if (gq == 0 && live && a.mean) a.mean[r] = bad ? nan : mean;
      if (gq == 1 && live && a.sd) a.sd[r] = bad ? nan : sd;

#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int j = gq + 4 * s;
        const double t = s ? tj1 : tj0;
        const int k = M - (int)(((s ? pk1 : pk0) >> (16 * gq)) & 0xFFFFull);
        const double p = (double)k / dM;
        const bool tfin = finite64(t);
        if (live && j < a.nt) {
          if (a.prob) a.prob[(size_t)j * a.rows + r] = (tfin && !bad) ? p : nan;
          if (ver && sg >= 0 && tfin && finite64(y) && w > 0.0) {
            if (bad) {
              ++n_bad[s];
            } else {
              const int o = (y > t) ? 1 : 0;
              atomicAdd(&tab_s[(j * (M + 1) + k) * 2 + o], 1u);
              const double e = p - (double)o;
              acc[s][0] += w;
              acc[s][1] += w * (e * e);
              acc[s][2] += w * p;
              acc[s][3] += w * (double)o;
            }
          }
        }
      }

      if constexpr (SORT) {
        quad_sort<LP>(d, gq);  // afterwards sorted position g LP + k is slot k of lane g
#pragma unroll 1
        for (int i = 0; i < a.nq; ++i) {
          const int lo = a.qlo[i], hi = a.qhi[i];  // (uniform)
          const double f = a.qf[i];
          const double vlo = __shfl(prod_pick<LP>(d, lo & (LP - 1)), (lo / LP) * 16 + n, 64);
          const double vhi = __shfl(prod_pick<LP>(d, hi & (LP - 1)), (hi / LP) * 16 + n, 64);
          const double v = (f == 0.0) ? vlo : __builtin_fmin(vhi, __builtin_fma(f, vhi - vlo, vlo));
          if (gq == (i & 3) && live) a.quant[(size_t)i * a.rows + r] = bad ? nan : v;
        }
      }
    }

    if (ver) {
      // the chunk's partial: for every threshold the 64 lane sums (wave, row lane) in index order
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int k = 0; k < kProdSums; ++k) red_s[(tid * 2 + s) * kProdSums + k] = acc[s][k];
        cnt_s[tid * 2 + s] = n_bad[s];
      }
      __syncthreads();
      // threshold j was finished by lane quarter j & 3 as its s = j >> 2: lane sum i is thread (i >> 4) * 64 + (j & 3) * 16 + (i & 15)
      // (the text of quad_chunk_partial)
      if (tid < kProdMax * kProdSums) {
        const int j = tid / kProdSums, k = tid % kProdSums;
        double sacc = 0.0;
        for (int i = 0; i < 64; ++i) sacc += red_s[((((i >> 4) * 64 + (j & 3) * 16 + (i & 15)) * 2) + (j >> 2)) * kProdSums + k];
        a.part[((size_t)ch * kProdMax + j) * kProdSums + k] = sacc;
      } else if (tid < kProdMax * kProdSums + kProdMax) {
        const int j = tid - kProdMax * kProdSums;
        long long sacc = 0;
        for (int i = 0; i < 64; ++i) sacc += cnt_s[(((i >> 4) * 64 + (j & 3) * 16 + (i & 15)) * 2) + (j >> 2)];
        a.cnt[(size_t)ch * kProdMax + j] = sacc;
      }
      __syncthreads();
    }
  }

  if (ver) {
    __syncthreads();
    if (cur_g >= 0)
      for (int i = tid; i < ntab; i += kQuadThreads) {
        const unsigned int v = tab_s[i];
        if (v) atomicAdd(&a.table[(size_t)cur_g * ntab + i], (unsigned long long)v);
      }
  }
}

template <bool SORT>
hipError_t launch_products_s(const ProdArgs& a, Elem elem, long grid, hipStream_t s) {
  return efa_host::launch_quad(a.M, elem, [&](auto nu_c, auto e) {
    hipLaunchKernelGGL((k_products<decltype(nu_c)::value, decltype(e), SORT>), dim3((unsigned)grid), dim3(kQuadThreads), 0, s, a);
    return hipGetLastError();
  });
}

hipError_t launch_products(const ProdArgs& a, Elem elem, int blocks, hipStream_t s) {
  if (a.M < 2 || a.M > kMaxMembers) return hipErrorInvalidValue;
  if (a.nchunks <= 0) return hipSuccess;
  long grid = a.nchunks < blocks ? a.nchunks : blocks;
  if (grid < 1) grid = 1;
  return a.nq > 0 ? launch_products_s<true>(a, elem, grid, s) : launch_products_s<false>(a, elem, grid, s);
}

}  // namespace
}  // namespace efa

// ---- the host side of efa_products_dev / efa_products_f32_dev ------------------------------------------------------------------
namespace efa_host {

using namespace efa;

// Like efa_verify_dev the call works in a buffer of its own (prod_ws) and neither reads nor writes what a later cycle reads.
// Nothing is written to the caller's arrays before every check has passed.
int products(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, long ncol, long n_lead, int nq, const double* q, int nt,
             const double* thr, double* mean_dev, double* sd_dev, double* quant_dev, double* prob_dev, const double* verif_dev,
             const int* slab_group, const double* col_weight_dev, long long* table, long long* n_bad, double* sums) {
  const char* me = elem == Elem::f32 ? "efa_products_f32_dev" : "efa_products_dev";
  if (M < 2 || M > kMaxMembers) return fail(EFA_ERR_INVALID, "%s: M=%d must be in [2,%d]", me, M, kMaxMembers);
  if (rows < 0 || ncol < 0 || n_lead < 0) return fail(EFA_ERR_INVALID, "%s: negative size", me);
  if (ncol * n_lead != rows) return fail(EFA_ERR_INVALID, "%s: rows=%ld must equal n_lead*ncol = %ld*%ld", me, rows, n_lead, ncol);
  if (!X_dev) return fail(EFA_ERR_INVALID, "%s: null device pointer", me);
  if (nq < 0 || nq > kProdMax) return fail(EFA_ERR_INVALID, "%s: nq=%d must be in [0,%d]", me, nq, kProdMax);
  if (nt < 0 || nt > kProdMax) return fail(EFA_ERR_INVALID, "%s: nt=%d must be in [0,%d]", me, nt, kProdMax);
  if (nq > 0 && !q) return fail(EFA_ERR_INVALID, "%s: null q", me);
  if (nt > 0 && !thr) return fail(EFA_ERR_INVALID, "%s: null thr", me);
  for (int i = 0; i < nq; ++i)
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(EFA_ERR_INVALID, "%s: q[%d] = %g must be in [0,1]", me, i, q[i]);
  for (long i = 0; i < n_lead * (long)nt; ++i)
    if (std::isinf(thr[i])) return fail(EFA_ERR_INVALID, "%s: thr[%ld][%ld] is infinite (NaN means no threshold)", me, i / nt, i % nt);
  if (nq > 0 && !quant_dev) return fail(EFA_ERR_INVALID, "%s: nq=%d but quant_dev is null", me, nq);
  if (nt > 0 && !prob_dev && !verif_dev) return fail(EFA_ERR_INVALID, "%s: nt=%d but prob_dev and verif_dev are both null", me, nt);
  int G = 0;
  if (verif_dev) {
    if (nt == 0) return fail(EFA_ERR_INVALID, "%s: verification needs a threshold (nt=0)", me);
    if (!slab_group) return fail(EFA_ERR_INVALID, "%s: null slab_group", me);
    if (!table != !n_bad || !table != !sums)
      return fail(EFA_ERR_INVALID, "%s: table, n_bad and sums go together (all null: no verification)", me);
    EFA_TRY(check_slab_groups(me, slab_group, n_lead, &G));
  }

  if (!table) {  // nothing to score into
    verif_dev = nullptr;
    G = 0;
  }

  c->products_us = 0;
  const size_t ntab = (size_t)nt * (M + 1) * 2;
  const size_t nh = (size_t)G * ntab, ngt = (size_t)G * nt;
  std::vector<long long> h_int(nh + ngt, 0);
  std::vector<double> h_sums(ngt * kProdSums, 0.0);
  if (rows > 0) {
    hipStream_t s = c->stream;
    const long tps = (ncol + 15) / 16;
    const long cps = (tps + kProdChunkTiles - 1) / kProdChunkTiles;
    const long nchunks = cps * n_lead;
    const int Gd = G > 0 ? G : 1;
    const int ntd = nt > 0 ? nt : 1;
    // prod_ws: part [nchunks][8][4] | sums [Gd][ntd][4] | thr [n_lead][8] | cnt [nchunks][8] | n_bad [Gd][ntd] | table [Gd][ntab] |
    //          slab groups [n_lead]
    const size_t n_tab = (size_t)Gd * (ntab ? ntab : 1);
    WsLayout ws;
    const auto r_part = ws.add<double>((size_t)nchunks * kProdMax * kProdSums), r_sums = ws.add<double>((size_t)Gd * ntd * kProdSums),
               r_thr = ws.add<double>((size_t)n_lead * kProdMax);
    const auto r_cnt = ws.add<long long>((size_t)nchunks * kProdMax), r_nbad = ws.add<long long>((size_t)Gd * ntd),
               r_tab = ws.add<long long>(n_tab);
    const auto r_sg = ws.add<int>((size_t)n_lead);
    EFA_TRY(c->prod_ws.reserve(ws.bytes()));
    double *d_part = r_part(c->prod_ws), *d_sums = r_sums(c->prod_ws), *d_thr = r_thr(c->prod_ws);
    long long *d_cnt = r_cnt(c->prod_ws), *d_nbad = r_nbad(c->prod_ws), *d_tab = r_tab(c->prod_ws);
    int* d_sg = r_sg(c->prod_ws);
    const std::vector<double> h_thr = pad_thresholds(thr, n_lead, nt, kProdMax);
    std::vector<int> h_sg((size_t)n_lead, -1);
    if (verif_dev)
      for (long l = 0; l < n_lead; ++l) h_sg[l] = slab_group[l];
    EFA_HIP(hipMemcpyAsync(d_thr, h_thr.data(), h_thr.size() * sizeof(double), hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemcpyAsync(d_sg, h_sg.data(), (size_t)n_lead * sizeof(int), hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemsetAsync(d_tab, 0, n_tab * sizeof(long long), s));
    ProdArgs a{};
    a.X = X_dev;
    a.verif = verif_dev;
    a.colw = col_weight_dev;
    a.sgroup = d_sg;
    a.thr = d_thr;
    a.ncol = ncol;
    a.n_lead = n_lead;
    a.rows = rows;
    a.nchunks = nchunks;
    a.cps = cps;
    a.M = M;
    a.al = pairs_aligned(X_dev, M, elem);
    a.nq = nq;
    a.nt = nt;
    for (int i = 0; i < nq; ++i) {  // numpy's linear rule: h = q (M - 1) in float64
      const double h = q[i] * (double)(M - 1);
      int lo = (int)std::floor(h);
      if (lo > M - 1) lo = M - 1;
      a.qlo[i] = lo;
      a.qhi[i] = lo + 1 < M - 1 ? lo + 1 : M - 1;
      a.qf[i] = h - (double)lo;
    }
    a.mean = mean_dev;
    a.sd = sd_dev;
    a.quant = quant_dev;
    a.prob = prob_dev;
    a.part = d_part;
    a.cnt = d_cnt;
    a.table = reinterpret_cast<unsigned long long*>(d_tab);
    EFA_TRY(interval_begin(c->prod_iv, s));
    EFA_HIP(launch_products(a, elem, (int)clamp_blocks(c->products_blocks, kProdBlocks), s));
    if (G > 0) {
      EFA_HIP((launch_group_reduce<kProdSums, 1>(G, nt, s, nchunks, cps, kProdMax, nullptr, d_sg, d_part, d_cnt, d_sums, d_nbad,
                                                 nullptr)));
    }
    EFA_TRY(interval_end(c->prod_iv, s));
    if (G > 0) {
      EFA_HIP(hipMemcpyAsync(h_int.data(), d_tab, nh * sizeof(long long), hipMemcpyDeviceToHost, s));
      EFA_HIP(hipMemcpyAsync(h_int.data() + nh, d_nbad, ngt * sizeof(long long), hipMemcpyDeviceToHost, s));
      EFA_HIP(hipMemcpyAsync(h_sums.data(), d_sums, h_sums.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    EFA_HIP(hipStreamSynchronize(s));
    EFA_TRY(interval_us(c->prod_iv, &c->products_us));
  }
  if (G > 0) {
    for (size_t i = 0; i < nh; ++i) table[i] = h_int[i];
    for (size_t i = 0; i < ngt; ++i) n_bad[i] = h_int[nh + i];
    for (size_t i = 0; i < h_sums.size(); ++i) sums[i] = h_sums[i];
  }
  return EFA_OK;
}

}  // namespace efa_host
