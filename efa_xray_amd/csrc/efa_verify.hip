// Ensemble verification against a gridded verifying state (Hamill 2001, Hersbach 2000, Ferro 2014).
//   For every state row i = lead*ncol + col with members x_i1..x_iM and a verifying value y_i: the number of members below and
//   equal to y, the rank of y among them (ties broken by a counter-based hash of (seed, global row)), the error of the ensemble
//   mean, the ensemble variance and the CRPS -- every float from the once-rounded d_m = x_im - y_i, in float64 -- and per group of
//   slabs the rank histogram, the counts and the weighted sums of the three.
//
// k_verify reads every row once, in the four-lane row layout (efa_quadrow.h): the whole row sits in registers, 2 NU doubles per
// lane.  below / equal / sum d / sum |d| / sum (d - err)^2 are lane-local plus two __shfl_xor steps.
//
// The CRPS needs the sorted d.  NU is a power of two, so a lane's LP = 2 NU slots are a power of two as well; slots beyond M hold
// +inf.  Every lane sorts its slots with a bitonic network whose comparators all point upwards, and the row's four lanes are
// merged by two bitonic stages: (g, g^1) exchange slot LP-1-k for slot k, the lower lane keeps the smaller; then (g, 3-g)
// likewise across the two pairs, a same-slot step inside each pair, and after each stage a lane-local bitonic merge.  Afterwards
// sorted position j = g LP + k is slot k of lane g, the +inf slots are the positions >= M, and every register index is a
// compile-time constant.
//
// Sums: a chunk is kVerChunkTiles tiles of one slab, whatever the grid; wave w takes its tiles w, w+4, ... in order, lane n adds
// its rows up, and the 64 lane sums of the chunk are added in index order into the chunk's partial.  k_group_reduce (efa_quadreduce.h) adds
// the partials of each group in a fixed order.  So the float sums depend on neither the grid nor the schedule; the histogram is
// integer adds in LDS and integer atomics in memory, whose result no order can change.  No floating-point atomics.
#include "efa_device.h"
#include "efa_diag.h"
#include "efa_quadreduce.h"
#include "efa_sortnet.h"

#include <cmath>
#include <vector>

namespace efa {
namespace {

constexpr int kVerBlocks = 2048;     // default grid cap of k_verify (option "verify_blocks" lowers it)
constexpr int kVerChunkTiles = 64;   // tiles per chunk: 1024 rows give one partial
constexpr int kVerSums = 5;          // sum w, w crps, w err, w err^2, w var
constexpr long kVerFlushChunks = 1L << 20;  // the LDS histogram (32-bit) goes to memory at least this often: < 2^31 rows

struct VerArgs {
  const void* X;
  const double* verif;   // [rows]
  const double* colw;    // [ncol] or null
  const int* sgroup;     // [n_lead], device copy
  long ncol, n_lead, col_offset, ncol_total;
  long nchunks, cps;     // chunks in all, chunks per slab
  int M, fair, al;       // al: the rows are aligned for the paired loads
  unsigned long long seed;
  int *below, *equal, *rank;   // [rows] each, or null
  double *crps, *err, *var;
  double* part;                // [nchunks][kVerSums]
  long long* cnt;              // [nchunks][2]: verified good rows, verified bad rows
  unsigned long long* hist;    // [G][M + 1]
};

// the tie-break: splitmix64 of the global row, scaled to [0, equal]
__device__ __forceinline__ int ver_pick(unsigned long long seed, unsigned long long R, int equal) {
  unsigned long long z = seed + (R + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (int)(((z >> 32) * (unsigned long long)(equal + 1)) >> 32);
}

// NU: chunks of 8 members the lanes hold, (M + 7) / 8 rounded up to a power of two: the sort network is that of LP = 2 NU slots
// whatever M is, so the six sizes are the only instantiations; which slots hold members is decided from M as the kernel runs
template <int NU, typename E>
__global__ __launch_bounds__(kQuadThreads) void k_verify(const VerArgs a) {
  constexpr int LP = 2 * NU;
  static_assert((NU & (NU - 1)) == 0, "the bitonic network needs a power of two");
  __shared__ unsigned int hist_s[kMaxMembers + 1];
  __shared__ double red_s[4 * 16 * kVerSums];
  __shared__ int cnt_s[4 * 16 * 2];
  const int M = a.M;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int g = lane >> 4, n = lane & 15;
  const double inf = __builtin_inf();
  const double nan = __builtin_nan("");
  const double dM = (double)M;
  const double D = a.fair ? dM * (double)(M - 1) : dM * dM;
  const long tps = (a.ncol + 15) / 16;
  const bool fields = a.below || a.equal || a.rank || a.crps || a.err || a.var;

  for (int i = tid; i <= M; i += kQuadThreads) hist_s[i] = 0u;
  __syncthreads();
  int cur_g = -1;  // the group the LDS histogram belongs to
  long since = 0;

#pragma unroll 1
  for (long ch = blockIdx.x; ch < a.nchunks; ch += gridDim.x) {
    const long lead = ch / a.cps, cc = ch % a.cps;
    const int sg = a.sgroup[lead];
    if (sg != cur_g || since >= kVerFlushChunks) {  // (uniform)
      __syncthreads();
      if (cur_g >= 0) quad_flush_table(hist_s, M + 1, a.hist + (size_t)cur_g * (M + 1), true);
      __syncthreads();
      cur_g = sg;
      since = 0;
    }
    ++since;
    const long t0 = cc * kVerChunkTiles;
    const long t1 = (t0 + kVerChunkTiles < tps) ? t0 + kVerChunkTiles : tps;
    double acc[kVerSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int n_good = 0, n_bad = 0;

#pragma unroll 1
    for (long tl = t0 + wv; tl < t1; tl += kQuadThreads / 64) {
      const long col = tl * 16 + n;
      const bool live = col < a.ncol;
      const long colc = live ? col : a.ncol - 1;
      const long r = lead * a.ncol + colc;
      if (sg < 0) {  // (uniform) a slab that is not verified: only the fields are written
        if (fields && g == 0 && live) {
          if (a.below) a.below[r] = -1;
          if (a.equal) a.equal[r] = -1;
          if (a.rank) a.rank[r] = -1;
          if (a.crps) a.crps[r] = nan;
          if (a.err) a.err[r] = nan;
          if (a.var) a.var[r] = nan;
        }
        continue;
      }
      const int gq = quad_lane_quarter(lane);
      const double y = a.verif[r];
      const double w = a.colw ? a.colw[colc] : 1.0;
      double d[LP];
      quad_load_row<NU, E>(a.X, r, M, gq, a.al, d);
      int lb = 0, le = 0;
      bool badl = false;
      double s4[4] = {0.0, 0.0, 0.0, 0.0}, a4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < LP; ++c) {
        const bool ok = quad_slot_ok(c, gq, M);
        const double xv = d[c];
        lb += (ok && xv < y) ? 1 : 0;
        le += (ok && xv == y) ? 1 : 0;
        const double dv = xv - y;
        badl = badl || (ok && !finite64(dv));
        s4[c & 3] += ok ? dv : 0.0;
        a4[c & 3] += ok ? __builtin_fabs(dv) : 0.0;
        d[c] = ok ? dv : inf;
      }
      const double d0 = __shfl(d[0], n, 64);  // member 0
      const bool diff = quad_differs<LP>(d, d0, gq, M);
      const double sum = quad_row_sum((s4[0] + s4[1]) + (s4[2] + s4[3]));
      const double asum = quad_row_sum((a4[0] + a4[1]) + (a4[2] + a4[3]));
      lb = quad_row_sum(lb);
      le = quad_row_sum(le);
      const bool varies = quad_row_any(diff, n);
      const bool bad = quad_row_any(badl, n);
      const double err = varies ? sum / dM : d0;  // the error of the mean, by the rule of quad_centred_ss
      const double var = quad_centred_ss<LP>(d, err, gq, M) / (double)(M - 1);

      quad_sort<LP>(d, gq);  // afterwards sorted position g LP + k is slot k of lane g
      double t4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < LP; ++k) {
        const int j = gq * LP + k;
        t4[k & 3] = __builtin_fma((double)(2 * j - M + 1), (j < M) ? d[k] : 0.0, t4[k & 3]);
      }
      const double ts = quad_row_sum((t4[0] + t4[1]) + (t4[2] + t4[3]));
      const double crps = asum / dM - ts / D;

      if (gq == 0 && live) {
        const bool verified = finite64(y) && w > 0.0;
        const bool good = verified && !bad;
        int rank = -1;
        if (good) {
          const unsigned long long R =
              (unsigned long long)lead * (unsigned long long)a.ncol_total + (unsigned long long)(a.col_offset + col);
          rank = lb + ver_pick(a.seed, R, le);
          atomicAdd(&hist_s[rank], 1u);
          acc[0] += w;
          acc[1] += w * crps;
          acc[2] += w * err;
          acc[3] += w * (err * err);
          acc[4] += w * var;
          ++n_good;
        } else if (verified) {
          ++n_bad;
        }
        if (fields) {
          if (a.below) a.below[r] = good ? lb : -1;
          if (a.equal) a.equal[r] = good ? le : -1;
          if (a.rank) a.rank[r] = rank;
          if (a.crps) a.crps[r] = good ? crps : nan;
          if (a.err) a.err[r] = good ? err : nan;
          if (a.var) a.var[r] = good ? var : nan;
        }
      }
    }

    // the chunk's partial: the 64 lane sums in index order
    if (g == 0) {
#pragma unroll
      for (int k = 0; k < kVerSums; ++k) red_s[(wv * 16 + n) * kVerSums + k] = acc[k];
      cnt_s[(wv * 16 + n) * 2] = n_good;
      cnt_s[(wv * 16 + n) * 2 + 1] = n_bad;
    }
    __syncthreads();
    if (tid < kVerSums)
      a.part[(size_t)ch * kVerSums + tid] = quad_chunk_partial<double>(red_s, [&](int i) { return i * kVerSums + tid; });
    else if (tid < kVerSums + 2)
      a.cnt[(size_t)ch * 2 + (tid - kVerSums)] = quad_chunk_partial<long long>(cnt_s, [&](int i) { return i * 2 + (tid - kVerSums); });
    __syncthreads();
  }

  __syncthreads();
  if (cur_g >= 0) quad_flush_table(hist_s, M + 1, a.hist + (size_t)cur_g * (M + 1), false);
}

hipError_t launch_verify(const VerArgs& a, Elem elem, int blocks, hipStream_t s) {
  if (a.M < 2 || a.M > kMaxMembers) return hipErrorInvalidValue;
  if (a.nchunks <= 0) return hipSuccess;
  long grid = a.nchunks < blocks ? a.nchunks : blocks;
  if (grid < 1) grid = 1;
  return efa_host::launch_quad(a.M, elem, [&](auto nu_c, auto e) {
    hipLaunchKernelGGL((k_verify<decltype(nu_c)::value, decltype(e)>), dim3((unsigned)grid), dim3(kQuadThreads), 0, s, a);
    return hipGetLastError();
  });
}

}  // namespace
}  // namespace efa

// ---- the host side of efa_verify_dev / efa_verify_f32_dev ----------------------------------------------------------------------
namespace efa_host {

using namespace efa;

// Like efa_obs_impact_dev and efa_sensitivity_dev the call works in a buffer of its own (ver_ws) and neither reads nor writes what
// a later cycle reads.  Nothing is written to the caller's arrays before every check has passed.
int verify(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, const double* verif_dev, long ncol, long n_lead,
           long col_offset, long ncol_total, const int* slab_group, const double* col_weight_dev, int fair, uint64_t seed,
           int* below_dev, int* equal_dev, int* rank_dev, double* crps_dev, double* err_dev, double* var_dev, long long* hist,
           long long* n, long long* n_bad, double* sums) {
  const char* me = elem == Elem::f32 ? "efa_verify_f32_dev" : "efa_verify_dev";
  if (M < 2 || M > kMaxMembers) return fail(EFA_ERR_INVALID, "%s: M=%d must be in [2,%d]", me, M, kMaxMembers);
  if (rows < 0 || ncol < 0 || n_lead < 0) return fail(EFA_ERR_INVALID, "%s: negative size", me);
  if (ncol * n_lead != rows) return fail(EFA_ERR_INVALID, "%s: rows=%ld must equal n_lead*ncol = %ld*%ld", me, rows, n_lead, ncol);
  if (col_offset < 0 || col_offset + ncol > ncol_total)
    return fail(EFA_ERR_INVALID, "%s: columns [%ld, %ld) do not lie in [0, ncol_total=%ld)", me, col_offset, col_offset + ncol,
                ncol_total);
  if (!X_dev || !verif_dev) return fail(EFA_ERR_INVALID, "%s: null device pointer", me);
  if (!slab_group) return fail(EFA_ERR_INVALID, "%s: null slab_group", me);
  int G = 0;
  EFA_TRY(check_slab_groups(me, slab_group, n_lead, &G));
  const bool no_groups = !hist && !n && !n_bad && !sums;  // fields only
  if (G > 0 && !no_groups && (!hist || !n || !n_bad || !sums))
    return fail(EFA_ERR_INVALID, "%s: hist, n, n_bad and sums go together (all null: fields only)", me);

  c->verify_us = 0;
  const size_t nh = (size_t)G * (M + 1);
  std::vector<long long> h_int(nh + 2 * (size_t)G, 0);
  std::vector<double> h_sums((size_t)G * kVerSums, 0.0);
  if (rows > 0) {
    hipStream_t s = c->stream;
    const long tps = (ncol + 15) / 16;
    const long cps = (tps + kVerChunkTiles - 1) / kVerChunkTiles;
    const long nchunks = cps * n_lead;
    const int Gd = G > 0 ? G : 1;
    // ver_ws: part [nchunks][5] | sums [Gd][5] | cnt [nchunks][2] | hist [Gd][M+1] | n [Gd] | n_bad [Gd] | slab groups [n_lead]
    const size_t n_hist = (size_t)Gd * (M + 1);
    WsLayout ws;
    const auto r_part = ws.add<double>((size_t)nchunks * kVerSums), r_sums = ws.add<double>((size_t)Gd * kVerSums);
    const auto r_cnt = ws.add<long long>((size_t)nchunks * 2), r_hist = ws.add<long long>(n_hist), r_n = ws.add<long long>(Gd),
               r_nbad = ws.add<long long>(Gd);
    const auto r_sg = ws.add<int>((size_t)n_lead);
    EFA_TRY(c->ver_ws.reserve(ws.bytes()));
    double *d_part = r_part(c->ver_ws), *d_sums = r_sums(c->ver_ws);
    long long *d_cnt = r_cnt(c->ver_ws), *d_hist = r_hist(c->ver_ws), *d_n = r_n(c->ver_ws), *d_nbad = r_nbad(c->ver_ws);
    int* d_sg = r_sg(c->ver_ws);
    EFA_HIP(hipMemcpyAsync(d_sg, slab_group, (size_t)n_lead * sizeof(int), hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemsetAsync(d_hist, 0, n_hist * sizeof(long long), s));
    VerArgs a{};
    a.X = X_dev;
    a.verif = verif_dev;
    a.colw = col_weight_dev;
    a.sgroup = d_sg;
    a.ncol = ncol;
    a.n_lead = n_lead;
    a.col_offset = col_offset;
    a.ncol_total = ncol_total;
    a.nchunks = nchunks;
    a.cps = cps;
    a.M = M;
    a.fair = fair ? 1 : 0;
    a.al = pairs_aligned(X_dev, M, elem);
    a.seed = seed;
    a.below = below_dev;
    a.equal = equal_dev;
    a.rank = rank_dev;
    a.crps = crps_dev;
    a.err = err_dev;
    a.var = var_dev;
    a.part = d_part;
    a.cnt = d_cnt;
    a.hist = reinterpret_cast<unsigned long long*>(d_hist);
    EFA_TRY(interval_begin(c->ver_iv, s));
    EFA_HIP(launch_verify(a, elem, (int)clamp_blocks(c->verify_blocks, kVerBlocks), s));
    EFA_HIP((launch_group_reduce<kVerSums, 2>(Gd, 1, s, nchunks, cps, 1, nullptr, d_sg, d_part, d_cnt, d_sums, d_n, d_nbad)));
    EFA_TRY(interval_end(c->ver_iv, s));
    if (G > 0) {
      EFA_HIP(hipMemcpyAsync(h_int.data(), d_hist, nh * sizeof(long long), hipMemcpyDeviceToHost, s));
      EFA_HIP(hipMemcpyAsync(h_int.data() + nh, d_n, (size_t)G * sizeof(long long), hipMemcpyDeviceToHost, s));
      EFA_HIP(hipMemcpyAsync(h_int.data() + nh + G, d_nbad, (size_t)G * sizeof(long long), hipMemcpyDeviceToHost, s));
      EFA_HIP(hipMemcpyAsync(h_sums.data(), d_sums, h_sums.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    EFA_HIP(hipStreamSynchronize(s));
    EFA_TRY(interval_us(c->ver_iv, &c->verify_us));
  }
  if (G > 0 && !no_groups) {
    for (size_t i = 0; i < nh; ++i) hist[i] = h_int[i];
    for (int g = 0; g < G; ++g) {
      n[g] = h_int[nh + g];
      n_bad[g] = h_int[nh + G + g];
    }
    for (size_t i = 0; i < h_sums.size(); ++i) sums[i] = h_sums[i];
  }
  return EFA_OK;
}

}  // namespace efa_host
