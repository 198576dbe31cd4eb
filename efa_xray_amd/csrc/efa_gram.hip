// The ensemble Gram matrix in a weighted norm: G = X'^T C X'/(M-1), M x M, the one object behind the
// between-member questions -- distances between members, EOFs / principal components, clusters of members.
//   For every state row i = lead*ncol + col with members x_i1..x_iM: mean_i = (sum_m x_im)/M, x'_im = x_im - mean_i, the row's
//   coefficient c_i = w_col s_lead^2, and over the used (s_lead > 0, w_col > 0), good (every member and w_col finite) rows
//   G_ab = (sum_i c_i x'_ia x'_ib)/(M-1), n = their number, sums = (sum w_col, sum c_i).  Every number in float64.
//
// k_gram is a tall-skinny symmetric rank-k update on the fp64 matrix cores; the contraction index of v_mfma_f64_16x16x4_f64 is the
// state row.
//   - A chunk is kGramRows = 32 consecutive rows of one slab, whatever the grid.  The workgroup stages it in LDS as doubles
//     (16-byte loads of two float64 members, 8-byte of two float32, where M is even and the base aligned; single elements
//     otherwise), rows of weight <= 0 are not read.  LPR lanes per row then form the row sum (a butterfly: every lane gets the same
//     bits), find out whether every member is finite and whether they are all equal (the mean is then the member itself, the
//     deviations exactly 0), and write x' back over x -- 0.0, by a select, for rows that are unused or bad, and in the member
//     slots beyond M and the rows beyond the chunk's last, which were staged as 0.0.
//   - The member tiles of 16 give T = ceil(M/16) tile rows, and every unordered pair of tiles {t, u} is computed once, as tile
//     (t, (t + s) mod T) with 0 <= s <= T/2 (for an even T the rows t >= T/2 stop at T/2 - 1).  Wave w owns tile rows w (T/2 + 1
//     slots) and T-1-w (the rest): T + 1 tiles whatever w.  The first T/2 tiles of x' are stored a second time behind the last,
//     so tile (t + s) mod T is read at t + s: a wave's operand addresses are two bases and constant offsets.  Per step of 4 rows,
//     lane (g = l>>4, n = l&15) reads x'[4k+g][16 (t + s) + n] once per slot as the B operand and forms the two A operands
//     c x'[4k+g][16 t + n] once per step: c enters on one side only.  The accumulators, 8 (T+1) registers, stay in registers
//     over all chunks of a stream.  (For an odd T the middle wave's two rows are one and the same.)
//   - Determinism: S streams, S = min(chunks, 256 x the workgroups a CU holds: 1024 or 768 for T <= 8, 256 above), whatever the grid; stream s takes chunks s, s+S, ... in
//     order, a workgroup takes whole streams and writes each stream's partial tiles (and the row statistics, summed in row-slot
//     order).  k_gram_reduce adds the streams' partials in an order the sizes alone decide (16 interleaved runs of streams, then
//     the 16 sums), for the elements a <= b (from the tile or from its transpose, whichever was computed), mirrors them and divides by
//     M-1: G[a][b] and G[b][a] are one number.  No floating-point atomics; the same inputs give the same bits for every grid.
#include "efa_device.h"
#include "efa_diag.h"
#include "efa_quadrow.h"

#include <cmath>
#include <vector>

namespace efa {
namespace {

typedef double gram_v4 __attribute__((ext_vector_type(4)));

constexpr int kGramRows = 32;            // rows per chunk: 8 MFMA steps of 4
constexpr int kGramBlocks = 2048;        // default grid cap of k_gram (option "gram_blocks" lowers it)
// Accumulation streams: 256 (the CUs) times the workgroups of the instantiation a CU holds at once (its registers and LDS decide;
// DESIGN.md 7q has the table), so that every stream is resident from the start.  A function of T alone, never of the grid.
constexpr int gram_stream_cap(int T) { return T > 8 ? 256 : (T <= 2 || T == 5) ? 1024 : 768; }
constexpr int kGramRedThreads = 256;

struct GramArgs {
  const void* X;
  const double* colw;   // [ncol] or null
  const double* scale;  // [n_lead], device copy
  long ncol, n_lead;
  int nchunks, cps;     // chunks in all, chunks per slab (the host refuses more than 2^31 - 1: no memory holds their rows)
  int M, nstreams;
  double* part;         // [nstreams][MP][MP], upper tiles only
  double* spart;        // [nstreams][2]: sum w, sum c
  long long* cpart;     // [nstreams][2]: good rows, bad rows
};

constexpr int gram_waves(int T) { return T > 8 ? 8 : 4; }

// T: tiles of 16 members ((M + 15) / 16).  AL: the rows are aligned for the paired loads (M even, base aligned to two elements).
template <int T, bool AL, typename E>
__global__ __launch_bounds__(64 * gram_waves(T)) void k_gram(const GramArgs a) {
  constexpr int NW = gram_waves(T), NTH = 64 * NW, MP = 16 * T;
  constexpr int TE = T / 2;         // the first TE member tiles are stored a second time behind the last: tile (t + s) mod T is tile t + s
  constexpr int H1 = T / 2 + 1, H2 = T + 1 - H1;  // slots of the wave's first and second tile row
  constexpr int LS = 16 * ((T + TE) | 1);  // row stride in LDS: = 16 mod 32 doubles, so lanes l and l+16 of an operand read fall on opposite halves of the bank row
  constexpr int LPR = NTH / kGramRows;  // lanes per row in the centring pass: 8 or 16
  constexpr int BL = 4;                 // loads per lane and batch of the staging
  __shared__ __align__(16) double Xs[kGramRows * LS];
  __shared__ double c_s[kGramRows];
  __shared__ double w_s[kGramRows];
  __shared__ double red_s[kGramRows * 2];
  __shared__ int cnt_s[kGramRows * 2];
  const int M = a.M;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, n = lane & 15;
  const int crow = tid / LPR, cj = tid % LPR;  // the centring pass: row of the chunk, lane of the row
  const bool mfma_wave = wv < (T + 1) / 2;
  const int r1 = wv, r2 = T - 1 - wv;  // the wave's tile rows
  const double dM = (double)M;

#pragma unroll 1
  for (int st = blockIdx.x; st < a.nstreams; st += gridDim.x) {
    gram_v4 acc[T + 1];
#pragma unroll
    for (int s = 0; s <= T; ++s) acc[s] = gram_v4{0.0, 0.0, 0.0, 0.0};
    double sum_w = 0.0, sum_c = 0.0;  // of row slot crow (lane cj == 0)
    int n_good = 0, n_bad = 0;

#pragma unroll 1
    for (long ch = st; ch < a.nchunks; ch += a.nstreams) {
      const int lead = (int)ch / a.cps;
      const long c0 = (long)((int)ch - lead * a.cps) * kGramRows;
      const double sc = a.scale[lead];
      if (!(sc > 0.0)) continue;  // (uniform) a slab of scale 0 is not read
      const long left = a.ncol - c0;
      const int nr = left < kGramRows ? (int)left : kGramRows;
      if (tid < kGramRows) {
        double w = 0.0;
        if (tid < nr) w = a.colw ? a.colw[c0 + tid] : 1.0;
        w_s[tid] = (w > 0.0) ? w : 0.0;  // 0: the row is not used (a NaN weight too)
      }
      __syncthreads();  // (also: the previous chunk's operand reads are done)
      const E* base = reinterpret_cast<const E*>(a.X) + (size_t)((long)lead * a.ncol + c0) * M;
      // BL paired loads (BL / 2 single ones) in flight per lane and batch: the accumulators leave no room for more at 16 tiles, and
      // eight cost the 80-member instantiation its fourth workgroup per CU (as did asking for the next chunk's weights early)
      if (AL) {
        typedef typename ElemPair<E>::type P2;
        constexpr int NP = kGramRows * MP / 2;
#pragma unroll 1
        for (int i0 = 0; i0 < NP; i0 += BL * NTH) {
          P2 v[BL];
#pragma unroll
          for (int i = 0; i < BL; ++i) {
            const int idx = i0 + i * NTH + tid;
            const int row = idx / (MP / 2), m = 2 * (idx % (MP / 2));
            v[i].x = 0;
            v[i].y = 0;
            if (idx < NP && m < M && w_s[row] > 0.0) v[i] = *reinterpret_cast<const P2*>(base + (size_t)row * M + m);
          }
#pragma unroll
          for (int i = 0; i < BL; ++i) {
            const int idx = i0 + i * NTH + tid;
            const int row = idx / (MP / 2), m = 2 * (idx % (MP / 2));
            if (idx < NP) *reinterpret_cast<double2*>(&Xs[row * LS + m]) = double2{(double)v[i].x, (double)v[i].y};
          }
        }
      } else {
        constexpr int NP = kGramRows * MP;
#pragma unroll 1
        for (int i0 = 0; i0 < NP; i0 += BL / 2 * NTH) {
          E v[BL / 2];
#pragma unroll
          for (int i = 0; i < BL / 2; ++i) {
            const int idx = i0 + i * NTH + tid;
            const int row = idx / MP, m = idx % MP;
            v[i] = 0;
            if (idx < NP && m < M && w_s[row] > 0.0) v[i] = base[(size_t)row * M + m];
          }
#pragma unroll
          for (int i = 0; i < BL / 2; ++i) {
            const int idx = i0 + i * NTH + tid;
            const int row = idx / MP, m = idx % MP;
            if (idx < NP) Xs[row * LS + m] = (double)v[i];
          }
        }
      }
      __syncthreads();

      {  // the row's mean leaves before anything is multiplied
        double* xr = Xs + crow * LS;
        const double w = w_s[crow];
        const double x0 = xr[0];
        double sum = 0.0;
        int flaw = 0;  // bit 0: a member is not finite; bit 1: a member differs from member 0
#pragma unroll 4
        for (int m = cj; m < M; m += LPR) {
          const double x = xr[m];
          sum += x;
          flaw |= (finite64(x) ? 0 : 1) | ((x != x0) ? 2 : 0);
        }
#pragma unroll
        for (int off = LPR / 2; off >= 1; off >>= 1) {
          sum += __shfl_xor(sum, off, 64);
          flaw |= __shfl_xor(flaw, off, 64);
        }
        const bool used = w > 0.0;
        const bool good = used && !(flaw & 1) && finite64(w);
        // a row whose members are all equal has deviations of exactly 0 (its sum / M need not give the member back)
        const double mean = (flaw & 2) ? sum / dM : x0;
        const double c = good ? w * (sc * sc) : 0.0;
#pragma unroll 4
        for (int m = cj; m < M; m += LPR) {
          const double d = good ? xr[m] - mean : 0.0;
          xr[m] = d;
          if (m < 16 * TE) xr[MP + m] = d;
        }
        if (cj == 0) {
          c_s[crow] = c;
          if (good) {
            sum_w += w;
            sum_c += c;
            ++n_good;
          } else if (used) {
            ++n_bad;
          }
        }
      }
      __syncthreads();

      if (mfma_wave) {
#pragma unroll 1
        for (int k = 0; k < kGramRows / 4; ++k) {
          const double* p1 = Xs + (4 * k + g) * LS + 16 * r1 + n;
          const double* p2 = Xs + (4 * k + g) * LS + 16 * r2 + n;
          const double c = c_s[4 * k + g];
          const double b1 = p1[0], b2 = p2[0];
          const double a1 = c * b1, a2 = c * b2;
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[0], 0, 0, 0);
#pragma unroll
          for (int s = 1; s < H1; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, p1[16 * s], acc[s], 0, 0, 0);
          acc[H1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, acc[H1], 0, 0, 0);
#pragma unroll
          for (int s = 1; s < H2; ++s) acc[H1 + s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, p2[16 * s], acc[H1 + s], 0, 0, 0);
        }
      }
    }

    // the stream's partial: its tiles, and the row slots' statistics in slot order
    if (mfma_wave) {
      double* out = a.part + (size_t)st * MP * MP;
#pragma unroll
      for (int s = 0; s <= T; ++s) {
        const int ta = s < H1 ? r1 : r2;
        const int tb = (ta + (s < H1 ? s : s - H1)) % T;  // (for an odd T the middle wave has r1 == r2 and writes the same tiles twice)
#pragma unroll
        for (int v = 0; v < 4; ++v) out[(size_t)(16 * ta + g + 4 * v) * MP + 16 * tb + n] = acc[s][v];
      }
    }
    if (cj == 0) {
      red_s[crow * 2] = sum_w;
      red_s[crow * 2 + 1] = sum_c;
      cnt_s[crow * 2] = n_good;
      cnt_s[crow * 2 + 1] = n_bad;
    }
    __syncthreads();
    if (tid < 2) {
      double s = 0.0;
      for (int i = 0; i < kGramRows; ++i) s += red_s[i * 2 + tid];
      a.spart[(size_t)st * 2 + tid] = s;
    } else if (tid < 4) {
      long long s = 0;
      for (int i = 0; i < kGramRows; ++i) s += cnt_s[i * 2 + (tid - 2)];
      a.cpart[(size_t)st * 2 + (tid - 2)] = s;
    }
    __syncthreads();
  }
}

// workgroup (a, tb): row a of G against member tile tb, for the tiles at or right of the diagonal.  Thread (gi = tid >> 4, bj =
// tid & 15) adds the partials of element (a, 16 tb + bj) of the streams gi, gi + 16, ... in that order; the 16 sums are added in
// the order of gi, divided by M-1 and written to G[a][b] and G[b][a].  Workgroup (0, 0) also adds the streams' row statistics:
// thread t those of streams t, t + 256, ..., then a tree over the threads.  The order is a function of the sizes alone.
__global__ __launch_bounds__(kGramRedThreads) void k_gram_reduce(int M, int MP, int nstreams, const double* __restrict__ part,
                                                                  const double* __restrict__ spart,
                                                                  const long long* __restrict__ cpart, double* __restrict__ G,
                                                                  double* __restrict__ sums, long long* __restrict__ cnt) {
  __shared__ double red_s[16][17];
  __shared__ double s_s[kGramRedThreads];
  __shared__ long long c_s[kGramRedThreads];
  const int tid = threadIdx.x;
  const int ra = (int)blockIdx.x, tb = (int)blockIdx.y;
  const int T = MP / 16;
  const size_t tile = (size_t)MP * MP;
  if (tb >= ra / 16) {  // (uniform)
    const int gi = tid >> 4, bj = tid & 15;
    const int b = 16 * tb + bj;
    // tile (A, B), A <= B, was computed as such when B - A <= T/2, and as its transpose (B, A) otherwise
    const bool direct = tb - ra / 16 <= T / 2;
    const double* p = part + (direct ? (size_t)ra * MP + b : (size_t)b * MP + ra);
    double s = 0.0;
#pragma unroll 4
    for (int st = gi; st < nstreams; st += 16) s += p[(size_t)st * tile];
    red_s[gi][bj] = s;
    __syncthreads();
    if (gi == 0 && b >= ra && b < M) {
      double t = 0.0;
      for (int i = 0; i < 16; ++i) t += red_s[i][bj];
      const double v = t / (double)(M - 1);
      G[(size_t)ra * M + b] = v;
      G[(size_t)b * M + ra] = v;
    }
  }
  if (ra != 0 || tb != 0) return;
  for (int k = 0; k < 4; ++k) {
    double s = 0.0;
    long long c = 0;
    for (int st = tid; st < nstreams; st += kGramRedThreads) {
      if (k < 2) s += spart[(size_t)st * 2 + k];
      else c += cpart[(size_t)st * 2 + (k - 2)];
    }
    s_s[tid] = s;
    c_s[tid] = c;
    __syncthreads();
    for (int off = kGramRedThreads / 2; off >= 1; off >>= 1) {
      if (tid < off) {
        s_s[tid] += s_s[tid + off];
        c_s[tid] += c_s[tid + off];
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (k < 2) sums[k] = s_s[0];
      else cnt[k - 2] = c_s[0];
    }
    __syncthreads();
  }
}

template <int T, typename E>
hipError_t gram_launch(const GramArgs& a, bool al, int grid, hipStream_t s) {
  if (al) hipLaunchKernelGGL((k_gram<T, true, E>), dim3((unsigned)grid), dim3(64 * gram_waves(T)), 0, s, a);
  else hipLaunchKernelGGL((k_gram<T, false, E>), dim3((unsigned)grid), dim3(64 * gram_waves(T)), 0, s, a);
  return hipGetLastError();
}

int gram_streams(int M, long nchunks) {
  const long cap = gram_stream_cap((M + 15) / 16);
  return (int)(nchunks < cap ? nchunks : cap);
}

hipError_t launch_gram(const GramArgs& a, Elem elem, int blocks, hipStream_t s) {
  if (a.M < 2 || a.M > kMaxMembers || a.nstreams < 1) return hipErrorInvalidValue;
  int grid = a.nstreams < blocks ? a.nstreams : blocks;
  if (grid < 1) grid = 1;
  const bool al = efa_host::pairs_aligned(a.X, a.M, elem);
  return dispatch_width((a.M + 15) / 16, WidthRange<1, kMaxMembers / 16>{}, [&](auto t_c) {
    constexpr int t = decltype(t_c)::value;
    return elem == Elem::f32 ? gram_launch<t, float>(a, al, grid, s) : gram_launch<t, double>(a, al, grid, s);
  });
}

}  // namespace
}  // namespace efa

// ---- the host side of efa_gram_dev / efa_gram_f32_dev ---------------------------------------------------------------------------
namespace efa_host {

using namespace efa;

// Like efa_verify_dev the call works in a buffer of its own (gram_ws) and neither reads nor writes what a later cycle reads.
// Nothing is written to the caller's arrays before every check has passed.
int gram(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, long ncol, long n_lead, const double* slab_scale,
         const double* col_weight_dev, double* gram_out, long long* n, long long* n_bad, double* sums) {
  const char* me = elem == Elem::f32 ? "efa_gram_f32_dev" : "efa_gram_dev";
  if (M < 2 || M > kMaxMembers) return fail(EFA_ERR_INVALID, "%s: M=%d must be in [2,%d]", me, M, kMaxMembers);
  if (rows < 0 || ncol < 0 || n_lead < 0) return fail(EFA_ERR_INVALID, "%s: negative size", me);
  if (ncol * n_lead != rows) return fail(EFA_ERR_INVALID, "%s: rows=%ld must equal n_lead*ncol = %ld*%ld", me, rows, n_lead, ncol);
  if (!X_dev) return fail(EFA_ERR_INVALID, "%s: null device pointer", me);
  if (!slab_scale) return fail(EFA_ERR_INVALID, "%s: null slab_scale", me);
  if (!gram_out || !n || !n_bad || !sums) return fail(EFA_ERR_INVALID, "%s: null output (gram, n, n_bad, sums)", me);
  bool any = false;
  for (long s = 0; s < n_lead; ++s) {
    if (!(std::isfinite(slab_scale[s]) && slab_scale[s] >= 0.0))
      return fail(EFA_ERR_INVALID, "%s: slab_scale[%ld] = %g is not finite and >= 0", me, s, slab_scale[s]);
    any = any || slab_scale[s] > 0.0;
  }
  const long cps = (ncol + kGramRows - 1) / kGramRows;
  const long nchunks = cps * n_lead;
  if (nchunks > 0x7fffffffL) return fail(EFA_ERR_INVALID, "%s: %ld chunks of %d rows are more than 2^31 - 1", me, nchunks, kGramRows);

  c->gram_us = 0;
  std::vector<double> h_G((size_t)M * M, 0.0);
  double h_sums[2] = {0.0, 0.0};
  long long h_cnt[2] = {0, 0};
  if (rows > 0 && any) {  // with every scale 0 nothing is read and nothing launched
    hipStream_t s = c->stream;
    const int MP = 16 * ((M + 15) / 16);
    const int S = gram_streams(M, nchunks);
    // gram_ws: part [S][MP][MP] | G [M][M] | spart [S][2] | sums [2] | cpart [S][2] | cnt [2] | scales [n_lead]
    const size_t n_G = (size_t)M * M;
    WsLayout ws;
    const auto r_part = ws.add<double>((size_t)S * MP * MP), r_G = ws.add<double>(n_G), r_sp = ws.add<double>((size_t)S * 2),
               r_sums = ws.add<double>(2);
    const auto r_cp = ws.add<long long>((size_t)S * 2), r_cnt = ws.add<long long>(2);
    const auto r_scale = ws.add<double>((size_t)n_lead);
    EFA_TRY(c->gram_ws.reserve(ws.bytes()));
    double *d_part = r_part(c->gram_ws), *d_G = r_G(c->gram_ws), *d_sp = r_sp(c->gram_ws), *d_sums = r_sums(c->gram_ws);
    long long *d_cp = r_cp(c->gram_ws), *d_cnt = r_cnt(c->gram_ws);
    double* d_scale = r_scale(c->gram_ws);
    EFA_HIP(hipMemcpyAsync(d_scale, slab_scale, (size_t)n_lead * sizeof(double), hipMemcpyHostToDevice, s));
    GramArgs a{};
    a.X = X_dev;
    a.colw = col_weight_dev;
    a.scale = d_scale;
    a.ncol = ncol;
    a.n_lead = n_lead;
    a.nchunks = (int)nchunks;
    a.cps = (int)cps;
    a.M = M;
    a.nstreams = S;
    a.part = d_part;
    a.spart = d_sp;
    a.cpart = d_cp;
    EFA_TRY(interval_begin(c->gram_iv, s));
    EFA_HIP(launch_gram(a, elem, (int)clamp_blocks(c->gram_blocks, kGramBlocks), s));
    hipLaunchKernelGGL(k_gram_reduce, dim3((unsigned)M, (unsigned)(MP / 16)), dim3(kGramRedThreads), 0, s, M, MP, S, d_part, d_sp, d_cp, d_G, d_sums,
                       d_cnt);
    EFA_HIP(hipGetLastError());
    EFA_TRY(interval_end(c->gram_iv, s));
    EFA_HIP(hipMemcpyAsync(h_G.data(), d_G, n_G * sizeof(double), hipMemcpyDeviceToHost, s));
    EFA_HIP(hipMemcpyAsync(h_sums, d_sums, sizeof(h_sums), hipMemcpyDeviceToHost, s));
    EFA_HIP(hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, s));
    EFA_HIP(hipStreamSynchronize(s));
    EFA_TRY(interval_us(c->gram_iv, &c->gram_us));
  }
  for (size_t i = 0; i < h_G.size(); ++i) gram_out[i] = h_G[i];
  *n = h_cnt[0];
  *n_bad = h_cnt[1];
  sums[0] = h_sums[0];
  sums[1] = h_sums[1];
  return EFA_OK;
}

}  // namespace efa_host
