// The probability-matched ensemble mean (Ebert 2001) and its patch-wise form (Clark 2017; Snook et al. 2019).
//   Row i = lead*ny*nx + y*nx + x with members x_i1..x_iM and a rank value f_i.  A SEGMENT is one patch of one slab: patch (Y, X)
//   holds the elements with y/py == Y and x/px == X (edge patches are smaller).  A row is EXCLUDED when f_i or a member is not
//   finite: its output is NaN, it enters no pool and it is counted in n_bad.  Within a segment with n included rows,
//     order = the included rows by f ascending, ties by row index ascending (-0.0 == +0.0),
//     pool  = the n M members of the included rows ascending (-0.0 stored as +0.0),
//   and the row at position r of order gets pool[r M + g].  A selection of input values: no arithmetic, bit equality.
//
// Everything is integer work on order-preserving keys: key(v) = bits(v + 0.0) with the sign bit flipped for v >= 0 and every bit
// flipped for v < 0, 64 bits for float64 and 32 for float32.  No finite value has the all-ones key, which an excluded row writes for
// its M pool keys and its rank key: they sort to the end of the segment, so a segment's size is fixed by the geometry and nothing
// is compacted.
//
// k_pm_keys is the only pass over the state.  A workgroup takes 256 consecutive rows of a slab per trip, reads their members as one
// contiguous stretch and writes the keys at the row's place in its segment: with h and w the patch's height and width,
//     pos = slab*ncol + Y*py*nx + X*h*px + (y - Y*py)*w + (x - X*px),
// closed form, so the kernels need no segment table.  The same place holds the row's rank key with the row as its payload.
//
// The sort is a segmented LSD radix sort, 8 bits a pass, stable, of 32- or 64-bit keys with or without a 32-bit payload: the pool
// (keys only, segments of n M keys) and the rank keys (payload, segments of n keys) go through the same kernels.  A BLOCK is a
// tile of at most kPmTile keys of one segment, a UNIT kPmUnit consecutive blocks of one segment; the host builds both tables.  One
// pass is four launches, ordered by the kernel boundaries alone (no workgroup waits for another):
//   k_pm_hist     the digit histogram of every block,
//   k_pm_usum     the sum of the histograms of every unit,
//   k_pm_segscan  per segment the exclusive scan over (digit, unit) of those sums,
//   k_pm_scatter  a block adds the histograms of the blocks before it in its unit, ranks its keys per digit in tile order (wave by
//                 wave: the lanes with the same digit find each other with eight ballots, the first of them takes the group's
//                 place from the wave's LDS counter) and stores them.
// Before the first pass k_pm_varbits ORs, over all keys, key ^ (first key of the segment): a byte that is zero there holds one digit
// in every segment and its pass is skipped.  The host reads that word once per batch; it is the only wait inside a call.
// The only atomics are integer: LDS counters whose sum is all that is read, the OR above and the n_bad counts.
#include "efa_device.h"
#include "efa_diag.h"
#include "efa_quadrow.h"

#include <cmath>
#include <vector>

namespace efa {
namespace {

constexpr int kPmThreads = 256;                     // 4 waves
constexpr int kPmWaves = kPmThreads / 64;
constexpr int kPmKpt = EFA_PM_TILE_KEYS / kPmThreads;  // keys of a thread: a wave holds 64 * kPmKpt consecutive keys of the tile
constexpr int kPmTile = EFA_PM_TILE_KEYS;           // keys of a block
constexpr int kPmUnit = EFA_PM_UNIT_BLOCKS;         // blocks of a unit
constexpr int kPmBlocks = 2048;                     // default grid cap of every kernel (option "pm_blocks" lowers it)
constexpr int kPmRows = 256;                        // rows of a trip of k_pm_keys

typedef unsigned long long u64;
typedef unsigned int u32;

struct PmBlk {   // a tile of one segment
  u64 start;     // its first key in the buffer
  u32 n;         // its keys, 1 .. kPmTile
  u32 seg;
  u32 unit;
  u32 ub0;       // the first block of its unit
};
struct PmUnit {
  u32 b0, nb;
};
struct PmSeg {
  u64 start, len;
  u32 u0, nu;
};

template <typename K>
struct PmKey;
template <>
struct PmKey<u64> {
  static __device__ __forceinline__ u64 enc(double v) {
    const u64 b = (u64)__double_as_longlong(v + 0.0);
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
  }
  static __device__ __forceinline__ double dec(u64 k) {
    return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
  }
};
template <>
struct PmKey<u32> {
  static __device__ __forceinline__ u32 enc(float v) {
    const u32 b = __float_as_uint(v + 0.0f);
    return b ^ ((b >> 31) ? ~0u : 0x80000000u);
  }
  static __device__ __forceinline__ double dec(u32 k) { return (double)__uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }
};

struct PmKeyArgs {
  const void* X;
  const double* f;       // [rows]
  const int* slabs;      // the batch's slabs
  long ncol, ntrips, tps;  // trips of the batch, trips per slab
  int ny, nx, py, px, M;
  void* pool;            // [R][M] keys
  u64* rkey;             // [R]
  u32* rpay;             // [R]: the row within the batch
  u64* nbad;             // [n_lead]
};

template <typename E, typename K>
__global__ __launch_bounds__(kPmThreads) void k_pm_keys(const PmKeyArgs a) {
  __shared__ u64 pos_s[kPmRows];
  __shared__ u32 bad_s[kPmRows];
  const int tid = threadIdx.x;
  const u32 M = (u32)a.M;
  K* pool = reinterpret_cast<K*>(a.pool);
#pragma unroll 1
  for (long t = blockIdx.x; t < a.ntrips; t += gridDim.x) {
    const long sb = t / a.tps;
    const long c0 = (t % a.tps) * kPmRows;
    const long lead = a.slabs[sb];
    const int nrow = (int)(a.ncol - c0 < kPmRows ? a.ncol - c0 : kPmRows);
    const long col = c0 + tid;
    u64 pos = 0;
    if (tid < nrow) {
      const int y = (int)(col / a.nx), x = (int)(col % a.nx);
      const int Y = y / a.py, X = x / a.px;
      const int h = a.ny - Y * a.py < a.py ? a.ny - Y * a.py : a.py;
      const int w = a.nx - X * a.px < a.px ? a.nx - X * a.px : a.px;
      pos = (u64)sb * a.ncol + (u64)Y * a.py * a.nx + (u64)X * h * a.px + (u64)(y - Y * a.py) * w + (u64)(x - X * a.px);
      pos_s[tid] = pos;
      bad_s[tid] = 0u;
    }
    __syncthreads();
    const E* p = reinterpret_cast<const E*>(a.X) + ((size_t)lead * a.ncol + c0) * M;
    const u32 total = (u32)nrow * M;
#pragma unroll 4
    for (u32 i = tid; i < total; i += kPmThreads) {
      const u32 rl = i / M, m = i - rl * M;
      const E v = p[i];
      if (!finite64((double)v)) bad_s[rl] = 1u;  // (every writer stores the same value)
      pool[pos_s[rl] * M + m] = PmKey<K>::enc(v);
    }
    __syncthreads();
    if (tid < nrow) {
      const double fv = a.f[(size_t)lead * a.ncol + col];
      const bool excl = bad_s[tid] != 0u || !finite64(fv);
      a.rkey[pos] = excl ? ~0ull : PmKey<u64>::enc(fv);
      a.rpay[pos] = (u32)(sb * a.ncol + col);
      if (excl) {  // rare: the row's pool keys once more, behind the barrier that orders them after the stores above
        atomicAdd(&a.nbad[lead], 1ull);
        for (u32 m = 0; m < M; ++m) pool[pos * M + m] = (K)~(K)0;
      }
    }
    __syncthreads();
  }
}

// OR over every key of key ^ (first key of its segment), into *mask
template <typename K>
__global__ __launch_bounds__(kPmThreads) void k_pm_varbits(const K* __restrict__ src, const PmBlk* __restrict__ blk, long nblk,
                                                         const PmSeg* __restrict__ seg, u64* mask) {
  const int tid = threadIdx.x;
  u64 acc = 0ull;
#pragma unroll 1
  for (long b = blockIdx.x; b < nblk; b += gridDim.x) {
    const PmBlk B = blk[b];
    const K first = src[seg[B.seg].start];
#pragma unroll 4
    for (u32 i = tid; i < B.n; i += kPmThreads) acc |= (u64)(src[B.start + i] ^ first);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc |= __shfl_xor(acc, off, 64);
  if ((tid & 63) == 0 && acc != 0ull) atomicOr(mask, acc);
}

template <typename K>
__global__ __launch_bounds__(kPmThreads) void k_pm_hist(const K* __restrict__ src, const PmBlk* __restrict__ blk, long nblk, int shift,
                                                      u32* __restrict__ hist) {
  __shared__ u32 h_s[256];
  const int tid = threadIdx.x;
#pragma unroll 1
  for (long b = blockIdx.x; b < nblk; b += gridDim.x) {
    const PmBlk B = blk[b];
    h_s[tid] = 0u;
    __syncthreads();
#pragma unroll 4
    for (u32 i = tid; i < B.n; i += kPmThreads) atomicAdd(&h_s[(u32)(src[B.start + i] >> shift) & 255u], 1u);
    __syncthreads();
    hist[(size_t)b * 256 + tid] = h_s[tid];
    __syncthreads();
  }
}

// thread d: the keys of digit d in every unit
__global__ __launch_bounds__(kPmThreads) void k_pm_usum(const u32* __restrict__ hist, const PmUnit* __restrict__ unit, long nunit,
                                                      u32* __restrict__ usum) {
  const int tid = threadIdx.x;
#pragma unroll 1
  for (long u = blockIdx.x; u < nunit; u += gridDim.x) {
    const PmUnit U = unit[u];
    u32 s = 0u;
#pragma unroll 8
    for (u32 i = 0; i < U.nb; ++i) s += hist[(size_t)(U.b0 + i) * 256 + tid];
    usum[(size_t)u * 256 + tid] = s;
  }
}

// per segment: ubase[unit][d] = the keys of the segment with a smaller digit, or with digit d in an earlier unit
__global__ __launch_bounds__(kPmThreads) void k_pm_segscan(const u32* __restrict__ usum, const PmSeg* __restrict__ seg, long nseg,
                                                         u64* __restrict__ ubase) {
  __shared__ u64 wave_s[kPmWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll 1
  for (long s = blockIdx.x; s < nseg; s += gridDim.x) {
    const PmSeg S = seg[s];
    u64 run = 0ull;
#pragma unroll 4
    for (u32 i = 0; i < S.nu; ++i) run += usum[(size_t)(S.u0 + i) * 256 + tid];
    // exclusive scan of the 256 totals: within the wave, then over the waves
    u64 inc = run;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u64 up = __shfl_up(inc, off, 64);
      inc += lane >= off ? up : 0ull;
    }
    __syncthreads();
    if (lane == 63) wave_s[wv] = inc;
    __syncthreads();
    u64 base = inc - run;
    for (int w = 0; w < wv; ++w) base += wave_s[w];
#pragma unroll 1
    for (u32 i = 0; i < S.nu; ++i) {
      ubase[(size_t)(S.u0 + i) * 256 + tid] = base;
      base += usum[(size_t)(S.u0 + i) * 256 + tid];
    }
  }
}

template <typename K, bool PAY>
__global__ __launch_bounds__(kPmThreads) void k_pm_scatter(const K* __restrict__ src, K* __restrict__ dst, const u32* __restrict__ psrc,
                                                         u32* __restrict__ pdst, const PmBlk* __restrict__ blk, long nblk,
                                                         const PmSeg* __restrict__ seg, const u32* __restrict__ hist,
                                                         const u64* __restrict__ ubase, int shift) {
  __shared__ u32 cnt_s[kPmWaves][256];
  __shared__ u64 base_s[kPmWaves][256];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const u64 below = (1ull << lane) - 1ull;
#pragma unroll 1
  for (long b = blockIdx.x; b < nblk; b += gridDim.x) {
    const PmBlk B = blk[b];
    const PmSeg S = seg[B.seg];
    // thread d: where digit d of this block starts in its segment
    u64 gb = ubase[(size_t)B.unit * 256 + tid];
#pragma unroll 4
    for (u32 bb = B.ub0; bb < (u32)b; ++bb) gb += hist[(size_t)bb * 256 + tid];
#pragma unroll
    for (int w = 0; w < kPmWaves; ++w) cnt_s[w][tid] = 0u;
    __syncthreads();

    K key[kPmKpt];
    u32 pay[kPmKpt];
    u32 loc[kPmKpt];
    const u32 t0 = (u32)wv * 64u * kPmKpt + (u32)lane;
#pragma unroll
    for (int j = 0; j < kPmKpt; ++j) {
      const u32 i = t0 + 64u * j;
      const bool ok = i < B.n;
      key[j] = ok ? src[B.start + i] : (K)0;
      if constexpr (PAY) pay[j] = ok ? psrc[B.start + i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kPmKpt; ++j) {
      const bool ok = t0 + 64u * j < B.n;
      const u32 d = (u32)(key[j] >> shift) & 255u;
      u64 m = __ballot(ok);  // the lanes of this round with the same digit
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const bool one = (d >> bit) & 1u;
        const u64 v = __ballot(ok && one);
        m &= one ? v : ~v;
      }
      m = ok ? m : 0ull;
      const int leader = ok ? __builtin_ctzll(m) : lane;
      u32 old = 0u;
      if (ok && lane == leader) old = atomicAdd(&cnt_s[wv][d], (u32)__popcll(m));
      old = __shfl(old, leader, 64);
      loc[j] = old + (u32)__popcll(m & below);
    }
    __syncthreads();
    {
      u64 run = gb;
#pragma unroll
      for (int w = 0; w < kPmWaves; ++w) {
        base_s[w][tid] = run;
        run += cnt_s[w][tid];
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPmKpt; ++j) {
      const bool ok = t0 + 64u * j < B.n;
      const u32 d = (u32)(key[j] >> shift) & 255u;
      const u64 pos = base_s[wv][d] + loc[j];
      if (ok && pos < S.len) {  // (pos < len whenever hist is this pass's histogram of src)
        dst[S.start + pos] = key[j];
        if constexpr (PAY) pdst[S.start + pos] = pay[j];
      }
    }
    __syncthreads();
  }
}

// position q of the sorted rank keys: the row that sits there gets pool key q M + g
template <typename K>
__global__ __launch_bounds__(kPmThreads) void k_pm_assign(const K* __restrict__ pool, const u64* __restrict__ rkey,
                                                        const u32* __restrict__ rpay, const int* __restrict__ slabs, long R, long ncol,
                                                        int M, int g, double* __restrict__ pm) {
  for (long q = (long)blockIdx.x * kPmThreads + threadIdx.x; q < R; q += (long)gridDim.x * kPmThreads) {
    const u32 r = rpay[q];
    if ((long)r >= R) continue;  // (never: the payloads are a permutation of the batch's rows)
    const long sb = r / ncol, col = r % ncol;
    pm[(size_t)slabs[sb] * ncol + col] = rkey[q] == ~0ull ? __builtin_nan("") : PmKey<K>::dec(pool[(size_t)q * M + g]);
  }
}

// the rows of the slabs that are not read
__global__ __launch_bounds__(kPmThreads) void k_pm_unread(long rows, long ncol, const int* __restrict__ active, double* __restrict__ pm) {
  for (long i = (long)blockIdx.x * kPmThreads + threadIdx.x; i < rows; i += (long)gridDim.x * kPmThreads)
    if (!active[i / ncol]) pm[i] = __builtin_nan("");
}

inline unsigned pm_grid(long n, long blocks) { return (unsigned)(n < blocks ? (n < 1 ? 1 : n) : blocks); }

// The blocks, units and segments of a buffer whose segments have the given lengths (in keys), in order.
struct PmTables {
  std::vector<PmBlk> blk;
  std::vector<PmUnit> unit;
  std::vector<PmSeg> seg;
  void add_segment(u64 len) {
    PmSeg S;
    S.start = seg.empty() ? 0ull : seg.back().start + seg.back().len;
    S.len = len;
    S.u0 = (u32)unit.size();
    for (u64 off = 0; off < len; off += kPmTile) {
      if (unit.size() == S.u0 || unit.back().nb == (u32)kPmUnit) unit.push_back(PmUnit{(u32)blk.size(), 0u});
      PmBlk B;
      B.start = S.start + off;
      B.n = (u32)(len - off < (u64)kPmTile ? len - off : (u64)kPmTile);
      B.seg = (u32)seg.size();
      B.unit = (u32)unit.size() - 1u;
      B.ub0 = unit.back().b0;
      blk.push_back(B);
      ++unit.back().nb;
    }
    S.nu = (u32)unit.size() - S.u0;
    seg.push_back(S);
  }
};

// what a sort of the first `nseg` segments of a table needs on the device
struct PmDevTables {
  const PmBlk* blk;
  const PmUnit* unit;
  const PmSeg* seg;
  long nblk, nunit, nseg;
};

struct PmScratch {
  u32* hist;   // [blocks][256]
  u32* usum;   // [units][256]
  u64* ubase;  // [units][256]
};

// the passes whose byte varies in `mask`, lowest first; returns the buffer (0: a, 1: b) that holds the result
template <typename K, bool PAY>
hipError_t pm_sort(K* a, K* b, u32* pa, u32* pb, const PmDevTables& t, const PmScratch& w, u64 mask, long blocks, hipStream_t s,
                   int* where, int* passes) {
  int cur = 0;
  for (int p = 0; p < (int)sizeof(K); ++p) {
    if (((mask >> (8 * p)) & 255ull) == 0ull) continue;
    const int shift = 8 * p;
    K* src = cur ? b : a;
    K* dst = cur ? a : b;
    u32* ps = cur ? pb : pa;
    u32* pd = cur ? pa : pb;
    hipLaunchKernelGGL(k_pm_hist<K>, dim3(pm_grid(t.nblk, blocks)), dim3(kPmThreads), 0, s, src, t.blk, t.nblk, shift, w.hist);
    hipLaunchKernelGGL(k_pm_usum, dim3(pm_grid(t.nunit, blocks)), dim3(kPmThreads), 0, s, w.hist, t.unit, t.nunit, w.usum);
    hipLaunchKernelGGL(k_pm_segscan, dim3(pm_grid(t.nseg, blocks)), dim3(kPmThreads), 0, s, w.usum, t.seg, t.nseg, w.ubase);
    hipLaunchKernelGGL((k_pm_scatter<K, PAY>), dim3(pm_grid(t.nblk, blocks)), dim3(kPmThreads), 0, s, src, dst, ps, pd, t.blk, t.nblk,
                       t.seg, w.hist, w.ubase, shift);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    cur ^= 1;
    ++*passes;
  }
  *where = cur;
  return hipSuccess;
}

}  // namespace
}  // namespace efa

// ---- the host side of efa_pm_mean_dev / efa_pm_mean_f32_dev --------------------------------------------------------------------
namespace efa_host {

using namespace efa;

// The call works in a buffer of its own (pm_ws) and neither reads nor writes what a later cycle reads.  Nothing is written to the
// caller's arrays before every check has passed.
int pm_mean(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, long ny, long nx, long n_lead, const double* rank_dev,
            const int* slab_on, long py, long px, int pick, double* pm_dev, long long* n_bad) {
  const char* me = elem == Elem::f32 ? "efa_pm_mean_f32_dev" : "efa_pm_mean_dev";
  if (!X_dev || !rank_dev || !pm_dev || !n_bad) return fail(EFA_ERR_INVALID, "%s: null X_dev, rank_dev, pm_dev or n_bad", me);
  if (M < 2 || M > kMaxMembers) return fail(EFA_ERR_INVALID, "%s: M=%d must be in [2,%d]", me, M, kMaxMembers);
  if (rows < 0 || ny < 0 || nx < 0 || n_lead < 0) return fail(EFA_ERR_INVALID, "%s: negative size", me);
  if (ny > (1L << 30) || nx > (1L << 30) || n_lead * ny * nx != rows)
    return fail(EFA_ERR_INVALID, "%s: rows=%ld must equal n_lead*ny*nx = %ld*%ld*%ld", me, rows, n_lead, ny, nx);
  if (py < 1 || py > ny) return fail(EFA_ERR_INVALID, "%s: py=%ld must be in [1,ny=%ld]", me, py, ny);
  if (px < 1 || px > nx) return fail(EFA_ERR_INVALID, "%s: px=%ld must be in [1,nx=%ld]", me, px, nx);
  if (pick < 0 || pick >= M) return fail(EFA_ERR_INVALID, "%s: pick=%d must be in [0,M=%d)", me, pick, M);
  const long ncol = ny * nx;
  if (ncol >= (1L << 32) || n_lead > (1L << 30)) return fail(EFA_ERR_INVALID, "%s: a slab of %ld rows is beyond the 32-bit row payload", me, ncol);

  c->pm_us = 0;
  c->pm_passes = c->pm_rank_passes = 0;
  std::vector<u64> h_nbad((size_t)n_lead, 0ull);
  if (rows > 0) {
    hipStream_t s = c->stream;
    const size_t ksize = elem_size(elem);
    std::vector<int> h_act((size_t)n_lead, 0), h_slabs;
    for (long l = 0; l < n_lead; ++l)
      if (!slab_on || slab_on[l]) {
        h_act[l] = 1;
        h_slabs.push_back((int)l);
      }
    const long nact = (long)h_slabs.size();
    // the segments of one slab, in the order of their place: bands of patches, the patches of a band from left to right
    const long npy = (ny + py - 1) / py, npx = (nx + px - 1) / px;
    const long seg_slab = npy * npx;
    // a batch: its two pooled buffers fit the cap, its rows the 32-bit payload; at least one slab
    size_t cap = (size_t)EFA_PM_WS_BYTES;
    if (c->pm_ws_bytes > 0 && (size_t)c->pm_ws_bytes < cap) cap = (size_t)c->pm_ws_bytes;
    long per_batch = (long)(cap / (2 * ksize * (size_t)M * (size_t)ncol));
    if (per_batch > ((1L << 32) - 1) / ncol) per_batch = ((1L << 32) - 1) / ncol;
    {  // ... and so do its histograms and scans: 16 bytes per digit of every block, a block per tile and at least one per segment
      size_t blk_slab = 0;
      for (long Y = 0; Y < npy; ++Y) {
        const long h = ny - Y * py < py ? ny - Y * py : py;
        for (long X = 0; X < npx; ++X) {
          const long w = nx - X * px < px ? nx - X * px : px;
          blk_slab += ((size_t)(h * w) * (size_t)M + kPmTile - 1) / kPmTile;
        }
      }
      const long fit = (long)(cap / (blk_slab * 256 * 16));
      if (per_batch > fit) per_batch = fit;
    }
    if (per_batch < 1) per_batch = 1;
    if (per_batch > nact) per_batch = nact > 0 ? nact : 1;
    // the tables of a full batch; a shorter last batch uses their leading part (slab after slab, nothing straddles a slab)
    PmTables tp, tr;  // the pool's and the rank keys'
    std::vector<long> pool_cut((size_t)per_batch + 1, 0), rank_cut((size_t)per_batch + 1, 0);  // blocks up to each slab
    std::vector<long> pool_ucut((size_t)per_batch + 1, 0), rank_ucut((size_t)per_batch + 1, 0);
    if (nact > 0) {
      for (long sb = 0; sb < per_batch; ++sb) {
        for (long Y = 0; Y < npy; ++Y) {
          const long h = ny - Y * py < py ? ny - Y * py : py;
          for (long X = 0; X < npx; ++X) {
            const long w = nx - X * px < px ? nx - X * px : px;
            tp.add_segment((u64)(h * w) * (u64)M);
            tr.add_segment((u64)(h * w));
          }
        }
        pool_cut[sb + 1] = (long)tp.blk.size();
        rank_cut[sb + 1] = (long)tr.blk.size();
        pool_ucut[sb + 1] = (long)tp.unit.size();
        rank_ucut[sb + 1] = (long)tr.unit.size();
      }
    }
    const size_t Rmax = nact > 0 ? (size_t)per_batch * ncol : 0;
    const size_t nblk = tp.blk.size() > tr.blk.size() ? tp.blk.size() : tr.blk.size();
    const size_t nunit = tp.unit.size() > tr.unit.size() ? tp.unit.size() : tr.unit.size();
    // pm_ws: pool a | pool b | rank keys a, b | rank payloads a, b | hist | usum | ubase | the two tables | n_bad | masks | slabs, flags
    // (every region starts on a 256-byte boundary)
    WsLayout ws(256);
    const auto r_pool_a = ws.add<char>(Rmax * M * ksize), r_pool_b = ws.add<char>(Rmax * M * ksize);
    const auto r_rk_a = ws.add<u64>(Rmax), r_rk_b = ws.add<u64>(Rmax);
    const auto r_rp_a = ws.add<u32>(Rmax), r_rp_b = ws.add<u32>(Rmax);
    const auto r_hist = ws.add<u32>(nblk * 256), r_usum = ws.add<u32>(nunit * 256);
    const auto r_ubase = ws.add<u64>(nunit * 256);
    const auto r_pblk = ws.add<PmBlk>(tp.blk.size());
    const auto r_punit = ws.add<PmUnit>(tp.unit.size());
    const auto r_pseg = ws.add<PmSeg>(tp.seg.size());
    const auto r_rblk = ws.add<PmBlk>(tr.blk.size());
    const auto r_runit = ws.add<PmUnit>(tr.unit.size());
    const auto r_rseg = ws.add<PmSeg>(tr.seg.size());
    const auto r_nbad = ws.add<u64>((size_t)n_lead), r_mask = ws.add<u64>(2);
    const auto r_act = ws.add<int>((size_t)n_lead), r_slabs = ws.add<int>((size_t)nact);
    EFA_TRY(c->pm_ws.reserve(ws.bytes()));
    const DevBuf& b = c->pm_ws;
    char *pool_a = r_pool_a(b), *pool_b = r_pool_b(b);
    u64 *rk_a = r_rk_a(b), *rk_b = r_rk_b(b);
    u32 *rp_a = r_rp_a(b), *rp_b = r_rp_b(b);
    PmScratch w;
    w.hist = r_hist(b);
    w.usum = r_usum(b);
    w.ubase = r_ubase(b);
    PmBlk *d_pblk = r_pblk(b), *d_rblk = r_rblk(b);
    PmUnit *d_punit = r_punit(b), *d_runit = r_runit(b);
    PmSeg *d_pseg = r_pseg(b), *d_rseg = r_rseg(b);
    u64 *d_nbad = r_nbad(b), *d_mask = r_mask(b);
    int *d_act = r_act(b), *d_slabs = r_slabs(b);
    if (nact > 0) {
      EFA_HIP(hipMemcpyAsync(d_pblk, tp.blk.data(), tp.blk.size() * sizeof(PmBlk), hipMemcpyHostToDevice, s));
      EFA_HIP(hipMemcpyAsync(d_punit, tp.unit.data(), tp.unit.size() * sizeof(PmUnit), hipMemcpyHostToDevice, s));
      EFA_HIP(hipMemcpyAsync(d_pseg, tp.seg.data(), tp.seg.size() * sizeof(PmSeg), hipMemcpyHostToDevice, s));
      EFA_HIP(hipMemcpyAsync(d_rblk, tr.blk.data(), tr.blk.size() * sizeof(PmBlk), hipMemcpyHostToDevice, s));
      EFA_HIP(hipMemcpyAsync(d_runit, tr.unit.data(), tr.unit.size() * sizeof(PmUnit), hipMemcpyHostToDevice, s));
      EFA_HIP(hipMemcpyAsync(d_rseg, tr.seg.data(), tr.seg.size() * sizeof(PmSeg), hipMemcpyHostToDevice, s));
      EFA_HIP(hipMemcpyAsync(d_slabs, h_slabs.data(), (size_t)nact * sizeof(int), hipMemcpyHostToDevice, s));
    }
    EFA_HIP(hipMemcpyAsync(d_act, h_act.data(), (size_t)n_lead * sizeof(int), hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemsetAsync(d_nbad, 0, (size_t)n_lead * sizeof(u64), s));
    const long blocks = clamp_blocks(c->pm_blocks, kPmBlocks);

    PmKeyArgs ka{};
    ka.X = X_dev;
    ka.f = rank_dev;
    ka.ncol = ncol;
    ka.tps = (ncol + kPmRows - 1) / kPmRows;
    ka.ny = (int)ny;
    ka.nx = (int)nx;
    ka.py = (int)py;
    ka.px = (int)px;
    ka.M = M;
    ka.pool = pool_a;
    ka.rkey = rk_a;
    ka.rpay = rp_a;
    ka.nbad = d_nbad;

    EFA_TRY(interval_begin(c->pm_iv, s));
    if (nact < n_lead) {
      hipLaunchKernelGGL(k_pm_unread, dim3(pm_grid((rows + kPmThreads - 1) / kPmThreads, blocks)), dim3(kPmThreads), 0, s, rows, ncol,
                         d_act, pm_dev);
      EFA_HIP(hipGetLastError());
    }
    for (long s0 = 0; s0 < nact; s0 += per_batch) {
      const long nb = s0 + per_batch < nact ? per_batch : nact - s0;
      const long R = nb * ncol;
      const PmDevTables dp{d_pblk, d_punit, d_pseg, pool_cut[nb], pool_ucut[nb], nb * seg_slab};
      const PmDevTables dr{d_rblk, d_runit, d_rseg, rank_cut[nb], rank_ucut[nb], nb * seg_slab};
      ka.slabs = d_slabs + s0;
      ka.ntrips = nb * ka.tps;
      EFA_HIP(hipMemsetAsync(d_mask, 0, 2 * sizeof(u64), s));
      if (elem == Elem::f32) {
        hipLaunchKernelGGL((k_pm_keys<float, u32>), dim3(pm_grid(ka.ntrips, blocks)), dim3(kPmThreads), 0, s, ka);
        hipLaunchKernelGGL(k_pm_varbits<u32>, dim3(pm_grid(dp.nblk, blocks)), dim3(kPmThreads), 0, s,
                           reinterpret_cast<const u32*>(pool_a), dp.blk, dp.nblk, dp.seg, d_mask);
      } else {
        hipLaunchKernelGGL((k_pm_keys<double, u64>), dim3(pm_grid(ka.ntrips, blocks)), dim3(kPmThreads), 0, s, ka);
        hipLaunchKernelGGL(k_pm_varbits<u64>, dim3(pm_grid(dp.nblk, blocks)), dim3(kPmThreads), 0, s,
                           reinterpret_cast<const u64*>(pool_a), dp.blk, dp.nblk, dp.seg, d_mask);
      }
      hipLaunchKernelGGL(k_pm_varbits<u64>, dim3(pm_grid(dr.nblk, blocks)), dim3(kPmThreads), 0, s, rk_a, dr.blk, dr.nblk, dr.seg,
                         d_mask + 1);
      EFA_HIP(hipGetLastError());
      u64 h_mask[2] = {0ull, 0ull};
      EFA_HIP(hipMemcpyAsync(h_mask, d_mask, sizeof(h_mask), hipMemcpyDeviceToHost, s));
      EFA_HIP(hipStreamSynchronize(s));  // the bytes that vary decide the passes
      int wp = 0, wr = 0, np = 0, nr = 0;
      if (elem == Elem::f32)
        EFA_HIP((pm_sort<u32, false>(reinterpret_cast<u32*>(pool_a), reinterpret_cast<u32*>(pool_b), nullptr, nullptr, dp, w, h_mask[0],
                                     blocks, s, &wp, &np)));
      else
        EFA_HIP((pm_sort<u64, false>(reinterpret_cast<u64*>(pool_a), reinterpret_cast<u64*>(pool_b), nullptr, nullptr, dp, w, h_mask[0],
                                     blocks, s, &wp, &np)));
      EFA_HIP((pm_sort<u64, true>(rk_a, rk_b, rp_a, rp_b, dr, w, h_mask[1], blocks, s, &wr, &nr)));
      c->pm_passes += np;
      c->pm_rank_passes += nr;
      const unsigned ag = pm_grid((R + kPmThreads - 1) / kPmThreads, blocks);
      if (elem == Elem::f32)
        hipLaunchKernelGGL(k_pm_assign<u32>, dim3(ag), dim3(kPmThreads), 0, s, reinterpret_cast<const u32*>(wp ? pool_b : pool_a),
                           wr ? rk_b : rk_a, wr ? rp_b : rp_a, d_slabs + s0, R, ncol, M, pick, pm_dev);
      else
        hipLaunchKernelGGL(k_pm_assign<u64>, dim3(ag), dim3(kPmThreads), 0, s, reinterpret_cast<const u64*>(wp ? pool_b : pool_a),
                           wr ? rk_b : rk_a, wr ? rp_b : rp_a, d_slabs + s0, R, ncol, M, pick, pm_dev);
      EFA_HIP(hipGetLastError());
    }
    EFA_TRY(interval_end(c->pm_iv, s));
    EFA_HIP(hipMemcpyAsync(h_nbad.data(), d_nbad, (size_t)n_lead * sizeof(u64), hipMemcpyDeviceToHost, s));
    EFA_HIP(hipStreamSynchronize(s));
    EFA_TRY(interval_us(c->pm_iv, &c->pm_us));
  }
  for (long l = 0; l < n_lead; ++l) n_bad[l] = (long long)h_nbad[l];
  return EFA_OK;
}

}  // namespace efa_host
