// Neighbourhood ensemble probabilities and the fractions skill score (Schwartz et al. 2010; Schwartz and Sobash 2017; Roberts and
// Lean 2008).
//   Row i = lead*ncol + y*nx + x with members x_i1..x_iM.  A row is VALID when every member is finite and, in a call with a
//   verifying value, y_i is finite.  Over the valid rows i' of the window W_r(y, x) of one slab (a square or a disc of radius r, cut
//   at the slab's edges, columns taken modulo nx when wrap_x is set), with k = #{m: x_m > t}:
//     NEP  = (double)(sum k_i') / ((double)M * (double)#{i'}),  NMEP = (double)#{m: some i' has x_i'm > t} / (double)M,
//     O    = (double)(sum (y_i' > t)) / (double)#{i'},
//   and per group of slabs, radius and threshold the sums of w, w (NEP - O)^2, w NEP^2, w O^2, w NEP, w O over the scored centres.
//   Everything is integer arithmetic up to the one division of a field.
//
// k_nbr_records is the only pass over the state.  It reads the rows in the four-lane row layout (efa_quadrow.h): lane g of a row
// holds members {8u+2g, 8u+2g+1}, so member m = 8u + 2g + e is bit 8(u & 7) + 2g + e of mask word u >> 3.  A lane builds its bits of every word, two __shfl_xor steps OR the
// four lanes of a row together, and k is the popcount.  Per row and threshold it leaves in the call's workspace a 16-bit k, and the
// mask words when NMEP is wanted; per row a 16-bit flag word: bit 0 valid, bit 1 "would be scored but has a member that is not
// finite", bit 8 + j the event o_j = (y > t_j).  An invalid row has k = 0, mask = 0 and no event bit: it adds nothing to a window.
//
// k_nbr_windows<HALO> takes one tile of kNbrTY x kNbrTX centres of one slab per workgroup and trip.  Per threshold the tile and its
// halo are staged in LDS as one 32-bit word per cell, k << 16 | o << 8 | valid, cells outside the slab as 0, and every LDS row is
// turned into its exclusive prefix sum by the wave that owns it (no field can carry into the next: a staged row has at most 192
// cells, so sum k <= 192*256 < 2^16 and the two counts <= 192 < 2^8).  A window sum is then a loop over dy of one difference of
// two prefix words, whatever the shape: the half-width of every |dy| comes with the arguments.  The mask OR runs over one 32-bit
// half of a mask word at a time in the same LDS array: level L of a doubling table (cell x holds the OR of cells x .. x + 2^L - 1
// of its row) is built in place from level L - 1, again by the wave that owns the row, and at level L a centre ORs in, for every dy
// whose span 2h + 1 has floor(log2) = L, the two table entries that cover the span.  Both cost O(2r + 1) per centre.
//
// Sums: a thread adds up its kNbrTY*kNbrTX/256 centres in index order, the workgroup adds its threads with a fixed butterfly and
// writes the tile's partial; k_group_reduce (efa_quadreduce.h) adds the partials of each group in a fixed order.  Tiles, not workgroups, own the
// partials, so the grid and the batching of the slabs change no bit.  No floating-point atomics.
#include "efa_device.h"
#include "efa_diag.h"
#include "efa_quadreduce.h"

#include <cmath>
#include <vector>

namespace efa {
namespace {

constexpr int kNbrThreads = kQuadThreads;
constexpr int kNbrBlocks = 2048;       // default grid cap of both kernels (option "neighbourhood_blocks" lowers it)
constexpr int kNbrMaxThr = EFA_NBR_MAX_THRESHOLDS;
constexpr int kNbrMaxRad = EFA_NBR_MAX_RADII;
constexpr int kNbrMaxR = EFA_NBR_MAX_RADIUS;
constexpr int kNbrTY = 16, kNbrTX = 64;  // centres of a tile
constexpr int kNbrSums = 6;            // sum w, w (P-O)^2, w P^2, w O^2, w P, w O
constexpr int kNbrCells = kNbrTY * kNbrTX / kNbrThreads;  // centres of a thread: rows wave, wave + 4, ... of the tile

struct NbrRecArgs {
  const void* X;
  const double* verif;   // [rows] or null
  const double* thr;     // [n_lead][kNbrMaxThr], device copy, NaN beyond nt
  const int* slabs;      // the batch's slabs
  long ncol, R;          // R: rows of the batch's records (slabs of the batch * ncol)
  long ntiles, tps;      // 16-row tiles of the batch, tiles per slab
  int M, al, nt, nw;     // nw = ceil(M / 64)
  unsigned short* flag;  // [R]
  unsigned short* k16;   // [nt][R]
  unsigned long long* mask;  // [nt][nw][R] (MASK only)
};

struct NbrWinArgs {
  const unsigned short* flag;
  const unsigned short* k16;
  const unsigned long long* mask;
  const double* thr;
  const int* sgroup;     // [n_lead], or null: nothing is scored
  const int* slabs;
  const double* colw;    // [ncol] or null
  long ncol, R, rows;
  long tile0, ntiles;    // the batch's first tile among the call's, its tiles
  int ny, nx, tyn, txn;  // tiles of a slab in y and x
  int M, nt, nw, nr, wrap;
  int hy, hx;            // the halo staged in y and x: the largest radius, cut to the grid
  int lmax;              // the highest level of the doubling table any span needs
  int ry[kNbrMaxRad];    // |dy| <= ry
  unsigned char hw[kNbrMaxRad][kNbrMaxR + 1];  // half-width of every |dy|, cut to hx
  double* nep;           // [nr][nt][rows] or null
  double* nmep;          // [nr][nt][rows] or null
  double* part;          // [tiles of the call][nr][nt][kNbrSums]
  long long* cnt;        // [tiles of the call][nr][nt][2]: scored centres, bad ones that would be scored
};

// the waves of a workgroup own whole LDS rows: what one lane wrote, another lane of the same wave may read behind this
__device__ __forceinline__ void nbr_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// NU: chunks of 8 members the lanes hold, (M + 7) / 8 rounded up to a power of two, as in k_products
template <int NU, typename E, bool MASK>
__global__ __launch_bounds__(kNbrThreads) void k_nbr_records(const NbrRecArgs a) {
  constexpr int LP = 2 * NU;
  constexpr int NW = (NU + 7) / 8;
  const int M = a.M;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = lane & 15;
  const bool ver = a.verif != nullptr;
  const long nwaves = (long)gridDim.x * (kNbrThreads / 64);

#pragma unroll 1
  for (long tl = (long)blockIdx.x * (kNbrThreads / 64) + wv; tl < a.ntiles; tl += nwaves) {
    const long sb = tl / a.tps, tt = tl % a.tps;
    const long lead = a.slabs[sb];
    const long col = tt * 16 + n;
    const bool live = col < a.ncol;
    const long colc = live ? col : a.ncol - 1;
    const long r = lead * a.ncol + colc;
    const size_t rec = (size_t)sb * a.ncol + colc;
    const int gq = quad_lane_quarter(lane);
    // (the loader and the count's row sum are written out, not taken from efa_quadrow.h: only so is the code the one measured
    // before the layout was shared, DESIGN.md 7j2.  The text is quad_load_row's and quad_row_sum's.)
    double d[LP];
    {
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
    const double y = ver ? a.verif[r] : 0.0;
    bool badl = false;
#pragma unroll
    for (int c = 0; c < LP; ++c) badl = badl || (quad_slot_ok(c, gq, M) && !finite64(d[c]));
    const bool bad = quad_row_any(badl, n);
    const bool yfin = !ver || finite64(y);
    const bool valid = !bad && yfin;
    unsigned int flags = (valid ? 1u : 0u) | ((bad && ver && yfin) ? 2u : 0u);
    const double* thr = a.thr + (size_t)lead * kNbrMaxThr;

#pragma unroll 1
    for (int j = 0; j < a.nt; ++j) {
      const double t = thr[j];  // (uniform; NaN: every comparison is false)
      int k = 0;
      if constexpr (MASK) {
        unsigned long long wd[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) wd[w] = 0ull;
#pragma unroll
        for (int c = 0; c < LP; ++c) {  // the lane's bits as lane g = 0 would hold them, moved to their place by one shift below
          const int u = c >> 1;
          wd[u >> 3] |= (quad_slot_ok(c, gq, M) && d[c] > t) ? 1ull << (8 * (u & 7) + (c & 1)) : 0ull;
        }
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          unsigned long long v = wd[w] << (2 * gq);
          v |= __shfl_xor(v, 16, 64);
          v |= __shfl_xor(v, 32, 64);
          k += __popcll(v);
          if (gq == (w & 3) && live && w < a.nw) a.mask[((size_t)j * a.nw + w) * a.R + rec] = valid ? v : 0ull;
        }
      } else {
#pragma unroll
        for (int c = 0; c < LP; ++c) k += (quad_slot_ok(c, gq, M) && d[c] > t) ? 1 : 0;
        k += __shfl_xor(k, 16, 64);
        k += __shfl_xor(k, 32, 64);
      }
      if (gq == 1 && live) a.k16[(size_t)j * a.R + rec] = (unsigned short)(valid ? k : 0);
      if (ver && valid && y > t) flags |= 1u << (8 + j);
    }
    if (gq == 0 && live) a.flag[rec] = (unsigned short)flags;
  }
}

// HALO: the largest halo the LDS array is laid out for
template <int HALO>
__global__ __launch_bounds__(kNbrThreads) void k_nbr_windows(const NbrWinArgs a) {
  constexpr int LW = kNbrTX + 2 * HALO + 1;        // words of an LDS row: the staged cells and the prefix sum's leading 0
  constexpr int LH = kNbrTY + 2 * HALO;
  constexpr int CPL = (kNbrTX + 2 * HALO + 63) / 64;  // staged cells of a row per lane
  __shared__ unsigned int P[LH * LW];
  __shared__ double red_s[kNbrThreads / 64][kNbrSums];
  __shared__ int redc_s[kNbrThreads / 64][2];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int hy = a.hy, hx = a.hx;
  const int SW = kNbrTX + 2 * hx, SH = kNbrTY + 2 * hy;
  const int nh = (a.M + 31) / 32;  // 32-bit halves of the mask words in use
  const long tps = (long)a.tyn * a.txn;
  const double nan = __builtin_nan("");
  const double dM = (double)a.M;
  const int cx = lane + hx;  // the centre's staged column

#pragma unroll 1
  for (long tl = blockIdx.x; tl < a.ntiles; tl += gridDim.x) {
    const long sb = tl / tps;
    const int trem = (int)(tl % tps);
    const int y0 = (trem / a.txn) * kNbrTY, x0 = (trem % a.txn) * kNbrTX;
    const long lead = a.slabs[sb];
    const int sg = a.sgroup ? a.sgroup[lead] : -1;
    const bool score = sg >= 0;  // (uniform)
    const int gx = x0 + lane;
    // the thread's centres: rows wv + 4 i of the tile, column lane
    long crow[kNbrCells];   // the centre's column of the slab, -1 beyond the grid
    double cw[kNbrCells];
    unsigned int cflag[kNbrCells];
#pragma unroll
    for (int i = 0; i < kNbrCells; ++i) {
      const int gy = y0 + wv + 4 * i;
      const bool in = gy < a.ny && gx < a.nx;
      crow[i] = in ? (long)gy * a.nx + gx : -1;
      cw[i] = 1.0;
      cflag[i] = 0u;
      if (in && score) {
        if (a.colw) cw[i] = a.colw[crow[i]];
        cflag[i] = a.flag[(size_t)sb * a.ncol + crow[i]];
      }
    }

#pragma unroll 1
    for (int j = 0; j < a.nt; ++j) {
      const double t = a.thr[(size_t)lead * kNbrMaxThr + j];
      if (!finite64(t)) {  // (uniform) no threshold j in this slab: NaN fields, nothing scored
#pragma unroll 1
        for (int ri = 0; ri < a.nr; ++ri)
#pragma unroll
          for (int i = 0; i < kNbrCells; ++i)
            if (crow[i] >= 0) {
              const size_t o = ((size_t)ri * a.nt + j) * a.rows + lead * a.ncol + crow[i];
              if (a.nep) a.nep[o] = nan;
              if (a.nmep) a.nmep[o] = nan;
            }
        continue;
      }

      // ---- the packed cells of the tile and its halo, every LDS row as its exclusive prefix sum ---------------------------------
      __syncthreads();
#pragma unroll 1
      for (int sy = wv; sy < SH; sy += kNbrThreads / 64) {
        const int gy = y0 - hy + sy;
        const bool yin = gy >= 0 && gy < a.ny;
        unsigned int carry = 0u;
        if (lane == 0) P[sy * LW] = 0u;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
          const int c = lane + 64 * i;
          int sx = x0 - hx + c;
          bool in = yin && c < SW;
          if (a.wrap) {
            sx %= a.nx;
            sx += sx < 0 ? a.nx : 0;
          } else {
            in = in && sx >= 0 && sx < a.nx;
          }
          unsigned int v = 0u;
          if (in) {
            const size_t rec = (size_t)sb * a.ncol + (size_t)gy * a.nx + sx;
            const unsigned int f = a.flag[rec];
            if (f & 1u) v = ((unsigned int)a.k16[(size_t)j * a.R + rec] << 16) | (((f >> (8 + j)) & 1u) << 8) | 1u;
          }
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) {
            const unsigned int up = __shfl_up(v, off, 64);
            v += lane >= off ? up : 0u;
          }
          v += carry;
          carry = __shfl(v, 63, 64);
          if (c < SW) P[sy * LW + c + 1] = v;
        }
      }
      __syncthreads();

      unsigned int cvalid = 0u;  // bit i: centre i is valid
#pragma unroll
      for (int i = 0; i < kNbrCells; ++i) {
        const int row = (wv + 4 * i + hy) * LW;
        cvalid |= ((P[row + cx + 1] - P[row + cx]) & 1u) << i;
      }

      if (a.nep || score) {
#pragma unroll 1
        for (int ri = 0; ri < a.nr; ++ri) {
          const int ry = a.ry[ri];
          double acc[kNbrSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
          int n_sc = 0, n_bad = 0;
#pragma unroll
          for (int i = 0; i < kNbrCells; ++i) {
            const int row0 = (wv + 4 * i + hy) * LW + cx;
            unsigned int S = 0u, nv = 0u, So = 0u;
#pragma unroll 1
            for (int dy = -ry; dy <= ry; ++dy) {
              const int h = a.hw[ri][dy < 0 ? -dy : dy];
              const unsigned int dd = P[row0 + dy * LW + h + 1] - P[row0 + dy * LW - h];
              S += dd >> 16;
              So += (dd >> 8) & 0xFFu;
              nv += dd & 0xFFu;
            }
            const bool ok = (cvalid >> i) & 1u;
            const double p = ok ? (double)S / (dM * (double)nv) : nan;
            if (crow[i] >= 0) {
              if (a.nep) a.nep[((size_t)ri * a.nt + j) * a.rows + lead * a.ncol + crow[i]] = p;
              if (score && cw[i] > 0.0) {
                if (ok) {
                  const double w = cw[i];
                  const double o = (double)So / (double)nv;
                  const double e = p - o;
                  ++n_sc;
                  acc[0] += w;
                  acc[1] += w * (e * e);
                  acc[2] += w * (p * p);
                  acc[3] += w * (o * o);
                  acc[4] += w * p;
                  acc[5] += w * o;
                } else if (cflag[i] & 2u) {
                  ++n_bad;
                }
              }
            }
          }
          if (score) {  // (uniform) the tile's partial: a butterfly over the lanes, then the four waves in order
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
              for (int q = 0; q < kNbrSums; ++q) acc[q] += __shfl_xor(acc[q], off, 64);
              n_sc += __shfl_xor(n_sc, off, 64);
              n_bad += __shfl_xor(n_bad, off, 64);
            }
            __syncthreads();
            if (lane == 0) {
#pragma unroll
              for (int q = 0; q < kNbrSums; ++q) red_s[wv][q] = acc[q];
              redc_s[wv][0] = n_sc;
              redc_s[wv][1] = n_bad;
            }
            __syncthreads();
            const size_t slot = ((size_t)(a.tile0 + tl) * a.nr + ri) * a.nt + j;
            if (tid < kNbrSums) {
              double s = 0.0;
              for (int w = 0; w < kNbrThreads / 64; ++w) s += red_s[w][tid];
              a.part[slot * kNbrSums + tid] = s;
            } else if (tid < kNbrSums + 2) {
              long long s = 0;
              for (int w = 0; w < kNbrThreads / 64; ++w) s += redc_s[w][tid - kNbrSums];
              a.cnt[slot * 2 + (tid - kNbrSums)] = s;
            }
          }
        }
      }

      // ---- the union of the member masks, one 32-bit half of a mask word at a time -------------------------------------------
      if (a.nmep) {
        int un[kNbrMaxRad][kNbrCells];
#pragma unroll
        for (int ri = 0; ri < kNbrMaxRad; ++ri)
#pragma unroll
          for (int i = 0; i < kNbrCells; ++i) un[ri][i] = 0;
#pragma unroll 1
        for (int hh = 0; hh < nh; ++hh) {
          const unsigned int* m32 = reinterpret_cast<const unsigned int*>(a.mask + ((size_t)j * a.nw + (hh >> 1)) * a.R) + (hh & 1);
          __syncthreads();
#pragma unroll 1
          for (int sy = wv; sy < SH; sy += kNbrThreads / 64) {
            const int gy = y0 - hy + sy;
            const bool yin = gy >= 0 && gy < a.ny;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
              const int c = lane + 64 * i;
              int sx = x0 - hx + c;
              bool in = yin && c < SW;
              if (a.wrap) {
                sx %= a.nx;
                sx += sx < 0 ? a.nx : 0;
              } else {
                in = in && sx >= 0 && sx < a.nx;
              }
              unsigned int v = 0u;
              if (in) v = m32[2 * ((size_t)sb * a.ncol + (size_t)gy * a.nx + sx)];
              if (c < SW) P[sy * LW + c] = v;
            }
          }
          unsigned int orv[kNbrMaxRad][kNbrCells];
#pragma unroll
          for (int ri = 0; ri < kNbrMaxRad; ++ri)
#pragma unroll
            for (int i = 0; i < kNbrCells; ++i) orv[ri][i] = 0u;
#pragma unroll 1
          for (int L = 0; L <= a.lmax; ++L) {
            if (L > 0) {  // level L from level L - 1, in place, every row by the wave that staged it
              const int s = 1 << (L - 1);
#pragma unroll 1
              for (int sy = wv; sy < SH; sy += kNbrThreads / 64) {
                unsigned int v[CPL];
                nbr_wave_sync();
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                  const int c = lane + 64 * i;
                  v[i] = 0u;
                  if (c < SW) v[i] = P[sy * LW + c] | (c + s < SW ? P[sy * LW + c + s] : 0u);
                }
                nbr_wave_sync();
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                  const int c = lane + 64 * i;
                  if (c < SW) P[sy * LW + c] = v[i];
                }
              }
            }
            __syncthreads();
            const int back = (1 << L) - 1;
#pragma unroll
            for (int ri = 0; ri < kNbrMaxRad; ++ri) {
              if (ri < a.nr) {
                const int ry = a.ry[ri];
#pragma unroll 1
                for (int dy = -ry; dy <= ry; ++dy) {
                  const int h = a.hw[ri][dy < 0 ? -dy : dy];
                  if (31 - __builtin_clz(2 * h + 1) != L) continue;  // (uniform)
#pragma unroll
                  for (int i = 0; i < kNbrCells; ++i) {
                    const int row0 = (wv + 4 * i + hy + dy) * LW + cx;
                    orv[ri][i] |= P[row0 - h] | P[row0 + h - back];
                  }
                }
              }
            }
            __syncthreads();
          }
#pragma unroll
          for (int ri = 0; ri < kNbrMaxRad; ++ri)
#pragma unroll
            for (int i = 0; i < kNbrCells; ++i) un[ri][i] += __popc(orv[ri][i]);
        }
#pragma unroll
        for (int ri = 0; ri < kNbrMaxRad; ++ri)
#pragma unroll
          for (int i = 0; i < kNbrCells; ++i)
            if (ri < a.nr && crow[i] >= 0)
              a.nmep[((size_t)ri * a.nt + j) * a.rows + lead * a.ncol + crow[i]] = ((cvalid >> i) & 1u) ? (double)un[ri][i] / dM : nan;
      }
    }
  }
}

// the rows of the slabs that are not read: NaN in every field
__global__ __launch_bounds__(kNbrThreads) void k_nbr_unread(long rows, long ncol, int nrt, const int* __restrict__ active,
                                                          double* __restrict__ nep, double* __restrict__ nmep) {
  const double nan = __builtin_nan("");
  for (long i = (long)blockIdx.x * kNbrThreads + threadIdx.x; i < rows; i += (long)gridDim.x * kNbrThreads) {
    if (active[i / ncol]) continue;
    for (int f = 0; f < nrt; ++f) {
      if (nep) nep[(size_t)f * rows + i] = nan;
      if (nmep) nmep[(size_t)f * rows + i] = nan;
    }
  }
}

template <bool MASK>
hipError_t launch_records_m(const NbrRecArgs& a, Elem elem, long grid, hipStream_t s) {
  return efa_host::launch_quad(a.M, elem, [&](auto nu_c, auto e) {
    hipLaunchKernelGGL((k_nbr_records<decltype(nu_c)::value, decltype(e), MASK>), dim3((unsigned)grid), dim3(kNbrThreads), 0, s, a);
    return hipGetLastError();
  });
}

hipError_t launch_records(const NbrRecArgs& a, Elem elem, long blocks, hipStream_t s) {
  if (a.M < 2 || a.M > kMaxMembers) return hipErrorInvalidValue;
  if (a.ntiles <= 0) return hipSuccess;
  long grid = (a.ntiles + kNbrThreads / 64 - 1) / (kNbrThreads / 64);
  if (grid > blocks) grid = blocks;
  return a.mask ? launch_records_m<true>(a, elem, grid, s) : launch_records_m<false>(a, elem, grid, s);
}

hipError_t launch_windows(const NbrWinArgs& a, long blocks, hipStream_t s) {
  if (a.ntiles <= 0) return hipSuccess;
  const long grid = a.ntiles < blocks ? a.ntiles : blocks;
  const int halo = a.hy > a.hx ? a.hy : a.hx;
  if (halo > kNbrMaxR) return hipErrorInvalidValue;
  if (halo <= 8) hipLaunchKernelGGL(k_nbr_windows<8>, dim3((unsigned)grid), dim3(kNbrThreads), 0, s, a);
  else if (halo <= 32) hipLaunchKernelGGL(k_nbr_windows<32>, dim3((unsigned)grid), dim3(kNbrThreads), 0, s, a);
  else hipLaunchKernelGGL(k_nbr_windows<kNbrMaxR>, dim3((unsigned)grid), dim3(kNbrThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace
}  // namespace efa

// ---- the host side of efa_neighbourhood_dev / efa_neighbourhood_f32_dev --------------------------------------------------------
namespace efa_host {

using namespace efa;

// Like efa_products_dev the call works in a buffer of its own (nbr_ws) and neither reads nor writes what a later cycle reads.
// Nothing is written to the caller's arrays before every check has passed.
int neighbourhood(efa_ctx* c, Elem elem, long rows, int M, const void* X_dev, long ny, long nx, long n_lead, int nt, const double* thr,
                  int nr, const int* radius, int shape, int wrap_x, double* nep_dev, double* nmep_dev, const double* verif_dev,
                  const int* slab_group, const double* col_weight_dev, double* sums, long long* n, long long* n_bad) {
  const char* me = elem == Elem::f32 ? "efa_neighbourhood_f32_dev" : "efa_neighbourhood_dev";
  if (!X_dev || !thr || !radius) return fail(EFA_ERR_INVALID, "%s: null X_dev, thr or radius", me);
  if (M < 2 || M > kMaxMembers) return fail(EFA_ERR_INVALID, "%s: M=%d must be in [2,%d]", me, M, kMaxMembers);
  if (rows < 0 || ny < 0 || nx < 0 || n_lead < 0) return fail(EFA_ERR_INVALID, "%s: negative size", me);
  if (ny > (1L << 30) || nx > (1L << 30) || n_lead * ny * nx != rows)
    return fail(EFA_ERR_INVALID, "%s: rows=%ld must equal n_lead*ny*nx = %ld*%ld*%ld", me, rows, n_lead, ny, nx);
  if (nt < 1 || nt > kNbrMaxThr) return fail(EFA_ERR_INVALID, "%s: nt=%d must be in [1,%d]", me, nt, kNbrMaxThr);
  if (nr < 1 || nr > kNbrMaxRad) return fail(EFA_ERR_INVALID, "%s: nr=%d must be in [1,%d]", me, nr, kNbrMaxRad);
  for (int i = 0; i < nr; ++i)
    if (radius[i] < 0 || radius[i] > kNbrMaxR)
      return fail(EFA_ERR_INVALID, "%s: radius[%d] = %d must be in [0,%d]", me, i, radius[i], kNbrMaxR);
  if (shape != 0 && shape != 1) return fail(EFA_ERR_INVALID, "%s: shape=%d must be 0 (square) or 1 (disc)", me, shape);
  if (wrap_x != 0 && wrap_x != 1) return fail(EFA_ERR_INVALID, "%s: wrap_x=%d must be 0 or 1", me, wrap_x);
  if (wrap_x)
    for (int i = 0; i < nr; ++i)
      if (2L * radius[i] + 1 > nx)
        return fail(EFA_ERR_INVALID, "%s: wrap_x needs 2*radius+1 <= nx, radius[%d] = %d and nx = %ld", me, i, radius[i], nx);
  for (long i = 0; i < n_lead * (long)nt; ++i)
    if (std::isinf(thr[i])) return fail(EFA_ERR_INVALID, "%s: thr[%ld][%ld] is infinite (NaN means no threshold)", me, i / nt, i % nt);
  if (!sums != !n || !sums != !n_bad) return fail(EFA_ERR_INVALID, "%s: sums, n and n_bad go together (all null: no scores)", me);
  const bool score = verif_dev && sums;
  if (!nep_dev && !nmep_dev && !score) return fail(EFA_ERR_INVALID, "%s: no output wanted (nep_dev, nmep_dev, and sums with verif_dev)", me);
  if (verif_dev && !slab_group) return fail(EFA_ERR_INVALID, "%s: verif_dev needs slab_group", me);
  int G = 0;
  if (verif_dev) EFA_TRY(check_slab_groups(me, slab_group, n_lead, &G));
  if (!score) G = 0;

  c->neighbourhood_us = 0;
  const int nrt = nr * nt;
  const size_t ngf = (size_t)G * nrt;
  std::vector<double> h_sums(ngf * kNbrSums, 0.0);
  std::vector<long long> h_cnt(2 * ngf, 0);
  if (rows > 0) {
    hipStream_t s = c->stream;
    const long ncol = ny * nx;
    const bool fields = nep_dev || nmep_dev;
    // the slabs that are read: a finite threshold, and a field or a group that wants them
    std::vector<int> h_sg((size_t)n_lead, -1), h_act((size_t)n_lead, 0), h_slabs;
    const std::vector<double> h_thr = pad_thresholds(thr, n_lead, nt, kNbrMaxThr);
    for (long l = 0; l < n_lead; ++l) {
      bool any = false;
      for (int j = 0; j < nt; ++j) any = any || std::isfinite(thr[(size_t)l * nt + j]);
      if (score) h_sg[l] = slab_group[l];
      if (any && (fields || h_sg[l] >= 0)) {
        h_act[l] = 1;
        h_slabs.push_back((int)l);
      }
    }
    const long nact = (long)h_slabs.size();
    const int tyn = (int)((ny + kNbrTY - 1) / kNbrTY), txn = (int)((nx + kNbrTX - 1) / kNbrTX);
    const long tps = (long)tyn * txn;
    const long tiles_all = nact * tps;
    const int nw = (M + 63) / 64;
    // the records of a batch of slabs fit the cap; a batch holds at least one slab
    const size_t per_row = 2 + 2 * (size_t)nt + (nmep_dev ? 8 * (size_t)nt * nw : 0);
    size_t cap = (size_t)EFA_NBR_WS_BYTES;
    if (c->nbr_ws_bytes > 0 && (size_t)c->nbr_ws_bytes < cap) cap = (size_t)c->nbr_ws_bytes;
    long per_batch = (long)(cap / (per_row * (size_t)ncol));
    if (per_batch < 1) per_batch = 1;
    if (per_batch > nact) per_batch = nact > 0 ? nact : 1;
    const size_t Rmax = (size_t)per_batch * ncol;
    // nbr_ws: mask [nt][nw][Rmax] | part [tiles][nrt][6] | cnt [tiles][nrt][2] | sums [G][nrt][6] | n, n_bad [G][nrt] |
    //         thr [n_lead][8] | slab groups, active flags [n_lead], active slabs [nact] | k16 [nt][Rmax] | flag [Rmax]
    const size_t n_part = score ? (size_t)tiles_all * nrt * kNbrSums : 0, n_cnt = score ? (size_t)tiles_all * nrt * 2 : 0;
    const size_t n_sums = ngf * kNbrSums;
    WsLayout ws;
    const auto r_mask = ws.add<unsigned long long>(nmep_dev ? (size_t)nt * nw * Rmax : 0);
    const auto r_part = ws.add<double>(n_part);
    const auto r_cnt = ws.add<long long>(n_cnt);  // (straight behind part: one memset clears both)
    const auto r_sums = ws.add<double>(n_sums);
    const auto r_n = ws.add<long long>(ngf), r_nbad = ws.add<long long>(ngf);  // (n | n_bad come back in one copy)
    const auto r_thr = ws.add<double>(h_thr.size());
    const auto r_sg = ws.add<int>((size_t)n_lead), r_act = ws.add<int>((size_t)n_lead), r_slabs = ws.add<int>((size_t)nact);
    ws.align_to(8);  // (the 16-bit records start on 8-byte boundaries)
    const auto r_k16 = ws.add<unsigned short>((size_t)nt * Rmax);
    ws.align_to(8);
    const auto r_flag = ws.add<unsigned short>(Rmax);
    EFA_TRY(c->nbr_ws.reserve(ws.bytes()));
    unsigned long long* d_mask = r_mask(c->nbr_ws);
    double *d_part = r_part(c->nbr_ws), *d_sums = r_sums(c->nbr_ws), *d_thr = r_thr(c->nbr_ws);
    long long *d_cnt = r_cnt(c->nbr_ws), *d_n = r_n(c->nbr_ws), *d_nbad = r_nbad(c->nbr_ws);
    int *d_sg = r_sg(c->nbr_ws), *d_act = r_act(c->nbr_ws), *d_slabs = r_slabs(c->nbr_ws);
    unsigned short *d_k16 = r_k16(c->nbr_ws), *d_flag = r_flag(c->nbr_ws);
    EFA_HIP(hipMemcpyAsync(d_thr, h_thr.data(), h_thr.size() * sizeof(double), hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemcpyAsync(d_sg, h_sg.data(), (size_t)n_lead * sizeof(int), hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemcpyAsync(d_act, h_act.data(), (size_t)n_lead * sizeof(int), hipMemcpyHostToDevice, s));
    if (nact > 0) EFA_HIP(hipMemcpyAsync(d_slabs, h_slabs.data(), (size_t)nact * sizeof(int), hipMemcpyHostToDevice, s));
    if (n_part) EFA_HIP(hipMemsetAsync(d_part, 0, (n_part + n_cnt) * 8, s));

    NbrRecArgs ra{};
    ra.X = X_dev;
    ra.verif = verif_dev;
    ra.thr = d_thr;
    ra.ncol = ncol;
    ra.tps = (ncol + 15) / 16;
    ra.M = M;
    ra.al = pairs_aligned(X_dev, M, elem);
    ra.nt = nt;
    ra.nw = nw;
    ra.flag = d_flag;
    ra.k16 = d_k16;
    ra.mask = nmep_dev ? d_mask : nullptr;
    NbrWinArgs wa{};
    wa.flag = d_flag;
    wa.k16 = d_k16;
    wa.mask = ra.mask;
    wa.thr = d_thr;
    wa.sgroup = score ? d_sg : nullptr;
    wa.colw = col_weight_dev;
    wa.ncol = ncol;
    wa.rows = rows;
    wa.ny = (int)ny;
    wa.nx = (int)nx;
    wa.tyn = tyn;
    wa.txn = txn;
    wa.M = M;
    wa.nt = nt;
    wa.nw = nw;
    wa.nr = nr;
    wa.wrap = wrap_x;
    int rmax = 0;
    for (int i = 0; i < nr; ++i) rmax = radius[i] > rmax ? radius[i] : rmax;
    // beyond the grid a window holds nothing: the halo, the dy and the half-widths are cut to it
    wa.hy = (int)(rmax < ny - 1 ? rmax : ny - 1);
    wa.hx = wrap_x ? rmax : (int)(rmax < nx - 1 ? rmax : nx - 1);
    wa.lmax = 0;
    for (int i = 0; i < nr; ++i) {
      const int r = radius[i];
      wa.ry[i] = r < wa.hy ? r : wa.hy;
      for (int dy = 0; dy <= kNbrMaxR; ++dy) {
        int h = 0;
        if (dy <= r) {
          h = r;
          if (shape == 1)
            while (h * h + dy * dy > r * r) --h;
        }
        if (h > wa.hx) h = wa.hx;
        wa.hw[i][dy] = (unsigned char)h;
        if (dy <= wa.ry[i]) {
          int L = 0;
          while ((2 << L) <= 2 * h + 1) ++L;
          if (L > wa.lmax) wa.lmax = L;
        }
      }
    }
    wa.nep = nep_dev;
    wa.nmep = nmep_dev;
    wa.part = d_part;
    wa.cnt = d_cnt;
    const long blocks = clamp_blocks(c->neighbourhood_blocks, kNbrBlocks);

    EFA_TRY(interval_begin(c->nbr_iv, s));
    if (fields && nact < n_lead) {
      long grid = (rows + kNbrThreads - 1) / kNbrThreads;
      if (grid > blocks) grid = blocks;
      hipLaunchKernelGGL(k_nbr_unread, dim3((unsigned)grid), dim3(kNbrThreads), 0, s, rows, ncol, nrt, d_act, nep_dev, nmep_dev);
      EFA_HIP(hipGetLastError());
    }
    for (long s0 = 0; s0 < nact; s0 += per_batch) {
      const long nb = s0 + per_batch < nact ? per_batch : nact - s0;
      ra.slabs = wa.slabs = d_slabs + s0;
      ra.R = wa.R = nb * ncol;
      ra.ntiles = nb * ra.tps;
      wa.tile0 = s0 * tps;
      wa.ntiles = nb * tps;
      EFA_HIP(launch_records(ra, elem, blocks, s));
      EFA_HIP(launch_windows(wa, blocks, s));
    }
    if (G > 0) {
      EFA_HIP((launch_group_reduce<kNbrSums, 2>(G, nrt, s, tiles_all, tps, nrt, d_slabs, d_sg, d_part, d_cnt, d_sums, d_n,
                                                d_nbad)));
    }
    EFA_TRY(interval_end(c->nbr_iv, s));
    if (G > 0) {
      EFA_HIP(hipMemcpyAsync(h_sums.data(), d_sums, n_sums * sizeof(double), hipMemcpyDeviceToHost, s));
      EFA_HIP(hipMemcpyAsync(h_cnt.data(), d_n, 2 * ngf * sizeof(long long), hipMemcpyDeviceToHost, s));
    }
    EFA_HIP(hipStreamSynchronize(s));
    EFA_TRY(interval_us(c->nbr_iv, &c->neighbourhood_us));
  }
  if (G > 0) {
    for (size_t i = 0; i < h_sums.size(); ++i) sums[i] = h_sums[i];
    for (size_t i = 0; i < ngf; ++i) {
      n[i] = h_cnt[i];
      n_bad[i] = h_cnt[ngf + i];
    }
  }
  return EFA_OK;
}

}  // namespace efa_host
