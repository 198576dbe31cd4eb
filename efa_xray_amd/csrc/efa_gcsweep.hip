// Localised (Gaspari-Cohn) state sweep in ONE pass over the state: every row is loaded once,
// all observations whose taper is non-zero for it are applied in order, and it is stored once.
//
// Reference semantics (ensrf.py:99-115): kcov is multiplied by a taper that depends only on the
// (y, x) column (distance_to_point + gaspari_cohn, broadcast over variable x time), and is
// exactly 0 beyond 2 x halfwidth, where the update leaves the row bit-unchanged.  So
//   1. k_gc_build evaluates haversine + Gaspari-Cohn ONCE per (column, observation) -- not per
//      state row -- and keeps, per block of 16 columns, the ascending list of observations with
//      any non-zero weight together with the 16 weights (off / cnt / idx / wts).  One pass over the
//      trigonometry: a latitude-only upper bound per block (k_gc_bound) and a device prefix sum
//      (k_gc_scan) place the lists; k_gc_order sorts the blocks longest list first;
//   2. k_sweep_gc gives each workgroup one column block; its 4 waves (4 columns each) walk the n_lead
//      variable x time slabs of those columns (quad per row), and for each group of slabs loop over the
//      block's active list only, staged through LDS 32 observations at a time.
// Work drops from P passes' worth to (active fraction) x P; HBM traffic to one read + one write.
#include "efa_device.h"
#include "efa_internal.h"
#include "efa_lane_dot.h"
#include "efa_rows.h"

#include <cstdlib>
#include <utility>

namespace efa {
namespace {

constexpr int kBlkCols = 16;  // columns per block == rows per wave in the quad layout

// One WAVE per column block: lane l = (column c = l & 15, observation slot o = l >> 4), four
// observations per step in ascending order.  Everything the list needs is wave-local (ballot +
// a running count in a scalar register), so the loop has no workgroup barrier; the exact
// latitude rejection keeps the trigonometry to the few observations near the block.
//
// The lists are built in ONE pass over the trigonometry: k_gc_bound counts, per block, the observations
// that survive the latitude test alone (an upper bound of the list length, no trigonometry), k_gc_scan
// turns the bounds into offsets on the device, and k_gc_build writes each block's entries at its offset
// and records the true length in cnt[b] (the space between a block's end and the next offset stays unused).
constexpr int kBuildWaves = 4;  // column blocks per workgroup

// the block's latitude range, the same in every lane
__device__ __forceinline__ void block_lat_range(bool col_ok, double la, double& la_lo, double& la_hi) {
  la_lo = col_ok ? la : 1e300;
  la_hi = col_ok ? la : -1e300;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    la_lo = fmin(la_lo, __shfl_xor(la_lo, m, 64));
    la_hi = fmax(la_hi, __shfl_xor(la_hi, m, 64));
  }
}

// 64 observations at once, lane <-> observation: the great-circle distance to ANY column of the
// block is at least R * (latitude gap to the block's range); beyond 2 x halfwidth the
// Gaspari-Cohn weight is exactly 0, so most observations never reach the trigonometry
__device__ __forceinline__ unsigned long long lat_candidates(long k, long P, double la_lo, double la_hi,
                                                             const double* __restrict__ ob_lat,
                                                             const double* __restrict__ ob_hw,
                                                             const double* __restrict__ coef) {
  bool cnd = false;
  if (k < P && coef[k * kCoefStride + 3] != 0.0) {
    const double hw = ob_hw[k], olat = ob_lat[k];
    const double gap = fmax(0.0, fmax(olat - la_hi, la_lo - olat));
    cnd = (kEarthRadiusKm * radians(gap) <= 2.0 * fabs(hw) * (1.0 + 1e-9)) || !(hw == hw);
  }
  return __ballot(cnd);
}

__global__ __launch_bounds__(64 * kBuildWaves) void k_gc_bound(long ncol, long nblk, long P,
                                                               const double* __restrict__ glat,
                                                               const double* __restrict__ ob_lat,
                                                               const double* __restrict__ ob_hw,
                                                               const double* __restrict__ coef, int* __restrict__ ub) {
  const int lane = threadIdx.x & 63;
  const long b = (long)blockIdx.x * kBuildWaves + (threadIdx.x >> 6);
  if (b >= nblk) return;
  const long col = b * kBlkCols + (lane & 15);
  const bool col_ok = col < ncol;
  double la_lo, la_hi;
  block_lat_range(col_ok, col_ok ? glat[col] : 0.0, la_lo, la_hi);
  int n = 0;
  for (long k0 = 0; k0 < P; k0 += 64) n += __builtin_popcountll(lat_candidates(k0 + lane, P, la_lo, la_hi, ob_lat, ob_hw, coef));
  if (lane == 0) ub[b] = n;
}

// off[b] = sum of ub[0..b), off[nblk] = total; one workgroup (nblk is ncol / 16: tens of thousands)
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_gc_scan(long nblk, const int* __restrict__ ub, long* __restrict__ off) {
  __shared__ long part[kScanThreads];
  const int t = threadIdx.x;
  const long per = (nblk + kScanThreads - 1) / kScanThreads;
  const long lo = (long)t * per, hi = (lo + per < nblk) ? lo + per : nblk;
  long sum = 0;
  for (long b = lo; b < hi; ++b) sum += ub[b];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {  // inclusive Hillis-Steele over the per-thread sums
    const long v = (t >= d) ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  long run = part[t] - sum;
  for (long b = lo; b < hi; ++b) {
    off[b] = run;
    run += ub[b];
  }
  if (t == kScanThreads - 1) off[nblk] = part[t];
}

// Per observation: cos/sin of latitude and longitude and s_lim = sin^2(|halfwidth| / R), the haversine argument at
// which the taper reaches exactly 0 (distance = 2 halfwidths).  With them the haversine argument of a (column, ob)
// pair costs ten multiply-adds and no trigonometry: k_gc_build uses that cheap value ONLY to reject pairs that are
// clearly beyond the cut-off (relative margin 1e-6); every pair it keeps is evaluated with the reference's formula.
constexpr int kObTrig = 6;  // doubles per ob: cos lat, sin lat, cos lon, sin lon, s_lim, (pad)
__global__ void k_gc_obtrig(long P, const double* __restrict__ ob_lat, const double* __restrict__ ob_lon,
                            const double* __restrict__ ob_hw, double* __restrict__ tab) {
  const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= P) return;
  const double plat = radians(ob_lat[k]), plon = radians(ob_lon[k]);
  const double ang = fabs(ob_hw[k]) / kEarthRadiusKm;  // half the cut-off angle
  double slim = sin(ang);
  slim = slim * slim;
  if (!(ang < 1.5)) slim = 4.0;  // cut-off beyond a quarter of the globe (or a NaN radius): nothing is rejected cheaply
  double* t = tab + k * kObTrig;
  t[0] = cos(plat);
  t[1] = sin(plat);
  t[2] = cos(plon);
  t[3] = sin(plon);
  t[4] = slim;
  t[5] = 0.0;
}

// order[i] = the block with the i-th longest list (counting sort on cnt >> shift, one workgroup): the sweep
// hands out blocks longest first, so the last workgroups to start are the cheapest ones.  On a regular
// lat/lon grid the lists near the poles are several times longer than near the equator, and in blockIdx
// order the polar rows are both the first and the LAST blocks: the tail of the launch then runs on a few CUs.
__global__ __launch_bounds__(kScanThreads) void k_gc_order(long nblk, const int* __restrict__ cnt, int shift,
                                                          int* __restrict__ order) {
  __shared__ int hist[kScanThreads];
  const int t = threadIdx.x;
  hist[t] = 0;
  __syncthreads();
  for (long b = t; b < nblk; b += kScanThreads) {
    int key = cnt[b] >> shift;
    key = kScanThreads - 1 - (key < kScanThreads ? key : kScanThreads - 1);
    atomicAdd(&hist[key], 1);
  }
  __syncthreads();
  const int mine = hist[t];
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const int v = (t >= d) ? hist[t - d] : 0;
    __syncthreads();
    hist[t] += v;
    __syncthreads();
  }
  const int excl = hist[t] - mine;
  __syncthreads();
  hist[t] = excl;
  __syncthreads();
  for (long b = t; b < nblk; b += kScanThreads) {
    int key = cnt[b] >> shift;
    key = kScanThreads - 1 - (key < kScanThreads ? key : kScanThreads - 1);
    order[atomicAdd(&hist[key], 1)] = (int)b;
  }
}

// COUNT_ONLY: the same pass without the lists -- cnt[b] and the pair total only (efa_gc_block_counts: the cost of a
// column block for the cost-balanced column split of distributed.py)
template <bool COUNT_ONLY>
__global__ __launch_bounds__(64 * kBuildWaves) void k_gc_build(long ncol, long nblk, long P,
                                                               const double* __restrict__ glat,
                                                               const double* __restrict__ glon,
                                                               const double* __restrict__ ob_lat,
                                                               const double* __restrict__ ob_lon,
                                                               const double* __restrict__ ob_hw,
                                                               const double* __restrict__ coef,
                                                               const double* __restrict__ obtrig, int* __restrict__ cnt,
                                                               const long* __restrict__ off, int* __restrict__ idx,
                                                               double* __restrict__ wts,
                                                               unsigned long long* __restrict__ npairs) {
  // Round 3: two steps per 64 observations.  (1) lane <-> observation: the latitude candidates run the trig-free rejection
  // against each of the block's columns (their cos / sin from LDS) and the survivors -- observations within reach of at least one
  // column -- go into a small per-wave queue in ascending order; (2) lane <-> (column, one of four queued observations): the
  // reference's formula, now with nearly every lane busy.  Before, (2) ran on the latitude candidates directly and a step of
  // four candidates paid for the trigonometry whenever any of its 64 pairs survived (about half of the steps, a few lanes each).
  __shared__ double coltrig[kBuildWaves][kBlkCols][4];
  __shared__ int queue[kBuildWaves][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long b = (long)blockIdx.x * kBuildWaves + wv;
  if (b >= nblk) return;  // (no workgroup barrier below)
  const int c = lane & 15, o = lane >> 4;
  const long col = b * kBlkCols + c;
  const bool col_ok = col < ncol;
  const int ncols_live = (int)((ncol - b * kBlkCols < kBlkCols) ? ncol - b * kBlkCols : kBlkCols);
  const double la = col_ok ? glat[col] : 0.0, lo = col_ok ? glon[col] : 0.0;
  const double cg = cos(radians(la)), sg = sin(radians(la)), cl = cos(radians(lo)), sl = sin(radians(lo));
  if (lane < kBlkCols) {
    coltrig[wv][lane][0] = cg;
    coltrig[wv][lane][1] = sg;
    coltrig[wv][lane][2] = cl;
    coltrig[wv][lane][3] = sl;
  }
  __builtin_amdgcn_wave_barrier();  // (one wave's LDS operations complete in order)
  double la_lo, la_hi;
  block_lat_range(col_ok, la, la_lo, la_hi);
  const long first = COUNT_ONLY ? 0 : off[b];
  long running = first;
  long pairs = 0;  // (column, observation) pairs with a non-zero taper: SURVEY.md 8d's bytes_touched
  int qh = 0, qn = 0;  // the queue's head and length (wave-uniform)
  auto drain = [&](bool all) {
    while (qn >= 4 || (all && qn > 0)) {  // four queued observations per step, ascending
      const int take = qn < 4 ? qn : 4;
      const long k = (o < take) ? queue[wv][(qh + o) & 127] : -1;
      qh += take;
      qn -= take;
      double w = 0.0;
      if (k >= 0 && col_ok) {
        const double* t = obtrig + k * kObTrig;
        const double2 tp = *reinterpret_cast<const double2*>(t), tl = *reinterpret_cast<const double2*>(t + 2);
        const double cc = tp.x * cg;
        const double h = 0.5 * (1.0 - (cc + tp.y * sg)) + cc * (0.5 * (1.0 - (tl.x * cl + tl.y * sl)));  // sin^2(d / 2R), cheaply
        if (!(h > t[4] * (1.0 + 1e-6) + 1e-13)) {  // not clearly beyond 2 halfwidths: the reference's own arithmetic decides
          const double hw = ob_hw[k], olat = ob_lat[k];
          w = gaspari_cohn(distance_to_point_km(la, lo, olat, ob_lon[k]), hw);
        }
      }
      const unsigned long long bal = __ballot(w != 0.0);
      if (bal == 0ull) continue;  // wave-uniform
      pairs += __builtin_popcountll(bal);
      int before = 0, total = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int f = ((bal >> (16 * i)) & 0xFFFFull) != 0ull ? 1 : 0;
        before += (i < o) ? f : 0;
        total += f;
      }
      if (!COUNT_ONLY && ((bal >> (16 * o)) & 0xFFFFull) != 0ull) {
        const long e = running + before;
        if (c == 0) idx[e] = (int)k;
        wts[e * kBlkCols + c] = w;
      }
      running += total;
    }
  };
  for (long k0 = 0; k0 < P; k0 += 64) {
    const unsigned long long cand = lat_candidates(k0 + lane, P, la_lo, la_hi, ob_lat, ob_hw, coef);
    if (cand == 0ull) continue;
    bool surv = false;
    if ((cand >> lane) & 1ull) {
      const double* t = obtrig + (k0 + lane) * kObTrig;
      const double2 tp = *reinterpret_cast<const double2*>(t), tl = *reinterpret_cast<const double2*>(t + 2);
      const double lim = t[4] * (1.0 + 1e-6) + 1e-13;
      for (int c2 = 0; c2 < ncols_live; ++c2) {
        const double cc = tp.x * coltrig[wv][c2][0];
        const double h = 0.5 * (1.0 - (cc + tp.y * coltrig[wv][c2][1])) + cc * (0.5 * (1.0 - (tl.x * coltrig[wv][c2][2] + tl.y * coltrig[wv][c2][3])));
        surv = surv || !(h > lim);
      }
    }
    const unsigned long long sm = __ballot(surv);
    if (sm == 0ull) continue;
    if (surv) queue[wv][(qh + qn + __builtin_popcountll(sm & ((1ull << lane) - 1ull))) & 127] = (int)(k0 + lane);
    qn += __builtin_popcountll(sm);
    __builtin_amdgcn_wave_barrier();
    drain(false);
  }
  drain(true);
  if (lane == 0) {
    cnt[b] = (int)(running - first);
    if (COUNT_ONLY && idx) idx[b] = (int)pairs;  // counting pass: the block's (column, observation) pairs
    if (npairs) atomicAdd(npairs, (unsigned long long)pairs);
  }
}

constexpr int kChunk = 32;  // active observations staged in LDS at a time

// k_sweep_gc (efa_gcsweep_kernels.h).  Workgroup = one column block.  Wave w owns columns 4w .. 4w+3 of the block; its 16 quads are 4 columns x 4
// variable x time slabs, RPL rows (slabs) per quad, so the four waves walk the same 4 RPL slabs of different
// columns in lock step.  The block's active observations are staged chunk by chunk into LDS ONCE per group
// of slabs (ye rows, tapers, coefficients), so the per-lane traffic of the inner loop is LDS only; a wave
// skips an observation whose taper is zero on all of ITS four columns (the list is per 16 columns, and a
// block spans up to 8 degrees of longitude: a sixth of the listed (column, ob) pairs have zero weight).
// Fetching ye per lane straight from L2 made the kernel vector-memory-issue bound (10 x 1 KB requests per
// wave and observation through one 64 B/clk path per CU).
// The kernel is bound by fp64 VALU issue (profiles/r02_cfg3_summary.txt: 57 % of its VALU instructions are the
// 4 M FMAs per (row, ob) the arithmetic needs, VALU busy 3/4 of the time); three waves per SIMD (<= 168 VGPRs)
// while two rows of up to 80 members fit that budget without spilling, two waves above (M <= 128 at one row per quad).
#ifndef EFA_GC_MINWAVES
#define EFA_GC_MINWAVES 3
#endif
#ifndef EFA_GC_RPL
#define EFA_GC_RPL 2
#endif
// Rows per quad (they share every ye row read from LDS and the staging of a chunk): 2 at three waves per SIMD up to 8 chunks;
// 4 at two waves for 9..10 chunks (65..80 members: configs[2], 64.0 -> 62.2 ms) and 3 at two waves for 11..13 chunks
// (81..104 members: configs[3], 151 -> 141 ms); the few registers that spill are row addresses and means, saved and
// reloaded once per group of slabs -- the loop over the observations stays spill-free (checked in the assembly).
#ifndef EFA_GC_RPL_MID
#define EFA_GC_RPL_MID 4
#endif
#ifndef EFA_GC_RPL_WIDE
#define EFA_GC_RPL_WIDE 3
#endif
#ifndef EFA_GC_RPL_XWIDE
#define EFA_GC_RPL_XWIDE 1  // at 14..16 chunks (105..128 members)
#endif
#ifndef EFA_GC_LANE
#define EFA_GC_LANE 1  // cycles of up to 104 members (an even number, aligned rows) run the row-per-lane kernel (k_sweep_gc_lane)
#endif
#ifndef EFA_GC_COLSPLIT
#define EFA_GC_COLSPLIT 1
#endif
// dot(x, ye) over the lane's slots with two FMA chains (the other row of the quad and the other waves
// of the SIMD fill the issue slots), then the quad total
template <int NC>
__device__ __forceinline__ double gc_dot(const double (&x)[2 * NC], const double (&y)[2 * NC]) {
  double s0 = x[0] * y[0], s1 = x[1] * y[1];
#pragma unroll
  for (int c = 1; c < NC; ++c) {
    s0 = __builtin_fma(x[2 * c], y[2 * c], s0);
    s1 = __builtin_fma(x[2 * c + 1], y[2 * c + 1], s1);
  }
  return group_sum<4>(s0 + s1);
}

// ---- adaptive inflation (Anderson 2009), fused into both sweep forms.  One state row's (lam, sd) is updated by
// one observation from what the sweep holds for the (row, ob) pair BEFORE the ob moves the row: w the taper on the row's column
// (0 for an ob not assimilated), dot = x'.y', ss = x'.x', and the ob's staged record o01 = {D^2, sigma_p^2}, o23 = {sigma_o^2,
// y'.y'}.  The formulas of §7c in forms that take fewer fp64 square roots and divides (each a multi-instruction sequence):
//   gamma = min(1, w |dot| rsqrt(ss y'.y')), tested for 0 before any of it;
//   g = (dtheta/theta)(D^2/theta^2 - 1) = sp2 gamma q (D^2 - theta^2) / (2 sqrt(lam) theta^4)   (theta itself is not needed);
//   lam_n = lam + 2 s^2 g / (1 + sqrt(1 + 4 s^2 g^2)), the root of DART's linear_bayes nearer lam, without cancellation;
//   l = E(lam_n + s) - E(lam_n) + log(theta(lam_n)/theta(lam_n + s))
//     = -(2 a0 + s) / (2 s) + D^2 (t1 - t0) / (2 t0 t1) + log(t0 / t1) / 2,   a0 = lam_n - lam, t = theta^2 at lam_n, lam_n + s.
__device__ __forceinline__ void anderson_update(double& lam, double& sd, double w, double dot, double ss, double2 o01, double2 o23,
                                                double lower, double upper, double sd_lower) {
  const double nn = ss * o23.y;
  const double wd = w * fabs(dot);
  if (!(wd > 0.0) || !(nn > 0.0) || !(sd > 0.0)) return;  // gamma = 0 (or no spread): nothing changes
  const double gamma = fmin(1.0, wd * rsqrt(nn));
  const double d2 = o01.x, sp2 = o01.y, so2 = o23.x;
  const double rl = sqrt(lam);
  const double q = 1.0 + gamma * (rl - 1.0);
  const double th2 = q * q * sp2 + so2;
  const double g = (sp2 * gamma * q * (d2 - th2)) / (2.0 * rl * (th2 * th2));
  const double s2 = sd * sd;
  double ln = lam + 2.0 * s2 * g / (1.0 + sqrt(1.0 + 4.0 * s2 * (g * g)));
  ln = fmin(fmax(ln, lower), upper);
  if (sd > sd_lower) {
    const double q0 = 1.0 + gamma * (sqrt(ln) - 1.0), q1 = 1.0 + gamma * (sqrt(ln + sd) - 1.0);
    const double t0 = q0 * q0 * sp2 + so2, t1 = q1 * q1 * sp2 + so2;  // theta^2 at lam_new and lam_new + sd
    const double ell = -(2.0 * (ln - lam) + sd) / (2.0 * sd) + d2 * (t1 - t0) / (2.0 * (t0 * t1)) + 0.5 * log(t0 / t1);
    if (ell < -0.010050335853501441) sd = fmin(fmax(sqrt(-s2 / (2.0 * ell)), sd_lower), sd);  // log(0.99)
  }
  lam = ln;
}
// x'.x' of the row after the ob: x' - kb y' (kb = the member gain), by the exact recursion
__device__ __forceinline__ double adapt_ss_after(double ss, double kb, double dot, double yy) {
  return fmax(ss - kb * (2.0 * dot - kb * yy), 0.0);
}

// waves per SIMD the register budget allows: RPL rows and one ye row of 2 NC doubles per lane, ~36 registers of everything else
constexpr int gc_min_waves(int NC, int RPL) {
  return (4 * NC * (RPL + 1) + 36 <= 168) ? EFA_GC_MINWAVES : (4 * NC * (RPL + 1) + 36 <= 256 || NC * (RPL + 1) <= 52) ? 2 : 1;
}


// ---------------------------------------------------------------------------------------------------------------
// Row-per-lane form of the same sweep (round 3).  A lane holds one WHOLE state row (up to 104 members in registers), so the
// dot x . ye is lane-local -- no quad butterflies -- and every fp64 instruction of the loop over the observations is a
// multiply-add: v_fmac_f64 with a DPP row_newbcast source, which takes one multiplicand from lane l of the lane's own
// 16-lane row.  Lane l of each row holds ye members l, 16 + l, 32 + l, ...: the whole ye vector sits in 5..7 registers
// per lane and is read from LDS with that many 8-byte reads per wave and observation (the quad form: 10..13 16-byte reads
// delivering the same row to each of 16 quads).  tools/dpp_fmac_probe.hip: the DPP form issues at the rate of the plain FMA.
// A wave is 4 columns x 16 slabs (the same four columns per wave as the quad form, so the same zero-taper skipping); the last,
// partial group of slabs of a column block is folded onto fewer waves (8 slabs: 8 columns per wave, two waves; 4 slabs: all
// 16 columns on one wave) instead of running with dead lanes.
// The DPP instructions are inline assembly (the compiler has no 64-bit DPP intrinsic).  Their DPP operand, ye, is written by
// LDS reads only, never by a VALU instruction, so the "VALU write -> DPP read" hazard (which the compiler does not track
// through inline assembly) cannot arise; tests/test_cpu_host.py checks the generated code for exactly that.
// fmac_bcast and lane_dot: efa_lane_dot.h (shared with the observation-impact contraction, efa_impact.hip).
// x[16 C + i] += (ye member 16 C + i) * nkb for the members of ye register C
template <int MP, int C, int... I>
__device__ __forceinline__ void lane_update_group(double (&x)[MP], double yc, double nkb, std::integer_sequence<int, I...>) {
  (fmac_bcast<I>(x[16 * C + I], yc, nkb), ...);
}
// The update walks the ye registers in order and re-loads each one with the NEXT active observation's members as soon as its
// sixteen multiply-adds are issued: the LDS latency of the next ye row hides behind the rest of this update and the head of
// the next dot, without a second set of ye registers (there are none to spare at 100 members).
template <int MP, int C = 0>
__device__ __forceinline__ void lane_update_prefetch(double (&x)[MP], double (&y)[(MP + 15) / 16], double nkb, const double* __restrict__ ynext) {
  constexpr int NG = (MP + 15) / 16;
  if constexpr (C < NG) {
    constexpr int n = (MP - 16 * C < 16) ? MP - 16 * C : 16;
    lane_update_group<MP, C>(x, y[C], nkb, std::make_integer_sequence<int, n>{});
    y[C] = ynext[16 * C];
    lane_update_prefetch<MP, C + 1>(x, y, nkb, ynext);
  }
}

// ADAPT: the same update without the prefetch -- the inflation update then runs while no ye register is live (at 100 members the
// row, the ye registers and the update's temporaries do not fit 256 registers together), and the next ye row is read after it
template <int MP, int C = 0>
__device__ __forceinline__ void lane_update(double (&x)[MP], const double (&y)[(MP + 15) / 16], double nkb) {
  constexpr int NG = (MP + 15) / 16;
  if constexpr (C < NG) {
    constexpr int n = (MP - 16 * C < 16) ? MP - 16 * C : 16;
    lane_update_group<MP, C>(x, y[C], nkb, std::make_integer_sequence<int, n>{});
    lane_update<MP, C + 1>(x, y, nkb);
  }
}

constexpr int kLaneMaxMembers = 104;
#ifndef EFA_GC_LANE_CHUNK
#define EFA_GC_LANE_CHUNK 32
#endif
constexpr int kChunkL = EFA_GC_LANE_CHUNK;  // observations staged at a time by the row-per-lane kernel (a 64-bit mask of them per wave)

// the kernel family of a launch: plain, adaptive inflation fused in, vertical factor (§7d), slab table (§7t; it
// carries the vertical factor too: it goes before the vertical family); the values are the option "gc_family"'s
// sampling error correction: the gain of the pair damped by the factor of its sample correlation
enum GcFamily : int { kGcPlain = 0, kGcAdapt = 1, kGcVloc = 2, kGcSlab = 3, kGcSec = 4 };
inline int gc_family(const GcSweepArgs& a) {
  return a.infl ? kGcAdapt : a.sec_tab ? kGcSec : a.slab_tab ? kGcSlab : a.lead_vert ? kGcVloc : kGcPlain;
}
// dispatch_family(fam, f) returns f(std::integral_constant<int, FAM>{}) for the FAM equal to fam
template <class F>
hipError_t dispatch_family(int fam, F&& f) {
  return dispatch_width(fam, std::integer_sequence<int, kGcPlain, kGcAdapt, kGcVloc, kGcSlab, kGcSec>{}, f);
}

// ---- sampling error correction (Anderson 2012), fused into both sweep forms.  The factor of one (row, ob) pair from
// what the sweep holds BEFORE the ob moves the row: dot = x'.y', ss = x'.x', yy = y'.y'.  |r| = |dot| rsqrt(ss yy), 0 when either
// norm is 0; the table (in LDS, node j at |r| = j / (T - 1)) is read piecewise linearly.  fmin returns its other argument for a
// NaN, so a poisoned row reads the last interval (its gain is NaN through dot all the same) and no index leaves [0, T - 2].
struct SecLookup {
  const double* tab;
  int T;
  __device__ __forceinline__ double operator()(double dot, double ss, double yy) const {
    const double nn = ss * yy;
    const double r = (nn > 0.0) ? fabs(dot) * rsqrt(nn) : 0.0;
    const double t = fmin(r, 1.0) * (double)(T - 1);
    int j = (int)t;
    j = (j < T - 2) ? j : T - 2;
    const double a0 = tab[j], a1 = tab[j + 1];
    return a0 + (t - (double)j) * (a1 - a0);
  }
};

// Waves per SIMD of the quad form.  With the update: one row per quad (gc_launch), and waves per SIMD for that row, one ye row and
// ~100 registers of everything else (the update's temporaries included); the vertical factor and the slab table take the launch
// shapes and rows per quad of the plain kernels (a few registers more per row for the factor)
constexpr int gc_adapt_min_waves(int NC) { return (4 * NC * 2 + 100 <= 168) ? 3 : (4 * NC * 2 + 100 <= 256) ? 2 : 1; }
// with the correction: x'.x' of every row and the lookup's temporaries (the reciprocal square root above all) on top of the plain
// kernel's budget -- measured 16 .. 26 registers; 40 more in the budget keep every instantiation clear of scratch (8 chunks of two
// rows, 168 + 2 spilled at three waves, go to two)
constexpr int gc_sec_min_waves(int NC, int RPL) {
  return (4 * NC * (RPL + 1) + 76 <= 168) ? EFA_GC_MINWAVES : (4 * NC * (RPL + 1) + 76 <= 256 || NC * (RPL + 1) <= 52) ? 2 : 1;
}
constexpr int gc_quad_waves(int FAM, int NC, int RPL) {
  return FAM == kGcAdapt ? gc_adapt_min_waves(NC) : FAM == kGcSec ? gc_sec_min_waves(NC, RPL) : gc_min_waves(NC, RPL);
}
// and of the row-per-lane form.  With the update, above 80 members at one wave per SIMD: the row, the ye registers and the
// update's temporaries spill at two; with the correction above 96 (the plain kernel's last spare registers at 100 and 104)
constexpr int gc_lane_waves(int FAM, int MP) { return ((FAM == kGcAdapt && MP > 80) || (FAM == kGcSec && MP > 96)) ? 1 : 2; }

#include "efa_gcsweep_kernels.h"

// The row-per-lane launch.  float32 rows exist in member form and without adaptive inflation only, which
// launch_sweep_gc has made sure of.
template <int FAM, typename E, int MP>
hipError_t gc_lane_launch(const GcSweepArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)(a.nblk * a.lead_split)), block(256);
  if constexpr (sizeof(E) != sizeof(double)) {
    if constexpr (FAM == kGcAdapt) return hipErrorInvalidValue;
    else hipLaunchKernelGGL((k_sweep_gc_lane<FAM, E, MP, true>), grid, block, 0, s, a);
  } else if (a.fused_members) {
    hipLaunchKernelGGL((k_sweep_gc_lane<FAM, E, MP, true>), grid, block, 0, s, a);
  } else {
    hipLaunchKernelGGL((k_sweep_gc_lane<FAM, E, MP, false>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus = n;
  }
  return cus;
}

template <int FAM, int NC>
hipError_t gc_launch(const GcSweepArgs& a0, hipStream_t s) {
  constexpr bool ADAPT = FAM == kGcAdapt;
  GcSweepArgs a = a0;
  const bool vec = (a.M % 2 == 0) && (a.ye_stride % 2 == 0) && aligned16(a.Xin) && aligned16(a.Xout) && aligned16(a.Ye);
  // rows per quad while they fit the register file; with the inflation update one (its per-row state and temporaries spill at more)
  // (with the correction one row fewer where the plain kernel holds more than two: its registers go to the lookup)
  constexpr int RPLP = ADAPT ? 1 : (NC <= 8) ? EFA_GC_RPL : (NC <= 10) ? EFA_GC_RPL_MID : (NC <= 13) ? EFA_GC_RPL_WIDE : (NC <= 16) ? EFA_GC_RPL_XWIDE : 1;
  constexpr int RPL = (FAM == kGcSec && RPLP > 2) ? RPLP - 1 : RPLP;
  // groups of slabs per column block: whole iterations of the slab loop (4 RPL slabs), as many as it takes to give
  // every CU a dozen workgroups, at most one group per iteration
  const int cus = device_cus();
  const long iters = (a.n_lead + 4 * RPL - 1) / (4 * RPL);
  long split = (12L * cus + a.nblk - 1) / a.nblk;
  if (split > iters) split = iters;
  if (split < 1) split = 1;
  a.lead_chunk = ((iters + split - 1) / split) * (4 * RPL);
  a.lead_split = (int)((a.n_lead + a.lead_chunk - 1) / a.lead_chunk);
  const dim3 grid((unsigned)(a.nblk * a.lead_split)), block(256);
  if (a.fused_members) {
    if (vec) hipLaunchKernelGGL((k_sweep_gc<FAM, NC, true, true, RPL>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_sweep_gc<FAM, NC, false, true, RPL>), grid, block, 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_sweep_gc<FAM, NC, true, false, RPL>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_sweep_gc<FAM, NC, false, false, RPL>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace

long gc_num_blocks(long ncol) { return (ncol + kBlkCols - 1) / kBlkCols; }

hipError_t launch_gc_bound(long ncol, long P, const double* glat, const double* ob_lat, const double* ob_hw,
                           const double* coef, int* ub, long* off, hipStream_t s) {
  const long nblk = gc_num_blocks(ncol);
  if (nblk <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gc_bound, dim3((unsigned)((nblk + kBuildWaves - 1) / kBuildWaves)), dim3(64 * kBuildWaves), 0, s, ncol,
                     nblk, P, glat, ob_lat, ob_hw, coef, ub);
  hipLaunchKernelGGL(k_gc_scan, dim3(1), dim3(kScanThreads), 0, s, nblk, ub, off);
  return hipGetLastError();
}

hipError_t launch_gc_fill(long ncol, long P, const double* glat, const double* glon, const double* ob_lat,
                          const double* ob_lon, const double* ob_hw, const double* coef, double* obtrig, const long* off,
                          int* cnt, int* idx, double* wts, int* order, unsigned long long* npairs, hipStream_t s) {
  const long nblk = gc_num_blocks(ncol);
  if (nblk <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gc_obtrig, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, ob_lat, ob_lon, ob_hw, obtrig);
  hipLaunchKernelGGL(k_gc_build<false>, dim3((unsigned)((nblk + kBuildWaves - 1) / kBuildWaves)), dim3(64 * kBuildWaves), 0, s,
                     ncol, nblk, P, glat, glon, ob_lat, ob_lon, ob_hw, coef, obtrig, cnt, off, idx, wts, npairs);
  int shift = 0;
  while ((P >> shift) >= kScanThreads) ++shift;
  hipLaunchKernelGGL(k_gc_order, dim3(1), dim3(kScanThreads), 0, s, nblk, cnt, shift, order);
  return hipGetLastError();
}

hipError_t launch_gc_count(long ncol, long P, const double* glat, const double* glon, const double* ob_lat,
                           const double* ob_lon, const double* ob_hw, const double* coef, double* obtrig, int* cnt,
                           int* blk_pairs, unsigned long long* npairs, hipStream_t s) {
  const long nblk = gc_num_blocks(ncol);
  if (nblk <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gc_obtrig, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, ob_lat, ob_lon, ob_hw, obtrig);
  hipLaunchKernelGGL(k_gc_build<true>, dim3((unsigned)((nblk + kBuildWaves - 1) / kBuildWaves)), dim3(64 * kBuildWaves), 0, s,
                     ncol, nblk, P, glat, glon, ob_lat, ob_lon, ob_hw, coef, obtrig, cnt, nullptr, blk_pairs, nullptr, npairs);
  return hipGetLastError();
}

// float64 rows serve every cycle; float32 rows the cycles of the row-per-lane kernel: what the float64 launch asks of
// a cycle before it takes that kernel, less the 16-byte alignment of the rows (float rows need 4)
bool sweep_gc_serves(Elem elem, int M, long ye_stride, const double* Ye) {
  if (M < 2 || M > kMaxMembers) return false;
  return elem == Elem::f64 || (EFA_GC_LANE && M <= kLaneMaxMembers && (M % 2 == 0) && (ye_stride % 2 == 0) && aligned16(Ye));
}

// 16-byte aligned float64 rows of up to 104 members (an even number of them), and the float32 rows: the row-per-lane kernel
int sweep_gc_form(const GcSweepArgs& a, Elem elem) {
  return (elem == Elem::f32 || (EFA_GC_LANE && a.M <= kLaneMaxMembers && (a.M % 2 == 0) && (a.ye_stride % 2 == 0) && aligned16(a.Xin) &&
                                aligned16(a.Xout) && aligned16(a.Ye)))
             ? 2
             : 1;
}

// The launcher is where a.Xin / a.Xout get their element type: elem picks the kernels that read them as float or as double rows.
hipError_t launch_sweep_gc(const GcSweepArgs& a, Elem elem, hipStream_t s) {
  const bool f32 = elem == Elem::f32;
  if (!sweep_gc_serves(elem, a.M, a.ye_stride, a.Ye)) return hipErrorInvalidValue;
  if (a.sec_tab && (a.sec_T < 2 || a.sec_T > kSecMaxT || !a.adapt_ob || a.infl || a.slab_tab || a.lead_vert)) return hipErrorInvalidValue;
  // float32 rows: member form, 4-byte aligned, no adaptive inflation (its update is float64 only)
  if (f32 && (!a.fused_members || a.infl || ((reinterpret_cast<uintptr_t>(a.Xin) | reinterpret_cast<uintptr_t>(a.Xout)) & 3u) != 0))
    return hipErrorInvalidValue;
  if (a.nblk <= 0 || a.n_lead <= 0) return hipSuccess;
  if (sweep_gc_form(a, elem) == 2) {
    GcSweepArgs l = a;
    l.lead_split = (int)((l.n_lead + 15) / 16);  // groups of 16 slabs: one workgroup each
    l.lead_chunk = 16;
    return dispatch_family(gc_family(a), [&](auto fam) {
      constexpr int FAM = fam;
      return dispatch_width((l.M + 3) / 4, WidthRange<1, kLaneMaxMembers / 4>{}, [&](auto q) {
        return f32 ? gc_lane_launch<FAM, float, 4 * q>(l, s) : gc_lane_launch<FAM, double, 4 * q>(l, s);
      });
    });
  }
  return dispatch_family(gc_family(a), [&](auto fam) {
    constexpr int FAM = fam;
    return dispatch_width(sweep_slots(a.M) / 8, SweepChunks{}, [&](auto nc) { return gc_launch<FAM, nc>(a, s); });
  });
}

}  // namespace efa
