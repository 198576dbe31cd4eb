// The two one-pass GC sweep kernels: k_sweep_gc (quad form) and k_sweep_gc_lane (row-per-lane form).  Included once by
// efa_gcsweep.hip, inside namespace efa::<anonymous>, after what the kernels use: GcFamily, the launch bounds gc_quad_waves and
// gc_lane_waves, kBlkCols, kChunk and kChunkL, EFA_GC_COLSPLIT, gc_dot, anderson_update, adapt_ss_after, lane_update and
// lane_update_prefetch (efa_gcsweep.hip), load_row, store_row, lds_read_row, group_rowsum and group_centered_sumsq (efa_rows.h),
// lane_dot (efa_lane_dot.h), vert_factor (efa_device.h) and GcSweepArgs (efa_internal.h).
// FAM is the kernel family (GcFamily): kGcAdapt fuses the adaptive-inflation update in (Anderson 2009); with
// kGcVloc and kGcSlab the taper carries a factor of each (slab, ob) pair: the vertical factor, evaluated while staging (DESIGN.md
// §7d), or with kGcSlab the entry of the slab table S[ob][slab], which holds the product of the vertical, temporal and variable
// factors.  kGcSec damps the gain of every (row, ob) pair by the sampling-error-correction factor alpha(|r|) of the
// pair's sample correlation (Anderson 2012): x'.x' of the row is kept as the adaptive family keeps it, y'.y' is the
// ob's staged record, the table sits in LDS.
// E is the element type of the state rows in memory as the row-per-lane kernel sees them: double, or float for a state stored as
// float32 (member form, no adaptive inflation; the quad kernel has no float32 form).
#ifndef EFA_GCSWEEP_KERNELS_H
#define EFA_GCSWEEP_KERNELS_H

template <int FAM, int NC, bool VEC, bool FUSED, int RPL>
__global__ __launch_bounds__(256, gc_quad_waves(FAM, NC, RPL)) void k_sweep_gc(const GcSweepArgs a) {
  constexpr bool ADAPT = FAM == kGcAdapt;
  constexpr bool VLOC = FAM == kGcVloc || FAM == kGcSlab;
  constexpr bool SLAB = FAM == kGcSlab;  // VLOC with the factor read from the slab table
  constexpr bool SEC = FAM == kGcSec;
  static_assert(!(ADAPT && VLOC), "adaptive inflation with vertical localisation is not built");
  static_assert(VLOC || !SLAB, "the slab table is a form of the per-slab factor");
  constexpr int L = 4;
  constexpr int S = 2 * L * NC;  // padded ye row (doubles)
  constexpr int NS = 4 * RPL;    // slabs of one iteration of the slab loop
  __shared__ __align__(16) double ye_s[kChunk * S];
  __shared__ __align__(16) double2 ab_s[kChunk * kBlkCols];  // per (staged ob, column): what scales (x . ye) in the row / in its mean
  __shared__ __align__(16) double aw_s[ADAPT ? kChunk * kBlkCols : 1];  // ADAPT: the taper per (staged ob, column), 0 if not assimilated
  __shared__ __align__(16) double2 ao_s[ADAPT ? 2 * kChunk : 1];         // ADAPT: the staged obs' records (adapt_ob)
  __shared__ __align__(16) double vf_s[VLOC ? kChunk * NS : 1];           // VLOC: the vertical factor per (staged ob, slab slot), 0 beyond the last slab
  __shared__ __align__(16) double sec_s[SEC ? kSecMaxT : 1];              // SEC: the table, staged once per workgroup
  __shared__ __align__(16) double yy_s[SEC ? kChunk : 1];                 // SEC: y'.y' of the staged obs
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int j = lane & 3, r = lane >> 2;
  // blockIdx.x = (position in the longest-first order) * lead_split + (group of slabs): a shard with few, long
  // column blocks (the polar ranks of a cost-balanced split) still fills the device and has no tail of whole blocks
  const long b = a.order[blockIdx.x / a.lead_split];
  const int lead_lo = (int)(blockIdx.x % a.lead_split) * (int)a.lead_chunk;
  const int lead_hi = (lead_lo + (int)a.lead_chunk < (int)a.n_lead) ? lead_lo + (int)a.lead_chunk : (int)a.n_lead;
  // quad r of wave w: column cq of the block, slab slot sq of the group of slabs
  const int cq = EFA_GC_COLSPLIT ? 4 * wave + (r & 3) : r;
  const int sq = EFA_GC_COLSPLIT ? (r >> 2) : wave;
  const long col = b * kBlkCols + cq;
  const bool col_ok = col < a.ncol;
  const int M = a.M;
  const double rM1 = 1.0 / (double)(M - 1);
  const long e0 = a.off[b], e1 = e0 + a.cnt[b];
  const SecLookup sec{sec_s, SEC ? a.sec_T : 2};
  if (SEC)  // (read behind the barriers of the first chunk's staging)
    for (int i = tid; i < a.sec_T; i += 256) sec_s[i] = a.sec_tab[i];

  // A quad holds RPL rows of the SAME column (slabs lead, lead + 4, ...): they share the taper and
  // every ye row read from LDS (the quad layout delivers each ye row once per quad), and a staged
  // chunk serves 4 RPL slabs instead of 4.
  for (int lead0 = lead_lo; lead0 < lead_hi; lead0 += 4 * RPL) {
    double x[RPL][2 * NC];
    double xm[RPL];
    double lam[RPL], sd[RPL], ss[RPL];  // ADAPT: the row's inflation and x'.x'; SEC: x'.x'
    bool live[RPL];
    bool touched[RPL];  // FUSED: some ob moved the row (a row no ob reaches goes out as it came in, see the store below)
    long row[RPL];
    bool any_live = false;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
      const int lead = lead0 + sq + 4 * q;
      live[q] = col_ok && lead < lead_hi;
      touched[q] = false;
      any_live = any_live || live[q];
      row[q] = (long)lead * a.ncol + col;
      xm[q] = 0.0;
      if (live[q]) {
        load_row<L, NC, VEC>(a.Xin + (size_t)row[q] * M, M, j, x[q]);
        if (!FUSED) xm[q] = a.xin[row[q]];
      } else {
#pragma unroll
        for (int c = 0; c < 2 * NC; ++c) x[q][c] = 0.0;
      }
      if (FUSED) {  // prior members in: remove the ensemble mean (assimilation.py:146-147)
        xm[q] = group_rowsum<L, NC>(x[q]) / (double)M;
        if (ADAPT || SEC) ss[q] = group_centered_sumsq<L, NC>(x[q], xm[q], M, j);
#pragma unroll
        for (int c = 0; c < 2 * NC; ++c) x[q][c] -= xm[q];  // padding slots never reach the output or the dot
      } else if (ADAPT || SEC) {
        ss[q] = group_centered_sumsq<L, NC>(x[q], 0.0, M, j);
      }
      if (ADAPT) {
        lam[q] = live[q] ? a.infl[2 * row[q]] : 1.0;
        sd[q] = live[q] ? a.infl[2 * row[q] + 1] : 0.0;
      }
    }
    for (long c0 = e0; c0 < e1; c0 += kChunk) {
      const int ne = (int)((e1 - c0 < kChunk) ? (e1 - c0) : kChunk);
      __syncthreads();  // previous chunk fully consumed
      // ---- cooperative staging of ne entries
      if (VEC) {
        constexpr int S2 = S / 2;
        const int M2 = M / 2;
        for (int i = tid; i < ne * S2; i += 256) {
          const int ee = i / S2, m2 = i - ee * S2;
          const int k = a.idx[c0 + ee];
          reinterpret_cast<double2*>(ye_s)[i] =
              (m2 < M2) ? reinterpret_cast<const double2*>(a.Ye + (size_t)k * a.ye_stride)[m2] : make_double2(0.0, 0.0);
        }
      } else {
        for (int i = tid; i < ne * S; i += 256) {
          const int ee = i / S, m = i - ee * S;
          const int k = a.idx[c0 + ee];
          ye_s[i] = (m < M) ? a.Ye[(size_t)k * a.ye_stride + m] : 0.0;
        }
      }
      // The gain scalars of ensrf.py:95-136 -- kcov = (x . ye)/(M-1), times the taper, /kdenom, times innov for the mean
      // and times beta for the members -- do not depend on the state row: they are folded ONCE per (ob, column) here,
      // A = w (1/(M-1)) (1/kdenom) beta and B = w (1/(M-1)) (1/kdenom) innov, instead of six dependent multiplications
      // per row and observation in a loop that is bound by the number of fp64 instructions it issues.
      for (int i = tid; i < ne * kBlkCols; i += 256) {
        const double w = a.wts[(size_t)c0 * kBlkCols + i];
        const double* ck = a.coef + (size_t)a.idx[c0 + i / kBlkCols] * kCoefStride;  // innov, 1/kdenom, beta, active
        const double g = (w * rM1) * ck[1];
        ab_s[i] = make_double2(g * ck[2], g * ck[0]);  // w == 0 (or an ob that is not assimilated): both exactly 0
        if (ADAPT) aw_s[i] = (ck[3] != 0.0) ? w : 0.0;
      }
      if (ADAPT)
        for (int i = tid; i < 2 * ne; i += 256) ao_s[i] = reinterpret_cast<const double2*>(a.adapt_ob + (size_t)a.idx[c0 + (i >> 1)] * 4)[i & 1];
      if (SEC)
        for (int i = tid; i < ne; i += 256) yy_s[i] = a.adapt_ob[(size_t)a.idx[c0 + i] * 4 + 3];
      if (VLOC)
        for (int i = tid; i < ne * NS; i += 256) {
          const int ee = i / NS, lead = lead0 + (i - ee * NS);
          const int k = a.idx[c0 + ee];
          if (SLAB) vf_s[i] = (lead < lead_hi) ? a.slab_tab[(size_t)k * a.n_lead + lead] : 0.0;  // NS consecutive doubles per staged ob
          else vf_s[i] = (lead < lead_hi) ? vert_factor(a.lead_vert[lead], a.ob_vert[k], a.ob_vhw[k]) : 0.0;
        }
      __syncthreads();
      // ---- apply the chunk to this wave's 16 RPL rows
      for (int ee = 0; ee < ne; ++ee) {
        const double2 ab = ab_s[ee * kBlkCols + cq];
        if (VLOC) {  // skipped unless the horizontal taper AND the vertical factor of one of the quad's slabs are non-zero somewhere
          bool vz = false;
#pragma unroll
          for (int q = 0; q < RPL; ++q) vz = vz || (vf_s[ee * NS + sq + 4 * q] != 0.0);
          if (!any_live || __ballot(ab.x != 0.0 && vz) == 0ull) continue;
        } else {
          if (!any_live || __ballot(ab.x != 0.0) == 0ull) continue;  // none of this wave's rows (dead slabs / zero taper)
        }
        double y[2 * NC];
        lds_read_row<L, NC>(ye_s + ee * S, j, y);
        double aw = 0.0;
        double2 o01, o23;
        if (ADAPT) {
          aw = aw_s[ee * kBlkCols + cq];
          o01 = ao_s[2 * ee];
          o23 = ao_s[2 * ee + 1];
        }
        double yy = 0.0;
        if (SEC) yy = yy_s[ee];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
          if (RPL > 2 && lead0 + 4 * q >= lead_hi) continue;  // wave-uniform: this slot is beyond the last slab in every quad
          const double dot = gc_dot<NC>(x[q], y);        // :95 (a dead row holds zeros: its dot, and so its update, is exactly 0)
          double2 abr = ab;
          if (VLOC) {  // the row's slab: both gain scalars times its vertical factor (1: unchanged bit for bit)
            const double v = vf_s[ee * NS + sq + 4 * q];
            abr.x = ab.x * v;
            abr.y = ab.y * v;
          }
          if (SEC) {  // both gain scalars times the factor of the pair's correlation, row and ob as they are before the ob (1: unchanged bit for bit)
            const double al = sec(dot, ss[q], yy);
            abr.x = ab.x * al;
            abr.y = ab.y * al;
          }
          xm[q] = __builtin_fma(abr.y, dot, xm[q]);      // :115, :119, :130
          const double kb = abr.x * dot;                 // :115, :119, :136
          if (FUSED) touched[q] = touched[q] || (abr.x != 0.0);
          if (ADAPT) {  // (each lane of the quad holds the quad's dot and x'.x': the four do the update alike)
            anderson_update(lam[q], sd[q], aw, dot, ss[q], o01, o23, a.infl_lower, a.infl_upper, a.infl_sd_lower);
            ss[q] = adapt_ss_after(ss[q], kb, dot, o23.y);
          }
          if (SEC) ss[q] = adapt_ss_after(ss[q], kb, dot, yy);
#pragma unroll
          for (int c = 0; c < 2 * NC; ++c) x[q][c] = __builtin_fma(-kb, y[c], x[q][c]);  // :141
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
      if (live[q]) {
        if (FUSED) {  // posterior members out (assimilation.py:168)
          if (touched[q]) {
#pragma unroll
            for (int c = 0; c < 2 * NC; ++c) x[q][c] += xm[q];
          } else {  // no ob reaches the row: its prior members bit for bit, which (x - mean) + mean is not
            load_row<L, NC, VEC>(a.Xin + (size_t)row[q] * M, M, j, x[q]);
          }
        }
        store_row<L, NC, VEC>(a.Xout + (size_t)row[q] * M, M, j, x[q]);
        if (!FUSED && j == 0) a.xout[row[q]] = xm[q];
        if (ADAPT && j == 0) {
          a.infl[2 * row[q]] = lam[q];
          a.infl[2 * row[q] + 1] = sd[q];
        }
      }
    }
  }
}

// E float: a lane still owns a whole row, loads it with the widest loads its alignment allows (16 bytes when M % 4 == 0
// and the base is 16-byte aligned, else 8 bytes, else 4) widened as they arrive, and rounds each posterior member once at its store; everything between is the float64
// arithmetic of the double kernel, in its order.
template <int FAM, typename E, int MP, bool FUSED>  // members padded to a multiple of 4; FUSED: prior members in, posterior members out
__global__ __launch_bounds__(256, gc_lane_waves(FAM, MP)) void k_sweep_gc_lane(const GcSweepArgs a) {
  constexpr bool ADAPT = FAM == kGcAdapt;
  constexpr bool VLOC = FAM == kGcVloc || FAM == kGcSlab;
  constexpr bool SLAB = FAM == kGcSlab;  // VLOC with the factor read from the slab table
  constexpr bool SEC = FAM == kGcSec;
  static_assert(!(ADAPT && VLOC), "adaptive inflation with vertical localisation is not built");
  static_assert(VLOC || !SLAB, "the slab table is a form of the per-slab factor");
  static_assert(sizeof(E) == sizeof(double) || (FUSED && !ADAPT), "float32 rows: member form, no adaptive inflation");
  constexpr int NG = (MP + 15) / 16;  // ye registers per lane
  constexpr int YS = 16 * NG;         // padded ye row in LDS (doubles)
  __shared__ __align__(16) double ye_s[kChunkL * YS];
  __shared__ __align__(16) double2 ab_s[kChunkL * kBlkCols];
  __shared__ __align__(16) double aw_s[ADAPT ? kChunkL * kBlkCols : 1];  // ADAPT: as in k_sweep_gc
  __shared__ __align__(16) double2 ao_s[ADAPT ? 2 * kChunkL : 1];
  __shared__ __align__(16) double vf_s[VLOC ? kChunkL * 16 : 1];  // VLOC: the vertical factor per (staged ob, slab of the group), 0 beyond the last
  __shared__ __align__(16) double sec_s[SEC ? kSecMaxT : 1];      // SEC: as in k_sweep_gc
  __shared__ __align__(16) double yy_s[SEC ? kChunkL : 1];
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  // One workgroup per (column block, group of 16 slabs), blocks longest list first, a block's groups next to each other (its
  // list stays in L2) but starting at a different group from block to block.  (The list is staged once per group of slabs
  // whichever workgroup takes it, so the fine split costs nothing.  The hardware deals consecutive workgroups to the eight
  // XCDs in turn: with several groups per workgroup and unequal parts, the larger parts of every block landed on the same
  // XCDs -- measured as up to 25 % imbalance on a polar shard; all blocks' first groups, then all second groups, ... is even
  // but 2.5 % slower on the whole grid, the lists leaving L2 between a block's groups.)
  const long pos = blockIdx.x / a.lead_split;
  const long b = a.order[pos];
  const int lead_lo = 16 * (int)((blockIdx.x % a.lead_split + pos) % a.lead_split);
  const int lead_hi = (lead_lo + 16 < (int)a.n_lead) ? lead_lo + 16 : (int)a.n_lead;
  const int M = a.M, M2 = M / 2;
  const double rM1 = 1.0 / (double)(M - 1);
  const long e0 = a.off[b], e1 = e0 + a.cnt[b];
  const auto seq = std::make_integer_sequence<int, MP>{};
  const SecLookup sec{sec_s, SEC ? a.sec_T : 2};
  if (SEC)  // (read behind the barriers of the first chunk's staging)
    for (int i = tid; i < a.sec_T; i += 256) sec_s[i] = a.sec_tab[i];

  for (int lead0 = lead_lo; lead0 < lead_hi; lead0 += 16) {
    // 16 slabs x 4 columns per wave; the last group of a block: the next power of two of what is left, more columns per wave
    const int rem = lead_hi - lead0;
    const int lg_cols = (rem > 8) ? 2 : (rem > 4) ? 3 : (rem > 2) ? 4 : (rem > 1) ? 5 : 6;
    const int ncw = 1 << lg_cols;                 // columns per wave
    const int cq = (lane & (ncw - 1)) + ncw * wave;
    const int lead = lead0 + (lane >> lg_cols);
    const long col = b * kBlkCols + cq;
    const bool live = cq < kBlkCols && col < a.ncol && lead < lead_hi;
    const bool any_live = __ballot(live) != 0ull;
    const long row = (long)lead * a.ncol + col;
    double x[MP];
    double xm = 0.0;
    double lam = 1.0, sd = 0.0, ss = 0.0;  // ADAPT: the row's inflation and x'.x'; SEC: x'.x'
    bool touched = false;                  // FUSED: some ob moved the row
    if (live && sizeof(E) != sizeof(double)) {
      const float* pf = reinterpret_cast<const float*>(a.Xin) + (size_t)row * M;
      if (M == MP && (reinterpret_cast<uintptr_t>(pf) & 15u) == 0) {  // M % 4 == 0 and a 16-byte aligned base: 16-byte loads
#pragma unroll
        for (int i = 0; i < MP / 4; ++i) {
          const float4 v = reinterpret_cast<const float4*>(pf)[i];
          x[4 * i] = v.x;
          x[4 * i + 1] = v.y;
          x[4 * i + 2] = v.z;
          x[4 * i + 3] = v.w;
        }
      } else if ((reinterpret_cast<uintptr_t>(pf) & 7u) == 0) {  // (M is even: uniform over the launch)
#pragma unroll
        for (int i = 0; i < MP / 2; ++i) {
          const float2 v = (i < M2) ? reinterpret_cast<const float2*>(pf)[i] : make_float2(0.f, 0.f);
          x[2 * i] = v.x;
          x[2 * i + 1] = v.y;
        }
      } else {
#pragma unroll
        for (int i = 0; i < MP; ++i) x[i] = (i < M) ? (double)pf[i] : 0.0;
      }
    } else if (live) {
      const double2* p = reinterpret_cast<const double2*>(a.Xin + (size_t)row * M);
      if (M == MP) {
#pragma unroll
        for (int i = 0; i < MP / 2; ++i) {
          const double2 v = p[i];
          x[2 * i] = v.x;
          x[2 * i + 1] = v.y;
        }
      } else {
#pragma unroll
        for (int i = 0; i < MP / 2; ++i) {
          const double2 v = (i < M2) ? p[i] : make_double2(0.0, 0.0);
          x[2 * i] = v.x;
          x[2 * i + 1] = v.y;
        }
      }
    }
    if (live) {
      if (FUSED) {  // prior members in: remove the ensemble mean (assimilation.py:146-147)
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
        for (int i = 0; i < MP; i += 4) {
          s0 += x[i];
          s1 += x[i + 1];
          s2 += x[i + 2];
          s3 += x[i + 3];
        }
        xm = ((s0 + s1) + (s2 + s3)) / (double)M;
#pragma unroll
        for (int i = 0; i < MP; ++i) x[i] = (i < M) ? x[i] - xm : 0.0;
      } else {
        xm = a.xin[row];
      }
      if (ADAPT) {
        lam = a.infl[2 * row];
        sd = a.infl[2 * row + 1];
      }
      if (ADAPT || SEC) {
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
#pragma unroll
        for (int i = 0; i < MP; i += 4) {  // (padding slots hold 0)
          q0 = __builtin_fma(x[i], x[i], q0);
          q1 = __builtin_fma(x[i + 1], x[i + 1], q1);
          q2 = __builtin_fma(x[i + 2], x[i + 2], q2);
          q3 = __builtin_fma(x[i + 3], x[i + 3], q3);
        }
        ss = (q0 + q1) + (q2 + q3);
      }
    } else {
#pragma unroll
      for (int i = 0; i < MP; ++i) x[i] = 0.0;
    }
    for (long c0 = e0; c0 < e1; c0 += kChunkL) {
      const int ne = (int)((e1 - c0 < kChunkL) ? (e1 - c0) : kChunkL);
      __syncthreads();  // previous chunk fully consumed
      {
        constexpr int S2 = YS / 2;
        for (int i = tid; i < ne * S2; i += 256) {
          const int ee = i / S2, m2 = i - ee * S2;
          const int k = a.idx[c0 + ee];
          reinterpret_cast<double2*>(ye_s)[i] =
              (m2 < M2) ? reinterpret_cast<const double2*>(a.Ye + (size_t)k * a.ye_stride)[m2] : make_double2(0.0, 0.0);
        }
      }
      for (int i = tid; i < ne * kBlkCols; i += 256) {  // the folded gain scalars, as in k_sweep_gc
        const double w = a.wts[(size_t)c0 * kBlkCols + i];
        const double* ck = a.coef + (size_t)a.idx[c0 + i / kBlkCols] * kCoefStride;
        const double g = (w * rM1) * ck[1];
        ab_s[i] = make_double2(g * ck[2], g * ck[0]);
        if (ADAPT) aw_s[i] = (ck[3] != 0.0) ? w : 0.0;
      }
      if (ADAPT)
        for (int i = tid; i < 2 * ne; i += 256) ao_s[i] = reinterpret_cast<const double2*>(a.adapt_ob + (size_t)a.idx[c0 + (i >> 1)] * 4)[i & 1];
      if (SEC)
        for (int i = tid; i < ne; i += 256) yy_s[i] = a.adapt_ob[(size_t)a.idx[c0 + i] * 4 + 3];
      if (VLOC)
        for (int i = tid; i < ne * 16; i += 256) {
          const int lead_i = lead0 + (i & 15);
          const int k = a.idx[c0 + (i >> 4)];
          if (SLAB) vf_s[i] = (lead_i < lead_hi) ? a.slab_tab[(size_t)k * a.n_lead + lead_i] : 0.0;  // 16 consecutive doubles per staged ob
          else vf_s[i] = (lead_i < lead_hi) ? vert_factor(a.lead_vert[lead_i], a.ob_vert[k], a.ob_vhw[k]) : 0.0;
        }
      __syncthreads();
      // the staged observations with a non-zero taper on any of this wave's columns, as a bit mask (wave-uniform); with the vertical
      // factor, on any of its columns AND any of its slabs: a wave skips the obs that none of its rows can reach
      bool mine = false;
      if (lane < ne && any_live) {
        const int c_lo = ncw * wave, c_hi = (c_lo + ncw < kBlkCols) ? c_lo + ncw : kBlkCols;
        for (int c = c_lo; c < c_hi; ++c) mine = mine || (ab_s[lane * kBlkCols + c].x != 0.0);
        if (VLOC && mine) {
          bool vz = false;
          for (int t = 0; t < (64 >> lg_cols) && t < 16; ++t) vz = vz || (vf_s[lane * 16 + t] != 0.0);
          mine = vz;
        }
      }
      unsigned long long todo = __ballot(mine);
      if (todo == 0ull) continue;
      const double2* abq = ab_s + (cq & (kBlkCols - 1));  // (a lane beyond the block's 16 columns holds a zero row: whatever it reads is multiplied by 0)
      const double* yq = ye_s + (lane & 15);
      const double* vq = vf_s + (VLOC ? (lane >> lg_cols) : 0);  // VLOC: the lane's slab slot (< 16 in every layout)
      int ee = __builtin_ctzll(todo);
      todo &= todo - 1;
      double2 ab = abq[ee * kBlkCols];
      if (VLOC) {  // the row's slab: both gain scalars times its vertical factor (1: unchanged bit for bit)
        const double v = vq[ee * 16];
        ab.x *= v;
        ab.y *= v;
      }
      double y[NG];
#pragma unroll
      for (int c = 0; c < NG; ++c) y[c] = yq[ee * YS + 16 * c];
      while (true) {
        const int en = (todo != 0ull) ? __builtin_ctzll(todo) : ee;  // the next one (after the last: itself again, harmlessly)
        const double dot = lane_dot<MP>(x, y, seq);      // :95
        double2 abn = abq[en * kBlkCols];
        if (VLOC) {
          const double vn = vq[en * 16];
          abn.x *= vn;
          abn.y *= vn;
        }
        double yy = 0.0;
        if (SEC) {  // both gain scalars times the factor of the pair's correlation, as in k_sweep_gc
          yy = yy_s[ee];
          const double al = sec(dot, ss, yy);
          ab.x *= al;
          ab.y *= al;
        }
        xm = __builtin_fma(ab.y, dot, xm);               // :115, :119, :130
        const double nkb = -(ab.x * dot);                // :115, :119, :136
        if (FUSED) touched = touched || (ab.x != 0.0);
        if (ADAPT) {
          lane_update<MP>(x, y, nkb);  // :141
          const double2 o23 = ao_s[2 * ee + 1];
          anderson_update(lam, sd, aw_s[ee * kBlkCols + (cq & (kBlkCols - 1))], dot, ss, ao_s[2 * ee], o23, a.infl_lower, a.infl_upper,
                          a.infl_sd_lower);
          ss = adapt_ss_after(ss, ab.x * dot, dot, o23.y);
#pragma unroll
          for (int c = 0; c < NG; ++c) y[c] = yq[en * YS + 16 * c];
        } else {
          if (SEC) ss = adapt_ss_after(ss, ab.x * dot, dot, yy);
          lane_update_prefetch<MP>(x, y, nkb, yq + en * YS);  // :141
        }
        if (todo == 0ull) break;
        todo &= todo - 1;
        ee = en;
        ab = abn;
      }
    }
    // FUSED, and no ob reaches the row: its prior members go out bit for bit, which (x - mean) + mean is not (-0.0: x + -0.0 is x)
    if constexpr (FUSED) {
      if (live && !touched) {
        if (sizeof(E) != sizeof(double)) {
          const float* pf = reinterpret_cast<const float*>(a.Xin) + (size_t)row * M;
#pragma unroll
          for (int i = 0; i < MP; ++i) x[i] = (i < M) ? (double)pf[i] : 0.0;
        } else {
          const double2* p = reinterpret_cast<const double2*>(a.Xin + (size_t)row * M);
#pragma unroll
          for (int i = 0; i < MP / 2; ++i) {
            const double2 v = (i < M2) ? p[i] : make_double2(0.0, 0.0);
            x[2 * i] = v.x;
            x[2 * i + 1] = v.y;
          }
        }
        xm = -0.0;
      }
    }
    if (live && sizeof(E) != sizeof(double)) {  // posterior members out, each rounded to float32 once
      float* pf = reinterpret_cast<float*>(a.Xout) + (size_t)row * M;
      if (M == MP && (reinterpret_cast<uintptr_t>(pf) & 15u) == 0) {
#pragma unroll
        for (int i = 0; i < MP / 4; ++i)
          reinterpret_cast<float4*>(pf)[i] = make_float4((float)(x[4 * i] + xm), (float)(x[4 * i + 1] + xm), (float)(x[4 * i + 2] + xm),
                                                         (float)(x[4 * i + 3] + xm));
      } else if ((reinterpret_cast<uintptr_t>(pf) & 7u) == 0) {
#pragma unroll
        for (int i = 0; i < MP / 2; ++i)
          if (i < M2) reinterpret_cast<float2*>(pf)[i] = make_float2((float)(x[2 * i] + xm), (float)(x[2 * i + 1] + xm));
      } else {
#pragma unroll
        for (int i = 0; i < MP; ++i)
          if (i < M) pf[i] = (float)(x[i] + xm);
      }
    } else if (live) {  // posterior members out (assimilation.py:168), or perturbations and mean
      double2* p = reinterpret_cast<double2*>(a.Xout + (size_t)row * M);
      const double add = FUSED ? xm : 0.0;
      if (M == MP) {
#pragma unroll
        for (int i = 0; i < MP / 2; ++i) p[i] = make_double2(x[2 * i] + add, x[2 * i + 1] + add);
      } else {
#pragma unroll
        for (int i = 0; i < MP / 2; ++i)
          if (i < M2) p[i] = make_double2(x[2 * i] + add, x[2 * i + 1] + add);
      }
      if (!FUSED) a.xout[row] = xm;
      if (ADAPT) {
        a.infl[2 * row] = lam;
        a.infl[2 * row + 1] = sd;
      }
    }
  }
}

#endif  // EFA_GCSWEEP_KERNELS_H
