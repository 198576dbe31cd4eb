// The body of the localised impact kernels (efa_impact.hip), included inside each of them: the statements of
// one kernel, written once.  In scope where it is included: the kernel's argument `const ImpactGcArgs a` and the constants
//   MP    members a lane holds at a time, a multiple of 4
//   WIDE  false: MP is M padded (M <= 104), the row mean comes from the registers as in the sweep's member form;
//         true: pieces of MP members, the mean from a first pass over the row
//   FAC   the factor of a (staged ob, slab of the group) pair on top of the horizontal taper (ImpactFactor)
// An include and not a function: k_sweep_gc_lane_impact keeps the instructions it had as a kernel of its own (a __forceinline__
// function handed the arguments compiles to other code).  It belongs to those two kernels of efa_impact.hip and to
// nothing else: that file defines EFA_IMPACT_LANE_BODY in front of them.
#ifndef EFA_IMPACT_LANE_BODY
#error "efa_impact_lane_body.h is the body of the impact kernels of efa_impact.hip: include it nowhere else"
#endif
  constexpr int NG = (MP + 15) / 16;  // ye registers per lane
  constexpr int YS = 16 * NG;         // padded ye row in LDS (doubles)
  __shared__ __align__(16) double ye_s[kImpChunk * YS];
  __shared__ __align__(16) double w_s[kImpChunk * kBlkCols];         // the taper per (staged ob, column)
  __shared__ __align__(16) double vf_s[FAC != kFacNone ? kImpChunk * 16 : 1];   // the factor per (staged ob, slab of the group)
  __shared__ double cs[kImpChunk * kCS];                             // per (staged ob, wave, quad): the quad's contribution
  __shared__ unsigned long long todo_s[4];                           // per wave: the staged obs it did not skip
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  // the hand-out order of k_sweep_gc_lane: blocks longest list first, a block's groups of slabs next to each other
  const long pos = blockIdx.x / a.lead_split;
  const long b = a.order[pos];
  const int grp = (int)((blockIdx.x % a.lead_split + pos) % a.lead_split);
  const int lead0 = 16 * grp;
  const int lead_hi = (lead0 + 16 < (int)a.n_lead) ? lead0 + 16 : (int)a.n_lead;
  const int M = a.M;
  const long e0 = a.off[b], e1 = e0 + a.cnt[b];
  const auto seq = std::make_integer_sequence<int, MP>{};
  // 16 slabs x 4 columns per wave; a group of fewer slabs: the next power of two, more columns per wave (as the sweep folds it)
  const int rem = lead_hi - lead0;
  const int lg_cols = (rem > 8) ? 2 : (rem > 4) ? 3 : (rem > 2) ? 4 : (rem > 1) ? 5 : 6;
  const int ncw = 1 << lg_cols;
  const int cq = (lane & (ncw - 1)) + ncw * wave;
  const int lead = lead0 + (lane >> lg_cols);
  const long col = b * kBlkCols + cq;
  const bool live = cq < kBlkCols && col < a.ncol && lead < lead_hi;
  const bool any_live = __ballot(live) != 0ull;
  const long row = live ? (long)lead * a.ncol + col : 0;
  const double* xrow = a.X + (size_t)row * M;
  const bool vec = (M % 2 == 0) && ((reinterpret_cast<uintptr_t>(a.X) & 15u) == 0);
  const double vi = live ? a.v[row] : 0.0;
  double xm = 0.0;
  if (WIDE && live) {  // the row mean, ahead of the pieces
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int i = 0;
    for (; i + 4 <= M; i += 4) {
      s0 += xrow[i];
      s1 += xrow[i + 1];
      s2 += xrow[i + 2];
      s3 += xrow[i + 3];
    }
    for (; i < M; ++i) s0 += xrow[i];
    xm = ((s0 + s1) + (s2 + s3)) / (double)M;
  }
  const double* wq = w_s + (cq & (kBlkCols - 1));  // (a lane beyond the block's 16 columns holds a zero row: whatever it reads is multiplied by 0)
  const double* yq = ye_s + (lane & 15);
  const double* vq = vf_s + (FAC != kFacNone ? (lane >> lg_cols) : 0);  // the lane's slab slot (< 16 in every layout)

  for (int m0 = 0; m0 < (WIDE ? M : 1); m0 += MP) {
    double x[MP];
    if (live) {
      load_piece<MP>(xrow, M, m0, vec, x);
      if (!WIDE) {  // remove the ensemble mean as the sweep's member form does
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
        for (int i = 0; i < MP; i += 4) {
          s0 += x[i];
          s1 += x[i + 1];
          s2 += x[i + 2];
          s3 += x[i + 3];
        }
        xm = ((s0 + s1) + (s2 + s3)) / (double)M;
      }
#pragma unroll
      for (int i = 0; i < MP; ++i) x[i] = (m0 + i < M) ? (x[i] - xm) * vi : 0.0;  // v_i Xf'_i
    } else {
#pragma unroll
      for (int i = 0; i < MP; ++i) x[i] = 0.0;
    }
    for (long c0 = e0; c0 < e1; c0 += kImpChunk) {
      const int ne = (int)((e1 - c0 < kImpChunk) ? (e1 - c0) : kImpChunk);
      __syncthreads();  // previous chunk fully consumed
      for (int i = tid; i < ne * YS; i += 256) {
        const int ee = i / YS, m = i - ee * YS;
        const int k = a.idx[c0 + ee];
        ye_s[i] = (m < MP && m0 + m < M) ? a.Yp[(size_t)k * M + m0 + m] : 0.0;
      }
      for (int i = tid; i < ne * kBlkCols; i += 256) w_s[i] = a.wts[(size_t)c0 * kBlkCols + i];
      if (FAC == kFacVert)
        for (int i = tid; i < ne * 16; i += 256) {
          const int lead_i = lead0 + (i & 15);
          const int k = a.idx[c0 + (i >> 4)];
          vf_s[i] = (lead_i < lead_hi) ? vert_factor(a.lead_vert[lead_i], a.ob_vert[k], a.ob_vhw[k]) : 0.0;
        }
      if (FAC == kFacTable)
        for (int i = tid; i < ne * 16; i += 256) {
          const int lead_i = lead0 + (i & 15);
          const int k = a.idx[c0 + (i >> 4)];
          vf_s[i] = (lead_i < lead_hi) ? a.slab_tab[(size_t)k * a.n_lead + lead_i] : 0.0;  // 16 consecutive doubles per staged ob
        }
      __syncthreads();
      // the staged obs with a non-zero taper on any of this wave's columns (and, with a factor, any of its slabs): wave-uniform mask
      bool mine = false;
      if (lane < ne && any_live) {
        const int c_lo = ncw * wave, c_hi = (c_lo + ncw < kBlkCols) ? c_lo + ncw : kBlkCols;
        for (int c = c_lo; c < c_hi; ++c) mine = mine || (w_s[lane * kBlkCols + c] != 0.0);
        if (FAC != kFacNone && mine) {
          bool vz = false;
          for (int t = 0; t < (64 >> lg_cols) && t < 16; ++t) vz = vz || (vf_s[lane * 16 + t] != 0.0);
          mine = vz;
        }
      }
      unsigned long long todo = __ballot(mine);
      if (lane == 0) todo_s[wave] = todo;
      if (todo != 0ull) {
        // Two ye register sets taken in turn: the LDS reads of the next ob's members are issued ahead of this ob's dot, and each
        // set is written by LDS reads only (no register copy between the sets: a VALU write ahead of a DPP read is the hazard
        // efa_lane_dot.h describes)
        auto one_ob = [&](int ee, const double (&y)[NG]) {
          double w = wq[ee * kBlkCols];
          if (FAC != kFacNone) w = w * vq[ee * 16];  // horizontal taper times the slab's factor, rounded once as the sweep does
          const double dot = lane_dot<MP>(x, y, seq);
          const double q = quad_sum(w * dot);
          if ((lane & 3) == 0) cs[ee * kCS + 16 * wave + (lane >> 2)] = q;
        };
        double ya[NG], yb[NG];
        int ea = __builtin_ctzll(todo), eb = 0;
        todo &= todo - 1;
#pragma unroll
        for (int c = 0; c < NG; ++c) ya[c] = yq[ea * YS + 16 * c];
        while (true) {
          const bool more_b = todo != 0ull;
          if (more_b) {
            eb = __builtin_ctzll(todo);
            todo &= todo - 1;
#pragma unroll
            for (int c = 0; c < NG; ++c) yb[c] = yq[eb * YS + 16 * c];
          }
          one_ob(ea, ya);
          if (!more_b) break;
          const bool more_a = todo != 0ull;
          if (more_a) {
            ea = __builtin_ctzll(todo);
            todo &= todo - 1;
#pragma unroll
            for (int c = 0; c < NG; ++c) ya[c] = yq[ea * YS + 16 * c];
          }
          one_ob(eb, yb);
          if (!more_a) break;
        }
      }
      __syncthreads();
      // per staged ob: its 4 x 16 quad sums in a fixed order (thread 4e + w adds wave w's sixteen, the four are added by quad_sum)
      {
        const int e = tid >> 2, wv = tid & 3;
        double s = 0.0;
        if (e < ne && ((todo_s[wv] >> e) & 1ull)) {
          const double* p = cs + e * kCS + 16 * wv;
#pragma unroll
          for (int i = 0; i < 16; ++i) s += p[i];
        }
        s = quad_sum(s);
        if (e < ne && wv == 0) {
          double* out = a.partial + (size_t)grp * a.cap + (c0 + e);
          *out = (m0 == 0) ? s : *out + s;  // (a later piece: the same thread wrote the earlier ones)
        }
      }
    }
  }
