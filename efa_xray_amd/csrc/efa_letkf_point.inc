// The body of k_letkf and k_letkf_cv (efa_letkf.hip), included as text into both: a kernel's argument block `a`, and the constants
// MODE, E, NTMAX, SLAB, CTRL and CV in scope.  With CV false every `if constexpr (CV)` is discarded and the kernel is the one without
// cross validation; a shared inlined function gave the existing instantiations other code (register numbering, hoisted address
// arithmetic), the text does not.  `a` must be of a dependent type, so that the discarded branches are not looked up.
  static_assert(!CTRL || MODE != kLetkfWeights, "the pair layout [M][M+1] has no place for w^c");
  static_assert(!CV || (MODE == kLetkfWeights && !SLAB && !CTRL), "cross validation: the plain weights mode only");
  extern __shared__ __align__(16) double letkf_smem[];
  const int M = a.M;
  const int tid = (int)threadIdx.x, nth = (int)blockDim.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nW = nth >> 6;
  const int T = letkf_tiles_side(M, CTRL), Sp = letkf_stage_pitch(M, CTRL), ntiles = T * (T + 1) / 2;
  double* G = letkf_smem;                     // the M x M array; before it the stage [32][Sp] | weights [32]
  double* wgt = G + kLetkfChunk * Sp;
  double* g_s = G + letkf_region(M, CTRL);
  double* f_s = g_s + M;
  double* h_s = f_s + M;
  double* n_s = h_s + M;
  double* mu_s = n_s + M;
  double* x_s = mu_s + M;                     // [4][M] rows of a batch: members, perturbations, then posterior perturbations
  double* z_s = x_s + kLetkfRows * M;         // [4][M] V^T x'
  double* mean_s = z_s + kLetkfRows * M;
  double* xam_s = mean_s + kLetkfRows;
  double* ssb_s = xam_s + kLetkfRows;
  double* infl_s = ssb_s + kLetkfRows;         // inflation (§7y-6): lambda_b | p3 | p1 | trace(C)
  int* rot_s = reinterpret_cast<int*>(mean_s + kLetkfSmall);
  int* nloc_s = rot_s + 2;
  double* gc_s = mean_s + kLetkfSmall + 2;    // CTRL: g^c [M] behind the ints (16-byte aligned); h^c takes n_s behind the sweeps

  long bid = (long)blockIdx.x, grp = 0, lead0 = 0, nlead_g = a.n_lead;  // the group, its first entry in grp_leads, its slabs
  const double* Sg = nullptr;                                            // S[.][rep[grp]], pitch sp
  long sp = 0;
  const int* leads = nullptr;
  if constexpr (SLAB) {
    grp = bid % a.grp.ngroups;
    bid = bid / a.grp.ngroups;
    lead0 = a.grp.grp_off[grp];
    nlead_g = a.grp.grp_off[grp + 1] - lead0;
    sp = a.grp.s_pitch;
    Sg = a.grp.S + a.grp.rep[grp];
    leads = a.grp.grp_leads + lead0;
  }
  const long bi = bid >> 4;
  const int cb = (int)(bid & 15);
  const long blk = a.order ? (long)a.order[bi] : bi;
  const long col = blk * 16 + cb;
  if (col >= a.npts) return;  // (uniform)
  const long off = a.off ? a.off[blk] : 0;
  const int n = a.cnt ? a.cnt[blk] : 0;

  // n_local: the listed obs whose taper on THIS column is not zero; under inflation p3, the sum of those tapers (each lane its
  // entries in list order, then the butterfly)
  const bool infl = a.infl != nullptr;  // (uniform)
  if (wave == 0) {
    int cl = 0;
    double p3 = 0.0;
    for (int e = lane; e < n; e += 64) {
      double w = a.wts[(size_t)(off + e) * 16 + cb];
      if constexpr (SLAB) w = w * Sg[(size_t)a.idx[off + e] * sp];
      cl += (w != 0.0) ? 1 : 0;
      if (infl && w != 0.0) p3 += w;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cl += __shfl_xor(cl, o, 64);
    if (infl) p3 = wave_sum(p3);
    if (lane == 0) {
      *nloc_s = cl;
      infl_s[0] = infl ? a.infl[grp * a.npts + col] : 1.0;
      infl_s[1] = p3;
    }
  }
  __syncthreads();
  const int nloc = *nloc_s;

  if (nloc == 0) {  // (uniform) no ob reaches the column: A = (M-1) I, no rotation, T = I, w = 0 -- the rows keep their bits
    if (MODE == kLetkfMembers) {
      const E* in = static_cast<const E*>(a.Xin);
      E* out = static_cast<E*>(a.Xout);
      if (in != out)
        for (long li = 0; li < nlead_g; ++li) {
          long l = li;
          if constexpr (SLAB) l = leads[li];
          const size_t base = (size_t)(l * a.npts + col) * M;
          for (int m = tid; m < M; m += nth) out[base + m] = in[base + m];
        }
      if constexpr (CTRL) {  // the control's rows likewise: copied bit for bit, or left alone in place
        const double* cin = letkf_kernarg()->ctl_in;
        double* cout = letkf_kernarg()->ctl_out;
        if (cin != cout)
          for (long li = tid; li < nlead_g; li += nth) {
            long l = li;
            if constexpr (SLAB) l = leads[li];
            cout[l * a.npts + col] = cin[l * a.npts + col];
          }
      }
    } else if (MODE == kLetkfPerts) {
      for (int m = tid; m < M; m += nth) a.Yp_out[(size_t)col * M + m] = a.Yp_in[(size_t)col * M + m];
      if (tid == 0) a.ym_out[col] = a.ym_in[col];
      if constexpr (CTRL) {
        if (tid == 0) letkf_kernarg()->ctl_out[col] = letkf_kernarg()->ctl_in[col];
      }
    } else {
      double* tw = a.Tw + (size_t)(grp * a.npts + col) * M * (M + 1);
      for (int e = tid; e < M * (M + 1); e += nth) {
        const int r = e / (M + 1), c = e - r * (M + 1);
        tw[e] = (r == c) ? 1.0 : 0.0;
      }
      if constexpr (CV) {  // no sub-solve either: (0, 0), and the point's row of the obs block keeps its bits
        if (a.cv.stats && tid < 2) a.cv.stats[2 * col + tid] = 0.0;
        if (a.Yp_in) {
          for (int m = tid; m < M; m += nth) a.Yp_out[(size_t)col * M + m] = a.Yp_in[(size_t)col * M + m];
          if (tid == 0) a.ym_out[col] = a.ym_in[col];
        }
      }
    }
    if (a.stats && tid < 3) a.stats[3 * (grp * a.npts + col) + tid] = 0.0;
    if (infl && a.infl_stats && tid < 4) a.infl_stats[4 * (grp * a.npts + col) + tid] = (tid < 3) ? 0.0 : __builtin_nan("");  // lambda keeps its bits
    return;
  }

  // ---- 1. Gram ----------------------------------------------------------------------------------------------------------------
  {
    const int g = lane >> 4, nn = lane & 15;
    int ca[kLetkfTiles], cbt[kLetkfTiles];
    letkf_v4 acc[kLetkfTiles];
#pragma unroll
    for (int t = 0; t < kLetkfTiles; ++t) {
      const int ti = wave + t * nW;
      int ta = 0, tb = 0;
      if (ti < ntiles) letkf_tile(ti, T, &ta, &tb);
      ca[t] = 16 * ta + nn;
      cbt[t] = 16 * tb + nn;
      acc[t] = letkf_v4{0.0, 0.0, 0.0, 0.0};
    }
    const int nchunks = (n + kLetkfChunk - 1) / kLetkfChunk;
#pragma unroll 1
    for (int ch = 0; ch < nchunks; ++ch) {
      __syncthreads();  // the previous chunk is consumed
      for (int e = tid; e < kLetkfChunk * Sp; e += nth) {
        const int r = e / Sp, c = e - r * Sp;
        const int en = ch * kLetkfChunk + r;
        double v = 0.0;
        if (en < n && c <= M + (CTRL ? 1 : 0)) {
          const long k = a.idx[off + en];
          if constexpr (CTRL) v = (c < M) ? a.Yp[(size_t)k * M + c] : (c == M) ? a.dr[2 * k] : letkf_kernarg()->dc[k];
          else v = (c < M) ? a.Yp[(size_t)k * M + c] : a.dr[2 * k];
        }
        G[e] = v;
      }
      if (tid < kLetkfChunk) {
        const int en = ch * kLetkfChunk + tid;
        double w = 0.0;
        if (en < n) {
          const long k = a.idx[off + en];
          w = a.wts[(size_t)(off + en) * 16 + cb];
          if constexpr (SLAB) w = w * Sg[(size_t)k * sp];
          w = w / a.dr[2 * k + 1];
        }
        wgt[tid] = w;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < kLetkfTiles; ++t) {
        if (wave + t * nW < ntiles) {  // (wave-uniform)
#pragma unroll
          for (int k = 0; k < kLetkfChunk / 4; ++k) {
            const int row = 4 * k + g;
            const double wv = wgt[row];
            const double ya = G[row * Sp + ca[t]], yb = G[row * Sp + cbt[t]];
            const double oa = (wv != 0.0) ? wv * ya : 0.0;  // a zero weight: exact zeros, whatever the row holds
            const double ob = (wv != 0.0) ? yb : 0.0;
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(oa, ob, acc[t], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();  // the stage is consumed: A goes over it
    const double shift = (double)(M - 1) / infl_s[0];  // the diagonal of A; (M-1)/1.0 is exact: no field, the bits without one
#pragma unroll
    for (int t = 0; t < kLetkfTiles; ++t) {
      const int ti = wave + t * nW;
      if (ti < ntiles) {
        int ta, tb;
        letkf_tile(ti, T, &ta, &tb);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int i = g + 4 * v, j = nn;
          const int I = 16 * ta + i, J = 16 * tb + j;
          if (ta == tb && i > j) continue;  // a diagonal tile holds each pair twice: the upper one is mirrored
          const double s = acc[t][v];
          if (I < M && J < M) {
            const double val = (I == J) ? s + shift : s;
            G[I * M + J] = val;
            G[J * M + I] = val;
            if constexpr (CV) {  // C itself, parked for the sub-solves
              double* Cg = a.cv.C + (size_t)col * M * M;
              Cg[I * M + J] = s;
              Cg[J * M + I] = s;
            }
            if (infl && I == J) n_s[I] = s;  // the diagonal of C, for its trace (n_s is free until the sweeps)
          } else if (I < M && J == M) {
            g_s[I] = s;
          } else if (CTRL && I < M && J == M + 1) {
            gc_s[I] = s;  // g^c; entries (M, M+1) and (M+1, M+1) are dropped
          } else if (infl && I == M && J == M) {
            infl_s[2] = s;  // p1 = sum_k w_k d_k^2
          }
        }
      }
    }
    __syncthreads();
    if (infl) {  // (uniform) trace(C) in a fixed order before the sweeps take n_s
      if (wave == 0) {
        double tr = 0.0;
        for (int j = lane; j < M; j += 64) tr += n_s[j];
        tr = wave_sum(tr);
        if (lane == 0) infl_s[3] = tr;
      }
      __syncthreads();
    }
  }

  // ---- 2. eigen-solve ---------------------------------------------------------------------------------------------------------
  const int sweeps = etkf_jacobi(M, G, n_s, rot_s, tid, nth);
  etkf_factors(M, G, g_s, mu_s, f_s, h_s, tid, nth);
  if constexpr (CTRL) {  // h^c_j = (V_j . g^c) / mu_j over n_s, which the sweeps have left; read behind the apply's first barrier
    const int nslots_c = nth >> 4, slot_c = tid >> 4, sl_c = tid & 15;
#pragma unroll 1
    for (int j = slot_c; j < M; j += nslots_c) {
      const double* cj = G + (size_t)j * M;
      double hg = 0.0;
      for (int i = sl_c; i < M; i += 16) hg = fma(cj[i], gc_s[i], hg);
      hg = group_sum<16>(hg);
      if (sl_c == 0) n_s[j] = hg / mu_s[j];
    }
  }
  if (a.stats && wave == 0) {
    const double shift = (double)(M - 1) / infl_s[0];
    double s = 0.0;
    for (int j = lane; j < M; j += 64) s += (mu_s[j] - shift) / mu_s[j];
    s = wave_sum(s);
    if (lane == 0) {
      a.stats[3 * (grp * a.npts + col)] = (double)nloc;
      a.stats[3 * (grp * a.npts + col) + 1] = s;
      a.stats[3 * (grp * a.npts + col) + 2] = (double)sweeps;
    }
  }

  // ---- 3. [T | w], factored ---------------------------------------------------------------------------------------------------
  if constexpr (CV) {  // w as etkf_assemble forms it (the mean keeps the full-ensemble gain), then T from the parked C
    double* tw = a.Tw + (size_t)col * M * (M + 1);
    for (int r = tid; r < M; r += nth) {
      double acc = 0.0;
      for (int j = 0; j < M; ++j) acc = fma(h_s[j], G[(size_t)j * M + r], acc);
      tw[(size_t)r * (M + 1) + M] = acc;
    }
    letkf_cv_transform(a, M, col, G, g_s, h_s, f_s, n_s, mu_s, x_s, z_s, mean_s, rot_s, tid, nth);
    return;
  }
  if (MODE == kLetkfWeights) {
    double* tw = a.Tw + (size_t)(grp * a.npts + col) * M * (M + 1);
    etkf_assemble(M, G, f_s, h_s, tw, (size_t)(M + 1), tw + M, (size_t)(M + 1), tid, nth);
    if (infl && tid == 0) letkf_inflation_estimate((size_t)(grp * a.npts + col), M, infl_s);
    return;
  }
  const bool rtps = MODE == kLetkfMembers && a.relax_kind == EFA_RELAX_RTPS && a.relax_alpha != 0.0;
  if (MODE == kLetkfMembers && a.relax_kind == EFA_RELAX_RTPP && a.relax_alpha != 0.0) {  // (uniform)
    for (int j = tid; j < M; j += nth) f_s[j] = (1.0 - a.relax_alpha) * f_s[j] + a.relax_alpha;
    __syncthreads();
  }

  // ---- 4. apply ---------------------------------------------------------------------------------------------------------------
  const int nslots = nth >> 4, slot = tid >> 4, sl = tid & 15;
  const long nrows = (MODE == kLetkfMembers) ? nlead_g : 1;
#pragma unroll 1
  for (long r0 = 0; r0 < nrows; r0 += kLetkfRows) {
    const int nr = (int)((nrows - r0 < kLetkfRows) ? nrows - r0 : kLetkfRows);
    for (int e = tid; e < nr * M; e += nth) {
      const int r = e / M, m = e - r * M;
      if (MODE == kLetkfMembers) {
        long l = r0 + r;
        if constexpr (SLAB) l = leads[l];
        x_s[e] = (double)static_cast<const E*>(a.Xin)[(size_t)(l * a.npts + col) * M + m];
      }
      else x_s[e] = a.Yp_in[(size_t)col * M + m];
    }
    __syncthreads();
    if (wave < nr) {  // the row's mean, its perturbations in place, the prior spread
      double* xr = x_s + wave * M;
      if (MODE == kLetkfMembers) {
        double s = 0.0;
        for (int m = lane; m < M; m += 64) s += xr[m];
        const double mean = wave_sum(s) / (double)M;
        double q = 0.0;
        for (int m = lane; m < M; m += 64) {
          const double p = xr[m] - mean;
          xr[m] = p;
          q = fma(p, p, q);
        }
        q = wave_sum(q);
        if (lane == 0) {
          mean_s[wave] = mean;
          ssb_s[wave] = q;
        }
      } else if (lane == 0) {
        mean_s[wave] = a.ym_in[col];
      }
    }
    __syncthreads();
    // z[r][j] = V_j . x'_r
#pragma unroll 1
    for (int pr = slot; pr < nr * M; pr += nslots) {
      const int r = pr / M, j = pr - r * M;
      const double* cj = G + (size_t)j * M;
      const double* xr = x_s + r * M;
      double d = 0.0;
      for (int i = sl; i < M; i += 16) d = fma(cj[i], xr[i], d);
      d = group_sum<16>(d);
      if (sl == 0) z_s[pr] = d;
    }
    __syncthreads();
    if (wave < nr) {  // xam = mean + x' w = mean + h . z
      const double* zr = z_s + wave * M;
      double s = 0.0;
      if constexpr (CTRL) {  // x_c^a = x_c + x' . w^c = x_c + h^c . z, by the wave that owns the row
        double sc = 0.0;
        for (int j = lane; j < M; j += 64) {
          s = fma(h_s[j], zr[j], s);
          sc = fma(n_s[j], zr[j], sc);
        }
        s = wave_sum(s);
        sc = wave_sum(sc);
        if (lane == 0) {
          xam_s[wave] = mean_s[wave] + s;
          long row = col;
          if (MODE == kLetkfMembers) {
            long l = r0 + wave;
            if constexpr (SLAB) l = leads[l];
            row = l * a.npts + col;
          }
          letkf_kernarg()->ctl_out[row] = letkf_kernarg()->ctl_in[row] + sc;  // (the pointers from the argument block, here)
        }
      } else {
        for (int j = lane; j < M; j += 64) s = fma(h_s[j], zr[j], s);
        s = wave_sum(s);
        if (lane == 0) xam_s[wave] = mean_s[wave] + s;
      }
    }
    // x'_a[r][b] = sum_j (f_j z[r][j]) V[b][j], over the prior perturbations (z holds all that is needed of them)
    for (int e = tid; e < nr * M; e += nth) {
      const int r = e / M, b = e - r * M;
      const double* zr = z_s + r * M;
      double acc = 0.0;
      for (int j = 0; j < M; ++j) acc = fma(f_s[j] * zr[j], G[(size_t)j * M + b], acc);
      x_s[e] = acc;
    }
    __syncthreads();
    if (wave < nr) {
      const double* pa = x_s + wave * M;
      const double xam = xam_s[wave];
      if (MODE == kLetkfMembers) {
        long l = r0 + wave;
        if constexpr (SLAB) l = leads[l];
        E* out = static_cast<E*>(a.Xout) + (size_t)(l * a.npts + col) * M;
        if (rtps) {  // the posterior members' own mean and spread, as the standalone pass takes them (§7b)
          double s = 0.0;
          for (int m = lane; m < M; m += 64) s += pa[m];
          const double pm = wave_sum(s) / (double)M;
          double q = 0.0;
          for (int m = lane; m < M; m += 64) {
            const double dv = pa[m] - pm;
            q = fma(dv, dv, q);
          }
          q = wave_sum(q);
          if (q > 0.0) {  // (wave-uniform) sigma_a == 0: the row stays as it is
            const double sc = (1.0 - a.relax_alpha) + a.relax_alpha * sqrt(ssb_s[wave] / q);
            const double base = xam + pm;
            for (int m = lane; m < M; m += 64) out[m] = letkf_round<E>(base + sc * (pa[m] - pm));
          } else {
            for (int m = lane; m < M; m += 64) out[m] = letkf_round<E>(xam + pa[m]);
          }
        } else {
          for (int m = lane; m < M; m += 64) out[m] = letkf_round<E>(xam + pa[m]);
        }
      } else {
        for (int m = lane; m < M; m += 64) a.Yp_out[(size_t)col * M + m] = pa[m];
        if (lane == 0) a.ym_out[col] = xam;
      }
    }
    __syncthreads();  // the batch's rows are stored: the next batch takes x_s
  }
  if (infl && tid == 0) letkf_inflation_estimate((size_t)(grp * a.npts + col), M, infl_s);
