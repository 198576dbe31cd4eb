// The streamed host-memory update (include/efa_hip.h: efa_ensrf_cycle_host, efa_ensrf_cycle_host_f32, efa_pinned_alloc / efa_pinned_free): the prior stays in
// host memory and crosses the device in chunks of (y, x) columns.  Upload of chunk i+1, state phase of chunk i and download of
// chunk i-1 overlap on three streams; Phase A runs on the context's stream while the first chunks upload.  No kernel lives here:
// a chunk is a column shard (row lead*(hi-lo) + (col-lo)), so the obs phase and the member-form state call serve it as they are.
#include "efa_driver.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

namespace {

using namespace efa_host;

// the block of efa_pinned_alloc that holds [p, p + bytes), or null
const PinnedBlock* find_block(const StreamState& st, const void* p, size_t bytes) {
  const char* a = static_cast<const char*>(p);
  for (const PinnedBlock& b : st.blocks) {
    const char* lo = static_cast<const char*>(b.p);
    if (a >= lo && a + bytes <= lo + b.bytes) return &b;
  }
  return nullptr;
}

// One call: the segments as they lie in host memory, the chunk plan and the ring.  esz: bytes per stored state element, 8
// (efa_ensrf_cycle_host) or 4 (efa_ensrf_cycle_host_f32): the images, the ring, the copies and their pitches are in these elements.
struct Call {
  int n_seg = 0, M = 0;
  size_t esz = sizeof(double);
  const void* const* in = nullptr;
  void* const* out = nullptr;
  const long* slabs = nullptr;
  long ncol = 0, n_lead = 0, cc = 0, nchunk = 0;  // columns, slabs of all segments, columns of a full chunk, chunks
  bool in_pinned = false, out_pinned = false;
  size_t slot_bytes = 0;  // one ring buffer: a full chunk
  long lo(long i) const { return i * cc; }
  long hi(long i) const { return std::min(ncol, (i + 1) * cc); }
  size_t chunk_bytes(long i) const { return (size_t)n_lead * (size_t)(hi(i) - lo(i)) * M * esz; }
};

// Bytes [b0, b1) of chunk i's device image <-> the caller's segments (to_stage: host segments -> image, else image -> segments).
// The image is slab after slab, each (hi-lo)*M elements; slab `lead` of the image is slab lead - lead0(v) of its segment v.
void copy_image_range(const Call& k, long i, char* image, size_t b0, size_t b1, bool to_stage) {
  const size_t slab_b = (size_t)(k.hi(i) - k.lo(i)) * k.M * k.esz;
  const size_t pitch_b = (size_t)k.ncol * k.M * k.esz, off_b = (size_t)k.lo(i) * k.M * k.esz;
  long lead0 = 0;
  for (int v = 0; v < k.n_seg; ++v) {
    for (long s = 0; s < k.slabs[v]; ++s) {
      const size_t i0 = (size_t)(lead0 + s) * slab_b, i1 = i0 + slab_b;
      const size_t a = std::max(i0, b0), b = std::min(i1, b1);
      if (a >= b) continue;
      const size_t host_off = (size_t)s * pitch_b + off_b + (a - i0);
      if (to_stage) std::memcpy(image + a, reinterpret_cast<const char*>(k.in[v]) + host_off, b - a);
      else std::memcpy(reinterpret_cast<char*>(k.out[v]) + host_off, image + a, b - a);
    }
    lead0 += k.slabs[v];
  }
}
// ... the whole image, by a few threads when it is large (one core copies a fraction of what the link moves: DESIGN.md 7f has the measured rate)
void copy_image(const Call& k, long i, char* image, bool to_stage) {
  const size_t total = k.chunk_bytes(i);
  const int T = total >= ((size_t)8 << 20) ? 4 : 1;
  if (T == 1) {
    copy_image_range(k, i, image, 0, total, to_stage);
    return;
  }
  std::thread th[3];
  const size_t part = ((total / T) + 63) & ~(size_t)63;
  for (int t = 1; t < T; ++t)
    th[t - 1] = std::thread([&k, i, image, to_stage, part, total, t] {
      copy_image_range(k, i, image, std::min(total, t * part), std::min(total, (t + 1) * part), to_stage);
    });
  copy_image_range(k, i, image, 0, std::min(total, part), to_stage);
  for (int t = 1; t < T; ++t) th[t - 1].join();
}

// chunk i between a pinned caller segment and its ring buffer, by DMA: one strided copy per segment
int copy_segments_dma(const Call& k, long i, char* dev, bool up, hipStream_t s) {
  const long cw = k.hi(i) - k.lo(i);
  const size_t slab_b = (size_t)cw * k.M * k.esz, pitch_b = (size_t)k.ncol * k.M * k.esz;
  const size_t off_b = (size_t)k.lo(i) * k.M * k.esz;
  long lead0 = 0;
  for (int v = 0; v < k.n_seg; ++v) {
    char* d = dev + (size_t)lead0 * slab_b;
    const long h = k.slabs[v];
    lead0 += h;
    if (h == 0) continue;
    const char* src = reinterpret_cast<const char*>(k.in[v]) + off_b;
    char* dst = reinterpret_cast<char*>(k.out[v]) + off_b;
    if (h == 1 || cw == k.ncol) {  // contiguous
      if (up) EFA_HIP(hipMemcpyAsync(d, src, slab_b * h, hipMemcpyHostToDevice, s));
      else EFA_HIP(hipMemcpyAsync(dst, d, slab_b * h, hipMemcpyDeviceToHost, s));
    } else if (up) {
      EFA_HIP(hipMemcpy2DAsync(d, slab_b, src, pitch_b, slab_b, (size_t)h, hipMemcpyHostToDevice, s));
    } else {
      EFA_HIP(hipMemcpy2DAsync(dst, pitch_b, d, slab_b, slab_b, (size_t)h, hipMemcpyDeviceToHost, s));
    }
  }
  return EFA_OK;
}

enum Ev { kUp0 = 0, kUp1, kSt0, kSt1, kDn0, kDn1, kPerChunk };

struct Pipe {
  efa_ctx* c;
  Call k;
  hipStream_t up, dn;
  hipEvent_t ev(long i, int which) const { return c->st.events[(size_t)i * kPerChunk + which]; }
  char* slot(long i) const { return static_cast<char*>(c->st.ring) + (size_t)(i % StreamState::kRing) * k.slot_bytes; }
};

// chunk i into its ring buffer, on the upload stream, once the download of the chunk that held the buffer is done
int issue_upload(const Pipe& p, long i) {
  const Call& k = p.k;
  StreamState& st = p.c->st;
  if (i >= StreamState::kRing) EFA_HIP(hipStreamWaitEvent(p.up, p.ev(i - StreamState::kRing, kDn1), 0));
  if (k.in_pinned) {
    EFA_HIP(hipEventRecord(p.ev(i, kUp0), p.up));
    EFA_TRY(copy_segments_dma(k, i, p.slot(i), true, p.up));
  } else {
    // the staging image is free once the copy of the chunk that used it last has left it: the one host wait of this path
    if (i >= StreamState::kStage) EFA_HIP(hipEventSynchronize(p.ev(i - StreamState::kStage, kUp1)));
    char* image = static_cast<char*>(st.stage_up[i % StreamState::kStage].p);
    copy_image(k, i, image, true);
    EFA_HIP(hipEventRecord(p.ev(i, kUp0), p.up));
    EFA_HIP(hipMemcpyAsync(p.slot(i), image, k.chunk_bytes(i), hipMemcpyHostToDevice, p.up));
  }
  EFA_HIP(hipEventRecord(p.ev(i, kUp1), p.up));
  return EFA_OK;
}

// chunk i out of its ring buffer, on the download stream, behind its state phase
int issue_download(const Pipe& p, long i) {
  const Call& k = p.k;
  StreamState& st = p.c->st;
  EFA_HIP(hipStreamWaitEvent(p.dn, p.ev(i, kSt1), 0));
  EFA_HIP(hipEventRecord(p.ev(i, kDn0), p.dn));
  if (k.out_pinned) EFA_TRY(copy_segments_dma(k, i, p.slot(i), false, p.dn));
  else EFA_HIP(hipMemcpyAsync(st.stage_dn[i % StreamState::kStage].p, p.slot(i), k.chunk_bytes(i), hipMemcpyDeviceToHost, p.dn));
  EFA_HIP(hipEventRecord(p.ev(i, kDn1), p.dn));
  return EFA_OK;
}

// staged download: chunk i from its pinned image into the caller's segments, once the copy has arrived
int drain_download(const Pipe& p, long i) {
  if (p.k.out_pinned) return EFA_OK;
  EFA_HIP(hipEventSynchronize(p.ev(i, kDn1)));
  copy_image(p.k, i, static_cast<char*>(p.c->st.stage_dn[i % StreamState::kStage].p), false);
  return EFA_OK;
}

// the state phase of chunk i, in place in its ring buffer, on the context's stream
int issue_state_phase(const Pipe& p, long i, int loc_mode, const double* grid_lat, const double* grid_lon, long* launches) {
  efa_ctx* c = p.c;
  const Call& k = p.k;
  const long cw = k.hi(i) - k.lo(i), rows = k.n_lead * cw;
  hipStream_t s = c->stream;
  EFA_HIP(hipStreamWaitEvent(s, p.ev(i, kUp1), 0));
  if (loc_mode == EFA_LOC_GC) {
    // the chunk's columns of the grid, from the copy of the whole grid the call put on the device: in stream order, no host wait
    // (an upload would copy from the caller's arrays and wait)
    EFA_TRY(c->grid.take_slice(s, c->st.grid.as<double>(), k.ncol, k.lo(i), cw));
  }
  EFA_HIP(hipEventRecord(p.ev(i, kSt0), s));
  const StateRows X{p.slot(i), p.slot(i), k.esz == sizeof(float) ? Elem::f32 : Elem::f64, rows, k.M};
  // the chunk loop keeps its own events: the context's per-call timing would make every state phase wait for its end
  StateCall sc;
  sc.grid_current = true;
  sc.timed = false;
  const double *glat = loc_mode == EFA_LOC_GC ? grid_lat + k.lo(i) : nullptr, *glon = loc_mode == EFA_LOC_GC ? grid_lon + k.lo(i) : nullptr;
  const long ncol = loc_mode == EFA_LOC_GC ? cw : rows, n_lead = loc_mode == EFA_LOC_GC ? k.n_lead : 1;
  EFA_TRY(state_cycle(c, X, glat, glon, ncol, n_lead, sc));
  *launches += c->state_launches;
  EFA_HIP(hipEventRecord(p.ev(i, kSt1), s));
  return EFA_OK;
}

long elapsed_us(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return (long)(ms * 1000.0f + 0.5f);
}

int run_pipeline(Pipe& p, long P, const double* HX, const ObsIn& ob, const double* grid_lat, const double* grid_lon, const DiagOut& diag) {
  efa_ctx* c = p.c;
  const int loc_mode = ob.loc_mode;
  StreamState& st = c->st;
  const Call& k = p.k;
  hipStream_t s = c->stream;
  const int M = k.M;
  // the copy streams take over from whatever the context issued before (the ring, the staging images), as a change of stream does
  EFA_HIP(hipEventRecord(c->ev_order, s));
  EFA_HIP(hipStreamWaitEvent(p.up, c->ev_order, 0));
  EFA_HIP(hipStreamWaitEvent(p.dn, c->ev_order, 0));
  // the obs block first, on the context's stream: Phase A needs nothing else
  EFA_TRY(st.HX.reserve((size_t)(P ? P : 1) * M * sizeof(double)));
  EFA_TRY(st.ym.reserve((size_t)(P ? P : 1) * sizeof(double)));
  if (P) {
    const size_t nb = (size_t)P * M * sizeof(double);
    EFA_TRY(st.pin_obs.reserve(nb));
    std::memcpy(st.pin_obs.p, HX, nb);
    EFA_HIP(hipMemcpyAsync(st.HX.p, st.pin_obs.p, nb, hipMemcpyHostToDevice, s));
    EFA_TRY(form_perts(c, P, M, st.HX.as<double>(), 1.0, st.ym.as<double>(), st.HX.as<double>()));  // assimilation.py:46-48
  }
  if (loc_mode == EFA_LOC_GC && k.nchunk > 0) {
    const size_t nb = (size_t)k.ncol * sizeof(double);
    EFA_TRY(st.pin_grid.reserve(2 * nb));
    EFA_TRY(st.grid.reserve(2 * nb));
    EFA_TRY(c->grid.reserve(k.cc));
    std::memcpy(st.pin_grid.p, grid_lat, nb);
    std::memcpy(static_cast<char*>(st.pin_grid.p) + nb, grid_lon, nb);
    EFA_HIP(hipMemcpyAsync(st.grid.p, st.pin_grid.p, 2 * nb, hipMemcpyHostToDevice, s));
  }
  // The first chunks go up while Phase A runs (its host round trips do not hold the upload stream).  From pinned memory queueing
  // them costs the host nothing; a staged chunk is a host copy first, so only chunk 0 is staged ahead of Phase A -- the obs block
  // is already on its way -- and chunk 1 follows once Phase A is done.
  long issued = 0;
  const long ahead = k.in_pinned ? StreamState::kRing - 1 : 1;
  for (; issued < k.nchunk && issued < ahead; ++issued) EFA_TRY(issue_upload(p, issued));
  EFA_TRY(obs_phase(c, M, P, st.ym.as<double>(), st.HX.as<double>(), ob, diag));
  long launches = 0;
  int rc = EFA_OK;
  for (long i = 0; i < k.nchunk && rc == EFA_OK; ++i) {
    rc = issue_state_phase(p, i, loc_mode, grid_lat, grid_lon, &launches);
    if (rc == EFA_OK) rc = issue_download(p, i);
    // up to chunk i+2, which goes into the ring buffer chunk i-1 is leaving (its download's event was recorded in the previous turn)
    while (rc == EFA_OK && issued < k.nchunk && issued <= i + StreamState::kRing - 1) {
      rc = issue_upload(p, issued);
      if (rc == EFA_OK) ++issued;
    }
    if (rc == EFA_OK && i > 0) rc = drain_download(p, i - 1);
  }
  if (rc == EFA_OK && k.nchunk > 0) rc = drain_download(p, k.nchunk - 1);
  EFA_TRY(rc);
  EFA_HIP(hipStreamSynchronize(p.dn));
  EFA_HIP(hipStreamSynchronize(p.up));
  EFA_HIP(hipStreamSynchronize(s));
  // efa_last_timing: state_ms is the sum over the chunks
  double state_ms = 0.0;
  st.h2d_us = st.d2h_us = 0;
  for (long i = 0; i < k.nchunk; ++i) {
    st.h2d_us += elapsed_us(p.ev(i, kUp0), p.ev(i, kUp1));
    st.d2h_us += elapsed_us(p.ev(i, kDn0), p.ev(i, kDn1));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.ev(i, kSt0), p.ev(i, kSt1)) == hipSuccess) state_ms += ms;
    else (void)hipGetLastError();
  }
  c->state_ms = state_ms;
  c->state_launches = launches;
  if (c->timing == 2) c->state_ms_sum += state_ms;
  return EFA_OK;
}

// efa_ensrf_cycle_host and efa_ensrf_cycle_host_f32: the state segments hold elements of esz bytes
int cycle_host(efa_ctx* c, size_t esz, int n_seg, const void* const* seg_prior, void* const* seg_post, const long* seg_slabs,
               long ncol, int M, long P, const double* HX, long chunk_cols, const ObsIn& ob, const double* grid_lat, const double* grid_lon,
               const DiagOut& diag) {
  const int loc_mode = ob.loc_mode;
  const char* who = esz == sizeof(float) ? "efa_ensrf_cycle_host_f32" : "efa_ensrf_cycle_host";
  EFA_TRY(use(c));
  const auto t0 = std::chrono::steady_clock::now();
  if (c->ai_field)
    return fail(EFA_ERR_INVALID, "%s: an adaptive-inflation field is set (its update needs the whole state resident)", who);
  if (sec_active(c)) return fail(EFA_ERR_INVALID, "%s: sampling error correction is set (the streamed update does not offer it)", who);
  if (n_seg < 0 || ncol < 0 || P < 0) return fail(EFA_ERR_INVALID, "%s: negative n_seg, ncol or P", who);
  if (M < 2) return fail(EFA_ERR_INVALID, "ensemble size M=%d must be >= 2 (covariance divides by M-1)", M);
  if (chunk_cols < 1) return fail(EFA_ERR_INVALID, "%s: chunk_cols=%ld must be >= 1", who, chunk_cols);
  if (loc_mode != EFA_LOC_NONE && loc_mode != EFA_LOC_GC) return fail(EFA_ERR_INVALID, "loc_mode %d", loc_mode);
  if (n_seg && (!seg_prior || !seg_post || !seg_slabs)) return fail(EFA_ERR_INVALID, "%s: null segment table", who);
  if (P && !HX) return fail(EFA_ERR_INVALID, "%s: null HX", who);
  EFA_TRY(check_batch_solver(c, loc_mode));  // (before the first upload)
  EFA_TRY(check_batch_obs(c, P, ob.error, ob.assim));
  Pipe p{};
  p.c = c;
  Call& k = p.k;
  k.n_seg = n_seg;
  k.M = M;
  k.esz = esz;
  k.in = seg_prior;
  k.out = seg_post;
  k.slabs = seg_slabs;
  k.ncol = ncol;
  const size_t col_b = (size_t)M * esz;
  k.in_pinned = k.out_pinned = true;
  for (int v = 0; v < n_seg; ++v) {
    if (seg_slabs[v] < 0) return fail(EFA_ERR_INVALID, "%s: segment %d has %ld slabs", who, v, seg_slabs[v]);
    k.n_lead += seg_slabs[v];
    if (seg_slabs[v] == 0 || ncol == 0) continue;
    if (!seg_prior[v] || !seg_post[v]) return fail(EFA_ERR_INVALID, "%s: segment %d is null", who, v);
    const size_t seg_b = (size_t)seg_slabs[v] * ncol * col_b;
    k.in_pinned = k.in_pinned && find_block(c->st, seg_prior[v], seg_b);
    k.out_pinned = k.out_pinned && find_block(c->st, seg_post[v], seg_b);
  }
  // the prior is never written, and no posterior segment is written twice: every posterior segment against every prior segment
  // and every other posterior segment
  for (int v = 0; v < n_seg && ncol > 0; ++v) {
    const char* b = reinterpret_cast<const char*>(seg_post[v]);
    const size_t bb = (size_t)seg_slabs[v] * ncol * col_b;
    for (int u = 0; u < n_seg && bb; ++u) {
      const size_t ub = (size_t)seg_slabs[u] * ncol * col_b;
      if (!ub) continue;
      const char* a = reinterpret_cast<const char*>(seg_prior[u]);
      if (!(a + ub <= b || b + bb <= a))
        return fail(EFA_ERR_INVALID, "%s: posterior segment %d overlaps prior segment %d (the prior is never written)", who, v, u);
      const char* o = reinterpret_cast<const char*>(seg_post[u]);
      if (u != v && !(o + ub <= b || b + bb <= o))
        return fail(EFA_ERR_INVALID, "%s: posterior segments %d and %d overlap", who, v, u);
    }
  }
  if (loc_mode == EFA_LOC_GC && k.n_lead * ncol > 0 && (!grid_lat || !grid_lon))
    return fail(EFA_ERR_INVALID, "GC localisation needs grid_lat/grid_lon");
  // cuts on multiples of 16 columns, the one-pass sweep's block; the last chunk takes the ragged rest
  k.cc = std::max(16L, chunk_cols / 16 * 16);
  if (k.cc > ncol) k.cc = std::max(ncol, 1L);
  k.nchunk = (k.n_lead > 0 && ncol > 0) ? (ncol + k.cc - 1) / k.cc : 0;
  k.slot_bytes = (size_t)k.n_lead * k.cc * col_b;
  StreamState& st = c->st;
  if (!c->up_stream) EFA_HIP(hipStreamCreateWithFlags(&c->up_stream.h, hipStreamNonBlocking));
  if (!c->dn_stream) EFA_HIP(hipStreamCreateWithFlags(&c->dn_stream.h, hipStreamNonBlocking));
  p.up = c->up_stream;
  p.dn = c->dn_stream;
  while (st.events.size() < (size_t)k.nchunk * kPerChunk) {
    hipEvent_t e = nullptr;
    EFA_HIP(hipEventCreate(&e));
    st.events.push_back(e);
  }
  const size_t ring_bytes = k.nchunk ? StreamState::kRing * k.slot_bytes : 0;
  if (st.ring_bytes != ring_bytes) {  // to the byte: "stream_peak_bytes" is what the call holds
    if (st.ring) EFA_HIP(hipFree(st.ring));
    st.ring = nullptr;
    st.ring_bytes = 0;
    if (ring_bytes) {
      const hipError_t e = hipMalloc(&st.ring, ring_bytes);
      if (e != hipSuccess) {
        st.ring = nullptr;
        return fail(EFA_ERR_HIP, "hipMalloc(%zu) for the chunk ring failed: %s", ring_bytes, hipGetErrorString(e));
      }
      st.ring_bytes = ring_bytes;
    }
  }
  if (k.nchunk) {
    for (int j = 0; j < StreamState::kStage; ++j) {
      if (!k.in_pinned) EFA_TRY(st.stage_up[j].reserve(k.slot_bytes));
      if (!k.out_pinned) EFA_TRY(st.stage_dn[j].reserve(k.slot_bytes));
    }
  }
  st.chunks = k.nchunk;
  st.peak_bytes = (long)ring_bytes;
  const int rc = run_pipeline(p, P, HX, ob, grid_lat, grid_lon, diag);
  if (rc != EFA_OK) {  // nothing of the call may still be in flight on the way out: it reads and writes the caller's memory
    const std::string msg = efa_last_error();
    (void)hipStreamSynchronize(p.up);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(p.dn);
    (void)hipGetLastError();
    return fail(rc, "%s", msg.c_str());
  }
  st.wall_us = (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  return EFA_OK;
}

}  // namespace

extern "C" {

int efa_pinned_alloc(efa_ctx* c, size_t bytes, void** host_out) {
  EFA_TRY(use(c));
  if (!host_out) return fail(EFA_ERR_INVALID, "null out pointer");
  *host_out = nullptr;
  void* p = nullptr;
  const size_t want = bytes ? bytes : 8;
  EFA_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
  c->st.blocks.push_back(PinnedBlock{p, want});
  *host_out = p;
  return EFA_OK;
}

int efa_pinned_free(efa_ctx* c, void* host) {
  EFA_TRY(use(c));
  if (!host) return EFA_OK;
  std::vector<PinnedBlock>& b = c->st.blocks;
  for (size_t i = 0; i < b.size(); ++i) {
    if (b[i].p != host) continue;
    b.erase(b.begin() + (long)i);
    EFA_HIP(hipHostFree(host));
    return EFA_OK;
  }
  return fail(EFA_ERR_INVALID, "efa_pinned_free: %p is not a block of efa_pinned_alloc on this context", host);
}

int efa_ensrf_cycle_host(efa_ctx* c, int n_seg, const double* const* seg_prior, double* const* seg_post, const long* seg_slabs,
                         long ncol, int M, long P, const double* HX, long chunk_cols, const double* ob_value,
                         const double* ob_error, const uint8_t* ob_assim, int loc_mode, const double* ob_lat, const double* ob_lon,
                         const double* ob_halfwidth_km, const double* grid_lat, const double* grid_lon, double* prior_mean,
                         double* prior_var, double* post_mean, double* post_var, uint8_t* assimilated) {
  return cycle_host(c, sizeof(double), n_seg, reinterpret_cast<const void* const*>(seg_prior), reinterpret_cast<void* const*>(seg_post),
                    seg_slabs, ncol, M, P, HX, chunk_cols, obs_in(ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon, ob_halfwidth_km),
                    grid_lat, grid_lon, diag_out(prior_mean, prior_var, post_mean, post_var, assimilated));
}

int efa_ensrf_cycle_host_f32(efa_ctx* c, int n_seg, const float* const* seg_prior, float* const* seg_post, const long* seg_slabs,
                             long ncol, int M, long P, const double* HX, long chunk_cols, const double* ob_value,
                             const double* ob_error, const uint8_t* ob_assim, int loc_mode, const double* ob_lat,
                             const double* ob_lon, const double* ob_halfwidth_km, const double* grid_lat, const double* grid_lon,
                             double* prior_mean, double* prior_var, double* post_mean, double* post_var, uint8_t* assimilated) {
  return cycle_host(c, sizeof(float), n_seg, reinterpret_cast<const void* const*>(seg_prior), reinterpret_cast<void* const*>(seg_post),
                    seg_slabs, ncol, M, P, HX, chunk_cols, obs_in(ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon, ob_halfwidth_km),
                    grid_lat, grid_lon, diag_out(prior_mean, prior_var, post_mean, post_var, assimilated));
}

}  // extern "C"
