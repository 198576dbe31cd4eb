// C-ABI shell of libefa_hip.so (see include/efa_hip.h): contexts, options and setters, memory helpers, the forward-operator
// wrappers, timing read-out and the public wrappers of the drivers (efa_driver.h says where those live).
#include "efa_driver.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {
thread_local std::string g_last_error;
}  // namespace

namespace efa_host {
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

int use(efa_ctx* c) {
  if (!c) return fail(EFA_ERR_INVALID, "null context");
  EFA_HIP(hipSetDevice(c->device));
  return EFA_OK;
}

int h2d(efa_ctx* c, DevBuf& b, const void* src, size_t bytes) {
  EFA_TRY(b.reserve(bytes ? bytes : 8));
  if (bytes) EFA_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
  return EFA_OK;
}

int form_perts(efa_ctx* c, long rows, int M, const double* X_dev, double scale, double* xm_dev, double* Xp_dev) {
  if (rows < 0 || M < 1 || M > efa::kMaxMembers) return fail(EFA_ERR_INVALID, "bad shape rows=%ld M=%d", rows, M);
  if (rows && (!X_dev || !xm_dev || !Xp_dev)) return fail(EFA_ERR_INVALID, "null pointer");
  EFA_HIP(efa::launch_form_perts(rows, M, X_dev, scale, xm_dev, Xp_dev, c->stream));
  return EFA_OK;
}

// "timing" 2 (deferred): no phase call waits for its own events -- the host may run ahead of the device from one cycle into the
// next.  An interval is read when its events are about to be recorded again (the calls in between have synchronised the stream
// since: the wait returns at once) or in efa_last_timing, and added to running sums.
namespace {
void harvest(Interval& iv, hipEvent_t end, double& last, double& sum) {
  if (!iv.pending) return;
  float ms = 0.f;
  if (hipEventSynchronize(end) == hipSuccess && hipEventElapsedTime(&ms, iv.begin, end) == hipSuccess) {
    last = ms;
    sum += ms;
  } else {
    (void)hipGetLastError();
  }
  iv.pending = false;
}
}  // namespace
void harvest_obs_ms(efa_ctx* c) { harvest(c->obs_iv, c->obs_ends_at, c->obs_ms, c->obs_ms_sum); }
void harvest_state_interval(efa_ctx* c, Interval& iv) { harvest(iv, iv.end, c->state_ms, c->state_ms_sum); }
void harvest_state_ms(efa_ctx* c) {
  harvest_state_interval(c, c->state_iv[0]);
  harvest_state_interval(c, c->state_iv[1]);
}
}  // namespace efa_host

using namespace efa_host;

namespace {

// what efa_ensrf_update_dev and efa_ensrf_cycle_dev check of the context's settings against a cycle's arguments, ahead of both phases
int check_cycle_settings(const efa_ctx* c, int loc_mode, long rows, long P, long n_lead) {
  EFA_TRY(check_adaptive(c, loc_mode, rows));
  EFA_TRY(check_vloc(c, loc_mode, P, n_lead));
  EFA_TRY(check_slab(c, loc_mode, P, n_lead));
  EFA_TRY(check_sec(c, loc_mode));
  return check_batch_solver(c, loc_mode);
}

}  // namespace

extern "C" {

int efa_abi_version(void) { return EFA_ABI_VERSION; }

const char* efa_last_error(void) { return g_last_error.c_str(); }

int efa_device_count(int* count) {
  if (!count) return fail(EFA_ERR_INVALID, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  *count = n;
  return EFA_OK;
}

int efa_ctx_create(int device_id, efa_ctx** out) {
  if (!out) return fail(EFA_ERR_INVALID, "null out pointer");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return fail(EFA_ERR_NO_DEVICE,
                "no HIP device visible (%s): libefa_hip has no CPU fallback and needs an MI355X (gfx950)",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  }
  if (device_id < 0 || device_id >= n) return fail(EFA_ERR_INVALID, "device_id %d out of range [0,%d)", device_id, n);
  hipDeviceProp_t prop;
  EFA_HIP(hipGetDeviceProperties(&prop, device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(EFA_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", device_id,
                prop.gcnArchName);
  EFA_HIP(hipSetDevice(device_id));
  efa_ctx* c = new (std::nothrow) efa_ctx();
  if (!c) return fail(EFA_ERR_INVALID, "out of host memory");
  c->device = device_id;
  c->cu_count = prop.multiProcessorCount;
  hipError_t es = hipStreamCreateWithFlags(&c->own_stream.h, hipStreamNonBlocking);
  if (es != hipSuccess) {
    delete c;
    return fail(EFA_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(es));
  }
  c->stream = c->own_stream;
  for (OwnedEvent* e : {&c->obs_iv.begin, &c->obs_iv.end, &c->state_iv[0].begin, &c->state_iv[0].end, &c->state_iv[1].begin,
                        &c->state_iv[1].end}) {
    hipError_t ee = hipEventCreate(&e->h);
    if (ee != hipSuccess) {
      delete c;
      return fail(EFA_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(ee));
    }
  }
  {
    hipError_t ee = hipEventCreateWithFlags(&c->ev_order.h, hipEventDisableTiming);
    if (ee != hipSuccess) {
      delete c;
      return fail(EFA_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(ee));
    }
  }
  *out = c;
  return EFA_OK;
}

int efa_ctx_destroy(efa_ctx* c) {
  if (!c) return EFA_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  release_comm(c);
  delete c;
  return EFA_OK;
}

namespace {
// The calls return with work still in the stream, and that work reads the context's own workspaces (the transform [T | w] behind
// the obs rows, the recorded trajectory, the active lists, the grid, the pair counter).  What is issued after a change of stream
// is therefore ordered behind everything issued before it: an event on the stream that is left, waited for on the device by the
// one that takes over.  No host wait; NULL (the legacy default stream) is a stream like any other here.
int change_stream(efa_ctx* c, hipStream_t to) {
  if (to == c->stream) return EFA_OK;
  EFA_HIP(hipEventRecord(c->ev_order, c->stream));
  EFA_HIP(hipStreamWaitEvent(to, c->ev_order, 0));
  c->stream = to;
  return EFA_OK;
}
}  // namespace

int efa_ctx_set_stream(efa_ctx* c, void* hip_stream) {
  EFA_TRY(use(c));
  // NULL is a valid handle: the device's legacy default stream (what torch uses unless told otherwise)
  return change_stream(c, reinterpret_cast<hipStream_t>(hip_stream));
}

namespace {
// The grid caps of the diagnostics' kernels (0: the default, which is also the bound); the results do not depend on them.
struct BlocksOption {
  const char* key;
  long efa_ctx::*member;
  long bound;
};
const BlocksOption kBlocksOptions[] = {{"verify_blocks", &efa_ctx::verify_blocks, 2048},
                                       {"products_blocks", &efa_ctx::products_blocks, 2048},
                                       {"gram_blocks", &efa_ctx::gram_blocks, 2048},
                                       {"neighbourhood_blocks", &efa_ctx::neighbourhood_blocks, 2048},
                                       {"pm_blocks", &efa_ctx::pm_blocks, 2048}};
const BlocksOption* blocks_option(const char* key) {
  for (const BlocksOption& o : kBlocksOptions)
    if (!strcmp(key, o.key)) return &o;
  return nullptr;
}
}  // namespace

int efa_ctx_set_option(efa_ctx* c, const char* key, long value) {
  EFA_TRY(use(c));
  if (!key) return fail(EFA_ERR_INVALID, "null option key");
  if (const BlocksOption* o = blocks_option(key)) {
    if (value < 0 || value > o->bound) return fail(EFA_ERR_INVALID, "%s must be in [0,%ld]", o->key, o->bound);
    c->*(o->member) = value;
  } else if (!strcmp(key, "obs_batch")) {
    if (value < 1 || value > efa::kMaxBatch) return fail(EFA_ERR_INVALID, "obs_batch must be in [1,%d]", efa::kMaxBatch);
    c->obs_batch = value;
  } else if (!strcmp(key, "path")) {
    if (value < EFA_PATH_AUTO || value > EFA_PATH_TRANSFORM) return fail(EFA_ERR_INVALID, "path must be 0,1,2");
    c->path = value;
  } else if (!strcmp(key, "timing")) {
    if (value < 0 || value > 2) return fail(EFA_ERR_INVALID, "timing must be 0, 1 or 2");
    harvest_obs_ms(c);
    harvest_state_ms(c);
    c->timing = value;
    c->state_ms_sum = c->obs_ms_sum = 0.0;
    c->state_launches_sum = 0;
  } else if (!strcmp(key, "gram")) {
    if (value < 0 || value > 2) return fail(EFA_ERR_INVALID, "gram must be 0, 1 or 2");
    c->use_gram = value;
  } else if (!strcmp(key, "pipeline")) {
    c->use_pipeline = value ? 1 : 0;
  } else if (!strcmp(key, "obs_solver")) {
    if (value < 0 || value > 1) return fail(EFA_ERR_INVALID, "obs_solver must be 0 (serial) or 1 (batch)");
    c->obs_solver = value;
  } else if (!strcmp(key, "gc_onepass")) {
    c->gc_onepass = value ? 1 : 0;
  } else if (!strcmp(key, "geometry_reuse")) {
    c->geometry_reuse = value ? 1 : 0;
  } else if (!strcmp(key, "own_stream")) {
    EFA_TRY(change_stream(c, c->own_stream));  // back to the context's private non-blocking stream
  } else if (!strcmp(key, "pipe_debug")) {
    c->pipe_debug = value;
  } else if (!strcmp(key, "spin_limit")) {
    if (value < 1) return fail(EFA_ERR_INVALID, "spin_limit must be positive");
    c->spin_limit = value;
  } else if (!strcmp(key, "spin_ms")) {
    c->spin_ms = value;
  } else if (!strcmp(key, "debug_occupy_blocks")) {
    c->dbg_occupy_blocks = value;
  } else if (!strcmp(key, "debug_occupy_ms")) {
    // diagnostic: on a stream of its own, debug_occupy_blocks workgroups hold 120 KB of LDS each (one per CU, and no
    // persistent Phase-A workgroup fits beside one) for `value` ms; value 0 waits for them to finish
    if (!c->dbg_stream) {
      // On a stream of the highest priority: the runtime keeps the hardware queues of each priority apart, so the occupier never
      // lands in the queue the context's own (default-priority) stream was given -- which, with few hardware queues and many
      // streams created in the process before, it otherwise can, and then it runs in front of Phase A instead of beside it.
      int least = 0, greatest = 0;
      EFA_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
      EFA_HIP(hipStreamCreateWithPriority(&c->dbg_stream.h, hipStreamNonBlocking, greatest));
    }
    if (value > 0) EFA_HIP(efa::launch_occupy((int)c->dbg_occupy_blocks, 120 * 1024, (double)value, c->dbg_stream));
    else EFA_HIP(hipStreamSynchronize(c->dbg_stream));
  } else if (!strcmp(key, "nbr_ws_bytes")) {
    // a lower cap of the records efa_neighbourhood_dev holds at a time (0: EFA_NBR_WS_BYTES); the results do not depend on it
    if (value < 0 || value > EFA_NBR_WS_BYTES) return fail(EFA_ERR_INVALID, "nbr_ws_bytes must be in [0,%ld]", (long)EFA_NBR_WS_BYTES);
    c->nbr_ws_bytes = value;
  } else if (!strcmp(key, "pm_ws_bytes")) {
    // a lower cap of the pooled buffers efa_pm_mean_dev holds at a time (0: EFA_PM_WS_BYTES); the results do not depend on it
    if (value < 0 || value > EFA_PM_WS_BYTES) return fail(EFA_ERR_INVALID, "pm_ws_bytes must be in [0,%ld]", (long)EFA_PM_WS_BYTES);
    c->pm_ws_bytes = value;
  } else if (!strcmp(key, "threads_hint")) {
  } else {
    return fail(EFA_ERR_INVALID, "unknown option '%s'", key);
  }
  return EFA_OK;
}

int efa_ctx_set_relaxation(efa_ctx* c, int kind, double alpha) {
  EFA_TRY(use(c));
  if (kind != EFA_RELAX_NONE && kind != EFA_RELAX_RTPP && kind != EFA_RELAX_RTPS)
    return fail(EFA_ERR_INVALID, "relaxation kind %d: expected EFA_RELAX_NONE (0), EFA_RELAX_RTPP (1) or EFA_RELAX_RTPS (2)", kind);
  if (kind != EFA_RELAX_NONE) {
    if (!std::isfinite(alpha)) return fail(EFA_ERR_INVALID, "relaxation factor must be a finite number");
    if (alpha < 0.0) return fail(EFA_ERR_INVALID, "relaxation factor %g must be >= 0", alpha);
    if (kind == EFA_RELAX_RTPP && alpha > 1.0) return fail(EFA_ERR_INVALID, "RTPP factor %g must be <= 1", alpha);
  }
  c->relax_kind = kind;
  c->relax_alpha = kind == EFA_RELAX_NONE ? 0.0 : alpha;
  return EFA_OK;
}

int efa_ctx_set_adaptive_inflation(efa_ctx* c, double* field_dev, long rows, double lower, double upper, double sd_lower) {
  EFA_TRY(use(c));
  if (!field_dev) {
    c->ai_field = nullptr;
    c->ai_rows = 0;
    return EFA_OK;
  }
  if (rows < 0) return fail(EFA_ERR_INVALID, "adaptive inflation: negative row count");
  if ((reinterpret_cast<uintptr_t>(field_dev) & 7u) != 0) return fail(EFA_ERR_INVALID, "adaptive inflation: field must be 8-byte aligned");
  if (!std::isfinite(lower) || !(lower > 0.0)) return fail(EFA_ERR_INVALID, "adaptive inflation: lower bound %g must be finite and > 0", lower);
  if (!std::isfinite(upper) || upper < lower)
    return fail(EFA_ERR_INVALID, "adaptive inflation: upper bound %g must be finite and >= the lower bound %g", upper, lower);
  if (!std::isfinite(sd_lower) || sd_lower < 0.0)
    return fail(EFA_ERR_INVALID, "adaptive inflation: sd lower bound %g must be finite and >= 0", sd_lower);
  c->ai_field = field_dev;
  c->ai_rows = rows;
  c->ai_lower = lower;
  c->ai_upper = upper;
  c->ai_sd_lower = sd_lower;
  return EFA_OK;
}

int efa_ctx_set_letkf_inflation(efa_ctx* c, double* field_dev, long nsolve, const double* ob_infl_dev, long P, double sigma_b,
                                double lower, double upper, double* infl_stats_dev) {
  EFA_TRY(use(c));
  if (!field_dev) {
    c->li_field = nullptr;
    c->li_ob = nullptr;
    c->li_stats = nullptr;
    c->li_nsolve = c->li_P = 0;
    return EFA_OK;
  }
  if (nsolve < 0 || P < 0) return fail(EFA_ERR_INVALID, "LETKF inflation: negative count (nsolve=%ld, P=%ld)", nsolve, P);
  if (((reinterpret_cast<uintptr_t>(field_dev) | reinterpret_cast<uintptr_t>(ob_infl_dev) | reinterpret_cast<uintptr_t>(infl_stats_dev)) & 7u) != 0)
    return fail(EFA_ERR_INVALID, "LETKF inflation: the arrays must be 8-byte aligned");
  if (!std::isfinite(sigma_b) || sigma_b < 0.0) return fail(EFA_ERR_INVALID, "LETKF inflation: sigma_b %g must be finite and >= 0", sigma_b);
  if (!std::isfinite(lower) || !(lower > 0.0)) return fail(EFA_ERR_INVALID, "LETKF inflation: lower bound %g must be finite and > 0", lower);
  if (!std::isfinite(upper) || upper < lower)
    return fail(EFA_ERR_INVALID, "LETKF inflation: upper bound %g must be finite and >= the lower bound %g", upper, lower);
  c->li_field = field_dev;
  c->li_nsolve = nsolve;
  c->li_ob = ob_infl_dev;
  c->li_P = P;
  c->li_sigma_b = sigma_b;
  c->li_lower = lower;
  c->li_upper = upper;
  c->li_stats = infl_stats_dev;
  return EFA_OK;
}

int efa_ctx_set_letkf_control(efa_ctx* c, const double* xc_dev, double* xc_post_dev, long rows, const double* yc_dev, double* yc_post_dev,
                              long P) {
  EFA_TRY(use(c));
  if (!xc_dev) {
    c->lc_xc = c->lc_yc = nullptr;
    c->lc_xc_post = c->lc_yc_post = nullptr;
    c->lc_rows = c->lc_P = 0;
    return EFA_OK;
  }
  if (rows < 0 || P < 0) return fail(EFA_ERR_INVALID, "LETKF control: negative count (rows=%ld, P=%ld)", rows, P);
  if (!xc_post_dev || (P > 0 && (!yc_dev || !yc_post_dev))) return fail(EFA_ERR_INVALID, "LETKF control: null array");
  const uintptr_t x0 = reinterpret_cast<uintptr_t>(xc_dev), x1 = reinterpret_cast<uintptr_t>(xc_post_dev);
  const uintptr_t y0 = reinterpret_cast<uintptr_t>(yc_dev), y1 = reinterpret_cast<uintptr_t>(yc_post_dev);
  if (((x0 | x1 | y0 | y1) & 7u) != 0) return fail(EFA_ERR_INVALID, "LETKF control: the arrays must be 8-byte aligned");
  const auto overlap = [](uintptr_t a, uintptr_t b, long n) {
    const uintptr_t nb = (uintptr_t)n * sizeof(double);
    return a < b + nb && b < a + nb;
  };
  if (x0 != x1 && overlap(x0, x1, rows))
    return fail(EFA_ERR_INVALID, "LETKF control: xc_post_dev overlaps xc_dev without coinciding with it (in place means the same address: "
                "a row's control value is read and written by the wave that owns the row)");
  if (overlap(y0, y1, P)) return fail(EFA_ERR_INVALID, "LETKF control: yc_post_dev overlaps yc_dev");
  c->lc_xc = xc_dev;
  c->lc_xc_post = xc_post_dev;
  c->lc_rows = rows;
  c->lc_yc = yc_dev;
  c->lc_yc_post = yc_post_dev;
  c->lc_P = P;
  return EFA_OK;
}

int efa_ctx_set_letkf_obs_cap(efa_ctx* c, const int* ob_class, long P, const long* cap, int nclass, double* reach_dev, long nsolve) {
  EFA_TRY(use(c));
  if (!cap) {
    c->oc_on = c->oc_has_class = false;
    c->oc_nclass = 0;
    c->oc_P = c->oc_nsolve = 0;
    c->oc_reach = nullptr;
    return EFA_OK;
  }
  if (nclass < 1 || nclass > 32) return fail(EFA_ERR_INVALID, "LETKF obs cap: nclass=%d must be within 1..32", nclass);
  if (P < 0 || nsolve < 0) return fail(EFA_ERR_INVALID, "LETKF obs cap: negative count (P=%ld, nsolve=%ld)", P, nsolve);
  for (int k = 0; k < nclass; ++k)
    if (cap[k] < 0) return fail(EFA_ERR_INVALID, "LETKF obs cap: the cap of class %d is %ld (must be >= 0, 0 meaning no limit)", k, cap[k]);
  if (ob_class)
    for (long k = 0; k < P; ++k)
      if (ob_class[k] < 0 || ob_class[k] >= nclass)
        return fail(EFA_ERR_INVALID, "LETKF obs cap: observation %ld has class %d, outside 0..%d", k, ob_class[k], nclass - 1);
  if ((reinterpret_cast<uintptr_t>(reach_dev) & 7u) != 0) return fail(EFA_ERR_INVALID, "LETKF obs cap: reach_dev must be 8-byte aligned");
  if (ob_class && P > 0) {
    EFA_TRY(h2d(c, c->oc_class, ob_class, (size_t)P * sizeof(int)));
    EFA_HIP(hipStreamSynchronize(c->stream));  // (the caller may reuse its array on return)
  }
  c->oc_on = true;
  c->oc_has_class = ob_class != nullptr && P > 0;
  c->oc_nclass = nclass;
  for (int k = 0; k < 32; ++k) c->oc_cap[k] = k < nclass ? (int)(cap[k] > 0x7FFFFFFFL ? 0x7FFFFFFFL : cap[k]) : 0;
  c->oc_P = P;
  c->oc_reach = reach_dev;
  c->oc_nsolve = reach_dev ? nsolve : 0;
  return EFA_OK;
}

int efa_ctx_set_letkf_cross_validation(efa_ctx* c, const int* group_of_member, int M, int ngroups, double* cv_stats_dev, long nsolve) {
  EFA_TRY(use(c));
  if (!group_of_member) {
    c->cv_on = false;
    c->cv_M = c->cv_ngroups = 0;
    c->cv_stats = nullptr;
    c->cv_nsolve = 0;
    return EFA_OK;
  }
  if (M < 4 || M > efa::kLetkfMaxM)
    return fail(EFA_ERR_INVALID, "LETKF cross validation: M=%d must be within 4..%d (two groups of two members at least; the LETKF's range)", M,
                efa::kLetkfMaxM);
  if (ngroups < 2) return fail(EFA_ERR_INVALID, "LETKF cross validation: ngroups=%d must be >= 2", ngroups);
  if (nsolve < 0) return fail(EFA_ERR_INVALID, "LETKF cross validation: negative count (nsolve=%ld)", nsolve);
  std::vector<int> size((size_t)ngroups, 0);
  for (int m = 0; m < M; ++m) {
    if (group_of_member[m] < 0 || group_of_member[m] >= ngroups)
      return fail(EFA_ERR_INVALID, "LETKF cross validation: member %d has the label %d, outside 0..%d", m, group_of_member[m], ngroups - 1);
    size[group_of_member[m]]++;
  }
  for (int k = 0; k < ngroups; ++k) {
    if (size[k] == 0) return fail(EFA_ERR_INVALID, "LETKF cross validation: the label %d is unused (every label 0..%d must be)", k, ngroups - 1);
    if (M - size[k] < 2)
      return fail(EFA_ERR_INVALID, "LETKF cross validation: group %d leaves an independent set of %d members (at least 2 are needed)", k,
                  M - size[k]);
  }
  if ((reinterpret_cast<uintptr_t>(cv_stats_dev) & 7u) != 0)
    return fail(EFA_ERR_INVALID, "LETKF cross validation: cv_stats_dev must be 8-byte aligned");
  // per group: the independent members ascending, then its own; and the independent set's size
  std::vector<int> h((size_t)ngroups * M + ngroups);
  for (int k = 0; k < ngroups; ++k) {
    int ni = 0, nh = M - size[k];
    for (int m = 0; m < M; ++m) h[(size_t)k * M + (group_of_member[m] != k ? ni++ : nh++)] = m;
    h[(size_t)ngroups * M + k] = M - size[k];
  }
  EFA_TRY(h2d(c, c->cv_lists, h.data(), h.size() * sizeof(int)));
  EFA_HIP(hipStreamSynchronize(c->stream));  // (h goes out of scope)
  c->cv_on = true;
  c->cv_M = M;
  c->cv_ngroups = ngroups;
  c->cv_stats = cv_stats_dev;
  c->cv_nsolve = cv_stats_dev ? nsolve : 0;
  return EFA_OK;
}

int efa_ctx_set_vertical_localization(efa_ctx* c, long n_lead, const double* lead_vert, long P, const double* ob_vert,
                                      const double* ob_vert_halfwidth) {
  EFA_TRY(use(c));
  if (!lead_vert) {
    if (c->vl_on) c->vl_serial++;
    c->vl_on = false;
    return EFA_OK;
  }
  if (n_lead <= 0) return fail(EFA_ERR_INVALID, "vertical localisation: n_lead=%ld must be > 0", n_lead);
  if (P < 0) return fail(EFA_ERR_INVALID, "vertical localisation: negative observation count");
  if (P > 0 && (!ob_vert || !ob_vert_halfwidth)) return fail(EFA_ERR_INVALID, "vertical localisation: null ob_vert/ob_vert_halfwidth");
  std::vector<double> v((size_t)(n_lead + 2 * P));
  bool any = false;
  for (long i = 0; i < n_lead; ++i) {
    if (std::isinf(lead_vert[i])) return fail(EFA_ERR_INVALID, "vertical localisation: slab %ld has an infinite coordinate", i);
    v[i] = lead_vert[i];
  }
  for (long k = 0; k < P; ++k) {
    const double z = ob_vert[k], h = ob_vert_halfwidth[k];
    if (std::isinf(z)) return fail(EFA_ERR_INVALID, "vertical localisation: observation %ld has an infinite coordinate", k);
    const bool none = std::isnan(z) || std::isnan(h);  // either missing: no vertical taper for this ob
    if (!none && !(std::isfinite(h) && h > 0.0))
      return fail(EFA_ERR_INVALID, "vertical localisation: observation %ld has half-width %g (must be finite and > 0, or NaN)", k, h);
    any = any || !none;
    v[n_lead + k] = none ? std::nan("") : z;
    v[n_lead + P + k] = none ? 1.0 : h;
  }
  if (c->vl_on && c->vl_nlead == n_lead && c->vl_P == P && std::memcmp(c->vl_host.data(), v.data(), v.size() * sizeof(double)) == 0)
    return EFA_OK;  // unchanged: nothing to copy, the geometry cache stays valid
  EFA_TRY(h2d(c, c->vl_dev, v.data(), v.size() * sizeof(double)));
  EFA_HIP(hipStreamSynchronize(c->stream));  // (v is gone on return)
  c->vl_host.swap(v);
  c->vl_nlead = n_lead;
  c->vl_P = P;
  c->vl_on = true;
  c->vl_any = any;
  c->vl_serial++;
  return EFA_OK;
}

int efa_ctx_set_slab_localization(efa_ctx* c, long n_lead, const double* lead_time, const int* lead_var, long n_var, long P,
                                  const double* ob_time, const double* ob_time_halfwidth, const int* ob_group, const int* ob_var,
                                  long n_group, const double* impact) {
  EFA_TRY(use(c));
  if (!lead_time && !impact) {
    if (c->sl_on) c->sl_serial++;
    c->sl_on = false;
    return EFA_OK;
  }
  if (n_lead <= 0) return fail(EFA_ERR_INVALID, "slab localisation: n_lead=%ld must be > 0", n_lead);
  if (P < 0) return fail(EFA_ERR_INVALID, "slab localisation: negative observation count");
  if (lead_time && P > 0 && (!ob_time || !ob_time_halfwidth))
    return fail(EFA_ERR_INVALID, "slab localisation: lead_time without ob_time/ob_time_halfwidth");
  if (impact) {
    if (n_var <= 0 || n_group <= 0) return fail(EFA_ERR_INVALID, "slab localisation: n_var=%ld and n_group=%ld must be > 0", n_var, n_group);
    if (!lead_var || (P > 0 && (!ob_group || !ob_var))) return fail(EFA_ERR_INVALID, "slab localisation: impact without lead_var/ob_group/ob_var");
  }
  const long nv = impact ? n_var : 1, ng = impact ? n_group : 0;
  const size_t nd = (size_t)(n_lead + 2 * P + ng * nv), ni = (size_t)(n_lead + 2 * P);
  std::vector<double> v(nd + (ni + 1) / 2, 0.0);
  std::vector<int> iv(ni, -1);
  const double nan = std::nan("");
  bool any = false;
  for (long i = 0; i < n_lead; ++i) {
    const double t = lead_time ? lead_time[i] : nan;
    if (std::isinf(t)) return fail(EFA_ERR_INVALID, "slab localisation: slab %ld has an infinite time", i);
    v[i] = std::isnan(t) ? nan : t;
  }
  for (long k = 0; k < P; ++k) {
    const double t = lead_time ? ob_time[k] : nan, h = lead_time ? ob_time_halfwidth[k] : nan;
    if (std::isinf(t)) return fail(EFA_ERR_INVALID, "slab localisation: observation %ld has an infinite time", k);
    if (!std::isnan(h) && !(std::isfinite(h) && h > 0.0))
      return fail(EFA_ERR_INVALID, "slab localisation: observation %ld has temporal half-width %g (must be finite and > 0, or NaN)", k, h);
    any = any || (!std::isnan(t) && !std::isnan(h));
    v[n_lead + k] = std::isnan(t) ? nan : t;
    v[n_lead + P + k] = std::isnan(h) ? nan : h;
  }
  if (impact) {
    for (long i = 0; i < ng * nv; ++i) {
      if (!(std::isfinite(impact[i]) && impact[i] >= 0.0 && impact[i] <= 1.0))
        return fail(EFA_ERR_INVALID, "slab localisation: impact[%ld][%ld] = %g is not in [0, 1]", i / nv, i % nv, impact[i]);
      v[n_lead + 2 * P + i] = impact[i];
    }
    for (long i = 0; i < n_lead; ++i) {
      if (lead_var[i] < 0 || lead_var[i] >= nv) return fail(EFA_ERR_INVALID, "slab localisation: slab %ld has variable %d (n_var=%ld)", i, lead_var[i], nv);
      iv[i] = lead_var[i];
    }
    for (long k = 0; k < P; ++k) {
      const int g = ob_group[k], w = ob_var[k];
      if (g < -1 || g >= ng) return fail(EFA_ERR_INVALID, "slab localisation: observation %ld has impact row %d (n_group=%ld)", k, g, ng);
      if (w < -1 || w >= nv) return fail(EFA_ERR_INVALID, "slab localisation: observation %ld has target variable %d (n_var=%ld)", k, w, nv);
      if (g >= 0 && w >= 0 && impact[g * nv + w] != 1.0)  // an ob's taper against itself stays 1 (the per-batch diagnostics, the pivots)
        return fail(EFA_ERR_INVALID, "slab localisation: observation %ld: the impact of its obtype on its own variable is %g, not 1", k,
                    impact[g * nv + w]);
      iv[n_lead + k] = g;
      iv[n_lead + P + k] = w;
      if (g >= 0)
        for (long u = 0; u < nv && !any; ++u) any = impact[g * nv + u] != 1.0;
    }
  }
  if (ni) std::memcpy(v.data() + nd, iv.data(), ni * sizeof(int));
  if (c->sl_on && c->sl_nlead == n_lead && c->sl_P == P && c->sl_nvar == nv && c->sl_ngroup == ng && c->sl_host.size() == v.size() &&
      std::memcmp(c->sl_host.data(), v.data(), v.size() * sizeof(double)) == 0)
    return EFA_OK;  // unchanged: nothing to copy, the geometry cache and the table stay valid
  EFA_TRY(h2d(c, c->sl_dev, v.data(), v.size() * sizeof(double)));
  EFA_HIP(hipStreamSynchronize(c->stream));  // (v is gone on return)
  c->sl_host.swap(v);
  c->sl_nlead = n_lead;
  c->sl_P = P;
  c->sl_nvar = nv;
  c->sl_ngroup = ng;
  c->sl_on = true;
  c->sl_any = any;
  c->sl_serial++;
  return EFA_OK;
}

int efa_slab_factor_table(efa_ctx* c, long P, long n_lead, double* table) {
  EFA_TRY(use(c));
  if (!c->sl_on) return fail(EFA_ERR_INVALID, "efa_slab_factor_table: slab localisation is not set");
  if (P != c->sl_P || n_lead != c->sl_nlead)
    return fail(EFA_ERR_INVALID, "efa_slab_factor_table: set for %ld observations and %ld slabs, asked for %ld and %ld", c->sl_P, c->sl_nlead, P, n_lead);
  if (c->vl_on && (c->vl_P != P || c->vl_nlead != n_lead))
    return fail(EFA_ERR_INVALID, "efa_slab_factor_table: vertical localisation is set for %ld observations and %ld slabs", c->vl_P, c->vl_nlead);
  EFA_TRY(ensure_slab_table(c));
  if (table && P * n_lead > 0)
    EFA_HIP(hipMemcpyAsync(table, c->sl_tab.p, (size_t)(P * n_lead) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  EFA_HIP(hipStreamSynchronize(c->stream));
  return EFA_OK;
}

int efa_ctx_set_sampling_error_correction(efa_ctx* c, const double* alpha, int T) {
  EFA_TRY(use(c));
  if (!alpha || T == 0) {
    c->sec_T = 0;
    return EFA_OK;
  }
  if (T < 2 || T > efa::kSecMaxT)
    return fail(EFA_ERR_INVALID, "sampling error correction: a table of T=%d nodes (2 .. %d are supported)", T, efa::kSecMaxT);
  for (int j = 0; j < T; ++j)
    if (!(std::isfinite(alpha[j]) && alpha[j] >= 0.0))
      return fail(EFA_ERR_INVALID, "sampling error correction: alpha[%d] = %g is not a finite number >= 0", j, alpha[j]);
  if (c->sec_T == T && std::memcmp(c->sec_host.data(), alpha, (size_t)T * sizeof(double)) == 0) return EFA_OK;  // unchanged
  std::vector<double> v(alpha, alpha + T);
  EFA_TRY(h2d(c, c->sec_dev, v.data(), v.size() * sizeof(double)));
  EFA_HIP(hipStreamSynchronize(c->stream));  // (v is gone on return)
  c->sec_host.swap(v);
  c->sec_T = T;
  return EFA_OK;
}

int efa_ctx_set_outlier_threshold(efa_ctx* c, double threshold) {
  EFA_TRY(use(c));
  if (!std::isfinite(threshold) || threshold < 0.0)
    return fail(EFA_ERR_INVALID, "outlier threshold %g must be a finite number >= 0 (0: off)", threshold);
  c->qc_threshold = threshold;
  return EFA_OK;
}

int efa_inflate_rows_dev(efa_ctx* c, long rows, int M, double* X_dev, const double* field_dev) {
  EFA_TRY(use(c));
  if (rows < 0 || M < 1 || M > efa::kMaxMembers) return fail(EFA_ERR_INVALID, "efa_inflate_rows_dev: bad shape rows=%ld M=%d", rows, M);
  if (rows && (!X_dev || !field_dev)) return fail(EFA_ERR_INVALID, "null pointer");
  EFA_HIP(efa::launch_inflate_rows(rows, M, X_dev, field_dev, c->stream));
  return EFA_OK;
}

int efa_ctx_get_option(efa_ctx* c, const char* key, long* value) {
  EFA_TRY(use(c));
  if (!key || !value) return fail(EFA_ERR_INVALID, "null argument");
  if (const BlocksOption* o = blocks_option(key)) *value = c->*(o->member);
  else if (!strcmp(key, "obs_batch")) *value = c->obs_batch;
  else if (!strcmp(key, "path")) *value = c->path;
  else if (!strcmp(key, "timing")) *value = c->timing;
  else if (!strcmp(key, "gram")) *value = c->use_gram;
  else if (!strcmp(key, "pipeline")) *value = c->use_pipeline;
  else if (!strcmp(key, "obs_solver")) *value = c->obs_solver;
  else if (!strcmp(key, "gc_onepass")) *value = c->gc_onepass;
  else if (!strcmp(key, "gc_family")) *value = c->gc_family_used;  // the last one-pass sweep: 0 plain, 1 adaptive, 2 vertical, 3 slab table, 4 SEC
  else if (!strcmp(key, "gc_form")) *value = c->gc_form_used;  // the last one-pass sweep: 1 quad kernel, 2 row-per-lane kernel
  else if (!strcmp(key, "sec_on")) *value = c->sec_T > 0 ? 1 : 0;  // efa_ctx_set_sampling_error_correction
  else if (!strcmp(key, "geometry_reuse")) *value = c->geometry_reuse;
  else if (!strcmp(key, "gc_active_pairs")) {
    EFA_TRY(read_gc_pairs(c));
    *value = c->gc_active_pairs;
  }
  else if (!strcmp(key, "spin_limit")) *value = c->spin_limit;
  else if (!strcmp(key, "spin_ms")) *value = c->spin_ms;
  else if (!strcmp(key, "cu_count")) *value = c->cu_count;
  else if (!strcmp(key, "phase_a_kind")) *value = c->phase_a_kind;
  else if (!strcmp(key, "pipe_dbg_addr")) *value = (long)reinterpret_cast<uintptr_t>(c->dbg.p);
  else if (!strcmp(key, "traj_addr")) *value = (long)reinterpret_cast<uintptr_t>(c->traj.p);  // (diagnostic tools only)
  else if (!strcmp(key, "device")) *value = c->device;
  else if (!strcmp(key, "f32_native")) *value = c->f32_native;  // the last efa_state_cycle_f32_dev / chunk of efa_ensrf_cycle_host_f32
  else if (!strcmp(key, "stream_chunks")) *value = c->st.chunks;  // the last efa_ensrf_cycle_host (efa_stream.hip)
  else if (!strcmp(key, "stream_peak_bytes")) *value = c->st.peak_bytes;
  else if (!strcmp(key, "stream_h2d_us")) *value = c->st.h2d_us;
  else if (!strcmp(key, "stream_d2h_us")) *value = c->st.d2h_us;
  else if (!strcmp(key, "stream_wall_us")) *value = c->st.wall_us;
  else if (!strcmp(key, "impact_us")) *value = c->impact_us;  // the last efa_obs_impact_dev (efa_impact.hip)
  else if (!strcmp(key, "sens_us")) *value = c->sens_us;  // the last efa_sensitivity_dev (efa_sensitivity.hip)
  else if (!strcmp(key, "verify_us")) *value = c->verify_us;  // the last efa_verify_dev (efa_verify.hip)
  else if (!strcmp(key, "products_us")) *value = c->products_us;  // the last efa_products_dev (efa_products.hip)
  else if (!strcmp(key, "gram_us")) *value = c->gram_us;  // the last efa_gram_dev (efa_gram.hip)
  else if (!strcmp(key, "neighbourhood_us")) *value = c->neighbourhood_us;  // the last efa_neighbourhood_dev (efa_neighbourhood.hip)
  else if (!strcmp(key, "nbr_ws_bytes")) *value = c->nbr_ws_bytes;
  else if (!strcmp(key, "pm_us")) *value = c->pm_us;  // the last efa_pm_mean_dev (efa_pmmean.hip)
  else if (!strcmp(key, "pm_passes")) *value = c->pm_passes;
  else if (!strcmp(key, "pm_rank_passes")) *value = c->pm_rank_passes;
  else if (!strcmp(key, "pm_ws_bytes")) *value = c->pm_ws_bytes;
  else return fail(EFA_ERR_INVALID, "unknown option '%s'", key);
  return EFA_OK;
}

int efa_ctx_synchronize(efa_ctx* c) {
  EFA_TRY(use(c));
  EFA_HIP(hipStreamSynchronize(c->stream));
  return EFA_OK;
}

int efa_malloc(efa_ctx* c, size_t bytes, void** dev_out) {
  EFA_TRY(use(c));
  if (!dev_out) return fail(EFA_ERR_INVALID, "null out pointer");
  *dev_out = nullptr;
  EFA_HIP(hipMalloc(dev_out, bytes ? bytes : 8));
  return EFA_OK;
}

int efa_free(efa_ctx* c, void* dev) {
  EFA_TRY(use(c));
  if (dev) EFA_HIP(hipFree(dev));
  return EFA_OK;
}

int efa_memcpy_h2d(efa_ctx* c, void* dst_dev, const void* src, size_t bytes) {
  EFA_TRY(use(c));
  if (bytes) {
    EFA_HIP(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, c->stream));
    EFA_HIP(hipStreamSynchronize(c->stream));
  }
  return EFA_OK;
}

int efa_memcpy_d2h(efa_ctx* c, void* dst, const void* src_dev, size_t bytes) {
  EFA_TRY(use(c));
  if (bytes) {
    EFA_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    EFA_HIP(hipStreamSynchronize(c->stream));
  }
  return EFA_OK;
}

int efa_memcpy_d2d(efa_ctx* c, void* dst_dev, const void* src_dev, size_t bytes) {
  EFA_TRY(use(c));
  if (bytes) EFA_HIP(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, c->stream));
  return EFA_OK;
}

int efa_form_perts_dev(efa_ctx* c, long rows, int M, const double* X_dev, double scale, double* xm_dev,
                       double* Xp_dev) {
  EFA_TRY(use(c));
  return form_perts(c, rows, M, X_dev, scale, xm_dev, Xp_dev);
}

int efa_posterior_dev(efa_ctx* c, long rows, int M, const double* xm_dev, const double* Xp_dev, double* post_dev) {
  EFA_TRY(use(c));
  if (rows < 0 || M < 1) return fail(EFA_ERR_INVALID, "bad shape rows=%ld M=%d", rows, M);
  if (rows && (!xm_dev || !Xp_dev || !post_dev)) return fail(EFA_ERR_INVALID, "null pointer");
  EFA_HIP(efa::launch_posterior(rows, M, xm_dev, Xp_dev, post_dev, c->stream));
  return EFA_OK;
}

int efa_forward_stencil_dev(efa_ctx* c, long rows, long row_offset, int M, const double* X_dev, long P, int npt,
                            const int64_t* idx, const double* wts, double* HX_dev) {
  EFA_TRY(use(c));
  if (rows < 0 || M < 1 || P < 0 || npt < 1) return fail(EFA_ERR_INVALID, "bad shape");
  if (P == 0) return EFA_OK;
  if (!X_dev || !idx || !wts || !HX_dev) return fail(EFA_ERR_INVALID, "null pointer");
  // staging of the stencil in grow-only context buffers (a hipMalloc/hipFree pair per call costs more than the kernel)
  // The caller's arrays are copied into pinned memory (free to be reused on return) and go to the device as ONE
  // asynchronous copy: no stream synchronisation here.  The pinned image is reused by the next call, which first waits
  // for this copy's event (long complete by then).
  const size_t n = (size_t)P * npt;
  const size_t half = (n * sizeof(int64_t) + 255) & ~(size_t)255;
  EFA_TRY(c->fs_idx.reserve(2 * half));
  EFA_TRY(c->pin_fs.reserve(2 * half));
  if (!c->ev_fs) EFA_HIP(hipEventCreateWithFlags(&c->ev_fs.h, hipEventDisableTiming));
  else EFA_HIP(hipEventSynchronize(c->ev_fs));
  // A fixed observing network hands over the same stencil cycle after cycle: when the pinned image still holds exactly these
  // indices and weights, the device copy made from it is current and nothing is copied (the copy itself is 8 us at 1e4 obs, but
  // a copy between two kernels idles the stream for ~10 us on either side).
  char* pin = static_cast<char*>(c->pin_fs.p);
  const bool same = c->fs_valid_n == n && c->fs_valid_dev == c->fs_idx.p && c->fs_valid_pin == c->pin_fs.p && std::memcmp(pin, idx, n * sizeof(int64_t)) == 0 &&
                    std::memcmp(pin + half, wts, n * sizeof(double)) == 0;
  if (!same) {
    std::memcpy(pin, idx, n * sizeof(int64_t));
    std::memcpy(pin + half, wts, n * sizeof(double));
    EFA_HIP(hipMemcpyAsync(c->fs_idx.p, c->pin_fs.p, half + n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    EFA_HIP(hipEventRecord(c->ev_fs, c->stream));
    c->fs_valid_n = n;
    c->fs_valid_dev = c->fs_idx.p;
    c->fs_valid_pin = c->pin_fs.p;
  }
  EFA_HIP(efa::launch_forward_stencil(rows, row_offset, M, X_dev, P, npt, c->fs_idx.as<int64_t>(),
                                      reinterpret_cast<const double*>(static_cast<const char*>(c->fs_idx.p) + half), HX_dev,
                                      c->stream));
  return EFA_OK;
}

int efa_interp_stencils(efa_ctx* c, int nvar, int nt, int ny, int nx, int latlon_1d, long n_grid, const double* grid_lat,
                        const double* grid_lon, const double* valid_times, long P, const int32_t* ob_var,
                        const double* ob_time, const double* ob_lat, const double* ob_lon, int64_t* sten_idx,
                        double* sten_wts, uint8_t* ob_status) {
  EFA_TRY(use(c));
  c->f_P = 0;
  if (nvar < 1 || nt < 1 || ny < 1 || nx < 1 || n_grid < 1 || P < 0)
    return fail(EFA_ERR_INVALID, "efa_interp_stencils: bad shape nvar=%d nt=%d ny=%d nx=%d n_grid=%ld P=%ld", nvar, nt, ny, nx, n_grid, P);
  if (!latlon_1d && n_grid != (long)ny * nx)
    return fail(EFA_ERR_INVALID, "efa_interp_stencils: 2-D lat/lon need n_grid = ny*nx = %ld, got %ld", (long)ny * nx, n_grid);
  if (P == 0) return EFA_OK;
  if (!grid_lat || !grid_lon || !valid_times || !ob_var || !ob_time || !ob_lat || !ob_lon)
    return fail(EFA_ERR_INVALID, "efa_interp_stencils: null input array");
  for (int i = 1; i < nt; ++i)
    if (!(valid_times[i] > valid_times[i - 1])) return fail(EFA_ERR_INVALID, "efa_interp_stencils: valid_times must ascend");
  const size_t dG = (size_t)n_grid * sizeof(double), dP = (size_t)P * sizeof(double);
  EFA_TRY(h2d(c, c->f_glat, grid_lat, dG));
  EFA_TRY(h2d(c, c->f_glon, grid_lon, dG));
  EFA_TRY(h2d(c, c->f_valids, valid_times, (size_t)nt * sizeof(double)));
  EFA_TRY(h2d(c, c->f_var, ob_var, (size_t)P * sizeof(int32_t)));
  EFA_TRY(h2d(c, c->f_time, ob_time, dP));
  EFA_TRY(h2d(c, c->f_lat, ob_lat, dP));
  EFA_TRY(h2d(c, c->f_lon, ob_lon, dP));
  EFA_TRY(c->f_sl.reserve(dG));
  EFA_TRY(c->f_cl.reserve(dG));
  EFA_TRY(c->f_near.reserve((size_t)P * 4 * sizeof(long)));
  EFA_TRY(c->f_idx.reserve((size_t)P * 8 * sizeof(long)));
  EFA_TRY(c->f_wts.reserve((size_t)P * 8 * sizeof(double)));
  EFA_TRY(c->f_status.reserve((size_t)P));
  efa::InterpArgs a{};
  a.P = P;
  a.nvar = nvar;
  a.nt = nt;
  a.ny = ny;
  a.nx = nx;
  a.latlon_1d = latlon_1d ? 1 : 0;
  a.n_grid = n_grid;
  a.glat = c->f_glat.as<double>();
  a.glon = c->f_glon.as<double>();
  a.sl = c->f_sl.as<double>();
  a.cl = c->f_cl.as<double>();
  a.valids = c->f_valids.as<double>();
  a.ob_var = c->f_var.as<int>();
  a.ob_time = c->f_time.as<double>();
  a.ob_lat = c->f_lat.as<double>();
  a.ob_lon = c->f_lon.as<double>();
  a.nearest = c->f_near.as<long>();
  a.sten_idx = c->f_idx.as<long>();
  a.sten_wts = c->f_wts.as<double>();
  a.status = c->f_status.as<unsigned char>();
  hipStream_t s = c->stream;
  EFA_HIP(efa::launch_interp_stencils(a, s));
  if (sten_idx) EFA_HIP(hipMemcpyAsync(sten_idx, c->f_idx.p, (size_t)P * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  if (sten_wts) EFA_HIP(hipMemcpyAsync(sten_wts, c->f_wts.p, (size_t)P * 8 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (ob_status) EFA_HIP(hipMemcpyAsync(ob_status, c->f_status.p, (size_t)P, hipMemcpyDeviceToHost, s));
  EFA_HIP(hipStreamSynchronize(s));  // the caller may reuse its input arrays on return
  c->f_P = P;
  return EFA_OK;
}

int efa_forward_interp_dev(efa_ctx* c, long ncol, long col_lo, long col_hi, long n_lead, int M, const double* X_dev,
                           double* HX_dev) {
  EFA_TRY(use(c));
  if (c->f_P <= 0) return fail(EFA_ERR_INVALID, "efa_forward_interp_dev called before efa_interp_stencils");
  if (ncol < 1 || col_lo < 0 || col_hi > ncol || col_lo > col_hi || n_lead < 1 || M < 1)
    return fail(EFA_ERR_INVALID, "efa_forward_interp_dev: bad shard [%ld,%ld) of %ld columns, n_lead=%ld, M=%d", col_lo, col_hi, ncol, n_lead, M);
  if (!X_dev || !HX_dev) return fail(EFA_ERR_INVALID, "null pointer");
  EFA_HIP(efa::launch_forward_cols(ncol, col_lo, col_hi, n_lead, M, X_dev, c->f_P, 8, c->f_idx.as<long>(), c->f_wts.as<double>(),
                                   HX_dev, c->stream));
  return EFA_OK;
}

int efa_obs_phase_dev(efa_ctx* c, int M, long P, double* ym_dev, double* Yp_dev, const double* ob_value,
                      const double* ob_error, const uint8_t* ob_assim, int loc_mode, const double* ob_lat,
                      const double* ob_lon, const double* ob_halfwidth_km, double* prior_mean, double* prior_var,
                      double* post_mean, double* post_var, uint8_t* assimilated) {
  EFA_TRY(use(c));
  return obs_phase(c, M, P, ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon, ob_halfwidth_km),
                   diag_out(prior_mean, prior_var, post_mean, post_var, assimilated));
}

int efa_state_phase_dev(efa_ctx* c, long rows, int M, const double* xm_in_dev, const double* Xp_in_dev,
                        double* xm_out_dev, double* Xp_out_dev, const double* grid_lat, const double* grid_lon,
                        long ncol, long n_lead) {
  EFA_TRY(use(c));
  return state_phase(c, rows, M, xm_in_dev, Xp_in_dev, xm_out_dev, Xp_out_dev, grid_lat, grid_lon, ncol, n_lead);
}

int efa_state_cycle_dev(efa_ctx* c, long rows, int M, const double* X_dev, double* post_dev, const double* grid_lat,
                        const double* grid_lon, long ncol, long n_lead) {
  EFA_TRY(use(c));
  return state_cycle(c, StateRows{X_dev, post_dev, Elem::f64, rows, M}, grid_lat, grid_lon, ncol, n_lead);
}

int efa_state_cycle_f32_dev(efa_ctx* c, long rows, int M, const float* X_dev, float* post_dev, const double* grid_lat,
                            const double* grid_lon, long ncol, long n_lead) {
  EFA_TRY(use(c));
  return state_cycle(c, StateRows{X_dev, post_dev, Elem::f32, rows, M}, grid_lat, grid_lon, ncol, n_lead);
}

int efa_ensrf_update_dev(efa_ctx* c, long rows, int M, long P, double* xm_dev, double* Xp_dev, double* ym_dev,
                         double* Yp_dev, const double* ob_value, const double* ob_error, const uint8_t* ob_assim,
                         int loc_mode, const double* ob_lat, const double* ob_lon, const double* ob_halfwidth_km,
                         const double* grid_lat, const double* grid_lon, long ncol, long n_lead, double* prior_mean,
                         double* prior_var, double* post_mean, double* post_var, uint8_t* assimilated) {
  EFA_TRY(use(c));
  EFA_TRY(check_cycle_settings(c, loc_mode, rows, P, n_lead));
  EFA_TRY(obs_phase(c, M, P, ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon, ob_halfwidth_km),
                    diag_out(prior_mean, prior_var, post_mean, post_var, assimilated)));
  EFA_TRY(state_phase(c, rows, M, xm_dev, Xp_dev, xm_dev, Xp_dev, grid_lat, grid_lon, ncol, n_lead));
  EFA_HIP(hipStreamSynchronize(c->stream));
  return EFA_OK;
}

int efa_ensrf_cycle_dev(efa_ctx* c, long rows, int M, long P, const double* X_dev, double* post_dev, double* ym_dev,
                        double* Yp_dev, int obs_block_out, const double* ob_value, const double* ob_error,
                        const uint8_t* ob_assim, int loc_mode, const double* ob_lat, const double* ob_lon,
                        const double* ob_halfwidth_km, const double* grid_lat, const double* grid_lon, long ncol, long n_lead,
                        double* prior_mean, double* prior_var, double* post_mean, double* post_var, uint8_t* assimilated) {
  EFA_TRY(use(c));
  if (rows < 0) return fail(EFA_ERR_INVALID, "negative row count");
  if (rows > 0 && (!X_dev || !post_dev)) return fail(EFA_ERR_INVALID, "null state pointer");
  EFA_TRY(check_cycle_settings(c, loc_mode, rows, P, n_lead));
  // Phase B may go into the stream before Phase A's status is known only if a wrong guess cannot cost the prior:
  // separate prior and posterior buffers (a redone Phase A needs the transform run again on the untouched prior)
  const StateRows r{X_dev, post_dev, Elem::f64, rows, M};
  const SpecRequest spec{X_dev, post_dev, (r.disjoint() && loc_mode == EFA_LOC_NONE) ? rows : 0, obs_block_out != 0};
  // the grid ahead of Phase A, while the device is still busy with the previous cycle
  StateCall sc;
  sc.grid_current = loc_mode == EFA_LOC_GC && rows > 0;
  if (sc.grid_current) {
    EFA_TRY(check_grid(loc_mode, grid_lat, grid_lon, ncol, n_lead, rows));
    EFA_TRY(c->grid.refresh(c->stream, grid_lat, grid_lon, ncol));
  }
  SpecResult done;
  EFA_TRY(obs_phase(c, M, P, ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon, ob_halfwidth_km),
                    diag_out(prior_mean, prior_var, post_mean, post_var, assimilated), spec, &done));
  // Phase B is in the stream already, behind the launch that turned out fine -- unless the outlier check rejected so many obs
  // that the state phase would not take the transform (none left, or "auto" with fewer): then it runs as it would have, over the
  // speculative posterior (the prior is untouched)
  const StatePlan plan = plan_state(c, true, r.elem, false, c->have_transform);
  if (done.launched && plan.route == Route::transform) {
    c->state_ms = 0.0;
    report_state_call(c, plan, r.elem, done.launches);
    return end_state_call(c, *done.interval, true, true);
  }
  return state_cycle(c, r, grid_lat, grid_lon, ncol, n_lead, sc);
}

int efa_ensrf_update(efa_ctx* c, long A, long N, int M, long P, double* xbm, double* Xbp, const double* ob_value,
                     const double* ob_error, const uint8_t* ob_assim, int loc_mode, const double* ob_lat,
                     const double* ob_lon, const double* ob_halfwidth_km, const double* grid_lat,
                     const double* grid_lon, long ncol, long n_lead, double* prior_mean, double* prior_var,
                     double* post_mean, double* post_var, uint8_t* assimilated) {
  EFA_TRY(use(c));
  if (N < 0 || P < 0 || A != N + P) return fail(EFA_ERR_INVALID, "A=%ld must equal N+P=%ld+%ld", A, N, P);
  EFA_TRY(check_common(M, P));
  if (A && (!xbm || !Xbp)) return fail(EFA_ERR_INVALID, "null xbm/Xbp");
  EFA_TRY(check_batch_solver(c, loc_mode));  // (before the first copy)
  EFA_TRY(check_batch_obs(c, P, ob_error, ob_assim));
  const size_t rowb = (size_t)M * sizeof(double);
  EFA_TRY(c->h_xm.reserve((size_t)(N ? N : 1) * sizeof(double)));
  EFA_TRY(c->h_Xp.reserve((size_t)(N ? N : 1) * rowb));
  EFA_TRY(c->h_ym.reserve((size_t)(P ? P : 1) * sizeof(double)));
  EFA_TRY(c->h_Yp.reserve((size_t)(P ? P : 1) * rowb));
  hipStream_t s = c->stream;
  if (N) {
    EFA_HIP(hipMemcpyAsync(c->h_xm.p, xbm, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemcpyAsync(c->h_Xp.p, Xbp, (size_t)N * rowb, hipMemcpyHostToDevice, s));
  }
  if (P) {
    EFA_HIP(hipMemcpyAsync(c->h_ym.p, xbm + N, (size_t)P * sizeof(double), hipMemcpyHostToDevice, s));
    EFA_HIP(hipMemcpyAsync(c->h_Yp.p, Xbp + (size_t)N * M, (size_t)P * rowb, hipMemcpyHostToDevice, s));
  }
  EFA_TRY(efa_ensrf_update_dev(c, N, M, P, c->h_xm.as<double>(), c->h_Xp.as<double>(), c->h_ym.as<double>(),
                               c->h_Yp.as<double>(), ob_value, ob_error, ob_assim, loc_mode, ob_lat, ob_lon,
                               ob_halfwidth_km, grid_lat, grid_lon, ncol, n_lead, prior_mean, prior_var, post_mean,
                               post_var, assimilated));
  if (N) {
    EFA_HIP(hipMemcpyAsync(xbm, c->h_xm.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
    EFA_HIP(hipMemcpyAsync(Xbp, c->h_Xp.p, (size_t)N * rowb, hipMemcpyDeviceToHost, s));
  }
  if (P) {
    EFA_HIP(hipMemcpyAsync(xbm + N, c->h_ym.p, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, s));
    EFA_HIP(hipMemcpyAsync(Xbp + (size_t)N * M, c->h_Yp.p, (size_t)P * rowb, hipMemcpyDeviceToHost, s));
  }
  EFA_HIP(hipStreamSynchronize(s));
  return EFA_OK;
}

int efa_cov_contract_f32_dev(efa_ctx* c, long N, int M, long P, const float* Xbp_f32_dev, const float* Ye_f32_dev,
                             float* C_f32_dev) {
  EFA_TRY(use(c));
  if (N < 0 || P < 0 || M < 4 || (M & 3) != 0)
    return fail(EFA_ERR_INVALID, "efa_cov_contract_f32_dev: need N,P >= 0 and M a positive multiple of 4 (M=%d)", M);
  if (N == 0 || P == 0) return EFA_OK;
  if (!Xbp_f32_dev || !Ye_f32_dev || !C_f32_dev) return fail(EFA_ERR_INVALID, "null pointer");
  if ((reinterpret_cast<uintptr_t>(Xbp_f32_dev) & 15u) || (reinterpret_cast<uintptr_t>(Ye_f32_dev) & 15u))
    return fail(EFA_ERR_INVALID, "operands must be 16-byte aligned");
  EFA_HIP(efa::launch_contract_f32(N, M, P, Xbp_f32_dev, Ye_f32_dev, C_f32_dev, c->stream));
  return EFA_OK;
}

int efa_obs_impact_dev(efa_ctx* c, long rows, int M, long P, const double* Xf_dev, const double* werr_dev, const double* Ya_dev,
                       const double* innov, const double* ob_error, const uint8_t* ob_used, int loc_mode, const double* ob_lat,
                       const double* ob_lon, const double* ob_halfwidth_km, const double* grid_lat, const double* grid_lon,
                       long ncol, long n_lead, double* impact) {
  EFA_TRY(use(c));
  return obs_impact(c, rows, M, P, Xf_dev, werr_dev, Ya_dev, obs_in(innov, ob_error, ob_used, loc_mode, ob_lat, ob_lon, ob_halfwidth_km),
                    grid_lat, grid_lon, ncol, n_lead, impact, false);
}

int efa_obs_impact_slab_dev(efa_ctx* c, long rows, int M, long P, const double* Xf_dev, const double* werr_dev, const double* Ya_dev,
                            const double* innov, const double* ob_error, const uint8_t* ob_used, int loc_mode, const double* ob_lat,
                            const double* ob_lon, const double* ob_halfwidth_km, const double* grid_lat, const double* grid_lon,
                            long ncol, long n_lead, double* impact) {
  EFA_TRY(use(c));
  return obs_impact(c, rows, M, P, Xf_dev, werr_dev, Ya_dev, obs_in(innov, ob_error, ob_used, loc_mode, ob_lat, ob_lon, ob_halfwidth_km),
                    grid_lat, grid_lon, ncol, n_lead, impact, true);
}

int efa_sensitivity_dev(efa_ctx* c, long rows, int M, int K, const double* X_dev, const double* J, long ncol, long n_lead,
                        const double* slab_error, const double* weights, const uint8_t* cand_dev, int n_targets, double* var_dev,
                        double* cov_dev, double* sens_dev, double* corr_dev, double* dvar_dev, double* score_dev, long* picked_row,
                        double* picked_score, double* metric_var) {
  EFA_TRY(use(c));
  return sensitivity(c, efa::Elem::f64, rows, M, K, X_dev, J, ncol, n_lead, slab_error, weights, cand_dev, n_targets, var_dev, cov_dev,
                     sens_dev, corr_dev, dvar_dev, score_dev, picked_row, picked_score, metric_var);
}

int efa_sensitivity_f32_dev(efa_ctx* c, long rows, int M, int K, const float* X_dev, const double* J, long ncol, long n_lead,
                            const double* slab_error, const double* weights, const uint8_t* cand_dev, int n_targets, double* var_dev,
                            double* cov_dev, double* sens_dev, double* corr_dev, double* dvar_dev, double* score_dev,
                            long* picked_row, double* picked_score, double* metric_var) {
  EFA_TRY(use(c));
  return sensitivity(c, efa::Elem::f32, rows, M, K, X_dev, J, ncol, n_lead, slab_error, weights, cand_dev, n_targets, var_dev, cov_dev,
                     sens_dev, corr_dev, dvar_dev, score_dev, picked_row, picked_score, metric_var);
}

int efa_verify_dev(efa_ctx* c, long rows, int M, const double* X_dev, const double* verif_dev, long ncol, long n_lead,
                   long col_offset, long ncol_total, const int* slab_group, const double* col_weight_dev, int fair, uint64_t seed,
                   int* below_dev, int* equal_dev, int* rank_dev, double* crps_dev, double* err_dev, double* var_dev,
                   long long* hist, long long* n, long long* n_bad, double* sums) {
  EFA_TRY(use(c));
  return verify(c, efa::Elem::f64, rows, M, X_dev, verif_dev, ncol, n_lead, col_offset, ncol_total, slab_group, col_weight_dev, fair,
                seed, below_dev, equal_dev, rank_dev, crps_dev, err_dev, var_dev, hist, n, n_bad, sums);
}

int efa_verify_f32_dev(efa_ctx* c, long rows, int M, const float* X_dev, const double* verif_dev, long ncol, long n_lead,
                       long col_offset, long ncol_total, const int* slab_group, const double* col_weight_dev, int fair,
                       uint64_t seed, int* below_dev, int* equal_dev, int* rank_dev, double* crps_dev, double* err_dev,
                       double* var_dev, long long* hist, long long* n, long long* n_bad, double* sums) {
  EFA_TRY(use(c));
  return verify(c, efa::Elem::f32, rows, M, X_dev, verif_dev, ncol, n_lead, col_offset, ncol_total, slab_group, col_weight_dev, fair,
                seed, below_dev, equal_dev, rank_dev, crps_dev, err_dev, var_dev, hist, n, n_bad, sums);
}

int efa_products_dev(efa_ctx* c, long rows, int M, const double* X_dev, long ncol, long n_lead, int nq, const double* q, int nt,
                     const double* thr, double* mean_dev, double* sd_dev, double* quant_dev, double* prob_dev,
                     const double* verif_dev, const int* slab_group, const double* col_weight_dev, long long* table,
                     long long* n_bad, double* sums) {
  EFA_TRY(use(c));
  return products(c, efa::Elem::f64, rows, M, X_dev, ncol, n_lead, nq, q, nt, thr, mean_dev, sd_dev, quant_dev, prob_dev, verif_dev,
                  slab_group, col_weight_dev, table, n_bad, sums);
}

int efa_products_f32_dev(efa_ctx* c, long rows, int M, const float* X_dev, long ncol, long n_lead, int nq, const double* q, int nt,
                         const double* thr, double* mean_dev, double* sd_dev, double* quant_dev, double* prob_dev,
                         const double* verif_dev, const int* slab_group, const double* col_weight_dev, long long* table,
                         long long* n_bad, double* sums) {
  EFA_TRY(use(c));
  return products(c, efa::Elem::f32, rows, M, X_dev, ncol, n_lead, nq, q, nt, thr, mean_dev, sd_dev, quant_dev, prob_dev, verif_dev,
                  slab_group, col_weight_dev, table, n_bad, sums);
}

int efa_gram_dev(efa_ctx* c, long rows, int M, const double* X_dev, long ncol, long n_lead, const double* slab_scale,
                 const double* col_weight_dev, double* gram, long long* n, long long* n_bad, double* sums) {
  EFA_TRY(use(c));
  return efa_host::gram(c, efa::Elem::f64, rows, M, X_dev, ncol, n_lead, slab_scale, col_weight_dev, gram, n, n_bad, sums);
}

int efa_gram_f32_dev(efa_ctx* c, long rows, int M, const float* X_dev, long ncol, long n_lead, const double* slab_scale,
                     const double* col_weight_dev, double* gram, long long* n, long long* n_bad, double* sums) {
  EFA_TRY(use(c));
  return efa_host::gram(c, efa::Elem::f32, rows, M, X_dev, ncol, n_lead, slab_scale, col_weight_dev, gram, n, n_bad, sums);
}

int efa_neighbourhood_dev(efa_ctx* c, long rows, int M, const double* X_dev, long ny, long nx, long n_lead, int nt, const double* thr,
                          int nr, const int* radius, int shape, int wrap_x, double* nep_dev, double* nmep_dev, const double* verif_dev,
                          const int* slab_group, const double* col_weight_dev, double* sums, long long* n, long long* n_bad) {
  EFA_TRY(use(c));
  return efa_host::neighbourhood(c, efa::Elem::f64, rows, M, X_dev, ny, nx, n_lead, nt, thr, nr, radius, shape, wrap_x, nep_dev,
                                 nmep_dev, verif_dev, slab_group, col_weight_dev, sums, n, n_bad);
}

int efa_neighbourhood_f32_dev(efa_ctx* c, long rows, int M, const float* X_dev, long ny, long nx, long n_lead, int nt,
                              const double* thr, int nr, const int* radius, int shape, int wrap_x, double* nep_dev, double* nmep_dev,
                              const double* verif_dev, const int* slab_group, const double* col_weight_dev, double* sums,
                              long long* n, long long* n_bad) {
  EFA_TRY(use(c));
  return efa_host::neighbourhood(c, efa::Elem::f32, rows, M, X_dev, ny, nx, n_lead, nt, thr, nr, radius, shape, wrap_x, nep_dev,
                                 nmep_dev, verif_dev, slab_group, col_weight_dev, sums, n, n_bad);
}

int efa_pm_mean_dev(efa_ctx* c, long rows, int M, const double* X_dev, long ny, long nx, long n_lead, const double* rank_dev,
                    const int* slab_on, long py, long px, int pick, double* pm_dev, long long* n_bad) {
  EFA_TRY(use(c));
  return efa_host::pm_mean(c, efa::Elem::f64, rows, M, X_dev, ny, nx, n_lead, rank_dev, slab_on, py, px, pick, pm_dev, n_bad);
}

int efa_pm_mean_f32_dev(efa_ctx* c, long rows, int M, const float* X_dev, long ny, long nx, long n_lead, const double* rank_dev,
                        const int* slab_on, long py, long px, int pick, double* pm_dev, long long* n_bad) {
  EFA_TRY(use(c));
  return efa_host::pm_mean(c, efa::Elem::f32, rows, M, X_dev, ny, nx, n_lead, rank_dev, slab_on, py, px, pick, pm_dev, n_bad);
}

int efa_etkf_solution(efa_ctx* c, int M, double* T, double* w, double* eig, double* stats, long* sweeps) {
  EFA_TRY(use(c));
  if (!c->have_traj || !c->batch_solved)
    return fail(EFA_ERR_INVALID, "efa_etkf_solution: the last obs phase did not run the batch solver (option obs_solver 1)");
  if (M != c->M) return fail(EFA_ERR_INVALID, "efa_etkf_solution: M=%d differs from the obs phase's M=%d", M, c->M);
  const long P = c->P;
  const efa::EtkfWs ws = efa::etkf_ws(c->etkf_buf.as<double>(), M, P);
  hipStream_t s = c->stream;
  const size_t dM = (size_t)M * sizeof(double);
  std::vector<double> h_w((size_t)M), h_g((size_t)M), h_mu((size_t)M);
  double h_qs[2] = {0.0, 0.0};  // q | sweeps
  EFA_HIP(hipMemcpyAsync(h_w.data(), c->ymw.as<double>() + P, dM, hipMemcpyDeviceToHost, s));
  EFA_HIP(hipMemcpyAsync(h_g.data(), ws.g, dM, hipMemcpyDeviceToHost, s));
  EFA_HIP(hipMemcpyAsync(h_mu.data(), ws.mu, dM, hipMemcpyDeviceToHost, s));
  EFA_HIP(hipMemcpyAsync(h_qs, ws.q, sizeof(h_qs), hipMemcpyDeviceToHost, s));
  if (T) EFA_HIP(hipMemcpyAsync(T, c->Yw.as<double>() + (size_t)P * M, (size_t)M * dM, hipMemcpyDeviceToHost, s));
  EFA_HIP(hipStreamSynchronize(s));
  std::sort(h_mu.begin(), h_mu.end(), [](double a, double b) {  // descending, NaNs last
    if (std::isnan(b)) return !std::isnan(a);
    return !std::isnan(a) && a > b;
  });
  double dfs = 0.0, gw = 0.0;
  for (int i = 0; i < M; ++i) {
    const double lam = h_mu[i] - (double)(M - 1);
    if (eig) eig[i] = lam;
    dfs += lam / h_mu[i];
    gw += h_g[i] * h_w[i];
  }
  if (w) std::memcpy(w, h_w.data(), dM);
  if (stats) {
    stats[0] = (double)c->n_active;
    stats[1] = h_qs[0];
    stats[2] = dfs;
    stats[3] = h_qs[0] - gw;
  }
  if (sweeps) *sweeps = (long)h_qs[1];
  return EFA_OK;
}

int efa_letkf_cycle_dev(efa_ctx* c, long rows, int M, long P, const double* X_dev, double* post_dev, double* ym_dev, double* Yp_dev,
                        int obs_block_out, const double* ob_value, const double* ob_error, const uint8_t* ob_assim,
                        const double* ob_lat, const double* ob_lon, const double* ob_halfwidth_km, const double* grid_lat,
                        const double* grid_lon, long ncol, long n_lead, double* prior_mean, double* prior_var, double* post_mean,
                        double* post_var, uint8_t* assimilated, double* col_stats_dev) {
  EFA_TRY(use(c));
  return efa_host::letkf_cycle(c, efa_host::StateRows{X_dev, post_dev, efa::Elem::f64, rows, M}, P,
                               ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, EFA_LOC_GC, ob_lat, ob_lon, ob_halfwidth_km),
                               obs_block_out ? ym_dev : nullptr, obs_block_out ? Yp_dev : nullptr, grid_lat, grid_lon, ncol, n_lead,
                               diag_out(prior_mean, prior_var, post_mean, post_var, assimilated), col_stats_dev, nullptr, false);
}

int efa_letkf_cycle_f32_dev(efa_ctx* c, long rows, int M, long P, const float* X_dev, float* post_dev, double* ym_dev, double* Yp_dev,
                            int obs_block_out, const double* ob_value, const double* ob_error, const uint8_t* ob_assim,
                            const double* ob_lat, const double* ob_lon, const double* ob_halfwidth_km, const double* grid_lat,
                            const double* grid_lon, long ncol, long n_lead, double* prior_mean, double* prior_var, double* post_mean,
                            double* post_var, uint8_t* assimilated, double* col_stats_dev) {
  EFA_TRY(use(c));
  return efa_host::letkf_cycle(c, efa_host::StateRows{X_dev, post_dev, efa::Elem::f32, rows, M}, P,
                               ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, EFA_LOC_GC, ob_lat, ob_lon, ob_halfwidth_km),
                               obs_block_out ? ym_dev : nullptr, obs_block_out ? Yp_dev : nullptr, grid_lat, grid_lon, ncol, n_lead,
                               diag_out(prior_mean, prior_var, post_mean, post_var, assimilated), col_stats_dev, nullptr, false);
}

int efa_letkf_weights_dev(efa_ctx* c, int M, long P, const double* ym_dev, const double* Yp_dev, const double* ob_value,
                          const double* ob_error, const uint8_t* ob_assim, const double* ob_lat, const double* ob_lon,
                          const double* ob_halfwidth_km, long npts, const double* pt_lat, const double* pt_lon, double* Tw_dev,
                          double* stats_dev) {
  EFA_TRY(use(c));
  return efa_host::letkf_weights(c, M, P, ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, EFA_LOC_GC, ob_lat, ob_lon, ob_halfwidth_km),
                                 npts, pt_lat, pt_lon, Tw_dev, stats_dev, false);
}

int efa_letkf_cycle_interp_dev(efa_ctx* c, long rows, int M, long P, const double* X_dev, double* post_dev, double* ym_dev,
                               double* Yp_dev, int obs_block_out, const double* ob_value, const double* ob_error,
                               const uint8_t* ob_assim, const double* ob_lat, const double* ob_lon, const double* ob_halfwidth_km,
                               const double* grid_lat, const double* grid_lon, long ny, long nx, long stride_y, long stride_x,
                               long n_lead, double* prior_mean, double* prior_var, double* post_mean, double* post_var,
                               uint8_t* assimilated, double* node_stats_dev) {
  EFA_TRY(use(c));
  const efa::LetkfMesh mesh{ny, nx, stride_y, stride_x};
  return efa_host::letkf_cycle(c, efa_host::StateRows{X_dev, post_dev, efa::Elem::f64, rows, M}, P,
                               ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, EFA_LOC_GC, ob_lat, ob_lon, ob_halfwidth_km),
                               obs_block_out ? ym_dev : nullptr, obs_block_out ? Yp_dev : nullptr, grid_lat, grid_lon, 0, n_lead,
                               diag_out(prior_mean, prior_var, post_mean, post_var, assimilated), node_stats_dev, &mesh, false);
}

int efa_letkf_cycle_interp_f32_dev(efa_ctx* c, long rows, int M, long P, const float* X_dev, float* post_dev, double* ym_dev,
                                   double* Yp_dev, int obs_block_out, const double* ob_value, const double* ob_error,
                                   const uint8_t* ob_assim, const double* ob_lat, const double* ob_lon, const double* ob_halfwidth_km,
                                   const double* grid_lat, const double* grid_lon, long ny, long nx, long stride_y, long stride_x,
                                   long n_lead, double* prior_mean, double* prior_var, double* post_mean, double* post_var,
                                   uint8_t* assimilated, double* node_stats_dev) {
  EFA_TRY(use(c));
  const efa::LetkfMesh mesh{ny, nx, stride_y, stride_x};
  return efa_host::letkf_cycle(c, efa_host::StateRows{X_dev, post_dev, efa::Elem::f32, rows, M}, P,
                               ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, EFA_LOC_GC, ob_lat, ob_lon, ob_halfwidth_km),
                               obs_block_out ? ym_dev : nullptr, obs_block_out ? Yp_dev : nullptr, grid_lat, grid_lon, 0, n_lead,
                               diag_out(prior_mean, prior_var, post_mean, post_var, assimilated), node_stats_dev, &mesh, false);
}

int efa_letkf_slab_cycle_dev(efa_ctx* c, long rows, int M, long P, const double* X_dev, double* post_dev, double* ym_dev,
                             double* Yp_dev, int obs_block_out, const double* ob_value, const double* ob_error, const uint8_t* ob_assim,
                             const double* ob_lat, const double* ob_lon, const double* ob_halfwidth_km, const double* grid_lat,
                             const double* grid_lon, long ncol, long n_lead, double* prior_mean, double* prior_var, double* post_mean,
                             double* post_var, uint8_t* assimilated, double* col_stats_dev) {
  EFA_TRY(use(c));
  return efa_host::letkf_cycle(c, efa_host::StateRows{X_dev, post_dev, efa::Elem::f64, rows, M}, P,
                               ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, EFA_LOC_GC, ob_lat, ob_lon, ob_halfwidth_km),
                               obs_block_out ? ym_dev : nullptr, obs_block_out ? Yp_dev : nullptr, grid_lat, grid_lon, ncol, n_lead,
                               diag_out(prior_mean, prior_var, post_mean, post_var, assimilated), col_stats_dev, nullptr, true);
}

int efa_letkf_slab_cycle_f32_dev(efa_ctx* c, long rows, int M, long P, const float* X_dev, float* post_dev, double* ym_dev,
                                 double* Yp_dev, int obs_block_out, const double* ob_value, const double* ob_error,
                                 const uint8_t* ob_assim, const double* ob_lat, const double* ob_lon, const double* ob_halfwidth_km,
                                 const double* grid_lat, const double* grid_lon, long ncol, long n_lead, double* prior_mean,
                                 double* prior_var, double* post_mean, double* post_var, uint8_t* assimilated, double* col_stats_dev) {
  EFA_TRY(use(c));
  return efa_host::letkf_cycle(c, efa_host::StateRows{X_dev, post_dev, efa::Elem::f32, rows, M}, P,
                               ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, EFA_LOC_GC, ob_lat, ob_lon, ob_halfwidth_km),
                               obs_block_out ? ym_dev : nullptr, obs_block_out ? Yp_dev : nullptr, grid_lat, grid_lon, ncol, n_lead,
                               diag_out(prior_mean, prior_var, post_mean, post_var, assimilated), col_stats_dev, nullptr, true);
}

int efa_letkf_slab_cycle_interp_dev(efa_ctx* c, long rows, int M, long P, const double* X_dev, double* post_dev, double* ym_dev,
                                    double* Yp_dev, int obs_block_out, const double* ob_value, const double* ob_error,
                                    const uint8_t* ob_assim, const double* ob_lat, const double* ob_lon, const double* ob_halfwidth_km,
                                    const double* grid_lat, const double* grid_lon, long ny, long nx, long stride_y, long stride_x,
                                    long n_lead, double* prior_mean, double* prior_var, double* post_mean, double* post_var,
                                    uint8_t* assimilated, double* node_stats_dev) {
  EFA_TRY(use(c));
  const efa::LetkfMesh mesh{ny, nx, stride_y, stride_x};
  return efa_host::letkf_cycle(c, efa_host::StateRows{X_dev, post_dev, efa::Elem::f64, rows, M}, P,
                               ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, EFA_LOC_GC, ob_lat, ob_lon, ob_halfwidth_km),
                               obs_block_out ? ym_dev : nullptr, obs_block_out ? Yp_dev : nullptr, grid_lat, grid_lon, 0, n_lead,
                               diag_out(prior_mean, prior_var, post_mean, post_var, assimilated), node_stats_dev, &mesh, true);
}

int efa_letkf_slab_cycle_interp_f32_dev(efa_ctx* c, long rows, int M, long P, const float* X_dev, float* post_dev, double* ym_dev,
                                        double* Yp_dev, int obs_block_out, const double* ob_value, const double* ob_error,
                                        const uint8_t* ob_assim, const double* ob_lat, const double* ob_lon,
                                        const double* ob_halfwidth_km, const double* grid_lat, const double* grid_lon, long ny, long nx,
                                        long stride_y, long stride_x, long n_lead, double* prior_mean, double* prior_var,
                                        double* post_mean, double* post_var, uint8_t* assimilated, double* node_stats_dev) {
  EFA_TRY(use(c));
  const efa::LetkfMesh mesh{ny, nx, stride_y, stride_x};
  return efa_host::letkf_cycle(c, efa_host::StateRows{X_dev, post_dev, efa::Elem::f32, rows, M}, P,
                               ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, EFA_LOC_GC, ob_lat, ob_lon, ob_halfwidth_km),
                               obs_block_out ? ym_dev : nullptr, obs_block_out ? Yp_dev : nullptr, grid_lat, grid_lon, 0, n_lead,
                               diag_out(prior_mean, prior_var, post_mean, post_var, assimilated), node_stats_dev, &mesh, true);
}

int efa_letkf_slab_weights_dev(efa_ctx* c, int M, long P, const double* ym_dev, const double* Yp_dev, const double* ob_value,
                               const double* ob_error, const uint8_t* ob_assim, const double* ob_lat, const double* ob_lon,
                               const double* ob_halfwidth_km, long npts, const double* pt_lat, const double* pt_lon, double* Tw_dev,
                               double* stats_dev) {
  EFA_TRY(use(c));
  return efa_host::letkf_weights(c, M, P, ym_dev, Yp_dev, obs_in(ob_value, ob_error, ob_assim, EFA_LOC_GC, ob_lat, ob_lon, ob_halfwidth_km),
                                 npts, pt_lat, pt_lon, Tw_dev, stats_dev, true);
}

int efa_letkf_slab_groups(efa_ctx* c, long n_lead, int* group_of, int* ngroups) {
  EFA_TRY(use(c));
  return efa_host::letkf_slab_group_table(c, n_lead, group_of, ngroups);
}

int efa_letkf_interp_apply_dev(efa_ctx* c, long rows, int M, const double* X_dev, double* post_dev, long ny, long nx, long stride_y,
                               long stride_x, long n_lead, const double* Tw_nodes_dev, const double* node_stats_dev) {
  EFA_TRY(use(c));
  return efa_host::letkf_interp_apply(c, efa_host::StateRows{X_dev, post_dev, efa::Elem::f64, rows, M},
                                      efa::LetkfMesh{ny, nx, stride_y, stride_x}, n_lead, Tw_nodes_dev, node_stats_dev);
}

int efa_letkf_interp_apply_f32_dev(efa_ctx* c, long rows, int M, const float* X_dev, float* post_dev, long ny, long nx, long stride_y,
                                   long stride_x, long n_lead, const double* Tw_nodes_dev, const double* node_stats_dev) {
  EFA_TRY(use(c));
  return efa_host::letkf_interp_apply(c, efa_host::StateRows{X_dev, post_dev, efa::Elem::f32, rows, M},
                                      efa::LetkfMesh{ny, nx, stride_y, stride_x}, n_lead, Tw_nodes_dev, node_stats_dev);
}

int efa_last_timing(efa_ctx* c, double* state_ms, double* obs_ms, long* state_launches, int* path_taken) {
  if (!c) return fail(EFA_ERR_INVALID, "null context");
  harvest_obs_ms(c);
  harvest_state_ms(c);
  if (c->timing == 2) {  // deferred: the sums over the calls since the previous efa_last_timing
    if (state_ms) *state_ms = c->state_ms_sum;
    if (obs_ms) *obs_ms = c->obs_ms_sum;
    if (state_launches) *state_launches = c->state_launches_sum;
    c->state_ms_sum = c->obs_ms_sum = 0.0;
    c->state_launches_sum = 0;
  } else {
    if (state_ms) *state_ms = c->state_ms;
    if (obs_ms) *obs_ms = c->obs_ms;
    if (state_launches) *state_launches = c->state_launches;
  }
  if (path_taken) *path_taken = c->path_taken;
  return EFA_OK;
}

int efa_fill_synthetic_dev(efa_ctx* c, long rows, long row_offset, int M, uint64_t seed, double sigma,
                           double* X_dev) {
  EFA_TRY(use(c));
  if (rows < 0 || M < 1) return fail(EFA_ERR_INVALID, "bad shape");
  if (rows && !X_dev) return fail(EFA_ERR_INVALID, "null pointer");
  EFA_HIP(efa::launch_fill_synthetic(rows, row_offset, M, seed, sigma, X_dev, c->stream));
  return EFA_OK;
}

// ---- cost of a column block under Gaspari-Cohn localisation (the sharding plan of SURVEY.md 8e) ------------
int efa_gc_block_counts(efa_ctx* c, long ncol, const double* grid_lat, const double* grid_lon, long P, const double* ob_lat,
                        const double* ob_lon, const double* ob_halfwidth_km, const uint8_t* ob_assim, int32_t* block_count,
                        int32_t* block_pairs, uint64_t* active_pairs) {
  EFA_TRY(use(c));
  if (ncol <= 0 || P < 0) return fail(EFA_ERR_INVALID, "bad shape");
  if (!grid_lat || !grid_lon || !block_count || (P && (!ob_lat || !ob_lon || !ob_halfwidth_km || !ob_assim)))
    return fail(EFA_ERR_INVALID, "null pointer");
  const long nblk = efa::gc_num_blocks(ncol);
  hipStream_t s = c->stream;
  std::vector<double> coef((size_t)(P ? P : 1) * efa::kCoefStride, 0.0), hw((size_t)(P ? P : 1), 1.0);
  for (long k = 0; k < P; ++k) {
    const bool on = ob_assim[k] != 0;
    coef[(size_t)k * efa::kCoefStride + 3] = on ? 1.0 : 0.0;
    if (on) {
      if (!(ob_halfwidth_km[k] == ob_halfwidth_km[k]) || ob_halfwidth_km[k] == 0.0)
        return fail(EFA_ERR_INVALID, "observation %ld: localize_radius must be a non-zero number", k);
      hw[k] = ob_halfwidth_km[k];
    }
  }
  EFA_TRY(h2d(c, c->gcc_lat, grid_lat, (size_t)ncol * sizeof(double)));
  EFA_TRY(h2d(c, c->gcc_lon, grid_lon, (size_t)ncol * sizeof(double)));
  EFA_TRY(h2d(c, c->gcc_oblat, ob_lat, (size_t)P * sizeof(double)));
  EFA_TRY(h2d(c, c->gcc_oblon, ob_lon, (size_t)P * sizeof(double)));
  EFA_TRY(h2d(c, c->gcc_obhw, hw.data(), (size_t)P * sizeof(double)));
  EFA_TRY(h2d(c, c->gcc_coef, coef.data(), (size_t)P * efa::kCoefStride * sizeof(double)));
  EFA_TRY(c->gcc_trig.reserve((size_t)(P ? P : 1) * 6 * sizeof(double)));
  EFA_TRY(c->gcc_cnt.reserve((size_t)2 * nblk * sizeof(int)));  // [counts | pairs]
  EFA_TRY(c->gcc_pairs.reserve(sizeof(unsigned long long)));
  EFA_HIP(hipMemsetAsync(c->gcc_pairs.p, 0, sizeof(unsigned long long), s));
  EFA_HIP(hipMemsetAsync(c->gcc_cnt.p, 0, (size_t)2 * nblk * sizeof(int), s));
  if (P > 0)
    EFA_HIP(efa::launch_gc_count(ncol, P, c->gcc_lat.as<double>(), c->gcc_lon.as<double>(), c->gcc_oblat.as<double>(),
                                 c->gcc_oblon.as<double>(), c->gcc_obhw.as<double>(), c->gcc_coef.as<double>(),
                                 c->gcc_trig.as<double>(), c->gcc_cnt.as<int>(), c->gcc_cnt.as<int>() + nblk,
                                 c->gcc_pairs.as<unsigned long long>(), s));
  unsigned long long pairs = 0;
  EFA_HIP(hipMemcpyAsync(block_count, c->gcc_cnt.p, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost, s));
  if (block_pairs)
    EFA_HIP(hipMemcpyAsync(block_pairs, c->gcc_cnt.as<int>() + nblk, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost, s));
  EFA_HIP(hipMemcpyAsync(&pairs, c->gcc_pairs.p, sizeof(pairs), hipMemcpyDeviceToHost, s));
  EFA_HIP(hipStreamSynchronize(s));
  if (active_pairs) *active_pairs = pairs;
  return EFA_OK;
}

}  // extern "C"
