// The host scaffolding the drivers of the diagnostics share (efa_verify.hip, efa_products.hip, efa_gram.hip, efa_neighbourhood.hip,
// efa_pmmean.hip; efa_sensitivity.hip records its intervals with it too, but adds up the time of its passes itself).  Not exported.
#pragma once
#include "efa_driver.h"

#include <cmath>
#include <vector>

namespace efa_host {

// ---- the device time of a call -----------------------------------------------------------------------------------------------------
// interval_begin creates the interval's events on first use and records the first, interval_end records the second, and once the
// stream has been synchronised interval_us reads the microseconds between them.
inline int interval_begin(Interval& iv, hipStream_t s) {
  if (!iv.begin.h) EFA_HIP(hipEventCreate(&iv.begin.h));
  if (!iv.end.h) EFA_HIP(hipEventCreate(&iv.end.h));
  EFA_HIP(hipEventRecord(iv.begin, s));
  return EFA_OK;
}
inline int interval_end(Interval& iv, hipStream_t s) {
  EFA_HIP(hipEventRecord(iv.end, s));
  return EFA_OK;
}
inline int interval_us(const Interval& iv, long* us) {
  float ms = 0.f;
  EFA_HIP(hipEventElapsedTime(&ms, iv.begin, iv.end));
  *us = (long)std::llround((double)ms * 1000.0);
  return EFA_OK;
}

// ---- a workspace carved into typed regions -------------------------------------------------------------------------------------------
// A driver declares its regions once, in the order efa_ctx.h documents: add<T>(n) gives the next region n elements of T, aligned
// to alignof(T) (or to the layout's min_align, if that is more; align_to(a) pads up to a multiple of a before the next one), and
// returns its handle.  bytes() is what reserve() needs; handle(buf) is the region's typed pointer in the reserved buffer.  Size
// and pointers come from the one declaration, so they cannot disagree.
class WsLayout {
 public:
  explicit WsLayout(size_t min_align = 1) : min_align_(min_align) {}
  template <typename T>
  struct Region {
    size_t offset = 0;
    T* operator()(const DevBuf& b) const { return reinterpret_cast<T*>(b.as<char>() + offset); }
  };
  template <typename T>
  Region<T> add(size_t n) {
    align_to(alignof(T) > min_align_ ? alignof(T) : min_align_);
    Region<T> r;
    r.offset = bytes_;
    bytes_ += n * sizeof(T);
    return r;
  }
  void align_to(size_t a) { bytes_ = (bytes_ + a - 1) / a * a; }
  size_t bytes() const { return bytes_; }

 private:
  size_t min_align_, bytes_ = 0;
};

// ---- argument checks and staging -------------------------------------------------------------------------------------------------------
// every slab's group is >= -1 (-1: not scored); *G: the number of groups, the largest index + 1
inline int check_slab_groups(const char* me, const int* slab_group, long n_lead, int* G) {
  *G = 0;
  for (long s = 0; s < n_lead; ++s) {
    if (slab_group[s] < -1) return fail(EFA_ERR_INVALID, "%s: slab_group[%ld] = %d must be >= -1", me, s, slab_group[s]);
    if (slab_group[s] + 1 > *G) *G = slab_group[s] + 1;
  }
  return EFA_OK;
}

// thr [n_lead][nt] as the kernels read it: [n_lead][width], NaN (no threshold) beyond nt
inline std::vector<double> pad_thresholds(const double* thr, long n_lead, int nt, int width) {
  std::vector<double> h((size_t)n_lead * width, std::nan(""));
  for (long l = 0; l < n_lead; ++l)
    for (int j = 0; j < nt; ++j) h[(size_t)l * width + j] = thr[(size_t)l * nt + j];
  return h;
}

// the rows are aligned for the paired loads: M even and the base aligned to two elements
inline bool pairs_aligned(const void* X, int M, efa::Elem elem) {
  return (M % 2 == 0) && (reinterpret_cast<uintptr_t>(X) % (2 * efa::elem_size(elem)) == 0);
}

// a "*_blocks" option: 0 or anything beyond the cap is the cap
inline long clamp_blocks(long option, long cap) { return (option < 1 || option > cap) ? cap : option; }

// ---- the launch of a kernel on the four-lane row layout (efa_quadrow.h) ------------------------------------------------------------
// NU is (M + 7) / 8 rounded up to a power of two: the sort network is that of 2 NU slots whatever M is, so the six sizes times the
// two element types are the only instantiations.  launch(nu_c, e) launches the kernel for NU = decltype(nu_c)::value and rows of
// decltype(e).
template <class F>
hipError_t launch_quad(int M, efa::Elem elem, F&& launch) {
  int nu_p = 1;
  while (nu_p * 8 < M) nu_p *= 2;
  return efa::dispatch_width(nu_p, std::integer_sequence<int, 1, 2, 4, 8, 16, 32>{}, [&](auto nu_c) {
    return elem == efa::Elem::f32 ? launch(nu_c, float{}) : launch(nu_c, double{});
  });
}

}  // namespace efa_host
