// The host driver of the LETKF entries: efa_letkf_cycle_dev and its f32 / interp / slab kin,
// efa_letkf_weights_dev / efa_letkf_slab_weights_dev, efa_letkf_interp_apply_dev and efa_letkf_slab_groups.  The kernels and their
// launchers are in efa_letkf.hip and efa_letkf_interp.hip.
//   obs    the per-ob arrays to the device, k_letkf_prior (flags, prior diagnostics, {d, r}), the lists at the ob positions (under
//          the slab settings scaled by k_letkf_obs_factor) and the obs block as P one-row columns (kLetkfPerts).
//   state  the lists of the grid's columns and ONE k_letkf launch (kLetkfMembers); with a mesh the lists of its nodes, the node
//          solve (kLetkfWeights) and k_letkf_interp.  Under the slab settings both take the groups (letkf_slab_groups) and run one
//          solve per (group, column or node).
//   inflation  the context's per-point field (efa_ctx_set_letkf_inflation), checked against the call before any
//          launch, goes with the launch that solves: the columns' or the nodes'; the obs block takes the fixed ob factors.
//   control  the context's deterministic control (efa_ctx_set_letkf_control), checked against the call before any
//          launch: its innovations d^c beside dr (k_letkf_control_prior), then a second right-hand side in the obs block's and the
//          columns' launch.  The plain and the slab cycle serve it; the interp cycles and the weights entries refuse it.
//   cap    the context's cap on the local obs of a solve (efa_ctx_set_letkf_obs_cap), checked against the call before
//          any launch: k_letkf_cap behind every list build (letkf_build_lists), so the obs', the grid's, the nodes' and the probe's
//          lists are capped in one place.  The plain and the interp cycles and efa_letkf_weights_dev serve it; the slab entries refuse it.
//   cross validation  the context's member groups (efa_ctx_set_letkf_cross_validation), checked against the call before
//          any launch: every solve runs k_letkf_cv, which leaves the recentred cross-validated T beside the plain w; the obs block's
//          rows are mapped in that launch, the state always by k_letkf_interp (without a mesh: on the unit mesh whose nodes are the
//          columns).  The plain and the interp cycles and efa_letkf_weights_dev serve it; the slab entries, and any call with an
//          inflation field or a control set, are refused while it is on.
#include "efa_driver.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

namespace efa_host {

using namespace efa;

namespace {

// the per-ob arrays of a call on the device, slices of c->letkf_ob
struct LetkfObs {
  long P = 0;
  double *value = nullptr, *error = nullptr, *lat = nullptr, *lon = nullptr, *hw = nullptr, *req = nullptr;
  double *act = nullptr, *dr = nullptr, *obtrig = nullptr, *dc = nullptr;
  double *prior_mean = nullptr, *prior_var = nullptr, *post_mean = nullptr, *post_var = nullptr;
  uint8_t* assimilated = nullptr;
  size_t diag_bytes() const { return 4 * (size_t)P * sizeof(double) + (size_t)P; }
};

// the lists of one set of points, slices of c->letkf_blk and the two entry buffers
struct LetkfLists {
  const long* off = nullptr;
  const int *cnt = nullptr, *order = nullptr, *idx = nullptr;
  const double* wts = nullptr;
};

// What no LETKF call serves, refused before anything is launched (include/efa_hip.h gives the reasons)
// slab: the calls of DESIGN.md §7y-3, which need the vertical and/or the slab setting, sized for this call (n_lead < 0: not checked)
int letkf_check_settings(const efa_ctx* c, const char* who, int M, long P, bool slab = false, long n_lead = -1) {
  if (M < 2) return fail(EFA_ERR_INVALID, "%s: ensemble size M=%d must be >= 2", who, M);
  if (M > kLetkfMaxM)
    return fail(EFA_ERR_INVALID, "%s: M=%d exceeds %d members, the range in which the eigen-solve's M x M array of a column fits in LDS",
                who, M, kLetkfMaxM);
  if (P < 0) return fail(EFA_ERR_INVALID, "%s: negative observation count", who);
  if (c->ai_field)
    return fail(EFA_ERR_INVALID, "%s: an adaptive-inflation field is set (its update follows the serial order of the obs, which a "
                "column's batch solve does not have)", who);
  if (!slab && c->vl_on)
    return fail(EFA_ERR_INVALID, "%s: vertical localisation is set (it needs a solve per (slab group, column): out of scope here, "
                "use efa_letkf_slab_cycle_dev / SlabLETKF)", who);
  if (!slab && c->sl_on)
    return fail(EFA_ERR_INVALID, "%s: slab (temporal / cross-variable) localisation is set (it needs a solve per (slab group, column): "
                "out of scope here, use efa_letkf_slab_cycle_dev / SlabLETKF)", who);
  if (slab) {
    if (!c->vl_on && !c->sl_on)
      return fail(EFA_ERR_INVALID, "%s: neither vertical nor slab (temporal / cross-variable) localisation is set: use the plain call "
                  "(efa_letkf_cycle_dev and its kin)", who);
    if (c->vl_on && (c->vl_P != P || (n_lead >= 0 && c->vl_nlead != n_lead)))
      return fail(EFA_ERR_INVALID, "%s: vertical localisation was set for %ld observations and %ld slabs, the call has %ld and n_lead=%ld",
                  who, c->vl_P, c->vl_nlead, P, n_lead);
    if (c->sl_on && (c->sl_P != P || (n_lead >= 0 && c->sl_nlead != n_lead)))
      return fail(EFA_ERR_INVALID, "%s: slab localisation was set for %ld observations and %ld slabs, the call has %ld and n_lead=%ld", who,
                  c->sl_P, c->sl_nlead, P, n_lead);
  }
  if (sec_active(c))
    return fail(EFA_ERR_INVALID, "%s: a sampling-error-correction table is set (it acts on the serial gain of one observation at a time)",
                who);
  return EFA_OK;
}

int letkf_check_obs(const char* who, long P, const double* ym_dev, const double* Yp_dev, const ObsIn& in) {
  if (P == 0) return EFA_OK;
  if (!ym_dev || !Yp_dev || !in.value || !in.error || !in.assim)
    return fail(EFA_ERR_INVALID, "%s: null observation array", who);
  if (!in.lat || !in.lon || !in.hw) return fail(EFA_ERR_INVALID, "%s: the taper needs ob_lat/ob_lon/ob_halfwidth_km", who);
  for (long k = 0; k < P; ++k) {
    if (!in.assim[k]) continue;
    if (!(std::isfinite(in.error[k]) && in.error[k] > 0.0))
      return fail(EFA_ERR_INVALID, "%s: observation %ld: error variance %g must be finite and > 0 (R-localisation divides by it)", who, k,
                  in.error[k]);
    if (!(in.hw[k] == in.hw[k]) || in.hw[k] == 0.0)
      return fail(EFA_ERR_INVALID, "%s: observation %ld: localize_radius must be a non-zero number", who, k);
  }
  return EFA_OK;
}

// the obs on the device, then their prior diagnostics, effective flags and {d, r}
int letkf_stage_obs(efa_ctx* c, int M, long P, const double* ym_dev, const double* Yp_dev, const ObsIn& in, LetkfObs* out) {
  hipStream_t s = c->stream;
  const size_t n = (size_t)P;
  // value | error | lat | lon | hw | requested [n each] | act [4n] | dr [2n] | obtrig [6n] | dc [n] | four diagnostics [n each] |
  // assimilated bytes
  EFA_TRY(c->letkf_ob.reserve((23 * n + 1) * sizeof(double) + n));
  double* d = c->letkf_ob.as<double>();
  LetkfObs o;
  o.P = P;
  o.value = d;
  o.error = d + n;
  o.lat = d + 2 * n;
  o.lon = d + 3 * n;
  o.hw = d + 4 * n;
  o.req = d + 5 * n;
  o.act = d + 6 * n;
  o.dr = d + 10 * n;
  o.obtrig = d + 12 * n;
  o.dc = d + 18 * n;
  o.prior_mean = d + 19 * n;
  o.prior_var = d + 20 * n;
  o.post_mean = d + 21 * n;
  o.post_var = d + 22 * n;
  o.assimilated = reinterpret_cast<uint8_t*>(d + 23 * n);
  // value and error of an ob that is not requested are not read: the device gets the neutral pair (0, 1), its radius a harmless 1
  std::vector<double> h(6 * n);
  for (size_t k = 0; k < n; ++k) {
    const bool on = in.assim[k] != 0;
    h[k] = on ? in.value[k] : 0.0;
    h[n + k] = on ? in.error[k] : 1.0;
    h[2 * n + k] = in.lat[k];
    h[3 * n + k] = in.lon[k];
    h[4 * n + k] = on ? in.hw[k] : 1.0;
    h[5 * n + k] = on ? 1.0 : 0.0;
  }
  EFA_HIP(hipMemcpyAsync(d, h.data(), 6 * n * sizeof(double), hipMemcpyHostToDevice, s));
  EFA_HIP(hipStreamSynchronize(s));  // (h goes out of scope)
  EFA_HIP(launch_letkf_prior(P, M, Yp_dev, ym_dev, o.value, o.error, o.req, c->qc_threshold * c->qc_threshold, o.prior_mean,
                             o.prior_var, o.assimilated, o.act, o.dr, s));
  // the control's innovations under the same effective flags
  if (c->lc_xc) EFA_HIP(launch_letkf_control_prior(P, o.value, c->lc_yc, o.assimilated, o.dc, s));
  *out = o;
  return EFA_OK;
}

// The lists of `npts` points (device lat / lon) against the obs, by the one-pass sweep's builders as they are; the flag entry of the
// coefficient table they read is the effective a_k.  One host round trip: the capacity.
// With the cap set k_letkf_cap follows the fill; reach (or null): where it leaves the points' counts before the cap.
int letkf_build_lists(efa_ctx* c, long npts, const double* plat, const double* plon, const LetkfObs& o, LetkfLists* out,
                      double* reach = nullptr) {
  hipStream_t s = c->stream;
  const long nblk = gc_num_blocks(npts);
  const size_t b8 = ((size_t)(nblk + 1) * sizeof(long) + 15) & ~(size_t)15, b4 = ((size_t)nblk * sizeof(int) + 15) & ~(size_t)15;
  EFA_TRY(c->letkf_blk.reserve(b8 + 3 * b4));
  EFA_TRY(c->letkf_pairs.reserve(sizeof(unsigned long long)));
  char* b = static_cast<char*>(c->letkf_blk.p);
  long* off = reinterpret_cast<long*>(b);
  int* cnt = reinterpret_cast<int*>(b + b8);
  int* ub = reinterpret_cast<int*>(b + b8 + b4);
  int* order = reinterpret_cast<int*>(b + b8 + 2 * b4);
  EFA_HIP(hipMemsetAsync(c->letkf_pairs.p, 0, sizeof(unsigned long long), s));
  EFA_HIP(launch_gc_bound(npts, o.P, plat, o.lat, o.hw, o.act, ub, off, s));
  long cap = 0;
  EFA_HIP(hipMemcpyAsync(&cap, off + nblk, sizeof(long), hipMemcpyDeviceToHost, s));
  EFA_HIP(hipStreamSynchronize(s));
  EFA_TRY(c->letkf_idx.reserve((size_t)(cap ? cap : 1) * sizeof(int)));
  EFA_TRY(c->letkf_wts.reserve((size_t)(cap ? cap : 1) * 16 * sizeof(double)));
  EFA_HIP(launch_gc_fill(npts, o.P, plat, plon, o.lat, o.lon, o.hw, o.act, o.obtrig, off, cnt, c->letkf_idx.as<int>(),
                         c->letkf_wts.as<double>(), order, c->letkf_pairs.as<unsigned long long>(), s));
  if (c->oc_on) {
    LetkfCapArgs ca{};
    ca.npts = npts;
    ca.off = off;
    ca.cnt = cnt;
    ca.idx = c->letkf_idx.as<int>();
    ca.wts = c->letkf_wts.as<double>();
    ca.ob_class = c->oc_has_class ? c->oc_class.as<int>() : nullptr;
    ca.nclass = c->oc_nclass;
    for (int k = 0; k < kLetkfCapClasses; ++k) ca.cap[k] = c->oc_cap[k];
    ca.reach = reach;
    EFA_HIP(launch_letkf_cap(ca, s));
  }
  out->off = off;
  out->cnt = cnt;
  out->order = order;
  out->idx = c->letkf_idx.as<int>();
  out->wts = c->letkf_wts.as<double>();
  return EFA_OK;
}

int letkf_upload_points(efa_ctx* c, long npts, const double* lat, const double* lon, const double** dlat, const double** dlon) {
  const size_t nb = (size_t)npts * sizeof(double);
  EFA_TRY(c->letkf_pts.reserve(2 * nb));
  double* d = c->letkf_pts.as<double>();
  EFA_HIP(hipMemcpyAsync(d, lat, nb, hipMemcpyHostToDevice, c->stream));
  EFA_HIP(hipMemcpyAsync(d + npts, lon, nb, hipMemcpyHostToDevice, c->stream));
  EFA_HIP(hipStreamSynchronize(c->stream));  // the caller may reuse its arrays on return
  *dlat = d;
  *dlon = d + npts;
  return EFA_OK;
}

// ... of the nodes of a mesh: a node is a grid column, its position is that column's
int letkf_upload_nodes(efa_ctx* c, const LetkfMesh& nodes, const double* grid_lat, const double* grid_lon, const double** dlat,
                       const double** dlon) {
  const long nyn = nodes.nyn(), nxn = nodes.nxn(), nnodes = nyn * nxn;
  std::vector<double> h(2 * (size_t)nnodes);
  for (long jy = 0; jy < nyn; ++jy)
    for (long jx = 0; jx < nxn; ++jx) {
      const long col = LetkfMesh::axis_node(jy, nodes.ny, nodes.sy) * nodes.nx + LetkfMesh::axis_node(jx, nodes.nx, nodes.sx);
      h[jy * nxn + jx] = grid_lat[col];
      h[nnodes + jy * nxn + jx] = grid_lon[col];
    }
  return letkf_upload_points(c, nnodes, h.data(), h.data() + nnodes, dlat, dlon);
}

LetkfArgs letkf_args(int M, long npts, const LetkfLists& l, const double* Yp, const LetkfObs& o) {
  LetkfArgs a{};
  a.npts = npts;
  a.n_lead = 1;
  a.M = M;
  a.off = l.off;
  a.cnt = l.cnt;
  a.order = l.order;
  a.idx = l.idx;
  a.wts = l.wts;
  a.Yp = Yp;
  a.dr = o.dr;
  a.relax_kind = EFA_RELAX_NONE;
  return a;
}

// The inflation setting against a call, before any launch: sized for its P and its `nsolve` solve points
// (nsolve < 0: the call solves at no state point), the field's values, and with `obs_block` the ob factors', finite and within the
// bounds.  Two small downloads.
int letkf_check_inflation(efa_ctx* c, const char* who, long P, long nsolve, bool obs_block) {
  if (!c->li_field) return EFA_OK;
  if (c->li_P != P) return fail(EFA_ERR_INVALID, "%s: the LETKF inflation was set for %ld observations, the call has %ld", who, c->li_P, P);
  if (nsolve >= 0 && c->li_nsolve != nsolve)
    return fail(EFA_ERR_INVALID, "%s: the LETKF inflation field was set for %ld solve points, the call has %ld (groups x columns, nodes or "
                "probe points)", who, c->li_nsolve, nsolve);
  std::vector<double> h;
  const auto check = [&](const double* dev, long n, const char* what) -> int {
    h.resize((size_t)n);
    EFA_HIP(hipMemcpyAsync(h.data(), dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    EFA_HIP(hipStreamSynchronize(c->stream));
    for (long i = 0; i < n; ++i)
      if (!(std::isfinite(h[i]) && h[i] >= c->li_lower && h[i] <= c->li_upper))
        return fail(EFA_ERR_INVALID, "%s: LETKF inflation: %s %ld is %g, not a finite value within [%g, %g]", who, what, i, h[i],
                    c->li_lower, c->li_upper);
    return EFA_OK;
  };
  if (nsolve > 0) EFA_TRY(check(c->li_field, nsolve, "the field's value"));
  if (obs_block && c->li_ob && P > 0) EFA_TRY(check(c->li_ob, P, "the factor of observation"));
  return EFA_OK;
}

// The control setting against a call, before any launch.  served: the plain and the slab cycle; every other entry
// that solves has no place for w^c (the pairs are laid out [M][M + 1]) and refuses the call while the setting is on.
int letkf_check_control(const efa_ctx* c, const char* who, bool served, long rows, long P) {
  if (!c->lc_xc) return EFA_OK;
  if (!served)
    return fail(EFA_ERR_INVALID, "%s: a LETKF control is set (efa_ctx_set_letkf_control): the pairs [T | w] this call solves or "
                "interpolates have no place for the control's weight vector w^c; weight interpolation of w^c is a follow-up", who);
  if (c->lc_rows != rows) return fail(EFA_ERR_INVALID, "%s: the LETKF control was set for %ld rows, the call has %ld", who, c->lc_rows, rows);
  if (c->lc_P != P) return fail(EFA_ERR_INVALID, "%s: the LETKF control was set for %ld observations, the call has %ld", who, c->lc_P, P);
  return EFA_OK;
}

// The cap setting against a call, before any launch.  served: the plain and the interp cycles and
// efa_letkf_weights_dev; nsolve: the state's solve points of the call (< 0: it solves at none).
int letkf_check_cap(const efa_ctx* c, const char* who, bool served, long P, long nsolve) {
  if (!c->oc_on) return EFA_OK;
  if (!served)
    return fail(EFA_ERR_INVALID, "%s: a LETKF obs cap is set (efa_ctx_set_letkf_obs_cap): under the vertical / slab settings the taper "
                "of a solve is a product per (slab group, column) while the lists' tapers, which the cap ranks, are per column; a cap "
                "per group is a follow-up", who);
  if (c->oc_P != P) return fail(EFA_ERR_INVALID, "%s: the LETKF obs cap was set for %ld observations, the call has %ld", who, c->oc_P, P);
  if (c->oc_reach && nsolve >= 0 && c->oc_nsolve != nsolve)
    return fail(EFA_ERR_INVALID, "%s: the LETKF obs cap's reach array was set for %ld solve points, the call has %ld (columns, nodes or "
                "probe points)", who, c->oc_nsolve, nsolve);
  return EFA_OK;
}

// The cross-validation setting against a call, before any launch.  Served by the plain and the interp cycles and
// efa_letkf_weights_dev, without an inflation field and without a control; nsolve: the state's solve points of the call (< 0: none).
int letkf_check_cv(const efa_ctx* c, const char* who, bool slab, int M, long nsolve) {
  if (!c->cv_on) return EFA_OK;
  if (slab)
    return fail(EFA_ERR_INVALID, "%s: a LETKF cross validation is set (efa_ctx_set_letkf_cross_validation): the solves per (slab group, "
                "column) under it are out of scope", who);
  if (c->li_field)
    return fail(EFA_ERR_INVALID, "%s: a LETKF cross validation and a LETKF inflation field are both set: the sub-solves under a per-point "
                "factor, and its estimate under them, are out of scope", who);
  if (c->lc_xc)
    return fail(EFA_ERR_INVALID, "%s: a LETKF cross validation and a LETKF control are both set: the cross-validated cycle applies the "
                "pairs [T | w], which have no place for the control's weight vector", who);
  if (c->cv_M != M) return fail(EFA_ERR_INVALID, "%s: the LETKF cross validation was set for %d members, the call has %d", who, c->cv_M, M);
  if (c->cv_stats && nsolve >= 0 && c->cv_nsolve != nsolve)
    return fail(EFA_ERR_INVALID, "%s: the LETKF cross validation's statistics were set for %ld solve points, the call has %ld (columns, "
                "nodes or probe points)", who, c->cv_nsolve, nsolve);
  return EFA_OK;
}

// ... as the launch takes it, with the scratch for `npts` points; stats: where the sub-solves' statistics go, or null
int letkf_cv_args(efa_ctx* c, int M, long npts, double* stats, LetkfCv* out) {
  if (c->cv_C.reserve((size_t)(npts > 0 ? npts : 1) * M * M * sizeof(double)) != EFA_OK)
    return fail(EFA_ERR_ALLOC, "LETKF cross validation: the scratch of %ld points x %d x %d doubles could not be allocated", npts, M, M);
  const int* l = c->cv_lists.as<int>();
  *out = LetkfCv{c->cv_ngroups, l, l + (size_t)c->cv_ngroups * M, c->cv_C.as<double>(), stats};
  return EFA_OK;
}

// ... into the arguments of the obs block's launch (y_c) or of the columns' (x_c)
void letkf_args_control(const efa_ctx* c, LetkfArgs* a, const LetkfObs& o, bool obs_block) {
  if (!c->lc_xc || !o.dc) return;  // (no obs: no solve, the driver copies the control)
  a->dc = o.dc;
  a->ctl_in = obs_block ? c->lc_yc : c->lc_xc;
  a->ctl_out = obs_block ? c->lc_yc_post : c->lc_xc_post;
}

// ... into the arguments of a state or node solve (the field, updated when sigma_b > 0) or of the obs block (the fixed ob factors)
void letkf_args_inflation(const efa_ctx* c, LetkfArgs* a, bool obs_block) {
  if (!c->li_field) return;
  a->infl_lo = c->li_lower;
  a->infl_hi = c->li_upper;
  if (obs_block) {
    a->infl = const_cast<double*>(c->li_ob);  // (never written: sigma2 = 0)
    return;
  }
  a->infl = c->li_field;
  a->infl_sigma2 = c->li_sigma_b * c->li_sigma_b;
  a->infl_stats = c->li_stats;
}

// the solve at `npts` points whose lists are built: [T | w] of each to Tw, the statistics to stats (or null); does not wait
// (grp: [T | w] of every (group, point), the statistics [group][point][3])
int letkf_solve_points(efa_ctx* c, int M, long npts, const LetkfLists& lists, const double* Yp_dev, const LetkfObs& o,
                       const LetkfGroups* grp, double* Tw, double* stats) {
  LetkfArgs a = letkf_args(M, npts, lists, Yp_dev, o);
  a.Tw = Tw;
  a.stats = stats;
  if (c->cv_on) {  // (checked: no groups, no inflation field) the recentred cross-validated T beside the same w
    LetkfCv cv{};
    EFA_TRY(letkf_cv_args(c, M, npts, c->cv_stats, &cv));
    EFA_HIP(launch_letkf_cv(a, cv, c->stream));
    return EFA_OK;
  }
  letkf_args_inflation(c, &a, false);
  EFA_HIP(launch_letkf(a, grp, kLetkfWeights, Elem::f64, c->stream));
  return EFA_OK;
}

// the mesh of a weight-interpolation call; *out has the strides cut to the axis (a stride beyond it gives the same nodes: the two ends)
int letkf_check_mesh(const char* who, const LetkfMesh& m, LetkfMesh* out) {
  if (m.ny < 1 || m.nx < 1) return fail(EFA_ERR_INVALID, "%s: the grid's shape (%ld, %ld) must be positive", who, m.ny, m.nx);
  if (m.ny > 0x7FFFFFF0L / m.nx) return fail(EFA_ERR_INVALID, "%s: %ld x %ld columns exceed the launch grid", who, m.ny, m.nx);
  if (m.sy < 1 || m.sx < 1) return fail(EFA_ERR_INVALID, "%s: the weight stride (%ld, %ld) must be >= 1 on both axes", who, m.sy, m.sx);
  *out = m;
  const long cy = m.ny > 2 ? m.ny - 1 : 1, cx = m.nx > 2 ? m.nx - 1 : 1;
  if (out->sy > cy) out->sy = cy;
  if (out->sx > cx) out->sx = cx;
  return EFA_OK;
}

// the member rows of a state call: pointers, alignment, overlap (rows == n_lead * ncol is each caller's own check)
int letkf_check_rows(const char* who, const StateRows& r) {
  if (r.rows < 0) return fail(EFA_ERR_INVALID, "%s: negative row count", who);
  if (r.rows == 0) return EFA_OK;
  if (!r.prior || !r.post) return fail(EFA_ERR_INVALID, "%s: null state pointer", who);
  if (r.elem == Elem::f32 && ((reinterpret_cast<uintptr_t>(r.prior) | reinterpret_cast<uintptr_t>(r.post)) & 3u) != 0)
    return fail(EFA_ERR_INVALID, "%s: state pointers must be 4-byte aligned", who);
  if (r.partial_overlap())
    return fail(EFA_ERR_INVALID, "%s: the posterior rows overlap the prior rows without coinciding with them (in place means the same "
                "address: a column's rows are read and written by its own workgroup only)", who);
  return EFA_OK;
}

// the interpolate-and-apply launch of the cycle and of efa_letkf_interp_apply_dev, under the context's relaxation; does not wait
int letkf_interp_launch(efa_ctx* c, const StateRows& r, const LetkfMesh& nodes, long n_lead, const double* Tw, const double* stats,
                        const LetkfGroups* grp) {
  LetkfInterpArgs a{};
  a.mesh = nodes;
  a.n_lead = n_lead;
  a.M = r.M;
  a.Xin = r.prior;
  a.Xout = r.post;
  a.Tw = Tw;
  a.stats = stats;
  a.relax_kind = c->relax_kind;
  a.relax_alpha = c->relax_alpha;
  EFA_HIP(launch_letkf_interp(a, grp, r.elem, c->stream));
  return EFA_OK;
}

// ---- the slab groups --------------------------------------------------------------------------------------------
// Slabs whose factors agree for every ob share one solve.  Decided here from the host copies of the two settings, without the
// table: the key of slab s is the bit pattern of lead_vert[s], lead_time[s] and lead_var[s], each only while that part can give a
// factor other than 1 (some ob carries vertical information; some ob has a time and a temporal half-width; some ob's impact row
// has an entry other than 1).  Equal keys imply equal columns of S.  Groups are numbered by first appearance; cached on the
// settings' serials, the device copy uploaded once per change.
uint64_t letkf_key_bits(double v) {
  if (v != v) return ~(uint64_t)0;  // every NaN is "no coordinate"
  uint64_t b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}

int letkf_groups(efa_ctx* c, long n_lead) {
  if (c->lg_vl_serial == c->vl_serial && c->lg_sl_serial == c->sl_serial && (long)c->lg_group_of.size() == n_lead &&
      c->lg_ptr == c->lg_dev.p && c->lg_dev.p)
    return EFA_OK;
  const bool vert = vl_active(c);
  bool temporal = false, variable = false;
  const double* lt = nullptr;
  const int* lvar = nullptr;
  if (c->sl_on) {
    const long P = c->sl_P, nv = c->sl_nvar, ng = c->sl_ngroup;
    const double* d = c->sl_host.data();
    const int* iv = reinterpret_cast<const int*>(d + c->sl_nlead + 2 * P + ng * nv);
    lt = d;
    lvar = iv;
    for (long k = 0; k < P && !temporal; ++k) temporal = d[c->sl_nlead + k] == d[c->sl_nlead + k] && d[c->sl_nlead + P + k] == d[c->sl_nlead + P + k];
    for (long k = 0; k < P && !variable; ++k) {
      const int g = iv[c->sl_nlead + k];
      if (g < 0) continue;
      for (long u = 0; u < nv && !variable; ++u) variable = d[c->sl_nlead + 2 * P + g * nv + u] != 1.0;
    }
  }
  std::map<std::tuple<uint64_t, uint64_t, int>, int> seen;
  std::vector<int> group_of((size_t)n_lead), rep;
  for (long sidx = 0; sidx < n_lead; ++sidx) {
    const auto key = std::make_tuple(vert ? letkf_key_bits(c->vl_host[sidx]) : (uint64_t)0, temporal ? letkf_key_bits(lt[sidx]) : (uint64_t)0,
                                     variable ? lvar[sidx] : 0);
    auto it = seen.find(key);
    if (it == seen.end()) {
      it = seen.emplace(key, (int)rep.size()).first;
      rep.push_back((int)sidx);
    }
    group_of[sidx] = it->second;
  }
  const int ng = (int)rep.size();
  std::vector<int> h((size_t)(2 * ng + 1 + n_lead));  // rep | grp_off | grp_leads
  std::vector<int> count((size_t)ng, 0);
  for (long sidx = 0; sidx < n_lead; ++sidx) count[group_of[sidx]]++;
  for (int g = 0; g < ng; ++g) {
    h[g] = rep[g];
    h[ng + g + 1] = h[ng + g] + count[g];
  }
  std::vector<int> fill((size_t)ng, 0);
  for (long sidx = 0; sidx < n_lead; ++sidx) {
    const int g = group_of[sidx];
    h[2 * ng + 1 + h[ng + g] + fill[g]++] = (int)sidx;
  }
  EFA_TRY(c->lg_dev.reserve(h.size() * sizeof(int)));
  EFA_HIP(hipMemcpyAsync(c->lg_dev.p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  EFA_HIP(hipStreamSynchronize(c->stream));  // (h goes out of scope)
  c->lg_group_of.swap(group_of);
  c->lg_ngroups = ng;
  c->lg_vl_serial = c->vl_serial;
  c->lg_sl_serial = c->sl_serial;
  c->lg_ptr = c->lg_dev.p;
  return EFA_OK;
}

// the table and the groups of a slab call, as the kernels take them (the settings were checked for this P and n_lead)
int letkf_slab_groups(efa_ctx* c, long n_lead, LetkfGroups* out) {
  EFA_TRY(ensure_slab_table(c));
  EFA_TRY(letkf_groups(c, n_lead));
  const int* d = c->lg_dev.as<int>();
  const int ng = c->lg_ngroups;
  *out = LetkfGroups{ng, n_lead, c->sl_tab.as<double>(), d, d + ng, d + 2 * ng + 1};
  return EFA_OK;
}

// the public entry a cycle speaks for in its messages
const char* letkf_cycle_name(bool slab, bool mesh, bool f32) {
  static const char* const names[8] = {"efa_letkf_cycle_dev",        "efa_letkf_cycle_f32_dev",
                                       "efa_letkf_cycle_interp_dev", "efa_letkf_cycle_interp_f32_dev",
                                       "efa_letkf_slab_cycle_dev",   "efa_letkf_slab_cycle_f32_dev",
                                       "efa_letkf_slab_cycle_interp_dev", "efa_letkf_slab_cycle_interp_f32_dev"};
  return names[4 * slab + 2 * mesh + f32];
}

}  // namespace

int letkf_cycle(efa_ctx* c, const StateRows& r, long P, const double* ym_dev, const double* Yp_dev, const ObsIn& ob, double* ym_out,
                double* Yp_out, const double* grid_lat, const double* grid_lon, long ncol, long n_lead, const DiagOut& diag,
                double* col_stats_dev, const LetkfMesh* mesh, bool slab) {
  const long rows = r.rows;
  const int M = r.M;
  const char* who = letkf_cycle_name(slab, mesh != nullptr, r.elem == Elem::f32);
  EFA_TRY(letkf_check_settings(c, who, M, P, slab, n_lead));
  EFA_TRY(letkf_check_control(c, who, mesh == nullptr, rows, P));
  LetkfMesh nodes{};
  if (mesh) {
    EFA_TRY(letkf_check_mesh(who, *mesh, &nodes));
    ncol = nodes.ncol();
    if (mesh->unit()) mesh = nullptr;  // every column is a node: the plain call, bit for bit (col_stats_dev: the nodes are the columns)
  }
  EFA_TRY(letkf_check_rows(who, r));
  if (rows > 0) EFA_TRY(check_grid(EFA_LOC_GC, grid_lat, grid_lon, ncol, n_lead, rows));
  EFA_TRY(letkf_check_obs(who, P, ym_dev, Yp_dev, ob));
  EFA_TRY(letkf_check_cap(c, who, !slab, P, rows > 0 ? (mesh ? nodes.nnodes() : ncol) : -1));
  EFA_TRY(letkf_check_cv(c, who, slab, M, rows > 0 ? (mesh ? nodes.nnodes() : ncol) : -1));
  // under cross validation the state is always "solve the points, then apply their pairs": without a mesh on the
  // unit mesh of one row whose nodes are the columns (a column then takes its own node's pair with the weight 1.0)
  const bool cv = c->cv_on;
  if (cv && !mesh) nodes = LetkfMesh{1, ncol, 1, 1};
  const bool paired = mesh != nullptr || cv;
  if (c->li_field) {  // one factor per solve: per (group,) column or node
    long nsolve = -1;
    if (rows > 0) {
      if (slab) EFA_TRY(letkf_groups(c, n_lead));
      nsolve = (slab ? (long)c->lg_ngroups : 1) * (mesh ? nodes.nnodes() : ncol);
    }
    EFA_TRY(letkf_check_inflation(c, who, P, nsolve, true));
  }
  hipStream_t s = c->stream;
  harvest_obs_ms(c);
  harvest_state_ms(c);
  c->obs_ms = c->state_ms = 0.0;
  c->state_launches = 0;
  c->phase_a_kind = slab ? (mesh ? 9 : 8) : (mesh ? 7 : 6);
  c->path_taken = EFA_PATH_TRANSFORM;
  if (c->timing) EFA_HIP(hipEventRecord(c->obs_iv.begin, s));

  // ---- the obs: flags and prior diagnostics, then the obs block as P more one-row columns, each solved at its own position ------
  LetkfObs o;
  LetkfLists lists;
  double *Yw = nullptr, *ymw = nullptr;
  if (P > 0) {
    EFA_TRY(letkf_stage_obs(c, M, P, ym_dev, Yp_dev, ob, &o));
    EFA_TRY(c->letkf_Yw.reserve(((size_t)P * M + (size_t)P) * sizeof(double)));
    Yw = c->letkf_Yw.as<double>();
    ymw = Yw + (size_t)P * M;
    EFA_TRY(letkf_build_lists(c, P, o.lat, o.lon, o, &lists));
    if (slab) {  // the obs-obs factors F(j, k) into the lists' tapers; the perturbation-form launch then runs as it is, one group
      const bool vert = vl_active(c);
      const SlabObs so = sl_active(c) ? sl_obs(c, 0) : SlabObs{};
      EFA_HIP(launch_letkf_obs_factor(P, lists.off, lists.cnt, lists.idx, c->letkf_wts.as<double>(), vert ? vl_obvert(c) : nullptr,
                                      vert ? vl_obvhw(c) : nullptr, sl_active(c) ? &so : nullptr, s));
    }
    LetkfArgs a = letkf_args(M, P, lists, Yp_dev, o);
    a.ym_in = ym_dev;
    a.Yp_in = Yp_dev;
    a.ym_out = ymw;
    a.Yp_out = Yw;
    if (cv) {  // every ob's own recentred [T | w] into the context's buffer, its row mapped behind it by the same workgroup
      if (c->cv_Tw.reserve((size_t)P * M * (M + 1) * sizeof(double)) != EFA_OK)
        return fail(EFA_ERR_ALLOC, "%s: the obs block's pair buffer of %ld x %d x %d doubles could not be allocated", who, P, M, M + 1);
      a.Tw = c->cv_Tw.as<double>();
      LetkfCv cva{};
      EFA_TRY(letkf_cv_args(c, M, P, nullptr, &cva));
      EFA_HIP(launch_letkf_cv(a, cva, s));
    } else {
      letkf_args_inflation(c, &a, true);
      letkf_args_control(c, &a, o, true);
      EFA_HIP(launch_letkf(a, nullptr, kLetkfPerts, Elem::f64, s));
    }
    EFA_HIP(launch_etkf_post(P, M, Yw, ymw, o.post_mean, o.post_var, s));
  }
  // ---- the state: the grid's lists (the obs' are consumed: the stream is in order), then ONE launch -----------------------------
  //      (with a mesh: the nodes' lists, then the node solve and the interpolate-and-apply launch)
  LetkfLists glists;
  const long nnodes = paired ? nodes.nnodes() : 0;
  double* node_stats = col_stats_dev;
  LetkfGroups groups{};
  if (rows > 0 && slab) EFA_TRY(letkf_slab_groups(c, n_lead, &groups));
  const LetkfGroups* grp = (rows > 0 && slab) ? &groups : nullptr;
  const size_t ngr = slab ? (size_t)groups.ngroups : 1;  // solves per column or node
  if (rows > 0 && paired) {
    if (c->letkf_Tw.reserve(ngr * (size_t)nnodes * M * (M + 1) * sizeof(double)) != EFA_OK)
      return fail(EFA_ERR_ALLOC, "%s: the node-pair buffer of %zu groups x %ld nodes x %d x %d doubles could not be allocated", who, ngr,
                  nnodes, M, M + 1);
    if (!node_stats) {  // the apply reads n_local of every node
      EFA_TRY(c->letkf_nst.reserve(3 * ngr * (size_t)nnodes * sizeof(double)));
      node_stats = c->letkf_nst.as<double>();
    }
  }
  if (rows > 0 && P > 0) {
    if (mesh) {
      const double *dlat = nullptr, *dlon = nullptr;
      EFA_TRY(letkf_upload_nodes(c, nodes, grid_lat, grid_lon, &dlat, &dlon));
      EFA_TRY(letkf_build_lists(c, nnodes, dlat, dlon, o, &glists, c->oc_reach));
    } else {
      EFA_TRY(c->grid.upload(s, grid_lat, grid_lon, ncol));
      EFA_TRY(letkf_build_lists(c, ncol, c->grid.lat.as<double>(), c->grid.lon.as<double>(), o, &glists, c->oc_reach));
    }
  } else if (rows > 0 && c->oc_on && c->oc_reach) {  // (P == 0: no lists, no ob reaches a point)
    EFA_HIP(hipMemsetAsync(c->oc_reach, 0, (size_t)c->oc_nsolve * sizeof(double), s));
  }
  if (c->timing) {
    EFA_HIP(hipEventRecord(c->obs_iv.end, s));
    c->obs_ends_at = c->obs_iv.end;
    c->obs_iv.pending = true;
    EFA_HIP(hipEventRecord(c->state_iv[0].begin, s));
  }
  if (rows > 0 && paired) {  // (P == 0: no lists, every node has the pair (I, 0) and no column changes)
    EFA_TRY(letkf_solve_points(c, M, nnodes, glists, Yp_dev, o, grp, c->letkf_Tw.as<double>(), node_stats));
    EFA_TRY(letkf_interp_launch(c, r, nodes, n_lead, c->letkf_Tw.as<double>(), node_stats, grp));
    c->state_launches = 2;
  } else if (rows > 0) {
    LetkfArgs a = letkf_args(M, ncol, glists, Yp_dev, o);  // (P == 0: no lists, every column keeps its rows)
    a.n_lead = n_lead;
    a.Xin = r.prior;
    a.Xout = r.post;
    a.stats = col_stats_dev;
    a.relax_kind = c->relax_kind;
    a.relax_alpha = c->relax_alpha;
    letkf_args_inflation(c, &a, false);
    letkf_args_control(c, &a, o, false);
    EFA_HIP(launch_letkf(a, grp, kLetkfMembers, r.elem, s));
    if (c->lc_xc && !a.dc && c->lc_xc_post != c->lc_xc)  // (P == 0: the control keeps its rows as every column does)
      EFA_HIP(hipMemcpyAsync(c->lc_xc_post, c->lc_xc, (size_t)rows * sizeof(double), hipMemcpyDeviceToDevice, s));
    c->state_launches = 1;
  }
  if (c->timing) {
    EFA_HIP(hipEventRecord(c->state_iv[0].end, s));
    c->state_iv[0].pending = true;
  }
  c->state_launches_sum += c->state_launches;
  // ---- the posterior obs block to the caller, behind every solve that read the prior one; the diagnostics ----------------------
  std::vector<char> hd;
  if (P > 0) {
    if (Yp_out) {
      EFA_HIP(hipMemcpyAsync(Yp_out, Yw, (size_t)P * M * sizeof(double), hipMemcpyDeviceToDevice, s));
      EFA_HIP(hipMemcpyAsync(ym_out, ymw, (size_t)P * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    hd.resize(o.diag_bytes());
    EFA_HIP(hipMemcpyAsync(hd.data(), o.prior_mean, hd.size(), hipMemcpyDeviceToHost, s));
  }
  EFA_HIP(hipStreamSynchronize(s));
  if (P > 0) {
    const size_t dP = (size_t)P * sizeof(double);
    const double* pm = reinterpret_cast<const double*>(hd.data() + 2 * dP);
    const double* pv = reinterpret_cast<const double*>(hd.data() + 3 * dP);
    const uint8_t* as = reinterpret_cast<const uint8_t*>(hd.data() + 4 * dP);
    if (diag.prior_mean) std::memcpy(diag.prior_mean, hd.data(), dP);
    if (diag.prior_var) std::memcpy(diag.prior_var, hd.data() + dP, dP);
    for (long k = 0; k < P; ++k) {
      if (diag.assimilated) diag.assimilated[k] = as[k];
      if (as[k]) {
        if (diag.post_mean) diag.post_mean[k] = pm[k];
        if (diag.post_var) diag.post_var[k] = pv[k];
      }
    }
  }
  if (c->timing == 1) {
    harvest_obs_ms(c);
    harvest_state_ms(c);
  }
  return EFA_OK;
}

int letkf_weights(efa_ctx* c, int M, long P, const double* ym_dev, const double* Yp_dev, const ObsIn& ob, long npts, const double* pt_lat,
                  const double* pt_lon, double* Tw_dev, double* stats_dev, bool slab) {
  const char* who = slab ? "efa_letkf_slab_weights_dev" : "efa_letkf_weights_dev";
  const long n_lead = c->sl_on ? c->sl_nlead : c->vl_nlead;  // (slab: the slabs are the settings' own)
  EFA_TRY(letkf_check_settings(c, who, M, P, slab, slab ? n_lead : -1));
  EFA_TRY(letkf_check_control(c, who, false, 0, P));
  if (npts < 0) return fail(EFA_ERR_INVALID, "%s: negative point count", who);
  if (npts > 0 && (!pt_lat || !pt_lon || !Tw_dev)) return fail(EFA_ERR_INVALID, "%s: null point or output array", who);
  EFA_TRY(letkf_check_obs(who, P, ym_dev, Yp_dev, ob));
  EFA_TRY(letkf_check_cap(c, who, !slab, P, npts));
  EFA_TRY(letkf_check_cv(c, who, slab, M, npts));
  if (npts == 0) return EFA_OK;
  if (c->li_field) {
    if (slab) EFA_TRY(letkf_groups(c, n_lead));
    EFA_TRY(letkf_check_inflation(c, who, P, (slab ? (long)c->lg_ngroups : 1) * npts, false));
  }
  hipStream_t s = c->stream;
  LetkfObs o;
  LetkfLists lists;
  if (P > 0) {
    const double *dlat = nullptr, *dlon = nullptr;
    EFA_TRY(letkf_stage_obs(c, M, P, ym_dev, Yp_dev, ob, &o));
    EFA_TRY(letkf_upload_points(c, npts, pt_lat, pt_lon, &dlat, &dlon));
    EFA_TRY(letkf_build_lists(c, npts, dlat, dlon, o, &lists, c->oc_reach));
  } else if (c->oc_on && c->oc_reach) {
    EFA_HIP(hipMemsetAsync(c->oc_reach, 0, (size_t)c->oc_nsolve * sizeof(double), s));
  }
  LetkfGroups groups{};
  if (slab) EFA_TRY(letkf_slab_groups(c, n_lead, &groups));
  EFA_TRY(letkf_solve_points(c, M, npts, lists, Yp_dev, o, slab ? &groups : nullptr, Tw_dev, stats_dev));
  EFA_HIP(hipStreamSynchronize(s));
  return EFA_OK;
}

int letkf_slab_group_table(efa_ctx* c, long n_lead, int* group_of, int* ngroups) {
  const char* who = "efa_letkf_slab_groups";
  if (!c->vl_on && !c->sl_on) return fail(EFA_ERR_INVALID, "%s: neither vertical nor slab localisation is set", who);
  if ((c->vl_on && c->vl_nlead != n_lead) || (c->sl_on && c->sl_nlead != n_lead))
    return fail(EFA_ERR_INVALID, "%s: the settings are not sized for n_lead=%ld", who, n_lead);
  if (c->vl_on && c->sl_on && c->vl_P != c->sl_P)
    return fail(EFA_ERR_INVALID, "%s: the vertical and the slab setting are sized for %ld and %ld observations", who, c->vl_P, c->sl_P);
  EFA_TRY(letkf_groups(c, n_lead));
  if (group_of) std::memcpy(group_of, c->lg_group_of.data(), (size_t)n_lead * sizeof(int));
  if (ngroups) *ngroups = c->lg_ngroups;
  return EFA_OK;
}

int letkf_interp_apply(efa_ctx* c, const StateRows& r, const LetkfMesh& mesh, long n_lead, const double* Tw_nodes_dev,
                       const double* node_stats_dev) {
  const char* who = r.elem == Elem::f32 ? "efa_letkf_interp_apply_f32_dev" : "efa_letkf_interp_apply_dev";
  EFA_TRY(letkf_check_settings(c, who, r.M, 0));
  LetkfMesh nodes{};
  EFA_TRY(letkf_check_mesh(who, mesh, &nodes));
  EFA_TRY(letkf_check_rows(who, r));
  if (r.rows == 0) return EFA_OK;
  if (n_lead < 1 || r.rows != n_lead * nodes.ncol())
    return fail(EFA_ERR_INVALID, "%s: rows=%ld is not n_lead=%ld times the grid's %ld columns", who, r.rows, n_lead, nodes.ncol());
  if (!Tw_nodes_dev) return fail(EFA_ERR_INVALID, "%s: null node pairs", who);
  EFA_TRY(letkf_interp_launch(c, r, nodes, n_lead, Tw_nodes_dev, node_stats_dev, nullptr));
  EFA_HIP(hipStreamSynchronize(c->stream));
  return EFA_OK;
}

}  // namespace efa_host
