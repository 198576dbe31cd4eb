// The multi-GPU exchange step: an RCCL communicator owned by the context, one all-reduce.
#include "efa_driver.h"

#include <dlfcn.h>

#include <cstring>

// ---- RCCL, bound at run time: a single-GPU caller never loads it ---------------------------------------
namespace {
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;
using namespace efa_host;

int rccl_load() {
  if (g_rccl.lib) return EFA_OK;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;
  for (const char* n : names) {
    h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (h) break;
  }
  if (!h) return fail(EFA_ERR_UNSUPPORTED, "librccl could not be opened: %s", dlerror());
  RcclApi a;
  a.lib = h;
  a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
  a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
  a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(h, "ncclAllReduce"));
  a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
  a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
  if (!a.GetUniqueId || !a.CommInitRank || !a.AllReduce || !a.CommDestroy || !a.GetErrorString) {
    dlclose(h);
    return fail(EFA_ERR_UNSUPPORTED, "librccl lacks an expected symbol");
  }
  g_rccl = a;
  return EFA_OK;
}
#define EFA_RCCL(expr)                                                                                       \
  do {                                                                                                       \
    ncclResult_t _r = (expr);                                                                                \
    if (_r != ncclSuccess) return fail(EFA_ERR_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(_r));      \
  } while (0)
}  // namespace

namespace efa_host {
void release_comm(efa_ctx* c) {
  if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
}
}  // namespace efa_host

extern "C" {

// ---- the one exchange step, owned by the library ------------------------------------------
int efa_comm_unique_id(uint8_t* id_out) {
  if (!id_out) return fail(EFA_ERR_INVALID, "null id");
  EFA_TRY(rccl_load());
  static_assert(sizeof(ncclUniqueId) == EFA_COMM_ID_BYTES, "EFA_COMM_ID_BYTES must be sizeof(ncclUniqueId)");
  ncclUniqueId id;
  EFA_RCCL(g_rccl.GetUniqueId(&id));
  std::memcpy(id_out, &id, sizeof(id));
  return EFA_OK;
}

int efa_comm_init(efa_ctx* c, const uint8_t* id, int rank, int world) {
  EFA_TRY(use(c));
  if (!id || world < 1 || rank < 0 || rank >= world) return fail(EFA_ERR_INVALID, "bad communicator arguments (rank %d of %d)", rank, world);
  if (c->comm) return fail(EFA_ERR_INVALID, "the context already owns a communicator (efa_comm_destroy first)");
  EFA_TRY(rccl_load());
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  EFA_RCCL(g_rccl.CommInitRank(&c->comm, world, uid, rank));
  c->comm_rank = rank;
  c->comm_world = world;
  return EFA_OK;
}

int efa_comm_destroy(efa_ctx* c) {
  EFA_TRY(use(c));
  if (!c->comm) return EFA_OK;
  EFA_HIP(hipStreamSynchronize(c->stream));
  EFA_RCCL(g_rccl.CommDestroy(c->comm));
  c->comm = nullptr;
  c->comm_rank = 0;
  c->comm_world = 1;
  return EFA_OK;
}

int efa_allreduce_sum_dev(efa_ctx* c, double* buf_dev, long count) {
  EFA_TRY(use(c));
  if (count < 0 || (count && !buf_dev)) return fail(EFA_ERR_INVALID, "bad buffer");
  if (!c->comm) return fail(EFA_ERR_INVALID, "no communicator: call efa_comm_init first");
  if (count == 0) return EFA_OK;
  EFA_RCCL(g_rccl.AllReduce(buf_dev, buf_dev, (size_t)count, ncclDouble, ncclSum, c->comm, c->stream));
  return EFA_OK;
}

}  // extern "C"
