// node_rccl.h -- part of node.cpp: RCCL loaded on first use, the error macros of the node's files, and the communicator
// for ranks that are processes (include/sipnet_amd.h: sipnet_comm_*).
#pragma once

namespace {

struct Rccl {
  void* handle = nullptr;
  decltype(&ncclCommInitAll) commInitAll = nullptr;
  decltype(&ncclCommDestroy) commDestroy = nullptr;
  decltype(&ncclAllGather) allGather = nullptr;
  decltype(&ncclGroupStart) groupStart = nullptr;
  decltype(&ncclGroupEnd) groupEnd = nullptr;
  decltype(&ncclGetErrorString) errorString = nullptr;
  decltype(&ncclGetVersion) getVersion = nullptr;
  decltype(&ncclGetUniqueId) getUniqueId = nullptr;     // (sipnet_comm_*: ranks that are processes)
  decltype(&ncclCommInitRank) commInitRank = nullptr;
  std::string path;
};

Rccl* loadRccl() {
  static Rccl r;
  static bool tried = false;
  if (tried) return r.handle ? &r : nullptr;
  tried = true;
  const char* names[] = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
  for (const char* n : names) {
    r.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (r.handle) {
      r.path = n;
      break;
    }
  }
  if (!r.handle) return nullptr;
#define RCCL_SYM(field, name)                                         \
  r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.handle, name)); \
  if (!r.field) {                                                     \
    r.handle = nullptr;                                               \
    return nullptr;                                                   \
  }
  RCCL_SYM(commInitAll, "ncclCommInitAll")
  RCCL_SYM(commDestroy, "ncclCommDestroy")
  RCCL_SYM(allGather, "ncclAllGather")
  RCCL_SYM(groupStart, "ncclGroupStart")
  RCCL_SYM(groupEnd, "ncclGroupEnd")
  RCCL_SYM(errorString, "ncclGetErrorString")
  RCCL_SYM(getVersion, "ncclGetVersion")
  RCCL_SYM(getUniqueId, "ncclGetUniqueId")
  RCCL_SYM(commInitRank, "ncclCommInitRank")
#undef RCCL_SYM
  return &r;
}

}  // namespace

// a HIP or RCCL call that must succeed: otherwise "<prefix><the call as written>: <the library's text for its status>" and
// SIPNET_ERR_NO_DEVICE
#define CALL_TRY(prefix, call, expr, ok, textOf)                          \
  do {                                                                    \
    const auto e_ = (expr);                                               \
    if (e_ != (ok)) {                                                     \
      setError(std::string(prefix) + call + ": " + textOf(e_));           \
      return SIPNET_ERR_NO_DEVICE;                                        \
    }                                                                     \
  } while (0)
#define NODE_HIP(expr) CALL_TRY("sipnet_node: ", #expr, expr, hipSuccess, hipGetErrorString)
#define NODE_RCCL(r, expr) CALL_TRY("sipnet_node: ", #expr, expr, ncclSuccess, (r)->errorString)
#define COMM_RCCL(r, expr) CALL_TRY("sipnet_comm: ", #expr, expr, ncclSuccess, (r)->errorString)
// a buffer's reserve: the node's prefix in front of its error text
#define NODE_BUF(call)                                                        \
  do {                                                                        \
    int rc_ = (call);                                                         \
    if (rc_) {                                                                \
      setError(std::string("sipnet_node: ") + sipnet_last_error());           \
      return rc_;                                                             \
    }                                                                         \
  } while (0)

// ---- a RCCL communicator for ranks that are processes (include/sipnet_amd.h: sipnet_comm_*) -------------------------------
struct sipnet_comm {
  Rccl* rccl = nullptr;
  ncclComm_t comm = nullptr;
  int32_t world = 0, rank = 0, device = 0;
};

extern "C" {

int sipnet_comm_unique_id(uint8_t id[128]) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  Rccl* r = loadRccl();
  if (!id || !r) {
    setError("sipnet_comm_unique_id: no usable RCCL (librccl.so.1)");
    return SIPNET_ERR_NO_DEVICE;
  }
  ncclUniqueId u;
  COMM_RCCL(r, r->getUniqueId(&u));
  memcpy(id, &u, sizeof u);
  return SIPNET_OK;
}
int sipnet_comm_create(const uint8_t id[128], int32_t world, int32_t rank, int32_t device, sipnet_comm** out) {
  if (!id || !out || world < 1 || rank < 0 || rank >= world) {
    setError("sipnet_comm_create: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  Rccl* r = loadRccl();
  if (!r) {
    setError("sipnet_comm_create: no usable RCCL (librccl.so.1)");
    return SIPNET_ERR_NO_DEVICE;
  }
  if (hipSetDevice(device) != hipSuccess) {
    (void)hipGetLastError();
    setError("sipnet_comm_create: no usable HIP device " + std::to_string(device));
    return SIPNET_ERR_NO_DEVICE;
  }
  ncclUniqueId u;
  memcpy(&u, id, sizeof u);
  sipnet_comm* c = new sipnet_comm();
  c->rccl = r;
  c->world = world;
  c->rank = rank;
  c->device = device;
  ncclResult_t nr = r->commInitRank(&c->comm, world, u, rank);
  if (nr != ncclSuccess) {
    setError(std::string("sipnet_comm_create: ncclCommInitRank: ") + r->errorString(nr));
    delete c;
    return SIPNET_ERR_NO_DEVICE;
  }
  *out = c;
  return SIPNET_OK;
}
int sipnet_comm_all_gather(sipnet_comm* c, const void* d_send, void* d_recv, int64_t bytes_per_rank, void* hip_stream) {
  if (!c || !d_send || !d_recv || bytes_per_rank <= 0) {
    setError("sipnet_comm_all_gather: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if (hipSetDevice(c->device) != hipSuccess) {
    (void)hipGetLastError();
    return SIPNET_ERR_NO_DEVICE;
  }
  COMM_RCCL(c->rccl, c->rccl->allGather(d_send, d_recv, (size_t)bytes_per_rank, ncclChar, c->comm, (hipStream_t)hip_stream));
  return SIPNET_OK;
}
int32_t sipnet_comm_world(const sipnet_comm* c) { return c ? c->world : 0; }
void sipnet_comm_destroy(sipnet_comm* c) {
  if (!c) return;
  if (c->comm) (void)c->rccl->commDestroy(c->comm);
  delete c;
}

}  // extern "C"
