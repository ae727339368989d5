// dev_buf.h -- the one owner of device and pinned-host memory: a pointer, its capacity in elements, grow-only.
//   DevBuf<T>: hipMalloc / hipFree;  PinnedBuf<T>: hipHostMalloc / hipHostFree.
// reserve() never waits for a stream or an event: a block that the device may still be using is the CALLER's to wait
// for, before the call (test `count > buf.capacity()` first where the wait is wanted only when the block grows).
// The destructor frees, with whatever device is current: the owners select theirs before they delete the object, and
// nothing of these types is a static or a thread_local object itself (a destructor at thread exit or at static
// destruction could run after the HIP runtime is gone) -- such scratch hangs off a raw pointer that is deleted explicitly.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/sipnet_amd.h"

namespace sipnet {
void setError(const std::string& s);

// bytes held right now by all buffers of the process (sipnet_debug_live_bytes)
inline std::atomic<int64_t> g_liveDeviceBytes{0}, g_livePinnedBytes{0};

struct DeviceMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return hipFree(p); }
  static std::atomic<int64_t>& live() { return g_liveDeviceBytes; }
  static const char* allocExpr() { return "hipMalloc(&ptr, count * sizeof(T))"; }
  static const char* freeExpr() { return "hipFree(ptr)"; }
};
struct PinnedMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static hipError_t free(void* p) { return hipHostFree(p); }
  static std::atomic<int64_t>& live() { return g_livePinnedBytes; }
  static const char* allocExpr() { return "hipHostMalloc(&ptr, count * sizeof(T), hipHostMallocDefault)"; }
  static const char* freeExpr() { return "hipHostFree(ptr)"; }
};

template <class T, class Mem>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      (void)release();
      p_ = o.p_;
      cap_ = o.cap_;
      o.p_ = nullptr;
      o.cap_ = 0;
    }
    return *this;
  }
  ~Buf() { (void)release(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }   // elements

  // free if set, then clear (may be called again)
  hipError_t release() {
    if (!p_) return hipSuccess;
    const hipError_t e = Mem::free(p_);
    Mem::live() -= (int64_t)(cap_ * sizeof(T));
    p_ = nullptr;
    cap_ = 0;
    return e;
  }
  // room for `count` elements: nothing if it is there, otherwise the old block goes and a block of exactly `count` comes
  // (its contents are not kept; a failure leaves the buffer empty).  *grew: the block is a fresh one.
  // tryReserve: the HIP status, for callers that word their own error; *failedExpr: the call that failed.
  hipError_t tryReserve(size_t count, bool* grew = nullptr, const char** failedExpr = nullptr) {
    if (grew) *grew = false;
    if (count <= cap_) return hipSuccess;
    if (failedExpr) *failedExpr = Mem::freeExpr();
    hipError_t e = release();
    if (e != hipSuccess) return e;
    if (failedExpr) *failedExpr = Mem::allocExpr();
    e = Mem::alloc((void**)&p_, count * sizeof(T));
    if (e != hipSuccess) {
      p_ = nullptr;
      return e;
    }
    cap_ = count;
    Mem::live() += (int64_t)(count * sizeof(T));
    if (grew) *grew = true;
    return hipSuccess;
  }
  // reserve: the project's status, and the error text of HIP_TRY
  int reserve(size_t count, bool* grew = nullptr) {
    const char* expr = "";
    const hipError_t e = tryReserve(count, grew, &expr);
    if (e == hipSuccess) return SIPNET_OK;
    setError(std::string(expr) + ": " + hipGetErrorString(e));
    return SIPNET_ERR_NO_DEVICE;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using PinnedBuf = Buf<T, PinnedMem>;

}  // namespace sipnet

// `call` returns the project's status (a reserve): leave with it unless it is SIPNET_OK
#define RC_TRY(call)       \
  do {                     \
    int rc_ = (call);      \
    if (rc_) return rc_;   \
  } while (0)
