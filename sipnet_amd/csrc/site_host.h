// site_host.h -- the host side that the per-site analyses share (enkf.hip, pf.hip, quantiles.hip): a refusal, the limit on a
// batch's columns, the bookkeeping of a call that writes the batch, a scratch block grown and carved into arrays from one
// description of its layout, the request for dynamic LDS past what a kernel may use unasked, what sipnet_batch_pf_info reports
// of the last call, and the copies of a synchronous form's check.  batch_impl.h stays the batch object and the stream bookkeeping.
#pragma once
#include <string>
#include <vector>

#include "batch_impl.h"

namespace sipnet {

// a refusal: "`name`: `why`" is the thread's error, `code` the status
inline int refuse(const char* name, const std::string& why, int code = SIPNET_ERR_BAD_ARGUMENT) {
  setError(std::string(name) + ": " + why);
  return code;
}

// the columns a batch may have in these calls (4 194 304); every caller words its own refusal
constexpr int64_t kMaxColumns = (int64_t)1 << 22;
inline bool tooManyColumns(const sipnet_batch* b) { return b->ncol > kMaxColumns; }

// An analysis is about to write the batch's state on `stream`: a forecast's log-weights belong to the particles as they
// were, the stream goes behind the batch's last launch, pending parameters are converted; ownRows: and every column gets
// its own parameter rows, because the analysis writes them too.
inline int beginWrite(sipnet_batch* b, hipStream_t stream, bool ownRows) {
  b->pfPre.valid = false;
  b->pfArm.set = false;
  RC_TRY(orderBehindBusy(b, stream));
  RC_TRY(flushParams(b, stream));
  return ownRows ? materializeParams(b, stream) : SIPNET_OK;
}

// A scratch block of the batch with room for `count` elements, as dev_buf.h asks: the host waits for the batch's launches
// before the block grows (the old one may still be read by a launch in flight), and only then.  This block alone: another
// may be in use by this very call.
template <class T>
int growScratch(sipnet_batch* b, DevBuf<T>& block, size_t count) {
  if (block.capacity() >= count) return SIPNET_OK;
  RC_TRY(waitIdle(b));
  return block.reserve(count);
}

// A byte block carved into typed arrays: the layout is written ONCE, as a function that takes its arrays from a Carver in order
// (wider element types first), and carveScratch runs it twice -- to measure, then over the block grown to that size.
struct Carver {
  unsigned char* base;   // null: measure only
  size_t bytes = 0;
  template <class T>
  T* take(size_t count) {
    T* p = base ? (T*)(base + bytes) : nullptr;
    bytes += count * sizeof(T);
    return p;
  }
};
template <class F>
int carveScratch(sipnet_batch* b, DevBuf<unsigned char>& block, F layout) {
  Carver measure{nullptr}, assign{nullptr};
  layout(measure);
  RC_TRY(growScratch(b, block, measure.bytes));
  assign.base = block.get();
  layout(assign);
  return SIPNET_OK;
}

// "A launch of `kernel` may use dynBytes of dynamic LDS": *ok, after the kernel was given the attribute where its static
// and dynamic LDS together pass the 48 KB a kernel may use unasked.  False where they pass the device's maximum or the
// request fails: the caller then keeps in global memory what it wanted in LDS (or takes its other path).
inline int ldsGranted(const void* kernel, size_t dynBytes, int device, bool* ok) {
  int ldsMax = 0;
  hipFuncAttributes attr;
  HIP_TRY(hipDeviceGetAttribute(&ldsMax, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  HIP_TRY(hipFuncGetAttributes(&attr, kernel));
  const size_t total = dynBytes + attr.sharedSizeBytes;
  *ok = total <= (size_t)ldsMax;
  if (*ok && total > 48 * 1024 &&
      hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dynBytes) != hipSuccess) {
    (void)hipGetLastError();
    *ok = false;
  }
  return 0;
}

// what sipnet_batch_pf_info reports of a per-site call: one workgroup per site (fused, grid = the sites) or launches per stage
inline void reportPath(sipnet_batch* b, bool fused, int32_t grid) {
  b->pfInfo.fused = fused ? 1 : 0;
  b->pfInfo.grid = grid;
  b->pfInfo.budget = 0;
  b->pfInfo.nSlots = b->ncol;
}

// a synchronous form's check: n elements at d (null: none) queued for h on `stream`; the caller waits for the stream once
template <class T>
int readBack(std::vector<T>& h, const T* d, size_t n, hipStream_t stream) {
  h.resize(d ? n : 0);
  if (!h.empty()) HIP_TRY(hipMemcpyAsync(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
  return SIPNET_OK;
}

}  // namespace sipnet
