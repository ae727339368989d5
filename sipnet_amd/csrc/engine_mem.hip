// engine_mem.hip -- device memory, copies and streams for callers of include/sipnet_amd.h that have no HIP runtime of their own.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sipnet_amd.h"
#include "batch_impl.h"

// rows of 8-byte words, pitches in words (sipnet_dev_to_dev_2d)
__global__ __launch_bounds__(256) void copyRows8Kernel(uint64_t* __restrict__ dst, size_t dstPitch, const uint64_t* __restrict__ src,
                                                       size_t srcPitch, size_t width, size_t rows) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= width) return;
  for (size_t r = blockIdx.y; r < rows; r += gridDim.y) dst[r * dstPitch + c] = src[r * srcPitch + c];
}

extern "C" {

void* sipnet_dev_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    setError("sipnet_dev_alloc: hipMalloc failed");
    return nullptr;
  }
  return p;
}
void sipnet_dev_free(void* p) {
  if (p) (void)hipFree(p);
}
int sipnet_dev_to_host(void* host, const void* dev, size_t bytes, void* hip_stream) {
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  HIP_TRY(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
  return SIPNET_OK;
}
int sipnet_dev_to_host_2d(void* host, size_t host_pitch, const void* dev, size_t dev_pitch, size_t width_bytes, size_t rows,
                          void* hip_stream) {
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  HIP_TRY(hipMemcpy2D(host, host_pitch, dev, dev_pitch, width_bytes, rows, hipMemcpyDeviceToHost));
  return SIPNET_OK;
}
int sipnet_dev_to_dev_2d(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width_bytes, size_t rows,
                         void* hip_stream) {
  if (!dst || !src || rows == 0 || width_bytes == 0) {
    setError("sipnet_dev_to_dev_2d: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  // a kernel of our own for the case that matters (8-byte elements): the runtime's 2-D copy moved 17 520 rows of 80 KB at
  // 0.5 GB/s (3 s per column of c10k's record), this streams them at the HBM rate
  if (((width_bytes | dst_pitch | src_pitch | (size_t)(uintptr_t)dst | (size_t)(uintptr_t)src) & 7) == 0) {
    const size_t w8 = width_bytes / 8;
    const dim3 grid((unsigned)((w8 + 255) / 256), (unsigned)(rows < 65535 ? rows : 65535));
    hipLaunchKernelGGL(copyRows8Kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, (uint64_t*)dst, dst_pitch / 8,
                       (const uint64_t*)src, src_pitch / 8, w8, rows);
    HIP_TRY(hipGetLastError());
    return SIPNET_OK;
  }
  HIP_TRY(hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, width_bytes, rows, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  return SIPNET_OK;
}
int sipnet_stream_sync(void* hip_stream) {
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  return SIPNET_OK;
}
void* sipnet_stream_create(int32_t device) {
  hipStream_t s = nullptr;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
    setError("sipnet_stream_create: hipStreamCreate failed");
    return nullptr;
  }
  return (void*)s;
}
void sipnet_stream_destroy(void* hip_stream) {
  if (hip_stream) (void)hipStreamDestroy((hipStream_t)hip_stream);
}

}  // extern "C"
