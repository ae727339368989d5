// node_reduce.h -- part of node.cpp: the kernels of sipnet_node_run_gathering_reduced, which make a segment's reduced block
// from its planes, and their launch.
#pragma once

namespace {
__global__ __launch_bounds__(256) void planesToF32Kernel(const double* __restrict__ src, float* __restrict__ dst, size_t n2) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // pairs (ld is even)
  if (i >= n2) return;
  const double2 v = ((const double2*)src)[i];
  ((float2*)dst)[i] = make_float2((float)v.x, (float)v.y);
}
// out[(v * groups + g) * ld + c] = sum over the steps t of group g, in step order, of plane v's [t][c]   (a thread = a column)
template <typename T>
__global__ __launch_bounds__(256) void sumStepsKernel(const T* __restrict__ planes, size_t planeStride, int32_t rows, int32_t k,
                                                      int32_t groups, int64_t ld, double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ld) return;
  const int g = blockIdx.y, v = blockIdx.z;
  const T* __restrict__ p = planes + (size_t)v * planeStride + (size_t)g * k * ld + c;
  const int cnt = (g + 1) * k <= rows ? k : rows - g * k;
  double acc = 0.0;
  int t = 0;
  for (; t + 8 <= cnt; t += 8) {   // eight loads in flight, added in step order
    T x[8];
#pragma unroll
    for (int q = 0; q < 8; q++) x[q] = p[(size_t)(t + q) * ld];
#pragma unroll
    for (int q = 0; q < 8; q++) acc += (double)x[q];
  }
  for (; t < cnt; t++) acc += (double)p[(size_t)t * ld];
  out[((size_t)v * groups + g) * ld + c] = acc;
}
}  // namespace

// planes [3][len][ld] (doubles, or floats when !f64) -> red on `stream`: SIPNET_GATHER_F32 the same as floats,
// SIPNET_GATHER_SUMS [3][rows][ld] sums over groups of sumSteps steps
static int launchReduce(int32_t form, bool f64, const void* planes, int32_t len, int64_t ld, int32_t sumSteps, int32_t rows,
                        void* red, hipStream_t stream) {
  if (form == SIPNET_GATHER_F32) {
    const size_t n2 = (size_t)3 * len * ld / 2;   // (ld is even)
    hipLaunchKernelGGL(planesToF32Kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, stream, (const double*)planes, (float*)red, n2);
  } else {
    const dim3 grid((unsigned)((ld + 255) / 256), (unsigned)rows, 3);
    if (f64)
      hipLaunchKernelGGL(sumStepsKernel<double>, grid, dim3(256), 0, stream, (const double*)planes, (size_t)len * ld, len, sumSteps, rows, ld, (double*)red);
    else
      hipLaunchKernelGGL(sumStepsKernel<float>, grid, dim3(256), 0, stream, (const float*)planes, (size_t)len * ld, len, sumSteps, rows, ld, (double*)red);
  }
  NODE_HIP(hipGetLastError());
  return SIPNET_OK;
}
