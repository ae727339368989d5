// fast_math_probe.hip -- test hook: the helpers of fast_math.h run on their own, one element per thread, compiled
// with the flags of step_fast.o (contraction fast, -fno-honor-nans, the same -D options), so that a test sees the
// polynomial, the Newton steps and the clamps as the throughput kernels get them.  sipnet_debug_fast_math; the
// contract is in include/sipnet_amd.h.  No step kernel source: not part of kernel_source_sha16.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sipnet_amd.h"
#include "fast_math.h"

namespace sipnet {
void setError(const std::string& s);

namespace {

constexpr int kProbeThreads = 256;

// one operation on one element at the precision R of the flux arithmetic: the operands narrowed to R, the
// result widened (RECR: the slot itself goes to recR<R>, which for float takes its low word)
template <class R>
__device__ __forceinline__ double probeOne(int32_t op, double x, double y, const Exp2Coef& EC) {
  switch (op) {
    case SIPNET_FM_EXP2: return (double)fexp2((R)x, EC);
    case SIPNET_FM_DIV: return (double)fdiv((R)x, (R)y);
    case SIPNET_FM_RMINV: return (double)rminv((R)x, (R)y);
    case SIPNET_FM_RMAX0: return (double)rmax0((R)x);
    case SIPNET_FM_CLIP01: return (double)clip01((R)x);
    default: return (double)recR<R>(x);   // SIPNET_FM_RECR
  }
}

template <class R>
__global__ __launch_bounds__(kProbeThreads) void fastMathProbeKernel(int32_t op, int64_t n, const double* __restrict__ x,
                                                                     const double* __restrict__ y,
                                                                     double* __restrict__ out) {
  const Exp2Coef EC = loadExp2Coef();   // as the step kernels obtain it: once, ahead of the work
  const int64_t i = (int64_t)blockIdx.x * kProbeThreads + threadIdx.x;
  if (i >= n) return;
  const double yi = y ? y[i] : 0.0;
  out[i] = probeOne<R>(op, x[i], yi, EC);
}

}  // namespace
}  // namespace sipnet

using namespace sipnet;

extern "C" int sipnet_debug_fast_math(int32_t op, int32_t prec, int64_t n, const double* d_x, const double* d_y,
                                      double* d_out, int32_t info[2]) {
  const char* fn = "sipnet_debug_fast_math";
  auto refuse = [&](const char* why) {
    setError(std::string(fn) + ": " + why);
    return (int)SIPNET_ERR_BAD_ARGUMENT;
  };
  if (op < SIPNET_FM_EXP2 || op > SIPNET_FM_RECR) return refuse("an unknown operation");
  if (prec != SIPNET_F64 && prec != SIPNET_F32_MIXED) return refuse("an unknown precision");
  if (n < 0) return refuse("a negative length");
  if (n > ((int64_t)1 << 31)) return refuse("more than 2^31 elements");
  if (n > 0 && (!d_x || !d_out)) return refuse("a NULL array");
  if (n > 0 && !d_y && (op == SIPNET_FM_DIV || op == SIPNET_FM_RMINV)) return refuse("a NULL second operand");
  if (info) {
    info[0] = SIPNET_EXP2_DEGREE;
    info[1] = SIPNET_FDIV_NEWTON;
  }
  if (n == 0) return SIPNET_OK;
  const unsigned grid = (unsigned)((n + kProbeThreads - 1) / kProbeThreads);
  if (prec == SIPNET_F64)
    hipLaunchKernelGGL(fastMathProbeKernel<double>, dim3(grid), dim3(kProbeThreads), 0, nullptr, op, n, d_x, d_y, d_out);
  else
    hipLaunchKernelGGL(fastMathProbeKernel<float>, dim3(grid), dim3(kProbeThreads), 0, nullptr, op, n, d_x, d_y, d_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    setError(std::string(fn) + ": " + hipGetErrorString(e));
    return SIPNET_ERR_NO_DEVICE;
  }
  return SIPNET_OK;
}
