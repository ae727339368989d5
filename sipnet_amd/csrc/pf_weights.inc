// pf_weights.inc -- the analysis as launches of their own: log-weights from an output plane and their block maxima
// (logWeightOf, logWeightKernel, blockFromWaveMaximaKernel, maxPartialKernel), THE fixed-point weight (pfFixedWeight) and the
// kernels that apply it to one batch's log-weights or to the ranks' gathered blocks (fixedWeightKernel,
// fixedWeightGatheredKernel; the blocks' layout: PeerPtrs, pf_gather.inc), the systematic draw over a prefix sum (ancestorKernel).

// logw[col] = -0.5 * ((sum_t plane[t][col] - obs) / sigma)^2, -inf for members that did not run
// (AgentStore: the log-weight is written through to device scope -- pfFusedKernel's phase 3 reads it from other workgroups,
// possibly on another XCD, inside the same launch)
template <typename T, bool AgentStore = false>
__device__ __forceinline__ double logWeightOf(const T* __restrict__ plane, int32_t nSteps, int64_t ld, int64_t c,
                                              const double* __restrict__ status, double obs, double invSigma,
                                              double* __restrict__ logw) {
  // the sum in step order; eight loads in flight at a time (one dependent load per step left the kernel
  // latency-bound: 25 MB in 14.7 us at C5's shape)
  double acc = 0.0;
  int t = 0;
  for (; t + 8 <= nSteps; t += 8) {
    T v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = plane[(int64_t)(t + k) * ld + c];
#pragma unroll
    for (int k = 0; k < 8; k++) acc += (double)v[k];
  }
  for (; t < nSteps; t++) acc += (double)plane[(int64_t)t * ld + c];
  const double z = (acc - obs) * invSigma;
  const double lw = (status[c] != 0.0) ? -INFINITY : -0.5 * z * z;
  if (AgentStore) __hip_atomic_store(&logw[c], lw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else logw[c] = lw;
  return lw;
}
// (part, if given: the block's maximum -- what maxPartialKernel would compute in a launch of its own)
template <typename T>
__global__ __launch_bounds__(256) void logWeightKernel(const T* __restrict__ plane, int32_t nSteps,
                                                       int64_t ld, int64_t ncol,
                                                       const double* __restrict__ status,
                                                       double obs, double invSigma,
                                                       double* __restrict__ logw, double* __restrict__ part,
                                                       int64_t npad) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double mine = -INFINITY;
  if (c < ncol) mine = logWeightOf(plane, nSteps, ld, c, status, obs, invSigma, logw);
  else if (c < npad) logw[c] = -INFINITY;   // slots of a rank's block no particle fills (ragged shards): weight zero
  if (part) {
    __shared__ double sm[256];
    sm[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
      __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
  }
}
// the same block (256-wide maxima behind the log-weights, -inf in the slots no particle fills) when the forecast's own launch
// has left the log-weights in place and one maximum per 64 columns (FastArgs::pfLogw): four of those per entry
__global__ __launch_bounds__(256) void blockFromWaveMaximaKernel(const double* __restrict__ waveMax, int64_t nWaves, int64_t ncol,
                                                               int64_t npad, double* __restrict__ logw, double* __restrict__ part) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nPart = (npad + 255) / 256;
  if (i < nPart) {
    double m = -INFINITY;
    for (int k = 0; k < 4; k++)
      if (4 * i + k < nWaves) m = fmax(m, waveMax[4 * i + k]);
    part[i] = m;
  }
  if (ncol + i < npad) logw[ncol + i] = -INFINITY;
}
// (the scratch blocks are freed by sipnet_pf_release_scratch, not by a thread-exit destructor: that
// may run after the HIP runtime has shut down)

// max of the log-weights: per-block partial maxima (the consumer, fixedWeightKernel, takes their maximum)
__global__ __launch_bounds__(256) void maxPartialKernel(const double* __restrict__ x, int64_t n,
                                                        double* __restrict__ part) {
  __shared__ double sm[256];
  double m = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    m = fmax(m, x[i]);
  sm[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}

// THE fixed-point weight of a log-weight lw under the maximum m: rint(2^30 exp(lw - m)), 0 for a particle that did not run
// (-inf) or a filter none of whose particles did.  Every device path takes it from here -- the separate-launch kernels, the
// one-launch analysis, one rank or many -- so that they agree to the bit (the numpy oracle's glibc exp may round a weight
// to the neighbouring integer; the tests allow that one unit and resample the DEVICE's integers exactly).
// 2^30 e^x = 2^(30 + x log2 e): n = rint(y), 2^(y - n) by the degree-11 interpolant of fast_math.h (|rel err| <= 1.7e-16),
// one v_ldexp -- a fifth of OCML's exp() + llrint(), which was what grew with the number of ranks: 8 x 131 072 slots cost
// every wavefront eight of them (7.9 us of the analysis launch, profiles/r06_pf_analysis_phases.txt).
__device__ __forceinline__ long long pfFixedWeight(double lw, double m) {
  const double x = lw - m;                  // <= 0 (NaN when both are -inf)
  if (!(x >= -21.5)) return 0;              // 2^30 e^x < 0.5 below that; also lw = -inf, m = -inf (NaN), NaN weights
  const double y = x * 1.4426950408889634074;
  const double n = __builtin_rint(y), f = y - n;
  double p = 4.4549605981865186e-10;
  p = __builtin_fma(p, f, 7.072585949269223e-09);
  p = __builtin_fma(p, f, 1.0178062445845774e-07);
  p = __builtin_fma(p, f, 1.321544258792169e-06);
  p = __builtin_fma(p, f, 1.525273382983612e-05);
  p = __builtin_fma(p, f, 0.0001540353044173605);
  p = __builtin_fma(p, f, 0.0013333558146416936);
  p = __builtin_fma(p, f, 0.009618129107606888);
  p = __builtin_fma(p, f, 0.0555041086648216);
  p = __builtin_fma(p, f, 0.24022650695910097);
  p = __builtin_fma(p, f, 0.6931471805599453);
  p = __builtin_fma(p, f, 1.0);
  return (long long)(int)__builtin_rint(__builtin_amdgcn_ldexp(p, (int)n + 30));   // (<= 2^30: an int)
}

// fixed-point weights: w = rint(exp(logw - max) * 2^30).  Integer weights make the prefix
// sum exact, so every rank computes bit-identical ancestors from the same gathered logw.
// (every block first takes the maximum of the `parts` partial maxima itself: one launch less)
__global__ __launch_bounds__(256) void fixedWeightKernel(const double* __restrict__ logw,
                                                         int64_t n, const double* __restrict__ part, int parts,
                                                         int64_t* __restrict__ w) {
  __shared__ double sm[256];
  double pm = -INFINITY;
  for (int k = threadIdx.x; k < parts; k += 256) pm = fmax(pm, part[k]);
  sm[threadIdx.x] = pm;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  w[i] = pfFixedWeight(logw[i], sm[0]);
}

// ancestor[j] = first slot i with cdf[i] > p_j, p_j = ((j0 + j + u0) * S) / nTotal  (S = cdf[nSlots-1] < 2^53)
// for the nOut particles j0 .. j0 + nOut - 1 of a filter of nTotal particles whose weights sit in nSlots >= nTotal
// slots (one rank: nSlots = nTotal = nOut, j0 = 0; several ranks: a rank resamples its own particles over the
// gathered weights of all, and slots no particle fills weigh nothing)
// (total, if wanted: the total integer weight, for the caller's "a particle survived" check)
__global__ __launch_bounds__(256) void ancestorKernel(const int64_t* __restrict__ cdf, int64_t nSlots, int64_t j0,
                                                      int64_t nOut, int64_t nTotal, double u0,
                                                      int32_t* __restrict__ anc, int64_t* __restrict__ total) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nOut) return;
  if (j == 0 && total) *total = cdf[nSlots - 1];
  const double S = (double)cdf[nSlots - 1];
  // S - 1 keeps the search inside the support when (j + u0) rounds up to n
  const double p = fmin((((double)(j0 + j) + u0) * S) / (double)nTotal, S - 1.0);
  int64_t lo = 0, hi = nSlots - 1;  // invariant: answer in [lo, hi]
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((double)cdf[mid] > p) {
      hi = mid;
    } else {
      lo = mid + 1;
    }
  }
  anc[j] = (int32_t)lo;
}

// fixed-point weights of all slots (fixedWeightKernel over the gathered blocks)
__global__ __launch_bounds__(256) void fixedWeightGatheredKernel(const double* __restrict__ gathered, int32_t world,
                                                                 int32_t nmax, int64_t stride, int64_t* __restrict__ w) {
  __shared__ double sm[256];
  const int P = (nmax + 255) / 256;
  double pm = -INFINITY;
  for (int k = threadIdx.x; k < world * P; k += 256) pm = fmax(pm, gathered[(int64_t)(k / P) * stride + nmax + k % P]);
  sm[threadIdx.x] = pm;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)world * nmax) return;
  w[i] = pfFixedWeight(gathered[(i / nmax) * stride + i % nmax], sm[0]);
}
