// site_device.h -- the device side that the per-site analyses share (enkf.hip, pf.hip, quantiles.hip and their .inc parts):
// the sums in their one order, a member's physical limits, and the parameter rows that are derived from listed ones.  Plain
// functions and templates, included INSIDE each unit's anonymous namespace like the .inc parts (so no include guard: once per
// unit).  fast_math.h has a kTiny of its own for the step kernels; no unit sees both.
//
// A floating-point sum is always taken in one order: the 256 columns of a chunk by an xor-shuffle butterfly inside each wave
// (waveSum), the four waves in order (combine4: ((w0 + w1) + w2) + w3), the chunks in order from 0.0 (siteSums).
constexpr double kTiny = 0.000001;   // TINY, common/util.h

__device__ __forceinline__ double waveSum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int waveSum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// The sum of an int over the workgroup's 256 threads (ints: any order), to every thread: the four wave totals through smI[4].
// The barrier discipline: ONE barrier, between the totals' stores and their loads.  Nothing waits before the stores or after
// the loads, so a caller that uses the same smI again puts a barrier between the two calls (blockCount does, behind its sum).
__device__ __forceinline__ int blockSum(int* smI, int v) {
  const int tid = (int)threadIdx.x;
  v = waveSum(v);
  if ((tid & 63) == 0) smI[tid >> 6] = v;
  __syncthreads();
  return smI[0] + smI[1] + smI[2] + smI[3];
}
// ... through g.smI, which is free again on return
template <class G>
__device__ int blockCount(G& g, int v) {
  const int n = blockSum(g.smI, v);
  __syncthreads();
  return n;
}
template <int kCap>
__device__ __forceinline__ double combine4(const double* smW, int q) {   // smW [4][kCap]: the waves in order
  return ((smW[q] + smW[kCap + q]) + smW[2 * kCap + q]) + smW[3 * kCap + q];
}

// A site of one chunk: the sums of val(q), q < V, over the workgroup's threads; thread tid < V gets row tid's, the chunk's sum
// added to 0.0 as the many-chunk form adds it.  g.smW [4 G::kCap].
template <class G, class F>
__device__ __forceinline__ double siteSums(G& g, int V, F val) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();   // (the last sums have been read)
  for (int q = 0; q < V; q++) {
    const double v = waveSum(val(q));
    if (lane == 0) g.smW[wave * G::kCap + q] = v;
  }
  __syncthreads();
  double t = 0.0;
  if (tid < V) t += combine4<G::kCap>(g.smW, tid);
  return t;
}
// A site of nCh chunks by one workgroup: the sums of val(j, q), q < V, in the fixed order -> g.tot.  g.smW [nCh][4 G::kCap],
// g.chunkTot [nCh][G::kCap].
template <class G, class F>
__device__ void siteSums(G& g, int V, int nCh, F val) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int q = 0; q < V; q++)
    for (int c = 0; c < nCh; c++) {
      const double v = waveSum(val((int64_t)c * 256 + tid, q));
      if (lane == 0) g.smW[c][wave * G::kCap + q] = v;
    }
  __syncthreads();
  for (int k = tid; k < V * nCh; k += 256) g.chunkTot[k / V][k % V] = combine4<G::kCap>(g.smW[k / V], k % V);
  __syncthreads();
  if (tid < V) {
    double t = 0.0;
    for (int c = 0; c < nCh; c++) t += g.chunkTot[c][tid];
    g.tot[tid] = t;
  }
  __syncthreads();
}

// ---- a member's physical limits ---------------------------------------------------------------------------------------------
// a pool's value clipped: nothing below 0, except in plantCAccountingDelta
__device__ __forceinline__ double poolLimit(int slot, double v) { return slot != ST_plantCAccountingDelta && v < 0.0 ? 0.0 : v; }
// hasSufficientBiomass (sipnet.c:1530-1536)
__device__ __forceinline__ bool sufficientBiomass(double wood, double delta, double fineRoot, double coarseRoot) {
  const double totalWood = wood + delta, totalRoot = fineRoot + coarseRoot;
  return wood > kTiny && totalWood > kTiny && totalRoot > kTiny;
}
// ensureAllocation's test (setupKernel, step_kernel.hip)
__device__ __forceinline__ bool allocationsOk(double leaf, double wood, double fine) {
  return !(leaf >= 1.0 || wood >= 1.0 || fine >= 1.0 || 1 - leaf - wood - fine < 0);
}

// ---- the rows that depend on listed parameter rows ------------------------------------------------------------------------------
// where leafAllocation .. psnTMin are among a call's listed rows, or -1
struct DerivedRows {
  int32_t leaf, wood, fineRoot, opt, tmin;
};
// ... filled from the list, whose row indices go to prmRow in the caller's order
inline DerivedRows derivedRowsOf(int32_t n, const sipnet_enkf_param* params, int32_t* prmRow) {
  DerivedRows r{-1, -1, -1, -1, -1};
  for (int k = 0; k < n; k++) {
    const int p = params[k].index;
    prmRow[k] = p;
    if (p == SP_leafAllocation) r.leaf = k;
    if (p == SP_woodAllocation) r.wood = k;
    if (p == SP_fineRootAllocation) r.fineRoot = k;
    if (p == SP_psnTOpt) r.opt = k;
    if (p == SP_psnTMin) r.tmin = k;
  }
  return r;
}
// now(k, row): the member's value of parameter row `row` -- listed row k's new value, or (k < 0) the row as it stands.
// The allocation test, where an allocation is listed:
template <class F>
__device__ __forceinline__ bool allocationsOk(const DerivedRows& r, F now) {
  if (r.leaf < 0 && r.wood < 0 && r.fineRoot < 0) return true;
  return allocationsOk(now(r.leaf, SP_leafAllocation), now(r.wood, SP_woodAllocation), now(r.fineRoot, SP_fineRootAllocation));
}
// ... and column col's derived rows written, by convertParamsKernel's expressions
template <class F>
__device__ __forceinline__ void writeDerivedRows(double* prm, int64_t ncol, int64_t col, const DerivedRows& r, F now) {
  if (r.opt >= 0 || r.tmin >= 0) {
    const double opt = now(r.opt, SP_psnTOpt), tmin = now(r.tmin, SP_psnTMin);
    prm[(int64_t)SP_psnTMax * ncol + col] = opt + (opt - tmin);
  }
  if (r.leaf >= 0 || r.wood >= 0 || r.fineRoot >= 0) {
    const double leaf = now(r.leaf, SP_leafAllocation), wood = now(r.wood, SP_woodAllocation), fine = now(r.fineRoot, SP_fineRootAllocation);
    prm[(int64_t)SP_coarseRootAllocation * ncol + col] = 1 - leaf - wood - fine;
  }
}
