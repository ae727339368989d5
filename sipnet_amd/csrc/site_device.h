// site_device.h -- the device side that the per-site analyses share (enkf.hip, pf.hip, quantiles.hip and their .inc parts):
// which members are live, the sums in their one order, a member's physical limits, and a call's listed parameter rows with the
// rows that are derived from them (ListedRows, MemberRows: what the particle moves of pf.hip write a member's rows through).  Plain
// functions and templates, included INSIDE each unit's anonymous namespace like the .inc parts (so no include guard: once per
// unit).  fast_math.h has a kTiny of its own for the step kernels; no unit sees both.
//
// A floating-point sum is always taken in one order: the 256 columns of a chunk by an xor-shuffle butterfly inside each wave
// (waveSum), the four waves in order (combine4: ((w0 + w1) + w2) + w3), the chunks in order from 0.0 (siteSums).
constexpr double kTiny = 0.000001;   // TINY, common/util.h

// member j of site s takes part: it is inside the site, the site ran, and so did the member (status row 0)
__device__ __forceinline__ bool memberLive(const int32_t* siteStatus, const double* state, int64_t ncol, int64_t M, int s, int64_t j) {
  return j < M && siteStatus[s] == 0 && state[(int64_t)ST_status * ncol + (int64_t)s * M + j] == 0.0;
}
template <class A>   // ... by a kernel's arguments
__device__ __forceinline__ bool liveIn(const A& a, int s, int64_t j) { return memberLive(a.siteStatus, a.state, a.ncol, a.M, s, j); }
template <class T>   // double, int, long long
__device__ __forceinline__ T waveSum(T v) {
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
// the sum of a site's per-chunk counts cnt[s][0 .. nCh), to every thread (counted == false: 0); blockSum's barrier and smI
__device__ __forceinline__ int chunkCounts(int* smI, const int32_t* cnt, int s, int nCh, bool counted = true) {
  int v = 0;
  if (counted)
    for (int c = (int)threadIdx.x; c < nCh; c += 256) v += cnt[(int64_t)s * nCh + c];
  return blockSum(smI, v);
}
// a site's four info words (one thread)
__device__ __forceinline__ void writeInfo4(int32_t* info, int s, int w0, int w1, int w2, int w3) {
  int32_t* o = info + 4 * (int64_t)s;
  o[0] = w0, o[1] = w1, o[2] = w2, o[3] = w3;
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

// The parameter rows a call lists (sipnet_enkf_params_check's), as a kernel's arguments carry them
struct ListedRows {
  int32_t nPrm;
  int32_t prmRow[SIPNET_ENKF_MAX_PARAMS];                            // the listed rows of prm, in the caller's order
  double lo[SIPNET_ENKF_MAX_PARAMS], hi[SIPNET_ENKF_MAX_PARAMS];     // their bounds, converted units
  DerivedRows rows;                                                  // where leafAllocation .. psnTMin are among them
};
// One member's listed rows while a move gives them new values: those of the five rows that the derived rows depend on stay in
// registers as they are set, so allocOk and commit read a listed row's new value (now) and any other row as it stands in prm.
struct MemberRows {
  const ListedRows& l;
  const double* prm;   // [NPARAMS][ncol]
  int64_t ncol, col;
  double leaf = 0.0, wood = 0.0, fine = 0.0, opt = 0.0, tmin = 0.0;
  __device__ __forceinline__ void set(int k, double v) {
    if (k == l.rows.leaf) leaf = v;
    if (k == l.rows.wood) wood = v;
    if (k == l.rows.fineRoot) fine = v;
    if (k == l.rows.opt) opt = v;
    if (k == l.rows.tmin) tmin = v;
  }
  // the member's value of one of the five rows: a listed one's (k >= 0) from its register
  __device__ __forceinline__ double now(int k, int row) const {
    if (k < 0) return prm[(int64_t)row * ncol + col];
    return row == SP_leafAllocation ? leaf : row == SP_woodAllocation ? wood : row == SP_fineRootAllocation ? fine : row == SP_psnTOpt ? opt : tmin;
  }
  __device__ __forceinline__ bool allocOk() const { return allocationsOk(l.rows, [&](int k, int row) { return now(k, row); }); }
  // the listed rows' new values nv[k], then the derived rows, into column col of out (unrolled: nv stays in registers)
  __device__ __forceinline__ void commit(double* out, const double* nv) const {
#pragma unroll
    for (int k = 0; k < SIPNET_ENKF_MAX_PARAMS; k++) {
      if (k >= l.nPrm) break;
      out[(int64_t)l.prmRow[k] * ncol + col] = nv[k];
    }
    writeDerivedRows(out, ncol, col, l.rows, [&](int k, int row) { return now(k, row); });
  }
};
