// quantiles_weighted.h -- the order statistics and moments of a series per (row, site) under per-member log-weights:
// sipnet_batch_plane_quantiles_weighted's kernels (a part of quantiles.hip, inside its anonymous namespace; keys, cells, the
// sort network, the radix select and the block sums are quantiles_core.h's).  The contract is in include/sipnet_amd.h.
//
// The weights are integers: w_j = pfFixedWeight(logw_j, the site's maximum) <= 2^30 (pf_weights.inc, the filter's own), so every
// cumulative weight, total and rank sum is exact in int64 and does not depend on the order it was added in.
//   wquantSiteKernel    one workgroup per site: the maximum of the used members' log-weights, the members' integers (0 for a
//                       member that is not used) into the batch's scratch as int32, their total S, the number n of positive
//                       ones and the site's code.  The cell kernels LOAD these integers (4 bytes a member and row) instead of
//                       the log-weight (8 bytes, and the exponential's dozen multiply-adds); a zero integer also stands for
//                       "not used", so they read neither the status row nor the log-weights.
//   wquantSortKernel    P >= 256 a power of two: 64-bit keys [P] and 32-bit weights [P] in LDS, 12 bytes an element, at most
//                       kWSortCap = 8 192 members (96 KiB).  A member without weight and the padding carry the pad key and
//                       weight 0.  sortKeys on (key, weight) pairs: equal keys stay where they are, which fixes the order
//                       of the CRPS's second sum over tied values.  Then thread t owns the sorted elements
//                       [t P/256, (t + 1) P/256): their weights' sum, one block scan of int64, and a walk of its run with the
//                       cumulative weight in hand gives the quantiles (C_(i-1) < T <= C_i), the two rank sums, the CRPS's two
//                       sums and the mean; a second walk the centred moment.
//   wquantSelectKernel  any M: RadixSelect with 64-bit sums of weights in the bins and the targets T as ranks (one target per
//                       quantile: nothing is interpolated).  The mean in the first read of the row, the centred moment in the
//                       second.

constexpr int kWSortCap = 8192;   // members the weighted sort path holds: 12 bytes each, 96 KiB

struct WSiteArgs {
  const double* logw;          // [ncol]
  const double* status;        // the batch's status row (live_only), or nullptr
  const int32_t* siteStatus;
  int32_t M;
  int32_t* w;                  // [ncol] scratch: the integers
  int64_t* site;               // [n_sites][3] scratch: {S, n, code}
  int64_t* siteOut;            // the caller's, or nullptr
  int64_t* fixedOut;           // [ncol] the caller's, or nullptr
};
struct WQuantArgs : QuantArgs {
  const int32_t* w;            // [ncol]
  const int64_t* site;         // [n_sites][3]
  double* moments;             // [cells][2] or nullptr
  int64_t* rank;               // [cells][2] or nullptr
};

// T of the contract: one rounded product (S < 2^53 is exact as a double)
__host__ __device__ inline int64_t wTargetOf(int64_t S, double q) {
  const int64_t t = (int64_t)ceil(q * (double)S);
  return t < 1 ? 1 : t;
}

__global__ __launch_bounds__(256) void wquantSiteKernel(WSiteArgs a) {
  __shared__ double smD[4];
  __shared__ long long smL[4];
  const int tid = (int)threadIdx.x, s = (int)blockIdx.x, M = a.M;
  const int64_t base = (int64_t)s * M;
  const bool siteLive = !a.status || a.siteStatus[s] == 0;
  const double* st = a.status ? a.status + base : nullptr;
  const auto used = [&](int j) { return siteLive && (!st || st[j] == 0.0); };
  double m = -INFINITY;
  for (int j = tid; j < M; j += 256)
    if (used(j)) m = fmax(m, a.logw[base + j]);   // (fmax: a NaN is no maximum)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  if ((tid & 63) == 0) smD[tid >> 6] = m;
  __syncthreads();
  m = fmax(fmax(smD[0], smD[1]), fmax(smD[2], smD[3]));
  const bool bad = m == INFINITY;   // a +inf log-weight among the used members: nothing of the site weighs anything
  long long sum = 0, cnt = 0;
  for (int j = tid; j < M; j += 256) {
    const long long w = (bad || !used(j)) ? 0 : pfFixedWeight(a.logw[base + j], m);
    a.w[base + j] = (int32_t)w;
    if (a.fixedOut) a.fixedOut[base + j] = w;
    sum += w;
    cnt += w > 0;
  }
  const long long S = groupSum(sum, smL), n = groupSum(cnt, smL);
  if (tid == 0) {
    const long long code = bad ? -2 : S == 0 ? 1 : 0;
    int64_t* o = a.site + 3 * (int64_t)s;
    o[0] = S, o[1] = n, o[2] = code;
    if (a.siteOut) {
      o = a.siteOut + 3 * (int64_t)s;
      o[0] = S, o[1] = n, o[2] = code;
    }
  }
}

struct WCell : Cell {
  int64_t S, code;
  bool scored;
};
__device__ __forceinline__ WCell cellOf(const WQuantArgs& a) {   // of a cell that exists
  WCell c;
  cellOf(a, c);
  c.S = a.site[3 * (int64_t)c.s];
  c.code = a.site[3 * (int64_t)c.s + 2];
  c.scored = a.obs && !c.yNan && !c.yBad;
  return c;
}
// A cell without a result, every thread of its workgroup: NaN in every floating-point output, rank by the reason (0: the site
// weighs nothing; -2: a +inf log-weight or a non-finite observation; -1: a NaN in the sample)
__device__ __forceinline__ void wBlank(const WQuantArgs& a, const WCell& c, long long rank, int tid) {
  if (tid < a.nq) a.quant[(int64_t)tid * a.cells + c.cell] = quietNaN();
  if (tid != 0) return;
  if (a.crps) a.crps[c.cell] = quietNaN();
  if (a.moments) a.moments[2 * c.cell] = a.moments[2 * c.cell + 1] = quietNaN();
  if (a.rank) a.rank[2 * c.cell] = a.rank[2 * c.cell + 1] = rank;
}
// the code of a site that is not analysed, or of a bad observation, decides before a value is read: true, and the cell is done
__device__ __forceinline__ bool wBlankBefore(const WQuantArgs& a, const WCell& c, int tid) {
  if (c.code == 0 && !c.yBad) return false;
  wBlank(a, c, c.code == 1 ? 0 : -2, tid);
  return true;
}
__device__ __forceinline__ void wWriteRank(const WQuantArgs& a, const WCell& c, long long less, long long eq) {
  if (!a.rank) return;
  a.rank[2 * c.cell] = c.yNan ? -1 : less;
  a.rank[2 * c.cell + 1] = c.yNan ? -1 : eq;
}

template <class T>
__global__ __launch_bounds__(256) void wquantSortKernel(WQuantArgs a, int P) {
  extern __shared__ uint64_t keys[];   // [P] keys, behind them [P] 32-bit weights
  __shared__ int sNan;
  __shared__ long long smL[8], sT[kQMax];
  __shared__ double smD[8];
  uint32_t* wts = reinterpret_cast<uint32_t*>(keys + P);
  const int tid = (int)threadIdx.x, M = a.M;
  if (cellIndex() >= a.cells) return;   // (the grid's last row may pass the cells; before anything of the cell is read)
  const WCell c = cellOf(a);
  if (wBlankBefore(a, c, tid)) return;
  if (tid == 0) sNan = 0;
  if (tid < a.nq) sT[tid] = wTargetOf(c.S, a.q[tid]);
  __syncthreads();
  {
    const int32_t* wRow = a.w + (int64_t)c.s * M;
    bool nan = false;
    forRow<T>(rowOf<T>(a, c), M, nullptr, true, tid, [&](int m, double x, bool) {
      uint32_t w = (uint32_t)wRow[m];
      uint64_t k = kPadKey;
      if (w) {
        if (x != x) {
          nan = true;
          w = 0;
        } else {
          k = keyOf(x);
        }
      }
      keys[m] = k;
      wts[m] = w;
    });
    padKeys<true>(keys, wts, M, P, tid);
    if (nan) atomicOr(&sNan, 1);
  }
  __syncthreads();
  if (sNan != 0) {   // (the whole workgroup: nothing to sort)
    wBlank(a, c, -1, tid);
    return;
  }
  sortKeys<true>(keys, wts, P, tid);
  // thread tid's run of the sorted elements; the elements with weight come first, so a zero weight ends a run
  const int per = P >> 8, i0 = tid * per;
  long long mine = 0;
  for (int i = i0; i < i0 + per; i++) mine += wts[i];
  const long long before = groupScan(mine, smL) - mine, S = c.S;
  const uint64_t ky = c.scored ? keyOf(c.y) : 0;
  const bool crps = a.crps && c.scored;
  long long C = before, less = 0, eq = 0;
  double s1 = 0.0, s2 = 0.0, sm = 0.0;
  for (int i = i0; i < i0 + per; i++) {
    const long long w = wts[i];
    if (w == 0) break;
    const uint64_t k = keys[i];
    const double x = valueOf(k), dw = (double)w;
    const long long Cprev = C;
    C += w;
    for (int t = 0; t < a.nq; t++)
      if (Cprev < sT[t] && sT[t] <= C) a.quant[(int64_t)t * a.cells + c.cell] = x;
    if (c.scored) {
      less += k < ky ? w : 0;
      eq += k == ky ? w : 0;
    }
    if (crps) {
      const double d = x - c.y;
      s1 += dw * fabs(d);
      s2 += (dw * (double)(Cprev + C - S)) * d;
    }
    if (a.moments) sm += dw * x;
  }
  if (a.rank) {
    groupSum2(less, eq, smL);
    if (tid == 0) wWriteRank(a, c, less, eq);
  }
  const double dS = (double)S;
  if (a.crps) {
    groupSum2(s1, s2, smD);
    if (tid == 0) a.crps[c.cell] = c.scored ? s1 / dS - s2 / (dS * dS) : quietNaN();
  }
  if (a.moments) {
    const double mean = groupSum(sm, smD) / dS;
    double sv = 0.0;
    for (int i = i0; i < i0 + per; i++) {
      const long long w = wts[i];
      if (w == 0) break;
      const double d = valueOf(keys[i]) - mean;
      sv += (double)w * (d * d);
    }
    sv = groupSum(sv, smD);
    if (tid == 0) {
      a.moments[2 * c.cell] = mean;
      a.moments[2 * c.cell + 1] = sv / dS;
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void wquantSelectKernel(WQuantArgs a) {
  __shared__ RadixSelect<unsigned long long, kQMax> sel;   // request i: quantile i's target
  __shared__ long long smL[4];
  __shared__ double smD[4];
  __shared__ int sNan;
  const int tid = (int)threadIdx.x, M = a.M;
  if (cellIndex() >= a.cells) return;   // (the grid's last row may pass the cells; before anything of the cell is read)
  const WCell c = cellOf(a);
  if (wBlankBefore(a, c, tid)) return;
  const T* row = rowOf<T>(a, c);
  const int32_t* wRow = a.w + (int64_t)c.s * M;
  if (tid == 0) sNan = 0;
  const uint64_t ky = c.scored ? keyOf(c.y) : 0;
  long long less = 0, eq = 0;
  double sm = 0.0;
  {   // the top byte of every key, and what is summed over all values
    bool nan = false;
    sel.first(row, M, nullptr, true, tid, [&](int m, double x, bool) -> unsigned long long {
      const long long w = wRow[m];
      if (w == 0) return 0;
      if (x != x) {
        nan = true;
        return 0;
      }
      if (c.scored) {
        const uint64_t k = keyOf(x);
        less += k < ky ? w : 0;
        eq += k == ky ? w : 0;
      }
      if (a.moments) sm += (double)w * x;
      return (unsigned long long)w;
    });
    if (nan) atomicOr(&sNan, 1);
  }
  __syncthreads();
  if (sNan != 0) {
    wBlank(a, c, -1, tid);
    return;
  }
  if (a.rank) {
    less = groupSum(less, smL);
    eq = groupSum(eq, smL);
    if (tid == 0) wWriteRank(a, c, less, eq);
  }
  const double dS = (double)c.S;
  double mean = 0.0, sv = 0.0;
  if (a.moments) mean = groupSum(sm, smD) / dS;
  sel.rest(
      row, M, nullptr, true, tid, a.nq, [&](int i) { return (unsigned long long)wTargetOf(c.S, a.q[i]); },
      [&](int shift, int m, double x, bool) -> unsigned long long {   // (no NaN among the weighted values here)
        const long long w = wRow[m];
        if (w != 0 && a.moments && shift == 48) {   // the second read of the row: the moment about the mean
          const double dx = x - mean;
          sv += (double)w * (dx * dx);
        }
        return (unsigned long long)w;
      });
  if (tid < a.nq) a.quant[(int64_t)tid * a.cells + c.cell] = sel.value(tid);
  if (a.moments) {
    sv = groupSum(sv, smD);
    if (tid == 0) {
      a.moments[2 * c.cell] = mean;
      a.moments[2 * c.cell + 1] = sv / dS;
    }
  }
}
