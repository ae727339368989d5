// quantiles_weighted.h -- the order statistics and moments of a series per (row, site) under per-member log-weights:
// sipnet_batch_plane_quantiles_weighted's kernels (a part of quantiles.hip, inside its anonymous namespace: keyOf, valueOf,
// forRow, cellIndex, shflKey and kPadKey are the unweighted call's).  The contract is in include/sipnet_amd.h.
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
//                       weight 0.  The bitonic network of quantSortKernel on (key, weight) pairs: both partners of a
//                       compare-exchange decide from the same two keys whether the pairs swap (equal keys stay).  Then thread t
//                       owns the sorted elements [t P/256, (t + 1) P/256): their weights' sum, one block scan of int64, and a
//                       walk of its run with the cumulative weight in hand gives the quantiles (C_(i-1) < T <= C_i), the two
//                       rank sums, the CRPS's two sums and the mean; a second walk the centred moment.
//   wquantSelectKernel  any M: quantSelectKernel with 64-bit sums of weights in the bins and the targets T instead of an index
//                       (one target per quantile: nothing is interpolated).  Eight reads of the row; the mean in the first, the
//                       centred moment in the second.
// Floating-point sums: a thread its elements in order, a wavefront by the xor butterfly, the four wavefronts in order.

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
struct WQuantArgs {
  const void* series;
  int64_t ld, cells;
  int32_t nSites, M, nq;
  double q[kQMax];
  const int32_t* w;            // [ncol]
  const int64_t* site;         // [n_sites][3]
  double* quant;               // [n_q][cells]
  double* moments;             // [cells][2] or nullptr
  const double* obs;           // [cells] or nullptr
  double* crps;                // [cells] or nullptr
  int64_t* rank;               // [cells][2] or nullptr
};

// T of the contract: one rounded product (S < 2^53 is exact as a double)
__host__ __device__ inline int64_t wTargetOf(int64_t S, double q) {
  const int64_t t = (int64_t)ceil(q * (double)S);
  return t < 1 ? 1 : t;
}

// sums over the workgroup's 256 threads, to every thread: a wavefront by the butterfly, the four in order.  One barrier
// before the totals are read and one after: sm is free again on return.
template <class V>
__device__ __forceinline__ V wBlockSum(V v, V* sm) {
  const int tid = (int)threadIdx.x;
  v = waveSum(v);
  if ((tid & 63) == 0) sm[tid >> 6] = v;
  __syncthreads();
  const V r = ((sm[0] + sm[1]) + sm[2]) + sm[3];
  __syncthreads();
  return r;
}
// the inclusive sum of v over the threads 0 .. tid
__device__ __forceinline__ long long wBlockScan(long long v, long long* sm) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const long long o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  if (lane == 63) sm[wave] = v;
  __syncthreads();
  for (int k = 0; k < wave; k++) v += sm[k];
  __syncthreads();
  return v;
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
  const long long S = wBlockSum(sum, smL), n = wBlockSum(cnt, smL);
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

// what a cell's workgroup knows before it reads a value
struct WCell {
  int64_t cell, S, code;
  int s;
  bool yNan, yBad, scored;
  double y;
};
__device__ __forceinline__ WCell wCellOf(const WQuantArgs& a) {   // of a cell that exists
  WCell c;
  c.cell = cellIndex();
  c.s = (int)(c.cell % a.nSites);
  c.S = a.site[3 * (int64_t)c.s];
  c.code = a.site[3 * (int64_t)c.s + 2];
  c.y = a.obs ? a.obs[c.cell] : 0.0;
  c.yNan = a.obs && c.y != c.y;
  c.yBad = a.obs && !c.yNan && isinf(c.y);
  c.scored = a.obs && !c.yNan && !c.yBad;
  return c;
}
template <class T>
__device__ __forceinline__ const T* wRowOf(const WQuantArgs& a, const WCell& c) {
  return (const T*)a.series + (c.cell / a.nSites) * a.ld + (int64_t)c.s * a.M;
}
// A cell without a result, every thread of its workgroup: NaN in every floating-point output, rank by the reason (0: the site
// weighs nothing; -2: a +inf log-weight or a non-finite observation; -1: a NaN in the sample)
__device__ __forceinline__ void wBlank(const WQuantArgs& a, const WCell& c, long long rank, int tid) {
  const double kNaN = __longlong_as_double(0x7ff8000000000000ll);
  if (tid < a.nq) a.quant[(int64_t)tid * a.cells + c.cell] = kNaN;
  if (tid != 0) return;
  if (a.crps) a.crps[c.cell] = kNaN;
  if (a.moments) a.moments[2 * c.cell] = a.moments[2 * c.cell + 1] = kNaN;
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

// One compare-exchange of the pairs (v, w) and the partner's (o, ow): lower: this element is the one with the smaller index.
// Both partners see the same two keys in the same roles, so they agree on the swap; equal keys stay where they are.
__device__ __forceinline__ void wExchange(uint64_t& v, uint32_t& w, uint64_t o, uint32_t ow, bool lower, bool asc) {
  const uint64_t first = lower ? v : o, second = lower ? o : v;
  if (asc ? first > second : first < second) {
    v = o;
    w = ow;
  }
}
// waveStepsOf of quantiles.hip on pairs: the steps whose partner is less than 64 elements away, three dwords by __shfl_xor
template <bool first, int kBatch>
__device__ __forceinline__ void wWaveStepsOf(uint64_t* keys, uint32_t* wts, int P, int tid, int k) {
  for (int base = 0; base < P; base += 256 * kBatch) {
    uint64_t v[kBatch];
    uint32_t w[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int i = base + u * 256 + tid;
      v[u] = i < P ? keys[i] : 0;   // (past P: a value nobody stores)
      w[u] = i < P ? wts[i] : 0;
    }
    for (int kk = first ? 2 : k; kk <= (first ? 64 : k); kk <<= 1)
      for (int j = first ? kk >> 1 : 32; j > 0; j >>= 1) {
        const bool lower = (tid & j) == 0;
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
          const bool asc = ((base + u * 256 + tid) & kk) == 0;
          const uint64_t o = shflKey(v[u], j);
          const uint32_t ow = (uint32_t)__shfl_xor((int)w[u], j, 64);
          wExchange(v[u], w[u], o, ow, lower, asc);
        }
      }
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int i = base + u * 256 + tid;
      if (i < P) {
        keys[i] = v[u];
        wts[i] = w[u];
      }
    }
  }
}
template <bool first>
__device__ __forceinline__ void wWaveSteps(uint64_t* keys, uint32_t* wts, int P, int tid, int k) {
  if (P >= 2048)
    wWaveStepsOf<first, 8>(keys, wts, P, tid, k);
  else if (P == 1024)
    wWaveStepsOf<first, 4>(keys, wts, P, tid, k);
  else if (P == 512)
    wWaveStepsOf<first, 2>(keys, wts, P, tid, k);
  else
    wWaveStepsOf<first, 1>(keys, wts, P, tid, k);
}

template <class T>
__global__ __launch_bounds__(256) void wquantSortKernel(WQuantArgs a, int P) {
  extern __shared__ uint64_t keys[];   // [P] keys, behind them [P] 32-bit weights
  __shared__ int sNan;
  __shared__ long long smL[4], sT[kQMax];
  __shared__ double smD[4];
  uint32_t* wts = reinterpret_cast<uint32_t*>(keys + P);
  const int tid = (int)threadIdx.x, M = a.M;
  if (cellIndex() >= a.cells) return;   // (the grid's last row may pass the cells; before anything of the cell is read)
  const WCell c = wCellOf(a);
  if (wBlankBefore(a, c, tid)) return;
  if (tid == 0) sNan = 0;
  if (tid < a.nq) sT[tid] = wTargetOf(c.S, a.q[tid]);
  __syncthreads();
  {
    const int32_t* wRow = a.w + (int64_t)c.s * M;
    bool nan = false;
    forRow<T>(wRowOf<T>(a, c), M, nullptr, true, tid, [&](int m, double x, bool) {
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
    for (int m = M + tid; m < P; m += 256) {
      keys[m] = kPadKey;
      wts[m] = 0;
    }
    if (nan) atomicOr(&sNan, 1);
  }
  __syncthreads();
  if (sNan != 0) {   // (the whole workgroup: nothing to sort)
    wBlank(a, c, -1, tid);
    return;
  }
  wWaveSteps<true>(keys, wts, P, tid, 0);
  __syncthreads();
  for (int k = 128; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= 64; j >>= 1) {   // four pairs a thread at a time: their loads in flight together
      for (int p0 = tid; p0 < (P >> 1); p0 += 256 * 4) {
        uint64_t u[4], v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int p = p0 + e * 256, i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
          if (p < (P >> 1)) {
            u[e] = keys[i];
            v[e] = keys[i | j];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int p = p0 + e * 256, i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
          if (p < (P >> 1) && (((i & k) == 0) ? u[e] > v[e] : u[e] < v[e])) {
            keys[i] = v[e];
            keys[i | j] = u[e];
            const uint32_t wi = wts[i], wj = wts[i | j];
            wts[i] = wj;
            wts[i | j] = wi;
          }
        }
      }
      __syncthreads();
    }
    wWaveSteps<false>(keys, wts, P, tid, k);
    __syncthreads();
  }
  // thread tid's run of the sorted elements; the elements with weight come first, so a zero weight ends a run
  const int per = P >> 8, i0 = tid * per;
  long long mine = 0;
  for (int i = i0; i < i0 + per; i++) mine += wts[i];
  const long long before = wBlockScan(mine, smL) - mine, S = c.S;
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
    less = wBlockSum(less, smL);
    eq = wBlockSum(eq, smL);
    if (tid == 0) wWriteRank(a, c, less, eq);
  }
  const double kNaN = __longlong_as_double(0x7ff8000000000000ll), dS = (double)S;
  if (a.crps) {
    s1 = wBlockSum(s1, smD);
    s2 = wBlockSum(s2, smD);
    if (tid == 0) a.crps[c.cell] = c.scored ? s1 / dS - s2 / (dS * dS) : kNaN;
  }
  if (a.moments) {
    const double mean = wBlockSum(sm, smD) / dS;
    double sv = 0.0;
    for (int i = i0; i < i0 + per; i++) {
      const long long w = wts[i];
      if (w == 0) break;
      const double d = valueOf(keys[i]) - mean;
      sv += (double)w * (d * d);
    }
    sv = wBlockSum(sv, smD);
    if (tid == 0) {
      a.moments[2 * c.cell] = mean;
      a.moments[2 * c.cell + 1] = sv / dS;
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void wquantSelectKernel(WQuantArgs a) {
  __shared__ unsigned long long hist[kQMax][257];   // (257: the targets' scans, a thread per row, on different banks)
  __shared__ uint64_t prefix[kQMax];                // the digits found so far of target t's key
  __shared__ long long want[kQMax];                 // what is left of its T among the keys that share the prefix (1-based)
  __shared__ int32_t slot[kQMax];                   // quantile i's target
  __shared__ long long smL[4];
  __shared__ double smD[4];
  __shared__ int sNan, sT;
  const int tid = (int)threadIdx.x, M = a.M;
  if (cellIndex() >= a.cells) return;   // (the grid's last row may pass the cells; before anything of the cell is read)
  const WCell c = wCellOf(a);
  if (wBlankBefore(a, c, tid)) return;
  const T* row = wRowOf<T>(a, c);
  const int32_t* wRow = a.w + (int64_t)c.s * M;
  if (tid == 0) {
    sNan = 0;
    sT = 0;
  }
  hist[0][tid] = 0;
  __syncthreads();
  const uint64_t ky = c.scored ? keyOf(c.y) : 0;
  long long less = 0, eq = 0;
  double sm = 0.0;
  {   // the top byte of every key, and what is summed over all values
    bool nan = false;
    forRow<T>(row, M, nullptr, true, tid, [&](int m, double x, bool) {
      const long long w = wRow[m];
      if (w == 0) return;
      if (x != x) {
        nan = true;
        return;
      }
      const uint64_t k = keyOf(x);
      atomicAdd(&hist[0][(int)(k >> 56)], (unsigned long long)w);
      if (c.scored) {
        less += k < ky ? w : 0;
        eq += k == ky ? w : 0;
      }
      if (a.moments) sm += (double)w * x;
    });
    if (nan) atomicOr(&sNan, 1);
  }
  __syncthreads();
  if (sNan != 0) {
    wBlank(a, c, -1, tid);
    return;
  }
  if (a.rank) {
    less = wBlockSum(less, smL);
    eq = wBlockSum(eq, smL);
    if (tid == 0) wWriteRank(a, c, less, eq);
  }
  const double dS = (double)c.S;
  double mean = 0.0, sv = 0.0;
  if (a.moments) mean = wBlockSum(sm, smD) / dS;
  if (tid == 0) {   // the distinct targets the quantiles need
    int T_ = 0;
    for (int i = 0; i < a.nq; i++) {
      const long long r = wTargetOf(c.S, a.q[i]);
      int t = 0;
      while (t < T_ && want[t] != r) t++;
      if (t == T_) want[T_++] = r;
      slot[i] = t;
    }
    sT = T_;
  }
  __syncthreads();
  const int nT = sT;
  // a target's next digit from its histogram: the first bin at which the running weight reaches what is left of T
  const auto scan = [&](int t, const unsigned long long* h, uint64_t pre) {
    long long r = want[t];
    int b = 0;
    for (; b < 255; b++) {
      const long long cnt = (long long)h[b];
      if (r <= cnt) break;
      r -= cnt;
    }
    want[t] = r;
    prefix[t] = (pre << 8) | (uint64_t)b;
  };
  if (tid < nT) scan(tid, hist[0], 0);
  __syncthreads();
  for (int shift = 48; shift >= 0; shift -= 8) {
    for (int e = tid; e < nT * 257; e += 256) hist[e / 257][e % 257] = 0;
    __syncthreads();
    const bool second = a.moments && shift == 48;   // the second read of the row: the moment about the mean
    forRow<T>(row, M, nullptr, true, tid, [&](int m, double x, bool) {
      const long long w = wRow[m];
      if (w == 0) return;   // (no NaN among the weighted values here)
      const uint64_t k = keyOf(x), top = k >> (shift + 8);
      const int d = (int)(k >> shift) & 255;
      for (int t = 0; t < nT; t++)
        if (prefix[t] == top) atomicAdd(&hist[t][d], (unsigned long long)w);
      if (second) {
        const double dx = x - mean;
        sv += (double)w * (dx * dx);
      }
    });
    __syncthreads();
    if (tid < nT) scan(tid, hist[tid], prefix[tid]);
    __syncthreads();
  }
  if (tid < a.nq) a.quant[(int64_t)tid * a.cells + c.cell] = valueOf(prefix[slot[tid]]);
  if (a.moments) {
    sv = wBlockSum(sv, smD);
    if (tid == 0) {
      a.moments[2 * c.cell] = mean;
      a.moments[2 * c.cell + 1] = sv / dS;
    }
  }
}
