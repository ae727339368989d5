// quantiles_core.h -- what the order statistics of a [rows][ld] series per (row, site) share, with and without weights (a part of
// quantiles.hip, inside its anonymous namespace; the statistics themselves: quantiles_plain.h, quantiles_weighted.h).
//
// A cell is (row r, site s): the values series[r][s M + j] of the site's used members, widened to double.  Both paths work on
// order-preserving 64-bit keys (keyOf: the double's bits, the sign bit flipped for a non-negative value, every bit for a
// negative one; -0.0 is made +0.0 first, so the zeros are one key).  A NaN among the used values is a flag of the cell, never a
// key.  One 256-thread workgroup per cell; the only waits are __syncthreads(); no grid barrier, no spin, no floating-point
// atomic (the integer atomics are LDS counters and histogram bins, whose totals do not depend on the order).
//   sortKeys     P >= 256 keys in LDS, a power of two, and with kW a 32-bit payload beside each (the weight): a bitonic
//                network.  The steps whose partner is less than 64 elements away run in registers by __shfl_xor (element
//                c 256 + tid: its partner is a lane of the same wavefront; eight chunks a thread at a time), the steps of
//                distance >= 64 in LDS.  Both partners of a compare-exchange decide from the same two keys whether they swap,
//                and with a payload equal keys stay where they are: the order of tied elements, which it makes visible, is
//                fixed.
//   RadixSelect  any M: a most-significant-digit radix select of at most kT targets, each a 1-based rank in the running total
//                of the elements' weights (a count of elements where every weight is 1).  The first read of the row is one
//                256-bin histogram of the keys' top byte; the caller's callable sees every element there and gathers what
//                needs every value.  Each of the seven reads that follow counts the next byte of the keys that share a
//                target's prefix, a histogram per distinct target.  Eight reads of the row.
// Floating-point sums: a thread its elements in forRow's order, a wavefront by the xor butterfly, the four wavefronts in order
// (groupSum).

constexpr int kQMax = SIPNET_QUANTILES_MAX;
constexpr uint64_t kPadKey = ~(uint64_t)0;       // above the key of +inf (the bits of a NaN: never a used value's key)

struct QuantArgs {             // of either call; PlainArgs and WQuantArgs add their own
  const void* series;
  int64_t ld, cells;
  int32_t nSites, M, nq;
  double q[kQMax];
  double* quant;               // [n_q][cells]
  const double* obs;           // [cells] or nullptr
  double* crps;                // [cells] or nullptr
};

__device__ __forceinline__ double quietNaN() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ uint64_t keyOf(double x) {   // x is no NaN
  if (x == 0.0) x = 0.0;
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double valueOf(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// the cell's row, every element once: f(member, its value as a double, is it used), thread tid of 256.  Which members a thread
// gets, and in which order, does not depend on the row's alignment (groups of 16 bytes' worth of members, then the tail one by
// one): a floating-point sum that a caller forms thread by thread is the same bits wherever the row lies in its tensor.
template <class T, class F>
__device__ __forceinline__ void forRow(const T* __restrict__ row, int M, const double* __restrict__ st, bool siteLive, int tid, F&& f) {
  constexpr int kPer = 16 / (int)sizeof(T);
  const int nVec = M / kPer;
  if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
    typedef T vec_t __attribute__((ext_vector_type(kPer)));
    const vec_t* __restrict__ rv = reinterpret_cast<const vec_t*>(row);
    for (int i = tid; i < nVec; i += 256) {
      const vec_t v = rv[i];
#pragma unroll
      for (int k = 0; k < kPer; k++) {
        const int m = i * kPer + k;
        f(m, (double)v[k], siteLive && (!st || st[m] == 0.0));
      }
    }
  } else {
    for (int i = tid; i < nVec; i += 256) {
      T v[kPer];
#pragma unroll
      for (int k = 0; k < kPer; k++) v[k] = row[i * kPer + k];
#pragma unroll
      for (int k = 0; k < kPer; k++) {
        const int m = i * kPer + k;
        f(m, (double)v[k], siteLive && (!st || st[m] == 0.0));
      }
    }
  }
  for (int m = nVec * kPer + tid; m < M; m += 256) f(m, (double)row[m], siteLive && (!st || st[m] == 0.0));
}

// what a cell's workgroup knows before it reads a value (PlainCell and WCell add their own)
struct Cell {
  int64_t cell;
  int s;
  bool yNan, yBad;
  double y;
};
__device__ __forceinline__ int64_t cellIndex() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }
__device__ __forceinline__ void cellOf(const QuantArgs& a, Cell& c) {   // of a cell that exists
  c.cell = cellIndex();
  c.s = (int)(c.cell % a.nSites);
  c.y = a.obs ? a.obs[c.cell] : 0.0;
  c.yNan = a.obs && c.y != c.y;
  c.yBad = a.obs && !c.yNan && isinf(c.y);
}
template <class T>
__device__ __forceinline__ const T* rowOf(const QuantArgs& a, const Cell& c) {
  return (const T*)a.series + (c.cell / a.nSites) * a.ld + (int64_t)c.s * a.M;
}

// sums over the workgroup's 256 threads, to every thread: a wavefront by the butterfly, the four in order.  One barrier
// before the totals are read and one after: sm [4] is free again on return.
template <class V>
__device__ __forceinline__ V groupSum(V v, V* sm) {
  const int tid = (int)threadIdx.x;
  v = waveSum(v);
  if ((tid & 63) == 0) sm[tid >> 6] = v;
  __syncthreads();
  const V r = ((sm[0] + sm[1]) + sm[2]) + sm[3];
  __syncthreads();
  return r;
}
// two such sums at once, each by groupSum's order of additions, behind one pair of barriers; sm [8]
template <class V>
__device__ __forceinline__ void groupSum2(V& a, V& b, V* sm) {
  const int tid = (int)threadIdx.x;
  a = waveSum(a);
  b = waveSum(b);
  if ((tid & 63) == 0) {
    sm[2 * (tid >> 6)] = a;
    sm[2 * (tid >> 6) + 1] = b;
  }
  __syncthreads();
  a = ((sm[0] + sm[2]) + sm[4]) + sm[6];
  b = ((sm[1] + sm[3]) + sm[5]) + sm[7];
  __syncthreads();
}
// the inclusive sum of v over the threads 0 .. tid
__device__ __forceinline__ long long groupScan(long long v, long long* sm) {
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

// ---- the sort network -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t shflKey(uint64_t v, int j) {
  const int lo = __shfl_xor((int)(uint32_t)v, j, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), j, 64);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
// The steps of the bitonic network whose partner is less than 64 elements away, on the elements c 256 + tid of kBatch chunks at
// a time (independent chains: the shuffles of one chunk hide behind the others'; P >= 256 kBatch).  first: the merges of
// 2 .. 64 elements from the start; else the steps 32 .. 1 of merge size k >= 128.  One compare-exchange of (v, w) with the
// partner's (o, ow): lower: this element is the one with the smaller index; both see the same two keys in the same roles.
template <bool kW, bool first, int kBatch>
__device__ __forceinline__ void waveStepsOf(uint64_t* keys, uint32_t* wts, int P, int tid, int k) {
  for (int base = 0; base < P; base += 256 * kBatch) {
    uint64_t v[kBatch];
    uint32_t w[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int i = base + u * 256 + tid;
      v[u] = i < P ? keys[i] : 0;   // (past P: a value nobody stores)
      if constexpr (kW) w[u] = i < P ? wts[i] : 0;
    }
    for (int kk = first ? 2 : k; kk <= (first ? 64 : k); kk <<= 1)
      for (int j = first ? kk >> 1 : 32; j > 0; j >>= 1) {
        const bool lower = (tid & j) == 0;
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
          // (keepsLess: the lower of an ascending pair, the upper of a descending one)
          const bool keepsLess = lower == (((base + u * 256 + tid) & kk) == 0);
          const uint64_t o = shflKey(v[u], j), mine = v[u];
          uint32_t ow = 0;
          if constexpr (kW) ow = (uint32_t)__shfl_xor((int)w[u], j, 64);
          // (the partner's only if it is strictly on the wrong side; as selects of values: they compile without a branch)
          v[u] = keepsLess ? (mine > o ? o : mine) : (mine < o ? o : mine);
          if constexpr (kW) w[u] = keepsLess ? (mine > o ? ow : w[u]) : (mine < o ? ow : w[u]);
        }
      }
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int i = base + u * 256 + tid;
      if (i < P) {
        keys[i] = v[u];
        if constexpr (kW) wts[i] = w[u];
      }
    }
  }
}
template <bool kW, bool first>
__device__ __forceinline__ void waveSteps(uint64_t* keys, uint32_t* wts, int P, int tid, int k) {
  if (P >= 2048)
    waveStepsOf<kW, first, 8>(keys, wts, P, tid, k);
  else if (P == 1024)
    waveStepsOf<kW, first, 4>(keys, wts, P, tid, k);
  else if (P == 512)
    waveStepsOf<kW, first, 2>(keys, wts, P, tid, k);
  else
    waveStepsOf<kW, first, 1>(keys, wts, P, tid, k);
}
// the elements from M up to P: the pad key (and no weight), as a member that is not used
template <bool kW>
__device__ __forceinline__ void padKeys(uint64_t* keys, uint32_t* wts, int M, int P, int tid) {
  for (int m = M + tid; m < P; m += 256) {
    keys[m] = kPadKey;
    if constexpr (kW) wts[m] = 0;
  }
}
// keys [P] ascending, every thread of the workgroup, the keys written and a barrier passed; kW: wts [P] travels with them
// (else wts is not touched).  Dynamic LDS of the caller: 8 bytes an element, 12 with the weights.
template <bool kW>
__device__ __forceinline__ void sortKeys(uint64_t* keys, uint32_t* wts, int P, int tid) {
  waveSteps<kW, true>(keys, wts, P, tid, 0);
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
          // ascending: swap if u > v, descending: if u < v, never equal keys (no branch chooses the compare).  Without
          // weights a swap of equal keys is invisible, and the test for it cost 3 % at 16 384 keys (NOTES.md, round 31): it
          // is compiled with the weights only.
          bool swap = (u[e] > v[e]) == ((i & k) == 0);
          if constexpr (kW) swap = swap & (u[e] != v[e]);
          if (p < (P >> 1) && swap) {
            keys[i] = v[e];
            keys[i | j] = u[e];
            if constexpr (kW) {
              const uint32_t wi = wts[i], wj = wts[i | j];
              wts[i] = wj;
              wts[i | j] = wi;
            }
          }
        }
      }
      __syncthreads();
    }
    waveSteps<kW, false>(keys, wts, P, tid, k);
    __syncthreads();
  }
}

// ---- the radix select -------------------------------------------------------------------------------------------------------
// The LDS of a select (a __shared__ object of the kernel) and its two stages.  C: the type of a weight and of a running
// total; kT: the targets a call may ask for.  A callable weightOf(..., member, value, used) returns the element's weight, 0
// for one to skip (not used, or a NaN: the caller's flag); it may sum what it likes of the element on the way.
template <class C, int kT>
struct RadixSelect {
  C hist[kT][257];        // (257: the targets' scans, a thread per row, on different banks)
  uint64_t prefix[kT];    // the digits found so far of target t's key
  C want[kT];             // what is left of its rank among the keys that share the prefix (1-based)
  int32_t slot[kT];       // request i's target
  int nT;

  // one read of the row: byte `shift / 8` of every weighted key into the histogram of each target whose prefix it shares
  // (top: the top byte, into the one histogram there is yet)
  template <bool top, class T, class F>
  __device__ __forceinline__ void count(const T* row, int M, const double* st, bool siteLive, int tid, int shift, int n, F&& weightOf) {
    forRow<T>(row, M, st, siteLive, tid, [&](int m, double x, bool used) {
      const auto w = weightOf(m, x, used);   // (a bool where every weight is 1: the compiler then adds the constant)
      if (!w) return;
      const uint64_t k = keyOf(x);
      const int d = (int)(k >> shift) & 255;
      if constexpr (top) {
        atomicAdd(&hist[0][d], (C)w);
      } else {
        const uint64_t pre = k >> (shift + 8);
        for (int t = 0; t < n; t++)
          if (prefix[t] == pre) atomicAdd(&hist[t][d], (C)w);
      }
    });
  }
  // a target's next digit from its histogram: the first bin at which the running total reaches what is left of its rank
  __device__ __forceinline__ void scan(int t, const C* h, uint64_t pre) {
    C r = want[t];
    int b = 0;
    for (; b < 255; b++) {
      const C cnt = h[b];
      if (r <= cnt) break;
      r -= cnt;
    }
    want[t] = r;
    prefix[t] = (pre << 8) | (uint64_t)b;
  }

  // The first read.  What the caller zeroed in LDS before is zero behind the barrier in here; the totals it adds there from
  // what weightOf gathered need its own barrier after.
  template <class T, class F>
  __device__ __forceinline__ void first(const T* row, int M, const double* st, bool siteLive, int tid, F&& weightOf) {
    hist[0][tid] = 0;
    __syncthreads();
    count<true>(row, M, st, siteLive, tid, 56, 1, weightOf);
  }
  // The seven reads that follow, for the requests i < nReq of the ranks rankOf(i) (thread 0 alone calls it): afterwards
  // valueOf(prefix[slot[i]]) is request i's value.  weightOf gets the shift of the read in front: 48 is the row's second read.
  template <class T, class R, class F>
  __device__ __forceinline__ void rest(const T* row, int M, const double* st, bool siteLive, int tid, int nReq, R&& rankOf,
                                       F&& weightOf) {
    if (tid == 0) {   // the distinct targets the requests need
      int T_ = 0;
      for (int i = 0; i < nReq; i++) {
        const C r = rankOf(i);
        int t = 0;
        while (t < T_ && want[t] != r) t++;
        if (t == T_) want[T_++] = r;
        slot[i] = t;
      }
      nT = T_;
    }
    __syncthreads();
    const int n = nT;
    if (tid < n) scan(tid, hist[0], 0);
    __syncthreads();
    for (int shift = 48; shift >= 0; shift -= 8) {
      for (int e = tid; e < n * 257; e += 256) hist[e / 257][e % 257] = 0;
      __syncthreads();
      count<false>(row, M, st, siteLive, tid, shift, n, [&](int m, double x, bool used) { return weightOf(shift, m, x, used); });
      __syncthreads();
      if (tid < n) scan(tid, hist[tid], prefix[tid]);
      __syncthreads();
    }
  }
  __device__ __forceinline__ double value(int i) const { return valueOf(prefix[slot[i]]); }
};
