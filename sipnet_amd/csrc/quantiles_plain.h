// quantiles_plain.h -- the unweighted order statistics of a series per (row, site): sipnet_batch_plane_quantiles' kernels (a
// part of quantiles.hip, inside its anonymous namespace; keys, cells, the sort network and the radix select are
// quantiles_core.h's).  The quantiles of Hyndman & Fan's type 7, the sample size, and against an observation the rank
// histogram's counts and the CRPS.  The contract is in include/sipnet_amd.h.
//   quantSortKernel    the cell's keys once into LDS, a member that is not used and the padding up to P as the largest key;
//                      sortKeys; then the quantiles, the two counts by binary search and the CRPS's two sums over the sorted
//                      values.  P x 8 bytes of dynamic LDS: at most kSortCap = 16 384 members, 128 KiB.
//   quantSelectKernel  any M: RadixSelect over counts of elements.  The first read also counts what needs every value (n, the
//                      NaN flag, #(x < y), #(x == y)); n gives the at most 2 n_q distinct order statistics wanted.
// Both form a quantile from its two order statistics by quantileOf, so their bits are the same.

constexpr int kTargets = 2 * kQMax;              // order statistics of a call at most: x_(lo) and x_(lo+1) per quantile
constexpr int kSortCap = 16384;                  // members the sort path holds: 128 KiB of the CU's 160 KiB of LDS

struct PlainArgs : QuantArgs {
  const double* status;        // the batch's status row [ncol] (live_only), or nullptr: every member is used
  const int32_t* siteStatus;
  int32_t* count;              // [cells] or nullptr
  int32_t* rank;               // [cells][2] or nullptr
};

// where quantile q of n >= 1 sorted values lies: between x_(lo) and x_(lo + 1), g of the way (g == 0: x_(lo) itself)
__host__ __device__ inline void positionOf(int32_t n, double q, int32_t* lo, double* g) {
  const double h = (double)(n - 1) * q, f = floor(h);
  *lo = (int32_t)f;
  *g = h - f;
}
// every operation rounded once (the file is built without contraction)
__device__ __forceinline__ double quantileOf(double xlo, double xhi, double g) {
  if (g == 0.0) return xlo;
  const double d = xhi - xlo, t = g * d;
  return xlo + t;
}

struct PlainCell : Cell {
  bool siteLive;
  const double* st;
};
__device__ __forceinline__ PlainCell cellOf(const PlainArgs& a) {   // of a cell that exists
  PlainCell c;
  cellOf(a, c);
  c.siteLive = !a.status || a.siteStatus[c.s] == 0;
  c.st = a.status ? a.status + (int64_t)c.s * a.M : nullptr;
  return c;
}

// the outputs of a cell that are codes or NaN whatever its values: a bad observation, a NaN among the values, no value
__device__ __forceinline__ void writeCounts(const PlainArgs& a, const Cell& c, int n, bool anyNan, int less, int eq, int tid) {
  if (tid != 0) return;
  if (a.count) a.count[c.cell] = n;
  if (a.rank) {
    const bool none = anyNan || c.yNan;
    a.rank[2 * c.cell] = c.yBad ? -2 : none ? -1 : less;
    a.rank[2 * c.cell + 1] = c.yBad ? -2 : none ? -1 : eq;
  }
}

template <class T>
__global__ __launch_bounds__(256) void quantSortKernel(PlainArgs a, int P) {
  extern __shared__ uint64_t keys[];   // [P]
  __shared__ int sN, sNan;
  __shared__ double smD[8];
  const int tid = (int)threadIdx.x, M = a.M;
  if (cellIndex() >= a.cells) return;   // (the grid's last row may pass the cells; before anything of the cell is read)
  const PlainCell c = cellOf(a);
  if (tid == 0) {
    sN = 0;
    sNan = 0;
  }
  __syncthreads();
  int mine = 0;
  bool nan = false;
  forRow<T>(rowOf<T>(a, c), M, c.st, c.siteLive, tid, [&](int m, double x, bool used) {
    uint64_t k = kPadKey;
    if (used) {
      mine++;
      if (x != x)
        nan = true;
      else
        k = keyOf(x);
    }
    keys[m] = k;
  });
  padKeys<false>(keys, nullptr, M, P, tid);
  if (mine) atomicAdd(&sN, mine);
  if (nan) atomicOr(&sNan, 1);
  __syncthreads();
  const int n = sN;
  const bool anyNan = sNan != 0, blank = anyNan || c.yBad || n == 0;
  if (blank) {   // (the whole workgroup: nothing to sort)
    if (tid < a.nq) a.quant[(int64_t)tid * a.cells + c.cell] = quietNaN();
    if (tid == 0 && a.crps) a.crps[c.cell] = quietNaN();
    writeCounts(a, c, n, anyNan, 0, 0, tid);
    return;
  }
  sortKeys<false>(keys, nullptr, P, tid);
  if (tid < a.nq) {
    int32_t lo;
    double g;
    positionOf(n, a.q[tid], &lo, &g);
    const double xlo = valueOf(keys[lo]), xhi = g == 0.0 ? xlo : valueOf(keys[lo + 1]);
    a.quant[(int64_t)tid * a.cells + c.cell] = quantileOf(xlo, xhi, g);
  }
  int less = 0, eq = 0;
  if (tid == 0 && a.rank && !c.yNan) {   // the first key >= the observation's, the first above it
    const uint64_t ky = keyOf(c.y);
    int l0 = 0, l1 = n;
    while (l0 < l1) {
      const int mid = (l0 + l1) >> 1;
      if (keys[mid] < ky) l0 = mid + 1; else l1 = mid;
    }
    less = l0;
    l1 = n;
    while (l0 < l1) {
      const int mid = (l0 + l1) >> 1;
      if (keys[mid] <= ky) l0 = mid + 1; else l1 = mid;
    }
    eq = l0 - less;
  }
  writeCounts(a, c, n, false, less, eq, tid);
  if (a.crps) {   // sum |d_i| and sum (2 i - n - 1) d_(i), d = x - y in sorted order, i = 1 .. n: a thread its elements in order
    double s1 = 0.0, s2 = 0.0;
    if (!c.yNan)
      for (int i = tid; i < n; i += 256) {
        const double d = valueOf(keys[i]) - c.y;
        s1 += fabs(d);
        s2 += (double)(2 * (i + 1) - n - 1) * d;
      }
    groupSum2(s1, s2, smD);
    const double dn = (double)n;
    if (tid == 0) a.crps[c.cell] = c.yNan ? quietNaN() : s1 / dn - s2 / (dn * dn);
  }
}

template <class T>
__global__ __launch_bounds__(256) void quantSelectKernel(PlainArgs a) {
  __shared__ RadixSelect<uint32_t, kTargets> sel;   // request 2 i + e: x_(lo) and x_(lo + 1) of quantile i (the same where g == 0)
  __shared__ int sN, sNan, sLess, sEq;
  const int tid = (int)threadIdx.x, M = a.M;
  if (cellIndex() >= a.cells) return;   // (the grid's last row may pass the cells; before anything of the cell is read)
  const PlainCell c = cellOf(a);
  const T* row = rowOf<T>(a, c);
  if (tid == 0) {
    sN = 0;
    sNan = 0;
    sLess = 0;
    sEq = 0;
  }
  {   // the top byte of every key, and what is counted over all values
    const bool scored = a.rank && a.obs && !c.yNan && !c.yBad;
    const uint64_t ky = scored ? keyOf(c.y) : 0;
    int mine = 0, less = 0, eq = 0;
    bool nan = false;
    sel.first(row, M, c.st, c.siteLive, tid, [&](int, double x, bool used) -> uint32_t {
      if (!used) return 0;
      mine++;
      if (x != x) {
        nan = true;
        return 0;
      }
      if (scored) {
        const uint64_t k = keyOf(x);
        less += k < ky;
        eq += k == ky;
      }
      return 1;
    });
    if (mine) atomicAdd(&sN, mine);
    if (nan) atomicOr(&sNan, 1);
    if (less) atomicAdd(&sLess, less);
    if (eq) atomicAdd(&sEq, eq);
  }
  __syncthreads();
  const int n = sN;
  const bool anyNan = sNan != 0, blank = anyNan || c.yBad || n == 0;
  writeCounts(a, c, n, anyNan, sLess, sEq, tid);
  if (blank) {
    if (tid < a.nq) a.quant[(int64_t)tid * a.cells + c.cell] = quietNaN();
    return;
  }
  sel.rest(
      row, M, c.st, c.siteLive, tid, 2 * a.nq,
      [&](int i) -> uint32_t {   // 1-based: x_(lo) is the element at which the running count reaches lo + 1
        int32_t lo;
        double g;
        positionOf(n, a.q[i >> 1], &lo, &g);
        return (uint32_t)(lo + ((i & 1) && g != 0.0 ? 1 : 0) + 1);
      },
      [&](int, int, double, bool used) { return used; });   // (no NaN among the used values here)
  if (tid < a.nq) {
    int32_t lo;
    double g;
    positionOf(n, a.q[tid], &lo, &g);
    a.quant[(int64_t)tid * a.cells + c.cell] = quantileOf(sel.value(2 * tid), sel.value(2 * tid + 1), g);
  }
}
