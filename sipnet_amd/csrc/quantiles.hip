// quantiles.hip -- order statistics of a [rows][ld] series per (row, site): sipnet_batch_plane_quantiles (the quantiles of
// Hyndman & Fan's type 7, the sample size, and against an observation the rank histogram's counts and the CRPS), with the
// host-only sipnet_quantile_positions and sipnet_quantile_lds_members.  The contract is in include/sipnet_amd.h.
//
// A cell is (row r, site s): the values series[r][s M + j] of the site's used members, widened to double.  Both paths work on
// order-preserving 64-bit keys (keyOf: the double's bits, the sign bit flipped for a non-negative value, every bit for a
// negative one; -0.0 is made +0.0 first, so the zeros are one key).  A NaN among the used values is a flag of the cell, never a
// key.  One 256-thread workgroup per cell; the only waits are __syncthreads(); no grid barrier, no spin, no floating-point
// atomic (the integer atomics are LDS counters and histogram bins, whose totals do not depend on the order).
//   quantSortKernel    the cell's keys once into LDS (16-byte loads where the row is aligned), a member that is not used and
//                      the padding up to the next power of two P >= 256 as the largest key; a bitonic network: the steps whose
//                      partner is less than 64 elements away run in registers by __shfl_xor (element c 256 + tid: its partner is
//                      a lane of the same wavefront; eight chunks a thread at a time), the steps of distance >= 64 in LDS; then
//                      the quantiles, the two counts by binary search and the CRPS's two sums over the sorted values, each
//                      thread its elements in order, the threads by a fixed tree.  P x 8 bytes of dynamic LDS: at most
//                      kSortCap = 16 384 members, 128 KiB.
//   quantSelectKernel  any M: a most-significant-digit radix select.  The first pass is one 256-bin histogram of the keys' top
//                      byte and counts what needs every value (n, the NaN flag, #(x < y), #(x == y)); n gives the at most 2 n_q
//                      distinct order statistics wanted, and each of the seven passes that follow re-reads the row and counts the
//                      next byte of the keys that share a target's prefix, a histogram per target.  Eight reads of the row.
// Both form a quantile from its two order statistics by quantileOf, so their bits are the same.
// quantiles_weighted.h: the same statistics and the moments under per-member log-weights
// (sipnet_batch_plane_quantiles_weighted), with the filter's fixed-point weight of pf_weights.inc.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>

#include "batch_impl.h"
#include "site_host.h"

namespace {

#include "site_device.h"

constexpr int kQMax = SIPNET_QUANTILES_MAX;
constexpr int kTargets = 2 * kQMax;              // order statistics of a call at most: x_(lo) and x_(lo+1) per quantile
constexpr int kSortCap = 16384;                  // members the sort path holds: 128 KiB of the CU's 160 KiB of LDS
constexpr uint64_t kPadKey = ~(uint64_t)0;       // above the key of +inf (the bits of a NaN: never a used value's key)

struct QuantArgs {
  const void* series;
  int64_t ld, ncol, cells;
  int32_t nSites, M, nq;
  double q[kQMax];
  const double* status;        // the batch's status row [ncol] (live_only), or nullptr: every member is used
  const int32_t* siteStatus;
  double* quant;               // [n_q][cells]
  int32_t* count;              // [cells] or nullptr
  const double* obs;           // [cells] or nullptr
  double* crps;                // [cells] or nullptr
  int32_t* rank;               // [cells][2] or nullptr
};

__device__ __forceinline__ uint64_t keyOf(double x) {   // x is no NaN
  if (x == 0.0) x = 0.0;
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double valueOf(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

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

// what a cell's workgroup knows before it reads a value
struct Cell {
  int64_t cell;
  int s;
  bool siteLive, yNan, yBad;
  double y;
  const double* st;
};
__device__ __forceinline__ int64_t cellIndex() { return (int64_t)blockIdx.y * gridDim.x + blockIdx.x; }
__device__ __forceinline__ Cell cellOf(const QuantArgs& a) {   // of a cell that exists
  Cell c;
  c.cell = cellIndex();
  c.s = (int)(c.cell % a.nSites);
  c.siteLive = !a.status || a.siteStatus[c.s] == 0;
  c.st = a.status ? a.status + (int64_t)c.s * a.M : nullptr;
  c.y = a.obs ? a.obs[c.cell] : 0.0;
  c.yNan = a.obs && c.y != c.y;
  c.yBad = a.obs && !c.yNan && isinf(c.y);
  return c;
}
template <class T>
__device__ __forceinline__ const T* rowOf(const QuantArgs& a, const Cell& c) {
  return (const T*)a.series + (c.cell / a.nSites) * a.ld + (int64_t)c.s * a.M;
}

// the outputs of a cell that are codes or NaN whatever its values: a bad observation, a NaN among the values, no value
__device__ __forceinline__ void writeCounts(const QuantArgs& a, const Cell& c, int n, bool anyNan, int less, int eq, int tid) {
  if (tid != 0) return;
  if (a.count) a.count[c.cell] = n;
  if (a.rank) {
    const bool none = anyNan || c.yNan;
    a.rank[2 * c.cell] = c.yBad ? -2 : none ? -1 : less;
    a.rank[2 * c.cell + 1] = c.yBad ? -2 : none ? -1 : eq;
  }
}

__device__ __forceinline__ uint64_t shflKey(uint64_t v, int j) {
  const int lo = __shfl_xor((int)(uint32_t)v, j, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), j, 64);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
// The steps of the bitonic network whose partner is less than 64 elements away, on the elements c 256 + tid of kBatch chunks at
// a time (independent chains: the shuffles of one chunk hide behind the others'; P >= 256 kBatch).  first: the merges of
// 2 .. 64 elements from the start; else the steps 32 .. 1 of merge size k >= 128.
template <bool first, int kBatch>
__device__ __forceinline__ void waveStepsOf(uint64_t* keys, int P, int tid, int k) {
  for (int base = 0; base < P; base += 256 * kBatch) {
    uint64_t v[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int i = base + u * 256 + tid;
      v[u] = i < P ? keys[i] : 0;   // (past P: a value nobody stores)
    }
    for (int kk = first ? 2 : k; kk <= (first ? 64 : k); kk <<= 1)
      for (int j = first ? kk >> 1 : 32; j > 0; j >>= 1) {
        const bool lower = (tid & j) == 0;
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
          const bool asc = ((base + u * 256 + tid) & kk) == 0;
          const uint64_t o = shflKey(v[u], j);
          v[u] = (lower == asc) ? (v[u] < o ? v[u] : o) : (v[u] < o ? o : v[u]);
        }
      }
#pragma unroll
    for (int u = 0; u < kBatch; u++) {
      const int i = base + u * 256 + tid;
      if (i < P) keys[i] = v[u];
    }
  }
}
template <bool first>
__device__ __forceinline__ void waveSteps(uint64_t* keys, int P, int tid, int k) {
  if (P >= 2048)
    waveStepsOf<first, 8>(keys, P, tid, k);
  else if (P == 1024)
    waveStepsOf<first, 4>(keys, P, tid, k);
  else if (P == 512)
    waveStepsOf<first, 2>(keys, P, tid, k);
  else
    waveStepsOf<first, 1>(keys, P, tid, k);
}

template <class T>
__global__ __launch_bounds__(256) void quantSortKernel(QuantArgs a, int P) {
  extern __shared__ uint64_t keys[];   // [P]
  __shared__ int sN, sNan;
  __shared__ double sW[8];
  const int tid = (int)threadIdx.x, M = a.M;
  if (cellIndex() >= a.cells) return;   // (the grid's last row may pass the cells; before anything of the cell is read)
  const Cell c = cellOf(a);
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
  for (int m = M + tid; m < P; m += 256) keys[m] = kPadKey;
  if (mine) atomicAdd(&sN, mine);
  if (nan) atomicOr(&sNan, 1);
  __syncthreads();
  const int n = sN;
  const bool anyNan = sNan != 0, blank = anyNan || c.yBad || n == 0;
  const double kNaN = __longlong_as_double(0x7ff8000000000000ll);
  if (blank) {   // (the whole workgroup: nothing to sort)
    if (tid < a.nq) a.quant[(int64_t)tid * a.cells + c.cell] = kNaN;
    if (tid == 0 && a.crps) a.crps[c.cell] = kNaN;
    writeCounts(a, c, n, anyNan, 0, 0, tid);
    return;
  }
  waveSteps<true>(keys, P, tid, 0);
  __syncthreads();
  for (int k = 128; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= 64; j >>= 1) {   // four pairs a thread at a time: their loads in flight together
      for (int p0 = tid; p0 < (P >> 1); p0 += 256 * 4) {
        uint64_t u[4], w[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int p = p0 + e * 256, i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
          if (p < (P >> 1)) {
            u[e] = keys[i];
            w[e] = keys[i | j];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int p = p0 + e * 256, i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
          if (p < (P >> 1) && (u[e] > w[e]) == ((i & k) == 0)) {
            keys[i] = w[e];
            keys[i | j] = u[e];
          }
        }
      }
      __syncthreads();
    }
    waveSteps<false>(keys, P, tid, k);
    __syncthreads();
  }
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
  if (a.crps) {
    // sum |d_i| and sum (2 i - n - 1) d_(i), d = x - y in sorted order, i = 1 .. n: a thread its elements in order, a wavefront
    // by the xor butterfly, the four wavefronts in order
    double s1 = 0.0, s2 = 0.0;
    if (!c.yNan)
      for (int i = tid; i < n; i += 256) {
        const double d = valueOf(keys[i]) - c.y;
        s1 += fabs(d);
        s2 += (double)(2 * (i + 1) - n - 1) * d;
      }
    s1 = waveSum(s1);
    s2 = waveSum(s2);
    if ((tid & 63) == 0) {
      sW[2 * (tid >> 6)] = s1;
      sW[2 * (tid >> 6) + 1] = s2;
    }
    __syncthreads();
    if (tid == 0) {
      const double t1 = ((sW[0] + sW[2]) + sW[4]) + sW[6], t2 = ((sW[1] + sW[3]) + sW[5]) + sW[7], dn = (double)n;
      a.crps[c.cell] = c.yNan ? kNaN : t1 / dn - t2 / (dn * dn);
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void quantSelectKernel(QuantArgs a) {
  __shared__ uint32_t hist[kTargets][257];   // (257: the targets' scans, a thread per row, on different banks)
  __shared__ uint64_t prefix[kTargets];      // the digits found so far of target t's key
  __shared__ int32_t want[kTargets];         // its 0-based rank among the keys that share the prefix
  __shared__ int32_t slot[kTargets];         // quantile i: the targets of x_(lo) and x_(lo + 1) (the same where g == 0)
  __shared__ int sN, sNan, sLess, sEq, sT;
  const int tid = (int)threadIdx.x, M = a.M;
  if (cellIndex() >= a.cells) return;   // (the grid's last row may pass the cells; before anything of the cell is read)
  const Cell c = cellOf(a);
  const T* row = rowOf<T>(a, c);
  if (tid == 0) {
    sN = 0;
    sNan = 0;
    sLess = 0;
    sEq = 0;
    sT = 0;
  }
  hist[0][tid] = 0;
  __syncthreads();
  {   // the top byte of every key, and what is counted over all values
    const bool scored = a.rank && a.obs && !c.yNan && !c.yBad;
    const uint64_t ky = scored ? keyOf(c.y) : 0;
    int mine = 0, less = 0, eq = 0;
    bool nan = false;
    forRow<T>(row, M, c.st, c.siteLive, tid, [&](int, double x, bool used) {
      if (!used) return;
      mine++;
      if (x != x) {
        nan = true;
        return;
      }
      const uint64_t k = keyOf(x);
      atomicAdd(&hist[0][(int)(k >> 56)], 1u);
      if (scored) {
        less += k < ky;
        eq += k == ky;
      }
    });
    if (mine) atomicAdd(&sN, mine);
    if (nan) atomicOr(&sNan, 1);
    if (less) atomicAdd(&sLess, less);
    if (eq) atomicAdd(&sEq, eq);
  }
  __syncthreads();
  const int n = sN;
  const bool anyNan = sNan != 0, blank = anyNan || c.yBad || n == 0;
  const double kNaN = __longlong_as_double(0x7ff8000000000000ll);
  writeCounts(a, c, n, anyNan, sLess, sEq, tid);
  if (blank) {
    if (tid < a.nq) a.quant[(int64_t)tid * a.cells + c.cell] = kNaN;
    return;
  }
  if (tid == 0) {   // the distinct order statistics the quantiles need
    int T_ = 0;
    for (int i = 0; i < a.nq; i++) {
      int32_t lo;
      double g;
      positionOf(n, a.q[i], &lo, &g);
      for (int e = 0; e < 2; e++) {
        const int32_t r = lo + (e == 1 && g != 0.0 ? 1 : 0);
        int t = 0;
        while (t < T_ && want[t] != r) t++;
        if (t == T_) want[T_++] = r;
        slot[2 * i + e] = t;
      }
    }
    sT = T_;
  }
  __syncthreads();
  const int nT = sT;
  // a target's next digit from its histogram: the first bin whose running count passes its rank
  const auto scan = [&](int t, const uint32_t* h, uint64_t pre) {
    int32_t r = want[t], b = 0;
    for (; b < 255; b++) {
      const int32_t cnt = (int32_t)h[b];
      if (r < cnt) break;
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
    forRow<T>(row, M, c.st, c.siteLive, tid, [&](int, double x, bool used) {
      if (!used) return;   // (no NaN among the used values here)
      const uint64_t k = keyOf(x), top = k >> (shift + 8);
      const int d = (int)(k >> shift) & 255;
      for (int t = 0; t < nT; t++)
        if (prefix[t] == top) atomicAdd(&hist[t][d], 1u);
    });
    __syncthreads();
    if (tid < nT) scan(tid, hist[tid], prefix[tid]);
    __syncthreads();
  }
  if (tid < a.nq) {
    int32_t lo;
    double g;
    positionOf(n, a.q[tid], &lo, &g);
    a.quant[(int64_t)tid * a.cells + c.cell] = quantileOf(valueOf(prefix[slot[2 * tid]]), valueOf(prefix[slot[2 * tid + 1]]), g);
  }
}

#include "pf_weights.inc"
#include "quantiles_weighted.h"

// n_q and the q of a call: 0, or the refusal
int checkQ(const char* name, int32_t n_q, const double* q) {
  if (!q) return refuse(name, "a NULL q");
  if (n_q < 1 || n_q > kQMax) return refuse(name, "n_q must be 1..16");
  for (int i = 0; i < n_q; i++)
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return refuse(name, "q[" + std::to_string(i) + "] is not a number in [0, 1]");
  return 0;
}

// the path a call with this M and path argument runs under a sort capacity of cap members: 1 sort, 2 selection, -1 refused
int32_t pathOf(int32_t n_members, int32_t path, int32_t cap) {
  if (n_members < 1 || path < 0 || path > 2 || (path == 1 && n_members > cap)) return -1;
  return path == 1 || (path == 0 && n_members <= cap) ? 1 : 2;
}

}  // namespace

extern "C" {

int32_t sipnet_quantile_lds_members(int32_t elem_is_f32) {
  (void)elem_is_f32;   // (floats are widened to 64-bit keys as well: one capacity)
  return kSortCap;
}

int32_t sipnet_quantile_path(int32_t n_members, int32_t elem_is_f32, int32_t path) {
  return pathOf(n_members, path, sipnet_quantile_lds_members(elem_is_f32));
}

int sipnet_quantile_positions(int32_t n, int32_t n_q, const double* q, int32_t* lo, double* g) {
  const char* name = "sipnet_quantile_positions";
  if (!lo || !g) return refuse(name, "a NULL lo or g");
  int rc = checkQ(name, n_q, q);
  if (rc) return rc;
  if (n < 1) return refuse(name, "n must be >= 1");
  for (int i = 0; i < n_q; i++) positionOf(n, q[i], &lo[i], &g[i]);
  return SIPNET_OK;
}

int sipnet_batch_plane_quantiles(sipnet_batch* b, const void* d_series, int32_t elem_is_f32, int32_t rows, int64_t ld, int32_t n_q,
                                 const double* q, int32_t live_only, int32_t path, double* d_quant, int32_t* d_count,
                                 const double* d_obs, double* d_crps, int32_t* d_rank, void* hip_stream) {
  const char* name = "sipnet_batch_plane_quantiles";
  if (!b || !d_series || !d_quant) return refuse(name, "a NULL batch, series or d_quant");
  int rc = checkQ(name, n_q, q);
  if (rc) return rc;
  if (rows < 1 || ld < b->ncol) return refuse(name, "needs rows >= 1 and ld >= ncol");
  if ((d_crps || d_rank) && !d_obs) return refuse(name, "d_crps and d_rank need d_obs");
  if (path < 0 || path > 2) return refuse(name, "path must be 0 (auto), 1 (sort) or 2 (selection)");
  const int32_t M = b->n_members;
  if (path == 1 && M > kSortCap) return refuse(name, "the sort path holds at most 16384 members (sipnet_quantile_lds_members)");
  const bool sort = sipnet_quantile_path(M, elem_is_f32, path) == 1;
  if (d_crps && !sort)
    return refuse(name, "the CRPS needs the sorted sample: the sort path only (at most 16384 members, path 0 or 1)");
  if (live_only && b->planDirty) return refuse(name, "live_only needs a batch that was set up (sipnet_batch_setup)");
  rc = useDevice(b);
  if (rc) return rc;
  const hipStream_t stream = (hipStream_t)hip_stream;
  if (live_only) {   // (the status row is the batch's: behind whatever of the batch is writing it)
    rc = orderBehindBusy(b, stream);
    if (rc) return rc;
  }
  QuantArgs a{};
  a.series = d_series;
  a.ld = ld;
  a.ncol = b->ncol;
  a.nSites = b->n_sites;
  a.cells = (int64_t)rows * b->n_sites;
  a.M = M;
  a.nq = n_q;
  for (int i = 0; i < n_q; i++) a.q[i] = q[i];
  a.status = live_only ? b->d_state + (size_t)ST_status * b->ncol : nullptr;
  a.siteStatus = b->d_siteStatus;
  a.quant = d_quant;
  a.count = d_count;
  a.obs = d_obs;
  a.crps = d_crps;
  a.rank = d_rank;
  // a workgroup per cell: rows of at most 2^20 workgroups (a grid's x dimension times the 256 threads must stay below 2^32)
  const unsigned gx = (unsigned)std::min<int64_t>(a.cells, (int64_t)1 << 20);
  const dim3 grid(gx, (unsigned)((a.cells + gx - 1) / gx));
  if (sort) {
    int P = 256;
    while (P < M) P <<= 1;
    const size_t ldsBytes = (size_t)P * sizeof(uint64_t);
    const auto kernel = elem_is_f32 ? quantSortKernel<float> : quantSortKernel<double>;
    if (ldsBytes > 32 * 1024)   // (beside its static LDS, past what a kernel may use unasked)
      HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes));
    hipLaunchKernelGGL(kernel, grid, dim3(256), ldsBytes, stream, a, P);
  } else {
    hipLaunchKernelGGL((elem_is_f32 ? quantSelectKernel<float> : quantSelectKernel<double>), grid, dim3(256), 0, stream, a);
  }
  HIP_TRY(hipGetLastError());
  b->pfInfo.fused = sort ? 1 : 0;   // (what sipnet_batch_pf_info reports of the last such call: which path ran)
  b->pfInfo.grid = (int32_t)std::min<int64_t>(a.cells, INT32_MAX);
  return live_only ? markBusy(b, stream) : SIPNET_OK;
}

int64_t sipnet_wquantile_target(int64_t S, double q) {
  if (S < 1 || S > ((int64_t)1 << 52) || !(q >= 0.0 && q <= 1.0)) return -1;
  return wTargetOf(S, q);
}

int32_t sipnet_wquantile_lds_members(int32_t elem_is_f32) {
  (void)elem_is_f32;   // (floats are widened to 64-bit keys as well: one capacity)
  return kWSortCap;
}

int32_t sipnet_wquantile_path(int32_t n_members, int32_t elem_is_f32, int32_t path) {
  return pathOf(n_members, path, sipnet_wquantile_lds_members(elem_is_f32));
}

int sipnet_batch_plane_quantiles_weighted(sipnet_batch* b, const void* d_series, int32_t elem_is_f32, int32_t rows, int64_t ld,
                                          const double* d_logw, int32_t n_q, const double* q, int32_t live_only, int32_t path,
                                          double* d_quant, int64_t* d_site_weight, int64_t* d_fixed_weights, double* d_moments,
                                          const double* d_obs, double* d_crps, int64_t* d_rank, void* hip_stream) {
  const char* name = "sipnet_batch_plane_quantiles_weighted";
  if (!b || !d_series || !d_quant) return refuse(name, "a NULL batch, series or d_quant");
  if (!d_logw) return refuse(name, "a NULL d_logw");
  int rc = checkQ(name, n_q, q);
  if (rc) return rc;
  if (rows < 1 || ld < b->ncol) return refuse(name, "needs rows >= 1 and ld >= ncol");
  if (tooManyColumns(b)) return refuse(name, "more than 4194304 columns (the total weight must stay exact in a double)");
  if ((d_crps || d_rank) && !d_obs) return refuse(name, "d_crps and d_rank need d_obs");
  if (path < 0 || path > 2) return refuse(name, "path must be 0 (auto), 1 (sort) or 2 (selection)");
  const int32_t M = b->n_members;
  if (path == 1 && M > kWSortCap) return refuse(name, "the sort path holds at most 8192 members (sipnet_wquantile_lds_members)");
  const bool sort = sipnet_wquantile_path(M, elem_is_f32, path) == 1;
  if (d_crps && !sort)
    return refuse(name, "the CRPS needs the sorted sample: the sort path only (at most 8192 members, path 0 or 1)");
  if (live_only && b->planDirty) return refuse(name, "live_only needs a batch that was set up (sipnet_batch_setup)");
  rc = useDevice(b);
  if (rc) return rc;
  const hipStream_t stream = (hipStream_t)hip_stream;
  // (the status row and the scratch are the batch's: behind whatever of the batch is writing or reading them)
  rc = orderBehindBusy(b, stream);
  if (rc) return rc;
  WSiteArgs sa{};
  rc = carveScratch(b, b->d_wquant, [&](Carver& c) {
    sa.site = c.take<int64_t>((size_t)3 * b->n_sites);
    sa.w = c.take<int32_t>((size_t)b->ncol);
  });
  if (rc) return rc;
  sa.logw = d_logw;
  sa.status = live_only ? b->d_state + (size_t)ST_status * b->ncol : nullptr;
  sa.siteStatus = b->d_siteStatus;
  sa.M = M;
  sa.siteOut = d_site_weight;
  sa.fixedOut = d_fixed_weights;
  hipLaunchKernelGGL(wquantSiteKernel, dim3((unsigned)b->n_sites), dim3(256), 0, stream, sa);
  HIP_TRY(hipGetLastError());
  WQuantArgs a{};
  a.series = d_series;
  a.ld = ld;
  a.nSites = b->n_sites;
  a.cells = (int64_t)rows * b->n_sites;
  a.M = M;
  a.nq = n_q;
  for (int i = 0; i < n_q; i++) a.q[i] = q[i];
  a.w = sa.w;
  a.site = sa.site;
  a.quant = d_quant;
  a.moments = d_moments;
  a.obs = d_obs;
  a.crps = d_crps;
  a.rank = d_rank;
  // a workgroup per cell: rows of at most 2^20 workgroups, as the unweighted call's
  const unsigned gx = (unsigned)std::min<int64_t>(a.cells, (int64_t)1 << 20);
  const dim3 grid(gx, (unsigned)((a.cells + gx - 1) / gx));
  if (sort) {
    int P = 256;
    while (P < M) P <<= 1;
    const size_t ldsBytes = (size_t)P * (sizeof(uint64_t) + sizeof(uint32_t));
    const auto kernel = elem_is_f32 ? wquantSortKernel<float> : wquantSortKernel<double>;
    if (ldsBytes > 32 * 1024)   // (beside its static LDS, past what a kernel may use unasked)
      HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes));
    hipLaunchKernelGGL(kernel, grid, dim3(256), ldsBytes, stream, a, P);
  } else {
    hipLaunchKernelGGL((elem_is_f32 ? wquantSelectKernel<float> : wquantSelectKernel<double>), grid, dim3(256), 0, stream, a);
  }
  HIP_TRY(hipGetLastError());
  b->pfInfo.fused = sort ? 1 : 0;   // (what sipnet_batch_pf_info reports of the last such call: which path ran)
  b->pfInfo.grid = (int32_t)std::min<int64_t>(a.cells, INT32_MAX);
  return markBusy(b, stream);   // (the scratch is in use until these launches are done)
}

}  // extern "C"
