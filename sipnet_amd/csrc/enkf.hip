// enkf.hip -- the three ensemble Kalman filter analyses of the member pools: sipnet_batch_enkf_analysis_sites (a filter per
// site), sipnet_batch_enkf_analysis_local (the localized serial filter across sites) and sipnet_batch_enkf_analysis_block (the
// block-local filter: every site on its own, in one pass).
//
// Site s owns columns [s M, (s + 1) M).  Its live members' analysed pools and predicted observations are the analysis's
// variables: working copies W[v][member], v < nA the analysed pools (in state-slot order), nA + i the h of operator i.
// The serial square-root update (EAKF, Whitaker & Hamill 2002) recomputes every observation's statistics from the current
// ensemble: sums of the variables, then centred sums against h_i.  A sum is always taken in ONE order: chunks of 256
// members, a chunk by a fixed tree (every wave by an xor-shuffle butterfly, then the four waves in order); the chunk totals
// in segments of segLen(nCh) >= 16 consecutive chunks, each in order from 0.0; one segment is the site's total, several (at
// most 64) are combined by one wave's xor-shuffle butterfly.  A site of the one-workgroup-per-site kernel has at most 16 chunks,
// one segment: so that kernel and the per-chunk launches give the same bits.  No grid barrier, no spin, no atomic.
// The localized analysis reuses the per-chunk launches around a launch per level of its host schedule: one workgroup per
// (observation slot, target site), in the one-workgroup sum order.  The block-local analysis reuses them around ONE launch, a
// workgroup per target site, that runs the target's serial update on its small sample covariance (below).
//
// The host side: every entry point is its checks (localChecks for the two with a localization, then enkfBegin), the scratch
// block (enkfScratch), the front of the per-chunk launches (enkfFront: load, codes, reach, inflation), a middle of its own, and
// the tail (enkfEnd: limits, info, bookkeeping).  The per-site call may instead run its one-workgroup-per-site kernel between
// scratch and tail.
// sipnet_batch_enkf_analysis_smooth is the joint call around a series stage of its own (below: enkfSmoothPrepKernel,
// enkfSmoothKernel): the update of the pools applied to the window's flux series, on a scratch block of its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "batch_impl.h"

namespace {

constexpr int kMaxObs = 16;
constexpr int kPools = 13;                 // state slots 0..12: the Envi pools
constexpr int kMaxVars = kPools + kMaxObs;
constexpr int kMaxGroupChunks = 16;        // one workgroup per site: sites of at most 16 x 256 members
constexpr int kLdsWork = 40 * 1024;        // ... whose working copies fit here stay in LDS, else in the scratch block
constexpr double kTiny = 0.000001;         // TINY, common/util.h
constexpr int kMaxPrm = SIPNET_ENKF_MAX_PARAMS;   // the joint analysis: analysed parameters, between the pools and the h
constexpr int kJointVars = kMaxVars + kMaxPrm;
constexpr int kAnalysed = 1, kNoObs = -1, kBadInput = -2, kTooFew = 0;

struct EnkfOp {
  int32_t kind, mask, plane, param;
  double scale;
};
struct EnkfArgs {
  static constexpr int kCap = kMaxVars;    // variables a site can have: the pitch of smW, part and stat
  static constexpr bool kJoint = false;
  EnkfOp op[kMaxObs];
  int32_t nObs, nA, nv, nCh;
  int32_t pool[kPools];                    // the analysed state slots, ascending
  const void* planes[3];
  int32_t nSteps;
  int64_t ld;
  const double* obs;                       // [n_sites][nObs]
  const double* sd;
  const double* infl;                      // [n_sites] or null
  int32_t* info;                           // [n_sites][4]
  double* state;                           // [NSTATE][ncol]
  int64_t ncol, M;
  const int32_t* siteStatus;
  const double* prm;                       // converted parameters: prm[p * prmPitch + (prmId ? prmId[col] : col)]
  int64_t prmPitch;
  const int32_t* prmId;
  double* work;                            // [nv][ncol]
  double* part;                            // split path: [n_sites][nCh][kMaxVars] a chunk's sums
  double* stat;                            // split path: [n_sites][kStat]
  int32_t* cnt;                            // split path: [n_sites][nCh] live members / members kept on their forecast
  int32_t* kept;
  int32_t* site;                           // split path: [n_sites][2] the site's code and live count (enkfCodeKernel)
  int32_t* src;                            // localized analysis: [n_sites] enkfCodeKernel's codes, kept (else null)
  int32_t useLds;                          // one workgroup per site: W in LDS ([nv][M])
};
// sipnet_batch_enkf_analysis_joint: the variables are the nPool analysed pools, the nPrm analysed parameters (nA = nPool +
// nPrm: whatever is not an h), then the h.  The kernels are the per-site call's, instantiated for these arguments.
struct JointArgs : EnkfArgs {
  static constexpr int kCap = kJointVars;
  static constexpr bool kJoint = true;
  int32_t nPool, nPrm;
  int32_t prmRow[kMaxPrm];                 // the analysed rows of prmOut, in the caller's order
  double lo[kMaxPrm], hi[kMaxPrm];         // their bounds, converted units
  const double* prmInfl;                   // [n_sites] or null: lambda of the parameter variables
  double* prmOut;                          // d_prm [NPARAMS][ncol], every column its own rows: read by the load, written by the limits
  int32_t leaf, wood, fineRoot, opt, tmin; // where leafAllocation .. psnTMin are among the analysed parameters, or -1
};

__device__ __forceinline__ bool liveAt(const EnkfArgs& a, int s, int64_t j) {
  return j < a.M && a.siteStatus[s] == 0 && a.state[(int64_t)ST_status * a.ncol + (int64_t)s * a.M + j] == 0.0;
}

// the site's inputs: kBadInput, kNoObs, or kAnalysed (before the live count); *used = observations that are not NaN
__host__ __device__ inline int siteInputs(const double* obs, const double* sd, const double* infl, int nObs, int s, int* used) {
  bool bad = false;
  int u = 0;
  for (int i = 0; i < nObs; i++) {
    const double y = obs[(int64_t)s * nObs + i], e = sd[(int64_t)s * nObs + i];
    if (y != y) continue;
    if (!(fabs(y) < INFINITY) || !(e > 0.0) || !(e < INFINITY)) bad = true;
    u++;
  }
  if (infl) {
    const double l = infl[s];
    if (!(l >= 1.0) || !(l < INFINITY)) bad = true;
  }
  *used = u;
  return bad ? kBadInput : (u == 0 ? kNoObs : kAnalysed);
}

// ... and the joint analysis's lambda of the parameters, checked like the other
template <class A>
__device__ __forceinline__ int siteInputsOf(const A& a, int s, int* used) {
  int code = siteInputs(a.obs, a.sd, a.infl, a.nObs, s, used);
  if constexpr (A::kJoint)
    if (a.prmInfl) {
      const double l = a.prmInfl[s];
      if (!(l >= 1.0) || !(l < INFINITY)) code = kBadInput;
    }
  return code;
}
// the joint analysis's lambda of variable q at site s: the parameters have their own
__device__ __forceinline__ double lambdaOf(const JointArgs& a, int s, int q) {
  if (q >= a.nPool && q < a.nA) return a.prmInfl ? a.prmInfl[s] : 1.0;
  return a.infl ? a.infl[s] : 1.0;
}
__device__ __forceinline__ bool inflates(const JointArgs& a, int s) {
  return (a.infl && a.infl[s] != 1.0) || (a.prmInfl && a.prmInfl[s] != 1.0);
}

// h of operator i for column col, from the forecast
template <typename T>
__device__ double predicted(const EnkfArgs& a, int i, int64_t col) {
  const EnkfOp& o = a.op[i];
  double sum = 0.0;
  if (o.kind == SIPNET_ENKF_POOLS) {
    for (int p = 0; p < kPools; p++)
      if (o.mask & (1 << p)) sum += a.state[(int64_t)p * a.ncol + col];
  } else {
    const T* pl = (const T*)a.planes[o.plane];
    for (int t = 0; t < a.nSteps; t++) sum += (double)pl[(int64_t)t * a.ld + col];
  }
  double h = o.scale * sum;
  if (o.param >= 0) h = h / a.prm[(int64_t)o.param * a.prmPitch + (a.prmId ? (int64_t)a.prmId[col] : col)];
  return h;
}

__device__ __forceinline__ double waveSum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// the sum of an int over the workgroup's 256 threads (ints: any order), to every thread: every wave by an xor-shuffle
// butterfly, the four wave totals through smI[4] (a second sum through the same smI needs a barrier first)
__device__ __forceinline__ int blockSum(int* smI, int v) {
  const int tid = (int)threadIdx.x;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((tid & 63) == 0) smI[tid >> 6] = v;
  __syncthreads();
  return smI[0] + smI[1] + smI[2] + smI[3];
}
template <int kCap>
__device__ __forceinline__ double combine4(const double* smW, int q) {   // smW [4][kCap]: the waves in order
  return ((smW[q] + smW[kCap + q]) + smW[2 * kCap + q]) + smW[3 * kCap + q];
}
// chunks per segment of a site of nCh chunks: at most 64 segments
constexpr int kMaxSegs = 64;
__device__ __forceinline__ int segLen(int nCh) { return nCh <= 16 * kMaxSegs ? 16 : (nCh + kMaxSegs - 1) / kMaxSegs; }
// variable q of an observation stage i: the analysed pools, then h_i (q = nA), then the later h
__device__ __forceinline__ int varOf(const EnkfArgs& a, int q, int i) { return q < a.nA ? q : q + i; }

// the observation's denominator var(h) + R (sd e) from h's centred sum hsum over n members; *alpha its square-root factor
__device__ __forceinline__ double obsDenom(double hsum, double n, double e, double* alpha) {
  const double R = e * e, varh = hsum / (n - 1.0), denom = varh + R;
  *alpha = 1.0 / (1.0 + sqrt(R / denom));
  return denom;
}
// the gains of observation i (sd e) from the centred sums: K_q and alpha K_q of variable q (q = nA: h_i itself, unused)
__device__ __forceinline__ void gains(const EnkfArgs& a, int q, int V, double n, const double* csum, double e, double* K,
                                      double* aK) {
  if (q >= V) return;
  double alpha;
  const double denom = obsDenom(csum[a.nA], n, e, &alpha);
  const double k = (csum[q] / (n - 1.0)) / denom;
  K[q] = k;
  aK[q] = alpha * k;
}
__device__ __forceinline__ double moved(double x, double K, double aK, double innov, double dh) { return (x + K * innov) - aK * dh; }
__device__ __forceinline__ double inflated(double x, double mean, double lam) { return mean + lam * (x - mean); }

// the physical limits of one live member: its analysed pools clipped, then hasSufficientBiomass (sipnet.c:1530-1536) of
// the result; false = the member keeps its forecast.  fin[v] gets the clipped values.
__device__ bool limited(const EnkfArgs& a, int nPool, int64_t col, const double* W, int64_t ldw, int64_t j, double* fin) {
  double f[kPools];
  for (int p = 0; p < kPools; p++) f[p] = a.state[(int64_t)p * a.ncol + col];
  bool finite = true;
  for (int q = 0; q < nPool; q++) {
    double v = W[(int64_t)q * ldw + j];
    if (a.pool[q] != ST_plantCAccountingDelta && v < 0.0) v = 0.0;
    finite = finite && fabs(v) < INFINITY;
    fin[q] = v;
    f[a.pool[q]] = v;
  }
  const double totalWood = f[ST_plantWoodC] + f[ST_plantCAccountingDelta], totalRoot = f[ST_fineRootC] + f[ST_coarseRootC];
  return finite && f[ST_plantWoodC] > kTiny && totalWood > kTiny && totalRoot > kTiny;
}

// the joint analysis's limits of one live member's parameters, after limited(): every analysed parameter clipped into its
// bounds, in place in W; false = one is not finite, or an allocation is analysed and the result fails ensureAllocation's test
// (setupKernel, step_kernel.hip) -- the member keeps its forecast
__device__ __forceinline__ double prmNow(const JointArgs& a, const double* W, int64_t ldw, int64_t j, int64_t col, int k, int row) {
  return k >= 0 ? W[(int64_t)(a.nPool + k) * ldw + j] : a.prmOut[(int64_t)row * a.ncol + col];
}
__device__ bool limitedParams(const JointArgs& a, int64_t col, double* W, int64_t ldw, int64_t j) {
  bool ok = true;
  for (int k = 0; k < a.nPrm; k++) {
    double* x = W + (int64_t)(a.nPool + k) * ldw + j;
    double v = *x;
    v = v < a.lo[k] ? a.lo[k] : (v > a.hi[k] ? a.hi[k] : v);
    ok = ok && fabs(v) < INFINITY;
    *x = v;
  }
  if (a.leaf >= 0 || a.wood >= 0 || a.fineRoot >= 0) {
    const double leaf = prmNow(a, W, ldw, j, col, a.leaf, SP_leafAllocation), wood = prmNow(a, W, ldw, j, col, a.wood, SP_woodAllocation),
                 fine = prmNow(a, W, ldw, j, col, a.fineRoot, SP_fineRootAllocation);
    if (leaf >= 1.0 || wood >= 1.0 || fine >= 1.0 || 1 - leaf - wood - fine < 0) ok = false;
  }
  return ok;
}
// ... and its rows written: the analysed ones, then the derived rows that depend on them, by convertParamsKernel's expressions
__device__ void writeParams(const JointArgs& a, int64_t col, const double* W, int64_t ldw, int64_t j) {
  for (int k = 0; k < a.nPrm; k++) a.prmOut[(int64_t)a.prmRow[k] * a.ncol + col] = W[(int64_t)(a.nPool + k) * ldw + j];
  if (a.opt >= 0 || a.tmin >= 0) {
    const double opt = prmNow(a, W, ldw, j, col, a.opt, SP_psnTOpt), tmin = prmNow(a, W, ldw, j, col, a.tmin, SP_psnTMin);
    a.prmOut[(int64_t)SP_psnTMax * a.ncol + col] = opt + (opt - tmin);
  }
  if (a.leaf >= 0 || a.wood >= 0 || a.fineRoot >= 0) {
    const double leaf = prmNow(a, W, ldw, j, col, a.leaf, SP_leafAllocation), wood = prmNow(a, W, ldw, j, col, a.wood, SP_woodAllocation),
                 fine = prmNow(a, W, ldw, j, col, a.fineRoot, SP_fineRootAllocation);
    a.prmOut[(int64_t)SP_coarseRootAllocation * a.ncol + col] = 1 - leaf - wood - fine;
  }
}
// one live member through the limits and, unless it keeps its forecast, written back: its analysed pools (and parameters)
template <class A>
__device__ __forceinline__ bool limitAndWrite(const A& a, int64_t col, double* W, int64_t ldw, int64_t j) {
  double fin[kPools];
  int nPool = a.nA;
  if constexpr (A::kJoint) nPool = a.nPool;
  bool ok = limited(a, nPool, col, W, ldw, j, fin);
  if constexpr (A::kJoint) ok = limitedParams(a, col, W, ldw, j) && ok;
  if (!ok) return false;
  for (int q = 0; q < nPool; q++) a.state[(int64_t)a.pool[q] * a.ncol + col] = fin[q];
  if constexpr (A::kJoint) writeParams(a, col, W, ldw, j);
  return true;
}

// ---- one workgroup per site -------------------------------------------------------------------------------------------
template <int kCapacity>
struct GroupLdsOf {
  static constexpr int kCap = kCapacity;
  double smW[kMaxGroupChunks][4 * kCap];
  double chunkTot[kMaxGroupChunks][kCap];
  double tot[kCap];
  double mean[kCap];
  double K[kCap], aK[kCap];
  int smI[4];
};
using GroupLds = GroupLdsOf<kMaxVars>;
// the site's sums of val(j, q), q < V, in the fixed order -> g.tot
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
template <class G>
__device__ int blockCount(G& g, int v) {
  const int n = blockSum(g.smI, v);
  __syncthreads();
  return n;
}

template <typename T, class A>
__global__ __launch_bounds__(256) void enkfSiteKernel(A a) {
  extern __shared__ double ldsWork[];
  __shared__ GroupLdsOf<A::kCap> g;
  const int tid = (int)threadIdx.x, s = (int)blockIdx.x, nCh = a.nCh, nA = a.nA, nv = a.nv;
  const int64_t base = (int64_t)s * a.M;
  double* W = a.useLds ? ldsWork : a.work + base;
  const int64_t ldw = a.useLds ? a.M : a.ncol;
  int used;
  int code = siteInputsOf(a, s, &used);
  int mine = 0;
  for (int64_t j = tid; j < a.M; j += 256) mine += liveAt(a, s, j) ? 1 : 0;
  const int n = blockCount(g, mine);
  if (code == kAnalysed && n < 2) code = kTooFew;
  if (code != kAnalysed) {
    if (tid == 0) {
      int32_t* inf = a.info + 4 * (int64_t)s;
      inf[0] = code; inf[1] = 0; inf[2] = n; inf[3] = 0;
    }
    return;
  }
  // the working copies: analysed pools and predicted observations of the live members (each member: its own thread throughout)
  for (int64_t j = tid; j < a.M; j += 256)
    if (liveAt(a, s, j)) {
      if constexpr (A::kJoint) {
        for (int q = 0; q < a.nPool; q++) W[(int64_t)q * ldw + j] = a.state[(int64_t)a.pool[q] * a.ncol + base + j];
        for (int k = 0; k < a.nPrm; k++) W[(int64_t)(a.nPool + k) * ldw + j] = a.prmOut[(int64_t)a.prmRow[k] * a.ncol + base + j];
      } else {
        for (int q = 0; q < nA; q++) W[(int64_t)q * ldw + j] = a.state[(int64_t)a.pool[q] * a.ncol + base + j];
      }
      for (int i = 0; i < a.nObs; i++) W[(int64_t)(nA + i) * ldw + j] = predicted<T>(a, i, base + j);
    }
  const double nd = (double)n;
  const double lam = a.infl ? a.infl[s] : 1.0;
  bool inflate = lam != 1.0;
  if constexpr (A::kJoint) inflate = inflates(a, s);
  if (inflate) {
    siteSums(g, nv, nCh, [&](int64_t j, int q) { return liveAt(a, s, j) ? W[(int64_t)q * ldw + j] : 0.0; });
    if (tid < nv) g.mean[tid] = g.tot[tid] / nd;
    __syncthreads();
    for (int64_t j = tid; j < a.M; j += 256)
      if (liveAt(a, s, j))
        for (int q = 0; q < nv; q++) {
          if constexpr (A::kJoint) {   // (a lambda per variable class; a class at 1 is left as it is)
            const double l = lambdaOf(a, s, q);
            if (l != 1.0) W[(int64_t)q * ldw + j] = inflated(W[(int64_t)q * ldw + j], g.mean[q], l);
          } else {
            W[(int64_t)q * ldw + j] = inflated(W[(int64_t)q * ldw + j], g.mean[q], lam);
          }
        }
  }
  for (int i = 0; i < a.nObs; i++) {
    const double y = a.obs[(int64_t)s * a.nObs + i];
    if (y != y) continue;
    const double e = a.sd[(int64_t)s * a.nObs + i];
    const int V = nv - i;
    const double* Wh = W + (int64_t)(nA + i) * ldw;
    siteSums(g, V, nCh, [&](int64_t j, int q) { return liveAt(a, s, j) ? W[(int64_t)varOf(a, q, i) * ldw + j] : 0.0; });
    if (tid < V) g.mean[tid] = g.tot[tid] / nd;
    __syncthreads();
    const double hbar = g.mean[nA];
    siteSums(g, V, nCh, [&](int64_t j, int q) {
      return liveAt(a, s, j) ? (W[(int64_t)varOf(a, q, i) * ldw + j] - g.mean[q]) * (Wh[j] - hbar) : 0.0;
    });
    gains(a, tid, V, nd, g.tot, e, g.K, g.aK);
    __syncthreads();
    const double innov = y - hbar;
    for (int64_t j = tid; j < a.M; j += 256)
      if (liveAt(a, s, j)) {
        const double dh = Wh[j] - hbar;
        for (int q = 0; q < V; q++)
          if (q != nA) {
            double* x = W + (int64_t)varOf(a, q, i) * ldw + j;
            *x = moved(*x, g.K[q], g.aK[q], innov, dh);
          }
      }
  }
  int kept = 0;
  for (int64_t j = tid; j < a.M; j += 256)
    if (liveAt(a, s, j) && !limitAndWrite(a, base + j, W, ldw, j)) kept++;
  kept = blockCount(g, kept);
  if (tid == 0) {
    int32_t* inf = a.info + 4 * (int64_t)s;
    inf[0] = kAnalysed; inf[1] = used; inf[2] = n; inf[3] = kept;
  }
}

// ---- the split path: grid (sites, chunks of 256 members), one launch per stage --------------------------------------------
// the site's code, as enkfCodeKernel left it
__device__ __forceinline__ int splitCode(const EnkfArgs& a, int s) { return a.site[2 * (int64_t)s]; }
// one workgroup per site: the sum of a site's per-chunk counts (ints: any order)
__device__ int siteCount(const int32_t* v, int64_t nCh) {
  __shared__ int smI[4];
  int c = 0;
  for (int64_t k = threadIdx.x; k < nCh; k += 256) c += v[k];
  return blockSum(smI, c);
}
// stage i (i < 0: the inflation) leaves site s alone: not analysed, not inflated, or no observation i
template <class A>
__device__ __forceinline__ bool stageSkipped(const A& a, int s, int i) {
  if (splitCode(a, s) != kAnalysed) return true;
  if constexpr (A::kJoint)
    if (i < 0) return !inflates(a, s);
  if (i < 0) return !(a.infl && a.infl[s] != 1.0);
  return a.obs[(int64_t)s * a.nObs + i] != a.obs[(int64_t)s * a.nObs + i];
}

template <typename T, class A>
__global__ __launch_bounds__(256) void enkfLoadKernel(A a) {
  __shared__ int smI[4];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int64_t j = (int64_t)blockIdx.y * 256 + tid, col = (int64_t)s * a.M + j;
  const bool live = liveAt(a, s, j);
  if (live) {
    if constexpr (A::kJoint) {
      for (int q = 0; q < a.nPool; q++) a.work[(int64_t)q * a.ncol + col] = a.state[(int64_t)a.pool[q] * a.ncol + col];
      for (int k = 0; k < a.nPrm; k++) a.work[(int64_t)(a.nPool + k) * a.ncol + col] = a.prmOut[(int64_t)a.prmRow[k] * a.ncol + col];
    } else {
      for (int q = 0; q < a.nA; q++) a.work[(int64_t)q * a.ncol + col] = a.state[(int64_t)a.pool[q] * a.ncol + col];
    }
    for (int i = 0; i < a.nObs; i++) a.work[(int64_t)(a.nA + i) * a.ncol + col] = predicted<T>(a, i, col);
  }
  const int n = blockSum(smI, live ? 1 : 0);
  if (tid == 0) a.cnt[(int64_t)s * a.nCh + blockIdx.y] = n;
}

// one workgroup per site, after the load: the live count and the site's code, once
template <class A>
__global__ __launch_bounds__(256) void enkfCodeKernel(A a) {
  const int s = (int)blockIdx.x;
  const int n = siteCount(a.cnt + (int64_t)s * a.nCh, a.nCh);
  if (threadIdx.x == 0) {
    int used;
    int code = siteInputsOf(a, s, &used);
    if (code == kAnalysed && n < 2) code = kTooFew;
    a.site[2 * (int64_t)s] = code;
    a.site[2 * (int64_t)s + 1] = n;
    if (a.src) a.src[s] = code;
  }
}

// a chunk's sums for stage i (i < 0: the inflation's means over all variables): centred = 0 the variables,
// 1 the centred products with h_i (means from stat)
template <class A>
__global__ __launch_bounds__(256) void enkfPartialKernel(A a, int i, int centred) {
  constexpr int kMaxVars = A::kCap, kStat = 3 * A::kCap;
  __shared__ double smW[4 * kMaxVars];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x, c = (int)blockIdx.y;
  if (stageSkipped(a, s, i)) return;
  const int ii = i < 0 ? 0 : i, V = a.nv - ii;
  const int64_t j = (int64_t)c * 256 + tid, col = (int64_t)s * a.M + j;
  const bool live = liveAt(a, s, j);
  const double* mean = a.stat + (int64_t)s * kStat;
  const double dh = live && centred ? a.work[(int64_t)(a.nA + ii) * a.ncol + col] - mean[a.nA] : 0.0;
  for (int q = 0; q < V; q++) {
    double v = 0.0;
    if (live) {
      const double x = a.work[(int64_t)varOf(a, q, ii) * a.ncol + col];
      v = centred ? (x - mean[q]) * dh : x;
    }
    v = waveSum(v);
    if ((tid & 63) == 0) smW[(tid >> 6) * kMaxVars + q] = v;
  }
  __syncthreads();
  if (tid < V) a.part[((int64_t)s * a.nCh + c) * kMaxVars + tid] = combine4<kMaxVars>(smW, tid);
}

// one workgroup per site: the chunks' sums (every segment of every variable in order; the segments by one wave's butterfly)
// -> the means (centred = 0) or the gains (centred = 1)
template <class A>
__global__ __launch_bounds__(256) void enkfFinalKernel(A a, int i, int centred) {
  constexpr int kMaxVars = A::kCap, kStat = 3 * A::kCap;
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (stageSkipped(a, s, i)) return;
  __shared__ double tot[kMaxVars], seg[kMaxSegs][kMaxVars];
  const int ii = i < 0 ? 0 : i, V = a.nv - ii, n = a.site[2 * (int64_t)s + 1];
  const int L = segLen(a.nCh), nSeg = (a.nCh + L - 1) / L;
  const double* part = a.part + (int64_t)s * a.nCh * kMaxVars;
  for (int k = tid; k < nSeg * V; k += 256) {   // (segment g of variable q)
    const int g = k / V, q = k % V, c1 = (g + 1) * L < a.nCh ? (g + 1) * L : a.nCh;
    double t = 0.0;
    for (int c = g * L; c < c1; c++) t += part[(int64_t)c * kMaxVars + q];
    seg[g][q] = t;
  }
  __syncthreads();
  if (nSeg == 1) {
    if (tid < V) tot[tid] = seg[0][tid];
  } else {
    const int lane = tid & 63;
    for (int q = tid >> 6; q < V; q += 4) {   // (every wave its own variables)
      const double t = waveSum(lane < nSeg ? seg[lane][q] : 0.0);
      if (lane == 0) tot[q] = t;
    }
  }
  __syncthreads();
  double* st = a.stat + (int64_t)s * kStat;
  if (!centred) {
    if (tid < V) st[tid] = tot[tid] / (double)n;
  } else {
    gains(a, tid, V, (double)n, tot, a.sd[(int64_t)s * a.nObs + i], st + kMaxVars, st + 2 * kMaxVars);
  }
}

// a chunk's members moved by observation i (i < 0: inflated)
template <class A>
__global__ __launch_bounds__(256) void enkfUpdateKernel(A a, int i) {
  constexpr int kMaxVars = A::kCap, kStat = 3 * A::kCap;
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (stageSkipped(a, s, i)) return;
  const int64_t j = (int64_t)blockIdx.y * 256 + tid, col = (int64_t)s * a.M + j;
  if (!liveAt(a, s, j)) return;
  const double* st = a.stat + (int64_t)s * kStat;
  if (i < 0) {
    if constexpr (A::kJoint) {   // (a lambda per variable class; a class at 1 is left as it is)
      for (int q = 0; q < a.nv; q++) {
        const double l = lambdaOf(a, s, q);
        double* x = a.work + (int64_t)q * a.ncol + col;
        if (l != 1.0) *x = inflated(*x, st[q], l);
      }
      return;
    }
    const double lam = a.infl[s];
    for (int q = 0; q < a.nv; q++) {
      double* x = a.work + (int64_t)q * a.ncol + col;
      *x = inflated(*x, st[q], lam);
    }
    return;
  }
  const int V = a.nv - i;
  const double hbar = st[a.nA], innov = a.obs[(int64_t)s * a.nObs + i] - hbar;
  const double dh = a.work[(int64_t)(a.nA + i) * a.ncol + col] - hbar;
  for (int q = 0; q < V; q++)
    if (q != a.nA) {
      double* x = a.work + (int64_t)varOf(a, q, i) * a.ncol + col;
      *x = moved(*x, st[kMaxVars + q], st[2 * kMaxVars + q], innov, dh);
    }
}

template <class A>
__global__ __launch_bounds__(256) void enkfLimitKernel(A a) {
  __shared__ int smI[4];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  if (splitCode(a, s) != kAnalysed) return;
  const int64_t j = (int64_t)blockIdx.y * 256 + tid, col = (int64_t)s * a.M + j;
  int kept = 0;
  if (liveAt(a, s, j) && !limitAndWrite(a, col, a.work + (int64_t)s * a.M, a.ncol, j)) kept = 1;
  kept = blockSum(smI, kept);
  if (tid == 0) a.kept[(int64_t)s * a.nCh + blockIdx.y] = kept;
}

// one workgroup per site
template <class A>
__global__ __launch_bounds__(256) void enkfInfoKernel(A a) {
  const int s = (int)blockIdx.x;
  const int code = splitCode(a, s);
  const int kept = code == kAnalysed ? siteCount(a.kept + (int64_t)s * a.nCh, a.nCh) : 0;
  if (threadIdx.x == 0) {
    int used;
    (void)siteInputsOf(a, s, &used);
    int32_t* inf = a.info + 4 * (int64_t)s;
    inf[0] = code; inf[1] = code == kAnalysed ? used : 0; inf[2] = a.site[2 * (int64_t)s + 1]; inf[3] = kept;
  }
}

// ---- the localized analysis (sipnet_batch_enkf_analysis_local) -------------------------------------------------------------
// One (slot, target) pair: observation i of site s moves the variables of site t (t in F(s)) with the taper rho.
struct LocalPair {
  int32_t s, i, t;
  double rho;
};

// one thread per site, after enkfCodeKernel: a site without observations (-1) that a source (a.src == 1) reaches gets 1, or 0
// with fewer than 2 live members.  The sources are read from a.src, which nothing here writes.
__global__ __launch_bounds__(256) void enkfReachKernel(EnkfArgs a, const int64_t* inPtr, const int32_t* in, int64_t nSites) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= nSites || a.src[t] != kNoObs) return;
  for (int64_t k = inPtr[t]; k < inPtr[t + 1]; k++)
    if (a.src[in[k]] == kAnalysed) {
      a.site[2 * t] = a.site[2 * t + 1] >= 2 ? kAnalysed : kTooFew;
      return;
    }
}

// one workgroup per (slot, target) pair of a level (M <= 4096: one segment, the one-workgroup-per-site sum order).  The slot's
// mean and spread of h = h_{s,i} over L_s first, as every pair of the slot computes them; then the means and centred sums of
// t's variables against h over J = L_s and L_t, and J's members moved.  t's variables: its analysed pools, then its h of the
// slots after (s, i) (all of them for t > s, those after i for t = s, none for t < s).  Pairs of one level write disjoint
// sites and read no h_{s,i} that another pair writes.
__global__ __launch_bounds__(256) void enkfLocalKernel(EnkfArgs a, const LocalPair* pairs, int64_t first) {
  __shared__ GroupLds g;
  const LocalPair p = pairs[first + blockIdx.x];
  const int s = p.s, i = p.i, t = p.t, tid = (int)threadIdx.x, nA = a.nA, nCh = a.nCh;
  const double y = a.obs[(int64_t)s * a.nObs + i];
  if (y != y || splitCode(a, s) != kAnalysed || splitCode(a, t) != kAnalysed) return;
  const double* h = a.work + (int64_t)(nA + i) * a.ncol + (int64_t)s * a.M;
  double* Wt = a.work + (int64_t)t * a.M;
  const int hFirst = t > s ? 0 : (t == s ? i + 1 : a.nObs);
  const int V = a.nObs - hFirst + nA;
  auto var = [&](int q) { return Wt + (int64_t)(q < nA ? q : q + hFirst) * a.ncol; };
  auto inJ = [&](int64_t j) { return liveAt(a, s, j) && liveAt(a, t, j); };
  int mine = 0;
  for (int64_t j = tid; j < a.M; j += 256) mine += inJ(j) ? 1 : 0;
  const int nJ = blockCount(g, mine);
  if (nJ < 2) return;
  const double n = (double)a.site[2 * (int64_t)s + 1];
  siteSums(g, 1, nCh, [&](int64_t j, int) { return liveAt(a, s, j) ? h[j] : 0.0; });
  const double hbar = g.tot[0] / n;
  siteSums(g, 1, nCh, [&](int64_t j, int) { return liveAt(a, s, j) ? (h[j] - hbar) * (h[j] - hbar) : 0.0; });
  double alpha;
  const double D = obsDenom(g.tot[0], n, a.sd[(int64_t)s * a.nObs + i], &alpha);
  const double nd = (double)nJ;
  siteSums(g, 1, nCh, [&](int64_t j, int) { return inJ(j) ? h[j] : 0.0; });
  const double hbarJ = g.tot[0] / nd;
  siteSums(g, V, nCh, [&](int64_t j, int q) { return inJ(j) ? var(q)[j] : 0.0; });
  if (tid < V) g.mean[tid] = g.tot[tid] / nd;
  __syncthreads();
  siteSums(g, V, nCh, [&](int64_t j, int q) { return inJ(j) ? (var(q)[j] - g.mean[q]) * (h[j] - hbarJ) : 0.0; });
  if (tid < V) {
    const double k = p.rho * ((g.tot[tid] / (nd - 1.0)) / D);
    g.K[tid] = k;
    g.aK[tid] = alpha * k;
  }
  __syncthreads();
  const double innov = y - hbar;
  for (int64_t j = tid; j < a.M; j += 256)
    if (inJ(j)) {
      const double dh = h[j] - hbar;
      for (int q = 0; q < V; q++) {
        double* x = var(q) + j;
        *x = moved(*x, g.K[q], g.aK[q], innov, dh);
      }
    }
}


// ---- the block-local analysis (sipnet_batch_enkf_analysis_block) -----------------------------------------------------------
// One workgroup per target site t, all targets in one launch.  t's variables are its nA analysed pools and p rows: the predicted
// observations h_{u,i} of the code-1 sites u that reach it (and its own), read over L_t from the working copies, which nothing
// writes after the inflation -- so the private copies of the contract need no memory.  The serial square-root update is linear
// in the variables, so it runs on their sample covariance: one pass over the members forms C = cov(variable, row) ([nA + p][p]),
// the chain of p updates works on C, the means and the transform T (variable = its forecast + sum_w T[.][w] (row w's forecast
// anomaly)) alone, and a last pass applies T to the members.  Since alpha (2 - alpha var(h) / D) = 1, a step takes C to its
// Schur complement: C[v][w] -= K_v C[h][w].
// The matrices: Cx, Tx [nA][p] of the pools; S [p][p] holds C of the rows in its upper triangle (S[k][w], w >= k) and T of the
// rows strictly below the diagonal (T[k][k] = 1 is implied).  They live in LDS, where the staging tile was, when every target's
// fit (kLds), else in the target's block of global memory.  Every sum is taken in one order: the members in order.
constexpr int kBlockRows = SIPNET_ENKF_BLOCK_MAX_ROWS;
constexpr int kBlockVars = kPools + kBlockRows;
constexpr int kTile = 32;                  // members staged per tile
constexpr int kBlockMembers = 256 * kMaxGroupChunks;
constexpr int kBatch = 8;                  // loads in flight per thread before their stores
constexpr int kBlockMaxTiles = 32 * 33 / 2 + 4 * 32;   // blocks of 4 x 4 entries of C at 128 rows and 13 pools
constexpr int kBlockSmall = 48;            // targets of up to this many rows and 512 members: 256 threads; else 1024 (the chain
                                           // is a chain of LDS latencies that more waves hide; small targets only pay for their
                                           // barriers).  The arithmetic does not depend on the number of threads.

struct BlockLds {
  int64_t rowOff[kBlockVars];              // variable v of member j: a.work[rowOff[v] + j] (v < nA: t's pools, then its rows)
  double y[kBlockRows], R[kBlockRows];
  double mean0[kBlockVars], mean[kBlockVars], K[kBlockVars];
  int32_t srcOk[kBlockRows];               // in-neighbour k: every member of L_t is live there
  double alpha;
  int32_t p, selfPos;
  unsigned char flag[kBlockRows];          // slot (source, operator) of t: 1 a row, 2 a dropped row
  uint16_t tile[kBlockMaxTiles];           // C's blocks of 4 x 4 entries: (row block << 8) | column block
  unsigned char live[kBlockMembers];
};
__host__ __device__ inline int round4(int x) { return (x + 3) & ~3; }
// doubles of a target's matrices and of the staging tile
__host__ __device__ inline size_t blockMatSize(int nA, int p) { return (size_t)(p + 2 * nA) * (size_t)p; }
__host__ __device__ inline int blockStagePitch(int nA, int p) { return round4(round4(p) + nA); }

template <bool kLds, int kBlockThreads>
__global__ __launch_bounds__(kBlockThreads) void enkfBlockKernel(EnkfArgs a, const int64_t* inPtr, const int32_t* in, const double* inRho,
                                                       double* matGlobal, int64_t matPitch, int32_t* rowsOut) {
  constexpr int kBlockTiles = (kBlockMaxTiles + kBlockThreads - 1) / kBlockThreads;   // blocks of 4 x 4 entries of C a thread owns
  extern __shared__ __attribute__((aligned(16))) double blockDyn[];
  __shared__ BlockLds g;
  const int t = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nA = a.nA;
  const int64_t M = a.M;
  if (splitCode(a, t) != kAnalysed) {
    if (rowsOut && tid < 2) rowsOut[2 * (int64_t)t + tid] = 0;
    return;
  }
  for (int64_t j = tid; j < M; j += kBlockThreads) g.live[j] = liveAt(a, t, j) ? 1 : 0;
  __syncthreads();
  // which in-neighbours cover L_t
  const int64_t in0 = inPtr[t], nIn = inPtr[t + 1] - in0;
  for (int k = wave; k < nIn; k += kBlockThreads / 64) {
    const int u = in[in0 + k];
    int missing = 0;
    if (splitCode(a, u) == kAnalysed)
      for (int64_t j = lane; j < M; j += 64) missing += g.live[j] && !liveAt(a, u, j) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) missing += __shfl_xor(missing, off, 64);
    if (lane == 0) g.srcOk[k] = missing == 0;
  }
  if (tid < nIn && in[in0 + tid] < t && (tid + 1 == nIn || in[in0 + tid + 1] > t)) g.selfPos = tid + 1;   // (one writer)
  if (tid == 0 && (nIn == 0 || in[in0] > t)) g.selfPos = 0;
  __syncthreads();
  // the rows in site-major order: t takes its place among its in-neighbours (ascending); a thread per slot (source, operator)
  const int nSlots = ((int)nIn + 1) * a.nObs;   // (at most kBlockRows: the host refuses lists beyond the cap)
  int flag = 0;                                 // 1 a row, 2 a dropped row
  double y = 0.0, R = 0.0;
  int64_t off = 0;
  if (tid < nSlots) {
    const int q = tid / a.nObs, i = tid - q * a.nObs, selfPos = g.selfPos;
    const bool self = q == selfPos;
    const int64_t k = in0 + (q < selfPos ? q : q - 1);
    const int u = self ? t : in[k];
    const double rho = self ? 1.0 : inRho[k], e = a.sd[(int64_t)u * a.nObs + i];
    y = a.obs[(int64_t)u * a.nObs + i];
    if (splitCode(a, u) == kAnalysed && y == y) flag = self || g.srcOk[k - in0] ? 1 : 2;
    R = (e * e) / rho;
    off = (int64_t)(nA + i) * a.ncol + (int64_t)u * M;
    g.flag[tid] = (unsigned char)flag;
  }
  __syncthreads();
  if (flag == 1) {
    int row = 0;
    for (int e = 0; e < tid; e++) row += g.flag[e] == 1 ? 1 : 0;
    g.rowOff[nA + row] = off;
    g.y[row] = y;
    g.R[row] = R;
  }
  if (tid < nA) g.rowOff[tid] = (int64_t)tid * a.ncol + (int64_t)t * M;
  if (tid == 0) {
    int p = 0, dropped = 0;
    for (int e = 0; e < nSlots; e++) {
      p += g.flag[e] == 1 ? 1 : 0;
      dropped += g.flag[e] == 2 ? 1 : 0;
    }
    g.p = p;
    if (rowsOut) {
      rowsOut[2 * (int64_t)t] = p;
      rowsOut[2 * (int64_t)t + 1] = dropped;
    }
  }
  __syncthreads();
  const int p = g.p, V = nA + p;
  if (p == 0) return;   // (its pools stay as inflated; the limits follow)
  const double nd = (double)a.site[2 * (int64_t)t + 1];
  const int P4 = round4(p), pitch = blockStagePitch(nA, p);
  double* stage = blockDyn;                                       // [kTile][pitch]: the rows first, then the pools
  double* S = kLds ? blockDyn : matGlobal + (int64_t)t * matPitch;
  double* Cx = S + (size_t)p * p;
  double* Tx = Cx + (size_t)nA * p;
  // the forecast means
  for (int vb = wave; vb < V; vb += kBlockThreads / 16) {   // (four variables of a wave at a time: their loads overlap)
    double sum[4] = {};
    for (int64_t j = lane; j < M; j += 64)
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (vb + kBlockThreads / 64 * u < V) sum[u] += g.live[j] ? a.work[g.rowOff[vb + kBlockThreads / 64 * u] + j] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const double tot = waveSum(sum[u]);
      if (lane == 0 && vb + kBlockThreads / 64 * u < V) g.mean0[vb + kBlockThreads / 64 * u] = g.mean[vb + kBlockThreads / 64 * u] = tot / nd;
    }
  }
  // the blocks of 4 x 4 entries of C in staging order (the rows, then the pools): of the rows' blocks only those on or above
  // the diagonal.  Block number k belongs to thread k % kBlockThreads.
  const int nWt = P4 / 4, nXt = (pitch - P4) / 4, nTri = nWt * (nWt + 1) / 2, nB = nTri + nXt * nWt;
  for (int rt = tid; rt < nWt + nXt; rt += kBlockThreads) {
    const int first = rt < nWt ? rt : 0, at = rt < nWt ? rt * nWt - rt * (rt - 1) / 2 : nTri + (rt - nWt) * nWt;
    for (int wt = first; wt < nWt; wt++) g.tile[at + wt - first] = (uint16_t)((rt << 8) | wt);
  }
  __syncthreads();
  // C: the centred products, a tile of members at a time.  A thread keeps its blocks in registers over all the tiles, so an
  // entry is the sum over the members in order, and the staging tile shares its LDS with the matrices, written afterwards.
  int r0[kBlockTiles], w0[kBlockTiles];
  double acc[kBlockTiles][4][4] = {};
#pragma unroll
  for (int k = 0; k < kBlockTiles; k++) {
    const int blk = tid + kBlockThreads * k;
    r0[k] = blk < nB ? 4 * (g.tile[blk] >> 8) : -1;
    w0[k] = blk < nB ? 4 * (g.tile[blk] & 255) : 0;
  }
  for (int64_t j0 = 0; j0 < M; j0 += kTile) {
    for (int k0 = tid; k0 < pitch * kTile; k0 += kBlockThreads * kBatch) {   // (a batch of loads, then its stores)
      double val[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; u++) {
        const int k = k0 + kBlockThreads * u, sv = k / kTile, jj = k % kTile;
        const int v = sv < P4 ? (sv < p ? nA + sv : -1) : (sv - P4 < nA ? sv - P4 : -1);
        const int64_t j = j0 + jj;
        val[u] = k < pitch * kTile && v >= 0 && j < M && g.live[j] ? a.work[g.rowOff[v] + j] - g.mean0[v] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kBatch; u++) {
        const int k = k0 + kBlockThreads * u;
        if (k < pitch * kTile) stage[(k % kTile) * pitch + k / kTile] = val[u];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kBlockTiles; k++)
      if (r0[k] >= 0)
        for (int jj = 0; jj < kTile; jj++) {
          const double2* ra = (const double2*)(stage + jj * pitch + r0[k]);
          const double2* wb = (const double2*)(stage + jj * pitch + w0[k]);
          const double2 a0 = ra[0], a1 = ra[1], b0 = wb[0], b1 = wb[1];
          const double av[4] = {a0.x, a0.y, a1.x, a1.y}, bv[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
          for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[k][r][c] += av[r] * bv[c];
        }
    __syncthreads();
  }
  for (size_t k = tid; k < blockMatSize(nA, p); k += kBlockThreads) S[k] = 0.0;   // (T starts at 0: its unit diagonal is implied)
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kBlockTiles; k++)
    if (r0[k] >= 0)
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int sv = r0[k] + r, w = w0[k] + c;
          if (w >= p) continue;
          if (sv < P4) {
            if (sv < p && w >= sv) S[(size_t)sv * p + w] = acc[k][r][c] / (nd - 1.0);
          } else if (sv - P4 < nA) {
            Cx[(size_t)(sv - P4) * p + w] = acc[k][r][c] / (nd - 1.0);
          }
        }
  __syncthreads();
  // the chain
  for (int l = 0; l < p; l++) {
    const double* Sl = S + (size_t)l * p;
    const double innov = g.y[l] - g.mean[nA + l];
    if (tid < V) {   // (the divisions and the square root in the few waves that hold a variable, not in all of them)
      const double R = g.R[l], D = Sl[l] + R;
      g.K[tid] = tid < nA ? Cx[(size_t)tid * p + l] / D : (tid - nA > l ? Sl[tid - nA] / D : 0.0);
      if (tid == 0) g.alpha = 1.0 / (1.0 + sqrt(R / D));
    }
    __syncthreads();
    const double alpha = g.alpha;
    if (tid < V) g.mean[tid] += g.K[tid] * innov;
    // the pools, then the rows after l: column w of kBatch of them at a time (their loads, then their stores).  Left of the
    // diagonal entry l the column is T's, right of it C's; of a row k's C only w >= k is kept.
    const int nR = nA + (p - 1 - l), w = tid & 127;
    if (w < p) {
      const double slw = Sl[w];
      for (int rb = tid >> 7; rb < nR; rb += kBlockThreads / 128 * kBatch) {
        double val[kBatch], K[kBatch];
        int at[kBatch];   // (the entry's place counted from S: S | Cx | Tx)
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
          const int r = rb + kBlockThreads / 128 * u, k = r < nA ? -1 : l + 1 + (r - nA);
          at[u] = -1;
          if (r < nR && (w <= l || k < 0 || w >= k)) at[u] = (k >= 0 ? k : p + (w <= l ? nA : 0) + r) * p + w;
          K[u] = r < nR ? g.K[k < 0 ? r : nA + k] : 0.0;
          val[u] = at[u] >= 0 && w != l ? S[at[u]] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kBatch; u++)
          if (at[u] >= 0) S[at[u]] = w < l ? val[u] - (alpha * K[u]) * slw : (w == l ? -(alpha * K[u]) : val[u] - K[u] * slw);
      }
    }
    __syncthreads();
  }
  // the members: forecast + the mean's shift + T x (the rows' forecast anomalies)
  for (int64_t j = tid; j < M; j += kBlockThreads)
    if (g.live[j]) {
      double acc[kPools] = {};
#pragma unroll 8
      for (int w = 0; w < p; w++) {
        const double d = a.work[g.rowOff[nA + w] + j] - g.mean0[nA + w];
#pragma unroll
        for (int q = 0; q < kPools; q++)
          if (q < nA) acc[q] += Tx[(size_t)q * p + w] * d;
      }
#pragma unroll
      for (int q = 0; q < kPools; q++)
        if (q < nA) {
          double* x = a.work + g.rowOff[q] + j;
          *x = (*x + (g.mean[q] - g.mean0[q])) + acc[q];
        }
    }
}

// ---- the smoother of a window's series (sipnet_batch_enkf_analysis_smooth) ------------------------------------------------
// The serial update is linear in a variable's forecast covariance with the used observations' inflated forecast h (the p <= 16
// rows).  With a_j member j's row anomalies (0 for a member that is not live) and c_z = lambda sum_j (z_j - zbar) a_j / (n - 1),
// a series element z gets  z_a[j] = zbar + lambda (z_j - zbar) + c_z . g + (c_z G) . a_j.  g [p] and G [p][p] come from the
// covariance-space chain of the block-local analysis, run on the rows' p x p covariance with p unit covariance vectors carried
// as "pool rows": their mean shifts are g, their transforms the rows of G.  The rows come from enkfFront, run on a working
// copy of their own that holds nothing but the h; enkfSmoothPrepKernel (a workgroup per site) leaves a, g, G, p and n;
// enkfSmoothKernel (the hot path: a workgroup per site and run of rows) touches every element once.
constexpr int kMaxSeries = SIPNET_ENKF_MAX_SERIES;
constexpr int kMetaG = kMaxObs, kMetaP = kMaxObs + kMaxObs * kMaxObs, kMetaN = kMetaP + 1, kMeta = kMetaP + 8;   // doubles per site

__global__ __launch_bounds__(256) void enkfSmoothPrepKernel(JointArgs a, double* meta) {
  __shared__ GroupLds g;
  __shared__ double sC[kMaxObs][kMaxObs + 1], sEc[kMaxObs][kMaxObs + 1], sT[kMaxObs][kMaxObs + 1], sMean[kMaxObs];
  __shared__ int sUsed[kMaxObs], sP;
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x, nCh = a.nCh;
  double* m = meta + (int64_t)s * kMeta;
  if (splitCode(a, s) != kAnalysed) {
    if (tid == 0) m[kMetaP] = m[kMetaN] = 0.0;
    return;
  }
  if (tid == 0) {
    int p = 0;
    for (int i = 0; i < a.nObs; i++) {
      const double y = a.obs[(int64_t)s * a.nObs + i];
      if (y == y) sUsed[p++] = i;
    }
    sP = p;
  }
  __syncthreads();
  const int p = sP;
  const double nd = (double)a.site[2 * (int64_t)s + 1];
  double* H = a.work + (int64_t)s * a.M;   // row i of member j: H[i ncol + j]; the anomalies of row w go to H[w ncol + j], w <= used[w]
  siteSums(g, p, nCh, [&](int64_t j, int q) { return liveAt(a, s, j) ? H[(int64_t)sUsed[q] * a.ncol + j] : 0.0; });
  if (tid < p) sMean[tid] = g.tot[tid] / nd;
  __syncthreads();
  for (int64_t j = tid; j < a.M; j += 256) {   // (a member is its own thread's: row w is written after row used[w] >= w was read)
    const bool live = liveAt(a, s, j);
    for (int w = 0; w < p; w++) {
      const double v = live ? H[(int64_t)sUsed[w] * a.ncol + j] - sMean[w] : 0.0;
      H[(int64_t)w * a.ncol + j] = v;
    }
  }
  __syncthreads();
  for (int l = 0; l < p; l++) {   // the rows' covariance, row l from the diagonal on
    siteSums(g, p - l, nCh, [&](int64_t j, int q) {
      return j < a.M ? H[(int64_t)l * a.ncol + j] * H[(int64_t)(l + q) * a.ncol + j] : 0.0;
    });
    if (tid < p - l) sC[l][l + tid] = sC[l + tid][l] = g.tot[tid] / (nd - 1.0);
    __syncthreads();
  }
  // the chain: thread (k, w) owns entry [k][w] of C (the rows' covariance), Ec (the unit vectors' covariance with the rows),
  // T (row k = sum_w T[k][w] a_w) and G; w = 0 also row k's mean and g[k]
  const int k = tid >> 4, w = tid & 15;
  const bool in = k < p && w < p;
  double c = in ? sC[k][w] : 0.0, ec = k == w ? 1.0 : 0.0, tt = ec, et = 0.0, shift = 0.0, mean = k < p ? sMean[k] : 0.0;
  __syncthreads();
  for (int l = 0; l < p; l++) {
    sC[k][w] = c; sEc[k][w] = ec; sT[k][w] = tt;
    if (w == 0) sMean[k] = mean;
    __syncthreads();
    const int i = sUsed[l];
    const double e = a.sd[(int64_t)s * a.nObs + i], R = e * e, D = sC[l][l] + R, alpha = 1.0 / (1.0 + sqrt(R / D));
    const double innov = a.obs[(int64_t)s * a.nObs + i] - sMean[l];
    const double Kz = sEc[k][l] / D, K = sC[k][l] / D, Tl = sT[l][w], Cl = sC[l][w];
    et -= (alpha * Kz) * Tl;
    ec -= Kz * Cl;
    c -= K * Cl;
    shift += Kz * innov;
    if (k > l) {
      tt -= (alpha * K) * Tl;
      mean += K * innov;
    }
    __syncthreads();
  }
  if (w == 0) m[k] = in ? shift : 0.0;
  m[kMetaG + tid] = in ? et : 0.0;
  if (tid == 0) {
    m[kMetaP] = (double)p;
    m[kMetaN] = nd;
  }
}

struct SmoothSeries {
  const void* src;
  void* dst;
  int64_t ld;
  int32_t rows, f32, firstBlock, pad;
};
struct SmoothArgs {
  SmoothSeries ser[kMaxSeries];
  int32_t nSeries, run;                    // rows a workgroup owns
  const double* anom;                      // [nObs][ncol]: row w of site s's member j at anom[w ncol + s M + j]
  const double* meta;                      // [n_sites][kMeta]
  const int32_t* site;                     // [n_sites][2] code, live members
  const double* infl;
  const int32_t* siteStatus;
  const double* status;                    // the state's status row
  int64_t ncol, M;
};
__device__ __forceinline__ double seriesLoad(const SmoothSeries& q, int64_t at) {
  return q.f32 ? (double)((const float*)q.src)[at] : ((const double*)q.src)[at];
}
__device__ __forceinline__ void seriesStore(const SmoothSeries& q, int64_t at, double v) {
  if (q.f32) ((float*)q.dst)[at] = (float)v;
  else ((double*)q.dst)[at] = v;
}
__device__ __forceinline__ void seriesCopy(const SmoothSeries& q, int64_t at) {   // (the bits, whatever they are)
  if (q.f32) ((uint32_t*)q.dst)[at] = ((const uint32_t*)q.src)[at];
  else ((uint64_t*)q.dst)[at] = ((const uint64_t*)q.src)[at];
}

// kLds: the site's anomalies staged in LDS ([p][M]); else read from the scratch block.  A row is reduced by a team of kWaves
// waves: one wave (sites of at most 1 024 members: the four waves of a workgroup each take a row of their own, and a row costs
// no barrier) or all sixteen of a 1 024-thread workgroup.  kCh: members a thread holds, 64 kWaves apart.  Every sum in one
// order: a thread's members in order, the wave's butterfly, the team's waves in order; the team is a function of M alone.
template <bool kLds, int kWaves, int kCh>
__global__ __launch_bounds__(kWaves == 1 ? 256 : 64 * kWaves) void enkfSmoothKernel(SmoothArgs a) {
  constexpr int kThreads = kWaves == 1 ? 256 : 64 * kWaves, kTeam = 64 * kWaves, kTeams = kThreads / kTeam;
  extern __shared__ __attribute__((aligned(16))) double smA[];
  __shared__ double part[kWaves][kMaxObs + 1], tz[kMaxObs + 1], sg[kMaxObs], sG[kMaxObs][kMaxObs];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, team = tid / kTeam, tt = tid % kTeam;
  SmoothSeries q = a.ser[0];   // (the series this workgroup's rows belong to; constant indices: the arguments stay in registers)
#pragma unroll
  for (int e = 1; e < kMaxSeries; e++)
    if (e < a.nSeries && (int)blockIdx.y >= a.ser[e].firstBlock) q = a.ser[e];
  const int r0 = ((int)blockIdx.y - q.firstBlock) * a.run, r1 = r0 + a.run < q.rows ? r0 + a.run : q.rows;
  const int64_t M = a.M, col0 = (int64_t)s * M;
  if (a.site[2 * (int64_t)s] != kAnalysed) {
    if (q.dst != q.src)
      for (int r = r0; r < r1; r++)
        for (int64_t j = tid; j < M; j += kThreads) seriesCopy(q, (int64_t)r * q.ld + col0 + j);
    return;
  }
  const double* m = a.meta + (int64_t)s * kMeta;
  const int p = (int)m[kMetaP];
  const double nd = m[kMetaN], lam = a.infl ? a.infl[s] : 1.0;
  bool live[kCh], mine[kCh];
#pragma unroll
  for (int c = 0; c < kCh; c++) {
    const int64_t j = (int64_t)c * kTeam + tt;
    mine[c] = j < M;
    live[c] = mine[c] && a.siteStatus[s] == 0 && a.status[col0 + j] == 0.0;
  }
  for (int k = tid; k < kMaxObs * kMaxObs; k += kThreads) sG[k >> 4][k & 15] = m[kMetaG + k];
  if (tid < kMaxObs) sg[tid] = m[tid];
  if constexpr (kLds)
    for (int w = 0; w < p; w++)
      for (int64_t j = tid; j < M; j += kThreads) smA[(int64_t)w * M + j] = a.anom[(int64_t)w * a.ncol + col0 + j];
  __syncthreads();
  auto A = [&](int w, int c) -> double {   // (only for a member of the site: mine[c])
    const int64_t j = (int64_t)c * kTeam + tt;
    if constexpr (kLds) return smA[(int64_t)w * M + j];
    else return a.anom[(int64_t)w * a.ncol + col0 + j];
  };
  for (int r = r0 + team; r < r1; r += kTeams) {   // (kWaves > 1: one team, the workgroup's barriers are uniform)
    const int64_t at0 = (int64_t)r * q.ld + col0 + tt;
    double z[kCh], acc = 0.0;
#pragma unroll
    for (int c = 0; c < kCh; c++) {
      z[c] = live[c] ? seriesLoad(q, at0 + c * kTeam) : 0.0;
      acc += z[c];
    }
    acc = waveSum(acc);
    if constexpr (kWaves > 1) {
      if (lane == 0) part[wave][kMaxObs] = acc;
      __syncthreads();
      acc = part[0][kMaxObs];
      for (int v = 1; v < kWaves; v++) acc += part[v][kMaxObs];
    }
    const double zbar = acc / nd;
    double d[kCh];
#pragma unroll
    for (int c = 0; c < kCh; c++) d[c] = live[c] ? z[c] - zbar : 0.0;
    double t = 0.0;   // thread w < p of the team: (c_z G)[w]; thread p: c_z . g
    for (int w = 0; w < p; w++) {
      double cs = 0.0;
#pragma unroll
      for (int c = 0; c < kCh; c++)
        if (mine[c]) cs = fma(d[c], A(w, c), cs);
      cs = waveSum(cs);
      if constexpr (kWaves > 1) {
        if (lane == 0) part[wave][w] = cs;
      } else {
        const double cz = lam * (cs / (nd - 1.0));
        t = fma(cz, lane < p ? sG[w][lane] : sg[w], t);
      }
    }
    if constexpr (kWaves > 1) {
      __syncthreads();
      if (tid <= p) {
        for (int k = 0; k < p; k++) {
          double cs = part[0][k];
          for (int v = 1; v < kWaves; v++) cs += part[v][k];
          const double cz = lam * (cs / (nd - 1.0));
          t = fma(cz, tid < p ? sG[k][tid] : sg[k], t);
        }
        tz[tid] = t;
      }
      __syncthreads();
    }
    double mv[kCh] = {};
    for (int w = 0; w < p; w++) {
      const double tw = kWaves > 1 ? tz[w] : __shfl(t, w, 64);
#pragma unroll
      for (int c = 0; c < kCh; c++)
        if (mine[c]) mv[c] = fma(tw, A(w, c), mv[c]);
    }
    const double shift = kWaves > 1 ? tz[p] : __shfl(t, p, 64);
#pragma unroll
    for (int c = 0; c < kCh; c++) {
      if (live[c]) {
        const double base = lam == 1.0 ? z[c] : fma(lam, d[c], zbar);
        seriesStore(q, at0 + c * kTeam, (base + shift) + mv[c]);
      } else if (mine[c] && q.dst != q.src) {
        seriesCopy(q, at0 + c * kTeam);
      }
    }
  }
}

}  // namespace

// a localization: the level-ordered table of (slot, target) pairs and the in-neighbour lists, on the batch's device
struct sipnet_enkf_local {
  sipnet_batch* b = nullptr;
  int32_t device = 0, nSites = 0, nObs = 0, nLevels = 0;
  bool serial = false;                     // sipnet_debug_enkf_local_serial: one slot per launch, in serial order
  std::vector<int64_t> levelOff;           // [nLevels + 1]: the pairs of level l are [levelOff[l], levelOff[l + 1])
  std::vector<int64_t> slotOff;            // [n_sites][n_obs]: where slot (s, i)'s 1 + deg(s) pairs start
  std::vector<int32_t> slotLen;
  LocalPair* d_pair = nullptr;
  int64_t* d_inPtr = nullptr;              // [n_sites + 1]: site t is a neighbour of the sites d_in[d_inPtr[t] ..)
  int32_t* d_in = nullptr;
  double* d_inRho = nullptr;               // the tapers rho_ut in d_in's order
  int32_t maxRows = 0;                     // the block-local analysis: the largest n_obs x (1 + in-neighbours) of a site
};

void enkfRelease(sipnet_batch* b) {
  if (b->d_enkf) (void)hipFree(b->d_enkf);
  b->d_enkf = nullptr;
  b->enkfBytes = 0;
  if (b->d_smooth) (void)hipFree(b->d_smooth);
  b->d_smooth = nullptr;
  b->smoothBytes = 0;
}

namespace {

// a refusal: "`name`: `why`" is the thread's error
int refuse(const char* name, const std::string& why) {
  setError(std::string(name) + ": " + why);
  return SIPNET_ERR_BAD_ARGUMENT;
}

// The checks and the arguments the three analyses share, up to the scratch block: 0, or the error (the message names `name`).
// The synchronous form (no d_site_info) reads obs, sd and inflation back and refuses a bad site before anything is written.
int enkfBegin(const char* name, sipnet_batch* b, int32_t n_obs, const sipnet_enkf_obs* ops, int32_t analysed_mask,
              const void* const d_planes[3], int32_t n_steps, int64_t ld, const double* d_obs, const double* d_sd,
              const double* d_inflation, int32_t* d_site_info, hipStream_t stream, EnkfArgs& a) {
  const int32_t allPools = (1 << kPools) - 1;
  if (!b || !ops || !d_obs || !d_sd) return refuse(name, "a NULL batch, operators, observations or sds");
  if (n_obs < 1 || n_obs > kMaxObs) return refuse(name, "n_obs must be 1..16");
  if (analysed_mask == 0 || (analysed_mask & ~allPools)) return refuse(name, "analysed_mask must name pools 0..12");
  bool planesUsed = false;
  for (int i = 0; i < n_obs; i++) {
    const sipnet_enkf_obs& o = ops[i];
    const std::string at = "operator " + std::to_string(i) + ": ";
    if (o.param < -1 || o.param >= SIPNET_NPARAMS) return refuse(name, at + "param is not a parameter index");
    if (o.kind == SIPNET_ENKF_POOLS) {
      if (o.pool_mask == 0 || (o.pool_mask & ~allPools)) return refuse(name, at + "pool_mask must name pools 0..12");
    } else if (o.kind == SIPNET_ENKF_PLANE) {
      if (o.plane < 0 || o.plane > 2) return refuse(name, at + "plane must be 0 (NEE), 1 (GPP) or 2 (ET)");
      if (!d_planes || !d_planes[o.plane]) return refuse(name, at + "its plane pointer is NULL");
      planesUsed = true;
    } else {
      return refuse(name, at + "unknown kind");
    }
  }
  if (planesUsed && (n_steps <= 0 || ld < b->ncol)) return refuse(name, "planes need n_steps > 0 and ld >= ncol");
  if (b->ncol > (int64_t)1 << 22) return refuse(name, "at most 4194304 members");
  if (b->pfPeers) return refuse(name, "this batch is connected to a filter across ranks (sipnet_batch_pf_connect)");
  int rc = useDevice(b);
  if (rc) return rc;
  const int64_t nSites = b->n_sites, M = b->n_members, ncol = b->ncol;
  if (!d_site_info) {   // the synchronous form: the inputs are checked before anything is launched
    std::vector<double> obs((size_t)(nSites * n_obs)), sd(obs.size()), infl(d_inflation ? (size_t)nSites : 0);
    HIP_TRY(hipMemcpyAsync(obs.data(), d_obs, obs.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(sd.data(), d_sd, sd.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (d_inflation) HIP_TRY(hipMemcpyAsync(infl.data(), d_inflation, infl.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int64_t s = 0; s < nSites; s++) {
      int used;
      if (siteInputs(obs.data(), sd.data(), d_inflation ? infl.data() : nullptr, n_obs, (int)s, &used) == kBadInput)
        return refuse(name, "site " + std::to_string(s) + ": bad input (a finite obs needs a finite sd > 0; the inflation must "
                            "be finite and >= 1); nothing was written");
    }
  }
  b->pfPre.valid = false;
  b->pfArm.set = false;
  rc = orderBehindBusy(b, stream);
  if (rc) return rc;
  rc = flushParams(b, stream);
  if (rc) return rc;

  a = EnkfArgs{};
  a.nObs = n_obs;
  for (int i = 0; i < n_obs; i++) a.op[i] = EnkfOp{ops[i].kind, ops[i].pool_mask, ops[i].plane, ops[i].param, ops[i].scale};
  for (int p = 0; p < kPools; p++)
    if (analysed_mask & (1 << p)) a.pool[a.nA++] = p;
  a.nv = a.nA + n_obs;
  a.nCh = (int32_t)((M + 255) / 256);
  for (int k = 0; k < 3; k++) a.planes[k] = d_planes ? d_planes[k] : nullptr;
  a.nSteps = n_steps;
  a.ld = ld;
  a.obs = d_obs;
  a.sd = d_sd;
  a.infl = d_inflation;
  a.state = b->d_state;
  a.ncol = ncol;
  a.M = M;
  a.siteStatus = b->d_siteStatus;
  if (b->prmIndexed) {   // (after a resampling with_params: column c's parameters are bank column d_prmId[c])
    a.prm = b->d_prmBank ? b->d_prmBank : b->d_prm;
    a.prmPitch = b->d_prmBank ? b->prmBankPitch : ncol;
    a.prmId = b->d_prmId;
  } else {
    a.prm = b->d_prm;
    a.prmPitch = ncol;
    a.prmId = nullptr;
  }
  return 0;
}

// The batch's scratch block sized, grown and carved, in this order: the working copies [nv][ncol] (workInGlobal: else they
// live in LDS) | part [sites][chunks][cap] | stat [sites][3 cap] (cap: the kernels' A::kCap) | matPerSite doubles of matrices per site | info [sites][4]
// (a.info is d_site_info where given) | cnt, kept [sites][chunks] | site [sites][2] | src [sites] (withSrc).  part, stat, cnt,
// kept and site are the per-chunk launches' (perChunk: without them the regions are empty, and cnt, kept and site, which the
// one-workgroup-per-site kernel never reads, all point at the end of info).  *mat, where asked for, gets the matrices' base.
int enkfScratch(sipnet_batch* b, EnkfArgs& a, int32_t* d_site_info, bool workInGlobal, bool perChunk, bool withSrc,
                size_t matPerSite, double** mat, int cap = kMaxVars) {
  const size_t nSites = (size_t)b->n_sites;
  const size_t nWork = workInGlobal ? (size_t)a.nv * (size_t)b->ncol : 0;
  const size_t nCnt = perChunk ? nSites * a.nCh : 0;
  const size_t nPart = nCnt * cap;
  const size_t nStat = perChunk ? nSites * 3 * cap : 0;
  const size_t nMat = nSites * matPerSite;
  const size_t nSite = perChunk ? 2 * nSites : 0;
  const size_t nInt = nSites * 4 + 2 * nCnt + nSite + (withSrc ? nSites : 0);
  const size_t bytes = (nWork + nPart + nStat + nMat) * sizeof(double) + nInt * sizeof(int32_t);
  if (b->enkfBytes < bytes) {
    int rc = waitIdle(b);   // (the old block may still be read by a launch in flight)
    if (rc) return rc;
    if (b->d_enkf) (void)hipFree(b->d_enkf);   // (this block alone: the smoother's may be in use by this very call)
    b->d_enkf = nullptr;
    b->enkfBytes = 0;
    HIP_TRY(hipMalloc(&b->d_enkf, bytes));
    b->enkfBytes = bytes;
  }
  a.work = (double*)b->d_enkf;
  a.part = a.work + nWork;
  a.stat = a.part + nPart;
  double* matrices = a.stat + nStat;
  int32_t* ints = (int32_t*)(matrices + nMat);
  a.info = d_site_info ? d_site_info : ints;
  a.cnt = ints + nSites * 4;
  a.kept = a.cnt + nCnt;
  a.site = a.kept + nCnt;
  a.src = withSrc ? a.site + nSite : nullptr;
  if (mat) *mat = matrices;
  return 0;
}

// the grids of the per-chunk launches: sites x chunks of 256 members, and sites
dim3 chunkGrid(const sipnet_batch* b, const EnkfArgs& a) { return dim3((unsigned)b->n_sites, (unsigned)a.nCh); }
dim3 siteGrid(const sipnet_batch* b) { return dim3((unsigned)b->n_sites); }

// the front of the per-chunk launches: the load (the planes' elements float or double), the codes, the sites that a
// localization's sources reach (L), the inflation
template <class A>
void enkfFront(const sipnet_batch* b, const A& a, int32_t elem_is_f32, const sipnet_enkf_local* L, hipStream_t stream) {
  const dim3 chunks = chunkGrid(b, a), sites = siteGrid(b);
  hipLaunchKernelGGL((elem_is_f32 ? enkfLoadKernel<float, A> : enkfLoadKernel<double, A>), chunks, dim3(256), 0, stream, a);
  hipLaunchKernelGGL(enkfCodeKernel<A>, sites, dim3(256), 0, stream, a);
  if (L)
    hipLaunchKernelGGL(enkfReachKernel, dim3((sites.x + 255) / 256), dim3(256), 0, stream, a, L->d_inPtr, L->d_in,
                       (int64_t)b->n_sites);
  bool inflation = a.infl != nullptr;
  if constexpr (A::kJoint) inflation = inflation || a.prmInfl != nullptr;
  if (inflation) {
    hipLaunchKernelGGL(enkfPartialKernel<A>, chunks, dim3(256), 0, stream, a, -1, 0);
    hipLaunchKernelGGL(enkfFinalKernel<A>, sites, dim3(256), 0, stream, a, -1, 0);
    hipLaunchKernelGGL(enkfUpdateKernel<A>, chunks, dim3(256), 0, stream, a, -1);
  }
}

// the tail of every analysis: the limits and the info of the per-chunk launches (perChunk: the one-workgroup-per-site kernel
// has done its own), the launches' error, what sipnet_batch_pf_info reports, the batch busy on the stream
template <class A>
int enkfEnd(sipnet_batch* b, const A& a, bool perChunk, int32_t fused, int32_t grid, hipStream_t stream) {
  if (perChunk) {
    hipLaunchKernelGGL(enkfLimitKernel<A>, chunkGrid(b, a), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(enkfInfoKernel<A>, siteGrid(b), dim3(256), 0, stream, a);
  }
  HIP_TRY(hipGetLastError());
  b->pfInfo.fused = fused;
  b->pfInfo.grid = grid;
  b->pfInfo.budget = 0;
  b->pfInfo.nSlots = b->ncol;
  return markBusy(b, stream);
}

// the per-site analysis between enkfBegin and the end of the call, for the per-site call's arguments or the joint call's
template <class A>
int enkfSites(sipnet_batch* b, A& a, int32_t n_obs, int32_t elem_is_f32, int32_t* d_site_info, hipStream_t stream) {
  const int64_t nSites = b->n_sites, M = b->n_members;
  // the per-chunk launches unless the sites outnumber the CUs four times over (profiles/r08_enkf_sites_time.txt: one
  // workgroup per site loses or ties at every shape up to 256 sites x 1 024 members -- 0.29 ms against 0.19); big sites or
  // SIPNET_KOPT_PF_MULTI_LAUNCH: always the launches
  const bool group = M <= 256 * kMaxGroupChunks && nSites >= 4 * (int64_t)b->numCUs &&
                     !(b->kernelOptions & SIPNET_KOPT_PF_MULTI_LAUNCH);
  const size_t ldsBytes = (size_t)a.nv * (size_t)M * sizeof(double);
  a.useLds = group && ldsBytes <= (size_t)kLdsWork;
  const auto siteKernel = elem_is_f32 ? enkfSiteKernel<float, A> : enkfSiteKernel<double, A>;
  if constexpr (A::kJoint)
    if (a.useLds) {   // (31 KB of static LDS and the working copies can pass 64 KB together: ask first, as the block-local analysis does)
      int ldsMax = 0;
      hipFuncAttributes attr;
      HIP_TRY(hipDeviceGetAttribute(&ldsMax, hipDeviceAttributeMaxSharedMemoryPerBlock, b->device));
      HIP_TRY(hipFuncGetAttributes(&attr, (const void*)siteKernel));
      if (ldsBytes + attr.sharedSizeBytes > (size_t)ldsMax) {
        a.useLds = 0;
      } else if (ldsBytes + attr.sharedSizeBytes > 64 * 1024 &&
                 hipFuncSetAttribute((const void*)siteKernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes) != hipSuccess) {
        (void)hipGetLastError();
        a.useLds = 0;
      }
    }
  int rc = enkfScratch(b, a, d_site_info, /*workInGlobal=*/!a.useLds, /*perChunk=*/!group, /*withSrc=*/false, 0, nullptr, A::kCap);
  if (rc) return rc;
  if (group) {
    hipLaunchKernelGGL(siteKernel, siteGrid(b), dim3(256), a.useLds ? ldsBytes : 0, stream, a);
  } else {
    const dim3 chunks = chunkGrid(b, a), sites = siteGrid(b);
    enkfFront(b, a, elem_is_f32, nullptr, stream);
    for (int i = 0; i < n_obs; i++) {
      hipLaunchKernelGGL(enkfPartialKernel<A>, chunks, dim3(256), 0, stream, a, i, 0);
      hipLaunchKernelGGL(enkfFinalKernel<A>, sites, dim3(256), 0, stream, a, i, 0);
      hipLaunchKernelGGL(enkfPartialKernel<A>, chunks, dim3(256), 0, stream, a, i, 1);
      hipLaunchKernelGGL(enkfFinalKernel<A>, sites, dim3(256), 0, stream, a, i, 1);
      hipLaunchKernelGGL(enkfUpdateKernel<A>, chunks, dim3(256), 0, stream, a, i);
    }
  }
  return enkfEnd(b, a, /*perChunk=*/!group, group ? 1 : 0, group ? (int32_t)b->n_sites : 0, stream);
}

// the checks of a localization's lists (withRho: and of its tapers)
int localLists(const char* name, int32_t nSites, int32_t nObs, const int64_t* ptr, const int32_t* nbr, const double* rho,
               bool withRho) {
  if (nObs < 1 || nObs > kMaxObs) return refuse(name, "n_obs must be 1..16");
  if (nSites < 1 || (int64_t)nSites * nObs > INT32_MAX) return refuse(name, "n_sites must be >= 1 (and n_sites x n_obs < 2^31)");
  if (!ptr) return refuse(name, "a NULL nbr_ptr");
  if (ptr[0] != 0) return refuse(name, "nbr_ptr[0] must be 0");
  for (int32_t s = 0; s < nSites; s++)
    if (ptr[s + 1] < ptr[s]) return refuse(name, "nbr_ptr must be non-decreasing (site " + std::to_string(s) + ")");
  if (ptr[nSites] > 0 && (!nbr || (withRho && !rho))) return refuse(name, "a NULL nbr or rho with neighbours listed");
  for (int32_t s = 0; s < nSites; s++)
    for (int64_t k = ptr[s]; k < ptr[s + 1]; k++) {
      const std::string at = "site " + std::to_string(s) + ", entry " + std::to_string(k - ptr[s]) + ": ";
      if (nbr[k] < 0 || nbr[k] >= nSites) return refuse(name, at + "neighbour index out of range");
      if (nbr[k] == s) return refuse(name, at + "a site is not its own neighbour");
      if (k > ptr[s] && nbr[k] <= nbr[k - 1]) return refuse(name, at + "a row must be strictly ascending (no duplicates)");
      if (withRho && !(rho[k] > 0.0 && rho[k] <= 1.0)) return refuse(name, at + "rho must be finite and in (0, 1]");
    }
  return 0;
}
// The localization's lists checked, and the greedy schedule of the slots (s, i) in serial order: level(s, i) = 1 + the last
// level that touched a site of F(s) = {s} + nbr(s) (none: -1, so empty lists give level i).  Conflicting slots (footprints that
// meet) are therefore in serial order, and the slots of one level have disjoint footprints.  level: [n_sites][n_obs].
int localSchedule(const char* name, int32_t nSites, int32_t nObs, const int64_t* ptr, const int32_t* nbr, const double* rho,
                  std::vector<int32_t>& level, int32_t* nLevels) {
  int rc = localLists(name, nSites, nObs, ptr, nbr, rho, true);
  if (rc) return rc;
  std::vector<int32_t> last((size_t)nSites, -1);
  level.assign((size_t)nSites * nObs, 0);
  int32_t top = -1;
  for (int32_t s = 0; s < nSites; s++)
    for (int32_t i = 0; i < nObs; i++) {
      int32_t l = last[s];
      for (int64_t k = ptr[s]; k < ptr[s + 1]; k++) l = last[nbr[k]] > l ? last[nbr[k]] : l;
      l += 1;
      last[s] = l;
      for (int64_t k = ptr[s]; k < ptr[s + 1]; k++) last[nbr[k]] = l;
      level[(size_t)s * nObs + i] = l;
      top = l > top ? l : top;
    }
  *nLevels = top + 1;
  return 0;
}
// n_obs x (1 + in-neighbours) of every site: the most rows a target of the block-local analysis can have
std::vector<int32_t> localRows(int32_t nSites, int32_t nObs, const int64_t* ptr, const int32_t* nbr) {
  std::vector<int32_t> rows((size_t)nSites, nObs);
  for (int64_t e = 0; e < ptr[nSites]; e++) {
    int32_t& r = rows[(size_t)nbr[e]];
    r = r > INT32_MAX - nObs ? INT32_MAX : r + nObs;
  }
  return rows;
}

// the checks the two analyses with a localization open with
int localChecks(const char* name, const sipnet_batch* b, const sipnet_enkf_local* L, int32_t n_obs) {
  if (!b || !L) return refuse(name, "a NULL batch or localization");
  if (L->b != b) return refuse(name, "the localization belongs to another batch");
  if (L->nObs != n_obs) return refuse(name, "the localization was made for n_obs = " + std::to_string(L->nObs));
  if (b->n_members > 256 * kMaxGroupChunks) return refuse(name, "at most 4096 members per site");
  return 0;
}


// ---- the joint analysis's parameters ------------------------------------------------------------------------------------------
const char* const kParamName[SIPNET_NPARAMS] = {
#define SIPNET_PARAM(index, field, file_name, rule) #field,
#include "../../include/sipnet_params.def"
#undef SIPNET_PARAM
};
// convertParamsKernel's per-year -> per-day rows: the converted value is the file value / 365.0
bool rateRow(int p) {
  switch (p) {
    case SP_baseVegResp: case SP_litterBreakdownRate: case SP_baseSoilResp: case SP_woodTurnoverRate:
    case SP_leafTurnoverRate: case SP_fineRootTurnoverRate: case SP_coarseRootTurnoverRate:
    case SP_baseCoarseRootResp: case SP_baseFineRootResp: return true;
    default: return false;
  }
}
// why row p cannot be analysed, or null: its converted value is neither the file value nor the file value / 365, or only
// setup reads it
const char* refusedRow(int p) {
  switch (p) {
    case SP_psnTMax: case SP_coarseRootAllocation:
      return "a derived row (rewritten from the rows it depends on)";
    case SP_plantWoodInit: case SP_laiInit: case SP_soilInit: case SP_soilWFracInit: case SP_litterInit: case SP_snowInit:
    case SP_minNInit: case SP_soilOrgNInit: case SP_litterOrgNInit: case SP_plantStorageNInit:
      return "an initial condition, which only setup reads";
    case SP_leafOnDay: case SP_leafOffDay: case SP_gddLeafOn: case SP_soilTempLeafOn:
      return "a phenology threshold (the gddLeafOn row is overloaded by the leaf-on mode)";
    case SP_fAnoxia: case SP_anaerobicDecompRate:
      return "a row the conversion clamps";
    default: return nullptr;
  }
}
// sipnet_enkf_params_check's checks; lo / hi (may be null): the bounds in converted units, by the conversion's own expression
int paramsCheck(const char* name, int32_t n, const sipnet_enkf_param* params, double* lo, double* hi) {
  if (n < 0 || n > kMaxPrm) return refuse(name, "n_params must be 0..16");
  if (n > 0 && !params) return refuse(name, "NULL params with n_params > 0");
  for (int k = 0; k < n; k++) {
    const sipnet_enkf_param& q = params[k];
    const std::string at = "parameter " + std::to_string(k) + ": ";
    if (q.index < 0 || q.index >= SIPNET_NPARAMS) return refuse(name, at + "index is not a parameter index");
    const std::string who = at + kParamName[q.index] + " ";
    if (const char* why = refusedRow(q.index)) return refuse(name, who + "is " + why);
    for (int e = 0; e < k; e++)
      if (params[e].index == q.index) return refuse(name, who + "is listed twice");
    if (!(fabs(q.lo) < INFINITY) || !(fabs(q.hi) < INFINITY)) return refuse(name, who + "has a bound that is not finite");
    if (!(q.lo < q.hi)) return refuse(name, who + "needs lo < hi");
    double l = q.lo, h = q.hi;
    if (rateRow(q.index)) {
      l /= 365.0;
      h /= 365.0;
    }
    if (lo) lo[k] = l;
    if (hi) hi[k] = h;
  }
  return 0;
}


// ---- the smoother's host side ----------------------------------------------------------------------------------------------
// the refusals of the series, before any launch
int smoothChecks(const char* name, const sipnet_batch* b, int32_t nSeries, const sipnet_enkf_series* series) {
  if (nSeries < 0 || nSeries > kMaxSeries) return refuse(name, "n_series must be 0.." + std::to_string(kMaxSeries));
  if (nSeries > 0 && !series) return refuse(name, "NULL series with n_series > 0");
  if (nSeries > 0 && b->n_members > 256 * kMaxGroupChunks) return refuse(name, "series need at most 4096 members per site");
  for (int k = 0; k < nSeries; k++) {
    const sipnet_enkf_series& q = series[k];
    const std::string at = "series " + std::to_string(k) + ": ";
    if (!q.src || !q.dst) return refuse(name, at + "a NULL src or dst");
    if (q.rows < 1) return refuse(name, at + "rows must be >= 1");
    if (q.ld < b->ncol) return refuse(name, at + "ld must be >= ncol");
    for (int e = 0; e < nSeries; e++) {
      if (e < k && series[e].dst == q.dst) return refuse(name, at + "its dst is also the dst of series " + std::to_string(e));
      if (e != k && series[e].src == q.dst) return refuse(name, at + "its dst is the src of series " + std::to_string(e));
    }
  }
  return 0;
}

// What the series stage keeps between its two halves.  The first half (smoothFront, before the pool analysis: it reads the
// forecast state and planes) forms the inflated h by enkfFront on a working copy of the stage's own and reduces them to a, g
// and G; the second (smoothSeries, after it: a series may be a plane the pool analysis reads) smooths the series.  The stage
// has its own scratch block, so the pool analysis runs on exactly what it runs on without series.
struct SmoothStage {
  SmoothArgs k;
  bool useLds = false;
  size_t ldsBytes = 0;
  int32_t blocks = 0;
};
// the kernel of a site of M members: teams of one wave up to 1 024 members (kCh = members a lane holds), else sixteen waves
template <bool kLds>
const void* smoothKernelOf(int64_t M) {
  if (M <= 64) return (const void*)enkfSmoothKernel<kLds, 1, 1>;
  if (M <= 128) return (const void*)enkfSmoothKernel<kLds, 1, 2>;
  if (M <= 256) return (const void*)enkfSmoothKernel<kLds, 1, 4>;
  if (M <= 512) return (const void*)enkfSmoothKernel<kLds, 1, 8>;
  if (M <= 1024) return (const void*)enkfSmoothKernel<kLds, 1, 16>;
  if (M <= 2048) return (const void*)enkfSmoothKernel<kLds, 16, 2>;
  return (const void*)enkfSmoothKernel<kLds, 16, 4>;
}

int smoothFront(sipnet_batch* b, const JointArgs& joint, int32_t elem_is_f32, int32_t nSeries, const sipnet_enkf_series* series,
                hipStream_t stream, SmoothStage& st) {
  const size_t nSites = (size_t)b->n_sites, ncol = (size_t)b->ncol;
  JointArgs a = joint;   // the h alone: no analysed pool, no analysed parameter (the codes still check both lambdas)
  a.nPool = a.nPrm = a.nA = 0;
  a.nv = a.nObs;
  a.useLds = 0;
  a.info = nullptr;
  a.src = nullptr;
  // the stage's block: the h, then their anomalies [n_obs][ncol] | part | stat | a site's g, G, p, n | cnt | site
  constexpr size_t cap = JointArgs::kCap;
  const size_t nWork = (size_t)a.nObs * ncol, nCnt = nSites * (size_t)a.nCh, nPart = nCnt * cap, nStat = nSites * 3 * cap,
               nMeta = nSites * kMeta;
  const size_t bytes = (nWork + nPart + nStat + nMeta) * sizeof(double) + (nCnt + 2 * nSites) * sizeof(int32_t);
  if (b->smoothBytes < bytes) {
    int rc = waitIdle(b);   // (the old block may still be read by a launch in flight)
    if (rc) return rc;
    if (b->d_smooth) HIP_TRY(hipFree(b->d_smooth));
    b->d_smooth = nullptr;
    b->smoothBytes = 0;
    HIP_TRY(hipMalloc(&b->d_smooth, bytes));
    b->smoothBytes = bytes;
  }
  a.work = (double*)b->d_smooth;
  a.part = a.work + nWork;
  a.stat = a.part + nPart;
  double* meta = a.stat + nStat;
  a.cnt = (int32_t*)(meta + nMeta);
  a.kept = a.cnt;   // (never written: the stage has no limits)
  a.site = a.cnt + nCnt;

  SmoothArgs& k = st.k;
  k = SmoothArgs{};
  k.nSeries = nSeries;
  int64_t totalRows = 0;
  for (int e = 0; e < nSeries; e++) totalRows += series[e].rows;
  // rows per workgroup: at least 16 (staging a site's anomalies costs about p / 2 rows' traffic, and a workgroup of one-wave
  // teams has four rows in flight), more once that still leaves eight workgroups per CU
  const int64_t want = totalRows * (int64_t)nSites / (8 * (int64_t)std::max(b->numCUs, 1));
  k.run = (int32_t)std::min<int64_t>(64, std::max<int64_t>(16, want));
  int64_t blocks = 0;
  for (int e = 0; e < nSeries; e++) {
    k.ser[e] = SmoothSeries{series[e].src, series[e].dst, series[e].ld, series[e].rows, series[e].elem_is_f32 ? 1 : 0, (int32_t)blocks, 0};
    blocks += (series[e].rows + k.run - 1) / k.run;
  }
  if (blocks > 65535) return refuse("sipnet_batch_enkf_analysis_smooth", "the series have too many rows for one launch");
  st.blocks = (int32_t)blocks;
  k.anom = a.work;
  k.meta = meta;
  k.site = a.site;
  k.infl = a.infl;
  k.siteStatus = a.siteStatus;
  k.status = a.state + (int64_t)ST_status * a.ncol;
  k.ncol = a.ncol;
  k.M = a.M;
  // the anomalies in LDS when [n_obs][M] fits beside the kernel's tables (SIPNET_KOPT_PF_MULTI_LAUNCH: always from scratch)
  st.ldsBytes = (size_t)a.nObs * (size_t)a.M * sizeof(double);
  st.useLds = !(b->kernelOptions & SIPNET_KOPT_PF_MULTI_LAUNCH);
  if (st.useLds) {
    int ldsMax = 0;
    hipFuncAttributes attr;
    const void* kernel = smoothKernelOf<true>(a.M);
    HIP_TRY(hipDeviceGetAttribute(&ldsMax, hipDeviceAttributeMaxSharedMemoryPerBlock, b->device));
    HIP_TRY(hipFuncGetAttributes(&attr, kernel));
    if (st.ldsBytes + attr.sharedSizeBytes > (size_t)ldsMax) {
      st.useLds = false;
    } else if (st.ldsBytes + attr.sharedSizeBytes > 48 * 1024 &&
               hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)st.ldsBytes) != hipSuccess) {
      (void)hipGetLastError();
      st.useLds = false;
    }
  }
  enkfFront(b, a, elem_is_f32, nullptr, stream);
  hipLaunchKernelGGL(enkfSmoothPrepKernel, siteGrid(b), dim3(256), 0, stream, a, meta);
  HIP_TRY(hipGetLastError());
  return 0;
}

int smoothSeries(sipnet_batch* b, const SmoothStage& st, hipStream_t stream) {
  const dim3 grid((unsigned)b->n_sites, (unsigned)st.blocks);
  void* args[] = {(void*)&st.k};
  const void* kernel = st.useLds ? smoothKernelOf<true>(st.k.M) : smoothKernelOf<false>(st.k.M);
  HIP_TRY(hipLaunchKernel(kernel, grid, dim3(st.k.M <= 1024 ? 256 : 1024), args, st.useLds ? st.ldsBytes : 0, stream));
  return markBusy(b, stream);
}

// sipnet_batch_enkf_analysis_joint, and with series sipnet_batch_enkf_analysis_smooth
int jointCall(const char* name, sipnet_batch* b, int32_t n_obs, const sipnet_enkf_obs* ops, int32_t analysed_mask, int32_t n_params,
              const sipnet_enkf_param* params, const void* const d_planes[3], int32_t elem_is_f32, int32_t n_steps, int64_t ld,
              const double* d_obs, const double* d_sd, const double* d_inflation, const double* d_param_inflation,
              int32_t n_series, const sipnet_enkf_series* series, int32_t* d_site_info, hipStream_t stream) {
  JointArgs a{};
  int rc = paramsCheck(name, n_params, params, a.lo, a.hi);
  if (rc) return rc;
  if (b && (rc = smoothChecks(name, b, n_series, series))) return rc;
  if (b && d_param_inflation && !d_site_info && !b->pfPeers) {   // the synchronous form: checked before anything is launched
    rc = useDevice(b);
    if (rc) return rc;
    std::vector<double> infl((size_t)b->n_sites);
    HIP_TRY(hipMemcpyAsync(infl.data(), d_param_inflation, infl.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (size_t s = 0; s < infl.size(); s++)
      if (!(infl[s] >= 1.0) || !(infl[s] < INFINITY))
        return refuse(name, "site " + std::to_string(s) + ": bad input (the parameter inflation must be finite and >= 1); "
                            "nothing was written");
  }
  // (enkfBegin fills the arguments the analyses share and leaves the bounds alone)
  rc = enkfBegin(name, b, n_obs, ops, analysed_mask, d_planes, n_steps, ld, d_obs, d_sd, d_inflation, d_site_info, stream, a);
  if (rc) return rc;
  rc = materializeParams(b, stream);   // (every column its own rows: the limits write them)
  if (rc) return rc;
  a.prm = b->d_prm;
  a.prmPitch = b->ncol;
  a.prmId = nullptr;
  a.prmOut = b->d_prm;
  a.prmInfl = d_param_inflation;
  a.nPool = a.nA;
  a.nPrm = n_params;
  a.nA += n_params;
  a.nv += n_params;
  a.leaf = a.wood = a.fineRoot = a.opt = a.tmin = -1;
  for (int k = 0; k < n_params; k++) {
    const int p = params[k].index;
    a.prmRow[k] = p;
    if (p == SP_leafAllocation) a.leaf = k;
    if (p == SP_woodAllocation) a.wood = k;
    if (p == SP_fineRootAllocation) a.fineRoot = k;
    if (p == SP_psnTOpt) a.opt = k;
    if (p == SP_psnTMin) a.tmin = k;
  }
  if (n_series == 0) return enkfSites(b, a, n_obs, elem_is_f32, d_site_info, stream);
  SmoothStage st;
  rc = smoothFront(b, a, elem_is_f32, n_series, series, stream, st);
  if (rc) return rc;
  rc = enkfSites(b, a, n_obs, elem_is_f32, d_site_info, stream);
  if (rc) return rc;
  return smoothSeries(b, st, stream);
}

}  // namespace

extern "C" {

int sipnet_batch_enkf_analysis_sites(sipnet_batch* b, int32_t n_obs, const sipnet_enkf_obs* ops, int32_t analysed_mask,
                                     const void* const d_planes[3], int32_t elem_is_f32, int32_t n_steps, int64_t ld,
                                     const double* d_obs, const double* d_sd, const double* d_inflation,
                                     int32_t* d_site_info, void* hip_stream) {
  hipStream_t stream = (hipStream_t)hip_stream;
  EnkfArgs a;
  int rc = enkfBegin("sipnet_batch_enkf_analysis_sites", b, n_obs, ops, analysed_mask, d_planes, n_steps, ld, d_obs, d_sd,
                     d_inflation, d_site_info, stream, a);
  if (rc) return rc;
  return enkfSites(b, a, n_obs, elem_is_f32, d_site_info, stream);
}

int sipnet_enkf_params_check(int32_t n_params, const sipnet_enkf_param* params, double* lo_converted, double* hi_converted) {
  return paramsCheck("sipnet_enkf_params_check", n_params, params, lo_converted, hi_converted);
}

int sipnet_batch_enkf_analysis_joint(sipnet_batch* b, int32_t n_obs, const sipnet_enkf_obs* ops, int32_t analysed_mask,
                                     int32_t n_params, const sipnet_enkf_param* params, const void* const d_planes[3],
                                     int32_t elem_is_f32, int32_t n_steps, int64_t ld, const double* d_obs, const double* d_sd,
                                     const double* d_inflation, const double* d_param_inflation, int32_t* d_site_info,
                                     void* hip_stream) {
  return jointCall("sipnet_batch_enkf_analysis_joint", b, n_obs, ops, analysed_mask, n_params, params, d_planes, elem_is_f32, n_steps,
                   ld, d_obs, d_sd, d_inflation, d_param_inflation, 0, nullptr, d_site_info, (hipStream_t)hip_stream);
}

int sipnet_batch_enkf_analysis_smooth(sipnet_batch* b, int32_t n_obs, const sipnet_enkf_obs* ops, int32_t analysed_mask,
                                      int32_t n_params, const sipnet_enkf_param* params, const void* const d_planes[3],
                                      int32_t elem_is_f32, int32_t n_steps, int64_t ld, const double* d_obs, const double* d_sd,
                                      const double* d_inflation, const double* d_param_inflation, int32_t n_series,
                                      const sipnet_enkf_series* series, int32_t* d_site_info, void* hip_stream) {
  return jointCall("sipnet_batch_enkf_analysis_smooth", b, n_obs, ops, analysed_mask, n_params, params, d_planes, elem_is_f32, n_steps,
                   ld, d_obs, d_sd, d_inflation, d_param_inflation, n_series, series, d_site_info, (hipStream_t)hip_stream);
}

int sipnet_batch_get_params(sipnet_batch* b, double* params, int32_t file_units, void* hip_stream) {
  const char* name = "sipnet_batch_get_params";
  if (!b || !params) return refuse(name, "a NULL batch or params");
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  rc = orderBehindBusy(b, stream);
  if (rc) return rc;
  rc = flushParams(b, stream);
  if (rc) return rc;
  // the rows a column carries: its own, or those of the column its index names (in the bank of a connected filter)
  const bool indexed = b->prmIndexed;
  const double* src = indexed && b->d_prmBank ? b->d_prmBank : b->d_prm;
  const int64_t pitch = indexed && b->d_prmBank ? b->prmBankPitch : b->ncol, ncol = b->ncol;
  std::vector<double> rows((size_t)pitch * SIPNET_NPARAMS);
  std::vector<int32_t> id(indexed ? (size_t)ncol : 0);
  HIP_TRY(hipMemcpyAsync(rows.data(), src, rows.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (indexed) HIP_TRY(hipMemcpyAsync(id.data(), b->d_prmId, id.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int p = 0; p < SIPNET_NPARAMS; p++) {
    const bool rate = file_units && rateRow(p);
    for (int64_t c = 0; c < ncol; c++) {
      const double v = rows[(size_t)p * pitch + (indexed ? (int64_t)id[c] : c)];
      params[c * SIPNET_NPARAMS + p] = rate ? v * 365.0 : v;
    }
  }
  return SIPNET_OK;
}

int sipnet_enkf_local_schedule(int32_t n_sites, int32_t n_obs, const int64_t* nbr_ptr, const int32_t* nbr, const double* rho,
                               int32_t* level_of_slot, int32_t* n_levels) {
  if (!n_levels) return refuse("sipnet_enkf_local_schedule", "a NULL n_levels");
  std::vector<int32_t> level;
  int rc = localSchedule("sipnet_enkf_local_schedule", n_sites, n_obs, nbr_ptr, nbr, rho, level, n_levels);
  if (rc) return rc;
  if (level_of_slot) std::copy(level.begin(), level.end(), level_of_slot);
  return SIPNET_OK;
}

void sipnet_enkf_local_destroy(sipnet_enkf_local* L) {
  if (!L) return;
  (void)hipSetDevice(L->device);
  if (L->d_pair) (void)hipFree(L->d_pair);
  if (L->d_inPtr) (void)hipFree(L->d_inPtr);
  if (L->d_in) (void)hipFree(L->d_in);
  if (L->d_inRho) (void)hipFree(L->d_inRho);
  delete L;
}

int sipnet_batch_enkf_local_create(sipnet_batch* b, int32_t n_obs, const int64_t* nbr_ptr, const int32_t* nbr,
                                   const double* rho, sipnet_enkf_local** out) {
  const char* name = "sipnet_batch_enkf_local_create";
  if (!b || !out) return refuse(name, "a NULL batch or out");
  *out = nullptr;
  std::vector<int32_t> level;
  int32_t nLevels = 0;
  const int32_t nSites = b->n_sites;
  int rc = localSchedule(name, nSites, n_obs, nbr_ptr, nbr, rho, level, &nLevels);
  if (rc) return rc;
  rc = useDevice(b);
  if (rc) return rc;
  // the pairs sorted by level; within a level by slot in serial order, a slot's own site first
  std::vector<int64_t> levelOff((size_t)nLevels + 1, 0);
  for (int32_t s = 0; s < nSites; s++)
    for (int32_t i = 0; i < n_obs; i++) levelOff[(size_t)level[(size_t)s * n_obs + i] + 1] += 1 + (nbr_ptr[s + 1] - nbr_ptr[s]);
  for (int32_t l = 0; l < nLevels; l++) levelOff[l + 1] += levelOff[l];
  std::vector<LocalPair> pairs((size_t)levelOff[nLevels]);
  std::vector<int64_t> fill(levelOff.begin(), levelOff.end() - 1), slotOff((size_t)nSites * n_obs);
  std::vector<int32_t> slotLen((size_t)nSites * n_obs);
  for (int32_t s = 0; s < nSites; s++)
    for (int32_t i = 0; i < n_obs; i++) {
      int64_t& k = fill[level[(size_t)s * n_obs + i]];
      slotOff[(size_t)s * n_obs + i] = k;
      slotLen[(size_t)s * n_obs + i] = (int32_t)(1 + nbr_ptr[s + 1] - nbr_ptr[s]);
      pairs[(size_t)k++] = LocalPair{s, i, s, 1.0};
      for (int64_t e = nbr_ptr[s]; e < nbr_ptr[s + 1]; e++) pairs[(size_t)k++] = LocalPair{s, i, nbr[e], rho[e]};
    }
  // the in-neighbour lists: site t is reached from the sites that list it
  std::vector<int64_t> inPtr((size_t)nSites + 1, 0);
  for (int64_t e = 0; e < nbr_ptr[nSites]; e++) inPtr[(size_t)nbr[e] + 1]++;
  for (int32_t t = 0; t < nSites; t++) inPtr[t + 1] += inPtr[t];
  std::vector<int32_t> in((size_t)inPtr[nSites]);
  std::vector<double> inRho(in.size());
  std::vector<int64_t> at(inPtr.begin(), inPtr.end() - 1);
  for (int32_t s = 0; s < nSites; s++)
    for (int64_t e = nbr_ptr[s]; e < nbr_ptr[s + 1]; e++) {
      inRho[(size_t)at[nbr[e]]] = rho[e];
      in[(size_t)at[nbr[e]]++] = s;
    }
  const std::vector<int32_t> rows = localRows(nSites, n_obs, nbr_ptr, nbr);

  sipnet_enkf_local* L = new sipnet_enkf_local;
  L->b = b;
  L->device = b->device;
  L->nSites = nSites;
  L->nObs = n_obs;
  L->nLevels = nLevels;
  L->maxRows = *std::max_element(rows.begin(), rows.end());
  L->levelOff = std::move(levelOff);
  L->slotOff = std::move(slotOff);
  L->slotLen = std::move(slotLen);
  auto upload = [](void** d, const void* h, size_t bytes) -> int {
    HIP_TRY(hipMalloc(d, bytes > 0 ? bytes : 8));
    if (bytes) HIP_TRY(hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice));
    return 0;
  };
  if ((rc = upload((void**)&L->d_pair, pairs.data(), pairs.size() * sizeof(LocalPair))) ||
      (rc = upload((void**)&L->d_inPtr, inPtr.data(), inPtr.size() * sizeof(int64_t))) ||
      (rc = upload((void**)&L->d_in, in.data(), in.size() * sizeof(int32_t))) ||
      (rc = upload((void**)&L->d_inRho, inRho.data(), inRho.size() * sizeof(double)))) {
    sipnet_enkf_local_destroy(L);
    return rc;
  }
  *out = L;
  return SIPNET_OK;
}

int32_t sipnet_enkf_local_levels(const sipnet_enkf_local* L) { return L ? L->nLevels : 0; }

int sipnet_debug_enkf_local_serial(sipnet_enkf_local* L, int32_t on) {
  if (!L) return refuse("sipnet_debug_enkf_local_serial", "a NULL localization");
  L->serial = on != 0;
  return SIPNET_OK;
}

int sipnet_batch_enkf_analysis_local(sipnet_batch* b, const sipnet_enkf_local* L, int32_t n_obs, const sipnet_enkf_obs* ops,
                                     int32_t analysed_mask, const void* const d_planes[3], int32_t elem_is_f32,
                                     int32_t n_steps, int64_t ld, const double* d_obs, const double* d_sd,
                                     const double* d_inflation, int32_t* d_site_info, void* hip_stream) {
  const char* name = "sipnet_batch_enkf_analysis_local";
  int rc = localChecks(name, b, L, n_obs);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  EnkfArgs a;
  rc = enkfBegin(name, b, n_obs, ops, analysed_mask, d_planes, n_steps, ld, d_obs, d_sd, d_inflation, d_site_info, stream, a);
  if (rc) return rc;
  rc = enkfScratch(b, a, d_site_info, /*workInGlobal=*/true, /*perChunk=*/true, /*withSrc=*/true, 0, nullptr);
  if (rc) return rc;
  enkfFront(b, a, elem_is_f32, L, stream);
  if (L->serial) {
    for (size_t k = 0; k < L->slotOff.size(); k++)
      hipLaunchKernelGGL(enkfLocalKernel, dim3((unsigned)L->slotLen[k]), dim3(256), 0, stream, a, L->d_pair, L->slotOff[k]);
  } else {
    for (int32_t l = 0; l < L->nLevels; l++)
      hipLaunchKernelGGL(enkfLocalKernel, dim3((unsigned)(L->levelOff[l + 1] - L->levelOff[l])), dim3(256), 0, stream, a,
                         L->d_pair, L->levelOff[l]);
  }
  return enkfEnd(b, a, /*perChunk=*/true, 0, 0, stream);
}

int sipnet_enkf_local_rows(int32_t n_sites, int32_t n_obs, const int64_t* nbr_ptr, const int32_t* nbr, int32_t* rows_of_site,
                           int32_t* max_rows) {
  int rc = localLists("sipnet_enkf_local_rows", n_sites, n_obs, nbr_ptr, nbr, nullptr, false);
  if (rc) return rc;
  const std::vector<int32_t> rows = localRows(n_sites, n_obs, nbr_ptr, nbr);
  if (rows_of_site) std::copy(rows.begin(), rows.end(), rows_of_site);
  if (max_rows) *max_rows = *std::max_element(rows.begin(), rows.end());
  return SIPNET_OK;
}

int sipnet_batch_enkf_analysis_block(sipnet_batch* b, const sipnet_enkf_local* L, int32_t n_obs, const sipnet_enkf_obs* ops,
                                     int32_t analysed_mask, const void* const d_planes[3], int32_t elem_is_f32,
                                     int32_t n_steps, int64_t ld, const double* d_obs, const double* d_sd,
                                     const double* d_inflation, int32_t* d_site_info, int32_t* d_rows, void* hip_stream) {
  const char* name = "sipnet_batch_enkf_analysis_block";
  int rc = localChecks(name, b, L, n_obs);
  if (rc) return rc;
  if (L->maxRows > kBlockRows)
    return refuse(name, "a site has " + std::to_string(L->maxRows) + " rows (n_obs x (1 + in-neighbours)); at most " +
                            std::to_string(kBlockRows) + " (SIPNET_ENKF_BLOCK_MAX_ROWS, sipnet_enkf_local_rows)");
  hipStream_t stream = (hipStream_t)hip_stream;
  EnkfArgs a;
  rc = enkfBegin(name, b, n_obs, ops, analysed_mask, d_planes, n_steps, ld, d_obs, d_sd, d_inflation, d_site_info, stream, a);
  if (rc) return rc;
  // the matrices of every target in LDS, where the staging tile was, when the largest fits beside the kernel's own LDS
  const size_t matDoubles = blockMatSize(a.nA, L->maxRows), stageDoubles = (size_t)kTile * blockStagePitch(a.nA, L->maxRows);
  int ldsMax = 0;
  hipFuncAttributes attr;
  HIP_TRY(hipDeviceGetAttribute(&ldsMax, hipDeviceAttributeMaxSharedMemoryPerBlock, b->device));
  const bool small = L->maxRows <= kBlockSmall && b->n_members <= 512;
  const void* ldsKernel = small ? (const void*)enkfBlockKernel<true, 256> : (const void*)enkfBlockKernel<true, 1024>;
  HIP_TRY(hipFuncGetAttributes(&attr, ldsKernel));
  const size_t ldsWant = std::max(stageDoubles, matDoubles) * sizeof(double);
  bool useLds = ldsWant + attr.sharedSizeBytes <= (size_t)ldsMax;
  if (useLds && ldsWant > 48 * 1024 &&
      hipFuncSetAttribute(ldsKernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsWant) != hipSuccess) {
    (void)hipGetLastError();
    useLds = false;
  }
  double* mat = nullptr;   // (a target's matrices in its block of the scratch, unless they are in LDS)
  rc = enkfScratch(b, a, d_site_info, /*workInGlobal=*/true, /*perChunk=*/true, /*withSrc=*/true, useLds ? 0 : matDoubles,
                   &mat);
  if (rc) return rc;
  enkfFront(b, a, elem_is_f32, L, stream);
  const size_t dyn = useLds ? ldsWant : stageDoubles * sizeof(double);
  double* matArg = useLds ? nullptr : mat;
  const int64_t matPitch = useLds ? 0 : (int64_t)matDoubles;
  auto launch = [&](auto kernel, int threads) {
    hipLaunchKernelGGL(kernel, siteGrid(b), dim3(threads), dyn, stream, a, L->d_inPtr, L->d_in, L->d_inRho, matArg, matPitch,
                       d_rows);
  };
  if (small) launch(useLds ? enkfBlockKernel<true, 256> : enkfBlockKernel<false, 256>, 256);
  else launch(useLds ? enkfBlockKernel<true, 1024> : enkfBlockKernel<false, 1024>, 1024);
  return enkfEnd(b, a, /*perChunk=*/true, useLds ? 1 : 0, (int32_t)b->n_sites, stream);
}

}  // extern "C"
