// enkf_common.inc -- what every EnKF kernel is written in (enkf.hip includes the parts).  Where the joint analysis differs from
// the per-site one, the difference is a function here, overloaded on (or forked by) the argument type.
constexpr int kMaxObs = 16;
constexpr int kPools = 13;                 // state slots 0..12: the Envi pools
constexpr int kMaxVars = kPools + kMaxObs;
constexpr int kMaxGroupChunks = 16;        // one workgroup per site: sites of at most 16 x 256 members
constexpr int kLdsWork = 40 * 1024;        // ... whose working copies fit here stay in LDS, else in the scratch block
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
  DerivedRows rows;                        // where leafAllocation .. psnTMin are among the analysed parameters
};

__device__ __forceinline__ bool liveAt(const EnkfArgs& a, int s, int64_t j) { return liveIn(a, s, j); }

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
// the lambda of variable q at site s (the joint analysis's parameters have their own), and whether site s inflates at all.
// lam: the site's one lambda, lambdaOf(a, s, 0), as the caller has read it (the joint analysis reads a lambda per class itself)
__device__ __forceinline__ double lambdaOf(const EnkfArgs& a, int s, int) { return a.infl ? a.infl[s] : 1.0; }
__device__ __forceinline__ double lambdaOf(const JointArgs& a, int s, int q) {
  if (q >= a.nPool && q < a.nA) return a.prmInfl ? a.prmInfl[s] : 1.0;
  return a.infl ? a.infl[s] : 1.0;
}
__device__ __forceinline__ bool inflates(const EnkfArgs&, int, double lam) { return lam != 1.0; }
__device__ __forceinline__ bool inflates(const JointArgs& a, int s, double) {
  return (a.infl && a.infl[s] != 1.0) || (a.prmInfl && a.prmInfl[s] != 1.0);
}
// the analysed pools among the variables: the first nA, or the joint analysis's first nPool
__device__ __forceinline__ int poolCount(const EnkfArgs& a) { return a.nA; }
__device__ __forceinline__ int poolCount(const JointArgs& a) { return a.nPool; }

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

// live member j (column col) loaded into its working copies W[v ldw + j]: the analysed pools, the joint analysis's analysed
// parameters, the h
template <typename T, class A>
__device__ __forceinline__ void loadMember(const A& a, double* W, int64_t ldw, int64_t j, int64_t col) {
  const int nPool = poolCount(a);
  for (int q = 0; q < nPool; q++) W[(int64_t)q * ldw + j] = a.state[(int64_t)a.pool[q] * a.ncol + col];
  if constexpr (A::kJoint)
    for (int k = 0; k < a.nPrm; k++) W[(int64_t)(nPool + k) * ldw + j] = a.prmOut[(int64_t)a.prmRow[k] * a.ncol + col];
  for (int i = 0; i < a.nObs; i++) W[(int64_t)(a.nA + i) * ldw + j] = predicted<T>(a, i, col);
}
// live member j of a site that inflates inflated about the means: every variable by the site's lambda (lam =
// lambdaOf(a, s, 0), which the caller reads once per site), or in the joint analysis by the lambda of its class, where a class
// at 1 is left as it is
__device__ __forceinline__ void inflateMember(const EnkfArgs& a, int, double* W, int64_t ldw, int64_t j, const double* mean, double lam) {
  for (int q = 0; q < a.nv; q++) W[(int64_t)q * ldw + j] = inflated(W[(int64_t)q * ldw + j], mean[q], lam);
}
__device__ __forceinline__ void inflateMember(const JointArgs& a, int s, double* W, int64_t ldw, int64_t j, const double* mean, double) {
  for (int q = 0; q < a.nv; q++)
    if (const double l = lambdaOf(a, s, q); l != 1.0) W[(int64_t)q * ldw + j] = inflated(W[(int64_t)q * ldw + j], mean[q], l);
}

// the physical limits of one live member: its analysed pools clipped, then hasSufficientBiomass (sipnet.c:1530-1536) of
// the result; false = the member keeps its forecast.  fin[v] gets the clipped values.
__device__ bool limited(const EnkfArgs& a, int nPool, int64_t col, const double* W, int64_t ldw, int64_t j, double* fin) {
  double f[kPools];
  for (int p = 0; p < kPools; p++) f[p] = a.state[(int64_t)p * a.ncol + col];
  bool finite = true;
  for (int q = 0; q < nPool; q++) {
    const double v = poolLimit(a.pool[q], W[(int64_t)q * ldw + j]);
    finite = finite && fabs(v) < INFINITY;
    fin[q] = v;
    f[a.pool[q]] = v;
  }
  return finite && sufficientBiomass(f[ST_plantWoodC], f[ST_plantCAccountingDelta], f[ST_fineRootC], f[ST_coarseRootC]);
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
  return allocationsOk(a.rows, [&](int k, int row) { return prmNow(a, W, ldw, j, col, k, row); }) && ok;
}
// ... and its rows written: the analysed ones, then the derived rows that depend on them, by convertParamsKernel's expressions
__device__ void writeParams(const JointArgs& a, int64_t col, const double* W, int64_t ldw, int64_t j) {
  for (int k = 0; k < a.nPrm; k++) a.prmOut[(int64_t)a.prmRow[k] * a.ncol + col] = W[(int64_t)(a.nPool + k) * ldw + j];
  writeDerivedRows(a.prmOut, a.ncol, col, a.rows, [&](int k, int row) { return prmNow(a, W, ldw, j, col, k, row); });
}
// one live member through the limits and, unless it keeps its forecast, written back: its analysed pools (and parameters)
template <class A>
__device__ __forceinline__ bool limitAndWrite(const A& a, int64_t col, double* W, int64_t ldw, int64_t j) {
  double fin[kPools];
  const int nPool = poolCount(a);
  bool ok = limited(a, nPool, col, W, ldw, j, fin);
  if constexpr (A::kJoint) ok = limitedParams(a, col, W, ldw, j) && ok;
  if (!ok) return false;
  for (int q = 0; q < nPool; q++) a.state[(int64_t)a.pool[q] * a.ncol + col] = fin[q];
  if constexpr (A::kJoint) writeParams(a, col, W, ldw, j);
  return true;
}

// ---- a site's sums by one workgroup (enkfSiteKernel, enkfLocalKernel, enkfSmoothPrepKernel) --------------------------------
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

// the site's code, as enkfCodeKernel left it
__device__ __forceinline__ int splitCode(const EnkfArgs& a, int s) { return a.site[2 * (int64_t)s]; }
