// pf_sites.inc -- the analysis of a batch of many sites, every site a filter of its own: SitesArgs, pfSitesKernel (one
// workgroup per site) and the split path's three launches (sitesChunkKernel, sitesWeightKernel, sitesAncestorKernel).
// Two weight sources: the sum of a plane against one observation per site (sipnet_batch_pf_analysis_sites), or log-weights
// the caller GIVES (sipnet_batch_pf_resample_sites: tempered by beta, with the effective sample size and the keep rule).

// ---- the analysis of a batch of many sites (sipnet_batch_pf_analysis_sites) -------------------------------------------
// Site s owns columns [s M, (s + 1) M) and is a filter of its own: its own maximum, integer prefix sum and systematic draw, its
// ancestors inside its own range.  Sites never wait for each other: one workgroup per site (pfSitesKernel) when the sites
// are small and at least as many as the CUs, else three launches (sitesChunkKernel | sitesWeightKernel | sitesAncestorKernel)
// -- no grid barrier, no spin, no atomic in either.  The values are pfFixedWeight's and ancestorKernel's rule, so one site gives
// sipnet_batch_pf_analysis's bits.
constexpr int kSitesLds = 4096;      // sites of at most this many particles: one workgroup, the site's weights in LDS (32 KB)
constexpr int kSitesMaxChunks = 1024;   // the split path: chunks per site at most (a chunk: 256 x 1, 2, .. 16 columns)
constexpr long long kSiteMissing = -1, kSiteInvalid = -2;   // site totals of a site without an observation / with bad arguments
constexpr long long kSiteKept = -3;   // given weights: the site's effective sample size is at least its ess_min, it keeps its particles
// 0: analysed; kSiteMissing: obs is NaN; kSiteInvalid: a non-finite obs, sigma not finite and > 0, u0 outside [0, 1)
__device__ __forceinline__ long long siteKind(double obs, double sigma, double u0) {
  if (obs != obs) return kSiteMissing;
  if (!(fabs(obs) < INFINITY) || !(sigma > 0.0) || !(sigma < INFINITY) || !(u0 >= 0.0) || !(u0 < 1.0)) return kSiteInvalid;
  return 0;
}
struct SitesArgs {
  const void* plane;
  int32_t nSteps;
  int64_t ld;
  int64_t M;                  // particles per site
  int32_t nChunks;            // split path: chunks per site
  int32_t chunk;              // ... of `chunk` columns: 256 x the smallest power of two that needs at most kSitesMaxChunks
  const double* status;
  const double* obs;          // [n_sites]
  const double* sigma;
  const double* u0;
  double* logw;               // [ncol]
  int64_t* w;                 // [ncol] fixed-point weights: the caller's, or scratch (split path; pfSitesKernel: may be null)
  int32_t* anc;               // [ncol] global columns
  int64_t* total;             // [n_sites] scratch, always written
  int64_t* totalOut;          // [n_sites] the caller's, may be null
  double* chunkMax;           // split path: [n_sites][nChunks]
  int64_t* chunkSum;          // [n_sites][nChunks]
  int64_t* threadIncl;        // [n_sites][nChunks][256] every thread's inclusive sum inside its chunk
  // given weights only (Given = true: logw is read, plane / obs / sigma are not)
  const double* beta;         // [n_sites] or null (1, the product is not formed)
  const double* essMin;       // [n_sites] or null (every site resamples, logw is not written)
  double* ess;                // [n_sites] or null
  int64_t* chunkSq;           // split path: [n_sites][nChunks][2] the chunk's sum of w^2, low 30 bits and the rest
};
// given weights: 0, or kSiteInvalid for u0 outside [0, 1), a beta not finite or <= 0, an ess_min that is NaN (a +inf
// log-weight shows only in the site's maximum)
__device__ __forceinline__ long long givenKind(const SitesArgs& a, int s) {
  const double u0 = a.u0[s];
  if (!(u0 >= 0.0) || !(u0 < 1.0)) return kSiteInvalid;
  if (a.beta && (!(a.beta[s] > 0.0) || !(a.beta[s] < INFINITY))) return kSiteInvalid;
  if (a.essMin && a.essMin[s] != a.essMin[s]) return kSiteInvalid;
  return 0;
}
template <bool Given>
__device__ __forceinline__ long long siteKindOf(const SitesArgs& a, int s) {
  if (Given) return givenKind(a, s);
  return siteKind(a.obs[s], a.sigma[s], a.u0[s]);
}
// the tempered log-weight of column c (NaN and -inf weigh nothing: pfFixedWeight)
__device__ __forceinline__ double givenLogw(const SitesArgs& a, int s, int64_t c) {
  const double lw = a.logw[c];
  return a.beta ? a.beta[s] * lw : lw;
}
// w^2 <= 2^60 in two totals that cannot overflow over 2^22 slots: the sum is exact, so it does not depend on the path
__device__ __forceinline__ void addSquare(long long w, long long* lo, long long* hi) {
  const long long q = w * w;
  *lo += q & ((1ll << 30) - 1);
  *hi += q >> 30;
}
// S^2 / sum w^2 of the integer weights (S > 0): every operand exact in a double, three roundings
__device__ __forceinline__ double essOf(long long S, long long sqLo, long long sqHi) {
  const double Sd = (double)S;
  return (Sd * Sd) / ((double)sqHi * 1073741824.0 + (double)sqLo);
}
// p(j) of ancestorKernel, for a site of M particles and total weight S
__device__ __forceinline__ double sitePoint(int64_t j, double u0, double S, double M) {
  return fmin((((double)j + u0) * S) / M, S - 1.0);
}
__device__ __forceinline__ void siteIdentity(const SitesArgs& a, int s, int64_t base, long long kind) {
  for (int64_t i = threadIdx.x; i < a.M; i += 256) a.anc[base + i] = (int32_t)(base + i);
  if (threadIdx.x == 0) {
    a.total[s] = kind;
    if (a.totalOut) a.totalOut[s] = kind;
  }
}
// a site that is not analysed (kind < 0): log-weights and weights 0, the particles stay
__device__ __forceinline__ void siteSkip(const SitesArgs& a, int64_t base) {
  for (int64_t i = threadIdx.x; i < a.M; i += 256) {
    a.logw[base + i] = 0.0;
    if (a.w) a.w[base + i] = 0;
  }
}
// One workgroup = one site (blockIdx.x), M <= kSitesLds: log-weights (lanes on neighbouring columns) and their maximum | the
// fixed-point weights of CONSECUTIVE slots per thread, one block scan | every particle's slot: bisection over the 256 inclusive
// sums, then a walk of that thread's weights.  The weights stay in LDS from phase 1 (as log-weights) to phase 3.
template <typename T, bool Given = false>
__global__ __launch_bounds__(256) void pfSitesKernel(SitesArgs a) {
  __shared__ double smD[256];
  __shared__ long long smWave[4];
  __shared__ long long incl[256];
  __shared__ union { double lw[kSitesLds]; long long w[kSitesLds]; } site;
  const int tid = (int)threadIdx.x, s = (int)blockIdx.x;
  const int64_t M = a.M, base = (int64_t)s * M;
  const double obs = Given ? 0.0 : a.obs[s], sigma = Given ? 1.0 : a.sigma[s], u0 = a.u0[s];
  const long long kind = siteKindOf<Given>(a, s);
  if (kind < 0) {
    if (!Given) siteSkip(a, base);   // (given weights: nothing of the site is written but its identity and its total)
    siteIdentity(a, s, base, kind);
    return;
  }
  const double invSigma = 1.0 / sigma;
  double mine = -INFINITY;
  for (int i = tid; i < M; i += 256) {
    const double lw = Given ? givenLogw(a, s, base + i)
                            : logWeightOf((const T*)a.plane, a.nSteps, a.ld, base + i, a.status, obs, invSigma, a.logw);
    site.lw[i] = lw;
    mine = fmax(mine, lw);
  }
  const double m = blockMax256(mine, smD);   // (its __syncthreads: every log-weight is in LDS)
  if (Given && m == INFINITY) {   // (the same m in every thread)
    siteIdentity(a, s, base, kSiteInvalid);
    return;
  }
  const int per = (int)((M + 255) >> 8);
  const int t0 = tid * per < M ? tid * per : (int)M, t1 = t0 + per < M ? t0 + per : (int)M;
  long long mySum = 0, sqLo = 0, sqHi = 0;
  for (int i = t0; i < t1; i++) {   // (this thread's slots only: the log-weight becomes the weight in place)
    const long long w = pfFixedWeight(site.lw[i], m);
    site.w[i] = w;
    mySum += w;
    if (Given) addSquare(w, &sqLo, &sqHi);
  }
  long long Sll;
  incl[tid] = blockScan256(mySum, smWave, &Sll);   // (its __syncthreads: every weight is in LDS)
  __syncthreads();
  if (a.w)
    for (int i = tid; i < M; i += 256) a.w[base + i] = site.w[i];
  if (Given && (a.ess || a.essMin)) {
    long long allLo, allHi;
    (void)blockScan256(sqLo, smWave, &allLo);
    (void)blockScan256(sqHi, smWave, &allHi);
    const double ess = Sll > 0 ? essOf(Sll, allLo, allHi) : 0.0;
    if (a.ess && tid == 0) a.ess[s] = ess;
    if (Sll > 0 && a.essMin && ess >= a.essMin[s]) {   // enough of the site still weighs something: it keeps its particles
      siteIdentity(a, s, base, kSiteKept);
      return;
    }
  }
  if (Sll == 0) {   // nobody of this site ran: it keeps its particles (the other sites go on)
    siteIdentity(a, s, base, 0);
    return;
  }
  const double S = (double)Sll, Md = (double)M;
  for (int j = tid; j < M; j += 256) {
    const double p = sitePoint(j, u0, S, Md);
    int tl = 0, th = 255;   // first thread with (double)incl > p (incl[255] = S > p: exists)
    while (tl < th) {
      const int mid = (tl + th) >> 1;
      if ((double)incl[mid] > p) th = mid; else tl = mid + 1;
    }
    long long run = tl > 0 ? incl[tl - 1] : 0;
    const int i0 = tl * per, iEnd = i0 + per < M ? i0 + per : (int)M;
    int found = iEnd - 1;
    for (int i = i0; i < iEnd; i++) {
      run += site.w[i];
      if ((double)run > p) { found = i; break; }
    }
    a.anc[base + j] = (int32_t)(base + found);
  }
  if (Given && a.essMin)   // resampled: the particles weigh the same again (the site's log-weights were all read in phase 1)
    for (int i = tid; i < M; i += 256) a.logw[base + i] = 0.0;
  if (tid == 0) {
    a.total[s] = Sll;
    if (a.totalOut) a.totalOut[s] = Sll;
  }
}
// split path, launch 1: chunk blockIdx.y of site blockIdx.x (x: up to 2^22 sites; y: at most 1024 chunks) -- log-weights and
// their maximum
template <typename T, bool Given = false>
__global__ __launch_bounds__(256) void sitesChunkKernel(SitesArgs a) {
  __shared__ double smD[256];
  const int s = (int)blockIdx.x, k = (int)blockIdx.y;
  const int64_t base = (int64_t)s * a.M, lo = (int64_t)k * a.chunk, hi = lo + a.chunk < a.M ? lo + a.chunk : a.M;
  const double obs = Given ? 0.0 : a.obs[s], sigma = Given ? 1.0 : a.sigma[s];
  if (siteKindOf<Given>(a, s) < 0) {   // (launch 2 writes the zeros)
    if (threadIdx.x == 0) a.chunkMax[(int64_t)s * a.nChunks + k] = -INFINITY;
    return;
  }
  const double invSigma = 1.0 / sigma;
  double mine = -INFINITY;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256)
    mine = fmax(mine, Given ? givenLogw(a, s, base + i)
                            : logWeightOf((const T*)a.plane, a.nSteps, a.ld, base + i, a.status, obs, invSigma, a.logw));
  mine = blockMax256(mine, smD);
  if (threadIdx.x == 0) a.chunkMax[(int64_t)s * a.nChunks + k] = mine;
}
// launch 2: the site's maximum, the chunk's fixed-point weights (chunk / 256 consecutive slots per thread), one block scan
// (given weights: a site that is invalid, by its arguments or by a +inf maximum, writes nothing here)
template <bool Given = false>
__global__ __launch_bounds__(256) void sitesWeightKernel(SitesArgs a) {
  __shared__ double smD[256];
  __shared__ long long smWave[4];
  const int tid = (int)threadIdx.x, s = (int)blockIdx.x, k = (int)blockIdx.y;
  const int64_t base = (int64_t)s * a.M, lo = (int64_t)k * a.chunk, hi = lo + a.chunk < a.M ? lo + a.chunk : a.M;
  const int64_t ck = (int64_t)s * a.nChunks + k;
  if (siteKindOf<Given>(a, s) < 0) {
    if (!Given)
      for (int64_t i = lo + tid; i < hi; i += 256) {
        a.logw[base + i] = 0.0;
        a.w[base + i] = 0;
      }
    return;
  }
  double pm = -INFINITY;
  for (int q = tid; q < a.nChunks; q += 256) pm = fmax(pm, a.chunkMax[(int64_t)s * a.nChunks + q]);
  const double m = blockMax256(pm, smD);
  if (Given && m == INFINITY) return;   // (launch 3 finds the same maximum and reports the site)
  const int per = a.chunk >> 8;
  const int64_t t0 = lo + (int64_t)tid * per < hi ? lo + (int64_t)tid * per : hi, t1 = t0 + per < hi ? t0 + per : hi;
  long long mySum = 0, sqLo = 0, sqHi = 0;
  for (int64_t i = t0; i < t1; i++) {
    const long long w = pfFixedWeight(Given ? givenLogw(a, s, base + i) : a.logw[base + i], m);
    a.w[base + i] = w;
    mySum += w;
    if (Given) addSquare(w, &sqLo, &sqHi);
  }
  long long chunkTotal;
  a.threadIncl[ck * 256 + tid] = blockScan256(mySum, smWave, &chunkTotal);
  if (tid == 0) a.chunkSum[ck] = chunkTotal;
  if (Given) {
    long long allLo, allHi;
    (void)blockScan256(sqLo, smWave, &allLo);
    (void)blockScan256(sqHi, smWave, &allHi);
    if (tid == 0) {
      a.chunkSq[2 * ck] = allLo;
      a.chunkSq[2 * ck + 1] = allHi;
    }
  }
}
// launch 3: particles [256 blockIdx.y, 256 blockIdx.y + 256) of site blockIdx.x -- the chunks' offsets, then each particle's
// chunk (bisection of the offsets in LDS), thread (bisection of that chunk's 256 inclusive sums) and slot (a walk of that thread's chunk / 256 <= 16 weights)
template <bool Given = false>
__global__ __launch_bounds__(256) void sitesAncestorKernel(SitesArgs a) {
  __shared__ long long smWave[4];
  __shared__ long long prefix[kSitesMaxChunks + 1];
  __shared__ double smD[Given ? 256 : 1];
  const int tid = (int)threadIdx.x, s = (int)blockIdx.x, nCh = a.nChunks;
  const int64_t base = (int64_t)s * a.M, jLo = (int64_t)blockIdx.y * 256;
  const double u0 = a.u0[s];
  long long kind = siteKindOf<Given>(a, s);
  if (Given && kind == 0) {   // a +inf log-weight: launch 2 wrote nothing of this site
    double pm = -INFINITY;
    for (int q = tid; q < nCh; q += 256) pm = fmax(pm, a.chunkMax[(int64_t)s * nCh + q]);
    if (blockMax256(pm, smD) == INFINITY) kind = kSiteInvalid;
  }
  auto identity = [&](long long tot) {
    const int64_t j = jLo + tid;
    if (j < a.M) a.anc[base + j] = (int32_t)(base + j);
    if (blockIdx.y == 0 && tid == 0) {
      a.total[s] = tot;
      if (a.totalOut) a.totalOut[s] = tot;
    }
  };
  if (kind < 0) { identity(kind); return; }
  {   // four consecutive chunk sums per thread (nCh <= 1024), one block scan
    constexpr int kPer = (kSitesMaxChunks + 255) / 256;
    long long v[kPer], sum = 0;
#pragma unroll
    for (int q = 0; q < kPer; q++) {
      const int c = tid * kPer + q;
      v[q] = c < nCh ? a.chunkSum[(int64_t)s * nCh + c] : 0;
      sum += v[q];
    }
    long long all;
    long long run = blockScan256(sum, smWave, &all) - sum;
    if (Given && (a.ess || a.essMin)) {   // the chunks' exact sums of squares; every workgroup of the site decides alike
      long long lo = 0, hi = 0, allLo, allHi;
      for (int c = tid; c < nCh; c += 256) {
        lo += a.chunkSq[2 * ((int64_t)s * nCh + c)];
        hi += a.chunkSq[2 * ((int64_t)s * nCh + c) + 1];
      }
      (void)blockScan256(lo, smWave, &allLo);
      (void)blockScan256(hi, smWave, &allHi);
      const double ess = all > 0 ? essOf(all, allLo, allHi) : 0.0;
      if (a.ess && blockIdx.y == 0 && tid == 0) a.ess[s] = ess;
      if (all > 0 && a.essMin && ess >= a.essMin[s]) { identity(kSiteKept); return; }
    }
    if (tid == 0) prefix[0] = 0;
#pragma unroll
    for (int q = 0; q < kPer; q++) {
      const int c = tid * kPer + q;
      run += v[q];
      if (c < nCh) prefix[c + 1] = run;
    }
    __syncthreads();
  }
  const long long Sll = prefix[nCh];
  if (Sll == 0) { identity(0); return; }
  const int64_t j = jLo + tid;
  if (j < a.M) {
    const double S = (double)Sll, p = sitePoint(j, u0, S, (double)a.M);
    int cl = 0, chh = nCh - 1;   // the chunk: first c with (double)prefix[c + 1] > p
    while (cl < chh) {
      const int mid = (cl + chh) >> 1;
      if ((double)prefix[mid + 1] > p) chh = mid; else cl = mid + 1;
    }
    const long long cbase = prefix[cl];
    const int64_t* inc = a.threadIncl + ((int64_t)s * nCh + cl) * 256;
    int tl = 0, th = 255;        // the thread: first t with (double)(cbase + inc[t]) > p
    while (tl < th) {
      const int mid = (tl + th) >> 1;
      if ((double)(cbase + inc[mid]) > p) th = mid; else tl = mid + 1;
    }
    long long run = cbase + (tl > 0 ? inc[tl - 1] : 0);
    const int per = a.chunk >> 8;
    const int64_t i0 = (int64_t)cl * a.chunk + (int64_t)tl * per, iEnd = i0 + per < a.M ? i0 + per : a.M;
    int64_t found = iEnd - 1;
    for (int64_t i = i0; i < iEnd; i++) {
      run += a.w[base + i];
      if ((double)run > p) { found = i; break; }
    }
    a.anc[base + j] = (int32_t)(base + found);
    if (Given && a.essMin) a.logw[base + j] = 0.0;   // resampled: the particles weigh the same again (launches 1, 2 read them)
  }
  if (blockIdx.y == 0 && tid == 0) {
    a.total[s] = Sll;
    if (a.totalOut) a.totalOut[s] = Sll;
  }
}
