// pf_temper.inc -- the tempering exponent of every site, chosen on the device (sipnet_batch_pf_temper_sites): the largest step
// d in (0, delta_max] that keeps the effective sample size of the tempered weights at a target, found by a fixed search of
// SIPNET_TEMPER_ROUNDS rounds of SIPNET_TEMPER_SECTIONS - 1 candidates each.  The weights are pf_sites.inc's: pfFixedWeight of
// the tempered log-weight v_c(d) under the site's maximum, the sum of squares exact in its two words (addSquare), essOf.  So
// the step this returns gives, as beta of sipnet_batch_pf_resample_sites, exactly the effective sample size it was chosen for.
//
// Two paths, the same bits.  One workgroup per site (temperGroupKernel, M <= kSitesLds, without carried log-weights): loglik
// staged once in LDS, every round one sweep of the thread's slots over all candidates and one block reduction; the whole
// search is one launch.  Per-chunk launches (temperChunkMaxKernel | temperChunkKernel per stage | temperTailKernel): a stage's launch
// leaves every chunk's exact partial triples in scratch, the next launch's workgroups each sum the site's partials and derive
// the new bracket -- every workgroup of a site decides alike, as in sitesAncestorKernel.  No atomic, no grid barrier, no spin.
// All sums are integers, so no reduction order shows; the only floating-point values a path could disturb are the candidates
// (temperCandidate) and the tempered log-weights (temperV), which are written with explicit operations.  The wave sums are
// site_device.h's (waveSum, blockSum); the host side, with the note on why d_base takes the launches, is pf_moves.inc.
constexpr int kTemperCand = SIPNET_TEMPER_SECTIONS - 1;   // candidates of a round
constexpr int kTemperWords = 3 * kTemperCand;             // a round's sums: S | squares, low word | squares, the rest
constexpr int32_t kTemperSearching = 3;                   // a site's state between the stages (never reported)

// a site between two stages of the search (the per-chunk path keeps one per stage in scratch)
struct TemperState {
  double lo, hi, essLo;     // the bracket, ESS(lo)
  int32_t code, finite;     // the code so far; the members whose value at d = 0 is finite
};
struct TemperArgs {
  const double* loglik;     // [ncol]
  const double* base;       // [ncol] or null
  const double* deltaMax;   // [n_sites] or null (1)
  const double* essTarget;  // [n_sites]
  double* delta;            // [n_sites]
  double* deltaHi;          // [n_sites] or null
  double* ess;              // [n_sites] or null
  double* logwOut;          // [ncol] or null (may be base)
  int32_t* info;            // [n_sites][2] or null
  int64_t M;
  int32_t nChunks, chunk;   // the per-chunk path: sitesGeometry's
  TemperState* state;       // [SIPNET_TEMPER_ROUNDS + 1][n_sites]
  double* chunkMax;         // [n_sites][nChunks][2] the chunks' maxima of loglik and of base
  int32_t* chunkCnt;        // [n_sites][nChunks] the chunks' members whose value at d = 0 is finite
  long long* partial;       // [2][n_sites][nChunks][kTemperWords] a stage's sums, stages alternating
  double* candMax;          // [n_sites][nChunks][kTemperCand] with base: the chunks' maxima of a stage's candidates
  int64_t nSites;
};

// THE tempered log-weight of a column at step d: the one rounded product d * loglik (what givenLogw forms from beta = d), or,
// over carried log-weights, the one fused multiply-add
template <bool Base>
__device__ __forceinline__ double temperV(double d, double ll, double base) {
#pragma clang fp contract(off)
  return Base ? __builtin_fma(d, ll, base) : __dmul_rn(d, ll);
}
// candidate i of the bracket [lo, hi]: lo + (hi - lo) * (i / 16), every operation rounded on its own
__device__ __forceinline__ double temperCandidate(double lo, double hi, int i) {
#pragma clang fp contract(off)
  const double step = __dmul_rn(__dsub_rn(hi, lo), (double)i * (1.0 / SIPNET_TEMPER_SECTIONS));
  return __dadd_rn(lo, step);
}
__device__ __forceinline__ double temperEss(long long S, long long sqLo, long long sqHi) {
  return S > 0 ? essOf(S, sqLo, sqHi) : 0.0;
}
// a site's scalars: false where they are bad input
__device__ __forceinline__ bool temperScalars(const TemperArgs& a, int s, double* dmax, double* target) {
  *dmax = a.deltaMax ? a.deltaMax[s] : 1.0;
  *target = a.essTarget[s];
  return *dmax > 0.0 && *dmax < INFINITY && *target > 0.0;
}
// the state before the first stage: bad input (the scalars, a +inf among loglik or base) or the bracket [0, delta_max]
__device__ __forceinline__ TemperState temperBegin(bool scalarsOk, double dmax, double maxLl, double maxBase, int finite) {
  TemperState st;
  const bool ok = scalarsOk && maxLl != INFINITY && maxBase != INFINITY;
  st.lo = 0.0;
  st.hi = ok ? dmax : 0.0;
  st.essLo = 0.0;
  st.code = ok ? kTemperSearching : -2;
  st.finite = ok ? finite : 0;
  return st;
}
// after the first stage (candidates 0 and delta_max; t: their sums): the codes 0, -1 and 2, or the search goes on
__device__ __forceinline__ void temperStart(TemperState& st, const long long (&t)[kTemperWords], double target) {
  const double ess0 = temperEss(t[0], t[kTemperCand], t[2 * kTemperCand]);
  const double essMax = temperEss(t[1], t[kTemperCand + 1], t[2 * kTemperCand + 1]);
  if (t[0] == 0) {
    st.hi = 0.0;
    st.code = 0;
  } else if (ess0 < target) {
    st.hi = 0.0;
    st.essLo = ess0;
    st.code = -1;
  } else if (essMax >= target) {
    st.lo = st.hi;
    st.essLo = essMax;
    st.code = 2;
  } else {
    st.essLo = ess0;
  }
}
// after a round (t: the sums of its candidates): k leading candidates keep the target; the bracket becomes [b_k, b_k+1]
__device__ __forceinline__ void temperAdvance(TemperState& st, const long long (&t)[kTemperWords], double target) {
  const double lo = st.lo, hi = st.hi;
  int k = 0;
  bool go = true;
#pragma unroll
  for (int j = 0; j < kTemperCand; j++) {
    const double e = temperEss(t[j], t[kTemperCand + j], t[2 * kTemperCand + j]);
    go = go && e >= target;
    if (go) {
      k = j + 1;
      st.essLo = e;
    }
  }
  if (k > 0) st.lo = temperCandidate(lo, hi, k);
  if (k < kTemperCand) st.hi = temperCandidate(lo, hi, k + 1);
}
// the state after stage `stage` (0: the first; 1 ..: the rounds) from the state before it and that stage's sums
__device__ __forceinline__ void temperDerive(TemperState& st, int stage, const long long (&t)[kTemperWords], double target) {
  if (st.code != kTemperSearching) return;
  if (stage == 0) temperStart(st, t, target);
  else temperAdvance(st, t, target);
  if (stage == SIPNET_TEMPER_ROUNDS && st.code == kTemperSearching) st.code = 1;
}
// the candidates of a round from the bracket of state st
__device__ __forceinline__ void temperCandidates(const TemperState& st, double (&d)[kTemperCand]) {
#pragma unroll
  for (int j = 0; j < kTemperCand; j++) d[j] = temperCandidate(st.lo, st.hi, j + 1);
}

// the sums of kTemperWords integers over the workgroup, to every thread (smSum [4][kTemperWords]; free again on return)
__device__ __forceinline__ void temperBlockSum(long long (&v)[kTemperWords], long long* smSum) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kTemperWords; q++) {
    const long long x = waveSum(v[q]);
    if (lane == 0) smSum[wave * kTemperWords + q] = x;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kTemperWords; q++)
    v[q] = smSum[q] + smSum[kTemperWords + q] + smSum[2 * kTemperWords + q] + smSum[3 * kTemperWords + q];
  __syncthreads();
}
// the maxima of kTemperCand doubles over the workgroup, to every thread (smMax [4][kTemperCand]; free again on return)
__device__ __forceinline__ void temperBlockMax(double (&v)[kTemperCand], double* smMax) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kTemperCand; q++) {
    double x = v[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off, 64));
    if (lane == 0) smMax[wave * kTemperCand + q] = x;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kTemperCand; q++)
    v[q] = fmax(fmax(smMax[q], smMax[kTemperCand + q]), fmax(smMax[2 * kTemperCand + q], smMax[3 * kTemperCand + q]));
  __syncthreads();
}
// one column's weight at step d under the maximum m into the sums of candidate j
template <bool Base>
__device__ __forceinline__ void temperAddOne(long long (&acc)[kTemperWords], int j, double d, double m, double ll, double base) {
  const long long w = pfFixedWeight(temperV<Base>(d, ll, base), m);
  acc[j] += w;
  addSquare(w, &acc[kTemperCand + j], &acc[2 * kTemperCand + j]);
}
// one column's weights at a round's candidates into the thread's sums
template <bool Base>
__device__ __forceinline__ void temperAdd(long long (&acc)[kTemperWords], const double (&d)[kTemperCand],
                                          const double (&m)[kTemperCand], double ll, double base) {
#pragma unroll
  for (int j = 0; j < kTemperCand; j++) temperAddOne<Base>(acc, j, d[j], m[j], ll, base);
}
// the first stage's two candidates, 0 and delta_max, as candidates 0 and 1
template <bool Base>
__device__ __forceinline__ void temperAddPair(long long (&acc)[kTemperWords], double dmax, double m0, double m1, double ll, double base) {
  temperAddOne<Base>(acc, 0, 0.0, m0, ll, base);
  temperAddOne<Base>(acc, 1, dmax, m1, ll, base);
}
// one column's tempered log-weights at a round's candidates into the thread's maxima (with base: every candidate has its own)
__device__ __forceinline__ void temperMaxAdd(double (&mx)[kTemperCand], const double (&d)[kTemperCand], double ll, double base) {
#pragma unroll
  for (int j = 0; j < kTemperCand; j++) mx[j] = fmax(mx[j], temperV<true>(d[j], ll, base));
}
// does column (ll, base) have a finite value at d = 0?
template <bool Base>
__device__ __forceinline__ int temperFinite(double ll, double base) {
  return fabs(temperV<Base>(0.0, ll, base)) < INFINITY ? 1 : 0;
}
// a site's results (one thread): its step, the bracket's end, ESS(step) and the info
__device__ __forceinline__ void temperWrite(const TemperArgs& a, int s, const TemperState& st) {
  a.delta[s] = st.lo;
  if (a.deltaHi) a.deltaHi[s] = st.hi;
  if (a.ess) a.ess[s] = st.essLo;
  if (a.info) {
    a.info[2 * s] = st.code;
    a.info[2 * s + 1] = st.finite;
  }
}

// One workgroup = one site (blockIdx.x), M <= kSitesLds, no carried log-weights (with them the call takes the per-chunk
// launches: pf_moves.inc says why).  Dynamic LDS: loglik [M].
__global__ __launch_bounds__(256) void temperGroupKernel(TemperArgs a) {
  extern __shared__ double temperLds[];
  __shared__ long long smSum[4 * kTemperWords];
  __shared__ double smD[256];
  __shared__ int smI[4];
  const int tid = (int)threadIdx.x, s = (int)blockIdx.x, M = (int)a.M;
  const int64_t col0 = (int64_t)s * a.M;
  double* ll = temperLds;
  double dmax, target;
  const bool scalarsOk = temperScalars(a, s, &dmax, &target);
  double mine = -INFINITY;
  int finite = 0;
  for (int i = tid; i < M; i += 256) {
    const double x = a.loglik[col0 + i];
    ll[i] = x;
    mine = fmax(mine, x);
    finite += temperFinite<false>(x, 0.0);
  }
  const double maxLl = blockMax256(mine, smD);   // (its __syncthreads: the site is in LDS)
  finite = blockSum(smI, finite);
  TemperState st = temperBegin(scalarsOk, dmax, maxLl, -INFINITY, finite);
  long long acc[kTemperWords];
  if (st.code == kTemperSearching) {   // the first stage: ESS(0) and ESS(delta_max)
    const double m0 = temperV<false>(0.0, maxLl, 0.0), m1 = temperV<false>(dmax, maxLl, 0.0);
#pragma unroll
    for (int q = 0; q < kTemperWords; q++) acc[q] = 0;
    for (int i = tid; i < M; i += 256) temperAddPair<false>(acc, dmax, m0, m1, ll[i], 0.0);
    temperBlockSum(acc, smSum);
    temperDerive(st, 0, acc, target);
  }
  for (int stage = 1; stage <= SIPNET_TEMPER_ROUNDS && st.code == kTemperSearching; stage++) {
    double d[kTemperCand], m[kTemperCand];
    temperCandidates(st, d);
#pragma unroll
    for (int j = 0; j < kTemperCand; j++) m[j] = temperV<false>(d[j], maxLl, 0.0);
#pragma unroll
    for (int q = 0; q < kTemperWords; q++) acc[q] = 0;
    for (int i = tid; i < M; i += 256) temperAdd<false>(acc, d, m, ll[i], 0.0);
    temperBlockSum(acc, smSum);
    temperDerive(st, stage, acc, target);
  }
  if (tid == 0) temperWrite(a, s, st);
  if (a.logwOut && st.code > 0)
    for (int i = tid; i < M; i += 256) a.logwOut[col0 + i] = temperV<false>(st.lo, ll[i], 0.0);
}

// ---- the per-chunk path: chunk blockIdx.y of site blockIdx.x ------------------------------------------------------------------
// launch 1: the chunk's maxima of loglik and of base, and its members whose value at d = 0 is finite
template <bool Base>
__global__ __launch_bounds__(256) void temperChunkMaxKernel(TemperArgs a) {
  __shared__ double smMax[4 * kTemperCand];
  __shared__ int smI[4];
  const int tid = (int)threadIdx.x, s = (int)blockIdx.x, k = (int)blockIdx.y;
  const int64_t col0 = (int64_t)s * a.M, lo = (int64_t)k * a.chunk, hi = lo + a.chunk < a.M ? lo + a.chunk : a.M;
  const int64_t ck = (int64_t)s * a.nChunks + k;
  double d[kTemperCand];
  int finite = 0;
#pragma unroll
  for (int j = 0; j < kTemperCand; j++) d[j] = -INFINITY;
  for (int64_t i = lo + tid; i < hi; i += 256) {
    const double x = a.loglik[col0 + i], y = Base ? a.base[col0 + i] : 0.0;
    d[0] = fmax(d[0], x);
    if (Base) d[1] = fmax(d[1], y);
    finite += temperFinite<Base>(x, y);
  }
  temperBlockMax(d, smMax);
  finite = blockSum(smI, finite);
  if (tid == 0) {
    a.chunkMax[2 * ck] = d[0];
    a.chunkMax[2 * ck + 1] = d[1];
    a.chunkCnt[ck] = finite;
  }
}
// what every workgroup of a site does first in the launches of stage `stage` (ROUNDS + 1: the tail): the site's state before
// that stage -- the first from the scalars and the chunks' maxima and counts, a later one from the state a stage earlier and
// that stage's partial sums.  *maxLl: the site's maximum of loglik.  smD [256], the others as temperBlockSum's.
__device__ __forceinline__ TemperState temperStateBefore(const TemperArgs& a, int s, int stage, double target, bool scalarsOk,
                                                         double dmax, double* maxLl, long long* smSum, double* smD, int* smI) {
  const int tid = (int)threadIdx.x, nCh = a.nChunks;
  double pl = -INFINITY, pb = -INFINITY;
  for (int q = tid; q < nCh; q += 256) {
    pl = fmax(pl, a.chunkMax[2 * ((int64_t)s * nCh + q)]);
    pb = fmax(pb, a.chunkMax[2 * ((int64_t)s * nCh + q) + 1]);
  }
  *maxLl = blockMax256(pl, smD);
  if (stage == 0) {
    const double maxBase = blockMax256(pb, smD);
    return temperBegin(scalarsOk, dmax, *maxLl, maxBase, chunkCounts(smI, a.chunkCnt, s, nCh));
  }
  TemperState st = a.state[(int64_t)(stage - 1) * a.nSites + s];
  if (st.code != kTemperSearching) return st;   // (the same in every thread)
  // lane q < kTemperWords of wave g sums word q of the chunks g, g + 4, ..: a chunk's words are one coalesced read
  const long long* part = a.partial + ((int64_t)((stage - 1) & 1) * a.nSites + s) * nCh * kTemperWords;
  const int q = tid & 63, g = tid >> 6;
  if (q < kTemperWords) {
    long long x = 0;
    for (int c = g; c < nCh; c += 4) x += part[(int64_t)c * kTemperWords + q];
    smSum[g * kTemperWords + q] = x;
  }
  __syncthreads();
  long long acc[kTemperWords];
#pragma unroll
  for (int w = 0; w < kTemperWords; w++)
    acc[w] = smSum[w] + smSum[kTemperWords + w] + smSum[2 * kTemperWords + w] + smSum[3 * kTemperWords + w];
  __syncthreads();
  temperDerive(st, stage - 1, acc, target);
  return st;
}
// a stage's launch (stage 0: the candidates 0 and delta_max; 1 .. ROUNDS: the rounds).  phase 1: the chunk's sums at the stage's
// candidates -> partial.  With base every candidate needs the site's own maximum, so a launch before it (phase 0) leaves the
// chunk's maxima at the candidates, and the site's state, which phase 1 then reads.
template <bool Base>
__global__ __launch_bounds__(256) void temperChunkKernel(TemperArgs a, int stage, int phase) {
  __shared__ long long smSum[4 * kTemperWords];
  __shared__ double smMax[4 * kTemperCand];
  __shared__ double smD[256];
  __shared__ int smI[4];
  const int tid = (int)threadIdx.x, s = (int)blockIdx.x, k = (int)blockIdx.y, nCh = a.nChunks;
  const int64_t col0 = (int64_t)s * a.M, lo = (int64_t)k * a.chunk, hi = lo + a.chunk < a.M ? lo + a.chunk : a.M;
  const int64_t ck = (int64_t)s * nCh + k;
  double dmax, target, maxLl = -INFINITY;
  const bool scalarsOk = temperScalars(a, s, &dmax, &target);
  TemperState st;
  if (Base && phase == 1) {
    st = a.state[(int64_t)stage * a.nSites + s];
  } else {
    st = temperStateBefore(a, s, stage, target, scalarsOk, dmax, &maxLl, smSum, smD, smI);
    if (k == 0 && tid == 0) a.state[(int64_t)stage * a.nSites + s] = st;
  }
  if (st.code != kTemperSearching) return;
  double d[kTemperCand], m[kTemperCand];
  if (stage == 0) {   // 0 and delta_max as candidates 0 and 1, the others at delta_max too (their sums are not read)
#pragma unroll
    for (int j = 0; j < kTemperCand; j++) d[j] = j == 0 ? 0.0 : dmax;
  } else {
    temperCandidates(st, d);
  }
  if (Base && phase == 0) {
#pragma unroll
    for (int j = 0; j < kTemperCand; j++) m[j] = -INFINITY;
    if (stage == 0) {
      for (int64_t i = lo + tid; i < hi; i += 256) {
        m[0] = fmax(m[0], temperV<true>(0.0, a.loglik[col0 + i], a.base[col0 + i]));
        m[1] = fmax(m[1], temperV<true>(dmax, a.loglik[col0 + i], a.base[col0 + i]));
      }
    } else {
      for (int64_t i = lo + tid; i < hi; i += 256) temperMaxAdd(m, d, a.loglik[col0 + i], a.base[col0 + i]);
    }
    temperBlockMax(m, smMax);
#pragma unroll
    for (int j = 0; j < kTemperCand; j++)
      if (tid == j) a.candMax[ck * kTemperCand + j] = m[j];
    return;
  }
  if (Base) {
#pragma unroll
    for (int j = 0; j < kTemperCand; j++) {
      double pm = -INFINITY;
      for (int q = tid; q < nCh; q += 256) pm = fmax(pm, a.candMax[((int64_t)s * nCh + q) * kTemperCand + j]);
      m[j] = pm;
    }
    temperBlockMax(m, smMax);
  } else {
#pragma unroll
    for (int j = 0; j < kTemperCand; j++) m[j] = temperV<false>(d[j], maxLl, 0.0);
  }
  long long acc[kTemperWords];
#pragma unroll
  for (int q = 0; q < kTemperWords; q++) acc[q] = 0;
  if (stage == 0) {
    for (int64_t i = lo + tid; i < hi; i += 256)
      temperAddPair<Base>(acc, dmax, m[0], m[1], a.loglik[col0 + i], Base ? a.base[col0 + i] : 0.0);
  } else {
    for (int64_t i = lo + tid; i < hi; i += 256) temperAdd<Base>(acc, d, m, a.loglik[col0 + i], Base ? a.base[col0 + i] : 0.0);
  }
  temperBlockSum(acc, smSum);
  long long* part = a.partial + ((int64_t)(stage & 1) * a.nSites * nCh + ck) * kTemperWords;
#pragma unroll
  for (int q = 0; q < kTemperWords; q++)
    if (tid == q) part[q] = acc[q];
}
// the last launch: the state after the last round; the site's results (chunk 0) and the chunk's tempered log-weights
template <bool Base>
__global__ __launch_bounds__(256) void temperTailKernel(TemperArgs a) {
  __shared__ long long smSum[4 * kTemperWords];
  __shared__ double smD[256];
  __shared__ int smI[4];
  const int tid = (int)threadIdx.x, s = (int)blockIdx.x, k = (int)blockIdx.y;
  const int64_t col0 = (int64_t)s * a.M, lo = (int64_t)k * a.chunk, hi = lo + a.chunk < a.M ? lo + a.chunk : a.M;
  double dmax, target, maxLl;
  const bool scalarsOk = temperScalars(a, s, &dmax, &target);
  const TemperState st = temperStateBefore(a, s, SIPNET_TEMPER_ROUNDS + 1, target, scalarsOk, dmax, &maxLl, smSum, smD, smI);
  if (k == 0 && tid == 0) temperWrite(a, s, st);
  if (a.logwOut && st.code > 0)
    for (int64_t i = lo + tid; i < hi; i += 256)
      a.logwOut[col0 + i] = temperV<Base>(st.lo, a.loglik[col0 + i], Base ? a.base[col0 + i] : 0.0);
}
