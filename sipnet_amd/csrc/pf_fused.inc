// pf_fused.inc -- the analysis in ONE launch: the SIPNET_PF_* defaults and the PF_STAMP probe, the kernel's arguments
// (FusedArgs), the two-level grid barrier in device memory (gridBarrier) and pfFusedKernel, whose phases are pf_weights.inc's
// launches.

// ---- the analysis in ONE launch (round 5; geometry, barrier and phases reworked in round 6) ------------------------
// Log-weights + maximum | fixed-point weights + prefix sum | ancestors were five launches plus hipCUB's two (and
// its temporaries' fills and copies): 40 us of a 200 us cycle at C5's shape for 15 us of work.  Here they are the
// phases of one kernel whose workgroups are all resident and meet at barriers in device memory.  Workgroup b owns the
// contiguous slots [b * chunk, (b + 1) * chunk) and, inside it, thread t the CONSECUTIVE slots [t * per, (t + 1) * per)
// (per = chunk / 256): a thread sums its own weights serially, ONE block scan per workgroup places the threads' sums
// (round 5 scanned every 256 slots with two __syncthreads: a term that grew with the number of ranks, 8 tiles per
// workgroup at 8 x 131 072 slots), the chunks' totals are summed by every workgroup for itself (<= 512 values), and
// every slot writes the run of particles that take it as their ancestor.  Integer weights: the result does not depend on
// the order of the additions, so the ancestors are those of fixedWeightKernel + DeviceScan + ancestorKernel bit for bit
// (tests/test_gpu_pf.py holds both paths to the same oracle).
// RESIDENCY.  A workgroup that spins at a device-memory barrier holds its CU slot: if not every workgroup of the grid
// is resident the launch never ends.  The grid is therefore sized by the host from what the device can hold
// (hipOccupancyMaxActiveBlocksPerMultiprocessor x the CUs, divided by the number of shards a node has put on the
// device: fusedBudget below) -- at most kFusedBlocks, and the multi-launch path when next to nothing fits -- and the
// barrier's poll has a budget: a workgroup that gives up marks the launch void (kPfVoid in the totals, the stuck word),
// poisons the barrier so that the others leave too, and exits.
#ifndef SIPNET_PF_BLOCKS
#define SIPNET_PF_BLOCKS 512
#endif
#ifndef SIPNET_PF_SLEEP
#define SIPNET_PF_SLEEP 2
#endif
#ifndef SIPNET_PF_SPIN_BUDGET
#define SIPNET_PF_SPIN_BUDGET (1 << 19)   // polls of ~0.5-1 us each: a few tenths of a second
#endif
constexpr int kFusedBlocks = SIPNET_PF_BLOCKS;   // (<= 512: phase 3 scans the chunk totals two per thread)
constexpr int kFusedMinBlocks = 8;               // fewer resident workgroups than this: the multi-launch path
constexpr int kFusedMaxPer = 16;                 // ... or more slots per thread than this (phase 3 adds a thread's weights up again)
constexpr long long kPfVoid = LLONG_MIN;         // "total weight" of a launch whose barrier gave up
#ifdef SIPNET_PF_STAMPS   // (probe, tools/pf_analysis_time.py: where the launch spends its time -- workgroup 0's clock at every phase)
__device__ unsigned long long g_pfStamps[8];
#define PF_STAMP(k)                                                                  \
  if (blockIdx.x == 0 && threadIdx.x == 0) {                                         \
    unsigned long long now_;                                                         \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");  \
    g_pfStamps[k] = now_;                                                            \
  }
#else
#define PF_STAMP(k)
#endif
struct FusedArgs {
  // phase 1 (the one-batch analysis): log-weights from the forecast's plane
  const void* plane;
  int32_t nSteps;
  int64_t ld, ncol;
  const double* status;
  double obs, invSigma;
  double* logw;              // [nSlots] written by phase 1, read by phase 2
  // phase 2 over gathered blocks instead (the filter across ranks): slot i = gathered[(i / nmax) * stride + i % nmax],
  // the blocks' maxima behind each rank's nmax log-weights
  const double* gathered;
  int32_t world, nmax;
  int64_t stride;
  int64_t nSlots, chunk;
  double* blockMax;          // [gridDim.x]
  // phase 1 done already by the forecast's own launch (FastArgs::pfLogw): logw is filled, preMax[nPre] are partial maxima
  const double* preMax;
  int32_t nPre;
  const double* logwIn;      // [nSlots] phase 2's input in the one-batch analysis (= logw)
  int64_t* threadIncl;       // [gridDim.x][256] every thread's inclusive sum of weights inside its chunk
  int64_t* blockSum;         // [gridDim.x]
  unsigned long long* barrier;   // THIS launch's barrier set (kBarSetWords words, all zero when the launch starts)
  unsigned long long* barrierAhead;   // the set of the launch kBarAhead launches from now: zeroed by this one
  unsigned long long* stuck;     // diagnostics: 1 << 63 | barrier number << 32 | workgroup of the first poll that gave up
  int32_t spinBudget;
  int32_t absent;            // test hook (sipnet_debug_pf_barrier): this workgroup leaves at once, without arriving; -1: nobody
  // phase 3
  int64_t j0, nOut, nTotal;
  double u0;
  int32_t* anc;
  int64_t* total;            // may be null
  int64_t* totalScratch;     // always written
};
// What the workgroups exchange (chunk maxima, chunk sums) is written and read with agent-scope relaxed atomics: such
// accesses are coherent across the chip's eight XCDs (each has an L2 of its own) without cache maintenance.  The first
// version used plain accesses and release / acquire fences at the barriers: an agent-scope release is an L2 write-back,
// an acquire an L2 invalidate -- 2 048 waves x 2 barriers of them made the launch 131 us.  Ordering: a workgroup's
// stores have been acknowledged (vmcnt(0)) before it arrives.
__device__ __forceinline__ void stAgent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ldAgent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void stAgent(long long* p, long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ long long ldAgent(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// The barrier itself.  Atomics of one address are served one after the other, ~18 ns each on this chip: 512 workgroups
// arriving at ONE counter made a barrier 9 us (measured with s_memrealtime stamps, profiles/r05_pf_analysis_variants.txt)
// -- more than a launch boundary.  Hence two levels: workgroups arrive at their GROUP's counter (kBarGroup of them per
// address); a group's last arrival goes on to the top counter; the top's last arrival releases every group through the
// group's own flag, which is what the group's workgroups poll (32 pollers per address instead of 512), 64 bytes apart.
// Round 6: every launch has a barrier SET of its own out of a ring of kBarSets (two barriers each, all words zero when
// the launch starts: launch L clears the set of launch L + kBarAhead, which nothing uses in between -- the launches of one
// scratch block are ordered by their stream).  Round 5's counters only ever grew across launches, which made every later
// launch depend on every earlier one having completed its barriers: a launch that failed to start, or a grid that was not
// co-resident, left the host's epoch ahead of the counters and the NEXT analysis spinning for ever.  Now a void launch
// spoils its own set only.
constexpr int kBarGroup = 32;
constexpr int kBarStride = 8;   // unsigned long longs between two counters: a line of their own
constexpr int kBarGroupsMax = (kFusedBlocks + kBarGroup - 1) / kBarGroup;
constexpr int kBarWords = kBarStride * (2 + 2 * kBarGroupsMax);   // one barrier: top counter, poison word, G counters, G flags
constexpr int kBarSetWords = 2 * kBarWords;                       // a launch passes at most two
constexpr int kBarSets = 64, kBarAhead = 32;
// false: the barrier gave up (this workgroup's poll ran out of budget, or another's did and poisoned the barrier) -- the
// launch is void and the caller returns; every thread of the workgroup gets the same answer
__device__ __forceinline__ bool gridBarrier(unsigned long long* bar, int which, const FusedArgs& a, int* smOk) {
  // bar[0]: top counter; bar[kBarStride]: poison; bar[kBarStride * (2 + g)]: group g's counter; bar[kBarStride * (2 + G + g)]: its flag
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's stores have been acknowledged
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nb = (int)gridDim.x, G = (nb + kBarGroup - 1) / kBarGroup, g = (int)blockIdx.x / kBarGroup;
    const int inGroup = (g == G - 1) ? nb - g * kBarGroup : kBarGroup;
    unsigned long long* flag = bar + kBarStride * (2 + G + g);
    unsigned long long* poison = bar + kBarStride;
    const unsigned long long arrived = __hip_atomic_fetch_add(bar + kBarStride * (2 + g), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived + 1 == (unsigned long long)inGroup) {
      const unsigned long long t = __hip_atomic_fetch_add(bar, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t + 1 == (unsigned long long)G)
        for (int k = 0; k < G; k++)
          __hip_atomic_store(bar + kBarStride * (2 + G + k), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    int ok = 1, polls = 0;
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull) {
      __builtin_amdgcn_s_sleep(SIPNET_PF_SLEEP);
      if ((++polls & 63) == 0) {
        if (__hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) { ok = 0; break; }
        if (polls >= a.spinBudget) {
          __hip_atomic_store(poison, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const unsigned long long rep = (1ull << 63) | ((unsigned long long)(unsigned)which << 32) | (unsigned)blockIdx.x;
          atomicCAS(a.stuck, 0ull, rep);
          ok = 0;
          break;
        }
      }
    }
    if (!ok) {   // the launch is void: say so where the host looks for the total weight
      if (a.total) __hip_atomic_store((long long*)a.total, kPfVoid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store((long long*)a.totalScratch, kPfVoid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    *smOk = ok;
  }
  __syncthreads();
  return *smOk != 0;
}
__device__ __forceinline__ double blockMax256(double v, double* sm) {
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + s]);
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();
  return r;
}
// inclusive sum over the 256 threads of a workgroup; *totalOut = the sum of all
__device__ __forceinline__ long long blockScan256(long long v, long long* smWave, long long* totalOut) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const long long o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  if (lane == 63) smWave[wave] = v;
  __syncthreads();
  long long before = 0;
  for (int k = 0; k < wave; k++) before += smWave[k];
  *totalOut = smWave[0] + smWave[1] + smWave[2] + smWave[3];
  __syncthreads();
  return v + before;
}
template <typename T, bool Gathered>
__global__ __launch_bounds__(256) void pfFusedKernel(FusedArgs a) {
  __shared__ double smD[256];
  __shared__ long long smWave[4];
  __shared__ long long prefix[kFusedBlocks + 1];
  __shared__ int smOk;
  const int tid = (int)threadIdx.x, nb = (int)gridDim.x, b = (int)blockIdx.x;
  const int64_t lo = (int64_t)b * a.chunk, hi = lo + a.chunk < a.nSlots ? lo + a.chunk : a.nSlots;
  // this thread's own consecutive slots [t0, t1)
  const int per = (int)(a.chunk >> 8);
  const int64_t t0 = lo + (int64_t)tid * per < hi ? lo + (int64_t)tid * per : hi, t1 = t0 + per < hi ? t0 + per : hi;
  int nBarrier = 0;
  double m = -INFINITY;
  PF_STAMP(0)
  // the barrier set of the launch kBarAhead launches from now (gridBarrier)
  if (b == 0)
    for (int k = tid; k < kBarSetWords; k += 256) a.barrierAhead[k] = 0ull;
  if (b == a.absent) return;
  if (!Gathered && a.preMax) {
    // ---- phase 1 was the forecast kernel's epilogue: only the maximum is left to take ----
    double pm = -INFINITY;
    for (int k = tid; k < a.nPre; k += 256) pm = fmax(pm, a.preMax[k]);
    m = blockMax256(pm, smD);
  } else if (!Gathered) {
    // ---- phase 1: this chunk's log-weights and their maximum (lanes on neighbouring columns of the plane) ----
    double mine = -INFINITY;
    for (int64_t i = lo + tid; i < hi; i += 256)
      mine = fmax(mine, logWeightOf<T, true>((const T*)a.plane, a.nSteps, a.ld, i, a.status, a.obs, a.invSigma, a.logw));
    mine = blockMax256(mine, smD);
    if (tid == 0) stAgent(&a.blockMax[b], mine);
    PF_STAMP(1)
    if (!gridBarrier(a.barrier + kBarWords * nBarrier, nBarrier, a, &smOk)) return;
    nBarrier++;
    PF_STAMP(2)
    double pm = -INFINITY;
    for (int k = tid; k < nb; k += 256) pm = fmax(pm, ldAgent(&a.blockMax[k]));
    m = blockMax256(pm, smD);
  } else {
    // the maximum over every rank's block maxima (512 workgroups read the same world x P doubles at the same time: each starts
    // with another rank's, and no division in the index -- 6.5 us at 8 x 512 maxima before, profiles/r06_pf_analysis_phases.txt)
    const int P = (a.nmax + 255) / 256;
    double pm = -INFINITY;
    for (int q = 0; q < a.world; q += 4) {   // (four ranks' loads in flight: one after the other they were 16 L2 round trips)
      const double* mx[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        int r = (q + u < a.world ? q + u : q) + b % a.world;
        r = r >= a.world ? r - a.world : r;
        mx[u] = a.gathered + (int64_t)r * a.stride + a.nmax;
      }
      for (int k = tid; k < P; k += 256) {
        const double v0 = mx[0][k], v1 = mx[1][k], v2 = mx[2][k], v3 = mx[3][k];
        pm = fmax(fmax(pm, fmax(v0, v1)), fmax(v2, v3));
      }
    }
    m = blockMax256(pm, smD);
    PF_STAMP(2)
  }
  // ---- phase 2: fixed-point weights (pfFixedWeight) of this thread's slots, summed; ONE block scan ----
  // slot i's log-weight, wherever it lies: the one-batch analysis' own vector, or rank (i / nmax)'s gathered block
  auto slotLogw = [&](int64_t i) -> double {
    if (!Gathered) return a.logwIn[i];
    const int64_t r = i / a.nmax;
    return a.gathered[r * a.stride + (i - r * a.nmax)];
  };
  long long mySum = 0;
  {
    int64_t r = 0, c = 0;   // (gathered blocks: slot i sits in rank r's block at column c)
    if (Gathered) { r = t0 / a.nmax; c = t0 - r * a.nmax; }
    for (int64_t i = t0; i < t1; i += 8) {
      double lw[8];
      const int n8 = t1 - i < 8 ? (int)(t1 - i) : 8;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        lw[k] = -INFINITY;
        if (k < n8) {
          if (Gathered) {
            lw[k] = a.gathered[r * a.stride + c];
            if (++c == a.nmax) { c = 0; r++; }
          } else {
            lw[k] = a.logwIn[i + k];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 8; k++) mySum += pfFixedWeight(lw[k], m);
    }
  }
  long long chunkTotal;
  const long long myIncl = blockScan256(mySum, smWave, &chunkTotal);
  // (the threads' inclusive sums inside the chunk: what another workgroup needs to place a particle in this chunk)
  stAgent((long long*)&a.threadIncl[(int64_t)b * 256 + tid], myIncl);
  if (tid == 0) stAgent((long long*)&a.blockSum[b], chunkTotal);
  PF_STAMP(3)
  if (!gridBarrier(a.barrier + kBarWords * nBarrier, nBarrier, a, &smOk)) return;
  nBarrier++;
  PF_STAMP(4)
  // ---- phase 3: the chunks' offsets (every workgroup for itself), then the ancestors of this workgroup's PARTICLES ----
  {
    // two entries per thread (nb <= 512), scanned as pairs
    const int k0 = 2 * tid, k1 = 2 * tid + 1;
    const long long s0 = k0 < nb ? ldAgent((const long long*)&a.blockSum[k0]) : 0, s1 = k1 < nb ? ldAgent((const long long*)&a.blockSum[k1]) : 0;
    long long all;
    const long long inc = blockScan256(s0 + s1, smWave, &all);
    if (tid == 0) prefix[0] = 0;
    if (k0 < nb) prefix[k0 + 1] = inc - s1;
    if (k1 < nb) prefix[k1 + 1] = inc;
    __syncthreads();
  }
  const long long Sll = prefix[nb];
  PF_STAMP(5)
  // ancestorKernel's rule, particle by particle: particle g takes the first slot i with cdf[i] > P(g), P(g) = min(((g + u0) S) /
  // nTotal, S - 1).  The launch's particles [j0, j0 + nOut) are dealt to the workgroups in equal contiguous shares -- round 5 and
  // the first round-6 version went slot by slot, every slot writing the run of particles that take it: across ranks a launch
  // writes only ITS rank's particles, whose slots sit in 1 / world of the chunks, so 64 of 512 workgroups did all the divisions and
  // stores of the phase (8 x 131 072 slots: ~15 us against 2.7 us for one rank's).  A particle finds its slot in three steps that
  // read nothing but sums: its CHUNK by bisection of the chunks' offsets (LDS), the THREAD of phase 2 whose slots hold it by
  // bisection of that chunk's 256 inclusive sums (LDS for the two chunks the workgroup's particles start in, device memory
  // for a particle further on), the SLOT by adding up that thread's <= 16 weights again (pfFixedWeight of log-weights that were
  // there before the launch, or came from phase 1 through agent-scope stores).  cdf is non-decreasing, so "first slot with
  // cdf > p" never lands on a slot that weighs nothing; S = 0 puts every particle on slot 0, as ancestorKernel does.
  const double S = (double)Sll, nTot = (double)a.nTotal;
  __shared__ long long inclA[256], inclB[256];
  __shared__ int chunkA;
  const int64_t share = (a.nOut + nb - 1) / nb;           // particles per workgroup
  const int64_t jLo = (int64_t)b * share, jHi = jLo + share < a.nOut ? jLo + share : a.nOut;
  auto chunkOf = [&](double p) -> int {                   // first c with (double)prefix[c + 1] > p
    int lo2 = 0, hi2 = nb - 1;
    while (lo2 < hi2) {
      const int mid = (lo2 + hi2) >> 1;
      if ((double)prefix[mid + 1] > p) hi2 = mid; else lo2 = mid + 1;
    }
    return lo2;
  };
  auto pOf = [&](int64_t j) -> double { return fmin((((double)(a.j0 + j) + a.u0) * S) / nTot, S - 1.0); };
  if (jLo < jHi) {
    if (tid == 0) chunkA = chunkOf(pOf(jLo));
    __syncthreads();
    const int cA = chunkA, cB = cA + 1 < nb ? cA + 1 : cA;
    inclA[tid] = ldAgent((const long long*)&a.threadIncl[(int64_t)cA * 256 + tid]);
    inclB[tid] = ldAgent((const long long*)&a.threadIncl[(int64_t)cB * 256 + tid]);
    __syncthreads();
    for (int64_t j = jLo + tid; j < jHi; j += 256) {
      const double p = pOf(j);
      const int c = chunkOf(p);
      const long long base = prefix[c];
      // the thread of phase 2: first t with (double)(base + incl[c][t]) > p  (incl[c][255] = the chunk's total: exists)
      int tl = 0, th = 255;
      if (c == cA || c == cB) {
        const long long* incl = c == cA ? inclA : inclB;
        while (tl < th) {
          const int mid = (tl + th) >> 1;
          if ((double)(base + incl[mid]) > p) th = mid; else tl = mid + 1;
        }
      } else {
        while (tl < th) {
          const int mid = (tl + th) >> 1;
          if ((double)(base + ldAgent((const long long*)&a.threadIncl[(int64_t)c * 256 + mid])) > p) th = mid; else tl = mid + 1;
        }
      }
      long long run = base;
      if (tl > 0) run += (c == cA) ? inclA[tl - 1] : (c == cB) ? inclB[tl - 1] : ldAgent((const long long*)&a.threadIncl[(int64_t)c * 256 + tl - 1]);
      // the slot: that thread's weights once more, until the sum passes p (eight log-weights requested at a time: one after
      // the other they were up to `per` L2 round trips per particle)
      const int64_t i0 = (int64_t)c * a.chunk + (int64_t)tl * per;
      const int64_t iEnd = i0 + per < a.nSlots ? i0 + per : a.nSlots;
      int64_t found = -1;
      for (int64_t i = i0; i < iEnd && found < 0; i += 8) {
        double lw[8];
#pragma unroll
        for (int k = 0; k < 8; k++) lw[k] = i + k < iEnd ? slotLogw(i + k) : -INFINITY;
#pragma unroll
        for (int k = 0; k < 8; k++) {
          run += pfFixedWeight(lw[k], m);
          if (found < 0 && (double)run > p) found = i + k;
        }
      }
      a.anc[j] = (int32_t)(found < 0 ? iEnd - 1 : found);
    }
  }
  // the total weight, last: a workgroup that gave up at a barrier has written kPfVoid there, and a launch is void as soon as
  // one did (gridBarrier) -- its poison word says so even if this workgroup was released in the same instant
  if (b == 0 && tid == 0) {
    bool spoilt = false;
    for (int k = 0; k < nBarrier; k++)
      spoilt = spoilt || __hip_atomic_load(a.barrier + kBarWords * k + kBarStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull;
    const long long tot = spoilt ? kPfVoid : Sll;
    if (a.total) *a.total = tot;
    *a.totalScratch = tot;
  }
  PF_STAMP(6)
}
