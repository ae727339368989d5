// pf_metropolis.inc -- a Metropolis move over the members of a site (sipnet_batch_mcmc_propose, sipnet_batch_mcmc_accept): the
// differential-evolution proposal of ter Braak (2006), x' = x_j + gamma (x_r1 - x_r2) (+ a small jitter), for the members of
// ONE HALF of a site with both partners drawn from the live members of the OTHER half (the complementary-ensemble construction
// of Foreman-Mackey et al. 2013), and the accept / restore step.  Given the other half the moving chains are independent and
// the proposal is symmetric, so a whole half moves at once and detailed balance holds exactly.
//
// The draw is pf_random.inc's counter-based Philox: one call per member, block kMcBlock, gives the two partner ranks (words 0
// and 1, mcDraws) and the accept step's uniform (word 2); the jitter's normals are blocks kMcJitterBlock ...  The listed rows and
// the write of a member's rows are site_device.h's (ListedRows, MemberRows), the host side is pf_moves.inc.  A partner is
// a RANK among the live members of the other half in ascending member index; a rank becomes a member by popcounts over the
// waves' __ballot masks of live lanes (the other half's lanes are the even or the odd bits) and a select of the n-th set bit
// in six halvings -- no loop over lanes, no list of live members in memory.
//
// Two paths with the same bits.  mcGroupKernel: one workgroup per site, for sites of one chunk (at most 256 members) -- the
// four masks through LDS, the listed rows staged in LDS so both partner gathers hit it and HBM is read once.  The split path
// for larger sites (and under SIPNET_KOPT_PF_MULTI_LAUNCH): mcMaskKernel (a chunk's four masks and counts) | mcSiteKernel (the
// counts to exclusive offsets in chunk order, the site's code) | mcProposeKernel (a rank's chunk by bisection of the offsets,
// its member from that chunk's masks, the partner rows from HBM) | mcInfoKernel.  Only the moving half is written and only the
// other half is gathered, so no launch reads a row that it writes.  The accept step is a launch per (site, chunk) in both
// paths: it reads no other column.  No atomic, no grid barrier, no spin.
constexpr int kMcDone = SIPNET_MCMC_DONE, kMcTooFew = SIPNET_MCMC_TOO_FEW, kMcBadInput = SIPNET_MCMC_BAD_INPUT,
              kMcNotSelected = SIPNET_MCMC_NOT_SELECTED;
constexpr int kMcOffCap = 2048;           // chunk offsets staged in LDS; a site of more chunks bisects the rest in global memory
constexpr uint64_t kMcEvenLanes = 0x5555555555555555ull;

struct McArgs : ListedRows {
  int32_t half;
  const double* gamma;                     // [n_sites] (propose)
  const double* jitter;                    // [n_sites] or null (propose)
  const double* beta;                      // [n_sites] or null: 1 (accept)
  DrawKey key;
  const int64_t* siteTotal;                // [n_sites] or null: every site (propose)
  int32_t* info;                           // [n_sites][4]
  const double* state;                     // [NSTATE][ncol]: the status row is read, nothing is written
  double* prm;                             // [NPARAMS][ncol], every column its own rows
  double* saved;                           // [nPrm][ncol]
  int32_t* moved;                          // [ncol]
  const double* logpNew;                   // [ncol] (accept)
  double* logpCur;                         // [ncol] (accept)
  int64_t ncol, M;
  const int32_t* siteStatus;
  int32_t nCh;                             // chunks of 256 members per site
  // per (site, chunk) scratch
  uint64_t* masks;                         // [n_sites][nCh][4] a chunk's live lanes, wave by wave (split propose)
  int32_t* cntB;                           // [n_sites][nCh] live members of the other half (split propose)
  int32_t* off;                            // [n_sites][nCh] ... as exclusive offsets in chunk order
  int32_t* cntA;                           // [n_sites][nCh] live members of the moving half; accept: live members
  int32_t* made;                           // [n_sites][nCh] proposals made; accept: members handled
  int32_t* taken;                          // [n_sites][nCh] accept: proposals accepted
  int32_t* site;                           // [n_sites][3] the site's code, nB and live members of the moving half
};

// the bits of a wave's live mask that belong to the moving half (other == false) or to the other one
__device__ __forceinline__ uint64_t mcHalfBits(const McArgs& a, uint64_t mask, bool other) {
  return mask & ((((a.half ^ (other ? 1 : 0)) & 1) == 0) ? kMcEvenLanes : ~kMcEvenLanes);
}
// a proposing site's inputs: kMcNotSelected, kMcBadInput, or kMcDone (before the count of partners)
__host__ __device__ inline int mcProposeInputs(const double* gamma, const double* jitter, const int64_t* siteTotal, int64_t s) {
  if (siteTotal && !(siteTotal[s] > 0)) return kMcNotSelected;
  if (!(fabs(gamma[s]) < INFINITY)) return kMcBadInput;
  if (jitter && (!(jitter[s] >= 0.0) || !(jitter[s] < INFINITY))) return kMcBadInput;
  return kMcDone;
}
// an accepting site's: a beta that is not finite or <= 0 is bad input
__host__ __device__ inline int mcAcceptInputs(const double* beta, int64_t s) {
  if (beta && (!(beta[s] > 0.0) || !(beta[s] < INFINITY))) return kMcBadInput;
  return kMcDone;
}
// the position of the n-th set bit of m (n from 0, n < popcount(m)): six popcount halvings
__device__ __forceinline__ int mcSelectBit(uint64_t m, int n) {
  int pos = 0;
#pragma unroll
  for (int t = 5; t >= 0; t--) {
    const int w = 1 << t;
    const int c = __popcll(m & (((uint64_t)1 << w) - 1));
    if (n >= c) {
      n -= c;
      pos += w;
      m >>= w;
    }
  }
  return pos;
}
// the lane of a chunk (0..255) that holds rank i (i < the chunk's count) among the set bits of its four masks pm
__device__ __forceinline__ int mcSelectLane(const uint64_t pm[4], int i) {
  int wave = 0;
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const int c = __popcll(pm[q]);
    if (wave == q && i >= c) {
      i -= c;
      wave = q + 1;
    }
  }
  const uint64_t m = wave == 0 ? pm[0] : wave == 1 ? pm[1] : wave == 2 ? pm[2] : pm[3];
  return 64 * wave + mcSelectBit(m, i);
}

// One live member of the moving half of a code-1 site: its proposal (x(k): its row k now; px(k, r): row k of member r of the
// site; memberOf(i): the member at rank i of the other half), the tests, and -- if the proposal is made -- the old rows saved,
// the new ones and the derived rows written.  false: not made, nothing written.
template <class X, class PX, class R>
__device__ __forceinline__ bool mcMember(const McArgs& a, int s, int64_t j, int nB, X x, PX px, R memberOf) {
  const int64_t col = (int64_t)s * a.M + j;
  const double gamma = a.gamma[s], w = a.jitter ? a.jitter[s] : 0.0;
  const uint32_t stream = a.key.streamOf(s), member = (uint32_t)j;
  int32_t i1, i2;
  uint32_t x2;
  mcDraws(a.key, stream, member, (uint32_t)nB, &i1, &i2, &x2);
  const int64_t r1 = memberOf(i1), r2 = memberOf(i2);
  bool ok = true;
  double nv[kRejPrm], old[kRejPrm];
  MemberRows mine{a, a.prm, a.ncol, col};
#pragma unroll
  for (int blk = 0; blk < kRejPrm / 4; blk++) {
    if (4 * blk >= a.nPrm) break;
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    if (w > 0.0) memberNormals(a.key, stream, member, kMcJitterBlock + (uint32_t)blk, 4 * blk + 2 < a.nPrm, z);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int k = 4 * blk + i;
      if (k >= a.nPrm) break;
      const double xj = x(k);
      double v = xj + gamma * (px(k, r1) - px(k, r2));
      if (w > 0.0) v = v + (w * (a.hi[k] - a.lo[k])) * z[i];
      ok = ok && fabs(v) < INFINITY && v >= a.lo[k] && v <= a.hi[k];
      nv[k] = v;
      old[k] = xj;
      mine.set(k, v);
    }
  }
  ok = mine.allocOk() && ok;
  if (!ok) return false;
  // (no unroll pragma: with the loop above unrolled the compiler already knows nPrm's range on every way here and takes this
  // loop apart itself -- asked to unroll what is left, it warns; the kernels' scratch size stays 0)
  for (int k = 0; k < kRejPrm; k++) {
    if (k >= a.nPrm) break;
    a.saved[(int64_t)k * a.ncol + col] = old[k];
  }
  mine.commit(a.prm, nv);
  return true;
}

// ---- one workgroup per site: sites of one chunk -----------------------------------------------------------------------
struct McGroupLds {
  double rows[kRejPrm][256];   // the listed rows of the site's live columns
  uint64_t mask[4];            // the waves' live lanes
  int smI[4];
};

__global__ __launch_bounds__(256) void mcGroupKernel(McArgs a) {
  __shared__ McGroupLds g;
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int64_t j = tid, col = (int64_t)s * a.M + j;
  int code = mcProposeInputs(a.gamma, a.jitter, a.siteTotal, s);
  const bool live = liveIn(a, s, j);
  const uint64_t ballot = __ballot(live);
  if ((tid & 63) == 0) g.mask[tid >> 6] = ballot;
  __syncthreads();
  uint64_t pm[4];
  int nA = 0, nB = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    pm[q] = mcHalfBits(a, g.mask[q], true);
    nB += __popcll(pm[q]);
    nA += __popcll(mcHalfBits(a, g.mask[q], false));
  }
  if (code == kMcDone && nB < 2) code = kMcTooFew;
  if (code != kMcDone) {
    if (j < a.M) a.moved[col] = 0;
    if (tid == 0) writeInfo4(a.info, s, code, 0, nA, nB);
    return;
  }
  for (int q = 0; q < a.nPrm; q++) g.rows[q][tid] = live ? a.prm[(int64_t)a.prmRow[q] * a.ncol + col] : 0.0;
  __syncthreads();
  int made = 0;
  if (live && (tid & 1) == a.half) {
    made = mcMember(a, s, j, nB, [&](int k) { return g.rows[k][tid]; },
                    [&](int k, int64_t r) { return g.rows[k][r]; }, [&](int i) { return (int64_t)mcSelectLane(pm, i); })
               ? 1 : 0;
  }
  if (j < a.M) a.moved[col] = made;
  const int nMade = blockSum(g.smI, made);
  if (tid == 0) writeInfo4(a.info, s, kMcDone, nMade, nA, nB);
}

// ---- the split path: (site, chunk) launches ----------------------------------------------------------------------------
// a chunk's four masks of live lanes, its live members of the other half and of the moving half
__global__ __launch_bounds__(256) void mcMaskKernel(McArgs a) {
  __shared__ uint64_t sm[4];
  const int s = (int)blockIdx.x, c = (int)blockIdx.y, tid = (int)threadIdx.x;
  const int64_t j = (int64_t)c * 256 + tid, at = (int64_t)s * a.nCh + c;
  const uint64_t ballot = __ballot(liveIn(a, s, j));
  if ((tid & 63) == 0) {
    sm[tid >> 6] = ballot;
    a.masks[4 * at + (tid >> 6)] = ballot;
  }
  __syncthreads();
  if (tid == 0) {
    int nA = 0, nB = 0;
    for (int q = 0; q < 4; q++) {
      nB += __popcll(mcHalfBits(a, sm[q], true));
      nA += __popcll(mcHalfBits(a, sm[q], false));
    }
    a.cntB[at] = nB;
    a.cntA[at] = nA;
  }
}
// the chunks' counts of the other half as exclusive offsets in chunk order; the site's code, nB and moving members
__global__ __launch_bounds__(256) void mcSiteKernel(McArgs a) {
  __shared__ int smB[256];
  __shared__ int smI[4];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int per = (a.nCh + 255) / 256, c0 = tid * per, c1 = c0 + per < a.nCh ? c0 + per : a.nCh;   // thread tid: chunks [c0, c1)
  const int64_t base = (int64_t)s * a.nCh;
  int mineB = 0, mineA = 0;
  for (int c = c0; c < c1; c++) {
    mineB += a.cntB[base + c];
    mineA += a.cntA[base + c];
  }
  smB[tid] = mineB;
  const int nA = blockSum(smI, mineA);   // (its barrier also stands between smB's stores and loads)
  int before = 0, nB = 0;
  for (int t = 0; t < 256; t++) {
    const int v = smB[t];
    before += t < tid ? v : 0;
    nB += v;
  }
  for (int c = c0; c < c1; c++) {
    a.off[base + c] = before;
    before += a.cntB[base + c];
  }
  int code = mcProposeInputs(a.gamma, a.jitter, a.siteTotal, s);
  if (code == kMcDone && nB < 2) code = kMcTooFew;
  if (tid == 0) a.site[3 * (int64_t)s] = code, a.site[3 * (int64_t)s + 1] = nB, a.site[3 * (int64_t)s + 2] = nA;
}
// the proposals of a chunk's members of the moving half; made[s][c] = how many were made
__global__ __launch_bounds__(256) void mcProposeKernel(McArgs a) {
  __shared__ int smOff[kMcOffCap];
  __shared__ int smI[4];
  const int s = (int)blockIdx.x, c = (int)blockIdx.y, tid = (int)threadIdx.x;
  const int64_t j = (int64_t)c * 256 + tid, col = (int64_t)s * a.M + j, base = (int64_t)s * a.nCh;
  if (a.site[3 * (int64_t)s] != kMcDone) {
    if (j < a.M) a.moved[col] = 0;
    return;
  }
  const int nB = a.site[3 * (int64_t)s + 1];
  const int staged = a.nCh < kMcOffCap ? a.nCh : kMcOffCap;
  for (int i = tid; i < staged; i += 256) smOff[i] = a.off[base + i];
  __syncthreads();
  int made = 0;
  if (liveIn(a, s, j) && (tid & 1) == a.half) {
    // the member at rank i of the other half: the last chunk whose offset is <= i, then the lane from that chunk's masks
    const auto memberOf = [&](int i) {
      int lo = 0, hi = a.nCh;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const int o = mid < staged ? smOff[mid] : a.off[base + mid];
        if (o <= i) lo = mid;
        else hi = mid;
      }
      const int o = lo < staged ? smOff[lo] : a.off[base + lo];
      uint64_t pm[4];
#pragma unroll
      for (int q = 0; q < 4; q++) pm[q] = mcHalfBits(a, a.masks[4 * (base + lo) + q], true);
      return (int64_t)lo * 256 + mcSelectLane(pm, i - o);
    };
    made = mcMember(a, s, j, nB, [&](int k) { return a.prm[(int64_t)a.prmRow[k] * a.ncol + col]; },
                    [&](int k, int64_t r) { return a.prm[(int64_t)a.prmRow[k] * a.ncol + (int64_t)s * a.M + r]; }, memberOf)
               ? 1 : 0;
  }
  if (j < a.M) a.moved[col] = made;
  const int nMade = blockSum(smI, made);
  if (tid == 0) a.made[base + c] = nMade;
}
__global__ __launch_bounds__(256) void mcInfoKernel(McArgs a) {
  __shared__ int smI[4];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int code = a.site[3 * (int64_t)s];
  const int nMade = chunkCounts(smI, a.made, s, a.nCh, code == kMcDone);
  if (tid == 0) writeInfo4(a.info, s, code, nMade, a.site[3 * (int64_t)s + 2], a.site[3 * (int64_t)s + 1]);
}

// ---- accept or restore --------------------------------------------------------------------------------------------------
// A chunk's columns with moved == 1: the comparison, then the new log-posterior kept or the saved rows put back and the
// derived rows derived again; moved cleared.  Whether the member is still live is NOT asked: a member that died in the
// proposal's run has a log-posterior of -inf and gets its rows back.  direct: the site is this one chunk, the info is written here.
__global__ __launch_bounds__(256) void mcAcceptKernel(McArgs a, int direct) {
  __shared__ int smI[3][4];
  const int s = (int)blockIdx.x, c = (int)blockIdx.y, tid = (int)threadIdx.x;
  const int64_t j = (int64_t)c * 256 + tid, col = (int64_t)s * a.M + j, at = (int64_t)s * a.nCh + c;
  const int code = mcAcceptInputs(a.beta, s);
  int handled = 0, taken = 0;
  if (code == kMcDone && j < a.M && a.moved[col] == 1) {
    handled = 1;
    uint32_t x[4];
    philox4x32_10((uint32_t)j, a.key.streamOf(s), kMcBlock, a.key.draw, a.key.key0, a.key.key1, x);
    const double u = uniformOf(x[2]);
    const double lpNew = a.logpNew[col], lpCur = a.logpCur[col];
    const double d = lpNew - lpCur;
    const double scaled = a.beta ? a.beta[s] * d : d;
    if (lpNew < INFINITY && scaled > log(u)) {
      taken = 1;
      a.logpCur[col] = lpNew;
    } else {
      const auto now = [&](int k, int row) { return a.prm[(int64_t)row * a.ncol + col]; };   // (the listed rows are back by then)
#pragma unroll
      for (int k = 0; k < kRejPrm; k++) {
        if (k >= a.nPrm) break;
        a.prm[(int64_t)a.prmRow[k] * a.ncol + col] = a.saved[(int64_t)k * a.ncol + col];
      }
      writeDerivedRows(a.prm, a.ncol, col, a.rows, now);
    }
    a.moved[col] = 0;
  }
  const int nLive = blockSum(smI[0], liveIn(a, s, j) ? 1 : 0);
  const int nHandled = blockSum(smI[1], handled);
  const int nTaken = blockSum(smI[2], taken);
  if (tid != 0) return;
  if (direct) {
    writeInfo4(a.info, s, code, nHandled, nTaken, nLive);
  } else {
    a.cntA[at] = nLive, a.made[at] = nHandled, a.taken[at] = nTaken;
  }
}
__global__ __launch_bounds__(256) void mcAcceptInfoKernel(McArgs a) {
  __shared__ int smI[3][4];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int nLive = chunkCounts(smI[0], a.cntA, s, a.nCh), nHandled = chunkCounts(smI[1], a.made, s, a.nCh),
            nTaken = chunkCounts(smI[2], a.taken, s, a.nCh);
  if (tid == 0) writeInfo4(a.info, s, mcAcceptInputs(a.beta, s), nHandled, nTaken, nLive);
}
