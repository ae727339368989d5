// pf_rejuvenate.inc -- particle rejuvenation after a resampling (sipnet_batch_pf_rejuvenate): the Liu & West (2001) kernel-
// shrinkage move of some of a site's parameter rows, and additive noise on pools.  SIPNET is deterministic, so two copies of
// a resampled particle stay identical for ever; this pass gives every copy its own draw again.
//
// The draw is pf_random.inc's counter-based Philox (blocks kRejRowBlock .. and kRejPoolBlock ..), the listed rows and the write
// of a member's rows are site_device.h's (ListedRows, MemberRows), the host side is pf_moves.inc.
// Two paths with the same bits.  rejGroupKernel: one workgroup per site, for sites of one chunk (at most 256 members) -- the
// moments of the listed rows over the site's live members (the means, then the centred sums), then the draw and the limits
// in a second sweep; the rows are staged in LDS, so HBM is read once.  The split path for larger sites (and under
// SIPNET_KOPT_PF_MULTI_LAUNCH): rejChunkKernel (a chunk's sums) | rejSiteKernel (the site's, in chunk order) twice -- sums,
// centred sums --, then rejApplyKernel | rejInfoKernel.  The draw is arithmetic (a double logarithm, square root, sine and
// cosine per pair of normals), so what counts is how many waves work at it: a workgroup that walked a whole site of several
// chunks was measured 1.3 to 8 x slower than the per-chunk launches (NOTES.md).  The sums' order is the same in both and
// depends on M only: the 256 columns of a chunk by an xor butterfly inside each wave, the four waves in order, the chunks in
// order from 0.0.  No atomic, no grid barrier, no spin.
constexpr int kRejPrm = SIPNET_ENKF_MAX_PARAMS;   // listed parameter rows at most
constexpr int kRejPools = 13;                     // state slots 0..12
constexpr int kRejDone = SIPNET_REJUVENATE_DONE, kRejTooFew = SIPNET_REJUVENATE_TOO_FEW, kRejBadInput = SIPNET_REJUVENATE_BAD_INPUT,
              kRejNotSelected = SIPNET_REJUVENATE_NOT_SELECTED;

// (keep mask, shrink and poolSd in front: behind the fields McArgs has too, rejApplyKernel compiled a quarter longer and ran a tenth slower)
struct RejArgs : ListedRows {
  int32_t mask;
  const double* shrink;                    // [n_sites] a, or null (nPrm == 0)
  const double* poolSd;                    // [n_sites][13], or null (mask == 0)
  DrawKey key;
  const int64_t* siteTotal;                // [n_sites] or null: every site
  int32_t* info;                           // [n_sites][4]
  double* state;                           // [NSTATE][ncol]
  double* prm;                             // [NPARAMS][ncol], every column its own rows
  int64_t ncol, M;
  const int32_t* siteStatus;
  int32_t nCh;                             // chunks of 256 members per site
  // split path
  double* part;                            // [n_sites][nCh][kRejPrm] a chunk's sums, then its centred sums
  double* stat;                            // [n_sites][2][kRejPrm] the site's means, then its sds
  int32_t* cnt;                            // [n_sites][nCh] live members
  int32_t* kept;                           // [n_sites][nCh] members that kept everything
  int32_t* site;                           // [n_sites][2] the site's code and live count
};

// the site's inputs: kRejNotSelected, kRejBadInput, or kRejDone (before the live count)
__host__ __device__ inline int rejSiteInputs(const double* shrink, const double* poolSd, const int64_t* siteTotal, int nPrm,
                                             int mask, int64_t s) {
  if (siteTotal && !(siteTotal[s] > 0)) return kRejNotSelected;
  if (nPrm > 0) {
    const double a = shrink[s];
    if (!(a > 0.0) || !(a <= 1.0)) return kRejBadInput;
  }
  for (int p = 0; p < kRejPools; p++)
    if (mask & (1 << p)) {
      const double q = poolSd[s * kRejPools + p];
      if (!(q >= 0.0) || !(q < INFINITY)) return kRejBadInput;
    }
  return kRejDone;
}
// rows + slots a code-1 site perturbs: the listed rows unless a == 1, the masked slots whose sd is not 0
__device__ __forceinline__ int rejPerturbed(const RejArgs& a, int s) {
  int n = (a.nPrm > 0 && a.shrink[s] != 1.0) ? a.nPrm : 0;
  for (int p = 0; p < kRejPools; p++)
    if ((a.mask & (1 << p)) && a.poolSd[(int64_t)s * kRejPools + p] > 0.0) n++;
  return n;
}

// One live member of a code-1 site: its listed rows moved (x(k): row k's value now; mean, hsd = h sd per row; shrinkA = a,
// rows untouched when it is 1), its masked pools perturbed, the limits, and -- unless the member keeps everything -- the
// write-back.  Every loop is unrolled over its compile-time extent, so the new values live in registers.  false: kept.
template <class X>
__device__ __forceinline__ bool rejMember(const RejArgs& a, int s, int64_t j, double shrinkA, const double* mean,
                                          const double* hsd, X x) {
  const int64_t col = (int64_t)s * a.M + j;
  const uint32_t stream = a.key.streamOf(s), member = (uint32_t)j;
  const bool rows = a.nPrm > 0 && shrinkA != 1.0;
  bool ok = true;
  double nv[kRejPrm];
  MemberRows mine{a, a.prm, a.ncol, col};
  if (rows) {
#pragma unroll
    for (int blk = 0; blk < kRejPrm / 4; blk++) {
      if (4 * blk >= a.nPrm) break;
      double z[4] = {0.0, 0.0, 0.0, 0.0};
      memberNormals(a.key, stream, member, kRejRowBlock + (uint32_t)blk, 4 * blk + 2 < a.nPrm, z);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int k = 4 * blk + i;
        if (k >= a.nPrm) break;
        const double m = mean[k];
        double v = (m + shrinkA * (x(k) - m)) + hsd[k] * z[i];
        if (v < a.lo[k]) v = a.lo[k] + (a.lo[k] - v);
        else if (v > a.hi[k]) v = a.hi[k] - (v - a.hi[k]);
        v = v < a.lo[k] ? a.lo[k] : (v > a.hi[k] ? a.hi[k] : v);
        ok = ok && fabs(v) < INFINITY;
        nv[k] = v;
        mine.set(k, v);
      }
    }
    ok = mine.allocOk() && ok;
  }
  // the pools: the masked slots with an sd above 0 perturbed and clipped; hasSufficientBiomass (sipnet.c:1530-1536) of the result
  double f[kRejPools];
  bool moved[kRejPools];
  const double* sd = a.poolSd + (int64_t)s * kRejPools;
#pragma unroll
  for (int blk = 0; blk < 4; blk++) {
    const int bits = (a.mask >> (4 * blk)) & 15;
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    if (bits) memberNormals(a.key, stream, member, kRejPoolBlock + (uint32_t)blk, (bits & 12) != 0, z);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int p = 4 * blk + i;
      if (p >= kRejPools) break;
      const double q = (bits & (1 << i)) ? sd[p] : 0.0;
      moved[p] = q > 0.0;
      const bool read = moved[p] || p == ST_plantWoodC || p == ST_plantCAccountingDelta || p == ST_fineRootC || p == ST_coarseRootC;
      double v = read ? a.state[(int64_t)p * a.ncol + col] : 0.0;
      if (moved[p]) {
        v = poolLimit(p, v + q * z[i]);
        ok = ok && fabs(v) < INFINITY;
      }
      f[p] = v;
    }
  }
  ok = ok && sufficientBiomass(f[ST_plantWoodC], f[ST_plantCAccountingDelta], f[ST_fineRootC], f[ST_coarseRootC]);
  if (!ok) return false;
#pragma unroll
  for (int p = 0; p < kRejPools; p++)
    if (moved[p]) a.state[(int64_t)p * a.ncol + col] = f[p];
  if (rows) mine.commit(a.prm, nv);
  return true;
}

// ---- one workgroup per site: sites of one chunk -----------------------------------------------------------------------
// A site of at most 256 members is one chunk, and the per-chunk launches would have one workgroup per site too: here their
// six launches are one, and the listed rows are read from HBM once (staged in LDS for the three sweeps).  The sums are the
// split path's: the chunk's sum by combine4, added to 0.0 (the one-chunk siteSums).
struct RejGroupLds {
  static constexpr int kCap = kRejPrm;
  double rows[kRejPrm][256];   // the listed rows of the site's columns
  double smW[4 * kRejPrm];
  double mean[kRejPrm], hsd[kRejPrm];
  int smI[4];
};

__global__ __launch_bounds__(256) void rejGroupKernel(RejArgs a) {
  __shared__ RejGroupLds g;
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int64_t j = tid, col = (int64_t)s * a.M + j;
  int code = rejSiteInputs(a.shrink, a.poolSd, a.siteTotal, a.nPrm, a.mask, s);
  const bool live = liveIn(a, s, j);
  const int n = blockCount(g, live ? 1 : 0);
  if (code == kRejDone && n < 2) code = kRejTooFew;
  if (code != kRejDone) {
    if (tid == 0) writeInfo4(a.info, s, code, 0, n, 0);
    return;
  }
  const double shrinkA = a.nPrm > 0 ? a.shrink[s] : 1.0;
  if (a.nPrm > 0 && shrinkA != 1.0) {
    for (int q = 0; q < a.nPrm; q++) g.rows[q][tid] = live ? a.prm[(int64_t)a.prmRow[q] * a.ncol + col] : 0.0;
    const double sum = siteSums(g, a.nPrm, [&](int q) { return g.rows[q][tid]; });
    if (tid < a.nPrm) g.mean[tid] = sum / (double)n;
    __syncthreads();
    const double csum = siteSums(g, a.nPrm, [&](int q) {
      const double d = g.rows[q][tid] - g.mean[q];
      return live ? d * d : 0.0;
    });
    if (tid < a.nPrm) g.hsd[tid] = sqrt((1.0 - shrinkA) * (1.0 + shrinkA)) * sqrt(csum / ((double)n - 1.0));
    __syncthreads();
  }
  int kept = 0;
  if (live) kept = rejMember(a, s, j, shrinkA, g.mean, g.hsd, [&](int k) { return g.rows[k][tid]; }) ? 0 : 1;
  const int nKept = blockSum(g.smI, kept);
  if (tid == 0) writeInfo4(a.info, s, kRejDone, rejPerturbed(a, s), n, nKept);
}

// ---- the split path: (site, chunk) launches ----------------------------------------------------------------------------
// a chunk's sums of the listed rows over its live members (pass 0, with the live count), or of their squared distances from
// the site's means (pass 1) -> part[s][c][q]
__global__ __launch_bounds__(256) void rejChunkKernel(RejArgs a, int pass) {
  __shared__ double smW[4 * kRejPrm];
  __shared__ int smI[4];
  const int s = (int)blockIdx.x, c = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t j = (int64_t)c * 256 + tid, col = (int64_t)s * a.M + j;
  const bool live = liveIn(a, s, j);
  if (pass == 0) {
    const int n = blockSum(smI, live ? 1 : 0);
    if (tid == 0) a.cnt[(int64_t)s * a.nCh + c] = n;
  } else if (a.site[2 * (int64_t)s] != kRejDone) {
    return;
  }
  const double* mean = a.stat + (int64_t)s * 2 * kRejPrm;
  for (int q = 0; q < a.nPrm; q++) {
    double v = 0.0;
    if (live) {
      const double x = a.prm[(int64_t)a.prmRow[q] * a.ncol + col];
      if (pass == 0) {
        v = x;
      } else {
        const double d = x - mean[q];
        v = d * d;
      }
    }
    v = waveSum(v);
    if (lane == 0) smW[wave * kRejPrm + q] = v;
  }
  __syncthreads();
  if (tid < a.nPrm) a.part[((int64_t)s * a.nCh + c) * kRejPrm + tid] = combine4<kRejPrm>(smW, tid);
}
// the site's sums from its chunks', in chunk order.  pass 0: the live count, the code, the means; pass 1: h sd
__global__ __launch_bounds__(256) void rejSiteKernel(RejArgs a, int pass) {
  __shared__ int smI[4];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  int n;
  if (pass == 0) {
    n = chunkCounts(smI, a.cnt, s, a.nCh);
    int code = rejSiteInputs(a.shrink, a.poolSd, a.siteTotal, a.nPrm, a.mask, s);
    if (code == kRejDone && n < 2) code = kRejTooFew;
    if (tid == 0) a.site[2 * (int64_t)s] = code, a.site[2 * (int64_t)s + 1] = n;
    if (code != kRejDone) return;
  } else {
    if (a.site[2 * (int64_t)s] != kRejDone) return;
    n = a.site[2 * (int64_t)s + 1];
  }
  // thread q adds row q's chunk sums in chunk order; the workgroup stages them 64 chunks at a time (coalesced loads in flight
  // together: one thread reading chunk after chunk pays a memory latency each)
  __shared__ double tile[64][kRejPrm + 1];
  const double* part = a.part + (int64_t)s * a.nCh * kRejPrm;
  double t = 0.0;
  for (int base = 0; base < a.nCh; base += 64) {
    const int here = a.nCh - base < 64 ? a.nCh - base : 64;
    for (int i = tid; i < here * kRejPrm; i += 256) tile[i / kRejPrm][i % kRejPrm] = (i % kRejPrm) < a.nPrm ? part[(int64_t)base * kRejPrm + i] : 0.0;
    __syncthreads();
    if (tid < a.nPrm)
      for (int c = 0; c < here; c++) t += tile[c][tid];
    __syncthreads();
  }
  if (tid >= a.nPrm) return;
  double* stat = a.stat + (int64_t)s * 2 * kRejPrm;
  if (pass == 0) {
    stat[tid] = t / (double)n;
  } else {
    const double shrinkA = a.shrink[s];
    stat[kRejPrm + tid] = sqrt((1.0 - shrinkA) * (1.0 + shrinkA)) * sqrt(t / ((double)n - 1.0));
  }
}
// the draw and the limits of a chunk's live members; kept[s][c] = its members that kept everything
__global__ __launch_bounds__(256) void rejApplyKernel(RejArgs a) {
  __shared__ int smI[4];
  const int s = (int)blockIdx.x, c = (int)blockIdx.y, tid = (int)threadIdx.x;
  if (a.site[2 * (int64_t)s] != kRejDone) return;
  const int64_t j = (int64_t)c * 256 + tid, col = (int64_t)s * a.M + j;
  const double* stat = a.stat + (int64_t)s * 2 * kRejPrm;
  const double shrinkA = a.nPrm > 0 ? a.shrink[s] : 1.0;
  int kept = 0;
  if (liveIn(a, s, j))
    kept = rejMember(a, s, j, shrinkA, stat, stat + kRejPrm, [&](int k) { return a.prm[(int64_t)a.prmRow[k] * a.ncol + col]; }) ? 0 : 1;
  const int nKept = blockSum(smI, kept);
  if (tid == 0) a.kept[(int64_t)s * a.nCh + c] = nKept;
}
__global__ __launch_bounds__(256) void rejInfoKernel(RejArgs a) {
  __shared__ int smI[4];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int code = a.site[2 * (int64_t)s];
  const int nKept = chunkCounts(smI, a.kept, s, a.nCh, code == kRejDone);
  if (tid == 0) writeInfo4(a.info, s, code, code == kRejDone ? rejPerturbed(a, s) : 0, a.site[2 * (int64_t)s + 1], nKept);
}
