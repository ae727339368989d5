// enkf_sharded.inc -- the per-site analysis of an ensemble sharded by member across ranks (sipnet_batch_enkf_shard_moments,
// sipnet_batch_enkf_analysis_sharded): its constants and its kernels (enkf.hip includes the parts).
// The filter is enkf_block.inc's, run on a site's small sample covariance: the covariance needs only centred moments of the
// members, and centred moments of disjoint shards combine exactly (Chan, Golub & LeVeque 1983).  A rank's moment block of site
// s is W = 2 + V + V n_obs doubles, V = nA + n_obs: {n_r, 0, mean_r [V], C_r [V][n_obs]}, C_r[v][i] = the sum over the shard's
// live members of (x_v - mean_r[v]) (h_i - mean_r[h_i]), not divided.  The first call writes this rank's blocks; the caller
// gathers every rank's; the second merges them in rank order, runs the chain on C / (n - 1) and applies the transform to this
// rank's own members.  Every rank merges the same bytes in the same order, so every rank holds the same T, bit for bit.
// Every sum is taken in one order: chunks of 256 members, a chunk by the fixed tree (waveSum, then the four waves in order),
// the chunk totals in segments of segLen(nCh) chunks, each in order from 0.0, the segments by one wave's butterfly (a site of
// at most 16 chunks: one segment, the plain sum in order).  No atomic, no grid barrier, no spin, no cap on the members.
constexpr int kShardEntries = kMaxVars * kMaxObs;                  // C_r of a site at most
constexpr int kShardPlan = 2 + kMaxVars + kPools + kPools * kMaxObs;   // a site's plan: what the apply pass reads
constexpr double kShardMaxCount = 4194304.0;                       // a block's count: an integer 0 .. the batch's most columns

__host__ __device__ inline int shardWords(int nA, int nObs) { return 2 + (nA + nObs) + (nA + nObs) * nObs; }
// a count as a rank wrote it: anything else is a foreign or torn buffer
__host__ __device__ inline bool shardCountOk(double c) { return c >= 0.0 && c <= kShardMaxCount && c == floor(c); }

// a chunk's sums of the V variables over its live members -> part[site][chunk][cap]
__global__ __launch_bounds__(256) void enkfShardSumKernel(EnkfArgs a, int cap) {
  __shared__ double smW[4 * kMaxVars];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x, c = (int)blockIdx.y;
  const int64_t j = (int64_t)c * 256 + tid, col = (int64_t)s * a.M + j;
  const bool live = liveAt(a, s, j);
  for (int q = 0; q < a.nv; q++) {
    const double v = waveSum(live ? a.work[(int64_t)q * a.ncol + col] : 0.0);
    if ((tid & 63) == 0) smW[(tid >> 6) * kMaxVars + q] = v;
  }
  __syncthreads();
  if (tid < a.nv) a.part[((int64_t)s * a.nCh + c) * cap + tid] = combine4<kMaxVars>(smW, tid);
}

// a chunk's centred products [V][n_obs] about the shard's means (in the site's block) -> part[site][chunk][cap]
__global__ __launch_bounds__(256) void enkfShardProductKernel(EnkfArgs a, int cap, const double* moments, int W) {
  __shared__ double smW[4 * kShardEntries];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x, c = (int)blockIdx.y, nObs = a.nObs;
  const int64_t j = (int64_t)c * 256 + tid, col = (int64_t)s * a.M + j;
  const bool live = liveAt(a, s, j);
  const double* mean = moments + (int64_t)s * W + 2;
  double dh[kMaxObs];
#pragma unroll
  for (int i = 0; i < kMaxObs; i++)
    dh[i] = live && i < nObs ? a.work[(int64_t)(a.nA + i) * a.ncol + col] - mean[a.nA + i] : 0.0;
  for (int v = 0; v < a.nv; v++) {
    const double dx = live ? a.work[(int64_t)v * a.ncol + col] - mean[v] : 0.0;
#pragma unroll
    for (int i = 0; i < kMaxObs; i++)
      if (i < nObs) {
        const double t = waveSum(dx * dh[i]);
        if ((tid & 63) == 0) smW[(tid >> 6) * kShardEntries + v * nObs + i] = t;
      }
  }
  __syncthreads();
  for (int e = tid; e < a.nv * nObs; e += 256) a.part[((int64_t)s * a.nCh + c) * cap + e] = combine4<kShardEntries>(smW, e);
}

// The chunk totals of a site's entries, a wave per entry (grid: sites x entries / 4), into the site's block.  centred = 0: the
// count and the means of the V variables (a site with no live member: zeros); 1: the V n_obs centred products.
__global__ __launch_bounds__(256) void enkfShardTotalKernel(EnkfArgs a, int cap, double* moments, int W, int centred) {
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, e = (int)blockIdx.y * 4 + (tid >> 6);
  if (e >= (centred ? a.nv * a.nObs : a.nv)) return;
  const int L = segLen(a.nCh), c0 = lane * L, c1 = c0 + L < a.nCh ? c0 + L : a.nCh;
  const double* part = a.part + (int64_t)s * a.nCh * cap + e;
  double t = 0.0;
  for (int c = c0; c < c1; c++) t += part[(int64_t)c * cap];
  t = waveSum(t);
  double* block = moments + (int64_t)s * W;
  if (centred) {
    if (lane == 0) block[2 + a.nv + e] = t;
    return;
  }
  int n = 0;
  for (int c = lane; c < a.nCh; c += 64) n += a.cnt[(int64_t)s * a.nCh + c];
  n = waveSum(n);
  if (lane == 0) {
    block[2 + e] = n > 0 ? t / (double)n : 0.0;
    if (e == 0) {
      block[0] = (double)n;
      block[1] = 0.0;
    }
  }
}

struct ShardLds {
  double C[kMaxVars][kMaxObs];             // the chain's cov(variable, row): the pools, then the used rows
  double T[kMaxVars][kMaxObs];
  double mean0[kMaxVars], d[kMaxVars];     // the union's forecast means of all V variables; a block's mean - the merged one
  double mean[kMaxVars], K[kMaxVars];      // the chain's means and gains: the pools, then the used rows
  double Tl[kMaxObs], Cl[kMaxObs], y[kMaxObs], R[kMaxObs];
  int32_t used[kMaxObs], pos[kMaxObs];     // the operator of row k; the row of operator i, or -1
  int32_t p, bad;
};
// One workgroup per site: the world blocks [world][n_sites][W] merged in rank order, the site's code from the union's n, the
// chain on C / (n - 1) (lambda^2 of it where the site inflates) -> a.site {code, n} and the site's plan: {the mask of the used
// operators, 0, mean0 [kMaxVars], the pools' mean shifts [kPools], T [kPools][kMaxObs] by operator}
__global__ __launch_bounds__(256) void enkfShardChainKernel(EnkfArgs a, const double* gathered, int world, int64_t nSites, int W,
                                                            double* plan) {
  __shared__ ShardLds g;
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x, nA = a.nA, nv = a.nv, nObs = a.nObs, E = nv * nObs;
  if (tid == 0) g.bad = 0;
  if (tid < nv) g.mean0[tid] = 0.0;
  __syncthreads();
  if (tid < world && !shardCountOk(gathered[((int64_t)tid * nSites + s) * W])) g.bad = 1;
  __syncthreads();
  if (g.bad) {
    if (tid == 0) {
      a.site[2 * (int64_t)s] = kBadInput;
      a.site[2 * (int64_t)s + 1] = 0;
    }
    return;
  }
  // the merge: a thread keeps its entries (tid, tid + 256) of C over the blocks
  double c[2] = {0.0, 0.0}, na = 0.0;
  for (int r = 0; r < world; r++) {
    const double* blk = gathered + ((int64_t)r * nSites + s) * W;
    const double nb = blk[0];
    if (nb == 0.0) continue;
    const double n = na + nb, f = na * nb / n;
    if (tid < nv) g.d[tid] = blk[2 + tid] - g.mean0[tid];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; u++)
      if (const int e = tid + 256 * u; e < E) c[u] += blk[2 + nv + e] + g.d[e / nObs] * g.d[nA + e % nObs] * f;
    if (tid < nv) g.mean0[tid] += g.d[tid] * (nb / n);
    __syncthreads();
    na = n;
  }
  int used;
  int code = siteInputs(a.obs, a.sd, a.infl, nObs, s, &used);
  if (code == kAnalysed && na < 2.0) code = kTooFew;
  if (tid == 0) {
    a.site[2 * (int64_t)s] = code;
    a.site[2 * (int64_t)s + 1] = (int32_t)na;
    int p = 0;
    for (int i = 0; i < nObs; i++) {
      const double y = a.obs[(int64_t)s * nObs + i], e = a.sd[(int64_t)s * nObs + i];
      g.pos[i] = y == y ? p : -1;
      if (y != y) continue;
      g.used[p] = i;
      g.y[p] = y;
      g.R[p] = e * e;
      p++;
    }
    g.p = p;
  }
  if (code != kAnalysed) return;
  __syncthreads();
  const int p = g.p, Vp = nA + p;
  const double lam = lambdaOf(a, s, 0), lam2 = inflates(a, s, lam) ? lam * lam : 1.0;
#pragma unroll
  for (int u = 0; u < 2; u++)
    if (const int e = tid + 256 * u; e < E) {
      const int v = e / nObs, w = g.pos[e % nObs], row = v < nA ? v : (g.pos[v - nA] >= 0 ? nA + g.pos[v - nA] : -1);
      if (w >= 0 && row >= 0) {
        g.C[row][w] = c[u] / (na - 1.0) * lam2;
        g.T[row][w] = 0.0;
      }
    }
  if (tid < Vp) g.mean[tid] = g.mean0[tid < nA ? tid : nA + g.used[tid - nA]];
  __syncthreads();
  for (int l = 0; l < p; l++) {
    const double R = g.R[l], D = g.C[nA + l][l] + R, alpha = 1.0 / (1.0 + sqrt(R / D)), innov = g.y[l] - g.mean[nA + l];
    if (tid < Vp) g.K[tid] = g.C[tid][l] / D;
    if (tid < p) {
      g.Tl[tid] = g.T[nA + l][tid] + (tid == l ? 1.0 : 0.0);
      g.Cl[tid] = g.C[nA + l][tid];
    }
    __syncthreads();
    if (tid < Vp) g.mean[tid] += g.K[tid] * innov;
    for (int e = tid; e < Vp * p; e += 256) {
      const int v = e / p, w = e % p;
      g.T[v][w] -= alpha * g.K[v] * g.Tl[w];
      g.C[v][w] -= g.K[v] * g.Cl[w];
    }
    __syncthreads();
  }
  double* out = plan + (int64_t)s * kShardPlan;
  if (tid == 0) {
    int mask = 0;
    for (int k = 0; k < p; k++) mask |= 1 << g.used[k];
    out[0] = (double)mask;
    out[1] = 0.0;
  }
  if (tid < nv) out[2 + tid] = g.mean0[tid];
  if (tid < nA) out[2 + kMaxVars + tid] = g.mean[tid] - g.mean0[tid];
  for (int e = tid; e < nA * nObs; e += 256) {
    const int q = e / nObs, i = e % nObs;
    out[2 + kMaxVars + kPools + q * kMaxObs + i] = g.pos[i] >= 0 ? g.T[q][g.pos[i]] : 0.0;
  }
}

// a chunk's live members of a code-1 site: forecast, inflated about the union's means, + the mean's shift + T x (the rows'
// anomalies about the union's forecast means); T from LDS, a thread per member
__global__ __launch_bounds__(256) void enkfShardApplyKernel(EnkfArgs a, const double* plan) {
  __shared__ double sm[kShardPlan];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x, nA = a.nA;
  if (splitCode(a, s) != kAnalysed) return;
  for (int k = tid; k < kShardPlan; k += 256) sm[k] = plan[(int64_t)s * kShardPlan + k];
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.y * 256 + tid;
  if (!liveAt(a, s, j)) return;
  const double *mean0 = sm + 2, *shift = mean0 + kMaxVars, *T = shift + kPools;
  const int mask = (int)sm[0];
  double* W = a.work + (int64_t)s * a.M;
  const double lam = lambdaOf(a, s, 0);
  if (inflates(a, s, lam)) inflateMember(a, s, W, a.ncol, j, mean0, lam);
  double acc[kPools] = {};
  for (int i = 0; i < a.nObs; i++) {
    if (!((mask >> i) & 1)) continue;
    const double d = W[(int64_t)(nA + i) * a.ncol + j] - mean0[nA + i];
#pragma unroll
    for (int q = 0; q < kPools; q++)
      if (q < nA) acc[q] += T[q * kMaxObs + i] * d;
  }
#pragma unroll
  for (int q = 0; q < kPools; q++)
    if (q < nA) {
      double* x = W + (int64_t)q * a.ncol + j;
      *x = (*x + shift[q]) + acc[q];
    }
}
