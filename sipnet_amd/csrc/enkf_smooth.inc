// enkf_smooth.inc -- the smoother of a window's series (sipnet_batch_enkf_analysis_smooth): the constants, arguments and two
// kernels of its series stage (enkf.hip includes the parts).
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
