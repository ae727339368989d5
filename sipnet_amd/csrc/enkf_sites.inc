// enkf_sites.inc -- the per-site analysis, for the per-site call's arguments (EnkfArgs) or the joint call's (JointArgs):
// enkfSiteKernel, one workgroup per site (enkfSites launches it), and the per-chunk kernels, one launch per stage (enkfFront,
// enkfSites' loop over the observations and enkfEnd launch them; the localized, block-local and smoothing calls reuse them).
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
    if (liveAt(a, s, j)) loadMember<T>(a, W, ldw, j, base + j);
  const double nd = (double)n;
  const double lam = lambdaOf(a, s, 0);
  if (inflates(a, s, lam)) {
    siteSums(g, nv, nCh, [&](int64_t j, int q) { return liveAt(a, s, j) ? W[(int64_t)q * ldw + j] : 0.0; });
    if (tid < nv) g.mean[tid] = g.tot[tid] / nd;
    __syncthreads();
    for (int64_t j = tid; j < a.M; j += 256)
      if (liveAt(a, s, j)) inflateMember(a, s, W, ldw, j, g.mean, lam);
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
  if (i < 0) return !inflates(a, s, lambdaOf(a, s, 0));
  return a.obs[(int64_t)s * a.nObs + i] != a.obs[(int64_t)s * a.nObs + i];
}

template <typename T, class A>
__global__ __launch_bounds__(256) void enkfLoadKernel(A a) {
  __shared__ int smI[4];
  const int s = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int64_t j = (int64_t)blockIdx.y * 256 + tid, col = (int64_t)s * a.M + j;
  const bool live = liveAt(a, s, j);
  if (live) loadMember<T>(a, a.work + (int64_t)s * a.M, a.ncol, j, col);
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
  if (i < 0) return inflateMember(a, s, a.work + (int64_t)s * a.M, a.ncol, j, st, lambdaOf(a, s, 0));
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
