// enkf_local.inc -- the localized analysis (sipnet_batch_enkf_analysis_local): its kernels (enkf.hip includes the parts).
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
