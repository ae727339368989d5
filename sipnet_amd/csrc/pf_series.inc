// pf_series.inc -- every member's log-likelihood of a window's series against observed series with gaps
// (sipnet_batch_series_loglik): LoglikArgs, the tile staging (loglikStage), the tile's sum (loglikTileSum), loglikKernel
// (path 1: a workgroup walks every tile of its columns) and loglikTileKernel + loglikCombineKernel (path 2: a grid over
// (tile, column chunk) and a second launch that adds the tiles' sums in tile order).
//
// A workgroup owns 256 neighbouring columns of ONE site, so its lanes read neighbouring addresses of a series row and the
// site's observation rows are the same for all of them: whether a row is a gap is uniform over the workgroup.  A tile is 256
// observation rows = the 256 threads: thread t stages row t -- the observation, 1 / sd and the row's constant -- and the used
// rows are COMPACTED in LDS (one ballot per wavefront), so the loop over the tile runs over used rows only and a gap row
// costs none of its sum_steps loads.  The order of the additions is the contract's (used rows ascending from +0.0 inside a
// tile, tiles ascending, terms ascending, then add), the same on both paths: an empty tile adds its +0.0 on both.
constexpr int kLoglikTile = SIPNET_LOGLIK_TILE_ROWS;
constexpr int kLoglikMaxTerms = SIPNET_LOGLIK_MAX_TERMS;
static_assert(kLoglikTile == 256, "a thread stages one row of a tile");
constexpr int kLoglikInFlight = 16;   // rows of a one-step term whose loads a lane issues before it adds the first
constexpr int kLoglikBad = 1 << 30;   // set in a tile's "rows used" when it holds bad input (the count is of its good rows)
struct LoglikTerm {
  const void* series;
  const double* obs;   // [n_sites][rows]
  const double* sd;
  int32_t rows, sumSteps, kind, tiles;
  double scale;
};
struct LoglikArgs {
  LoglikTerm term[kLoglikMaxTerms];
  int32_t nTerms, normalise, chunksPerSite, tilesTotal;
  int64_t ld, M, ncol;
  const double* status;
  const double* add;       // [ncol] or null; may be `out`
  double* out;             // [ncol]
  double* parts;           // [nTerms][ncol] or null
  int32_t* used;           // [n_sites][nTerms] or null
  int32_t* siteInfo;       // [n_sites][2] or null
  double* partial;         // path 2: [tilesTotal][ncol] the tiles' sums
  int32_t* tileUsed;       // path 2: [n_sites][tilesTotal] rows used, | kLoglikBad
};
struct LoglikLds {
  double obs[kLoglikTile], inv[kLoglikTile], cst[kLoglikTile];   // of the used rows, compacted
  unsigned short row[kLoglikTile];                               // ... and which row of the tile each is
  int waveUsed[4], waveBad[4];
};
// Stage tile `tile` of term t for site s: -> the number of used rows (the same in every thread), | kLoglikBad when a row has
// a non-NaN non-finite obs or, its obs not NaN, an sd not finite and > 0 (such a row is not counted).  The first barrier
// also ends the reads of the tile before.
__device__ __forceinline__ int loglikStage(const LoglikTerm& t, int normalise, int s, int tile, LoglikLds& L) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = (int64_t)tile * kLoglikTile + tid;
  bool use = false, bad = false;
  double y = 0.0, inv = 0.0, cst = 0.0;
  if (r < t.rows) {
    y = t.obs[(int64_t)s * t.rows + r];
    if (y == y) {   // (a gap's sd is not read)
      const double sd = t.sd[(int64_t)s * t.rows + r];
      if (!(fabs(y) < INFINITY) || !(sd > 0.0) || !(sd < INFINITY)) {
        bad = true;
      } else {
        use = true;
        inv = 1.0 / sd;
        if (normalise) cst = t.kind == SIPNET_LOGLIK_LAPLACE ? -(log(sd) + 0.69314718055994530942) : -(log(sd) + 0.91893853320467274178);
      }
    }
  }
  const unsigned long long mask = __ballot(use), badMask = __ballot(bad);
  __syncthreads();
  if (lane == 0) {
    L.waveUsed[wave] = __popcll(mask);
    L.waveBad[wave] = badMask != 0 ? 1 : 0;
  }
  __syncthreads();
  int pos = __popcll(mask & ((1ull << lane) - 1ull));
  for (int k = 0; k < wave; k++) pos += L.waveUsed[k];
  if (use) {
    L.obs[pos] = y;
    L.inv[pos] = inv;
    L.cst[pos] = cst;
    L.row[pos] = (unsigned short)tid;
  }
  const int nUsed = L.waveUsed[0] + L.waveUsed[1] + L.waveUsed[2] + L.waveUsed[3];
  const int anyBad = L.waveBad[0] | L.waveBad[1] | L.waveBad[2] | L.waveBad[3];
  __syncthreads();
  return anyBad ? nUsed | kLoglikBad : nUsed;
}
// one row's term from the modelled value h: a subtract, a multiply and a fused multiply-add (Gauss; with cst = 0 the bits of
// logWeightOf's -0.5 z z), or an abs and a fused multiply-add (Laplace)
__device__ __forceinline__ double loglikRowTerm(double h, double y, double inv, double cst, bool laplace) {
  const double d = h - y;
  if (laplace) return __builtin_fma(-fabs(d), inv, cst);
  const double z = d * inv;
  return __builtin_fma(-0.5 * z, z, cst);
}
// The staged tile's sum for column c: used rows ascending from +0.0.  Independent loads in flight per lane -- kLoglikInFlight
// rows at a time when a row is one series row, eight steps of a row's sum otherwise (logWeightOf's finding: one dependent
// load per step left such a pass latency-bound) -- and the additions still in the defined order.
template <typename T>
__device__ __forceinline__ double loglikTileSum(const LoglikTerm& t, const LoglikLds& L, int nUsed, int tile, int64_t ld, int64_t c) {
  const T* __restrict__ x = (const T*)t.series;
  const int64_t row0 = (int64_t)tile * kLoglikTile;
  const bool laplace = t.kind == SIPNET_LOGLIK_LAPLACE;
  const double scale = t.scale;
  double sum = 0.0;
  if (t.sumSteps == 1) {
    int i = 0;
    for (; i + kLoglikInFlight <= nUsed; i += kLoglikInFlight) {
      T v[kLoglikInFlight];
#pragma unroll
      for (int k = 0; k < kLoglikInFlight; k++) v[k] = x[(row0 + L.row[i + k]) * ld + c];
#pragma unroll
      for (int k = 0; k < kLoglikInFlight; k++)
        sum += loglikRowTerm(scale * (double)v[k], L.obs[i + k], L.inv[i + k], L.cst[i + k], laplace);
    }
    for (; i < nUsed; i++)
      sum += loglikRowTerm(scale * (double)x[(row0 + L.row[i]) * ld + c], L.obs[i], L.inv[i], L.cst[i], laplace);
    return sum;
  }
  const int n = t.sumSteps;
  for (int i = 0; i < nUsed; i++) {
    const T* __restrict__ p = x + (row0 + L.row[i]) * n * ld + c;
    double acc = 0.0;
    int q = 0;
    for (; q + 8 <= n; q += 8) {
      T v[8];
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = p[(int64_t)(q + k) * ld];
#pragma unroll
      for (int k = 0; k < 8; k++) acc += (double)v[k];
    }
    for (; q < n; q++) acc += (double)p[(int64_t)q * ld];
    sum += loglikRowTerm(scale * acc, L.obs[i], L.inv[i], L.cst[i], laplace);
  }
  return sum;
}
// workgroup blockIdx -> its site, its column (clamped into the site for the loads) and whether the lane has one
struct LoglikCols {
  int s, chunk;
  int64_t c;
  bool mine;
};
__device__ __forceinline__ LoglikCols loglikCols(const LoglikArgs& a, int64_t group) {
  LoglikCols k;
  k.s = (int)(group / a.chunksPerSite);
  k.chunk = (int)(group - (int64_t)k.s * a.chunksPerSite);
  const int64_t j = (int64_t)k.chunk * 256 + threadIdx.x;
  k.mine = j < a.M;
  k.c = (int64_t)k.s * a.M + (k.mine ? j : a.M - 1);
  return k;
}
// what a column gets once its terms' sums are known (the member and site rules); the site's first workgroup reports the site
__device__ __forceinline__ void loglikFinish(const LoglikArgs& a, const LoglikCols& k, const double* termSum, const int* termUsed,
                                             bool bad) {
  int all = 0;   // (the loops over the terms are unrolled: the arrays stay in registers)
#pragma unroll
  for (int q = 0; q < kLoglikMaxTerms; q++)
    if (q < a.nTerms) all += termUsed[q];
  if (k.mine) {
    const bool dead = a.status[k.c] != 0.0;
    double total = 0.0;
#pragma unroll
    for (int q = 0; q < kLoglikMaxTerms; q++)
      if (q < a.nTerms) {
        const double part = bad ? NAN : dead ? -INFINITY : termSum[q];
        if (a.parts) a.parts[(int64_t)q * a.ncol + k.c] = part;
        total += part;
      }
    if (!bad && !dead && a.add) total += a.add[k.c];
    a.out[k.c] = bad ? NAN : dead ? -INFINITY : total;
  }
  if (k.chunk == 0 && threadIdx.x == 0) {
    if (a.used) {
#pragma unroll
      for (int q = 0; q < kLoglikMaxTerms; q++)
        if (q < a.nTerms) a.used[k.s * a.nTerms + q] = termUsed[q];
    }
    if (a.siteInfo) {
      a.siteInfo[2 * k.s] = bad ? -2 : all > 0 ? 1 : -1;
      a.siteInfo[2 * k.s + 1] = all;
    }
  }
}
// path 1: workgroup blockIdx.x = (site, column chunk) walks every tile of every term
template <typename T>
__global__ __launch_bounds__(256) void loglikKernel(LoglikArgs a) {
  __shared__ LoglikLds L;
  const LoglikCols k = loglikCols(a, blockIdx.x);
  double termSum[kLoglikMaxTerms];
  int termUsed[kLoglikMaxTerms];
  bool bad = false;
#pragma unroll
  for (int q = 0; q < kLoglikMaxTerms; q++) {
    termSum[q] = 0.0;
    termUsed[q] = 0;
    if (q < a.nTerms) {
      const LoglikTerm& t = a.term[q];
      for (int tile = 0; tile < t.tiles; tile++) {
        const int n = loglikStage(t, a.normalise, k.s, tile, L);
        termUsed[q] += n & ~kLoglikBad;
        if (n & kLoglikBad) {   // (the site's columns become NaN)
          bad = true;
          continue;
        }
        termSum[q] += loglikTileSum<T>(t, L, n, tile, a.ld, k.c);
      }
    }
  }
  loglikFinish(a, k, termSum, termUsed, bad);
}
// path 2, launch 1: workgroup blockIdx.x = tile index (over all terms) * groups + (site, column chunk): one tile's sum
template <typename T>
__global__ __launch_bounds__(256) void loglikTileKernel(LoglikArgs a, int64_t groups) {
  __shared__ LoglikLds L;
  const int64_t y = (int64_t)blockIdx.x / groups;
  const LoglikCols k = loglikCols(a, (int64_t)blockIdx.x - y * groups);
  int q = 0, tile = (int)y;
  while (tile >= a.term[q].tiles) tile -= a.term[q++].tiles;   // (y < tilesTotal)
  const LoglikTerm& t = a.term[q];
  const int n = loglikStage(t, a.normalise, k.s, tile, L);
  if (k.chunk == 0 && threadIdx.x == 0) a.tileUsed[(int64_t)k.s * a.tilesTotal + y] = n;
  if (n & kLoglikBad) return;   // (the site's columns become NaN: launch 2 does not read the tiles' sums)
  const double sum = loglikTileSum<T>(t, L, n, tile, a.ld, k.c);
  if (k.mine) a.partial[y * a.ncol + k.c] = sum;
}
// launch 2: workgroup blockIdx.x = (site, column chunk) adds its columns' tile sums in tile order
__global__ __launch_bounds__(256) void loglikCombineKernel(LoglikArgs a) {
  const LoglikCols k = loglikCols(a, blockIdx.x);
  double termSum[kLoglikMaxTerms];
  int termUsed[kLoglikMaxTerms];
  bool bad = false;
  const int32_t* tu = a.tileUsed + (int64_t)k.s * a.tilesTotal;
  for (int y = 0; y < a.tilesTotal; y++) bad = bad || (tu[y] & kLoglikBad) != 0;
  int y = 0;
#pragma unroll
  for (int q = 0; q < kLoglikMaxTerms; q++) {
    termSum[q] = 0.0;
    termUsed[q] = 0;
    if (q < a.nTerms)
      for (int tile = 0; tile < a.term[q].tiles; tile++, y++) {
        termUsed[q] += tu[y] & ~kLoglikBad;
        if (!bad) termSum[q] += a.partial[(int64_t)y * a.ncol + k.c];
      }
  }
  loglikFinish(a, k, termSum, termUsed, bad);
}
