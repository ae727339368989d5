// enkf_block.inc -- the block-local analysis (sipnet_batch_enkf_analysis_block): its constants and its kernel (enkf.hip
// includes the parts).
// One workgroup per target site t, all targets in one launch.  t's variables are its nA analysed pools and p rows: the predicted
// observations h_{u,i} of the code-1 sites u that reach it (and its own), read over L_t from the working copies, which nothing
// writes after the inflation -- so the private copies of the contract need no memory.  The serial square-root update is linear
// in the variables, so it runs on their sample covariance: one pass over the members forms C = cov(variable, row) ([nA + p][p]),
// the chain of p updates works on C, the means and the transform T (variable = its forecast + sum_w T[.][w] (row w's forecast
// anomaly)) alone, and a last pass applies T to the members.  Since alpha (2 - alpha var(h) / D) = 1, a step takes C to its
// Schur complement: C[v][w] -= K_v C[h][w].
// The matrices: Cx, Tx [nA][p] of the pools; S [p][p] holds C of the rows in its upper triangle (S[k][w], w >= k) and T of the
// rows strictly below the diagonal (T[k][k] = 1 is implied).  They live in LDS, where the staging tile was, when every target's
// fit (kLds), else in the target's block of global memory.  Every sum is taken in one order: the members in order.
constexpr int kBlockRows = SIPNET_ENKF_BLOCK_MAX_ROWS;
constexpr int kBlockVars = kPools + kBlockRows;
constexpr int kTile = 32;                  // members staged per tile
constexpr int kBlockMembers = 256 * kMaxGroupChunks;
constexpr int kBatch = 8;                  // loads in flight per thread before their stores
constexpr int kBlockMaxTiles = 32 * 33 / 2 + 4 * 32;   // blocks of 4 x 4 entries of C at 128 rows and 13 pools
constexpr int kBlockSmall = 48;            // targets of up to this many rows and 512 members: 256 threads; else 1024 (the chain
                                           // is a chain of LDS latencies that more waves hide; small targets only pay for their
                                           // barriers).  The arithmetic does not depend on the number of threads.

struct BlockLds {
  int64_t rowOff[kBlockVars];              // variable v of member j: a.work[rowOff[v] + j] (v < nA: t's pools, then its rows)
  double y[kBlockRows], R[kBlockRows];
  double mean0[kBlockVars], mean[kBlockVars], K[kBlockVars];
  int32_t srcOk[kBlockRows];               // in-neighbour k: every member of L_t is live there
  double alpha;
  int32_t p, selfPos;
  unsigned char flag[kBlockRows];          // slot (source, operator) of t: 1 a row, 2 a dropped row
  uint16_t tile[kBlockMaxTiles];           // C's blocks of 4 x 4 entries: (row block << 8) | column block
  unsigned char live[kBlockMembers];
};
__host__ __device__ inline int round4(int x) { return (x + 3) & ~3; }
// doubles of a target's matrices and of the staging tile
__host__ __device__ inline size_t blockMatSize(int nA, int p) { return (size_t)(p + 2 * nA) * (size_t)p; }
__host__ __device__ inline int blockStagePitch(int nA, int p) { return round4(round4(p) + nA); }

template <bool kLds, int kBlockThreads>
__global__ __launch_bounds__(kBlockThreads) void enkfBlockKernel(EnkfArgs a, const int64_t* inPtr, const int32_t* in, const double* inRho,
                                                       double* matGlobal, int64_t matPitch, int32_t* rowsOut) {
  constexpr int kBlockTiles = (kBlockMaxTiles + kBlockThreads - 1) / kBlockThreads;   // blocks of 4 x 4 entries of C a thread owns
  extern __shared__ __attribute__((aligned(16))) double blockDyn[];
  __shared__ BlockLds g;
  const int t = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nA = a.nA;
  const int64_t M = a.M;
  if (splitCode(a, t) != kAnalysed) {
    if (rowsOut && tid < 2) rowsOut[2 * (int64_t)t + tid] = 0;
    return;
  }
  for (int64_t j = tid; j < M; j += kBlockThreads) g.live[j] = liveAt(a, t, j) ? 1 : 0;
  __syncthreads();
  // which in-neighbours cover L_t
  const int64_t in0 = inPtr[t], nIn = inPtr[t + 1] - in0;
  for (int k = wave; k < nIn; k += kBlockThreads / 64) {
    const int u = in[in0 + k];
    int missing = 0;
    if (splitCode(a, u) == kAnalysed)
      for (int64_t j = lane; j < M; j += 64) missing += g.live[j] && !liveAt(a, u, j) ? 1 : 0;
    missing = waveSum(missing);
    if (lane == 0) g.srcOk[k] = missing == 0;
  }
  if (tid < nIn && in[in0 + tid] < t && (tid + 1 == nIn || in[in0 + tid + 1] > t)) g.selfPos = tid + 1;   // (one writer)
  if (tid == 0 && (nIn == 0 || in[in0] > t)) g.selfPos = 0;
  __syncthreads();
  // the rows in site-major order: t takes its place among its in-neighbours (ascending); a thread per slot (source, operator)
  const int nSlots = ((int)nIn + 1) * a.nObs;   // (at most kBlockRows: the host refuses lists beyond the cap)
  int flag = 0;                                 // 1 a row, 2 a dropped row
  double y = 0.0, R = 0.0;
  int64_t off = 0;
  if (tid < nSlots) {
    const int q = tid / a.nObs, i = tid - q * a.nObs, selfPos = g.selfPos;
    const bool self = q == selfPos;
    const int64_t k = in0 + (q < selfPos ? q : q - 1);
    const int u = self ? t : in[k];
    const double rho = self ? 1.0 : inRho[k], e = a.sd[(int64_t)u * a.nObs + i];
    y = a.obs[(int64_t)u * a.nObs + i];
    if (splitCode(a, u) == kAnalysed && y == y) flag = self || g.srcOk[k - in0] ? 1 : 2;
    R = (e * e) / rho;
    off = (int64_t)(nA + i) * a.ncol + (int64_t)u * M;
    g.flag[tid] = (unsigned char)flag;
  }
  __syncthreads();
  if (flag == 1) {
    int row = 0;
    for (int e = 0; e < tid; e++) row += g.flag[e] == 1 ? 1 : 0;
    g.rowOff[nA + row] = off;
    g.y[row] = y;
    g.R[row] = R;
  }
  if (tid < nA) g.rowOff[tid] = (int64_t)tid * a.ncol + (int64_t)t * M;
  if (tid == 0) {
    int p = 0, dropped = 0;
    for (int e = 0; e < nSlots; e++) {
      p += g.flag[e] == 1 ? 1 : 0;
      dropped += g.flag[e] == 2 ? 1 : 0;
    }
    g.p = p;
    if (rowsOut) {
      rowsOut[2 * (int64_t)t] = p;
      rowsOut[2 * (int64_t)t + 1] = dropped;
    }
  }
  __syncthreads();
  const int p = g.p, V = nA + p;
  if (p == 0) return;   // (its pools stay as inflated; the limits follow)
  const double nd = (double)a.site[2 * (int64_t)t + 1];
  const int P4 = round4(p), pitch = blockStagePitch(nA, p);
  double* stage = blockDyn;                                       // [kTile][pitch]: the rows first, then the pools
  double* S = kLds ? blockDyn : matGlobal + (int64_t)t * matPitch;
  double* Cx = S + (size_t)p * p;
  double* Tx = Cx + (size_t)nA * p;
  // the forecast means
  for (int vb = wave; vb < V; vb += kBlockThreads / 16) {   // (four variables of a wave at a time: their loads overlap)
    double sum[4] = {};
    for (int64_t j = lane; j < M; j += 64)
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (vb + kBlockThreads / 64 * u < V) sum[u] += g.live[j] ? a.work[g.rowOff[vb + kBlockThreads / 64 * u] + j] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const double tot = waveSum(sum[u]);
      if (lane == 0 && vb + kBlockThreads / 64 * u < V) g.mean0[vb + kBlockThreads / 64 * u] = g.mean[vb + kBlockThreads / 64 * u] = tot / nd;
    }
  }
  // the blocks of 4 x 4 entries of C in staging order (the rows, then the pools): of the rows' blocks only those on or above
  // the diagonal.  Block number k belongs to thread k % kBlockThreads.
  const int nWt = P4 / 4, nXt = (pitch - P4) / 4, nTri = nWt * (nWt + 1) / 2, nB = nTri + nXt * nWt;
  for (int rt = tid; rt < nWt + nXt; rt += kBlockThreads) {
    const int first = rt < nWt ? rt : 0, at = rt < nWt ? rt * nWt - rt * (rt - 1) / 2 : nTri + (rt - nWt) * nWt;
    for (int wt = first; wt < nWt; wt++) g.tile[at + wt - first] = (uint16_t)((rt << 8) | wt);
  }
  __syncthreads();
  // C: the centred products, a tile of members at a time.  A thread keeps its blocks in registers over all the tiles, so an
  // entry is the sum over the members in order, and the staging tile shares its LDS with the matrices, written afterwards.
  int r0[kBlockTiles], w0[kBlockTiles];
  double acc[kBlockTiles][4][4] = {};
#pragma unroll
  for (int k = 0; k < kBlockTiles; k++) {
    const int blk = tid + kBlockThreads * k;
    r0[k] = blk < nB ? 4 * (g.tile[blk] >> 8) : -1;
    w0[k] = blk < nB ? 4 * (g.tile[blk] & 255) : 0;
  }
  for (int64_t j0 = 0; j0 < M; j0 += kTile) {
    for (int k0 = tid; k0 < pitch * kTile; k0 += kBlockThreads * kBatch) {   // (a batch of loads, then its stores)
      double val[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; u++) {
        const int k = k0 + kBlockThreads * u, sv = k / kTile, jj = k % kTile;
        const int v = sv < P4 ? (sv < p ? nA + sv : -1) : (sv - P4 < nA ? sv - P4 : -1);
        const int64_t j = j0 + jj;
        val[u] = k < pitch * kTile && v >= 0 && j < M && g.live[j] ? a.work[g.rowOff[v] + j] - g.mean0[v] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kBatch; u++) {
        const int k = k0 + kBlockThreads * u;
        if (k < pitch * kTile) stage[(k % kTile) * pitch + k / kTile] = val[u];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kBlockTiles; k++)
      if (r0[k] >= 0)
        for (int jj = 0; jj < kTile; jj++) {
          const double2* ra = (const double2*)(stage + jj * pitch + r0[k]);
          const double2* wb = (const double2*)(stage + jj * pitch + w0[k]);
          const double2 a0 = ra[0], a1 = ra[1], b0 = wb[0], b1 = wb[1];
          const double av[4] = {a0.x, a0.y, a1.x, a1.y}, bv[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
          for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[k][r][c] += av[r] * bv[c];
        }
    __syncthreads();
  }
  for (size_t k = tid; k < blockMatSize(nA, p); k += kBlockThreads) S[k] = 0.0;   // (T starts at 0: its unit diagonal is implied)
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kBlockTiles; k++)
    if (r0[k] >= 0)
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int sv = r0[k] + r, w = w0[k] + c;
          if (w >= p) continue;
          if (sv < P4) {
            if (sv < p && w >= sv) S[(size_t)sv * p + w] = acc[k][r][c] / (nd - 1.0);
          } else if (sv - P4 < nA) {
            Cx[(size_t)(sv - P4) * p + w] = acc[k][r][c] / (nd - 1.0);
          }
        }
  __syncthreads();
  // the chain
  for (int l = 0; l < p; l++) {
    const double* Sl = S + (size_t)l * p;
    const double innov = g.y[l] - g.mean[nA + l];
    if (tid < V) {   // (the divisions and the square root in the few waves that hold a variable, not in all of them)
      const double R = g.R[l], D = Sl[l] + R;
      g.K[tid] = tid < nA ? Cx[(size_t)tid * p + l] / D : (tid - nA > l ? Sl[tid - nA] / D : 0.0);
      if (tid == 0) g.alpha = 1.0 / (1.0 + sqrt(R / D));
    }
    __syncthreads();
    const double alpha = g.alpha;
    if (tid < V) g.mean[tid] += g.K[tid] * innov;
    // the pools, then the rows after l: column w of kBatch of them at a time (their loads, then their stores).  Left of the
    // diagonal entry l the column is T's, right of it C's; of a row k's C only w >= k is kept.
    const int nR = nA + (p - 1 - l), w = tid & 127;
    if (w < p) {
      const double slw = Sl[w];
      for (int rb = tid >> 7; rb < nR; rb += kBlockThreads / 128 * kBatch) {
        double val[kBatch], K[kBatch];
        int at[kBatch];   // (the entry's place counted from S: S | Cx | Tx)
#pragma unroll
        for (int u = 0; u < kBatch; u++) {
          const int r = rb + kBlockThreads / 128 * u, k = r < nA ? -1 : l + 1 + (r - nA);
          at[u] = -1;
          if (r < nR && (w <= l || k < 0 || w >= k)) at[u] = (k >= 0 ? k : p + (w <= l ? nA : 0) + r) * p + w;
          K[u] = r < nR ? g.K[k < 0 ? r : nA + k] : 0.0;
          val[u] = at[u] >= 0 && w != l ? S[at[u]] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kBatch; u++)
          if (at[u] >= 0) S[at[u]] = w < l ? val[u] - (alpha * K[u]) * slw : (w == l ? -(alpha * K[u]) : val[u] - K[u] * slw);
      }
    }
    __syncthreads();
  }
  // the members: forecast + the mean's shift + T x (the rows' forecast anomalies)
  for (int64_t j = tid; j < M; j += kBlockThreads)
    if (g.live[j]) {
      double acc[kPools] = {};
#pragma unroll 8
      for (int w = 0; w < p; w++) {
        const double d = a.work[g.rowOff[nA + w] + j] - g.mean0[nA + w];
#pragma unroll
        for (int q = 0; q < kPools; q++)
          if (q < nA) acc[q] += Tx[(size_t)q * p + w] * d;
      }
#pragma unroll
      for (int q = 0; q < kPools; q++)
        if (q < nA) {
          double* x = a.work + g.rowOff[q] + j;
          *x = (*x + (g.mean[q] - g.mean0[q])) + acc[q];
        }
    }
}
