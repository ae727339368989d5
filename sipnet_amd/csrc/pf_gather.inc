// pf_gather.inc -- the column gathers that move a member's checkpoint (state rows, ring rows, parameter rows or the parameter
// index): gatherMemberKernel, from the batch's own matrices and from packed blocks received from other ranks (RecvMap), and
// gatherPeerKernel, straight out of the peers' matrices (PeerPtrs); the small kernels that go with them (exponentCheckKernel,
// iotaKernel, copyRowsKernel); and, host code, the one launch of gatherMemberKernel (GatherCall, launchGatherMember).

constexpr int kMaxBlocks = 16;  // source ranks whose packed blocks one gather can read

// Where the received columns live: block s holds [rows][n[s]] doubles at off[s]; received
// column k (0-based over all blocks) is in the block with start[s] <= k < start[s+1].
struct RecvMap {
  int32_t nBlocks;
  int64_t start[kMaxBlocks + 1];
  int64_t off[kMaxBlocks];
  int64_t n[kMaxBlocks];
};

// dst[row][j] = (src[j] < ncol) ? own[row][src[j]] : recv(row + recvRow0, src[j] - ncol)
// One thread moves kGatherRows rows of its column: the source index is read once and
// kGatherRows independent loads are in flight per thread (HBM-bound streaming copy).
constexpr int kGatherRows = 8;
// rows of 8-byte words the ring takes in a packed block (a row of floats = half a row of words; 250 is even)
static inline int ringWords(bool ringF32) { return ringF32 ? SIPNET_RING_SLOTS / 2 : SIPNET_RING_SLOTS; }
static_assert(SIPNET_RING_SLOTS % 2 == 0, "a packed block keeps the parameter rows 8-byte aligned");
// One launch for the three matrices of a member's checkpoint (state rows, ring rows,
// then parameter rows: the row order of a packed block): blockIdx.y walks the row groups of all three,
// so a resampling or a pack is one kernel instead of three (launch gaps were a third of the analysis
// step's GPU time, profiles/r02_c5.md)
struct GatherPart {
  const void* own;     // [rows][ownPitch] of 8-byte (doubles) or 4-byte (floats: the ring of an fp32-mixed batch) elements
  void* dst;           // [rows][dstPitch]
  int32_t rows, group0;   // group0: first row group (blockIdx.y) of this part
  int32_t recvRow0;       // where the part starts inside a packed block, in rows of 8-byte words
  int32_t elem4;          // 4-byte elements
  const int32_t* remap;   // null, or: an OWN source column s is read from column remap[s] (the parameter bank's index)
};
struct GatherParts {
  GatherPart p[3];
  int32_t n;
};
template <typename T>
__device__ __forceinline__ void gatherRows(const GatherPart& part, int row0, int nr, int64_t s, int64_t j, int64_t ownPitch,
                                           int64_t ncol, const double* __restrict__ recv, const RecvMap& map,
                                           int64_t dstPitch) {
  T v[kGatherRows];
  if (s < ncol) {
    const T* __restrict__ p = (const T*)part.own + (int64_t)row0 * ownPitch + (part.remap ? (int64_t)part.remap[s] : s);
    if (nr == kGatherRows) {
#pragma unroll
      for (int r = 0; r < kGatherRows; r++) v[r] = p[(int64_t)r * ownPitch];
    } else {
      for (int r = 0; r < nr; r++) v[r] = p[(int64_t)r * ownPitch];
    }
  } else {
    const int64_t kk = s - ncol;
    int blk = 0;
    for (int q = 1; q < map.nBlocks; q++)
      if (kk >= map.start[q]) blk = q;
    // (the part's first word inside the block, then rows of the part's own element type)
    const T* __restrict__ p = (const T*)(recv + map.off[blk] + (int64_t)part.recvRow0 * map.n[blk]) +
                              (int64_t)row0 * map.n[blk] + (kk - map.start[blk]);
    for (int r = 0; r < nr; r++) v[r] = p[(int64_t)r * map.n[blk]];
  }
  T* __restrict__ q = (T*)part.dst + (int64_t)row0 * dstPitch + j;
  if (nr == kGatherRows) {
#pragma unroll
    for (int r = 0; r < kGatherRows; r++) q[(int64_t)r * dstPitch] = v[r];
  } else {
    for (int r = 0; r < nr; r++) q[(int64_t)r * dstPitch] = v[r];
  }
}
__global__ __launch_bounds__(256) void gatherMemberKernel(GatherParts parts, int64_t ownPitch, int64_t ncol,
                                                          const double* __restrict__ recv, RecvMap map,
                                                          const int32_t* __restrict__ src, int64_t nOut,
                                                          int64_t dstPitch) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nOut) return;
  int k = 0;
  for (int q = 1; q < parts.n; q++)
    if ((int)blockIdx.y >= parts.p[q].group0) k = q;
  const GatherPart part = parts.p[k];
  const int row0 = ((int)blockIdx.y - part.group0) * kGatherRows;
  const int nr = part.rows - row0 < kGatherRows ? part.rows - row0 : kGatherRows;
  // (clamped: the index vector of an analysis whose launch was void -- pfFusedKernel's barrier gave up -- is whatever the
  // caller's buffer held; the results are void either way, the reads must stay inside the matrices)
  int64_t s = src[j];
  const int64_t sMax = ncol + (map.nBlocks > 0 ? map.start[map.nBlocks] : 0) - 1;
  s = s < 0 ? 0 : s > sMax ? sMax : s;
  if (part.elem4) gatherRows<float>(part, row0, nr, s, j, ownPitch, ncol, recv, map, dstPitch);
  else gatherRows<double>(part, row0, nr, s, j, ownPitch, ncol, recv, map, dstPitch);
}

// ---- a filter spread over ranks, without an all-to-all: every rank reads the ancestors it needs straight out
// of its peers' checkpoint matrices (peer-mapped HBM over xGMI; sipnet_batch_pf_publish / _connect) -------------
// What the ranks all-gather is one block per rank: [nmax log-weights (slots past the rank's own particles: -inf) |
// P = ceil(nmax / 256) block maxima of them], stride = nmax + P doubles.  Slot s * nmax + c = particle c of rank s.
constexpr int kMaxPeers = 16;
struct PeerPtrs {            // kernel argument: where rank s keeps its particles' checkpoint matrices
  int32_t world, nmax;
  const double* state[kMaxPeers];
  const void* ring[kMaxPeers];
  const void* third[kMaxPeers];   // the converted parameter rows [NPARAMS][pitch] -- or, with all ranks' parameters replicated
                                  // on every rank (sipnet_batch::d_prmBank), the particles' index into that bank [pitch] int32
  int32_t pitch[kMaxPeers];  // particles of rank s = the leading dimension of its matrices
  int32_t rank;                   // the reading rank
  unsigned long long* crossing;   // += particles read from another rank's matrices (null: not counted)
};

// dst[row][j] = matrix of rank (anc[j] / nmax)[row][anc[j] % nmax] for the three matrices of a checkpoint
struct PeerPart {
  void* dst;
  int32_t rows, group0, elem4;
};
struct PeerParts {
  PeerPart p[3];
  int32_t n;
};
template <typename T>
__device__ __forceinline__ void gatherPeerRows(const T* __restrict__ p, int64_t srcPitch, T* __restrict__ q,
                                               int64_t dstPitch, int nr) {
  T v[kGatherRows];
  if (nr == kGatherRows) {
#pragma unroll
    for (int r = 0; r < kGatherRows; r++) v[r] = p[(int64_t)r * srcPitch];
#pragma unroll
    for (int r = 0; r < kGatherRows; r++) q[(int64_t)r * dstPitch] = v[r];
  } else {
    for (int r = 0; r < nr; r++) v[r] = p[(int64_t)r * srcPitch];
    for (int r = 0; r < nr; r++) q[(int64_t)r * dstPitch] = v[r];
  }
}
__global__ __launch_bounds__(256) void gatherPeerKernel(PeerParts parts, PeerPtrs peers,
                                                        const int32_t* __restrict__ anc, int64_t nOut,
                                                        int64_t dstPitch) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nOut) return;
  int k = 0;
  for (int q = 1; q < parts.n; q++)
    if ((int)blockIdx.y >= parts.p[q].group0) k = q;
  const PeerPart part = parts.p[k];
  const int row0 = ((int)blockIdx.y - part.group0) * kGatherRows;
  const int nr = part.rows - row0 < kGatherRows ? part.rows - row0 : kGatherRows;
  int32_t a = anc[j];   // (clamped like gatherMemberKernel's: a void analysis leaves the caller's buffer as it was)
  a = a < 0 ? 0 : a;
  int s = a / peers.nmax;
  s = s >= peers.world ? peers.world - 1 : s;
  const int64_t pitch = peers.pitch[s];
  int64_t c = a - s * peers.nmax;
  c = c >= pitch ? pitch - 1 : c;
  const void* base = k == 0 ? (const void*)peers.state[s] : k == 1 ? peers.ring[s] : peers.third[s];
  if (blockIdx.y == 0 && peers.crossing) {   // how many of this rank's particles crossed a link (sipnet_batch_pf_info)
    const unsigned long long far = __ballot(s != peers.rank);
    if ((threadIdx.x & 63) == 0 && far) atomicAdd(peers.crossing, (unsigned long long)__popcll(far));
  }
  if (part.elem4)
    gatherPeerRows<float>((const float*)base + (int64_t)row0 * pitch + c, pitch, (float*)part.dst + (int64_t)row0 * dstPitch + j,
                          dstPitch, nr);
  else
    gatherPeerRows<double>((const double*)base + (int64_t)row0 * pitch + c, pitch,
                           (double*)part.dst + (int64_t)row0 * dstPitch + j, dstPitch, nr);
}

// 1 when any member needs the generic-exponent kernel variant (dVpdExp != 2 or
// soilRespMoistEffect != 1), see engine.hip set_params
__global__ __launch_bounds__(256) void exponentCheckKernel(const double* __restrict__ prm,
                                                           int64_t ncol, int32_t* __restrict__ flag) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  if (prm[(int64_t)SP_dVpdExp * ncol + c] != 2.0 ||
      prm[(int64_t)SP_soilRespMoistEffect * ncol + c] != 1.0)
    atomicOr(flag, 1);
}

__global__ __launch_bounds__(256) void iotaKernel(int32_t* p, int64_t n, int32_t first = 0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = first + (int32_t)i;
}
// rows of doubles from a peer's matrix (pitch srcPitch) into columns col0.. of the bank (sipnet_batch_pf_connect)
__global__ __launch_bounds__(256) void copyRowsKernel(double* __restrict__ dst, int64_t dstPitch, const double* __restrict__ src,
                                                      int64_t srcPitch, int64_t width, int32_t rows) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= width) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) dst[(int64_t)r * dstPitch + c] = src[(int64_t)r * srcPitch + c];
}

// ---- host: the one launch of gatherMemberKernel ---------------------------------------------------------------------
static inline int rowGroups(int rows) { return (rows + kGatherRows - 1) / kGatherRows; }   // blockIdx.y values a part takes
// What launchGatherMember moves: state + ring (+ parameters) of the columns src[0..nOut), one launch.  A caller sets the
// fields it uses; the rest stay null.
struct GatherCall {
  // sources [rows][ncol] -- ncol: their leading dimension AND the number of own source columns
  const double* state = nullptr;   // with ring; null: neither
  const void* ring = nullptr;
  bool ringF32 = false;            // the ring rows are floats, in the batch and in a packed block (SIPNET_RING_SLOTS / 2 rows of words)
  const double* prm = nullptr;     // null: no parameter rows
  int64_t ncol = 0;
  // destinations [rows][dstPitch]
  double* dState = nullptr;
  void* dRing = nullptr;
  double* dPrm = nullptr;
  int64_t dstPitch = 0;
  // source columns >= ncol: received packed blocks
  const double* recv = nullptr;
  RecvMap map{};
  // dst column j <- source column src[j], j < nOut
  const int32_t* src = nullptr;
  int64_t nOut = 0;
  const int32_t* prmRemap = nullptr;   // the batch's parameter index (null: parameters in column order): the parameter rows are read through it
  // resampling with an index instead of the parameter rows (then prm must be null): idNew[j] = idOld[src[j]]
  const int32_t* idOld = nullptr;
  int32_t* idNew = nullptr;
  hipStream_t stream = nullptr;
};
void launchGatherMember(const GatherCall& g) {
  if (g.nOut <= 0) return;
  GatherParts parts{};
  parts.n = 0;
  int total = 0;
  if (g.state) {
    parts.p[parts.n++] = GatherPart{g.state, g.dState, SIPNET_NSTATE, total, 0, 0, nullptr};
    total += rowGroups(SIPNET_NSTATE);
    parts.p[parts.n++] = GatherPart{g.ring, g.dRing, SIPNET_RING_SLOTS, total, SIPNET_NSTATE, g.ringF32 ? 1 : 0, nullptr};
    total += rowGroups(SIPNET_RING_SLOTS);
  }
  if (g.prm) {
    parts.p[parts.n++] = GatherPart{g.prm, g.dPrm, SIPNET_NPARAMS, total, SIPNET_NSTATE + ringWords(g.ringF32), 0, g.prmRemap};
    total += rowGroups(SIPNET_NPARAMS);
  } else if (g.idOld) {   // one row of 4-byte elements
    parts.p[parts.n++] = GatherPart{g.idOld, g.idNew, 1, total, 0, 1, nullptr};
    total += 1;
  }
  dim3 grid((unsigned)((g.nOut + 255) / 256), (unsigned)total);
  hipLaunchKernelGGL(gatherMemberKernel, grid, dim3(256), 0, g.stream, parts, g.ncol, g.ncol, g.recv, g.map, g.src, g.nOut, g.dstPitch);
}
