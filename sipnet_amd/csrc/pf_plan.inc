// pf_plan.inc -- the exchange plan of a resampling whose checkpoints travel in packed blocks (sipnet_pf_exchange_plan): who
// sends which columns to whom, from the global ancestor vector.

// ---- exchange plan of a resampling over `world` ranks with n particles each ----------------
// The global ancestor vector (identical on every rank, non-decreasing) is cut into destination
// blocks [d*n, (d+1)*n); inside a block the ancestors owned by source rank s (anc / n == s) are
// contiguous.  A particle that has to cross ranks (s != d) travels ONCE per destination: the
// first of a run of equal ancestors inside a destination block is its "head".
//   first[d][s]  first index of block d whose ancestor belongs to rank >= s   (binary search)
//   head[i]      1 when entry i is a cross-rank head                          (exclusive scan -> P)
//   count[d][s]  = P[first[d][s+1]] - P[first[d][s]]                          (columns d receives from s)
constexpr int kMaxWorld = 64;
__global__ void planFirstKernel(const int32_t* __restrict__ anc, int64_t n, int32_t world,
                                int64_t* __restrict__ first) {
  const int d = blockIdx.x, s = threadIdx.x;  // s in 0..world
  if (s > world) return;
  const int64_t target = (int64_t)s * n;      // first ancestor value owned by rank s
  int64_t lo = (int64_t)d * n, hi = lo + n;   // lower bound of `target` in anc[lo, hi)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)anc[mid] < target) lo = mid + 1; else hi = mid;
  }
  first[(int64_t)d * (world + 1) + s] = lo;
}
// (also validates the vector: every ancestor inside [0, total) and non-decreasing -- anything else
// (NaN weights upstream, a caller's bug) raises *bad and the plan's indices are never used)
__global__ __launch_bounds__(256) void planHeadKernel(const int32_t* __restrict__ anc, int64_t n,
                                                      int64_t total, int32_t* __restrict__ head,
                                                      int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t a = anc[i];
  if (a < 0 || a >= total || (i > 0 && anc[i - 1] > a)) {
    atomicOr(bad, 1);
    head[i] = 0;
    return;
  }
  const int64_t d = i / n, s = a / n;
  const bool newRun = (i % n == 0) || anc[i - 1] != a;
  head[i] = (newRun && s != d) ? 1 : 0;
}
// one block: counts, the bases of this rank's send / receive blocks (in rank order, self skipped)
__global__ void planCountKernel(const int64_t* __restrict__ first, const int32_t* __restrict__ P,
                                const int32_t* __restrict__ head, int64_t total, int32_t world,
                                int32_t rank, int64_t* __restrict__ counts /* [2][world]: send, recv */,
                                int64_t* __restrict__ bases /* [2][world] */) {
  if (threadIdx.x != 0) return;
  if (counts[2 * kMaxWorld * 2] != 0) {   // (the validity flag lives behind the counts and bases)
    for (int q = 0; q < 2 * world; q++) counts[q] = 0, bases[q] = 0;
    return;
  }
  auto Pat = [&](int64_t i) -> int64_t { return i < total ? (int64_t)P[i] : (int64_t)P[total - 1] + head[total - 1]; };
  int64_t sb = 0, rb = 0;
  for (int q = 0; q < world; q++) {
    const int64_t* fs = first + (int64_t)q * (world + 1);       // destination q, what I (rank) send it
    const int64_t send = q == rank ? 0 : Pat(fs[rank + 1]) - Pat(fs[rank]);
    const int64_t* fr = first + (int64_t)rank * (world + 1);    // my block, what comes from source q
    const int64_t recv = q == rank ? 0 : Pat(fr[q + 1]) - Pat(fr[q]);
    counts[q] = send;
    counts[world + q] = recv;
    bases[q] = sb;
    bases[world + q] = rb;
    sb += send;
    rb += recv;
  }
}
__global__ __launch_bounds__(256) void planFillKernel(const int32_t* __restrict__ anc, int64_t n,
                                                      int64_t total, int32_t world, int32_t rank,
                                                      const int64_t* __restrict__ first,
                                                      const int32_t* __restrict__ P,
                                                      const int32_t* __restrict__ head,
                                                      const int64_t* __restrict__ bases,
                                                      int32_t* __restrict__ sendCols,
                                                      int32_t* __restrict__ src, const int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (*bad) return;
  const int64_t a = anc[i];
  const int64_t d = i / n, s = a / n, lo = (int64_t)rank * n;
  if (s == rank && d != rank && head[i]) {   // a column of mine that rank d needs (once)
    const int64_t f = first[d * (world + 1) + rank];
    sendCols[bases[d] + ((int64_t)P[i] - (int64_t)P[f])] = (int32_t)(a - lo);
  }
  if (d == rank) {                           // where my new column j comes from
    const int64_t j = i - lo;
    if (s == rank) {
      src[j] = (int32_t)(a - lo);
    } else {
      const int64_t f = first[(int64_t)rank * (world + 1) + s];
      const int64_t k = ((int64_t)P[i] + head[i] - 1) - (int64_t)P[f];   // index among the heads from s
      src[j] = (int32_t)(n + bases[world + s] + k);
    }
  }
}
