// node_run.h -- part of node.cpp: the run paths.  runShards: every shard's launch into the common [n_steps] layout
// (sipnet_node_run / _forecast).  runGathering: the run in segments, each gathered on the shards' second streams under the
// next one's kernel (sipnet_node_run_gathering / _reduced).
#pragma once

using LastRun = sipnet_node::LastRun;

// a shard's planes and statistics block for runs of up to n_steps records (called on the shard's thread)
static int growRunBuffers(sipnet_node* nd, Shard& sh, int32_t n_steps) {
  const size_t planeBytes = (size_t)3 * n_steps * nd->ld * nd->elem();
  const size_t statDoubles = (size_t)3 * n_steps * nd->maxSites * 2;
  NODE_HIP(hipStreamSynchronize(sh.stream));
  NODE_BUF(sh.planes.reserve(planeBytes));
  NODE_BUF(sh.stats.reserve(statDoubles));
  // columns past a shard's own (the padding up to the common leading dimension) and the statistics of
  // sites it does not have stay zero: no kernel ever writes them, whatever the length of a run
  NODE_HIP(hipMemsetAsync(sh.planes, 0, planeBytes, sh.stream));
  NODE_HIP(hipMemsetAsync(sh.stats, 0, statDoubles * sizeof(double), sh.stream));
  return SIPNET_OK;
}

// does a site of the shard end before record `upTo`?  Then the kernels leave rows of the shard's planes unwritten, and
// what stands there depends on the layout of the run before (plain or segmented): such a shard's planes are cleared
// at the start of every run
static bool shardEndsEarly(const Shard& sh, int32_t upTo) {
  for (int32_t s = 0; s < sh.nSites; s++)
    if (sipnet_batch_site_nsteps(sh.batch, s) < upTo) return true;
  return false;
}

// a shard with fewer sites than the largest, or a shorter run: its block [3][nLoc][nSites][2] was produced compactly and
// is spread out to the common shape [3][n_steps][maxSites][2] (everything else stays zero)
static int spreadStats(sipnet_node* nd, Shard& sh, int32_t n_steps, int32_t nLoc) {
  const size_t row = (size_t)sh.nSites * 2 * sizeof(double), commonRow = (size_t)nd->maxSites * 2 * sizeof(double);
  if (nLoc != n_steps) NODE_HIP(hipMemsetAsync(sh.stats, 0, (size_t)3 * n_steps * commonRow, sh.stream));
  for (int v = 0; v < 3; v++)
    NODE_HIP(hipMemcpy2DAsync(sh.stats + (size_t)v * n_steps * nd->maxSites * 2, commonRow, sh.statsCompact + (size_t)v * nLoc * sh.nSites * 2,
                              row, row, (size_t)nLoc, hipMemcpyDeviceToDevice, sh.stream));
  return SIPNET_OK;
}

// one shard's part of runShards (on the shard's thread)
static int runShard(sipnet_node* nd, Shard& sh, int32_t step0, int32_t n_steps, bool withStats, bool grow) {
  if (grow) RC_TRY(growRunBuffers(nd, sh, n_steps));
  char* p = (char*)sh.planes.get();
  const size_t one = (size_t)n_steps * nd->ld * nd->elem();
  if (!grow && shardEndsEarly(sh, step0 + n_steps)) NODE_HIP(hipMemsetAsync(p, 0, 3 * one, sh.stream));
  // (site shards may hold forcings of different lengths: a shard runs to the end of ITS longest site; the rows
  // past it stay what they are -- zero -- in the common [n_steps] layout)
  const int32_t have = sipnet_batch_nsteps(sh.batch);
  const int32_t nLoc = step0 + n_steps <= have ? n_steps : have - step0;
  if (nLoc <= 0) return SIPNET_OK;
  if (!withStats) return sipnet_batch_run(sh.batch, step0, nLoc, p, p + one, p + 2 * one, nullptr, nd->ld, sh.stream);
  if (sh.nSites == nd->maxSites && nLoc == n_steps)
    return sipnet_batch_run_stats(sh.batch, step0, n_steps, p, p + one, p + 2 * one, nd->ld, sh.stats, sh.stream);
  const size_t compactDoubles = (size_t)3 * nLoc * sh.nSites * 2;
  if (compactDoubles > sh.statsCompact.capacity()) {
    NODE_HIP(hipStreamSynchronize(sh.stream));
    NODE_BUF(sh.statsCompact.reserve(compactDoubles));
  }
  RC_TRY(sipnet_batch_run_stats(sh.batch, step0, nLoc, p, p + one, p + 2 * one, nd->ld, sh.statsCompact, sh.stream));
  return spreadStats(nd, sh, n_steps, nLoc);
}

static int runShards(sipnet_node* nd, int32_t step0, int32_t n_steps, bool withStats) {
  if (!nd || n_steps <= 0) {
    setError("sipnet_node_run: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  const bool grow = n_steps > nd->nAlloc;
  RC_TRY(onEveryShard(nd, [&](int k) -> int { return runShard(nd, nd->shards[k], step0, n_steps, withStats, grow); }));
  if (grow) nd->nAlloc = n_steps;
  nd->last = LastRun();
  nd->last.nRun = n_steps;
  nd->last.step0 = step0;
  return SIPNET_OK;
}

// The north star's exchange as written, overlapped (SURVEY 8(e) "Collective": "gather per chunk ... overlapped on a
// side stream"): the run is cut into segments -- one launch each -- and the member-resolved planes of segment j
// travel (one all-gather per segment, on every shard's SECOND stream) under the step kernel of segment j + 1.
// Every segment has its own place in the shard's planes and in the gathered block, so nothing is double-buffered
// and nothing waits for a consumer (288 GB of HBM: the gathered year of c4's shape is 8 x 13.8 GB).
// ---- member-resolved outputs that fit under the kernel (round 6) ------------------------------------------------------
// The raw fp64 planes of a year are 4.3 GB per rank at 10 240 members: ~100 ms of xGMI time against 8 ms of compute.  What a
// consumer of the reference's per-step output (sipnet.c:453-473) aggregates anyway travels instead: the same planes as floats
// (half the bytes), or every member's sums over groups of sum_steps steps (daily sums of a half-hourly year: 1 / 48 of the
// bytes, 90 MB per rank) -- produced from segment j's planes on the shard's SECOND stream while segment j + 1 computes (the
// step kernel of such a shape leaves compute units idle and uses a few per cent of the HBM bandwidth), then all-gathered there.

// form: 0 the planes themselves (sipnet_node_run_gathering), SIPNET_GATHER_F32, SIPNET_GATHER_SUMS (sumSteps steps per group);
// any other form was refused by sipnet_node_run_gathering_reduced
static int checkGathering(const sipnet_node* nd, int32_t step0, int32_t n_steps, int32_t n_segments, int32_t form, int32_t sumSteps) {
  if (!nd || n_steps <= 0 || n_segments <= 0 || n_segments > n_steps || step0 < 0) {
    setError("sipnet_node_run_gathering: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if (form == SIPNET_GATHER_F32 && nd->precision != SIPNET_F64) {
    setError("sipnet_node_run_gathering_reduced: the planes of an fp32-mixed node are floats already (sipnet_node_run_gathering)");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if (form == SIPNET_GATHER_SUMS && (sumSteps <= 0 || n_segments > (n_steps + sumSteps - 1) / sumSteps)) {
    setError("sipnet_node_run_gathering_reduced: sum_steps > 0 and at most one segment per group of steps");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  return SIPNET_OK;
}

// the blocks of a gathering run, the shard's streams idle before a block is replaced (on the shard's thread)
static int reserveGathering(sipnet_node* nd, Shard& sh, const LastRun& run, bool grow) {
  const size_t n = nd->shards.size();
  const size_t redBytes = run.form ? (size_t)3 * run.redCuts.back() * nd->ld * run.redElem() : 0;
  const size_t planeBytes = (size_t)3 * run.nRun * nd->ld * nd->elem();
  if (redBytes > sh.reduced.capacity() || redBytes * n > sh.gatheredReduced.capacity()) {
    NODE_HIP(hipStreamSynchronize(sh.stream));
    NODE_HIP(hipStreamSynchronize(sh.gatherStream));
    NODE_BUF(sh.reduced.reserve(redBytes));
    NODE_BUF(sh.gatheredReduced.reserve(redBytes * n));
  }
  if (grow) {
    NODE_HIP(hipStreamSynchronize(sh.gatherStream));
    RC_TRY(growRunBuffers(nd, sh, run.nRun));
  }
  if (!run.form && planeBytes * n > sh.gatheredPlanes.capacity()) {
    NODE_HIP(hipStreamSynchronize(sh.stream));
    NODE_HIP(hipStreamSynchronize(sh.gatherStream));
    NODE_BUF(sh.gatheredPlanes.reserve(planeBytes * n));
  }
  return SIPNET_OK;
}

// segment j of a gathering run as one shard sees it
struct Segment {
  int32_t first, len;   // its records: [first, first + len)
  int32_t nLoc;         // of which the shard's forcings have this many (a site shard whose sites end early: fewer, or <= 0)
  size_t planeOff;      // bytes: the segment [3][len][ld] in the shard's planes; n times that in the gathered planes
  int32_t rows;         // the segment [3][rows][ld] in the reduced block ...
  size_t redOff;        // ... at this many bytes; n times that in the gathered one
};
static Segment segmentOf(const sipnet_node* nd, const LastRun& run, int j, int32_t have) {
  Segment s;
  s.first = run.step0 + run.cuts[j];
  s.len = run.cuts[j + 1] - run.cuts[j];
  s.nLoc = s.first + s.len <= have ? s.len : have - s.first;
  s.planeOff = (size_t)3 * run.cuts[j] * nd->ld * nd->elem();
  s.rows = run.redCuts[j + 1] - run.redCuts[j];
  s.redOff = (size_t)3 * run.redCuts[j] * nd->ld * run.redElem();
  return s;
}

// what a segment's all-gather sends, and where shard k's device receives everybody's
struct Block {
  const void* send;
  void* recv;
  size_t bytes;
};

// producer 1: the segment's step kernel writes its planes; they travel themselves, or reducedFromPlanes takes them
// (a site shard whose forcings end inside the segment: the rows past its end travel as zeros)
static int planesInLaunch(sipnet_node* nd, Shard& sh, const LastRun& run, const Segment& seg, Block* blk) {
  char* p = (char*)sh.planes.get() + seg.planeOff;
  const size_t one = (size_t)seg.len * nd->ld * nd->elem();   // one variable of the segment
  if (seg.nLoc > 0)   // (a failure is told to the barrier: the other shards give up at their next arrival)
    RC_TRY(sipnet_batch_run(sh.batch, seg.first, seg.nLoc, p, p + one, p + 2 * one, nullptr, nd->ld, sh.stream));
  *blk = {p, run.form ? nullptr : (char*)sh.gatheredPlanes.get() + nd->shards.size() * seg.planeOff, 3 * one};
  return SIPNET_OK;
}

// producer 2: the sums come out of the step kernel's own launch (sipnet_batch_run_sums: no planes are written at all)
static int sumsInLaunch(sipnet_node* nd, Shard& sh, const LastRun& run, const Segment& seg, Block* blk) {
  const size_t oneRed = (size_t)seg.rows * nd->ld;
  double* r = (double*)((char*)sh.reduced.get() + seg.redOff);
  if (seg.nLoc < seg.len) NODE_HIP(hipMemsetAsync(r, 0, 3 * oneRed * sizeof(double), sh.stream));   // (groups past a shard's last record: zero)
  if (seg.nLoc > 0)
    RC_TRY(sipnet_batch_run_sums(sh.batch, seg.first, seg.nLoc, run.sumSteps, r, r + oneRed, r + 2 * oneRed, nd->ld, sh.stream));
  *blk = {r, (char*)sh.gatheredReduced.get() + nd->shards.size() * seg.redOff, 3 * oneRed * sizeof(double)};
  return SIPNET_OK;
}

// producer 3: the segment's reduced block [3][rows][ld], made from its planes (*blk) on the second stream
static int reducedFromPlanes(sipnet_node* nd, Shard& sh, const LastRun& run, const Segment& seg, Block* blk) {
  char* r = (char*)sh.reduced.get() + seg.redOff;
  RC_TRY(launchReduce(run.form, nd->precision == SIPNET_F64, blk->send, seg.len, nd->ld, run.sumSteps, seg.rows, r, sh.gatherStream));
  *blk = {r, (char*)sh.gatheredReduced.get() + nd->shards.size() * seg.redOff, (size_t)3 * seg.rows * nd->ld * run.redElem()};
  return SIPNET_OK;
}

// shard k's host thread walks the segments on its own: launch, hand over to the second stream, all-gather there
// (RCCL: one communicator per thread, the multi-thread idiom; shards sharing a device: event-ordered copies, the
// threads meeting at a host barrier per segment)
static int gatherSegments(sipnet_node* nd, int k, const LastRun& run, bool grow) {
  Shard& sh = nd->shards[k];
  const int32_t have = sipnet_batch_nsteps(sh.batch);
  if (!grow && shardEndsEarly(sh, run.step0 + run.nRun))
    NODE_HIP(hipMemsetAsync(sh.planes, 0, (size_t)3 * run.nRun * nd->ld * nd->elem(), sh.stream));
  for (int j = 0; j + 1 < (int)run.cuts.size(); j++) {
    const Segment seg = segmentOf(nd, run, j, have);
    Block blk;
    RC_TRY(run.inKernel ? sumsInLaunch(nd, sh, run, seg, &blk) : planesInLaunch(nd, sh, run, seg, &blk));
    // the second stream takes over: what it does from here on comes after the segment's launch
    NODE_HIP(hipEventRecord(sh.evSeg, sh.stream));
    NODE_HIP(hipStreamWaitEvent(sh.gatherStream, sh.evSeg, 0));
    if (run.form && !run.inKernel) RC_TRY(reducedFromPlanes(nd, sh, run, seg, &blk));
    RC_TRY(allGatherShard(nd, k, blk.send, blk.recv, blk.bytes, sh.gatherStream));
  }
  return SIPNET_OK;
}

static int runGathering(sipnet_node* nd, int32_t step0, int32_t n_steps, int32_t n_segments, int32_t form = 0, int32_t sumSteps = 0) {
  RC_TRY(checkGathering(nd, step0, n_steps, n_segments, form, sumSteps));
  LastRun run;   // what this run leaves, if it succeeds
  run.nRun = n_steps;
  run.step0 = step0;
  run.segmented = true;
  run.form = form;
  run.sumSteps = sumSteps;
  sipnet::segmentCuts(step0, n_steps, n_segments, form, sumSteps, &run.cuts, &run.redCuts);
  // sums: inside the step kernel's own launch where every shard's batch has such a kernel, else the planes summed by a
  // pass on the second stream
  run.inKernel = form == SIPNET_GATHER_SUMS;
  for (const Shard& sh : nd->shards) run.inKernel = run.inKernel && sipnet_batch_sums_in_kernel(sh.batch) != 0;
  const bool grow = n_steps > nd->nAlloc;
  RC_TRY(onEveryShard(nd, [&](int k) -> int { return reserveGathering(nd, nd->shards[k], run, grow); }));
  if (grow) nd->nAlloc = n_steps;
  RC_TRY(onEveryShard(nd, [&](int k) -> int { return gatherSegments(nd, k, run, grow); }));
  // whatever follows on a shard's stream (the next run writes the same planes) comes after its gathers
  RC_TRY(inShardOrder(nd, [](Shard& sh) -> int {
    NODE_HIP(hipSetDevice(sh.device));
    NODE_HIP(hipEventRecord(sh.evGathered, sh.gatherStream));
    NODE_HIP(hipStreamWaitEvent(sh.stream, sh.evGathered, 0));
    return SIPNET_OK;
  }));
  nd->last = std::move(run);
  return SIPNET_OK;
}
