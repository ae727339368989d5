// node_shard.h -- part of node.cpp: one shard of a node -- its device, its ranges, its batch, streams, events, communicator
// rank and device blocks -- opened by one call and released by one.
#pragma once

namespace {

// a shard's blocks, together so that they go together, with the shard's device current (Shard::close)
struct ShardBlocks {
  // planes [3][n_run][ld] (element type by precision), statistics [3][n_run][maxSites][2], gathered statistics
  // [n][3][n_run][maxSites][2], gathered planes [n][3][n_run][ld] (on request); every block has its own capacity
  DevBuf<unsigned char> planes, gatheredPlanes;   // bytes: the element type goes by the precision
  DevBuf<double> stats, gatheredStats, statsCompact;
  // particle filter: the gathered log-weight blocks, this shard's particles' ancestors, a ring of total weights
  DevBuf<double> pfGathered;
  DevBuf<int32_t> pfAnc;
  DevBuf<int64_t> pfTotals;
  DevBuf<unsigned char> reduced, gatheredReduced;   // bytes (sipnet_node_run_gathering_reduced)
};

struct Shard : ShardBlocks {
  int32_t device = 0;
  // members [first, first + count) of every site (member mode: sites0 = 0, nSites = n_sites)
  // or sites [sites0, sites0 + nSites) with all members (site mode: first = 0, count = n_members)
  int32_t first = 0, count = 0, sites0 = 0, nSites = 0;
  sipnet_batch* batch = nullptr;
  hipStream_t stream = nullptr, gatherStream = nullptr;   // the all-gathers of a gathering run are on the second
  hipEvent_t evSeg = nullptr, evGathered = nullptr;       // a segment is ready for / the gathers are through on the second stream
  hipEvent_t evReady = nullptr, evCopied = nullptr;       // event-ordered transport
  const void* agSend = nullptr;                           // event-ordered transport: the block the others copy from
  ncclComm_t comm = nullptr;                              // null: event-ordered copies (a device is listed twice)

  Shard() = default;
  Shard(const Shard&) = delete;
  Shard& operator=(const Shard&) = delete;

  bool hasSite(int32_t site) const { return site >= sites0 && site < sites0 + nSites; }

  // batch, streams and events on `device`; `sameDevice` shards share it.  fn: the entry point, for the error text
  int open(const int32_t* flags, int32_t precision, int32_t sameDevice, const char* fn) {
    RC_TRY(sipnet_batch_create(flags, nSites, count, precision, device, &batch));
    // shards that share a device analyse at the same time: each may keep 1 / (their number) of it spinning (pf.hip fusedBudget)
    RC_TRY(sipnet_batch_set_device_share(batch, sameDevice));
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&evReady, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&evCopied, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&gatherStream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&evSeg, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&evGathered, hipEventDisableTiming) != hipSuccess) {
      setError(std::string(fn) + ": hipStreamCreate / hipEventCreate failed");
      return SIPNET_ERR_NO_DEVICE;
    }
    return SIPNET_OK;
  }

  // both streams idle (whatever of them exists)
  void sync() const {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (gatherStream) (void)hipStreamSynchronize(gatherStream);
  }

  // everything the shard holds, given back with its device current; whatever open() did not reach is skipped, and a
  // second call finds nothing left
  void close(Rccl* rccl) {
    (void)hipSetDevice(device);
    if (comm) rccl->commDestroy(comm);
    comm = nullptr;
    static_cast<ShardBlocks&>(*this) = ShardBlocks();
    for (hipEvent_t* ev : {&evReady, &evCopied, &evSeg, &evGathered}) {
      if (*ev) (void)hipEventDestroy(*ev);
      *ev = nullptr;
    }
    if (gatherStream) (void)hipStreamDestroy(gatherStream);
    if (batch) sipnet_batch_destroy(batch);
    if (stream) (void)hipStreamDestroy(stream);
    gatherStream = stream = nullptr;
    batch = nullptr;
  }
};

}  // namespace
