// node_gather.h -- part of node.cpp (after struct sipnet_node): a task on every shard, and the all-gathers among the shards.
#pragma once

// f(k) for every shard k, each on the shard's own host thread (a node of one shard: on the caller's);
// returns when all have returned, the first failure wins
template <class F>
static int onEveryShard(sipnet_node* nd, F f) {
  const int bad = nd->pool.run(f);
  if (bad < 0) return SIPNET_OK;
  setError("device " + std::to_string(nd->shards[bad].device) + " (shard " + std::to_string(bad) + "): " + nd->pool.msg[bad]);
  return nd->pool.rc[bad];
}

// f(shard) for every shard in shard order on the caller's thread, the first failure wins
template <class F>
static int inShardOrder(sipnet_node* nd, F f) {
  for (Shard& sh : nd->shards) RC_TRY(f(sh));
  return SIPNET_OK;
}

// the shards' host threads meet (shard_pool.h: HostBarrier); a shard whose task has failed breaks the meeting
static int meet(sipnet_node* nd) {
  if (nd->pool.bar.arrive()) return SIPNET_OK;
  setError("sipnet_node: another shard failed");
  return SIPNET_ERR_INTERNAL;
}

// All-gather of `bytes` per shard among the shards, called by shard k's thread from inside an onEveryShard
// task: recv = [n][bytes] on shard k's device, send = this shard's block (may be its own slice of recv).
// RCCL when every shard has a device of its own; otherwise copies ordered by events (see node.cpp's header).
static int allGatherShard(sipnet_node* nd, int k, const void* send, void* recv, size_t bytes, hipStream_t stream = nullptr) {
  Shard& me = nd->shards[k];
  if (!stream) stream = me.stream;
  if (nd->rccl) {
    // A collective nobody may be missing from: a shard whose task has failed (its launch, an upload) returns WITHOUT
    // enqueuing its part, and the others' ncclAllGather would then never complete -- the next synchronisation of their
    // streams would hang instead of reporting the error.  So the shards' host threads first agree that all of them
    // have come this far (the host barrier; a failed shard breaks it): either everybody enqueues or nobody does.
    RC_TRY(meet(nd));
    NODE_RCCL(nd->rccl, nd->rccl->allGather(send, recv, bytes, ncclChar, me.comm, stream));
    return SIPNET_OK;
  }
  me.agSend = send;
  NODE_HIP(hipEventRecord(me.evReady, stream));
  RC_TRY(meet(nd));
  for (int s = 0; s < nd->n(); s++) {
    const Shard& sh = nd->shards[s];
    char* dst = (char*)recv + (size_t)s * bytes;
    if (s != k) NODE_HIP(hipStreamWaitEvent(stream, sh.evReady, 0));
    if ((const void*)dst != sh.agSend) NODE_HIP(hipMemcpyAsync(dst, sh.agSend, bytes, hipMemcpyDeviceToDevice, stream));
  }
  NODE_HIP(hipEventRecord(me.evCopied, stream));
  RC_TRY(meet(nd));
  // what follows on this stream may overwrite the block the others copy from
  for (const Shard& sh : nd->shards)
    if (&sh != &me) NODE_HIP(hipStreamWaitEvent(stream, sh.evCopied, 0));
  return SIPNET_OK;
}

// ONE all-gather of a whole block of the last run, `count` elements of elemBytes per shard: recv(shard) is the shard's
// gathered buffer -- grown here to n blocks, its stream idle first -- and send(shard) its own block.  RCCL: one thread,
// the per-device calls of the collective fused (its single-process idiom); else the event-ordered copies.
template <class Send, class Recv>
static int gatherWhole(sipnet_node* nd, Send send, Recv recv, size_t count, ncclDataType_t type, size_t elemBytes) {
  const size_t n = nd->shards.size();
  RC_TRY(inShardOrder(nd, [&](Shard& sh) -> int {
    auto& buf = recv(sh);
    const size_t want = count * n * elemBytes / sizeof(*buf.get());
    if (want <= buf.capacity()) return SIPNET_OK;
    NODE_HIP(hipSetDevice(sh.device));
    NODE_HIP(hipStreamSynchronize(sh.stream));
    NODE_BUF(buf.reserve(want));
    return SIPNET_OK;
  }));
  if (!nd->rccl)
    return onEveryShard(nd, [&](int k) -> int {
      Shard& sh = nd->shards[k];
      return allGatherShard(nd, k, send(sh), recv(sh).get(), count * elemBytes);
    });
  NODE_RCCL(nd->rccl, nd->rccl->groupStart());
  RC_TRY(inShardOrder(nd, [&](Shard& sh) -> int {
    NODE_HIP(hipSetDevice(sh.device));
    NODE_RCCL(nd->rccl, nd->rccl->allGather(send(sh), recv(sh).get(), count, type, sh.comm, sh.stream));
    return SIPNET_OK;
  }));
  NODE_RCCL(nd->rccl, nd->rccl->groupEnd());
  return SIPNET_OK;
}
