// node_pf.h -- part of node.cpp: the particle filter over the node's shards (BASELINE config C5; SURVEY 8(e) "PF extra
// exchange").  ONE all-gather of the log-weight blocks per cycle, after which every shard reads the ancestors it needs
// straight out of its peers' HBM (pf.hip: sipnet_batch_pf_resample_peers).
#pragma once

extern "C" {

int sipnet_node_pf_connect(sipnet_node* nd, int32_t with_params) {
  if (!nd || nd->mode != SIPNET_SHARD_MEMBERS || nd->n_sites != 1 || nd->n() > 16) {
    setError("sipnet_node_pf_connect: a filter needs ONE site, its particles sharded as members over at most 16 devices");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  const int n = nd->n();
  std::vector<sipnet_pf_peer> peers(n);
  RC_TRY(onEveryShard(nd, [&](int k) -> int { return sipnet_batch_pf_publish(nd->shards[k].batch, with_params, &peers[k]); }));
  RC_TRY(onEveryShard(nd, [&](int k) -> int {
    Shard& sh = nd->shards[k];
    RC_TRY(sipnet_batch_pf_connect(sh.batch, n, k, peers.data()));
    NODE_HIP(hipStreamSynchronize(sh.stream));
    const int64_t L = sipnet_batch_pf_block_len(sh.batch);
    NODE_BUF(sh.pfGathered.reserve((size_t)n * L));
    NODE_BUF(sh.pfAnc.reserve((size_t)sh.count));
    NODE_BUF(sh.pfTotals.reserve(sipnet_node::kPfTotals));
    NODE_HIP(hipMemset(sh.pfTotals, 0xff, sipnet_node::kPfTotals * sizeof(int64_t)));   // -1: "no cycle wrote this slot"
    return SIPNET_OK;
  }));
  nd->pfBlock = sipnet_batch_pf_block_len(nd->shards[0].batch);
  nd->pfConnected = true;
  nd->pfCycles = 0;
  return SIPNET_OK;
}

int sipnet_node_pf_arm(sipnet_node* nd, double obs, double sigma) {
  if (!nd || !nd->pfConnected || !(sigma > 0)) {
    setError("sipnet_node_pf_arm: needs sipnet_node_pf_connect and sigma > 0");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  // (host-only: every shard's next forecast launch is told where its log-weight block lies -- its slice of the all-gather's
  // buffer -- and what it will be weighed against)
  for (int k = 0; k < nd->n(); k++)
    RC_TRY(sipnet_batch_pf_arm(nd->shards[k].batch, obs, sigma, nd->shards[k].pfGathered + (size_t)k * nd->pfBlock));
  return SIPNET_OK;
}

int sipnet_node_pf_analysis(sipnet_node* nd, int32_t variable, double obs, double sigma, double u0) {
  if (!nd || !nd->pfConnected || nd->last.nRun <= 0 || variable < 0 || variable > 2) {
    setError("sipnet_node_pf_analysis: needs sipnet_node_pf_connect and a forecast (sipnet_node_forecast / _run)");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if (nd->last.segmented) {   // the planes lie segment by segment ([3][len_j][ld] each): a plane is not one [n_run][ld] block
    setError("sipnet_node_pf_analysis: the last run was sipnet_node_run_gathering (segmented planes); forecast with "
             "sipnet_node_forecast / sipnet_node_run");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  const int slot = nd->pfCycles % sipnet_node::kPfTotals;
  const int32_t nRun = nd->last.nRun;
  RC_TRY(onEveryShard(nd, [&](int k) -> int {
    Shard& sh = nd->shards[k];
    const char* plane = (const char*)sh.planes.get() + (size_t)variable * nRun * nd->ld * nd->elem();
    double* mine = sh.pfGathered + (size_t)k * nd->pfBlock;
    RC_TRY(sipnet_batch_pf_local_weights(sh.batch, plane, nd->precision == SIPNET_F32_MIXED, nRun, nd->ld, obs, sigma, mine, sh.stream));
    RC_TRY(allGatherShard(nd, k, mine, sh.pfGathered, (size_t)nd->pfBlock * sizeof(double)));   // in place
    return sipnet_batch_pf_resample_peers(sh.batch, sh.pfGathered, u0, sh.pfAnc, sh.pfTotals + slot, sh.stream);
  }));
  nd->pfCycles++;
  return SIPNET_OK;
}

int sipnet_node_pf_check(sipnet_node* nd, int32_t* n_cycles_checked) {
  if (!nd || !nd->pfConnected) return SIPNET_ERR_BAD_ARGUMENT;
  const int m = std::min<int>(nd->pfCycles, sipnet_node::kPfTotals);
  std::vector<int64_t> t0(sipnet_node::kPfTotals), tk(sipnet_node::kPfTotals);
  for (int k = 0; k < nd->n(); k++) {
    const Shard& sh = nd->shards[k];
    NODE_HIP(hipSetDevice(sh.device));
    NODE_HIP(hipStreamSynchronize(sh.stream));
    NODE_HIP(hipMemcpy(tk.data(), sh.pfTotals, tk.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (k == 0) t0 = tk;
    for (int c = 0; c < m; c++) {
      if (tk[c] == SIPNET_PF_VOID_TOTAL) {
        setError("sipnet_node_pf_check: a cycle's analysis kernel gave up at its grid barrier on shard " + std::to_string(k) +
                 " (its workgroups were not all resident: something else held device " + std::to_string(sh.device) +
                 "); that cycle's resampling is void");
        return SIPNET_ERR_INTERNAL;
      }
      if (tk[c] != t0[c]) {
        setError("sipnet_node_pf_check: the shards disagree on a cycle's total weight (the gathered blocks differ)");
        return SIPNET_ERR_INTERNAL;
      }
      if (tk[c] <= 0) {
        setError("sipnet_node_pf_check: a cycle ended with every particle at zero weight");
        return SIPNET_ERR_BAD_PARAMETER;
      }
    }
  }
  if (n_cycles_checked) *n_cycles_checked = m;
  nd->pfCycles = 0;
  return SIPNET_OK;
}

int32_t* sipnet_node_pf_ancestors(sipnet_node* nd, int32_t k) { const Shard* sh = shardOf(nd, k); return sh ? sh->pfAnc.get() : nullptr; }
int64_t sipnet_node_pf_block_len(const sipnet_node* nd) { return nd ? nd->pfBlock : 0; }

}  // extern "C"
