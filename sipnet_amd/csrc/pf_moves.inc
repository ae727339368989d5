// pf_moves.inc -- the host side of the three particle moves, included by pf.hip behind its own host code (PfScratch, scratchOf
// and sitesGeometry are pf.hip's): the rejuvenation (pf_rejuvenate.inc), the Metropolis move over members (pf_metropolis.inc),
// the tempering exponent of every site (pf_temper.inc), and the host forms of the draw (pf_random.inc).  What the moves of
// parameter rows share comes first: the listed rows' check, the batch's refusals, the batch's arrays bound, the path and its
// grids, the tail of a call.  Every scratch block is carved by site_host.h's carveScratch from one description of its layout.

// the listed rows checked by the joint analysis's rules, its refusal under this entry point's name; the bounds converted
static int listedRowsCheck(const char* who, int32_t n, const sipnet_enkf_param* params, double* lo, double* hi) {
  if (sipnet_enkf_params_check(n, params, lo, hi) == SIPNET_OK) return SIPNET_OK;
  const std::string why = sipnet_last_error(), from = "sipnet_enkf_params_check: ";
  return refuse(who, why.compare(0, from.size(), from) == 0 ? why.substr(from.size()) : why);
}
// a batch whose members' rows a move may write, or the refusal
static int movableBatch(const char* who, const sipnet_batch* b) {
  if (!b) return refuse(who, "a NULL batch");
  if (tooManyColumns(b)) return refuse(who, "at most 4194304 columns");
  if (b->planDirty) return refuse(who, "needs a batch that was set up (sipnet_batch_setup): the members' status is read");
  if (b->pfPeers) return refuse(who, "this batch is connected to a filter across ranks (sipnet_batch_pf_connect)");
  return SIPNET_OK;
}
// the listed rows and the batch's shape into a move's arguments (the bounds are there: listedRowsCheck)
template <class A>
static void moveShape(A& a, const sipnet_batch* b, int32_t n_params, const sipnet_enkf_param* params) {
  a.nPrm = n_params;
  a.rows = derivedRowsOf(n_params, params, a.prmRow);
  a.ncol = b->ncol;
  a.M = b->n_members;
  a.nCh = (int32_t)((b->n_members + 255) / 256);
}
// the move is about to write the batch (beginWrite; ownRows: every column its own rows, the move writes them), and its kernels
// address the batch's arrays as they are then
template <class A>
static int moveBegin(sipnet_batch* b, hipStream_t stream, bool ownRows, A& a) {
  RC_TRY(beginWrite(b, stream, ownRows));
  a.state = b->d_state;
  a.prm = b->d_prm;
  a.siteStatus = b->d_siteStatus;
  return SIPNET_OK;
}
// one workgroup per site when the sites are one chunk each, else the per-chunk launches (pf_rejuvenate.inc says why)
struct MoveGrids {
  bool split;
  dim3 sites, chunks;
  MoveGrids(const sipnet_batch* b, int32_t nCh)
      : split(nCh > 1 || (b->kernelOptions & SIPNET_KOPT_PF_MULTI_LAUNCH)), sites((unsigned)b->n_sites), chunks((unsigned)b->n_sites, (unsigned)nCh) {}
};
// the tail of a move: the launches' error, what sipnet_batch_pf_info reports, the batch busy on the stream
static int moveLaunched(sipnet_batch* b, hipStream_t stream, bool fused) {
  HIP_TRY(hipGetLastError());
  reportPath(b, fused, fused ? (int32_t)b->n_sites : 0);
  return markBusy(b, stream);
}

// ---- rejuvenation: the batch's scratch block carved -- the split path's chunk sums and site statistics, the info (a.info is
// d_site_info where given), the split path's counts and codes
static int rejScratch(sipnet_batch* b, RejArgs& a, int32_t* d_site_info, bool split) {
  const size_t nSites = (size_t)b->n_sites, nCnt = split ? nSites * (size_t)a.nCh : 0;
  return carveScratch(b, scratchOf(b).d_rejuv, [&](Carver& c) {
    a.part = c.take<double>(nCnt * kRejPrm);
    a.stat = c.take<double>(split ? nSites * 2 * kRejPrm : 0);
    int32_t* info = c.take<int32_t>(nSites * 4);
    a.info = d_site_info ? d_site_info : info;
    a.cnt = c.take<int32_t>(nCnt);
    a.kept = c.take<int32_t>(nCnt);
    a.site = c.take<int32_t>(split ? 2 * nSites : 0);
  });
}

// ---- the Metropolis move over members.  What both of its calls refuse before any launch, in this order: the listed rows (the joint analysis's checks; the
// bounds converted into a), the half, a NULL required array (named by `missing`), then the batch; the device made current.
static int mcBegin(const char* who, sipnet_batch* b, int32_t n_params, const sipnet_enkf_param* params, int32_t half,
                   const char* missing, McArgs& a) {
  if (n_params < 1 || n_params > kRejPrm) return refuse(who, "n_params must be 1.." + std::to_string(kRejPrm));
  RC_TRY(listedRowsCheck(who, n_params, params, a.lo, a.hi));
  if (half != 0 && half != 1) return refuse(who, "half must be 0 or 1");
  if (missing) return refuse(who, std::string("a NULL ") + missing);
  RC_TRY(movableBatch(who, b));
  a.half = half;
  moveShape(a, b, n_params, params);
  return useDevice(b);
}
// the batch's scratch block carved: the chunks' masks, the fallback info (a.info is d_site_info where given), the chunks'
// counts and the sites' codes
static int mcScratch(sipnet_batch* b, McArgs& a, int32_t* d_site_info) {
  const size_t nSites = (size_t)b->n_sites, nCnt = nSites * (size_t)a.nCh;
  return carveScratch(b, scratchOf(b).d_mcmc, [&](Carver& c) {
    a.masks = c.take<uint64_t>(4 * nCnt);
    int32_t* info = c.take<int32_t>(4 * nSites);
    a.info = d_site_info ? d_site_info : info;
    a.cntB = c.take<int32_t>(nCnt);
    a.off = c.take<int32_t>(nCnt);
    a.cntA = c.take<int32_t>(nCnt);
    a.made = c.take<int32_t>(nCnt);
    a.taken = c.take<int32_t>(nCnt);
    a.site = c.take<int32_t>(3 * nSites);
  });
}

// ---- the tempering exponent of every site.  The synchronous form's check: the arguments read back, the first bad site named
static int temperCheck(const char* who, const sipnet_batch* b, const TemperArgs& a, hipStream_t stream) {
  const size_t nSites = (size_t)b->n_sites, M = (size_t)b->n_members;
  std::vector<double> loglik, base, dmax, target;
  RC_TRY(readBack(loglik, a.loglik, (size_t)b->ncol, stream));
  RC_TRY(readBack(base, a.base, (size_t)b->ncol, stream));
  RC_TRY(readBack(dmax, a.deltaMax, nSites, stream));
  RC_TRY(readBack(target, a.essTarget, nSites, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (size_t s = 0; s < nSites; s++) {
    const double dm = a.deltaMax ? dmax[s] : 1.0;
    bool ok = dm > 0.0 && std::isfinite(dm) && target[s] > 0.0;
    for (size_t c = s * M; ok && c < (s + 1) * M; c++)
      ok = loglik[c] != INFINITY && (!a.base || base[c] != INFINITY);
    if (!ok)
      return refuse(who, "site " + std::to_string(s) + ": bad input (delta_max must be finite and > 0, the target > 0, no +inf among "
                         "loglik or base); nothing was written");
  }
  return SIPNET_OK;
}
// the per-chunk path's scratch carved: the states of the stages, the chunks' maxima, candidate maxima, partial sums and counts
static int temperScratch(sipnet_batch* b, TemperArgs& a) {
  const size_t nSites = (size_t)b->n_sites, nCk = nSites * (size_t)a.nChunks;
  return carveScratch(b, scratchOf(b).d_temper, [&](Carver& c) {
    a.state = c.take<TemperState>((size_t)(SIPNET_TEMPER_ROUNDS + 1) * nSites);
    a.chunkMax = c.take<double>(2 * nCk);
    a.candMax = c.take<double>(a.base ? nCk * kTemperCand : 0);
    a.partial = c.take<long long>(2 * nCk * kTemperWords);
    a.chunkCnt = c.take<int32_t>(nCk);
  });
}
template <bool Base>
static int temperLaunch(sipnet_batch* b, TemperArgs& a, bool split, hipStream_t stream) {
  const dim3 sites((unsigned)b->n_sites), chunks((unsigned)b->n_sites, (unsigned)a.nChunks);
  // One workgroup per site only without carried log-weights.  With them that kernel (15 maxima and 45 sums per thread in
  // registers, both arrays in LDS) reported an ESS(delta) that the filter did not reproduce at a few sites in a hundred, about
  // 1e-9 off, while the per-chunk launches did at every one; the cause is not found, so d_base takes the launches that are right.
  if (!split && !Base) {   // the site's loglik in LDS: past 48 KB a kernel has to ask
    const size_t ldsBytes = (size_t)a.M * sizeof(double);
    bool ok = false;
    RC_TRY(ldsGranted((const void*)temperGroupKernel, ldsBytes, b->device, &ok));
    if (ok) {
      hipLaunchKernelGGL(temperGroupKernel, sites, dim3(256), ldsBytes, stream, a);
      HIP_TRY(hipGetLastError());
      reportPath(b, true, (int32_t)b->n_sites);
      return SIPNET_OK;
    }
  }
  RC_TRY(temperScratch(b, a));
  hipLaunchKernelGGL(temperChunkMaxKernel<Base>, chunks, dim3(256), 0, stream, a);
  for (int stage = 0; stage <= SIPNET_TEMPER_ROUNDS; stage++) {
    if (Base) hipLaunchKernelGGL(temperChunkKernel<Base>, chunks, dim3(256), 0, stream, a, stage, 0);
    hipLaunchKernelGGL(temperChunkKernel<Base>, chunks, dim3(256), 0, stream, a, stage, 1);
  }
  hipLaunchKernelGGL(temperTailKernel<Base>, chunks, dim3(256), 0, stream, a);
  HIP_TRY(hipGetLastError());
  reportPath(b, false, 0);
  return SIPNET_OK;
}

extern "C" {

void sipnet_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
}

void sipnet_rejuvenate_normals(uint64_t seed, uint32_t draw, uint32_t stream, uint32_t member, uint32_t block, double z[4]) {
  memberNormals(drawKeyOf(seed, draw, nullptr), stream, member, block, true, z);
}

int sipnet_mcmc_draws(uint64_t seed, uint32_t draw, uint32_t stream, uint32_t member, int32_t n_other, int32_t idx[2], double* u) {
  if (n_other < 2 || !idx || !u) return refuse("sipnet_mcmc_draws", "n_other must be at least 2; idx and u must not be NULL");
  uint32_t x2;
  mcDraws(drawKeyOf(seed, draw, nullptr), stream, member, (uint32_t)n_other, &idx[0], &idx[1], &x2);
  *u = uniformOf(x2);
  return SIPNET_OK;
}

int sipnet_batch_pf_rejuvenate(sipnet_batch* b, int32_t n_params, const sipnet_enkf_param* params, const double* d_shrink,
                               int32_t pool_mask, const double* d_pool_sd, uint64_t seed, uint32_t draw,
                               const uint32_t* d_stream, const int64_t* d_site_total, int32_t* d_site_info, void* hip_stream) {
  const char* who = "sipnet_batch_pf_rejuvenate";
  RejArgs a{};
  RC_TRY(listedRowsCheck(who, n_params, params, a.lo, a.hi));
  if (n_params > 0 && !d_shrink) return refuse(who, "n_params > 0 needs d_shrink");
  if (pool_mask & ~((1 << kRejPools) - 1)) return refuse(who, "pool_mask must name pools 0..12");
  if (pool_mask && !d_pool_sd) return refuse(who, "a pool_mask needs d_pool_sd");
  if (n_params == 0 && pool_mask == 0) return refuse(who, "nothing to do (n_params == 0 and pool_mask == 0)");
  RC_TRY(movableBatch(who, b));
  RC_TRY(useDevice(b));
  hipStream_t stream = (hipStream_t)hip_stream;
  moveShape(a, b, n_params, params);
  a.mask = pool_mask;
  a.shrink = d_shrink;
  a.poolSd = d_pool_sd;
  a.key = drawKeyOf(seed, draw, d_stream);
  a.siteTotal = d_site_total;
  if (!d_site_info) {   // the synchronous form's check: shrink, pool_sd and the totals read back, the first bad selected site named
    const size_t nSites = (size_t)b->n_sites;
    std::vector<double> shrink, sd;
    std::vector<int64_t> total;
    RC_TRY(readBack(shrink, n_params > 0 ? d_shrink : nullptr, nSites, stream));
    RC_TRY(readBack(sd, pool_mask ? d_pool_sd : nullptr, nSites * kRejPools, stream));
    RC_TRY(readBack(total, d_site_total, nSites, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (size_t s = 0; s < nSites; s++)
      if (rejSiteInputs(shrink.data(), sd.data(), d_site_total ? total.data() : nullptr, n_params, pool_mask, (int64_t)s) == kRejBadInput)
        return refuse(who, "site " + std::to_string(s) + ": bad input (the shrink factor must lie in (0, 1]; a masked pool sd must be "
                           "finite and >= 0); nothing was written");
  }
  RC_TRY(moveBegin(b, stream, /*ownRows=*/n_params > 0, a));
  const MoveGrids g(b, a.nCh);
  RC_TRY(rejScratch(b, a, d_site_info, g.split));
  if (!g.split) {
    hipLaunchKernelGGL(rejGroupKernel, g.sites, dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL(rejChunkKernel, g.chunks, dim3(256), 0, stream, a, 0);
    hipLaunchKernelGGL(rejSiteKernel, g.sites, dim3(256), 0, stream, a, 0);
    if (n_params > 0) {
      hipLaunchKernelGGL(rejChunkKernel, g.chunks, dim3(256), 0, stream, a, 1);
      hipLaunchKernelGGL(rejSiteKernel, g.sites, dim3(256), 0, stream, a, 1);
    }
    hipLaunchKernelGGL(rejApplyKernel, g.chunks, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(rejInfoKernel, g.sites, dim3(256), 0, stream, a);
  }
  return moveLaunched(b, stream, !g.split);
}

int sipnet_batch_mcmc_propose(sipnet_batch* b, int32_t n_params, const sipnet_enkf_param* params, const double* d_gamma,
                              const double* d_jitter, int32_t half, uint64_t seed, uint32_t draw, const uint32_t* d_stream,
                              const int64_t* d_site_total, double* d_saved, int32_t* d_moved, int32_t* d_site_info,
                              void* hip_stream) {
  const char* who = "sipnet_batch_mcmc_propose";
  McArgs a{};
  RC_TRY(mcBegin(who, b, n_params, params, half, !d_gamma ? "d_gamma" : !d_saved ? "d_saved" : !d_moved ? "d_moved" : nullptr, a));
  hipStream_t stream = (hipStream_t)hip_stream;
  const int64_t nSites = b->n_sites;
  a.gamma = d_gamma;
  a.jitter = d_jitter;
  a.siteTotal = d_site_total;
  a.saved = d_saved;
  a.moved = d_moved;
  a.key = drawKeyOf(seed, draw, d_stream);
  if (!d_site_info) {   // the synchronous form's check: gamma, jitter and the totals read back, the first bad selected site named
    std::vector<double> gamma, jitter;
    std::vector<int64_t> total;
    RC_TRY(readBack(gamma, d_gamma, (size_t)nSites, stream));
    RC_TRY(readBack(jitter, d_jitter, (size_t)nSites, stream));
    RC_TRY(readBack(total, d_site_total, (size_t)nSites, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int64_t s = 0; s < nSites; s++)
      if (mcProposeInputs(gamma.data(), d_jitter ? jitter.data() : nullptr, d_site_total ? total.data() : nullptr, s) == kMcBadInput)
        return refuse(who, "site " + std::to_string(s) + ": bad input (gamma must be finite; a jitter must be finite and >= 0); nothing was written");
  }
  RC_TRY(moveBegin(b, stream, /*ownRows=*/true, a));
  RC_TRY(mcScratch(b, a, d_site_info));
  const MoveGrids g(b, a.nCh);
  if (!g.split) {
    hipLaunchKernelGGL(mcGroupKernel, g.sites, dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL(mcMaskKernel, g.chunks, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(mcSiteKernel, g.sites, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(mcProposeKernel, g.chunks, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(mcInfoKernel, g.sites, dim3(256), 0, stream, a);
  }
  return moveLaunched(b, stream, !g.split);
}

int sipnet_batch_mcmc_accept(sipnet_batch* b, int32_t n_params, const sipnet_enkf_param* params, const double* d_saved,
                             int32_t* d_moved, const double* d_logp_new, double* d_logp_cur, const double* d_beta, uint64_t seed,
                             uint32_t draw, const uint32_t* d_stream, int32_t* d_site_info, void* hip_stream) {
  const char* who = "sipnet_batch_mcmc_accept";
  McArgs a{};
  RC_TRY(mcBegin(who, b, n_params, params, 0,
                 !d_saved ? "d_saved" : !d_moved ? "d_moved" : !d_logp_new ? "d_logp_new" : !d_logp_cur ? "d_logp_cur" : nullptr, a));
  hipStream_t stream = (hipStream_t)hip_stream;
  const int64_t nSites = b->n_sites;
  a.beta = d_beta;
  a.saved = const_cast<double*>(d_saved);
  a.moved = d_moved;
  a.logpNew = d_logp_new;
  a.logpCur = d_logp_cur;
  a.key = drawKeyOf(seed, draw, d_stream);
  if (!d_site_info && d_beta) {   // the synchronous form's check: beta read back, the first bad site named
    std::vector<double> beta;
    RC_TRY(readBack(beta, d_beta, (size_t)nSites, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int64_t s = 0; s < nSites; s++)
      if (mcAcceptInputs(beta.data(), s) == kMcBadInput)
        return refuse(who, "site " + std::to_string(s) + ": bad input (beta must be finite and > 0); nothing was written");
  }
  RC_TRY(moveBegin(b, stream, /*ownRows=*/true, a));
  RC_TRY(mcScratch(b, a, d_site_info));
  const bool direct = a.nCh == 1;   // (a site of one chunk writes its info itself; the counts of more chunks meet in a launch of their own)
  const MoveGrids g(b, a.nCh);
  hipLaunchKernelGGL(mcAcceptKernel, g.chunks, dim3(256), 0, stream, a, direct ? 1 : 0);
  if (!direct) hipLaunchKernelGGL(mcAcceptInfoKernel, g.sites, dim3(256), 0, stream, a);
  return moveLaunched(b, stream, direct);
}

int sipnet_batch_pf_temper_sites(sipnet_batch* b, const double* d_loglik, const double* d_base, const double* d_delta_max,
                                 const double* d_ess_target, double* d_delta, double* d_delta_hi, double* d_ess,
                                 double* d_logw_out, int32_t* d_site_info, void* hip_stream) {
  const char* who = "sipnet_batch_pf_temper_sites";
  if (!b || !d_loglik || !d_ess_target || !d_delta) return refuse(who, "a NULL batch, d_loglik, d_ess_target or d_delta");
  if (tooManyColumns(b)) return refuse(who, "at most 4194304 columns");
  if (b->pfPeers) return refuse(who, "this batch is connected to a filter across ranks (sipnet_batch_pf_connect)");
  RC_TRY(useDevice(b));
  hipStream_t stream = (hipStream_t)hip_stream;
  TemperArgs a{};
  a.loglik = d_loglik;
  a.base = d_base;
  a.deltaMax = d_delta_max;
  a.essTarget = d_ess_target;
  a.delta = d_delta;
  a.deltaHi = d_delta_hi;
  a.ess = d_ess;
  a.logwOut = d_logw_out;
  a.info = d_site_info;
  a.M = b->n_members;
  a.nSites = b->n_sites;
  if (!d_site_info) RC_TRY(temperCheck(who, b, a, stream));
  int chunk, nChunks;
  const bool split = sitesGeometry(b, &chunk, &nChunks);   // (the many-site analysis's rule)
  a.chunk = chunk;
  a.nChunks = nChunks;
  return d_base ? temperLaunch<true>(b, a, split, stream) : temperLaunch<false>(b, a, split, stream);
}

}  // extern "C"
