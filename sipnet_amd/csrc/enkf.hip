// enkf.hip -- the ensemble Kalman filter analyses of the member pools: sipnet_batch_enkf_analysis_sites (a filter per
// site), _local (the localized serial filter across sites), _block (the block-local filter: every site on its own, in one
// pass), _joint (the filter per site with analysed parameters among its variables), _smooth (the joint call, and its update
// applied to the window's flux series) and _sharded (the filter per site of an ensemble sharded by member across ranks, from
// the moment blocks of sipnet_batch_enkf_shard_moments).
//
// Site s owns columns [s M, (s + 1) M).  Its live members' analysed pools and predicted observations are the analysis's
// variables: working copies W[v][member], v < nA the analysed pools (in state-slot order; the joint analysis: then the
// analysed parameters), nA + i the h of operator i.
// The serial square-root update (EAKF, Whitaker & Hamill 2002) recomputes every observation's statistics from the current
// ensemble: sums of the variables, then centred sums against h_i.  A sum is always taken in ONE order: chunks of 256
// members, a chunk by a fixed tree (every wave by an xor-shuffle butterfly, then the four waves in order); the chunk totals
// in segments of segLen(nCh) >= 16 consecutive chunks, each in order from 0.0; one segment is the site's total, several (at
// most 64) are combined by one wave's xor-shuffle butterfly.  A site of the one-workgroup-per-site kernel has at most 16 chunks,
// one segment: so that kernel and the per-chunk launches give the same bits.  No grid barrier, no spin, no atomic.
//
// This file is the one translation unit and the host side; the device code is in parts, included below in this order:
//   site_device.h     what pf.hip and quantiles.hip share with this unit: the sums in their one order, the pieces of a member's
//                     limits, the derived parameter rows (site_host.h: the host's refusals, bookkeeping and scratch growth)
//   enkf_common.inc   what every kernel is written in: the arguments (EnkfArgs, JointArgs), a site's inputs, predicted(), the
//                     gains, a member's load, inflation and limits.  Every difference between
//                     the joint and the per-site arguments is a function here: no kernel body forks on the argument type.
//   enkf_sites.inc    enkfSiteKernel (one workgroup per site: enkfSites) and the per-chunk kernels, a launch per stage: load,
//                     code, partial, final, update (enkfFront, enkfSites), limit, info (enkfEnd); for either arguments
//   enkf_local.inc    enkfReachKernel (enkfFront, given a localization); enkfLocalKernel, a workgroup per (observation slot,
//                     target site): a launch per level of the host schedule (sipnet_batch_enkf_analysis_local)
//   enkf_block.inc    enkfBlockKernel, a workgroup per target site running its serial update on its small sample covariance:
//                     ONE launch (sipnet_batch_enkf_analysis_block)
//   enkf_sharded.inc  the moments of a rank's members (enkfShardSum / Product / TotalKernel), the merge of the ranks' blocks and
//                     the chain (enkfShardChainKernel, a workgroup per site), the transform applied (enkfShardApplyKernel)
//   enkf_smooth.inc   enkfSmoothPrepKernel (smoothFront, before the pool analysis) and enkfSmoothKernel (smoothSeries, after)
//
// The host side: every entry point fills an EnkfCall and is its checks (localChecks for the two with a localization, then
// enkfBegin), the scratch block (enkfScratch), the front of the per-chunk launches (enkfFront: load, codes, reach, inflation),
// a middle of its own, and the tail (enkfEnd: limits, info, bookkeeping).  The per-site and joint calls (enkfSites) may
// instead run the one-workgroup-per-site kernel between scratch and tail.  The smoothing call is the joint call (jointCall)
// around a series stage that runs the same front on a scratch block of its own.  Whoever wants dynamic LDS asks ldsGranted.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "batch_impl.h"
#include "site_host.h"

namespace {

#include "site_device.h"
#include "enkf_common.inc"
#include "enkf_sites.inc"
#include "enkf_local.inc"
#include "enkf_block.inc"
#include "enkf_sharded.inc"
#include "enkf_smooth.inc"

}  // namespace

// a localization: the level-ordered table of (slot, target) pairs and the in-neighbour lists, on the batch's device
struct sipnet_enkf_local {
  sipnet_batch* b = nullptr;
  int32_t device = 0, nSites = 0, nObs = 0, nLevels = 0;
  bool serial = false;                     // sipnet_debug_enkf_local_serial: one slot per launch, in serial order
  std::vector<int64_t> levelOff;           // [nLevels + 1]: the pairs of level l are [levelOff[l], levelOff[l + 1])
  std::vector<int64_t> slotOff;            // [n_sites][n_obs]: where slot (s, i)'s 1 + deg(s) pairs start
  std::vector<int32_t> slotLen;
  DevBuf<LocalPair> d_pair;
  DevBuf<int64_t> d_inPtr;                 // [n_sites + 1]: site t is a neighbour of the sites d_in[d_inPtr[t] ..)
  DevBuf<int32_t> d_in;
  DevBuf<double> d_inRho;                  // the tapers rho_ut in d_in's order
  int32_t maxRows = 0;                     // the block-local analysis: the largest n_obs x (1 + in-neighbours) of a site
};

namespace {

// what every analysis is called with, as its extern "C" function received it
struct EnkfCall {
  sipnet_batch* b;
  int32_t n_obs;
  const sipnet_enkf_obs* ops;
  int32_t analysed_mask;
  const void* const* d_planes;
  int32_t elem_is_f32, n_steps;
  int64_t ld;
  const double *d_obs, *d_sd, *d_inflation;
  int32_t* d_site_info;
  hipStream_t stream;
  bool momentsOnly = false;                // sipnet_batch_enkf_shard_moments: no observations, nothing of the batch written
};

// The checks and the arguments the analyses share, up to the scratch block: 0, or the error (the message names `name`).
// The synchronous form (no d_site_info) reads obs, sd and inflation back and refuses a bad site before anything is written.
int enkfBegin(const char* name, const EnkfCall& c, EnkfArgs& a, bool ownRows = false) {
  sipnet_batch* const b = c.b;
  const int32_t n_obs = c.n_obs;
  const hipStream_t stream = c.stream;
  const int32_t allPools = (1 << kPools) - 1;
  if (!b || !c.ops || (!c.momentsOnly && (!c.d_obs || !c.d_sd))) return refuse(name, "a NULL batch, operators, observations or sds");
  if (n_obs < 1 || n_obs > kMaxObs) return refuse(name, "n_obs must be 1..16");
  if (c.analysed_mask == 0 || (c.analysed_mask & ~allPools)) return refuse(name, "analysed_mask must name pools 0..12");
  bool planesUsed = false;
  for (int i = 0; i < n_obs; i++) {
    const sipnet_enkf_obs& o = c.ops[i];
    const std::string at = "operator " + std::to_string(i) + ": ";
    if (o.param < -1 || o.param >= SIPNET_NPARAMS) return refuse(name, at + "param is not a parameter index");
    if (o.kind == SIPNET_ENKF_POOLS) {
      if (o.pool_mask == 0 || (o.pool_mask & ~allPools)) return refuse(name, at + "pool_mask must name pools 0..12");
    } else if (o.kind == SIPNET_ENKF_PLANE) {
      if (o.plane < 0 || o.plane > 2) return refuse(name, at + "plane must be 0 (NEE), 1 (GPP) or 2 (ET)");
      if (!c.d_planes || !c.d_planes[o.plane]) return refuse(name, at + "its plane pointer is NULL");
      planesUsed = true;
    } else {
      return refuse(name, at + "unknown kind");
    }
  }
  if (planesUsed && (c.n_steps <= 0 || c.ld < b->ncol)) return refuse(name, "planes need n_steps > 0 and ld >= ncol");
  if (tooManyColumns(b)) return refuse(name, "at most 4194304 members");
  if (b->pfPeers) return refuse(name, "this batch is connected to a filter across ranks (sipnet_batch_pf_connect)");
  int rc = useDevice(b);
  if (rc) return rc;
  const int64_t nSites = b->n_sites, M = b->n_members, ncol = b->ncol;
  if (!c.d_site_info && !c.momentsOnly) {   // the synchronous form: the inputs are checked before anything is launched
    std::vector<double> obs, sd, infl;
    RC_TRY(readBack(obs, c.d_obs, (size_t)(nSites * n_obs), stream));
    RC_TRY(readBack(sd, c.d_sd, obs.size(), stream));
    RC_TRY(readBack(infl, c.d_inflation, (size_t)nSites, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int64_t s = 0; s < nSites; s++) {
      int used;
      if (siteInputs(obs.data(), sd.data(), c.d_inflation ? infl.data() : nullptr, n_obs, (int)s, &used) == kBadInput)
        return refuse(name, "site " + std::to_string(s) + ": bad input (a finite obs needs a finite sd > 0; the inflation must "
                            "be finite and >= 1); nothing was written");
    }
  }
  if (c.momentsOnly) {   // (nothing of the batch is written: what a forecast has left stays good)
    RC_TRY(orderBehindBusy(b, stream));
    RC_TRY(flushParams(b, stream));
  } else {
    RC_TRY(beginWrite(b, stream, ownRows));
  }

  a = EnkfArgs{};
  a.nObs = n_obs;
  for (int i = 0; i < n_obs; i++) a.op[i] = EnkfOp{c.ops[i].kind, c.ops[i].pool_mask, c.ops[i].plane, c.ops[i].param, c.ops[i].scale};
  for (int p = 0; p < kPools; p++)
    if (c.analysed_mask & (1 << p)) a.pool[a.nA++] = p;
  a.nv = a.nA + n_obs;
  a.nCh = (int32_t)((M + 255) / 256);
  for (int k = 0; k < 3; k++) a.planes[k] = c.d_planes ? c.d_planes[k] : nullptr;
  a.nSteps = c.n_steps;
  a.ld = c.ld;
  a.obs = c.d_obs;
  a.sd = c.d_sd;
  a.infl = c.d_inflation;
  a.state = b->d_state;
  a.ncol = ncol;
  a.M = M;
  a.siteStatus = b->d_siteStatus;
  if (b->prmIndexed) {   // (after a resampling with_params: column c's parameters are bank column d_prmId[c])
    a.prm = b->d_prmBank ? b->d_prmBank : b->d_prm;
    a.prmPitch = b->d_prmBank ? b->prmBankPitch : ncol;
    a.prmId = b->d_prmId;
  } else {
    a.prm = b->d_prm;
    a.prmPitch = ncol;
    a.prmId = nullptr;
  }
  return 0;
}

// A scratch block of the batch (b->d_enkf, or the series stage's b->d_smooth) sized, grown and carved, in
// this order: the working copies [nv][ncol] (workInGlobal: else they live in LDS) | part [sites][chunks][cap] | stat [sites]
// [3 cap] (cap: the kernels' A::kCap) | matPerSite doubles per site (the block-local matrices, the series stage's g and G) | info
// [sites][4] (a.info is d_site_info where given) | cnt, kept [sites][chunks] | site [sites][2] | src [sites] (withSrc).  part,
// stat, cnt, kept and site are the per-chunk launches' (perChunk: without them the regions are empty, and cnt, kept and site,
// which the one-workgroup-per-site kernel never reads, all point at the end of info).  *mat, where asked for, gets the base of
// the doubles per site.
int enkfScratch(sipnet_batch* b, DevBuf<unsigned char>& block, EnkfArgs& a, int32_t* d_site_info, bool workInGlobal,
                bool perChunk, bool withSrc, size_t matPerSite, double** mat, int cap = kMaxVars) {
  const size_t nSites = (size_t)b->n_sites;
  const size_t nWork = workInGlobal ? (size_t)a.nv * (size_t)b->ncol : 0;
  const size_t nCnt = perChunk ? nSites * a.nCh : 0;
  const size_t nPart = nCnt * cap;
  const size_t nStat = perChunk ? nSites * 3 * cap : 0;
  const size_t nMat = nSites * matPerSite;
  const size_t nSite = perChunk ? 2 * nSites : 0;
  const size_t nInt = nSites * 4 + 2 * nCnt + nSite + (withSrc ? nSites : 0);
  const size_t bytes = (nWork + nPart + nStat + nMat) * sizeof(double) + nInt * sizeof(int32_t);
  RC_TRY(growScratch(b, block, bytes));
  a.work = (double*)block.get();
  a.part = a.work + nWork;
  a.stat = a.part + nPart;
  double* matrices = a.stat + nStat;
  int32_t* ints = (int32_t*)(matrices + nMat);
  a.info = d_site_info ? d_site_info : ints;
  a.cnt = ints + nSites * 4;
  a.kept = a.cnt + nCnt;
  a.site = a.kept + nCnt;
  a.src = withSrc ? a.site + nSite : nullptr;
  if (mat) *mat = matrices;
  return 0;
}

// the grids of the per-chunk launches: sites x chunks of 256 members, and sites
dim3 chunkGrid(const sipnet_batch* b, const EnkfArgs& a) { return dim3((unsigned)b->n_sites, (unsigned)a.nCh); }
dim3 siteGrid(const sipnet_batch* b) { return dim3((unsigned)b->n_sites); }

// some site may inflate: the call has a lambda
bool mayInflate(const EnkfArgs& a) { return a.infl != nullptr; }
bool mayInflate(const JointArgs& a) { return a.infl != nullptr || a.prmInfl != nullptr; }
// the front of the per-chunk launches: the load (the planes' elements float or double), the codes, the sites that a
// localization's sources reach (L), the inflation
template <class A>
void enkfFront(const EnkfCall& c, const A& a, const sipnet_enkf_local* L) {
  const hipStream_t stream = c.stream;
  const dim3 chunks = chunkGrid(c.b, a), sites = siteGrid(c.b);
  hipLaunchKernelGGL((c.elem_is_f32 ? enkfLoadKernel<float, A> : enkfLoadKernel<double, A>), chunks, dim3(256), 0, stream, a);
  hipLaunchKernelGGL(enkfCodeKernel<A>, sites, dim3(256), 0, stream, a);
  if (L)
    hipLaunchKernelGGL(enkfReachKernel, dim3((sites.x + 255) / 256), dim3(256), 0, stream, a, L->d_inPtr, L->d_in,
                       (int64_t)c.b->n_sites);
  if (mayInflate(a)) {
    hipLaunchKernelGGL(enkfPartialKernel<A>, chunks, dim3(256), 0, stream, a, -1, 0);
    hipLaunchKernelGGL(enkfFinalKernel<A>, sites, dim3(256), 0, stream, a, -1, 0);
    hipLaunchKernelGGL(enkfUpdateKernel<A>, chunks, dim3(256), 0, stream, a, -1);
  }
}

// the tail of every analysis: the limits and the info of the per-chunk launches (perChunk: the one-workgroup-per-site kernel
// has done its own), the launches' error, what sipnet_batch_pf_info reports, the batch busy on the stream
template <class A>
int enkfEnd(const EnkfCall& c, const A& a, bool perChunk, int32_t fused, int32_t grid) {
  sipnet_batch* const b = c.b;
  if (perChunk) {
    hipLaunchKernelGGL(enkfLimitKernel<A>, chunkGrid(b, a), dim3(256), 0, c.stream, a);
    hipLaunchKernelGGL(enkfInfoKernel<A>, siteGrid(b), dim3(256), 0, c.stream, a);
  }
  HIP_TRY(hipGetLastError());
  reportPath(b, fused != 0, grid);
  return markBusy(b, c.stream);
}

// the per-site analysis between enkfBegin and the end of the call, for the per-site call's arguments or the joint call's
template <class A>
int enkfSites(const EnkfCall& c, A& a) {
  sipnet_batch* const b = c.b;
  const hipStream_t stream = c.stream;
  const int64_t nSites = b->n_sites, M = b->n_members;
  // the per-chunk launches unless the sites outnumber the CUs four times over (profiles/r08_enkf_sites_time.txt: one
  // workgroup per site loses or ties at every shape up to 256 sites x 1 024 members -- 0.29 ms against 0.19); big sites or
  // SIPNET_KOPT_PF_MULTI_LAUNCH: always the launches
  const bool group = M <= 256 * kMaxGroupChunks && nSites >= 4 * (int64_t)b->numCUs &&
                     !(b->kernelOptions & SIPNET_KOPT_PF_MULTI_LAUNCH);
  const size_t ldsBytes = (size_t)a.nv * (size_t)M * sizeof(double);
  bool lds = group && ldsBytes <= (size_t)kLdsWork;   // (the working copies in LDS: beside 19.5 KB of static LDS, the joint call's 30)
  const auto siteKernel = c.elem_is_f32 ? enkfSiteKernel<float, A> : enkfSiteKernel<double, A>;
  int rc = lds ? ldsGranted((const void*)siteKernel, ldsBytes, b->device, &lds) : 0;
  if (rc) return rc;
  a.useLds = lds;
  rc = enkfScratch(b, b->d_enkf, a, c.d_site_info, /*workInGlobal=*/!a.useLds, /*perChunk=*/!group,
                   /*withSrc=*/false, 0, nullptr, A::kCap);
  if (rc) return rc;
  if (group) {
    hipLaunchKernelGGL(siteKernel, siteGrid(b), dim3(256), a.useLds ? ldsBytes : 0, stream, a);
  } else {
    const dim3 chunks = chunkGrid(b, a), sites = siteGrid(b);
    enkfFront(c, a, nullptr);
    for (int i = 0; i < c.n_obs; i++) {
      hipLaunchKernelGGL(enkfPartialKernel<A>, chunks, dim3(256), 0, stream, a, i, 0);
      hipLaunchKernelGGL(enkfFinalKernel<A>, sites, dim3(256), 0, stream, a, i, 0);
      hipLaunchKernelGGL(enkfPartialKernel<A>, chunks, dim3(256), 0, stream, a, i, 1);
      hipLaunchKernelGGL(enkfFinalKernel<A>, sites, dim3(256), 0, stream, a, i, 1);
      hipLaunchKernelGGL(enkfUpdateKernel<A>, chunks, dim3(256), 0, stream, a, i);
    }
  }
  return enkfEnd(c, a, /*perChunk=*/!group, group ? 1 : 0, group ? (int32_t)b->n_sites : 0);
}

// the checks of a localization's lists (withRho: and of its tapers)
int localLists(const char* name, int32_t nSites, int32_t nObs, const int64_t* ptr, const int32_t* nbr, const double* rho,
               bool withRho) {
  if (nObs < 1 || nObs > kMaxObs) return refuse(name, "n_obs must be 1..16");
  if (nSites < 1 || (int64_t)nSites * nObs > INT32_MAX) return refuse(name, "n_sites must be >= 1 (and n_sites x n_obs < 2^31)");
  if (!ptr) return refuse(name, "a NULL nbr_ptr");
  if (ptr[0] != 0) return refuse(name, "nbr_ptr[0] must be 0");
  for (int32_t s = 0; s < nSites; s++)
    if (ptr[s + 1] < ptr[s]) return refuse(name, "nbr_ptr must be non-decreasing (site " + std::to_string(s) + ")");
  if (ptr[nSites] > 0 && (!nbr || (withRho && !rho))) return refuse(name, "a NULL nbr or rho with neighbours listed");
  for (int32_t s = 0; s < nSites; s++)
    for (int64_t k = ptr[s]; k < ptr[s + 1]; k++) {
      const std::string at = "site " + std::to_string(s) + ", entry " + std::to_string(k - ptr[s]) + ": ";
      if (nbr[k] < 0 || nbr[k] >= nSites) return refuse(name, at + "neighbour index out of range");
      if (nbr[k] == s) return refuse(name, at + "a site is not its own neighbour");
      if (k > ptr[s] && nbr[k] <= nbr[k - 1]) return refuse(name, at + "a row must be strictly ascending (no duplicates)");
      if (withRho && !(rho[k] > 0.0 && rho[k] <= 1.0)) return refuse(name, at + "rho must be finite and in (0, 1]");
    }
  return 0;
}
// The localization's lists checked, and the greedy schedule of the slots (s, i) in serial order: level(s, i) = 1 + the last
// level that touched a site of F(s) = {s} + nbr(s) (none: -1, so empty lists give level i).  Conflicting slots (footprints that
// meet) are therefore in serial order, and the slots of one level have disjoint footprints.  level: [n_sites][n_obs].
int localSchedule(const char* name, int32_t nSites, int32_t nObs, const int64_t* ptr, const int32_t* nbr, const double* rho,
                  std::vector<int32_t>& level, int32_t* nLevels) {
  int rc = localLists(name, nSites, nObs, ptr, nbr, rho, true);
  if (rc) return rc;
  std::vector<int32_t> last((size_t)nSites, -1);
  level.assign((size_t)nSites * nObs, 0);
  int32_t top = -1;
  for (int32_t s = 0; s < nSites; s++)
    for (int32_t i = 0; i < nObs; i++) {
      int32_t l = last[s];
      for (int64_t k = ptr[s]; k < ptr[s + 1]; k++) l = last[nbr[k]] > l ? last[nbr[k]] : l;
      l += 1;
      last[s] = l;
      for (int64_t k = ptr[s]; k < ptr[s + 1]; k++) last[nbr[k]] = l;
      level[(size_t)s * nObs + i] = l;
      top = l > top ? l : top;
    }
  *nLevels = top + 1;
  return 0;
}
// n_obs x (1 + in-neighbours) of every site: the most rows a target of the block-local analysis can have
std::vector<int32_t> localRows(int32_t nSites, int32_t nObs, const int64_t* ptr, const int32_t* nbr) {
  std::vector<int32_t> rows((size_t)nSites, nObs);
  for (int64_t e = 0; e < ptr[nSites]; e++) {
    int32_t& r = rows[(size_t)nbr[e]];
    r = r > INT32_MAX - nObs ? INT32_MAX : r + nObs;
  }
  return rows;
}

// the checks the two analyses with a localization open with
int localChecks(const char* name, const sipnet_batch* b, const sipnet_enkf_local* L, int32_t n_obs) {
  if (!b || !L) return refuse(name, "a NULL batch or localization");
  if (L->b != b) return refuse(name, "the localization belongs to another batch");
  if (L->nObs != n_obs) return refuse(name, "the localization was made for n_obs = " + std::to_string(L->nObs));
  if (b->n_members > 256 * kMaxGroupChunks) return refuse(name, "at most 4096 members per site");
  return 0;
}


// ---- the joint analysis's parameters ------------------------------------------------------------------------------------------
const char* const kParamName[SIPNET_NPARAMS] = {
#define SIPNET_PARAM(index, field, file_name, rule) #field,
#include "../../include/sipnet_params.def"
#undef SIPNET_PARAM
};
// convertParamsKernel's per-year -> per-day rows: the converted value is the file value / 365.0
bool rateRow(int p) {
  switch (p) {
    case SP_baseVegResp: case SP_litterBreakdownRate: case SP_baseSoilResp: case SP_woodTurnoverRate:
    case SP_leafTurnoverRate: case SP_fineRootTurnoverRate: case SP_coarseRootTurnoverRate:
    case SP_baseCoarseRootResp: case SP_baseFineRootResp: return true;
    default: return false;
  }
}
// why row p cannot be analysed, or null: its converted value is neither the file value nor the file value / 365, or only
// setup reads it
const char* refusedRow(int p) {
  switch (p) {
    case SP_psnTMax: case SP_coarseRootAllocation:
      return "a derived row (rewritten from the rows it depends on)";
    case SP_plantWoodInit: case SP_laiInit: case SP_soilInit: case SP_soilWFracInit: case SP_litterInit: case SP_snowInit:
    case SP_minNInit: case SP_soilOrgNInit: case SP_litterOrgNInit: case SP_plantStorageNInit:
      return "an initial condition, which only setup reads";
    case SP_leafOnDay: case SP_leafOffDay: case SP_gddLeafOn: case SP_soilTempLeafOn:
      return "a phenology threshold (the gddLeafOn row is overloaded by the leaf-on mode)";
    case SP_fAnoxia: case SP_anaerobicDecompRate:
      return "a row the conversion clamps";
    default: return nullptr;
  }
}
// sipnet_enkf_params_check's checks; lo / hi (may be null): the bounds in converted units, by the conversion's own expression
int paramsCheck(const char* name, int32_t n, const sipnet_enkf_param* params, double* lo, double* hi) {
  if (n < 0 || n > kMaxPrm) return refuse(name, "n_params must be 0..16");
  if (n > 0 && !params) return refuse(name, "NULL params with n_params > 0");
  for (int k = 0; k < n; k++) {
    const sipnet_enkf_param& q = params[k];
    const std::string at = "parameter " + std::to_string(k) + ": ";
    if (q.index < 0 || q.index >= SIPNET_NPARAMS) return refuse(name, at + "index is not a parameter index");
    const std::string who = at + kParamName[q.index] + " ";
    if (const char* why = refusedRow(q.index)) return refuse(name, who + "is " + why);
    for (int e = 0; e < k; e++)
      if (params[e].index == q.index) return refuse(name, who + "is listed twice");
    if (!(fabs(q.lo) < INFINITY) || !(fabs(q.hi) < INFINITY)) return refuse(name, who + "has a bound that is not finite");
    if (!(q.lo < q.hi)) return refuse(name, who + "needs lo < hi");
    double l = q.lo, h = q.hi;
    if (rateRow(q.index)) {
      l /= 365.0;
      h /= 365.0;
    }
    if (lo) lo[k] = l;
    if (hi) hi[k] = h;
  }
  return 0;
}


// ---- the smoother's host side ----------------------------------------------------------------------------------------------
// the refusals of the series, before any launch
int smoothChecks(const char* name, const sipnet_batch* b, int32_t nSeries, const sipnet_enkf_series* series) {
  if (nSeries < 0 || nSeries > kMaxSeries) return refuse(name, "n_series must be 0.." + std::to_string(kMaxSeries));
  if (nSeries > 0 && !series) return refuse(name, "NULL series with n_series > 0");
  if (nSeries > 0 && b->n_members > 256 * kMaxGroupChunks) return refuse(name, "series need at most 4096 members per site");
  for (int k = 0; k < nSeries; k++) {
    const sipnet_enkf_series& q = series[k];
    const std::string at = "series " + std::to_string(k) + ": ";
    if (!q.src || !q.dst) return refuse(name, at + "a NULL src or dst");
    if (q.rows < 1) return refuse(name, at + "rows must be >= 1");
    if (q.ld < b->ncol) return refuse(name, at + "ld must be >= ncol");
    for (int e = 0; e < nSeries; e++) {
      if (e < k && series[e].dst == q.dst) return refuse(name, at + "its dst is also the dst of series " + std::to_string(e));
      if (e != k && series[e].src == q.dst) return refuse(name, at + "its dst is the src of series " + std::to_string(e));
    }
  }
  return 0;
}

// What the series stage keeps between its two halves.  The first half (smoothFront, before the pool analysis: it reads the
// forecast state and planes) forms the inflated h by enkfFront on a working copy of the stage's own and reduces them to a, g
// and G; the second (smoothSeries, after it: a series may be a plane the pool analysis reads) smooths the series.
struct SmoothStage {
  SmoothArgs k;
  bool useLds = false;
  size_t ldsBytes = 0;
  int32_t blocks = 0;
};
// the kernel of a site of M members: teams of one wave up to 1 024 members (kCh = members a lane holds), else sixteen waves
template <bool kLds>
const void* smoothKernelOf(int64_t M) {
  if (M <= 64) return (const void*)enkfSmoothKernel<kLds, 1, 1>;
  if (M <= 128) return (const void*)enkfSmoothKernel<kLds, 1, 2>;
  if (M <= 256) return (const void*)enkfSmoothKernel<kLds, 1, 4>;
  if (M <= 512) return (const void*)enkfSmoothKernel<kLds, 1, 8>;
  if (M <= 1024) return (const void*)enkfSmoothKernel<kLds, 1, 16>;
  if (M <= 2048) return (const void*)enkfSmoothKernel<kLds, 16, 2>;
  return (const void*)enkfSmoothKernel<kLds, 16, 4>;
}

int smoothFront(const EnkfCall& c, const JointArgs& joint, int32_t nSeries, const sipnet_enkf_series* series, SmoothStage& st) {
  sipnet_batch* const b = c.b;
  const size_t nSites = (size_t)b->n_sites;
  JointArgs a = joint;   // the h alone: no analysed pool, no analysed parameter (the codes still check both lambdas)
  a.nPool = a.nPrm = a.nA = 0;
  a.nv = a.nObs;
  // the stage's block: the h, then their anomalies [n_obs][ncol] | the per-chunk regions | a site's g, G, p, n.  A block of its
  // own, not a corner of the batch's: the pool analysis that follows carves b->d_enkf for itself, and so runs on exactly what
  // it runs on without series.
  double* meta = nullptr;
  int rc = enkfScratch(b, b->d_smooth, a, nullptr, /*workInGlobal=*/true, /*perChunk=*/true, /*withSrc=*/false,
                       kMeta, &meta, JointArgs::kCap);
  if (rc) return rc;

  SmoothArgs& k = st.k;
  k = SmoothArgs{};
  k.nSeries = nSeries;
  int64_t totalRows = 0;
  for (int e = 0; e < nSeries; e++) totalRows += series[e].rows;
  // rows per workgroup: at least 16 (staging a site's anomalies costs about p / 2 rows' traffic, and a workgroup of one-wave
  // teams has four rows in flight), more once that still leaves eight workgroups per CU
  const int64_t want = totalRows * (int64_t)nSites / (8 * (int64_t)std::max(b->numCUs, 1));
  k.run = (int32_t)std::min<int64_t>(64, std::max<int64_t>(16, want));
  int64_t blocks = 0;
  for (int e = 0; e < nSeries; e++) {
    k.ser[e] = SmoothSeries{series[e].src, series[e].dst, series[e].ld, series[e].rows, series[e].elem_is_f32 ? 1 : 0, (int32_t)blocks, 0};
    blocks += (series[e].rows + k.run - 1) / k.run;
  }
  if (blocks > 65535) return refuse("sipnet_batch_enkf_analysis_smooth", "the series have too many rows for one launch");
  st.blocks = (int32_t)blocks;
  k.anom = a.work;
  k.meta = meta;
  k.site = a.site;
  k.infl = a.infl;
  k.siteStatus = a.siteStatus;
  k.status = a.state + (int64_t)ST_status * a.ncol;
  k.ncol = a.ncol;
  k.M = a.M;
  // the anomalies in LDS when [n_obs][M] fits beside the kernel's tables (SIPNET_KOPT_PF_MULTI_LAUNCH: always from scratch)
  st.ldsBytes = (size_t)a.nObs * (size_t)a.M * sizeof(double);
  st.useLds = !(b->kernelOptions & SIPNET_KOPT_PF_MULTI_LAUNCH);
  rc = st.useLds ? ldsGranted(smoothKernelOf<true>(a.M), st.ldsBytes, b->device, &st.useLds) : 0;
  if (rc) return rc;
  enkfFront(c, a, nullptr);
  hipLaunchKernelGGL(enkfSmoothPrepKernel, siteGrid(b), dim3(256), 0, c.stream, a, meta);
  HIP_TRY(hipGetLastError());
  return 0;
}

int smoothSeries(sipnet_batch* b, const SmoothStage& st, hipStream_t stream) {
  const dim3 grid((unsigned)b->n_sites, (unsigned)st.blocks);
  void* args[] = {(void*)&st.k};
  const void* kernel = st.useLds ? smoothKernelOf<true>(st.k.M) : smoothKernelOf<false>(st.k.M);
  HIP_TRY(hipLaunchKernel(kernel, grid, dim3(st.k.M <= 1024 ? 256 : 1024), args, st.useLds ? st.ldsBytes : 0, stream));
  return markBusy(b, stream);
}

// sipnet_batch_enkf_analysis_joint, and with series sipnet_batch_enkf_analysis_smooth
int jointCall(const char* name, const EnkfCall& c, int32_t n_params, const sipnet_enkf_param* params,
              const double* d_param_inflation, int32_t n_series, const sipnet_enkf_series* series) {
  sipnet_batch* const b = c.b;
  const hipStream_t stream = c.stream;
  JointArgs a{};
  int rc = paramsCheck(name, n_params, params, a.lo, a.hi);
  if (rc) return rc;
  if (b && (rc = smoothChecks(name, b, n_series, series))) return rc;
  if (b && d_param_inflation && !c.d_site_info && !b->pfPeers) {   // the synchronous form: checked before anything is launched
    rc = useDevice(b);
    if (rc) return rc;
    std::vector<double> infl;
    RC_TRY(readBack(infl, d_param_inflation, (size_t)b->n_sites, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (size_t s = 0; s < infl.size(); s++)
      if (!(infl[s] >= 1.0) || !(infl[s] < INFINITY))
        return refuse(name, "site " + std::to_string(s) + ": bad input (the parameter inflation must be finite and >= 1); "
                            "nothing was written");
  }
  // (enkfBegin fills the arguments the analyses share and leaves the bounds alone; every column its own rows: the limits
  // write them, and a.prm is b->d_prm in column order)
  rc = enkfBegin(name, c, a, /*ownRows=*/true);
  if (rc) return rc;
  a.prmOut = b->d_prm;
  a.prmInfl = d_param_inflation;
  a.nPool = a.nA;
  a.nPrm = n_params;
  a.nA += n_params;
  a.nv += n_params;
  a.rows = derivedRowsOf(n_params, params, a.prmRow);
  if (n_series == 0) return enkfSites(c, a);
  SmoothStage st;
  rc = smoothFront(c, a, n_series, series, st);
  if (rc) return rc;
  rc = enkfSites(c, a);
  if (rc) return rc;
  return smoothSeries(b, st, stream);
}

}  // namespace

extern "C" {

int sipnet_batch_enkf_analysis_sites(sipnet_batch* b, int32_t n_obs, const sipnet_enkf_obs* ops, int32_t analysed_mask,
                                     const void* const d_planes[3], int32_t elem_is_f32, int32_t n_steps, int64_t ld,
                                     const double* d_obs, const double* d_sd, const double* d_inflation,
                                     int32_t* d_site_info, void* hip_stream) {
  const EnkfCall c{b, n_obs, ops, analysed_mask, d_planes, elem_is_f32, n_steps, ld, d_obs, d_sd, d_inflation, d_site_info,
                   (hipStream_t)hip_stream};
  EnkfArgs a;
  int rc = enkfBegin("sipnet_batch_enkf_analysis_sites", c, a);
  if (rc) return rc;
  return enkfSites(c, a);
}

int sipnet_enkf_params_check(int32_t n_params, const sipnet_enkf_param* params, double* lo_converted, double* hi_converted) {
  return paramsCheck("sipnet_enkf_params_check", n_params, params, lo_converted, hi_converted);
}

int sipnet_batch_enkf_analysis_joint(sipnet_batch* b, int32_t n_obs, const sipnet_enkf_obs* ops, int32_t analysed_mask,
                                     int32_t n_params, const sipnet_enkf_param* params, const void* const d_planes[3],
                                     int32_t elem_is_f32, int32_t n_steps, int64_t ld, const double* d_obs, const double* d_sd,
                                     const double* d_inflation, const double* d_param_inflation, int32_t* d_site_info,
                                     void* hip_stream) {
  const EnkfCall c{b, n_obs, ops, analysed_mask, d_planes, elem_is_f32, n_steps, ld, d_obs, d_sd, d_inflation, d_site_info,
                   (hipStream_t)hip_stream};
  return jointCall("sipnet_batch_enkf_analysis_joint", c, n_params, params, d_param_inflation, 0, nullptr);
}

int sipnet_batch_enkf_analysis_smooth(sipnet_batch* b, int32_t n_obs, const sipnet_enkf_obs* ops, int32_t analysed_mask,
                                      int32_t n_params, const sipnet_enkf_param* params, const void* const d_planes[3],
                                      int32_t elem_is_f32, int32_t n_steps, int64_t ld, const double* d_obs, const double* d_sd,
                                      const double* d_inflation, const double* d_param_inflation, int32_t n_series,
                                      const sipnet_enkf_series* series, int32_t* d_site_info, void* hip_stream) {
  const EnkfCall c{b, n_obs, ops, analysed_mask, d_planes, elem_is_f32, n_steps, ld, d_obs, d_sd, d_inflation, d_site_info,
                   (hipStream_t)hip_stream};
  return jointCall("sipnet_batch_enkf_analysis_smooth", c, n_params, params, d_param_inflation, n_series, series);
}

int sipnet_batch_get_params(sipnet_batch* b, double* params, int32_t file_units, void* hip_stream) {
  const char* name = "sipnet_batch_get_params";
  if (!b || !params) return refuse(name, "a NULL batch or params");
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  rc = orderBehindBusy(b, stream);
  if (rc) return rc;
  rc = flushParams(b, stream);
  if (rc) return rc;
  // the rows a column carries: its own, or those of the column its index names (in the bank of a connected filter)
  const bool indexed = b->prmIndexed;
  const double* src = indexed && b->d_prmBank ? b->d_prmBank : b->d_prm;
  const int64_t pitch = indexed && b->d_prmBank ? b->prmBankPitch : b->ncol, ncol = b->ncol;
  std::vector<double> rows((size_t)pitch * SIPNET_NPARAMS);
  std::vector<int32_t> id(indexed ? (size_t)ncol : 0);
  HIP_TRY(hipMemcpyAsync(rows.data(), src, rows.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (indexed) HIP_TRY(hipMemcpyAsync(id.data(), b->d_prmId, id.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int p = 0; p < SIPNET_NPARAMS; p++) {
    const bool rate = file_units && rateRow(p);
    for (int64_t c = 0; c < ncol; c++) {
      const double v = rows[(size_t)p * pitch + (indexed ? (int64_t)id[c] : c)];
      params[c * SIPNET_NPARAMS + p] = rate ? v * 365.0 : v;
    }
  }
  return SIPNET_OK;
}

int sipnet_enkf_local_schedule(int32_t n_sites, int32_t n_obs, const int64_t* nbr_ptr, const int32_t* nbr, const double* rho,
                               int32_t* level_of_slot, int32_t* n_levels) {
  if (!n_levels) return refuse("sipnet_enkf_local_schedule", "a NULL n_levels");
  std::vector<int32_t> level;
  int rc = localSchedule("sipnet_enkf_local_schedule", n_sites, n_obs, nbr_ptr, nbr, rho, level, n_levels);
  if (rc) return rc;
  if (level_of_slot) std::copy(level.begin(), level.end(), level_of_slot);
  return SIPNET_OK;
}

void sipnet_enkf_local_destroy(sipnet_enkf_local* L) {
  if (!L) return;
  (void)hipSetDevice(L->device);
  delete L;
}

int sipnet_batch_enkf_local_create(sipnet_batch* b, int32_t n_obs, const int64_t* nbr_ptr, const int32_t* nbr,
                                   const double* rho, sipnet_enkf_local** out) {
  const char* name = "sipnet_batch_enkf_local_create";
  if (!b || !out) return refuse(name, "a NULL batch or out");
  *out = nullptr;
  std::vector<int32_t> level;
  int32_t nLevels = 0;
  const int32_t nSites = b->n_sites;
  int rc = localSchedule(name, nSites, n_obs, nbr_ptr, nbr, rho, level, &nLevels);
  if (rc) return rc;
  rc = useDevice(b);
  if (rc) return rc;
  // the pairs sorted by level; within a level by slot in serial order, a slot's own site first
  std::vector<int64_t> levelOff((size_t)nLevels + 1, 0);
  for (int32_t s = 0; s < nSites; s++)
    for (int32_t i = 0; i < n_obs; i++) levelOff[(size_t)level[(size_t)s * n_obs + i] + 1] += 1 + (nbr_ptr[s + 1] - nbr_ptr[s]);
  for (int32_t l = 0; l < nLevels; l++) levelOff[l + 1] += levelOff[l];
  std::vector<LocalPair> pairs((size_t)levelOff[nLevels]);
  std::vector<int64_t> fill(levelOff.begin(), levelOff.end() - 1), slotOff((size_t)nSites * n_obs);
  std::vector<int32_t> slotLen((size_t)nSites * n_obs);
  for (int32_t s = 0; s < nSites; s++)
    for (int32_t i = 0; i < n_obs; i++) {
      int64_t& k = fill[level[(size_t)s * n_obs + i]];
      slotOff[(size_t)s * n_obs + i] = k;
      slotLen[(size_t)s * n_obs + i] = (int32_t)(1 + nbr_ptr[s + 1] - nbr_ptr[s]);
      pairs[(size_t)k++] = LocalPair{s, i, s, 1.0};
      for (int64_t e = nbr_ptr[s]; e < nbr_ptr[s + 1]; e++) pairs[(size_t)k++] = LocalPair{s, i, nbr[e], rho[e]};
    }
  // the in-neighbour lists: site t is reached from the sites that list it
  std::vector<int64_t> inPtr((size_t)nSites + 1, 0);
  for (int64_t e = 0; e < nbr_ptr[nSites]; e++) inPtr[(size_t)nbr[e] + 1]++;
  for (int32_t t = 0; t < nSites; t++) inPtr[t + 1] += inPtr[t];
  std::vector<int32_t> in((size_t)inPtr[nSites]);
  std::vector<double> inRho(in.size());
  std::vector<int64_t> at(inPtr.begin(), inPtr.end() - 1);
  for (int32_t s = 0; s < nSites; s++)
    for (int64_t e = nbr_ptr[s]; e < nbr_ptr[s + 1]; e++) {
      inRho[(size_t)at[nbr[e]]] = rho[e];
      in[(size_t)at[nbr[e]]++] = s;
    }
  const std::vector<int32_t> rows = localRows(nSites, n_obs, nbr_ptr, nbr);

  sipnet_enkf_local* L = new sipnet_enkf_local;
  L->b = b;
  L->device = b->device;
  L->nSites = nSites;
  L->nObs = n_obs;
  L->nLevels = nLevels;
  L->maxRows = *std::max_element(rows.begin(), rows.end());
  L->levelOff = std::move(levelOff);
  L->slotOff = std::move(slotOff);
  L->slotLen = std::move(slotLen);
  auto upload = [](auto& d, const auto& h) -> int {   // (an empty list: 8 bytes, not a null pointer)
    const size_t elem = sizeof(h[0]);
    RC_TRY(d.reserve(h.empty() ? (8 + elem - 1) / elem : h.size()));
    if (!h.empty()) HIP_TRY(hipMemcpy(d, h.data(), h.size() * elem, hipMemcpyHostToDevice));
    return 0;
  };
  if ((rc = upload(L->d_pair, pairs)) || (rc = upload(L->d_inPtr, inPtr)) || (rc = upload(L->d_in, in)) ||
      (rc = upload(L->d_inRho, inRho))) {
    sipnet_enkf_local_destroy(L);
    return rc;
  }
  *out = L;
  return SIPNET_OK;
}

int32_t sipnet_enkf_local_levels(const sipnet_enkf_local* L) { return L ? L->nLevels : 0; }

int sipnet_debug_enkf_local_serial(sipnet_enkf_local* L, int32_t on) {
  if (!L) return refuse("sipnet_debug_enkf_local_serial", "a NULL localization");
  L->serial = on != 0;
  return SIPNET_OK;
}

int sipnet_batch_enkf_analysis_local(sipnet_batch* b, const sipnet_enkf_local* L, int32_t n_obs, const sipnet_enkf_obs* ops,
                                     int32_t analysed_mask, const void* const d_planes[3], int32_t elem_is_f32,
                                     int32_t n_steps, int64_t ld, const double* d_obs, const double* d_sd,
                                     const double* d_inflation, int32_t* d_site_info, void* hip_stream) {
  const char* name = "sipnet_batch_enkf_analysis_local";
  int rc = localChecks(name, b, L, n_obs);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  const EnkfCall c{b, n_obs, ops, analysed_mask, d_planes, elem_is_f32, n_steps, ld, d_obs, d_sd, d_inflation, d_site_info, stream};
  EnkfArgs a;
  rc = enkfBegin(name, c, a);
  if (rc) return rc;
  rc = enkfScratch(b, b->d_enkf, a, d_site_info, /*workInGlobal=*/true, /*perChunk=*/true, /*withSrc=*/true, 0,
                   nullptr);
  if (rc) return rc;
  enkfFront(c, a, L);
  if (L->serial) {
    for (size_t k = 0; k < L->slotOff.size(); k++)
      hipLaunchKernelGGL(enkfLocalKernel, dim3((unsigned)L->slotLen[k]), dim3(256), 0, stream, a, L->d_pair, L->slotOff[k]);
  } else {
    for (int32_t l = 0; l < L->nLevels; l++)
      hipLaunchKernelGGL(enkfLocalKernel, dim3((unsigned)(L->levelOff[l + 1] - L->levelOff[l])), dim3(256), 0, stream, a,
                         L->d_pair, L->levelOff[l]);
  }
  return enkfEnd(c, a, /*perChunk=*/true, 0, 0);
}

int sipnet_enkf_local_rows(int32_t n_sites, int32_t n_obs, const int64_t* nbr_ptr, const int32_t* nbr, int32_t* rows_of_site,
                           int32_t* max_rows) {
  int rc = localLists("sipnet_enkf_local_rows", n_sites, n_obs, nbr_ptr, nbr, nullptr, false);
  if (rc) return rc;
  const std::vector<int32_t> rows = localRows(n_sites, n_obs, nbr_ptr, nbr);
  if (rows_of_site) std::copy(rows.begin(), rows.end(), rows_of_site);
  if (max_rows) *max_rows = *std::max_element(rows.begin(), rows.end());
  return SIPNET_OK;
}

int sipnet_batch_enkf_analysis_block(sipnet_batch* b, const sipnet_enkf_local* L, int32_t n_obs, const sipnet_enkf_obs* ops,
                                     int32_t analysed_mask, const void* const d_planes[3], int32_t elem_is_f32,
                                     int32_t n_steps, int64_t ld, const double* d_obs, const double* d_sd,
                                     const double* d_inflation, int32_t* d_site_info, int32_t* d_rows, void* hip_stream) {
  const char* name = "sipnet_batch_enkf_analysis_block";
  int rc = localChecks(name, b, L, n_obs);
  if (rc) return rc;
  if (L->maxRows > kBlockRows)
    return refuse(name, "a site has " + std::to_string(L->maxRows) + " rows (n_obs x (1 + in-neighbours)); at most " +
                            std::to_string(kBlockRows) + " (SIPNET_ENKF_BLOCK_MAX_ROWS, sipnet_enkf_local_rows)");
  hipStream_t stream = (hipStream_t)hip_stream;
  const EnkfCall c{b, n_obs, ops, analysed_mask, d_planes, elem_is_f32, n_steps, ld, d_obs, d_sd, d_inflation, d_site_info, stream};
  EnkfArgs a;
  rc = enkfBegin(name, c, a);
  if (rc) return rc;
  // the matrices of every target in LDS, where the staging tile was, when the largest fits beside the kernel's own LDS
  const size_t matDoubles = blockMatSize(a.nA, L->maxRows), stageDoubles = (size_t)kTile * blockStagePitch(a.nA, L->maxRows);
  const bool small = L->maxRows <= kBlockSmall && b->n_members <= 512;
  const void* ldsKernel = small ? (const void*)enkfBlockKernel<true, 256> : (const void*)enkfBlockKernel<true, 1024>;
  const size_t ldsWant = std::max(stageDoubles, matDoubles) * sizeof(double);
  bool useLds;
  rc = ldsGranted(ldsKernel, ldsWant, b->device, &useLds);
  if (rc) return rc;
  double* mat = nullptr;   // (a target's matrices in its block of the scratch, unless they are in LDS)
  rc = enkfScratch(b, b->d_enkf, a, d_site_info, /*workInGlobal=*/true, /*perChunk=*/true, /*withSrc=*/true,
                   useLds ? 0 : matDoubles, &mat);
  if (rc) return rc;
  enkfFront(c, a, L);
  const size_t dyn = useLds ? ldsWant : stageDoubles * sizeof(double);
  double* matArg = useLds ? nullptr : mat;
  const int64_t matPitch = useLds ? 0 : (int64_t)matDoubles;
  auto launch = [&](auto kernel, int threads) {
    hipLaunchKernelGGL(kernel, siteGrid(b), dim3(threads), dyn, stream, a, L->d_inPtr, L->d_in, L->d_inRho, matArg, matPitch,
                       d_rows);
  };
  if (small) launch(useLds ? enkfBlockKernel<true, 256> : enkfBlockKernel<false, 256>, 256);
  else launch(useLds ? enkfBlockKernel<true, 1024> : enkfBlockKernel<false, 1024>, 1024);
  return enkfEnd(c, a, /*perChunk=*/true, useLds ? 1 : 0, (int32_t)b->n_sites);
}

int32_t sipnet_enkf_moment_words(int32_t n_analysed_pools, int32_t n_obs) {
  if (n_analysed_pools < 1 || n_analysed_pools > kPools || n_obs < 1 || n_obs > kMaxObs) return -1;
  return shardWords(n_analysed_pools, n_obs);
}

int sipnet_batch_enkf_shard_moments(sipnet_batch* b, int32_t n_obs, const sipnet_enkf_obs* ops, int32_t analysed_mask,
                                    const void* const d_planes[3], int32_t elem_is_f32, int32_t n_steps, int64_t ld,
                                    double* d_moments, void* hip_stream) {
  const char* name = "sipnet_batch_enkf_shard_moments";
  if (!d_moments) return refuse(name, "a NULL d_moments");
  hipStream_t stream = (hipStream_t)hip_stream;
  const EnkfCall c{b, n_obs, ops, analysed_mask, d_planes, elem_is_f32, n_steps, ld, nullptr, nullptr, nullptr, nullptr, stream,
                   /*momentsOnly=*/true};
  EnkfArgs a;
  int rc = enkfBegin(name, c, a);
  if (rc) return rc;
  const int cap = a.nv * a.nObs, W = shardWords(a.nA, a.nObs);   // (part: a chunk's sums [nv], then its products [nv][n_obs])
  rc = enkfScratch(b, b->d_enkf, a, nullptr, /*workInGlobal=*/true, /*perChunk=*/true, /*withSrc=*/false, 0,
                   nullptr, cap);
  if (rc) return rc;
  const dim3 chunks = chunkGrid(b, a);
  const auto totals = [&](int entries) { return dim3((unsigned)b->n_sites, (unsigned)((entries + 3) / 4)); };
  hipLaunchKernelGGL((elem_is_f32 ? enkfLoadKernel<float, EnkfArgs> : enkfLoadKernel<double, EnkfArgs>), chunks, dim3(256), 0,
                     stream, a);
  hipLaunchKernelGGL(enkfShardSumKernel, chunks, dim3(256), 0, stream, a, cap);
  hipLaunchKernelGGL(enkfShardTotalKernel, totals(a.nv), dim3(256), 0, stream, a, cap, d_moments, W, 0);
  hipLaunchKernelGGL(enkfShardProductKernel, chunks, dim3(256), 0, stream, a, cap, (const double*)d_moments, W);
  hipLaunchKernelGGL(enkfShardTotalKernel, totals(cap), dim3(256), 0, stream, a, cap, d_moments, W, 1);
  HIP_TRY(hipGetLastError());
  return markBusy(b, stream);
}

int sipnet_batch_enkf_analysis_sharded(sipnet_batch* b, int32_t n_obs, const sipnet_enkf_obs* ops, int32_t analysed_mask,
                                       const void* const d_planes[3], int32_t elem_is_f32, int32_t n_steps, int64_t ld,
                                       const double* d_obs, const double* d_sd, const double* d_inflation, int32_t world,
                                       const double* d_gathered, int32_t* d_site_info, void* hip_stream) {
  const char* name = "sipnet_batch_enkf_analysis_sharded";
  if (world < 1 || world > 64) return refuse(name, "world must be 1..64");
  if (!d_gathered) return refuse(name, "a NULL d_gathered");
  hipStream_t stream = (hipStream_t)hip_stream;
  const EnkfCall c{b, n_obs, ops, analysed_mask, d_planes, elem_is_f32, n_steps, ld, d_obs, d_sd, d_inflation, d_site_info, stream};
  EnkfArgs a;
  int rc = enkfBegin(name, c, a);
  if (rc) return rc;
  const int64_t nSites = b->n_sites;
  const int W = shardWords(a.nA, a.nObs);
  if (!d_site_info) {   // the synchronous form: the blocks' counts are checked before anything is launched
    std::vector<double> counts((size_t)world * (size_t)nSites);
    HIP_TRY(hipMemcpy2DAsync(counts.data(), sizeof(double), d_gathered, (size_t)W * sizeof(double), sizeof(double), counts.size(),
                             hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int32_t r = 0; r < world; r++)
      for (int64_t s = 0; s < nSites; s++)
        if (!shardCountOk(counts[(size_t)r * nSites + s]))
          return refuse(name, "site " + std::to_string(s) + ": bad input (the count of rank " + std::to_string(r) +
                              "'s moment block is not an integer 0..4194304); nothing was written");
  }
  double* plan = nullptr;
  rc = enkfScratch(b, b->d_enkf, a, d_site_info, /*workInGlobal=*/true, /*perChunk=*/true, /*withSrc=*/false,
                   kShardPlan, &plan);
  if (rc) return rc;
  hipLaunchKernelGGL((elem_is_f32 ? enkfLoadKernel<float, EnkfArgs> : enkfLoadKernel<double, EnkfArgs>), chunkGrid(b, a), dim3(256),
                     0, stream, a);
  hipLaunchKernelGGL(enkfShardChainKernel, siteGrid(b), dim3(256), 0, stream, a, d_gathered, world, nSites, W, plan);
  hipLaunchKernelGGL(enkfShardApplyKernel, chunkGrid(b, a), dim3(256), 0, stream, a, (const double*)plan);
  return enkfEnd(c, a, /*perChunk=*/true, 0, 0);
}

}  // extern "C"
