// pf.hip -- particle-filter analysis step for an ensemble batch (BASELINE config C5,
// SURVEY.md 8(e) "PF extra exchange"): likelihood weights from an output plane, systematic
// resampling over the GLOBAL particle set, and the column gathers that move member state
// (carried state vector + running-mean ring, optionally the converted parameters) inside a
// GPU and into / out of the packed blocks that travel between GPUs.
//
// The reference has no particle filter (PEcAn drives one process per particle and copies
// restart files between cycles, docs/developer-guide/restart-checkpoint.md); what a cycle
// exchanges there is exactly a member's checkpoint, which is what these kernels move.
//
// All gather kernels are HBM-bound column gathers over SoA matrices [rows][ncol]: thread = column,
// blockIdx.y = row, so reads of the index vector and writes are coalesced; after systematic
// resampling ancestors are non-decreasing, so the gathered reads are near-coalesced too.
//
// This file is the one translation unit (the one tools/build_variants.py compiles with -DSIPNET_PF_*) and the host side; the
// device code is in parts, each with its own header comment, included below in this order: site_device.h (the sums in their
// one order, a member's limits, the listed and derived rows, shared with enkf.hip), pf_gather.inc, pf_weights.inc,
// pf_fused.inc, pf_plan.inc, pf_sites.inc, pf_series.inc, pf_random.inc, pf_rejuvenate.inc, pf_metropolis.inc, pf_temper.inc.
// Refusals, the bookkeeping of a call that writes the batch, the scratch blocks' growth and carving and the synchronous forms'
// copies are site_host.h's.
//
// The host side runs three filters.  One batch (sipnet_batch_pf_analysis): takePfPre, the one launch (fusedSetup) or the
// launches of their own, checkTotal, the resampling gather (resampleColumns).  Many sites (sipnet_batch_pf_analysis_sites, and
// sipnet_batch_pf_resample_sites from given log-weights): sitesBegin, the weights' source, sitesFinish.  Across ranks by peer
// reads: sipnet_batch_pf_publish, _connect (mapPeer, fillBank) and _resample_peers (peerTable, peerAncestors, peerGather).
// Beside them the series weights (sipnet_batch_series_loglik) and, their host side in pf_moves.inc (included behind it), the
// rejuvenation (sipnet_batch_pf_rejuvenate), the Metropolis move over members (sipnet_batch_mcmc_propose, sipnet_batch_mcmc_accept)
// and the tempering exponent that keeps an effective sample size (sipnet_batch_pf_temper_sites).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <unistd.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/sipnet_amd.h"
#include "batch_impl.h"
#include "site_host.h"

namespace sipnet {
namespace {

#include "site_device.h"
#include "pf_gather.inc"
#include "pf_weights.inc"
#include "pf_fused.inc"
#include "pf_plan.inc"
#include "pf_sites.inc"
#include "pf_series.inc"
#include "pf_random.inc"
#include "pf_rejuvenate.inc"
#include "pf_metropolis.inc"
#include "pf_temper.inc"

}  // namespace
}  // namespace sipnet

using namespace sipnet;

// Host side of PeerPtrs: for each of the two buffers a batch's checkpoint matrices alternate between (a resampling
// gathers into the spare and swaps), where every rank keeps them.  All ranks resample in lockstep, so the local
// parity says which buffer is current everywhere.
struct PfPeers {
  int32_t world = 1, rank = 0, nmax = 0, withParams = 0;
  int64_t nTotal = 0, first = 0;       // particles of all ranks; global index of this rank's first particle
  int32_t count[kMaxPeers] = {};
  const double* state[2][kMaxPeers] = {};
  const void* ring[2][kMaxPeers] = {};
  const double* prm[2][kMaxPeers] = {};
  const int32_t* ids[2][kMaxPeers] = {};   // byIndex: the particles' index into the replicated parameter bank
  bool byIndex = false;                // all ranks' parameters are in sipnet_batch::d_prmBank; particles carry an index
  bool bankLost = false;               // ... and this batch has since changed its parameters or moved rows: connect again
  std::vector<void*> opened;           // hipIpcOpenMemHandle mappings, closed on release
  int parity = 0;
};
// a connection goes: its hipIpcOpenMemHandle mappings are closed, the table is freed (null: nothing)
static void closePeers(PfPeers* pp) {
  if (!pp) return;
  for (void* p : pp->opened) (void)hipIpcCloseMemHandle(p);
  delete pp;
}

// the connection's parameter bank is no longer what the particles' indices mean (new parameters were set, or a resampling
// moved parameter ROWS): the batch goes back to its own column-order block
void pfDropBank(sipnet_batch* b) {
  if (!b->d_prmBank) return;
  (void)hipDeviceSynchronize();
  (void)b->d_prmBank.release();
  b->prmBankPitch = 0;
  b->prmIndexed = false;
  if (b->pfPeers) b->pfPeers->bankLost = true;
}

// The second copies a resampling gathers into before it swaps (batch_impl.h), made on first use: state and ring, the
// parameter rows, the particles' parameter index (both copies of it)
static int ensureSpares(sipnet_batch* b, bool state, bool params, bool index) {
  const size_t nc = (size_t)b->ncol;
  if (state) {
    RC_TRY(b->d_state2.reserve(nc * SIPNET_NSTATE));
    RC_TRY(b->d_ring2.reserve(ringDoubles(b)));
  }
  if (params) RC_TRY(b->d_prm2.reserve(nc * SIPNET_NPARAMS));
  if (index) {
    RC_TRY(b->d_prmId.reserve(nc));
    RC_TRY(b->d_prmId2.reserve(nc));
  }
  return SIPNET_OK;
}

// The parameter bank back in column order (batch_impl.h): gather through the index into the spare, swap.
int materializeParams(sipnet_batch* b, hipStream_t stream) {
  if (!b->prmIndexed) return SIPNET_OK;
  {   // (the last launch may have run on another stream)
    int rcO = orderBehindBusy(b, stream);
    if (rcO) return rcO;
  }
  GatherCall g;   // dst column j <- source column d_prmId[j]
  g.src = b->d_prmId;
  g.nOut = g.dstPitch = b->ncol;
  g.stream = stream;
  // a connected filter: the rows out of the bank of all ranks' parameters into d_prm, the index stays what it is; else out of
  // d_prm into the spare, and swap
  const bool bank = (bool)b->d_prmBank;
  if (!bank) RC_TRY(ensureSpares(b, /*state=*/false, /*params=*/true, /*index=*/false));
  g.prm = bank ? b->d_prmBank.get() : b->d_prm.get();
  g.ncol = bank ? b->prmBankPitch : b->ncol;
  g.dPrm = bank ? b->d_prm.get() : b->d_prm2.get();
  launchGatherMember(g);
  HIP_TRY(hipGetLastError());
  if (!bank) std::swap(b->d_prm, b->d_prm2);
  b->prmIndexed = false;
  return markBusy(b, stream);
}

// What follows a resampling gather into the spares: the copies it wrote become the current ones -- state and ring, and the
// parameter index or the parameter rows if they moved -- and a connected batch's peers find them under the other parity
// (connected ranks resample in lockstep, whichever entry point they use)
static void adoptSpares(sipnet_batch* b, bool index, bool rows) {
  std::swap(b->d_state, b->d_state2);
  std::swap(b->d_ring, b->d_ring2);
  if (index) std::swap(b->d_prmId, b->d_prmId2);
  else if (rows) std::swap(b->d_prm, b->d_prm2);
  if (b->pfPeers) b->pfPeers->parity ^= 1;
}

#ifdef SIPNET_PF_STAMPS
extern "C" int sipnet_debug_read_pf_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pfStamps), 8 * sizeof(unsigned long long));
}
#endif

extern "C" {

int32_t sipnet_pf_member_words(int32_t with_params) {
  return SIPNET_NSTATE + SIPNET_RING_SLOTS + (with_params ? SIPNET_NPARAMS : 0);
}

int32_t sipnet_batch_member_words(const sipnet_batch* b, int32_t with_params) {
  if (!b) return -1;
  return SIPNET_NSTATE + ringWords(b->precision == SIPNET_F32_MIXED) + (with_params ? SIPNET_NPARAMS : 0);
}

// d_part (optional, DEVICE, one double per 256 columns): the blocks' maxima, for the resampling that follows
// (npad >= ncol: log-weight slots to fill, the ones past the batch's particles with -inf)
static int logWeights(sipnet_batch* b, const void* d_plane, int32_t elem_is_f32, int32_t n_steps, int64_t ld,
                      double obs, double sigma, double* d_logw, double* d_part, void* hip_stream, int64_t npad = 0) {
  if (!b || !d_plane || !d_logw || n_steps <= 0 || ld < b->ncol || !(sigma > 0))
    return refuse("sipnet_batch_pf_log_weights", "bad argument");
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  if (npad < b->ncol) npad = b->ncol;
  const int grid = (int)((npad + 255) / 256);
  const double* status = b->d_state + (size_t)ST_status * b->ncol;
  if (elem_is_f32) {
    hipLaunchKernelGGL(logWeightKernel<float>, dim3(grid), dim3(256), 0, stream,
                       (const float*)d_plane, n_steps, ld, b->ncol, status, obs, 1.0 / sigma, d_logw, d_part, npad);
  } else {
    hipLaunchKernelGGL(logWeightKernel<double>, dim3(grid), dim3(256), 0, stream,
                       (const double*)d_plane, n_steps, ld, b->ncol, status, obs, 1.0 / sigma, d_logw, d_part, npad);
  }
  HIP_TRY(hipGetLastError());
  return SIPNET_OK;
}

extern "C" int sipnet_batch_pf_log_weights(sipnet_batch* b, const void* d_plane, int32_t elem_is_f32,
                                           int32_t n_steps, int64_t ld, double obs, double sigma,
                                           double* d_logw, void* hip_stream) {
  return logWeights(b, d_plane, elem_is_f32, n_steps, ld, obs, sigma, d_logw, nullptr, hip_stream);
}

// scratch of the resampling, kept between calls: one per batch for the sipnet_batch_pf_* entry points (it goes with the
// batch), one per host thread for the batch-less sipnet_pf_* ones (sipnet_pf_release_scratch)
struct PfScratch {
  int device = -1;
  DevBuf<double> d_max;    // partial maxima of the log-weights (one per 256 weights at most)
  DevBuf<int64_t> d_w;     // [n]: its capacity is the number of weights the scratch was made for
  DevBuf<int64_t> d_cdf;
  DevBuf<unsigned char> d_tmp;
  size_t tmpBytes = 0;
  // the one-launch analysis (pfFusedKernel): chunk totals + the total weight, the ring of per-launch barrier sets (all
  // zero at allocation; launch L uses set L % kBarSets and clears set (L + kBarAhead) % kBarSets), the stuck report
  DevBuf<int64_t> d_blockSum;      // [kFusedBlocks] + 1: the total
  DevBuf<int64_t> d_threadIncl;    // [kFusedBlocks][256]
  DevBuf<unsigned long long> d_barrier;   // [kBarSets][kBarSetWords] + 1: the stuck word
  unsigned long long launches = 0;      // fused launches that were accepted by the runtime
  int occ[3] = {-1, -1, -1};            // resident workgroups per CU of pfFusedKernel<float,false> / <double,false> / <double,true>
  DevBuf<unsigned char> d_sites;        // sipnet_batch_pf_analysis_sites (sitesScratchFor), bytes
  DevBuf<double> d_loglik;              // sipnet_batch_series_loglik, path 2: [terms' tiles][ncol] the tiles' sums
  DevBuf<int32_t> d_loglikUsed;         // ... and [n_sites][terms' tiles] the tiles' rows used
  DevBuf<unsigned char> d_rejuv;        // sipnet_batch_pf_rejuvenate (rejScratch), bytes
  DevBuf<unsigned char> d_mcmc;         // sipnet_batch_mcmc_propose / _accept (mcScratch), bytes
  DevBuf<unsigned char> d_temper;       // sipnet_batch_pf_temper_sites, per-chunk path (temperScratch), bytes
};
namespace {
constexpr int kMaxParts = 256;
constexpr size_t kBarrierWords = (size_t)kBarSets * kBarSetWords + 1;   // + the stuck word
// the host thread's scratch: a heap object behind a raw pointer that only sipnet_pf_release_scratch deletes -- a thread_local
// OBJECT's destructor would free at thread exit, possibly after the HIP runtime is gone
thread_local PfScratch* g_pf = nullptr;
PfScratch* threadScratch() {
  if (!g_pf) g_pf = new PfScratch();
  return g_pf;
}
}  // namespace

// scratch for n weights (the partial maxima: one per 256 of them at most)
static int pfScratchFor(PfScratch& sc, int64_t n, hipStream_t stream) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (sc.device != dev || (int64_t)sc.d_w.capacity() < n) {
    sc = PfScratch();   // (everything goes, the many-site block too; d_w, whose capacity says "made", comes last)
    sc.device = dev;
    RC_TRY(sc.d_max.reserve((size_t)((n + 255) / 256 + kMaxParts)));
    RC_TRY(sc.d_cdf.reserve((size_t)n));
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, sc.tmpBytes, (int64_t*)nullptr, sc.d_cdf.get(), (int)n, stream));
    RC_TRY(sc.d_tmp.reserve(sc.tmpBytes));
    RC_TRY(sc.d_blockSum.reserve((size_t)(kFusedBlocks + 1)));
    RC_TRY(sc.d_threadIncl.reserve((size_t)kFusedBlocks * 256));
    RC_TRY(sc.d_barrier.reserve(kBarrierWords));
    HIP_TRY(hipMemsetAsync(sc.d_barrier, 0, kBarrierWords * sizeof(unsigned long long), stream));
    RC_TRY(sc.d_w.reserve((size_t)n));
  }
  return SIPNET_OK;
}
// How many workgroups of the one-launch analysis may spin at its barriers at once: what the device holds
// (hipOccupancyMaxActiveBlocksPerMultiprocessor x its CUs -- the batch's numCUs: a partitioned device reports its own) over
// the number of filters that may analyse on this device at the same time (sipnet_batch_set_device_share: a node's shards on
// one device), at most kFusedBlocks.  which: 0 pfFusedKernel<float, false>, 1 <double, false>, 2 <double, true>.
static int fusedBudget(PfScratch& sc, const sipnet_batch* b, int which) {
  if (sc.occ[which] < 0) {
    int occ = 0;
    hipError_t e = which == 0   ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, pfFusedKernel<float, false>, 256, 0)
                   : which == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, pfFusedKernel<double, false>, 256, 0)
                                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, pfFusedKernel<double, true>, 256, 0);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      occ = 0;   // (unknown: the multi-launch path)
    }
    sc.occ[which] = occ;
  }
  const int64_t share = b->deviceShare > 0 ? b->deviceShare : 1;
  const int64_t fit = (int64_t)sc.occ[which] * b->numCUs / share;
  return (int)(fit < kFusedBlocks ? fit : kFusedBlocks);
}
// may the analysis over nSlots weights be ONE launch of at most `budget` resident workgroups?
static bool fusable(int64_t nSlots, int budget) {
  return budget >= kFusedMinBlocks && (nSlots + 255) / 256 <= (int64_t)budget * kFusedMaxPer;
}
// geometry of the one-launch analysis over nSlots weights with at most `budget` workgroups: contiguous chunks of whole tiles
static void fusedGeometry(int64_t nSlots, int budget, int* grid, int64_t* chunk) {
  const int64_t tiles = (nSlots + 255) / 256;
  const int64_t nb = tiles < budget ? tiles : budget;
  const int64_t tilesPer = (tiles + nb - 1) / nb;
  *chunk = tilesPer * 256;
  *grid = (int)((nSlots + *chunk - 1) / *chunk);
}
// this launch's barrier set and the one it clears for a later launch; fusedLaunched() once the runtime has accepted the launch
static void fusedBarrier(PfScratch& sc, FusedArgs* fa, int spinBudget) {
  fa->barrier = sc.d_barrier + (size_t)(sc.launches % kBarSets) * kBarSetWords;
  fa->barrierAhead = sc.d_barrier + (size_t)((sc.launches + kBarAhead) % kBarSets) * kBarSetWords;
  fa->stuck = sc.d_barrier + (size_t)kBarSets * kBarSetWords;
  fa->spinBudget = spinBudget > 0 ? spinBudget : SIPNET_PF_SPIN_BUDGET;
}
// a launch the runtime refused has not touched its set (nor cleared the one ahead): the next one takes the same set
static int fusedLaunched(PfScratch& sc) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return refuse("pfFusedKernel", hipGetErrorString(e), SIPNET_ERR_INTERNAL);
  sc.launches++;
  return SIPNET_OK;
}
// the report a void launch left (gridBarrier), for the error message; clears it
static std::string fusedStuckReport(PfScratch& sc, hipStream_t stream) {
  unsigned long long rep = 0;
  unsigned long long* d = sc.d_barrier + (size_t)kBarSets * kBarSetWords;
  if (hipMemcpyAsync(&rep, d, sizeof rep, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
    (void)hipGetLastError();
    return "the analysis kernel's grid barrier gave up";
  }
  (void)hipMemsetAsync(d, 0, sizeof rep, stream);
  return "the analysis kernel's grid barrier gave up (barrier " + std::to_string((unsigned)((rep >> 32) & 0x7fffffffu)) + ", workgroup " +
         std::to_string((unsigned)(rep & 0xffffffffu)) + "): its workgroups were not all resident -- another kernel held the device, or more filters "
         "analyse on it at once than sipnet_batch_set_device_share says; the launch's results are void";
}
static PfScratch& scratchOf(sipnet_batch* b) {
  if (!b->pfScratch) b->pfScratch = new PfScratch();
  return *b->pfScratch;
}
// What both one-launch analyses ask of the scratch block.  Decides whether the analysis over nSlots weights is ONE launch
// (which: fusedBudget's), records that, the budget and the grid in pfInfo, and if it is, fills what does not depend on the
// caller: geometry, the exchange areas, this launch's barrier set, the absent hook (spent here), where the total goes.
static bool fusedSetup(sipnet_batch* b, PfScratch& sc, int which, int64_t nSlots, FusedArgs* fa, int* grid) {
  const int budget = (b->kernelOptions & SIPNET_KOPT_PF_MULTI_LAUNCH) ? 0 : fusedBudget(sc, b, which);
  b->pfInfo.fused = fusable(nSlots, budget) ? 1 : 0;
  b->pfInfo.budget = budget;
  b->pfInfo.grid = 0;
  if (!b->pfInfo.fused) return false;
  fa->nSlots = nSlots;
  fusedGeometry(nSlots, budget, grid, &fa->chunk);
  b->pfInfo.grid = *grid;
  fa->blockMax = sc.d_max;
  fa->threadIncl = sc.d_threadIncl;
  fa->blockSum = sc.d_blockSum;
  fusedBarrier(sc, fa, b->pfSpinBudget);
  fa->absent = b->pfDebugAbsent;
  b->pfDebugAbsent = -1;
  fa->totalScratch = sc.d_blockSum + kFusedBlocks;
  return true;
}
// The one host round trip of an analysis whose caller did not ask for the total on the device: a filter with no surviving
// particle must be reported, and so must a void launch (what its barrier left: fusedStuckReport).  who: the entry point.
static int checkTotal(PfScratch& sc, const int64_t* d_total, const char* who, hipStream_t stream) {
  int64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (total == kPfVoid) return refuse(who, fusedStuckReport(sc, stream), SIPNET_ERR_INTERNAL);
  if (total <= 0) return refuse(who, "every particle has zero weight", SIPNET_ERR_BAD_PARAMETER);
  return SIPNET_OK;
}
// Has the forecast's own launch left the log-weights of exactly this plane, observation and sigma in d_logw
// (sipnet_batch_pf_arm)?  Asked once: whatever it left is spent.  Then pfPre.nMax maxima are in d_pfPreMax.
static bool takePfPre(sipnet_batch* b, const void* d_plane, int32_t elem_is_f32, int32_t n_steps, int64_t ld, double obs,
                      double sigma, const double* d_logw) {
  const sipnet_batch::PfPre& pre = b->pfPre;
  const bool have = pre.valid && pre.plane == d_plane && pre.nSteps == n_steps && pre.ld == ld && pre.obs == obs &&
                    pre.sigma == sigma && pre.d_logw == d_logw && elem_is_f32 == (b->precision == SIPNET_F32_MIXED);
  b->pfPre.valid = false;
  return have;
}

// partsGiven > 0: the partial maxima of d_logw are in the scratch block already (logWeights put them there)
// (partPtr: where those maxima are, when not in the scratch block)
static int ancestorsImpl(PfScratch& sc, const double* d_logw, int64_t n, double u0, int32_t* d_ancestors,
                         int64_t* d_fixed_weights, int64_t* d_total, int partsGiven, void* hip_stream,
                         const double* partPtr = nullptr) {
  if (!d_logw || !d_ancestors || n <= 0 || n > kMaxColumns || !(u0 >= 0.0) || !(u0 < 1.0))
    return refuse("sipnet_pf_systematic_ancestors", "bad argument (n <= 4194304, 0 <= u0 < 1)");
  hipStream_t stream = (hipStream_t)hip_stream;
  int rc = pfScratchFor(sc, n, stream);
  if (rc) return rc;
  const int grid = (int)((n + 255) / 256);
  int parts = partsGiven;
  if (parts <= 0) {
    parts = grid < kMaxParts ? grid : kMaxParts;
    hipLaunchKernelGGL(maxPartialKernel, dim3(parts), dim3(256), 0, stream, d_logw, n, sc.d_max);
  }
  hipLaunchKernelGGL(fixedWeightKernel, dim3(grid), dim3(256), 0, stream, d_logw, n, partPtr ? partPtr : sc.d_max, parts, sc.d_w);
  size_t tmpBytes = sc.tmpBytes;
  HIP_TRY(hipcub::DeviceScan::InclusiveSum(sc.d_tmp, tmpBytes, sc.d_w.get(), sc.d_cdf.get(), (int)n, stream));
  hipLaunchKernelGGL(ancestorKernel, dim3(grid), dim3(256), 0, stream, sc.d_cdf, n, (int64_t)0, n, n, u0, d_ancestors,
                     d_total);
  HIP_TRY(hipGetLastError());
  if (d_fixed_weights)
    HIP_TRY(hipMemcpyAsync(d_fixed_weights, sc.d_w, (size_t)n * sizeof(int64_t),
                           hipMemcpyDeviceToDevice, stream));
  return SIPNET_OK;
}

extern "C" int sipnet_pf_systematic_ancestors_async(const double* d_logw, int64_t n, double u0,
                                                    int32_t* d_ancestors, int64_t* d_fixed_weights,
                                                    int64_t* d_total, void* hip_stream) {
  return ancestorsImpl(*threadScratch(), d_logw, n, u0, d_ancestors, d_fixed_weights, d_total, 0, hip_stream);
}

int sipnet_pf_systematic_ancestors(const double* d_logw, int64_t n, double u0,
                                   int32_t* d_ancestors, int64_t* d_fixed_weights,
                                   void* hip_stream) {
  int rc = sipnet_pf_systematic_ancestors_async(d_logw, n, u0, d_ancestors, d_fixed_weights,
                                                nullptr, hip_stream);
  if (rc) return rc;
  // (the total is the last entry of the prefix sum: never negative, so never a void launch's)
  PfScratch& sc = *threadScratch();
  return checkTotal(sc, sc.d_cdf + (n - 1), "sipnet_pf_systematic_ancestors", (hipStream_t)hip_stream);
}

namespace {
struct PlanScratch {
  int device = -1;
  DevBuf<int32_t> d_head, d_P;           // [total]; d_P's capacity is the total the scratch was made for
  DevBuf<int64_t> d_first, d_counts;     // [(kMaxWorld+1)*kMaxWorld], [4*kMaxWorld]
  DevBuf<unsigned char> d_tmp;
  size_t tmpBytes = 0;
};
thread_local PlanScratch* g_plan = nullptr;   // (a heap object, see g_pf)
}  // namespace

int sipnet_pf_exchange_plan(const int32_t* d_ancestors, int64_t n_local, int32_t world, int32_t rank,
                            int32_t* d_send_cols, int32_t* d_src, int64_t* send_counts,
                            int64_t* recv_counts, void* hip_stream) {
  if (!d_ancestors || !d_send_cols || !d_src || !send_counts || !recv_counts || n_local <= 0 ||
      world < 1 || world > kMaxWorld || rank < 0 || rank >= world ||
      n_local * world > (int64_t)1 << 30)
    return refuse("sipnet_pf_exchange_plan", "bad argument (world <= 64)");
  hipStream_t stream = (hipStream_t)hip_stream;
  const int64_t total = n_local * world;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (!g_plan) g_plan = new PlanScratch();
  PlanScratch& sc = *g_plan;
  if (sc.device != dev || (int64_t)sc.d_P.capacity() < total) {
    sc = PlanScratch();   // (d_P, whose capacity says "made", comes last)
    sc.device = dev;
    RC_TRY(sc.d_head.reserve((size_t)total));
    RC_TRY(sc.d_first.reserve((size_t)(kMaxWorld + 1) * kMaxWorld));
    RC_TRY(sc.d_counts.reserve((size_t)(4 * kMaxWorld + 1)));   // counts, bases, validity flag
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, sc.tmpBytes, sc.d_head.get(), (int32_t*)nullptr, (int)total, stream));
    RC_TRY(sc.d_tmp.reserve(sc.tmpBytes));
    RC_TRY(sc.d_P.reserve((size_t)total));
  }
  const int grid = (int)((total + 255) / 256);
  hipLaunchKernelGGL(planFirstKernel, dim3(world), dim3(kMaxWorld + 1), 0, stream, d_ancestors, n_local,
                     world, sc.d_first);
  int32_t* d_bad = (int32_t*)(sc.d_counts + 4 * kMaxWorld);
  HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(int64_t), stream));
  hipLaunchKernelGGL(planHeadKernel, dim3(grid), dim3(256), 0, stream, d_ancestors, n_local, total, sc.d_head, d_bad);
  size_t tmpBytes = sc.tmpBytes;
  HIP_TRY(hipcub::DeviceScan::ExclusiveSum(sc.d_tmp, tmpBytes, sc.d_head.get(), sc.d_P.get(), (int)total, stream));
  int64_t* d_bases = sc.d_counts + 2 * kMaxWorld;
  hipLaunchKernelGGL(planCountKernel, dim3(1), dim3(64), 0, stream, sc.d_first, sc.d_P, sc.d_head, total,
                     world, rank, sc.d_counts, d_bases);
  hipLaunchKernelGGL(planFillKernel, dim3(grid), dim3(256), 0, stream, d_ancestors, n_local, total, world,
                     rank, sc.d_first, sc.d_P, sc.d_head, d_bases, d_send_cols, d_src, d_bad);
  HIP_TRY(hipGetLastError());
  // the one host round trip of the plan: the split sizes of the all-to-all
  int64_t h[4 * kMaxWorld + 1];
  HIP_TRY(hipMemcpyAsync(h, sc.d_counts, (size_t)(4 * kMaxWorld + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (h[4 * kMaxWorld] != 0)
    return refuse("sipnet_pf_exchange_plan", "the ancestor vector is not non-decreasing inside [0, world * n_local)");
  for (int q = 0; q < world; q++) {
    send_counts[q] = h[q];
    recv_counts[q] = h[world + q];
  }
  return SIPNET_OK;
}

void sipnet_pf_release_scratch(void) {
  delete g_pf;
  g_pf = nullptr;
  delete g_plan;
  g_plan = nullptr;
}

int sipnet_batch_pack_members(sipnet_batch* b, const int32_t* d_cols, int64_t n,
                              int32_t with_params, double* d_buf, void* hip_stream) {
  if (!b || n < 0 || (n > 0 && (!d_cols || !d_buf)))
    return refuse("sipnet_batch_pack_members", "bad argument");
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  rc = flushParams(b, stream);
  if (rc) return rc;
  // block layout: [NSTATE rows | RING_SLOTS rows (fp32-mixed batches: of floats) | NPARAMS rows] x n columns
  GatherCall g;
  g.state = b->d_state;
  g.ring = b->d_ring;
  g.ringF32 = b->precision == SIPNET_F32_MIXED;
  g.prm = with_params ? b->d_prm.get() : nullptr;
  g.ncol = b->ncol;
  g.src = d_cols;
  g.nOut = g.dstPitch = n;
  g.dState = d_buf;
  g.dRing = d_buf + (size_t)SIPNET_NSTATE * n;
  g.dPrm = d_buf + (size_t)(SIPNET_NSTATE + ringWords(g.ringF32)) * n;
  g.prmRemap = b->prmIndexed ? b->d_prmId.get() : nullptr;   // (a resampled index: the rows are read through it)
  g.stream = stream;
  launchGatherMember(g);
  HIP_TRY(hipGetLastError());
  return SIPNET_OK;
}

// resampleColumns, the parameters before the gather.  Every particle is here and carries its parameters (byIndex): they stay
// where set_params put them, an index is resampled (4 bytes per particle instead of 640; the one-wave forecast kernel reads
// through it).  With blocks received from other ranks the rows themselves travel, as before.
static int settleParams(sipnet_batch* b, bool withParams, bool byIndex, hipStream_t stream) {
  if (withParams && !byIndex) {
    int rc = materializeParams(b, stream);
    if (rc) return rc;
    pfDropBank(b);   // (parameter ROWS are about to move: the connection's index means nothing afterwards)
    RC_TRY(ensureSpares(b, /*state=*/false, /*params=*/true, /*index=*/false));
  }
  if (byIndex) {
    RC_TRY(ensureSpares(b, /*state=*/false, /*params=*/false, /*index=*/true));
    if (b->d_prmBank) {
      b->prmIndexed = true;   // (a connected filter's index is always current: slots of the bank)
    } else if (!b->prmIndexed) {
      const int64_t nc = b->ncol;
      hipLaunchKernelGGL(iotaKernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, stream, b->d_prmId, nc);
      b->prmIndexed = true;
    }
  }
  return SIPNET_OK;
}
// resampleColumns, where the received columns are: n_blocks packed blocks of block_cols[s] columns x words rows, one behind
// the other in d_recv
static int recvMapOf(int32_t n_blocks, const int64_t* block_cols, int words, const double* d_recv, RecvMap* map) {
  map->nBlocks = n_blocks;
  int64_t start = 0, off = 0;
  for (int s = 0; s < n_blocks; s++) {
    if (block_cols[s] < 0)
      return refuse("sipnet_batch_resample", "negative block size");
    map->start[s] = start;
    map->off[s] = off;
    map->n[s] = block_cols[s];
    start += block_cols[s];
    off += block_cols[s] * words;
  }
  map->start[n_blocks] = start;
  if (start > 0 && !d_recv)
    return refuse("sipnet_batch_resample", "received columns announced but no buffer given");
  return SIPNET_OK;
}
// resampleColumns, after the gather: parameters that arrived from other ranks may change which kernel variant the batch
// needs (one host round trip)
static int widenExponents(sipnet_batch* b, hipStream_t stream) {
  DevBuf<int32_t> d_flag;
  RC_TRY(d_flag.reserve(1));
  HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), stream));
  hipLaunchKernelGGL(exponentCheckKernel, dim3((unsigned)((b->ncol + 255) / 256)), dim3(256), 0,
                     stream, b->d_prm, b->ncol, d_flag);
  int32_t flag = 0;
  HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(d_flag.release());
  if (flag != 0) b->genericExponents = true;  // only ever widened: plain-exponent kernels must never see a general exponent
  return SIPNET_OK;
}

// sipnet_batch_resample's gather without its one-site check (sipnet_batch_pf_analysis_sites: ancestors that never leave
// their site's columns)
static int resampleColumns(sipnet_batch* b, const int32_t* d_src, const double* d_recv, int32_t n_blocks,
                           const int64_t* block_cols, int32_t with_params, void* hip_stream) {
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  b->pfPre.valid = false;   // (a forecast's log-weights belong to the particles as they were)
  b->pfArm.set = false;
  rc = flushParams(b, stream);
  if (rc) return rc;
  RC_TRY(ensureSpares(b, /*state=*/true, /*params=*/false, /*index=*/false));
  const bool byIndex = with_params && n_blocks == 0;
  if (b->d_prmBank && !with_params)
    return refuse("sipnet_batch_resample", "this batch is connected to a filter whose particles carry their parameters "
                  "(sipnet_batch_pf_connect): resample with_params");
  rc = settleParams(b, with_params != 0, byIndex, stream);
  if (rc) return rc;
  GatherCall g;
  rc = recvMapOf(n_blocks, block_cols, sipnet_batch_member_words(b, with_params), d_recv, &g.map);
  if (rc) return rc;
  g.state = b->d_state;
  g.ring = b->d_ring;
  g.ringF32 = b->precision == SIPNET_F32_MIXED;
  g.prm = (with_params && !byIndex) ? b->d_prm.get() : nullptr;
  g.recv = d_recv;
  g.src = d_src;
  g.ncol = g.nOut = g.dstPitch = b->ncol;
  g.dState = b->d_state2;
  g.dRing = b->d_ring2;
  g.dPrm = b->d_prm2;
  g.idOld = byIndex ? b->d_prmId.get() : nullptr;
  g.idNew = byIndex ? b->d_prmId2.get() : nullptr;
  g.stream = stream;
  launchGatherMember(g);
  HIP_TRY(hipGetLastError());
  adoptSpares(b, byIndex, with_params != 0);
  rc = markBusy(b, stream);   // (an upload of new parameters waits for the gather that is writing them)
  if (rc) return rc;
  if (with_params && g.map.start[n_blocks] > 0) return widenExponents(b, stream);
  return SIPNET_OK;
}

int sipnet_batch_resample(sipnet_batch* b, const int32_t* d_src, const double* d_recv,
                          int32_t n_blocks, const int64_t* block_cols, int32_t with_params,
                          void* hip_stream) {
  if (!b || !d_src || n_blocks < 0 || n_blocks > kMaxBlocks || (n_blocks > 0 && !block_cols))
    return refuse("sipnet_batch_resample", "bad argument");
  if (b->n_sites != 1)
    return refuse("sipnet_batch_resample", "particles of different sites must not mix (n_sites must be 1)");
  return resampleColumns(b, d_src, d_recv, n_blocks, block_cols, with_params, hip_stream);
}

int sipnet_batch_pf_analysis(sipnet_batch* b, const void* d_plane, int32_t elem_is_f32, int32_t n_steps,
                             int64_t ld, double obs, double sigma, double u0, int32_t with_params,
                             double* d_logw, int32_t* d_ancestors, int64_t* d_total, void* hip_stream) {
  if (!b || !d_logw || !d_ancestors)
    return refuse("sipnet_batch_pf_analysis", "bad argument");
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  PfScratch& sc = scratchOf(b);
  rc = pfScratchFor(sc, b->ncol, stream);
  if (rc) return rc;
  if (!d_plane || n_steps <= 0 || ld < b->ncol || !(sigma > 0) || !(u0 >= 0.0) || !(u0 < 1.0) || tooManyColumns(b))
    return refuse("sipnet_batch_pf_analysis", "bad argument (sigma > 0, 0 <= u0 < 1, at most 4194304 particles)");
  const bool havePre = takePfPre(b, d_plane, elem_is_f32, n_steps, ld, obs, sigma, d_logw);
  int64_t* d_sum = sc.d_blockSum + kFusedBlocks;   // the total weight, whichever path wrote it
  FusedArgs fa{};
  int grid;
  if (fusedSetup(b, sc, elem_is_f32 ? 0 : 1, b->ncol, &fa, &grid)) {
    // log-weights, fixed-point weights, prefix sum and ancestors: ONE launch (pfFusedKernel)
    fa.plane = d_plane;
    fa.nSteps = n_steps;
    fa.ld = ld;
    fa.ncol = b->ncol;
    fa.status = b->d_state + (size_t)ST_status * b->ncol;
    fa.obs = obs;
    fa.invSigma = 1.0 / sigma;
    fa.logw = d_logw;
    fa.logwIn = d_logw;
    fa.preMax = havePre ? b->d_pfPreMax.get() : nullptr;
    fa.nPre = havePre ? b->pfPre.nMax : 0;
    fa.j0 = 0;
    fa.nOut = fa.nTotal = b->ncol;
    fa.u0 = u0;
    fa.anc = d_ancestors;
    fa.total = d_total;
    if (elem_is_f32) hipLaunchKernelGGL((pfFusedKernel<float, false>), dim3(grid), dim3(256), 0, stream, fa);
    else hipLaunchKernelGGL((pfFusedKernel<double, false>), dim3(grid), dim3(256), 0, stream, fa);
    rc = fusedLaunched(sc);
    if (rc) return rc;
  } else {
    // next to nothing of the device is ours to spin on (a sliver of a partitioned device, many filters sharing it): the
    // phases as launches of their own -- log-weights + 256-wide maxima | fixed-point weights | prefix sum | ancestors
    int parts = b->pfPre.nMax;
    if (!havePre) {
      rc = logWeights(b, d_plane, elem_is_f32, n_steps, ld, obs, sigma, d_logw, sc.d_max, hip_stream);
      if (rc) return rc;
      parts = (int)((b->ncol + 255) / 256);
    }
    rc = ancestorsImpl(sc, d_logw, b->ncol, u0, d_ancestors, nullptr, d_sum, parts, hip_stream,
                       havePre ? b->d_pfPreMax.get() : nullptr);
    if (rc) return rc;
    if (d_total) HIP_TRY(hipMemcpyAsync(d_total, d_sum, sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
  }
  if (!d_total) {   // the synchronous check of sipnet_pf_systematic_ancestors
    rc = checkTotal(sc, d_sum, "sipnet_batch_pf_analysis", stream);
    if (rc) return rc;
  }
  return sipnet_batch_resample(b, d_ancestors, nullptr, 0, nullptr, with_params, hip_stream);
}

// scratch of the many-site analysis carved into sa: the sites' totals, and for the split path the chunks' maxima, sums and
// threads' sums and the chunks' sums of squares that given weights' effective sample size needs
static int sitesScratchFor(sipnet_batch* b, PfScratch& sc, SitesArgs& sa, bool split) {
  const size_t nSites = (size_t)b->n_sites, nCk = split ? nSites * (size_t)sa.nChunks : 0;
  return carveScratch(b, sc.d_sites, [&](Carver& c) {
    sa.total = c.take<int64_t>(nSites);
    sa.chunkMax = c.take<double>(nCk);
    sa.chunkSum = c.take<int64_t>(nCk);
    sa.threadIncl = c.take<int64_t>(nCk * 256);
    sa.chunkSq = c.take<int64_t>(2 * nCk);
  });
}

// the many-site analysis on the device: one workgroup per site in one launch, or (split) chunks of sa.chunk columns in three
// (given: the weight source is the caller's log-weights, sipnet_batch_pf_resample_sites)
static void sitesLaunch(SitesArgs& sa, PfScratch& sc, int64_t nSites, bool split, bool f32, hipStream_t stream, bool given) {
  const dim3 sites((unsigned)nSites);
  if (!split) {
    if (given) hipLaunchKernelGGL((pfSitesKernel<double, true>), sites, dim3(256), 0, stream, sa);
    else if (f32) hipLaunchKernelGGL(pfSitesKernel<float>, sites, dim3(256), 0, stream, sa);
    else hipLaunchKernelGGL(pfSitesKernel<double>, sites, dim3(256), 0, stream, sa);
    return;
  }
  if (!sa.w) sa.w = sc.d_w;
  const dim3 chunks((unsigned)nSites, (unsigned)sa.nChunks);
  const dim3 tiles((unsigned)nSites, (unsigned)((sa.M + 255) / 256));
  if (given) {
    hipLaunchKernelGGL((sitesChunkKernel<double, true>), chunks, dim3(256), 0, stream, sa);
    hipLaunchKernelGGL(sitesWeightKernel<true>, chunks, dim3(256), 0, stream, sa);
    hipLaunchKernelGGL(sitesAncestorKernel<true>, tiles, dim3(256), 0, stream, sa);
    return;
  }
  if (f32) hipLaunchKernelGGL(sitesChunkKernel<float>, chunks, dim3(256), 0, stream, sa);
  else hipLaunchKernelGGL(sitesChunkKernel<double>, chunks, dim3(256), 0, stream, sa);
  hipLaunchKernelGGL(sitesWeightKernel<false>, chunks, dim3(256), 0, stream, sa);
  hipLaunchKernelGGL(sitesAncestorKernel<false>, tiles, dim3(256), 0, stream, sa);
}
// the synchronous checks of the many-site analysis, before anything is resampled: the sites' totals, read back
// (who: the entry point; invalid: what makes a site's arguments bad there)
static int sitesCheck(PfScratch& sc, int64_t nSites, hipStream_t stream, const char* who, const char* invalid) {
  std::vector<int64_t> tot;
  RC_TRY(readBack(tot, (const int64_t*)sc.d_sites.get(), (size_t)nSites, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int64_t s = 0; s < nSites; s++)
    if (tot[(size_t)s] == kSiteInvalid)
      return refuse(who, "site " + std::to_string(s) + ": bad argument (" + invalid + "); nothing was resampled");
  for (int64_t s = 0; s < nSites; s++)
    if (tot[(size_t)s] == 0)
      return refuse(who, "site " + std::to_string(s) + ": every particle has zero weight; nothing was resampled", SIPNET_ERR_BAD_PARAMETER);
  return SIPNET_OK;
}
// the many-site analysis' path and the split path's chunks (256 x a power of two columns, at most kSitesMaxChunks per site).
// One workgroup per site only when the sites fill the device: fewer sites than CUs leave CUs idle while a few of them
// read all the planes (64 x 4096 particles: 0.22 ms against 0.14 split, profiles/r07_pf_sites_time.txt)
static bool sitesGeometry(const sipnet_batch* b, int* chunk, int* nChunks) {
  const int64_t M = b->n_members;
  *chunk = 256;   // (at least two workgroups per CU for the log-weights of a few big sites)
  while ((M + *chunk - 1) / *chunk > kSitesMaxChunks) *chunk *= 2;
  *nChunks = (int)((M + *chunk - 1) / *chunk);
  return M > kSitesLds || b->n_sites < b->numCUs || (b->kernelOptions & SIPNET_KOPT_PF_MULTI_LAUNCH);
}

// What the two many-site entry points do before their own arguments: the refusal of a connected batch, the device, whatever a
// forecast has left is spent, the scratch, the path (*split) and the geometry, and of sa what does not depend on the weights' source
static int sitesBegin(const char* who, sipnet_batch* b, const double* d_u0, double* d_logw, int32_t* d_ancestors,
                      int64_t* d_fixed_weights, int64_t* d_site_total, hipStream_t stream, SitesArgs& sa, bool* split) {
  if (b->pfPeers)
    return refuse(who, "this batch is connected to a filter across ranks (sipnet_batch_pf_connect): resample through "
                       "sipnet_batch_pf_resample_peers");
  RC_TRY(useDevice(b));
  b->pfPre.valid = false;
  PfScratch& sc = scratchOf(b);
  RC_TRY(pfScratchFor(sc, b->ncol, stream));
  int chunk, nChunks;
  *split = sitesGeometry(b, &chunk, &nChunks);
  sa = SitesArgs{};
  sa.M = b->n_members;
  sa.nChunks = nChunks;
  sa.chunk = chunk;
  RC_TRY(sitesScratchFor(b, sc, sa, *split));
  sa.u0 = d_u0;
  sa.logw = d_logw;
  sa.w = d_fixed_weights;
  sa.anc = d_ancestors;
  sa.totalOut = d_site_total;
  return SIPNET_OK;
}
// ... and after them: the launches and their error, what sipnet_batch_pf_info reports, the synchronous form's check (invalid:
// what makes a site's arguments bad at this entry point), the resampling
static int sitesFinish(const char* who, sipnet_batch* b, SitesArgs& sa, bool split, bool f32, bool given, const char* invalid,
                       int32_t with_params, hipStream_t stream) {
  PfScratch& sc = scratchOf(b);
  sitesLaunch(sa, sc, b->n_sites, split, f32, stream, given);
  HIP_TRY(hipGetLastError());
  reportPath(b, !split, split ? 0 : (int32_t)b->n_sites);
  if (!sa.totalOut) RC_TRY(sitesCheck(sc, b->n_sites, stream, who, invalid));
  return resampleColumns(b, sa.anc, nullptr, 0, nullptr, with_params, stream);
}

int sipnet_batch_pf_analysis_sites(sipnet_batch* b, const void* d_plane, int32_t elem_is_f32, int32_t n_steps, int64_t ld,
                                   const double* d_obs, const double* d_sigma, const double* d_u0, int32_t with_params,
                                   double* d_logw, int32_t* d_ancestors, int64_t* d_fixed_weights, int64_t* d_site_total,
                                   void* hip_stream) {
  const char* who = "sipnet_batch_pf_analysis_sites";
  if (!b || !d_plane || !d_obs || !d_sigma || !d_u0 || !d_logw || !d_ancestors || n_steps <= 0 || ld < b->ncol ||
      tooManyColumns(b))
    return refuse(who, "bad argument (device pointers, n_steps > 0, ld >= ncol, at most 4194304 particles)");
  SitesArgs sa;
  bool split;
  RC_TRY(sitesBegin(who, b, d_u0, d_logw, d_ancestors, d_fixed_weights, d_site_total, (hipStream_t)hip_stream, sa, &split));
  sa.plane = d_plane;
  sa.nSteps = n_steps;
  sa.ld = ld;
  sa.status = b->d_state + (size_t)ST_status * b->ncol;
  sa.obs = d_obs;
  sa.sigma = d_sigma;
  return sitesFinish(who, b, sa, split, elem_is_f32 != 0, /*given=*/false, "a finite obs needs a finite sigma > 0; 0 <= u0 < 1",
                     with_params, (hipStream_t)hip_stream);
}

int sipnet_batch_pf_resample_sites(sipnet_batch* b, double* d_logw, const double* d_u0, const double* d_beta,
                                   const double* d_ess_min, int32_t with_params, int32_t* d_ancestors,
                                   int64_t* d_fixed_weights, int64_t* d_site_total, double* d_ess, void* hip_stream) {
  const char* who = "sipnet_batch_pf_resample_sites";
  if (!b || !d_logw || !d_u0 || !d_ancestors || tooManyColumns(b))
    return refuse(who, "bad argument (device pointers d_logw, d_u0, d_ancestors; at most 4194304 particles)");
  SitesArgs sa;
  bool split;
  RC_TRY(sitesBegin(who, b, d_u0, d_logw, d_ancestors, d_fixed_weights, d_site_total, (hipStream_t)hip_stream, sa, &split));
  sa.beta = d_beta;
  sa.essMin = d_ess_min;
  sa.ess = d_ess;
  return sitesFinish(who, b, sa, split, false, /*given=*/true,
                     "0 <= u0 < 1, a finite beta > 0, an ess_min that is not NaN, no +inf log-weight", with_params,
                     (hipStream_t)hip_stream);
}

// ---- series likelihood weights ---------------------------------------------------------------------------------------
static int loglikRefuse(const std::string& why) { return refuse("sipnet_batch_series_loglik", why); }
// the synchronous form's check: obs and sd read back, the first site and term with bad input named
static int loglikCheck(const sipnet_batch* b, int32_t n_terms, const sipnet_loglik_term* terms, hipStream_t stream) {
  std::vector<double> obs, sd;
  for (int q = 0; q < n_terms; q++) {
    const size_t n = (size_t)b->n_sites * (size_t)terms[q].rows;
    RC_TRY(readBack(obs, terms[q].d_obs, n, stream));
    RC_TRY(readBack(sd, terms[q].d_sd, n, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (size_t i = 0; i < n; i++) {
      const double y = obs[i];
      if (y != y) continue;
      if (std::isfinite(y) && sd[i] > 0.0 && std::isfinite(sd[i])) continue;
      return loglikRefuse("site " + std::to_string(i / (size_t)terms[q].rows) + ", term " + std::to_string(q) + ", row " +
                          std::to_string(i % (size_t)terms[q].rows) +
                          ": bad input (an obs that is not NaN must be finite and needs a finite sd > 0); nothing was written");
    }
  }
  return SIPNET_OK;
}

int sipnet_batch_series_loglik(sipnet_batch* b, int32_t n_terms, const sipnet_loglik_term* terms, int32_t elem_is_f32,
                               int64_t ld, int32_t normalise, int32_t path, const double* d_add, double* d_loglik,
                               double* d_parts, int32_t* d_used, int32_t* d_site_info, void* hip_stream) {
  if (!b || !terms || !d_loglik) return loglikRefuse("a NULL batch, terms or d_loglik");
  if (n_terms < 1 || n_terms > kLoglikMaxTerms) return loglikRefuse("n_terms must be 1.." + std::to_string(kLoglikMaxTerms));
  if (ld < b->ncol) return loglikRefuse("ld < ncol");
  if (tooManyColumns(b)) return loglikRefuse("at most 4194304 columns");
  if (path < 0 || path > 2) return loglikRefuse("path must be 0 (auto), 1 or 2");
  LoglikArgs a{};
  int64_t tilesTotal = 0;
  for (int q = 0; q < n_terms; q++) {
    const sipnet_loglik_term& t = terms[q];
    const std::string who = "term " + std::to_string(q) + ": ";
    if (!t.d_series || !t.d_obs || !t.d_sd) return loglikRefuse(who + "a NULL series, obs or sd");
    if (t.kind != SIPNET_LOGLIK_GAUSS && t.kind != SIPNET_LOGLIK_LAPLACE) return loglikRefuse(who + "kind must be SIPNET_LOGLIK_GAUSS or SIPNET_LOGLIK_LAPLACE");
    if (t.rows < 1 || t.sum_steps < 1) return loglikRefuse(who + "rows and sum_steps must be at least 1");
    if (!std::isfinite(t.scale)) return loglikRefuse(who + "the scale is not finite");
    LoglikTerm& k = a.term[q];
    k.series = t.d_series;
    k.obs = t.d_obs;
    k.sd = t.d_sd;
    k.rows = t.rows;
    k.sumSteps = t.sum_steps;
    k.kind = t.kind;
    k.tiles = (int32_t)(((int64_t)t.rows + kLoglikTile - 1) / kLoglikTile);
    k.scale = t.scale;
    tilesTotal += k.tiles;
  }
  if (b->planDirty) return loglikRefuse("needs a batch that was set up (sipnet_batch_setup): the members' status is read");
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  const int64_t M = b->n_members, nSites = b->n_sites, chunksPerSite = (M + 255) / 256, groups = nSites * chunksPerSite;
  // path 2 when the columns alone leave the device short of workgroups (10 240 members x 17 520 rows: 40 of them on 256 CUs)
  // and there is more than one tile to spread
  bool two = path == 2 || (path == 0 && tilesTotal > 1 && groups < 2 * (int64_t)b->numCUs);
  if (two && groups * tilesTotal > (int64_t)INT32_MAX) {
    if (path == 2) return loglikRefuse("path 2 would need more than INT32_MAX workgroups");
    two = false;
  }
  if (!d_site_info) {
    rc = loglikCheck(b, n_terms, terms, stream);
    if (rc) return rc;
  }
  a.nTerms = n_terms;
  a.normalise = normalise != 0;
  a.chunksPerSite = (int32_t)chunksPerSite;
  a.tilesTotal = (int32_t)tilesTotal;
  a.ld = ld;
  a.M = M;
  a.ncol = b->ncol;
  a.status = b->d_state + (size_t)ST_status * b->ncol;
  a.add = d_add;
  a.out = d_loglik;
  a.parts = d_parts;
  a.used = d_used;
  a.siteInfo = d_site_info;
  if (!two) {
    if (elem_is_f32) hipLaunchKernelGGL(loglikKernel<float>, dim3((unsigned)groups), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(loglikKernel<double>, dim3((unsigned)groups), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return SIPNET_OK;
  }
  PfScratch& sc = scratchOf(b);
  RC_TRY(growScratch(b, sc.d_loglik, (size_t)tilesTotal * (size_t)b->ncol));
  RC_TRY(growScratch(b, sc.d_loglikUsed, (size_t)tilesTotal * (size_t)nSites));
  a.partial = sc.d_loglik;
  a.tileUsed = sc.d_loglikUsed;
  const dim3 grid((unsigned)(groups * tilesTotal));
  if (elem_is_f32) hipLaunchKernelGGL(loglikTileKernel<float>, grid, dim3(256), 0, stream, a, groups);
  else hipLaunchKernelGGL(loglikTileKernel<double>, grid, dim3(256), 0, stream, a, groups);
  hipLaunchKernelGGL(loglikCombineKernel, dim3((unsigned)groups), dim3(256), 0, stream, a);
  HIP_TRY(hipGetLastError());
  return SIPNET_OK;
}

}  // extern "C"

#include "pf_moves.inc"

// ---- the filter across ranks by peer reads --------------------------------------------------------------------
void pfRelease(sipnet_batch* b) {
  delete b->pfScratch;
  b->pfScratch = nullptr;
  closePeers(b->pfPeers);
  b->pfPeers = nullptr;
}

static_assert(sizeof(hipIpcMemHandle_t) <= sizeof(((sipnet_pf_peer*)nullptr)->ipc[0]), "sipnet_pf_peer::ipc holds a hipIpcMemHandle_t");

extern "C" {

int sipnet_batch_pf_publish(sipnet_batch* b, int32_t with_params, sipnet_pf_peer* out) {
  if (!b || !out)
    return refuse("sipnet_batch_pf_publish", "bad argument");
  if (b->n_sites != 1)
    return refuse("sipnet_batch_pf_publish", "particles of different sites must not mix (n_sites must be 1)");
  int rc = useDevice(b);
  if (rc) return rc;
  rc = ensureSpares(b, /*state=*/true, /*params=*/with_params != 0, /*index=*/false);
  if (rc) return rc;
  rc = waitIdle(b);                      // (whatever stream the batch last ran on: the spares and the parameters settle)
  if (rc) return rc;
  rc = flushParams(b, nullptr);          // (peers will read the converted block)
  if (rc) return rc;
  rc = materializeParams(b, nullptr);    // (... in column order: peers address a particle's rows by its column)
  if (rc) return rc;
  pfDropBank(b);                         // (an earlier connection's bank: the next connect builds a new one)
  rc = waitIdle(b);
  if (rc) return rc;
  memset(out, 0, sizeof *out);
  out->process_id = (int64_t)getpid();
  out->device = b->device;
  out->n_particles = (int32_t)b->ncol;
  out->precision = b->precision;
  out->with_params = with_params ? 1 : 0;
  out->generic_exponents = b->genericExponents ? 1 : 0;
  const bool byIndex = with_params && !(b->kernelOptions & SIPNET_KOPT_PF_MOVE_PARAMS);
  out->params_by_index = byIndex ? 1 : 0;
  // the particles' index into the bank of all ranks' parameters (filled by connect), double-buffered like the state
  if (byIndex) RC_TRY(ensureSpares(b, /*state=*/false, /*params=*/false, /*index=*/true));
  void* ptr[8] = {b->d_state, b->d_state2, b->d_ring, b->d_ring2, with_params ? b->d_prm : nullptr,
                  with_params ? b->d_prm2 : nullptr, byIndex ? b->d_prmId : nullptr, byIndex ? b->d_prmId2 : nullptr};
  out->ipc_valid = 1;
  for (int k = 0; k < 8; k++) {
    out->address[k] = (uint64_t)(uintptr_t)ptr[k];
    if (!ptr[k]) continue;
    hipIpcMemHandle_t h;
    if (hipIpcGetMemHandle(&h, ptr[k]) != hipSuccess) {   // peers inside this process do not need it
      (void)hipGetLastError();
      out->ipc_valid = 0;
      continue;
    }
    memcpy(out->ipc[k], &h, sizeof h);
  }
  return SIPNET_OK;
}

// (a refusal of connect; the caller takes the half-made table down: closePeers)
static int connectRefused(const std::string& why, int code) { return refuse("sipnet_batch_pf_connect", why, code); }
// connect, for rank s: its descriptor agrees with mine, its particles are counted, and its eight matrices are addressable
// from here -- same process (the node object): the addresses themselves, and peer access to its device; another process:
// its allocations mapped (dmabuf IPC)
static int mapPeer(const sipnet_batch* b, PfPeers* pp, int s, const sipnet_pf_peer& q, const sipnet_pf_peer& me) {
  if (q.precision != me.precision || q.with_params != me.with_params || q.params_by_index != me.params_by_index || q.n_particles <= 0)
    return connectRefused("rank " + std::to_string(s) + " published another precision / parameter mode", SIPNET_ERR_BAD_ARGUMENT);
  pp->count[s] = q.n_particles;
  if (q.n_particles > pp->nmax) pp->nmax = q.n_particles;
  if (s < pp->rank) pp->first += q.n_particles;
  pp->nTotal += q.n_particles;
  void* ptr[8];
  if (q.process_id == me.process_id) {
    for (int k = 0; k < 8; k++) ptr[k] = (void*)(uintptr_t)q.address[k];
    if (q.device != b->device) {
      hipError_t e = hipDeviceEnablePeerAccess(q.device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
        return connectRefused(std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e), SIPNET_ERR_NO_DEVICE);
      (void)hipGetLastError();
    }
  } else {
    if (!q.ipc_valid) return connectRefused("rank " + std::to_string(s) + " could not export IPC handles", SIPNET_ERR_NO_DEVICE);
    for (int k = 0; k < 8; k++) {
      ptr[k] = nullptr;
      if (!q.address[k]) continue;
      hipIpcMemHandle_t h;
      memcpy(&h, q.ipc[k], sizeof h);
      hipError_t e = hipIpcOpenMemHandle(&ptr[k], h, hipIpcMemLazyEnablePeerAccess);
      if (e != hipSuccess) return connectRefused(std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e), SIPNET_ERR_NO_DEVICE);
      pp->opened.push_back(ptr[k]);
    }
  }
  for (int par = 0; par < 2; par++) {
    pp->state[par][s] = (const double*)ptr[0 + par];
    pp->ring[par][s] = ptr[2 + par];
    pp->prm[par][s] = (const double*)ptr[4 + par];
    pp->ids[par][s] = (const int32_t*)ptr[6 + par];
  }
  return SIPNET_OK;
}
// connect: every rank's converted parameters, once: [NPARAMS][world * nmax], rank s's particle c in column s * nmax + c (the
// slot numbering of the weights).  Parameters are constants of a particle; what a resampling moves from now on is this column
// number -- 4 bytes instead of 640, and the forecast's parameter reads stay in local HBM.  (The peers' blocks are read
// where they are: peer-mapped HBM, as every later gather reads state and ring.)
static int fillBank(sipnet_batch* b, const PfPeers* pp) {
  const int64_t pitch = (int64_t)pp->world * pp->nmax;
  pfDropBank(b);
  if (b->d_prmBank.tryReserve((size_t)pitch * SIPNET_NPARAMS) != hipSuccess) {
    (void)hipGetLastError();
    return connectRefused("no memory for the bank of all ranks' parameters (SIPNET_KOPT_PF_MOVE_PARAMS does without)", SIPNET_ERR_INTERNAL);
  }
  b->prmBankPitch = pitch;
  for (int s = 0; s < pp->world; s++) {
    const int64_t cnt = pp->count[s];
    hipLaunchKernelGGL(copyRowsKernel, dim3((unsigned)((cnt + 255) / 256), 8), dim3(256), 0, nullptr, b->d_prmBank + (int64_t)s * pp->nmax,
                       pitch, pp->prm[0][s], cnt, cnt, (int32_t)SIPNET_NPARAMS);
  }
  hipLaunchKernelGGL(iotaKernel, dim3((unsigned)((b->ncol + 255) / 256)), dim3(256), 0, nullptr, b->d_prmId, b->ncol, (int32_t)(pp->rank * pp->nmax));
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    pfDropBank(b);
    return connectRefused(std::string("filling the parameter bank: ") + hipGetErrorString(e), SIPNET_ERR_INTERNAL);
  }
  b->prmIndexed = false;   // (d_prm is current too: nothing has been resampled yet)
  return SIPNET_OK;
}

// Four steps: my own descriptor is this batch as it stands | the old connection goes (before the peers are looked at: a failed
// connect leaves none) | every peer is mapped (mapPeer) | the parameter bank (fillBank) and the crossing counter
int sipnet_batch_pf_connect(sipnet_batch* b, int32_t world, int32_t rank, const sipnet_pf_peer* peers) {
  if (!b || !peers || world < 1 || world > kMaxPeers || rank < 0 || rank >= world)
    return refuse("sipnet_batch_pf_connect", "bad argument (world <= 16)");
  int rc = useDevice(b);
  if (rc) return rc;
  const sipnet_pf_peer& me = peers[rank];
  if (me.process_id != (int64_t)getpid() || me.address[0] != (uint64_t)(uintptr_t)b->d_state.get() ||
      me.address[1] != (uint64_t)(uintptr_t)b->d_state2.get() || me.n_particles != b->ncol)
    return connectRefused("peers[rank] is not what this batch published (publish, then connect, with no resampling in between)",
                          SIPNET_ERR_BAD_ARGUMENT);
  closePeers(b->pfPeers);
  b->pfPeers = nullptr;
  PfPeers* pp = new PfPeers();
  pp->world = world;
  pp->rank = rank;
  pp->withParams = me.with_params;
  auto fail = [&](int code) {
    closePeers(pp);
    return code;
  };
  bool generic = false;
  for (int s = 0; s < world; s++) {
    rc = mapPeer(b, pp, s, peers[s], me);
    if (rc) return fail(rc);
    generic = generic || peers[s].generic_exponents != 0;
  }
  if ((int64_t)world * pp->nmax > kMaxColumns) return fail(connectRefused("more than 4 194 304 weight slots", SIPNET_ERR_BAD_ARGUMENT));
  // particles carry their parameters between ranks: every rank runs the kernel variant the most general
  // parameter set anywhere needs (decided here, once -- not by a device -> host check after every exchange)
  if (generic && me.with_params) b->genericExponents = true;
  pp->byIndex = me.params_by_index != 0;
  if (pp->byIndex) {
    rc = fillBank(b, pp);
    if (rc) return fail(rc);
  }
  if (b->d_pfCrossing.tryReserve(1) != hipSuccess ||
      hipMemset(b->d_pfCrossing, 0, sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    pfDropBank(b);
    return fail(connectRefused("no memory for the crossing counter", SIPNET_ERR_INTERNAL));
  }
  b->pfInfo.cycles = 0;
  b->pfPeers = pp;
  pp->bankLost = false;
  return SIPNET_OK;
}

int64_t sipnet_batch_pf_block_len(const sipnet_batch* b) {
  if (!b) return -1;
  const int64_t nmax = b->pfPeers ? b->pfPeers->nmax : b->ncol;
  return nmax + (nmax + 255) / 256;
}

int sipnet_batch_pf_local_weights(sipnet_batch* b, const void* d_plane, int32_t elem_is_f32, int32_t n_steps,
                                  int64_t ld, double obs, double sigma, double* d_block, void* hip_stream) {
  if (!b || !d_block)
    return refuse("sipnet_batch_pf_local_weights", "bad argument");
  const int64_t nmax = b->pfPeers ? b->pfPeers->nmax : b->ncol;
  // the forecast's launch was told of this analysis (sipnet_batch_pf_arm with d_logw = this block) and has left the
  // log-weights in it: only the 256-wide maxima and the empty slots remain (wavefront k covers columns 64 k .. 64 k + 63
  // when the one site's members are a multiple of 64)
  const bool havePre = takePfPre(b, d_plane, elem_is_f32, n_steps, ld, obs, sigma, d_block) && b->n_sites == 1 && b->ncol % 64 == 0;
  if (havePre) {
    int rc = useDevice(b);
    if (rc) return rc;
    const int64_t work = std::max<int64_t>((nmax + 255) / 256, nmax - b->ncol);
    hipLaunchKernelGGL(blockFromWaveMaximaKernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                       b->d_pfPreMax, b->ncol / 64, b->ncol, nmax, d_block, d_block + nmax);
    HIP_TRY(hipGetLastError());
    return SIPNET_OK;
  }
  return logWeights(b, d_plane, elem_is_f32, n_steps, ld, obs, sigma, d_block, d_block + nmax, hip_stream, nmax);
}

// resample_peers, step 1: where every rank keeps its particles' matrices right now -- the connection's table under the current
// parity, or this batch alone (not connected: a filter of one rank, parameters travel with the particles)
struct PeerFilter {
  PeerPtrs tab{};
  int64_t nTotal = 0, first = 0;   // particles of all ranks; global index of this rank's first particle
  bool withParams = true, byIndex = false;
};
static int peerTable(const sipnet_batch* b, PeerFilter* f) {
  PeerPtrs& tab = f->tab;
  if (!b->pfPeers) {
    tab.world = 1;
    tab.nmax = (int32_t)b->ncol;
    tab.rank = 0;
    tab.state[0] = b->d_state;
    tab.ring[0] = b->d_ring;
    tab.third[0] = b->d_prm;
    tab.pitch[0] = (int32_t)b->ncol;
    f->nTotal = b->ncol;
    return SIPNET_OK;
  }
  const PfPeers& pp = *b->pfPeers;
  tab.world = pp.world;
  tab.nmax = pp.nmax;
  tab.rank = pp.rank;
  for (int s = 0; s < pp.world; s++) {
    tab.state[s] = pp.state[pp.parity][s];
    tab.ring[s] = pp.ring[pp.parity][s];
    tab.third[s] = f->byIndex ? (const void*)pp.ids[pp.parity][s] : (const void*)pp.prm[pp.parity][s];
    tab.pitch[s] = pp.count[s];
  }
  f->nTotal = pp.nTotal;
  f->first = pp.first;
  f->withParams = pp.withParams != 0;
  if (tab.state[pp.rank] != b->d_state || (f->byIndex && tab.third[pp.rank] != (const void*)b->d_prmId))
    return refuse("sipnet_batch_pf_resample_peers", "the batch was resampled behind the peers' back", SIPNET_ERR_INTERNAL);
  tab.crossing = b->d_pfCrossing;
  return SIPNET_OK;
}
// resample_peers, step 2: weights over all slots, prefix sum, the ancestors of MY particles -- one launch (pfFusedKernel), or
// the same as launches of their own (see sipnet_batch_pf_analysis)
static int peerAncestors(sipnet_batch* b, PfScratch& sc, const PeerFilter& f, const double* d_gathered, double u0,
                         int32_t* d_ancestors, int64_t* d_total, hipStream_t stream) {
  const PeerPtrs& tab = f.tab;
  const int64_t nSlots = (int64_t)tab.world * tab.nmax, stride = tab.nmax + (tab.nmax + 255) / 256, n = b->ncol;
  FusedArgs fa{};
  int grid;
  const bool fused = fusedSetup(b, sc, 2, nSlots, &fa, &grid);
  b->pfInfo.nSlots = nSlots;
  if (fused) {
    fa.gathered = d_gathered;
    fa.world = tab.world;
    fa.nmax = tab.nmax;
    fa.stride = stride;
    fa.j0 = f.first;
    fa.nOut = n;
    fa.nTotal = f.nTotal;
    fa.u0 = u0;
    fa.anc = d_ancestors;
    fa.total = d_total;
    hipLaunchKernelGGL((pfFusedKernel<double, true>), dim3(grid), dim3(256), 0, stream, fa);
    return fusedLaunched(sc);
  }
  int64_t* d_sum = sc.d_blockSum + kFusedBlocks;
  const int gridW = (int)((nSlots + 255) / 256);
  hipLaunchKernelGGL(fixedWeightGatheredKernel, dim3(gridW), dim3(256), 0, stream, d_gathered, tab.world, tab.nmax, stride, sc.d_w);
  size_t tmpBytes = sc.tmpBytes;
  HIP_TRY(hipcub::DeviceScan::InclusiveSum(sc.d_tmp, tmpBytes, sc.d_w.get(), sc.d_cdf.get(), (int)nSlots, stream));
  hipLaunchKernelGGL(ancestorKernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sc.d_cdf, nSlots, f.first, n, f.nTotal, u0,
                     d_ancestors, d_sum);
  HIP_TRY(hipGetLastError());
  if (d_total) HIP_TRY(hipMemcpyAsync(d_total, d_sum, sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
  return SIPNET_OK;
}
// resample_peers, step 3: every particle's checkpoint from wherever its ancestor lives, into the spares
static int peerGather(sipnet_batch* b, const PeerFilter& f, const int32_t* d_ancestors, hipStream_t stream) {
  const int64_t n = b->ncol;
  PeerParts parts{};
  parts.p[0] = PeerPart{b->d_state2, SIPNET_NSTATE, 0, 0};
  parts.p[1] = PeerPart{b->d_ring2, SIPNET_RING_SLOTS, rowGroups(SIPNET_NSTATE), b->precision == SIPNET_F32_MIXED ? 1 : 0};
  parts.n = 2;
  int total = rowGroups(SIPNET_NSTATE) + rowGroups(SIPNET_RING_SLOTS);
  if (f.byIndex) {          // the particle's column in the bank of all ranks' parameters: one row of 4-byte elements
    parts.p[2] = PeerPart{b->d_prmId2, 1, total, 1};
    parts.n = 3;
    total += 1;
  } else if (f.withParams) {
    parts.p[2] = PeerPart{b->d_prm2, SIPNET_NPARAMS, total, 0};
    parts.n = 3;
    total += rowGroups(SIPNET_NPARAMS);
  }
  hipLaunchKernelGGL(gatherPeerKernel, dim3((unsigned)((n + 255) / 256), (unsigned)total), dim3(256), 0, stream, parts, f.tab,
                     d_ancestors, n, n);
  HIP_TRY(hipGetLastError());
  return SIPNET_OK;
}

int sipnet_batch_pf_resample_peers(sipnet_batch* b, const double* d_gathered, double u0, int32_t* d_ancestors,
                                   int64_t* d_total, void* hip_stream) {
  if (!b || !d_gathered || !d_ancestors || !(u0 >= 0.0) || !(u0 < 1.0))
    return refuse("sipnet_batch_pf_resample_peers", "bad argument (0 <= u0 < 1)");
  if (b->n_sites != 1)
    return refuse("sipnet_batch_pf_resample_peers", "particles of different sites must not mix (n_sites must be 1)");
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  rc = flushParams(b, stream);
  if (rc) return rc;
  PeerFilter f;
  f.byIndex = b->pfPeers && b->pfPeers->byIndex;
  if (f.byIndex && (b->pfPeers->bankLost || !b->d_prmBank))
    return refuse("sipnet_batch_pf_resample_peers", "this rank's parameters were set anew (or moved as rows by "
                  "sipnet_batch_resample) after sipnet_batch_pf_connect replicated them on every rank: publish and connect again");
  if (!f.byIndex) {
    rc = materializeParams(b, stream);   // (peers read a particle's parameter rows by its column)
    if (rc) return rc;
  }
  rc = peerTable(b, &f);
  if (rc) return rc;
  rc = ensureSpares(b, /*state=*/true, /*params=*/f.withParams && !f.byIndex, /*index=*/false);
  if (rc) return rc;
  PfScratch& sc = scratchOf(b);
  rc = pfScratchFor(sc, (int64_t)f.tab.world * f.tab.nmax, stream);
  if (rc) return rc;
  rc = peerAncestors(b, sc, f, d_gathered, u0, d_ancestors, d_total, stream);
  if (rc) return rc;
  rc = peerGather(b, f, d_ancestors, stream);
  if (rc) return rc;
  adoptSpares(b, f.byIndex, f.withParams);
  if (f.byIndex) b->prmIndexed = true;   // (d_prm, the column-order copy, is behind the index now: materializeParams)
  if (b->pfPeers) b->pfInfo.cycles++;
  return markBusy(b, stream);
}

// what the last analysis did, and how many of this rank's particles have crossed ranks (see sipnet_amd.h)
int sipnet_batch_pf_info(sipnet_batch* b, sipnet_pf_info* out, void* hip_stream) {
  if (!b || !out)
    return refuse("sipnet_batch_pf_info", "bad argument");
  int rc = useDevice(b);
  if (rc) return rc;
  memset(out, 0, sizeof *out);
  out->fused = b->pfInfo.fused;
  out->grid = b->pfInfo.grid;
  out->budget = b->pfInfo.budget;
  out->world = b->pfPeers ? b->pfPeers->world : 1;
  out->n_slots = b->pfInfo.nSlots;
  out->cycles = b->pfInfo.cycles;
  out->params_by_index = b->d_prmBank ? 1 : 0;
  out->device_share = b->deviceShare;
  if (b->d_pfCrossing) {
    unsigned long long c = 0;
    HIP_TRY(hipMemcpyAsync(&c, b->d_pfCrossing, sizeof c, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
    out->crossing = (int64_t)c;
  }
  return SIPNET_OK;
}

}  // extern "C"
