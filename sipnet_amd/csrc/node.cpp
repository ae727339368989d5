// node.cpp -- one node, several GPUs, behind the C boundary (include/sipnet_amd.h, sipnet_node_*).
//
// The reference runs one process per ensemble member (frontend.c:212-250 is its whole host side);
// the north star asks for the ensemble axis sharded over the GPUs of one node with ONE RCCL
// all-gather over xGMI of the output block, issued from the C host.  A sipnet_node is that host
// object: per listed device one SHARD = one sipnet_batch, one HIP stream, one RCCL communicator rank
// (ncclCommInitAll) and one host thread that lives as long as the node and enqueues the shard's work.
// Two ways to cut the batch (SURVEY 8(e) "Partitioning"):
//   SIPNET_SHARD_MEMBERS  every shard holds a contiguous range of every site's members (c10k, c3, c5);
//   SIPNET_SHARD_SITES    every shard holds whole sites with all their members, so a site's forcing,
//                         events and plan exist on ONE device only (c4: 32 of 256 sites per GPU).
// The forward model has no coupling between members, so the step kernels never exchange anything;
// the collectives are all-gathers of what the shards computed:
//   sipnet_node_gather_stats   the per-(variable, step, site) sum / sum of squares block of every
//                              shard (0.84 MB per device and year) -- the default exchange;
//   sipnet_node_gather_planes  the north star's exchange as written: the member-resolved planes;
//   sipnet_node_pf_analysis    the particle filter's one exchange step: ONE all-gather of the
//                              log-weight blocks, after which every shard reads the ancestors it needs
//                              straight out of its peers' HBM (pf.hip: sipnet_batch_pf_resample_peers).
// RCCL is loaded on first use (dlopen of librccl.so.1: a process that already holds one -- PyTorch
// ships its own -- keeps using that one; a single-GPU batch never pays for the 570 MB library).
// Without a usable RCCL sipnet_node_create fails loudly; there is no fallback path.
// A device listed more than once (sipnet_node_create_sharded only) puts several shards on it -- the
// rehearsal of an N-shard run on a smaller machine.  RCCL refuses two ranks on one device, so such a
// node's all-gathers are device-to-device copies ordered by HIP events between the shards' streams;
// sharding, uploads, kernels, the peer tables and the gathered layouts are the same code.
// The parts (this file includes them: one translation unit): node_rccl.h the RCCL loader, the error macros and sipnet_comm_*;
// node_shard.h one shard; node_gather.h a task on every shard and the all-gathers; node_reduce.h the kernels of the reduced
// gathers; node_cuts.h the segment cuts; node_run.h the run paths; node_pf.h the particle filter's node calls.  Here: the
// node itself, its creation and the entry points.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sipnet_amd.h"
#include "dev_buf.h"
#include "shard_pool.h"

using sipnet::DevBuf;
using sipnet::setError;

#include "node_rccl.h"
#include "node_shard.h"

struct sipnet_node {
  int32_t flags[SIPNET_NFLAGS];
  int32_t n_sites = 0, n_members = 0, precision = 0, mode = SIPNET_SHARD_MEMBERS;
  std::vector<Shard> shards;   // (never resized after createNode: a Shard is not copied)
  Rccl* rccl = nullptr;        // null: event-ordered copies (a device is listed twice)
  int32_t maxCount = 0;   // member mode: members per shard, rounded up to even; site mode: n_members
  int32_t maxSites = 0;   // site mode: sites per shard at most; member mode: n_sites
  int64_t ld = 0;         // maxSites * maxCount: every shard's planes have this leading dimension
  int32_t nAlloc = 0;     // the records the shards' planes and statistics were last laid out and zeroed for
  // What the last successful run left on the shards, assigned as a whole (runShards, runGathering).
  // Plain (sipnet_node_run / _forecast): planes [3][nRun][ld] and, after a run, statistics -- gather_stats, gather_planes
  // and pf_analysis want this.  Segmented (sipnet_node_run_gathering): segment j at rows [3 * cuts[j], 3 * cuts[j + 1]) of
  // every shard's planes ([3][len_j][ld] each) and at [n][3][len_j][ld] from element n * 3 * ld * cuts[j] of the gathered
  // planes.  Reduced (sipnet_node_run_gathering_reduced, form != 0): what travelled instead of the planes -- per shard
  // [3][R][ld] (segment by segment, like the planes), gathered [n][3][R_j][ld] per segment; R rows = steps
  // (SIPNET_GATHER_F32, floats) or groups of sumSteps steps (SIPNET_GATHER_SUMS, doubles); redCuts: the segments' first rows.
  struct LastRun {
    int32_t nRun = 0, step0 = 0;
    bool segmented = false;
    std::vector<int32_t> cuts, redCuts;
    int32_t form = 0, sumSteps = 0;
    bool inKernel = false;   // the sums came out of the step kernels' own launches (no planes were written)
    bool plain() const { return nRun > 0 && !segmented; }
    bool reduced() const { return segmented && form != 0; }
    int32_t nSegments() const { return segmented ? (int32_t)cuts.size() - 1 : 0; }
    size_t redElem() const { return form == SIPNET_GATHER_F32 ? sizeof(float) : sizeof(double); }
  } last;
  // particle filter (the shards hold the blocks)
  bool pfConnected = false;
  int64_t pfBlock = 0;
  int32_t pfCycles = 0;
  static constexpr int kPfTotals = 64;
  // the shards' host threads, the task hand-over and the barrier they meet at (shard_pool.h: no HIP in it)
  sipnet::ShardPool pool;

  size_t elem() const { return precision == SIPNET_F64 ? 8 : 4; }
  int n() const { return (int)shards.size(); }
};

// shard k, or null where there is none
static const Shard* shardOf(const sipnet_node* nd, int32_t k) { return (nd && k >= 0 && k < nd->n()) ? &nd->shards[k] : nullptr; }

#include "node_gather.h"
#include "node_reduce.h"
#include "node_cuts.h"
#include "node_run.h"

// ---- creation ----------------------------------------------------------------------------------------------------------
// the arguments of sipnet_node_create[_sharded]; *shared: a device is listed more than once
static int checkCreate(const char* fn, const int32_t* flags, int32_t n_sites, int32_t n_members, const int32_t* devices,
                       int32_t n_devices, int32_t mode, bool allowShared, sipnet_node** out, bool* shared) {
  if (!flags || !out || !devices || n_devices <= 0 || n_devices > 64 || n_sites <= 0 || n_members <= 0 ||
      (mode != SIPNET_SHARD_MEMBERS && mode != SIPNET_SHARD_SITES) ||
      (mode == SIPNET_SHARD_MEMBERS ? n_members : n_sites) < n_devices) {
    setError(std::string(fn) + ": bad argument (needs at least one member -- or, sharding sites, one site -- per device)");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  const int have = sipnet_device_count();
  *shared = false;
  for (int k = 0; k < n_devices; k++) {
    if (devices[k] < 0 || devices[k] >= have) {
      setError(std::string(fn) + ": no usable HIP device " + std::to_string(devices[k]) + " (this engine has no CPU path)");
      return SIPNET_ERR_NO_DEVICE;
    }
    for (int j = 0; j < k; j++)
      if (devices[j] == devices[k]) *shared = true;
  }
  if (*shared && !allowShared) {
    setError("sipnet_node_create: a device is listed twice");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  return SIPNET_OK;
}

// the shards' devices and ranges -- contiguous, sizes differ by at most one -- and the common leading dimension
static void cutShards(sipnet_node* nd, const int32_t* devices, int32_t n_devices) {
  const bool members = nd->mode == SIPNET_SHARD_MEMBERS;
  const int32_t total = members ? nd->n_members : nd->n_sites;
  nd->shards = std::vector<Shard>(n_devices);
  int32_t most = 0;
  for (int k = 0; k < n_devices; k++) {
    Shard& sh = nd->shards[k];
    const int32_t a = (int32_t)((int64_t)total * k / n_devices), z = (int32_t)((int64_t)total * (k + 1) / n_devices);
    sh.device = devices[k];
    sh.first = members ? a : 0;
    sh.count = members ? z - a : nd->n_members;
    sh.sites0 = members ? 0 : a;
    sh.nSites = members ? nd->n_sites : z - a;
    most = std::max(most, z - a);
  }
  nd->maxCount = members ? (most + 1) & ~1 : nd->n_members;   // even: 16-byte aligned fp64 rows
  nd->maxSites = members ? nd->n_sites : most;
  nd->ld = (int64_t)nd->maxSites * nd->maxCount;
}

// every shard's batch, streams and events, then -- no device listed twice -- one RCCL communicator rank each
static int openShards(sipnet_node* nd, const char* fn) {
  std::vector<int> devices;
  for (const Shard& sh : nd->shards) devices.push_back(sh.device);
  for (Shard& sh : nd->shards)
    RC_TRY(sh.open(nd->flags, nd->precision, (int32_t)std::count(devices.begin(), devices.end(), sh.device), fn));
  if (!nd->rccl) return SIPNET_OK;
  std::vector<ncclComm_t> comms(nd->n(), nullptr);
  ncclResult_t nr = nd->rccl->commInitAll(comms.data(), nd->n(), devices.data());
  if (nr != ncclSuccess) {
    setError(std::string(fn) + ": ncclCommInitAll: " + nd->rccl->errorString(nr));
    return SIPNET_ERR_NO_DEVICE;
  }
  for (int k = 0; k < nd->n(); k++) nd->shards[k].comm = comms[k];
  return SIPNET_OK;
}

static int createNode(const int32_t* flags, int32_t n_sites, int32_t n_members, int32_t precision,
                      const int32_t* devices, int32_t n_devices, int32_t mode, bool allowShared, sipnet_node** out) {
  const char* fn = allowShared ? "sipnet_node_create_sharded" : "sipnet_node_create";
  bool shared = false;
  RC_TRY(checkCreate(fn, flags, n_sites, n_members, devices, n_devices, mode, allowShared, out, &shared));
  Rccl* r = nullptr;
  if (!shared) {
    r = loadRccl();
    if (!r) {
      const char* why = dlerror();
      setError(std::string(fn) + ": RCCL (librccl.so.1) cannot be loaded: " + (why ? why : "missing symbol"));
      return SIPNET_ERR_NO_DEVICE;
    }
  }
  sipnet_node* nd = new sipnet_node();
  memcpy(nd->flags, flags, sizeof nd->flags);
  nd->n_sites = n_sites;
  nd->n_members = n_members;
  nd->precision = precision;
  nd->mode = mode;
  nd->rccl = r;
  cutShards(nd, devices, n_devices);
  const int rc = openShards(nd, fn);
  if (rc != SIPNET_OK) {
    const std::string keep = sipnet_last_error();
    sipnet_node_destroy(nd);
    setError(keep);
    return rc;
  }
  // one host thread per shard from here on (none for a node of one shard: its tasks run on the caller's thread)
  nd->pool.start(n_devices, [nd](int k) { return hipSetDevice(nd->shards[k].device) == hipSuccess; },
                 [] { return std::string(sipnet_last_error()); }, SIPNET_ERR_NO_DEVICE);
  *out = nd;
  return SIPNET_OK;
}

// f(shard, the site's index inside the shard's batch) for the shards that hold `site`, the first failure wins: sites
// sharded, the ONE shard that owns the site; members sharded, every shard (same index)
template <class F>
static int onShardsWithSite(sipnet_node* nd, int32_t site, F f) {
  return inShardOrder(nd, [&](Shard& sh) -> int { return sh.hasSite(site) ? f(sh, site - sh.sites0) : SIPNET_OK; });
}

// the ensemble's totals [3][n_run][n_sites][2] on the host from shard 0's copy of everybody's block: members sharded -- the
// shards' blocks added up in shard order (deterministic); sites sharded -- shard k's sites stand at sites0[k] ..
// (concatenation along the site axis)
static int hostTotals(sipnet_node* nd, size_t block, double* host_total) {
  const int n = nd->n();
  const Shard& sh0 = nd->shards[0];
  std::vector<double> all(block * n);
  NODE_HIP(hipSetDevice(sh0.device));
  NODE_HIP(hipStreamSynchronize(sh0.stream));   // shard 0's copy of everybody's block: complete when its all-gather is
  NODE_HIP(hipMemcpy(all.data(), sh0.gatheredStats, all.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (nd->mode == SIPNET_SHARD_MEMBERS) {
    for (size_t i = 0; i < block; i++) {
      double s = 0.0;
      for (int k = 0; k < n; k++) s += all[(size_t)k * block + i];
      host_total[i] = s;
    }
    return SIPNET_OK;
  }
  for (int k = 0; k < n; k++)
    for (size_t vt = 0; vt < (size_t)3 * nd->last.nRun; vt++)
      memcpy(host_total + (vt * nd->n_sites + nd->shards[k].sites0) * 2, all.data() + (size_t)k * block + vt * nd->maxSites * 2,
             (size_t)nd->shards[k].nSites * 2 * sizeof(double));
  return SIPNET_OK;
}

extern "C" {

int sipnet_node_create(const int32_t* flags, int32_t n_sites, int32_t n_members, int32_t precision,
                       const int32_t* devices, int32_t n_devices, sipnet_node** out) {
  return createNode(flags, n_sites, n_members, precision, devices, n_devices, SIPNET_SHARD_MEMBERS, false, out);
}
int sipnet_node_create_sharded(const int32_t* flags, int32_t n_sites, int32_t n_members, int32_t precision,
                               const int32_t* devices, int32_t n_devices, int32_t shard_mode, sipnet_node** out) {
  return createNode(flags, n_sites, n_members, precision, devices, n_devices, shard_mode, true, out);
}

void sipnet_node_destroy(sipnet_node* nd) {
  if (!nd) return;
  nd->pool.stop();
  for (const Shard& sh : nd->shards) sh.sync();   // every shard idle before any gives anything back
  for (Shard& sh : nd->shards) sh.close(nd->rccl);
  delete nd;
}

int32_t sipnet_node_n_devices(const sipnet_node* nd) { return nd ? nd->n() : 0; }
int32_t sipnet_node_shard_mode(const sipnet_node* nd) { return nd ? nd->mode : -1; }
sipnet_batch* sipnet_node_batch(sipnet_node* nd, int32_t k) { const Shard* sh = shardOf(nd, k); return sh ? sh->batch : nullptr; }
void* sipnet_node_stream(sipnet_node* nd, int32_t k) { const Shard* sh = shardOf(nd, k); return sh ? (void*)sh->stream : nullptr; }
int sipnet_node_member_range(const sipnet_node* nd, int32_t k, int32_t* first, int32_t* count) {
  const Shard* sh = shardOf(nd, k);
  if (!sh) return SIPNET_ERR_BAD_ARGUMENT;
  if (first) *first = sh->first;
  if (count) *count = sh->count;
  return SIPNET_OK;
}
int sipnet_node_site_range(const sipnet_node* nd, int32_t k, int32_t* first, int32_t* count) {
  const Shard* sh = shardOf(nd, k);
  if (!sh) return SIPNET_ERR_BAD_ARGUMENT;
  if (first) *first = sh->sites0;
  if (count) *count = sh->nSites;
  return SIPNET_OK;
}
int64_t sipnet_node_ld(const sipnet_node* nd) { return nd ? nd->ld : 0; }

const char* sipnet_node_collective_library(const sipnet_node* nd) {
  static thread_local std::string s;
  if (!nd) return "";
  if (!nd->rccl) return "event-ordered device copies (shards share a device; no RCCL communicator)";
  int v = 0;
  nd->rccl->getVersion(&v);
  s = nd->rccl->path + " (RCCL " + std::to_string(v) + ")";
  return s.c_str();
}

int sipnet_node_set_climate(sipnet_node* nd, int32_t site, int32_t n_steps, const double* clim,
                            const int32_t* year, const int32_t* day) {
  if (!nd || site < 0 || site >= nd->n_sites) {
    setError("sipnet_node_set_climate: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  return onShardsWithSite(nd, site, [&](Shard& sh, int32_t local) { return sipnet_batch_set_climate(sh.batch, local, n_steps, clim, year, day); });
}
int sipnet_node_set_events(sipnet_node* nd, int32_t site, int32_t n_events, const sipnet_event* events) {
  if (!nd || site < 0 || site >= nd->n_sites) {
    setError("sipnet_node_set_events: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  return onShardsWithSite(nd, site, [&](Shard& sh, int32_t local) { return sipnet_batch_set_events(sh.batch, local, n_events, events); });
}
int sipnet_node_set_params(sipnet_node* nd, int32_t site, int32_t first_member, int32_t count, const double* raw) {
  if (!nd || !raw || first_member < 0 || count <= 0 || first_member + count > nd->n_members ||
      (site != SIPNET_ALL_SITES && (site < 0 || site >= nd->n_sites))) {
    setError("sipnet_node_set_params: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  return onEveryShard(nd, [&](int k) -> int {
    const Shard& sh = nd->shards[k];
    if (site != SIPNET_ALL_SITES && !sh.hasSite(site)) return SIPNET_OK;
    const int32_t a = std::max(first_member, sh.first), z = std::min(first_member + count, sh.first + sh.count);
    if (z <= a) return SIPNET_OK;
    return sipnet_batch_set_params(sh.batch, site == SIPNET_ALL_SITES ? site : site - sh.sites0, a - sh.first, z - a,
                                   raw + (size_t)(a - first_member) * SIPNET_NPARAMS);
  });
}
int sipnet_node_set_math(sipnet_node* nd, int32_t policy) {
  if (!nd) return SIPNET_ERR_BAD_ARGUMENT;
  return inShardOrder(nd, [&](Shard& sh) { return sipnet_batch_set_math(sh.batch, policy); });
}
int sipnet_node_set_kernel(sipnet_node* nd, int32_t kernel, int32_t options) {
  if (!nd) return SIPNET_ERR_BAD_ARGUMENT;
  return inShardOrder(nd, [&](Shard& sh) { return sipnet_batch_set_kernel(sh.batch, kernel, options); });
}

int sipnet_node_setup(sipnet_node* nd) {
  if (!nd) return SIPNET_ERR_BAD_ARGUMENT;
  return onEveryShard(nd, [&](int k) -> int { return sipnet_batch_setup(nd->shards[k].batch, nd->shards[k].stream); });
}

int sipnet_node_run(sipnet_node* nd, int32_t step0, int32_t n_steps) { return runShards(nd, step0, n_steps, true); }
int sipnet_node_forecast(sipnet_node* nd, int32_t step0, int32_t n_steps) { return runShards(nd, step0, n_steps, false); }
int sipnet_node_run_gathering(sipnet_node* nd, int32_t step0, int32_t n_steps, int32_t n_segments) {
  return runGathering(nd, step0, n_steps, n_segments);
}
int sipnet_node_run_gathering_reduced(sipnet_node* nd, int32_t step0, int32_t n_steps, int32_t n_segments, int32_t form,
                                      int32_t sum_steps) {
  if (form != SIPNET_GATHER_F32 && form != SIPNET_GATHER_SUMS) {
    setError("sipnet_node_run_gathering_reduced: form must be SIPNET_GATHER_F32 or SIPNET_GATHER_SUMS");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  return runGathering(nd, step0, n_steps, n_segments, form, sum_steps);
}

// ---- what the last run left ------------------------------------------------------------------------------------------------
int32_t sipnet_node_reduced_in_kernel(const sipnet_node* nd) { return (nd && nd->last.reduced() && nd->last.inKernel) ? 1 : 0; }
void* sipnet_node_gathered_reduced(sipnet_node* nd, int32_t k, int32_t segment, int32_t* first_row, int32_t* n_rows, int32_t* elem_bytes) {
  const Shard* sh = shardOf(nd, k);
  if (!sh || !nd->last.reduced() || segment < 0 || segment >= nd->last.nSegments()) return nullptr;
  const LastRun& run = nd->last;
  if (first_row) *first_row = run.redCuts[segment];
  if (n_rows) *n_rows = run.redCuts[segment + 1] - run.redCuts[segment];
  if (elem_bytes) *elem_bytes = (int32_t)run.redElem();
  return (char*)sh->gatheredReduced.get() + (size_t)nd->n() * 3 * run.redCuts[segment] * nd->ld * run.redElem();
}
int32_t sipnet_node_n_segments(const sipnet_node* nd) { return nd ? nd->last.nSegments() : 0; }
void* sipnet_node_gathered_segment(sipnet_node* nd, int32_t k, int32_t segment, int32_t* first_step, int32_t* n_steps) {
  const Shard* sh = shardOf(nd, k);
  if (!sh || segment < 0 || segment >= nd->last.nSegments()) return nullptr;
  const LastRun& run = nd->last;
  if (first_step) *first_step = run.step0 + run.cuts[segment];
  if (n_steps) *n_steps = run.cuts[segment + 1] - run.cuts[segment];
  return (char*)sh->gatheredPlanes.get() + (size_t)nd->n() * 3 * run.cuts[segment] * nd->ld * nd->elem();
}

int sipnet_node_sync(sipnet_node* nd) {
  if (!nd) return SIPNET_ERR_BAD_ARGUMENT;
  return inShardOrder(nd, [](Shard& sh) -> int {
    NODE_HIP(hipSetDevice(sh.device));
    NODE_HIP(hipStreamSynchronize(sh.stream));
    return SIPNET_OK;
  });
}

int sipnet_node_get_status(sipnet_node* nd, int32_t* status) {
  if (!nd || !status) return SIPNET_ERR_BAD_ARGUMENT;
  std::vector<int32_t> loc;
  return inShardOrder(nd, [&](Shard& sh) -> int {
    NODE_HIP(hipSetDevice(sh.device));
    loc.resize((size_t)sh.nSites * sh.count);
    RC_TRY(sipnet_batch_get_status(sh.batch, loc.data(), sh.stream));   // synchronises the shard's stream
    for (int32_t s = 0; s < sh.nSites; s++)
      memcpy(status + (size_t)(sh.sites0 + s) * nd->n_members + sh.first, loc.data() + (size_t)s * sh.count, (size_t)sh.count * sizeof(int32_t));
    return SIPNET_OK;
  });
}

void* sipnet_node_planes(sipnet_node* nd, int32_t k) { const Shard* sh = shardOf(nd, k); return sh ? sh->planes.get() : nullptr; }
double* sipnet_node_stats(sipnet_node* nd, int32_t k) { const Shard* sh = shardOf(nd, k); return sh ? sh->stats.get() : nullptr; }
double* sipnet_node_gathered_stats(sipnet_node* nd, int32_t k) { const Shard* sh = shardOf(nd, k); return sh ? sh->gatheredStats.get() : nullptr; }
void* sipnet_node_gathered_planes(sipnet_node* nd, int32_t k) { const Shard* sh = shardOf(nd, k); return sh ? sh->gatheredPlanes.get() : nullptr; }

// ONE all-gather: every shard's statistics block of the last sipnet_node_run to every shard
int sipnet_node_gather_stats(sipnet_node* nd, double* host_total) {
  if (!nd || !nd->last.plain()) {
    setError("sipnet_node_gather_stats: nothing has run (sipnet_node_run_gathering leaves no statistics)");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  const size_t block = (size_t)3 * nd->last.nRun * nd->maxSites * 2;  // doubles per shard
  RC_TRY(gatherWhole(nd, [](Shard& sh) { return sh.stats.get(); }, [](Shard& sh) -> DevBuf<double>& { return sh.gatheredStats; },
                     block, ncclDouble, sizeof(double)));
  return host_total ? hostTotals(nd, block, host_total) : SIPNET_OK;
}

// ONE all-gather of the member-resolved planes of the last run: on every shard
// gathered[(k * 3 + v) * n_run + t][ld] = shard k's plane v; inside a row shard k's column of (its local site s,
// its member m) is s * count_k + m -- the site stride is the SHARD's member count, not the common maximum --
// and the columns from n_sites_k * count_k to ld are zero
int sipnet_node_gather_planes(sipnet_node* nd) {
  if (!nd || !nd->last.plain()) {
    setError("sipnet_node_gather_planes: nothing has run (after sipnet_node_run_gathering the planes are gathered already)");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  const size_t count = (size_t)3 * nd->last.nRun * nd->ld;  // elements per shard
  return gatherWhole(nd, [](Shard& sh) { return sh.planes.get(); }, [](Shard& sh) -> DevBuf<unsigned char>& { return sh.gatheredPlanes; },
                     count, nd->precision == SIPNET_F64 ? ncclDouble : ncclFloat, nd->elem());
}

}  // extern "C"

#include "node_pf.h"
