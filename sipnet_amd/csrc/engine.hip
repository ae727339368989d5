// engine.hip -- the batch object behind include/sipnet_amd.h: HBM layout, create / destroy, the events and parameters
// handed over, setup, the switches.  Its parts: engine_plan.hip (site plans and the climate they are built from),
// engine_run.hip (kernel choice and launches), engine_state.hip (state, rings, restart checkpoints), engine_mem.hip (device
// memory and streams for callers without a HIP runtime of their own).  No CPU compute path exists here: every compute entry
// point needs a HIP device and reports SIPNET_ERR_NO_DEVICE otherwise.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/sipnet_amd.h"
#include "batch_impl.h"

namespace sipnet {
thread_local std::string g_lastError;
void setError(const std::string& s) { g_lastError = s; }
}  // namespace sipnet

// The parameter half of setupModel() (sipnet.c:1873-1916) for everything set_params has staged, on the caller's
// stream: ONE upload of the raw rows, one conversion launch per set_params call; from here on the converted block
// is the only copy of the members' parameters on the device.  The caller records the batch busy behind it.
int flushParams(sipnet_batch* b, hipStream_t stream) {
  if (b->pendingParams.empty()) return SIPNET_OK;
  {   // new rows are converted into column order: a resampled index must be resolved first
    int rcM = materializeParams(b, stream);
    if (rcM) return rcM;
    // (... and the copy of this rank's parameters that a connected filter's peers hold is out of date: connect again)
    pfDropBank(b);
  }
  if (b->hostRawUsed * SIPNET_NPARAMS > b->d_rawStage.capacity()) {
    RC_TRY(waitIdle(b));
    RC_TRY(b->d_rawStage.reserve(b->hostRawUsed * SIPNET_NPARAMS));
  }
  // The conversion writes d_prm: it must not start while this batch's last launch -- possibly on ANOTHER stream of
  // the caller's (a node shard's, the null stream of pf_publish) -- still reads it.  A device-side wait, no host stall.
  {
    int rcO = orderBehindBusy(b, stream);
    if (rcO) return rcO;
  }
  // (an earlier conversion on `stream` may still read the device block: the copy stream waits for the caller's first)
  HIP_TRY(hipEventRecord(b->evOrder, stream));
  HIP_TRY(hipStreamWaitEvent(b->upStream, b->evOrder, 0));
  HIP_TRY(hipMemcpyAsync(b->d_rawStage, b->hostRaw, b->hostRawUsed * SIPNET_NPARAMS * sizeof(double), hipMemcpyHostToDevice, b->upStream));
  int rcS = joinUploads(b, stream);
  if (rcS) return rcS;
  for (const auto& p : b->pendingParams)
    launchConvertParams(b->d_rawStage + p.row0 * SIPNET_NPARAMS, b->d_prm, b->ncol, p.col0, p.count,
                        b->flags[SIPNET_F_GDD] ? 0 : b->flags[SIPNET_F_SOIL_PHENOL] ? 1 : 2, stream, p.nRep, b->n_members);
  HIP_TRY(hipGetLastError());
  b->pendingParams.clear();
  b->hostRawUsed = 0;
  return markBusy(b, stream);   // (whoever flushes next, on whatever stream, waits for these conversions)
}

extern "C" {

const char* sipnet_version(void) { return "sipnet_amd 0.1 (reference SIPNET 2.1.0)"; }
const char* sipnet_last_error(void) { return g_lastError.c_str(); }

int sipnet_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int sipnet_batch_create(const int32_t* flags, int32_t n_sites, int32_t n_members,
                        int32_t precision, int32_t device, sipnet_batch** out) {
  if (!flags || !out || n_sites <= 0 || n_members <= 0 ||
      (precision != SIPNET_F64 && precision != SIPNET_F32_MIXED)) {
    setError("sipnet_batch_create: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  // flag coupling rules, common/context.c:195-223
  if ((flags[SIPNET_F_SOIL_PHENOL] && flags[SIPNET_F_GDD]) ||
      (flags[SIPNET_F_NITROGEN_CYCLE] &&
       !(flags[SIPNET_F_LITTER_POOL] && flags[SIPNET_F_ANAEROBIC])) ||
      (flags[SIPNET_F_ANAEROBIC] && !flags[SIPNET_F_WATER_HRESP]) ||
      (flags[SIPNET_F_CARBON_SATURATION] && !flags[SIPNET_F_LITTER_POOL])) {
    setError("sipnet_batch_create: incompatible model flags (context.c:195-223)");
    return SIPNET_ERR_BAD_PARAMETER;
  }
  if (sipnet_device_count() <= device || device < 0) {
    setError("sipnet_batch_create: no usable HIP device (this engine has no CPU path)");
    return SIPNET_ERR_NO_DEVICE;
  }
  sipnet_batch* b = new sipnet_batch();
  memcpy(b->flags, flags, sizeof(b->flags));
  b->n_sites = n_sites;
  b->n_members = n_members;
  b->precision = precision;
  b->device = device;
  b->ncol = (int64_t)n_sites * n_members;

  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) b->numCUs = prop.multiProcessorCount;
  }
  b->fastMath = (precision == SIPNET_F32_MIXED);
  b->sc.resize(n_sites);
  b->devSite.assign(n_sites, 0);
  b->events.resize(n_sites);
  b->resume.resize(n_sites);
  b->resumeProcessed.assign(n_sites, 0);
  b->siteStatus.assign(n_sites, 0);
  int rc = useDevice(b);
  if (rc) { delete b; return rc; }
  const size_t nc = (size_t)b->ncol;
  hipError_t e = hipSuccess;
  if (e == hipSuccess) e = b->d_prm.tryReserve(nc * SIPNET_NPARAMS);
  if (e == hipSuccess) e = b->d_state.tryReserve(nc * SIPNET_NSTATE);
  if (e == hipSuccess) e = b->d_ring.tryReserve(ringDoubles(b));
  if (e == hipSuccess) e = b->d_siteStatus.tryReserve(n_sites);
  if (e == hipSuccess) e = b->d_siteStart.tryReserve(n_sites);
  if (e == hipSuccess) e = b->d_siteBase.tryReserve((size_t)3 * n_sites);
  if (e == hipSuccess) e = b->d_scratchRow.tryReserve(nc);
  if (e == hipSuccess) e = hipMemset(b->d_prm, 0, nc * SIPNET_NPARAMS * sizeof(double));
  if (e == hipSuccess) e = hipMemset(b->d_state, 0, nc * SIPNET_NSTATE * sizeof(double));
  // (the slots no step has written yet travel with a member's checkpoint and are read back by get_rings: zeros, not what the
  // allocation held)
  if (e == hipSuccess) e = hipMemset(b->d_ring, 0, ringDoubles(b) * sizeof(double));
  if (e == hipSuccess) e = hipEventCreate(&b->ev0);
  if (e == hipSuccess) e = hipEventCreate(&b->ev1);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evBusy, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evStaged, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evOrder, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b->evPlanDone, hipEventDisableTiming);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->upStream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    setError(std::string("sipnet_batch_create: ") + hipGetErrorString(e));
    sipnet_batch_destroy(b);
    return SIPNET_ERR_NO_DEVICE;
  }
  *out = b;
  return SIPNET_OK;
}

void sipnet_batch_destroy(sipnet_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  pfRelease(b);
  for (SiteClim& c : b->sc)
    if (c.evCopied) (void)hipEventDestroy(c.evCopied);
  if (b->evPlanDone) (void)hipEventDestroy(b->evPlanDone);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  if (b->evBusy) (void)hipEventDestroy(b->evBusy);
  if (b->evStaged) (void)hipEventDestroy(b->evStaged);
  if (b->evOrder) (void)hipEventDestroy(b->evOrder);
  if (b->upStream) (void)hipStreamDestroy(b->upStream);
  delete b;
}

int sipnet_batch_set_events(sipnet_batch* b, int32_t site, int32_t n_events,
                            const sipnet_event* events) {
  if (!b || site < 0 || site >= b->n_sites || n_events < 0 || (n_events > 0 && !events)) {
    setError("sipnet_batch_set_events: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  for (int i = 0; i < n_events; i++) {
    if (events[i].type < SIPNET_EV_FERT || events[i].type > SIPNET_EV_LEAFOFF) {
      setError("sipnet_batch_set_events: unknown event type");
      return SIPNET_ERR_UNKNOWN_EVENT;
    }
    // events.c:334-341: records must be in time-ascending order
    if (i > 0 && (events[i].year < events[i - 1].year ||
                  (events[i].year == events[i - 1].year && events[i].day < events[i - 1].day))) {
      setError("sipnet_batch_set_events: event records must be in time-ascending order");
      return SIPNET_ERR_INPUT_FILE;
    }
  }
  b->events[site].assign(events, events + n_events);
  b->planDirty = true;
  return SIPNET_OK;
}

int sipnet_batch_set_params(sipnet_batch* b, int32_t site, int32_t first_member,
                            int32_t count, const double* raw) {
  if (!b || (site != SIPNET_ALL_SITES && (site < 0 || site >= b->n_sites)) || first_member < 0 || count <= 0 ||
      first_member + count > b->n_members || !raw) {
    setError("sipnet_batch_set_params: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  const int32_t nRep = site == SIPNET_ALL_SITES ? b->n_sites : 1;
  if (site == SIPNET_ALL_SITES) site = 0;
  int rc = useDevice(b);
  if (rc) return rc;
  for (int32_t m = 0; m < count; m++) {
    const double* r = raw + (size_t)m * SIPNET_NPARAMS;
    if (r[SP_dVpdExp] != 2.0 || r[SP_soilRespMoistEffect] != 1.0) b->genericExponents = true;
  }
  const int64_t col0 = (int64_t)site * b->n_members + first_member;
  // no upload of earlier rows may still be reading the staging block (an event is recorded behind the copy)
  rc = waitStaged(b);
  if (rc) return rc;
  const size_t need = b->hostRawUsed + (size_t)count;
  const size_t rawCap = b->hostRaw.capacity() / SIPNET_NPARAMS;   // rows
  if (need > rawCap) {   // (the one block that keeps its contents when it grows: into a fresh one, at least twice as large)
    PinnedBuf<double> bigger;
    RC_TRY(bigger.reserve((need > 2 * rawCap ? need : 2 * rawCap) * SIPNET_NPARAMS));
    if (b->hostRawUsed) memcpy(bigger, b->hostRaw, b->hostRawUsed * SIPNET_NPARAMS * sizeof(double));
    b->hostRaw = std::move(bigger);
  }
  memcpy(b->hostRaw + b->hostRawUsed * SIPNET_NPARAMS, raw, (size_t)count * SIPNET_NPARAMS * sizeof(double));
  b->pendingParams.push_back({b->hostRawUsed, col0, count, nRep});
  b->hostRawUsed = need;
  return SIPNET_OK;
}

int sipnet_batch_setup(sipnet_batch* b, void* hip_stream) {
  if (!b) return SIPNET_ERR_BAD_ARGUMENT;
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  b->pfPre.valid = false;   // (log-weights a forecast left, an analysis it was armed for: of the state this call replaces)
  b->pfArm.set = false;
  if (b->planDirty) {
    rc = uploadPlan(b, stream);
    if (rc) return rc;
  }
  rc = flushParams(b, stream);
  if (rc) return rc;
  rc = materializeParams(b, stream);   // (setupModel() for every column from the parameters it carries now)
  if (rc) return rc;
  SetupArgs a;
  a.siteStart = b->d_siteStart;
  a.prm = b->d_prm;
  a.state = b->d_state;
  a.ring = b->d_ring;
  a.ringF32 = b->precision == SIPNET_F32_MIXED;
  a.ncol = b->ncol;
  a.n_sites = b->n_sites;
  a.n_members = b->n_members;
  memcpy(a.flags, b->flags, sizeof(a.flags));
  a.siteStatus = b->d_siteStatus;
  launchSetup(a, stream);
  HIP_TRY(hipGetLastError());
  if (b->d_diag) HIP_TRY(hipMemsetAsync(b->d_diag, 0, (size_t)4 * b->ncol * sizeof(double), stream));
  rc = markBusy(b, stream);
  if (rc) return rc;
  b->stepsDone = 0;
  // a site-fatal plan condition is reported like the reference's exit code
  for (int s = 0; s < b->n_sites; s++) {
    if (b->siteStatus[s] != SIPNET_OK) {
      setError("site " + std::to_string(s) + ": " + b->plans[s].message);
      return b->siteStatus[s];
    }
  }
  return SIPNET_OK;
}

int sipnet_batch_set_math(sipnet_batch* b, int32_t policy) {
  if (!b || (policy != SIPNET_MATH_STRICT && policy != SIPNET_MATH_FAST)) {
    setError("sipnet_batch_set_math: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if (b->precision == SIPNET_F32_MIXED && policy == SIPNET_MATH_STRICT) {
    setError("sipnet_batch_set_math: an fp32-mixed batch has no strict-order arithmetic");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  b->fastMath = policy == SIPNET_MATH_FAST;
  return SIPNET_OK;
}

int sipnet_batch_set_kernel(sipnet_batch* b, int32_t kernel, int32_t options) {
  if (!b || kernel < SIPNET_KERNEL_AUTO || kernel > SIPNET_KERNEL_COOP_NCYCLE_PAIR ||
      (options & ~(SIPNET_KOPT_ONE_WAVE_PER_SIMD | SIPNET_KOPT_RUNTIME_FLAGS | SIPNET_KOPT_FULL_STATE |
                   SIPNET_KOPT_NO_REGULAR_TILES | SIPNET_KOPT_STATS_IN_KERNEL | SIPNET_KOPT_BOUNDED_WAITS | SIPNET_KOPT_WAIT_SELFTEST |
                   SIPNET_KOPT_HOST_PLAN | SIPNET_KOPT_DEVICE_PLAN | SIPNET_KOPT_PF_MULTI_LAUNCH | SIPNET_KOPT_PF_MOVE_PARAMS))) {
    setError("sipnet_batch_set_kernel: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if ((options ^ b->kernelOptions) & (SIPNET_KOPT_HOST_PLAN | SIPNET_KOPT_DEVICE_PLAN)) b->planDirty = true;   // (who builds the plan has changed)
  b->kernelPolicy = kernel;
  b->kernelOptions = options;
  return SIPNET_OK;
}

int sipnet_batch_set_device_share(sipnet_batch* b, int32_t n_filters) {
  if (!b || n_filters < 1 || n_filters > 1024) {
    setError("sipnet_batch_set_device_share: bad argument (1 <= n_filters <= 1024)");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  b->deviceShare = n_filters;
  return SIPNET_OK;
}

int sipnet_debug_set_num_cus(sipnet_batch* b, int32_t num_cus) {
  if (!b || num_cus < 1 || num_cus > 4096) return SIPNET_ERR_BAD_ARGUMENT;
  b->numCUs = num_cus;
  return SIPNET_OK;
}

int sipnet_debug_pf_barrier(sipnet_batch* b, int32_t spin_budget, int32_t absent_workgroup) {
  if (!b || spin_budget < 0) return SIPNET_ERR_BAD_ARGUMENT;
  b->pfSpinBudget = spin_budget;
  b->pfDebugAbsent = absent_workgroup;
  return SIPNET_OK;
}

int sipnet_debug_live_bytes(int64_t* device_bytes, int64_t* pinned_bytes) {
  if (device_bytes) *device_bytes = g_liveDeviceBytes.load();
  if (pinned_bytes) *pinned_bytes = g_livePinnedBytes.load();
  return SIPNET_OK;
}

int sipnet_batch_enable_diagnostics(sipnet_batch* b, int32_t on) {
  if (!b) return SIPNET_ERR_BAD_ARGUMENT;
  int rc = useDevice(b);
  if (rc) return rc;
  if (on && !b->d_diag) {
    RC_TRY(b->d_diag.reserve((size_t)4 * b->ncol));
    HIP_TRY(hipMemset(b->d_diag, 0, (size_t)4 * b->ncol * sizeof(double)));
  } else if (!on && b->d_diag) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(b->d_diag.release());
  }
  return SIPNET_OK;
}

int sipnet_batch_get_diagnostics(sipnet_batch* b, int64_t* n_clamp_warn, int64_t* n_balance_warn,
                                 double* max_abs_dC, double* max_abs_dN, void* hip_stream) {
  if (!b) return SIPNET_ERR_BAD_ARGUMENT;
  if (!b->d_diag) {
    setError("sipnet_batch_get_diagnostics: call sipnet_batch_enable_diagnostics first");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  int rc = useDevice(b);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  std::vector<double> tmp((size_t)4 * b->ncol);
  HIP_TRY(hipMemcpy(tmp.data(), b->d_diag, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t c = 0; c < b->ncol; c++) {
    if (n_clamp_warn) n_clamp_warn[c] = (int64_t)tmp[c];
    if (n_balance_warn) n_balance_warn[c] = (int64_t)tmp[(size_t)b->ncol + c];
    if (max_abs_dC) max_abs_dC[c] = tmp[(size_t)2 * b->ncol + c];
    if (max_abs_dN) max_abs_dN[c] = tmp[(size_t)3 * b->ncol + c];
  }
  return SIPNET_OK;
}

int64_t sipnet_batch_ncol(const sipnet_batch* b) { return b ? b->ncol : 0; }
int32_t sipnet_batch_nsteps(const sipnet_batch* b) { return b ? b->n_steps : 0; }
int32_t sipnet_batch_site_nsteps(const sipnet_batch* b, int32_t site) {
  return (b && site >= 0 && site < b->n_sites) ? b->sc[site].n : 0;
}

}  // extern "C"
