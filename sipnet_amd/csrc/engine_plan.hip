// engine_plan.hip -- the site plans of a batch (engine.hip): the climate handed over, the plan threads, pinned staging and
// the copy stream's event ordering, the device-built plans, uploadPlan and the per-step records sent on first use.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sipnet_amd.h"
#include "batch_impl.h"
#include "plan_pool.h"

static double nowMs() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// -DSIPNET_TRACE_HOST (diagnostic build): where the host side of an upload spends its time / blocks
#ifdef SIPNET_TRACE_HOST
#define TRACE_T(label) fprintf(stderr, "  [host %.3f] %s\n", nowMs(), label)
#else
#define TRACE_T(label)
#endif

// Site plans are independent of each other: they are built by a pool of host threads (one site
// at a time each).  What every launch needs (ring evictions, events, site status, the first
// record's phenology inputs) is uploaded right away; the per-step records -- 256 B per step for
// the strict-order kernel, 256 B per step for the throughput kernels -- are flattened and uploaded
// on the first launch that reads them (ensureStepRecs / ensureFastRecs), so a batch pays for the
// record type it uses only.  bench.py reports the sum as plan_ms.
static int planThreadsFor(int nS) {
  int n = (int)std::thread::hardware_concurrency();
  if (n < 1) n = 1;
  if (n > 16) n = 16;
  return n > nS ? nS : n;
}
// (a worker that fails -- f returns false, or throws: std::bad_alloc on a huge forcing must not reach
// std::terminate in the caller's process -- stops the others at their next site; *failed says so)
template <class F>
static void forEachSite(int nS, int nThreads, std::atomic<bool>* failed, F f) {
  PlanPool::get().run(nS, nThreads, [&](int s) {
    if (failed->load()) return;
    bool ok = false;
    try {
      ok = f(s);
    } catch (...) {
      ok = false;
    }
    if (!ok) failed->store(true);
  });
}

// flat record buffers are written by the worker threads (first touch in parallel), so they are
// allocated without value-initialisation; the batch keeps them for the next hand-over of a forcing
// device buffer for `count` records; a launch that still reads the previous plan (on any stream)
// must have finished before the first site's records land in it
template <class Rec>
static int reserveRecords(sipnet_batch* b, DevBuf<Rec>& buf, size_t count) {
  if (count > buf.capacity()) RC_TRY(waitIdle(b));
  return buf.reserve(count);
}

// Which record type the next launch will read, as far as it is known at setup time: the
// throughput kernels' FastRec, or the strict-order kernel's StepRec.
static bool wantsFastRecs(const sipnet_batch* b) {
  return b->fastMath && b->kernelPolicy != SIPNET_KERNEL_STRICT;
}

// One pass per site (buildSitePlan) writes the record type the batch is set up for straight
// into the flat upload buffer; the other type is produced by a second pass only if a launch ever
// asks for it (ensureRecords).
// (the pinned host blocks are kept between hand-overs of a forcing: a fresh buffer costs its
// first touch -- 143 MB at c4: 24 ms of page faults, more than building the records -- and its pinning)


// ---- device-built site plans (plan_device.h) ---------------------------------------------------------------------------
// Who builds the plans of a hand-over?  The device, unless told otherwise (SIPNET_KOPT_HOST_PLAN) -- or unless this batch's
// own last launch is still running: a caller who hands the next forcing over while the previous one computes (one batch
// back to back, or two batches taking turns: bench.py's pipelined leg) has made the GPU the bottleneck, its host cores are
// idle, and the four plan kernels would only queue behind the step kernel (measured: c2x16 pipelined 9.6 -> 10.1 ms per
// forcing with them, against 14.1 -> 10.7 ms for a forcing handed to an idle device).  SIPNET_KOPT_DEVICE_PLAN: always.
static bool mayBuildOnDevice(const sipnet_batch* b) {
  if (!wantsFastRecs(b) || (b->kernelOptions & SIPNET_KOPT_HOST_PLAN)) return false;
  if (b->kernelOptions & SIPNET_KOPT_DEVICE_PLAN) return true;
  return !stillRunning(const_cast<sipnet_batch*>(b));
}
// the site's forcing block -> its device block, asynchronously on the copy stream (behind the plan kernels that may still
// be reading the previous forcing there)
static int sendClimate(sipnet_batch* b, int32_t site) {
  SiteClim& c = b->sc[site];
  const size_t bytes = SiteClim::bytesFor(c.n);
  if (bytes > c.dev.capacity()) {
    if (b->planKernelsQueued) HIP_TRY(hipEventSynchronize(b->evPlanDone));
    RC_TRY(c.dev.reserve(bytes + bytes / 8));
  }
  if (b->planKernelsQueued) HIP_TRY(hipStreamWaitEvent(b->upStream, b->evPlanDone, 0));
  HIP_TRY(hipMemcpyAsync(c.dev, c.host, bytes, hipMemcpyHostToDevice, b->upStream));
  if (!c.evCopied) HIP_TRY(hipEventCreateWithFlags(&c.evCopied, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c.evCopied, b->upStream));
  c.copyQueued = true;
  c.onDevice = true;
  return SIPNET_OK;
}
// The plan threads' pass over a site before anybody builds its records (plan.cpp buildSitePlanLight): the GDD chain, the
// events per record and the tillage series, the site-fatal conditions -- and may the DEVICE build the records?  Every step
// (and every whole entry of a resumed ring) at least kDevPlanMinLen long, so that the ring cannot overflow; no site-fatal
// condition (the host path words the reference's message); step lengths in long runs: one lane walks the ring's schedule
// outside such runs at ~0.5 us a step (profiles/r05_plan_device.txt; a host core builds a whole step in 0.07 us), so a
// half-daily forcing like niwot's stays with the host unless SIPNET_KOPT_DEVICE_PLAN asks.
static bool devicePrepass(sipnet_batch* b, int32_t s, PlanLight* out) {
  const SiteClim& c = b->sc[s];
  const size_t nT = (size_t)b->n_steps;
  const bool ev = b->hostEv.get() != nullptr;
  unsigned char* e = ev ? b->hostEv + (size_t)s * nT * 24 : nullptr;
  const PlanCarry* init = b->resume[s].set ? &b->resume[s] : nullptr;
  *out = buildSitePlanLight(b->flags, c.n, c.clim(), c.year(), c.day(), (int32_t)b->events[s].size(), b->events[s].data(), init,
                            kDevPlanMinLen, kDevPlanMinRun, b->hostGdd + (size_t)s * nT, (int32_t*)e, (int32_t*)(e + 4 * nT),
                            (double*)(e + 8 * nT), (double*)(e + 16 * nT));
  if (out->status != SIPNET_OK || !out->lengthsOk) return false;
  if (init) {   // the ring a checkpoint hands over: its whole entries (all but the front one) count like steps
    const RingSched& r = init->ring;
    for (int i = (r.start + 1) % SIPNET_RING_SLOTS; i != (r.last + 1) % SIPNET_RING_SLOTS && r.start != r.last; i = (i + 1) % SIPNET_RING_SLOTS)
      if (!(r.w[i] >= kDevPlanMinLen)) return false;
    if (!(r.w[r.start] > 0)) return false;
    // ... and together they carry the 5-day window: a ring that holds more reaches the reference's "ring full" stop
    // (runmean.c:93-95), one that holds less runs empty -- the host builder reports the first and walks the second as the
    // reference does; the device walk is only handed rings it cannot leave (its status word is a debugging aid)
    double sum = 0.0;
    for (int i = r.start;; i = (i + 1) % SIPNET_RING_SLOTS) {
      sum += r.w[i];
      if (i == r.last) break;
    }
    if (!(std::fabs(sum - 5.0) <= 1e-9)) return false;
  }
  return out->walked <= kDevPlanMaxWalked || (b->kernelOptions & SIPNET_KOPT_DEVICE_PLAN);
}

static int buildAndUpload(sipnet_batch* b, bool fastType, bool first, hipStream_t stream) {
  const double t0 = nowMs();
  const int nS = b->n_sites, nT = b->n_steps;   // nT: the longest site's records = the stride of the record arrays
  const int nThreads = planThreadsFor(nS);
  const size_t nFast = (size_t)nS * nT + kFastTile, nSteps = (size_t)nS * nT;
  TRACE_T("plan: begin");
  // the staging block must be free (the copies of the previous hand-over done: an event behind them); the DEVICE
  // records may still be read by this batch's last launch -- then the sites are built first (host only) and sent
  // once that launch has finished, instead of as they are built
  int rc = waitStaged(b);
  if (rc) return rc;
  rc = fastType ? reserveRecords(b, b->d_fast, nFast) : reserveRecords(b, b->d_plan, nSteps);
  if (rc) return rc;
  const bool deferCopies = stillRunning(b);
  // (sites whose records the device builds itself need no staging: plan_device.h)
  const bool devPass = fastType && first && b->nDevSites > 0;
  const bool anyHostSite = !devPass || b->nDevSites < nS;
  if (anyHostSite) rc = fastType ? b->hostFast.reserve(nFast) : b->hostSteps.reserve(nSteps);
  if (rc) return rc;
  TRACE_T("plan: reserved");
  FastRec* const fast = b->hostFast;
  StepRec* const steps = b->hostSteps;
  // every worker sends off the site it has just built while the others go on building: asynchronous copies out
  // of the pinned block on the caller's stream (the setup and step kernels that follow on it are ordered behind
  // them; the host does not wait, and nothing here needs a compute queue)
  std::atomic<int> copyErr{0};
  std::atomic<int64_t> copyUs{0};
  std::atomic<bool> failed{false};
  forEachSite(nS, nThreads, &failed, [&](int s) -> bool {
    const int nTs = b->siteSteps[s];            // this site's own length (its tail of the stride is never read)
    if (devPass && b->devSite[s]) {             // what the host still needs of such a site: setupModel()'s inputs, its events
      PlanLight& l = b->planLight[s];
      SitePlan p;
      p.startCumGdd = l.startCumGdd;
      p.startTsoil = l.startTsoil;
      p.startDayTime = l.startDayTime;
      p.events = std::move(l.events);
      b->plans[s] = std::move(p);
      return true;
    }
    SitePlan p = buildSitePlan(b->flags, nTs, b->sc[s].clim(), b->sc[s].year(), b->sc[s].day(),
                               (int32_t)b->events[s].size(), b->events[s].data(),
                               b->resume[s].set ? &b->resume[s] : nullptr, nullptr, /*wantSteps=*/false,
                               fastType ? nullptr : steps + (size_t)s * nT,
                               fastType ? fast + (size_t)s * nT : nullptr,
                               /*narrowFast=*/b->precision == SIPNET_F32_MIXED);
    if (first) b->plans[s] = std::move(p);
    const double c0 = nowMs();
    const size_t tail = (fastType && s == nS - 1) ? kFastTile : 0;  // tile padding after the last site
    if (tail) memset((void*)(fast + (size_t)nS * nT), 0, tail * sizeof(FastRec));
    if (deferCopies) return true;
    hipError_t e = hipSetDevice(b->device);
    if (e == hipSuccess) {
      e = fastType ? hipMemcpyAsync(b->d_fast + (size_t)s * nT, fast + (size_t)s * nT, ((size_t)nT + tail) * sizeof(FastRec),
                                    hipMemcpyHostToDevice, b->upStream)
                   : hipMemcpyAsync(b->d_plan + (size_t)s * nT, steps + (size_t)s * nT, (size_t)nT * sizeof(StepRec),
                                    hipMemcpyHostToDevice, b->upStream);
    }
    if (e != hipSuccess) {
      int none = 0;
      copyErr.compare_exchange_strong(none, (int)e);   // the FIRST error is the one reported
    }
    copyUs.fetch_add((int64_t)((nowMs() - c0) * 1e3));
    return e == hipSuccess;
  });
  if (copyErr.load() != 0) {
    setError(std::string("sipnet_batch: uploading the site records failed: ") + hipGetErrorString((hipError_t)copyErr.load()));
    return SIPNET_ERR_INTERNAL;
  }
  if (failed.load()) {
    setError("sipnet_batch: building the site plans failed (out of host memory?)");
    return SIPNET_ERR_INTERNAL;
  }
  if (deferCopies && anyHostSite) {   // once this batch's last launch is through with the old records
    rc = waitIdle(b);
    if (rc) return rc;
    if (!devPass) {   // everything in one piece
      if (fastType) HIP_TRY(hipMemcpyAsync(b->d_fast, fast, nFast * sizeof(FastRec), hipMemcpyHostToDevice, b->upStream));
      else HIP_TRY(hipMemcpyAsync(b->d_plan, steps, nSteps * sizeof(StepRec), hipMemcpyHostToDevice, b->upStream));
    } else {
      for (int s2 = 0; s2 < nS; s2++)
        if (!b->devSite[s2])
          HIP_TRY(hipMemcpyAsync(b->d_fast + (size_t)s2 * nT, fast + (size_t)s2 * nT,
                                 ((size_t)nT + (s2 == nS - 1 ? kFastTile : 0)) * sizeof(FastRec), hipMemcpyHostToDevice, b->upStream));
    }
  }
  if (deferCopies && !anyHostSite) {
    // every site is the device's (SIPNET_KOPT_DEVICE_PLAN forced while the previous launch still runs): nothing above has
    // waited for that launch, and the copy stream is about to overwrite what it reads -- the tile padding here, the site
    // bases / status / starts / events in uploadPlan.  A device-side wait: the host does not stop.
    rc = orderBehindBusy(b, b->upStream);
    if (rc) return rc;
  }
  // the tile padding behind the last site, when that one is the device's
  if (devPass && b->devSite[nS - 1]) HIP_TRY(hipMemsetAsync(b->d_fast + (size_t)nS * nT, 0, kFastTile * sizeof(FastRec), b->upStream));
  TRACE_T("plan: sites built, copies enqueued");
  (fastType ? b->fastRecsUploaded : b->stepRecsUploaded) = true;
  // wall time of the whole pass; the workers' share spent enqueueing the copies is reported as the upload part
  // (the copies themselves run on the stream, under the build of the following sites)
  const double wall = nowMs() - t0, copyShare = copyUs.load() * 1e-3 / nThreads;
  b->planBuildMs += wall - (copyShare < wall ? copyShare : wall);
  b->planUploadMs += copyShare < wall ? copyShare : wall;
  rc = joinUploads(b, stream);
  return rc ? rc : markBusy(b, stream);
}

// FastRec::log2vpd of the device-built records -- read only by members whose dVpdExp is not 2 (FastArgs::plainExp): the
// host's log2 (glibc's, as plan.cpp takes it), computed by the plan threads when such a member exists, sent and written
// into the records; the device's own log2 differs from it in the last bit now and then.
int fillDeviceLog2(sipnet_batch* b, hipStream_t stream) {
  const int nS = b->n_sites, nT = b->n_steps, nDev = b->nDevSites;
  int rc = waitStaged(b);
  if (rc) return rc;
  rc = b->hostLog2.reserve((size_t)nDev * nT);
  if (rc) return rc;
  std::vector<int> siteOf;
  for (int s = 0; s < nS; s++)
    if (b->devSite[s]) siteOf.push_back(s);
  std::atomic<bool> none{false};
  forEachSite(nDev, planThreadsFor(nDev), &none, [&](int d) -> bool {
    const SiteClim& c = b->sc[siteOf[d]];
    double* out = b->hostLog2 + (size_t)d * nT;
    for (int32_t t = 0; t < c.n; t++) {
      const double vpd = c.clim()[(size_t)SIPNET_NCLIM * t + 5];
      out[t] = std::log2(vpd > 0 ? vpd : 0.000001);   // plan.cpp: log2 of vpd, of TINY (common/util.h:14) when not positive
    }
    return true;
  });
  HIP_TRY(hipMemcpyAsync(b->d_devLog2, b->hostLog2, (size_t)nDev * nT * sizeof(double), hipMemcpyHostToDevice, b->upStream));
  rc = joinUploads(b, stream);
  if (rc) return rc;
  launchDevicePlanLog2(b->devPlan.sites, nDev, nT, b->devPlanMaxSteps, b->d_fast, b->d_devLog2, b->precision == SIPNET_F32_MIXED, stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(b->evPlanDone, stream));
  b->devLog2Done = true;
  return markBusy(b, stream);
}

// Room for a device-built site's eviction list.  Every eviction either removes a whole entry (at most one per entry that ever
// lived: the n inserted ones + the preK a checkpoint's ring starts with, one for a fresh ring) or ends its step (at most n):
// 2 n + preK, + 8 spare.  The walk and planRunsKernel are also handed the number and stop writing at it (DevPlanSite::opCap).
static int32_t devRingPreK(const sipnet_batch* b, int s) {
  if (!b->resume[s].set) return 1;
  const RingSched& r = b->resume[s].ring;
  return (r.last - r.start + SIPNET_RING_SLOTS) % SIPNET_RING_SLOTS + 1;
}
static size_t devRingOpRoom(const sipnet_batch* b, int s) { return (size_t)2 * b->siteSteps[s] + devRingPreK(b, s) + 8; }

// The device-built sites' records: scratch carved out of one block, the site table sent, the four plan kernels queued on
// the caller's stream behind the climate copies.
static int buildOnDevice(sipnet_batch* b, const std::vector<int32_t>& bases, hipStream_t stream) {
  const int nS = b->n_sites, nT = b->n_steps, nDev = b->nDevSites;
  auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const int32_t runCap = devPlanRunCap(nT), nBlk = (nT + 255) / 256;
  const size_t perStep = (size_t)nDev * nT;
  const size_t offSites = 0, offLen = offSites + align(nDev * sizeof(DevPlanSite)), offGdd = offLen + align(perStep * sizeof(double)),
               offSeq = offGdd + align(perStep * sizeof(double)), offRuns = offSeq + align(perStep * sizeof(DevPlanSeq)),
               offOut = offRuns + align((size_t)nDev * runCap * sizeof(DevPlanRun)), offLog2 = offOut + align((size_t)nDev * 8 * sizeof(int32_t)),
               offBlk = offLog2 + align(perStep * sizeof(double)), offPre = offBlk + align((size_t)nDev * nBlk * 2 * sizeof(int32_t)),
               offEv = offPre + align((size_t)nDev * SIPNET_RING_SLOTS * sizeof(double)),
               total = offEv + (b->hostEv ? align(perStep * 24) : 0);
  // (the events block: evFirst[nDev][nT], evCount[nDev][nT], dTill[nDev][nT], tillAfter[nDev][nT])
  const size_t offEvCount = offEv + perStep * 4, offDTill = offEv + perStep * 8, offTillAfter = offEv + perStep * 16;
  if (total > b->d_planScratch.capacity()) {
    if (b->planKernelsQueued) HIP_TRY(hipEventSynchronize(b->evPlanDone));
    RC_TRY(b->d_planScratch.reserve(total));
  }
  // the site table (pinned staging: the small-array block is free again only after its copies, so a block of its own)
  std::vector<DevPlanSite> tab(nDev);
  std::vector<double> preW((size_t)nDev * SIPNET_RING_SLOTS, 0.0);
  int32_t maxSteps = 0;
  // (the scratch block is rewritten: behind the previous forcing's plan kernels)
  if (b->planKernelsQueued) HIP_TRY(hipStreamWaitEvent(b->upStream, b->evPlanDone, 0));
  for (int s = 0, d = 0; s < nS; s++) {
    if (!b->devSite[s]) continue;
    SiteClim& c = b->sc[s];
    if (!c.onDevice) {
      int rc = sendClimate(b, s);
      if (rc) return rc;
    }
    // the host's GDD chains (uploadPlan): one copy per run of neighbouring device-built sites (32 copies of 140 KB kept the
    // copy stream busy for 0.6 ms; rows are nT apart on both sides)
    if (b->flags[SIPNET_F_GDD] && (s == 0 || !b->devSite[s - 1])) {
      int e = s;
      while (e < nS && b->devSite[e]) e++;
      HIP_TRY(hipMemcpyAsync(b->d_planScratch + offGdd + (size_t)d * nT * sizeof(double), b->hostGdd + (size_t)s * nT,
                             (size_t)(e - s) * nT * sizeof(double), hipMemcpyHostToDevice, b->upStream));
    }
    const bool hasEv = b->planLight[s].hasEvents && b->hostEv;
    if (hasEv) {   // the events on each record and the tillage series (plan.cpp buildSitePlanLight)
      const unsigned char* h = b->hostEv + (size_t)s * nT * 24;
      unsigned char* dv = b->d_planScratch;
      HIP_TRY(hipMemcpyAsync(dv + offEv + (size_t)d * nT * 4, h, (size_t)c.n * 4, hipMemcpyHostToDevice, b->upStream));
      HIP_TRY(hipMemcpyAsync(dv + offEvCount + (size_t)d * nT * 4, h + 4 * (size_t)nT, (size_t)c.n * 4, hipMemcpyHostToDevice, b->upStream));
      HIP_TRY(hipMemcpyAsync(dv + offDTill + (size_t)d * nT * 8, h + 8 * (size_t)nT, (size_t)c.n * 8, hipMemcpyHostToDevice, b->upStream));
      HIP_TRY(hipMemcpyAsync(dv + offTillAfter + (size_t)d * nT * 8, h + 16 * (size_t)nT, (size_t)c.n * 8, hipMemcpyHostToDevice, b->upStream));
    }
    DevPlanSite& e = tab[d];
    e.clim = c.devClim();
    e.year = c.devYear();
    e.day = c.devDay();
    e.preW = (const double*)(b->d_planScratch + offPre) + (size_t)d * SIPNET_RING_SLOTS;
    e.n = c.n;
    e.site = s;
    e.opBase = bases[3 * s];
    // the ring the walk starts from: a fresh one (one entry carrying the 5-day window, runmean.c:44-52), or a checkpoint's
    double* pw = preW.data() + (size_t)d * SIPNET_RING_SLOTS;
    if (b->resume[s].set) {
      const PlanCarry& rc0 = b->resume[s];
      e.preK = devRingPreK(b, s);
      e.preStart = rc0.ring.start;
      e.preIns = 0;
      for (int i = 0; i < e.preK; i++) pw[i] = rc0.ring.w[(rc0.ring.start + i) % SIPNET_RING_SLOTS];
      e.phenInit = rc0.phenLastYear;
      e.trackInit = rc0.trackLastYear;
    } else {
      e.preK = 1;
      e.preStart = 0;
      e.preIns = -1;
      pw[0] = 5.0;                // MEAN_NPP_DAYS, sipnet.c:39
      e.phenInit = c.year()[0];   // sipnet.c:1524
      e.trackInit = -1;           // sipnet.c:1412
    }
    e.hasEvents = hasEv ? 1 : 0;
    e.opCap = (int32_t)devRingOpRoom(b, s);
    d++;
    maxSteps = std::max(maxSteps, c.n);
  }
  // (a pageable source: the runtime stages these few hundred bytes itself before the call returns)
  HIP_TRY(hipMemcpyAsync(b->d_planScratch + offSites, tab.data(), nDev * sizeof(DevPlanSite), hipMemcpyHostToDevice, b->upStream));
  HIP_TRY(hipMemcpyAsync(b->d_planScratch + offPre, preW.data(), preW.size() * sizeof(double), hipMemcpyHostToDevice, b->upStream));
  int rc = joinUploads(b, stream);
  if (rc) return rc;
  DevPlanArgs& a = b->devPlan;
  a.sites = (const DevPlanSite*)(b->d_planScratch + offSites);
  a.nDev = nDev;
  a.nT = nT;
  a.fast = b->d_fast;
  a.ringOps = b->d_ringOps;
  a.lenC = (double*)(b->d_planScratch + offLen);
  a.gddAfter = (const double*)(b->d_planScratch + offGdd);
  a.evFirst = (const int32_t*)(b->d_planScratch + offEv);
  a.evCount = (const int32_t*)(b->d_planScratch + offEvCount);
  a.dTill = (const double*)(b->d_planScratch + offDTill);
  a.tillAfter = (const double*)(b->d_planScratch + offTillAfter);
  a.seq = (DevPlanSeq*)(b->d_planScratch + offSeq);
  a.runs = (DevPlanRun*)(b->d_planScratch + offRuns);
  a.runCap = runCap;
  a.blockInfo = (int32_t*)(b->d_planScratch + offBlk);
  a.nBlk = nBlk;
  a.siteOut = (int32_t*)(b->d_planScratch + offOut);
  a.flagGdd = b->flags[SIPNET_F_GDD] != 0;
  a.phenMode = b->flags[SIPNET_F_GDD] ? 0 : b->flags[SIPNET_F_SOIL_PHENOL] ? 1 : 2;
  a.moistHResp = b->flags[SIPNET_F_WATER_HRESP] != 0;
  a.narrow = b->precision == SIPNET_F32_MIXED;
  a.convS = planConvS();
  a.convE = planConvE();
  b->d_devLog2 = (double*)(b->d_planScratch + offLog2);
  b->devPlanMaxSteps = maxSteps;
  launchDevicePlan(a, maxSteps, stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(b->evPlanDone, stream));
  b->planKernelsQueued = true;
  b->devLog2Done = false;
  rc = markBusy(b, stream);
  if (rc) return rc;
  return b->genericExponents ? fillDeviceLog2(b, stream) : SIPNET_OK;
}

int uploadPlan(sipnet_batch* b, hipStream_t stream) {
  // every site needs a forcing; they may differ in length (a launch advances each site to the end of ITS records)
  const int nS = b->n_sites;
  b->siteSteps.assign(nS, 0);
  b->n_steps = 0;
  for (int s = 0; s < nS; s++) {
    if (b->sc[s].n <= 0) {
      setError("sipnet_batch: climate not set for every site");
      return SIPNET_ERR_BAD_ARGUMENT;
    }
    b->siteSteps[s] = b->sc[s].n;
    if (b->siteSteps[s] > b->n_steps) b->n_steps = b->siteSteps[s];
  }
  b->plans.clear();
  b->plans.resize(nS);
  b->stepRecsUploaded = false;
  b->fastRecsUploaded = false;
  b->planBuildMs = b->planUploadMs = 0.0;
  b->planThreads = planThreadsFor(nS);
  // which sites' records the device builds from the climate it has been sent (plan_device.h)
  std::fill(b->devSite.begin(), b->devSite.end(), 0);
  b->nDevSites = 0;
  if (mayBuildOnDevice(b)) {
    int rcW = waitStaged(b);   // (the previous hand-over's copies out of the staging blocks)
    if (rcW) return rcW;
    rcW = b->hostGdd.reserve((size_t)nS * b->n_steps);
    if (rcW) return rcW;
    bool anyEvents = false;
    for (int s = 0; s < nS; s++)
      anyEvents |= (b->flags[SIPNET_F_EVENTS] && !b->events[s].empty()) || (b->resume[s].set && b->resume[s].dTill != 0.0);
    if (anyEvents) {
      rcW = b->hostEv.reserve((size_t)nS * b->n_steps * 24);
      if (rcW) return rcW;
    } else if (b->hostEv) {   // (no site has events this time: the block is not looked at)
      HIP_TRY(b->hostEv.release());
    }
    b->planLight.assign(nS, PlanLight{});
    std::atomic<bool> none{false};
    forEachSite(nS, b->planThreads, &none, [&](int s) -> bool {
      b->devSite[s] = devicePrepass(b, s, &b->planLight[s]) ? 1 : 0;
      return true;
    });
    for (int s = 0; s < nS; s++) b->nDevSites += b->devSite[s];
    // the plan kernels overwrite records this batch's last launch may still be reading on another stream
    if (b->nDevSites) {
      int rcO = orderBehindBusy(b, stream);
      if (rcO) return rcO;
    }
  }
  int rc = buildAndUpload(b, wantsFastRecs(b), /*first=*/true, stream);
  if (rc) return rc;
  const double t0 = nowMs();
  // ring evictions and events of all sites in one array each; the records index them site-locally
  // and the kernels add the site's base
  std::vector<int32_t> bases((size_t)3 * nS);   // per site: ring-op base, event base, number of records
  std::vector<SiteStart> starts(nS);
  size_t nOps = 0, nEv = 0;
  for (int s = 0; s < nS; s++) {
    const SitePlan& p = b->plans[s];
    b->siteStatus[s] = p.status;
    bases[3 * s] = (int32_t)nOps;
    bases[3 * s + 1] = (int32_t)nEv;
    bases[3 * s + 2] = b->siteSteps[s];
    nOps += b->devSite[s] ? devRingOpRoom(b, s) : p.ringOps.size();   // (the device's list: room for the bound)
    nEv += p.events.size();
    starts[s] = SiteStart{p.startCumGdd, p.startTsoil, p.startDayTime};
  }
  const double t1 = nowMs();
  RC_TRY(b->d_ringOps.reserve(nOps + 1));
  RC_TRY(b->d_events.reserve(nEv + 1));
  // the small arrays: flattened into one pinned block and sent on the same stream (buildAndUpload has waited for
  // every launch that might still read the previous plan; an empty list keeps one inert entry)
  // (ring evictions: the HOST-built sites' only -- a device-built site's list is written by its walk, and its room in the flat
  // array, 2 n + preK + 8 entries, is not sent: 18 MB and 0.32 ms of the copy stream at 32 sites x 17 520 records)
  size_t nHostOps = 0;
  for (int s = 0; s < nS; s++)
    if (!b->devSite[s]) nHostOps += b->plans[s].ringOps.size();
  const size_t opsBytes = (nHostOps ? nHostOps : 1) * sizeof(RingOp), evBytes = (nEv ? nEv : 1) * sizeof(EvRec);
  auto align16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const size_t offEv = align16(opsBytes), offStatus = offEv + align16(evBytes), offStart = offStatus + align16(nS * sizeof(int32_t)),
               offBase = offStart + align16(nS * sizeof(SiteStart)), total = offBase + align16(bases.size() * sizeof(int32_t));
  rc = b->hostMisc.reserve(total);
  if (rc) return rc;
  RingOp* hOps = (RingOp*)b->hostMisc.get();
  EvRec* hEv = (EvRec*)(b->hostMisc + offEv);
  std::vector<size_t> hostOff(nS, 0);
  {
    size_t off = 0;
    for (int s = 0; s < nS; s++) {
      const SitePlan& p = b->plans[s];
      hostOff[s] = off;
      if (!b->devSite[s] && !p.ringOps.empty()) {
        memcpy(hOps + off, p.ringOps.data(), p.ringOps.size() * sizeof(RingOp));
        off += p.ringOps.size();
      }
      if (!p.events.empty()) memcpy(hEv + bases[3 * s + 1], p.events.data(), p.events.size() * sizeof(EvRec));
    }
  }
  if (nEv == 0) hEv[0] = EvRec{0, 0, {0, 0, 0, 0}};
  memcpy(b->hostMisc + offStatus, b->siteStatus.data(), nS * sizeof(int32_t));
  memcpy(b->hostMisc + offStart, starts.data(), nS * sizeof(SiteStart));
  memcpy(b->hostMisc + offBase, bases.data(), bases.size() * sizeof(int32_t));
  if (nOps == 0) {
    hOps[0] = RingOp{0.0, 0, -1};
    HIP_TRY(hipMemcpyAsync(b->d_ringOps, hOps, sizeof(RingOp), hipMemcpyHostToDevice, b->upStream));
  }
  for (int s = 0; s < nS;) {   // runs of neighbouring host-built sites: contiguous here and there
    if (b->devSite[s]) { s++; continue; }
    int e = s;
    size_t cnt = 0;
    while (e < nS && !b->devSite[e]) cnt += b->plans[e++].ringOps.size();
    if (cnt) HIP_TRY(hipMemcpyAsync(b->d_ringOps + bases[3 * s], hOps + hostOff[s], cnt * sizeof(RingOp), hipMemcpyHostToDevice, b->upStream));
    s = e;
  }
  HIP_TRY(hipMemcpyAsync(b->d_events, hEv, evBytes, hipMemcpyHostToDevice, b->upStream));
  HIP_TRY(hipMemcpyAsync(b->d_siteStatus, b->hostMisc + offStatus, nS * sizeof(int32_t), hipMemcpyHostToDevice, b->upStream));
  HIP_TRY(hipMemcpyAsync(b->d_siteStart, b->hostMisc + offStart, nS * sizeof(SiteStart), hipMemcpyHostToDevice, b->upStream));
  HIP_TRY(hipMemcpyAsync(b->d_siteBase, b->hostMisc + offBase, bases.size() * sizeof(int32_t), hipMemcpyHostToDevice, b->upStream));
  rc = joinUploads(b, stream);
  if (rc) return rc;
  rc = markBusy(b, stream);
  if (rc) return rc;
  TRACE_T("plan: small arrays enqueued");
  if (b->nDevSites) {
    rc = buildOnDevice(b, bases, stream);
    if (rc) return rc;
  }
  b->planDirty = false;
  b->exportCacheSite = -1;
  b->planBuildMs += t1 - t0;
  b->planUploadMs += nowMs() - t1;
  return SIPNET_OK;
}

int ensureStepRecs(sipnet_batch* b, hipStream_t stream) {  // records of the strict-order kernel
  return b->stepRecsUploaded ? SIPNET_OK : buildAndUpload(b, /*fastType=*/false, /*first=*/false, stream);
}
int ensureFastRecs(sipnet_batch* b, hipStream_t stream) {  // records of the throughput kernels
  return b->fastRecsUploaded ? SIPNET_OK : buildAndUpload(b, /*fastType=*/true, /*first=*/false, stream);
}

// the host side of a hand-over of one site's forcing, in three parts so that the copies of several sites can run on the
// plan threads (sipnet_batch_set_climate_sites): room in the pinned block, the copy, the send-off
static int climateReserve(sipnet_batch* b, int32_t site, int32_t n_steps) {
  SiteClim& c = b->sc[site];
  const size_t bytes = SiteClim::bytesFor(n_steps);
  // the previous forcing's copy out of this block must be through before the host writes it again
  if (c.copyQueued) HIP_TRY(hipEventSynchronize(c.evCopied));
  c.copyQueued = false;
  if (bytes > c.host.capacity()) RC_TRY(c.host.reserve(bytes + bytes / 8));
  c.n = n_steps;
  c.onDevice = false;
  return SIPNET_OK;
}
static void climateCopy(sipnet_batch* b, int32_t site, const double* clim, const int32_t* year, const int32_t* day) {
  SiteClim& c = b->sc[site];
  memcpy(c.host, clim, (size_t)c.n * SIPNET_NCLIM * sizeof(double));
  memcpy((void*)c.year(), year, (size_t)c.n * sizeof(int32_t));
  memcpy((void*)c.day(), day, (size_t)c.n * sizeof(int32_t));
}
static void climateDone(sipnet_batch* b) {
  b->n_steps = 0;   // the longest site set so far (sites may differ in length; the plan is rebuilt anyway)
  for (int s = 0; s < b->n_sites; s++) b->n_steps = std::max<int32_t>(b->n_steps, b->sc[s].n);
  b->planDirty = true;
}

extern "C" {

int sipnet_batch_set_climate(sipnet_batch* b, int32_t site, int32_t n_steps,
                             const double* clim, const int32_t* year, const int32_t* day) {
  if (!b || site < 0 || site >= b->n_sites || n_steps <= 0 || !clim || !year || !day) {
    setError("sipnet_batch_set_climate: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  int rc = useDevice(b);
  if (rc) return rc;
  rc = climateReserve(b, site, n_steps);
  if (rc) return rc;
  climateCopy(b, site, clim, year, day);
  climateDone(b);
  // a batch that may build the site's plan on the device sends the forcing off now: the copy runs under the caller's
  // preparation of the next site (63 MB at 32 sites x 17 520 records, against 143 MB of host-built records)
  return mayBuildOnDevice(b) ? sendClimate(b, site) : SIPNET_OK;
}

int sipnet_batch_set_climate_sites(sipnet_batch* b, int32_t first_site, int32_t count, const int32_t* n_steps,
                                   const double* const* clim, const int32_t* const* year, const int32_t* const* day) {
  if (!b || first_site < 0 || count <= 0 || first_site + count > b->n_sites || !n_steps || !clim || !year || !day) {
    setError("sipnet_batch_set_climate_sites: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  for (int32_t k = 0; k < count; k++) {
    if (n_steps[k] <= 0 || !clim[k] || !year[k] || !day[k]) {
      setError("sipnet_batch_set_climate_sites: bad argument");
      return SIPNET_ERR_BAD_ARGUMENT;
    }
  }
  int rc = useDevice(b);
  if (rc) return rc;
  for (int32_t k = 0; k < count; k++) {
    rc = climateReserve(b, first_site + k, n_steps[k]);
    if (rc) return rc;
  }
  // (each thread sends its site off as soon as it is copied, so the DMA of the first sites runs under the copies of the
  // others.  Eight threads: the copies are bound by the host's memory fabric -- 63 MB in 1.6 ms = 39 GB/s of copy on this
  // box, the 36 us DMAs wait for them; sixteen threads were slower, 1.9 ms, and slowed the DMAs to 55 us)
  const bool send = mayBuildOnDevice(b);
  std::atomic<int> firstErr{0};
  std::string errText;
  std::mutex errMu;
  PlanPool::get().run(count, std::min(planThreadsFor(count), 8), [&](int k) {
    climateCopy(b, first_site + k, clim[k], year[k], day[k]);
    if (!send) return;
    int rcS = useDevice(b);
    if (!rcS) rcS = sendClimate(b, first_site + k);
    int none = 0;
    if (rcS && firstErr.compare_exchange_strong(none, rcS)) {
      std::lock_guard<std::mutex> lk(errMu);
      errText = sipnet_last_error();   // (the error text is per thread: carried to the caller's)
    }
  });
  climateDone(b);
  if (firstErr.load()) {
    setError(errText);
    return firstErr.load();
  }
  return SIPNET_OK;
}

}  // extern "C"
