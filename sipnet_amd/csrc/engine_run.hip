// engine_run.hip -- one launch of a batch (engine.hip): which step kernel, what it needs on the device first, the launch, the
// statistics behind it.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/sipnet_amd.h"
#include "batch_impl.h"

// The shape-based kernel choice of SIPNET_KERNEL_AUTO (also exported as sipnet_kernel_choice, so
// that tools and tests can ask without a device).
// Few 64-member chunks per CU: the step is bound by what one wavefront can issue, so three
// wavefronts share each chunk (step_coop.hip) -- with the chunk's ring in LDS when there is
// at most one chunk per CU (c10k 9.0 vs 18.2 ms); up to two per CU as ONE eight-wave workgroup
// per CU carrying two chunks with their rings in HBM, which keeps every carbon wave alone on
// its SIMD (c4 10.6 ms; two three-wave workgroups per CU: 12.4; one-wave kernel: 19.3).
// Up to four per CU: one twelve-wave workgroup per four chunks, every SIMD running the three
// waves of one chunk (c3 13.0 ms; one-wave kernel 15.3); no full-state build of that one (VGPRs).
// Bigger batches fill the SIMDs with the one-wave kernel, two waves per SIMD.
// The nitrogen-cycle flag set has cooperative kernels of its own (lean state; a soil wave S next to
// L, W, C: one chunk per CU in 213 registers / 71 KB of LDS, or two chunks per eight-wave workgroup);
// every other optional flag set takes the one-wave kernel.  Strict arithmetic and the debug plane: the strict-order kernel.  Full records,
// diagnostics and SIPNET_KOPT_FULL_STATE: the "Full" instantiations of the same throughput kernels.
// wantFull: 0 lean, 1 record / SIPNET_KOPT_FULL_STATE, 2 diagnostics counters as well
static int autoKernel(const int32_t* flags, int32_t n_sites, int32_t n_members, bool fastMath, bool debugPlane,
                      int wantFull, int32_t numCUs, bool f32) {
  const bool defaultFlags = isDefaultFlagSet(flags);
  const int64_t blocks = (int64_t)n_sites * ((n_members + 63) / 64);
  if (!fastMath || debugPlane) return SIPNET_KERNEL_STRICT;
  if (!flags[SIPNET_F_NITROGEN_CYCLE]) {
    // default physics, or -- up to two chunks per CU -- its optional-physics instantiations
    // (growth respiration, leaf water, flooding, litter pool, carbon saturation, anaerobic: run-time flags)
    const bool ext = !defaultFlags;
    if (blocks <= (int64_t)numCUs) return SIPNET_KERNEL_COOP_LDS;
    if (blocks <= 2 * (int64_t)numCUs) return SIPNET_KERNEL_COOP_PAIR;
    // (four chunks per CU with optional physics: the fp32-mixed build only -- the fp64 one would spill, step_coop.hip)
    if ((!ext || f32) && blocks <= 4 * (int64_t)numCUs && !wantFull) return SIPNET_KERNEL_COOP_QUAD;
    return SIPNET_KERNEL_ONE_WAVE;
  }
  // the nitrogen cycle (with litter pool + anaerobic, which it requires), alone or with the other options; full state
  // (record, every accumulator) and the diagnostics counters (wantFull == 2) too -- the plant side's mass totals travel to
  // the soil wave through eleven more mailbox rows: two slots of them on the one-chunk layout, one per chunk on the two-chunk
  // layout (round 6: the carbon wave waits for the soil wave's balance check of the step before; coop_mailboxes.inc)
  if (blocks <= (int64_t)numCUs) return SIPNET_KERNEL_COOP_NCYCLE;
  if (blocks <= 2 * (int64_t)numCUs) return SIPNET_KERNEL_COOP_NCYCLE_PAIR;
  return SIPNET_KERNEL_ONE_WAVE;
}

// Which cooperative kernel sums a batch's outputs over groups of steps inside its own launch (sipnet_batch_run_sums):
// throughput arithmetic (fp64 or fp32-mixed), any flag set, no record / diagnostics / full state -- AUTO's choice for the shape,
// or a throughput kernel forced.  0: none (the strict-order kernel).
static int sumsKernelFor(const sipnet_batch* b) {
  if (!b->fastMath || b->d_diag || (b->kernelOptions & SIPNET_KOPT_FULL_STATE)) return 0;
  int kernel = b->kernelPolicy;
  if (kernel == SIPNET_KERNEL_AUTO) kernel = autoKernel(b->flags, b->n_sites, b->n_members, true, false, 0, b->numCUs, false);
  if (kernel == SIPNET_KERNEL_ONE_WAVE) return kernel;
  const bool ncyc = b->flags[SIPNET_F_NITROGEN_CYCLE] != 0;
  if (ncyc) return (kernel == SIPNET_KERNEL_COOP_NCYCLE || kernel == SIPNET_KERNEL_COOP_NCYCLE_PAIR) ? kernel : 0;
  return (kernel == SIPNET_KERNEL_COOP_LDS || kernel == SIPNET_KERNEL_COOP_HBM || kernel == SIPNET_KERNEL_COOP_PAIR ||
          kernel == SIPNET_KERNEL_COOP_QUAD) ? kernel : 0;   // (a forced four-chunk layout the batch cannot take: the launch path says so)
}

// What the four run entry points ask of runImpl.  The planes are doubles, or -- fp32-mixed batches -- floats; with sumEvery
// they take the sums over groups of steps instead (sipnet_batch_run_sums).
struct RunCall {
  int32_t step0, n_steps;
  void *d_nee, *d_gpp, *d_et;
  double *d_rec, *d_dbg;
  int64_t ld;
  double* d_stats = nullptr;
  int32_t sumEvery = 0;
};

static int chunksPerSite(const sipnet_batch* b) { return (b->n_members + 63) / 64; }
// full state: the record, the diagnostics counters or SIPNET_KOPT_FULL_STATE -- the "Full" instantiations (autoKernel)
static bool wantsFullState(const sipnet_batch* b, const double* d_rec) {
  return d_rec || b->d_diag || (b->kernelOptions & SIPNET_KOPT_FULL_STATE);
}

static int checkRunCall(const sipnet_batch* b, const RunCall& c) {
  if (!b || c.step0 < 0 || c.n_steps < 0 || c.step0 + c.n_steps > b->n_steps) {
    setError("sipnet_batch_run: step range outside the climate record");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if ((c.d_nee || c.d_gpp || c.d_et || c.d_rec) && c.ld < b->ncol) {
    setError("sipnet_batch_run: ld smaller than the number of columns");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if (b->planDirty) {
    setError("sipnet_batch_run: call sipnet_batch_setup after changing climate/events");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  return SIPNET_OK;
}

// ---- kernel choice (sipnet_batch_set_kernel); nothing here reads the environment ----------
// AUTO's choice for the shape, or the kernel the caller forced -- unless the batch cannot take it.
static int resolveKernel(const sipnet_batch* b, const double* d_rec, const double* d_dbg, int* out) {
  const bool defaultFlags = isDefaultFlagSet(b->flags);
  int kernel = b->kernelPolicy;
  const bool wantFull = wantsFullState(b, d_rec);
  if (kernel == SIPNET_KERNEL_AUTO) {
    kernel = autoKernel(b->flags, b->n_sites, b->n_members, b->fastMath, d_dbg != nullptr, b->d_diag ? 2 : wantFull ? 1 : 0, b->numCUs,
                        b->precision == SIPNET_F32_MIXED);
  } else if (kernel != SIPNET_KERNEL_STRICT) {
    if (!b->fastMath) {
      setError("sipnet_batch_run: the throughput kernels need SIPNET_MATH_FAST (sipnet_batch_set_math)");
      return SIPNET_ERR_BAD_ARGUMENT;
    }
    if (d_dbg) {
      setError("sipnet_batch_run_debug: the debug plane is written by the strict-order kernel only");
      return SIPNET_ERR_BAD_ARGUMENT;
    }
    if (kernel == SIPNET_KERNEL_COOP_NCYCLE || kernel == SIPNET_KERNEL_COOP_NCYCLE_PAIR) {
      if (!b->flags[SIPNET_F_NITROGEN_CYCLE]) {
        setError("sipnet_batch_run: the nitrogen-cycle cooperative kernels run flag sets with the nitrogen cycle on (records, "
                 "SIPNET_KOPT_FULL_STATE and the diagnostics counters included)");
        return SIPNET_ERR_BAD_ARGUMENT;
      }
    } else if (kernel != SIPNET_KERNEL_ONE_WAVE && b->flags[SIPNET_F_NITROGEN_CYCLE]) {
      setError("sipnet_batch_run: a flag set with the nitrogen cycle takes SIPNET_KERNEL_COOP_NCYCLE(_PAIR) or the one-wave kernel");
      return SIPNET_ERR_BAD_ARGUMENT;
    } else if (kernel == SIPNET_KERNEL_COOP_QUAD && !defaultFlags && b->precision != SIPNET_F32_MIXED) {
      setError("sipnet_batch_run: the optional-physics instantiations of the cooperative kernel carry one or two chunks per "
               "workgroup (four in an fp32-mixed batch only: the fp64 build would spill)");
      return SIPNET_ERR_BAD_ARGUMENT;
    }
    if (kernel == SIPNET_KERNEL_COOP_QUAD && wantFull) {
      setError("sipnet_batch_run: the four-chunk cooperative kernel has no full-state instantiation "
               "(records, diagnostics, SIPNET_KOPT_FULL_STATE)");
      return SIPNET_ERR_BAD_ARGUMENT;
    }
  }
  // the throughput kernels index the ring [slot][col] with 32-bit element offsets (the strict-order kernel
  // uses 64-bit ones and takes any size)
  if (kernel != SIPNET_KERNEL_STRICT && b->ncol * SIPNET_RING_SLOTS >= (int64_t)1 << 31) {
    setError("sipnet_batch_run: the throughput kernels need n_sites * n_members * 250 < 2^31 (8.5 M columns per "
             "batch); split the ensemble into several batches or use SIPNET_MATH_STRICT");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  *out = kernel;
  return SIPNET_OK;
}

// what the chosen kernel reads, brought up to date on the caller's stream: its record type, the device-built records'
// log2vpd, the parameters in column order
static int prepareInputs(sipnet_batch* b, int kernel, hipStream_t stream) {
  int rc = kernel != SIPNET_KERNEL_STRICT ? ensureFastRecs(b, stream) : ensureStepRecs(b, stream);
  // (a member with dVpdExp != 2 has appeared since the device built its records: their log2vpd field, plan_device.h)
  if (!rc && kernel != SIPNET_KERNEL_STRICT && b->nDevSites && b->genericExponents && !b->devLog2Done) rc = fillDeviceLog2(b, stream);
  if (rc) return rc;
  // a resampled parameter index (particle filter): the one-wave kernel reads through it, every other kernel gets the
  // parameters back in column order first
  if (b->prmIndexed && kernel != SIPNET_KERNEL_ONE_WAVE) return materializeParams(b, stream);
  return SIPNET_OK;
}

// Does this kernel sum the ensemble statistics inside its own launch (sipnet_batch_run_stats)?  A wavefront of the
// cooperative kernel sums the planes' tiles per chunk while they are still in L2; any other kernel is
// followed by three streaming reductions over the finished planes
// (measured, DESIGN.md section 5: on the one-chunk-per-CU layout, whose fourth wavefront does the
// summing, the launch grows by 3-5 % against 10-15 % for the three passes; on the two- / four-chunk
// layouts the light wave would do it and its loads cost more than the passes -- SIPNET_KOPT_STATS_IN_KERNEL
// forces it there for tests and measurements)
static bool sumsStatsInLaunch(const sipnet_batch* b, int kernel) {
  return kernel == SIPNET_KERNEL_COOP_LDS || kernel == SIPNET_KERNEL_COOP_PAIR ||
         (kernel == SIPNET_KERNEL_COOP_QUAD && b->precision == SIPNET_F32_MIXED) ||
         ((b->kernelOptions & SIPNET_KOPT_STATS_IN_KERNEL) && kernel != SIPNET_KERNEL_STRICT &&
          kernel != SIPNET_KERNEL_ONE_WAVE && kernel != SIPNET_KERNEL_COOP_NCYCLE &&
          kernel != SIPNET_KERNEL_COOP_NCYCLE_PAIR);
}

// room for the per-chunk sums such a launch leaves (d_statsPart)
static int reserveStatsScratch(sipnet_batch* b, int32_t n_steps, hipStream_t stream) {
  const size_t need = (size_t)3 * b->n_sites * chunksPerSite(b) * n_steps * 2;
  if (need > b->d_statsPart.capacity()) {
    HIP_TRY(hipStreamSynchronize(stream));
    RC_TRY(b->d_statsPart.reserve(need));
  }
  // sites of different lengths: the rows past a site's last record are never written -- zero sums there
  bool ragged = false;
  for (int s = 0; s < b->n_sites; s++) ragged = ragged || b->siteSteps[s] != b->n_steps;
  if (ragged) HIP_TRY(hipMemsetAsync(b->d_statsPart, 0, need * sizeof(double), stream));
  return SIPNET_OK;
}

// a particle filter's forecast (sipnet_batch_pf_arm): the one-wave kernel's lean build leaves the log-weights too
static int armForecast(sipnet_batch* b, const RunCall& c, int kernel, bool wantFull, bool armed, FastArgs* f) {
  f->pfLogw = nullptr;
  f->pfBlockMax = nullptr;
  f->pfObs = f->pfInvSigma = 0.0;
  if (!armed) return SIPNET_OK;
  const int64_t blocks1 = (int64_t)b->n_sites * chunksPerSite(b);
  bool sameLength = true;
  for (int s = 0; s < b->n_sites; s++) sameLength = sameLength && b->siteSteps[s] >= c.step0 + c.n_steps;
  if (kernel == SIPNET_KERNEL_ONE_WAVE && !wantFull && c.d_nee && sameLength) {
    RC_TRY(b->d_pfPreMax.reserve((size_t)blocks1));
    f->pfLogw = b->pfArm.d_logw;
    f->pfBlockMax = b->d_pfPreMax;
    f->pfObs = b->pfArm.obs;
    f->pfInvSigma = 1.0 / b->pfArm.sigma;
    b->pfPre.valid = true;
    b->pfPre.plane = c.d_nee;
    b->pfPre.nSteps = c.n_steps;
    b->pfPre.nMax = (int32_t)blocks1;
    b->pfPre.ld = c.ld;
    b->pfPre.obs = b->pfArm.obs;
    b->pfPre.sigma = b->pfArm.sigma;
    b->pfPre.d_logw = b->pfArm.d_logw;
  }
  return SIPNET_OK;
}

// everything else a throughput kernel is handed (step_fast.hip / step_coop.hip)
static void fillFastArgs(const sipnet_batch* b, const RunCall& c, int kernel, bool wantFull, bool statsInLaunch, FastArgs* out) {
  FastArgs& f = *out;
  f.fast = b->d_fast;
  f.ringOps = b->d_ringOps;
  f.events = b->d_events;
  f.siteBase = b->d_siteBase;
  // (a particle filter's batch after a resampling: the one-wave kernel reads the parameters through the particles' index --
  // into the batch's own block, or into the bank of all ranks' parameters of a connected filter)
  const bool throughIndex = b->prmIndexed && kernel == SIPNET_KERNEL_ONE_WAVE;
  f.prm = (throughIndex && b->d_prmBank) ? b->d_prmBank : b->d_prm;
  f.prmPitch = (throughIndex && b->d_prmBank) ? b->prmBankPitch : b->ncol;
  f.prmId = throughIndex ? b->d_prmId : nullptr;
  f.sumEvery = c.sumEvery;
  f.padEnd = 0;
  f.state = b->d_state;
  f.ring = b->d_ring;
  f.nee = c.d_nee;
  f.gpp = c.d_gpp;
  f.et = c.d_et;
  f.ncol = b->ncol;
  f.ld = c.ld;
  f.n_sites = b->n_sites;
  f.n_members = b->n_members;
  f.n_steps_total = b->n_steps;
  f.step0 = c.step0;
  f.n_steps = c.n_steps;
  f.plainExp = b->genericExponents ? 0 : 1;
  f.rec = c.d_rec;
  f.diag = b->d_diag;
  f.full = wantFull ? 1 : 0;
  f.options = b->kernelOptions;
  f.scratchRow = b->d_scratchRow;
  memcpy(f.flags, b->flags, sizeof(f.flags));
  f.numCUs = b->numCUs;
  f.statsPart = (c.d_stats && statsInLaunch) ? b->d_statsPart : nullptr;
  f.statsChunks = b->n_sites * chunksPerSite(b);
}

// throughput path: which of the five launchers.  *boundedWaits: the diagnostic build went out (reportStuckWait)
static int launchThroughput(sipnet_batch* b, const RunCall& c, int kernel, bool statsInLaunch, bool armed, hipStream_t stream,
                            bool* boundedWaits) {
  const bool wantFull = wantsFullState(b, c.d_rec);
  FastArgs f;
  RC_TRY(armForecast(b, c, kernel, wantFull, armed, &f));
  fillFastArgs(b, c, kernel, wantFull, statsInLaunch, &f);
  const int32_t sumEvery = c.sumEvery;
  const int layout = kernel == SIPNET_KERNEL_COOP_LDS ? COOP_RING_LDS
                     : kernel == SIPNET_KERNEL_COOP_PAIR ? COOP_PAIR
                     : kernel == SIPNET_KERNEL_COOP_QUAD ? COOP_QUAD
                     : kernel == SIPNET_KERNEL_COOP_NCYCLE ? COOP_NCYCLE
                     : kernel == SIPNET_KERNEL_COOP_NCYCLE_PAIR ? COOP_NCYCLE_PAIR : COOP_RING_HBM;
  *boundedWaits = (b->kernelOptions & SIPNET_KOPT_BOUNDED_WAITS) && kernel != SIPNET_KERNEL_ONE_WAVE && !wantFull && !sumEvery;
  if (kernel == SIPNET_KERNEL_ONE_WAVE && sumEvery) sums2::launchStepFastSums(f, b->precision, b->kernelOptions, stream, &b->lastLaunch);
  else if (kernel == SIPNET_KERNEL_ONE_WAVE) launchStepFast(f, b->precision, b->kernelOptions, stream, &b->lastLaunch);
  else if (*boundedWaits) bounded::launchStepCoop(f, b->precision, layout, stream, &b->lastLaunch);
  else if (sumEvery && (b->precision != SIPNET_F64 || layout == COOP_QUAD)) sums2::launchStepCoopSums(f, b->precision, layout, stream, &b->lastLaunch);
  else launchStepCoop(f, b->precision, layout, stream, &b->lastLaunch);
  return SIPNET_OK;
}

// the strict-order kernel (step_kernel.hip)
static void launchStrict(sipnet_batch* b, const RunCall& c, hipStream_t stream) {
  KernelArgs a;
  a.plan = b->d_plan;
  a.ringOps = b->d_ringOps;
  a.events = b->d_events;
  a.siteBase = b->d_siteBase;
  a.prm = b->d_prm;
  a.state = b->d_state;
  a.ring = b->d_ring;
  a.nee = c.d_nee;
  a.gpp = c.d_gpp;
  a.et = c.d_et;
  a.rec = c.d_rec;
  a.dbg = c.d_dbg;
  a.diag = b->d_diag;
  a.ncol = b->ncol;
  a.ld = c.ld;
  a.n_sites = b->n_sites;
  a.n_members = b->n_members;
  a.n_steps_total = b->n_steps;
  a.step0 = c.step0;
  a.n_steps = c.n_steps;
  memcpy(a.flags, b->flags, sizeof(a.flags));
  launchStep(a, b->precision, b->fastMath, stream, &b->lastLaunch);
}

// the statistics block of sipnet_batch_run_stats from what the launch left
static void finishStats(sipnet_batch* b, const RunCall& c, bool statsInLaunch, hipStream_t stream) {
  if (statsInLaunch) {
    launchFinishStats(b->d_statsPart, c.n_steps, b->n_sites, chunksPerSite(b), c.d_stats, stream);
  } else {
    const bool f32 = b->precision == SIPNET_F32_MIXED;
    const size_t plane = (size_t)c.n_steps * b->n_sites * 2;
    launchReducePlane(c.d_nee, f32, c.n_steps, c.ld, b->n_sites, b->n_members, c.d_stats, stream);
    launchReducePlane(c.d_gpp, f32, c.n_steps, c.ld, b->n_sites, b->n_members, c.d_stats + plane, stream);
    launchReducePlane(c.d_et, f32, c.n_steps, c.ld, b->n_sites, b->n_members, c.d_stats + 2 * plane, stream);
  }
}

// the diagnostic build (SIPNET_KOPT_BOUNDED_WAITS): did a hand-over wait give up?
static int reportStuckWait(sipnet_batch* b, hipStream_t stream) {
  unsigned long long stuck[2] = {0, 0};
  if (bounded::readCoopStuck(stuck, stream) != 0) {
    setError("sipnet_batch_run: reading the bounded-wait report failed");
    return SIPNET_ERR_INTERNAL;
  }
  if (stuck[0] != 0) {
    setError("sipnet_batch_run: hand-over wait " + std::to_string((unsigned)((stuck[0] >> 32) & 0x7fffffffu)) + " (step_coop.hip, \"hand-over waits\") of workgroup " +
             std::to_string(stuck[1]) + " gave up at step " + std::to_string((int)(unsigned)(stuck[0] & 0xffffffffu)) + " of " + b->lastLaunch.kernel +
             ": a producer never posted (the launch's results are void)");
    return SIPNET_ERR_INTERNAL;
  }
  return SIPNET_OK;
}

static int runImpl(sipnet_batch* b, const RunCall& c, void* hip_stream) {
  int rc = checkRunCall(b, c);
  if (rc || c.n_steps == 0) return rc;
  RC_TRY(useDevice(b));
  hipStream_t stream = (hipStream_t)hip_stream;
  RC_TRY(flushParams(b, stream));   // (parameters set after the last setup: a particle filter's, a re-draw)
  int kernel = SIPNET_KERNEL_STRICT;
  RC_TRY(resolveKernel(b, c.d_rec, c.d_dbg, &kernel));
  RC_TRY(prepareInputs(b, kernel, stream));
  const bool statsInLaunch = sumsStatsInLaunch(b, kernel);
  if (c.d_stats && statsInLaunch) RC_TRY(reserveStatsScratch(b, c.n_steps, stream));
  // the timing events around the step kernel: for a long launch, or when asked for (sipnet_batch_time_next_launch) -- a
  // particle filter's 48-step forecasts run back to back with their analyses, and two event records per cycle cost the
  // device ~10 us of 165 (batch_impl.h markBusy)
  const bool timeIt = c.n_steps >= 512 || b->timeNext;
  b->timeNext = false;
  if (timeIt) HIP_TRY(hipEventRecord(b->ev0, stream));
  // log-weights a previous forecast left belong to the state BEFORE this launch, and an armed analysis belongs to THIS
  // launch, whichever kernel it takes
  const bool armed = b->pfArm.set;
  b->pfArm.set = false;
  b->pfPre.valid = false;
  bool boundedWaits = false;
  if (kernel != SIPNET_KERNEL_STRICT) RC_TRY(launchThroughput(b, c, kernel, statsInLaunch, armed, stream, &boundedWaits));
  else launchStrict(b, c, stream);
  HIP_TRY(hipGetLastError());
  if (timeIt) HIP_TRY(hipEventRecord(b->ev1, stream));
  if (c.d_stats) {
    finishStats(b, c, statsInLaunch, stream);
    HIP_TRY(hipGetLastError());
  }
  b->timed = timeIt;
  b->stepsDone = (b->stepsDone == c.step0) ? c.step0 + c.n_steps : -1;
  rc = markBusy(b, stream);
  if (!rc && c.n_steps >= 512) rc = recordBusy(b);   // (a long launch: the event now, batch_impl.h markBusy)
  if (rc) return rc;
  return boundedWaits ? reportStuckWait(b, stream) : SIPNET_OK;
}

extern "C" {

int sipnet_batch_run(sipnet_batch* b, int32_t step0, int32_t n_steps, void* d_nee,
                     void* d_gpp, void* d_et, double* d_rec, int64_t ld, void* hip_stream) {
  return runImpl(b, RunCall{step0, n_steps, d_nee, d_gpp, d_et, d_rec, nullptr, ld}, hip_stream);
}

int sipnet_batch_run_stats(sipnet_batch* b, int32_t step0, int32_t n_steps, void* d_nee, void* d_gpp,
                           void* d_et, int64_t ld, double* d_stats, void* hip_stream) {
  if (!d_nee || !d_gpp || !d_et || !d_stats) {
    setError("sipnet_batch_run_stats: needs the three planes and the statistics block");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  return runImpl(b, RunCall{step0, n_steps, d_nee, d_gpp, d_et, nullptr, nullptr, ld, d_stats}, hip_stream);
}

int sipnet_batch_run_debug(sipnet_batch* b, int32_t step0, int32_t n_steps, double* d_rec,
                           double* d_dbg, int64_t ld, void* hip_stream) {
  if (!d_rec || !d_dbg) {
    setError("sipnet_batch_run_debug: needs both the record and the debug plane");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  return runImpl(b, RunCall{step0, n_steps, nullptr, nullptr, nullptr, d_rec, d_dbg, ld}, hip_stream);
}

int32_t sipnet_batch_sums_in_kernel(const sipnet_batch* b) { return b ? (sumsKernelFor(b) != 0) : 0; }

int sipnet_batch_run_sums(sipnet_batch* b, int32_t step0, int32_t n_steps, int32_t sum_steps, double* d_nee_sums, double* d_gpp_sums,
                          double* d_et_sums, int64_t ld, void* hip_stream) {
  if (!b || sum_steps <= 0) {
    setError("sipnet_batch_run_sums: sum_steps must be positive");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if (!sumsKernelFor(b)) {
    setError("sipnet_batch_run_sums: no kernel sums this batch's outputs inside its launch (SIPNET_MATH_FAST, no diagnostics / "
             "full state: sipnet_batch_sums_in_kernel); run the planes and sum them");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  return runImpl(b, RunCall{step0, n_steps, d_nee_sums, d_gpp_sums, d_et_sums, nullptr, nullptr, ld, nullptr, sum_steps}, hip_stream);
}

int32_t sipnet_kernel_choice(const int32_t* flags, int32_t n_sites, int32_t n_members, int32_t precision,
                             int32_t math, int32_t want_full, int32_t num_cus) {
  if (!flags || n_sites <= 0 || n_members <= 0 || num_cus <= 0) return -1;
  const bool fast = precision == SIPNET_F32_MIXED || math == SIPNET_MATH_FAST;
  return autoKernel(flags, n_sites, n_members, fast, false, want_full, num_cus, precision == SIPNET_F32_MIXED);
}

double sipnet_batch_last_kernel_ms(sipnet_batch* b) {
  if (!b || !b->timed) return -1.0;
  if (hipSetDevice(b->device) != hipSuccess) return -1.0;
  if (hipEventSynchronize(b->ev1) != hipSuccess) return -1.0;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, b->ev0, b->ev1) != hipSuccess) return -1.0;
  b->lastMs = ms;
  return (double)ms;
}

int sipnet_batch_pf_arm(sipnet_batch* b, double obs, double sigma, double* d_logw) {
  if (!b || !d_logw || !(sigma > 0)) {
    setError("sipnet_batch_pf_arm: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  b->pfArm.set = true;
  b->pfArm.obs = obs;
  b->pfArm.sigma = sigma;
  b->pfArm.d_logw = d_logw;
  return SIPNET_OK;
}

int sipnet_batch_time_next_launch(sipnet_batch* b) {
  if (!b) return SIPNET_ERR_BAD_ARGUMENT;
  b->timeNext = true;
  return SIPNET_OK;
}

int sipnet_batch_last_launch(sipnet_batch* b, sipnet_launch_info* out) {
  if (!b || !out) return SIPNET_ERR_BAD_ARGUMENT;
  memset(out, 0, sizeof(*out));
  snprintf(out->kernel, sizeof out->kernel, "%s", b->lastLaunch.kernel);
  out->grid = b->lastLaunch.grid;
  out->block_threads = b->lastLaunch.block;
  out->waves_per_simd = b->lastLaunch.wavesPerSimd;
  out->lds_bytes = b->lastLaunch.ldsBytes;
  out->num_cus = b->numCUs;
  out->plan_threads = b->planThreads;
  out->plan_build_ms = b->planBuildMs;
  out->plan_upload_ms = b->planUploadMs;
  out->plan_device_sites = b->nDevSites;
  return SIPNET_OK;
}
const char* sipnet_batch_last_kernel_name(sipnet_batch* b) { return b ? b->lastLaunch.kernel : ""; }

int sipnet_batch_reduce_plane(sipnet_batch* b, const void* d_plane, int32_t elem_is_f32,
                              int32_t n_steps, int64_t ld, double* d_stats,
                              void* hip_stream) {
  if (!b || !d_plane || !d_stats || n_steps <= 0 || ld < b->ncol) {
    setError("sipnet_batch_reduce_plane: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  int rc = useDevice(b);
  if (rc) return rc;
  launchReducePlane(d_plane, elem_is_f32 != 0, n_steps, ld, b->n_sites, b->n_members,
                    d_stats, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError());
  return SIPNET_OK;
}

}  // extern "C"
