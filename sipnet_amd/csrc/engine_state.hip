// engine_state.hip -- what the host reads out of a batch (engine.hip) and writes into it: state, running-mean rings, status,
// the restart checkpoints, a site's plan series.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "../../include/sipnet_amd.h"
#include "batch_impl.h"

// The running-mean ring on the device, [SIPNET_RING_SLOTS][ncol]: doubles, or -- fp32-mixed batches -- floats:
// the values are NPP rates, which such a batch computes in fp32, so the narrower store loses nothing and
// halves what a resampling moves (a ring value IMPORTED from a checkpoint is rounded to fp32 there).
// Host <-> device copies of ncols columns from col0, host side [slot][ncols] doubles.
static int ringToHost(sipnet_batch* b, int64_t col0, int64_t ncols, double* out) {
  const size_t eb = ringElemBytes(b);
  if (eb == sizeof(double)) {
    HIP_TRY(hipMemcpy2D(out, (size_t)ncols * eb, b->d_ring + col0, (size_t)b->ncol * eb, (size_t)ncols * eb,
                        SIPNET_RING_SLOTS, hipMemcpyDeviceToHost));
    return SIPNET_OK;
  }
  std::vector<float> tmp((size_t)ncols * SIPNET_RING_SLOTS);
  HIP_TRY(hipMemcpy2D(tmp.data(), (size_t)ncols * eb, (const float*)b->d_ring.get() + col0, (size_t)b->ncol * eb,
                      (size_t)ncols * eb, SIPNET_RING_SLOTS, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < tmp.size(); i++) out[i] = (double)tmp[i];
  return SIPNET_OK;
}
static int ringFromHost(sipnet_batch* b, int64_t col0, int64_t ncols, const double* in) {
  const size_t eb = ringElemBytes(b);
  if (eb == sizeof(double)) {
    HIP_TRY(hipMemcpy2D(b->d_ring + col0, (size_t)b->ncol * eb, in, (size_t)ncols * eb, (size_t)ncols * eb,
                        SIPNET_RING_SLOTS, hipMemcpyHostToDevice));
    return SIPNET_OK;
  }
  std::vector<float> tmp((size_t)ncols * SIPNET_RING_SLOTS);
  for (size_t i = 0; i < tmp.size(); i++) tmp[i] = (float)in[i];
  HIP_TRY(hipMemcpy2D((float*)b->d_ring.get() + col0, (size_t)b->ncol * eb, tmp.data(), (size_t)ncols * eb,
                      (size_t)ncols * eb, SIPNET_RING_SLOTS, hipMemcpyHostToDevice));
  return SIPNET_OK;
}

// ---- restart checkpoints ------------------------------------------------------
namespace {
constexpr double kTinyBiomass = 0.000001;  // common/util.h:14
constexpr double kRingWindow = 5.0;        // MEAN_NPP_DAYS, sipnet.c:39

bool sufficientBiomass(const double* envi) {  // hasSufficientBiomass(), sipnet.c:1530-1537
  return envi[0] > kTinyBiomass && envi[0] + envi[12] > kTinyBiomass &&
         envi[7] + envi[6] > kTinyBiomass;
}
// the trackers a member carries in its state block: the row there, the checkpoint's tracker (imported and exported)
struct CarriedTracker { int st, rt; };
constexpr CarriedTracker kCarriedTrackers[] = {
    {ST_totGpp, SIPNET_RT_TOTGPP},       {ST_totRtot, SIPNET_RT_TOTRTOT},       {ST_totRa, SIPNET_RT_TOTRA},
    {ST_totRh, SIPNET_RT_TOTRH},         {ST_totNpp, SIPNET_RT_TOTNPP},         {ST_totNee, SIPNET_RT_TOTNEE},
    {ST_yearlyGpp, SIPNET_RT_YEARLYGPP}, {ST_yearlyRtot, SIPNET_RT_YEARLYRTOT}, {ST_yearlyRa, SIPNET_RT_YEARLYRA},
    {ST_yearlyRh, SIPNET_RT_YEARLYRH},   {ST_yearlyNpp, SIPNET_RT_YEARLYNPP},   {ST_yearlyNee, SIPNET_RT_YEARLYNEE},
    {ST_yearlyLitter, SIPNET_RT_YEARLYLITTER}};
int nextSlot(int i) { return (i + 1) % SIPNET_RING_SLOTS; }
int prevSlot(int i) { return (i + SIPNET_RING_SLOTS - 1) % SIPNET_RING_SLOTS; }

bool sameLayout(const sipnet_restart& r, const RingSched& s) {
  if (r.mean_start != s.start || r.mean_last != s.last) return false;
  for (int i = s.start;; i = nextSlot(i)) {
    if (r.mean_weights[i] != s.w[i]) return false;
    if (i == s.last) break;
  }
  return true;
}

// Re-express a member's ring on the site's layout: entries are matched newest first; the
// member's remaining (older) entries must all hold zero, which any layout represents.
bool relayRing(const sipnet_restart& r, const RingSched& s, double* values) {
  for (int i = 0; i < SIPNET_RING_SLOTS; i++) values[i] = 0.0;
  int im = r.mean_last, is = s.last;
  for (;;) {
    bool restZero = true;
    for (int k = r.mean_start;; k = nextSlot(k)) {
      if (r.mean_values[k] != 0.0) restZero = false;
      if (k == im) break;
    }
    if (restZero) return true;
    if (r.mean_weights[im] != s.w[is]) return false;
    values[is] = r.mean_values[im];
    if (im == r.mean_start) return true;
    if (is == s.start) return false;
    im = prevSlot(im);
    is = prevSlot(is);
  }
}
}  // namespace

extern "C" {

// state is exchanged with the host as [ncol][NSTATE]; HBM holds [NSTATE][ncol]
int sipnet_batch_get_state(sipnet_batch* b, double* state, void* hip_stream) {
  if (!b || !state) return SIPNET_ERR_BAD_ARGUMENT;
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  HIP_TRY(hipStreamSynchronize(stream));
  std::vector<double> tmp((size_t)b->ncol * SIPNET_NSTATE);
  HIP_TRY(hipMemcpy(tmp.data(), b->d_state, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int k = 0; k < SIPNET_NSTATE; k++)
    for (int64_t c = 0; c < b->ncol; c++)
      state[c * SIPNET_NSTATE + k] = tmp[(size_t)k * b->ncol + c];
  return SIPNET_OK;
}

int sipnet_batch_set_state(sipnet_batch* b, const double* state, void* hip_stream) {
  if (!b || !state) return SIPNET_ERR_BAD_ARGUMENT;
  b->pfPre.valid = false;
  b->pfArm.set = false;
  int rc = useDevice(b);
  if (rc) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  HIP_TRY(hipStreamSynchronize(stream));
  std::vector<double> tmp((size_t)b->ncol * SIPNET_NSTATE);
  for (int k = 0; k < SIPNET_NSTATE; k++)
    for (int64_t c = 0; c < b->ncol; c++)
      tmp[(size_t)k * b->ncol + c] = state[c * SIPNET_NSTATE + k];
  HIP_TRY(hipMemcpy(b->d_state, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
  b->stepsDone = -1;  // the caller moved the state; only it knows to which record
  return SIPNET_OK;
}

int sipnet_batch_get_ring(sipnet_batch* b, int64_t col, double* values, void* hip_stream) {
  if (!b || !values || col < 0 || col >= b->ncol) return SIPNET_ERR_BAD_ARGUMENT;
  int rc = useDevice(b);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  return ringToHost(b, col, 1, values);
}

int sipnet_batch_get_rings(sipnet_batch* b, double* rings, void* hip_stream) {
  if (!b || !rings) return SIPNET_ERR_BAD_ARGUMENT;
  int rc = useDevice(b);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  std::vector<double> tmp((size_t)b->ncol * SIPNET_RING_SLOTS);
  rc = ringToHost(b, 0, b->ncol, tmp.data());
  if (rc) return rc;
  for (int k = 0; k < SIPNET_RING_SLOTS; k++)
    for (int64_t c = 0; c < b->ncol; c++)
      rings[c * SIPNET_RING_SLOTS + k] = tmp[(size_t)k * b->ncol + c];
  return SIPNET_OK;
}

int sipnet_batch_set_rings(sipnet_batch* b, const double* rings, void* hip_stream) {
  if (!b || !rings) return SIPNET_ERR_BAD_ARGUMENT;
  int rc = useDevice(b);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  std::vector<double> tmp((size_t)b->ncol * SIPNET_RING_SLOTS);
  for (int k = 0; k < SIPNET_RING_SLOTS; k++)
    for (int64_t c = 0; c < b->ncol; c++)
      tmp[(size_t)k * b->ncol + c] = rings[c * SIPNET_RING_SLOTS + k];
  return ringFromHost(b, 0, b->ncol, tmp.data());
}

int sipnet_batch_get_status(sipnet_batch* b, int32_t* status, void* hip_stream) {
  if (!b || !status) return SIPNET_ERR_BAD_ARGUMENT;
  int rc = useDevice(b);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  std::vector<double> tmp((size_t)b->ncol);
  HIP_TRY(hipMemcpy(tmp.data(), b->d_state + (size_t)ST_status * b->ncol,
                    tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t c = 0; c < b->ncol; c++) status[c] = (int32_t)tmp[c];
  return SIPNET_OK;
}

int sipnet_batch_set_resume(sipnet_batch* b, int32_t site, const sipnet_restart* r) {
  if (!b || site < 0 || site >= b->n_sites) {
    setError("sipnet_batch_set_resume: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  PlanCarry& c = b->resume[site];
  c = PlanCarry{};
  b->resumeProcessed[site] = 0;
  b->planDirty = true;
  if (!r) return SIPNET_OK;
  if (r->mean_length != SIPNET_RING_SLOTS || r->mean_start < 0 ||
      r->mean_start >= SIPNET_RING_SLOTS || r->mean_last < 0 ||
      r->mean_last >= SIPNET_RING_SLOTS) {  // restart.c:727-733, :987-992
    setError("Restart mean-tracker length or cursor out of range");
    return SIPNET_ERR_RESTART;
  }
  c.set = true;
  b->resumeProcessed[site] = r->processed_steps;  // the count runs on, restart.c:912-920
  c.gdd = r->trackers[SIPNET_RT_GDD];
  c.trackLastYear = r->trackers_last_year;
  c.phenLastYear = r->phenology_last_year;
  c.dTill = r->d_till_mod;
  c.ring.start = r->mean_start;
  c.ring.last = r->mean_last;
  for (int i = 0; i < SIPNET_RING_SLOTS; i++) {
    c.ring.w[i] = r->mean_weights[i];
    c.ring.insStep[i] = 0;
  }
  return SIPNET_OK;
}

int sipnet_batch_import_restart(sipnet_batch* b, int32_t site, int32_t first_member,
                                int32_t count, const sipnet_restart* r, void* hip_stream) {
  if (!b || site < 0 || site >= b->n_sites || first_member < 0 || count <= 0 ||
      first_member + count > b->n_members || !r) {
    setError("sipnet_batch_import_restart: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if (b->planDirty || !b->resume[site].set) {
    setError("sipnet_batch_import_restart: call sipnet_batch_set_resume and "
             "sipnet_batch_setup first");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  b->pfPre.valid = false;
  b->pfArm.set = false;
  int rc = useDevice(b);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  const PlanCarry& c = b->resume[site];
  const int64_t col0 = (int64_t)site * b->n_members + first_member;
  const size_t pitchD = (size_t)b->ncol * sizeof(double), pitchH = (size_t)count * sizeof(double);
  // current state block [NSTATE][count]: keeps what setup decided (status, diagnostics)
  std::vector<double> st((size_t)SIPNET_NSTATE * count), ring((size_t)SIPNET_RING_SLOTS * count);
  HIP_TRY(hipMemcpy2D(st.data(), pitchH, b->d_state + col0, pitchD, pitchH, SIPNET_NSTATE,
                      hipMemcpyDeviceToHost));
  double vals[SIPNET_RING_SLOTS];
  for (int32_t m = 0; m < count; m++) {
    const sipnet_restart& k = r[m];
    const std::string who = "member " + std::to_string(first_member + m) + " of site " +
                            std::to_string(site);
    for (int i = 0; i < SIPNET_NFLAGS; i++) {
      if (k.flags[i] != b->flags[i]) {
        setError("Restart context mismatch: model flags must match checkpoint exactly (" + who + ")");
        return SIPNET_ERR_RESTART;
      }
    }
    if (k.trackers[SIPNET_RT_GDD] != c.gdd || k.trackers_last_year != c.trackLastYear ||
        k.phenology_last_year != c.phenLastYear || k.d_till_mod != c.dTill) {
      setError("sipnet_batch_import_restart: " + who + " disagrees with the site's resume "
               "state (gdd, lastYear or d_till_mod); members of a site share one forcing history");
      return SIPNET_ERR_RESTART;
    }
    if ((k.is_alive != 0) != sufficientBiomass(k.envi)) {
      setError("sipnet_batch_import_restart: survival.isAlive of " + who +
               " contradicts its pools (sipnet.c:1530-1544)");
      return SIPNET_ERR_RESTART;
    }
    if (k.mean_length != SIPNET_RING_SLOTS || k.mean_start < 0 ||
        k.mean_start >= SIPNET_RING_SLOTS || k.mean_last < 0 ||
        k.mean_last >= SIPNET_RING_SLOTS) {
      setError("Restart mean-tracker length or cursor out of range (" + who + ")");
      return SIPNET_ERR_RESTART;
    }
    if (sameLayout(k, c.ring)) {
      memcpy(vals, k.mean_values, sizeof vals);
    } else if (!relayRing(k, c.ring, vals)) {
      setError("sipnet_batch_import_restart: running-mean ring layout of " + who +
               " cannot be expressed on the site's layout");
      return SIPNET_ERR_RESTART;
    }
    for (int i = 0; i < SIPNET_RING_SLOTS; i++) ring[(size_t)i * count + m] = vals[i];
    double* s = st.data() + m;
    auto S = [&](int row) -> double& { return s[(size_t)row * count]; };
    for (int i = 0; i < 13; i++) S(i) = k.envi[i];
    S(ST_ringSum) = k.mean_sum;
    for (const CarriedTracker& t : kCarriedTrackers) S(t.st) = k.trackers[t.rt];
    S(ST_phenBits) = (double)((k.did_leaf_growth ? 1 : 0) | (k.did_leaf_fall ? 2 : 0));
    S(ST_ringValidFrom) = 0.0;
  }
  HIP_TRY(hipMemcpy2D(b->d_state + col0, pitchD, st.data(), pitchH, pitchH, SIPNET_NSTATE,
                      hipMemcpyHostToDevice));
  return ringFromHost(b, col0, count, ring.data());
}

int sipnet_batch_export_restart(sipnet_batch* b, int32_t site, int32_t member,
                                int32_t n_steps_done, const double* last_rec,
                                const double* prev_pools, sipnet_restart* out,
                                void* hip_stream) {
  if (!b || site < 0 || site >= b->n_sites || member < 0 || member >= b->n_members || !out) {
    setError("sipnet_batch_export_restart: bad argument");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if (b->planDirty) {
    setError("sipnet_batch_export_restart: no run to take a checkpoint of");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  if (n_steps_done <= 0 || n_steps_done > b->siteSteps[site]) {  // restart.c:933-937
    setError("Cannot write restart checkpoint: no timestep processed");
    return SIPNET_ERR_RESTART;
  }
  // (a site shorter than the batch's longest stops at its own last record)
  if (b->stepsDone >= 0 && std::min(b->stepsDone, b->siteSteps[site]) != n_steps_done) {
    setError("sipnet_batch_export_restart: the carried state is at record " +
             std::to_string(b->stepsDone) + ", not " + std::to_string(n_steps_done));
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  int rc = useDevice(b);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  const int64_t col = (int64_t)site * b->n_members + member;
  const size_t pitchD = (size_t)b->ncol * sizeof(double);
  double st[SIPNET_NSTATE], ring[SIPNET_RING_SLOTS];
  HIP_TRY(hipMemcpy2D(st, sizeof(double), b->d_state + col, pitchD, sizeof(double),
                      SIPNET_NSTATE, hipMemcpyDeviceToHost));
  rc = ringToHost(b, col, 1, ring);
  if (rc) return rc;
  if ((int)st[ST_status] != SIPNET_OK) {
    setError("sipnet_batch_export_restart: member did not run (status " +
             std::to_string((int)st[ST_status]) + ")");
    return (int)st[ST_status];
  }

  // what the plan owns, after n_steps_done records
  const int n = n_steps_done;
  // (cached: a CLI exporting every member of a site asks for the same boundary again and again)
  if (b->exportCacheSite != site || b->exportCacheN != n) {
    b->exportHead = buildSitePlan(
        b->flags, n, b->sc[site].clim(), b->sc[site].year(), b->sc[site].day(),
        (int32_t)b->events[site].size(), b->events[site].data(),
        b->resume[site].set ? &b->resume[site] : nullptr, &b->exportFin);
    b->exportCacheSite = site;
    b->exportCacheN = n;
  }
  const PlanCarry& fin = b->exportFin;
  const SitePlan& head = b->exportHead;
  const double* lastClim = b->sc[site].clim() + (size_t)SIPNET_NCLIM * (n - 1);

  memset(out, 0, sizeof(*out));
  snprintf(out->model_version, sizeof out->model_version, "2.1.0");
  {
    std::string info = sipnet_version();
    for (char& ch : info)
      if (ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n') ch = '_';
    snprintf(out->build_info, sizeof out->build_info, "%s", info.c_str());
  }
  out->checkpoint_utc_epoch = (int64_t)time(nullptr);
  out->processed_steps = b->resumeProcessed[site] + n;
  memcpy(out->flags, b->flags, sizeof out->flags);
  out->boundary_year = b->sc[site].year()[n - 1];
  out->boundary_day = b->sc[site].day()[n - 1];
  out->boundary_time = lastClim[10];
  out->boundary_length = lastClim[0];
  for (int i = 0; i < 13; i++) out->envi[i] = st[i];
  double* T = out->trackers;
  if (last_rec) {  // the per-step trackers of the last record, sipnet.c:1433-1497
    T[SIPNET_RT_GPP] = last_rec[1];
    T[SIPNET_RT_RTOT] = last_rec[10];
    T[SIPNET_RT_RA] = last_rec[8];
    T[SIPNET_RT_RH] = last_rec[9];
    T[SIPNET_RT_RROOT] = last_rec[7];
    T[SIPNET_RT_RSOIL] = last_rec[6];
    T[SIPNET_RT_RABOVEGROUND] = last_rec[5];
    T[SIPNET_RT_NPP] = last_rec[4];
    T[SIPNET_RT_NEE] = last_rec[0];
    T[SIPNET_RT_WOODCREATION] = last_rec[11];
    T[SIPNET_RT_ET] = last_rec[2];
    T[SIPNET_RT_SOILWETNESSFRAC] = last_rec[12];
    T[SIPNET_RT_METHANE] = last_rec[31];
    T[SIPNET_RT_N2O] = last_rec[27];
    T[SIPNET_RT_NLEACHING] = last_rec[28];
    T[SIPNET_RT_NFIXATION] = last_rec[29];
    T[SIPNET_RT_NUPTAKE] = last_rec[30];
    T[SIPNET_RT_MEANNPP] = last_rec[32];
  } else {
    T[SIPNET_RT_MEANNPP] = st[ST_ringSum] / kRingWindow;
  }
  T[SIPNET_RT_GDD] = fin.gdd;
  for (const CarriedTracker& t : kCarriedTrackers) T[t.rt] = st[t.st];
  out->trackers_last_year = fin.trackLastYear;
  const int phenBits = (int)st[ST_phenBits];
  out->did_leaf_growth = phenBits & 1;
  out->did_leaf_fall = (phenBits >> 1) & 1;
  out->phenology_last_year = fin.phenLastYear;
  out->is_alive = sufficientBiomass(out->envi) ? 1 : 0;
  out->d_till_mod = fin.dTill;
  // harvest fractions of the last record's events (events.c:467-469, :553-562)
  if (prev_pools && b->flags[SIPNET_F_EVENTS]) {
    const StepRec& ls = head.steps[n - 1];
    const double woodC = prev_pools[0] + prev_pools[12];
    const double above = woodC + prev_pools[1], below = prev_pools[7] + prev_pools[6];
    for (int e = 0; e < ls.evCount; e++) {
      const EvRec& ev = head.events[ls.evFirst + e];
      if (ev.type == SIPNET_EV_HARVEST && above + below > kTinyBiomass) {
        out->harvest_frac_removed += (ev.p[0] * above + ev.p[1] * below) / (above + below);
        out->harvest_frac_transferred += (ev.p[2] * above + ev.p[3] * below) / (above + below);
      }
    }
  }

  // running-mean ring in the reference's own layout
  out->mean_length = SIPNET_RING_SLOTS;
  out->mean_tot_weight = kRingWindow;
  out->mean_sum = st[ST_ringSum];
  const int validFrom = (int)st[ST_ringValidFrom];
  if (validFrom <= 0) {
    // a member that never died holds exactly the plan's ring
    out->mean_start = fin.ring.start;
    out->mean_last = fin.ring.last;
    for (int i = 0; i < SIPNET_RING_SLOTS; i++) {
      out->mean_weights[i] = fin.ring.w[i];
      out->mean_values[i] = ring[i];
    }
  } else {
    // the reference reset this member's ring when it died (sipnet.c:1757) and inserted
    // again from record validFrom on: replay that schedule, take the values by insert step
    RingSched fresh;
    bool overflow = false;
    for (int t = validFrom; t < n; t++)
      fresh.advance(t, b->sc[site].clim()[(size_t)SIPNET_NCLIM * t], nullptr, &overflow);
    out->mean_start = fresh.start;
    out->mean_last = fresh.last;
    for (int i = 0; i < SIPNET_RING_SLOTS; i++) out->mean_weights[i] = fresh.w[i];
    for (int i = fresh.start;; i = nextSlot(i)) {
      const int ins = fresh.insStep[i];
      if (ins >= validFrom) {
        for (int j = 0; j < SIPNET_RING_SLOTS; j++) {
          if (fin.ring.insStep[j] == ins) {
            out->mean_values[i] = ring[j];
            break;
          }
        }
      }
      if (i == fresh.last) break;
    }
  }
  return SIPNET_OK;
}

int sipnet_batch_get_site_series(sipnet_batch* b, int32_t site, double* gdd,
                                 double* d_till_mod) {
  if (!b || site < 0 || site >= b->n_sites || b->planDirty ||
      (int)b->plans.size() != b->n_sites)
    return SIPNET_ERR_BAD_ARGUMENT;
  if (b->devSite[site] && b->plans[site].gddAfter.empty()) {   // a device-built site: the series from a host pass of its own
    const SiteClim& c = b->sc[site];
    SitePlan hp = buildSitePlan(b->flags, c.n, c.clim(), c.year(), c.day(), (int32_t)b->events[site].size(), b->events[site].data(),
                                b->resume[site].set ? &b->resume[site] : nullptr, nullptr, /*wantSteps=*/false);
    b->plans[site].gddAfter = std::move(hp.gddAfter);
    b->plans[site].dTill = std::move(hp.dTill);
  }
  const SitePlan& p = b->plans[site];
  for (int t = 0; t < b->siteSteps[site]; t++) {   // (the site's own length: sipnet_batch_nsteps is the longest site's)
    if (gdd) gdd[t] = p.gddAfter[t];
    if (d_till_mod) d_till_mod[t] = p.dTill[t];
  }
  return SIPNET_OK;
}

/* Test hook: the records and ring evictions the DEVICE built for `site` (plan_device.h) against buildSitePlan()'s on the
 * host, byte by byte.  ignore_log2 != 0: FastRec::log2vpd is left out (it is only filled when a member reads it). */
int sipnet_debug_plan_compare(sipnet_batch* b, int32_t site, int32_t ignore_log2, int64_t* n_records_differing,
                              int64_t* n_ops_differing, int32_t* first_step, int32_t* first_offset, int32_t* device_info) {
  if (!b || site < 0 || site >= b->n_sites || b->planDirty || !b->devSite[site]) {
    setError("sipnet_debug_plan_compare: not a device-built site");
    return SIPNET_ERR_BAD_ARGUMENT;
  }
  int rc = useDevice(b);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  const SiteClim& c = b->sc[site];
  const int n = c.n;
  std::vector<FastRec> host(n), dev(n);
  SitePlan hp = buildSitePlan(b->flags, n, c.clim(), c.year(), c.day(), (int32_t)b->events[site].size(), b->events[site].data(),
                              b->resume[site].set ? &b->resume[site] : nullptr, nullptr, /*wantSteps=*/false, nullptr, host.data(),
                              b->precision == SIPNET_F32_MIXED);
  HIP_TRY(hipMemcpy(dev.data(), b->d_fast + (size_t)site * b->n_steps, (size_t)n * sizeof(FastRec), hipMemcpyDeviceToHost));
  int d = 0;
  for (int s = 0; s < site; s++) d += b->devSite[s];
  int32_t out4[8];
  HIP_TRY(hipMemcpy(out4, b->devPlan.siteOut + 8 * d, sizeof out4, hipMemcpyDeviceToHost));
  if (device_info) memcpy(device_info, out4, sizeof out4);
  int64_t nr = 0, no = 0;
  int32_t fs = -1, fo = -1;
  for (int t = 0; t < n; t++) {
    if (ignore_log2) dev[t].log2vpd = host[t].log2vpd;
    if (memcmp(&host[t], &dev[t], sizeof(FastRec)) != 0) {
      if (fs < 0) {
        fs = t;
        const unsigned char *x = (const unsigned char*)&host[t], *y = (const unsigned char*)&dev[t];
        for (size_t k = 0; k < sizeof(FastRec); k++)
          if (x[k] != y[k]) { fo = (int32_t)k; break; }
      }
      nr++;
    }
  }
  std::vector<RingOp> ops(hp.ringOps.size() + 1);
  std::vector<int32_t> base(3);
  HIP_TRY(hipMemcpy(base.data(), b->d_siteBase + 3 * site, 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (!hp.ringOps.empty())
    HIP_TRY(hipMemcpy(ops.data(), b->d_ringOps + base[0], hp.ringOps.size() * sizeof(RingOp), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < hp.ringOps.size(); k++)
    if (memcmp(&ops[k], &hp.ringOps[k], sizeof(RingOp)) != 0) no++;
  if ((size_t)out4[1] != hp.ringOps.size()) no += 1 + llabs((long long)out4[1] - (long long)hp.ringOps.size());
  // (the event records the light pass matched to the climate records)
  const std::vector<EvRec>& evs = b->plans[site].events;
  if (evs.size() != hp.events.size() || (!evs.empty() && memcmp(evs.data(), hp.events.data(), evs.size() * sizeof(EvRec)) != 0)) no += 1000000;
  if (n_records_differing) *n_records_differing = nr;
  if (n_ops_differing) *n_ops_differing = no;
  if (first_step) *first_step = fs;
  if (first_offset) *first_offset = fo;
  return SIPNET_OK;
}

}  // extern "C"
