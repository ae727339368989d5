// cli_inputs.h -- part of sipnet_cli.cpp: what lies between the command line and the run -- one directory's configuration
// and input files resolved into a Run, the restart checkpoints it resumes from, and the --ensemble-params table.
#pragma once

struct Run {
  std::string dir;           // absolute (--sites); empty for the run of the process's own directory
  Context ctx;               // the command line's options over the directory's sipnet.in
  int32_t flags[SIPNET_NFLAGS];
  std::vector<double> params;
  sipnet_clim_table* clim = nullptr;
  sipnet_event* events = nullptr;
  int32_t nEvents = 0;
  int T = 0;
  bool hasResume = false;    // RESTART_IN: the checkpoint this run resumes from (restartLoadCheckpoint, restart.c:968-996)
  sipnet_restart resume;
  std::string restartOut;    // RESTART_OUT as an absolute path ("" = none)
};
void freeRun(Run& r) {
  sipnet_clim_free(r.clim);
  sipnet_io_free(r.events);
}

// what the site plan takes from a checkpoint (sipnet_batch_set_resume): members of one site must agree in it
bool samePlanCarry(const sipnet_restart& a, const sipnet_restart& b) {
  return a.trackers[SIPNET_RT_GDD] == b.trackers[SIPNET_RT_GDD] && a.trackers_last_year == b.trackers_last_year &&
         a.phenology_last_year == b.phenology_last_year && a.d_till_mod == b.d_till_mod && a.mean_start == b.mean_start &&
         a.mean_last == b.mean_last && a.processed_steps == b.processed_steps &&
         memcmp(a.mean_weights, b.mean_weights, sizeof a.mean_weights) == 0;
}

bool sameForcing(const Run& a, const Run& b) {
  if (a.T != b.T || a.nEvents != b.nEvents || a.hasResume != b.hasResume) return false;
  if (a.hasResume && !samePlanCarry(a.resume, b.resume)) return false;
  if (memcmp(sipnet_clim_data(a.clim), sipnet_clim_data(b.clim), (size_t)a.T * SIPNET_NCLIM * sizeof(double)) != 0) return false;
  if (memcmp(sipnet_clim_year(a.clim), sipnet_clim_year(b.clim), (size_t)a.T * sizeof(int32_t)) != 0) return false;
  if (memcmp(sipnet_clim_day(a.clim), sipnet_clim_day(b.clim), (size_t)a.T * sizeof(int32_t)) != 0) return false;
  for (int k = 0; k < a.nEvents; k++) {
    const sipnet_event &x = a.events[k], &y = b.events[k];
    if (x.type != y.type || x.year != y.year || x.day != y.day || memcmp(x.p, y.p, sizeof x.p) != 0) return false;
  }
  return true;
}

// restartLoadCheckpoint (restart.c:968-996): the checkpoint at `path` and its checks, with the reference's log lines
void readResume(const std::string& path, const int32_t* flags, const sipnet_clim_table* clim, sipnet_restart& r) {
  check(sipnet_io_read_restart(path.c_str(), &r), "reading restart checkpoint");
  const int T = sipnet_clim_nsteps(clim);
  const double* c0 = sipnet_clim_data(clim);
  int32_t warn = 0;
  check(sipnet_restart_check(&r, flags, T > 0, T > 0 ? sipnet_clim_year(clim)[0] : 0, T > 0 ? sipnet_clim_day(clim)[0] : 0,
                             T > 0 ? c0[10] : 0.0, T > 0 ? c0[0] : 0.0, &warn), "restart checkpoint");
  if (warn & SIPNET_RESTART_WARN_BOUNDARY_NOT_MIDNIGHT)
    logWarning("Restart checkpoint boundary in " + path + " is more than one timestep before "
               "midnight; there is a time gap on resume.\n");
  if (warn & SIPNET_RESTART_WARN_BUILD_INFO)
    logInfo(std::string("Restart build info mismatch: checkpoint=") + r.build_info + "\n");
  if (warn & SIPNET_RESTART_WARN_TIME_GAP)
    logWarning("Restart resumed segment starts more than one timestep after midnight "
               "checkpoint boundary; there is a time gap\n");
}

// frontend.c:164-209: the derived file names, and --dump-config before any input is read
void deriveNames(Context& ctx) {
  const std::string prefix = ctx.s("filePrefix");
  ctx.setStr("paramFile", prefix + ".param", SRC_CALCULATED);
  ctx.setStr("climFile", prefix + ".clim", SRC_CALCULATED);
  if (ctx.i("doMainOutput")) ctx.setStr("outFile", prefix + ".out", SRC_CALCULATED);
  if (!ctx.i("dumpConfig")) return;
  ctx.setStr("outConfigFile", prefix + ".config", SRC_CALCULATED);
  FILE* f = fopen((prefix + ".config").c_str(), "w");
  if (!f) die(6, "Error opening " + prefix + ".config for writing\n");
  printConfig(ctx, f);
  fclose(f);
}

// One directory's run, from r.ctx (the command line's options) to its inputs in memory; the process is inside the
// directory.  The run of the process's own directory takes QUIET from its sipnet.in; under --sites (r.dir set) the
// command line alone decides it, and --debug-log is refused.  The restart checkpoints follow in resolveRestart: an
// ensemble reads its table first and has one checkpoint per member.
void resolveRun(Run& r) {
  Context& ctx = r.ctx;
  const bool underSites = !r.dir.empty();
  if (ctx.s("filePrefix").empty()) die(3, "filePrefix must be set for SIPNET to run\n");
  readInputFile(ctx);
  if (!underSites) g_quiet = ctx.i("quiet") != 0;
  checkFlagCoupling(ctx);
  if (underSites && !ctx.s("debugLogPrefix").empty()) die(8, "--sites does not combine with --debug-log (" + r.dir + ")\n");
  deriveNames(ctx);
  const int32_t fl[SIPNET_NFLAGS] = {ctx.i("events"), ctx.i("gdd"), ctx.i("growthResp"), ctx.i("leafWater"), ctx.i("litterPool"),
                                     ctx.i("snow"), ctx.i("soilPhenol"), ctx.i("waterHResp"), ctx.i("nitrogenCycle"),
                                     ctx.i("anaerobic"), ctx.i("flooding"), ctx.i("carbonSaturation")};
  memcpy(r.flags, fl, sizeof fl);
  // initModel (sipnet.c:2001-2009)
  r.params.resize(SIPNET_NPARAMS);
  check(sipnet_io_read_params(ctx.s("paramFile").c_str(), r.flags, r.params.data(), nullptr), "reading parameters");
  check(sipnet_io_read_clim(ctx.s("climFile").c_str(), r.flags[SIPNET_F_GDD], &r.clim), "reading climate");
  r.T = sipnet_clim_nsteps(r.clim);
  if (ctx.i("events")) {
    check(sipnet_io_read_events((ctx.s("eventsPrefix") + ".in").c_str(), r.flags, r.params.data(), &r.events, &r.nEvents),
          "reading events");
    if (r.nEvents == 0) logInfo("No event file found, assuming no input events\n");
  }
}
// RESTART_IN / RESTART_OUT of a run that is one member
void resolveRestart(Run& r) {
  if (!r.ctx.s("restartIn").empty()) {
    readResume(r.ctx.s("restartIn"), r.flags, r.clim, r.resume);
    r.hasResume = true;
  }
  if (!r.ctx.s("restartOut").empty()) r.restartOut = joinPath(r.dir, r.ctx.s("restartOut"));
}

// --ensemble-params: a whitespace table, first line = parameter names, one row per member overriding those parameters of
// `base`; returns the members' rows, [M][SIPNET_NPARAMS]
std::vector<double> readMemberTable(const std::string& path, const std::vector<double>& base) {
  std::ifstream in(path);
  if (!in) die(6, "Error opening " + path + " for reading\n");
  std::string line;
  std::getline(in, line);
  std::istringstream hs(line);
  std::vector<int> cols;
  for (std::string name; hs >> name;) {
    const int idx = sipnet_param_index(name.c_str());
    if (idx < 0) die(5, "unknown parameter " + name + " in " + path + "\n");
    cols.push_back(idx);
  }
  std::vector<double> members;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::vector<double> row(base);
    size_t k = 0;
    for (double v; ls >> v && k < cols.size(); k++) row[cols[k]] = v;
    if (k == 0) continue;
    if (k != cols.size()) die(5, "short row in " + path + "\n");
    members.insert(members.end(), row.begin(), row.end());
  }
  if (members.empty()) die(5, "no members in " + path + "\n");
  logInfo("ensemble of " + std::to_string(members.size() / SIPNET_NPARAMS) + " members in one batch\n");
  return members;
}

// One site of a batch: its forcing (events, climate, and the plan's carry of a resumed run) is `forcing`'s; its M
// members' parameter rows and, when the site resumes, their checkpoints.
struct SiteInput {
  const Run* forcing;
  const double* params;           // [M][SIPNET_NPARAMS]
  const sipnet_restart* resume;   // [M], or nullptr
};
// a batch of sites.size() sites x M members on `device`, set up and ready to run
void setupBatch(Batch& batch, const int32_t* flags, int M, int device, bool fastMath, const std::vector<SiteInput>& sites) {
  check(sipnet_batch_create(flags, (int)sites.size(), M, SIPNET_F64, device, &batch.b), "creating batch");
  sipnet_batch* b = batch.b;
  check(sipnet_batch_set_math(b, fastMath ? SIPNET_MATH_FAST : SIPNET_MATH_STRICT), "math policy");
  if (g_kernelOptions) check(sipnet_batch_set_kernel(b, SIPNET_KERNEL_AUTO, g_kernelOptions), "kernel options");
  for (int s = 0; s < (int)sites.size(); s++) {
    const Run& r = *sites[s].forcing;
    check(sipnet_batch_set_events(b, s, r.nEvents, r.events), "events");
    check(sipnet_batch_set_climate(b, s, r.T, sipnet_clim_data(r.clim), sipnet_clim_year(r.clim), sipnet_clim_day(r.clim)), "climate");
    check(sipnet_batch_set_params(b, s, 0, M, sites[s].params), "parameters");
    if (sites[s].resume) check(sipnet_batch_set_resume(b, s, &sites[s].resume[0]), "restart checkpoint");
  }
  check(sipnet_batch_setup(b, nullptr), "setupModel");
  for (int s = 0; s < (int)sites.size(); s++)   // every member from its own checkpoint
    if (sites[s].resume) check(sipnet_batch_import_restart(b, s, 0, M, sites[s].resume, nullptr), "restart checkpoint");
}
