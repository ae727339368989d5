// cli_ensemble.h -- part of sipnet_cli.cpp: the run of the process's own directory -- one run, or one member per row of
// --ensemble-params -- as per-step statistics through the node object (--ensemble-stats) or as the members' files and / or
// the ensemble block, sharded by member over --devices.
#pragma once

struct Ensemble {
  Run run;                               // every member's forcing, flags and output options
  std::string table;                     // --ensemble-params ("" = the single run)
  std::string mathArg;                   // --math
  std::vector<int> devices;              // one shard of members each
  BlockSpec block;
  std::vector<double> members;           // [M][SIPNET_NPARAMS]
  int M = 1;
  std::vector<sipnet_restart> resume;    // RESTART_IN: one per member (<path>.<m> in an ensemble)
  sipnet_ensemble_file* blockFile = nullptr;   // created once; every shard streams its own member range into it
  int hostThreads = 1;
  StatusSink sink;

  const std::string& debugLog() const { return run.ctx.s("debugLogPrefix"); }
  const std::string& restartOut() const { return run.ctx.s("restartOut"); }
  bool wantText() const { return !block.on() || block.text; }
  bool needRec() const { return wantText() || !restartOut().empty() || (block.on() && !block.planesOnly()); }
  bool fastByDefault() const { return mathArg == "fast" || (mathArg == "auto" && !table.empty()); }
  int sumK() const { return block.on() ? block.sums : 0; }
  int nGroups() const { return sumK() > 0 ? (run.T + sumK() - 1) / sumK() : 0; }
  std::string tag(int member) const { return table.empty() ? "" : "." + std::to_string(member); }
};

// the inputs of the run and of its members, then the first device call
void loadEnsemble(Ensemble& e) {
  resolveRun(e.run);
  e.members = e.table.empty() ? e.run.params : readMemberTable(e.table, e.run.params);
  e.M = (int)(e.members.size() / SIPNET_NPARAMS);
  const std::string restartIn = e.run.ctx.s("restartIn");
  if (!restartIn.empty()) {
    e.resume.resize(e.M);
    for (int m = 0; m < e.M; m++) readResume(restartIn + e.tag(m), e.run.flags, e.run.clim, e.resume[m]);
  }
  checkDevices(e.devices);
  if ((int)e.devices.size() > e.M) e.devices.resize(e.M);
}

// ---- --ensemble-stats: the ensemble as ONE node object -- shards, RCCL ranks and the all-gather behind the C-ABI ----
sipnet_node* runNode(const Ensemble& e) {
  const Run& r = e.run;
  std::vector<int32_t> devs(e.devices.begin(), e.devices.end());
  sipnet_node* nd = nullptr;
  check(sipnet_node_create(r.flags, 1, e.M, SIPNET_F64, devs.data(), (int32_t)devs.size(), &nd), "creating the node");
  logInfo("ensemble of " + std::to_string(e.M) + " members on " + std::to_string(devs.size()) +
          " device(s), collectives: " + sipnet_node_collective_library(nd) + "\n");
  check(sipnet_node_set_math(nd, e.mathArg == "strict" ? SIPNET_MATH_STRICT : SIPNET_MATH_FAST), "math policy");
  if (g_kernelOptions) check(sipnet_node_set_kernel(nd, SIPNET_KERNEL_AUTO, g_kernelOptions), "kernel options");
  check(sipnet_node_set_events(nd, 0, r.nEvents, r.events), "events");
  check(sipnet_node_set_climate(nd, 0, r.T, sipnet_clim_data(r.clim), sipnet_clim_year(r.clim), sipnet_clim_day(r.clim)), "climate");
  check(sipnet_node_set_params(nd, 0, 0, e.M, e.members.data()), "parameters");
  check(sipnet_node_setup(nd), "setupModel");
  check(sipnet_node_run(nd, 0, r.T), "run");
  return nd;
}
// `year day time n mean/sd of NEE, GPP, ET` per step from total[3][T][2], the members' sums and sums of squares
void writeStats(const std::string& path, const Run& r, int M, const std::vector<double>& total) {
  FILE* f = fopen(path.c_str(), "w");
  if (!f) die(6, "Error opening " + path + " for writing\n");
  if (r.ctx.i("printHeader")) fprintf(f, "year day time n meanNEE sdNEE meanGPP sdGPP meanET sdET\n");
  const double* cd = sipnet_clim_data(r.clim);
  for (int t = 0; t < r.T; t++) {
    fprintf(f, "%4d %3d %5.2f %d", sipnet_clim_year(r.clim)[t], sipnet_clim_day(r.clim)[t], cd[(size_t)t * SIPNET_NCLIM + 10], M);
    for (int v = 0; v < 3; v++) {
      const double s1 = total[((size_t)v * r.T + t) * 2], s2 = total[((size_t)v * r.T + t) * 2 + 1];
      // (s2 - s1^2 / M) / M in extended precision: s2 / M - mean^2 cancels badly when |mean| >> sd
      const long double s1l = s1, s2l = s2;
      const double mean = s1 / M, var = (double)((s2l - s1l * s1l / (long double)M) / (long double)M);
      fprintf(f, " %.10g %.10g", mean, var > 0 ? sqrt(var) : 0.0);
    }
    fprintf(f, "\n");
  }
  fclose(f);
}
int runEnsembleStats(Ensemble& e, const std::string& statsFile) {
  if (!e.resume.empty() || !e.restartOut().empty() || !e.debugLog().empty())
    die(8, "--ensemble-stats does not combine with restart checkpoints or --debug-log\n");
  sipnet_node* nd = runNode(e);
  std::vector<double> total((size_t)3 * e.run.T * 2);
  check(sipnet_node_gather_stats(nd, total.data()), "all-gather of the statistics");
  std::vector<int32_t> status(e.M);   // (synchronises every shard's stream: the runs are complete when it returns)
  check(sipnet_node_get_status(nd, status.data()), "status");
  reportStatus(status.data(), e.M, [](int m) { return "member " + std::to_string(m); }, e.sink);
  if (std::count(status.begin(), status.end(), 0) != e.M) die(e.sink.worst.load(), "the statistics would include members that did not run\n");
  writeStats(statsFile, e.run, e.M, total);
  sipnet_node_destroy(nd);
  freeRun(e.run);
  return 0;
}

// ---- the members' files and / or the block: contiguous member ranges, one host thread and one batch per device ----
struct Shard {
  int index, m0, Ms;       // members [m0, m0 + Ms) of the ensemble
  Batch batch;
  const double* params;    // [Ms][SIPNET_NPARAMS]
  std::vector<double> state0;
};
// the members of a shard that did not run, by their index in the ensemble
std::vector<int32_t> shardStatus(Ensemble& e, const Shard& sh) {
  std::vector<int32_t> status(sh.Ms);
  check(sipnet_batch_get_status(sh.batch.b, status.data(), nullptr), "status");
  reportStatus(status.data(), sh.Ms, [&](int m) { return "member " + std::to_string(sh.m0 + m); }, e.sink);
  return status;
}

// The block of sums: out of the step kernel's own launch where the batch has such a kernel (1 / K of the bytes ever leave
// the kernel), else the planes summed on the host in step order.
void shardSums(Ensemble& e, Shard& sh) {
  sipnet_batch* b = sh.batch.b;
  const int T = e.run.T, Ms = sh.Ms, sumK = e.sumK(), nGroups = e.nGroups();
  const bool inKernel = sipnet_batch_sums_in_kernel(b) != 0;
  const size_t rows = inKernel ? (size_t)nGroups : (size_t)T;
  const DevMem out((size_t)3 * rows * Ms);
  double* dOut = out.p;
  if (inKernel)
    check(sipnet_batch_run_sums(b, 0, T, sumK, dOut, dOut + rows * Ms, dOut + 2 * rows * Ms, Ms, nullptr), "run");
  else
    check(sipnet_batch_run(b, 0, T, dOut, dOut + rows * Ms, dOut + 2 * rows * Ms, nullptr, Ms, nullptr), "run");
  shardStatus(e, sh);
  std::vector<double> host(rows * Ms), sums;
  for (int v = 0; v < 3; v++) {
    check(sipnet_dev_to_host(host.data(), dOut + (size_t)v * rows * Ms, rows * Ms * sizeof(double), nullptr), "copy back");
    const double* src = host.data();
    if (!inKernel) {
      sums.assign((size_t)nGroups * Ms, 0.0);
      for (int t = 0; t < T; t++) {
        double* acc = &sums[(size_t)(t / sumK) * Ms];
        const double* row = &host[(size_t)t * Ms];
        for (int m = 0; m < Ms; m++) acc[m] += row[m];
      }
      src = sums.data();
    }
    check(sipnet_io_ensemble_put(e.blockFile, v, 0, nGroups, sh.m0, Ms, src, Ms, 0), "writing the ensemble block");
  }
  if (sh.index == 0)
    logInfo(std::string("ensemble block: sums over groups of ") + std::to_string(sumK) + " steps, " +
            (inKernel ? "from the step kernel's launch (" : "from the planes, on the host (") + sipnet_batch_last_kernel_name(b) + ")\n");
}

// the block alone, three planes: the lean kernels, nothing but the planes leaves the device
void shardPlanes(Ensemble& e, Shard& sh) {
  const int T = e.run.T, Ms = sh.Ms;
  const DevMem planes((size_t)3 * T * Ms);
  check(sipnet_batch_run(sh.batch.b, 0, T, planes.p, planes.p + (size_t)T * Ms, planes.p + (size_t)2 * T * Ms, nullptr, Ms, nullptr), "run");
  shardStatus(e, sh);
  putBlock(e.blockFile, e.block, T, Ms, T, 0, Ms, sh.m0, planes.p, nullptr);
}

// The block alone, named `.out` columns: the 44-column record exists on the device only, a segment of steps at a time
// (the whole record of 10 240 members x a half-hourly year is 63 GB: allocating it took 25 s of a 27 s run).
void shardColumns(Ensemble& e, Shard& sh) {
  const int T = e.run.T, Ms = sh.Ms;
  int64_t segSteps = (int64_t)(3.0e9 / ((double)SIPNET_NREC * Ms * sizeof(double)));
  segSteps = std::max<int64_t>(16, segSteps & ~(int64_t)15);
  if (e.block.segment > 0) segSteps = e.block.segment;
  if (segSteps > T) segSteps = T;
  const DevMem seg((size_t)segSteps * SIPNET_NREC * Ms);
  for (int t0 = 0; t0 < T; t0 += (int)segSteps) {
    const int len = (int)std::min<int64_t>(segSteps, T - t0);
    check(sipnet_batch_run(sh.batch.b, t0, len, nullptr, nullptr, nullptr, seg.p, Ms, nullptr), "run");
    putBlock(e.blockFile, e.block, len, Ms, len, 0, Ms, sh.m0, nullptr, seg.p, t0);
  }
  shardStatus(e, sh);
}

// the 44-column record of the whole run on the device; with --debug-log the per-step flux / tracker dump of debug_log.c
void runRecord(const Ensemble& e, const Shard& sh, double* dRec, double* dDbg) {
  const int T = e.run.T;
  if (dDbg) {
    check(sipnet_batch_run_debug(sh.batch.b, 0, T, dRec, dDbg, sh.Ms, nullptr), "run");
    return;
  }
  const double t0 = nowSeconds();
  check(sipnet_batch_run(sh.batch.b, 0, T, nullptr, nullptr, nullptr, dRec, sh.Ms, nullptr), "run");
  check(sipnet_stream_sync(nullptr), "run");
  char msg[160];
  snprintf(msg, sizeof msg, "members %d..%d: %d steps with the 44-column record in %.3f s\n", sh.m0, sh.m0 + sh.Ms - 1, T, nowSeconds() - t0);
  logInfo(msg);
}
// The text of an ensemble is the slow part of the job (about 120 MB/s of printf per host thread against tens of ms of GPU
// time), so members are formatted by a pool of host threads; only the checkpoint export, which talks to the GPU through
// the one batch handle, is serialised.
void writeShardFiles(Ensemble& e, const Shard& sh, const std::vector<int32_t>& status, const std::vector<double>& rec,
                     const std::vector<double>& dbg) {
  const int T = e.run.T, Ms = sh.Ms;
  const Context& ctx = e.run.ctx;
  std::mutex gpuMutex;
  std::atomic<int> next{0};
  auto worker = [&]() {
    std::vector<double> one((size_t)T * SIPNET_NREC), oneDbg(dbg.empty() ? 0 : (size_t)T * SIPNET_NDBG);
    for (int m = next.fetch_add(1); m < Ms; m = next.fetch_add(1)) {
      if (status[m] != 0) continue;
      extractMember(one, rec, T, SIPNET_NREC, Ms, m);
      if (!dbg.empty()) extractMember(oneDbg, dbg, T, SIPNET_NDBG, Ms, m);
      const std::string tag = e.tag(sh.m0 + m);
      const Member mem{sh.batch.b, 0, m, &e.run, sh.params + (size_t)m * SIPNET_NPARAMS, sh.state0.data() + (size_t)m * SIPNET_NSTATE,
                       one.data(), oneDbg.data()};
      writeMemberFiles(mem, memberFiles(ctx, e.wantText(), ctx.s("filePrefix") + tag, ctx.s("eventsPrefix") + tag,
                                        e.debugLog().empty() ? "" : e.debugLog() + tag, e.restartOut().empty() ? "" : e.restartOut() + tag),
                       gpuMutex, e.sink.logMutex);
    }
  };
  runThreads(std::max(1, std::min({e.hostThreads / (int)e.devices.size(), Ms, 64})), worker);
}
// the full record: the members' text files, checkpoints and debug logs, and the block beside them
void shardRecord(Ensemble& e, Shard& sh) {
  const size_t recElems = (size_t)e.run.T * SIPNET_NREC * sh.Ms;
  const size_t dbgElems = e.debugLog().empty() ? 0 : (size_t)e.run.T * SIPNET_NDBG * sh.Ms;
  const DevMem dRec(recElems), dDbg(dbgElems);
  runRecord(e, sh, dRec.p, dDbg.p);
  if (e.blockFile) putBlock(e.blockFile, recordColumns(e.block), e.run.T, sh.Ms, e.run.T, 0, sh.Ms, sh.m0, nullptr, dRec.p);
  // (what follows needs every record on the host)
  std::vector<double> rec(recElems), dbg(dbgElems);
  check(sipnet_dev_to_host(rec.data(), dRec.p, recElems * sizeof(double), nullptr), "copy back");
  if (dbgElems) check(sipnet_dev_to_host(dbg.data(), dDbg.p, dbgElems * sizeof(double), nullptr), "copy back");
  writeShardFiles(e, sh, shardStatus(e, sh), rec, dbg);
}

void runShard(Ensemble& e, int index) {
  const int nShards = (int)e.devices.size();
  Shard sh;
  sh.index = index;
  sh.m0 = (int)((int64_t)e.M * index / nShards);
  sh.Ms = (int)((int64_t)e.M * (index + 1) / nShards) - sh.m0;
  sh.params = e.members.data() + (size_t)sh.m0 * SIPNET_NPARAMS;
  // A single run writes the reference's bytes: strict operation order (never the environment's choice).  An ensemble runs
  // on the throughput kernels (their Full instantiations write the same 44-column record; <= 2e-14 from the strict kernel
  // on the fluxes, invisible at the precision `.out` prints) unless --math strict asks otherwise; --debug-log needs strict.
  const bool fastMath = e.debugLog().empty() && e.fastByDefault();
  setupBatch(sh.batch, e.run.flags, sh.Ms, e.devices[index], fastMath,
             {SiteInput{&e.run, sh.params, e.resume.empty() ? nullptr : e.resume.data() + sh.m0}});
  sh.state0.resize((size_t)sh.Ms * SIPNET_NSTATE);
  check(sipnet_batch_get_state(sh.batch.b, sh.state0.data(), nullptr), "state");
  if (!e.needRec() && e.sumK() > 0)
    shardSums(e, sh);
  else if (!e.needRec())
    shardPlanes(e, sh);
  else if (!e.wantText() && e.restartOut().empty() && e.debugLog().empty())
    shardColumns(e, sh);
  else
    shardRecord(e, sh);
}

void createEnsembleBlock(Ensemble& e) {
  std::string attrs = "parameter_table=" + e.table + "\nmath=" + (e.fastByDefault() ? "fast" : "strict");
  if (e.sumK() > 0) {
    if (!e.restartOut().empty() || !e.debugLog().empty()) die(8, "--ensemble-out-sums does not combine with restart output / --debug-log\n");
    e.blockFile = createSumsBlock(e.block, e.run.T, e.M, e.run.clim, attrs + "\nsums_over_steps=" + std::to_string(e.sumK()));
  } else {
    e.blockFile = createBlock(e.block, e.block.path, e.run.T, e.M, e.run.clim, nullptr, attrs);
  }
}
int runEnsemble(Ensemble& e) {
  const int nShards = (int)e.devices.size();
  if (nShards > 1) logInfo("ensemble sharded over " + std::to_string(nShards) + " device(s)\n");
  if (e.block.on() && !e.debugLog().empty()) die(8, "--ensemble-out does not combine with --debug-log\n");
  if (e.block.on()) createEnsembleBlock(e);
  e.hostThreads = hostThreadCount();
  runShards(nShards, [&](int k) { runShard(e, k); });
  if (e.blockFile) check(sipnet_io_ensemble_close(e.blockFile), "closing the ensemble block");
  freeRun(e.run);
  return e.sink.worst.load();
}
