// cli_sites.h -- part of sipnet_cli.cpp: --sites, many run directories in few batches.  Runs with the same model flags
// share a batch, runs with identical forcing (and resume state) are members of one site of it, and every directory gets
// the files its own run would have written.
#pragma once

std::vector<std::string> readSiteList(const std::string& listFile) {
  std::ifstream in(listFile);
  if (!in) die(6, "Error opening " + listFile + " for reading\n");
  std::vector<std::string> dirs;
  for (std::string line; std::getline(in, line);) {
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.erase(hash);
    const size_t a = line.find_first_not_of(" \t\r"), z = line.find_last_not_of(" \t\r");
    if (a == std::string::npos) continue;
    dirs.push_back(line.substr(a, z - a + 1));
  }
  if (dirs.empty()) die(5, "no run directories in " + listFile + "\n");
  return dirs;
}

// every directory resolved like a run started inside it, under the options of this command line
std::vector<Run> resolveSites(const Context& cliCtx, const std::vector<std::string>& dirs) {
  char cwd0[4096];
  if (!getcwd(cwd0, sizeof cwd0)) die(1, "getcwd failed\n");
  std::vector<Run> runs(dirs.size());
  for (size_t k = 0; k < dirs.size(); k++) {
    if (chdir(cwd0) != 0 || chdir(dirs[k].c_str()) != 0) die(6, "cannot enter run directory " + dirs[k] + "\n");
    char here[4096];
    if (!getcwd(here, sizeof here)) die(1, "getcwd failed\n");
    runs[k].dir = here;
    runs[k].ctx = cliCtx;
    resolveRun(runs[k]);
    resolveRestart(runs[k]);
  }
  if (chdir(cwd0) != 0) die(1, "cannot return to the start directory\n");
  return runs;
}

using SiteList = std::vector<std::vector<int>>;   // [site][member] -> run index
// batches: same model flags (any length); inside a batch, runs with identical forcing (and resume state) are members of ONE site
std::vector<SiteList> groupRuns(const std::vector<Run>& runs) {
  std::vector<char> done(runs.size(), 0);
  std::vector<SiteList> groups;
  for (size_t lead = 0; lead < runs.size(); lead++) {
    if (done[lead]) continue;
    SiteList sites;
    for (size_t k = lead; k < runs.size(); k++) {
      if (done[k] || memcmp(runs[k].flags, runs[lead].flags, sizeof runs[k].flags) != 0) continue;
      done[k] = 1;
      auto st = std::find_if(sites.begin(), sites.end(), [&](const std::vector<int>& s) { return sameForcing(runs[s[0]], runs[k]); });
      if (st == sites.end())
        sites.push_back({(int)k});
      else
        st->push_back((int)k);
    }
    groups.push_back(std::move(sites));
  }
  return groups;
}

// what the batches of a --sites process share
struct SitesJob {
  std::vector<Run> runs;
  std::vector<int> devices;
  BlockSpec block;
  bool fastMath, wantText;
  size_t nSitesTotal = 0;
  int hostThreads = 1, nBatches = 0;
  std::mutex batchMutex;
  StatusSink sink;
};
// one block per distinct forcing: FILE itself when there is one, else <stem>.<first run><ext>
std::string blockPathOf(const SitesJob& job, int firstRun) {
  const std::string& path = job.block.path;
  if (job.nSitesTotal == 1) return path;
  const size_t slash = path.find_last_of('/'), dot = path.find_last_of('.');
  const bool hasExt = dot != std::string::npos && (slash == std::string::npos || dot > slash);
  const std::string stem = hasExt ? path.substr(0, dot) : path, ext = hasExt ? path.substr(dot) : "";
  return stem + "." + std::to_string(firstRun) + ext;
}

// One batch: a contiguous range of a flag set's sites on one device.
struct Part {
  SiteList sites;
  int device, nParts;
  int S, M = 0, T = 0;          // sites x the widest site's members; T: the longest forcing (its sites may be shorter)
  bool anyCheckpoint = false;
  Batch batch;
  std::vector<double> state0;
  struct Job { int run, site, member; int64_t col; };
  std::vector<Job> jobs;        // the runs, in ascending column order
  int64_t ncol() const { return (int64_t)S * M; }
};
void shapePart(const SitesJob& job, Part& p) {
  p.S = (int)p.sites.size();
  for (auto& st : p.sites) {
    p.M = std::max(p.M, (int)st.size());
    p.T = std::max(p.T, job.runs[st[0]].T);
    for (int k : st) p.anyCheckpoint = p.anyCheckpoint || !job.runs[k].restartOut.empty();
  }
  for (int s = 0; s < p.S; s++)
    for (int m = 0; m < (int)p.sites[s].size(); m++) p.jobs.push_back({p.sites[s][m], s, m, (int64_t)s * p.M + m});
}
// (a site with fewer runs than the widest one: its first run's parameters and checkpoint fill the rest)
void setupPartBatch(const SitesJob& job, Part& p) {
  std::vector<std::vector<double>> rows(p.S, std::vector<double>((size_t)p.M * SIPNET_NPARAMS));
  std::vector<std::vector<sipnet_restart>> cks(p.S);
  std::vector<SiteInput> inputs;
  for (int s = 0; s < p.S; s++) {
    const Run& r0 = job.runs[p.sites[s][0]];
    if (r0.hasResume) cks[s].resize(p.M);
    for (int m = 0; m < p.M; m++) {
      const Run& r = job.runs[p.sites[s][m < (int)p.sites[s].size() ? m : 0]];
      memcpy(rows[s].data() + (size_t)m * SIPNET_NPARAMS, r.params.data(), SIPNET_NPARAMS * sizeof(double));
      if (r0.hasResume) cks[s][m] = r.resume;
    }
    inputs.push_back({&r0, rows[s].data(), r0.hasResume ? cks[s].data() : nullptr});
  }
  setupBatch(p.batch, job.runs[p.sites[0][0]].flags, p.M, p.device, job.fastMath, inputs);
}

// the runs of the batch that did not run, by their directories
std::vector<int32_t> partStatus(SitesJob& job, const Part& p) {
  std::vector<int32_t> status(p.ncol());
  check(sipnet_batch_get_status(p.batch.b, status.data(), nullptr), "status");
  std::vector<int32_t> ofJob;
  for (const auto& j : p.jobs) ofJob.push_back(status[j.col]);
  reportStatus(ofJob.data(), (int)ofJob.size(), [&](int j) { return job.runs[p.jobs[j].run].dir; }, job.sink);
  return status;
}

// one block per site: its runs are the members
void writeSiteBlocks(const SitesJob& job, const Part& p, const double* dPlanes, const double* dRec) {
  for (int s = 0; s < p.S; s++) {
    const std::vector<int>& site = p.sites[s];
    const Run& r0 = job.runs[site[0]];
    const int n = (int)site.size();
    std::vector<int32_t> ids(site.begin(), site.end());
    std::string attrs = "run_dirs=";
    for (int m = 0; m < n; m++) attrs += (m ? " " : "") + job.runs[site[m]].dir;
    attrs += "\nmath=" + std::string(job.fastMath ? "fast" : "strict");
    sipnet_ensemble_file* f = createBlock(job.block, blockPathOf(job, site[0]), r0.T, n, r0.clim, ids.data(), attrs);
    putBlock(f, dRec ? recordColumns(job.block) : job.block, r0.T, p.ncol(), p.T, (int64_t)s * p.M, n, 0, dPlanes, dRec);
    check(sipnet_io_ensemble_close(f), "closing the ensemble block");
  }
}

// every run's files, into its own directory (absolute paths), by a pool of host threads
void writePartFiles(SitesJob& job, const Part& p, const std::vector<int32_t>& status, const std::vector<double>& rec) {
  std::mutex gpuMutex;
  std::atomic<int> next{0};
  auto worker = [&]() {
    std::vector<double> one((size_t)p.T * SIPNET_NREC);
    for (int j = next.fetch_add(1); j < (int)p.jobs.size(); j = next.fetch_add(1)) {
      const Part::Job& jb = p.jobs[j];
      const Run& r = job.runs[jb.run];
      if (status[jb.col] != 0) continue;
      extractMember(one, rec, r.T, SIPNET_NREC, p.ncol(), jb.col);   // (this run's own length, not the batch's longest)
      const Member mem{p.batch.b, jb.site, jb.member, &r, r.params.data(), p.state0.data() + (size_t)jb.col * SIPNET_NSTATE, one.data(), nullptr};
      writeMemberFiles(mem, memberFiles(r.ctx, job.wantText, joinPath(r.dir, r.ctx.s("filePrefix")), joinPath(r.dir, r.ctx.s("eventsPrefix")),
                                        "", r.restartOut), gpuMutex, job.sink.logMutex);
    }
  };
  runThreads(std::max(1, std::min({job.hostThreads / p.nParts, (int)p.jobs.size(), 64})), worker);
}

void runPart(SitesJob& job, Part& p) {
  shapePart(job, p);
  {
    std::lock_guard<std::mutex> lock(job.batchMutex);
    job.nBatches++;
    logInfo("batch " + std::to_string(job.nBatches) + " (device " + std::to_string(p.device) + "): " + std::to_string(p.S) +
            " site(s) x up to " + std::to_string(p.M) + " member(s), up to " + std::to_string(p.T) + " steps\n");
  }
  setupPartBatch(job, p);
  const bool hostFiles = job.wantText || p.anyCheckpoint;
  if (hostFiles) {
    p.state0.resize((size_t)p.ncol() * SIPNET_NSTATE);
    check(sipnet_batch_get_state(p.batch.b, p.state0.data(), nullptr), "state");
  }
  // the block alone, planes: the lean kernels and three planes; anything else needs the 44-column record
  const bool needRec = hostFiles || (job.block.on() && !job.block.planesOnly());
  const size_t plane = (size_t)p.T * p.ncol(), recElems = needRec ? plane * SIPNET_NREC : 0;
  const DevMem dRec(recElems), dPlanes(needRec ? 0 : 3 * plane);
  if (needRec)
    check(sipnet_batch_run(p.batch.b, 0, p.T, nullptr, nullptr, nullptr, dRec.p, p.ncol(), nullptr), "run");
  else
    check(sipnet_batch_run(p.batch.b, 0, p.T, dPlanes.p, dPlanes.p + plane, dPlanes.p + 2 * plane, nullptr, p.ncol(), nullptr), "run");
  const std::vector<int32_t> status = partStatus(job, p);
  if (job.block.on()) writeSiteBlocks(job, p, dPlanes.p, dRec.p);
  if (!hostFiles) return;
  std::vector<double> rec(recElems);
  check(sipnet_dev_to_host(rec.data(), dRec.p, recElems * sizeof(double), nullptr), "copy back");
  writePartFiles(job, p, status, rec);
}

int runSites(const Context& cliCtx, const std::string& listFile, const std::string& mathArg, const std::vector<int>& devices,
             const BlockSpec& block) {
  SitesJob job;
  job.runs = resolveSites(cliCtx, readSiteList(listFile));
  checkDevices(devices);
  job.devices = devices;
  job.block = block;
  job.fastMath = mathArg == "fast" || (mathArg == "auto" && block.on() && !block.text);
  job.wantText = !block.on() || block.text;
  job.hostThreads = hostThreadCount();
  const std::vector<SiteList> groups = groupRuns(job.runs);
  for (const auto& sites : groups) job.nSitesTotal += sites.size();
  for (const SiteList& sites : groups) {
    // the sites of a flag set are dealt to the listed devices in contiguous ranges (whole sites per device, as
    // SIPNET_SHARD_SITES does: a site's forcing, events and plan exist on one device only); each range is one batch,
    // driven by a host thread of its own
    const int nParts = std::max(1, std::min((int)devices.size(), (int)sites.size()));
    runShards(nParts, [&](int k) {
      Part p;
      p.sites.assign(sites.begin() + sites.size() * k / nParts, sites.begin() + sites.size() * (k + 1) / nParts);
      p.device = devices[k];
      p.nParts = nParts;
      runPart(job, p);
    });
  }
  logInfo(std::to_string(job.runs.size()) + " run(s) in " + std::to_string(job.nBatches) + " batch(es)\n");
  for (auto& r : job.runs) freeRun(r);
  return job.sink.worst.load();
}
