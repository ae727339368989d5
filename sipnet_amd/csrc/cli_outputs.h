// cli_outputs.h -- part of sipnet_cli.cpp: what a batch that has run leaves behind on the host side -- the report of the
// members that did not run, and one member's files.
#pragma once

// the worst status of the process's runs, and the lock its host threads log under
struct StatusSink {
  std::atomic<int> worst{0};
  std::mutex logMutex;
};
// The runs of a batch that did not run: status[k] of the run that nameOf(k) names ("member 12", a run directory), one
// line each in ascending order.
template <class NameOf>
void reportStatus(const int32_t* status, int n, NameOf&& nameOf, StatusSink& sink) {
  for (int k = 0; k < n; k++) {
    if (status[k] == 0) continue;
    std::lock_guard<std::mutex> lock(sink.logMutex);
    logError(nameOf(k) + ": status " + std::to_string(status[k]) +
             " (NPP allocation params must be less than one individually and add to less than one)\n");
    int w = sink.worst.load();
    while (status[k] > w && !sink.worst.compare_exchange_weak(w, status[k])) {}
  }
}

// column `col` of a device-layout result src[T][width][ld] as one member's dense dst[T][width]
void extractMember(std::vector<double>& dst, const std::vector<double>& src, int T, int width, int64_t ld, int64_t col) {
  for (int t = 0; t < T; t++)
    for (int k = 0; k < width; k++) dst[(size_t)t * width + k] = src[((size_t)t * width + k) * ld + col];
}

// One member of a batch that has run its site to the end: where it sits in the batch and what it gave.
struct Member {
  sipnet_batch* b;
  int site, member;
  const Run* run;         // its forcing, flags and PRINT_HEADER
  const double* params;   // its parameter row
  const double* state0;   // its state before the first step
  const double* rec;      // [T][SIPNET_NREC]
  const double* dbg;      // [T][SIPNET_NDBG], with --debug-log
};
// the names its files go by; an empty one is not written
struct MemberFiles {
  std::string out, eventsOut, debugLog, checkpoint, singleStem;
};
// The text files follow the run's output flags: <stem>.out, <eventsStem>.out, <stem>.NEE ...
MemberFiles memberFiles(const Context& ctx, bool wantText, const std::string& stem, const std::string& eventsStem,
                        const std::string& debugLog, const std::string& checkpoint) {
  MemberFiles f;
  if (wantText && ctx.i("doMainOutput")) f.out = stem + ".out";
  if (wantText && ctx.i("events")) f.eventsOut = eventsStem + ".out";
  if (wantText && ctx.i("doSingleOutputs")) f.singleStem = stem;
  f.debugLog = debugLog;
  f.checkpoint = checkpoint;
  return f;
}

// restartWriteCheckpoint (restart.c:932-996)
void writeCheckpoint(const Member& m, std::mutex& gpuMutex, std::mutex& logMutex, const std::string& path) {
  const int T = m.run->T;
  const double* prevPools = T >= 2 ? m.rec + (size_t)(T - 2) * SIPNET_NREC + 14 : m.state0;
  sipnet_restart ck;
  {
    std::lock_guard<std::mutex> lock(gpuMutex);   // (the export talks to the GPU through the one batch handle)
    check(sipnet_batch_export_restart(m.b, m.site, m.member, T, m.rec + (size_t)(T - 1) * SIPNET_NREC, prevPools, &ck, nullptr),
          "restart checkpoint");
  }
  int32_t warn = 0;
  check(sipnet_restart_check_boundary_for_write(&ck, &warn), "restart checkpoint");
  if (warn & SIPNET_RESTART_WARN_BOUNDARY_NOT_MIDNIGHT) {
    std::lock_guard<std::mutex> lock(logMutex);
    logWarning("Restart checkpoint " + path + " ends more than one timestep before midnight; "
               "there will be a time gap if this file is used to resume.\n");
  }
  check(sipnet_io_write_restart(path.c_str(), &ck), "writing restart checkpoint");
}

// sipnet.c:1993-1998, outputItems.c:126-150
void writeSingleOutputs(const std::string& stem, int T, const double* rec) {
  const struct { const char* name; int col; } items[] = {{"NEE", 0}, {"NEE_cum", 3}, {"GPP", 1}, {"GPP_cum", 35}};
  for (const auto& it : items) {
    FILE* f = fopen((stem + "." + it.name).c_str(), "w");
    if (!f) die(6, std::string("Error opening single output file for ") + it.name + "\n");
    for (int t = 0; t < T; t++) fprintf(f, "%f ", rec[(size_t)t * SIPNET_NREC + it.col]);
    fprintf(f, "\n");
    fclose(f);
  }
}

void writeMemberFiles(const Member& m, const MemberFiles& names, std::mutex& gpuMutex, std::mutex& logMutex) {
  const Run& r = *m.run;
  const int header = r.ctx.i("printHeader");
  const int32_t *year = sipnet_clim_year(r.clim), *day = sipnet_clim_day(r.clim);
  const double* clim = sipnet_clim_data(r.clim);
  if (!names.debugLog.empty())
    check(sipnet_io_write_debug_logs(names.debugLog.c_str(), header, r.T, year, day, clim, m.rec, m.dbg), "writing debug logs");
  if (!names.out.empty()) check(sipnet_io_write_out(names.out.c_str(), header, r.T, year, day, clim, m.rec), "writing output");
  if (!names.eventsOut.empty())
    check(sipnet_io_write_events_out(names.eventsOut.c_str(), header, r.flags, m.params, r.T, year, day, clim, r.nEvents, r.events,
                                     m.rec, m.state0), "writing events.out");
  if (!names.checkpoint.empty()) writeCheckpoint(m, gpuMutex, logMutex, names.checkpoint);
  if (!names.singleStem.empty()) writeSingleOutputs(names.singleStem, r.T, m.rec);
}
