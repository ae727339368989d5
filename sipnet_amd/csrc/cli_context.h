// cli_context.h -- part of sipnet_cli.cpp: the run's configuration as the reference keeps it (context.c): defaults, sipnet.in,
// the flag options, --dump-config, the flag-coupling rules, and the usage text.
#pragma once

enum Source { SRC_DEFAULT = 0, SRC_FILE, SRC_CLI, SRC_CALCULATED };
const char* sourceName(int s) {
  static const char* n[] = {"DEFAULT", "INPUT_FILE", "COMMAND_LINE", "CALCULATED"};
  return n[s];
}

struct Entry {
  std::string printName;
  bool isInt;
  int ival;
  std::string sval;
  int source;
};

// context.c:76-90
std::string keyOf(const std::string& name) {
  std::string k;
  for (char c : name)
    if (isalnum((unsigned char)c)) k += (char)tolower((unsigned char)c);
  if (k == "filename") k = "fileprefix";
  return k;
}

struct Context {
  std::map<std::string, Entry> m;  // ordered by key == HASH_SORT(by_name)
  void addInt(const char* name, const char* print, int v) { m[keyOf(name)] = {print, true, v, "", SRC_DEFAULT}; }
  void addStr(const char* name, const char* print, const char* v) { m[keyOf(name)] = {print, false, 0, v, SRC_DEFAULT}; }
  Entry* find(const std::string& name) {
    auto it = m.find(keyOf(name));
    return it == m.end() ? nullptr : &it->second;
  }
  void setInt(const std::string& name, int v, int src) {
    Entry* e = find(name);
    if (e && e->source <= src) { e->ival = v; e->source = src; }
  }
  void setStr(const std::string& name, const std::string& v, int src) {
    Entry* e = find(name);
    if (e && e->source <= src) { e->sval = v; e->source = src; }
  }
  int i(const char* name) const { return m.at(keyOf(name)).ival; }
  const std::string& s(const char* name) const { return m.at(keyOf(name)).sval; }
};

void initContext(Context& c) {  // context.c:26-71
  c.addInt("events", "EVENTS", 1);
  c.addInt("gdd", "GDD", 1);
  c.addInt("growthResp", "GROWTH_RESP", 0);
  c.addInt("leafWater", "LEAF_WATER", 0);
  c.addInt("litterPool", "LITTER_POOL", 0);
  c.addInt("snow", "SNOW", 1);
  c.addInt("soilPhenol", "SOIL_PHENOL", 0);
  c.addInt("waterHResp", "WATER_HRESP", 1);
  c.addInt("nitrogenCycle", "NITROGEN_CYCLE", 0);
  c.addInt("anaerobic", "ANAEROBIC", 0);
  c.addInt("flooding", "FLOODING", 0);
  c.addInt("carbonSaturation", "CARBON_SATURATION", 0);
  c.addInt("doMainOutput", "DO_MAIN_OUTPUT", 1);
  c.addInt("doSingleOutputs", "DO_SINGLE_OUTPUT", 0);
  c.addInt("dumpConfig", "DUMP_CONFIG", 0);
  c.addInt("printHeader", "PRINT_HEADER", 1);
  c.addInt("quiet", "QUIET", 0);
  c.addStr("paramFile", "PARAM_FILE", "");
  c.addStr("climFile", "CLIM_FILE", "");
  c.addStr("outFile", "OUT_FILE", "");
  c.addStr("outConfigFile", "OUT_CONFIG_FILE", "");
  c.addStr("eventsPrefix", "EVENTS_PREFIX", "events");
  c.addStr("inputFile", "INPUT_FILE", "sipnet.in");
  c.addStr("restartIn", "RESTART_IN", "");
  c.addStr("restartOut", "RESTART_OUT", "");
  c.addStr("debugLogPrefix", "DEBUG_LOG_PREFIX", "");
  c.addStr("filePrefix", "FILE_PREFIX", "sipnet");
}

const char* kFlagOpts[][2] = {  // cli.c:20-44 option name -> context field
    {"events", "events"}, {"gdd", "gdd"}, {"growth-resp", "growthResp"},
    {"leaf-water", "leafWater"}, {"litter-pool", "litterPool"}, {"snow", "snow"},
    {"soil-phenol", "soilPhenol"}, {"water-hresp", "waterHResp"},
    {"nitrogen-cycle", "nitrogenCycle"}, {"anaerobic", "anaerobic"}, {"flooding", "flooding"},
    {"carbon-saturation", "carbonSaturation"}, {"do-main-output", "doMainOutput"},
    {"do-single-outputs", "doSingleOutputs"}, {"dump-config", "dumpConfig"},
    {"print-header", "printHeader"}, {"quiet", "quiet"}};
constexpr int kNumFlagOpts = sizeof(kFlagOpts) / sizeof(kFlagOpts[0]);

void usage(const char* prog) {
  printf("Usage: %s [OPTIONS]\n\n", prog);
  printf("Run SIPNET model for one site with configured options (MI355X engine).\n\n");
  printf("  -i, --input-file <path>     Name of input config file ('sipnet.in')\n");
  printf("  -f, --file-prefix <name>    Prefix of climate and parameter files ('sipnet')\n");
  printf("      --file-name <name>      Backward-compatible alias for --file-prefix\n");
  printf("  -e, --events-prefix <name>  Prefix of events input/output files ('events')\n");
  printf("Model flags (prepend 'no-' to force off): --anaerobic --events --flooding --gdd\n");
  printf("  --growth-resp --leaf-water --litter-pool --nitrogen-cycle --snow --soil-phenol\n");
  printf("  --water-hresp --carbon-saturation\n");
  printf("Output flags: --do-main-output --do-single-outputs --dump-config --print-header --quiet\n");
  printf("      --restart-in <path>     Read a restart checkpoint from path\n");
  printf("      --restart-out <path>    Write a restart checkpoint to path at end of run\n");
  printf("  --ensemble-params <file>    run one member per row of a parameter table in one batch\n");
  printf("  --math strict|fast|auto     arithmetic of the step kernel (auto: strict for one run, fast for an ensemble)\n");
  printf("  --devices <list>            HIP devices the ensemble shards across, e.g. 0-7 or 0,2,3 ('0')\n");
  printf("  --ensemble-stats <file>     per-step ensemble mean / sd of NEE, GPP, ET instead of the members' files\n");
  printf("  --sites <file>              run every directory listed in <file> (one per line) in shared batches\n");
  printf("  --ensemble-out <file.nc>    (--ensemble-params / --sites) all members' outputs as one NetCDF-3 block instead of\n");
  printf("                              the members' text files: nee, gpp, evapotranspiration -- or, with\n");
  printf("      --ensemble-out-columns <a,b,..|all>  the named .out columns; --ensemble-out-f32 stores floats;\n");
  printf("      --ensemble-out-sums <K>  (planes only) every member's sums over groups of K steps (48: daily sums);\n");
  printf("      --ensemble-text         writes the text files as well\n");
  printf("  --bounded-waits             cooperative kernels with bounded hand-over waits (a stuck wait is reported, not a hang)\n");
  printf("  -h, --help   -v, --version\n");
}

// frontend.c:35-128
void readInputFile(Context& c) {
  const std::string path = c.s("inputFile");
  logInfo("Reading config from file " + path + "\n");
  std::ifstream in(path);
  if (!in) die(6, "Error opening " + path + " for reading\n");
  std::string line;
  while (std::getline(in, line)) {
    const size_t bang = line.find('!');
    if (bang != std::string::npos) line.erase(bang);
    // name: up to " \t=:" ; value: up to " \t=:\n\r"
    std::vector<std::string> tok;
    size_t i = 0;
    while (i < line.size() && tok.size() < 2) {
      while (i < line.size() && strchr(" \t=:\r\n", line[i])) i++;
      size_t j = i;
      while (j < line.size() && !strchr(" \t=:\r\n", line[j])) j++;
      if (j > i) tok.push_back(line.substr(i, j - i));
      i = j;
    }
    if (tok.empty()) continue;
    if (strcasecmp(tok[0].c_str(), "runtype") == 0) {
      if (tok.size() > 1 && strcasecmp(tok[1].c_str(), "standard") != 0)
        die(3, "RUNTYPE is obsolete; only 'standard' is accepted. Please fix " + path + " and re-run\n");
      continue;
    }
    Entry* e = c.find(tok[0]);
    if (!e) {
      logInfo("ignoring input file parameter " + tok[0] + "\n");
      continue;
    }
    if (tok.size() < 2)
      die(3, "Error in input file: No value given for input item " + tok[0] + "\n");
    if (e->isInt) {
      char* end = nullptr;
      const long v = strtol(tok[1].c_str(), &end, 0);
      if (*end) die(3, "ERROR in input file: Invalid value for " + tok[0] + ": " + tok[1] + "\n");
      c.setInt(tok[0], (int)v, SRC_FILE);
    } else {
      c.setStr(tok[0], tok[1] == "none" ? "" : tok[1], SRC_FILE);
    }
  }
}

// context.c:225-268
void printConfig(const Context& c, FILE* f) {
  unsigned width = 0;
  for (auto& kv : c.m)
    if (!kv.second.isInt) width = std::max<unsigned>(width, (unsigned)kv.second.printName.size());
  if (c.i("printHeader")) {
    char ts[100];
    time_t now;
    time(&now);
    strftime(ts, sizeof ts, "%Y-%m-%d %H:%M:%S UTC", gmtime(&now));
    fprintf(f, "Final config for SIPNET run at %s\n", ts);
    fprintf(f, "%21s %13s %*s\n", "Name", "Source", width, "Value");
  }
  for (auto& kv : c.m) {
    const Entry& e = kv.second;
    if (e.isInt)
      fprintf(f, "%21s %13s %*d\n", e.printName.c_str(), sourceName(e.source), width, e.ival);
    else
      fprintf(f, "%21s %13s %*s\n", e.printName.c_str(), sourceName(e.source), width, e.sval.c_str());
  }
}


// validateContext (context.c:195-223): the flag-coupling rules, every broken one named before the process ends
void checkFlagCoupling(const Context& ctx) {
  bool bad = false;
  if (ctx.i("soilPhenol") && ctx.i("gdd")) { logError("soil-phenol and gdd may not both be turned on\n"); bad = true; }
  if (ctx.i("nitrogenCycle") && !(ctx.i("litterPool") && ctx.i("anaerobic"))) {
    logError("nitrogen-cycle requires both litter-pool and anaerobic to be turned on\n"); bad = true; }
  if (ctx.i("anaerobic") && !ctx.i("waterHResp")) { logError("anaerobic requires water-hresp to be turned on\n"); bad = true; }
  if (ctx.i("carbonSaturation") && !ctx.i("litterPool")) { logError("carbon-saturation requires litter-pool to be turned on\n"); bad = true; }
  if (bad) exit(3);
}
