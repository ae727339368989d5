// sipnet_cli.cpp -- `sipnet`-compatible command line over the C-ABI (drop-in at the process
// level, the boundary PEcAn uses: one working directory with sipnet.in / <prefix>.param /
// <prefix>.clim / <events>.in, producing <prefix>.out, <events>.out, <prefix>.config).
//
// Behaviour mirrored from the reference (paths relative to the reference's src/):
//   option table and precedence     sipnet/cli.c:20-57,144-229; common/context.c:17-25,143-170
//   sipnet.in syntax                sipnet/frontend.c:35-128
//   flag coupling rules             common/context.c:195-223
//   derived file names, run order   sipnet/frontend.c:130-253
//   --dump-config format            common/context.c:225-268
//   single-variable outputs         sipnet/outputItems.c:126-150, sipnet/sipnet.c:1993-1998
//   restart checkpoints             sipnet/sipnet.c:1963-1989, sipnet/restart.c:932-996
// The model itself runs on the GPU through libsipnet_amd.so; there is no CPU model here.
//
// Additive extension (never changes single-run behaviour):
//   --devices LIST           HIP devices the ensemble shards across (0-7, 0,2,3; default 0): member
//                            rows are split into contiguous ranges, one host thread + one batch
//                            per device, every shard writes its own members' files; with --sites:
//                            the sites of a flag set in contiguous ranges, one batch per device
//   --math strict|fast|auto  step-kernel arithmetic: strict = the reference's operation order (the
//                            default for a single run), fast = the throughput kernels (the default
//                            with --ensemble-params)
//   --ensemble-params FILE   whitespace table, first line = parameter names, one row per
//                            member overriding those parameters; every member runs in ONE
//                            batch and writes <prefix>.<m>.out (m = 0..M-1); restart paths
//                            get the same .<m> suffix; the members' text files are written
//                            by a pool of host threads
//   --ensemble-stats FILE    (with --ensemble-params) the ensemble's per-step statistics instead of
//                            the members' files: the members shard over --devices as ONE sipnet_node
//                            (one RCCL rank per device), every device runs its members on the
//                            throughput kernels, ONE all-gather of the statistics block joins them,
//                            and FILE gets `year day time n mean/sd of NEE, GPP, ET` per step
//   --ensemble-out FILE      (with --ensemble-params or --sites) every member's outputs as ONE NetCDF-3 block
//                            (include/sipnet_amd.h "ensemble output block": dimensions time x member, the `.out`
//                            columns' names and units) INSTEAD of the members' text files: nee, gpp and
//                            evapotranspiration by default -- the lean throughput kernels, three planes -- or the
//                            `.out` columns named with --ensemble-out-columns a,b,c|all (the 44-column record);
//                            --ensemble-out-f32 stores floats; --ensemble-text writes the text files as well;
//                            --ensemble-out-sums K (the three planes only): every member's SUMS over groups of K steps
//                            instead of the steps (K = 48: daily NEE / GPP / ET of a half-hourly forcing; the block's
//                            time axis holds each group's first record, its step length the group's) -- summed inside
//                            the step kernel's launch where the batch has such a kernel (sipnet_batch_run_sums), else
//                            from the planes on the host;
//                            --ensemble-out-segment N holds N steps of the record on the device at a time (default:
//                            about 3 GB worth -- the whole record of 10 240 members x a year would be 63 GB).
//                            Device shards stream their member ranges into the one file.  With --sites one block
//                            per distinct forcing: FILE itself when there is one, else <stem>.<k><ext> with k = the
//                            position in the list of the site's first run; member = position in the list, the global
//                            attribute run_dirs names the directories
//   --bounded-waits          (throughput kernels) the cooperative kernels' build whose hand-over waits have a budget of polls:
//                            a wait that never ends is reported (SIPNET_ERR_INTERNAL, exit 7, naming the wait and step)
//                            instead of hanging the GPU -- ~10 % slower, same bits; for boxes where a hang costs the machine
//   --sites FILE             stacking at the process boundary PEcAn uses: FILE lists run directories (one per
//                            line, `#` comments), each with its own sipnet.in / <prefix>.param / <prefix>.clim /
//                            <events>.in.  Every directory is resolved exactly like a run started inside it (the
//                            options of THIS command line take precedence over each sipnet.in, cli.c:144-229), runs
//                            whose forcing (climate + events) is identical become members of one site, runs with the
//                            same model flags share ONE batch (whatever their lengths), and every directory gets the files its
//                            own run would have written (<prefix>.out, <events>.out, <prefix>.config, single-variable
//                            outputs) -- byte for byte with --math auto / strict (the strict-order kernel), to the last
//                            printed digit with --math fast (the throughput kernels).  RESTART_IN / RESTART_OUT of a
//                            directory's sipnet.in are honoured (PEcAn's assimilation cycles: one directory per member
//                            and cycle, sipnet.c:1963-1989, restart.c:932-996): runs share a site only when their
//                            checkpoints agree in what the site plan owns (year-to-date GDD, year counters, tillage
//                            modifier, ring layout, processed steps), every member resumes from its own checkpoint
//                            and is checkpointed at the end of ITS forcing
//
// Parts (one translation unit; this file includes them in this order):
//   cli_support.h    logging, fatal conditions on host threads, return codes, paths, --devices, the memory and batch holders
//   cli_context.h    the configuration (context.c): defaults, sipnet.in, --dump-config, flag-coupling rules, usage
//   cli_block.h      the ensemble output block: its columns, its creation, device results into it
//   cli_inputs.h     one directory resolved into a run, restart checkpoints, the --ensemble-params table, batch set-up
//   cli_outputs.h    the report of members that did not run; one member's files
//   cli_ensemble.h   --ensemble-stats through the node object; the ensemble sharded over devices, four shard modes
//   cli_sites.h      --sites: directories into batches and sites, one batch's run, every directory's files
#include <getopt.h>
#include <unistd.h>
#include <cmath>
#include <sched.h>
#include <strings.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sipnet_amd.h"

namespace {

#include "cli_support.h"
#include "cli_context.h"
#include "cli_block.h"
#include "cli_inputs.h"
#include "cli_outputs.h"
#include "cli_ensemble.h"
#include "cli_sites.h"

}  // namespace

int main(int argc, char** argv) {
  Context ctx;
  initContext(ctx);

  // ---- command line (cli.c:144-229) ----
  std::vector<option> opts;
  static int tmpFlag = 0;
  for (int k = 0; k < kNumFlagOpts; k++) {
    opts.push_back({kFlagOpts[k][0], no_argument, &tmpFlag, 1});
    opts.push_back({strdup((std::string("no-") + kFlagOpts[k][0]).c_str()), no_argument, &tmpFlag, 0});
  }
  enum { OPT_RIN = 1001, OPT_ROUT, OPT_DBG, OPT_ENS, OPT_DEV, OPT_MATH, OPT_ESTATS, OPT_SITES, OPT_EOUT, OPT_ECOLS, OPT_EF32, OPT_ETEXT, OPT_BOUNDED, OPT_ESEG, OPT_ESUMS };
  opts.push_back({"input-file", required_argument, nullptr, 'i'});
  opts.push_back({"file-prefix", required_argument, nullptr, 'f'});
  opts.push_back({"file-name", required_argument, nullptr, 'f'});
  opts.push_back({"events-prefix", required_argument, nullptr, 'e'});
  opts.push_back({"restart-in", required_argument, nullptr, OPT_RIN});
  opts.push_back({"restart-out", required_argument, nullptr, OPT_ROUT});
  opts.push_back({"debug-log", required_argument, nullptr, OPT_DBG});
  opts.push_back({"ensemble-params", required_argument, nullptr, OPT_ENS});
  opts.push_back({"devices", required_argument, nullptr, OPT_DEV});
  opts.push_back({"math", required_argument, nullptr, OPT_MATH});
  opts.push_back({"ensemble-stats", required_argument, nullptr, OPT_ESTATS});
  opts.push_back({"sites", required_argument, nullptr, OPT_SITES});
  opts.push_back({"ensemble-out", required_argument, nullptr, OPT_EOUT});
  opts.push_back({"ensemble-out-columns", required_argument, nullptr, OPT_ECOLS});
  opts.push_back({"ensemble-out-f32", no_argument, nullptr, OPT_EF32});
  opts.push_back({"ensemble-text", no_argument, nullptr, OPT_ETEXT});
  opts.push_back({"bounded-waits", no_argument, nullptr, OPT_BOUNDED});
  opts.push_back({"ensemble-out-segment", required_argument, nullptr, OPT_ESEG});
  opts.push_back({"ensemble-out-sums", required_argument, nullptr, OPT_ESUMS});
  opts.push_back({"help", no_argument, nullptr, 'h'});
  opts.push_back({"version", no_argument, nullptr, 'v'});
  opts.push_back({nullptr, 0, nullptr, 0});
  std::string ensembleStats, sitesFile, blockColumns, devicesArg = "0";
  Ensemble ens;
  ens.mathArg = "auto";
  BlockSpec& block = ens.block;
  int longIndex = 0, ch;
  while ((ch = getopt_long(argc, argv, "he:f:i:v", opts.data(), &longIndex)) != -1) {
    switch (ch) {
      case 0: ctx.setInt(kFlagOpts[longIndex / 2][1], tmpFlag, SRC_CLI); break;
      case 'f': ctx.setStr("filePrefix", optarg, SRC_CLI); break;
      case 'e': ctx.setStr("eventsPrefix", optarg, SRC_CLI); break;
      case 'i': ctx.setStr("inputFile", optarg, SRC_CLI); break;
      case OPT_RIN: ctx.setStr("restartIn", optarg, SRC_CLI); break;
      case OPT_ROUT: ctx.setStr("restartOut", optarg, SRC_CLI); break;
      case OPT_DBG: ctx.setStr("debugLogPrefix", optarg, SRC_CLI); break;
      case OPT_ENS: ens.table = optarg; break;
      case OPT_DEV: devicesArg = optarg; break;
      case OPT_MATH: ens.mathArg = optarg; break;
      case OPT_ESTATS: ensembleStats = optarg; break;
      case OPT_SITES: sitesFile = optarg; break;
      case OPT_EOUT: block.path = optarg; break;
      case OPT_ECOLS: blockColumns = optarg; break;
      case OPT_EF32: block.f32 = true; break;
      case OPT_ETEXT: block.text = true; break;
      case OPT_BOUNDED: g_kernelOptions |= SIPNET_KOPT_BOUNDED_WAITS; break;
      case OPT_ESEG: block.segment = atoi(optarg); break;
      case OPT_ESUMS: block.sums = atoi(optarg); if (block.sums <= 0) die(8, "--ensemble-out-sums needs a positive number of steps\n"); break;
      case 'h': usage(argv[0]); return 0;
      case 'v': printf("SIPNET version 2.1.0 (%s)\n", sipnet_version()); return 0;
      default: usage(argv[0]); return 8;  // EXIT_CODE_BAD_CLI_ARGUMENT
    }
  }
  ens.devices = parseDevices(devicesArg);  // syntax errors are CLI errors (exit 8)
  if (ens.mathArg != "auto" && ens.mathArg != "strict" && ens.mathArg != "fast") {
    logError("--math takes strict, fast or auto\n");
    return 8;
  }
  if (!ensembleStats.empty() && ens.table.empty()) {
    logError("--ensemble-stats needs --ensemble-params\n");
    return 8;
  }
  if (block.on() ? (ens.table.empty() && sitesFile.empty()) || !ensembleStats.empty()
                 : (!blockColumns.empty() || block.f32 || block.text)) {
    logError("--ensemble-out needs --ensemble-params or --sites (not --ensemble-stats); "
             "--ensemble-out-columns / -f32 / --ensemble-text need --ensemble-out\n");
    return 8;
  }
  if (!blockColumns.empty()) parseBlockColumns(block, blockColumns);
  if (block.sums > 0 && (!block.on() || !block.planesOnly() || block.text || !sitesFile.empty())) {
    logError("--ensemble-out-sums sums the three planes of --ensemble-params ... --ensemble-out (no --ensemble-out-columns, "
             "--ensemble-text or --sites)\n");
    return 8;
  }
  g_quiet = ctx.i("quiet") != 0;
  if (!sitesFile.empty()) {
    if (!ens.table.empty() || !ensembleStats.empty()) {
      logError("--sites does not combine with --ensemble-params / --ensemble-stats\n");
      return 8;
    }
    return runSites(ctx, sitesFile, ens.mathArg, ens.devices, block);
  }
  ens.run.ctx = ctx;
  loadEnsemble(ens);
  return ensembleStats.empty() ? runEnsemble(ens) : runEnsembleStats(ens, ensembleStats);
}
