// cli_support.h -- part of sipnet_cli.cpp: logging, fatal conditions on host threads, the C-ABI's return codes, time, paths,
// the --devices list, and the two holders that give device memory and a batch back.
#pragma once

bool g_quiet = false;
int32_t g_kernelOptions = 0;   // SIPNET_KOPT_* for every batch this process creates (--bounded-waits)
void logInfo(const std::string& s) { if (!g_quiet) printf("[INFO   ] %s", s.c_str()); }
void logError(const std::string& s) { printf("[ERROR  ] %s", s.c_str()); }
void logWarning(const std::string& s) { printf("[WARNING] %s", s.c_str()); }

// A fatal condition ends the process with the reference's exit code -- from the main thread.  Host threads (device
// shards, file writers) must not call exit() while other threads hold batches: they throw, the first error is kept, and
// the main thread reports it after the joins.
struct Fatal {
  int code;
  std::string msg;
};
thread_local bool t_worker = false;
[[noreturn]] void die(int code, const std::string& msg) {
  if (t_worker) throw Fatal{code, msg};
  logError(msg);
  exit(code);
}
struct FirstFatal {
  std::mutex mu;
  bool set = false;
  Fatal f{0, ""};
  void take(const Fatal& x) {
    std::lock_guard<std::mutex> lock(mu);
    if (!set) {
      set = true;
      f = x;
    }
  }
  void exitIfSet() {   // main thread, after the joins
    if (set) {
      logError(f.msg);
      exit(f.code);
    }
  }
};
template <class F>
void guarded(FirstFatal& sink, F&& fn) {   // body of a host thread
  t_worker = true;
  try {
    fn();
  } catch (const Fatal& f) {
    sink.take(f);
  }
}
// run `fn` on n host threads (inline when n == 1); a fatal condition in any of them ends the process afterwards
template <class F>
void runThreads(int n, F&& fn) {
  if (n <= 1) {
    fn();
    return;
  }
  FirstFatal sink;
  std::vector<std::thread> pool;
  for (int i = 0; i < n; i++) pool.emplace_back([&]() { guarded(sink, fn); });
  for (auto& th : pool) th.join();
  if (sink.set) die(sink.f.code, sink.f.msg);   // (rethrown when this is itself a worker thread)
}
// the main thread's device shards: fn(0) inline when there is one, else fn(k) on a host thread each; the first fatal
// condition ends the process after the joins
template <class F>
void runShards(int n, F&& fn) {
  if (n == 1) {
    fn(0);
    return;
  }
  FirstFatal sink;
  std::vector<std::thread> shards;
  for (int k = 0; k < n; k++) shards.emplace_back([&, k]() { guarded(sink, [&]() { fn(k); }); });
  for (auto& th : shards) th.join();
  sink.exitIfSet();
}
// the host threads this process may run on
int hostThreadCount() {
  cpu_set_t cpus;
  return sched_getaffinity(0, sizeof cpus, &cpus) == 0 ? CPU_COUNT(&cpus) : 1;
}

// a path named in a sipnet.in, seen from outside its directory
std::string joinPath(const std::string& dir, const std::string& p) {
  return (!p.empty() && p[0] == '/') ? p : dir + "/" + p;
}

double nowSeconds() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
void check(int rc, const char* what) {
  if (rc != SIPNET_OK) die(rc >= 100 ? 1 : rc, std::string(what) + ": " + sipnet_last_error() + "\n");
}

// "--devices 0-7", "0,2,3", "0,0" (two shards on one device): HIP device ordinals, one shard each
std::vector<int> parseDevices(const std::string& arg) {
  std::vector<int> out;
  std::istringstream in(arg);
  for (std::string tok; std::getline(in, tok, ',');) {
    if (tok.empty()) continue;
    const size_t dash = tok.find('-', 1);
    char* end = nullptr;
    const long a = strtol(tok.c_str(), &end, 10);
    long z = a;
    if (dash != std::string::npos) {
      if (end != tok.c_str() + dash) die(8, "bad --devices list: " + arg + "\n");
      z = strtol(tok.c_str() + dash + 1, &end, 10);
    }
    if (*end || a < 0 || z < a || z - a > 1023) die(8, "bad --devices list: " + arg + "\n");
    for (long d = a; d <= z; d++) out.push_back((int)d);
  }
  if (out.empty()) die(8, "bad --devices list: " + arg + "\n");
  return out;
}
// every listed device exists (the first device call of a run)
void checkDevices(const std::vector<int>& devices) {
  const int have = sipnet_device_count();
  for (int d : devices)
    if (d >= have)
      die(1, "--devices names device " + std::to_string(d) + " but only " + std::to_string(have) +
                 " HIP device(s) are visible (this engine has no CPU path)\n");
}

// doubles on the device (sipnet_dev_alloc), given back when the holder goes; none for zero elements
struct DevMem {
  double* p = nullptr;
  explicit DevMem(size_t elems) {
    if (elems && !(p = (double*)sipnet_dev_alloc(elems * sizeof(double)))) die(1, std::string(sipnet_last_error()) + "\n");
  }
  ~DevMem() { if (p) sipnet_dev_free(p); }
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
};
// a batch (sipnet_batch_create), destroyed when the holder goes
struct Batch {
  sipnet_batch* b = nullptr;
  Batch() = default;
  ~Batch() { if (b) sipnet_batch_destroy(b); }
  Batch(const Batch&) = delete;
  Batch& operator=(const Batch&) = delete;
};
