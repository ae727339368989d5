// cli_block.h -- part of sipnet_cli.cpp: the ensemble output block (--ensemble-out), its creation and the way a device
// result gets into it.
#pragma once

struct BlockSpec {
  std::string path;                // empty: no block
  std::vector<int> cols;           // `.out` column indices (sipnet_io_out_column); empty: the three planes
  bool f32 = false, text = false;  // store floats; write the members' text files as well
  int segment = 0;                 // --ensemble-out-segment: steps of the record held on the device at a time (0: ~3 GB worth)
  int sums = 0;                    // --ensemble-out-sums K: sums over groups of K steps instead of the steps (planes only)
  bool on() const { return !path.empty(); }
  bool planesOnly() const { return cols.empty(); }
};
void parseBlockColumns(BlockSpec& spec, const std::string& arg) {
  if (arg == "all") {
    for (int k = 0; k < sipnet_io_out_column_count(); k++) spec.cols.push_back(k);
    return;
  }
  std::istringstream in(arg);
  for (std::string tok; std::getline(in, tok, ',');) {
    if (tok.empty()) continue;
    const int k = sipnet_io_out_column_index(tok.c_str());
    if (k < 0) die(8, "--ensemble-out-columns: unknown .out column " + tok + "\n");
    spec.cols.push_back(k);
  }
  if (spec.cols.empty()) die(8, "--ensemble-out-columns: no columns\n");
}
sipnet_ensemble_file* createBlock(const BlockSpec& spec, const std::string& path, int T, int M, const sipnet_clim_table* clim,
                                  const int32_t* memberIds, const std::string& attrs) {
  std::vector<const char*> names;
  if (spec.planesOnly()) {
    names = {"nee", "gpp", "evapotranspiration"};
  } else {
    for (int k : spec.cols) {
      const char* nm = nullptr;
      check(sipnet_io_out_column(k, &nm, nullptr, nullptr, nullptr), "column table");
      names.push_back(nm);
    }
  }
  sipnet_ensemble_file* f = nullptr;
  check(sipnet_io_ensemble_create(path.c_str(), T, M, sipnet_clim_year(clim), sipnet_clim_day(clim), sipnet_clim_data(clim),
                                  memberIds, (int32_t)names.size(), names.data(), nullptr, spec.f32 ? SIPNET_NC_F32 : SIPNET_NC_F64,
                                  attrs.c_str(), &f), "creating the ensemble block");
  return f;
}
// --ensemble-out-sums K: the block's rows are the groups of K steps -- each group's first record on the time axis, its step
// length the group's
sipnet_ensemble_file* createSumsBlock(const BlockSpec& spec, int T, int M, const sipnet_clim_table* clim, const std::string& attrs) {
  const int nGroups = (T + spec.sums - 1) / spec.sums;
  std::vector<int32_t> gy(nGroups), gd(nGroups);
  std::vector<double> gc((size_t)nGroups * SIPNET_NCLIM);
  const double* cd = sipnet_clim_data(clim);
  for (int g = 0; g < nGroups; g++) {
    const int t0 = g * spec.sums, t1 = std::min(T, t0 + spec.sums);
    gy[g] = sipnet_clim_year(clim)[t0];
    gd[g] = sipnet_clim_day(clim)[t0];
    memcpy(&gc[(size_t)g * SIPNET_NCLIM], cd + (size_t)t0 * SIPNET_NCLIM, SIPNET_NCLIM * sizeof(double));
    double len = 0.0;
    for (int t = t0; t < t1; t++) len += cd[(size_t)t * SIPNET_NCLIM];
    gc[(size_t)g * SIPNET_NCLIM] = len;
  }
  const char* names[3] = {"nee", "gpp", "evapotranspiration"};
  sipnet_ensemble_file* f = nullptr;
  check(sipnet_io_ensemble_create(spec.path.c_str(), nGroups, M, gy.data(), gd.data(), gc.data(), nullptr, 3, names, nullptr,
                                  spec.f32 ? SIPNET_NC_F32 : SIPNET_NC_F64, attrs.c_str(), &f), "creating the ensemble block");
  return f;
}
// the block's variables as columns of the 44-column record: beside text files or checkpoints a block of the three planes
// comes from the record too, where they are the columns nee, gpp and evapotranspiration
BlockSpec recordColumns(const BlockSpec& spec) {
  BlockSpec asCols = spec;
  if (spec.planesOnly())
    asCols.cols = {sipnet_io_out_column_index("nee"), sipnet_io_out_column_index("gpp"), sipnet_io_out_column_index("evapotranspiration")};
  return asCols;
}
// members [col0, col0 + n) of a device result -> members [member0, member0 + n) of the block, one variable at a time
// (a dense [T][n] host array per variable: nothing the size of the record ever exists on the host).
// planes: dPlanes[3][Tld][ld] (NEE, GPP, ET); records: dRec[Tld][SIPNET_NREC][ld].
// (step0: the file rows the device arrays' T rows go to -- a run cut into segments fills the block segment by segment)
void putBlock(sipnet_ensemble_file* f, const BlockSpec& spec, int T, int64_t ld, int64_t Tld, int64_t col0, int n, int member0,
              const double* dPlanes, const double* dRec, int step0 = 0) {
  std::vector<double> host((size_t)T * n), second;
  const size_t w = (size_t)n * sizeof(double), dense = (size_t)T * w;
  double tFetch = 0.0, tPut = 0.0;
  // a column of the device result is T pieces of n doubles, ld (planes) or SIPNET_NREC x ld (records) doubles apart: gathered
  // into a dense device array first (a device-side copy), then ONE dense copy to the host -- row pieces straight over
  // PCIe took 3 s per column of 10 240 members x 17 520 steps, this takes 0.15 s
  const bool strided = spec.planesOnly() ? ld != n : true;
  const DevMem gathered(strided ? (size_t)T * n : 0);
  double* dDense = gathered.p;
  auto fetch = [&](std::vector<double>& dst, const double* src, size_t pitch) {
    const double t0 = nowSeconds();
    if (!strided) {
      check(sipnet_dev_to_host(dst.data(), src, dense, nullptr), "copy back");
    } else {
      check(sipnet_dev_to_dev_2d(dDense, w, src, pitch, w, (size_t)T, nullptr), "gathering a column");
      check(sipnet_dev_to_host(dst.data(), dDense, dense, nullptr), "copy back");
    }
    tFetch += nowSeconds() - t0;
  };
  auto put = [&](int v) {
    const double t0 = nowSeconds();
    check(sipnet_io_ensemble_put(f, v, step0, T, member0, n, host.data(), n, 0), "writing the ensemble block");
    tPut += nowSeconds() - t0;
  };
  if (spec.planesOnly()) {
    for (int v = 0; v < 3; v++) {
      fetch(host, dPlanes + ((size_t)v * Tld) * ld + col0, (size_t)ld * sizeof(double));
      put(v);
    }
  } else {
    const size_t pitch = (size_t)SIPNET_NREC * ld * sizeof(double);
    for (size_t v = 0; v < spec.cols.size(); v++) {
      int32_t r0 = 0, r1 = -1;
      check(sipnet_io_out_column(spec.cols[v], nullptr, &r0, &r1, nullptr), "column table");
      fetch(host, dRec + (size_t)r0 * ld + col0, pitch);
      if (r1 >= 0) {   // total wood = plantWoodC + accounting delta (state.c:17-19)
        second.resize(host.size());
        fetch(second, dRec + (size_t)r1 * ld + col0, pitch);
        for (size_t i = 0; i < host.size(); i++) host[i] += second[i];
      }
      put((int)v);
    }
  }
  char msg[200];
  snprintf(msg, sizeof msg, "ensemble block: members %d..%d, steps %d..%d, %zu variable(s): device -> host %.2f s, conversion + file %.2f s\n",
           member0, member0 + n - 1, step0, step0 + T - 1, spec.planesOnly() ? (size_t)3 : spec.cols.size(), tFetch, tPut);
  logInfo(msg);
}
