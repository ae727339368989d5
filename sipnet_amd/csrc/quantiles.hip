// quantiles.hip -- order statistics of a [rows][ld] series per (row, site): sipnet_batch_plane_quantiles and, under per-member
// log-weights, sipnet_batch_plane_quantiles_weighted, with the host-only sipnet_quantile_positions, sipnet_wquantile_target and
// the two capacities and path rules.  The contract is in include/sipnet_amd.h.  This file: the host side, the checks and the
// launch of both calls once.  The kernels: quantiles_core.h (keys, cells, block sums, the sort network, the radix select),
// quantiles_plain.h, quantiles_weighted.h (with the filter's fixed-point weight of pf_weights.inc).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>

#include "batch_impl.h"
#include "site_host.h"

namespace {

#include "site_device.h"
#include "quantiles_core.h"
#include "quantiles_plain.h"
#include "pf_weights.inc"
#include "quantiles_weighted.h"

// n_q and the q of a call: 0, or the refusal
int checkQ(const char* name, int32_t n_q, const double* q) {
  if (!q) return refuse(name, "a NULL q");
  if (n_q < 1 || n_q > kQMax) return refuse(name, "n_q must be 1..16");
  for (int i = 0; i < n_q; i++)
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return refuse(name, "q[" + std::to_string(i) + "] is not a number in [0, 1]");
  return 0;
}

// the path a call with this M and path argument runs under a sort capacity of cap members: 1 sort, 2 selection, -1 refused
int32_t pathOf(int32_t n_members, int32_t path, int32_t cap) {
  if (n_members < 1 || path < 0 || path > 2 || (path == 1 && n_members > cap)) return -1;
  return path == 1 || (path == 0 && n_members <= cap) ? 1 : 2;
}

// one call's arguments that both calls have, and what differs between the two on the host: the sort path's capacity, the
// function that tells it, its LDS per element
struct QuantCall {
  const char* name;
  int32_t cap;
  const char* capName;
  size_t ldsPer;
  sipnet_batch* b;
  const void* d_series;
  int32_t rows;
  int64_t ld;
  int32_t n_q;
  const double* q;
  int32_t live_only, path;
  double* d_quant;
  const double* d_obs;
  double* d_crps;
  const void* d_rank;
};

// The refusals both calls share, in three steps (the weighted call has one of its own behind each of the first two): 0, or the
// refusal.  The last makes the batch's device current and tells whether the sort path runs.
int checkPointers(const QuantCall& k) {
  return !k.b || !k.d_series || !k.d_quant ? refuse(k.name, "a NULL batch, series or d_quant") : 0;
}
int checkShape(const QuantCall& k) {
  const int rc = checkQ(k.name, k.n_q, k.q);
  if (rc) return rc;
  return k.rows < 1 || k.ld < k.b->ncol ? refuse(k.name, "needs rows >= 1 and ld >= ncol") : 0;
}
int checkPath(const QuantCall& k, bool* sort) {
  const char* name = k.name;
  if ((k.d_crps || k.d_rank) && !k.d_obs) return refuse(name, "d_crps and d_rank need d_obs");
  if (k.path < 0 || k.path > 2) return refuse(name, "path must be 0 (auto), 1 (sort) or 2 (selection)");
  const int32_t M = k.b->n_members;
  const std::string cap = std::to_string(k.cap);
  if (k.path == 1 && M > k.cap) return refuse(name, "the sort path holds at most " + cap + " members (" + k.capName + ")");
  *sort = pathOf(M, k.path, k.cap) == 1;
  if (k.d_crps && !*sort)
    return refuse(name, "the CRPS needs the sorted sample: the sort path only (at most " + cap + " members, path 0 or 1)");
  if (k.live_only && k.b->planDirty) return refuse(name, "live_only needs a batch that was set up (sipnet_batch_setup)");
  return useDevice(k.b);
}

// the common arguments into a (the caller has set its own), and one of the two kernels over the cells
template <class A>
int launchCells(const QuantCall& k, bool sort, void (*sortKernel)(A, int), void (*selectKernel)(A), A a, hipStream_t stream) {
  sipnet_batch* b = k.b;
  const int32_t M = b->n_members;
  a.series = k.d_series;
  a.ld = k.ld;
  a.nSites = b->n_sites;
  a.cells = (int64_t)k.rows * b->n_sites;
  a.M = M;
  a.nq = k.n_q;
  for (int i = 0; i < k.n_q; i++) a.q[i] = k.q[i];
  a.quant = k.d_quant;
  a.obs = k.d_obs;
  a.crps = k.d_crps;
  // a workgroup per cell: rows of at most 2^20 workgroups (a grid's x dimension times the 256 threads must stay below 2^32)
  const unsigned gx = (unsigned)std::min<int64_t>(a.cells, (int64_t)1 << 20);
  const dim3 grid(gx, (unsigned)((a.cells + gx - 1) / gx));
  if (sort) {
    int P = 256;
    while (P < M) P <<= 1;
    const size_t ldsBytes = (size_t)P * k.ldsPer;
    if (ldsBytes > 32 * 1024)   // (beside its static LDS, past what a kernel may use unasked)
      HIP_TRY(hipFuncSetAttribute((const void*)sortKernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes));
    hipLaunchKernelGGL(sortKernel, grid, dim3(256), ldsBytes, stream, a, P);
  } else {
    hipLaunchKernelGGL(selectKernel, grid, dim3(256), 0, stream, a);
  }
  HIP_TRY(hipGetLastError());
  b->pfInfo.fused = sort ? 1 : 0;   // (what sipnet_batch_pf_info reports of the last such call: which path ran)
  b->pfInfo.grid = (int32_t)std::min<int64_t>(a.cells, INT32_MAX);
  return SIPNET_OK;
}

}  // namespace

extern "C" {

int32_t sipnet_quantile_lds_members(int32_t elem_is_f32) {
  (void)elem_is_f32;   // (floats are widened to 64-bit keys as well: one capacity)
  return kSortCap;
}

int32_t sipnet_quantile_path(int32_t n_members, int32_t elem_is_f32, int32_t path) {
  return pathOf(n_members, path, sipnet_quantile_lds_members(elem_is_f32));
}

int sipnet_quantile_positions(int32_t n, int32_t n_q, const double* q, int32_t* lo, double* g) {
  const char* name = "sipnet_quantile_positions";
  if (!lo || !g) return refuse(name, "a NULL lo or g");
  int rc = checkQ(name, n_q, q);
  if (rc) return rc;
  if (n < 1) return refuse(name, "n must be >= 1");
  for (int i = 0; i < n_q; i++) positionOf(n, q[i], &lo[i], &g[i]);
  return SIPNET_OK;
}

int sipnet_batch_plane_quantiles(sipnet_batch* b, const void* d_series, int32_t elem_is_f32, int32_t rows, int64_t ld, int32_t n_q,
                                 const double* q, int32_t live_only, int32_t path, double* d_quant, int32_t* d_count,
                                 const double* d_obs, double* d_crps, int32_t* d_rank, void* hip_stream) {
  const QuantCall k{"sipnet_batch_plane_quantiles", kSortCap, "sipnet_quantile_lds_members", sizeof(uint64_t), b, d_series, rows, ld,
                    n_q, q, live_only, path, d_quant, d_obs, d_crps, d_rank};
  bool sort = false;
  int rc = checkPointers(k);
  if (!rc) rc = checkShape(k);
  if (!rc) rc = checkPath(k, &sort);
  if (rc) return rc;
  const hipStream_t stream = (hipStream_t)hip_stream;
  if (live_only) {   // (the status row is the batch's: behind whatever of the batch is writing it)
    rc = orderBehindBusy(b, stream);
    if (rc) return rc;
  }
  PlainArgs a{};
  a.status = live_only ? b->d_state + (size_t)ST_status * b->ncol : nullptr;
  a.siteStatus = b->d_siteStatus;
  a.count = d_count;
  a.rank = d_rank;
  rc = launchCells(k, sort, elem_is_f32 ? quantSortKernel<float> : quantSortKernel<double>,
                   elem_is_f32 ? quantSelectKernel<float> : quantSelectKernel<double>, a, stream);
  return rc || !live_only ? rc : markBusy(b, stream);
}

int64_t sipnet_wquantile_target(int64_t S, double q) {
  if (S < 1 || S > ((int64_t)1 << 52) || !(q >= 0.0 && q <= 1.0)) return -1;
  return wTargetOf(S, q);
}

int32_t sipnet_wquantile_lds_members(int32_t elem_is_f32) {
  (void)elem_is_f32;   // (floats are widened to 64-bit keys as well: one capacity)
  return kWSortCap;
}

int32_t sipnet_wquantile_path(int32_t n_members, int32_t elem_is_f32, int32_t path) {
  return pathOf(n_members, path, sipnet_wquantile_lds_members(elem_is_f32));
}

int sipnet_batch_plane_quantiles_weighted(sipnet_batch* b, const void* d_series, int32_t elem_is_f32, int32_t rows, int64_t ld,
                                          const double* d_logw, int32_t n_q, const double* q, int32_t live_only, int32_t path,
                                          double* d_quant, int64_t* d_site_weight, int64_t* d_fixed_weights, double* d_moments,
                                          const double* d_obs, double* d_crps, int64_t* d_rank, void* hip_stream) {
  const QuantCall k{"sipnet_batch_plane_quantiles_weighted", kWSortCap, "sipnet_wquantile_lds_members",
                    sizeof(uint64_t) + sizeof(uint32_t), b, d_series, rows, ld, n_q, q, live_only, path, d_quant, d_obs, d_crps, d_rank};
  const char* name = k.name;
  bool sort = false;
  int rc = checkPointers(k);
  if (rc) return rc;
  if (!d_logw) return refuse(name, "a NULL d_logw");
  rc = checkShape(k);
  if (rc) return rc;
  if (tooManyColumns(b)) return refuse(name, "more than 4194304 columns (the total weight must stay exact in a double)");
  rc = checkPath(k, &sort);
  if (rc) return rc;
  const hipStream_t stream = (hipStream_t)hip_stream;
  // (the status row and the scratch are the batch's: behind whatever of the batch is writing or reading them)
  rc = orderBehindBusy(b, stream);
  if (rc) return rc;
  WSiteArgs sa{};
  rc = carveScratch(b, b->d_wquant, [&](Carver& c) {
    sa.site = c.take<int64_t>((size_t)3 * b->n_sites);
    sa.w = c.take<int32_t>((size_t)b->ncol);
  });
  if (rc) return rc;
  sa.logw = d_logw;
  sa.status = live_only ? b->d_state + (size_t)ST_status * b->ncol : nullptr;
  sa.siteStatus = b->d_siteStatus;
  sa.M = b->n_members;
  sa.siteOut = d_site_weight;
  sa.fixedOut = d_fixed_weights;
  hipLaunchKernelGGL(wquantSiteKernel, dim3((unsigned)b->n_sites), dim3(256), 0, stream, sa);
  HIP_TRY(hipGetLastError());
  WQuantArgs a{};
  a.w = sa.w;
  a.site = sa.site;
  a.moments = d_moments;
  a.rank = d_rank;
  rc = launchCells(k, sort, elem_is_f32 ? wquantSortKernel<float> : wquantSortKernel<double>,
                   elem_is_f32 ? wquantSelectKernel<float> : wquantSelectKernel<double>, a, stream);
  return rc ? rc : markBusy(b, stream);   // (the scratch is in use until these launches are done)
}

}  // extern "C"
