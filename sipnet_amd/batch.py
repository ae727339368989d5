"""Batch: an ensemble x site batch resident in HBM (sipnet_batch of the C-ABI).

Mirrors the reference call sequence of frontend.c:212-250 --
initModel / initEvents / setupModel / runModelOutput / cleanupModel -- for many
members and sites at once.  Outputs live in torch CUDA tensors that the caller
(or this class) allocates; the C-ABI only ever sees their raw device pointers.
"""
import collections
import ctypes as C
import weakref

import numpy as np

from ._lib import (F64, KERNEL_AUTO, LOGLIK_GAUSS, LOGLIK_LAPLACE, LOGLIK_MAX_TERMS, MCMC_INFO_WORDS, NDBG, NPARAMS, NREC, NSTATE, RING_SLOTS,
                   REJUVENATE_INFO_WORDS, TEMPER_INFO_WORDS, EnkfObs, EnkfParam, EnkfSeries, Event, LaunchInfo, LoglikTerm, PfInfo, PfPeer, Restart, c_array, check, lib, ptr)
from .config import pool_mask
from .enkf_local import EnkfLocalization


PlaneQuantiles = collections.namedtuple("PlaneQuantiles", "quant count crps rank path")

WeightedQuantiles = collections.namedtuple("WeightedQuantiles", "quant site_weight crps rank moments fixed path")

# the EnKF analyses' arguments in the groups their C signatures have: ops (n_obs, operators, analysed mask), planes (pointers,
# elements are floats, n_steps, ld), obs (obs, sd, inflation), info (d_site_info); held: what the pointers point into
EnkfArgs = collections.namedtuple("EnkfArgs", "ops planes obs info held")


def _dense(x, dtype, n=None):
    """x is a contiguous device tensor of dtype (and of n elements)"""
    return x.is_cuda and x.dtype == dtype and x.is_contiguous() and (n is None or x.numel() == n)


def quantile_lds_members(f32=False):
    """the largest member count per site that Batch.plane_quantiles' sort path takes (sipnet_quantile_lds_members)"""
    return int(lib().sipnet_quantile_lds_members(int(bool(f32))))


def quantile_positions(n, q):
    """where the type-7 quantiles q of n sorted values lie (sipnet_quantile_positions, host only): (lo int32 [n_q], g
    float64 [n_q]) -- Q = x[lo] when g == 0, else x[lo] + g (x[lo + 1] - x[lo]); the expressions the device uses"""
    qs = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)).reshape(-1))
    lo = np.zeros(qs.size, dtype=np.int32)
    g = np.zeros(qs.size)
    check(lib().sipnet_quantile_positions(int(n), int(qs.size), ptr(qs), ptr(lo), ptr(g)), "quantile_positions")
    return lo, g


def wquantile_lds_members(f32=False):
    """the largest member count per site that Batch.plane_quantiles_weighted's sort path takes (sipnet_wquantile_lds_members)"""
    return int(lib().sipnet_wquantile_lds_members(int(bool(f32))))


def wquantile_target(S, q):
    """the cumulative integer weight T = max(1, ceil(q S)) at which the weighted quantile q of a sample of total weight S is
    read (sipnet_wquantile_target, host only: the expression the device uses)"""
    T = int(lib().sipnet_wquantile_target(int(S), float(q)))
    if T < 0:
        raise ValueError("wquantile_target: S must be 1..2^52 and q a number in [0, 1]")
    return T


def philox4x32_10(ctr, key):
    """Philox4x32-10 (sipnet_philox4x32_10, host only): counter (4 x uint32), key (2 x uint32) -> uint32 [4]"""
    c = np.ascontiguousarray(np.asarray(ctr, dtype=np.uint32).reshape(4))
    k = np.ascontiguousarray(np.asarray(key, dtype=np.uint32).reshape(2))
    out = np.zeros(4, dtype=np.uint32)
    lib().sipnet_philox4x32_10(ptr(c), ptr(k), ptr(out))
    return out


def rejuvenate_normals(seed, draw, stream, member, block):
    """the four normals Batch.pf_rejuvenate gives one block of one member (sipnet_rejuvenate_normals, host only): listed
    parameter k takes normal k & 3 of block k >> 2, state slot p normal p & 3 of block 4 + (p >> 2); member: the column's
    index inside its site; stream: the site's stream -> float64 [4]"""
    z = np.zeros(4)
    lib().sipnet_rejuvenate_normals(int(seed) & (2 ** 64 - 1), int(draw) & 0xffffffff, int(stream) & 0xffffffff,
                                    int(member) & 0xffffffff, int(block) & 0xffffffff, ptr(z))
    return z


def liu_west_shrink(delta):
    """the shrink factor a = (3 delta - 1) / (2 delta) of Liu & West's discount delta in (1/3, 1] (0.95 .. 0.99 is usual);
    Batch.pf_rejuvenate's kernel then has h^2 = 1 - a^2"""
    return (3.0 * delta - 1.0) / (2.0 * delta)


def mcmc_draws(seed, draw, stream, member, n_other):
    """what Batch.mcmc_propose / mcmc_accept draw for one member (sipnet_mcmc_draws, host only): the ranks i1 != i2 of its two
    partners among the n_other >= 2 live members of the other half, in ascending member index, and the accept step's
    uniform u in (0, 1) -> (i1, i2, u)"""
    idx = np.zeros(2, dtype=np.int32)
    u = np.zeros(1)
    check(lib().sipnet_mcmc_draws(int(seed) & (2 ** 64 - 1), int(draw) & 0xffffffff, int(stream) & 0xffffffff,
                                  int(member) & 0xffffffff, int(n_other), ptr(idx), ptr(u)), "mcmc_draws")
    return int(idx[0]), int(idx[1]), float(u[0])


def demc_gamma(n_params):
    """ter Braak's (2006) scale of the differential-evolution proposal for n_params moved rows: 2.38 / sqrt(2 n_params)"""
    return 2.38 / np.sqrt(2.0 * n_params)


def loglik_term(series, obs, sd, kind=LOGLIK_GAUSS, scale=1.0, sum_steps=1):
    """one observed series of Batch.series_loglik: series [rows * sum_steps][ld] (a contiguous 2-D float32 / float64 device
    tensor: a plane of run(), an array of run_sums(), a smoothed series) against obs and sd [n_sites][rows] (array-likes,
    uploaded as float64, or float64 device tensors; obs NaN: a gap; sd: the Gaussian sigma or the Laplace scale b).  Row r
    is compared with scale * (the sum of series rows r * sum_steps .. (r + 1) * sum_steps - 1).  The batch checks the shapes."""
    if kind not in (LOGLIK_GAUSS, LOGLIK_LAPLACE):
        raise ValueError("loglik_term: kind must be LOGLIK_GAUSS or LOGLIK_LAPLACE")
    t = LoglikTerm(0, 0, 0, 0, int(sum_steps), int(kind), 0, float(scale))
    t.held = (series, obs, sd)
    return t


class Batch:
    def __init__(self, flags, n_sites, n_members, precision=F64, device=0, fast_math=None,
                 kernel=KERNEL_AUTO, kernel_options=0):
        """fast_math (fp64 batches): True = throughput kernels, False / None = strict reference
        order (the library default; no environment variable changes it).  kernel /
        kernel_options: sipnet_batch_set_kernel (KERNEL_* / KOPT_* of _lib)."""
        import torch  # device memory + streams only
        self._torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("sipnet_amd.Batch needs a HIP device (no CPU path exists)")
        self.L = lib()
        self.flags = list(flags)
        self.n_sites, self.n_members = int(n_sites), int(n_members)
        self.ncol = self.n_sites * self.n_members
        self.precision = precision
        self.device = torch.device("cuda", device)
        self.out_dtype = torch.float64 if precision == F64 else torch.float32
        h = C.c_void_p()
        fl = (C.c_int32 * 12)(*self.flags)
        check(self.L.sipnet_batch_create(fl, self.n_sites, self.n_members, precision,
                                         device, C.byref(h)), "batch_create")
        self.h = h
        self.n_steps = 0
        if fast_math is not None and precision == F64:
            self.set_math(fast_math)
        if kernel != KERNEL_AUTO or kernel_options:
            self.set_kernel(kernel, kernel_options)

    def set_math(self, fast):
        """sipnet_batch_set_math: arithmetic policy of an fp64 batch (strict order / throughput)"""
        check(self.L.sipnet_batch_set_math(self.h, 1 if fast else 0), "set_math")

    def set_kernel(self, kernel=KERNEL_AUTO, options=0):
        """sipnet_batch_set_kernel: force one step kernel (KERNEL_ONE_WAVE / COOP_LDS / COOP_HBM /
        STRICT) or go back to the shape-based choice (KERNEL_AUTO)."""
        check(self.L.sipnet_batch_set_kernel(self.h, int(kernel), int(options)), "set_kernel")

    def enable_diagnostics(self, on=True):
        """count the reference's per-step clamp / mass-balance warnings per member"""
        check(self.L.sipnet_batch_enable_diagnostics(self.h, int(on)), "enable_diagnostics")

    def get_diagnostics(self):
        """-> dict(n_clamp_warn[ncol], n_balance_warn[ncol], max_abs_dC[ncol], max_abs_dN[ncol])"""
        c = np.zeros(self.ncol, dtype=np.int64)
        w = np.zeros(self.ncol, dtype=np.int64)
        dc, dn = np.zeros(self.ncol), np.zeros(self.ncol)
        check(self.L.sipnet_batch_get_diagnostics(self.h, c.ctypes.data, w.ctypes.data, dc.ctypes.data,
                                                  dn.ctypes.data, self._stream()), "get_diagnostics")
        return dict(n_clamp_warn=c, n_balance_warn=w, max_abs_dC=dc, max_abs_dN=dn)

    def last_launch(self):
        """What the last run() launched: dict(kernel, grid, block_threads, waves_per_simd,
        lds_bytes, num_cus, plan_threads, plan_build_ms, plan_upload_ms)."""
        li = LaunchInfo()
        check(self.L.sipnet_batch_last_launch(self.h, C.byref(li)), "last_launch")
        return li.as_dict()

    # -- lifetime ---------------------------------------------------------------
    def close(self):
        for loc in list(getattr(self, "_localizations", ())):   # (a localization must go before its batch)
            loc.close()
        if getattr(self, "h", None):
            self.L.sipnet_batch_destroy(self.h)
            self.h = None
            # the batch-less sipnet_pf_* entry points (dist.pf_systematic_ancestors, pf_exchange_plan) keep device
            # scratch per host thread; nothing else frees it
            self.L.sipnet_pf_release_scratch()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    # -- inputs -----------------------------------------------------------------
    def set_climate(self, site, clim):
        check(self.L.sipnet_batch_set_climate(self.h, site, clim.n_steps, clim.data.ctypes.data,
                                              clim.year.ctypes.data, clim.day.ctypes.data),
              "set_climate")
        self.n_steps = int(self.L.sipnet_batch_nsteps(self.h))     # the longest site's (sites may differ in length)

    def set_climates(self, clims, first_site=0):
        """sipnet_batch_set_climate_sites: the forcings of sites first_site.. in one call (copied on the plan threads)"""
        n = len(clims)
        ns = (C.c_int32 * n)(*[c.n_steps for c in clims])
        cp = (C.c_void_p * n)(*[c.data.ctypes.data for c in clims])
        yp = (C.c_void_p * n)(*[c.year.ctypes.data for c in clims])
        dp = (C.c_void_p * n)(*[c.day.ctypes.data for c in clims])
        check(self.L.sipnet_batch_set_climate_sites(self.h, first_site, n, ns, cp, yp, dp), "set_climate_sites")
        self.n_steps = int(self.L.sipnet_batch_nsteps(self.h))

    def site_n_steps(self, site):
        """the number of records of this site's forcing (self.n_steps is the longest site's)"""
        return int(self.L.sipnet_batch_site_nsteps(self.h, site))

    def set_events(self, site, events):
        check(self.L.sipnet_batch_set_events(self.h, site, len(events), c_array(Event, events)), "set_events")

    def set_params(self, site, raw, first_member=0):
        """site: a site index, or None / ALL_SITES = the same members at every site (one upload)"""
        if site is None:
            site = -1   # SIPNET_ALL_SITES
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        if raw.ndim == 1:
            raw = np.broadcast_to(raw, (self.n_members, NPARAMS)).copy()
        assert raw.shape[1] == NPARAMS
        check(self.L.sipnet_batch_set_params(self.h, site, first_member, raw.shape[0],
                                             raw.ctypes.data), "set_params")

    def setup(self):
        """== setupModel() for every member (sipnet.c:1858-1951)."""
        check(self.L.sipnet_batch_setup(self.h, self._stream()), "setup")

    # -- run --------------------------------------------------------------------
    def alloc_outputs(self, n_steps, full=False):
        t = self._torch
        planes = t.empty((3, n_steps, self.ncol), dtype=self.out_dtype, device=self.device)
        return planes, self._rec(n_steps) if full else None

    def _rec(self, n_steps):
        return self._torch.empty((n_steps, NREC, self.ncol), dtype=self._torch.float64, device=self.device)

    def _steps(self, step0, n_steps):
        """n_steps None: from step0 to the end of the (longest) forcing"""
        return self.n_steps - step0 if n_steps is None else n_steps

    def _plane(self, plane):
        """the four plane arguments of a [rows][ld] tensor: pointer, elements are floats, rows, ld"""
        return ptr(plane), int(plane.dtype == self._torch.float32), plane.shape[0], plane.shape[1]

    def run(self, step0=0, n_steps=None, planes=None, rec=None, want_planes=True, full=False):
        """== the time loop of runModelOutput() (sipnet.c:1969-1982).

        Returns (planes, rec): planes[3][n_steps][ncol] = NEE, GPP, ET per step;
        rec[n_steps][36][ncol] full records when `full`."""
        n_steps = self._steps(step0, n_steps)
        if planes is None and want_planes:
            planes, _ = self.alloc_outputs(n_steps, False)
        if rec is None and full:
            rec = self._rec(n_steps)
        nee, gpp, et = (planes[0], planes[1], planes[2]) if planes is not None else (None, None, None)
        check(self.L.sipnet_batch_run(self.h, step0, n_steps, ptr(nee), ptr(gpp), ptr(et), ptr(rec), self.ncol,
                                      self._stream()), "run")
        return planes, rec

    def run_debug(self, step0=0, n_steps=None):
        """The same advance with the reference's `--debug-log` content (debug_log.c:285-312).

        Returns (rec[n_steps][NREC][ncol], dbg[n_steps][NDBG][ncol]) device tensors."""
        t = self._torch
        n_steps = self._steps(step0, n_steps)
        rec = self._rec(n_steps)
        dbg = t.empty((n_steps, NDBG, self.ncol), dtype=t.float64, device=self.device)
        check(self.L.sipnet_batch_run_debug(self.h, step0, n_steps, ptr(rec), ptr(dbg), self.ncol, self._stream()), "run_debug")
        return rec, dbg

    def run_stats(self, step0=0, n_steps=None, planes=None, stats=None):
        """run() + the ensemble statistics of the three planes from the same launch
        (sipnet_batch_run_stats): stats[3][n_steps][n_sites][2] = sum, sum of squares over each
        site's members.  planes: a [3][>= n_steps][ld >= ncol] device tensor of the batch's output
        dtype whose three planes are contiguous (a slice along the step axis is; the row pitch is
        ld, columns past ncol are neither read nor written).  Returns (planes, stats)."""
        t = self._torch
        n_steps = self._steps(step0, n_steps)
        if planes is None:
            planes, _ = self.alloc_outputs(n_steps, False)
        ok = (t.is_tensor(planes) and planes.is_cuda and planes.dim() == 3 and planes.shape[0] == 3
              and planes.dtype == self.out_dtype and planes.shape[1] >= n_steps and planes.shape[2] >= self.ncol)
        nee, gpp, et = (planes[0], planes[1], planes[2]) if ok else (None, None, None)
        if not ok or not (nee.is_contiguous() and gpp.is_contiguous() and et.is_contiguous()):
            raise ValueError(f"run_stats: planes must be a [3][>= {n_steps}][ld >= {self.ncol}] {self.out_dtype} device tensor "
                             "with contiguous planes")
        if stats is None:
            stats = t.empty((3, n_steps, self.n_sites, 2), dtype=t.float64, device=self.device)
        assert _dense(stats, t.float64)
        check(self.L.sipnet_batch_run_stats(self.h, step0, n_steps, ptr(nee), ptr(gpp), ptr(et), planes.shape[2], ptr(stats),
                                            self._stream()), "run_stats")
        return planes, stats

    def reduce_plane(self, plane, stats=None):
        """Per (row, site) ensemble sum and sum of squares of one plane: a contiguous 2-D float32 /
        float64 device tensor [rows][ld >= ncol] (the row pitch is ld; columns past ncol are not read)
        -> stats[rows][n_sites][2] (float64, on device)."""
        t = self._torch
        if (not t.is_tensor(plane) or not plane.is_cuda or plane.dim() != 2 or plane.dtype not in (t.float32, t.float64)
                or not plane.is_contiguous() or plane.shape[1] < self.ncol):
            raise ValueError(f"reduce_plane: plane must be a contiguous 2-D float32 / float64 device tensor [rows][ld >= {self.ncol}]")
        n_steps = plane.shape[0]
        if stats is None:
            stats = t.empty((n_steps, self.n_sites, 2), dtype=t.float64, device=self.device)
        elif not t.is_tensor(stats) or not _dense(stats, t.float64, n_steps * self.n_sites * 2):
            raise ValueError(f"reduce_plane: stats must be a contiguous float64 device tensor of {n_steps} x {self.n_sites} x 2")
        check(self.L.sipnet_batch_reduce_plane(self.h, *self._plane(plane), ptr(stats), self._stream()), "reduce_plane")
        return stats

    def _quantile_series(self, what, series):
        """the series of plane_quantiles and plane_quantiles_weighted, checked -> its plane arguments"""
        t = self._torch
        if (not t.is_tensor(series) or not series.is_cuda or series.dim() != 2 or series.dtype not in (t.float32, t.float64)
                or not series.is_contiguous() or series.shape[1] < self.ncol):
            raise ValueError(f"{what}: series must be a contiguous 2-D float32 / float64 device tensor [rows][ld >= {self.ncol}]")
        return self._plane(series)

    def _quantile_call(self, what, path_of, plane, q, obs, want_crps, want_rank, path):
        """what the two calls marshal alike behind the series; path_of: the library's path rule of the call -> (the q array,
        the path that will run (-1: the call refuses), obs on the device, want_crps, want_rank, the cells' shape)"""
        t = self._torch
        _, f32, rows, _ = plane
        qs = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)).reshape(-1))
        ran = int(path_of(self.n_members, f32, int(path)))      # (host only: the library's own rule)
        if want_crps is None:
            want_crps = obs is not None and ran == 1
        if want_rank is None:
            want_rank = obs is not None
        if obs is not None:
            obs = t.as_tensor(obs, dtype=t.float64).to(self.device).contiguous()
            if obs.numel() != rows * self.n_sites:
                raise ValueError(f"{what}: obs needs rows x n_sites = {rows * self.n_sites} values, got {obs.numel()}")
        return qs, ran, obs, want_crps, want_rank, (rows, self.n_sites)

    def plane_quantiles(self, series, q, live_only=True, obs=None, want_crps=None, want_rank=None, path=0, out=None):
        """Per (row, site) order statistics of a series over each site's members (sipnet_batch_plane_quantiles): the type-7
        quantiles q (numpy's "linear"), the sample size, and against obs[rows][n_sites] the rank histogram's counts
        {#(x < y), #(x == y)} and the CRPS.  series: a plane of run(), one of run_sums' arrays or a smoothed series -- any
        2-D contiguous float32 / float64 device tensor [rows][ld], ld >= ncol.  live_only: only the sites' live members
        (the batch must have been set up); else all members, and the batch need only exist.  want_crps / want_rank: None =
        whenever obs is given (the CRPS: and the sort path runs).  path: 0 auto, 1 the sort path (at most
        quantile_lds_members() members per site), 2 the selection path (any size, no CRPS).  out: a PlaneQuantiles (or a
        tuple quant, count, crps, rank) of an earlier call to write into.  -> PlaneQuantiles(quant[n_q][rows][n_sites] f64,
        count[rows][n_sites] i32, crps[rows][n_sites] f64 or None, rank[rows][n_sites][2] i32 or None, path: the one that
        ran), tensors on the device.  The batch is not changed."""
        t = self._torch
        what = "plane_quantiles"
        plane = self._quantile_series(what, series)
        qs, ran, obs, want_crps, want_rank, cells = self._quantile_call(what, self.L.sipnet_quantile_path, plane, q, obs, want_crps,
                                                                         want_rank, path)
        n_q = int(qs.size)
        parts = [None] * 4 if out is None else list(out)[:4]

        def part(k, wanted, shape, dtype, name):
            x = parts[k]
            if not wanted:
                return None
            if x is None:
                return t.empty(shape, dtype=dtype, device=self.device)
            if not _dense(x, dtype) or tuple(x.shape) != tuple(shape):
                raise ValueError(f"{what}: out's {name} must be a contiguous device tensor {tuple(shape)} of {dtype}")
            return x

        quant = part(0, True, (n_q,) + cells, t.float64, "quant")
        count = part(1, True, cells, t.int32, "count")
        crps = part(2, want_crps, cells, t.float64, "crps")
        rank = part(3, want_rank, cells + (2,), t.int32, "rank")
        check(self.L.sipnet_batch_plane_quantiles(self.h, *plane, n_q, ptr(qs), int(bool(live_only)), int(path), ptr(quant),
                                                  ptr(count), ptr(obs), ptr(crps), ptr(rank), self._stream()), what)
        return PlaneQuantiles(quant, count, crps, rank, ran)

    def plane_quantiles_weighted(self, series, logw, q, live_only=True, obs=None, want_crps=None, want_rank=None, want_moments=False,
                                 path=0, return_fixed=False):
        """plane_quantiles under per-member log-weights (sipnet_batch_plane_quantiles_weighted): per (row, site) the
        weighted quantiles q (the inverted weighted distribution function, not interpolated: type 1 at equal weights), the
        weighted mean and centred second moment, and against obs[rows][n_sites] the rank sums {sum of w over x < y, over
        x == y} and the weighted CRPS -- for the sites that keep their particles in the importance-sampling cycle.  logw:
        float64 device tensor [ncol] (series_loglik's out, pf_temper_sites' out; NaN and -inf weigh nothing); the weights are
        the filter's integers rint(2^30 exp(logw - the site's maximum)).  series, live_only, obs, want_crps / want_rank
        (None: whenever obs is given; the CRPS: and the sort path runs) and path as plane_quantiles, the sort path taking at
        most wquantile_lds_members() members per site.  -> WeightedQuantiles(quant[n_q][rows][n_sites] f64,
        site_weight[n_sites][3] i64 = {S, n, code}, crps[rows][n_sites] f64 or None, rank[rows][n_sites][2] i64 or None,
        moments[rows][n_sites][2] f64 or None, fixed[ncol] i64 or None (return_fixed: the integers the call used), path: the
        one that ran), tensors on the device.  The batch is not changed."""
        t = self._torch
        what = "plane_quantiles_weighted"
        plane = self._quantile_series(what, series)
        if not t.is_tensor(logw) or not _dense(logw, t.float64, self.ncol):
            raise ValueError(f"{what}: logw must be a contiguous float64 device tensor of {self.ncol} values")
        qs, ran, obs, want_crps, want_rank, cells = self._quantile_call(what, self.L.sipnet_wquantile_path, plane, q, obs, want_crps,
                                                                         want_rank, path)
        n_q = int(qs.size)

        def new(wanted, shape, dtype):
            return t.empty(shape, dtype=dtype, device=self.device) if wanted else None

        quant = new(True, (n_q,) + cells, t.float64)
        site_weight = new(True, (self.n_sites, 3), t.int64)
        fixed = new(return_fixed, (self.ncol,), t.int64)
        moments = new(want_moments, cells + (2,), t.float64)
        crps = new(want_crps, cells, t.float64)
        rank = new(want_rank, cells + (2,), t.int64)
        check(self.L.sipnet_batch_plane_quantiles_weighted(self.h, *plane, ptr(logw), n_q, ptr(qs), int(bool(live_only)), int(path),
                                                           ptr(quant), ptr(site_weight), ptr(fixed), ptr(moments), ptr(obs),
                                                           ptr(crps), ptr(rank), self._stream()), what)
        return WeightedQuantiles(quant, site_weight, crps, rank, moments, fixed, ran)

    def time_next_launch(self):
        """bracket the next run()'s step kernel with the timing events whatever its length (launches of 512 steps and
        more always are): last_kernel_ms() after it"""
        check(self.L.sipnet_batch_time_next_launch(self.h), "time_next_launch")

    def last_kernel_ms(self):
        return self.L.sipnet_batch_last_kernel_ms(self.h)

    # -- state ------------------------------------------------------------------
    def get_state(self):
        st = np.zeros((self.ncol, NSTATE))
        check(self.L.sipnet_batch_get_state(self.h, st.ctypes.data, self._stream()), "get_state")
        return st

    def set_state(self, st):
        st = np.ascontiguousarray(st, dtype=np.float64)
        assert st.shape == (self.ncol, NSTATE)
        check(self.L.sipnet_batch_set_state(self.h, st.ctypes.data, self._stream()), "set_state")

    def get_status(self):
        s = np.zeros(self.ncol, dtype=np.int32)
        check(self.L.sipnet_batch_get_status(self.h, s.ctypes.data, self._stream()), "get_status")
        return s

    def get_ring(self, col):
        v = np.zeros(RING_SLOTS)
        check(self.L.sipnet_batch_get_ring(self.h, col, v.ctypes.data, self._stream()), "get_ring")
        return v

    def get_rings(self):
        r = np.zeros((self.ncol, RING_SLOTS))
        check(self.L.sipnet_batch_get_rings(self.h, r.ctypes.data, self._stream()), "get_rings")
        return r

    def set_rings(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64)
        assert r.shape == (self.ncol, RING_SLOTS)
        check(self.L.sipnet_batch_set_rings(self.h, r.ctypes.data, self._stream()), "set_rings")

    def checkpoint(self):
        """Complete per-member carried state: (state[ncol][32], rings[ncol][250])."""
        return self.get_state(), self.get_rings()

    def restore(self, ckpt):
        self.set_state(ckpt[0])
        self.set_rings(ckpt[1])

    # -- restart checkpoints (sipnet.c:1963-1989, restart.c) ---------------------
    def set_resume(self, site, restart):
        """Site-uniform part of a checkpoint (gdd, lastYear, d_till_mod, ring layout); call
        before setup().  restart=None clears it."""
        ptr = C.byref(restart) if restart is not None else None
        check(self.L.sipnet_batch_set_resume(self.h, site, ptr), "set_resume")

    def import_restart(self, site, restarts, first_member=0):
        """After setup(): overwrite the carried state of len(restarts) members of `site`."""
        arr = (Restart * len(restarts))(*restarts)
        check(self.L.sipnet_batch_import_restart(self.h, site, first_member, len(restarts), arr,
                                                 self._stream()), "import_restart")

    def run_sums(self, step0, n_steps, sum_steps, out=None):
        """sipnet_batch_run_sums: every member's sums over groups of sum_steps steps, summed inside the step kernel's
        launch -> f64 device tensor [3][groups][ncol] (NEE, GPP, ET)"""
        t = self._torch
        groups = (n_steps + sum_steps - 1) // sum_steps
        if out is None:
            out = t.empty((3, groups, self.ncol), dtype=t.float64, device=self.device)
        assert _dense(out, t.float64) and out.shape == (3, groups, self.ncol)
        check(self.L.sipnet_batch_run_sums(self.h, int(step0), int(n_steps), int(sum_steps), ptr(out[0]), ptr(out[1]),
                                           ptr(out[2]), self.ncol, self._stream()), "run_sums")
        return out

    def sums_in_kernel(self):
        return bool(self.L.sipnet_batch_sums_in_kernel(self.h))

    def export_restart(self, site, member, n_steps_done, last_rec=None, prev_pools=None):
        """Checkpoint of one member after n_steps_done records (restartWriteCheckpoint)."""
        r = Restart()
        lr = pp = None
        if last_rec is not None:
            lr = np.ascontiguousarray(last_rec, dtype=np.float64)
            assert lr.shape == (NREC,)
        if prev_pools is not None:
            pp = np.ascontiguousarray(prev_pools, dtype=np.float64)
            assert pp.shape[0] >= 13
        check(self.L.sipnet_batch_export_restart(
            self.h, site, member, int(n_steps_done), lr.ctypes.data if lr is not None else None,
            pp.ctypes.data if pp is not None else None, C.byref(r), self._stream()), "export_restart")
        return r

    # -- particle-filter analysis step (pf.hip; BASELINE config C5) ---------------
    def pf_log_weights(self, plane, obs, sigma, out=None):
        """Gaussian log-likelihood of an observed flux sum: plane[T][ncol] (NEE, GPP or ET
        plane of the forecast) -> logw[ncol] f64 on the device."""
        t = self._torch
        if out is None:
            out = t.empty(self.ncol, dtype=t.float64, device=self.device)
        check(self.L.sipnet_batch_pf_log_weights(self.h, *self._plane(plane), float(obs), float(sigma), ptr(out),
                                                 self._stream()), "pf_log_weights")
        return out

    def pf_arm(self, obs, sigma):
        """sipnet_batch_pf_arm: the next run() (one-wave kernel, planes only) also leaves the log-weights that
        pf_analysis_local(planes[0], obs, sigma, ...) would otherwise compute in a pass of its own"""
        check(self.L.sipnet_batch_pf_arm(self.h, float(obs), float(sigma), ptr(self._pf_buffers()[0])), "pf_arm")

    def _pf_buffers(self):
        """(log-weights f64 [ncol], ancestors int32 [ncol]) of pf_arm and pf_analysis_local, made once"""
        if getattr(self, "_pf_buf", None) is None:
            t = self._torch
            self._pf_buf = (t.empty(self.ncol, dtype=t.float64, device=self.device),
                            t.empty(self.ncol, dtype=t.int32, device=self.device))
        return self._pf_buf

    def pf_arm_block(self, obs, sigma, block):
        """the same for a connected filter: the next run() leaves the log-weights in `block` (this rank's slice of the
        all-gather's buffer, pf_local_weights' target), which then only adds the block maxima"""
        check(self.L.sipnet_batch_pf_arm(self.h, float(obs), float(sigma), ptr(block)), "pf_arm")

    def pf_analysis_local(self, plane, obs, sigma, u0, with_params=False, total_out=None):
        """log-weights -> systematic resampling -> resample, all particles in this batch, ONE library call
        (sipnet_batch_pf_analysis).  Returns (ancestors int32 [ncol], logw f64 [ncol]) on the device."""
        logw, anc = self._pf_buffers()
        check(self.L.sipnet_batch_pf_analysis(self.h, *self._plane(plane), float(obs), float(sigma), float(u0), int(with_params),
                                              ptr(logw), ptr(anc), ptr(total_out), self._stream()), "pf_analysis")
        return anc, logw

    def pf_analysis_sites(self, plane, obs, sigma, u0, with_params=False, total_out=None, return_fixed=False):
        """every site a filter of its own, one library call (sipnet_batch_pf_analysis_sites): obs, sigma, u0 hold one
        value per site (array-likes, uploaded as float64, or float64 device tensors; obs NaN: no observation).
        total_out: int64 device tensor [n_sites] for the sites' total weights (no host synchronisation).  Returns
        (ancestors int32 [ncol] -- global columns --, logw f64 [ncol][, fixed-point weights int64 [ncol]]) on the device."""
        t = self._torch

        def per_site(x):
            x = self._flat64(x)
            assert x.numel() == self.n_sites
            return x

        obs, sigma, u0 = per_site(obs), per_site(sigma), per_site(u0)
        logw = t.empty(self.ncol, dtype=t.float64, device=self.device)
        anc = t.empty(self.ncol, dtype=t.int32, device=self.device)
        fixed = t.empty(self.ncol, dtype=t.int64, device=self.device) if return_fixed else None
        if total_out is not None:
            assert _dense(total_out, t.int64, self.n_sites)
        check(self.L.sipnet_batch_pf_analysis_sites(self.h, *self._plane(plane), ptr(obs), ptr(sigma), ptr(u0), int(with_params),
                                                    ptr(logw), ptr(anc), ptr(fixed), ptr(total_out), self._stream()),
              "pf_analysis_sites")
        return (anc, logw, fixed) if return_fixed else (anc, logw)

    def series_loglik(self, terms, normalise=True, add=None, out=None, parts_out=None, used_out=None, info_out=None, path=0):
        """every member's log-likelihood of a window against observed series with gaps (sipnet_batch_series_loglik).  terms:
        sa.loglik_term(...) values, at most sa.LOGLIK_MAX_TERMS, all of one dtype and row pitch; normalise: with the
        densities' constants; add: float64 device tensor [ncol] added last (may be `out`: weights carried over windows).
        out [ncol] f64, parts_out [n_terms][ncol] f64 (each term's own sum), used_out [n_sites][n_terms] int32 (rows used),
        info_out [n_sites][2] int32 ({code, rows used}; no host synchronisation -- without it the call checks obs and sd
        first and raises before anything is written): device tensors to write into.  path: 0 auto, 1 one launch, 2 tiles'
        sums and their sum (the same bits).  -> out.  The batch is not changed."""
        t = self._torch
        what = "series_loglik"
        terms = list(terms)
        if not 1 <= len(terms) <= LOGLIK_MAX_TERMS:
            raise ValueError(f"{what}: needs 1..{LOGLIK_MAX_TERMS} terms")
        layouts, desc, held = set(), [], []
        for k, term in enumerate(terms):
            series, obs, sd = term.held
            if (not t.is_tensor(series) or not series.is_cuda or series.dim() != 2 or series.dtype not in (t.float32, t.float64)
                    or not series.is_contiguous() or series.shape[1] < self.ncol):
                raise ValueError(f"{what}: term {k}: series must be a contiguous 2-D float32 / float64 device tensor "
                                 f"[rows * sum_steps][ld >= {self.ncol}]")
            p, f32, n, ld = self._plane(series)
            if term.sum_steps < 1 or n < term.sum_steps or n % term.sum_steps:
                raise ValueError(f"{what}: term {k}: {n} series rows are no multiple of sum_steps = {term.sum_steps}")
            rows = n // term.sum_steps
            obs = self._upload(what, obs, self.n_sites * rows, f"term {k}'s obs")
            sd = self._upload(what, sd, self.n_sites * rows, f"term {k}'s sd")
            layouts.add((f32, ld))
            held += [obs, sd]
            desc.append(LoglikTerm(series.data_ptr(), obs.data_ptr(), sd.data_ptr(), rows, term.sum_steps, term.kind, 0, term.scale))
        if len(layouts) > 1:
            raise ValueError(f"{what}: the terms' series differ in dtype or row pitch: " + str(sorted(layouts)))
        f32, ld = layouts.pop()

        def dense(x, dtype, n, name):
            if x is not None and not _dense(x, dtype, n):
                raise ValueError(f"{what}: {name} must be a contiguous device tensor of {n} {dtype} values")
            return x

        add = dense(add, t.float64, self.ncol, "add")
        if out is None:
            out = t.empty(self.ncol, dtype=t.float64, device=self.device)
        dense(out, t.float64, self.ncol, "out")
        dense(parts_out, t.float64, len(terms) * self.ncol, "parts_out")
        dense(used_out, t.int32, self.n_sites * len(terms), "used_out")
        dense(info_out, t.int32, 2 * self.n_sites, "info_out")
        check(self.L.sipnet_batch_series_loglik(self.h, len(desc), c_array(LoglikTerm, desc), f32, ld, int(bool(normalise)),
                                                int(path), ptr(add), ptr(out), ptr(parts_out), ptr(used_out), ptr(info_out),
                                                self._stream()), what)
        return out

    def pf_resample_sites(self, logw, u0, beta=None, ess_min=None, with_params=False, total_out=None, ess_out=None,
                          return_fixed=False):
        """the many-site analysis from log-weights the caller gives (sipnet_batch_pf_resample_sites): everything of
        pf_analysis_sites after its log-weights.  logw: float64 device tensor [ncol] (series_loglik's out, or anything else;
        NaN and -inf weigh nothing); u0, beta (None: 1; in (0, 1] it tempers), ess_min (None: every site resamples and logw
        is not written; else a site whose effective sample size is at least ess_min[s] keeps its particles -- total -3 --
        and a site that resamples gets its log-weights set to 0): one value per site.  total_out: int64 device tensor
        [n_sites] (no host synchronisation); ess_out: float64 device tensor [n_sites].  Returns (ancestors int32 [ncol] --
        global columns --[, fixed-point weights int64 [ncol]]) on the device."""
        t = self._torch
        what = "pf_resample_sites"
        if not t.is_tensor(logw) or not _dense(logw, t.float64, self.ncol):
            raise ValueError(f"{what}: logw must be a contiguous float64 device tensor of {self.ncol} values")
        u0 = self._upload(what, u0, self.n_sites, "u0")
        beta = self._upload(what, beta, self.n_sites, "beta")
        ess_min = self._upload(what, ess_min, self.n_sites, "ess_min")
        if u0 is None:
            raise ValueError(f"{what}: u0 needs {self.n_sites} values")
        if total_out is not None and not _dense(total_out, t.int64, self.n_sites):
            raise ValueError(f"{what}: total_out must be a contiguous int64 device tensor of {self.n_sites} values")
        if ess_out is not None and not _dense(ess_out, t.float64, self.n_sites):
            raise ValueError(f"{what}: ess_out must be a contiguous float64 device tensor of {self.n_sites} values")
        anc = t.empty(self.ncol, dtype=t.int32, device=self.device)
        fixed = t.empty(self.ncol, dtype=t.int64, device=self.device) if return_fixed else None
        check(self.L.sipnet_batch_pf_resample_sites(self.h, ptr(logw), ptr(u0), ptr(beta), ptr(ess_min), int(with_params),
                                                    ptr(anc), ptr(fixed), ptr(total_out), ptr(ess_out), self._stream()), what)
        return (anc, fixed) if return_fixed else anc

    def pf_temper_sites(self, loglik, ess_target, base=None, delta_max=None, out=None, info_out=None):
        """the tempering exponent of every site, chosen on the device (sipnet_batch_pf_temper_sites): the largest step delta in
        (0, delta_max] at which the tempered weights -- delta * loglik, or base + delta * loglik over carried log-weights --
        keep an effective sample size of at least ess_target, by the fixed search of sa.TEMPER_ROUNDS rounds of
        sa.TEMPER_SECTIONS - 1 candidates.  loglik: float64 device tensor [ncol] (series_loglik's out, or anything else);
        base: float64 device tensor [ncol] or None (0); ess_target, delta_max (None: 1; in a tempering run 1 - phi): one value
        per site; out: float64 device tensor [ncol] that takes the tempered log-weights of the sites with code 1 or 2 (may
        be base itself); info_out: int32 device tensor [n_sites][2] for {code, members whose value at delta = 0 is finite}
        (no host synchronisation); without it the arguments are checked first and a site with bad input raises before
        anything is written.  delta as beta of pf_resample_sites gives exactly the returned ess.  -> (delta, delta_hi, ess),
        float64 device tensors [n_sites]."""
        t = self._torch
        what = "pf_temper_sites"
        for x, name, needed in ((loglik, "loglik", True), (base, "base", False), (out, "out", False)):
            if (x is None and needed) or (x is not None and (not t.is_tensor(x) or not _dense(x, t.float64, self.ncol))):
                raise ValueError(f"{what}: {name} must be a contiguous float64 device tensor of {self.ncol} values")
        ess_target = self._upload(what, ess_target, self.n_sites, "ess_target")
        delta_max = self._upload(what, delta_max, self.n_sites, "delta_max")
        if ess_target is None:
            raise ValueError(f"{what}: ess_target needs {self.n_sites} values")
        self._info_out(what, info_out, TEMPER_INFO_WORDS)
        delta, delta_hi, ess = (t.zeros(self.n_sites, dtype=t.float64, device=self.device) for _ in range(3))
        check(self.L.sipnet_batch_pf_temper_sites(self.h, ptr(loglik), ptr(base), ptr(delta_max), ptr(ess_target), ptr(delta),
                                                  ptr(delta_hi), ptr(ess), ptr(out), ptr(info_out), self._stream()), what)
        return delta, delta_hi, ess

    def pf_rejuvenate(self, params, shrink, pools=None, pool_sd=None, seed=0, draw=0, streams=None, site_total=None,
                      info_out=None):
        """particle rejuvenation after a resampling (sipnet_batch_pf_rejuvenate): the Liu-West move of the listed parameter
        rows about the site's mean, x' = m + a (x - m) + sqrt(1 - a^2) sd z, reflected and clipped into the bounds, and
        additive noise q z on pools; z from the counter-based generator (sa.rejuvenate_normals), nothing drawn on the host.
        params: sa.enkf_param(name, lo, hi), at most sa.ENKF_MAX_PARAMS (() for none); shrink: a in (0, 1] per site
        (sa.liu_west_shrink(delta); 1 leaves the rows as they are; None with no params); pools: the pool names that get
        noise, pool_sd: [n_sites][13] their sds by state slot (0: the slot stays); seed, draw: the generator's key and the
        cycle number; streams: a uint32 per site that names its random stream (None: the site's index); site_total: int64
        device tensor [n_sites], pf_resample_sites' total_out -- only sites with a total > 0 (the resampled ones) are
        touched (None: every site); info_out: int32 device tensor [n_sites][4] for {code, rows + slots perturbed, live
        members, members kept} (no host synchronisation); without it the call checks shrink and pool_sd first and raises
        before anything is written."""
        what = "pf_rejuvenate"
        prm = list(params)
        mask = pool_mask(pools) if pools else 0
        shrink = self._upload(what, shrink, self.n_sites, "shrink")
        pool_sd = self._upload(what, pool_sd, self.n_sites * 13, "pool_sd")
        streams = self._streams(what, streams)
        self._site_total(what, site_total)
        self._info_out(what, info_out, REJUVENATE_INFO_WORDS)
        check(self.L.sipnet_batch_pf_rejuvenate(self.h, len(prm), c_array(EnkfParam, prm), ptr(shrink), mask, ptr(pool_sd),
                                                int(seed) & (2 ** 64 - 1), int(draw) & 0xffffffff, ptr(streams), ptr(site_total),
                                                ptr(info_out), self._stream()), what)

    def _streams(self, what, streams):
        """the sites' uint32 random streams on the device (None stays None)"""
        if streams is None:
            return None
        streams = np.ascontiguousarray(np.asarray(streams, dtype=np.uint32).reshape(-1))
        if streams.size != self.n_sites:
            raise ValueError(f"{what}: streams needs {self.n_sites} values, got {streams.size}")
        return self._torch.from_numpy(streams.view(np.int32)).to(self.device)

    def _info_out(self, what, info_out, words):
        """info_out (None: the synchronous form) checked: `words` int32 per site"""
        t = self._torch
        if info_out is not None and (not t.is_tensor(info_out) or not _dense(info_out, t.int32, words * self.n_sites)):
            raise ValueError(f"{what}: info_out must be a contiguous int32 device tensor of n_sites x {words}")

    def _site_total(self, what, site_total):
        """site_total (None: every site) checked: pf_resample_sites' total_out"""
        t = self._torch
        if site_total is not None and (not t.is_tensor(site_total) or not _dense(site_total, t.int64, self.n_sites)):
            raise ValueError(f"{what}: site_total must be a contiguous int64 device tensor of {self.n_sites} values")

    def mcmc_propose(self, params, gamma, jitter=None, half=0, seed=0, draw=0, streams=None, site_total=None, saved=None,
                     moved=None, info_out=None):
        """the proposal of a Metropolis move over the members of every site (sipnet_batch_mcmc_propose): the live members
        of one half (half = 0: even member index, 1: odd) get x' = x + gamma (x_r1 - x_r2) (+ jitter (hi - lo) z) in the
        listed parameter rows, both partners drawn from the live members of the other half (sa.mcmc_draws); a proposal
        outside the bounds is not made.  params: sa.enkf_param(name, lo, hi), 1..sa.ENKF_MAX_PARAMS; gamma
        (sa.demc_gamma(n)) and jitter (None: none): one value per site; seed, draw, streams, site_total: as pf_rejuvenate;
        saved: float64 device tensor [n_params][ncol], moved: int32 device tensor [ncol] (made when None); info_out: int32
        device tensor [n_sites][4] for {code, proposed, live members of the half, live members of the other half} (no host
        synchronisation); without it gamma and jitter are checked first.  -> (saved, moved), for mcmc_accept after
        setup(), run() and series_loglik()."""
        t = self._torch
        what = "mcmc_propose"
        prm = list(params)
        gamma = self._upload(what, gamma, self.n_sites, "gamma")
        jitter = self._upload(what, jitter, self.n_sites, "jitter")
        if gamma is None:
            raise ValueError(f"{what}: gamma needs {self.n_sites} values")
        streams = self._streams(what, streams)
        self._info_out(what, info_out, MCMC_INFO_WORDS)
        self._site_total(what, site_total)
        if saved is None:
            saved = t.zeros((max(len(prm), 1), self.ncol), dtype=t.float64, device=self.device)
        if moved is None:
            moved = t.zeros(self.ncol, dtype=t.int32, device=self.device)
        if not _dense(saved, t.float64, max(len(prm), 1) * self.ncol) or not _dense(moved, t.int32, self.ncol):
            raise ValueError(f"{what}: saved must be a contiguous float64 device tensor [n_params][{self.ncol}], moved an int32 one [{self.ncol}]")
        check(self.L.sipnet_batch_mcmc_propose(self.h, len(prm), c_array(EnkfParam, prm), ptr(gamma), ptr(jitter), int(half),
                                               int(seed) & (2 ** 64 - 1), int(draw) & 0xffffffff, ptr(streams), ptr(site_total),
                                               ptr(saved), ptr(moved), ptr(info_out), self._stream()), what)
        return saved, moved

    def mcmc_accept(self, params, saved, moved, logp_new, logp_cur, beta=None, seed=0, draw=0, streams=None, info_out=None):
        """the accept step of the move (sipnet_batch_mcmc_accept): a column with moved == 1 keeps its proposal iff
        logp_new < inf and beta (logp_new - logp_cur) > log u, and then logp_cur takes logp_new; else its listed rows come
        back from saved, bit for bit.  params, seed, draw, streams: as given to mcmc_propose; logp_new, logp_cur: float64
        device tensors [ncol] (logp_cur is updated in place); beta: one value per site (None: 1); info_out: int32 device
        tensor [n_sites][4] for {code, proposed, accepted, live members}.  moved is cleared."""
        t = self._torch
        what = "mcmc_accept"
        prm = list(params)
        beta = self._upload(what, beta, self.n_sites, "beta")
        streams = self._streams(what, streams)
        self._info_out(what, info_out, MCMC_INFO_WORDS)
        for x, dtype, n, name in ((saved, t.float64, max(len(prm), 1) * self.ncol, "saved"), (moved, t.int32, self.ncol, "moved"),
                                  (logp_new, t.float64, self.ncol, "logp_new"), (logp_cur, t.float64, self.ncol, "logp_cur")):
            if not t.is_tensor(x) or not _dense(x, dtype, n):
                raise ValueError(f"{what}: {name} must be a contiguous device tensor of {n} {dtype} values")
        check(self.L.sipnet_batch_mcmc_accept(self.h, len(prm), c_array(EnkfParam, prm), ptr(saved), ptr(moved), ptr(logp_new),
                                              ptr(logp_cur), ptr(beta), int(seed) & (2 ** 64 - 1), int(draw) & 0xffffffff,
                                              ptr(streams), ptr(info_out), self._stream()), what)

    def enkf_analysis_sites(self, obs, sd, operators, analysed, planes=None, inflation=None, info_out=None):
        """an ensemble Kalman filter analysis of the member pools, every site a filter of its own, one library call
        (sipnet_batch_enkf_analysis_sites).  obs, sd: [n_sites][n_obs] (array-likes, uploaded as float64, or float64 device
        tensors; obs NaN: not observed); operators: sa.enkf_pools / sa.enkf_plane, one per observation column; analysed:
        the pool names the update writes; planes: run()'s [3][n_steps][ld] tensor, or a list of three (None for planes no
        operator reads); inflation: one value per site (None: 1).  info_out: int32 device tensor [n_sites][4] for
        {code, observations used, live members, members kept on their forecast} (no host synchronisation); without it the
        call checks the inputs first and raises before anything is written."""
        a = self._enkf_args("enkf_analysis_sites", obs, sd, operators, analysed, planes, inflation, info_out)
        check(self.L.sipnet_batch_enkf_analysis_sites(self.h, *a.ops, *a.planes, *a.obs, a.info, self._stream()),
              "enkf_analysis_sites")

    def enkf_analysis_joint(self, obs, sd, operators, analysed, params, planes=None, inflation=None, param_inflation=None,
                            info_out=None):
        """a joint state-parameter ensemble Kalman filter analysis, every site a filter of its own
        (sipnet_batch_enkf_analysis_joint): enkf_analysis_sites with some of the members' parameters as analysed variables
        next to the pools.  params: sa.enkf_param(name, lo, hi), at most sa.ENKF_MAX_PARAMS (bounds in file units; the
        members' converted rows are clipped into them and rewritten); param_inflation: one value per site for the
        parameter variables (None: 1); the other arguments as enkf_analysis_sites."""
        what = "enkf_analysis_joint"
        a = self._enkf_args(what, obs, sd, operators, analysed, planes, inflation, info_out)
        prm, pinfl = self._enkf_params(what, params, param_inflation)
        check(self.L.sipnet_batch_enkf_analysis_joint(self.h, *a.ops, *prm, *a.planes, *a.obs, ptr(pinfl), a.info,
                                                      self._stream()), what)

    def enkf_analysis_smooth(self, obs, sd, operators, analysed, series, params=(), planes=None, inflation=None,
                             param_inflation=None, info_out=None):
        """an ensemble Kalman smoother of the window's series (sipnet_batch_enkf_analysis_smooth): enkf_analysis_joint (with
        params=() enkf_analysis_sites), and the same update applied to per-member series of the forecast window.  series: a
        list of device tensors [rows][ld] (float64 or float32, unit column stride, ld >= ncol), smoothed in place, or of
        (src, dst) pairs of the same shape, dtype and pitch; a 3-d tensor (run()'s [3][n_steps][ld] planes, run_sums()'s
        [3][groups][ncol]) counts as one series per leading index.  At most sa.ENKF_MAX_SERIES.  Live members of analysed
        sites get the filter's value, everything else dst = src.  Returns the list of dst tensors; the other arguments as
        enkf_analysis_joint."""
        t = self._torch
        what = "enkf_analysis_smooth"
        a = self._enkf_args(what, obs, sd, operators, analysed, planes, inflation, info_out)
        prm, pinfl = self._enkf_params(what, params, param_inflation)
        pairs = []
        for item in series:
            src, dst = item if isinstance(item, (tuple, list)) else (item, item)
            if src.dim() == 3 and dst.dim() == 3 and src.shape[0] == dst.shape[0]:
                pairs += [(src[k], dst[k]) for k in range(src.shape[0])]
            else:
                pairs.append((src, dst))
        desc = []
        for k, (src, dst) in enumerate(pairs):
            for x in (src, dst):
                if not x.is_cuda or x.dim() != 2 or x.dtype not in (t.float32, t.float64) or x.stride(1) != 1:
                    raise ValueError(f"{what}: series {k} must be a [rows][ld] float32 / float64 device tensor with unit "
                                     "column stride")
            if src.dtype != dst.dtype or src.shape[0] != dst.shape[0] or src.stride(0) != dst.stride(0):
                raise ValueError(f"{what}: series {k}: src and dst differ in dtype, rows or row pitch")
            if src.shape[1] < self.ncol:
                raise ValueError(f"{what}: series {k} has {src.shape[1]} columns, the batch {self.ncol}")
            ld = src.stride(0) if src.shape[0] > 1 else src.shape[1]
            desc.append(EnkfSeries(src.data_ptr(), dst.data_ptr(), src.shape[0], int(src.dtype == t.float32), ld))
        check(self.L.sipnet_batch_enkf_analysis_smooth(self.h, *a.ops, *prm, *a.planes, *a.obs, ptr(pinfl), len(pairs),
                                                       c_array(EnkfSeries, desc), a.info, self._stream()), what)
        return [dst for _, dst in pairs]

    def get_params(self, file_units=False):
        """the parameters every column carries (sipnet_batch_get_params) -> [ncol][80]: the converted rows as the kernels
        read them, or with file_units the nine per-year rates back in file units (x 365)"""
        p = np.zeros((self.ncol, NPARAMS))
        check(self.L.sipnet_batch_get_params(self.h, p.ctypes.data, int(bool(file_units)), self._stream()), "get_params")
        return p

    def enkf_localization(self, nbr_ptr, nbr, rho, n_obs):
        """a localization of this batch's sites for enkf_analysis_local (sipnet_batch_enkf_local_create): site s's neighbours
        nbr[nbr_ptr[s]:nbr_ptr[s + 1]] (strictly ascending, not s) with tapers rho in (0, 1] -- e.g. sa.gaspari_cohn's CSR
        arrays -- for n_obs observation columns.  -> an EnkfLocalization (.n_levels, .close()); closing the batch closes it."""
        loc = EnkfLocalization(self, nbr_ptr, nbr, rho, n_obs)
        if not hasattr(self, "_localizations"):
            self._localizations = weakref.WeakSet()
        self._localizations.add(loc)
        return loc

    def enkf_analysis_local(self, local, obs, sd, operators, analysed, planes=None, inflation=None, info_out=None):
        """a localized ensemble Kalman filter analysis across the sites (sipnet_batch_enkf_analysis_local): member j of every
        site is one member of a joint ensemble, and an observation moves the sites of its footprint, weighted by the
        localization's tapers.  local: enkf_localization(...) of this batch with n_obs = len(operators); the other
        arguments as enkf_analysis_sites."""
        loc = self._open_localization("enkf_analysis_local", local)
        a = self._enkf_args("enkf_analysis_local", obs, sd, operators, analysed, planes, inflation, info_out)
        check(self.L.sipnet_batch_enkf_analysis_local(self.h, loc, *a.ops, *a.planes, *a.obs, a.info, self._stream()),
              "enkf_analysis_local")

    def enkf_analysis_block(self, local, obs, sd, operators, analysed, planes=None, inflation=None, info_out=None,
                            rows_out=None):
        """a block-local ensemble Kalman filter analysis (sipnet_batch_enkf_analysis_block): every site is analysed on its
        own, from its observations and those of the sites that reach it, each with its variance divided by the taper --
        one pass, a constant number of launches.  A different filter from enkf_analysis_local (which keeps the serial
        order across sites); pick this one for regional batches.  local: enkf_localization(...) of this batch with
        n_obs = len(operators) and max_rows <= sa.ENKF_BLOCK_MAX_ROWS; rows_out: int32 device tensor [n_sites][2] for
        {rows used, rows dropped}; the other arguments as enkf_analysis_sites."""
        loc = self._open_localization("enkf_analysis_block", local)
        if rows_out is not None and not _dense(rows_out, self._torch.int32, 2 * self.n_sites):
            raise ValueError("enkf_analysis_block: rows_out must be a contiguous int32 device tensor of n_sites x 2")
        a = self._enkf_args("enkf_analysis_block", obs, sd, operators, analysed, planes, inflation, info_out)
        check(self.L.sipnet_batch_enkf_analysis_block(self.h, loc, *a.ops, *a.planes, *a.obs, a.info, ptr(rows_out),
                                                      self._stream()), "enkf_analysis_block")

    def enkf_moment_words(self, operators, analysed):
        """doubles in one site's moment block of enkf_shard_moments (sipnet_enkf_moment_words)"""
        return int(self.L.sipnet_enkf_moment_words(bin(pool_mask(analysed)).count("1"), len(list(operators))))

    def enkf_shard_moments(self, operators, analysed, planes=None, out=None):
        """this batch's share of a per-site EnKF analysis over an ensemble sharded by member across ranks
        (sipnet_batch_enkf_shard_moments): per site the live count, the means and the centred products of the analysed pools
        and predicted observations over this batch's live members -> a float64 device tensor [n_sites][W], W =
        enkf_moment_words(operators, analysed).  out: a contiguous float64 device tensor of that size to write into (a rank's
        slice of the all-gather's buffer).  The batch is not changed; operators, analysed and planes as enkf_analysis_sites."""
        t = self._torch
        what = "enkf_shard_moments"
        ops = list(operators)
        a = self._enkf_args(what, None, None, ops, analysed, planes, None, None)
        W = self.enkf_moment_words(ops, analysed)
        if W < 0:
            raise ValueError(f"{what}: needs 1..16 operators and 1..13 analysed pools")
        if out is None:
            out = t.empty((self.n_sites, W), dtype=t.float64, device=self.device)
        elif not _dense(out, t.float64, self.n_sites * W):
            raise ValueError(f"{what}: out must be a contiguous float64 device tensor of n_sites x {W}")
        check(self.L.sipnet_batch_enkf_shard_moments(self.h, *a.ops, *a.planes, ptr(out), self._stream()), what)
        return out.view(self.n_sites, W)

    def enkf_analysis_sharded(self, gathered, obs, sd, operators, analysed, planes=None, inflation=None, info_out=None):
        """the per-site EnKF analysis of an ensemble sharded by member across ranks, this batch's members moved
        (sipnet_batch_enkf_analysis_sharded).  gathered: every rank's enkf_shard_moments in rank order, a contiguous float64
        device tensor [world][n_sites][W]; obs, sd and inflation must be the same on every rank.  info_out[s] = {code,
        observations used, live members of the union, members of this batch kept on their forecast}; the other arguments as
        enkf_analysis_sites.  dist.enkf_analysis_sharded does the moments, the all-gather and this call."""
        t = self._torch
        what = "enkf_analysis_sharded"
        ops = list(operators)
        W = self.enkf_moment_words(ops, analysed)
        if not _dense(gathered, t.float64) or gathered.dim() != 3 or tuple(gathered.shape[1:]) != (self.n_sites, W):
            raise ValueError(f"{what}: gathered must be a contiguous float64 device tensor [world][{self.n_sites}][{W}]")
        a = self._enkf_args(what, obs, sd, ops, analysed, planes, inflation, info_out)
        check(self.L.sipnet_batch_enkf_analysis_sharded(self.h, *a.ops, *a.planes, *a.obs, int(gathered.shape[0]), ptr(gathered),
                                                        a.info, self._stream()), what)

    @staticmethod
    def _open_localization(what, local):
        """the handle of an EnkfLocalization that has not been closed"""
        if getattr(local, "h", None) is None:
            raise ValueError(f"{what}: the localization is closed")
        return local.h

    def _flat64(self, x):
        """x (an array-like or a tensor) as a contiguous flat float64 tensor on the batch's device"""
        t = self._torch
        return t.as_tensor(x, dtype=t.float64).reshape(-1).to(self.device).contiguous()

    def _upload(self, what, x, n, name):
        """_flat64(x), which must hold n values; None stays None"""
        if x is None:
            return None
        x = self._flat64(x)
        if x.numel() != n:
            raise ValueError(f"{what}: {name} needs {n} values, got {x.numel()}")
        return x

    def _enkf_params(self, what, params, param_inflation):
        """the joint analyses' (n_params, EnkfParam array), and the checked param_inflation on the device (None: 1), which
        the caller holds until the call"""
        prm = list(params)
        return (len(prm), c_array(EnkfParam, prm)), self._upload(what, param_inflation, self.n_sites, "param_inflation")

    def _enkf_args(self, what, obs, sd, operators, analysed, planes, inflation, info_out):
        """the EnKF analyses' arguments from n_obs to d_site_info as an EnkfArgs; it holds the uploaded tensors the
        pointers point into, so it must live until the call"""
        t = self._torch
        ops = list(operators)
        n_obs = len(ops)
        if obs is not None:                              # (None: a call without observations, enkf_shard_moments)
            obs = self._upload(what, obs, self.n_sites * n_obs, "obs")
            sd = self._upload(what, sd, self.n_sites * n_obs, "sd")
        infl = self._upload(what, inflation, self.n_sites, "inflation")
        arr = c_array(EnkfObs, ops)
        ptrs = (C.c_void_p * 3)()
        f32, n_steps, ld = 0, 0, 0
        if planes is not None:
            layouts = set()
            for k in range(3):
                p = planes[k]
                if p is None:
                    continue
                if not p.is_cuda or p.dim() != 2 or p.dtype not in (t.float32, t.float64) or p.stride(1) != 1:
                    raise ValueError(f"{what}: a plane must be a [n_steps][ld] float32 / float64 device tensor "
                                     "with unit column stride")
                ptrs[k] = p.data_ptr()
                layouts.add((int(p.dtype == t.float32), p.shape[0], p.stride(0)))
            if len(layouts) > 1:
                raise ValueError(f"{what}: the planes differ in dtype, step count or row pitch: " + str(layouts))
            if layouts:
                f32, n_steps, ld = layouts.pop()
        if info_out is not None and not _dense(info_out, t.int32, 4 * self.n_sites):
            raise ValueError(f"{what}: info_out must be a contiguous int32 device tensor of n_sites x 4")
        return EnkfArgs((n_obs, arr, pool_mask(analysed)), (ptrs if planes is not None else None, f32, n_steps, ld),
                        (ptr(obs), ptr(sd), ptr(infl)), ptr(info_out), (obs, sd, infl))

    # -- the filter across ranks by peer reads (sipnet_batch_pf_publish / _connect / _resample_peers) ----------
    def pf_publish(self, with_params=True):
        """-> bytes of this batch's sipnet_pf_peer descriptor (exchange them, then pf_connect)"""
        d = PfPeer()
        check(self.L.sipnet_batch_pf_publish(self.h, int(with_params), C.byref(d)), "pf_publish")
        return bytes(d)

    def pf_connect(self, descriptors, rank):
        """descriptors: every rank's pf_publish() bytes in rank order"""
        arr = c_array(PfPeer, [PfPeer.from_buffer_copy(x) for x in descriptors])
        check(self.L.sipnet_batch_pf_connect(self.h, len(descriptors), int(rank), arr), "pf_connect")
        self._pf_gathered = None

    def pf_block_len(self):
        return int(self.L.sipnet_batch_pf_block_len(self.h))

    def pf_info(self):
        """sipnet_batch_pf_info: what the last analysis did (one launch or several, its grid, the resident-workgroup
        budget) and how many of this rank's particles have crossed ranks since pf_connect (synchronises the stream)"""
        d = PfInfo()
        check(self.L.sipnet_batch_pf_info(self.h, C.byref(d), self._stream()), "pf_info")
        return d.as_dict()

    def debug_set_num_cus(self, n):
        """test hook: pretend the device has n compute units (32 = one partition of a CPX-mode MI355X)"""
        check(self.L.sipnet_debug_set_num_cus(self.h, int(n)), "debug_set_num_cus")

    def debug_pf_barrier(self, spin_budget=0, absent_workgroup=-1):
        """test hook: the poll budget of the one-launch analysis' barriers, and a workgroup of the NEXT such launch that
        leaves without arriving (the "grid not co-resident" path)"""
        check(self.L.sipnet_debug_pf_barrier(self.h, int(spin_budget), int(absent_workgroup)), "debug_pf_barrier")

    def set_device_share(self, n_filters):
        """sipnet_batch_set_device_share: how many filters analyse on this device at the same time"""
        check(self.L.sipnet_batch_set_device_share(self.h, int(n_filters)), "set_device_share")

    def pf_local_weights(self, plane, obs, sigma, block):
        """this rank's block [nmax log-weights | block maxima] of the all-gather, into `block` (f64 device
        tensor of pf_block_len() entries, e.g. this rank's slice of the gathered buffer)"""
        assert _dense(block, self._torch.float64, self.pf_block_len())
        check(self.L.sipnet_batch_pf_local_weights(self.h, *self._plane(plane), float(obs), float(sigma), ptr(block),
                                                   self._stream()), "pf_local_weights")
        return block

    def pf_resample_peers(self, gathered, u0, ancestors=None, total_out=None):
        """gathered[world][pf_block_len()]: every rank's block.  Resamples this rank's particles from wherever
        their ancestors live (peer reads); returns the ancestors' slots (int32 [ncol])."""
        t = self._torch
        assert _dense(gathered, t.float64)
        if ancestors is None:
            ancestors = t.empty(self.ncol, dtype=t.int32, device=self.device)
        check(self.L.sipnet_batch_pf_resample_peers(self.h, ptr(gathered), float(u0), ptr(ancestors), ptr(total_out),
                                                    self._stream()), "pf_resample_peers")
        return ancestors

    def pack_members(self, cols, with_params=False):
        """cols: int32 device tensor of local column indices -> packed block [words][n] of 8-byte words
        (state rows, ring rows -- floats for an fp32-mixed batch --, parameter rows)"""
        t = self._torch
        words = self.L.sipnet_batch_member_words(self.h, int(with_params))
        cols = cols.to(device=self.device, dtype=t.int32).contiguous()
        buf = t.empty((words, cols.numel()), dtype=t.float64, device=self.device)
        if cols.numel():
            check(self.L.sipnet_batch_pack_members(self.h, ptr(cols), cols.numel(), int(with_params), ptr(buf),
                                                   self._stream()), "pack_members")
        return buf

    def resample(self, src, recv=None, block_cols=(), with_params=False):
        """Column j becomes its ancestor src[j]: < ncol = own old column, ncol + k = received
        column k of `recv` (concatenated packed blocks with block_cols[s] columns each)."""
        t = self._torch
        src = src.to(device=self.device, dtype=t.int32).contiguous()
        assert src.numel() == self.ncol
        bc = c_array(C.c_int64, [int(x) for x in block_cols])
        rp = ptr(recv) if recv is not None and recv.numel() else None
        check(self.L.sipnet_batch_resample(self.h, ptr(src), rp, len(block_cols), bc, int(with_params), self._stream()),
              "resample")

    def site_series(self, site):
        g = np.zeros(self.n_steps)
        d = np.zeros(self.n_steps)
        check(self.L.sipnet_batch_get_site_series(self.h, site, g.ctypes.data, d.ctypes.data),
              "site_series")
        return g, d


def debug_live_bytes():
    """test hook (sipnet_debug_live_bytes): -> (device bytes, pinned host bytes) that the library's own objects hold right now,
    process-wide; back at an earlier reading once everything made since has been closed"""
    dev, pin = C.c_int64(0), C.c_int64(0)
    check(lib().sipnet_debug_live_bytes(C.byref(dev), C.byref(pin)), "debug_live_bytes")
    return dev.value, pin.value


def debug_fast_math(op, x, y=None, prec=F64, info=None):
    """test hook (sipnet_debug_fast_math): the throughput kernels' arithmetic helper `op` (_lib.FM_EXP2, FM_DIV, FM_RMINV,
    FM_RMAX0, FM_CLIP01, FM_RECR) on every element of the float64 tensor x (and y, for FM_DIV and FM_RMINV), as those kernels
    compile it; prec F32_MIXED: the float overload on the narrowed operands (FM_RECR: on the slot's low word), widened.
    info: a list that receives the exp2 polynomial's degree and the division's Newton steps of the loaded library.
    -> the results, a float64 tensor of x's shape on x's device"""
    import torch
    x = x.to(dtype=torch.float64).contiguous()
    assert x.is_cuda, "debug_fast_math: x must be on the device"
    if y is not None:
        y = y.to(device=x.device, dtype=torch.float64).contiguous()
        assert y.numel() == x.numel()
    out = torch.empty_like(x)
    words = (C.c_int32 * 2)()
    with torch.cuda.device(x.device):
        torch.cuda.current_stream().synchronize()       # (the hook launches on the null stream)
        check(lib().sipnet_debug_fast_math(int(op), int(prec), x.numel(), ptr(x) if x.numel() else None,
                                           ptr(y) if y is not None and y.numel() else None,
                                           ptr(out) if x.numel() else None, words), "debug_fast_math")
    if info is not None:
        info[:] = [words[0], words[1]]
    return out
