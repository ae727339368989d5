"""sipnet_amd -- MI355X-native SIPNET flux-integration engine.

Host-side mirror of the reference's C interface for the hot path
(/root/reference/src/sipnet/sipnet.h:26-64) over the C-ABI in
include/sipnet_amd.h.  PyTorch is used only for device memory, streams and
torch.distributed; all model arithmetic runs in hand-written HIP kernels
(sipnet_amd/csrc/step_kernel.hip).
"""
from ._lib import (KERNEL_AUTO, KERNEL_COOP_HBM, KERNEL_COOP_LDS, KERNEL_COOP_PAIR, KERNEL_COOP_QUAD, KERNEL_COOP_NCYCLE, KERNEL_COOP_NCYCLE_PAIR, KERNEL_ONE_WAVE, KERNEL_STRICT,
                   KOPT_FULL_STATE, KOPT_NO_REGULAR_TILES, KOPT_ONE_WAVE_PER_SIMD, KOPT_RUNTIME_FLAGS,
                   KOPT_STATS_IN_KERNEL, KOPT_BOUNDED_WAITS, KOPT_WAIT_SELFTEST, KOPT_HOST_PLAN, KOPT_DEVICE_PLAN,
                   KOPT_PF_MULTI_LAUNCH, KOPT_PF_MOVE_PARAMS, PF_VOID_TOTAL)
from ._lib import (LOGLIK_GAUSS, LOGLIK_LAPLACE, LOGLIK_MAX_TERMS, LOGLIK_TILE_ROWS)
from ._lib import (ENKF_MAX_PARAMS, ENKF_MAX_SERIES, F32_MIXED, F64, NCLIM, NFLAGS, NPARAMS, NREC, NSTATE, RING_SLOTS,
                   Event, Restart, SipnetError, lib)
from .config import (DEFAULT_FLAGS, FLAG_NAMES, PARAM_NAMES, POOLS, enkf_param, enkf_plane, enkf_pools, flags_from, read_config)
from .io import (ClimTable, format_out_header, format_out_row, read_clim, read_events,
                 read_params, read_restart, check_restart, write_debug_logs, write_events_out, write_out,
                 write_restart)
from .batch import (Batch, PlaneQuantiles, WeightedQuantiles, wquantile_lds_members, wquantile_target, debug_fast_math, debug_live_bytes, liu_west_shrink, loglik_term, philox4x32_10, quantile_lds_members,
                    quantile_positions, rejuvenate_normals, demc_gamma, mcmc_draws)
from ._lib import (REJUVENATE_BAD_INPUT, REJUVENATE_DONE, REJUVENATE_INFO_WORDS, REJUVENATE_NOT_SELECTED, REJUVENATE_TOO_FEW)
from ._lib import (MCMC_BAD_INPUT, MCMC_DONE, MCMC_INFO_WORDS, MCMC_NOT_SELECTED, MCMC_TOO_FEW)
from ._lib import (TEMPER_BAD_INPUT, TEMPER_END, TEMPER_FOUND, TEMPER_INFO_WORDS, TEMPER_NO_WEIGHT, TEMPER_ROUNDS, TEMPER_SECTIONS,
                   TEMPER_UNREACHABLE)
from .enkf_local import ENKF_BLOCK_MAX_ROWS, EnkfLocalization, enkf_local_rows, enkf_local_schedule, gaspari_cohn

__all__ = [
    "Batch", "PlaneQuantiles", "debug_live_bytes", "debug_fast_math", "quantile_positions", "quantile_lds_members", "WeightedQuantiles", "wquantile_target", "wquantile_lds_members", "EnkfLocalization", "enkf_local_schedule", "enkf_local_rows", "ENKF_BLOCK_MAX_ROWS", "gaspari_cohn", "ClimTable", "Event", "Restart", "SipnetError", "read_restart", "write_restart",
    "check_restart", "lib", "read_clim", "read_params",
    "read_events", "write_out", "write_events_out", "write_debug_logs", "format_out_header", "format_out_row", "read_config",
    "flags_from", "FLAG_NAMES", "POOLS", "enkf_pools", "enkf_plane", "enkf_param", "ENKF_MAX_PARAMS", "ENKF_MAX_SERIES", "DEFAULT_FLAGS", "PARAM_NAMES", "F64", "F32_MIXED",
    "KERNEL_AUTO", "KERNEL_ONE_WAVE", "KERNEL_COOP_LDS", "KERNEL_COOP_HBM", "KERNEL_COOP_PAIR", "KERNEL_COOP_QUAD", "KERNEL_COOP_NCYCLE", "KERNEL_COOP_NCYCLE_PAIR", "KERNEL_STRICT",
    "KOPT_ONE_WAVE_PER_SIMD", "KOPT_RUNTIME_FLAGS", "KOPT_FULL_STATE", "KOPT_NO_REGULAR_TILES", "KOPT_STATS_IN_KERNEL", "KOPT_BOUNDED_WAITS", "KOPT_WAIT_SELFTEST", "KOPT_HOST_PLAN", "KOPT_DEVICE_PLAN", "KOPT_PF_MULTI_LAUNCH", "KOPT_PF_MOVE_PARAMS", "PF_VOID_TOTAL",
    "NPARAMS", "NFLAGS", "NCLIM", "NREC", "NSTATE", "RING_SLOTS",
    "philox4x32_10", "rejuvenate_normals", "liu_west_shrink", "REJUVENATE_INFO_WORDS", "REJUVENATE_DONE", "REJUVENATE_TOO_FEW",
    "REJUVENATE_BAD_INPUT", "REJUVENATE_NOT_SELECTED",
    "mcmc_draws", "demc_gamma", "MCMC_INFO_WORDS", "MCMC_DONE", "MCMC_TOO_FEW", "MCMC_BAD_INPUT", "MCMC_NOT_SELECTED",
    "TEMPER_SECTIONS", "TEMPER_ROUNDS", "TEMPER_INFO_WORDS", "TEMPER_FOUND", "TEMPER_END", "TEMPER_NO_WEIGHT", "TEMPER_UNREACHABLE",
    "TEMPER_BAD_INPUT",
    "loglik_term", "LOGLIK_GAUSS", "LOGLIK_LAPLACE", "LOGLIK_MAX_TERMS", "LOGLIK_TILE_ROWS",
]
