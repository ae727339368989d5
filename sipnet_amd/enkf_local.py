"""Localization for the ensemble Kalman filters across the sites of one batch (sipnet_batch_enkf_analysis_local, the serial
filter over the joint ensemble, and sipnet_batch_enkf_analysis_block, the block-local one): the Gaspari-Cohn taper of the
distances between sites, the host schedule of the observation slots, the row counts of the block-local analysis, and the
localization object Batch.enkf_localization returns."""
import ctypes as C

import numpy as np

from ._lib import check, lib

EARTH_RADIUS_KM = 6371.0
ENKF_BLOCK_MAX_ROWS = 128   # SIPNET_ENKF_BLOCK_MAX_ROWS


def _csr(nbr_ptr, nbr, rho):
    ptr = np.ascontiguousarray(nbr_ptr, dtype=np.int64).reshape(-1)
    idx = np.ascontiguousarray(nbr, dtype=np.int32).reshape(-1)
    w = np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
    if ptr.size < 1:
        raise ValueError("nbr_ptr needs n_sites + 1 entries")
    if idx.size != w.size:
        raise ValueError(f"nbr and rho differ in length: {idx.size} and {w.size}")
    if ptr.size > 1 and ptr[-1] > idx.size:
        raise ValueError(f"nbr_ptr ends at {int(ptr[-1])}, past the {idx.size} neighbours given")
    return ptr, idx, w


def _ptr(a):
    """the void* argument for a numpy array, NULL for an empty one (_lib.ptr keeps an empty array's address)"""
    return C.c_void_p(a.ctypes.data) if a.size else None


def enkf_local_schedule(nbr_ptr, nbr, rho, n_obs):
    """the host schedule of sipnet_batch_enkf_analysis_local (sipnet_enkf_local_schedule) for n_sites = len(nbr_ptr) - 1
    sites -> (level [n_sites][n_obs] int32, n_levels).  Raises SipnetError on a list the library refuses."""
    ptr, idx, w = _csr(nbr_ptr, nbr, rho)
    n_sites = ptr.size - 1
    level = np.zeros((max(n_sites, 0), max(int(n_obs), 0)), dtype=np.int32)
    n_levels = C.c_int32(0)
    check(lib().sipnet_enkf_local_schedule(n_sites, int(n_obs), _ptr(ptr), _ptr(idx), _ptr(w), _ptr(level),
                                           C.byref(n_levels)), "enkf_local_schedule")
    return level, int(n_levels.value)


def enkf_local_rows(nbr_ptr, nbr, n_obs):
    """the row counts of sipnet_batch_enkf_analysis_block (sipnet_enkf_local_rows, host only) for n_sites = len(nbr_ptr) - 1
    sites: n_obs x (1 + in-neighbours) of every site -> (rows [n_sites] int32, the largest).  The call refuses a batch whose
    largest exceeds sa.ENKF_BLOCK_MAX_ROWS.  Raises SipnetError on a list the library refuses."""
    ptr, idx, _ = _csr(nbr_ptr, nbr, np.zeros(np.asarray(nbr).size))
    n_sites = ptr.size - 1
    rows = np.zeros(max(n_sites, 0), dtype=np.int32)
    most = C.c_int32(0)
    check(lib().sipnet_enkf_local_rows(n_sites, int(n_obs), _ptr(ptr), _ptr(idx), _ptr(rows), C.byref(most)),
          "enkf_local_rows")
    return rows, int(most.value)


def gaspari_cohn(lat_deg, lon_deg, half_width_km):
    """the Gaspari-Cohn (1999, eq. 4.10) fifth-order taper of the great-circle distance d between sites on a 6371 km sphere,
    with half-width c = half_width_km (1 at d = 0, 5/24 at d = c, 0 from d = 2c) -> CSR (nbr_ptr int64, nbr int32,
    rho float64) of every pair of distinct sites with rho > 0, rows ascending: Batch.enkf_localization's arguments."""
    lat = np.radians(np.asarray(lat_deg, dtype=np.float64).reshape(-1))
    lon = np.radians(np.asarray(lon_deg, dtype=np.float64).reshape(-1))
    if lat.shape != lon.shape:
        raise ValueError("lat_deg and lon_deg differ in length")
    c = float(half_width_km)
    if not (c > 0.0 and np.isfinite(c)):
        raise ValueError("half_width_km must be finite and > 0")
    n = lat.size
    ptr = np.zeros(n + 1, dtype=np.int64)
    nbrs, rhos = [], []
    coslat = np.cos(lat)
    for s in range(n):
        # haversine, in terms symmetric in the two sites: d(s, t) == d(t, s) bit for bit
        a = np.sin(np.abs(lat - lat[s]) * 0.5) ** 2 + (coslat * coslat[s]) * np.sin(np.abs(lon - lon[s]) * 0.5) ** 2
        d = 2.0 * EARTH_RADIUS_KM * np.arcsin(np.sqrt(np.minimum(a, 1.0)))
        rho = taper(d / c)
        keep = np.flatnonzero(rho > 0.0)
        keep = keep[keep != s]
        nbrs.append(keep.astype(np.int32))
        rhos.append(rho[keep])
        ptr[s + 1] = ptr[s] + keep.size
    nbr = np.concatenate(nbrs) if n else np.zeros(0, np.int32)
    rho = np.concatenate(rhos) if n else np.zeros(0)
    return ptr, nbr.astype(np.int32), np.minimum(rho, 1.0)


def taper(r):
    """the Gaspari-Cohn fifth-order piecewise rational function of r = d / c (c the half-width)"""
    r = np.abs(np.asarray(r, dtype=np.float64))
    out = np.zeros_like(r)
    a = r <= 1.0
    b = (r > 1.0) & (r < 2.0)
    x = r[a]
    out[a] = (((-0.25 * x + 0.5) * x + 0.625) * x - 5.0 / 3.0) * x * x + 1.0
    x = r[b]
    out[b] = ((((x / 12.0 - 0.5) * x + 0.625) * x + 5.0 / 3.0) * x - 5.0) * x + 4.0 - 2.0 / (3.0 * x)
    return out


class EnkfLocalization:
    """a localization of one batch's sites (sipnet_enkf_local): made by Batch.enkf_localization, closed before its batch
    (Batch.close does that).  n_levels: level launches per enkf_analysis_local; max_rows: the largest row count of a site
    in enkf_analysis_block (sa.enkf_local_rows)."""

    def __init__(self, batch, nbr_ptr, nbr, rho, n_obs):
        self.h = None
        ptr, idx, w = _csr(nbr_ptr, nbr, rho)
        if ptr.size != batch.n_sites + 1:
            raise ValueError(f"enkf_localization: nbr_ptr needs n_sites + 1 = {batch.n_sites + 1} entries, got {ptr.size}")
        self.L = batch.L
        self.n_obs = int(n_obs)
        h = C.c_void_p()
        check(self.L.sipnet_batch_enkf_local_create(batch.h, self.n_obs, _ptr(ptr), _ptr(idx), _ptr(w), C.byref(h)),
              "enkf_localization")
        self.h = h
        self.max_rows = enkf_local_rows(ptr, idx, self.n_obs)[1]

    @property
    def n_levels(self):
        return int(self.L.sipnet_enkf_local_levels(self.h)) if self.h else 0

    def debug_serial(self, on=True):
        """one observation slot per launch, in serial order (sipnet_debug_enkf_local_serial): the test of the schedule"""
        check(self.L.sipnet_debug_enkf_local_serial(self.h, int(bool(on))), "debug_enkf_local_serial")

    def close(self):
        if getattr(self, "h", None):
            self.L.sipnet_enkf_local_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
