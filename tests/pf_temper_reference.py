"""The search of sipnet_batch_pf_temper_sites in numpy (tests/test_pf_temper.py pins it, tests/test_gpu_pf_temper.py holds the
kernels to it): the fixed rounds over an `ess` callable that evaluates a list of steps at once -- a longdouble ESS of real
weights, or a probe of the device through pf_resample_sites -- and that longdouble ESS.  No tests here."""
import numpy as np

SECTIONS, ROUNDS = 16, 8           # SIPNET_TEMPER_SECTIONS, SIPNET_TEMPER_ROUNDS
FOUND, END, NO_WEIGHT, UNREACHABLE, BAD_INPUT = 1, 2, 0, -1, -2


def candidates(lo, hi):
    """b_i = lo + (hi - lo) * (i * 0.0625), i = 1 .. 15: float64, the product and the sum each rounded on their own"""
    lo, hi = np.float64(lo), np.float64(hi)
    width = hi - lo
    return np.array([lo + width * np.float64(i * 0.0625) for i in range(1, SECTIONS)], dtype=np.float64)


def bad_scalars(delta_max, target):
    """the scalars that make a site bad input"""
    return not (np.isfinite(delta_max) and delta_max > 0.0) or not target > 0.0


def search(ess, delta_max, target, trace=None):
    """-> (code, delta, delta_hi, ess(delta)).  ess(d): float64 array of steps -> their effective sample sizes (0 where
    nothing weighs anything); it is asked for [0], [delta_max] and then ROUNDS times for the 15 candidates.  trace: a
    list that takes every round's (lo, hi, k)."""
    delta_max, target = np.float64(delta_max), np.float64(target)
    if bad_scalars(delta_max, target):
        return BAD_INPUT, 0.0, 0.0, 0.0
    e0 = np.float64(ess(np.array([0.0]))[0])
    if e0 == 0.0:
        return NO_WEIGHT, 0.0, 0.0, 0.0
    if e0 < target:
        return UNREACHABLE, 0.0, 0.0, float(e0)
    e_max = np.float64(ess(np.array([delta_max]))[0])
    if e_max >= target:
        return END, float(delta_max), float(delta_max), float(e_max)
    lo, hi, e_lo = np.float64(0.0), delta_max, e0
    for _ in range(ROUNDS):
        b = candidates(lo, hi)
        e = np.asarray(ess(b), dtype=np.float64)
        k = 0
        while k < SECTIONS - 1 and e[k] >= target:
            k += 1
        if trace is not None:
            trace.append((float(lo), float(hi), k))
        if k > 0:
            lo, e_lo = b[k - 1], e[k - 1]
        if k < SECTIONS - 1:
            hi = b[k]
    return FOUND, float(lo), float(hi), float(e_lo)


def tempered(d, loglik, base=None):
    """v_c(d) in longdouble, unrounded but for the inputs: d * loglik (+ base); a member whose loglik is not finite stays NaN
    at d = 0 as on the device"""
    L = np.longdouble
    with np.errstate(invalid="ignore", over="ignore"):
        v = L(d) * np.asarray(loglik, dtype=np.float64).astype(L)
        if base is not None:
            v = v + np.asarray(base, dtype=np.float64).astype(L)
    return v


def ess_real(d, loglik, base=None):
    """the effective sample size of the real weights exp(v_c(d) - max) in longdouble (NaN and -inf weigh nothing) -> longdouble"""
    v = tempered(d, loglik, base)
    live = np.isfinite(v)
    if not live.any():
        return np.longdouble(0.0)
    w = np.exp(v[live] - v[live].max())
    return w.sum() ** 2 / (w * w).sum()


def ess_real_of(loglik, base=None):
    """-> the callable search() wants, over ess_real"""
    return lambda ds: np.array([float(ess_real(d, loglik, base)) for d in ds])
