"""Helpers of tests/test_pf_edges.py (which pins them) and tests/test_gpu_pf_edges.py (which holds the kernels to them): the
fixed-point weight of sipnet_amd/csrc/pf_weights.inc against an exponential of higher precision, with a derived tolerance;
crafted log-weights whose integer weights are known in advance, placed where the many-site searches of pf_sites.inc change
level (a thread's first and last slot, threads and chunks that weigh nothing, a last chunk of one column); and planes whose
step-order sums cancel large rows down to a wanted log-weight.  No tests here."""
import numpy as np

G = 1 << 30                     # the weight of a site's best particle
LOG2E = 1.4426950408889634      # pfFixedWeight's constant (the double nearest log2 e)
LN2 = 0.6931471805599453
CUT = -21.5                     # pfFixedWeight's cut-off
THREADS = 256                   # threads of a workgroup of the many-site kernels
SITES_LDS = 4096                # kSitesLds: sites of more particles take the split path whatever is forced
MAX_CHUNKS = 1024               # kSitesMaxChunks

# log-weights (under a maximum of 0) whose integer is beyond doubt: 2^30 e^-20 = 2.2131.., 2^30 e^-21.4 = 0.54575..
LW_OF = {G: 0.0, 2: -20.0, 1: -21.4}
ZEROS = (-np.inf, np.nan, -1000.0)   # all weigh nothing

PATTERNS = ("first", "last", "uniform", "slot_ends", "slot_starts", "thread_gaps", "chunk_gaps", "last_chunk_only",
            "ones_and_a_giant", "two_giants", "sparse")
U0S = (0.0, 0.5, 1.0 - 2.0 ** -53, 5e-324, 0.377)

# the shapes of the ancestor tests: next to 256, 512 and kSitesLds on both paths; on the split path one site each where the
# chunk doubles (262 144: 1024 chunks of 256; 262 145: 513 chunks of 512, the last of one column; 524 289: 513 chunks of 1024)
GROUP_M = (2, 255, 256, 257, 511, 512, 513, 4095, 4096)
SPLIT_M = GROUP_M + (4097,)
BIG_M = (262144, 262145, 524289)


def shapes():
    """every (path, M) the ancestor tests run"""
    return [("group", M) for M in GROUP_M] + [("split", M) for M in SPLIT_M + BIG_M]


def rounds(n_sites):
    """-> a list of rounds, each a list of (pattern name, u0) for the batch's sites: patterns and u0 rotate over the sites
    so that every pattern is met (and, over the shapes, every u0 by every pattern)"""
    n_rounds = -(-len(PATTERNS) // n_sites)
    return [[(PATTERNS[(r * n_sites + s) % len(PATTERNS)], U0S[(r * (n_sites + 1) + s) % len(U0S)]) for s in range(n_sites)]
            for r in range(n_rounds)]


def longdouble_is_wide():
    """np.longdouble carries at least the x87 format's 64-bit significand (else the reference is no better than the
    device: the callers skip)"""
    return np.finfo(np.longdouble).nmant >= 63


def fixed_weight_exact(lw, m):
    """rint(2^30 e^(lw - m)) from an exponential of higher precision -> (nearest integer int64, d, tol), arrays like lw.

    x = fl(lw - m) is formed in float64: that difference is part of the operation's definition (pfFixedWeight gets lw and
    m and subtracts them in double).  2^30 e^x is then evaluated in np.longdouble (64-bit significand: its own error, a few
    1e-19 relative, is far below everything here).  d is the distance of that value from the nearest half-integer, i.e.
    from the nearest point where the rounding changes; tol is what the device's value may be off by:

        tol(x) = w * (ln 2 * |y| * 2^-52 + 1e-15),     w = 2^30 e^x,  y = x * log2(e)

    derived, not measured, from the steps of pfFixedWeight that are not exact:
      * y = fl(x * LOG2E), with LOG2E the double nearest log2 e: one rounding of the product (2^-53 relative) and the
        constant's own (at most 2^-53 relative) -- together at most 2^-52 relative on y, i.e. |y| 2^-52 absolute on the
        exponent, i.e. ln 2 * |y| * 2^-52 relative on 2^y;
      * the degree-11 interpolant of 2^f on [-1/2, 1/2]: |relative error| <= 1.7e-16 as documented, plus the eleven
        fused multiply-adds of its Horner form, each at most 2^-53 of a partial result that the factor |f| <= 1/2 damps
        geometrically: below 2 * 2^-53 + ... < 3e-16 in all; 1e-15 covers both with a margin of two;
      * n = rint(y), f = y - n (Sterbenz: exact) and the ldexp by n + 30 are exact (no result here is subnormal).
    Wherever d > tol the device's integer must BE the reference's; only where d <= tol may it be the neighbour.  tol never
    exceeds about 1.2e-6 weight units (at x near 0, where w = 2^30), so such points are about one in a million.

    The result is 0, with d = inf and tol = 0, for a NaN x (NaN log-weights; -inf under -inf), for -inf and for x < -21.5:
    the exact value is below 2^30 e^-21.5 = 0.4938 there, so the cut-off agrees with true rounding (which first gives 1 at
    x = ln(0.5 / 2^30) = -21.48756..)."""
    assert longdouble_is_wide(), "np.longdouble has no 64-bit significand here"
    L = np.longdouble
    lw = np.asarray(lw, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        x = lw - np.asarray(m, dtype=np.float64)      # (m: one maximum, or one per entry)
    live = x >= CUT                                   # (False for NaN)
    xs = np.where(live, x, 0.0)
    w = np.exp(xs.astype(L)) * L(G)
    near = np.rint(w)
    d = np.abs((w - np.floor(w)) - L(0.5))
    tol = w * (L(LN2) * np.abs(xs * LOG2E).astype(L) * L(2.0 ** -52) + L(1e-15))
    near = np.where(live, near, 0).astype(np.int64)
    d = np.where(live, d, np.inf).astype(np.float64)
    tol = np.where(live, tol, 0.0).astype(np.float64)
    return near, d, tol


def uniform_x(n, seed=20):
    """n values uniform in [-21.6, 0] (a tenth below the cut-off to the maximum)"""
    return np.random.default_rng(seed).uniform(-21.6, 0.0, n)


def directed_x():
    """-> (x [n], want [n] or -1 where the value is left to the reference): the points where a polynomial, a cut-off or a
    rounding rule that is slightly off shows first"""
    x, want = [], []
    for k in range(4):                                # either side of the first four rounding points
        for sign, w in ((-1.0, k), (1.0, k + 1)):
            x.append(float(np.log(np.longdouble((k + 0.5) * (1.0 + sign * 1e-6)) / np.longdouble(G))))
            want.append(w)
    for v, w in ((CUT, 0), (np.nextafter(CUT, 0.0), 0), (-21.4876, 0), (-21.4875, 1)):   # the cut-off; true rounding's start
        x.append(v)
        want.append(w)
    for v, w in ((-0.0, G), (5e-324, G), (-1e308, 0), (-np.inf, 0), (np.nan, 0)):
        x.append(v)
        want.append(w)
    for j in range(1, 31):                            # 2^(30 - j), up to the double's distance from -j ln 2
        x.append(-j * LN2)
        want.append(1 << (30 - j))
    return np.array(x), np.array(want, dtype=np.int64)


def geometry(M, path):
    """-> (per, chunk, n_chunks) of a site of M particles: path "group" (pfSitesKernel: one chunk of 256 threads x per =
    ceil(M / 256) consecutive slots) or "split" (chunks of 256 x per columns, per the smallest power of two that needs at
    most 1024 chunks)"""
    if path == "group":
        assert M <= SITES_LDS
        per = (M + THREADS - 1) // THREADS
        return per, THREADS * per, 1
    chunk = THREADS
    while (M + chunk - 1) // chunk > MAX_CHUNKS:
        chunk *= 2
    return chunk // THREADS, chunk, (M + chunk - 1) // chunk


def pattern(name, M, per, chunk, seed=0, k=None):
    """-> (logw float64 [M], fixed int64 [M]): log-weights of one site and their integer weights, known in advance (only
    LW_OF's and ZEROS' values are used; every pattern holds at least one 0.0, so the site's maximum is 0).  per, chunk:
    geometry() of the path the pattern is laid out for -- slot i belongs to chunk i // chunk, thread (i % chunk) // per."""
    i = np.arange(M)
    c, t, slot = i // chunk, (i % chunk) // per, i % per
    last_chunk = (M - 1) // chunk
    fixed = np.zeros(M, dtype=np.int64)
    if name == "first":
        fixed[0] = G
    elif name == "last":
        fixed[M - 1] = G
    elif name == "uniform":
        fixed[:] = G
    elif name == "slot_ends":
        fixed[slot == per - 1] = G
    elif name == "slot_starts":
        fixed[slot == 0] = G
    elif name == "thread_gaps":
        fixed[np.isin(t, (0, 1, THREADS - 2, THREADS - 1))] = G
    elif name == "chunk_gaps":
        fixed[(c == 0) | (c == last_chunk)] = G
    elif name == "last_chunk_only":
        fixed[c == last_chunk] = G
    elif name == "ones_and_a_giant":
        fixed[:] = 1
        fixed[M // 3] = G
    elif name == "two_giants":
        fixed[:] = 2
        fixed[0] = fixed[M - 1] = G
    elif name == "sparse":
        rng = np.random.default_rng(seed)
        fixed[rng.choice(M, size=max(1, M // 100), replace=False)] = G
    elif name == "k_giants":
        assert 1 <= k <= M
        fixed[(np.arange(k) * M) // k] = G
    else:
        raise ValueError(name)
    assert (fixed == G).any()
    logw = np.empty(M)
    if name == "sparse":                               # "the rest alternates NaN and -inf"
        logw[:] = np.where(i % 2 == 0, np.nan, -np.inf)
    else:
        logw[:] = np.asarray(ZEROS)[(i + seed) % len(ZEROS)]
    for w, lw in LW_OF.items():
        logw[fixed == w] = lw
    return logw, fixed


def _exact_rows(s, L, rng, fine):
    """[L][n] rows whose sum is s [n] (multiples of 2^-12, at most 1008) with every partial sum exact in fp64: s itself in
    one row, the others large and cancelling (pairs +B, -B and, for an odd count, one triple B1, B2, -(B1 + B2)).  B is
    about 2e7 .. 7e7: 16 x an integer of 21 or 22 bits (exactly representable in float32, as their sums are), or, fine, a
    multiple of 2^-12 with 37 or 38 significant bits (float64 only)."""
    n = len(s)
    if L == 1:
        return s[None, :].copy()
    if L == 2:
        return np.stack([s + 8.0, np.full(n, -8.0)])

    def big():
        return rng.integers(1 << 36, 1 << 38, size=n) / 4096.0 if fine else 16.0 * rng.integers(1 << 20, 1 << 22, size=n)

    rows = [s]
    other = L - 1
    if other % 2:
        b1, b2 = big(), big()
        rows += [b1, b2, -(b1 + b2)]
        other -= 3
    for _ in range(other // 2):
        b = big()
        rows += [b, -b]
    return np.stack([rows[q] for q in rng.permutation(L)])


def cancelling_plane(lw_target, n_steps, ld, dtype, seed=0):
    """-> plane [n_steps][ld] of `dtype` (np.float32 / np.float64) whose first len(lw_target) columns sum, in step order in
    fp64, to s = sqrt(-2 lw_target) rounded to a multiple of 2^-12 -- so that against obs = 0, sigma = 1 column c's
    log-weight is -s^2 / 2, lw_target[c] to about 1e-3 (near enough for LW_OF's integers to stay beyond doubt, also under a
    common shift of a site's targets: equal targets give bit-equal log-weights).  Targets that are -inf or NaN ("weighs
    nothing") sum to 1e3: a log-weight of -5e5.  The expected log-weight is oracle.pf_oracle.log_weights of this very plane.

    The rows: large ones that cancel, so that a row skipped, read twice or read at the wrong stride leaves about 1e7 and the
    column weighs nothing.  Every partial sum is exact in fp64 (_exact_rows), so the step-order sum IS the sum; float32
    planes hold only values that float32 represents exactly, float64 planes values of up to 38 significant bits that it
    does not.  The pad columns ncol .. ld hold 1e300 (float32: 3e38): nothing that reads one keeps a finite log-weight."""
    lw_target = np.asarray(lw_target, dtype=np.float64)
    ncol = len(lw_target)
    assert ld >= ncol and n_steps >= 1
    rng = np.random.default_rng(seed)
    with np.errstate(invalid="ignore"):
        s = np.where(lw_target > -np.inf, np.sqrt(-2.0 * lw_target), 1e3)
    s = np.rint(np.where(np.isnan(s), 1e3, s) * 4096.0) / 4096.0
    assert (s <= 1000.0).all()
    rows = _exact_rows(s, n_steps, rng, fine=dtype == np.float64)
    plane = np.full((n_steps, ld), 1e300 if dtype == np.float64 else 3e38, dtype=dtype)
    plane[:, :ncol] = rows
    assert (plane[:, :ncol].astype(np.float64) == rows).all()                # (float32: nothing was rounded)
    return plane
