"""Reference for sipnet_batch_pf_rejuvenate (no GPU, no library): Philox4x32-10 in numpy uint64, the Box-Muller normals and
the whole update -- the Liu-West move of listed parameter rows, the pool noise, the limits, the member rule, the codes -- in
np.longdouble, restated from include/sipnet_amd.h.  Everything is vectorised over members."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))
TINY = 0.000001
INFO_WORDS = 4
DONE, TOO_FEW, BAD_INPUT, NOT_SELECTED = 1, 0, -2, -3
NPOOLS = 13
WOOD, COARSE_ROOT, FINE_ROOT, DELTA = 0, 6, 7, 12
PSN_TMIN, PSN_TOPT, PSN_TMAX = 7, 8, 9
LEAF_ALLOC, WOOD_ALLOC, FINE_ALLOC, COARSE_ALLOC = 37, 45, 46, 47
RATE_ROWS = (17, 19, 26, 38, 41, 48, 49, 50, 51)             # converted = file value / 365.0
Z_MAX = 6.764     # sqrt(2 ln 2^33)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (any integer arrays of 32-bit values, broadcast against each other) -> uint64 [..., 4]"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], shape).copy() for i in range(4)]
    k = [np.broadcast_to(key[..., i], shape).copy() for i in range(2)]
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + np.uint64(W0)) & MASK32, (k[1] + np.uint64(W1)) & MASK32]
    return np.stack(c, axis=-1)


def normals(seed, draw, stream, member, block):
    """the four normals of ctr = {member, stream, block, draw} under key = {seed & 0xffffffff, seed >> 32} -> (z, r), both
    longdouble [..., 4]: r the radius sqrt(-2 ln u) of the pair the normal belongs to"""
    seed = int(seed) & (2 ** 64 - 1)
    member, stream, block, draw = np.broadcast_arrays(np.asarray(member, dtype=np.uint64), np.asarray(stream, dtype=np.uint64),
                                                      np.asarray(block, dtype=np.uint64), np.asarray(draw, dtype=np.uint64))
    x = philox4x32_10(np.stack([member, stream, block, draw], axis=-1), np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    z = np.zeros(x.shape, dtype=LD)
    r = np.zeros(x.shape, dtype=LD)
    for i in (0, 2):
        u = (x[..., i].astype(LD) + LD(0.5)) * LD(2) ** -32
        v = (x[..., i + 1].astype(LD) + LD(0.5)) * LD(2) ** -32
        rad = np.sqrt(LD(-2) * np.log(u))
        z[..., i] = rad * np.cos(LD(2) * PI * v)
        z[..., i + 1] = rad * np.sin(LD(2) * PI * v)
        r[..., i] = r[..., i + 1] = rad
    return z, r


def param_normal(seed, draw, stream, member, k):
    """(z, r) of listed parameter k: normal k & 3 of block k >> 2"""
    z, r = normals(seed, draw, stream, member, k >> 2)
    return z[..., k & 3], r[..., k & 3]


def pool_normal(seed, draw, stream, member, p):
    """(z, r) of state slot p: normal p & 3 of block 4 + (p >> 2)"""
    z, r = normals(seed, draw, stream, member, 4 + (p >> 2))
    return z[..., p & 3], r[..., p & 3]


def liu_west_shrink(delta):
    return (3.0 * delta - 1.0) / (2.0 * delta)


def converted_bounds(params):
    """[(row, lo, hi)] in file units -> lo, hi in converted units (the nine rate rows / 365.0)"""
    lo = np.array([(l / 365.0 if row in RATE_ROWS else l) for row, l, _ in params])
    hi = np.array([(h / 365.0 if row in RATE_ROWS else h) for row, _, h in params])
    return lo, hi


def site_code(s, n_params, shrink, mask, pool_sd, site_total):
    if site_total is not None and not site_total[s] > 0:
        return NOT_SELECTED
    if n_params > 0 and not (shrink[s] > 0.0 and shrink[s] <= 1.0):
        return BAD_INPUT
    for p in range(NPOOLS):
        if mask >> p & 1 and not (pool_sd[s, p] >= 0.0 and np.isfinite(pool_sd[s, p])):
            return BAD_INPUT
    return DONE


def move(x, a, z):
    """the Liu-West move of one row's live values x (longdouble) -> (x' before the limits, m, sd, h)"""
    n = len(x)
    m = x.sum() / LD(n)
    sd = np.sqrt(((x - m) ** 2).sum() / LD(n - 1))
    h = np.sqrt((LD(1) - LD(a)) * (LD(1) + LD(a)))
    return (m + LD(a) * (x - m)) + h * sd * z, m, sd, h


def reflect_clip(v, lo, hi):
    v = np.where(v < lo, lo + (lo - v), np.where(v > hi, hi - (v - hi), v))
    return np.minimum(np.maximum(v, lo), hi)


def rejuvenate(state, prm, site_status, n_sites, params, shrink, mask, pool_sd, seed, draw, streams=None, site_total=None):
    """state [ncol][32], prm [ncol][80] (converted rows), site_status [n_sites], params [(row, lo, hi)] (file units), shrink
    [n_sites] or None, mask and pool_sd [n_sites][13] (None with mask 0) -> (state', prm', info [n_sites][4], tol_state
    [ncol][13], tol_prm [ncol][80], margin [ncol]).  tol_*: 2^-53 x the scale of the comparison's bound for that value --
    (n + 16) (mean|x| + |x| + h sd r) for a listed row, 16 (|x| + q r) for a slot --, 0 where nothing may differ.  margin: the
    smallest distance of a member's allocation and biomass decisions from their thresholds over the sum of the bounds of
    the values that enter it (inf where no decision is taken): above 1, no rounding within the bound can flip it."""
    ncol = state.shape[0]
    M = ncol // n_sites
    rows = [r for r, _, _ in params]
    lo, hi = converted_bounds(params)
    shrink = None if shrink is None else np.asarray(shrink, dtype=np.float64).reshape(n_sites)
    pool_sd = None if pool_sd is None else np.asarray(pool_sd, dtype=np.float64).reshape(n_sites, NPOOLS)
    out_state, out_prm = state.copy(), prm.copy()
    info = np.zeros((n_sites, INFO_WORDS), dtype=np.int32)
    tol_state = np.zeros((ncol, NPOOLS))
    tol_prm = np.zeros((ncol, 80))
    margin = np.full(ncol, np.inf)
    eps = 2.0 ** -53
    for s in range(n_sites):
        cols = np.arange(s * M, (s + 1) * M)
        live = cols[(state[cols, 29] == 0)] if site_status[s] == 0 else cols[:0]
        n = len(live)
        code = site_code(s, len(params), shrink, mask, pool_sd, site_total)
        if code == DONE and n < 2:
            code = TOO_FEW
        info[s] = (code, 0, n, 0)
        if code != DONE:
            continue
        member = live - s * M
        stream = s if streams is None else int(streams[s])
        a = shrink[s] if params else 1.0
        move_rows = bool(params) and a != 1.0
        ok = np.ones(n, dtype=bool)
        new_prm = {}
        bound = {}
        if move_rows:
            for k, row in enumerate(rows):
                x = prm[live, row].astype(LD)
                z, r = param_normal(seed, draw, stream, member, k)
                v, m, sd, h = move(x, a, z)
                v = reflect_clip(v, LD(lo[k]), LD(hi[k]))
                ok &= np.isfinite(v.astype(np.float64))
                new_prm[row] = v.astype(np.float64)
                bound[row] = (n + 16) * eps * (np.abs(x).mean() + np.abs(x) + h * sd * r).astype(np.float64)
        perturbed = len(rows) if move_rows else 0
        new_pool = {}
        pbound = {}
        for p in range(NPOOLS):
            if not (mask >> p & 1) or not pool_sd[s, p] > 0.0:
                continue
            perturbed += 1
            x = state[live, p].astype(LD)
            z, r = pool_normal(seed, draw, stream, member, p)
            v = x + LD(pool_sd[s, p]) * z
            if p != DELTA:
                v = np.maximum(v, LD(0))
            ok &= np.isfinite(v.astype(np.float64))
            new_pool[p] = v.astype(np.float64)
            pbound[p] = 16 * eps * (np.abs(x) + LD(pool_sd[s, p]) * r).astype(np.float64)

        def pool(p):
            return new_pool[p] if p in new_pool else state[live, p]

        def pool_tol(p):
            return pbound[p] if p in pbound else np.zeros(n)

        def thresholds(values_and_tols):
            """min over the decisions of |value - threshold| / (sum of the entering bounds), inf where that sum is 0"""
            worst = np.full(n, np.inf)
            for dist, tol in values_and_tols:
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(tol > 0, np.abs(dist) / tol, np.inf)
                worst = np.minimum(worst, ratio)
            return worst

        wood, delta, fine, coarse = pool(WOOD), pool(DELTA), pool(FINE_ROOT), pool(COARSE_ROOT)
        ok &= (wood > TINY) & (wood + delta > TINY) & (fine + coarse > TINY)
        decisions = [(wood - TINY, pool_tol(WOOD)), (wood + delta - TINY, pool_tol(WOOD) + pool_tol(DELTA)),
                     (fine + coarse - TINY, pool_tol(FINE_ROOT) + pool_tol(COARSE_ROOT))]
        if move_rows and any(r in rows for r in (LEAF_ALLOC, WOOD_ALLOC, FINE_ALLOC)):
            al = [new_prm.get(r, prm[live, r]) for r in (LEAF_ALLOC, WOOD_ALLOC, FINE_ALLOC)]
            at = [bound.get(r, np.zeros(n)) for r in (LEAF_ALLOC, WOOD_ALLOC, FINE_ALLOC)]
            rest = 1 - al[0] - al[1] - al[2]
            ok &= ~((al[0] >= 1.0) | (al[1] >= 1.0) | (al[2] >= 1.0) | (rest < 0))
            decisions += [(1.0 - al[i], at[i]) for i in range(3)] + [(rest, at[0] + at[1] + at[2] + 4 * eps)]
        margin[live] = thresholds(decisions)
        w = live[ok]
        for row, v in new_prm.items():
            out_prm[w, row] = v[ok]
            tol_prm[w, row] = bound[row][ok]
        for p, v in new_pool.items():
            out_state[w, p] = v[ok]
            tol_state[w, p] = pbound[p][ok]
        if move_rows and (PSN_TOPT in rows or PSN_TMIN in rows):
            opt, tmin = out_prm[w, PSN_TOPT], out_prm[w, PSN_TMIN]
            out_prm[w, PSN_TMAX] = opt + (opt - tmin)
            tol_prm[w, PSN_TMAX] = 2 * tol_prm[w, PSN_TOPT] + tol_prm[w, PSN_TMIN] + 4 * eps * (np.abs(opt) + np.abs(tmin))
        if move_rows and any(r in rows for r in (LEAF_ALLOC, WOOD_ALLOC, FINE_ALLOC)):
            out_prm[w, COARSE_ALLOC] = 1 - out_prm[w, LEAF_ALLOC] - out_prm[w, WOOD_ALLOC] - out_prm[w, FINE_ALLOC]
            tol_prm[w, COARSE_ALLOC] = tol_prm[w, LEAF_ALLOC] + tol_prm[w, WOOD_ALLOC] + tol_prm[w, FINE_ALLOC] + 4 * eps
        info[s] = (DONE, perturbed, n, n - int(ok.sum()))
    return out_state, out_prm, info, tol_state, tol_prm, margin
