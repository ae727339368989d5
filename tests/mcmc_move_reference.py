"""Reference for sipnet_batch_mcmc_propose / sipnet_batch_mcmc_accept (no GPU, no library): the differential-evolution
proposal of one half of every site from partners of the other half, the tests that keep a proposal from being made, the accept
/ restore step and the info words, in np.longdouble on (state, params) arrays as Batch.get_state / get_params return them,
restated from include/sipnet_amd.h.  Philox and the normals are tests/pf_rejuvenate_reference.py's.  chain() runs the whole
sampler on the CPU against a callable log-density."""
import numpy as np

from tests import pf_rejuvenate_reference as rr

LD = np.longdouble
EPS = 2.0 ** -53
INFO_WORDS = 4
DONE, TOO_FEW, BAD_INPUT, NOT_SELECTED = 1, 0, -2, -3
BLOCK, JITTER_BLOCK = 8, 12
ALLOC = (rr.LEAF_ALLOC, rr.WOOD_ALLOC, rr.FINE_ALLOC)


def draws(seed, draw, stream, member, n_other):
    """the member's Philox call ctr = {member, stream, 8, draw} -> (i1, i2 int64, u longdouble): the ranks of its two
    partners among n_other, and the accept step's uniform (x2 + 0.5) 2^-32"""
    seed = int(seed) & (2 ** 64 - 1)
    member = np.asarray(member, dtype=np.uint64)
    ctr = np.stack(np.broadcast_arrays(member, np.uint64(int(stream) & 0xFFFFFFFF), np.uint64(BLOCK),
                                       np.uint64(int(draw) & 0xFFFFFFFF)), axis=-1)
    x = rr.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    n = np.uint64(n_other)
    i1 = (x[..., 0] * n) >> np.uint64(32)
    i2 = (x[..., 1] * (n - np.uint64(1))) >> np.uint64(32)
    i2 = i2 + (i2 >= i1).astype(np.uint64)
    u = (x[..., 2].astype(LD) + LD(0.5)) * LD(2) ** -32
    return i1.astype(np.int64), i2.astype(np.int64), u


def demc_gamma(n_params):
    return 2.38 / np.sqrt(2.0 * n_params)


def propose_code(s, gamma, jitter, site_total):
    if site_total is not None and not site_total[s] > 0:
        return NOT_SELECTED
    if not np.isfinite(gamma[s]):
        return BAD_INPUT
    if jitter is not None and not (jitter[s] >= 0.0 and np.isfinite(jitter[s])):
        return BAD_INPUT
    return DONE


def _derive(out_prm, tol_prm, w, rows):
    """psnTMax and coarseRootAllocation of the columns w from the rows they derive from, by the conversion's expressions"""
    if rr.PSN_TOPT in rows or rr.PSN_TMIN in rows:
        opt, tmin = out_prm[w, rr.PSN_TOPT], out_prm[w, rr.PSN_TMIN]
        out_prm[w, rr.PSN_TMAX] = opt + (opt - tmin)
        if tol_prm is not None:
            tol_prm[w, rr.PSN_TMAX] = 2 * tol_prm[w, rr.PSN_TOPT] + tol_prm[w, rr.PSN_TMIN] + 4 * EPS * (np.abs(opt) + np.abs(tmin))
    if any(r in rows for r in ALLOC):
        out_prm[w, rr.COARSE_ALLOC] = 1 - out_prm[w, rr.LEAF_ALLOC] - out_prm[w, rr.WOOD_ALLOC] - out_prm[w, rr.FINE_ALLOC]
        if tol_prm is not None:
            tol_prm[w, rr.COARSE_ALLOC] = tol_prm[w, rr.LEAF_ALLOC] + tol_prm[w, rr.WOOD_ALLOC] + tol_prm[w, rr.FINE_ALLOC] + 4 * EPS


def _ratio(dist, tol):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tol > 0, np.abs(dist) / tol, np.inf)


def propose(state, prm, site_status, n_sites, params, gamma, jitter, half, seed, draw, streams=None, site_total=None):
    """state [ncol][32], prm [ncol][80] (converted rows), params [(row, lo, hi)] (file units), gamma [n_sites], jitter
    [n_sites] or None -> (prm', saved [n_params][ncol] (NaN where nothing was saved), moved [ncol] int32, info [n_sites][4],
    tol_prm [ncol][80], margin [ncol]).
    tol_prm: the bound of the comparison, derived and not measured: a new value is x_j + gamma (x_r1 - x_r2) + (w (hi - lo)) z,
    a handful of roundings each relative to one of its terms (fused or not), so 8 x 2^-53 (|x_j| + |gamma| (|x_r1| + |x_r2|) +
    w (hi - lo) |z|), plus the device normal's own 8 x 2^-53 r scaled by w (hi - lo); 0 where nothing may differ.
    margin: per member the smallest distance of a decision (each bound test, the allocation test) from its threshold over
    the bound of the value that enters it; inf where no decision is taken.  Above 1 no rounding within the bound flips it."""
    ncol = state.shape[0]
    M = ncol // n_sites
    rows = [r for r, _, _ in params]
    lo, hi = rr.converted_bounds(params)
    gamma = np.asarray(gamma, dtype=np.float64).reshape(n_sites)
    jitter = None if jitter is None else np.asarray(jitter, dtype=np.float64).reshape(n_sites)
    out_prm = prm.copy()
    saved = np.full((len(params), ncol), np.nan)
    moved = np.zeros(ncol, dtype=np.int32)
    info = np.zeros((n_sites, INFO_WORDS), dtype=np.int32)
    tol_prm = np.zeros((ncol, 80))
    margin = np.full(ncol, np.inf)
    j = np.arange(M)
    for s in range(n_sites):
        live = (state[s * M:(s + 1) * M, 29] == 0) & (site_status[s] == 0)
        A, B = j[live & ((j & 1) == half)], j[live & ((j & 1) != half)]
        nA, nB = len(A), len(B)
        code = propose_code(s, gamma, jitter, site_total)
        if code == DONE and nB < 2:
            code = TOO_FEW
        info[s] = (code, 0, nA, nB)
        if code != DONE or nA == 0:
            continue
        stream = s if streams is None else int(streams[s])
        i1, i2, _ = draws(seed, draw, stream, A, nB)
        assert (i1 != i2).all() and (i1 < nB).all() and (i2 < nB).all()
        cj, c1, c2 = s * M + A, s * M + B[i1], s * M + B[i2]
        g, w = LD(gamma[s]), (0.0 if jitter is None else float(jitter[s]))
        ok = np.ones(nA, dtype=bool)
        worst = np.full(nA, np.inf)
        new, bound = {}, {}
        for k, row in enumerate(rows):
            xj, x1, x2 = prm[cj, row].astype(LD), prm[c1, row].astype(LD), prm[c2, row].astype(LD)
            v = xj + g * (x1 - x2)
            tol = 8 * EPS * (np.abs(xj) + abs(g) * (np.abs(x1) + np.abs(x2)))
            if w > 0.0:
                z, r = rr.normals(seed, draw, stream, A, JITTER_BLOCK + (k >> 2))
                span = LD(w) * (LD(hi[k]) - LD(lo[k]))
                v = v + span * z[..., k & 3]
                tol = tol + 8 * EPS * span * (np.abs(z[..., k & 3]) + r[..., k & 3])
            tol = tol.astype(np.float64)
            v64 = v.astype(np.float64)
            ok &= np.isfinite(v64) & np.asarray(v >= LD(lo[k])) & np.asarray(v <= LD(hi[k]))
            worst = np.minimum(worst, np.minimum(_ratio((v - LD(lo[k])).astype(np.float64), tol),
                                                 _ratio((LD(hi[k]) - v).astype(np.float64), tol)))
            new[row], bound[row] = v64, tol
        if any(r in rows for r in ALLOC):
            al = [new.get(r, prm[cj, r]) for r in ALLOC]
            at = [bound.get(r, np.zeros(nA)) for r in ALLOC]
            rest = 1 - al[0] - al[1] - al[2]
            ok &= ~((al[0] >= 1.0) | (al[1] >= 1.0) | (al[2] >= 1.0) | (rest < 0))
            for dist, tol in [(1.0 - al[i], at[i]) for i in range(3)] + [(rest, at[0] + at[1] + at[2] + 4 * EPS)]:
                worst = np.minimum(worst, _ratio(dist, tol))
        margin[cj] = worst
        wcols = cj[ok]
        for k, row in enumerate(rows):
            saved[k, wcols] = prm[wcols, row]
            out_prm[wcols, row] = new[row][ok]
            tol_prm[wcols, row] = bound[row][ok]
        _derive(out_prm, tol_prm, wcols, rows)
        moved[wcols] = 1
        info[s] = (DONE, int(ok.sum()), nA, nB)
    return out_prm, saved, moved, info, tol_prm, margin


def accept(state, prm, site_status, n_sites, params, saved, moved, logp_new, logp_cur, beta, seed, draw, streams=None):
    """the accept step on prm [ncol][80] as it stands after the proposal (and whatever ran since) -> (prm', moved', logp_cur',
    info [n_sites][4], margin [ncol], accepted [ncol] bool).  A rejected column gets its listed rows back from saved and its
    derived rows derived again, in doubles: nothing to round, so no tolerance.  margin: |beta (new - cur) - log u| over
    8 x 2^-53 (|beta (new - cur)| + |log u|), inf where the comparison is decided by an infinity or a NaN."""
    ncol = state.shape[0]
    M = ncol // n_sites
    rows = [r for r, _, _ in params]
    beta = None if beta is None else np.asarray(beta, dtype=np.float64).reshape(n_sites)
    out_prm, out_moved, out_cur = prm.copy(), np.asarray(moved).copy(), np.asarray(logp_cur, dtype=np.float64).copy()
    info = np.zeros((n_sites, INFO_WORDS), dtype=np.int32)
    margin = np.full(ncol, np.inf)
    accepted = np.zeros(ncol, dtype=bool)
    for s in range(n_sites):
        cols = np.arange(s * M, (s + 1) * M)
        n = int(((state[cols, 29] == 0) & (site_status[s] == 0)).sum())
        if beta is not None and not (beta[s] > 0.0 and np.isfinite(beta[s])):
            info[s] = (BAD_INPUT, 0, 0, n)
            continue
        idx = cols[np.asarray(moved)[cols] == 1]
        stream = s if streams is None else int(streams[s])
        _, _, u = draws(seed, draw, stream, idx - s * M, 2)
        new, cur = np.asarray(logp_new, dtype=np.float64)[idx], out_cur[idx]
        with np.errstate(invalid="ignore", over="ignore"):
            lhs = (LD(1.0) if beta is None else LD(beta[s])) * (new.astype(LD) - cur.astype(LD))
            logu = np.log(u)
            acc = np.asarray(new < np.inf) & np.asarray(lhs > logu)
            m = np.where(np.isfinite(lhs.astype(np.float64)),
                         np.abs(lhs - logu) / (8 * EPS * (np.abs(lhs) + np.abs(logu))), np.inf).astype(np.float64)
        margin[idx] = m
        accepted[idx] = acc
        out_cur[idx[acc]] = new[acc]
        back = idx[~acc]
        for k, row in enumerate(rows):
            out_prm[back, row] = saved[k, back]
        _derive(out_prm, None, back, rows)
        out_moved[idx] = 0
        info[s] = (DONE, len(idx), int(acc.sum()), n)
    return out_prm, out_moved, out_cur, info, margin, accepted


def chain(logdens, x0, lo, hi, gamma, jitter, sweeps, seed, stream=0, rows=(4, 11)):
    """the whole sampler on the CPU: one site whose M members start at x0 [M][d], `sweeps` full sweeps (half 0, then half 1;
    half-sweep `it` uses half = it & 1 and draw = it), the target logdens(x [n][d]) -> [n] on the box [lo, hi] ->
    (samples [sweeps][M][d] after each full sweep, acceptance rate of the proposals made).  The d moved rows are `rows` of a
    [M][80] parameter array (rows whose converted value is the file value, none of them derived from)."""
    x0 = np.asarray(x0, dtype=np.float64)
    M, d = x0.shape
    rows = list(rows)[:d]
    assert len(rows) == d and not set(rows) & set(rr.RATE_ROWS)
    params = [(rows[k], float(lo[k]), float(hi[k])) for k in range(d)]
    state = np.zeros((M, 32))
    prm = np.zeros((M, 80))
    prm[:, rows] = x0
    status = np.zeros(1)
    cur = np.asarray(logdens(prm[:, rows]), dtype=np.float64)
    out = np.zeros((sweeps, M, d))
    made = taken = 0
    for it in range(2 * sweeps):
        prop, saved, moved, _, _, _ = propose(state, prm, status, 1, params, [gamma], None if jitter is None else [jitter],
                                              it & 1, seed, it, streams=[stream])
        new = np.asarray(logdens(prop[:, rows]), dtype=np.float64)
        prm, _, cur, info, _, _ = accept(state, prop, status, 1, params, saved, moved, new, cur, None, seed, it, streams=[stream])
        made += int(info[0, 1])
        taken += int(info[0, 2])
        if it & 1:
            out[it >> 1] = prm[:, rows]
    return out, taken / max(made, 1)
