"""The weighted order statistics (sipnet_batch_plane_quantiles_weighted: wquantSiteKernel, wquantSortKernel, wquantSelectKernel
of quantiles_weighted.h) at their value, score and size edges, against tests/wquantile_reference.py.

Everywhere: the reference starts from the device's integers after check_integers has held them to weights_of; quantiles, n,
S, codes, rank sums and (where the exact value is further from a half than the tolerance) the integers are compared for
equality; moments and CRPS are held to the bounds derived in the docstring of tests/test_gpu_wquantiles.py
(wr.moments_bounds, wr.crps_bound), and both paths are forced where the size allows (tests/wquantile_gpu_common.py: analyse).

A  the sort path between its tested sizes: P = 2048, 4096 and 8192 on both sides of the powers of two (per = 8, 16, 32
   sorted elements a thread; at 4096 two passes of the eight-element register batch and of the four-pair LDS loop).
B  special values: zeros of both signs, infinities, denormals, a large mean, large magnitudes, equal values, a NaN.
   Two allowances, both the issue's: the moments and the CRPS of a cell with an infinite value under weight are recorded, not
   asserted (the contract is silent); the two denormal rows add wr.denormal_allowance(n) = (2 n + 8) 2^-1074 to the mean's and
   the CRPS's bounds, and their m2 must be exactly 0 where the true one is below every double (the row k * 5e-324: a squared
   deviation underflows.  The row k * 2^-149 holds normal doubles: its m2 is about 1e-78 and is held to its relative bound).
   The large-magnitude row is 1e140 z in doubles and 1e30 z in floats (1e140 is no float).
C  every kind of observation, beside a site of code 1 and a site of code -2.
D  the quantile list: unsorted, repeated, sixteen distinct, sixteen of which several share a target; T = 1 on a member of
   integer weight 1; one member at 2^30 among members at 1; equal weights against numpy's "inverted_cdf"; the rows of
   d_quant past n_q and the optional outputs of the C entry point.
E  the selection path alone: 65 537 members, and 2 x 2 097 152 float members (the column limit; S = 2^51 at equal weights).
F  a forecast's NEE plane, run_sums' daily sums and a smoothed series under log-weights from series_loglik carried past a
   pf_resample_sites that kept one site and resampled the others.
G  a site's outputs do not depend on its neighbours; two different calls on one batch without a synchronisation between
   them, on the current stream and on another one.

Every test prints the largest fraction of each bound it met as `wq-edges <group>: mean, m2, crps`."""
import ctypes as C

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib, synth
from sipnet_amd.config import param_index as pi
from tests import pf_edges_reference as er
from tests import wquantile_reference as wr
from tests.enkf_gpu_common import ANALYSED, BASE, DEV, bits, carried_params, observe, operators, sites_batch
from tests.wquantile_gpu_common import (G, Q6, SELECT, SORT, Worst, analyse, bare, dev, host_of, on_device, random_logw, same, same_bits,
                                        same_outputs, widened)

pytestmark = pytest.mark.gpu
DTYPES = [(torch.float64, "f64"), (torch.float32, "f32")]
Q16 = [0.61, 0.07, 0.999, 0.33, 0.0, 0.5, 0.25, 1.0, 0.001, 0.75, 0.9, 0.42, 0.975, 0.025, 0.13, 0.8]


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


def a_weight_in_every_site(logw, n_sites, M, rng, value=-699.0):
    logw[np.arange(n_sites) * M + rng.integers(0, M, n_sites)] = value
    return logw


# ---- A: the sort path between its tested sizes ------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2047, 2048, 2049, 4095, 4096, 4097, 8191])
def test_the_sort_path_between_its_tested_sizes(M):
    n_sites, rows = (3 if M <= 2049 else 2), 2
    rng = np.random.default_rng(900 + M)
    worst = Worst(f"A M={M}")
    b = bare(n_sites, M)
    host = rng.normal(size=(rows, n_sites * M)) * 3.0 - 1.0
    host[:, ::7] = np.round(host[:, ::7])                                # some ties
    logw = a_weight_in_every_site(random_logw(rng, n_sites * M), n_sites, M, rng)
    # (the pairwise CRPS costs seconds a cell from 4095 members on: one cell per size there)
    crps_cells = None if M <= 2049 else {(1, n_sites - 1)}
    for dtype, pad in ((torch.float64, 0), (torch.float32, 5), (torch.float64, 3)):
        x = widened(host, dtype)
        obs = x[:, rng.integers(0, M, n_sites) + M * np.arange(n_sites)].copy()      # a member's value: a tie with y
        obs[0, 0] += 0.37
        analyse(b, host, logw, Q6, obs, dtype, pad, crps_cells=crps_cells, worst=worst, what=(M, dtype, pad))
    b.close()
    worst.report()


# ---- B: special values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tname", DTYPES, ids=[d[1] for d in DTYPES])
@pytest.mark.parametrize("M", [257, 1000])
def test_special_values(M, dtype, tname):
    n_sites = 3
    rng = np.random.default_rng(700 + M)
    logw = rng.normal(size=n_sites * M) * 2.0
    logw[rng.random(n_sites * M) < 0.1] = -np.inf                        # about a tenth weighs nothing
    for s in range(n_sites):
        logw[s * M + 1] = -np.inf
        logw[[s * M, s * M + 2]] = [-0.5, 0.25]
    weighs = np.isfinite(logw)                                           # (within 21.5 of the maximum, all of them)
    host, obs = wr.special_rows(rng, n_sites, M, dtype == torch.float32, weighs)
    row = {name: r for r, name in enumerate(wr.SPECIAL_ROWS)}
    b = bare(n_sites, M)
    worst = Worst(f"B M={M} {tname}")
    got, want = analyse(b, host, logw, Q6, obs, dtype, denormal_rows=wr.DENORMAL_ROWS, worst=worst, what=(M, tname))
    assert ((got.fixed > 0) == weighs).all()
    S = got.site[:, 0]
    both = {SORT: got, SELECT: host_of(b.plane_quantiles_weighted(on_device(host, dtype), dev(logw), Q6, live_only=False, obs=obs,
                                                                    want_moments=True, path=SELECT))}
    b.close()
    # the zeros: one key, so every member ties with y = +0.0; the sums of +-0.0 are zeros
    r = row["zeros"]
    assert (got.quant[:, r] == 0.0).all() and (got.rank[r, :, 0] == 0).all() and (got.rank[r, :, 1] == S).all()
    assert (got.moments[r] == 0.0).all() and (got.crps[r] == 0.0).all()
    r = row["zeros among others"]
    x = host[r].reshape(n_sites, M)
    assert (np.signbit(x) & (x == 0.0)).any() and (~np.signbit(x) & (x == 0.0)).any()
    np.testing.assert_array_equal(got.rank[r, :, 1], [got.fixed[s * M:(s + 1) * M][x[s] == 0.0].sum() for s in range(n_sites)])
    # the infinities: site 0 holds both under weight, the last site only under weight 0
    r = row["infinities"]
    assert got.quant[0, r, 0] == -np.inf and got.quant[1, r, 0] == np.inf and np.isfinite(got.quant[:, r, n_sites - 1]).all()
    assert got.quant[1, r, 1] == np.inf and np.isfinite(got.quant[0, r, 1])                    # site 1: only +inf under weight
    xs = host[r, :M]
    assert got.rank[r, 0, 0] == got.fixed[:M][xs < obs[r, 0]].sum() >= got.fixed[:M][xs == -np.inf].sum() > 0
    for path, g in both.items():
        for s in range(n_sites):
            xw = host[r, s * M:(s + 1) * M][got.fixed[s * M:(s + 1) * M] > 0]
            if not np.isfinite(xw).all():
                print("wq-edges B infinite values under weight (recorded, not asserted): M=%d %s path %d site %d: +inf x %d, -inf x %d"
                      " -> mean %r m2 %r crps %r" % (M, tname, path, s, (xw == np.inf).sum(), (xw == -np.inf).sum(), g.moments[r, s, 0],
                                                     g.moments[r, s, 1], None if g.crps is None else g.crps[r, s]))
    r = row["denormals"]
    if dtype == torch.float64:
        assert (host[r] > 0.0).all() and (host[r] < 2.0 ** -1022).all() and (got.moments[r, :, 1] == 0.0).all()
        assert (got.moments[r, :, 0] > 0.0).all() and (got.quant[:, r] > 0.0).all()
    else:
        assert (host[r] == 0.0).all()                                    # (5e-324 is no float: the row reads as zeros)
    r = row["float denormals"]
    assert (host[r] > 0.0).all() and (host[r] < 2.0 ** -126).all() and (got.moments[r, :, 1] > 0.0).all()
    r = row["equal values"]
    assert (got.quant[:, r] == host[r, 0]).all() and (got.rank[r, :, 0] == 0).all() and (got.rank[r, :, 1] == S).all()
    r = row["nan"]
    assert want[3][r].tolist() == [False, True, False] and got.rank[r, 1].tolist() == [-1, -1] and np.isnan(got.quant[:, r, 1]).all()
    worst.report()


# ---- C: scores and their codes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 257, 1000])
def test_scores_and_their_codes(M):
    """sites 0 and 1: weights with zeros among them; site 2: only -inf log-weights (code 1); site 3: a +inf log-weight (code -2)"""
    n_sites = 4
    rng = np.random.default_rng(600 + M)
    logw = rng.normal(size=n_sites * M) * 2.0
    logw[1::4] = -np.inf
    logw[[0, M, M + M - 1]] = [0.5, 0.7, 0.1]
    logw[2 * M:3 * M] = -np.inf
    logw[4 * M - 1] = np.inf
    if M > 3:
        logw[2 * M + 5] = np.nan
    weighs = np.isfinite(logw[:M]), np.isfinite(logw[M:2 * M])
    parts = [wr.score_rows(rng, M, weighs[s % 2]) for s in range(n_sites)]
    host = np.concatenate([p[0] for p in parts], axis=1)
    obs = np.stack([p[1] for p in parts], axis=1)
    row = {name: r for r, name in enumerate(wr.OBS_KINDS)}
    b = bare(n_sites, M)
    worst = Worst(f"C M={M}")
    got, want = analyse(b, host, logw, Q6, obs, worst=worst, what=M)     # (the reference's cell() decides everything)
    assert got.site[:, 2].tolist() == [0, 0, 1, -2] and got.site[2:, :2].tolist() == [[0, 0], [0, 0]]
    S = got.site[:2, 0]
    series, lw = on_device(host), dev(logw)
    for path in (SORT, SELECT):
        g = host_of(b.plane_quantiles_weighted(series, lw, Q6, live_only=False, obs=obs, want_crps=path == SORT, want_moments=True,
                                               path=path))
        bare_ = host_of(b.plane_quantiles_weighted(series, lw, Q6, live_only=False, want_moments=True, path=path))
        assert bare_.rank is None and bare_.crps is None
        np.testing.assert_array_equal(g.rank[row["below"], :2], [[0, 0], [0, 0]])
        np.testing.assert_array_equal(g.rank[row["above"], :2], np.stack([S, [0, 0]], axis=1))
        assert (g.rank[row["tied"], :2, 1] > 0).all() and (g.rank[row["+0 against -0"], :2, 1] > 0).all()
        assert (g.rank[row["ties weight 0 only"], :2, 1] == 0).all()
        for name in ("inside", "inside, mean 1e6"):
            assert (g.rank[row[name], :2, 0] > 0).all() and (g.rank[row[name], :2, 0] < S).all() and np.isfinite(g.moments[row[name], :2]).all()
        # y NaN: not scored, quantiles and moments as without an observation -- the same bits as the call without one
        r = row["nan"]
        assert (g.rank[r, :2] == -1).all() and (path != SORT or np.isnan(g.crps[r]).all())
        same_bits(g.quant[:, r], bare_.quant[:, r], (path, "quant under a NaN observation"))
        same_bits(g.moments[r], bare_.moments[r], (path, "moments under a NaN observation"))
        assert np.isfinite(g.quant[:, r, :2]).all() and np.isfinite(g.moments[r, :2]).all()
        # every other finite row is untouched by its neighbours' observations too
        finite = [k for k, name in enumerate(wr.OBS_KINDS) if name not in ("+inf", "-inf")]
        same_bits(g.quant[:, finite], bare_.quant[:, finite], path)
        same_bits(g.moments[finite], bare_.moments[finite], path)
        for name in ("+inf", "-inf"):
            r = row[name]
            assert (g.rank[r, :2] == -2).all() and np.isnan(g.quant[:, r]).all() and np.isnan(g.moments[r]).all()
            assert path != SORT or np.isnan(g.crps[r]).all()
        # the sites' codes go before the observation's: code 1 gives {0, 0}, code -2 gives {-2, -2}, whatever y is
        assert (g.rank[:, 2] == 0).all() and (g.rank[:, 3] == -2).all()
        assert np.isnan(g.quant[:, :, 2:]).all() and np.isnan(g.moments[:, 2:]).all() and (path != SORT or np.isnan(g.crps[:, 2:]).all())
    b.close()
    worst.report()


# ---- D: the quantile list and the targets -----------------------------------------------------------------------------------
def colliding(S, n=16):
    """n different q in (0, 1) of which every group of four shares one target T of the total S (sa.wquantile_target says so)"""
    out = []
    for q0 in (0.37, 0.052, 0.81, 0.66):
        T = sa.wquantile_target(S, q0)
        group, q = [q0], q0
        while len(group) < 4:
            q = float(np.nextafter(q, 0.0))
            if sa.wquantile_target(S, q) != T:
                break
            group.append(q)
        assert len(group) == 4 and len(set(group)) == 4, (S, q0)
        out += group
    return [out[(5 * i) % n] for i in range(n)]                          # (not sorted, the groups apart)


@pytest.mark.parametrize("M", [300, 8193])
def test_the_quantile_list_and_the_targets(M):
    n_sites, rows = 3, 2
    paths = (SORT, SELECT) if M == 300 else (SELECT,)
    rng = np.random.default_rng(40 + M)
    worst = Worst(f"D M={M}")
    b = bare(n_sites, M)
    host = np.round(rng.normal(size=(rows, n_sites * M)) * 3.0, 2)
    obs = host[:, [7, M + 7, 2 * M + 7]].copy()
    logw = a_weight_in_every_site(random_logw(rng, n_sites * M), n_sites, M, rng)
    crps_cells = None if M == 300 else set()
    got, _ = analyse(b, host, logw, [0.9, 0.1, 0.5, 0.9, 0.0, 0.5, 1.0, 0.1], obs, paths=paths, worst=worst,
                     what="unsorted and repeated")
    np.testing.assert_array_equal(bits(got.quant[[0, 1, 2]]), bits(got.quant[[3, 7, 5]]))
    got, _ = analyse(b, host, logw, Q16, obs, paths=paths, crps_cells=crps_cells, worst=worst, what="sixteen distinct")
    assert len(set(Q16)) == 16 and len({sa.wquantile_target(int(got.site[0, 0]), q) for q in Q16}) == 16
    S0 = int(got.site[0, 0])
    q_same = colliding(S0)
    assert len(set(q_same)) == 16 and len({sa.wquantile_target(S0, q) for q in q_same}) == 4        # (at site 0: four targets)
    got, _ = analyse(b, host, logw, q_same, obs, paths=paths, crps_cells=crps_cells, worst=worst, what="sixteen, four targets")
    groups = {}
    for k, q in enumerate(q_same):
        groups.setdefault(sa.wquantile_target(S0, q), []).append(k)
    for ks in groups.values():
        for k in ks[1:]:
            np.testing.assert_array_equal(bits(got.quant[k, :, 0]), bits(got.quant[ks[0], :, 0]))

    # T = 1: the smallest value under weight belongs to a member of integer weight 1
    lw_one = np.zeros(n_sites * M)
    j0 = np.arange(n_sites) * M + np.array([0, M // 2, M - 1])
    lw_one[j0] = er.LW_OF[1]
    x_one = host.copy()
    x_one[:, j0] = -50.0
    q_one = [0.0, 1e-300, 1e-13, 0.5, 1.0]
    got, _ = analyse(b, x_one, lw_one, q_one, np.full((rows, n_sites), -50.0), paths=paths, crps_cells=crps_cells, worst=worst,
                     what="T = 1")
    assert (got.fixed[j0] == 1).all() and (got.site[:, 0] == (M - 1) * G + 1).all()
    assert [sa.wquantile_target(int(got.site[0, 0]), q) for q in q_one[:3]] == [1, 1, 1]
    assert (got.quant[:3] == -50.0).all() and (got.quant[3:] > -50.0).all() and (got.rank == [0, 1]).all()

    # one member at G, every other at weight 1, the values 0 .. M - 1, the heavy member holds the value M // 2: k = M // 2 light
    # members lie below it, so T <= k reads the T-th light value, k < T <= k + G the heavy member's, T > k + G the light
    # members above it.  With S = G + M - 1 that leaves the heavy member every q from about k / 2^30 to 1 - (M - 1 - k) / 2^30
    h = np.arange(n_sites) * M + M // 3
    lw_heavy = np.full(n_sites * M, er.LW_OF[1])
    lw_heavy[h] = 0.0
    x_heavy = np.stack([np.concatenate([rng.permutation(M) for _ in range(n_sites)]) for _ in range(rows)]).astype(np.float64)
    for r in range(rows):
        for s in range(n_sites):
            j = s * M + int(np.flatnonzero(x_heavy[r, s * M:(s + 1) * M] == M // 2)[0])
            x_heavy[r, [j, h[s]]] = x_heavy[r, [h[s], j]]
    q_heavy = [0.0, 1e-9, 1e-6, 1e-5, 0.25, 0.5, 0.75, 1.0 - 1e-5, 1.0 - 1e-7, 1.0 - 1e-10, 1.0]
    got, _ = analyse(b, x_heavy, lw_heavy, q_heavy, np.full((rows, n_sites), float(M // 2)), paths=paths, crps_cells=crps_cells,
                     worst=worst, what="one heavy member")
    assert (got.site[:, 0] == G + M - 1).all() and (got.fixed[h] == G).all() and (np.delete(got.fixed, h) == 1).all()
    assert (got.quant[0] == 0.0).all() and (got.quant[-1] == M - 1.0).all() and (got.quant[1] == 1.0).all()      # T = 1, S, 2
    assert (got.quant[4:8] == M // 2).all() and (got.rank == [M // 2, G]).all()
    assert (got.quant[-2] == M - 1.0).all() and (got.quant[-3] > M // 2).all()

    # equal weights: Hyndman & Fan's type 1 by numpy, which shares no code with the reference
    q_eq = [0.0, 1.0, 0.5] + [(j + 0.5) / M for j in range(3, M, M // 13)][:13]
    assert len(q_eq) == 16
    got, _ = analyse(b, host, np.full(n_sites * M, -3.25), q_eq, obs, paths=paths, crps_cells=crps_cells, worst=worst,
                     what="equal weights")
    assert (got.fixed == G).all()
    for s in range(n_sites):
        same(got.quant[:, :, s], np.quantile(host[:, s * M:(s + 1) * M], q_eq, axis=1, method="inverted_cdf"), s)
    b.close()
    worst.report()


@pytest.mark.parametrize("M", [300, 8193])
def test_what_the_c_entry_point_writes(M):
    """d_quant with sixteen rows: the rows from n_q on keep their fill; an optional output passed as NULL changes no bit of
    the others"""
    L = sa.lib()
    n_sites, rows, n_q = 3, 2, 5
    rng = np.random.default_rng(70 + M)
    b = bare(n_sites, M)
    series = on_device(np.round(rng.normal(size=(rows, n_sites * M)), 2))
    logw = dev(a_weight_in_every_site(random_logw(rng, n_sites * M), n_sites, M, rng))
    obs = dev(rng.normal(size=(rows, n_sites)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    qs = (C.c_double * n_q)(0.5, 0.0, 1.0, 0.3, 0.5)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())

    def call(path, leave=()):
        out = dict(quant=torch.full((16, rows, n_sites), -7.0, dtype=torch.float64, device=DEV),
                   site=torch.full((n_sites, 3), -7, dtype=torch.int64, device=DEV),
                   fixed=torch.full((n_sites * M,), -7, dtype=torch.int64, device=DEV),
                   moments=torch.full((rows, n_sites, 2), -7.0, dtype=torch.float64, device=DEV),
                   crps=torch.full((rows, n_sites), -7.0, dtype=torch.float64, device=DEV) if path == SORT else None,
                   rank=torch.full((rows, n_sites, 2), -7, dtype=torch.int64, device=DEV))
        for name in leave:
            out[name] = None
        y = None if "obs" in leave else obs
        rc = L.sipnet_batch_plane_quantiles_weighted(b.h, ptr(series), 0, rows, n_sites * M, ptr(logw), n_q, qs, 0, path, ptr(out["quant"]),
                                                     ptr(out["site"]), ptr(out["fixed"]), ptr(out["moments"]), ptr(y), ptr(out["crps"]),
                                                     ptr(out["rank"]), stream)
        assert rc == _lib.OK, (L.sipnet_last_error(), path, leave)
        torch.cuda.synchronize()
        return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}

    for path in ((SORT, SELECT) if M == 300 else (SELECT,)):
        full = call(path)
        assert (full["quant"][n_q:] == -7.0).all() and not (full["quant"][:n_q] == -7.0).any()
        assert not (full["site"] == -7).any() and not (full["fixed"] == -7).any() and not (full["moments"] == -7.0).any()
        assert not (full["rank"] == -7).any() and (path != SORT or not (full["crps"] == -7.0).any())
        for leave in (("site",), ("fixed",), ("moments",), ("crps",), ("rank",), ("crps", "rank"), ("crps", "rank", "obs"),
                      ("site", "fixed", "moments", "crps", "rank", "obs")):
            part = call(path, leave)
            for name, x in part.items():
                if x is not None:
                    same_bits(x, full[name], (path, leave, name))
    b.close()


# ---- E: the selection path where it is alone --------------------------------------------------------------------------------
def test_the_selection_path_at_65537_members():
    n_sites, M, rows = 2, 65537, 2
    rng = np.random.default_rng(65537)
    host = rng.normal(size=(rows, n_sites * M)) * 3.0 - 1.0
    host[:, ::7] = np.round(host[:, ::7])
    logw = a_weight_in_every_site(random_logw(rng, n_sites * M), n_sites, M, rng)
    obs = host[:, [11, M + 11]].copy()
    obs[0, 0] += 0.37
    b = bare(n_sites, M)
    worst = Worst(f"E M={M}")
    got, _ = analyse(b, host, logw, Q6, obs, paths=(SELECT,), worst=worst, what=M)
    b.close()
    assert (got.rank >= 0).all() and (got.rank[1, 1, 1] > 0 or got.fixed[M + 11] == 0)
    worst.report()


@pytest.mark.parametrize("weights", ["random", "equal"])
def test_the_selection_path_at_the_column_limit(weights):
    """2 sites x 2 097 152 float members, ncol = 4 194 304: at equal log-weights every integer is 2^30 and S = 2^51, next to
    the 2^52 up to which a total is exact as a double"""
    n_sites, M = 2, 1 << 21
    rng = np.random.default_rng(21)
    host = widened(rng.normal(size=(1, n_sites * M)) * 3.0 - 1.0, torch.float32)
    obs = host[:, [11, M + 11]].copy()
    if weights == "random":
        logw = a_weight_in_every_site(random_logw(rng, n_sites * M), n_sites, M, rng)
    else:
        logw = np.full(n_sites * M, -3.25)
    b = bare(n_sites, M, sa.F32_MIXED)
    assert b.ncol == 4194304
    worst = Worst(f"E column limit, {weights} weights")
    got, _ = analyse(b, host, logw, Q6, obs, torch.float32, paths=(SELECT,), worst=worst, what=weights)
    b.close()
    if weights == "equal":
        assert (got.fixed == G).all() and got.site.tolist() == [[1 << 51, M, 0]] * 2
        for s in range(n_sites):
            xs = host[0, s * M:(s + 1) * M]
            same(got.quant[:, 0, s], np.quantile(xs, Q6, method="inverted_cdf"), s)
            assert got.rank[0, s].tolist() == [int((xs < obs[0, s]).sum()) * G, int((xs == obs[0, s]).sum()) * G]
    worst.report()


# ---- F: real series and the weights of a kept site --------------------------------------------------------------------------
@pytest.mark.parametrize("prec,M", [(sa.F64, 70), (sa.F32_MIXED, 300)], ids=["f64", "f32"])
def test_real_series_under_the_weights_of_a_kept_site(base, prec, M):
    n_sites, steps = 3, 96
    members = synth.perturbed_params(base, n_sites * M, seed=1)
    members[5, pi("leafAllocation")] = 0.9                               # site 0: a member that never runs (status 3)
    members[5, pi("woodAllocation")] = 0.9
    members[M + 9, pi("plantWoodInit")] = 1e-4                           # site 1: a member that starves inside the window
    members[M + 9, pi("laiInit")] = 1e-4
    b = sites_batch(members, n_sites, prec)
    planes = torch.zeros((3, steps, b.ncol), dtype=b.out_dtype, device=DEV)
    b.run(0, steps, planes=planes)
    b2 = sites_batch(members, n_sites, prec)
    sums = b2.run_sums(0, steps, 48)
    b2.close()
    dtype = planes.dtype
    assert dtype == (torch.float32 if prec == sa.F32_MIXED else torch.float64) and sums.dtype == torch.float64
    nee = planes[0].clone()
    st0 = b.get_state()
    used0 = st0[:, 29] == 0
    assert not used0[5] and used0[M + 9] and used0[2 * M:].all()
    ops = operators()
    o, sd = observe(st0, [p.cpu().numpy() for p in planes], carried_params(b), n_sites, ops, np.random.default_rng(5))
    b.enkf_analysis_smooth(o, sd, ops, ANALYSED, [planes], planes=planes)
    smoothed = planes[0]
    assert not torch.equal(smoothed, nee)

    # the window's log-weights, then the step that keeps site 2 (total -3) and resamples sites 0 and 1
    x = nee.double().cpu().numpy().reshape(steps, n_sites, M)
    live = used0.reshape(n_sites, M)
    centre = np.stack([np.median(x[:, s, live[s]], axis=1) for s in range(n_sites)])          # [n_sites][steps]
    spread = np.stack([x[:, s, live[s]].std(axis=1) for s in range(n_sites)]) + 1e-3 * np.abs(centre).mean()
    y_lik = centre + 0.5 * spread * np.random.default_rng(6).standard_normal(centre.shape)
    logw = b.series_loglik([sa.loglik_term(nee, y_lik, 8.0 * spread)])
    lw0 = logw.cpu().numpy().copy()
    assert np.isneginf(lw0[5]) and np.isfinite(lw0[used0]).all()
    first = host_of(b.plane_quantiles_weighted(nee, logw, Q6, live_only=False, return_fixed=True))
    w = first.fixed.reshape(n_sites, M).astype(np.float64)
    ess_host = w.sum(axis=1) ** 2 / (w * w).sum(axis=1)
    ess_min = ess_host * np.array([2.0, 2.0, 0.5])
    total = torch.full((n_sites,), -7, dtype=torch.int64, device=DEV)
    ess = torch.full((n_sites,), -7.0, dtype=torch.float64, device=DEV)
    b.pf_resample_sites(logw, [0.1, 0.3, 0.5], ess_min=ess_min, with_params=True, total_out=total, ess_out=ess)
    tot, ess = total.cpu().numpy(), ess.cpu().numpy()
    print("effective sample sizes", ess, "by the integers", ess_host, "totals", tot)
    assert tot[2] == -3 and tot[0] > 0 and tot[1] > 0
    np.testing.assert_allclose(ess[:2], ess_host[:2], rtol=1e-6)         # (both sides of every threshold by a factor of two)
    carried = logw.cpu().numpy()
    assert (carried[:2 * M] == 0.0).all()
    np.testing.assert_array_equal(bits(carried[2 * M:]), bits(lw0[2 * M:]))

    used = b.get_state()[:, 29] == 0
    before = [bits(b.get_state()), bits(b.get_rings()), bits(b.get_params())]
    worst = Worst("F " + ("f64" if prec == sa.F64 else "f32"))
    daily = sums[0]
    for name, series in (("nee", nee), ("daily sums", daily), ("smoothed", smoothed)):
        host = series.double().cpu().numpy()
        xs = host.reshape(host.shape[0], n_sites, M)
        obs = np.stack([np.median(xs[:, s, used.reshape(n_sites, M)[s]], axis=1) for s in range(n_sites)], axis=1) + 0.01
        got, _ = analyse(b, host, carried, Q6, obs, series.dtype, used=used, live=True, series=series, worst=worst, what=name)
        for s in (0, 1):                                                  # resampled: log-weights 0, the live sample at equal weights
            sl = slice(s * M, (s + 1) * M)
            np.testing.assert_array_equal(got.fixed[sl], np.where(used[sl], G, 0))
            assert got.site[s].tolist() == [int(used[sl].sum()) * G, int(used[sl].sum()), 0]
            same(got.quant[:, :, s], np.quantile(xs[:, s, used[sl]], Q6, axis=1, method="inverted_cdf"), (name, s))
        all_ = host_of(b.plane_quantiles_weighted(series, dev(carried), Q6, live_only=False, return_fixed=True))
        assert used[2 * M:].all() and got.site[2].tolist() == all_.site[2].tolist() and 1 < got.site[2, 1] <= M
        same_bits(got.fixed[2 * M:], all_.fixed[2 * M:], name)
        same_bits(got.quant[:, :, 2], all_.quant[:, :, 2], name)
    after = [bits(b.get_state()), bits(b.get_rings()), bits(b.get_params())]
    for p, q in zip(before, after):
        np.testing.assert_array_equal(p, q)
    # the kept site's S is the filter's own total of the same log-weights, bit for bit
    total = torch.full((n_sites,), -7, dtype=torch.int64, device=DEV)
    _, fixed = b.pf_resample_sites(dev(carried), [0.1, 0.3, 0.5], total_out=total, return_fixed=True)
    assert int(total[2]) == int(all_.site[2, 0]) == int(got.site[2, 0])
    same_bits(fixed.cpu().numpy()[2 * M:], got.fixed[2 * M:])
    b.close()
    worst.report()


# ---- G: independence, order and streams -------------------------------------------------------------------------------------
def every_output(b, series, lw, obs, path):
    return host_of(b.plane_quantiles_weighted(series, lw, Q16, live_only=False, obs=obs, want_crps=path == SORT, want_moments=True,
                                              path=path, return_fixed=True))


@pytest.mark.parametrize("M", [257, 8193])
def test_a_site_depends_on_nothing_but_its_own_columns(M):
    rows = 3
    rng = np.random.default_rng(M)
    x = np.round(rng.normal(size=(rows, M)) * 3.0, 2)
    lw = a_weight_in_every_site(random_logw(rng, M), 1, M, rng)
    y = x[:, 4] + np.array([0.0, 0.37, -0.2])
    left, right = rng.normal(size=(rows, M)) * 1e3, -x
    left[1, 3] = np.nan                                                  # a neighbour with a NaN under weight, one of code -2
    lw_left, lw_right = rng.normal(size=M), rng.normal(size=M) * 5.0
    lw_left[3] = 0.0
    lw_right[M // 2] = np.inf
    for path in ((SORT, SELECT) if M <= 8192 else (SELECT,)):
        one = bare(1, M)
        alone = every_output(one, on_device(x, pad=1), dev(lw), y.reshape(rows, 1), path)
        one.close()
        three = bare(3, M)
        obs3 = np.stack([y + 1.0, y, np.full(rows, np.nan)], axis=1)
        mid = every_output(three, on_device(np.concatenate([left, x, right], axis=1), pad=1), dev(np.concatenate([lw_left, lw, lw_right])),
                           obs3, path)
        three.close()
        assert mid.site[:, 2].tolist() == [0, 0, -2] and np.isnan(mid.quant[:, 1, 0]).all() and alone.site[0, 1] > 1
        same_bits(mid.quant[:, :, 1], alone.quant[:, :, 0], path)
        same_bits(mid.site[1], alone.site[0], path)
        same_bits(mid.rank[:, 1], alone.rank[:, 0], path)
        same_bits(mid.moments[:, 1], alone.moments[:, 0], path)
        same_bits(mid.fixed[M:2 * M], alone.fixed, path)
        if path == SORT:
            same_bits(mid.crps[:, 1], alone.crps[:, 0], path)


@pytest.mark.parametrize("stream", ["current", "another"])
def test_two_different_calls_with_no_synchronisation_between_them(stream):
    """the second call's site pre-pass overwrites the scratch integers the first call's cell kernels read: the stream's
    order keeps them apart.  Each call equals the same call made alone on a fresh batch."""
    n_sites, rows = 3, 48
    for M, path in ((8192, SORT), (8193, SELECT), (300, SORT)):
        rng = np.random.default_rng(M + 5)
        calls = []
        for k in range(2):
            host = np.round(rng.normal(size=(rows, n_sites * M)) * (1.0 + k), 2)
            logw = a_weight_in_every_site(random_logw(rng, n_sites * M, 1.0 + 2.0 * k), n_sites, M, rng)
            calls.append((on_device(host), dev(logw), dev(host[:, [1, M + 1, 2 * M + 1]] + 0.1 * k)))
        alone = []
        for args in calls:
            b = bare(n_sites, M)
            alone.append(every_output(b, *args, path))
            b.close()
        assert not np.array_equal(alone[0].fixed, alone[1].fixed) and not np.array_equal(alone[0].quant, alone[1].quant)
        b = bare(n_sites, M)
        kw = dict(live_only=False, want_crps=path == SORT, want_moments=True, path=path, return_fixed=True)
        if stream == "current":
            res = [b.plane_quantiles_weighted(s, lw, Q16, obs=y, **kw) for s, lw, y in calls]
            torch.cuda.synchronize()
        else:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())                # (the inputs were made on the current stream)
            with torch.cuda.stream(side):
                assert torch.cuda.current_stream() == side
                res = [b.plane_quantiles_weighted(s, lw, Q16, obs=y, **kw) for s, lw, y in calls]
            side.synchronize()
            torch.cuda.current_stream().wait_stream(side)
        for k in range(2):
            same_outputs(host_of(res[k]), alone[k], (stream, M, path, k))
        b.close()
