"""The weighted order statistics on the GPU (sipnet_batch_plane_quantiles_weighted, Batch.plane_quantiles_weighted) against
tests/wquantile_reference.py.

What is exact: the device's integer weights (return_fixed) lie within one unit of rint(2^30 e^(lw - m)) from the exponential of
higher precision of tests/pf_edges_reference.py (and ARE it wherever the exact value is further from a half than the derived
tolerance), and equal sipnet_batch_pf_resample_sites' with live_only = False; FROM the device's integers the quantiles, n, S,
the site codes and both rank sums equal the reference, and the two paths equal each other, bit for bit.

What is bounded, the bounds written down before the first run on a GPU (p = w / S, n the sample size, u = 2^-53):
  mean   |err| <= (n + 16) u sum p |x|.  The terms are fl((double) w x): one rounding each (w is exact); any fixed order of
         adding n terms stays within (n - 1) u sum |terms| to first order; the division by (double) S, exact, rounds once.
         n + 16 leaves the margin of the bound (n_used + 16) 2^-53 sum |terms| that the ensemble sums are held to.
  m2     |err| <= (n + 16) u m2 + 2 (the mean's bound)^2.  With the computed mean off by e, sum p (x - mean - e)^2 = m2 + e^2
         exactly, since the cross term is sum p (x - mean) = 0; a term fl(w fl(fl(x - mean)^2)) carries four roundings, the
         sum n - 1 additions, the division one.
  crps   |err| <= 4 (n + 2) u sum p |x - y|, the unweighted call's 4 (n + 2) 2^-53 mean |x - y| with the mean weighted: both
         sums of the sorted form have terms of at most p |d| (the coefficient (C_(i-1) + C_i - S) / S lies in [-1, 1]), a
         term carries at most three roundings, a sum n - 1 additions, the quotients three more: (2 n + 6) u sum p |d|.
The references are the definitions in np.longdouble (the CRPS: the pairwise energy form).  No allowance is fitted to the
kernels; every test prints the largest fraction of each bound it met.  The helpers (analyse, check_integers, check_floats,
...) are tests/wquantile_gpu_common.py's, shared with tests/test_gpu_wquantiles_edges.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import sipnet_amd as sa
from sipnet_amd import _lib
from tests import pf_edges_reference as er
from tests.enkf_gpu_common import BASE, DEV, bits, crafted
from tests.wquantile_gpu_common import (G, Q6, SELECT, SORT, analyse, bare, dev, host_of, on_device, random_logw, same_bits,
                                        scenario_batches, widened)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base():
    return sa.read_params(BASE, sa.flags_from())[0]


@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025])
def test_paths_and_sizes(M):
    n_sites, rows = 3, 3
    rng = np.random.default_rng(300 + M)
    b = bare(n_sites, M)
    host = rng.normal(size=(rows, n_sites * M)) * 3.0 - 1.0
    host[:, ::7] = np.round(host[:, ::7])                                # some ties
    logw = random_logw(rng, n_sites * M)
    logw[np.arange(n_sites) * M + rng.integers(0, M, n_sites)] = -699.0  # (every site has a member with weight)
    for dtype, pad in ((torch.float64, 0), (torch.float32, 5), (torch.float64, 3)):
        x = widened(host, dtype)
        obs = x[:, rng.integers(0, M, n_sites) + M * np.arange(n_sites)].copy()      # a member's value: a tie with y
        obs[0, 0] += 0.37
        analyse(b, host, logw, Q6, obs, dtype, pad, what=(M, dtype, pad))
    b.close()


def test_the_capacity_edge_and_the_automatic_choice():
    cap = sa.wquantile_lds_members(False)
    assert cap == 8192
    rng = np.random.default_rng(7)
    for M, auto in ((cap, SORT), (cap + 1, SELECT)):
        n_sites, rows = 3, 3
        host = rng.normal(size=(rows, n_sites * M))
        host[:, ::5] = np.round(host[:, ::5], 1)
        logw = random_logw(rng, n_sites * M, 1.0)
        obs = host[:, [5, M + 5, 2 * M + 5]].copy()
        b = bare(n_sites, M)
        series, lw = on_device(host), dev(logw)
        res = b.plane_quantiles_weighted(series, lw, Q6, live_only=False, obs=obs, want_moments=True)
        assert res.path == auto and b.pf_info()["fused"] == (1 if auto == SORT else 0) and (res.crps is not None) == (auto == SORT)
        got, want = analyse(b, host, logw, Q6, obs, paths=(SORT, SELECT) if auto == SORT else (SELECT,), crps_cells={(0, 0)}, what=M)
        same_bits(host_of(res).quant, got.quant, M)
        if auto == SELECT:
            for kw in (dict(path=SORT), dict(obs=obs, want_crps=True)):
                with pytest.raises(sa.SipnetError):
                    b.plane_quantiles_weighted(series, lw, Q6, live_only=False, **kw)
        b.close()


@pytest.mark.parametrize("M", [257, 1000])
def test_crafted_weights(M):
    rng = np.random.default_rng(50 + M)
    rows = 3
    ninf = np.full(M, -np.inf)

    def values():
        return rng.normal(size=(rows, M))

    def lw_at(idx, v=0.0):
        lw = ninf.copy()
        lw[np.atleast_1d(idx)] = v
        return lw

    sc = {}
    x_equal = values()
    sc["equal"] = (np.full(M, -3.25), x_equal, x_equal[:, 4].copy())
    sc["one member"] = (lw_at(M // 2, 12.5), values(), np.zeros(rows))
    sc["first only"] = (lw_at(0), values(), np.zeros(rows))
    sc["last only"] = (lw_at(M - 1), values(), np.zeros(rows))
    sc["alternating"] = (np.where(np.arange(M) % 2 == 0, 0.0, -np.inf), values(), np.zeros(rows))
    wave = rng.normal(size=M)
    wave[64:128] = -np.inf
    sc["a wavefront at -inf"] = (wave, values(), np.zeros(rows))
    x_nan0 = values()
    x_nan0[:, 10] = np.nan
    lw_nan0 = rng.normal(size=M)
    lw_nan0[10] = -np.inf
    sc["nan under weight 0"] = (lw_nan0, x_nan0, np.zeros(rows))
    x_nan1 = values()
    x_nan1[1, 10] = np.nan                                               # row 1 only
    sc["nan under weight"] = (rng.normal(size=M), x_nan1, np.zeros(rows))
    sc["only -inf"] = (ninf.copy(), values(), np.zeros(rows))
    lw_pinf = rng.normal(size=M)
    lw_pinf[M - 2] = np.inf
    sc["a +inf"] = (lw_pinf, values(), np.zeros(rows))
    x_ties = np.tile(np.array([2.0, 1.0, 2.0, 3.0, 1.0, 2.0]), (rows, M // 6 + 1))[:, :M]
    lw_ties = np.tile(np.array([er.LW_OF[G], er.LW_OF[2], er.LW_OF[1], er.LW_OF[2], er.LW_OF[1], er.LW_OF[G]]), M // 6 + 1)[:M]
    sc["ties, weights differ"] = (lw_ties, x_ties, np.array([2.0, 1.0, 2.5]))
    # four members of weight 2^30 each (S = 2^32): q = k / 4 puts T ON the cumulative weight C_(k-1), q = k / 4 + 2^-32 on
    # C_(k-1) + 1 -- both products exact
    x_four = values()
    x_four[:, [3, 70, 200, M - 1]] = [40.0, 10.0, 30.0, 20.0]
    sc["T on C and on C + 1"] = (lw_at([3, 70, 200, M - 1], -5.0), x_four, np.array([10.0, 25.0, 50.0]))
    q = [0.0, 1.0, 0.25, 0.5, 0.75, 0.25 + 2.0 ** -32, 0.5 + 2.0 ** -32, 0.75 + 2.0 ** -32, 0.1, 0.9]
    got = scenario_batches(M, sc, q, rows)

    g = got["equal"]                                                     # against the unweighted call
    b = bare(1, M)
    plain = b.plane_quantiles(on_device(x_equal), q, live_only=False, obs=sc["equal"][2].reshape(rows, 1), want_crps=False)
    b.close()
    assert list(g.site) == [M * G, M, 0] and (g.fixed == G).all()
    np.testing.assert_array_equal(g.rank, plain.rank.cpu().numpy()[:, 0].astype(np.int64) * G)
    assert (plain.count.cpu().numpy() == g.site[1]).all()
    np.testing.assert_array_equal(bits(g.quant[:2]), bits(plain.quant.cpu().numpy()[:2, :, 0]))
    for name, idx in (("one member", M // 2), ("first only", 0), ("last only", M - 1)):
        g, x = got[name], sc[name][1]
        assert list(g.site) == [G, 1, 0], name
        np.testing.assert_array_equal(g.quant, np.tile(x[:, idx], (len(q), 1)), err_msg=name)
        np.testing.assert_array_equal(g.moments, np.stack([x[:, idx], np.zeros(rows)], axis=1), err_msg=name)
        np.testing.assert_array_equal(g.crps, np.abs(x[:, idx]), err_msg=name)
        np.testing.assert_array_equal(g.rank, np.stack([np.where(x[:, idx] < 0, G, 0), np.zeros(rows, np.int64)], axis=1), err_msg=name)
    g = got["alternating"]
    assert list(g.site) == [(M + 1) // 2 * G, (M + 1) // 2, 0] and (g.fixed[1::2] == 0).all()
    np.testing.assert_array_equal(g.quant[0], sc["alternating"][1][:, ::2].min(axis=1))
    np.testing.assert_array_equal(g.quant[1], sc["alternating"][1][:, ::2].max(axis=1))
    g = got["a wavefront at -inf"]
    assert (g.fixed[64:128] == 0).all() and g.site[1] == (g.fixed > 0).sum() <= M - 64
    g = got["nan under weight 0"]
    assert g.fixed[10] == 0 and not np.isnan(g.quant).any() and not np.isnan(g.moments).any() and not np.isnan(g.crps).any()
    g = got["nan under weight"]
    assert g.fixed[10] > 0 and np.isnan(g.quant[:, 1]).all() and np.isnan(g.moments[1]).all() and np.isnan(g.crps[1])
    assert list(g.rank[1]) == [-1, -1] and not np.isnan(g.quant[:, [0, 2]]).any() and (g.rank[[0, 2]] >= 0).all()
    g = got["only -inf"]
    assert list(g.site) == [0, 0, 1] and np.isnan(g.quant).all() and np.isnan(g.moments).all() and np.isnan(g.crps).all()
    assert (g.rank == 0).all() and (g.fixed == 0).all()
    g = got["a +inf"]
    assert list(g.site) == [0, 0, -2] and np.isnan(g.quant).all() and np.isnan(g.moments).all() and np.isnan(g.crps).all()
    assert (g.rank == -2).all() and (g.fixed == 0).all()
    g = got["ties, weights differ"]
    assert set(g.fixed) == {G, 2, 1}
    w1, w2, w3 = (int(g.fixed[x_ties[0] == v].sum()) for v in (1.0, 2.0, 3.0))
    np.testing.assert_array_equal(g.rank, [[w1, w2], [0, w1], [w1 + w2, 0]])
    g = got["T on C and on C + 1"]
    assert list(g.site) == [4 * G, 4, 0]
    assert [sa.wquantile_target(4 * G, v) for v in q[2:8]] == [G, 2 * G, 3 * G, G + 1, 2 * G + 1, 3 * G + 1]
    np.testing.assert_array_equal(g.quant[:8, 0], [10.0, 40.0, 10.0, 20.0, 30.0, 20.0, 30.0, 40.0])
    np.testing.assert_array_equal(g.rank, [[0, G], [2 * G, 0], [4 * G, 0]])


@pytest.mark.parametrize("prec", [sa.F64, sa.F32_MIXED], ids=["f64", "f32"])
def test_live_members_only_and_the_filters_integers(base, prec):
    """site 0: three members dead; site 1: all dead; site 2: one live; site 3: all live.  The dead columns hold NaN, and the
    largest log-weight of site 0 is a dead member's: the maximum is taken over the used members."""
    n_sites, M, rows = 4, 70, 3
    dead = [5, 17, 69] + list(range(M, 2 * M)) + [c for c in range(2 * M, 3 * M) if c != 2 * M + 33]
    rng = np.random.default_rng(13)
    b, st = crafted(base, n_sites, M, prec, rng.uniform(1.0, 100.0, (n_sites * M, 13)), dead=dead)
    used = st[:, 29] == 0
    assert used.sum() == n_sites * M - len(dead)
    host = rng.normal(size=(rows, n_sites * M))
    host[:, ~used] = np.nan
    logw = rng.normal(size=n_sites * M) * 2.0
    logw[17] = 30.0
    obs = rng.normal(size=(rows, n_sites))
    dtype = torch.float32 if prec == sa.F32_MIXED else torch.float64
    got, want = analyse(b, host, logw, Q6, obs, dtype, 3, used=used, live=True, what="live")
    assert list(got.site[:, 1]) == [(got.fixed[:M] > 0).sum(), 0, 1, (got.fixed[3 * M:] > 0).sum()] and list(got.site[:, 2]) == [0, 1, 0, 0]
    assert got.fixed[:M].max() == G and got.fixed[17] == 0 and (got.fixed[~used] == 0).all()
    np.testing.assert_array_equal(got.quant[:, :, 2], np.tile(widened(host, dtype)[:, 2 * M + 33], (len(Q6), 1)))
    # all members: the integers and the totals are the filter's own, bit for bit (the values are then NaN where a dead member
    # weighs something)
    all_, _ = analyse(b, host, logw, Q6, obs, dtype, 3, what="all")
    assert all_.fixed[17] == G
    total = torch.full((n_sites,), -7, dtype=torch.int64, device=DEV)
    _, fixed = b.pf_resample_sites(dev(logw), [0.5] * n_sites, total_out=total, return_fixed=True)
    same_bits(all_.fixed, fixed.cpu().numpy())
    np.testing.assert_array_equal(all_.site[:, 0], total.cpu().numpy())
    b.close()


def test_more_cells_than_one_row_of_the_grid():
    """2^20 + 3 cells of one member each (the grid is rows of 2^20 workgroups): every cell its own value"""
    rows = (1 << 20) + 3
    host = np.random.default_rng(12).normal(size=(rows, 1))
    obs = host + 1.0
    b = bare(1, 1)
    series, lw = on_device(host), dev([-3.0])
    for path in (SORT, SELECT):
        got = host_of(b.plane_quantiles_weighted(series, lw, [0.0, 0.5], live_only=False, obs=obs, want_crps=path == SORT,
                                                 want_moments=True, path=path))
        assert np.array_equal(got.quant[0, :, 0], host[:, 0]) and np.array_equal(got.quant[1, :, 0], host[:, 0]), path
        assert list(got.site[0]) == [G, 1, 0] and (got.rank == [G, 0]).all(), path
        assert np.array_equal(got.moments[:, 0, 0], host[:, 0]) and (got.moments[:, 0, 1] == 0.0).all(), path
        if path == SORT:
            assert np.array_equal(got.crps[:, 0], np.abs(host[:, 0] - obs[:, 0]))
    b.close()


def test_the_batch_is_left_as_it_was_and_a_repeated_call_gives_the_same_bits(base):
    n_sites, M, rows = 3, 300, 3
    rng = np.random.default_rng(8)
    b, _ = crafted(base, n_sites, M, sa.F64, rng.uniform(1.0, 100.0, (n_sites * M, 13)), dead=[3, 370])
    before = [bits(b.get_state()), bits(b.get_rings()), bits(b.get_params())]
    series, lw = on_device(rng.normal(size=(rows, n_sites * M))), dev(rng.normal(size=n_sites * M) * 2.0)
    obs = rng.normal(size=(rows, n_sites))
    for path in (SORT, SELECT):
        for live in (True, False):
            kw = dict(live_only=live, obs=obs, want_crps=path == SORT, want_moments=True, path=path, return_fixed=True)
            one = host_of(b.plane_quantiles_weighted(series, lw, Q6, **kw))
            two = host_of(b.plane_quantiles_weighted(series, lw, Q6, **kw))
            for x, y in zip(one, two):
                assert (x is None) == (y is None)
                if x is not None:
                    same_bits(x, y, (path, live))
    after = [bits(b.get_state()), bits(b.get_rings()), bits(b.get_params())]
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)
    b.close()


def test_refusals_write_nothing():
    L = sa.lib()
    n_sites, M, rows = 3, 64, 3
    cap = sa.wquantile_lds_members(False)
    small, big = bare(n_sites, M), bare(1, cap + 1)
    many = sa.Batch(sa.flags_from(), 2, (1 << 21) + 1, sa.F32_MIXED)    # more than 4 194 304 columns
    series = on_device(np.zeros((rows, n_sites * M)))
    wide = on_device(np.zeros((rows, cap + 1)))
    huge = torch.zeros((1, many.ncol), dtype=torch.float32, device=DEV)
    logw = dev(np.zeros(n_sites * M))
    logw_wide, logw_huge = dev(np.zeros(cap + 1)), torch.zeros(many.ncol, dtype=torch.float64, device=DEV)
    quant = torch.full((16, rows, n_sites), -7.0, dtype=torch.float64, device=DEV)
    site = torch.full((n_sites, 3), -7, dtype=torch.int64, device=DEV)
    fixed = torch.full((n_sites * M,), -7, dtype=torch.int64, device=DEV)
    moments = torch.full((rows, n_sites, 2), -7.0, dtype=torch.float64, device=DEV)
    crps = torch.full((rows, n_sites), -7.0, dtype=torch.float64, device=DEV)
    rank = torch.full((rows, n_sites, 2), -7, dtype=torch.int64, device=DEV)
    obs = torch.zeros((rows, n_sites), dtype=torch.float64, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(b=small, s=series, f32=0, r=rows, ld=n_sites * M, lw=logw, q=(0.5,), n_q=None, live=0, path=0, qt=quant, sw=site,
             fx=fixed, mo=moments, y=obs, cr=None, rk=None):
        qs = None if q is None else (C.c_double * max(len(q), 1))(*q)
        ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        return L.sipnet_batch_plane_quantiles_weighted(b.h if b is not None else None, ptr(s), f32, r, ld, ptr(lw),
                                                       len(q) if n_q is None else n_q, qs, live, path, ptr(qt), ptr(sw), ptr(fx),
                                                       ptr(mo), ptr(y), ptr(cr), ptr(rk), stream)

    cases = {
        "a NULL batch": dict(b=None), "a NULL series": dict(s=None), "a NULL q": dict(q=None, n_q=1), "a NULL d_quant": dict(qt=None),
        "a NULL d_logw": dict(lw=None),
        "rows 0": dict(r=0), "ld below ncol": dict(ld=n_sites * M - 1),
        "n_q 0": dict(q=(), n_q=0), "n_q 17": dict(q=(0.5,) * 17),
        "q nan": dict(q=(0.5, float("nan"))), "q below 0": dict(q=(-0.1,)), "q above 1": dict(q=(0.2, 1.1)), "q inf": dict(q=(float("inf"),)),
        "crps without obs": dict(y=None, cr=crps), "rank without obs": dict(y=None, rk=rank),
        "path -1": dict(path=-1), "path 3": dict(path=3),
        "the sort path beyond its capacity": dict(b=big, s=wide, ld=cap + 1, lw=logw_wide, path=1),
        "crps on the forced selection path": dict(cr=crps, path=2),
        "crps on the selection path by size": dict(b=big, s=wide, ld=cap + 1, lw=logw_wide, cr=crps),
        "live members of a batch that is not set up": dict(live=1),
        "more than 4194304 columns": dict(b=many, s=huge, f32=1, r=1, ld=many.ncol, lw=logw_huge, path=2),
    }
    for name, kw in cases.items():
        assert call(**kw) == _lib.ERR_BAD_ARGUMENT, name
        assert b"sipnet_batch_plane_quantiles_weighted: " in L.sipnet_last_error(), name
    assert b"4194304" in L.sipnet_last_error()
    torch.cuda.synchronize()
    assert (quant == -7.0).all() and (site == -7).all() and (fixed == -7).all() and (moments == -7.0).all()
    assert (crps == -7.0).all() and (rank == -7).all()
    assert call(cr=crps, rk=rank) == _lib.OK                            # the call itself is sound
    torch.cuda.synchronize()
    assert (quant[0] == 0.0).all() and (quant[1:] == -7.0).all() and (site == torch.tensor([M * G, M, 0], device=DEV)).all()
    assert (fixed == G).all() and (moments == 0.0).all() and (crps == 0.0).all() and (rank == torch.tensor([0, M * G], device=DEV)).all()
    for b in (small, big, many):
        b.close()
