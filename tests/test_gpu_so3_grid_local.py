"""GPU: the neighbour-limited kernel sum over the SO(3) grid (rnf_so3_grid_local_sum) against the fp64 bracket of
tests/test_so3_grid_local_host.py, its bit-level invariances, and what is built on it: grid_diffuse_local, grid_filter_step,
grid_pose_filter.

The bracket here is the same brute force over ALL Q rows with the mask d^2 <= cut -+ delta, in torch fp64 on the device, chunked over the
queries; the rows that pass d^2 <= cut + delta are kept as (query, row, d^2) triples and every sum is formed from them."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import flow_oracle as orc
from rotationnormflow_amd import grid_pose, harness, make_config, synth
from rotationnormflow_amd.utils import kde, sd
from tests import test_so3_grid_local_host as hl
from tests.gpu_helpers import product_flow
from tests.test_so3_kde_host import log_normaliser

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=8)
def device_grid(level, kind):
    off = hl.offset_of(kind)
    return sd.generate_healpix_grid(recursion_level=level, device=DEV, offset=None if off is None else dev(off)), (None if off is None else dev(off))


# ---- the restatement on the device ---------------------------------------------------------------------------------------------------

def pairs_within(grid, queries, d2_max, budget=1 << 25):
    """(i, j, d2): every (query, grid row) with fp64 |G_j - Q_i|_F^2 <= d2_max, brute force over all rows, chunked over the queries"""
    G64, Q64 = grid.reshape(-1, 9).double(), queries.reshape(-1, 9).double()
    step = max(1, budget // len(G64))
    I, J, D = [], [], []
    for i0 in range(0, len(Q64), step):
        q = Q64[i0:i0 + step]
        d2 = torch.zeros(len(q), len(G64), dtype=torch.float64, device=grid.device)
        for k in range(9):
            d2 += (q[:, k, None] - G64[None, :, k]) ** 2
        i, j = torch.nonzero(d2 <= d2_max, as_tuple=True)
        I.append(i + i0)
        J.append(j)
        D.append(d2[i, j])
    return torch.cat(I), torch.cat(J), torch.cat(D)


def bracket_from_pairs(pairs, m, kappa, d2_cut, lw=None):
    """hl.local_sum_fp64's dictionary (as numpy) from the pairs within cut + delta"""
    i, j, d2 = pairs
    delta = hl.delta_of(d2_cut)
    G = 1 if lw is None else lw.shape[0]
    l_kappa = float(log_normaliser(kappa))
    res = {}
    for name, keep in (("lo", d2 <= d2_cut - delta), ("hi", d2 <= d2_cut + delta)):
        ii, jj, dd = i[keep], j[keep], d2[keep]
        res["count_" + name] = torch.bincount(ii, minlength=m).cpu().numpy()
        vals, Es = [], []
        for g in range(G):
            w = torch.zeros_like(dd) if lw is None else lw[g].double()[jj]
            nan = torch.zeros(m, dtype=torch.bool, device=dd.device).index_put_((ii[torch.isnan(w)],), torch.tensor(True, device=dd.device))
            t = torch.where(torch.isnan(w), torch.full_like(dd, -math.inf), w - 0.5 * kappa * dd)
            top = torch.full((m,), -math.inf, dtype=torch.float64, device=dd.device).scatter_reduce(0, ii, t, "amax")
            safe = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
            s = torch.zeros(m, dtype=torch.float64, device=dd.device).index_add_(0, ii, torch.exp(t - safe[ii]))
            v = torch.where(torch.isfinite(top), safe + torch.log(s) - l_kappa, torch.full_like(top, -math.inf))
            e_term = torch.where(t == top[ii], 0.5 * kappa * dd + torch.nan_to_num(w, posinf=0.0, neginf=0.0).abs(), torch.zeros_like(dd))
            E = torch.zeros(m, dtype=torch.float64, device=dd.device).scatter_reduce(0, ii, e_term, "amax")
            vals.append(torch.where(nan, torch.full_like(v, math.nan), v))
            Es.append(torch.where(torch.isfinite(top), E, torch.zeros_like(E)))
        res[name], res["E_" + name] = torch.stack(vals).cpu().numpy(), torch.stack(Es).cpu().numpy()
    res["E"] = np.maximum(res["E_lo"], res["E_hi"])
    return res


def dense_d2(grid, queries):
    """fp64 |G_j - Q_i|_F^2 [m,Q] whole (levels 1 and 2)"""
    G64, Q64 = grid.reshape(-1, 9).double(), queries.reshape(-1, 9).double()
    d2 = torch.zeros(len(Q64), len(G64), dtype=torch.float64, device=grid.device)
    for k in range(9):
        d2 += (Q64[:, k, None] - G64[None, :, k]) ** 2
    return d2


def bracket_dense(d2, kappa, d2_cut, lw=None):
    """hl.local_sum_fp64 in torch on the device, from the whole matrix of distances: row reductions, no scatter"""
    m, Q = d2.shape
    delta, l_kappa = hl.delta_of(d2_cut), float(log_normaliser(kappa))
    lw64 = torch.zeros(1, Q, dtype=torch.float64, device=d2.device) if lw is None else lw.double()
    rows = torch.arange(m, device=d2.device)
    res = {}
    for name, mask in (("lo", d2 <= d2_cut - delta), ("hi", d2 <= d2_cut + delta)):
        res["count_" + name] = mask.sum(dim=1).cpu().numpy()
        vals, Es = [], []
        for w in lw64:
            nan = (mask & torch.isnan(w)[None, :]).any(dim=1)
            t = torch.where(mask, w[None, :] - 0.5 * kappa * d2, torch.full_like(d2, -math.inf))
            t = torch.where(torch.isnan(t), torch.full_like(t, -math.inf), t)
            top, at = t.max(dim=1)
            safe = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
            v = torch.where(torch.isfinite(top), safe + torch.log(torch.exp(t - safe[:, None]).sum(dim=1)) - l_kappa, torch.full_like(top, -math.inf))
            E = 0.5 * kappa * d2[rows, at] + torch.nan_to_num(w[at], posinf=0.0, neginf=0.0).abs()
            vals.append(torch.where(nan, torch.full_like(v, math.nan), v))
            Es.append(torch.where(torch.isfinite(top), E, torch.zeros_like(E)))
        res[name], res["E_" + name] = torch.stack(vals).cpu().numpy(), torch.stack(Es).cpu().numpy()
    res["E"] = np.maximum(res["E_lo"], res["E_hi"])
    return res


def picked_rows(level):
    """Grid rows nearest both poles, at phi ~ 0 on several rings and on the rings about the cap boundaries, at tilts 0, 1, the last and the
    middle one"""
    ns = 2 ** level
    npix, ntilt = 12 * ns * ns, 6 * ns
    pix = list(range(4)) + list(range(npix - 4, npix))
    for ring in sorted({1, 2, ns - 1, ns, ns + 1, 2 * ns, 3 * ns - 1, 3 * ns, 3 * ns + 1, 4 * ns - 2, 4 * ns - 1} & set(range(1, 4 * ns))):
        if ring < ns:
            first, count = 2 * ring * (ring - 1), 4 * ring
        elif ring <= 3 * ns:
            first, count = 2 * ns * (ns - 1) + (ring - ns) * 4 * ns, 4 * ns
        else:
            k = 4 * ns - ring
            first, count = npix - 2 * k * (k + 1), 4 * k
        pix += [first, first + count - 1]                                  # the ring's pixels on either side of phi = 0
    tilts = sorted({0, 1, ntilt - 1, ntilt // 2})
    return np.unique(np.array([t * npix + p for t in tilts for p in pix], np.int64))


@functools.lru_cache(maxsize=8)
def sampled_case(level, kind, m):
    """(grid, offset, queries [m,3,3] on the device): the picked grid rows, the special off-grid queries, random grid rows and random rotations;
    m = 0: every grid row and the special queries"""
    grid, off = device_grid(level, kind)
    special, _ = hl.special_queries(level, kind)
    if m == 0:
        return grid, off, torch.cat([grid, dev(special)])
    rows = picked_rows(level)
    rng = np.random.default_rng(level)
    more = rng.integers(0, grid.shape[0], max(0, m - len(rows) - len(special)))
    q = torch.cat([grid[dev(rows)], dev(special), grid[dev(more)]])[:m]
    assert q.shape[0] == m and len(rows) + len(special) <= m
    return grid, off, q.contiguous()


def device_local_sum(level, grid, queries, kappa, cut, lw, off):
    out, count = kde.so3_grid_local_log_sum(grid, level, kappa, d2_cut=cut, queries=queries, log_weights=lw, offset=off, return_count=True)
    return out.reshape(-1, queries.shape[0]).cpu().numpy(), count.cpu().numpy()


# ---- the device against the bracket --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level,kind,m", [(1, "none", 0), (1, "fixed", 0), (2, "none", 0), (2, "fixed", 0), (3, "fixed", 2048), (4, "fixed", 512),
                                          (5, "none", 512), (5, "fixed", 512)])
def test_device_lies_in_the_bracket(level, kind, m):
    grid, off, queries = sampled_case(level, kind, m)
    Q, mq = grid.shape[0], queries.shape[0]
    lw5 = dev(hl.log_weights_of(Q, 5, 20 + level))
    nearest = pairs_within(grid, queries[Q:], 8.0)[2].min().item() if m == 0 else 1e-4          # of the off-grid queries
    cuts = hl.cuts_of(level, nearest) if level <= 2 else (hl.chord2(hl.spacing_deg(level)), hl.chord2(15.0))
    kappas = hl.KAPPAS if level <= 2 else (kde.LOCAL_NATS * 2 / hl.chord2(15.0), 1e4)
    worst = 0.0
    d2 = dense_d2(grid, queries) if level <= 2 else None                   # levels 1 and 2: the whole matrix; above: the pairs within the cut
    for cut in cuts:
        pairs = pairs_within(grid, queries, cut + hl.delta_of(cut)) if d2 is None else None
        bracket = (lambda kappa, lw: bracket_dense(d2, kappa, cut, lw)) if d2 is not None else (            # noqa: E731
            lambda kappa, lw: bracket_from_pairs(pairs, mq, kappa, cut, lw))
        for kappa in kappas:
            out5, count = device_local_sum(level, grid, queries, kappa, cut, lw5, off)
            ref = bracket(kappa, lw5)
            worst = max(worst, hl.check_bracket(out5, count, ref, (level, kind, cut, kappa, "G=5")))
            out3, count3 = device_local_sum(level, grid, queries, kappa, cut, lw5[:3], off)
            out1, count1 = device_local_sum(level, grid, queries, kappa, cut, lw5[4:], off)
            assert np.array_equal(out3.view(np.int32), out5[:3].view(np.int32)) and np.array_equal(out1.view(np.int32), out5[4:].view(np.int32))
            assert np.array_equal(count, count3) and np.array_equal(count, count1)
            out0, count0 = device_local_sum(level, grid, queries, kappa, cut, None, off)
            worst = max(worst, hl.check_bracket(out0, count0, bracket(kappa, None), (level, kind, cut, kappa, "no weights")))
            assert np.array_equal(count, count0)
    print("level %d offset %s: %d queries, worst distance beyond the bracket / gate %.3f" % (level, kind, mq, worst))


def test_device_near_rotations_and_sentinels():
    def fn(level, grid, queries, kappa, cut, lw, off):
        return device_local_sum(level, dev(grid), dev(queries), kappa, cut, dev(lw), dev(off))
    hl.check_near_rotation(fn, 2, "fixed")
    hl.check_sentinels(fn)


# ---- bit equality ----------------------------------------------------------------------------------------------------------------------

def _bits(x):
    return x.contiguous().view(torch.int32)


def test_a_result_does_not_depend_on_the_call(monkeypatch):
    level = 3
    grid, off, queries = sampled_case(level, "fixed", 2048)
    Q = grid.shape[0]
    lw = dev(hl.log_weights_of(Q, 3, 3))
    kappa, cut = 264.0, hl.chord2(15.0)
    call = lambda q, w: kde.so3_grid_local_log_sum(grid, level, kappa, d2_cut=cut, queries=q, log_weights=w, offset=off, return_count=True)  # noqa: E731
    whole, count = call(queries[:937], lw)
    again, _ = call(queries[:937], lw)
    assert torch.equal(_bits(whole), _bits(again))                          # from run to run
    for i in (0, 5, 936):
        one, c1 = call(queries[i:i + 1], lw)
        assert torch.equal(_bits(one[:, 0]), _bits(whole[:, i])) and c1[0] == count[i]
    part, c64 = call(queries[100:164], lw)
    assert torch.equal(_bits(part), _bits(whole[:, 100:164])) and torch.equal(c64, count[100:164])
    rev, crev = call(queries[:937].flip(0).contiguous(), lw)
    assert torch.equal(_bits(rev.flip(1)), _bits(whole)) and torch.equal(crev.flip(0), count)
    g1, _ = call(queries[:937], lw[1:2])                                    # G = 3 against G = 1, and the group's position
    assert torch.equal(_bits(g1[0]), _bits(whole[1]))
    swapped, _ = call(queries[:937], lw.flip(0).contiguous())
    assert torch.equal(_bits(swapped.flip(0)), _bits(whole))
    monkeypatch.setattr(kde, "LOCAL_QUERY_TILE", 100)                       # the Python tiling forced small
    monkeypatch.setattr(kde, "LOCAL_GROUP_TILE", 2)
    tiled, ctiled = call(queries[:937], lw)
    assert torch.equal(_bits(tiled), _bits(whole)) and torch.equal(ctiled, count)
    rows, crows = kde.so3_grid_local_log_sum(grid, level, kappa, d2_cut=cut, log_weights=lw[0], offset=off, return_count=True)   # the grid rows, tiled
    monkeypatch.undo()
    rows1, crows1 = kde.so3_grid_local_log_sum(grid, level, kappa, d2_cut=cut, log_weights=lw[0], offset=off, return_count=True)  # .. and by the null pointer
    assert rows.shape == (Q,) and torch.equal(_bits(rows), _bits(rows1)) and torch.equal(crows, crows1)


def test_device_gives_the_host_builds_bits_at_level_2():
    grid, off = device_grid(2, "fixed")
    g_host, o_host = grid.cpu().numpy(), off.cpu().numpy()
    lw = hl.log_weights_of(len(g_host), 2, 4)
    for kappa, cut in ((64.0, hl.chord2(30.0)), (1e4, hl.chord2(15.0)), (4.0, 8.0)):
        want, wcount = hl.host_local_sum(2, g_host, None, kappa, cut, lw, o_host)
        got, count = kde.so3_grid_local_log_sum(grid, 2, kappa, d2_cut=cut, log_weights=dev(lw), offset=off, return_count=True)
        assert np.array_equal(count.cpu().numpy(), wcount)
        same = got.cpu().numpy().view(np.int32) == want.view(np.int32)
        print("kappa %g cut %.4f: %d of %d outputs differ from the host build" % (kappa, cut, int((~same).sum()), same.size))
        assert same.all()


def test_graph_capture_replays_the_eager_result():
    grid, off, queries = sampled_case(3, "fixed", 2048)
    lw = dev(hl.log_weights_of(grid.shape[0], 3, 6))

    def step():
        return kde.so3_grid_local_log_sum(grid, 3, 264.0, queries=queries, log_weights=lw, offset=off, return_count=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager, ecount = (x.clone() for x in step())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                           # a host read-back would fail the capture
        out, count = step()
    for _ in range(2):
        out.fill_(float("nan"))
        count.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager)) and torch.equal(count, ecount)


# ---- diffusion and the filter --------------------------------------------------------------------------------------------------------

MODE_A = hl._rx(np.asarray(0.4))[()] @ hl._rz(np.asarray(1.1))[()] @ hl._rx(np.asarray(2.0))[()]
MODE_B = MODE_A @ np.diag([-1.0, -1.0, 1.0])


def mf_log_density(grid64, mode, kappa):
    return kappa * (np.einsum("qij,ij->q", grid64, mode) - 3.0) - float(log_normaliser(kappa))


def two_mode_logp(grid):
    """A strictly positive two-mode posterior on the grid rows: 0.6 MF(20 A) + 0.4 MF(20 B) + 1e-3, fp32 [1,Q]"""
    g = grid.cpu().numpy().astype(np.float64)
    p = 0.6 * np.exp(mf_log_density(g, MODE_A, 20.0)) + 0.4 * np.exp(mf_log_density(g, MODE_B, 20.0)) + 1e-3
    return np.log(p).astype(np.float32)[None]


def diffuse_fp64(logp, grid, kappa, cut, pairs=None):
    """grid_diffuse_local's definition in fp64 from the pairs within the cut (``pairs``: those of ``pairs_within(grid, grid, cut)``)
    -> [B,Q] float64 on the device"""
    Q = grid.shape[0]
    i, j, d2 = pairs_within(grid, grid, cut) if pairs is None else pairs
    k = torch.exp(-0.5 * kappa * d2 - float(log_normaliser(kappa)))
    Z = torch.zeros(Q, dtype=torch.float64, device=grid.device).index_add_(0, j, k) / Q
    p = torch.softmax(logp.double(), dim=1)
    out = torch.zeros_like(p)
    for b in range(p.shape[0]):
        out[b].index_add_(0, i, p[b][j] / Z[j] * k)
    return torch.log(out)


@pytest.mark.parametrize("level", [2, 3])
def test_grid_diffuse_local_is_a_markov_kernel_on_the_grid(level):
    grid, off = device_grid(level, "fixed")
    Q = grid.shape[0]
    logp = torch.cat([dev(two_mode_logp(grid)), dev(np.random.default_rng(level).standard_normal((1, Q)).astype(np.float32) * 3.0)])
    for kappa, radius in ((264.0, 4.0 if level == 3 else 8.0), (264.0, None), (16.0, 180.0)):
        out = harness.grid_diffuse_local(logp, grid, level, kappa, radius_deg=radius, offset=off)
        assert tuple(out.shape) == (2, Q) and out.dtype == torch.float32
        norm = torch.logsumexp(out.double(), dim=1) - math.log(Q)
        print("level %d kappa %g radius %s: log of the grid mass %s" % (level, kappa, radius, norm.cpu().numpy()))
        assert norm.abs().max() <= 2e-6


def test_grid_diffuse_local_at_180_degrees_is_grid_diffuse():
    grid, off = device_grid(2, "fixed")
    logp = dev(two_mode_logp(grid))
    for kappa in (4.0, 64.0):
        local = harness.grid_diffuse_local(logp, grid, 2, kappa, radius_deg=180.0, offset=off).double()
        dense = harness.grid_diffuse(logp, grid, kappa).double()
        pairs = pairs_within(grid, grid, 8.0 + 1e-3)                        # every pair
        ref = diffuse_fp64(logp, grid, kappa, None, pairs)
        # the gate, with E = (kappa/2) d^2 + |lw| of each output's largest term, lw = log p_j - log Z_j
        i, j, d2 = pairs
        Q = grid.shape[0]
        logZ = torch.log(torch.zeros(Q, dtype=torch.float64, device=DEV).index_add_(0, j, torch.exp(-0.5 * kappa * d2 - float(log_normaliser(kappa)))) / Q)
        lw = torch.log_softmax(logp.double(), 1)[0] - logZ
        t = lw[j] - 0.5 * kappa * d2
        top = torch.full((Q,), -math.inf, dtype=torch.float64, device=DEV).scatter_reduce(0, i, t, "amax")
        E = torch.zeros(Q, dtype=torch.float64, device=DEV).scatter_reduce(0, i, torch.where(t == top[i], 0.5 * kappa * d2 + lw[j].abs(), torch.zeros_like(t)), "amax")
        g = 1e-6 * E + 4e-6
        err_l, err_d, diff = (local - ref).abs()[0], (dense - ref).abs()[0], (local - dense).abs()[0]
        print("kappa %g: worst / gate: |local - fp64| %.3f, |dense - fp64| %.3f, |local - dense| %.3f (gate %.3g .. %.3g)" % (
            kappa, float((err_l / g).max()), float((err_d / g).max()), float((diff / g).max()), float(g.min()), float(g.max())))
        assert (diff <= g).all() and (err_l <= g).all()


def test_grid_diffuse_local_with_a_kernel_sharper_than_a_cell_is_the_identity():
    grid, off = device_grid(2, "fixed")
    Q = grid.shape[0]
    logp = dev(two_mode_logp(grid))
    start = torch.log_softmax(logp.double(), dim=1) + math.log(Q)
    out = harness.grid_diffuse_local(logp, grid, 2, 1e6, offset=off).double()
    E = (start - math.log(Q) - (-float(log_normaliser(1e6)) - math.log(Q))).abs()      # the row's own term: its log-weight log p_i - log Z_i
    err = (out - start).abs()
    print("kappa 1e6: worst |out - start| / gate %.3f" % float((err / (1e-6 * E + 4e-6)).max()))
    assert (err <= 1e-6 * E + 4e-6).all()


def test_grid_diffuse_local_at_level_4_against_the_truncated_restatement():
    level, kappa, radius = 4, 264.0, 15.0
    grid, off = device_grid(level, "fixed")
    Q = grid.shape[0]
    g64 = grid.cpu().numpy().astype(np.float64)
    logp = dev(np.stack([two_mode_logp(grid)[0], mf_log_density(g64, MODE_B, 50.0).astype(np.float32)]))
    out = harness.grid_diffuse_local(logp, grid, level, kappa, radius_deg=radius, offset=off)
    assert tuple(out.shape) == (2, Q)
    pick = np.random.default_rng(1).choice(Q, 512, replace=False)
    special = picked_rows(level)[:128]                                      # poles, phi ~ 0, cap boundaries
    pick[:len(special)] = special
    rows = dev(np.unique(pick))
    assert len(rows) >= 500
    cut = hl.chord2(radius)
    # Z on the neighbours of the sampled rows from fp64 pairs (there a pair within delta of the cut carries e^-18 of the row's own term),
    # then the sampled rows' sums as the bracket of the membership: on the tail of a sharp posterior the largest term of a sum lies AT
    # the cut, so a pair within delta of it, which fp32 and fp64 may place on either side, is worth a few per cent of the sum
    delta = hl.delta_of(cut)
    i, j, d2 = pairs_within(grid, grid[rows], cut + delta)
    near = torch.unique(j)
    ni, nj, nd2 = pairs_within(grid, grid[near], cut, budget=1 << 27)
    l_kappa = float(log_normaliser(kappa))
    Z = torch.zeros(len(near), dtype=torch.float64, device=DEV).index_add_(0, ni, torch.exp(-0.5 * kappa * nd2 - l_kappa)) / Q
    logZ = torch.full((Q,), math.nan, dtype=torch.float64, device=DEV)
    logZ[near] = torch.log(Z)
    lp = torch.log_softmax(logp.double(), dim=1)
    for b in range(2):
        refs, E = {}, None
        for name, keep in (("lo", d2 <= cut - delta), ("hi", d2 <= cut + delta)):
            ii, jj, dd = i[keep], j[keep], d2[keep]
            t = lp[b][jj] - logZ[jj] - 0.5 * kappa * dd - l_kappa
            top = torch.full((len(rows),), -math.inf, dtype=torch.float64, device=DEV).scatter_reduce(0, ii, t, "amax")
            refs[name] = top + torch.log(torch.zeros(len(rows), dtype=torch.float64, device=DEV).index_add_(0, ii, torch.exp(t - top[ii])))
            E = torch.zeros(len(rows), dtype=torch.float64, device=DEV).scatter_reduce(
                0, ii, torch.where(t == top[ii], 0.5 * kappa * dd + (lp[b][jj] - logZ[jj]).abs(), torch.zeros_like(t)), "amax")
        # the bound: the second pass's gate 1e-6 E + 4e-6 with E of the largest term; the first pass's gate on log Z, whose largest term
        # is the row itself (E = 0): 4e-6; the one fp32 rounding of the log-weights: 2^-24 |lw| <= 6e-8 E
        bound = 1.06e-6 * E + 8e-6
        got = out[b][rows].double()
        beyond = torch.maximum(refs["lo"] - got, got - refs["hi"])
        print("level 4 image %d: worst distance beyond the bracket / bound %.3f (the bracket is up to %.3g wide)" % (
            b, float((beyond / bound).max()), float((refs["hi"] - refs["lo"]).max())))
        assert torch.isfinite(got).all() and (beyond <= bound).all()


def test_grid_filter_step_is_the_normalised_product_and_concentrates():
    level, kappa, radius = 3, 264.0, 15.0
    grid, off = device_grid(level, "fixed")
    Q = grid.shape[0]
    g64 = grid.cpu().numpy().astype(np.float64)
    prior = dev(two_mode_logp(grid))
    like = dev(mf_log_density(g64, MODE_A, 20.0).astype(np.float32)[None])
    step = harness.grid_filter_step(prior, like, grid, level, kappa, radius_deg=radius, offset=off)
    assert set(step) == {"posterior", "log_evidence", "predicted"} and step["posterior"].dtype == torch.float32
    assert torch.equal(step["predicted"], harness.grid_diffuse_local(prior, grid, level, kappa, radius, off))
    joint = step["predicted"].double() + like.double()
    ev = torch.logsumexp(joint, dim=1) - math.log(Q)
    assert (step["log_evidence"] - ev).abs().max() <= 1e-12 and step["log_evidence"].dtype == torch.float64
    assert (step["posterior"].double() - (joint - ev[:, None])).abs().max() <= 1e-6 * joint.abs().max() + 1e-6      # one fp32 rounding
    assert (torch.logsumexp(step["posterior"].double(), 1) - math.log(Q)).abs().max() <= 2e-6
    # five steps against the fp64 filter: the same operator from fp64 pairs
    near_a = dev(np.einsum("qij,ij->q", g64, MODE_A) > 1.0 + 2.0 * math.cos(math.radians(30.0)))     # within 30 degrees of the true mode
    post, post64 = prior, prior.double()
    pairs = pairs_within(grid, grid, hl.chord2(radius))
    for _ in range(5):
        post = harness.grid_filter_step(post, like, grid, level, kappa, radius_deg=radius, offset=off)["posterior"]
        j64 = diffuse_fp64(post64, grid, kappa, None, pairs) + like.double()
        post64 = j64 - (torch.logsumexp(j64, dim=1, keepdim=True) - math.log(Q))
    mass = float(torch.softmax(post.double(), 1)[0][near_a].sum())
    mass64 = float(torch.softmax(post64, 1)[0][near_a].sum())
    start = float(torch.softmax(prior.double(), 1)[0][near_a].sum())
    print("mass within 30 degrees of the true mode: prior %.4f, after five steps %.6f (fp64 filter %.6f)" % (start, mass, mass64))
    assert start < 0.7 and mass > 0.9 and mass > mass64 - 0.01


def test_grid_pose_filter_on_a_small_conditional_flow():
    cfg = make_config(layers=3, condition=1, feature_dim=16, rot="16Trans")
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=4, regime="default")
    fl = product_flow(cfg, w)
    T, level = 3, 2
    feat = torch.from_numpy(synth.features(T, 16, seed=1)).cuda()
    O = torch.from_numpy(synth.uniform_rotations(1, seed=9)[0])
    res = harness.grid_pose_filter(fl, feat, 64.0, recursion_level=level, offset=O)
    Q = 72 * 8 ** level
    assert tuple(res["est"].shape) == (T, 3, 3) and tuple(res["index"].shape) == (T,) and tuple(res["log_evidence"].shape) == (T,)
    assert tuple(res["posterior"].shape) == (Q,) and tuple(res["grid"].shape) == (Q, 3, 3)
    assert torch.isfinite(res["est"]).all() and torch.isfinite(res["log_evidence"]).all() and torch.isfinite(res["posterior"]).all()
    assert abs(float(torch.logsumexp(res["posterior"].double(), 0)) - math.log(Q)) <= 2e-6
    est, best, index, _ = harness.grid_estimate_rotations(fl, feat, recursion_level=level, offset=O)
    assert int(res["index"][0]) == int(index[0]) and torch.equal(res["est"][0], est[0])      # frame 0: a uniform prior
    assert torch.equal(res["est"], res["grid"][res["index"]])
    again = harness.grid_pose_filter(fl, feat, 64.0, recursion_level=level, offset=O, images_per_launch=1)
    assert torch.equal(again["index"], res["index"])
    cfg = make_config(layers=2, condition=1, feature_dim=16, lu=1)          # Condition16TransLU: batch-coupled
    coupled = product_flow(cfg, synth.fill_state_dict(orc.state_shapes(cfg), seed=5, regime="trained"))
    with pytest.raises(ValueError, match="batch-coupled"):
        harness.grid_pose_filter(coupled, feat, 64.0, recursion_level=1)
