"""CPU: the max-plus pass over the SO(3) grid's neighbourhoods (csrc/so3_grid_local.h, rnf_so3_grid_local_max) and the fp64 references
of what is built on it (grid_viterbi, grid_smooth); tests/test_gpu_so3_grid_viterbi.py imports the references, the cases and the checks.

``local_max_fp64`` is the numpy fp64 restatement: brute force over ALL Q rows with the mask d^2 <= cut, from the same fp32 inputs.  As
for the sum (tests/test_so3_grid_local_host.py) the fp32 membership and the fp64 d^2 may disagree within delta of the cut, so the
restatement gives a bracket: with excl = {d^2 <= cut - delta} and incl = {d^2 <= cut + delta},
    count_excl <= count <= count_incl,    max_excl - gate(E) <= out <= max_incl + gate(E),    arg in incl,
    |arg's own fp64 term - out| <= gate(E),      gate = 1e-6 E + 4e-6, E = (kappa/2) d^2 + |lw| of the largest term.
The recursions' references work on the neighbour lists of the fp64 distances; at the radii used no pair of grid rows lies within 9e-4
of the cut (against delta = 4e-6), so the fp32 and fp64 memberships agree and the reference is a single answer."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib
from tests.test_so3_grid_local_host import (KAPPAS, LEVELS, case, chord2, cuts_of, delta_of, dist2_fp64, grid_of, log_weights_of, offset_of,
                                            special_queries, thinned)
from tests.test_so3_kde_host import gate, log_normaliser, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_so3_grid_viterbi.cpp")
OUT = os.path.join(HERE, "csrc", "_host_so3_grid_viterbi.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f)
        for f in ("so3_grid_local.h", "so3_kernel_sum.h", "fisher_exact.h", "fisher_math.h")]


def _host_lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    return C.CDLL(OUT)


def host_local_max(level, grid, queries, kappa, d2_cut, log_weights=None, offset=None):
    """The host build of the kernel's arithmetic -> (float32 [G,m], int32 [G,m], int32 [m])"""
    h = _host_lib()
    Gr = np.ascontiguousarray(grid, np.float32).reshape(-1, 9)
    Qr = None if queries is None else np.ascontiguousarray(queries, np.float32).reshape(-1, 9)
    m = len(Gr) if Qr is None else len(Qr)
    lw = None if log_weights is None else np.ascontiguousarray(log_weights, np.float32).reshape(-1, len(Gr))
    G = 1 if lw is None else len(lw)
    off = None if offset is None else np.ascontiguousarray(offset, np.float32).reshape(9)
    out, arg, count = np.empty((G, m), np.float32), np.empty((G, m), np.int32), np.empty(m, np.int32)
    h.hsgv_local_max(int(level), ptr(off), ptr(Gr), ptr(Qr), ptr(lw), C.c_longlong(m), G, C.c_double(kappa), C.c_double(d2_cut), ptr(out), ptr(arg),
                     ptr(count))
    return out, arg, count


# ---- the restatement of the pass ---------------------------------------------------------------------------------------------------------

def check_max(out, arg, count, d2, kappa, d2_cut, log_weights, what):
    """out, arg [G,m] and count [m] against the bracket from the fp64 distances d2 [m,Q] (numpy) -> the worst distance beyond the
    bracket in gates.  No NaN log-weight is expected here (check_max_sentinels has them)."""
    m, Q = d2.shape
    lw = np.zeros((1, Q)) if log_weights is None else np.asarray(log_weights, np.float32).reshape(-1, Q).astype(np.float64)
    out, arg = np.asarray(out, np.float64).reshape(len(lw), m), np.asarray(arg).reshape(len(lw), m)
    l_kappa, delta = float(log_normaliser(kappa)), delta_of(d2_cut)
    excl, incl = d2 <= d2_cut - delta, d2 <= d2_cut + delta
    assert (excl.sum(axis=1) <= count).all() and (count <= incl.sum(axis=1)).all(), (what, "count")
    rows, worst = np.arange(m), 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(len(lw)):
            term = lw[g][None, :] - 0.5 * kappa * d2 - l_kappa
            E_all = 0.5 * kappa * d2 + np.abs(np.nan_to_num(lw[g], posinf=0.0, neginf=0.0))[None, :]
            t_lo, t_hi = np.where(excl, term, -np.inf), np.where(incl, term, -np.inf)
            lo, hi = t_lo.max(axis=1), t_hi.max(axis=1)
            E = np.maximum(np.where(np.isfinite(lo), E_all[rows, t_lo.argmax(axis=1)], 0.0), np.where(np.isfinite(hi), E_all[rows, t_hi.argmax(axis=1)], 0.0))
            gt = gate(E)
            assert not np.isnan(out[g]).any(), what
            assert (out[g] >= lo - gt).all(), (what, g, "below the bracket", float(np.max(lo - out[g] - gt)))
            assert (out[g] <= hi + gt).all(), (what, g, "above the bracket", float(np.max(out[g] - hi - gt)))
            live = np.isfinite(out[g])
            assert ((arg[g] >= 0) == live).all() and (arg[g][~live] == -1).all() and (arg[g] < Q).all(), (what, g, "arg")
            a = np.where(live, arg[g], 0)
            assert incl[rows, a][live].all(), (what, g, "arg is no member")
            own = term[rows, a]
            gown = gate(np.maximum(E, E_all[rows, a]))
            assert (np.abs(own - out[g])[live] <= gown[live]).all(), (what, g, "arg's own term", float(np.max((np.abs(own - out[g]) / gown)[live])))
            fin = live & np.isfinite(lo)
            if fin.any():
                worst = max(worst, float(np.max((np.maximum(lo - out[g], out[g] - hi) / gt)[fin])))
    return worst


def check_max_level(fn, level, kind, kappas=KAPPAS, pick=None):
    """``fn(level, grid, queries, kappa, d2_cut, log_weights, offset)`` -> (out, arg, count) against the bracket for every cut and kappa"""
    grid, queries, d2, n_grid = case(level, kind)
    if pick is not None:
        queries, d2 = queries[pick], d2[pick]
        off_grid = np.asarray(pick) >= n_grid
    else:
        off_grid = np.arange(len(queries)) >= n_grid
    nearest = float(d2[off_grid].min()) if off_grid.any() else 1e-3
    lw = log_weights_of(len(grid), 2, level)[1:]                           # one row, half of its entries -inf
    worst = 0.0
    for cut in cuts_of(level, nearest):
        for kappa in kappas:
            for w in (None, lw):
                out, arg, count = fn(level, grid, queries, kappa, cut, w, offset_of(kind))
                worst = max(worst, check_max(out, arg, count, d2, kappa, cut, w, (level, kind, cut, kappa, w is not None)))
                if cut == 8.0:
                    assert (count == len(grid)).all()
    print("level %d offset %s: worst distance beyond the bracket / gate %.3f" % (level, kind, worst))


def check_max_ties(fn, level=1, kind="fixed"):
    """kappa = 0 and zero weights: every member ties, the smallest row wins; the grid rows as queries with zero weights: arg[i] == i"""
    grid, queries, d2, n_grid = case(level, kind)
    Q = len(grid)
    first = lambda mask: np.where(mask.any(axis=1), mask.argmax(axis=1), Q)            # noqa: E731  the smallest member (Q: none)
    for cut in (chord2(20.0), chord2(40.0), chord2(90.0), 8.0):
        delta = delta_of(cut)
        for w in (None, np.zeros((2, Q), np.float32)):
            out, arg, count = fn(level, grid, queries, 0.0, cut, w, offset_of(kind))
            lo, hi = first(d2 <= cut + delta), first(d2 <= cut - delta)
            for g in range(len(arg)):
                a = np.where(arg[g] < 0, Q, arg[g])
                assert (lo <= a).all() and (a <= hi).all(), (cut, g)
                assert (out[g][arg[g] >= 0] == 0.0).all()                               # l(0) = 0 and every term is 0
    for kappa, cut in ((4.0, chord2(40.0)), (64.0, 0.0), (1e4, 8.0)):
        out, arg, count = fn(level, grid, grid, kappa, cut, None, offset_of(kind))
        assert np.array_equal(arg[0], np.arange(Q)), (kappa, cut)


def check_max_sentinels(fn, level=1, kind="fixed"):
    grid = grid_of(level, kind)
    Q = len(grid)
    queries, _ = special_queries(level, kind)
    d2 = dist2_fp64(grid, queries)
    cut, delta = chord2(40.0), delta_of(chord2(40.0))
    assert not ((d2 > cut - delta) & (d2 <= cut + delta)).any()             # no pair at the cut: the sets are exact
    inside = d2 <= cut
    off = offset_of(kind)
    lw = np.zeros((3, Q), np.float32)
    lw[0, inside[0]] = -np.inf                                              # query 0: a massless neighbourhood
    lw[1, np.flatnonzero(inside[1])[0]] = np.nan                            # query 1: a NaN inside
    lw[2, np.flatnonzero(inside[2])[::2]] = -np.inf                         # query 2: half of its rows drop out
    out, arg, count = fn(level, grid, queries, 16.0, cut, lw, off)
    assert np.array_equal(count, inside.sum(axis=1))
    assert np.isneginf(out[0, 0]) and arg[0, 0] == -1 and np.isnan(out[1, 1]) and arg[1, 1] == -1
    nan_in = inside[:, np.isnan(lw[1])].any(axis=1)
    assert np.array_equal(np.isnan(out[1]), nan_in) and (arg[1][nan_in] == -1).all() and (arg[1][~nan_in] >= 0).all()
    assert np.isfinite(out[2, 2]) and arg[2, 2] >= 0 and np.isfinite(lw[2, arg[2, 2]]) and inside[2, arg[2, 2]]
    check_max(out[[0, 2]], arg[[0, 2]], count, d2, 16.0, cut, lw[[0, 2]], "sentinels")
    out, arg, count = fn(level, grid, queries, 16.0, 0.0, None, off)         # off-grid queries at cut 0: empty neighbourhoods
    assert np.isneginf(out).all() and (arg == -1).all() and (count == 0).all()
    bad = queries.copy()
    bad[3, 1, 1], bad[5, 0, 2] = np.nan, np.inf
    bad[7] *= 4.0                                                           # finite, further than any cut from every rotation
    out, arg, count = fn(level, grid, bad, 16.0, cut, None, off)
    assert np.isnan(out[0, [3, 5]]).all() and (count[[3, 5]] == 0).all() and (arg[0, [3, 5]] == -1).all()
    assert np.isneginf(out[0, 7]) and count[7] == 0 and arg[0, 7] == -1
    rest = np.delete(np.arange(len(bad)), [3, 5, 7])
    assert np.isfinite(out[0, rest]).all() and (arg[0, rest] >= 0).all() and np.array_equal(count[rest], inside.sum(axis=1)[rest])


# ---- the model of the recursions in fp64, on neighbour lists --------------------------------------------------------------------------

RECURSION_CASES = ((1, 40.0), (2, 25.0), (2, 40.0))     # (level, radius in degrees); neighbourhoods of 9-12, 17-23 and 79-86 rows
T_FRAMES, B_SEQ, KAPPA = 6, 3, 64.0
BUMP_KAPPA = 30.0                                       # concentration of the likelihood's bumps: a width of 1 / sqrt(30) rad = 10.5 degrees


class Model:
    """The truncated motion kernel among the grid rows in fp64: nbr [Q,K] the members of N(i) (padded with -1), lk [Q,K] log k (padded
    with -inf), log_z [Q] = log Z_j, gap = the smallest |d^2 - cut| over all pairs"""

    def __init__(self, grid, kappa, radius_deg):
        g = np.asarray(grid, np.float32)
        self.Q, self.kappa, self.cut = len(g), kappa, chord2(radius_deg)
        lists, gap = [], np.inf
        for i0 in range(0, self.Q, 512):
            d2 = dist2_fp64(g, g[i0:i0 + 512])
            gap = min(gap, float(np.abs(d2 - self.cut).min()))
            for row in d2:
                j = np.flatnonzero(row <= self.cut)
                lists.append((j, row[j]))
        K = max(len(j) for j, _ in lists)
        self.gap, self.sizes = gap, (min(len(j) for j, _ in lists), K)
        self.nbr = np.full((self.Q, K), -1, np.int64)
        self.lk = np.full((self.Q, K), -np.inf)
        for i, (j, d) in enumerate(lists):
            self.nbr[i, :len(j)] = j
            self.lk[i, :len(j)] = -0.5 * kappa * d - float(log_normaliser(kappa))
        self.log_z = _lse(self.lk, axis=1) - math.log(self.Q)

    def gather(self, v):
        """v [.., Q] -> its values on the neighbour lists [.., Q, K] (-inf on the padding)"""
        return np.where(self.nbr >= 0, v[..., np.maximum(self.nbr, 0)], -np.inf)

    def diffuse(self, logp):
        """grid_diffuse_local's definition: log sum_{j in N(i)} softmax(logp)_j k / Z_j   [.., Q]"""
        lw = logp - _lse(logp, axis=-1)[..., None] - self.log_z
        return _lse(self.gather(lw) + self.lk, axis=-1)

    def initial(self, log_prior, shape):
        return np.zeros(shape) if log_prior is None else np.broadcast_to(self.diffuse(np.asarray(log_prior, np.float64)), shape)


def _lse(x, axis):
    with np.errstate(invalid="ignore", divide="ignore"):
        top = np.max(x, axis=axis, keepdims=True)
        safe = np.where(np.isfinite(top), top, 0.0)
        return np.squeeze(safe, axis) + np.log(np.exp(x - safe).sum(axis=axis))


@functools.lru_cache(maxsize=8)
def model_of(level, kind, radius_deg, kappa=KAPPA):
    return Model(grid_of(level, kind), kappa, radius_deg)


def viterbi_fp64(model, ll, log_prior=None):
    """The dense Viterbi optimum of ll [B,T,Q] (fp32 values) -> dict(path [B,T], score [B], W: the largest finite magnitude among the
    re-centred delta, log Z and the log-likelihoods -- what the device's recursion stores in fp32)"""
    ll = np.asarray(ll, np.float32).astype(np.float64)
    B, T, Q = ll.shape
    log_q = math.log(Q)
    delta = model.initial(log_prior, (B, Q)) - log_q + ll[:, 0]
    finite = lambda x: float(np.abs(x[np.isfinite(x)]).max())                          # noqa: E731
    W = max(finite(ll), finite(model.log_z), finite(delta - delta.max(axis=1, keepdims=True)))
    back = np.zeros((T, B, Q), np.int64)
    for t in range(1, T):
        cand = model.gather(delta - model.log_z) + model.lk                            # [B,Q,K]
        k = cand.argmax(axis=2)
        back[t] = model.nbr[np.arange(Q)[None, :], k]
        delta = ll[:, t] + cand.max(axis=2) - log_q
        W = max(W, finite(delta - delta.max(axis=1, keepdims=True)))
    path = np.zeros((B, T), np.int64)
    path[:, T - 1] = delta.argmax(axis=1)
    for t in range(T - 1, 0, -1):
        path[:, t - 1] = back[t][np.arange(B), path[:, t]]
    return dict(path=path, score=delta.max(axis=1), W=W)


def joint_fp64(model, ll, path, log_prior=None):
    """log p(path, y) [B] of paths [B,T] in fp64 (-inf where a step leaves its neighbourhood), and the largest fp64 d^2 of a step"""
    ll = np.asarray(ll, np.float32).astype(np.float64)
    B, T, Q = ll.shape
    rows = np.arange(B)
    total = model.initial(log_prior, (B, Q))[rows, path[:, 0]] - math.log(Q) + ll[rows, 0, path[:, 0]]
    worst = 0.0
    for t in range(1, T):
        j, i = path[:, t - 1], path[:, t]
        hit = model.nbr[i] == j[:, None]
        lk = np.where(hit.any(axis=1), model.lk[i, hit.argmax(axis=1)], -np.inf)
        worst = max(worst, float(np.max(-(lk + float(log_normaliser(model.kappa))) / (0.5 * model.kappa))) if model.kappa > 0 else 0.0)
        total = total + lk - model.log_z[j] - math.log(Q) + ll[rows, t, i]
    return total, worst


def forward_backward_fp64(model, ll, log_prior=None):
    """-> dict(filtered, smoothed, backward [B,T,Q], evidence [B,T], W): the forward-backward recursion of grid_smooth in fp64 (frame 0 of
    a uniform prior: its normalised likelihood, nothing diffused)"""
    ll = np.asarray(ll, np.float32).astype(np.float64)
    B, T, Q = ll.shape
    log_q = math.log(Q)
    filtered, evidence = np.empty((B, T, Q)), np.empty((B, T))
    post = None if log_prior is None else np.broadcast_to(np.asarray(log_prior, np.float64), (B, Q))
    for t in range(T):
        joint = ll[:, t] + (0.0 if post is None else model.diffuse(post))
        evidence[:, t] = _lse(joint, axis=1) - log_q
        post = filtered[:, t] = joint - evidence[:, t, None]
    backward = np.zeros((B, T, Q))
    for t in range(T - 2, -1, -1):
        backward[:, t] = _lse(model.gather(ll[:, t + 1] + backward[:, t + 1]) + model.lk, axis=2) - model.log_z - log_q - evidence[:, t + 1, None]
    smoothed = filtered + backward
    finite = lambda x: float(np.abs(x[np.isfinite(x)]).max())                          # noqa: E731
    return dict(filtered=filtered, smoothed=smoothed, backward=backward, evidence=evidence,
                W=max(finite(ll), finite(model.log_z), finite(filtered), finite(backward), finite(ll[:, 1:] + backward[:, 1:])))


def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = math.radians(deg)
    return np.eye(3) + math.sin(r) * K + (1.0 - math.cos(r)) * K @ K


def trajectory(seed, T=T_FRAMES, step_deg=10.0):
    """T rotations [T,3,3] fp64 turning ``step_deg`` per frame about a fixed axis, from a seeded start"""
    rng = np.random.default_rng(seed)
    start, axis = _rot(rng.standard_normal(3), rng.uniform(0, 180)), rng.standard_normal(3)
    return np.stack([start @ _rot(axis, step_deg * t) for t in range(T)])


def bumps(grid, centres, weights, kappa=BUMP_KAPPA):
    """log sum_c weights_c exp(-(kappa/2) |G - centres_c|_F^2) on the grid rows, fp32 [Q]"""
    g = np.asarray(grid, np.float64)
    d2 = ((g[None] - np.asarray(centres)[:, None]) ** 2).sum(axis=(2, 3))
    return _lse(np.log(np.asarray(weights))[:, None] - 0.5 * kappa * d2, axis=0).astype(np.float32)


@functools.lru_cache(maxsize=8)
def sequences(level, kind, B=B_SEQ, T=T_FRAMES):
    """Log-likelihoods [B,T,Q] fp32: two matrix-Fisher bumps per frame, one on a trajectory that turns 10 degrees per frame, one (the
    lighter) on a second trajectory"""
    grid = grid_of(level, kind)
    out = np.empty((B, T, len(grid)), np.float32)
    for b in range(B):
        main, other = trajectory(100 + b, T), trajectory(200 + b, T)
        for t in range(T):
            out[b, t] = bumps(grid, [main[t], other[t]], [0.7, 0.3])
    out.setflags(write=False)
    return out


FLIP = np.diag([-1.0, -1.0, 1.0])                        # Rz(180 degrees): the two-fold symmetry
SYMMETRIC_ODDS = (0.3, -0.6, 0.6, -0.6, 0.6, -0.6)       # log(w_A / w_B) per frame: the running sum alternates about 0, weights about 1/2


@functools.lru_cache(maxsize=4)
def symmetric_sequence(level, kind):
    """A two-fold symmetric object: bumps at R_t and R_t Rz(180), the weights alternating about one half so that the filter's leading
    branch changes from frame to frame -> (ll [1,T,Q] fp32, the two branches [2,T,3,3])"""
    grid = grid_of(level, kind)
    main = trajectory(7)
    branches = np.stack([main, main @ FLIP])
    ll = np.stack([bumps(grid, branches[:, t], [1.0 / (1.0 + math.exp(-o)), 1.0 / (1.0 + math.exp(o))]) for t, o in enumerate(SYMMETRIC_ODDS)])
    return ll[None], branches


def recursion_tolerance(model, W, sums, stored):
    """The bound on a chained result: ``sums`` neighbour-limited passes, each within gate(E) of its fp64 value -- E = (kappa/2) d^2 + |lw|
    of a term is at most (kappa/2) cut + 2 W, lw being the difference of two stored numbers -- and ``stored`` fp32 intermediates of
    magnitude at most W, each off by up to 3 roundings of 2^-24 W (its own and those of the two fp32 numbers it was formed from)"""
    return sums * gate(0.5 * model.kappa * model.cut + 2.0 * W) + stored * 3.0 * 2.0 ** -24 * W


def angle_deg(a, b):
    """the rotation angle between a [..,3,3] and b [..,3,3] in degrees"""
    c = 0.5 * (np.einsum("...ij,...ij->...", np.asarray(a, np.float64), np.asarray(b, np.float64)) - 1.0)
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


# ---- tests -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["none", "fixed"])
@pytest.mark.parametrize("level", LEVELS)
def test_host_max_lies_in_the_bracket_for_every_cut_and_kappa(level, kind):
    """As for the sum: at level 2 every query runs every cut at kappa = 64, every eighth grid row and every special query the full product"""
    if level < 2:
        check_max_level(host_local_max, level, kind)
    else:
        check_max_level(host_local_max, level, kind, kappas=(64.0,))
        check_max_level(host_local_max, level, kind, pick=thinned(level, kind))


def test_host_max_ties_go_to_the_smallest_row():
    check_max_ties(host_local_max)
    check_max_ties(host_local_max, 0, "none")


def test_host_max_sentinels():
    check_max_sentinels(host_local_max)


def test_host_max_groups_and_null_queries():
    grid = grid_of(1, "fixed")
    lw = log_weights_of(len(grid), 5, 5)
    a = host_local_max(1, grid, None, 64.0, chord2(30.0), lw, offset_of("fixed"))
    b = host_local_max(1, grid, grid[::-1], 64.0, chord2(30.0), lw[3:4], offset_of("fixed"))
    assert np.array_equal(a[0][3, ::-1].view(np.int32), b[0][0].view(np.int32)) and np.array_equal(a[1][3, ::-1], b[1][0])
    assert np.array_equal(a[2][::-1], b[2])


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20


def _args(**kw):
    base = dict(level=2, offset=_FAKE, grid=_FAKE, queries=_FAKE * 2, log_weights=_FAKE, m=1000, G=3, kappa=64.0, d2_cut=0.5, out=_FAKE, arg=_FAKE,
                count=_FAKE)
    base.update(kw)
    return _lib.So3GridLocalMax(**base)


def _refused(a, text):
    L = _lib.lib()
    assert L.rnf_so3_grid_local_max(C.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert text in msg, msg


def test_c_abi_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.rnf_abi_version() == 8
    who = "RnfSo3GridLocalMax"
    aligned4 = who + ": offset, log_weights, out, arg and count must be 4-byte aligned"
    aligned16 = who + ": grid and queries must be 16-byte aligned"
    for bad, text in ((dict(level=-1), who + ".level=-1 outside 0..6"), (dict(level=7), who + ".level=7 outside 0..6"),
                      (dict(G=0), who + ".G=0 outside 1..65535"), (dict(G=65536), who + ".G=65536 outside 1..65535"),
                      (dict(m=-1), who + ".m=-1 outside 0..2^31-1"), (dict(m=1 << 31), who + ".m=2147483648 outside 0..2^31-1"),
                      (dict(kappa=-1.0), who + ".kappa=-1 outside 0..1e6"), (dict(kappa=1.0000001e6), "kappa="), (dict(kappa=float("nan")), "kappa=nan"),
                      (dict(d2_cut=-1e-9), who + ".d2_cut=-1e-09 outside 0..8"), (dict(d2_cut=8.0000001), "d2_cut="),
                      (dict(d2_cut=float("nan")), "d2_cut=nan"), (dict(d2_cut=float("inf")), "d2_cut=inf"),
                      (dict(grid=_FAKE + 4), aligned16), (dict(queries=_FAKE + 8), aligned16), (dict(out=_FAKE + 2), aligned4),
                      (dict(arg=_FAKE + 2), aligned4), (dict(log_weights=_FAKE + 1), aligned4), (dict(count=_FAKE + 2), aligned4),
                      (dict(offset=_FAKE + 3), aligned4),
                      (dict(queries=None), who + ": null queries stand for the grid rows, but m=1000 and level 2 has 4608"),
                      (dict(grid=None), who + ": null grid, out or arg"), (dict(out=None), who + ": null grid, out or arg"),
                      (dict(arg=None), who + ": null grid, out or arg")):
        _refused(_args(**bad), text)
    a = _args()
    a.struct_bytes += 8
    _refused(a, who + ".struct_bytes does not match the library's %d" % C.sizeof(_lib.So3GridLocalMax))
    assert L.rnf_so3_grid_local_max(C.byref(_args(m=0, out=None, grid=None, arg=None))) == 0     # m = 0 is a no-op


def test_header_declares_the_struct_the_binding_mirrors():
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    start = "typedef struct RnfSo3GridLocalMax {"
    body = header[header.index(start) + len(start):header.index("} RnfSo3GridLocalMax;")]
    names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
    assert names == [f for f, _ in _lib.So3GridLocalMax._fields_], names
    sum_fields = [f for f, _ in _lib.So3GridLocalSum._fields_]
    assert [f for f in names if f != "arg"] == sum_fields and names.index("arg") == names.index("out") + 1       # the sum's arguments, plus arg
    assert "rnf_so3_grid_local_max" in _lib.EXPORTS and "#define RNF_ABI_VERSION 8" in header
    assert "int rnf_so3_grid_local_max(const RnfSo3GridLocalMax *max);" in header
    assert "rnf_so3_grid_local_max_workspace_bytes" not in header                               # no workspace, no companion
    device = open(os.path.join(root, "rotationnormflow_amd", "csrc", "so3_grid_local.h")).read()
    assert device.count("const float d2 = ks::dist2(") == 1 and device.count("void sweep(") == 1  # ONE enumeration, shared by the passes


def test_python_entry_points_validate_their_arguments():
    from rotationnormflow_amd import grid_pose, harness
    from rotationnormflow_amd.utils import kde
    assert harness.so3_grid_local_log_max is kde.so3_grid_local_log_max
    for name in ("grid_viterbi", "grid_smooth", "grid_pose_smooth"):
        assert getattr(harness, name) is getattr(grid_pose, name)
    grid = torch.zeros(72, 3, 3)
    with pytest.raises(ValueError, match="so3_grid_local_log_max: grid is on the CPU.*no CPU fallback"):
        kde.so3_grid_local_log_max(grid, 0, 4.0)
    with pytest.raises(ValueError, match="so3_grid_local_log_max: grid"):
        kde.so3_grid_local_log_max(torch.zeros(72, 9), 0, 4.0)
    with pytest.raises(ValueError, match="level=7"):
        kde.so3_grid_local_log_max(grid, 7, 4.0)
    with pytest.raises(ValueError, match="level 1 has 576"):
        kde.so3_grid_local_log_max(grid, 1, 4.0)
    for fn in (grid_pose.grid_viterbi, grid_pose.grid_smooth):
        who = fn.__name__
        with pytest.raises(ValueError, match=who + ".*GPU only"):
            fn(torch.zeros(2, 3, 72), grid, 0, 4.0)
        with pytest.raises(ValueError, match=who + ": log_likelihood"):
            fn(torch.zeros(72), grid, 0, 4.0)
        with pytest.raises(ValueError, match=who + ": grid"):
            fn(torch.zeros(3, 72), torch.zeros(71, 3, 3), 0, 4.0)
        with pytest.raises(ValueError, match=who + ": grid holds 72 rows, level 1"):
            fn(torch.zeros(3, 72), grid, 1, 4.0)
        with pytest.raises(ValueError, match="at least one frame"):
            fn(torch.zeros(2, 0, 72), grid, 0, 4.0)
    with pytest.raises(ValueError, match="kappa is required"):
        grid_pose.grid_pose_smooth(None)


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_so3_grid_viterbi.cpp (its own main: the max pass at levels 0 to 2 at every cut, with -inf and NaN log-weights
    and non-finite queries) built with the host-side address and undefined-behaviour sanitizers (-Xarch_host: host code only, nothing
    for the GPU) and run as a process of its own."""
    exe = str(tmp_path / "sanitize_so3_grid_viterbi")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_so3_grid_viterbi.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)


# ---- the references themselves ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level,radius", RECURSION_CASES)
def test_no_pair_of_grid_rows_lies_at_the_recursions_cuts(level, radius):
    """What makes the fp64 reference of the recursions a single answer: the fp32 and fp64 memberships agree"""
    for kind in ("none", "fixed"):
        model = model_of(level, kind, radius)
        print("level %d radius %g offset %s: neighbourhoods of %d-%d rows, nearest pair %.2e from the cut" % ((level, radius, kind) + model.sizes + (model.gap,)))
        assert model.gap >= 9e-4 and model.gap > 100 * delta_of(model.cut)


def test_reference_viterbi_beats_every_perturbed_path_and_the_smoother_has_unit_mass():
    model = model_of(1, "fixed", 40.0)
    ll = sequences(1, "fixed")
    prior = bumps(grid_of(1, "fixed"), [trajectory(100)[0]], [1.0], 4.0)
    for lp in (None, prior):
        v = viterbi_fp64(model, ll, lp)
        score, worst = joint_fp64(model, ll, v["path"], lp)
        assert np.abs(score - v["score"]).max() <= 1e-9 and worst <= model.cut
        rng = np.random.default_rng(0)
        for _ in range(50):                                                 # no other path scores higher
            other = v["path"].copy()
            b, t = rng.integers(B_SEQ), rng.integers(T_FRAMES)
            other[b, t] = model.nbr[other[b, t], rng.integers((model.nbr[other[b, t]] >= 0).sum())]
            assert (joint_fp64(model, ll, other, lp)[0] <= score + 1e-9).all()
        fb = forward_backward_fp64(model, ll, lp)
        mass = _lse(fb["smoothed"], axis=2) - math.log(model.Q)
        assert np.abs(mass).max() <= 1e-10 and np.abs(_lse(fb["filtered"], axis=2) - math.log(model.Q)).max() <= 1e-10
        one = viterbi_fp64(model, ll[:, :1], lp)                            # T = 1: the arg-max of pi_0 l_0
        assert np.array_equal(one["path"][:, 0], (model.initial(lp, ll[:, 0].shape) + ll[:, 0]).argmax(axis=1))


@pytest.mark.parametrize("level,radius", [(2, 25.0), (2, 40.0)])
def test_the_symmetric_sequence_makes_the_fp64_filter_hop_and_the_fp64_path_stay(level, radius):
    """The precondition of the feature's test, on the reference: the fp64 filter's per-frame arg-max jumps beyond the radius at least
    once; the fp64 Viterbi path never does and stays on one branch"""
    model = model_of(level, "fixed", radius)
    ll, branches = symmetric_sequence(level, "fixed")
    grid = grid_of(level, "fixed")
    fb = forward_backward_fp64(model, ll)
    hops = angle_deg(grid[fb["filtered"][0].argmax(axis=1)][1:], grid[fb["filtered"][0].argmax(axis=1)][:-1])
    print("filter arg-max steps (degrees):", np.round(hops, 1))
    assert (hops > radius).sum() >= 1
    path = viterbi_fp64(model, ll)["path"][0]
    assert (angle_deg(grid[path][1:], grid[path][:-1]) <= radius).all()
    assert branch_distance(grid[path], branches, level).min() <= 0.0


def branch_distance(est, branches, level):
    """[2]: for either branch, the largest angle from est [T,3,3] to it minus (the grid spacing + the bump width), in degrees"""
    allowed = 360.0 / (6 * 2 ** level) + math.degrees(1.0 / math.sqrt(BUMP_KAPPA))
    return np.array([angle_deg(est, branches[s]).max() - allowed for s in range(2)])
