"""CPU: the anisotropic variant of the neighbour-limited passes (csrc/so3_grid_local.h, rnf_so3_grid_local_fisher), the motion models
built on it (utils/kde.py: motion_factors, motion_matrix; grid_pose: the ``motion`` keyword), and their fp64 references.

A member's term is lw - 1/2 tr(W K W^T) - l(K), W = Q_i - G_j, membership the isotropic passes' fp32 d^2 <= cut.  The restatement is brute
force over ALL rows in fp64 from the same fp32 inputs; as in tests/test_so3_grid_local_host.py it gives a BRACKET between the sets
d^2 <= cut -+ delta, delta = delta_of(cut), with the gate 1e-6 E + 4e-6, E = (|K|_F / 2) d^2 + |lw| of the largest term (|K|_F bounds the
largest |eigenvalue|, so E bounds the magnitude of the numbers the term is formed from).  ``MotionModel`` and the three recursions below
are the fp64 references of grid_diffuse_local, grid_filter_step, grid_smooth and grid_viterbi with a motion;
tests/test_gpu_so3_grid_local_fisher.py imports them, the cases and the checks."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib, synth
from tests import fisher_exact as fe
from tests.test_so3_grid_local_host import (check_bracket, chord2, delta_of, dist2_fp64, grid_of, log_weights_of, offset_of, spacing_deg,
                                            special_queries)
from tests.test_so3_grid_viterbi_host import _lse, _rot, bumps
from tests.test_so3_kde_host import gate, log_normaliser, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_so3_grid_local_fisher.cpp")
OUT = os.path.join(HERE, "csrc", "_host_so3_grid_local_fisher.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f)
        for f in ("so3_grid_local.h", "so3_kernel_sum.h", "fisher_exact.h", "fisher_math.h")]
LEVELS = (0, 1, 2)
_U, _, _VT = np.linalg.svd(synth.uniform_rotations(1, seed=77).astype(np.float64).reshape(3, 3))
V_AXES = _U @ _VT                                                                      # the fixed random principal axes, orthogonal in fp64
SPECTRA = ((64.0, 64.0, 64.0), (200.0, 5.0, 5.0), (40.0, 12.0, -3.0), (1e4, 1e4, 1e4), (0.0, 0.0, 0.0))
DRIFT = _rot((0.3, -0.5, 0.8), 11.0)                                                   # the shift of the second set of queries


def concentration_of(s, V=V_AXES):
    """V diag(s) V^T, symmetric to the last bit; kappa I exactly where the three values agree"""
    if s[0] == s[1] == s[2]:
        return s[0] * np.eye(3)
    K = (V * np.asarray(s, np.float64)) @ V.T
    return 0.5 * (K + K.T)


KS = tuple(concentration_of(s) for s in SPECTRA)


def _host_lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    h = C.CDLL(OUT)
    h.hsglf_log_normaliser.restype = h.hsglf_log_normaliser_iso.restype = C.c_double
    return h


def _host_call(fn, level, grid, queries, shape, d2_cut, log_weights, offset, with_arg):
    Gr = np.ascontiguousarray(grid, np.float32).reshape(-1, 9)
    Qr = None if queries is None else np.ascontiguousarray(queries, np.float32).reshape(-1, 9)
    m = len(Gr) if Qr is None else len(Qr)
    lw = None if log_weights is None else np.ascontiguousarray(log_weights, np.float32).reshape(-1, len(Gr))
    G = 1 if lw is None else len(lw)
    off = None if offset is None else np.ascontiguousarray(offset, np.float32).reshape(9)
    out, count = np.empty((G, m), np.float32), np.empty(m, np.int32)
    arg = np.empty((G, m), np.int32) if with_arg else None
    fn(int(level), ptr(off), ptr(Gr), ptr(Qr), ptr(lw), C.c_longlong(m), G, shape, C.c_double(d2_cut), ptr(out), ptr(arg), ptr(count))
    return (out, arg, count) if with_arg else (out, count)


def host_local_fisher(level, grid, queries, K, d2_cut, log_weights=None, offset=None, with_arg=False):
    """The host build of the anisotropic arithmetic -> (float32 [G,m], int32 [m]), with ``with_arg`` (out, int32 arg [G,m], count)"""
    Kc = np.ascontiguousarray(K, np.float64).reshape(9)
    return _host_call(_host_lib().hsglf_local, level, grid, queries, ptr(Kc), d2_cut, log_weights, offset, with_arg)


def host_local_iso(level, grid, queries, kappa, d2_cut, log_weights=None, offset=None, with_arg=False):
    return _host_call(_host_lib().hsglf_local_iso, level, grid, queries, C.c_double(kappa), d2_cut, log_weights, offset, with_arg)


def host_log_normaliser(K):
    return float(_host_lib().hsglf_log_normaliser(ptr(np.ascontiguousarray(K, np.float64).reshape(9))))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def eigenvalues(K):
    return np.linalg.eigvalsh(0.5 * (np.asarray(K, np.float64) + np.asarray(K, np.float64).T))[::-1]


def log_normaliser_fisher(K):
    """l(K) = c(K) - tr K from the exact reference of tests/fisher_exact.py"""
    s = eigenvalues(K)
    return 0.0 if not s.any() else float(fe.log_c(s) - s.sum())


def quad_fp64(grid, queries, K):
    """1/2 tr(W K W^T) [m,Q], W = Q_i - G_j, in fp64 from the fp32 entries: 1/2 (tr Q K Q^T + tr G K G^T) - tr(Q K G^T), whose
    cancellation costs 1e-16 |K| |entries|^2 -- 1e-11 at the largest K here, far below the gate"""
    K = np.asarray(K, np.float64)
    K = 0.5 * (K + K.T)
    Gr = np.asarray(grid, np.float32).astype(np.float64).reshape(-1, 3, 3)
    Qr = np.asarray(queries, np.float32).astype(np.float64).reshape(-1, 3, 3)
    gk, qk = Gr @ K, Qr @ K
    a, b = np.einsum("irc,irc->i", qk, Qr), np.einsum("jrc,jrc->j", gk, Gr)
    return 0.5 * (a[:, None] + b[None, :]) - qk.reshape(len(Qr), 9) @ Gr.reshape(len(Gr), 9).T


def local_fisher_fp64(d2, quad, K, d2_cut, log_weights=None):
    """The bracket of tests/test_so3_grid_local_host.py's local_sum_fp64 on the anisotropic term, with the max-plus pass next to it
    -> dict(lo, hi, count_lo, count_hi, E, max_lo, max_hi, E_max [G,m], term [G,m,Q] where it fits, Kn)"""
    m, Q = d2.shape
    lw = np.zeros((1, Q)) if log_weights is None else np.asarray(log_weights, np.float32).reshape(-1, Q).astype(np.float64)
    l_k, delta, Kn = log_normaliser_fisher(K), delta_of(d2_cut), float(np.linalg.norm(K))
    res = {}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for name, mask in (("lo", d2 <= d2_cut - delta), ("hi", d2 <= d2_cut + delta)):
            res["count_" + name] = mask.sum(axis=1)
            vals, Es, tops = [], [], []
            for g in range(len(lw)):
                t = np.where(mask, lw[g][None, :] - quad, -np.inf)
                nan = (mask & np.isnan(lw[g])[None, :]).any(axis=1)
                t = np.where(np.isnan(t), -np.inf, t)
                top, at = t.max(axis=1), t.argmax(axis=1)
                safe = np.where(np.isfinite(top), top, 0.0)
                v = safe + np.log(np.exp(t - safe[:, None]).sum(axis=1)) - l_k
                v = np.where(np.isfinite(top), v, -np.inf)
                vals.append(np.where(nan, np.nan, v))
                tops.append(np.where(nan, np.nan, top - l_k))
                Es.append(np.where(np.isfinite(top), 0.5 * Kn * d2[np.arange(m), at] + np.abs(np.nan_to_num(lw[g][at], posinf=0.0, neginf=0.0)), 0.0))
            res[name], res["E_" + name], res["max_" + name] = np.stack(vals), np.stack(Es), np.stack(tops)
    res["E"] = np.maximum(res["E_lo"], res["E_hi"])
    res["mask_hi"], res["lw"], res["l_k"], res["Kn"] = d2 <= d2_cut + delta, lw, l_k, Kn
    return res


def check_max_bracket(out, arg, count, ref, d2, quad, what):
    """The max-plus pass against the bracket: the value, the count, and the arg -- a member whose own fp64 term is the value within the
    gate -- as tests/test_so3_grid_viterbi_host.py's check_max"""
    out = np.asarray(out, np.float64)
    m, Q = d2.shape
    rows = np.arange(m)
    assert (ref["count_lo"] <= count).all() and (count <= ref["count_hi"]).all(), (what, "count")
    gt = gate(ref["E"])
    worst = 0.0
    for g in range(len(out)):
        lo, hi = ref["max_lo"][g], ref["max_hi"][g]
        assert not np.isnan(out[g]).any(), what
        assert (out[g] >= lo - gt[g]).all(), (what, g, "below the bracket", float(np.max(lo - out[g] - gt[g])))
        assert (out[g] <= hi + gt[g]).all(), (what, g, "above the bracket", float(np.max(out[g] - hi - gt[g])))
        live = np.isfinite(out[g])
        assert ((arg[g] >= 0) == live).all() and (arg[g][~live] == -1).all() and (arg[g] < Q).all(), (what, g, "arg")
        a = np.where(live, arg[g], 0)
        assert ref["mask_hi"][rows, a][live].all(), (what, g, "arg is no member")
        with np.errstate(invalid="ignore"):
            own = ref["lw"][g][a] - quad[rows, a] - ref["l_k"]
            E_own = 0.5 * ref["Kn"] * d2[rows, a] + np.abs(np.nan_to_num(ref["lw"][g][a], posinf=0.0, neginf=0.0))
            gown = gate(np.maximum(ref["E"][g], E_own))
            assert (np.abs(own - out[g])[live] <= gown[live]).all(), (what, g, "arg's own term")
            fin = live & np.isfinite(lo)
            if fin.any():
                worst = max(worst, float(np.max((np.maximum(lo - out[g], out[g] - hi) / gt[g])[fin])))
    return worst


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

def shifted_rows(grid, drift=DRIFT):
    """C = grid Delta in fp32, as grid_pose forms it: three fp32 products and two sums per entry"""
    g, d = np.asarray(grid, np.float32), np.asarray(drift, np.float64).astype(np.float32)
    return np.stack([g[..., 0] * d[0, c] + g[..., 1] * d[1, c] + g[..., 2] * d[2, c] for c in range(3)], axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=6)
def fisher_case(level, kind):
    """(grid, queries = every grid row, every row of the shifted grid, the special ones; fp64 distances [m,Q]; the number of grid rows)"""
    grid = grid_of(level, kind)
    extra, _ = special_queries(level, kind)
    queries = np.concatenate([grid, shifted_rows(grid), extra])
    d2 = dist2_fp64(grid, queries)
    for x in (queries, d2):
        x.setflags(write=False)
    return grid, queries, d2, len(grid)


def cuts_of(level):
    """0, one grid spacing, 15 and 60 degrees, and 8 (everything)"""
    return (0.0, chord2(spacing_deg(level)), chord2(15.0), chord2(60.0), 8.0)


def check_fisher_level(fn, level, kind, Ks=KS, pick=None, with_arg=False, weights=(False, True)):
    """``fn(level, grid, queries, K, d2_cut, log_weights, offset, with_arg)`` against the bracket for every cut and concentration;
    ``pick``: indices into the case's queries (default: all)"""
    grid, queries, d2, n_grid = fisher_case(level, kind)
    if pick is not None:
        queries, d2 = queries[pick], d2[pick]
    on_grid = (np.arange(len(fisher_case(level, kind)[1])) if pick is None else np.asarray(pick)) < n_grid
    lw = log_weights_of(len(grid), 2, level)[1:]                           # one row, half of its entries -inf
    worst = 0.0
    for K in Ks:
        quad = quad_fp64(grid, queries, K)
        for cut in cuts_of(level):
            for w in [lw if on else None for on in weights]:
                ref = local_fisher_fp64(d2, quad, K, cut, w)
                what = (level, kind, cut, tuple(np.round(eigenvalues(K), 3)), w is not None, with_arg)
                if with_arg:
                    out, arg, count = fn(level, grid, queries, K, cut, w, offset_of(kind), True)
                    worst = max(worst, check_max_bracket(out, arg, count, ref, d2, quad, what))
                else:
                    out, count = fn(level, grid, queries, K, cut, w, offset_of(kind), False)
                    worst = max(worst, check_bracket(out, count, ref, what))
                if cut == 0.0:
                    assert (count[on_grid] >= 1).all()
                if cut == 8.0:
                    assert (count == len(grid)).all()
    print("level %d offset %s %s: worst distance beyond the bracket / gate %.3f" % (level, kind, "max" if with_arg else "sum", worst))


def thinned(level, kind, stride=8):
    """Every ``stride``-th grid row and shifted row, and every special query of the case"""
    _, queries, _, n_grid = fisher_case(level, kind)
    return np.concatenate([np.arange(0, 2 * n_grid, stride), np.arange(2 * n_grid, len(queries))])


# ---- the fp64 references of the recursions with a motion ---------------------------------------------------------------------------------

def motion_factors_fp64(A):
    """(drift, concentration, s) by the proper SVD of tests/fisher_exact.py"""
    U, s, V = (x[0] for x in fe.proper_svd64(np.asarray(A, np.float64)))
    K = (V * s) @ V.T
    return U @ V.T, 0.5 * (K + K.T), s


class MotionModel:
    """The truncated transition of one motion A on the grid rows in fp64, from the fp32 rows and the fp32 shifted rows C the device
    forms.  By destination i: src [Q,Ka] the sources j with d^2(C_j, G_i) <= cut (padded with -1), lk [Q,Ka] log k(C_j, G_i); by source
    j: dst [Q,Kb], lk_t [Q,Kb]; log_z [Q] = log Z_j (-inf: an empty neighbourhood); gap = the smallest |d^2 - cut| over all pairs."""

    def __init__(self, grid, A, radius_deg):
        g = np.asarray(grid, np.float32)
        drift, K, s = motion_factors_fp64(A)
        self.Q, self.K, self.s, self.cut, self.Kn = len(g), K, s, chord2(radius_deg), float(np.linalg.norm(K))
        self.rows = shifted_rows(g, drift) if np.abs(drift - np.eye(3)).max() > 1e-7 else g
        l_k = log_normaliser_fisher(K)
        d2 = dist2_fp64(self.rows, g)                                       # [i, j]: destination G_i against source C_j
        self.gap = float(np.abs(d2 - self.cut).min())
        lk = np.where(d2 <= self.cut, -quad_fp64(self.rows, g, K) - l_k, -np.inf)
        self.src, self.lk = self._lists(lk)
        self.dst, self.lk_t = self._lists(lk.T)
        self.log_z = _lse(self.lk_t, axis=1) - math.log(self.Q)
        self.sizes = (int((d2 <= self.cut).sum(axis=0).min()), int((d2 <= self.cut).sum(axis=0).max()))

    @staticmethod
    def _lists(lk):
        member = np.isfinite(lk)
        width = int(member.sum(axis=1).max())
        order = np.argsort(~member, axis=1, kind="stable")[:, :width]       # the members first, in increasing index
        vals = np.take_along_axis(lk, order, axis=1)
        return np.where(np.isfinite(vals), order, -1), vals

    @staticmethod
    def gather(index, v):
        return np.where(index >= 0, v[..., np.maximum(index, 0)], -np.inf)

    def minus_log_z(self, x):
        with np.errstate(invalid="ignore"):
            return np.where(np.isneginf(self.log_z), -np.inf, x - self.log_z)

    def diffuse(self, logp):
        """log sum_{j in N(i)} softmax(logp)_j k(C_j, G_i) / Z_j   [.., Q]"""
        return _lse(self.gather(self.src, self.minus_log_z(logp - _lse(logp, axis=-1)[..., None])) + self.lk, axis=-1)

    def best(self, delta):
        """max_j and arg max_j (the smallest j on a tie) of delta_j - log Z_j + log k(C_j, G_i)"""
        cand = self.gather(self.src, self.minus_log_z(delta)) + self.lk
        k = cand.argmax(axis=-1)
        return cand.max(axis=-1), np.take_along_axis(np.broadcast_to(self.src, cand.shape), k[..., None], axis=-1)[..., 0]

    def backward(self, lw):
        """log sum_{i in N(j)} k(C_j, G_i) exp(lw_i) - log Z_j - log Q   [.., Q]; -inf where Z_j = 0"""
        return self.minus_log_z(_lse(self.gather(self.dst, lw) + self.lk_t, axis=-1)) - math.log(self.Q)


def _finite(x):
    x = np.asarray(x)
    return float(np.abs(x[np.isfinite(x)]).max()) if np.isfinite(x).any() else 0.0


def models_of(grid, motion, radius_deg, T):
    """One MotionModel per step 0 .. T-2 ([3,3]: the same one)"""
    motion = np.asarray(motion, np.float64)
    if motion.ndim == 2:
        return [MotionModel(grid, motion, radius_deg)] * max(T - 1, 1)
    built = {}
    return [built.setdefault(a.tobytes(), MotionModel(grid, a, radius_deg)) for a in motion]


def filter_fp64(models, ll, log_prior=None):
    """grid_smooth's forward chain -> (filtered [B,T,Q], evidence [B,T], predicted [B,T,Q]); frame 0 of a uniform prior is its normalised
    likelihood, a prior is taken through models[0]"""
    ll = np.asarray(ll, np.float32).astype(np.float64)
    B, T, Q = ll.shape
    filtered, evidence, predicted = np.empty((B, T, Q)), np.empty((B, T)), np.zeros((B, T, Q))
    post = None if log_prior is None else np.broadcast_to(np.asarray(log_prior, np.float64), (B, Q))
    for t in range(T):
        if post is not None:
            predicted[:, t] = models[max(t - 1, 0)].diffuse(post)
        joint = ll[:, t] + predicted[:, t]
        evidence[:, t] = _lse(joint, axis=1) - math.log(Q)
        post = filtered[:, t] = joint - evidence[:, t, None]
    return filtered, evidence, predicted


def smooth_fp64(models, ll, log_prior=None):
    """-> dict(filtered, smoothed, backward [B,T,Q], evidence [B,T], W) of grid_smooth with a motion"""
    ll = np.asarray(ll, np.float32).astype(np.float64)
    B, T, Q = ll.shape
    filtered, evidence, _ = filter_fp64(models, ll, log_prior)
    backward = np.zeros((B, T, Q))
    for t in range(T - 2, -1, -1):
        backward[:, t] = models[t].backward(ll[:, t + 1] + backward[:, t + 1]) - evidence[:, t + 1, None]
    both = filtered + backward
    smoothed = both - (_lse(both, axis=2) - math.log(Q))[..., None]
    W = max(_finite(ll), max(_finite(m.log_z) for m in models), _finite(filtered), _finite(backward), _finite(ll[:, 1:] + backward[:, 1:]))
    return dict(filtered=filtered, smoothed=smoothed, backward=backward, evidence=evidence, W=W)


def viterbi_fp64(models, ll, log_prior=None):
    """-> dict(path [B,T], score [B] = log p(path, y), W) of grid_viterbi with a motion"""
    ll = np.asarray(ll, np.float32).astype(np.float64)
    B, T, Q = ll.shape
    log_q = math.log(Q)
    first = np.zeros((B, Q)) if log_prior is None else np.broadcast_to(models[0].diffuse(np.asarray(log_prior, np.float64)), (B, Q))
    delta = first - log_q + ll[:, 0]
    W = max(_finite(ll), max(_finite(m.log_z) for m in models), _finite(delta - delta.max(axis=1, keepdims=True)))
    back = np.zeros((T, B, Q), np.int64)
    for t in range(1, T):
        best, back[t] = models[t - 1].best(delta)
        delta = ll[:, t] + best - log_q
        W = max(W, _finite(delta - delta.max(axis=1, keepdims=True)))
    path = np.zeros((B, T), np.int64)
    path[:, T - 1] = delta.argmax(axis=1)
    for t in range(T - 1, 0, -1):
        path[:, t - 1] = back[t][np.arange(B), path[:, t]]
    return dict(path=path, score=delta.max(axis=1), W=W)


def joint_fp64(models, ll, path, log_prior=None):
    """log p(path, y) [B] of paths [B,T] in fp64 (-inf where a step leaves its neighbourhood)"""
    ll = np.asarray(ll, np.float32).astype(np.float64)
    B, T, Q = ll.shape
    rows = np.arange(B)
    first = np.zeros((B, Q)) if log_prior is None else np.broadcast_to(models[0].diffuse(np.asarray(log_prior, np.float64)), (B, Q))
    total = first[rows, path[:, 0]] - math.log(Q) + ll[rows, 0, path[:, 0]]
    for t in range(1, T):
        mo, j, i = models[t - 1], path[:, t - 1], path[:, t]
        hit = mo.src[i] == j[:, None]
        lk = np.where(hit.any(axis=1), mo.lk[i, hit.argmax(axis=1)], -np.inf)
        total = total + lk - mo.log_z[j] - math.log(Q) + ll[rows, t, i]
    return total


def recursion_tolerance(models, W, sums, stored):
    """tests/test_so3_grid_viterbi_host.py's bound with E <= (|K|_F / 2) cut + 2 W of the loosest bound among the models"""
    E = max(0.5 * m.Kn * m.cut for m in models) + 2.0 * W
    return sums * gate(E) + stored * 3.0 * 2.0 ** -24 * W


# the recursions' cases: (level, radius), at or above the floor of a drifting model (37.5 and 18.75 degrees); no pair (C_j, G_i) lies
# within 8 delta of these cuts for DRIFT without an offset
RECURSION_CASES = ((1, 47.0), (2, 33.0))
MOTION_TIGHT = DRIFT @ concentration_of((200.0, 40.0, 40.0))                             # drifting and anisotropic
MOTION_SIGNED = DRIFT @ concentration_of((40.0, 12.0, -3.0))
T_FRAMES, B_SEQ = 4, 2


def time_varying(T=T_FRAMES):
    """[T-1,3,3]: two distinct matrices, the second one twice in a row"""
    other = _rot((0.3, -0.5, 0.8), 11.0) @ concentration_of((90.0, 60.0, 20.0))
    return np.stack([MOTION_TIGHT] + [other] * (T - 2))


@functools.lru_cache(maxsize=4)
def drift_sequences(level, kind="none", B=B_SEQ, T=T_FRAMES):
    """Log-likelihoods [B,T,Q] fp32: two bumps per frame, the heavier one on a trajectory that follows DRIFT from a seeded start"""
    grid = grid_of(level, kind)
    out = np.empty((B, T, len(grid)), np.float32)
    for b in range(B):
        rng = np.random.default_rng(300 + b)
        x, y = _rot(rng.standard_normal(3), rng.uniform(0, 180)), _rot(rng.standard_normal(3), rng.uniform(0, 180))
        for t in range(T):
            out[b, t] = bumps(grid, [x, y], [0.7, 0.3])
            x, y = x @ DRIFT, y @ _rot((1.0, 0.2, 0.0), 14.0)
    out.setflags(write=False)
    return out


# ---- the behaviour case: a two-mode likelihood turning 10 degrees per frame about body z ---------------------------------------------

TURN = _rot((0.0, 0.0, 1.0), 10.0)
SIGMA_DEG = (2.0, 2.0, 4.0)
KAPPA_MATCHED = 1.0 / (2.0 * math.radians(4.0) ** 2)          # isotropic: rotation-vector variance 1 / (2 kappa) = (4 degrees)^2


def turning_sequence(level, kind="none", T=6):
    """-> (ll [1,T,Q] fp32, the true branch [T,3,3]): bumps at x_t = x_0 Rz(10 t) (weight 0.6) and on a second branch that turns the
    other way about another axis (0.4)"""
    grid = grid_of(level, kind)
    x0, y0 = _rot((0.2, 1.0, -0.4), 65.0), _rot((-0.7, 0.1, 0.5), 140.0)
    true = np.stack([x0 @ _rot((0.0, 0.0, 1.0), 10.0 * t) for t in range(T)])
    other = np.stack([y0 @ _rot((1.0, 0.0, 0.3), -10.0 * t) for t in range(T)])
    ll = np.stack([bumps(grid, [true[t], other[t]], [0.6, 0.4], kappa=120.0) for t in range(T)])
    return ll[None], true


# ---- tests: the pass ---------------------------------------------------------------------------------------------------------------------

def test_the_identity_of_the_quadratic_form_holds_for_rotations():
    """tr(A^T Q^T G) - (s1 + s2 + s3) = -1/2 tr(W K W^T), W = G - Q Delta, and the bound -(s2 + s3)/4 |W|^2"""
    R = fe.uniform_rotations64(400, 5).reshape(2, 200, 3, 3)
    for s in ((40.0, 12.0, 3.0), (40.0, 12.0, -3.0), (200.0, 5.0, 5.0)):
        A = _rot((1.0, 2.0, 0.5), 33.0) @ concentration_of(s)
        drift, K, sv = motion_factors_fp64(A)
        assert np.allclose(sv, s, rtol=1e-12) and np.allclose(drift @ K, A, atol=1e-12)
        W = R[1] - R[0] @ drift
        lhs = np.einsum("ij,nki,nkj->n", A, R[0], R[1]) - sum(s)
        rhs = -0.5 * np.einsum("nri,ij,nrj->n", W, K, W)
        assert np.abs(lhs - rhs).max() <= 1e-11 * max(s)
        assert (rhs <= -(sv[1] + sv[2]) / 4.0 * np.einsum("nri,nri->n", W, W) + 1e-9).all()


@pytest.mark.parametrize("with_arg", [False, True], ids=["sum", "max"])
@pytest.mark.parametrize("kind", ["none", "fixed"])
@pytest.mark.parametrize("level", LEVELS)
def test_host_build_lies_in_the_bracket_for_every_cut_and_concentration(level, kind, with_arg):
    """Every cut and every concentration, with and without log-weights; the queries are every grid row, every row of the shifted grid and
    the special ones.  At level 2 (9 266 queries against 4 608 rows) every query runs every cut at V diag(200, 5, 5) V^T with log-weights,
    and every sixteenth row and every special query runs the full product."""
    if level < 2:
        check_fisher_level(host_local_fisher, level, kind, with_arg=with_arg)
    else:
        check_fisher_level(host_local_fisher, level, kind, Ks=KS[1:2], with_arg=with_arg, weights=(True,))
        check_fisher_level(host_local_fisher, level, kind, pick=thinned(level, kind, 16), with_arg=with_arg)


def test_host_term_and_membership_are_bit_symmetric_at_level_1():
    """The term of (query C_a, row G_b) is the term of (query G_b, row C_a) bit for bit, and membership agrees: group a carries weight on
    row a alone, so out[a][b] is that one term (the sum of one term is the term: exp2(0) = 1, log2(1) = 0)"""
    grid = grid_of(1, "none")
    rows = shifted_rows(grid)
    Q = len(grid)
    onehot = np.full((Q, Q), -np.inf, np.float32)
    onehot[np.arange(Q), np.arange(Q)] = 0.0
    for K, deg in ((KS[1], 20.0), (KS[2], 33.0), (KS[0], 47.0), (KS[2], 47.0)):
        if True:
            a, ca = host_local_fisher(1, grid, rows, K, chord2(deg), onehot)           # a[b][i]: row G_b, query C_i
            b, cb = host_local_fisher(1, rows, grid, K, chord2(deg), onehot, offset=DRIFT)   # b[a][i]: row C_a, query G_i
            assert np.array_equal(np.isfinite(a), np.isfinite(b).T)
            assert np.array_equal(a.view(np.uint32), b.T.view(np.uint32))
            assert np.array_equal(np.isfinite(a).sum(axis=0), ca) and np.array_equal(np.isfinite(b).sum(axis=0), cb)
            assert np.isfinite(a).any()
            am, ja, _ = host_local_fisher(1, grid, rows, K, chord2(deg), onehot, with_arg=True)
            assert np.array_equal(am.view(np.uint32), a.view(np.uint32)) and (ja[np.isfinite(am)] == np.nonzero(np.isfinite(am))[0]).all()


def test_isotropic_concentration_lies_within_the_gate_of_the_isotropic_pass_and_normalisers_agree():
    h = _host_lib()
    grid, queries, d2, _ = fisher_case(1, "fixed")
    lw = log_weights_of(len(grid), 2, 3)
    for kappa in (0.0, 4.0, 64.0, 1e4):
        l_iso = float(h.hsglf_log_normaliser_iso(C.c_double(kappa)))
        assert host_log_normaliser(kappa * np.eye(3)) == l_iso, kappa                     # kappa I takes the Bessel form itself
        near = host_log_normaliser(np.diag([kappa, kappa, kappa * (1.0 - 1e-12)]))     # .. and the quadrature agrees within its gate
        assert abs(near - l_iso) <= 1e-10 * max(1.0, abs(l_iso + 3.0 * kappa)) + 1e-11 * kappa, kappa
        assert abs(l_iso - float(log_normaliser(kappa))) <= 1e-10 * max(1.0, abs(l_iso))
        for cut in (chord2(15.0), chord2(60.0), 8.0):
            a, ca = host_local_fisher(1, grid, queries, kappa * np.eye(3), cut, lw, offset_of("fixed"))
            b, cb = host_local_iso(1, grid, queries, kappa, cut, lw, offset_of("fixed"))
            assert np.array_equal(ca, cb) and np.array_equal(np.isfinite(a), np.isfinite(b))
            E = 0.5 * kappa * math.sqrt(3.0) * np.minimum(d2.max(axis=1), cut + 1e-3) + np.abs(lw[np.isfinite(lw)]).max()
            fin = np.isfinite(a)
            assert (np.abs(a.astype(np.float64) - b)[fin] <= (2.0 * gate(E))[None, :].repeat(2, axis=0)[fin]).all(), (kappa, cut)
            am, ja, _ = host_local_fisher(1, grid, queries, kappa * np.eye(3), cut, lw, offset_of("fixed"), with_arg=True)
            bm, jb, _ = host_local_iso(1, grid, queries, kappa, cut, lw, offset_of("fixed"), with_arg=True)
            fin = np.isfinite(am)
            assert (np.abs(am.astype(np.float64) - bm)[fin] <= (2.0 * gate(E))[None, :].repeat(2, axis=0)[fin]).all()


def test_log_normaliser_matches_the_exact_reference():
    for K in KS + (concentration_of((3e4, 2e4, 1e4)), concentration_of((30.0, 20.0, -10.0)), concentration_of((1e4, 1.0, 1e-3))):
        want = log_normaliser_fisher(K)
        s = eigenvalues(K)
        lc = fe.log_c(s) if s.any() else 0.0
        assert abs(host_log_normaliser(K) - want) <= 1e-10 * max(1.0, abs(lc)), (s, host_log_normaliser(K), want)


def test_host_eigenvalues_and_refusals_of_a_concentration():
    h = _host_lib()
    rng = np.random.default_rng(2)
    for _ in range(50):
        M = rng.standard_normal((3, 3)) * 10.0 ** rng.uniform(-3, 4)
        K = np.ascontiguousarray(0.5 * (M + M.T))
        ev = np.empty(3)
        h.hsglf_eigenvalues(ptr(K), ptr(ev))
        assert np.abs(ev - eigenvalues(K)).max() <= 1e-12 * np.linalg.norm(K)
    defect = lambda K: h.hsglf_concentration_defect(ptr(np.ascontiguousarray(K, np.float64)))   # noqa: E731
    for K in KS:
        assert defect(K) == 0
    assert defect(np.diag([5.0, 5.0, -5.0])) == 0 and defect(concentration_of((5.0, 5.0, -5.0))) == 0     # a pair sum of exactly zero
    bad = KS[1].copy()
    bad[0, 1] += 1e-6
    assert defect(bad) == 2
    bad = KS[1].copy()
    bad[2, 2] = np.inf
    assert defect(bad) == 1
    assert defect(np.diag([5.0, -2.0, -2.0])) == 3 and defect(concentration_of((5.0, 1.0, -2.0))) == 3 and defect(-KS[0]) == 3
    assert defect(concentration_of((3.0001e4, 1.0, 1.0))) == 4 and defect(concentration_of((3e4, 3e4, 3e4))) == 0


def test_host_sentinels():
    """-inf and NaN log-weights, non-finite queries and empty neighbourhoods behave as the isotropic passes document"""
    level, kind, K = 1, "fixed", KS[2]
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
    quad = quad_fp64(grid, queries, K)
    ref = local_fisher_fp64(d2, quad, K, cut, lw)
    for with_arg in (False, True):
        res = host_local_fisher(level, grid, queries, K, cut, lw, off, with_arg)
        out, count = res[0], res[-1]
        want = ref["max_hi"] if with_arg else ref["hi"]
        assert np.array_equal(count, inside.sum(axis=1))
        assert np.isneginf(out[0, 0]) and np.isnan(out[1, 1])
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(out), ~ok)
        fin = ok & np.isfinite(want)
        assert (np.abs(out[fin] - want[fin]) <= gate(ref["E"][fin])).all() and np.array_equal(np.isneginf(out), ok & np.isneginf(want))
        if with_arg:
            assert (res[1][~fin] == -1).all() and (res[1][fin] >= 0).all()
        bad = queries.copy()
        bad[3, 1, 1], bad[5, 0, 2] = np.nan, np.inf
        bad[7] *= 4.0                                                       # finite, further than any cut from every rotation
        res = host_local_fisher(level, grid, bad, K, cut, None, off, with_arg)
        out, count = res[0], res[-1]
        assert np.isnan(out[0, [3, 5]]).all() and (count[[3, 5]] == 0).all()
        assert np.isneginf(out[0, 7]) and count[7] == 0
        rest = np.delete(np.arange(len(bad)), [3, 5, 7])
        assert np.isfinite(out[0, rest]).all() and np.array_equal(count[rest], inside.sum(axis=1)[rest])
        res = host_local_fisher(level, grid, queries, K, 0.0, None, off, with_arg)       # off-grid queries at cut 0: empty
        assert np.isneginf(res[0]).all() and (res[-1] == 0).all()


@pytest.mark.parametrize("level", [1, 2, 3])
def test_every_shifted_row_has_a_neighbour_at_the_floor_radius(level):
    """count >= 1 at the floor for five random drifts: a drifted row always finds a grid row"""
    from rotationnormflow_amd.utils import kde
    grid = grid_of(level, "none") if level < 3 else None
    if grid is None:
        from tests.test_so3_grid import healpix_grid_fp64
        grid = healpix_grid_fp64(level).astype(np.float32)
    floor = kde.local_floor_d2_cut(level)
    assert abs(floor - chord2(1.25 * spacing_deg(level))) < 1e-15
    drifts = synth.uniform_rotations(5, seed=9).astype(np.float64).reshape(5, 3, 3)
    for k, drift in enumerate(drifts):
        rows = shifted_rows(grid, drift)
        pick = rows if level < 3 else rows[k::11]
        _, count = host_local_fisher(level, grid, pick, KS[1], floor)
        assert (count >= 1).all(), (level, k, int((count == 0).sum()))


# ---- tests: the references of the recursions --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level,radius", RECURSION_CASES)
def test_no_pair_of_shifted_and_grid_rows_lies_at_the_recursions_cuts(level, radius):
    """The fp32 membership of the kernel and the fp64 membership of the references agree: no pair (C_j, G_i) within 8 delta of the cut"""
    for motion in (MOTION_TIGHT, time_varying()[1]):
        m = MotionModel(grid_of(level, "none"), motion, radius)
        assert m.gap > 8.0 * delta_of(m.cut), (level, radius, m.gap)
        assert m.sizes[0] >= 1


def test_reference_recursions_are_consistent():
    """The references against themselves at level 1: the truncated, row-normalised operator is a Markov kernel, the smoother has unit
    mass and ends on the filter, the Viterbi score is the joint of its own path and beats perturbed paths, and K = kappa I without a
    drift reproduces the isotropic model of tests/test_so3_grid_viterbi_host.py"""
    from tests import test_so3_grid_viterbi_host as iso
    level, radius = RECURSION_CASES[0]
    grid, ll = grid_of(level, "none"), drift_sequences(level)
    Q = len(grid)
    rng = np.random.default_rng(0)
    for motion in (MOTION_TIGHT, MOTION_SIGNED, time_varying()):
        models = models_of(grid, motion, radius, T_FRAMES)
        logp = rng.standard_normal((2, Q)) * 3.0
        assert np.abs(_lse(models[0].diffuse(logp), axis=1) - math.log(Q)).max() <= 1e-12
        prior = rng.standard_normal(Q)
        sm = smooth_fp64(models, ll, prior)
        assert np.abs(_lse(sm["smoothed"], axis=2) - math.log(Q)).max() <= 1e-11
        assert np.abs(sm["smoothed"][:, -1] - sm["filtered"][:, -1]).max() <= 1e-12
        vit = viterbi_fp64(models, ll, prior)
        assert np.abs(joint_fp64(models, ll, vit["path"], prior) - vit["score"]).max() <= 1e-9
        for _ in range(20):
            other = vit["path"].copy()
            other[rng.integers(0, B_SEQ), rng.integers(0, T_FRAMES)] = rng.integers(0, Q)
            assert (joint_fp64(models, ll, other, prior) <= vit["score"] + 1e-9).all()
    ref = iso.Model(grid, 64.0, radius)
    mine = [MotionModel(grid, 64.0 * np.eye(3), radius)] * (T_FRAMES - 1)
    a, b = iso.forward_backward_fp64(ref, ll), smooth_fp64(mine, ll)
    assert np.abs(a["backward"] - b["backward"]).max() <= 1e-9 and np.abs(a["evidence"] - b["evidence"]).max() <= 1e-9
    assert np.array_equal(iso.viterbi_fp64(ref, ll)["path"], viterbi_fp64(mine, ll)["path"])


def test_the_drift_model_explains_a_turning_object_better_than_the_matched_isotropic_one_at_level_2():
    """The sign the GPU test relies on at level 3, in the fp64 reference at level 2: the summed log-evidence of the sequence that turns
    10 degrees per frame about body z is higher under motion_matrix(drift = Rz(10), sigma = (2, 2, 4)) than under the isotropic kappa
    matched to 4 degrees"""
    from rotationnormflow_amd.utils import kde
    from tests import test_so3_grid_viterbi_host as iso
    level = 2
    grid = grid_of(level, "none")
    ll, _ = turning_sequence(level)
    A = kde.motion_matrix(drift=TURN, sigma_deg=SIGMA_DEG)
    drift, K, s = kde.motion_factors(A)
    radius = math.degrees(math.acos(1.0 - kde.local_default_d2_cut_fisher(s, level, True) / 4.0))
    with_drift = filter_fp64(models_of(grid, A, radius, ll.shape[1]), ll)[1].sum()
    radius_iso = math.degrees(math.acos(1.0 - kde.local_default_d2_cut(KAPPA_MATCHED) / 4.0))
    without = iso.forward_backward_fp64(iso.Model(grid, KAPPA_MATCHED, radius_iso), ll)["evidence"].sum()
    print("summed log-evidence: drift model %.3f, matched isotropic %.3f" % (with_drift, without))
    assert with_drift > without + 1.0


# ---- tests: the Python layers without a device ------------------------------------------------------------------------------------------

def test_motion_factors_and_motion_matrix():
    from rotationnormflow_amd.utils import kde
    rng = np.random.default_rng(4)
    for _ in range(20):
        A = rng.standard_normal((3, 3)) * 10.0 ** rng.uniform(-1, 3)
        drift, K, s = kde.motion_factors(A)
        d2, K2, s2 = motion_factors_fp64(A)
        assert np.allclose(s, s2, rtol=1e-12, atol=1e-12 * abs(s2[0])) and s[0] >= s[1] >= abs(s[2]) and np.sign(s[2]) == np.sign(np.linalg.det(A))
        assert np.allclose(drift @ K, A, atol=1e-12 * s[0]) and np.allclose(K, K2, atol=1e-9 * s[0]) and np.array_equal(K, K.T)
        assert abs(np.linalg.det(drift) - 1.0) < 1e-12 and np.allclose(drift.T @ drift, np.eye(3), atol=1e-12)
    for form in (A.tolist(), torch.from_numpy(A), torch.from_numpy(A).float()):
        assert np.allclose(kde.motion_factors(form)[1], K, rtol=1e-5, atol=1e-5 * s[0])
    for bad in (np.full((3, 3), np.nan), np.eye(3) * np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            kde.motion_factors(bad)
    with pytest.raises(ValueError, match=r"\[3,3\]"):
        kde.motion_factors(np.eye(4))
    assert "read back" in kde.motion_factors.__doc__.lower()
    # degrees: the variance about axis k is 1 / (s_i + s_j)
    A = kde.motion_matrix(drift=TURN, sigma_deg=(2.0, 3.0, 4.0), axes=V_AXES)
    drift, K, s = kde.motion_factors(A)
    assert np.allclose(drift, TURN, atol=1e-12)
    ev, vec = np.linalg.eigh(K)
    for k, sig in enumerate((2.0, 3.0, 4.0)):
        along = np.einsum("i,ij,j->", V_AXES[:, k], K, V_AXES[:, k])
        assert abs(1.0 / (np.trace(K) - along) - math.radians(sig) ** 2) <= 1e-12
    assert np.allclose(kde.motion_factors(kde.motion_matrix(sigma_deg=(4.0, 4.0, 4.0)))[1], KAPPA_MATCHED * np.eye(3), rtol=1e-12)
    for bad in ((1.0, 2.0), (1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError, match="sigma_deg"):
            kde.motion_matrix(sigma_deg=bad)
    with pytest.raises(ValueError, match="rotation"):
        kde.motion_matrix(drift=2.0 * np.eye(3))
    # the default cut: 72 / (s2 + s3), 36 / kappa for kappa I, 8 where s2 + s3 <= 9, the floor only with a drift
    assert abs(kde.local_default_d2_cut_fisher((64.0, 64.0, 64.0), 2, False) - kde.local_default_d2_cut(64.0)) < 1e-15
    assert kde.local_default_d2_cut_fisher((200.0, 5.0, 4.0), 2, False) == 8.0 and kde.local_default_d2_cut_fisher((40.0, 12.0, -3.0), 2, True) == 8.0
    assert abs(kde.local_default_d2_cut_fisher((200.0, 5.0, 5.0), 2, True) - 7.2) < 1e-15
    assert kde.local_default_d2_cut_fisher((1e4, 1e4, 1e4), 2, False) == 36.0 / 1e4
    assert kde.local_default_d2_cut_fisher((1e4, 1e4, 1e4), 2, True) == kde.local_floor_d2_cut(2) == chord2(1.25 * 15.0)


_FAKE = 1 << 20


def _args(**kw):
    base = dict(level=2, offset=_FAKE, grid=_FAKE, queries=_FAKE * 2, log_weights=_FAKE, m=1000, G=3, d2_cut=0.5, out=_FAKE, arg=_FAKE, count=_FAKE)
    base.update(kw)
    K = base.pop("K", KS[2])
    return _lib.So3GridLocalFisher(concentration=(C.c_double * 9)(*np.asarray(K, np.float64).reshape(9)), **base)


def _refused(a, word):
    L = _lib.lib()
    assert L.rnf_so3_grid_local_fisher(C.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Every refusal happens before a launch (the pointers are never dereferenced)"""
    L = _lib.lib()
    assert L.rnf_abi_version() == 8
    asym, inf, nan = KS[1].copy(), KS[1].copy(), KS[1].copy()
    asym[0, 2] += 1e-6
    inf[1, 1], nan[0, 1] = np.inf, np.nan
    for bad, word in ((dict(K=asym), "not symmetric"), (dict(K=inf), "non-finite"), (dict(K=nan), "non-finite"),
                      (dict(K=np.diag([5.0, -2.0, -2.0])), "negative sum"), (dict(K=-KS[0]), "negative sum"),
                      (dict(K=concentration_of((3.0001e4, 5.0, 5.0))), "beyond 3e4"), (dict(K=np.diag([5.0, 5.0, -4e4])), "negative sum"),
                      (dict(level=-1), "level="), (dict(level=7), "level="), (dict(G=0), "G="), (dict(G=65536), "G="), (dict(m=-1), "m="),
                      (dict(m=1 << 31), "m="), (dict(d2_cut=-1e-9), "d2_cut="), (dict(d2_cut=8.0000001), "d2_cut="),
                      (dict(d2_cut=float("nan")), "d2_cut="), (dict(d2_cut=float("inf")), "d2_cut="), (dict(grid=_FAKE + 4), "aligned"),
                      (dict(queries=_FAKE + 8), "aligned"), (dict(out=_FAKE + 2), "aligned"), (dict(log_weights=_FAKE + 1), "aligned"),
                      (dict(count=_FAKE + 2), "aligned"), (dict(arg=_FAKE + 2), "aligned"), (dict(offset=_FAKE + 3), "aligned"),
                      (dict(queries=None), "null queries"), (dict(grid=None), "null"), (dict(out=None), "null")):
        _refused(_args(**bad), word)
    a = _args()
    a.struct_bytes += 8
    _refused(a, "struct_bytes")
    assert L.rnf_so3_grid_local_fisher(C.byref(_args(m=0, out=None, grid=None))) == 0      # m = 0 is a no-op
    assert L.rnf_so3_grid_local_fisher(C.byref(_args(m=0, arg=None, K=np.zeros((3, 3))))) == 0


def test_header_declares_the_struct_the_binding_mirrors():
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    body = header[header.index("typedef struct RnfSo3GridLocalFisher {") + 37:header.index("} RnfSo3GridLocalFisher;")]
    names = [re.sub(r"\[\d+\]$", "", decl.split()[-1].lstrip("*")) for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
    assert names == [f for f, _ in _lib.So3GridLocalFisher._fields_], names
    assert "double concentration[9]" in body and dict(_lib.So3GridLocalFisher._fields_)["concentration"] is C.c_double * 9
    assert C.sizeof(_lib.So3GridLocalFisher) == C.sizeof(_lib.So3GridLocalMax) + 64        # nine doubles in place of one
    assert "rnf_so3_grid_local_fisher" in _lib.EXPORTS and "#define RNF_ABI_VERSION 8" in header
    assert C.sizeof(_lib.So3GridLocalSum) == 104 and C.sizeof(_lib.So3GridLocalMax) == 112  # the existing structs keep their sizes


def test_python_entry_points_validate_their_arguments():
    from rotationnormflow_amd import grid_pose, harness
    from rotationnormflow_amd.utils import kde
    for name in ("grid_diffuse_local", "grid_filter_step", "grid_viterbi", "grid_smooth", "grid_pose_filter", "grid_pose_smooth"):
        assert getattr(harness, name) is getattr(grid_pose, name)
        assert "motion" in getattr(grid_pose, name).__code__.co_varnames
    grid, ll = torch.zeros(72, 3, 3), torch.zeros(2, 72)
    A = torch.from_numpy(MOTION_TIGHT)
    for fn, args in ((grid_pose.grid_diffuse_local, (ll, grid, 0)), (grid_pose.grid_filter_step, (ll, ll, grid, 0)),
                     (grid_pose.grid_viterbi, (ll, grid, 0)), (grid_pose.grid_smooth, (ll, grid, 0))):
        with pytest.raises(ValueError, match="exactly one of kappa and motion"):
            fn(*args)
        with pytest.raises(ValueError, match="exactly one of kappa and motion"):
            fn(*args, kappa=4.0, motion=A)
        with pytest.raises(ValueError, match="GPU"):
            fn(*args, motion=A)
        with pytest.raises(ValueError, match="motion"):
            fn(*args, motion=torch.zeros(3, 4))
        with pytest.raises(ValueError, match="non-finite"):
            fn(*args, motion=A * float("nan"))
    for fn in (grid_pose.grid_viterbi, grid_pose.grid_smooth):                   # T = 2: one matrix per step
        with pytest.raises(ValueError, match=r"\[1,3,3\]"):
            fn(ll, grid, 0, motion=torch.stack([A, A]))
    with pytest.raises(ValueError, match=r"motion"):
        grid_pose.grid_diffuse_local(ll, grid, 0, motion=torch.stack([A]))        # one step takes one matrix
    with pytest.raises(ValueError, match="exactly one of kappa and concentration"):
        kde.so3_grid_local_log_sum(grid, 0)
    with pytest.raises(ValueError, match="exactly one of kappa and concentration"):
        kde.so3_grid_local_log_max(grid, 0, 4.0, concentration=np.eye(3))
    with pytest.raises(ValueError, match="GPU"):
        kde.so3_grid_local_log_sum(grid, 0, concentration=KS[1])


def test_a_radius_under_the_floor_is_refused_from_the_arguments_alone():
    """Decided on the host numbers before any device work: the refusal needs no GPU"""
    from rotationnormflow_amd import grid_pose
    grid, ll = torch.zeros(4608, 3, 3), torch.zeros(2, 4608)
    for fn, args in ((grid_pose.grid_diffuse_local, (ll, grid, 2)), (grid_pose.grid_filter_step, (ll, ll, grid, 2)),
                     (grid_pose.grid_viterbi, (ll, grid, 2)), (grid_pose.grid_smooth, (ll, grid, 2))):
        with pytest.raises(ValueError, match="below 1.25 grid spacings"):
            fn(*args, radius_deg=15.0, motion=MOTION_TIGHT)
        with pytest.raises(ValueError, match="GPU"):                              # 1.25 * 15 degrees: at the floor, and no drift: no floor
            fn(*args, radius_deg=18.75, motion=MOTION_TIGHT)
        with pytest.raises(ValueError, match="GPU"):
            fn(*args, radius_deg=15.0, motion=concentration_of((200.0, 40.0, 40.0)))
        with pytest.raises(ValueError, match="beyond 3e4"):
            fn(*args, motion=DRIFT @ concentration_of((4e4, 40.0, 40.0)))
    step = grid_pose._MotionStep(concentration_of((200.0, 40.0, 40.0)), grid, 2, 15.0, None, "grid_diffuse_local")
    assert not step.drifting and step.rows is step.grid and step.cut == chord2(15.0)
    step = grid_pose._MotionStep(MOTION_TIGHT, grid, 2, None, None, "grid_diffuse_local")
    assert step.drifting and abs(step.cut - 72.0 / 80.0) < 1e-12 and step.rows.shape == (4608, 3, 3) and step.rows_offset.dtype == torch.float32
    assert np.allclose(step.rows_offset.numpy(), DRIFT, atol=1e-7)
    assert grid_pose._isotropic(64.0 * np.eye(3)) == 64.0 and grid_pose._isotropic(KS[1]) is None and grid_pose._isotropic(-np.eye(3)) is None


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_so3_grid_local_fisher.cpp (its own main: level 0 to 2 enumerations at this file's cuts and concentrations,
    both passes) built with the host-side address and undefined-behaviour sanitizers (-Xarch_host: host code only, nothing for the GPU)
    and run as a process of its own."""
    exe = str(tmp_path / "sanitize_so3_grid_local_fisher")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_so3_grid_local_fisher.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)
