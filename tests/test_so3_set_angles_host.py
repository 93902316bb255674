"""CPU: the distribution function of the angle to the nearest member of a set (csrc/so3_set_angle_cdf.h, rnf_so3_set_angle_cdf), the
symmetry groups of utils/symmetry.py and what is built on them.

``set_angle_cdf_fp64`` is the numpy fp64 restatement: tests/test_so3_angles_host.angle_cdf_fp64's pieces -- d2 from the nine
differences, the indicator d2 <= tau, theta = 2 asin(min(1, sqrt(d2 / 8))), weights by an explicit softmax, the same gate terms -- with
d2 = min over the live members of a set.  tests/test_gpu_so3_set_angles.py imports it, the cases and the gates.

The gates are tests/test_so3_angles_host.py's, verbatim: min of numbers each within 1e-6 (relatively) of its fp64 value is within
1e-6 of the fp64 min, so d2 keeps its bound and everything derived from it does.
  mass:   |mass - ref| <= U + 4e-6 ref + 2^-23, U = sum_j w_j [|d2_64 - tau| <= 1e-6 d2_64], with U <= 0.01 asserted on the restatement
          for every (set, threshold) below 180 degrees (a condition on the case, not a measurement of the code).
  angles: g_ij = min(delta / (4 sin theta), sqrt(delta / 2)) + 1e-6 theta + 4e-7, delta = 1e-6 d2;
          |mean_angle - ref| <= sum_j w_j g_ij,  |mean_sq_angle - ref| <= sum_j w_j 2 theta_ij g_ij + 1e-6 ref.
  radii:  the bracket rule of tests/test_so3_angles_host.check_quantile.
Centres are random (uniform or clustered), never a grid; the sets are orbits of random estimates under point groups (K = 1, 2, 12, 60,
720: C1, C2, T, I, D360).

Measured, the worst fraction of each gate over test_host_build_against_the_restatement: mass 0.076, mean_angle 0.192, mean_sq_angle
0.100; the largest undecided weight of a case 2.9e-5 (the cap is 0.01).  The MI355X's figures are in tests/test_gpu_so3_set_angles.py;
DESIGN.md 3.3g has both."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib
from rotationnormflow_amd.utils import symmetry
from tests.test_so3_angles_host import (EPS, FLT_MAX, OUTPUTS, STEP_DEG, THRESHOLDS_DEG, U_CAP, angle_deg, check_quantile, settle,  # noqa: F401
                                        tau_of)
from tests.test_so3_kde_host import draw, make_case, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_so3_set_angle_cdf.cpp")
OUT = os.path.join(HERE, "csrc", "_host_so3_set_angle_cdf.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f)
        for f in ("so3_set_angle_cdf.h", "so3_angle_cdf.h", "so3_kernel_sum.h", "fisher_exact.h", "fisher_math.h")]
GROUP_OF = {1: "C1", 2: "C2", 12: "T", 24: "O", 36: "D18", 60: "I", 720: "D360"}


def _host_lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    h = C.CDLL(OUT)
    h.hsac_workspace_bytes.restype = C.c_ulonglong
    return h


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def set_angle_cdf_fp64(centres, sets, taus, log_weights=None, group_queries=False):
    """The outputs of rnf_so3_set_angle_cdf in fp64 from the fp32 inputs.  ``sets`` [m,K,3,3] or [G,m,K,3,3]; ``taus`` float32 [T]
    shared, [G,T,m] per (group, set), or None.  -> dict of mass, U [G,T,m], mean_angle, mean_sq_angle, gate_mean, gate_sq [G,m], as
    tests/test_so3_angles_host.angle_cdf_fp64."""
    Cn = np.asarray(centres, np.float32).reshape(-1, 9).astype(np.float64)
    n = len(Cn)
    lw = None if log_weights is None else np.asarray(log_weights, np.float32).reshape(-1, n).astype(np.float64)
    Qa = np.asarray(sets, np.float32).astype(np.float64)
    K = Qa.shape[-3]
    Qa = Qa.reshape(-1, Qa.shape[-4], K, 9) if group_queries else Qa.reshape(1, -1, K, 9)
    G = len(Qa) if group_queries else (1 if lw is None else len(lw))
    m = Qa.shape[1]
    if lw is None:
        lw = np.zeros((G, n))
    tq = None
    if taus is not None:
        tq = np.asarray(taus, np.float32).astype(np.float64)
        tq = np.broadcast_to(tq[None, :, None], (G, len(tq), m)) if tq.ndim == 1 else tq.reshape(G, -1, m)
    T = 0 if tq is None else tq.shape[1]
    res = {k: np.full((G, T, m), np.nan) for k in ("mass", "U")}
    res.update({k: np.full((G, m), np.nan) for k in ("mean_angle", "mean_sq_angle", "gate_mean", "gate_sq")})
    c_ok = np.isfinite(Cn).all(axis=1)
    Cz = np.where(c_ok[:, None], Cn, 0.0)
    d2 = None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for g in range(G):
            Qs = Qa[g if group_queries else 0]                           # [m,K,9]
            live_member = np.isfinite(Qs).all(axis=2)                    # [m,K]
            q_ok = live_member.any(axis=1)
            live = lw[g] != -np.inf
            if np.isnan(lw[g]).any() or (live & ~c_ok).any() or not live.any() or np.isposinf(lw[g]).any():
                continue
            if group_queries or d2 is None:
                d2 = np.full((m, n), np.inf)
                for s in range(K):                                       # the min over the live members, one member at a time
                    diff = np.where(live_member[:, s, None], Qs[:, s], 0.0)[:, None, :] - Cz[None, :, :]
                    d2s = np.einsum("ijk,ijk->ij", diff, diff)
                    d2 = np.where(live_member[:, s, None], np.minimum(d2, d2s), d2)
                d2 = np.where(q_ok[:, None], d2, 0.0)                    # a set of padding only: its outputs are NaN below
                theta = 2.0 * np.arcsin(np.minimum(1.0, np.sqrt(d2 / 8.0)))
                delta = 1e-6 * d2
                sin = np.sin(theta)
                gij = np.minimum(np.where(sin > 0, delta / (4.0 * np.where(sin > 0, sin, 1.0)), np.inf), np.sqrt(delta / 2.0)) + 1e-6 * theta + 4e-7
            mx = lw[g][live].max()
            w = np.where(live, np.exp(lw[g] - mx), 0.0)
            w /= w.sum()
            for t in range(T):
                tau = tq[g, t][:, None]
                res["mass"][g, t] = ((d2 <= tau) * w[None, :]).sum(axis=1)
                res["U"][g, t] = ((np.abs(d2 - tau) <= delta) * w[None, :]).sum(axis=1)
                res["mass"][g, t][~q_ok | np.isnan(tq[g, t])] = np.nan
            res["mean_angle"][g] = theta @ w
            res["mean_sq_angle"][g] = (theta * theta) @ w
            res["gate_mean"][g] = gij @ w
            res["gate_sq"][g] = (2.0 * theta * gij) @ w + 1e-6 * res["mean_sq_angle"][g]
            for k in ("mean_angle", "mean_sq_angle"):
                res[k][g][~q_ok] = np.nan
    return res


def host_set_angle_cdf(centres, sets, log_weights=None, group_queries=False, thresholds=None, query_tau=None, moments=True, mass=True):
    """The host build of the kernels' arithmetic -> dict of float32 arrays with a leading G"""
    h = _host_lib()
    Cn = np.ascontiguousarray(centres, np.float32).reshape(-1, 9)
    n = len(Cn)
    Qr = np.ascontiguousarray(sets, np.float32)
    lw = None if log_weights is None else np.ascontiguousarray(log_weights, np.float32).reshape(-1, n)
    G = Qr.shape[0] if group_queries else (1 if lw is None else len(lw))
    m, K = Qr.shape[-4], Qr.shape[-3]
    th = None if thresholds is None else np.ascontiguousarray(np.atleast_1d(thresholds), np.float64)
    qt = None if query_tau is None else np.ascontiguousarray(query_tau, np.float32).reshape(G, -1, m)
    T = len(th) if th is not None else (qt.shape[1] if qt is not None else 0)
    out = {}
    if mass:
        out["mass"] = np.full((G, T, m), 7.0, np.float32)
    if moments:
        out["mean_angle"], out["mean_sq_angle"] = np.full((G, m), 7.0, np.float32), np.full((G, m), 7.0, np.float32)
    h.hsac_set_angle_cdf(ptr(Cn), ptr(Qr), ptr(lw), C.c_longlong(n), C.c_longlong(m), K, G, int(group_queries), T, ptr(th), ptr(qt),
                         *[ptr(out.get(k)) for k in OUTPUTS])
    return out


def host_single_angle_cdf(centres, queries, log_weights=None, group_queries=False, thresholds=None, query_tau=None, moments=True):
    """ac::host_angle_cdf from the same host build: the K = 1 counterpart"""
    h = _host_lib()
    Cn = np.ascontiguousarray(centres, np.float32).reshape(-1, 9)
    n = len(Cn)
    Qr = np.ascontiguousarray(queries, np.float32)
    lw = None if log_weights is None else np.ascontiguousarray(log_weights, np.float32).reshape(-1, n)
    G = Qr.shape[0] if group_queries else (1 if lw is None else len(lw))
    m = Qr.shape[-3]
    th = None if thresholds is None else np.ascontiguousarray(np.atleast_1d(thresholds), np.float64)
    qt = None if query_tau is None else np.ascontiguousarray(query_tau, np.float32).reshape(G, -1, m)
    T = len(th) if th is not None else (qt.shape[1] if qt is not None else 0)
    out = {"mass": np.full((G, T, m), 7.0, np.float32)}
    if moments:
        out["mean_angle"], out["mean_sq_angle"] = np.full((G, m), 7.0, np.float32), np.full((G, m), 7.0, np.float32)
    h.hsac_angle_cdf(ptr(Cn), ptr(Qr), ptr(lw), C.c_longlong(n), C.c_longlong(m), G, int(group_queries), T, ptr(th), ptr(qt),
                     *[ptr(out.get(k)) for k in OUTPUTS])
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

def group_of(K):
    return symmetry.point_group(GROUP_OF[K]).numpy()


def make_set_case(n, m, K, G, kind="clustered", seed=0):
    """Random centres [n,3,3] of ``kind``; m sets [m,K,3,3]: the orbits under the point group of order K of estimates drawn half like
    the centres and half uniformly; log-weights None (G = 1) or [G,n] = 3 N(0, 1) whose row 1 has half its entries -inf"""
    Cn, Er, _ = make_case(n, m, kind, False, seed)
    sets = (Er.astype(np.float64)[:, None] @ group_of(K).astype(np.float64)[None]).astype(np.float32)
    lw = None
    if G > 1:
        rng = np.random.default_rng(500 + seed + n + G)
        lw = (3.0 * rng.standard_normal((G, n))).astype(np.float32)
        lw[1, rng.permutation(n)[:n // 2]] = -np.inf
    return Cn, sets, lw


def per_group_sets(sets, G):
    """One array of sets per group from one: group g takes it rolled by 2 g sets"""
    return np.stack([np.roll(sets, 2 * g, axis=0) for g in range(G)])


# (n, m, K, G, T, thresholds per set, sets per group, moments): every n, K, m, G, T, both forms and both moment settings of the issue
CASES = [
    (1, 1, 1, 1, 1, False, False, True),
    (63, 3, 2, 3, 3, False, False, True),
    (64, 65, 12, 1, 8, False, False, False),
    (65, 3, 60, 5, 8, False, False, True),
    (65, 65, 2, 3, 8, False, True, True),
    (4096, 65, 12, 3, 3, True, True, True),
    (4097, 3, 720, 1, 8, False, False, True),
    (4097, 65, 60, 3, 0, False, False, True),
    (4097, 1, 12, 5, 1, True, False, False),
    (4097, 3, 12, 5, 3, False, False, False),
    (130, 1400, 12, 3, 8, False, False, True),      # the device takes a thread per set from 4097 (group, set, chunk)s on, a wave below
    (130, 1400, 12, 3, 3, True, True, False),       # likewise, with thresholds per set and sets per group
]
DEG_OF_T = {0: (), 1: (30.0,), 3: (15.0, 30.0, 120.0), 8: THRESHOLDS_DEG}


@functools.lru_cache(maxsize=None)
def set_reference(n, m, K, G, T, per_set, per_group, moments):
    """(case, shared thresholds in degrees or None, query_tau or None, restatement): computed once per case and left unchanged.  A
    shared threshold whose band is too heavy moves by tests/test_so3_angles_host.settle's rule, decided on the restatement alone; a
    per-set threshold is drawn uniformly in (0, 180) degrees."""
    Cn, sets, lw = make_set_case(n, m, K, G)
    grouped = per_group or per_set
    if per_group:
        sets = per_group_sets(sets, G)
    elif per_set and G > 1:
        sets = np.stack([sets] * G)                                      # query_tau comes with a G: the library's form has sets per group
    label = "n %d m %d K %d G %d T %d per-set %d per-group %d" % (n, m, K, G, T, per_set, per_group)
    deg, tau = None, None
    if per_set:
        tau = tau_of(np.random.default_rng(9 + n + K).uniform(0.02, np.pi - 0.02, G * T * m)).reshape(G, T, m)
        ref = set_angle_cdf_fp64(Cn, sets, tau, lw, G > 1 and grouped)
    elif T:
        deg, ref = settle(DEG_OF_T[T], lambda d: set_angle_cdf_fp64(Cn, sets, tau_of(np.deg2rad(d)), lw, per_group), label)
        deg = tuple(deg)
    else:
        ref = set_angle_cdf_fp64(Cn, sets, None, lw, per_group)
    for a in list(ref.values()) + [Cn, sets] + ([lw] if lw is not None else []) + ([tau] if tau is not None else []):
        a.setflags(write=False)
    return (Cn, sets, lw, G > 1 and grouped), deg, tau, ref, label


WORST = {}                                                               # the largest fraction of each gate seen, per caller


def check_set_against(got, ref, deg, moments, who, label):
    """tests/test_so3_angles_host.check_against for outputs that may lack the moments or the masses: the same gates"""
    got = {k: np.asarray(v, np.float64) for k, v in got.items()}
    T = ref["mass"].shape[1]
    assert got["mass"].shape == ref["mass"].shape, label
    frac = {}
    for t in range(T):
        full = deg is not None and deg[t] >= 180.0
        U = np.zeros_like(ref["U"][:, t]) if full else ref["U"][:, t]
        assert (U <= U_CAP).all(), (label, "threshold", t, "undecided weight", float(U.max()))      # the band cannot hide a failure
        assert np.isfinite(got["mass"][:, t]).all() and np.isfinite(ref["mass"][:, t]).all(), label
        err = np.abs(got["mass"][:, t] - ref["mass"][:, t])
        if full:                                                         # the sum of the weights: no band
            assert (np.abs(got["mass"][:, t] - 1.0) <= 4e-6).all(), label
        frac["mass"] = np.maximum(frac.get("mass", 0.0), (err / (U + 4e-6 * ref["mass"][:, t] + 2.0 ** -23)).max())
    assert (got["mass"] >= 0.0).all() and (got["mass"] <= 1.0).all()
    if moments:
        assert got["mean_angle"].shape == ref["mean_angle"].shape and np.isfinite(got["mean_angle"]).all() and np.isfinite(got["mean_sq_angle"]).all()
        frac["mean_angle"] = (np.abs(got["mean_angle"] - ref["mean_angle"]) / ref["gate_mean"]).max()
        frac["mean_sq_angle"] = (np.abs(got["mean_sq_angle"] - ref["mean_sq_angle"]) / ref["gate_sq"]).max()
    else:
        assert "mean_angle" not in got and "mean_sq_angle" not in got
    print("%s: worst fraction of the gate %s; largest undecided weight %.2e" % (
        label, ", ".join("%s %.3f" % kv for kv in frac.items()), float(ref["U"].max()) if T else 0.0))
    for k, v in frac.items():
        WORST[who, k] = max(WORST.get((who, k), 0.0), float(v))
        assert v <= 1.0, (label, k, v)


def check_set_case(fn, case, who="host"):
    """``fn(centres, sets, log_weights, group_queries, thresholds=radians, query_tau=, moments=)`` against the restatement"""
    (Cn, sets, lw, grouped), deg, tau, ref, label = set_reference(*case)
    moments = case[7]
    got = fn(Cn, sets, lw, grouped, thresholds=np.deg2rad(deg) if deg else None, query_tau=tau, moments=moments)
    check_set_against(got, ref, deg, moments, who, label)
    return got


def check_set_bit_identities(fn, single):
    """The identities of include/rnf_hip.h beside RnfSo3SetAngleCdf, on ``fn``'s own bits; ``single``: rnf_so3_angle_cdf's counterpart"""
    Cn, sets, lw = make_set_case(4097, 9, 12, 3)
    th = np.deg2rad([15.0, 30.0, 60.0, 90.0, 120.0])
    whole = fn(Cn, sets, lw, False, thresholds=th)
    # K = 1: rnf_so3_angle_cdf's bits, shared thresholds and per query, one group and three, with and without moments
    one = sets[:, :1]
    tau = np.broadcast_to(tau_of(th)[None, :, None], (3, 5, 9)).copy()
    for lwk in (None, lw):
        for mom in (True, False):
            a, b = fn(Cn, one, lwk, False, thresholds=th, moments=mom), single(Cn, one[:, 0], lwk, False, thresholds=th, moments=mom)
            assert all(np.array_equal(a[k], b[k]) for k in a), (lwk is None, mom)
    a = fn(Cn, np.stack([one] * 3), lw, True, query_tau=tau)
    b = single(Cn, np.stack([one[:, 0]] * 3), lw, True, query_tau=tau)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # padding (NaN, inf, trailing and interleaved) and a permutation of the members
    rng = np.random.default_rng(3)
    padded = np.full((9, 30, 3, 3), np.nan, np.float32)
    slots = np.sort(rng.permutation(30)[:12])
    padded[:, slots] = sets[:, rng.permutation(12)]
    padded[:, [s for s in range(30) if s not in slots][0], 1, 1] = np.inf
    got = fn(Cn, padded, lw, False, thresholds=th)
    assert all(np.array_equal(got[k], whole[k]) for k in OUTPUTS)
    trailing = np.concatenate([sets, np.full((9, 1, 3, 3), np.nan, np.float32)], axis=1)
    got = fn(Cn, trailing, lw, False, thresholds=th)
    assert all(np.array_equal(got[k], whole[k]) for k in OUTPUTS)
    # thresholds split over calls, and as query_tau
    for a0, b0 in ((0, 1), (1, 3), (3, 5), (0, 4)):
        assert np.array_equal(fn(Cn, sets, lw, False, thresholds=th[a0:b0], moments=False)["mass"], whole["mass"][:, a0:b0])
    per = fn(Cn, np.stack([sets] * 3), lw, True, query_tau=tau)
    assert all(np.array_equal(per[k], whole[k]) for k in OUTPUTS)
    # the moments alone
    alone = fn(Cn, sets, lw, False)
    assert alone["mass"].shape == (3, 0, 9) and all(np.array_equal(alone[k], whole[k]) for k in OUTPUTS[1:])
    # group 2 of 3 alone; later sets dropped; the set's position; shared against per-group sets
    assert all(np.array_equal(fn(Cn, sets, lw[2:], False, thresholds=th)[k][0], whole[k][2]) for k in OUTPUTS)
    assert all(np.array_equal(fn(Cn, sets[:5], lw, False, thresholds=th)[k], whole[k][..., :5]) for k in OUTPUTS)
    rolled = fn(Cn, per_group_sets(sets, 3), lw, True, thresholds=th)
    for g in range(3):
        assert all(np.array_equal(np.roll(whole[k][g], 2 * g, axis=-1), rolled[k][g]) for k in OUTPUTS), g


def check_set_edge_cases(fn):
    n, m, K = 130, 7, 12
    Cn, sets, lw = make_set_case(n, m, K, 3)
    th = np.deg2rad([30.0, 90.0, 180.0])

    def nan_rows(got, g):
        return all(np.isnan(got[k][g]).all() for k in OUTPUTS)

    def fin_rows(got, g):
        return all(np.isfinite(got[k][g]).all() for k in OUTPUTS)

    clean = fn(Cn, sets, lw, False, thresholds=th)
    assert all(fin_rows(clean, g) for g in range(3))
    empty = sets.copy()
    empty[2, :, 0, 0] = np.nan                                           # a set of padding only: NaN, alone
    empty[4, :6] = np.inf
    got = fn(Cn, empty, lw, False, thresholds=th)
    for k in OUTPUTS:
        assert np.isnan(got[k][..., 2]).all() and np.isfinite(np.delete(got[k], 2, axis=-1)).all(), k
        assert np.array_equal(np.delete(got[k], [2, 4], axis=-1), np.delete(clean[k], [2, 4], axis=-1)), k
    dead = lw[1] == -np.inf
    bad = Cn.copy()
    bad[dead, 1, 1] = np.nan                                             # non-finite centres where group 1 has no weight
    bad[np.flatnonzero(dead)[0]] = np.inf
    got = fn(bad, sets, lw, False, thresholds=th)
    assert nan_rows(got, 0) and nan_rows(got, 2) and fin_rows(got, 1)
    assert all(np.array_equal(got[k][1], clean[k][1]) for k in OUTPUTS)  # left out whatever its entries
    lwn = lw.copy()
    lwn[2, 129] = np.nan
    got = fn(Cn, sets, lwn, False, thresholds=th)
    assert nan_rows(got, 2) and fin_rows(got, 0) and fin_rows(got, 1)
    lwd = lw.copy()
    lwd[0] = -np.inf                                                     # a group with no mass
    got = fn(Cn, sets, lwd, False, thresholds=th)
    assert nan_rows(got, 0) and fin_rows(got, 1) and fin_rows(got, 2)
    tau = np.full((1, 4, m), 2.0, np.float32)                            # a NaN slot is NaN alone, a negative one 0, FLT_MAX everything
    tau[0, 1], tau[0, 2], tau[0, 3] = np.nan, -1.0, FLT_MAX
    tau[0, 0, 5] = np.nan
    got = fn(Cn, sets, None, False, query_tau=tau)
    assert np.isnan(got["mass"][0, 1]).all() and (got["mass"][0, 2] == 0).all() and (np.abs(got["mass"][0, 3] - 1.0) <= 4e-6).all()
    assert np.isnan(got["mass"][0, 0, 5]) and np.isfinite(np.delete(got["mass"][0, 0], 5)).all() and np.isfinite(got["mean_angle"]).all()


def check_set_mass_orderings(fn):
    """The mass does not decrease with the threshold; a set's mass is at least each member's alone and at most their sum"""
    Cn, sets, lw = make_set_case(4097, 5, 12, 3)
    th = np.deg2rad(5.0 + np.arange(8) * 12.0)
    mass = fn(Cn, sets, lw, False, thresholds=th, moments=False)["mass"]
    assert (np.diff(mass, axis=1) >= 0).all()
    members = np.stack([fn(Cn, sets[:, s:s + 1], lw, False, thresholds=th, moments=False)["mass"] for s in range(12)])
    # the same non-negative weights in the same order, with an indicator that is nowhere smaller: fp32 rounding keeps the order
    assert (mass >= members.max(axis=0)).all()
    assert (mass <= members.astype(np.float64).sum(axis=0) + 12 * 2.0 ** -23).all()
    assert (mass[:, -1] > members[:, :, -1].max(axis=0)).all()           # a union of balls, not one ball


# ---- tests -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-m%d-K%d-G%d-T%d-%d%d%d" % c)
def test_host_build_against_the_restatement(case):
    check_set_case(host_set_angle_cdf, case)


def test_undecided_weight_stays_under_the_cap():
    """The condition of this file's docstring on the restatement alone: orbits of random estimates against random centres"""
    th = tau_of(np.deg2rad([5.0, 15.0, 30.0, 60.0, 90.0, 120.0, 150.0]))
    worst = 0.0
    for n in (63, 255, 4097):
        for K in (1, 12, 24, 36, 60):
            for G in (1, 3):
                Cn, sets, lw = make_set_case(n, 4, K, G, "uniform", seed=K)
                worst = max(worst, float(np.nanmax(set_angle_cdf_fp64(Cn, sets, th, lw)["U"])))
    print("largest undecided weight %.4f" % worst)
    assert worst <= U_CAP


def test_host_bit_identities():
    check_set_bit_identities(host_set_angle_cdf, host_single_angle_cdf)


def test_host_edge_cases():
    check_set_edge_cases(host_set_angle_cdf)


def test_host_mass_orderings():
    check_set_mass_orderings(host_set_angle_cdf)


def test_host_quantile_brackets_the_level():
    from rotationnormflow_amd.utils import angles
    Cn, sets, lw = make_set_case(4097, 5, 12, 3)
    levels, tol = (0.5, 0.9), 1e-3

    def quantile(lv, tol):
        rep = np.concatenate([sets] * len(lv), axis=0)

        def cdf(thresholds=None, query_tau=None):
            th = None if thresholds is None else [float(thresholds)]
            qt = None if query_tau is None else query_tau.numpy()
            sets_g = np.stack([rep] * 3) if qt is not None else rep
            got = host_set_angle_cdf(Cn, sets_g, lw, qt is not None, thresholds=th, query_tau=qt, moments=False)["mass"]
            return torch.from_numpy(got.astype(np.float64))
        passes = max(1, math.ceil(math.log(math.pi / tol) / math.log(9.0) - 1e-12))
        return {k: v.numpy() for k, v in angles._quantile_search(cdf, 3, 5, list(lv), passes, torch.device("cpu")).items()}

    def cdf64(theta):
        tau = np.where(theta >= np.pi, np.float32(FLT_MAX), (8.0 * np.sin(0.5 * theta) ** 2).astype(np.float32))[:, None, :].astype(np.float32)
        ref = set_angle_cdf_fp64(Cn, np.stack([sets] * 3), tau, lw, True)
        return ref["mass"][:, 0], ref["U"][:, 0]

    out = check_quantile(quantile, cdf64, levels, tol)
    assert out["radius"].shape == (3, 2, 5) and (out["radius"][:, 1] >= out["radius"][:, 0]).all()


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20
_TH = (C.c_double * 8)(*np.deg2rad(THRESHOLDS_DEG))


def _args(**kw):
    base = dict(centres=_FAKE, queries=_FAKE * 2, log_weights=_FAKE, n=4608, m=1000, K=60, G=3, T=8, thresholds=C.addressof(_TH), mass=_FAKE,
                mean_angle=_FAKE, mean_sq_angle=_FAKE)
    base.update(kw)
    a = _lib.So3SetAngleCdf(**base)
    a.workspace, a.workspace_bytes = _FAKE, _lib.lib().rnf_so3_set_angle_cdf_workspace_bytes(C.byref(a))
    return a


def _refused(a, word):
    L = _lib.lib()
    assert L.rnf_so3_set_angle_cdf(C.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg and "RnfSo3SetAngleCdf" in msg, msg


def test_c_abi_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.rnf_abi_version() == 8
    a = _args()
    rule = (8 * 3 * 10 * 2 * 1000 + 16 * 3 * 2 + 8 * 3 + 4 * 3 * 4608 + 15) // 16 * 16
    assert a.workspace_bytes == rule == _host_lib().hsac_workspace_bytes(C.c_longlong(4608), C.c_longlong(1000), 3, 10)
    assert _args(K=1).workspace_bytes == rule == _args(K=4096).workspace_bytes                # the workspace does not grow with K
    single = _lib.So3AngleCdf(centres=_FAKE, queries=_FAKE, n=4608, m=1000, G=3, T=8, mass=_FAKE, mean_angle=_FAKE)
    assert L.rnf_so3_angle_cdf_workspace_bytes(C.byref(single)) == rule
    assert _args(mean_angle=None, mean_sq_angle=None).workspace_bytes == (8 * 3 * 8 * 2 * 1000 + 16 * 3 * 2 + 8 * 3 + 4 * 3 * 4608 + 15) // 16 * 16
    for bad, word in ((dict(G=0), "G="), (dict(G=65536), "G="), (dict(n=0), "n="), (dict(n=(1 << 24) + 1), "n="), (dict(m=-1), "m="),
                      (dict(m=1 << 31), "m="), (dict(T=-1), "T="), (dict(T=9), "T="), (dict(K=0), "K="), (dict(K=4097), "K="),
                      (dict(K=-3), "K=")):
        _refused(_args(**bad), word)
        assert L.rnf_so3_set_angle_cdf_workspace_bytes(C.byref(_lib.So3SetAngleCdf(**{**dict(n=10, m=10, K=1, G=1, T=1), **bad}))) == 0
    _refused(_args(T=0, thresholds=None, mean_angle=None, mean_sq_angle=None), "T=0 requires")
    _refused(_args(T=0), "T=0 with")
    _refused(_args(query_tau=_FAKE), "both thresholds and query_tau")
    _refused(_args(thresholds=None), "neither thresholds nor query_tau")
    for k, v in enumerate((-1e-9, np.pi * (1 + 1e-15), float("nan"), float("inf"))):
        th = (C.c_double * 8)(*np.deg2rad(THRESHOLDS_DEG))
        th[k] = v
        _refused(_args(thresholds=C.addressof(th)), "thresholds[%d]" % k)
    _refused(_args(centres=_FAKE + 4), "aligned")
    _refused(_args(queries=_FAKE + 8), "aligned")
    _refused(_args(centres=None), "null")
    _refused(_args(queries=None), "null")
    _refused(_args(G=65535, n=1 << 24, m=(1 << 31) - 1), "tile")         # a workspace no size_t holds
    a = _args()
    a.workspace_bytes -= 1
    _refused(a, "workspace")
    a = _args()
    a.workspace += 4
    _refused(a, "workspace")
    a = _args()
    a.struct_bytes += 8
    _refused(a, "struct_bytes")
    assert L.rnf_so3_set_angle_cdf_workspace_bytes(C.byref(a)) == 0
    assert L.rnf_so3_set_angle_cdf(C.byref(_args(m=0))) == 0             # a no-op
    assert C.sizeof(_lib.So3AngleCdf) == 128                             # the old struct stays as it was


def test_header_declares_the_struct_the_binding_mirrors():
    import re
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    body = header[header.index("typedef struct RnfSo3SetAngleCdf {") + 33:header.index("} RnfSo3SetAngleCdf;")]
    names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
    assert names == [f for f, _ in _lib.So3SetAngleCdf._fields_], names
    assert names[0] == "struct_bytes" and names[-3:] == ["workspace", "workspace_bytes", "stream"] and "K" in names
    assert {"rnf_so3_set_angle_cdf", "rnf_so3_set_angle_cdf_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "#define RNF_ABI_VERSION 8" in header
    h = _host_lib()
    assert h.hsac_groups_for(6) == 4 and h.hsac_groups_for(10) == 2
    wave = lambda m, nchunk, G, K: h.hsac_wave_per_set(C.c_longlong(m), C.c_longlong(nchunk), C.c_longlong(G), K)      # noqa: E731
    assert wave(8, 9, 16, 60) and not wave(64, 9, 16, 60) and wave(4096, 1, 1, 8) and not wave(4097, 1, 1, 8) and not wave(1366, 1, 3, 12) and not wave(4, 1, 1, 7)


# ---- symmetry groups ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,order", [("C1", 1), ("C2", 2), ("C7", 7), ("C360", 360), ("D1", 2), ("D3", 6), ("D360", 720), ("T", 12), ("O", 24),
                                        ("I", 60)])
def test_point_group_is_a_group_of_rotations(name, order):
    S = symmetry.point_group(name)
    assert S.dtype == torch.float32 and tuple(S.shape) == (order, 3, 3)
    assert torch.equal(S[0], torch.eye(3))
    S64 = S.numpy().astype(np.float64)
    assert np.abs(np.linalg.det(S64) - 1.0).max() <= 1e-6
    assert np.abs(S64 @ S64.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
    sub = S64 if order <= 60 else S64[:: order // 24]                    # every product and every inverse is a member, to 1e-6
    prod = (sub[:, None] @ S64[None]).reshape(-1, 1, 9)
    assert (np.abs(prod - S64.reshape(1, -1, 9)).max(axis=2).min(axis=1) <= 1e-6).all()
    inv = sub.transpose(0, 2, 1).reshape(-1, 1, 9)
    assert (np.abs(inv - S64.reshape(1, -1, 9)).max(axis=2).min(axis=1) <= 1e-6).all()
    pair = np.abs(S64.reshape(-1, 1, 9) - S64.reshape(1, -1, 9)).max(axis=2) + np.eye(order)
    assert pair.min() > 1e-3                                             # no member twice


def test_point_group_refuses_other_names():
    for bad in ("", "C0", "D", "S4", "Oh", "c3", 3):
        with pytest.raises(ValueError, match="point_group"):
            symmetry.point_group(bad)
    with pytest.raises(ValueError, match="4096"):
        symmetry.point_group("D2049")


def test_orbit_and_symmetry_from_truths():
    R = torch.from_numpy(draw("uniform", 6, 5)).reshape(2, 3, 3, 3)
    for name in ("C5", "D4", "T", "O", "I"):
        S = symmetry.point_group(name)
        orb = symmetry.orbit(R, S)
        assert tuple(orb.shape) == (2, 3, len(S), 3, 3) and torch.equal(orb[..., 0, :, :], R)
        assert (orb[1, 2, 3 % len(S)] - R[1, 2] @ S[3 % len(S)]).abs().max() <= 1e-6      # right multiplication, member by member
        back = symmetry.symmetry_from_truths(orb)
        assert tuple(back.shape) == tuple(orb.shape) and (back - S).abs().max() <= 4e-6
    S = symmetry.point_group("T")
    orb = symmetry.orbit(R, S).clone()
    orb[0, 1, 5] = float("nan")                                          # a padding truth stays a padding member
    back = symmetry.symmetry_from_truths(orb)
    assert torch.isnan(back[0, 1, 5]).all() and torch.isfinite(back[0, 1, :5]).all() and torch.isfinite(back[1]).all()
    per = symmetry.orbit(R[:, 0], torch.stack([S, S]))                   # one group per estimate
    assert torch.equal(per, symmetry.orbit(R, S)[:, 0])
    for bad in (torch.zeros(3), torch.zeros(2, 3, 4)):
        with pytest.raises(ValueError, match="orbit"):
            symmetry.orbit(bad, S)
        with pytest.raises(ValueError, match="symmetry_from_truths"):
            symmetry.symmetry_from_truths(bad)
    with pytest.raises(ValueError, match="symmetry"):
        symmetry.orbit(R, torch.zeros(3, 3))


@pytest.mark.parametrize("name,radius", [("O", 63.0), ("I", 63.0)])
def test_covering_radius_and_full_mass_at_120_degrees(name, radius):
    """Every rotation is within 63 degrees of a member of O (62.8) and of I (44.5): the ball of 120 degrees about an orbit holds every
    centre, and the mass is the sum of the weights"""
    S = symmetry.point_group(name).numpy()
    Cn, sets, lw = make_set_case(4097, 3, len(S), 3, "uniform")
    near = angle_deg(sets[:, None, :], Cn[None, :, None]).min(axis=2)    # [m,n]
    assert near.max() < radius
    got = host_set_angle_cdf(Cn, sets, lw, False, thresholds=np.deg2rad([radius, 120.0]), moments=False)["mass"]
    assert (np.abs(got - 1.0) <= 4e-6).all()


def test_python_entry_points_validate_their_arguments():
    from rotationnormflow_amd import grid_pose, harness
    from rotationnormflow_amd.utils import angles
    R = torch.eye(3).expand(5, 3, 3).contiguous()
    with pytest.raises(ValueError, match="query_sets"):
        angles.so3_set_angle_cdf(R, R, [0.1])
    with pytest.raises(ValueError, match="query_sets"):
        angles.so3_set_angle_cdf(R, R[None], [0.1], group_queries=True)
    with pytest.raises(ValueError, match="members"):
        angles.so3_set_angle_cdf(R, torch.zeros(2, 0, 3, 3), [0.1])
    with pytest.raises(ValueError, match="members"):
        angles.so3_set_angle_quantile(R, torch.zeros(1, 4097, 3, 3), [0.5])
    with pytest.raises(ValueError, match="centres"):
        angles.so3_set_angle_cdf(R, R[:, None], [0.1])                   # on the CPU
    with pytest.raises(ValueError, match="centres"):
        angles.so3_set_angle_quantile(R, R[:, None], [0.5])
    lp, grid = torch.zeros(2, 72), torch.zeros(72, 3, 3)
    with pytest.raises(ValueError, match="sets"):
        harness.grid_set_error(lp, grid, torch.zeros(2, 4, 3, 3))
    with pytest.raises(ValueError, match="GPU"):
        harness.grid_set_error(lp, grid, torch.zeros(2, 4, 5, 3, 3))
    with pytest.raises(ValueError, match="thresholds_deg"):
        harness.grid_set_error(lp, grid, torch.zeros(2, 4, 5, 3, 3), thresholds_deg=(190.0,))
    with pytest.raises(ValueError, match="level"):
        harness.grid_set_error(lp, grid, torch.zeros(2, 4, 5, 3, 3), levels=(0.0,))
    with pytest.raises(ValueError, match="est"):
        harness.grid_error_symmetric(lp, grid, torch.zeros(3, 4, 3, 3), symmetry.point_group("T"))
    with pytest.raises(ValueError, match="symmetry=None"):
        harness.grid_error_symmetric(lp, grid, torch.zeros(2, 4, 3, 3))
    with pytest.raises(ValueError, match="symmetry=None"):
        harness.grid_error_symmetric(lp, grid, torch.zeros(2, 4, 3, 3), gt=torch.zeros(2, 3, 3))
    with pytest.raises(ValueError, match="symmetry"):
        harness.grid_error_symmetric(lp, grid, torch.zeros(2, 4, 3, 3), torch.zeros(3, 12, 3, 3))
    with pytest.raises(ValueError, match="gt"):
        harness.grid_error_symmetric(lp, grid, torch.zeros(2, 4, 3, 3), symmetry.point_group("T"), gt=torch.zeros(3, 3, 3))
    with pytest.raises(ValueError, match="GPU"):
        harness.grid_error_symmetric(lp, grid, torch.zeros(2, 4, 3, 3), symmetry.point_group("T"))
    with pytest.raises(ValueError, match="symmetric"):                   # grid_error keeps its refusal
        harness.grid_error(lp, grid, torch.zeros(2, 4, 3, 3), gt=torch.zeros(2, 3, 3, 3))
    assert harness.grid_set_error is grid_pose.grid_set_error and harness.grid_error_symmetric is grid_pose.grid_error_symmetric
    assert harness.grid_pose_error_symmetric is grid_pose.grid_pose_error_symmetric and angles.MAX_MEMBERS == 4096 == symmetry.MAX_ORDER


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_so3_set_angle_cdf.cpp (its own main) built with the host-side address and undefined-behaviour sanitizers
    (-Xarch_host: host code only, nothing for the GPU) and run as a process of its own."""
    exe = str(tmp_path / "sanitize_so3_set_angle_cdf")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_so3_set_angle_cdf.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)
