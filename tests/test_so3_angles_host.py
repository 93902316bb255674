"""CPU: the distribution function of the geodesic angle (csrc/so3_angle_cdf.h, rnf_so3_angle_cdf) and what is built on it.

``angle_cdf_fp64`` is the numpy fp64 restatement of the definition from the same fp32 inputs -- d2 from the nine differences, the
indicator d2 <= tau, theta = 2 asin(min(1, sqrt(d2 / 8))), weights by an explicit softmax -- with the edge cases of include/rnf_hip.h;
tests/test_gpu_so3_angles.py imports it, the cases and the gates.  Here the host build of the header (the same row functions in the
kernels' order) is held to it, and the edge cases, the C ABI's refusals, the workspace rule, the struct against its binding, the bracket
search of utils/angles.py (on the host build) and the Python argument checks are exercised without a device.

The gates.  The fp32 d2 is within 1e-6 of the fp64 one, relatively (the constant of tests/test_so3_kde_host.py's gate; 3.0e-7 at most
was measured on these cases).
  mass:   |mass - ref| <= U + 4e-6 ref + 2^-23, U = sum_j w_j [|d2_64 - tau| <= 1e-6 d2_64]: the weight of the pairs that rounding may
          put on either side of the threshold.  So that the band cannot hide a failure, U <= 0.01 is asserted on the restatement for
          every (query, threshold) below 180 degrees that a test uses.  At 180 degrees there is no band: the mass is the sum of the weights.
  angles: per pair delta = 1e-6 d2 and g_ij = min(delta / (4 sin theta), sqrt(delta / 2)) + 1e-6 theta + 4e-7 -- d theta = d d2 /
          (4 sin theta), capped at the half turn where pi - theta = sqrt((8 - d2) / 2) --
          |mean_angle - ref| <= sum_j w_j g_ij,   |mean_sq_angle - ref| <= sum_j w_j 2 theta_ij g_ij + 1e-6 ref.
  radii:  with the returned lo, hi: F64(lo) - U(lo) - eps < alpha <= F64(hi) + U(hi) + eps, eps = 4e-6 + 2^-23, and hi - lo <= tol.

Measured, the worst fraction of each gate over test_host_build_against_the_restatement (n <= 4097, m <= 1000): mass 0.996 -- a pair
inside the band on the other side, so that the error is that pair's weight -- and 0.102 of 4e-6 ref + 2^-23 beyond the band; mean_angle
0.343; mean_sq_angle 0.343.  Per-query thresholds: 0.015, 0.052, 0.053.  The MI355X's figures are in tests/test_gpu_so3_angles.py;
DESIGN.md 3.3f has both."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib
from tests.test_so3_kde_host import draw, make_case, ptr, rodrigues  # noqa: F401  (re-exported for the GPU tests)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_so3_angle_cdf.cpp")
OUT = os.path.join(HERE, "csrc", "_host_so3_angle_cdf.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f)
        for f in ("so3_angle_cdf.h", "so3_kernel_sum.h", "fisher_exact.h", "fisher_math.h")]
THRESHOLDS_DEG = (5.0, 15.0, 30.0, 60.0, 90.0, 120.0, 150.0, 180.0)
FLT_MAX = float(np.finfo(np.float32).max)
EPS = 4e-6 + 2.0 ** -23
U_CAP = 0.01
OUTPUTS = ("mass", "mean_angle", "mean_sq_angle")
STEP_DEG = 0.01                                                          # a threshold whose band is too heavy moves by multiples of this


def _host_lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    h = C.CDLL(OUT)
    h.hac_workspace_bytes.restype = C.c_ulonglong
    return h


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def tau_of(theta):
    """tau of shared angles in radians: 8 sin^2(theta / 2) in fp64 rounded once to fp32, FLT_MAX from pi on -> float32 array"""
    theta = np.atleast_1d(np.asarray(theta, np.float64))
    return np.where(theta >= np.pi, np.float32(FLT_MAX), (8.0 * np.sin(0.5 * theta) ** 2).astype(np.float32)).astype(np.float32)


def angle_cdf_fp64(centres, queries, taus, log_weights=None, group_queries=False):
    """The outputs of rnf_so3_angle_cdf in fp64 from the fp32 inputs, with the edge cases of include/rnf_hip.h.  ``taus``: float32 [T]
    shared, or [G,T,m] per (group, query), or None (T = 0).  -> dict of mass [G,T,m], U [G,T,m] (the undecided weight of this file's
    docstring), mean_angle, mean_sq_angle, gate_mean, gate_sq [G,m]."""
    Cn = np.asarray(centres, np.float32).reshape(-1, 9).astype(np.float64)
    n = len(Cn)
    lw = None if log_weights is None else np.asarray(log_weights, np.float32).reshape(-1, n).astype(np.float64)
    Qa = np.asarray(queries, np.float32).astype(np.float64)
    Qa = Qa.reshape(-1, Qa.shape[-3], 9) if group_queries else Qa.reshape(1, -1, 9)
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
    d2 = None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for g in range(G):
            Qr = Qa[g if group_queries else 0]
            q_ok = np.isfinite(Qr).all(axis=1)
            live = lw[g] != -np.inf
            if np.isnan(lw[g]).any() or (live & ~c_ok).any() or not live.any() or np.isposinf(lw[g]).any():
                continue
            if group_queries or d2 is None:
                diff = np.where(q_ok[:, None], Qr, 0.0)[:, None, :] - np.where(c_ok[:, None], Cn, 0.0)[None, :, :]
                d2 = np.einsum("ijk,ijk->ij", diff, diff)                # the pairs of a row that is not finite never count
                del diff
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
                bad = ~q_ok | np.isnan(tq[g, t])
                res["mass"][g, t][bad] = np.nan
            res["mean_angle"][g] = theta @ w
            res["mean_sq_angle"][g] = (theta * theta) @ w
            res["gate_mean"][g] = gij @ w
            res["gate_sq"][g] = (2.0 * theta * gij) @ w + 1e-6 * res["mean_sq_angle"][g]
            for k in ("mean_angle", "mean_sq_angle"):
                res[k][g][~q_ok] = np.nan
    return res


def angle_deg(A, B):
    """The angle between rotations [..,3,3], in degrees (fp64)"""
    tr = np.einsum("...ij,...ij->...", np.asarray(A, np.float64), np.asarray(B, np.float64))
    return np.degrees(np.arccos(np.clip(0.5 * (tr - 1.0), -1.0, 1.0)))


def host_angle_cdf(centres, queries, log_weights=None, group_queries=False, thresholds=None, query_tau=None, moments=True, mass=True):
    """The host build of the kernels' arithmetic -> dict of float32 arrays with a leading G.  ``thresholds``: angles in radians (shared);
    ``query_tau`` float32 [G,T,m]."""
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
    out = {}
    if mass:
        out["mass"] = np.full((G, T, m), 7.0, np.float32)
    if moments:
        out["mean_angle"], out["mean_sq_angle"] = np.full((G, m), 7.0, np.float32), np.full((G, m), 7.0, np.float32)
    h.hac_angle_cdf(ptr(Cn), ptr(Qr), ptr(lw), C.c_longlong(n), C.c_longlong(m), G, int(group_queries), T, ptr(th), ptr(qt),
                    *[ptr(out.get(k)) for k in OUTPUTS])
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

def group_sets(Qr, G):
    """One set of queries per group from one set: group g takes it rolled by 7 g rows"""
    return np.stack([np.roll(Qr, 7 * g, axis=0) for g in range(G)])


def settle(nominal_deg, restate, label=""):
    """The rule that moves a threshold whose band is too heavy: ``restate(degrees)`` -> the restatement at those shared thresholds;
    threshold t below 180 degrees moves to nominal + STEP_DEG, + 2 STEP_DEG, .. until its undecided weight is within U_CAP for every
    (group, query).  -> (degrees, restatement)"""
    deg = list(nominal_deg)
    for attempt in range(1, 17):
        ref = restate(deg)
        heavy = [t for t in range(len(deg)) if deg[t] < 180.0 and np.nanmax(ref["U"][:, t]) > U_CAP]
        if not heavy:
            break
        for t in heavy:
            deg[t] = nominal_deg[t] + attempt * STEP_DEG
            print("%s: threshold %g degrees moved to %g" % (label, nominal_deg[t], deg[t]))
    return deg, ref


@functools.lru_cache(maxsize=6)
def reference(n, m, kind, weighted, group_queries=False):
    """(case, thresholds in degrees, restatement): computed once per case, and left unchanged.  A threshold below 180 degrees within
    1e-6 (relatively, in d2) of which the case has pairs that carry more than U_CAP of a query's weight -- one pair is enough while
    n < 100 -- is moved by STEP_DEG, then 2 STEP_DEG, .. until the restatement's undecided weight is within the cap for every query:
    a property of the case and the restatement alone."""
    Cn, Qr, lw = make_case(n, m, kind, weighted)
    if group_queries:
        Qr = group_sets(Qr, 3 if weighted else 1)
    deg, ref = settle(THRESHOLDS_DEG, lambda d: angle_cdf_fp64(Cn, Qr, tau_of(np.deg2rad(d)), lw, group_queries),
                      "n %d m %d %s weighted %d per-group %d" % (n, m, kind, weighted, group_queries))
    for a in list(ref.values()) + [Cn, Qr] + ([lw] if lw is not None else []):
        a.setflags(write=False)
    return (Cn, Qr, lw), tuple(deg), ref


WORST = {}                                                               # the largest fraction of each gate seen, per caller


def check_against(got, ref, deg, who, label):
    """The outputs ``got`` against the restatement ``ref`` on the gates of this file's docstring; ``deg``: the shared thresholds in degrees,
    or None where they are per query (then every slot has its band)"""
    got = {k: np.asarray(v, np.float64) for k, v in got.items()}
    T = ref["mass"].shape[1]
    assert got["mass"].shape == ref["mass"].shape and got["mean_angle"].shape == ref["mean_angle"].shape
    assert all(np.isfinite(got[k]).all() and np.isfinite(ref[k]).all() for k in OUTPUTS), label
    frac = {}
    for t in range(T):
        full = deg is not None and deg[t] >= 180.0
        U = np.zeros_like(ref["U"][:, t]) if full else ref["U"][:, t]
        assert (U <= U_CAP).all(), (label, "threshold", t, "undecided weight", float(U.max()))      # the band cannot hide a failure
        err = np.abs(got["mass"][:, t] - ref["mass"][:, t])
        if full:                                                         # the sum of the weights: no band
            assert (np.abs(got["mass"][:, t] - 1.0) <= 4e-6).all(), label
        frac["mass"] = np.maximum(frac.get("mass", 0.0), (err / (U + 4e-6 * ref["mass"][:, t] + 2.0 ** -23)).max())
        frac["mass_rounding"] = np.maximum(frac.get("mass_rounding", 0.0), (np.maximum(err - U, 0.0) / (4e-6 * ref["mass"][:, t] + 2.0 ** -23)).max())
    assert (got["mass"] >= 0.0).all() and (got["mass"] <= 1.0).all()
    frac["mean_angle"] = (np.abs(got["mean_angle"] - ref["mean_angle"]) / ref["gate_mean"]).max()
    frac["mean_sq_angle"] = (np.abs(got["mean_sq_angle"] - ref["mean_sq_angle"]) / ref["gate_sq"]).max()
    print("%s: worst fraction of the gate %s; largest undecided weight %.2e" % (
        label, ", ".join("%s %.3f" % kv for kv in frac.items()), float(ref["U"].max()) if T else 0.0))
    for k, v in frac.items():
        WORST[who, k] = max(WORST.get((who, k), 0.0), float(v))
        assert v <= 1.0, (label, k, v)


def check_case(fn, n, m, kind, weighted, group_queries=False, who="host"):
    """``fn(centres, queries, log_weights, group_queries, thresholds=radians)`` against the restatement on the gates"""
    (Cn, Qr, lw), deg, ref = reference(n, m, kind, weighted, group_queries)
    got = fn(Cn, Qr, lw, group_queries, thresholds=np.deg2rad(deg))
    check_against(got, ref, deg, who, "n %d m %d %s weighted %d per-group %d" % (n, m, kind, weighted, group_queries))


def query_tau_case(n=4097, m=65, kind="clustered", G=3, T=3, seed=9):
    """A case with thresholds per (group, query): tau of angles drawn uniformly in (0, 180) degrees, queries per group"""
    Cn, Qr, lw = make_case(n, m, kind, True)
    Qg = group_sets(Qr, G)
    tau = tau_of(np.random.default_rng(seed).uniform(0.02, np.pi - 0.02, G * T * m)).reshape(G, T, m)
    return Cn, Qg, lw, tau


def check_query_tau(fn, who="host"):
    Cn, Qg, lw, tau = query_tau_case()
    ref = angle_cdf_fp64(Cn, Qg, tau, lw, True)
    check_against(fn(Cn, Qg, lw, True, query_tau=tau), ref, None, who, "per-query thresholds")
    # the same thresholds shared by the groups' shared queries: [1,T,m] is not a form of the library, so group by group
    one = fn(Cn, Qg[1:2], lw[1:2], True, query_tau=tau[1:2])
    assert np.array_equal(one["mass"][0], fn(Cn, Qg, lw, True, query_tau=tau)["mass"][1])


def check_edge_cases(fn):
    """The edge cases of include/rnf_hip.h beside RnfSo3AngleCdf, for every output of the (group, query)"""
    n, m = 130, 70
    Cn, Qr, lw = make_case(n, m, "uniform", True)
    th = np.deg2rad([30.0, 90.0, 180.0])

    def nan_rows(got, g):
        return all(np.isnan(got[k][g]).all() for k in OUTPUTS)

    def fin_rows(got, g):
        return all(np.isfinite(got[k][g]).all() for k in OUTPUTS)

    dead = lw[1] == -np.inf
    bad = Cn.copy()
    bad[dead, 1, 1] = np.nan                                             # NaN entries where group 1 has no weight: groups 0 and 2 hold them
    bad[np.flatnonzero(dead)[0]] = np.inf
    got, clean = fn(bad, Qr, lw, False, thresholds=th), fn(Cn, Qr, lw, False, thresholds=th)
    assert nan_rows(got, 0) and nan_rows(got, 2) and fin_rows(got, 1)
    assert all(np.array_equal(got[k][1], clean[k][1]) for k in OUTPUTS)  # left out whatever its entries
    ref = angle_cdf_fp64(bad, Qr, tau_of(th), lw)
    assert (np.abs(got["mass"][1] - ref["mass"][1]) <= ref["U"][1] + 4e-6 * ref["mass"][1] + 2.0 ** -23).all()
    lwn = lw.copy()
    lwn[2, 129] = np.nan
    got = fn(Cn, Qr, lwn, False, thresholds=th)
    assert nan_rows(got, 2) and fin_rows(got, 0) and fin_rows(got, 1)
    lwd = lw.copy()
    lwd[0] = -np.inf                                                     # a group with no mass
    got = fn(Cn, Qr, lwd, False, thresholds=th)
    assert nan_rows(got, 0) and fin_rows(got, 1) and fin_rows(got, 2)
    Qb = Qr.copy()
    Qb[3, 0, 2], Qb[69, 2, 2] = np.inf, np.nan
    got = fn(Cn, Qb, None, False, thresholds=th)
    for k in OUTPUTS:
        assert np.isnan(got[k][0][..., [3, 69]]).all(), k
        assert np.isfinite(np.delete(got[k][0], [3, 69], axis=-1)).all(), k
    # thresholds per query: a NaN entry is NaN for its slot only, a negative one gives 0, FLT_MAX everything
    tau = np.full((1, 4, m), 2.0, np.float32)
    tau[0, 1], tau[0, 2], tau[0, 3] = np.nan, -1.0, FLT_MAX
    tau[0, 0, 5] = np.nan
    got = fn(Cn, Qr, None, False, query_tau=tau)
    assert np.isnan(got["mass"][0, 1]).all() and (got["mass"][0, 2] == 0).all() and (np.abs(got["mass"][0, 3] - 1.0) <= 4e-6).all()
    assert np.isnan(got["mass"][0, 0, 5]) and np.isfinite(np.delete(got["mass"][0, 0], 5)).all() and np.isfinite(got["mean_angle"]).all()
    # one centre: its own distribution function; the query that is the centre has angle 0 and all of the mass at tau = 0
    one, q = draw("uniform", 1, 21), np.concatenate([draw("uniform", 5, 22), draw("uniform", 1, 21)])
    got = fn(one, q, None, False, thresholds=[0.0, np.pi])
    ang = 2.0 * np.arcsin(np.minimum(1.0, np.sqrt(((q.astype(np.float64) - one.astype(np.float64)) ** 2).sum(axis=(1, 2)) / 8.0)))
    assert (got["mass"][0, 0] == [0, 0, 0, 0, 0, 1]).all() and (got["mass"][0, 1] == 1).all()
    assert (np.abs(got["mean_angle"][0] - ang) <= 1e-6 * ang + 4e-7).all() and got["mean_angle"][0, 5] == 0.0
    assert (np.abs(got["mean_sq_angle"][0] - ang ** 2) <= 2e-6 * ang ** 2 + 4e-7).all()
    # T = 0: the moments alone, with the bits they have beside thresholds; the masses alone likewise
    alone, both = fn(Cn, Qr, lw, False), fn(Cn, Qr, lw, False, thresholds=th)
    assert alone["mass"].shape == (3, 0, m) and all(np.array_equal(alone[k], both[k]) for k in OUTPUTS[1:])
    assert np.array_equal(fn(Cn, Qr, lw, False, thresholds=th, moments=False)["mass"], both["mass"])


def check_quantile(quantile, cdf64, levels=(0.5, 0.9), tol=1e-3):
    """``quantile(levels, tol)`` -> dict of numpy [G,L,m] (radius, lo, mass_lo, mass_hi) against ``cdf64(theta [G,m]) -> (F64, U)``, the
    restatement at per-query angles: the bracket of this file's docstring"""
    out = quantile(levels, tol)
    lo, hi = out["lo"], out["radius"]
    assert np.isfinite(hi).all() and (hi - lo <= tol).all() and (lo >= 0).all() and (hi <= np.pi).all()
    for k, a in enumerate(levels):
        f_lo, u_lo = cdf64(lo[:, k])
        f_hi, u_hi = cdf64(hi[:, k])
        top = hi[:, k] >= np.pi                                          # pi is taken to satisfy every level
        zero = hi[:, k] == 0.0                                           # radius 0: the mass at tau = 0 reaches the level; there is no lo
        # no cap on the band here: hi sits just above the jump that carries F over the level, within tol in angle -- near the half turn,
        # where d tau / d theta = 4 sin theta vanishes, and for a tol of a few bands, the jump itself lies inside the band of hi
        assert ((f_lo - u_lo - EPS < a) | zero).all() and ((a <= f_hi + u_hi + EPS) | top).all(), a
        assert (lo[:, k][zero] == 0.0).all()
    return out


# ---- tests -------------------------------------------------------------------------------------------------------------------------------

def test_tau_of_the_library_is_the_restatements():
    h = _host_lib()
    th = np.deg2rad(np.array(THRESHOLDS_DEG + (0.0, 179.9)))
    tau = np.empty(len(th), np.float32)
    h.hac_tau(ptr(th), len(th), ptr(tau))
    assert np.array_equal(tau, tau_of(th)) and tau[7] == np.float32(FLT_MAX) and tau[8] == 0.0 and tau[9] < 8.0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 4095, 4096, 4097])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("weighted", [False, True])
def test_host_build_against_the_restatement(n, kind, weighted):
    for m in (1, 65, 1000):
        check_case(host_angle_cdf, n, m, kind, weighted)
    check_case(host_angle_cdf, n, 65, kind, weighted, True)
    print("worst fractions so far:", {k[1]: round(v, 4) for k, v in WORST.items() if k[0] == "host"})


def test_host_thresholds_per_query():
    check_query_tau(host_angle_cdf)


def test_host_edge_cases():
    check_edge_cases(host_angle_cdf)


def test_host_mass_does_not_decrease_with_the_threshold():
    """On the host build's own bits: the indicators are nested and every sum adds the same non-negative weights in the same order"""
    Cn, Qr, lw = make_case(4097, 65, "clustered", True)
    for lo in (0.0, 22.5):
        th = np.deg2rad(lo + np.arange(8) * 22.5)
        mass = host_angle_cdf(Cn, Qr, lw, thresholds=th, moments=False)["mass"]
        assert (np.diff(mass, axis=1) >= 0).all()
    tight = tau_of(np.deg2rad(30.0))[0]
    tau = np.broadcast_to(np.array([np.nextafter(tight, np.float32(0)), tight, np.nextafter(tight, np.float32(9))], np.float32)[None, :, None], (3, 3, 65))
    assert (np.diff(host_angle_cdf(Cn, Qr, lw, query_tau=tau, moments=False)["mass"], axis=1) >= 0).all()


def test_host_mass_of_a_threshold_does_not_depend_on_the_others():
    """mass[g][t][i] bit-identical whether threshold t is passed alone or among 8, shared or as query_tau, with or without the moments"""
    Cn, Qr, lw = make_case(4097, 65, "clustered", True)
    th = np.deg2rad(THRESHOLDS_DEG)
    whole = host_angle_cdf(Cn, Qr, lw, thresholds=th)
    for t in range(8):
        assert np.array_equal(host_angle_cdf(Cn, Qr, lw, thresholds=th[t:t + 1], moments=False)["mass"][:, 0], whole["mass"][:, t]), t
    for a, b in ((0, 3), (3, 8), (1, 3)):                               # 3, 5 and 2 slots: the kernels of 4, 8 and 2
        assert np.array_equal(host_angle_cdf(Cn, Qr, lw, thresholds=th[a:b])["mass"], whole["mass"][:, a:b])
    tau = np.broadcast_to(tau_of(th)[None, :, None], (3, 8, 65))
    per = host_angle_cdf(Cn, Qr, lw, query_tau=tau)
    assert all(np.array_equal(per[k], whole[k]) for k in OUTPUTS)


def test_host_result_does_not_depend_on_the_batch():
    Cn, Qr, lw = make_case(4097, 300, "clustered", True)
    th = np.deg2rad([15.0, 30.0, 120.0])
    whole = host_angle_cdf(Cn, Qr, lw, thresholds=th)
    head = host_angle_cdf(Cn, Qr[:200], lw, thresholds=th)               # later queries dropped
    tail = host_angle_cdf(Cn, Qr, lw[2:], thresholds=th)                 # earlier groups dropped
    per = host_angle_cdf(Cn, np.stack([Qr] * 3), lw, True, thresholds=th)   # the same queries passed per group
    for k in OUTPUTS:
        assert np.array_equal(whole[k][..., :200], head[k]), k
        assert np.array_equal(whole[k][2:], tail[k]), k
        assert np.array_equal(whole[k], per[k]), k
    rolled = host_angle_cdf(Cn, group_sets(Qr, 3), lw, True, thresholds=th)
    for g in range(3):
        assert np.array_equal(np.roll(whole["mass"][g], 7 * g, axis=-1), rolled["mass"][g]), g


def host_quantile(Cn, Qr, lw, group_queries=False):
    """utils/angles.py's bracket search on the host build -> quantile(levels, tol) of check_quantile"""
    from rotationnormflow_amd.utils import angles
    G = Qr.shape[0] if group_queries else (1 if lw is None else len(lw))
    m = Qr.shape[-3]

    def quantile(levels, tol):
        Qrep = np.concatenate([Qr] * len(levels), axis=-3)              # the queries once per level, as so3_angle_quantile passes them

        def cdf(thresholds=None, query_tau=None):
            th = None if thresholds is None else [float(thresholds)]
            qt = None if query_tau is None else query_tau.numpy()
            return torch.from_numpy(host_angle_cdf(Cn, Qrep, lw, group_queries, thresholds=th, query_tau=qt, moments=False)["mass"].astype(np.float64))

        passes = max(1, math.ceil(math.log(math.pi / tol) / math.log(9.0) - 1e-12))
        return {k: v.numpy() for k, v in angles._quantile_search(cdf, G, m, list(levels), passes, torch.device("cpu")).items()}
    return quantile


def restatement_at_angles(Cn, Qr, lw, group_queries=False):
    """-> cdf64(theta [G,m]) -> (F64, U) [G,m] at tau = (float)(8 sin^2(theta / 2)), per query"""
    def cdf64(theta):
        tau = np.where(theta >= np.pi, np.float32(FLT_MAX), (8.0 * np.sin(0.5 * theta) ** 2).astype(np.float32))[:, None, :]
        ref = angle_cdf_fp64(Cn, Qr, tau.astype(np.float32), lw, group_queries)
        return ref["mass"][:, 0], ref["U"][:, 0]
    return cdf64


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_host_quantile_brackets_the_level(kind):
    Cn, Qr, lw = make_case(4097, 65, kind, True)
    out = check_quantile(host_quantile(Cn, Qr, lw), restatement_at_angles(Cn, Qr, lw))
    assert out["radius"].shape == (3, 2, 65) and (out["radius"][:, 1] >= out["radius"][:, 0]).all()
    assert (out["mass_lo"] < np.array([0.5, 0.9])[None, :, None]).all() and (out["mass_hi"] >= np.float32(0.5)).all()
    tight = check_quantile(host_quantile(Cn, Qr, lw), restatement_at_angles(Cn, Qr, lw), tol=1e-5)
    assert (np.abs(tight["radius"] - out["radius"]) <= 1e-3).all()
    parts = [host_quantile(Cn, Qr[i:i + 16], lw)((0.5, 0.9), 1e-3) for i in range(0, 65, 16)]      # tiling gives the same bits
    assert all(np.array_equal(np.concatenate([p[k] for p in parts], axis=2), out[k]) for k in out)


def test_host_quantile_is_zero_where_the_query_is_a_centre_that_heavy():
    Cn, Qr, _ = make_case(255, 8, "uniform", False)
    lw = np.zeros((1, 255), np.float32)
    lw[0, 17] = np.log(254.0 * 1.5)                                      # centre 17 carries 0.6 of the mass
    Qr = Qr.copy()
    Qr[3] = Cn[17]
    out = check_quantile(host_quantile(Cn, Qr, lw), restatement_at_angles(Cn, Qr, lw))
    assert out["radius"][0, 0, 3] == 0.0 and out["lo"][0, 0, 3] == 0.0 and abs(out["mass_hi"][0, 0, 3] - 0.6) <= 1e-6
    assert out["radius"][0, 1, 3] > 0.0 and (np.delete(out["radius"][0, 0], 3) > 0.0).all()


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20
_TH = (C.c_double * 8)(*np.deg2rad(THRESHOLDS_DEG))


def _args(**kw):
    base = dict(centres=_FAKE, queries=_FAKE * 2, log_weights=_FAKE, n=4608, m=1000, G=3, T=8, thresholds=C.addressof(_TH), mass=_FAKE,
                mean_angle=_FAKE, mean_sq_angle=_FAKE)
    base.update(kw)
    a = _lib.So3AngleCdf(**base)
    a.workspace, a.workspace_bytes = _FAKE, _lib.lib().rnf_so3_angle_cdf_workspace_bytes(C.byref(a))
    return a


def _refused(a, word):
    L = _lib.lib()
    assert L.rnf_so3_angle_cdf(C.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def test_c_abi_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.rnf_abi_version() == 8
    a = _args()
    assert a.workspace_bytes == (8 * 3 * 10 * 2 * 1000 + 16 * 3 * 2 + 8 * 3 + 4 * 3 * 4608 + 15) // 16 * 16      # the rule of include/rnf_hip.h
    assert a.workspace_bytes == _host_lib().hac_workspace_bytes(C.c_longlong(4608), C.c_longlong(1000), 3, 10)
    assert _args(mean_angle=None, mean_sq_angle=None).workspace_bytes == (8 * 3 * 8 * 2 * 1000 + 16 * 3 * 2 + 8 * 3 + 4 * 3 * 4608 + 15) // 16 * 16
    assert _args(mass=None, mean_sq_angle=None).workspace_bytes == (8 * 3 * 2 * 2 * 1000 + 16 * 3 * 2 + 8 * 3 + 4 * 3 * 4608 + 15) // 16 * 16
    for bad, word in ((dict(G=0), "G="), (dict(G=65536), "G="), (dict(n=0), "n="), (dict(n=(1 << 24) + 1), "n="), (dict(m=-1), "m="),
                      (dict(m=1 << 31), "m="), (dict(T=-1), "T="), (dict(T=9), "T=")):
        _refused(_args(**bad), word)
        assert L.rnf_so3_angle_cdf_workspace_bytes(C.byref(_lib.So3AngleCdf(**{**dict(n=10, m=10, G=1, T=1), **bad}))) == 0
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
    assert L.rnf_so3_angle_cdf_workspace_bytes(C.byref(a)) == 0
    assert L.rnf_so3_angle_cdf(C.byref(_args(m=0))) == 0                 # a no-op
    assert L.rnf_so3_angle_cdf(C.byref(_args(m=0, T=0, thresholds=None))) == 0
    assert L.rnf_so3_angle_cdf_workspace_bytes(C.byref(_args(m=0))) == (16 * 3 * 2 + 8 * 3 + 4 * 3 * 4608 + 15) // 16 * 16


def test_header_declares_the_struct_the_binding_mirrors():
    import re
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    body = header[header.index("typedef struct RnfSo3AngleCdf {") + 30:header.index("} RnfSo3AngleCdf;")]
    names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
    assert names == [f for f, _ in _lib.So3AngleCdf._fields_], names
    assert names[0] == "struct_bytes" and names[-3:] == ["workspace", "workspace_bytes", "stream"]
    assert {"rnf_so3_angle_cdf", "rnf_so3_angle_cdf_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "#define RNF_ABI_VERSION 8" in header
    assert "8 G S ceil(n / 4096) m + 16 G ceil(n / 4096) + 8 G + 4 G n rounded up to 16" in header
    device = open(os.path.join(root, "rotationnormflow_amd", "csrc", "so3_angle_cdf.h")).read()
    assert "bit-identical from run to run" in device and "bit-identical from run to run" in header[header.index("RnfSo3KernelMoments;"):]
    assert "no flags pass" in device and "ks::dist2" in device


def test_python_entry_points_validate_their_arguments():
    from rotationnormflow_amd import grid_pose, harness
    from rotationnormflow_amd.utils import angles
    R = torch.eye(3).expand(5, 3, 3).contiguous()
    with pytest.raises(ValueError, match="centres"):
        angles.so3_angle_cdf(R, R, [0.1])                                # on the CPU
    with pytest.raises(ValueError, match="centres"):
        angles.so3_angle_cdf(torch.zeros(5, 9), R, [0.1])
    with pytest.raises(ValueError, match="centres"):
        angles.so3_angle_quantile(R, R, [0.5])
    with pytest.raises(ValueError, match="GPU"):
        grid_pose.grid_error(torch.zeros(2, 72), torch.zeros(72, 3, 3), torch.zeros(2, 4, 3, 3))
    with pytest.raises(ValueError, match="est"):
        harness.grid_error(torch.zeros(2, 72), torch.zeros(72, 3, 3), torch.zeros(3, 4, 3, 3))
    with pytest.raises(ValueError, match="GPU"):
        harness.grid_ball_estimate(torch.zeros(2, 72), torch.zeros(72, 3, 3))
    with pytest.raises(ValueError, match="radius_deg"):
        harness.grid_ball_estimate(torch.zeros(2, 72), torch.zeros(72, 3, 3), radius_deg=200.0)
    with pytest.raises(ValueError, match="candidates"):
        harness.grid_ball_estimate(torch.zeros(2, 72), torch.zeros(72, 3, 3), candidates=0)
    with pytest.raises(ValueError, match="symmetric"):
        harness.grid_error(torch.zeros(2, 72), torch.zeros(72, 3, 3), torch.zeros(2, 4, 3, 3), gt=torch.zeros(2, 3, 3, 3))
    with pytest.raises(ValueError, match="level"):
        harness.grid_error(torch.zeros(2, 72), torch.zeros(72, 3, 3), torch.zeros(2, 4, 3, 3), levels=(1.0,))
    with pytest.raises(ValueError, match="thresholds_deg"):
        harness.grid_error(torch.zeros(2, 72), torch.zeros(72, 3, 3), torch.zeros(2, 4, 3, 3), thresholds_deg=(190.0,))
    assert harness.grid_pose_error is grid_pose.grid_pose_error and harness.grid_pose_ball_estimate is grid_pose.grid_pose_ball_estimate
    assert angles.MAX_THRESHOLDS == 8 and angles.SLOT_BYTES == 8


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_so3_angle_cdf.cpp (its own main: ragged sizes, -inf weights, NaN rows, T = 8 and T = 0, thresholds per query,
    queries per group) built with the host-side address and undefined-behaviour sanitizers (-Xarch_host: host code only, nothing for
    the GPU) and run as a process of its own."""
    exe = str(tmp_path / "sanitize_so3_angle_cdf")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_so3_angle_cdf.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)
