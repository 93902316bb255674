"""CPU: the moments of the pairwise matrix-Fisher kernel sum (csrc/so3_kernel_moments.h, rnf_so3_kernel_moments) and what is built on them.

``kernel_moments_fp64`` is the numpy fp64 restatement of the definition from the same fp32 inputs -- responsibilities r_ij by an
explicit softmax of the difference-form exponents, M_i = sum_j r_ij C_j, D_i = sum_j r_ij d2_ij, the polar factor by LAPACK's SVD --
and ``mean_shift_fp64`` iterates it; tests/test_gpu_so3_moments.py imports both, the cases and the gates.  Here the host build of the
header (the same arithmetic in the kernels' order) is held to them, l'(kappa) to the integral over the rotation angle, and the edge cases,
the C ABI's refusals, the workspace rule, the struct against its binding and the Python argument checks are exercised without a device.

The gates follow the derivation of the kernel sum's gate (tests/test_so3_kde_host.py): the exponent of pair (i, j) carries an absolute
error of at most eps_ij = 1e-6 E_ij + 4e-6 with E_ij = (kappa/2) d2_ij + |lw_j|, which is the relative error of its weight; the part
common to all j cancels in the normalisation, so the responsibilities move by at most 2 r_ij eps_ij and, the entries of a rotation
being at most 1 in size,
    |mean - ref| <= 2 sum_j r_ij eps_ij            (max over the nine entries),
    |msd - ref|  <= 2 sum_j r_ij eps_ij d2_ij + 1e-6 D_i   (the second term: d2 itself is an fp32 sum of nine squares),
    |log_density - ref| <= gate(E) as in tests/test_so3_kde_host.py,
    |dlogp_dkappa - ref| <= gate_msd / 2 + 1e-9 |l'(kappa)|."""
import ctypes as C
import functools
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch
from scipy import integrate

from rotationnormflow_amd import _lib
from tests.test_so3_kde_host import draw, gate, kernel_sum_fp64, log_normaliser, make_case, ptr, rodrigues  # noqa: F401  (re-exported for the GPU tests)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_so3_kernel_moments.cpp")
OUT = os.path.join(HERE, "csrc", "_host_so3_kernel_moments.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f)
        for f in ("so3_kernel_moments.h", "so3_kernel_sum.h", "so3_math.h", "fisher_exact.h", "fisher_math.h")]
KAPPAS_HOST = (0.0, 4.0, 64.0, 16384.0)
OUTPUTS = ("log_density", "mean", "msd", "rotation", "step")
ORTH = 16 * 2.0 ** -23                                                   # polar3 returns a rotation to this, or NaN (csrc/so3_math.h)


def _host_lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    h = C.CDLL(OUT)
    h.hkm_workspace_bytes.restype = C.c_ulonglong
    return h


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def dlog_normaliser_quad(kappa):
    """l'(kappa) = -E[d2] / 2 = -4 int exp(-4 kappa s^2) s^4 dt / int exp(-4 kappa s^2) s^2 dt over the rotation angle t, s = sin(t/2):
    two positive integrands, split as the normaliser test of tests/test_so3_kde_host.py splits its one"""
    cut = min(np.pi, 12.0 / np.sqrt(max(kappa, 1.0)))
    val = []
    for p in (4, 2):
        f = lambda t: np.exp(-4.0 * kappa * np.sin(0.5 * t) ** 2) * np.sin(0.5 * t) ** p     # noqa: E731
        v = integrate.quad(f, 0.0, cut, epsabs=0.0, epsrel=1e-13, limit=400)[0]
        if cut < np.pi:                                                  # below exp(-144) of the first part: its own accuracy is moot
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", integrate.IntegrationWarning)
                v += integrate.quad(f, cut, np.pi, epsabs=0.0, epsrel=1e-13, limit=400)[0]
        val.append(v)
    return -4.0 * val[0] / val[1]


def polar_fp64(M):
    """The rotation closest to each M [..,3,3] (U V^T of the SVD) where det M > 0, else NaN"""
    M = np.asarray(M, np.float64)
    out = np.full(M.shape, np.nan)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(M).all(axis=(-2, -1)) & (np.linalg.det(np.where(np.isfinite(M), M, 0.0)) > 0.0)
    if ok.any():
        U, _, Vt = np.linalg.svd(M[ok])
        out[ok] = U @ Vt
    return out


def kernel_moments_fp64(centres, queries, kappa, log_weights=None, group_queries=False):
    """The outputs of rnf_so3_kernel_moments in fp64 from the fp32 inputs, with the edge cases of include/rnf_hip.h -> dict of
    log_density [G,m], mean [G,m,3,3], msd [G,m], rotation [G,m,3,3], step [G,m], dlogp_dkappa [G,m] and the gates E, gate_mean,
    gate_msd [G,m] of this file's docstring.  ``kappa`` may be a tuple: then a list of such dicts, from one set of distances.
    With eps_ij = 1e-6 ((kappa/2) d2_ij + |lw_j|) + 4e-6 the gates' sums are sum_j r_ij eps_ij = 1e-6 ((kappa/2) D_i + sum_j r_ij |lw_j|)
    + 4e-6 and sum_j r_ij eps_ij d2_ij = 1e-6 ((kappa/2) sum_j r_ij d2_ij^2 + sum_j r_ij d2_ij |lw_j|) + 4e-6 D_i."""
    kappas = tuple(kappa) if isinstance(kappa, (tuple, list)) else (kappa,)
    Cn = np.asarray(centres, np.float32).reshape(-1, 9).astype(np.float64)
    n = len(Cn)
    lw = None if log_weights is None else np.asarray(log_weights, np.float32).reshape(-1, n).astype(np.float64)
    Qa = np.asarray(queries, np.float32).astype(np.float64)
    Qa = Qa.reshape(-1, Qa.shape[-3], 9) if group_queries else Qa.reshape(1, -1, 9)
    G = len(Qa) if group_queries else (1 if lw is None else len(lw))
    m = Qa.shape[1]
    if lw is None:
        lw = np.zeros((G, n))
    out = []
    for _ in kappas:
        res = {k: np.full((G, m) + ((3, 3) if k in ("mean", "rotation") else ()), np.nan) for k in OUTPUTS + ("dlogp_dkappa",)}
        res.update({k: np.zeros((G, m)) for k in ("E", "gate_mean", "gate_msd")})
        out.append(res)
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
            lwl = np.where(live, lw[g], 0.0)
            mx = lw[g][live].max()
            log_z = mx + np.log(np.exp(lw[g][live] - mx).sum())
            Cl = np.where(live[:, None], Cn, 0.0)
            for kap, res in zip(kappas, out):
                t = lw[g][None, :] - 0.5 * kap * d2                      # -inf where the centre is left out
                at = t.argmax(axis=1)
                top = t[np.arange(m), at]
                r = np.exp(t - top[:, None])
                S = r.sum(axis=1)
                r /= S[:, None]
                rd = r * d2
                msd, msd2 = rd.sum(axis=1), (rd * d2).sum(axis=1)
                eps1 = 1e-6 * (0.5 * kap * msd + r @ np.abs(lwl)) + 4e-6
                eps2 = 1e-6 * (0.5 * kap * msd2 + rd @ np.abs(lwl)) + 4e-6 * msd
                mean = (r @ Cl).reshape(m, 3, 3)
                lp = top + np.log(S) - log_z - float(log_normaliser(kap))
                mean[~q_ok], msd[~q_ok], lp[~q_ok] = np.nan, np.nan, np.nan
                rot = polar_fp64(mean)
                res["log_density"][g], res["E"][g] = lp, np.where(q_ok, 0.5 * kap * d2[np.arange(m), at] + np.abs(lwl[at]), 0.0)
                res["gate_mean"][g], res["gate_msd"][g] = 2.0 * eps1, 2.0 * eps2 + 1e-6 * np.nan_to_num(msd)
                res["mean"][g], res["msd"][g], res["rotation"][g] = mean, msd, rot
                res["step"][g] = np.sqrt(((rot - Qr.reshape(m, 3, 3)) ** 2).sum(axis=(1, 2)))
                res["dlogp_dkappa"][g] = -0.5 * msd - dlog_normaliser_quad(kap)
    return out if isinstance(kappa, (tuple, list)) else out[0]


def mean_shift_fp64(centres, starts, kappa, tol=1e-6, max_steps=200):
    """R <- polar(M(R)) in fp64 until every step |polar(M) - R|_F is below ``tol`` -> (endpoints [s,3,3], steps taken, the smallest det M
    met on the way)"""
    cur = np.asarray(starts, np.float64).copy()
    Cn = np.asarray(centres, np.float64).reshape(-1, 9)
    min_det = np.inf
    for it in range(max_steps):
        diff = cur.reshape(-1, 1, 9) - Cn[None]
        t = -0.5 * kappa * np.einsum("ijk,ijk->ij", diff, diff)
        r = np.exp(t - t.max(axis=1, keepdims=True))
        M = ((r / r.sum(axis=1, keepdims=True)) @ Cn).reshape(-1, 3, 3)
        min_det = min(min_det, float(np.linalg.det(M).min()))
        new = polar_fp64(M)
        step = np.sqrt(((new - cur) ** 2).sum(axis=(1, 2)))
        cur = new
        if (step < tol).all():
            return cur, it + 1, min_det
    return cur, max_steps, min_det


def angle_deg(A, B):
    """The angle between rotations [..,3,3], in degrees (fp64)"""
    tr = np.einsum("...ij,...ij->...", np.asarray(A, np.float64), np.asarray(B, np.float64))
    return np.degrees(np.arccos(np.clip(0.5 * (tr - 1.0), -1.0, 1.0)))


def host_kernel_moments(centres, queries, kappa, log_weights=None, group_queries=False, project=True):
    """The host build of the kernels' arithmetic -> dict of float32 arrays with a leading G, and dlogp_dkappa (fp64)"""
    h = _host_lib()
    Cn = np.ascontiguousarray(centres, np.float32).reshape(-1, 9)
    n = len(Cn)
    Qr = np.ascontiguousarray(queries, np.float32)
    lw = None if log_weights is None else np.ascontiguousarray(log_weights, np.float32).reshape(-1, n)
    G = Qr.shape[0] if group_queries else (1 if lw is None else len(lw))
    m = Qr.shape[-3]
    out = {k: np.full((G, m) + ((3, 3) if k in ("mean", "rotation") else ()), 7.0, np.float32) for k in OUTPUTS if project or k not in ("rotation", "step")}
    h.hkm_kernel_moments(ptr(Cn), ptr(Qr), ptr(lw), C.c_longlong(n), C.c_longlong(m), G, C.c_double(kappa), int(group_queries),
                         *[ptr(out.get(k)) for k in OUTPUTS])
    dl = np.empty(1)
    h.hkm_dlog_normaliser(ptr(np.array([float(kappa)])), 1, ptr(dl))
    out["dlogp_dkappa"] = -0.5 * out["msd"].astype(np.float64) - dl[0]
    return out


def host_kernel_sum1(centres, queries, kappa, log_weights=None):
    h = _host_lib()
    Cn = np.ascontiguousarray(centres, np.float32).reshape(-1, 9)
    Qr = np.ascontiguousarray(queries, np.float32).reshape(-1, 9)
    lw = None if log_weights is None else np.ascontiguousarray(log_weights, np.float32).reshape(-1, len(Cn))
    out = np.empty((1 if lw is None else len(lw), len(Qr)), np.float32)
    h.hkm_kernel_sum(ptr(Cn), ptr(Qr), ptr(lw), C.c_longlong(len(Cn)), C.c_longlong(len(Qr)), len(out), C.c_double(kappa), ptr(out))
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

def group_sets(Qr, G):
    """One set of queries per group from one set: group g takes it rolled by 7 g rows"""
    return np.stack([np.roll(Qr, 7 * g, axis=0) for g in range(G)])


@functools.lru_cache(maxsize=4)
def references(n, m, kind, weighted, kappas, group_queries):
    """(case, {kappa: restatement}): computed once per case from one set of distances, and left unchanged"""
    Cn, Qr, lw = make_case(n, m, kind, weighted)
    if group_queries:
        Qr = group_sets(Qr, 3 if weighted else 1)
    refs = kernel_moments_fp64(Cn, Qr, tuple(kappas), lw, group_queries)
    for ref in refs:
        for a in ref.values():
            a.setflags(write=False)
    for a in (Cn, Qr, lw):
        if a is not None:
            a.setflags(write=False)
    return (Cn, Qr, lw), dict(zip(kappas, refs))


WORST = {}                                                               # the largest fraction of each gate seen, per caller


def check_case(fn, n, m, kind, weighted, kappa, group_queries, who="host", kappas=KAPPAS_HOST):
    """``fn(centres, queries, kappa, log_weights, group_queries, project)`` against the restatement on the gates; ``kappas``: the list
    ``kappa`` is one of (their restatements are computed together)"""
    (Cn, Qr, lw), refs = references(n, m, kind, weighted, tuple(kappas), group_queries)
    ref = refs[kappa]
    got = {k: np.asarray(v, np.float64) for k, v in fn(Cn, Qr, kappa, lw, group_queries, True).items()}
    for k in OUTPUTS:
        assert got[k].shape == ref[k].shape, k
    assert all(np.isfinite(got[k]).all() and np.isfinite(ref[k]).all() for k in ("log_density", "mean", "msd", "dlogp_dkappa"))
    dl = abs(dlog_normaliser_quad(kappa))
    frac = dict(log_density=np.abs(got["log_density"] - ref["log_density"]) / gate(ref["E"]),
                mean=np.abs(got["mean"] - ref["mean"]).max(axis=(2, 3)) / ref["gate_mean"],
                msd=np.abs(got["msd"] - ref["msd"]) / ref["gate_msd"],
                dlogp_dkappa=np.abs(got["dlogp_dkappa"] - ref["dlogp_dkappa"]) / (0.5 * ref["gate_msd"] + 1e-9 * dl))
    print("n %d m %d %s weighted %d kappa %g per-group %d: worst fraction of the gate %s" % (
        n, m, kind, weighted, kappa, group_queries, ", ".join("%s %.3f" % (k, v.max()) for k, v in frac.items())))
    for k, v in frac.items():
        WORST[who, k] = max(WORST.get((who, k), 0.0), float(v.max()))
        assert (v <= 1.0).all(), k
    # the projection: a rotation to polar3's own tolerance wherever the mean has a direction, NaN elsewhere; the step is its distance
    has = np.isfinite(ref["rotation"]).all(axis=(2, 3))
    R = got["rotation"]
    fin = np.isfinite(R).all(axis=(2, 3))
    assert not (fin & ~has).any() and np.array_equal(np.isnan(got["step"]), ~fin)
    assert (np.abs(np.swapaxes(R[fin], 1, 2) @ R[fin] - np.eye(3)) <= 2 * ORTH).all() and (np.linalg.det(R[fin]) > 0).all()
    Qg = np.broadcast_to(np.asarray(Qr, np.float64).reshape((-1, m, 3, 3)), R.shape)
    dist = np.sqrt(((R - Qg) ** 2).sum(axis=(2, 3)))
    assert (np.abs(got["step"] - dist)[fin] <= 2e-7 + 1e-6 * dist[fin]).all()
    # where the restatement's mean is well conditioned (smallest singular value >= 0.1) polar3 must have converged, and a perturbation dM
    # moves the polar factor by at most 2 |dM|_F / (s2 + s3) (Li 1995) <= 3 * 2 gate_mean / 0.2, plus polar3's own 16 * 2^-23
    well = has & (np.linalg.svd(np.where(has[..., None, None], ref["mean"], np.eye(3)), compute_uv=False)[..., 2] >= 0.1)
    assert fin[well].all()
    assert (np.abs(R - ref["rotation"]).max(axis=(2, 3))[well] <= 30.0 * ref["gate_mean"][well] + ORTH).all()


def check_edge_cases(fn):
    """The edge cases of tests/test_so3_kde_host.py check_edge_cases, for every output of the (group, query)"""
    n, m = 130, 70
    Cn, Qr, lw = make_case(n, m, "uniform", True)

    def nan_rows(got, g):
        return all(np.isnan(got[k][g]).all() for k in OUTPUTS)

    def fin_rows(got, g, but_rotation=False):
        return all(np.isfinite(got[k][g]).all() for k in (OUTPUTS[:3] if but_rotation else OUTPUTS))

    dead = lw[1] == -np.inf
    bad = Cn.copy()
    bad[dead, 1, 1] = np.nan                                             # NaN entries where group 1 has no weight: groups 0 and 2 hold them
    bad[np.flatnonzero(dead)[0]] = np.inf
    got = fn(bad, Qr, 64.0, lw, False, True)
    ref = kernel_moments_fp64(bad, Qr, 64.0, lw)
    clean = fn(Cn, Qr, 64.0, lw, False, True)
    assert nan_rows(got, 0) and nan_rows(got, 2) and fin_rows(got, 1, True)
    assert (np.abs(got["mean"][1] - ref["mean"][1]).max(axis=(1, 2)) <= ref["gate_mean"][1]).all()
    assert all(np.array_equal(got[k][1], clean[k][1], equal_nan=True) for k in OUTPUTS)      # left out whatever its entries
    lwn = lw.copy()
    lwn[2, 129] = np.nan
    got = fn(Cn, Qr, 64.0, lwn, False, True)
    assert nan_rows(got, 2) and fin_rows(got, 0, True) and fin_rows(got, 1, True)
    lwd = lw.copy()
    lwd[0] = -np.inf
    got = fn(Cn, Qr, 64.0, lwd, False, True)
    assert nan_rows(got, 0) and fin_rows(got, 1, True) and fin_rows(got, 2, True)
    Qb = Qr.copy()
    Qb[3, 0, 2], Qb[69, 2, 2] = np.inf, np.nan
    got = fn(Cn, Qb, 64.0, None, False, True)
    for k in OUTPUTS:
        assert np.isnan(got[k][0][[3, 69]]).all(), k
    assert all(np.isfinite(np.delete(got[k][0], [3, 69], axis=0)).all() for k in OUTPUTS[:3])
    # kappa = 0: mean = sum_j w_j C_j for every query, the density uniform
    got = fn(Cn, Qr, 0.0, lw, False, True)
    w = np.exp(lw.astype(np.float64) - lw.astype(np.float64).max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    want = (w @ Cn.reshape(n, 9).astype(np.float64)).reshape(3, 1, 3, 3)
    assert (np.abs(got["mean"] - want).max(axis=(2, 3)) <= 2 * (w * (1e-6 * np.abs(np.where(np.isfinite(lw), lw, 0.0)) + 4e-6)).sum(axis=1)[:, None]).all()
    assert np.abs(got["log_density"]).max() <= 4e-6
    # three half-turns about orthogonal axes average to -I / 3: no mean direction
    half = np.stack([np.diag(d) for d in ([1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0])]).astype(np.float32)
    got = fn(half, np.eye(3, dtype=np.float32)[None], 0.0, None, False, True)
    assert np.abs(got["mean"][0, 0] + np.eye(3) / 3.0).max() <= 1e-7 and np.isfinite(got["log_density"]).all()
    assert np.isnan(got["rotation"]).all() and np.isnan(got["step"]).all() and abs(got["msd"][0, 0] - 8.0) <= 1e-6
    # one centre: mean = C, rotation = polar3(C) within 4 * 2^-23 of C, msd = d2
    one, q = draw("uniform", 1, 21), draw("uniform", 5, 22)
    got = fn(one, q, 64.0, None, False, True)
    d2 = ((q.astype(np.float64) - one.astype(np.float64)) ** 2).sum(axis=(1, 2))
    assert np.array_equal(got["mean"][0], np.broadcast_to(one, (5, 3, 3))) and (np.abs(got["rotation"][0] - one).max() <= 4 * 2.0 ** -23)
    assert (np.abs(got["msd"][0] - d2) <= 1e-6 * d2).all() and (np.abs(got["step"][0] - np.sqrt(d2)) <= 2e-6).all()
    got = fn(one, q, 64.0, None, False, False)                           # without the projection: three outputs
    assert "rotation" not in got and "step" not in got and np.array_equal(got["mean"][0], np.broadcast_to(one, (5, 3, 3)))


# ---- tests -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kappa", [0.0, 0.5, 3.0, 50.0, 1e3, 1e4])
def test_normaliser_derivative_is_the_mean_squared_distance_over_the_rotation_angle(kappa):
    h = _host_lib()
    dl = np.empty(1)
    h.hkm_dlog_normaliser(ptr(np.array([kappa])), 1, ptr(dl))
    want = dlog_normaliser_quad(kappa)
    print("kappa %g: l' %.15g, integral %.15g, relative difference %.2e" % (kappa, dl[0], want, abs(dl[0] - want) / abs(want)))
    assert abs(dl[0] - want) <= 1e-9 * abs(want)
    if kappa == 0.0:
        assert dl[0] == -3.0


def test_normaliser_derivative_is_continuous_where_its_two_forms_meet():
    h = _host_lib()
    k = np.array([16.0 * (1 - 2.0 ** -40), 16.0, 1e5, 1e6])
    dl = np.empty(4)
    h.hkm_dlog_normaliser(ptr(k), 4, ptr(dl))
    assert abs(dl[0] - dl[1]) <= 1e-12 * abs(dl[1])
    for kappa, got in zip(k[2:], dl[2:]):                                # -3 / (2 kappa) (1 + 1 / (8 kappa) + ..): the series' first terms
        assert abs(got - dlog_normaliser_quad(kappa)) <= 1e-9 * abs(got) and abs(got + 1.5 / kappa * (1 + 0.125 / kappa)) <= 2.0 / kappa ** 3


@pytest.mark.parametrize("n,m", [(1, 1), (63, 65), (65, 65), (4097, 65)])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("weighted", [False, True])
def test_host_build_against_the_restatement(n, m, kind, weighted):
    for group_queries in (False, True):
        for kappa in KAPPAS_HOST:
            check_case(host_kernel_moments, n, m, kind, weighted, kappa, group_queries)
    print("worst fractions so far:", {k[1]: round(v, 4) for k, v in WORST.items() if k[0] == "host"})


@pytest.mark.parametrize("weighted", [False, True])
def test_host_log_density_is_the_kernel_sums_bit_for_bit(weighted):
    Cn, Qr, lw = make_case(4097, 65, "clustered", weighted)
    for kappa in KAPPAS_HOST:
        assert np.array_equal(host_kernel_moments(Cn, Qr, kappa, lw)["log_density"], host_kernel_sum1(Cn, Qr, kappa, lw))


def test_host_result_does_not_depend_on_the_batch():
    Cn, Qr, lw = make_case(4097, 300, "clustered", True)
    whole = host_kernel_moments(Cn, Qr, 64.0, lw)
    head = host_kernel_moments(Cn, Qr[:200], 64.0, lw)                   # later queries dropped
    tail = host_kernel_moments(Cn, Qr, 64.0, lw[2:])                     # earlier groups dropped
    per = host_kernel_moments(Cn, np.stack([Qr] * 3), 64.0, lw, True)    # the same queries passed per group
    for k in OUTPUTS:
        assert np.array_equal(whole[k][:, :200], head[k], equal_nan=True), k
        assert np.array_equal(whole[k][2:], tail[k], equal_nan=True), k
        assert np.array_equal(whole[k], per[k], equal_nan=True), k
    rolled = host_kernel_moments(Cn, group_sets(Qr, 3), 64.0, lw, True)
    for g in range(3):
        assert np.array_equal(np.roll(whole["mean"][g], 7 * g, axis=0), rolled["mean"][g]), g


def test_restatement_restates_the_kernel_sums_log_density():
    Cn, Qr, lw = make_case(130, 70, "clustered", True)
    for kappa, ref in zip((0.0, 64.0), kernel_moments_fp64(Cn, Qr, (0.0, 64.0), lw)):
        want, E = kernel_sum_fp64(Cn, Qr, (kappa,), lw)
        assert np.abs(ref["log_density"] - want[:, 0]).max() <= 1e-12 and np.allclose(ref["E"], E[:, 0], rtol=1e-12, atol=0)


def test_host_edge_cases():
    check_edge_cases(host_kernel_moments)


@pytest.mark.parametrize("kappa", [4.0, 64.0])
def test_gradient_identity_on_the_restatement(kappa):
    """kappa (M - Q) is the gradient of the difference-form log-sum-exp: torch fp64 autograd, to 1e-10.  Pins the formula, not the kernel."""
    Cn, Qr, lw = make_case(65, 33, "clustered", True)
    ref = kernel_moments_fp64(Cn, Qr, kappa, lw)
    Ct, lwt = torch.tensor(Cn, dtype=torch.float64).reshape(-1, 9), torch.tensor(lw, dtype=torch.float64)
    for g in range(3):
        Q = torch.tensor(Qr, dtype=torch.float64).reshape(-1, 9).requires_grad_(True)
        lp = torch.logsumexp(lwt[g][None, :] - 0.5 * kappa * ((Q[:, None, :] - Ct[None]) ** 2).sum(dim=2), dim=1)
        (grad,) = torch.autograd.grad(lp.sum(), Q)
        want = kappa * (ref["mean"][g] - Qr.astype(np.float64))
        assert np.abs(grad.numpy().reshape(-1, 3, 3) - want).max() <= 1e-10
        assert np.abs(lp.detach().numpy() - float(torch.logsumexp(lwt[g], 0)) - (ref["log_density"][g] - float(
            kernel_sum_fp64(Cn[:1], Cn[:1], (kappa,))[0][0, 0, 0]))).max() <= 1e-9      # and the value: the same sum, up to -l(kappa)


@functools.lru_cache(maxsize=1)
def two_mode_reference():
    """(the two-mode set, its first 256 rotations' mean-shift endpoints at kappa = 32 in fp64, steps, min det M): shared with the GPU tests"""
    from tests.test_gpu_so3_kde import two_mode_samples
    train = two_mode_samples(4096, 11)
    ends, steps, min_det = mean_shift_fp64(train, train[:256], 32.0)
    train.setflags(write=False)
    ends.setflags(write=False)
    return train, ends, steps, min_det


TWO_MODES = np.stack([np.eye(3), np.diag([-1.0, -1.0, 1.0])])


def cluster(ends, separation_deg=15.0):
    """Greedy clusters of endpoints: the first endpoint opens one, an endpoint further than the separation from every centre another ->
    (centres [k,3,3], the label of each endpoint)"""
    centres, label = [], np.empty(len(ends), int)
    for i, R in enumerate(ends):
        a = [float(angle_deg(R, c)) for c in centres]
        if not a or min(a) > separation_deg:
            centres.append(R)
            a.append(0.0)
        label[i] = int(np.argmin(a))
    return np.stack(centres), label


def test_mean_shift_on_the_restatement_finds_the_two_modes():
    train, ends, steps, min_det = two_mode_reference()
    centres, label = cluster(ends)
    off = [float(angle_deg(centres, M).min()) for M in TWO_MODES]
    print("fp64 mean shift, kappa 32: %d steps, %d clusters, %.3f and %.3f degrees from the modes, min det M %.3f, shares %s" % (
        steps, len(centres), off[0], off[1], min_det, np.bincount(label) / len(label)))
    assert steps <= 32 and len(centres) == 2 and max(off) <= 2.0 and min_det > 0.5
    assert (angle_deg(ends, centres[label]) <= 0.01).all()               # each cluster is one point


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20


def _args(**kw):
    base = dict(centres=_FAKE, queries=_FAKE * 2, log_weights=_FAKE, n=4608, m=1000, G=3, kappa=64.0, log_density=_FAKE, mean=_FAKE,
                msd=_FAKE, rotation=_FAKE, step=_FAKE)
    base.update(kw)
    a = _lib.So3KernelMoments(**base)
    a.workspace, a.workspace_bytes = _FAKE, _lib.lib().rnf_so3_kernel_moments_workspace_bytes(C.byref(a))
    return a


def _refused(a, word):
    L = _lib.lib()
    assert L.rnf_so3_kernel_moments(C.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def test_c_abi_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.rnf_abi_version() == 8
    a = _args()
    assert a.workspace_bytes == (92 * 3 * 2 * 1000 + 16 * 3 * 2 + 8 * 3 + 4 * 2 + 15) // 16 * 16             # the rule of include/rnf_hip.h
    assert a.workspace_bytes == _host_lib().hkm_workspace_bytes(C.c_longlong(4608), C.c_longlong(1000), 3)
    for bad, word in ((dict(G=0), "G="), (dict(G=65536), "G="), (dict(n=0), "n="), (dict(n=(1 << 24) + 1), "n="), (dict(m=-1), "m="),
                      (dict(m=1 << 31), "m=")):
        _refused(_args(**bad), word)
        assert L.rnf_so3_kernel_moments_workspace_bytes(C.byref(_lib.So3KernelMoments(**{**dict(n=10, m=10, G=1), **bad}))) == 0
    for k in (-1.0, 1.0000001e6, float("nan"), float("inf")):
        _refused(_args(kappa=k), "kappa")
    _refused(_args(centres=_FAKE + 4), "aligned")
    _refused(_args(queries=_FAKE + 8), "aligned")
    _refused(_args(rotation=None), "step requires rotation")
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
    assert L.rnf_so3_kernel_moments_workspace_bytes(C.byref(a)) == 0
    dl = C.c_double(0.0)
    assert L.rnf_so3_kernel_moments(C.byref(_args(m=0, kappa=0.0, dlog_normaliser=C.addressof(dl)))) == 0 and dl.value == -3.0      # a no-op
    assert L.rnf_so3_kernel_moments_workspace_bytes(C.byref(_args(m=0))) == (16 * 3 * 2 + 8 * 3 + 4 * 2 + 15) // 16 * 16


def test_header_declares_the_struct_the_binding_mirrors():
    import re
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    body = header[header.index("typedef struct RnfSo3KernelMoments {") + 35:header.index("} RnfSo3KernelMoments;")]
    names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
    assert names == [f for f, _ in _lib.So3KernelMoments._fields_], names
    assert {"rnf_so3_kernel_moments", "rnf_so3_kernel_moments_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "#define RNF_ABI_VERSION 8" in header
    assert "92 G ceil(n / 4096) m + 16 G ceil(n / 4096) + 8 G + 4 ceil(n / 4096) rounded up to 16" in header
    device = open(os.path.join(root, "rotationnormflow_amd", "csrc", "so3_kernel_moments.h")).read()
    assert "bit-identical from run to run" in device and "bit-identical from run to run" in header[header.index("RnfSo3KernelSum;"):]


def test_python_entry_points_validate_their_arguments():
    from rotationnormflow_amd import grid_pose, harness
    from rotationnormflow_amd.utils import kde
    R = torch.eye(3).expand(5, 3, 3).contiguous()
    with pytest.raises(ValueError, match="centres"):
        kde.so3_kernel_moments(R, R, 4.0)                                # on the CPU
    with pytest.raises(ValueError, match="centres"):
        kde.so3_kernel_moments(torch.zeros(5, 9), R, 4.0)
    with pytest.raises(ValueError, match="rotations"):
        harness.kde_modes(R, 4.0)
    with pytest.raises(ValueError, match="kappa=2000000"):
        kde.so3_kernel_moments(R, R, 2e6)
    with pytest.raises(ValueError, match="one concentration"):
        kde.so3_kernel_moments(R, R, [4.0, 8.0])
    with pytest.raises(ValueError, match="GPU"):
        grid_pose.grid_modes_refine(torch.zeros(2, 72), torch.zeros(72, 3, 3), torch.zeros(2, 4, 3, 3))
    with pytest.raises(ValueError, match="est"):
        harness.grid_modes_refine(torch.zeros(2, 72), torch.zeros(72, 3, 3), torch.zeros(3, 4, 3, 3))
    assert harness.grid_pose_modes_refined is grid_pose.grid_pose_modes_refined and kde.MOMENT_BYTES == 92
    for name in ("score", "mean_shift", "modes", "sample"):
        assert callable(getattr(kde.SO3KernelDensity, name))
    assert "no gradient" not in kde.SO3KernelDensity.__doc__.lower() and "no ``sample" not in kde.SO3KernelDensity.__doc__


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_so3_kernel_moments.cpp (its own main: ragged sizes, -inf weights, NaN rows, the det <= 0 case, queries per
    group) built with the host-side address and undefined-behaviour sanitizers (-Xarch_host: host code only, nothing for the GPU) and
    run as a process of its own."""
    exe = str(tmp_path / "sanitize_so3_kernel_moments")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_so3_kernel_moments.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)
