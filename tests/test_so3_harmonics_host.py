"""CPU: harmonic analysis on SO(3) (csrc/so3_harmonics.h: rnf_so3_wigner, rnf_so3_fourier, rnf_so3_fourier_eval) and
utils/harmonics.py.

The fp64 restatement, which tests/test_gpu_so3_harmonics.py imports with the cases and the gates:
  ``wigner_slow``    D^l(R) from its definition Y_l(R x) = D^l(R) Y_l(x): scipy's sph_harm_y at 400 points and least squares.
  ``wigner_fp64``    the bulk route: Wigner's closed-form SUM over k for the complex matrix in the Cayley-Klein pair of the fp64
                     quaternion (a polynomial with factorial weights, no recurrence in l: not the kernel's route), accumulated in
                     extended precision, and the fixed change of basis to the real harmonics.  Held to the slow one at 1e-12.
  ``fourier_fp64``   F_g^l = sum_j w_gj D^l(C_j) with an explicit softmax and the edge cases of include/rnf_hip.h.
  ``density_fp64``   f_gi = sum c_g . D(Q_i).
  ``character_density``  sum_j w_j sum_l (2l+1) h_l chi_l(theta_ij), chi_l = 1 + 2 sum_{k<=l} cos(k theta): the basis-free oracle.
Every route starts from the fp32 rows projected to the nearest rotation in fp64 (polar factor).

The gates.  Entries of D are at most 1 in size and come from a recurrence of l - l0 steps on powers of up to 2l factors:
  matrices   |D - ref| <= C_ENTRY (l + 1) 2^-23 per entry; on the kernel's output alone |D D^T - I| and |D(R1) D(R2) - D(R1 R2)|
             <= C_ENTRY (l + 1)(2l + 1) 2^-23 per entry, and D^1 is the permuted row to 2^-23.
  analysis   |F - ref| <= C_ENTRY (l + 1) 2^-23 per coefficient: the weights sum to 1.
  synthesis  |f - ref| <= K_SYNTH (L + 1) 2^-23 S + 2^-23 |ref|, S the l1 norm of the coefficients handed to the synthesis.
C_ENTRY and K_SYNTH are four times the worst ratio measured on the host build on the cases of this file (the margin covers the
device's contracted fmas): 0.794 (l + 1) 2^-23 on the 200 rows of the matrices test, so C_ENTRY = 3.2; 0.0095 (L + 1) 2^-23 S at the
chunk boundary (0.0032 on the synthesis cases), so K_SYNTH = 0.038.  The worst fractions of the gates on the host build are therefore
0.248 (matrices), 0.130 (analysis), 0.083 (synthesis), 0.246 (chunk boundary), 0.072 / 0.059 (orthogonality / product); D^1 is
within 0.25 of 2^-23 of the permuted row.
The MI355X's figures are in tests/test_gpu_so3_harmonics.py; DESIGN.md 3.3i has both."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy.special import ive, sph_harm_y

from rotationnormflow_amd import _lib
from rotationnormflow_amd.utils import harmonics

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_so3_harmonics.cpp")
OUT = os.path.join(HERE, "csrc", "_host_so3_harmonics.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f)
        for f in ("so3_harmonics.h", "so3_angle_cdf.h", "so3_kernel_sum.h", "fisher_exact.h", "fisher_math.h")]
EPS = 2.0 ** -23
C_ENTRY = 3.2
K_SYNTH = 0.038
LMAX = 16


def _host_lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    h = C.CDLL(OUT)
    h.hsh_fourier_workspace_bytes.restype = C.c_ulonglong
    h.hsh_records_bytes.restype = C.c_ulonglong
    return h


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def count(L):
    return (L + 1) * (2 * L + 1) * (2 * L + 3) // 3


def offset(l):
    return l * (4 * l * l - 1) // 3


def block(v, l):
    """degree l of coefficient vectors [..,C_L] as [..,2l+1,2l+1]"""
    return v[..., offset(l):offset(l + 1)].reshape(v.shape[:-1] + (2 * l + 1, 2 * l + 1))


def degree_of_entry(L):
    """[C_L] the degree of each entry"""
    return np.concatenate([np.full((2 * l + 1) ** 2, l) for l in range(L + 1)])


# ---- the host build ----------------------------------------------------------------------------------------------------------------------

def host_wigner(R, L):
    R = np.ascontiguousarray(R, np.float32).reshape(-1, 9)
    out = np.empty((len(R), count(L)), np.float32)
    _host_lib().hsh_wigner(ptr(R), C.c_longlong(len(R)), L, ptr(out))
    return out


def host_fourier(Cn, L, lw=None):
    Cn = np.ascontiguousarray(Cn, np.float32).reshape(-1, 9)
    lw = None if lw is None else np.ascontiguousarray(lw, np.float32).reshape(-1, len(Cn))
    G = 1 if lw is None else len(lw)
    out = np.empty((G, count(L)), np.float32)
    _host_lib().hsh_fourier(ptr(Cn), ptr(lw), C.c_longlong(len(Cn)), G, L, ptr(out))
    return out


def host_density(coeffs, Q, L, group_queries=False):
    coeffs = np.ascontiguousarray(coeffs, np.float32).reshape(-1, count(L))
    Q = np.ascontiguousarray(Q, np.float32)
    m = Q.shape[-3]
    out = np.empty((len(coeffs), m), np.float32)
    _host_lib().hsh_fourier_eval(ptr(coeffs), ptr(Q), C.c_longlong(m), len(coeffs), int(group_queries), L, ptr(out))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def project(R32):
    """fp32 rows [..,3,3] -> the nearest rotations in fp64 (the polar factor); rows that are not finite come back as NaN"""
    R = np.asarray(R32, np.float32).astype(np.float64).reshape(-1, 3, 3)
    ok = np.isfinite(R).all(axis=(1, 2))
    U, _, Vt = np.linalg.svd(np.where(ok[:, None, None], R, np.eye(3)))
    d = np.sign(np.linalg.det(U @ Vt))
    U[:, :, 2] *= d[:, None]
    P = U @ Vt
    P[~ok] = np.nan
    return P


def quaternions(R):
    """fp64 rotations [n,3,3] -> unit quaternions (w, x, y, z) [n,4], by the largest of the four candidates"""
    m = R
    t = np.stack([1 + m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2], 1 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2],
                  1 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2], 1 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]], axis=1)
    a, b, c = m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]
    p, q, r = m[:, 0, 1] + m[:, 1, 0], m[:, 0, 2] + m[:, 2, 0], m[:, 1, 2] + m[:, 2, 1]
    cand = np.stack([np.stack([t[:, 0], a, b, c], 1), np.stack([a, t[:, 1], p, q], 1), np.stack([b, p, t[:, 2], r], 1),
                     np.stack([c, q, r, t[:, 3]], 1)], axis=1)
    best = np.argmax(t, axis=1)
    quat = cand[np.arange(len(m)), best]
    return quat / np.linalg.norm(quat, axis=1, keepdims=True)


def real_sh(l, x):
    """Y_l of unit vectors [P,3] -> [P,2l+1], m = -l..l, the basis of include/rnf_hip.h"""
    theta, phi = np.arccos(np.clip(x[:, 2], -1, 1)), np.arctan2(x[:, 1], x[:, 0])
    out = np.zeros((len(x), 2 * l + 1))
    for m in range(-l, l + 1):
        y = sph_harm_y(l, abs(m), theta, phi)
        out[:, m + l] = y.real if m == 0 else np.sqrt(2) * (-1) ** m * (y.real if m > 0 else y.imag)
    return out


@functools.lru_cache(maxsize=None)
def _points():
    x = np.random.default_rng(400).normal(size=(400, 3))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def wigner_slow(l, R):
    """D^l of ONE fp64 rotation from the definition: least squares of Y_l(R x) against Y_l(x) over 400 points"""
    X = _points()
    Dt, *_ = np.linalg.lstsq(real_sh(l, X), real_sh(l, X @ R.T), rcond=None)
    return Dt.T


@functools.lru_cache(maxsize=None)
def _basis_change(l):
    """U with Y_real = U Y_complex"""
    U = np.zeros((2 * l + 1, 2 * l + 1), complex)
    U[l, l] = 1
    s = 1 / np.sqrt(2)
    for m in range(1, l + 1):
        U[l + m, l + m], U[l + m, l - m] = (-1) ** m * s, s
        U[l - m, l + m], U[l - m, l - m] = -1j * (-1) ** m * s, 1j * s
    return U


def wigner_fp64(R, L):
    """D^l, l <= L, of fp64 rotations [n,3,3] -> [n,C_L]: the complex matrix by Wigner's sum over k,
        D_c[m'][m] = sum_k (-1)^(k-m+m') sqrt((l+m')!(l-m')!(l+m)!(l-m)!) / ((l+m-k)! k! (l-k-m')! (k-m+m')!)
                     a^(l+m-k) conj(a)^(l-m'-k) b^(k+m'-m) conj(b)^k,        a = w + iz, b = y - ix,
    in extended precision, then U D_c U^dagger."""
    n = len(R)
    ok = np.isfinite(R).all(axis=(1, 2))
    q = quaternions(np.where(ok[:, None, None], R, np.eye(3))).astype(np.longdouble)
    a, b = q[:, 0] + 1j * q[:, 3], q[:, 2] - 1j * q[:, 1]
    pw = lambda z: np.stack([z ** k for k in range(2 * L + 1)])          # noqa: E731
    A, Ac, B, Bc = pw(a), pw(np.conj(a)), pw(b), pw(np.conj(b))
    fact = [math.factorial(k) for k in range(2 * L + 2)]
    out = np.empty((n, count(L)))
    for l in range(L + 1):
        Dc = np.zeros((n, 2 * l + 1, 2 * l + 1), np.clongdouble)
        for mp in range(-l, l + 1):
            for m in range(-l, l + 1):
                norm = np.sqrt(np.longdouble(fact[l + mp] * fact[l - mp] * fact[l + m] * fact[l - m]))
                acc = np.zeros(n, np.clongdouble)
                for k in range(max(0, m - mp), min(l + m, l - mp) + 1):
                    w = np.longdouble(fact[l + m - k] * fact[k] * fact[l - k - mp] * fact[k - m + mp])
                    acc += ((-1) ** (k - m + mp) * norm / w) * A[l + m - k] * Ac[l - mp - k] * B[k + mp - m] * Bc[k]
                Dc[:, mp + l, m + l] = acc
        U = _basis_change(l)
        D = np.einsum("pa,nab,qb->npq", U, Dc.astype(complex), U.conj())
        out[:, offset(l):offset(l + 1)] = D.real.reshape(n, -1)
    out[~ok] = np.nan
    return out


def softmax_rows(lw, c_ok):
    """[G,n] log-weights, [n] whether a centre is finite -> (w [G,n], bad [G]) with the edge cases of include/rnf_hip.h"""
    G, n = lw.shape
    w, bad = np.zeros((G, n)), np.zeros(G, bool)
    for g in range(G):
        live = lw[g] != -np.inf
        if np.isnan(lw[g]).any() or (live & ~c_ok).any() or not live.any() or np.isposinf(lw[g]).any():
            bad[g] = True
            continue
        e = np.where(live, np.exp(lw[g] - lw[g][live].max()), 0.0)
        w[g] = e / e.sum()
    return w, bad


def _weights(Cn32, lw):
    Cn = np.asarray(Cn32, np.float32).reshape(-1, 3, 3)
    c_ok = np.isfinite(Cn).all(axis=(1, 2))
    lw = np.zeros((1, len(Cn))) if lw is None else np.asarray(lw, np.float32).astype(np.float64).reshape(-1, len(Cn))
    return Cn, c_ok, softmax_rows(lw, c_ok)


def fourier_fp64(Cn32, L, lw=None):
    """[G,C_L] fp64: sum_j w_gj D(C_j); a group that the edge cases make NaN is NaN"""
    Cn, c_ok, (w, bad) = _weights(Cn32, lw)
    D = np.where(c_ok[:, None], np.nan_to_num(wigner_fp64(project(Cn), L)), 0.0)
    F = w @ D
    F[bad] = np.nan
    return F


def density_fp64(coeffs, Q32, L, group_queries=False):
    """[G,m] fp64: coeffs [G,C_L] . D(Q_i); Q32 [m,3,3] or [G,m,3,3]"""
    c = np.asarray(coeffs, np.float64).reshape(-1, count(L))
    Q = np.asarray(Q32, np.float32)
    if group_queries:
        return np.stack([wigner_fp64(project(Q[g]), L) @ c[g] for g in range(len(c))])
    return c @ wigner_fp64(project(Q), L).T


def characters(cos_theta, L):
    """chi_l(theta) = sin((2l+1) theta / 2) / sin(theta / 2) = 1 + 2 sum_{k=1..l} cos(k theta) -> [..,L+1]"""
    theta = np.arccos(np.clip(cos_theta, -1.0, 1.0))
    ck = np.stack([np.cos(k * theta) for k in range(L + 1)], axis=-1)
    return 2.0 * np.cumsum(ck, axis=-1) - 1.0


def character_density(Cn32, lw, Q32, h):
    """sum_j w_gj sum_l (2l+1) h_l chi_l(theta_ij) -> [G,m] fp64"""
    Cn, c_ok, (w, bad) = _weights(Cn32, lw)
    Cp, Qp = project(np.where(c_ok[:, None, None], Cn, np.eye(3, dtype=np.float32))), project(Q32)
    cos = (np.einsum("jab,iab->ji", Cp, Qp) - 1.0) / 2.0                  # [n,m]
    L = len(h) - 1
    kern = characters(cos, L) @ (np.asarray(h, np.float64) * (2 * np.arange(L + 1) + 1))
    out = w @ kern
    out[bad] = np.nan
    return out


def scaled(coeffs, h, L):
    """(2l+1) h_l applied to coefficient vectors, as utils/harmonics.py does before the synthesis"""
    return coeffs * np.concatenate([np.full((2 * l + 1) ** 2, (2 * l + 1) * h[l]) for l in range(L + 1)])


def entry_gate(L):
    return C_ENTRY * (degree_of_entry(L) + 1) * EPS


def synthesis_gate(coeffs, ref, L):
    """[G,m] for coefficients [G,C_L] (as handed to the synthesis) and the reference [G,m]"""
    S = np.abs(np.asarray(coeffs, np.float64)).sum(axis=-1).reshape(-1, 1)
    return K_SYNTH * (L + 1) * EPS * S + EPS * np.abs(ref)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

def rodrigues(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def uniform_rotations(n, seed):
    q = np.random.default_rng(seed).normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)
    return R.reshape(n, 3, 3).astype(np.float32)


def euler_zyz(alpha, beta, gamma):
    return rodrigues([0, 0, 1], alpha) @ rodrigues([0, 1, 0], beta) @ rodrigues([0, 0, 1], gamma)


def special_rows():
    """The rows where a chart would be singular or a quaternion candidate changes"""
    rows = [np.eye(3), rodrigues([1, 0, 0], np.pi), rodrigues([0, 1, 0], np.pi), rodrigues([0, 0, 1], np.pi), rodrigues([1, 1, 1], np.pi)]
    rows += [euler_zyz(0.7, b, -1.9) for b in (0.0, np.pi, 1e-4, np.pi - 1e-4, 3e-5, np.pi - 3e-5)]
    rows += [rodrigues([0.3, -0.5, 0.8], 1e-4), rodrigues([0.3, -0.5, 0.8], np.pi - 1e-4)]
    rows += [rodrigues([0.2, 0.3, 0.1], 0.4), rodrigues([1, 0.1, 0.2], 3.0), rodrigues([0.1, 1, 0.2], 3.0), rodrigues([0.2, 0.1, 1], 3.0)]  # w, x, y, z
    rows += [1.001 * rodrigues([0.5, -0.1, 0.7], 1.3)]
    return np.stack(rows).astype(np.float32)


@functools.lru_cache(maxsize=None)
def matrix_rows():
    """200 rows: the special ones, then uniform ones"""
    sp = special_rows()
    return np.concatenate([sp, uniform_rotations(200 - len(sp), 11)])


@functools.lru_cache(maxsize=None)
def matrix_reference():
    return wigner_fp64(project(matrix_rows()), LMAX)


def weight_rows(G, n, seed):
    """G rows of log-weights: random ones, the second holds -inf, the third is a spike"""
    rng = np.random.default_rng(seed)
    lw = rng.normal(size=(G, n)).astype(np.float32) * 2
    if G > 1 and n > 1:
        lw[1, rng.integers(0, n, size=max(1, n // 3))] = -np.inf
        lw[1, 0] = 0.5
    if G > 2:
        lw[2] = -30.0
        lw[2, n // 2] = 9.0
    return lw


ANALYSIS_CASES = [(n, G, L) for n in (1, 63, 65) for G in (1, 5) for L in (0, 1, 2, 7, 16)]
SYNTHESIS_CASES = [(m, G, gq) for m in (1, 65, 257) for G in (1, 5) for gq in (False, True)]
SYNTHESIS_L = 16


@functools.lru_cache(maxsize=None)
def analysis_centres():
    return uniform_rotations(65, 21)


@functools.lru_cache(maxsize=None)
def analysis_reference_D():
    return wigner_fp64(project(analysis_centres()), LMAX)


def analysis_reference(n, G, L):
    """(centres [n,3,3], lw [G,n] or None, reference [G,C_L])"""
    Cn = analysis_centres()[:n]
    lw = weight_rows(G, n, 100 + n) if G > 1 else None
    w, bad = softmax_rows(np.zeros((1, n)) if lw is None else lw.astype(np.float64), np.ones(n, bool))
    assert not bad.any()
    return Cn, lw, w @ analysis_reference_D()[:n, :count(L)]


@functools.lru_cache(maxsize=None)
def synthesis_queries():
    """[5,257,3,3]: set 0 serves the shared case"""
    return uniform_rotations(5 * 257, 31).reshape(5, 257, 3, 3)


@functools.lru_cache(maxsize=None)
def synthesis_D():
    return wigner_fp64(project(synthesis_queries().reshape(-1, 3, 3)), SYNTHESIS_L).reshape(5, 257, -1)


@functools.lru_cache(maxsize=None)
def synthesis_coefficients():
    """[5,C_L] float32: random, not from an analysis, decaying with the degree like a smooth density's"""
    rng = np.random.default_rng(41)
    c = rng.normal(size=(5, count(SYNTHESIS_L))) * np.exp(-0.2 * degree_of_entry(SYNTHESIS_L))
    return c.astype(np.float32)


def synthesis_reference(m, G, gq):
    """(coeffs [G,C_L], queries [m,3,3] or [G,m,3,3], reference [G,m])"""
    c, Q, D = synthesis_coefficients()[:G], synthesis_queries(), synthesis_D()
    if gq:
        return c, Q[:G, :m], np.stack([D[g, :m] @ c[g].astype(np.float64) for g in range(G)])
    return c, Q[0, :m], c.astype(np.float64) @ D[0, :m].T


def fisher_multipliers_ref(kappa, L):
    x = 2.0 * kappa
    return np.array([(ive(l, x) - ive(l + 1, x)) / ((2 * l + 1) * (ive(0, x) - ive(1, x))) for l in range(L + 1)])


@functools.lru_cache(maxsize=None)
def chunk_case():
    """n = 4097 centres, G = 2, L = 8, kappa = 8, 16 queries -> (centres, lw, queries, h, character sums [2,16])"""
    Cn, Q = uniform_rotations(4097, 51), uniform_rotations(16, 52)
    lw = np.random.default_rng(53).normal(size=(2, 4097)).astype(np.float32)
    lw[1, 4096] = 6.0                                                     # the centre past the chunk boundary carries weight
    h = harmonics.fisher_multipliers(8.0, 8).numpy()
    return Cn, lw, Q, h, character_density(Cn, lw, Q, h)


def worst(err, gate):
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(err / gate))


# ---- tests -------------------------------------------------------------------------------------------------------------------------------

def test_the_two_fp64_routes_agree_and_obey_the_identities():
    R = project(np.concatenate([special_rows()[:8], uniform_rotations(12, 5)]))
    fast = wigner_fp64(R, LMAX)
    for i, Ri in enumerate(R):
        for l in range(LMAX + 1):
            assert np.abs(block(fast[i], l) - wigner_slow(l, Ri)).max() <= 1e-12, (i, l)
    p = [1, 2, 0]
    assert np.abs(block(fast, 1) - R[:, p][:, :, p]).max() <= 1e-14 and np.abs(fast[:, 0] - 1).max() <= 1e-15
    cos = (np.trace(R, axis1=1, axis2=2) - 1) / 2
    tr = np.stack([np.trace(block(fast, l), axis1=1, axis2=2) for l in range(LMAX + 1)], axis=1)
    assert np.abs(tr - characters(cos, LMAX)).max() <= 1e-11
    both = wigner_fp64(R[:10] @ R[10:], 8)
    for l in range(9):
        assert np.abs(block(fast[:10, :count(8)], l) @ block(fast[10:, :count(8)], l) - block(both, l)).max() <= 1e-13
        assert np.abs(block(wigner_fp64(R.transpose(0, 2, 1), 8), l) - block(fast[:, :count(8)], l).transpose(0, 2, 1)).max() <= 1e-13


def product_rows():
    """R_(2i) R_(2i+1) of the matrix rows (projected first), rounded to fp32"""
    P = project(matrix_rows())
    return (P[0::2] @ P[1::2]).astype(np.float32)


def check_matrices(fn, what=""):
    """The gates of the matrices test on ``fn(rows [n,3,3], L) -> [n,C_L]``; prints the worst fractions"""
    rows, ref = matrix_rows(), matrix_reference()
    D, D2 = fn(rows, LMAX).astype(np.float64), fn(product_rows(), LMAX).astype(np.float64)
    f_entry = worst(np.abs(D - ref), entry_gate(LMAX)[None])
    p = [1, 2, 0]
    d1 = np.abs(block(D, 1) - project(rows)[:, p][:, :, p]).max()
    f_orth = f_prod = 0.0
    for l in range(LMAX + 1):
        Dl = block(D, l)
        gate = C_ENTRY * (l + 1) * (2 * l + 1) * EPS
        f_orth = max(f_orth, np.abs(Dl @ Dl.transpose(0, 2, 1) - np.eye(2 * l + 1)).max() / gate)
        f_prod = max(f_prod, np.abs(Dl[0::2] @ Dl[1::2] - block(D2, l)).max() / gate)
    print(f"{what}matrices: entry {f_entry:.3f} of the gate (C_ENTRY = {C_ENTRY}), D^1 {d1 / EPS:.3f} of 2^-23, orthogonality {f_orth:.3f}, "
          f"product {f_prod:.3f}")
    assert f_entry <= 1.0 and d1 <= EPS and f_orth <= 1.0 and f_prod <= 1.0
    return f_entry


def test_host_matrices_against_the_restatement():
    check_matrices(host_wigner, "host ")
    bad = matrix_rows()[:3].copy()
    bad[1, 0, 2] = np.nan
    out = host_wigner(bad, 3)
    assert np.isnan(out[1]).all() and np.isfinite(out[[0, 2]]).all()
    assert np.array_equal(host_wigner(matrix_rows()[:9], 5), host_wigner(matrix_rows()[:9], LMAX)[:, :count(5)])      # bits do not depend on L


def check_analysis(fn, what=""):
    f = 0.0
    for n, G, L in ANALYSIS_CASES:
        Cn, lw, ref = analysis_reference(n, G, L)
        got = fn(Cn, L, lw).astype(np.float64).reshape(G, -1)
        assert got.shape == ref.shape
        f = max(f, worst(np.abs(got - ref), entry_gate(L)[None]))
        assert np.abs(got[:, 0] - 1).max() <= 2 * EPS
    print(f"{what}analysis: {f:.3f} of the gate")
    assert f <= 1.0
    return f


def test_host_analysis_against_the_restatement():
    check_analysis(host_fourier, "host ")


def check_chunk_boundary(fourier, density, what=""):
    Cn, lw, Q, h, ref = chunk_case()
    F = fourier(Cn, 8, lw)
    c = scaled(F.astype(np.float64), h, 8).astype(np.float32)
    got = density(c, Q, 8).astype(np.float64)
    f = worst(np.abs(got - ref), synthesis_gate(c, ref, 8))
    print(f"{what}chunk boundary: {f:.3f} of the gate (K_SYNTH = {K_SYNTH})")
    assert f <= 1.0
    return f


def test_host_chunk_boundary_against_the_character_sum():
    check_chunk_boundary(host_fourier, host_density, "host ")


def check_synthesis(fn, what=""):
    f = 0.0
    for m, G, gq in SYNTHESIS_CASES:
        c, Q, ref = synthesis_reference(m, G, gq)
        got = fn(c, Q, SYNTHESIS_L, gq).astype(np.float64)
        f = max(f, worst(np.abs(got - ref), synthesis_gate(c, ref, SYNTHESIS_L)))
    print(f"{what}synthesis: {f:.3f} of the gate (K_SYNTH = {K_SYNTH})")
    assert f <= 1.0
    return f


def test_host_synthesis_against_the_restatement():
    check_synthesis(host_density, "host ")


def test_character_sum_equals_the_synthesis_of_the_analysis_in_fp64():
    Cn, Q = uniform_rotations(9, 61), uniform_rotations(7, 62)
    lw = weight_rows(3, 9, 63)
    h = harmonics.heat_multipliers(0.05, 8).numpy()
    a = density_fp64(scaled(fourier_fp64(Cn, 8, lw), h, 8), Q, 8)
    assert np.abs(a - character_density(Cn, lw, Q, h)).max() <= 1e-12


def test_helpers_exact_algebra_on_cpu_tensors():
    L = 6
    Ra, Rb = uniform_rotations(7, 71), uniform_rotations(5, 72)
    lwa, lwb = np.random.default_rng(73).normal(size=7).astype(np.float32), np.random.default_rng(74).normal(size=5).astype(np.float32)
    Fa, Fb = torch.from_numpy(fourier_fp64(Ra, L, lwa)[0]), torch.from_numpy(fourier_fp64(Rb, L, lwb)[0])
    Pa, Pb = project(Ra), project(Rb)
    prod = (Pa[:, None] @ Pb[None]).reshape(35, 3, 3)
    lwp = (lwa[:, None].astype(np.float64) + lwb[None]).reshape(35)
    wa = softmax_rows(lwa[None].astype(np.float64), np.ones(7, bool))[0][0]
    wp = softmax_rows(lwp[None], np.ones(35, bool))[0][0]
    ref = wp @ wigner_fp64(prod, L)
    assert np.abs(harmonics.compose(Fa, Fb, L).numpy() - ref).max() <= 1e-13
    rel = (Pa.transpose(0, 2, 1)[:, None] @ Pb[None]).reshape(35, 3, 3)
    assert np.abs(harmonics.compose(Fa, Fb, L, invert_a=True).numpy() - wp @ wigner_fp64(rel, L)).max() <= 1e-13
    inv = wa @ wigner_fp64(Pa.transpose(0, 2, 1), L)
    one = torch.from_numpy(wigner_fp64(np.eye(3)[None], L)[0])
    assert np.abs(harmonics.compose(Fa, one, L, invert_a=True).numpy() - inv).max() <= 1e-13
    cos = (np.einsum("iab,jab->ij", Pa, Pa) - 1) / 2
    ps = np.einsum("i,j,ijl->l", wa, wa, characters(cos, L) * (2 * np.arange(L + 1) + 1))
    assert np.abs(harmonics.power_spectrum(Fa, L).numpy() - ps).max() <= 1e-13
    both = torch.stack([Fa, Fa])                                          # groups, views and the way back
    assert harmonics.power_spectrum(both, L).shape == (2, L + 1)
    assert torch.equal(harmonics.from_blocks(harmonics.blocks(both, L)), both) and harmonics.blocks(both, L)[3].shape == (2, 7, 7)
    assert harmonics.blocks(both, L)[2].data_ptr() == both[:, harmonics.degree_offset(2):].data_ptr()
    assert [harmonics.coefficient_count(k) for k in (0, 1, 8, 16)] == [1, 10, 969, 6545] and harmonics.MAX_DEGREE == 16
    assert all(harmonics.degree_offset(l + 1) == harmonics.coefficient_count(l) == _host_lib().hsh_coefficient_count(l) for l in range(17))


@pytest.mark.parametrize("kappa", [0.05, 1.0, 30.0, 1e3])
def test_fisher_multipliers_against_scipy(kappa):
    got, ref = harmonics.fisher_multipliers(kappa, LMAX).numpy(), fisher_multipliers_ref(kappa, LMAX)
    assert got.dtype == np.float64 and got[0] == 1.0
    assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max() and np.all(np.abs(got - ref) <= 1e-9 * np.abs(ref) + 1e-300)
    assert np.array_equal(harmonics.fisher_multipliers(0.0, 3).numpy(), [1.0, 0.0, 0.0, 0.0])
    assert np.allclose(harmonics.heat_multipliers(0.1, 3).numpy(), np.exp(-0.1 * np.array([0, 2, 6, 12])), rtol=1e-15)


def test_fisher_multipliers_are_the_kernels_angle_integral():
    """a_l = the integral of chi_l k_kappa / (2l+1) over the angle: density (1 - cos t) / pi on [0, pi], k = exp(2 kappa (cos t - 1)) / c"""
    t = (np.arange(200000) + 0.5) * np.pi / 200000
    for kappa in (0.3, 4.0, 16.0):
        k = np.exp(2 * kappa * (np.cos(t) - 1)) * (1 - np.cos(t))
        ref = (characters(np.cos(t), 8) * k[:, None]).sum(0) / k.sum() / (2 * np.arange(9) + 1)
        assert np.abs(harmonics.fisher_multipliers(kappa, 8).numpy() - ref).max() <= 1e-8


def test_host_bit_identity_across_groups_degrees_and_tilings():
    Cn, lw = analysis_centres(), weight_rows(5, 65, 81)
    F5 = host_fourier(Cn, 16, lw)
    assert np.array_equal(host_fourier(Cn, 16, lw[3:4])[0], F5[3])        # alone and as the fourth of five
    assert np.array_equal(host_fourier(Cn, 7, lw[3:4])[0], F5[3, :count(7)])      # the degrees split over two calls
    assert np.array_equal(host_fourier(Cn, 9, lw)[:, count(7):], F5[:, count(7):count(9)])
    c, Q = synthesis_coefficients(), synthesis_queries()
    full = host_density(c, Q[0], SYNTHESIS_L)
    assert np.array_equal(host_density(c[2:3], Q[0, 100:130], SYNTHESIS_L)[0], full[2, 100:130])
    grouped = host_density(c, np.broadcast_to(Q[0], Q.shape).copy(), SYNTHESIS_L, True)
    assert np.array_equal(grouped, full)


def test_host_edge_cases():
    Cn, Q = analysis_centres().copy(), synthesis_queries()[0, :6].copy()
    lw = weight_rows(5, 65, 91)
    lw[1, 7] = -np.inf
    Cn[7, 1, 1] = np.nan                                                  # dead in group 1, live elsewhere
    lw[4] = -np.inf                                                       # no mass
    F = host_fourier(Cn, 8, lw)
    assert np.isfinite(F[1]).all() and np.isnan(F[[0, 2, 3, 4]]).all()
    clean = analysis_centres().copy()
    keep = np.delete(np.arange(65), 7)
    ref = fourier_fp64(clean[keep], 8, lw[1:2, keep])
    assert worst(np.abs(F[1:2] - ref), entry_gate(8)[None]) <= 1.0         # the dead centre is left out whatever its entries
    assert np.isnan(fourier_fp64(Cn, 8, lw)[[0, 2, 3, 4]]).all() and np.isfinite(fourier_fp64(Cn, 8, lw)[1]).all()
    lwn = weight_rows(2, 65, 92)
    lwn[0, 64] = np.nan
    Fn = host_fourier(clean, 8, lwn)
    assert np.isnan(Fn[0]).all() and np.isfinite(Fn[1]).all()
    Q[2, 0, 0] = np.inf
    c = synthesis_coefficients()[:3, :count(8)].copy()
    c[1, 5] = np.nan
    f = host_density(c, Q, 8)
    assert np.isnan(f[:, 2]).all() and np.isnan(f[1]).all() and np.isfinite(np.delete(f[[0, 2]], 2, axis=1)).all()


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------

_FAKE = 1 << 20


def _bytes(name, a):
    return getattr(_lib.lib(), f"rnf_{name}_workspace_bytes")(C.byref(a))


def _refused(name, a, word):
    L = _lib.lib()
    assert getattr(L, "rnf_" + name)(C.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def _fourier_args(**kw):
    a = _lib.So3Fourier(**{**dict(centres=_FAKE, log_weights=_FAKE, n=4608, G=3, lmax=8, out=_FAKE), **kw})
    a.workspace, a.workspace_bytes = _FAKE, _bytes("so3_fourier", a)
    return a


def _eval_args(**kw):
    a = _lib.So3FourierEval(**{**dict(coeffs=_FAKE, queries=_FAKE, m=1000, G=3, lmax=8, out=_FAKE), **kw})
    a.workspace, a.workspace_bytes = _FAKE, _bytes("so3_fourier_eval", a)
    return a


def _wigner_args(**kw):
    a = _lib.So3Wigner(**{**dict(rotations=_FAKE, n=100, lmax=8, out=_FAKE), **kw})
    a.workspace, a.workspace_bytes = _FAKE, _bytes("so3_wigner", a)
    return a


def test_c_abi_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.rnf_abi_version() == 8
    rec = (4 * 17 * 17 * (2 + 4 * 8) + 15) // 16 * 16
    a = _fourier_args()
    assert a.workspace_bytes == (8 * 3 * 2 * 969 + 16 * 3 * 2 + 8 * 3 + 4 * 3 * 4608 + 15) // 16 * 16 + 4 * 4608 * (8 * 8 + 16) + rec
    assert a.workspace_bytes == _host_lib().hsh_fourier_workspace_bytes(C.c_longlong(4608), 3, 8)
    assert _eval_args().workspace_bytes == rec == _wigner_args().workspace_bytes == _host_lib().hsh_records_bytes(8)
    for name, make, cases in (
            ("so3_fourier", _fourier_args, ((dict(lmax=-1), "lmax="), (dict(lmax=17), "lmax="), (dict(G=0), "G="), (dict(G=65536), "G="),
                                            (dict(n=0), "n="), (dict(n=(1 << 24) + 1), "n="))),
            ("so3_fourier_eval", _eval_args, ((dict(lmax=-1), "lmax="), (dict(lmax=17), "lmax="), (dict(G=0), "G="), (dict(G=65536), "G="),
                                              (dict(m=-1), "m="), (dict(m=1 << 31), "m="))),
            ("so3_wigner", _wigner_args, ((dict(lmax=-1), "lmax="), (dict(lmax=17), "lmax="), (dict(n=-1), "n="), (dict(n=(1 << 24) + 1), "n=")))):
        for bad, word in cases:
            arg = make(**bad)
            _refused(name, arg, word)
            assert arg.workspace_bytes == 0
        a = make()
        a.workspace_bytes -= 1
        _refused(name, a, "workspace")
        a = make()
        a.workspace += 8
        _refused(name, a, "aligned")
        a = make(workspace=None)
        a.workspace = None
        _refused(name, a, "workspace")
        a = make()
        a.struct_bytes += 8
        _refused(name, a, "struct_bytes")
        assert _bytes(name, a) == 0
    for name, make, ptrs in (("so3_fourier", _fourier_args, ("centres", "out")), ("so3_fourier_eval", _eval_args, ("coeffs", "queries", "out")),
                             ("so3_wigner", _wigner_args, ("rotations", "out"))):
        for p in ptrs:
            _refused(name, make(**{p: None}), "null")
    assert L.rnf_so3_fourier_eval(C.byref(_eval_args(m=0))) == 0 and L.rnf_so3_wigner(C.byref(_wigner_args(n=0))) == 0      # no-ops


def test_header_declares_the_structs_the_bindings_mirror():
    import re
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    for cname, cls in (("RnfSo3Wigner", _lib.So3Wigner), ("RnfSo3Fourier", _lib.So3Fourier), ("RnfSo3FourierEval", _lib.So3FourierEval)):
        body = header[header.index("typedef struct %s {" % cname) + len(cname) + 17:header.index("} %s;" % cname)]
        names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
        assert names == [f for f, _ in cls._fields_], names
        assert names[0] == "struct_bytes" and names[-3:] == ["workspace", "workspace_bytes", "stream"]
    assert {"rnf_so3_wigner", "rnf_so3_fourier", "rnf_so3_fourier_eval", "rnf_so3_wigner_workspace_bytes", "rnf_so3_fourier_workspace_bytes",
            "rnf_so3_fourier_eval_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "#define RNF_ABI_VERSION 8" in header and "#define RNF_SO3_MAX_DEGREE 16" in header and _lib.SO3_MAX_DEGREE == 16


def test_python_entry_points_validate_their_arguments():
    from rotationnormflow_amd import grid_pose, harness
    R = torch.eye(3).expand(5, 3, 3).contiguous()
    with pytest.raises(ValueError, match="CPU"):
        harmonics.wigner_matrices(R, 2)
    with pytest.raises(ValueError, match="CPU"):
        harmonics.so3_fourier(R, 2)
    with pytest.raises(ValueError, match="CPU"):
        harmonics.so3_fourier_density(torch.zeros(10), R, 1)
    for bad in (-1, 17, 2.0, True):
        with pytest.raises(ValueError, match="lmax"):
            harmonics.so3_fourier(R, bad)
        with pytest.raises(ValueError, match="lmax"):
            harmonics.coefficient_count(bad)
    with pytest.raises(ValueError, match="coeffs"):
        harmonics.so3_fourier_density(torch.zeros(11), R, 1)
    with pytest.raises(ValueError, match="coeffs"):
        harmonics.blocks(torch.zeros(3, 11), 1)
    with pytest.raises(ValueError, match="block 1"):
        harmonics.from_blocks([torch.zeros(1, 1), torch.zeros(2, 2)])
    with pytest.raises(ValueError, match="side"):
        harmonics.rotate(torch.zeros(10), torch.eye(3), 1, side="up")
    with pytest.raises(ValueError, match="kappa"):
        harmonics.fisher_multipliers(-1.0, 3)
    with pytest.raises(ValueError, match="t="):
        harmonics.heat_multipliers(float("nan"), 3)
    lp, grid = torch.zeros(2, 72), torch.zeros(72, 3, 3)
    for fn in (grid_pose.grid_spectrum, grid_pose.grid_diffuse_spectral):
        with pytest.raises(ValueError, match="GPU"):
            fn(lp, grid)
        with pytest.raises(ValueError, match="grid"):
            fn(lp, torch.zeros(71, 3, 3))
    with pytest.raises(ValueError, match="GPU"):
        grid_pose.grid_compose(lp, lp, grid)
    with pytest.raises(ValueError, match="grid_diffuse_local"):
        grid_pose._spectral_multiplier(200.0, None, 8, "grid_diffuse_spectral")
    with pytest.raises(ValueError, match="one of the two"):
        grid_pose._spectral_multiplier(2.0, 0.1, 8, "grid_diffuse_spectral")
    with pytest.raises(ValueError, match="required"):
        grid_pose._spectral_multiplier(None, None, 8, "grid_diffuse_spectral")
    h, trunc = grid_pose._spectral_multiplier(2.0, None, 8, "grid_diffuse_spectral")
    assert trunc == float(17 * h[8]) and trunc < 1e-2
    for name in ("grid_spectrum", "grid_diffuse_spectral", "grid_compose", "grid_pose_spectrum"):
        assert getattr(harness, name) is getattr(grid_pose, name)


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_so3_harmonics.cpp (its own main: ragged sizes across the tile and chunk boundaries, L = 0 and 16, -inf and NaN
    rows, queries per group) built with the host-side address and undefined-behaviour sanitizers (-Xarch_host: host code only, nothing
    for the GPU) and run as a process of its own."""
    exe = str(tmp_path / "sanitize_so3_harmonics")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_so3_harmonics.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)
