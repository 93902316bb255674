"""CPU: the host build of csrc/fisher_exact.h -- the scaled Bessel functions, the fixed 224-node quadrature of the exact matrix-Fisher
log-normaliser c, its derivative dc/ds = E[Q] and dc/dA = E[R] -- against scipy's ``ive`` and the independent fp64 references of
tests/fisher_exact.py.  The host build adds the nodes in the order of the device kernel (64 lane sums, then the xor butterfly), so what
passes here is the arithmetic the wave-per-matrix kernel runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.special import ive

from tests import fisher_exact as fe

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_fisher_exact.cpp")
OUT = os.path.join(HERE, "csrc", "_host_fisher_exact.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f) for f in ("fisher_exact.h", "fisher_math.h")]

# the list of tests/test_fisher_exact.py
S_CHECK = [(0.0, 0.0, 0.0), (1.0, 0.5, -0.3), (5.0, 3.0, 1.0), (5.0, 1.0, -1.0), (2.0, 2.0, 2.0), (4.0, 4.0, 1.0), (3.0, 3.0, -3.0),
           (1e-4, 2e-5, 0.0), (30.0, 20.0, 10.0), (3e4, 2e4, 1e4), (1e4, 1.0, 1e-3)]


@pytest.fixture(scope="module")
def hfe():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    lib = C.CDLL(OUT)
    lib.hfe_bessel_split.restype = C.c_double
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _from_s(hfe, S):
    S = np.ascontiguousarray(S, np.float64).reshape(-1, 3)
    B = S.shape[0]
    c, m, h = np.empty(B), np.empty((B, 3)), np.empty(B)
    hfe.hfe_from_s(ptr(S), B, ptr(c), ptr(m), ptr(h))
    return c, m, h


def _exact(hfe, A):
    A = np.ascontiguousarray(A, np.float64).reshape(-1, 3, 3)
    B = A.shape[0]
    c, dc, h = np.empty(B), np.empty((B, 3, 3)), np.empty(B)
    hfe.hfe_exact(ptr(A), B, ptr(c), ptr(dc), ptr(h))
    return c, dc, h


def test_scaled_bessel_functions_against_scipy(hfe):
    """bessel_i0e / bessel_i1e: relative error <= 1e-12 on [1e-8, 1e5], at 0 and on both sides of the series / Chebyshev crossover."""
    split = hfe.hfe_bessel_split()
    x = np.concatenate([[0.0], np.logspace(-8, 5, 2000), [np.nextafter(split, 0.0), split, np.nextafter(split, np.inf)]])
    i0, i1 = np.empty_like(x), np.empty_like(x)
    hfe.hfe_bessel(ptr(x), len(x), ptr(i0), ptr(i1))
    r0 = np.abs(i0 - ive(0, x)) / ive(0, x)
    r1 = np.abs(i1[1:] - ive(1, x[1:])) / ive(1, x[1:])
    print("max relative error: i0e %.3g, i1e %.3g" % (r0.max(), r1.max()))
    assert i0[0] == 1.0 and i1[0] == 0.0
    assert r0.max() <= 1e-12 and r1.max() <= 1e-12
    # odd / even continuation and the limits the quadrature relies on for non-finite input
    xn = np.array([-3.0, -20.0, np.inf, np.nan])
    j0, j1 = np.empty_like(xn), np.empty_like(xn)
    hfe.hfe_bessel(ptr(xn), len(xn), ptr(j0), ptr(j1))
    assert np.allclose(j0[:2], ive(0, xn[:2]), rtol=1e-12, atol=0) and np.allclose(j1[:2], ive(1, xn[:2]), rtol=1e-12, atol=0)
    assert j0[2] == 0.0 and j1[2] == 0.0 and np.isnan(j0[3]) and np.isnan(j1[3])


def test_nodes_are_a_rule_on_the_interval(hfe):
    """224 nodes, (1 - u) + (1 + u) = 2, weights positive and summing to 2, symmetric about 0, exact for polynomials of degree 31 per panel."""
    n = hfe.hfe_nodes()
    assert n == 224
    om, op, w = np.empty(n), np.empty(n), np.empty(n)
    for j in range(n):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        hfe.hfe_node(j, C.byref(a), C.byref(b), C.byref(c))
        om[j], op[j], w[j] = a.value, b.value, c.value
    assert (om > 0).all() and (op > 0).all() and (w > 0).all()
    assert np.abs(om + op - 2.0).max() <= 4e-16
    assert abs(w.sum() - 2.0) <= 1e-15
    assert (om == op[::-1]).all() and (w == w[::-1]).all()
    assert (np.diff(op) > 0).all() and op[0] < 1e-8 and om[-1] < 1e-8
    u = 0.5 * (op - om)
    for k in (2, 6, 20):
        assert abs(np.dot(w, u ** k) - 2.0 / (k + 1)) <= 1e-14


def test_host_c_and_dcds_against_the_reference(hfe):
    _, s_edge, _ = fe.proper_svd64(fe.EDGE_STACK)
    S = np.concatenate([np.array(S_CHECK), s_edge])
    names = [str(s) for s in S_CHECK] + fe.EDGE_NAMES
    c, m, _ = _from_s(hfe, S)
    worst_c = worst_m = 0.0
    for b, name in enumerate(names):
        want, mq = fe.log_c(S[b]), fe.mean_Q(S[b])
        ec, em = abs(c[b] - want) / max(1.0, abs(want)), np.abs(m[b] - mq).max()
        worst_c, worst_m = max(worst_c, ec), max(worst_m, em)
        assert ec <= 1e-10, (name, c[b], want)
        assert em <= 1e-9, (name, m[b], mq)
    print("worst |c - log_c| / max(1, |log_c|) = %.3g, worst |dc/ds - mean_Q| = %.3g" % (worst_c, worst_m))
    c0, m0, h0 = _from_s(hfe, np.zeros((1, 3)))
    assert abs(c0[0]) <= 1e-15 and np.abs(m0).max() <= 1e-15 and abs(h0[0]) <= 1e-15


def test_host_entropy_against_the_reference(hfe):
    """The entropy integral (no cancellation of c against tr(A^T E[R])) against log_c - sum s mean_Q where that difference is well
    conditioned in fp64: |s| <= 30."""
    S = np.array([s for s in S_CHECK if max(np.abs(s)) <= 30.0])
    _, _, h = _from_s(hfe, S)
    for b in range(len(S)):
        want = fe.log_c(S[b]) - float((S[b] * fe.mean_Q(S[b])).sum())
        assert abs(h[b] - want) <= 1e-10 * max(1.0, abs(want)), (S[b], h[b], want)
        assert h[b] <= 1e-15


def test_host_dcdA_against_the_reference(hfe):
    c, dc, _ = _exact(hfe, fe.EDGE_STACK)
    U, s, V = fe.proper_svd64(fe.EDGE_STACK)
    for b, name in enumerate(fe.EDGE_NAMES):
        want = U[b] @ np.diag(fe.mean_Q(s[b])) @ V[b].T
        err = np.abs(dc[b] - want).max()
        lc = fe.log_c(s[b])
        assert abs(c[b] - lc) <= 1e-10 * max(1.0, abs(lc)), name
        if name in ("zero", "2I", "2rot", "minus3I"):               # mean_Q constant on the repeated values: any valid SVD gives the same matrix
            assert err <= 1e-9, (name, err)
        elif s[b, 1] > 1e-6 * s[b, 0]:
            assert err <= 1e-9 * max(1.0, s[b, 0] / s[b, 1]), (name, err)
        else:                                                       # rank 1: the singular vectors of the zero values are free
            assert abs(np.linalg.norm(dc[b]) - np.linalg.norm(want)) <= 1e-9, name
            assert abs((fe.EDGE_STACK[b] * (dc[b] - want)).sum()) <= 1e-9 * max(1.0, s[b, 0]), name


def test_host_propagates_nan_and_inf(hfe):
    A = np.stack([np.full((3, 3), np.nan), np.diag([np.inf, 1.0, 1.0]), np.diag([1.0, np.nan, 2.0])])
    with np.errstate(all="ignore"):
        c, dc, _ = _exact(hfe, A)
    assert np.isnan(c).all()
