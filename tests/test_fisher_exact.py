"""CPU: the exact matrix-Fisher references (tests/fisher_exact.py) checked on their own, and the host build of csrc/fisher_math.h (proper SVD
and the closed-form log-constants with their derivative) against them on the shared edge matrices EDGE_A: zero and rank-deficient A,
repeated and sign-cancelling singular values, negative determinants, unsorted and permutation inputs, 1e-4 .. 1e4 scales."""
import ctypes as C

import numpy as np
import pytest

from tests import fisher_exact as fe
from tests.test_host_grad import hg, ptr  # noqa: F401  (module fixture: host build of fisher_math.h)

S_CHECK = [(0.0, 0.0, 0.0), (1.0, 0.5, -0.3), (5.0, 3.0, 1.0), (5.0, 1.0, -1.0), (2.0, 2.0, 2.0), (4.0, 4.0, 1.0), (3.0, 3.0, -3.0),
           (1e-4, 2e-5, 0.0), (30.0, 20.0, 10.0), (3e4, 2e4, 1e4), (1e4, 1.0, 1e-3)]


@pytest.mark.parametrize("s", S_CHECK)
def test_reference_is_symmetric_in_the_integration_order(s):
    """All six orderings (i, j, k) of the 1-D integral give the same log c; the two analytic routes to E[Q] agree."""
    perms = list(fe.PERMS) + [(1, 0, 2), (0, 2, 1), (2, 1, 0)]
    lc = np.array([fe.log_c(s, p) for p in perms])
    assert np.isfinite(lc).all()
    assert np.ptp(lc) < 1e-10 * max(1.0, abs(lc[0]))
    m = fe.mean_Q(s)
    assert np.abs(m - fe.mean_Q_by_u(s)).max() < 1e-10
    assert (np.abs(m) <= 1.0).all()


def test_reference_at_zero_and_small_s():
    assert fe.log_c((0.0, 0.0, 0.0)) == 0.0
    assert (fe.mean_Q((0.0, 0.0, 0.0)) == 0.0).all()
    # small s: E_unif[Q_ii^2] = 1/3, E_unif[Q_00 Q_11 Q_22] = 1/6 -> c = 1 + |s|^2 / 6 + s0 s1 s2 / 6 + O(s^4) (the type-0 form)
    s = np.array([3e-4, -2e-4, 1e-4])
    assert abs(fe.log_c(s) - np.log1p((s ** 2).sum() / 6.0 + s.prod() / 6.0)) < 1e-15
    assert np.abs(fe.mean_Q(s) - (s / 3.0 + s[[1, 2, 0]] * s[[2, 0, 1]] / 6.0)).max() < 1e-11


@pytest.mark.parametrize("s", [(1.0, 0.5, -0.3), (3.0, 2.0, 1.0), (2.0, 2.0, 2.0), (4.0, 1.0, -1.0), (2.5, 2.5, -0.5)])
def test_reference_against_monte_carlo(s):
    """log c, E[Q] and c(2S) against a plain fp64 Monte-Carlo over 2^20 uniform rotations, within 5 standard errors."""
    n = 1 << 20
    s = np.array(s)
    Q = fe.uniform_rotations64(n, seed=int(1000 * s[0] + 100 * s[1]) & 0xFFFF)
    d = np.einsum("nii->ni", Q)
    w = np.exp(d @ s)                                               # exp(tr(S Q))
    c = np.exp(fe.log_c(s))
    assert abs(w.mean() - c) < 5 * w.std() / np.sqrt(n)
    dw = d * w[:, None]                                             # d c / d s_i = E_unif[Q_ii exp(tr(S Q))] = c E[Q_ii]
    assert (np.abs(dw.mean(0) - c * fe.mean_Q(s)) < 5 * dw.std(0) / np.sqrt(n)).all()
    w2 = w * w                                                      # E_unif[exp(2 tr(S Q))] = c(2S)
    assert abs(w2.mean() - np.exp(fe.log_c(2 * s))) < 5 * w2.std() / np.sqrt(n)
    assert abs(np.sqrt(w.var() / c ** 2) / fe.mc_rel_std(s) - 1.0) < 0.05


@pytest.mark.parametrize("shape", [(3.0, 2.0, 1.0), (1.0, 1.0, -0.5), (5.0, 1.0, 1.0)])
def test_type1_normaliser_is_the_laplace_limit(shape):
    """log c - c_type1 > 0 and shrinks like 1/t along s = t * shape (t = 10 .. 1e4)."""
    t = np.array([10.0, 100.0, 1000.0, 1e4])
    d = np.array([fe.log_c(x * np.array(shape)) - fe.log_const_t1(x * np.array(shape))[0] for x in t])
    assert (d > 0).all()
    ratio = d[1:] / d[:-1]
    assert (np.abs(ratio - 0.1) < 0.02).all(), ratio
    td = t * d
    assert abs(td[-1] / td[-2] - 1.0) < 2e-3, td


def _host_const(hg, A, norm_type):  # noqa: F811
    A = np.ascontiguousarray(A, np.float64)
    B = A.shape[0]
    Q = float((A ** 2).sum())
    c, dc = np.zeros(B), np.zeros((B, 3, 3))
    U, S, V = np.zeros((B, 3, 3)), np.zeros((B, 3)), np.zeros((B, 3, 3))
    with np.errstate(all="ignore"):
        hg.hg_fisher_const(ptr(A), B, norm_type, C.c_double(Q), ptr(c), ptr(dc), ptr(U), ptr(S), ptr(V))
    return c, dc, U, S, V


def test_host_proper_svd_on_edge_matrices(hg):  # noqa: F811
    """proper_svd3 on every EDGE_A matrix: U, V rotations, U diag(s) V^T = A, s ordered and signed as the reference's LAPACK proper SVD."""
    A = fe.EDGE_STACK
    _, _, U, S, V = _host_const(hg, A, 1)
    _, s_ref, _ = fe.proper_svd64(A)
    eye = np.eye(3)
    for b, name in enumerate(fe.EDGE_NAMES):
        scale = max(1.0, s_ref[b, 0])
        for M in (U[b], V[b]):
            assert np.abs(M.T @ M - eye).max() < 1e-12, name
            assert abs(np.linalg.det(M) - 1.0) < 1e-12, name
        assert np.abs(U[b] @ np.diag(S[b]) @ V[b].T - A[b]).max() < 1e-12 * scale, name
        assert np.abs(S[b] - s_ref[b]).max() < 1e-12 * scale, (name, S[b], s_ref[b])
        assert S[b, 0] >= S[b, 1] and S[b, 1] >= abs(S[b, 2]) - 1e-12 * scale, name


def test_host_log_constants_on_edge_matrices(hg):  # noqa: F811
    """fisher_log_const (types 0 and 1) and its derivative against the fp64 closed forms on EDGE_A; where the reference's type-1 value is
    infinite (a proper singular-value pair sums to exactly 0) the host gives +inf too."""
    A = fe.EDGE_STACK
    U_ref, s_ref, V_ref = fe.proper_svd64(A)
    c, dc, _, _, _ = _host_const(hg, A, 1)
    want = fe.log_const_t1(s_ref)
    with np.errstate(all="ignore"):
        dwant = fe.dlog_const_t1(U_ref, s_ref, V_ref)
    for b, name in enumerate(fe.EDGE_NAMES):
        if name in fe.INF_T1_EXACT:
            assert c[b] == np.inf, (name, c[b])
            continue
        if name in fe.INF_T1:                                       # infinite in exact arithmetic, rounding decides both values
            continue
        assert np.isfinite(want[b]), name
        assert abs(c[b] - want[b]) < 1e-12 * max(1.0, abs(want[b])), (name, c[b], want[b])
        # U, V come from the eigenvectors of A^T A: the smaller singular vectors lose digits with the condition s0 / s1
        assert np.abs(dc[b] - dwant[b]).max() < 1e-11 * max(1.0, s_ref[b, 0] / s_ref[b, 1]) * max(1.0, np.abs(dwant[b]).max()), name
    # type 0: batch-coupled through Q = sum_b |A_b|_F^2 (zero rows included), derivative for fixed Q = cofactor / (6 D)
    c0, dc0, _, _, _ = _host_const(hg, A, 0)
    want0 = fe.log_const_t0(A)
    assert np.abs(c0 - want0).max() < 1e-12 * max(1.0, np.abs(want0).max())
    D = 1.0 + (A ** 2).sum() / 6.0 + np.linalg.det(A) / 6.0
    dwant0 = np.stack([_cofactor(a) for a in A]) / (6.0 * D[:, None, None])
    assert np.abs(dc0 - dwant0).max() < 1e-13 * np.abs(dwant0).max()
    # a batch of one zero matrix: Q = 0, det = 0 -> c = 0 exactly
    z, dz, _, _, _ = _host_const(hg, np.zeros((1, 3, 3)), 0)
    assert z[0] == 0.0 and (dz == 0.0).all()


def _cofactor(a):
    """d det(a) / d a (rows: cofactors), valid for singular a too."""
    out = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            m = np.delete(np.delete(a, i, 0), j, 1)
            out[i, j] = (-1) ** (i + j) * (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])
    return out
