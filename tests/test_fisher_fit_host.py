"""CPU: the host build of csrc/fisher_fit.h -- the Hessian of the exact matrix-Fisher log-normaliser c, the damped Newton solve of
grad c(s) = d and the fit A = U diag(s) V^T of a moment matrix -- against the independent fp64 references of tests/fisher_exact.py
(``mean_Q``, ``log_c``, ``proper_svd64``).  The host build adds the quadrature nodes in the order of the device kernel (64 lane sums,
then the xor butterfly), so what passes here is the arithmetic the wave-per-matrix kernel runs.

RESIDUAL is the gate on |mean_Q(s_fit) - d|_inf, the quantity the solve controls; |s_fit - s| is gated at RESIDUAL / lambda_min(H_ref)
per row, because that is how a residual in d moves s.  Measured on this host build over S_CHECK plus the proper singular values of
EDGE_A: the largest residual is 3.81e-11 (at (1e4, 1, 1e-3) and EDGE_A's "aniso": the reference's and the 224-node rule's mean_Q differ
by that much there; the solve's own stop rule is 5e-14).  RESIDUAL = 8 x 3.81e-11 = 3.1e-10, inside the 1e-9 allowed at most."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import fisher_exact as fe
from tests.test_fisher_exact_host import S_CHECK

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_fisher_fit.cpp")
OUT = os.path.join(HERE, "csrc", "_host_fisher_fit.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f) for f in ("fisher_fit.h", "fisher_exact.h", "fisher_math.h")]

RESIDUAL = 3.1e-10
CAPPED, NOT_CONVERGED, INPUT = 1, 2, 4
# S_CHECK reaches 3e4: the round trips run with a cap above it, the status tests with the default 1e4
CAP_ROUND_TRIP = 1e5
EPS32 = 2.0 ** -23


@pytest.fixture(scope="module")
def hff():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    return C.CDLL(OUT)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def full(h):
    return np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]])


def hessian(hff, S):
    S = np.ascontiguousarray(S, np.float64).reshape(-1, 3)
    m, H = np.empty((len(S), 3)), np.empty((len(S), 6))
    hff.hff_hessian(ptr(S), len(S), ptr(m), ptr(H))
    return m, H


def solve(hff, D, cap=1e4, max_iter=0):
    D = np.ascontiguousarray(D, np.float64).reshape(-1, 3)
    B = len(D)
    s, H, it, st = np.empty((B, 3)), np.empty((B, 6)), np.empty(B, np.int32), np.empty(B, np.int32)
    hff.hff_solve(ptr(D), B, C.c_double(cap), int(max_iter), ptr(s), ptr(H), ptr(it), ptr(st))
    return s, H, it, st


def fit(hff, M, cap=1e4, max_iter=0):
    M = np.ascontiguousarray(M, np.float64).reshape(-1, 3, 3)
    B = len(M)
    A, s, H, it, st = np.empty((B, 3, 3)), np.empty((B, 3)), np.empty((B, 6)), np.empty(B, np.int32), np.empty(B, np.int32)
    hff.hff_fit(ptr(M), B, C.c_double(cap), int(max_iter), ptr(A), ptr(s), ptr(H), ptr(it), ptr(st))
    return A, s, H, it, st


def reference_hessian(s, scale=1.0):
    """d mean_Q / d s by central differences with per-coordinate steps h_j = 1e-3 max(1, |s_j|) * scale, and the scheme's own error: the
    truncation error of D(h) is (D(h) - D(2h)) / 3 to leading order, and the reference's mean_Q is good to 1e-13 (its two routes agree
    to that), which the difference amplifies by 1 / h."""
    s = np.asarray(s, np.float64)
    out, err = np.empty((3, 3)), np.empty((3, 3))
    for j in range(3):
        h = 1e-3 * max(1.0, abs(s[j])) * scale
        e = np.zeros(3)
        e[j] = h
        d1 = (fe.mean_Q(s + e) - fe.mean_Q(s - e)) / (2 * h)
        d2 = (fe.mean_Q(s + 2 * e) - fe.mean_Q(s - 2 * e)) / (4 * h)
        out[:, j] = d1
        err[:, j] = np.abs(d1 - d2) + 2e-13 / h
    return out, err


def lambda_min_ref(s):
    """The smallest eigenvalue of the reference Hessian (symmetrised differences of fe.mean_Q)."""
    h = reference_hessian(s)[0]
    return float(np.linalg.eigvalsh(0.5 * (h + h.T)).min())


def test_hessian_against_differences_of_the_reference(hff):
    """H = d2c/ds2 against central differences of fe.mean_Q.  Tolerance per entry: the scheme's own error estimate |D(h) - D(2h)| (three
    times the leading truncation term of D(h)) plus the reference's 1e-13 over h, twice; H symmetric by construction (six numbers),
    eigenvalues >= 0 to rounding (1e-15 of the largest)."""
    S = np.array(S_CHECK)
    m, H = hessian(hff, S)
    for b, s in enumerate(S):
        want, err = reference_hessian(s)
        got = full(H[b])
        excess = np.abs(got - want) - err
        print(s, "max |H - D| = %.3g, allowed there %.3g" % (np.abs(got - want).max(), err.flat[np.abs(got - want).argmax()]))
        assert (excess <= 0).all(), (s, got, want, err)
        lam = np.linalg.eigvalsh(got)
        assert lam.min() >= -1e-15 * lam.max(), (s, lam)
        assert np.abs(m[b] - fe.mean_Q(s)).max() <= 1e-9
    assert np.allclose(full(H[0]), np.eye(3) / 3.0, rtol=0, atol=1e-15)          # Haar: Cov(Q_ii, Q_jj) = delta_ij / 3


def _round_trip_rows():
    _, s_edge, _ = fe.proper_svd64(fe.EDGE_STACK)
    S = np.concatenate([np.array(S_CHECK), s_edge])
    return S, [str(s) for s in S_CHECK] + fe.EDGE_NAMES


def test_round_trip_residual_and_s(hff):
    """s -> d = fe.mean_Q(s) -> fit: |fe.mean_Q(s_fit) - d|_inf <= RESIDUAL and |s_fit - s|_inf <= RESIDUAL / lambda_min(H_ref), per row."""
    S, names = _round_trip_rows()
    D = np.array([fe.mean_Q(s) for s in S])
    s_fit, H, it, st = solve(hff, D, cap=CAP_ROUND_TRIP)
    worst = 0.0
    for b, name in enumerate(names):
        res = np.abs(fe.mean_Q(s_fit[b]) - D[b]).max()
        lam = lambda_min_ref(S[b])
        worst = max(worst, res)
        print("%-28s iterations %2d residual %.3g |ds| %.3g lambda_min %.3g" % (name, it[b], res, np.abs(s_fit[b] - S[b]).max(), lam))
        assert st[b] == 0, (name, st[b])
        assert res <= RESIDUAL, (name, res)
        assert np.abs(s_fit[b] - S[b]).max() <= RESIDUAL / lam, (name, s_fit[b], S[b], lam)
        slack = 1e-13 * max(1.0, s_fit[b, 0])          # s follows d's order, and mean_Q orders equal values only up to rounding
        assert s_fit[b, 0] >= s_fit[b, 1] - slack and s_fit[b, 1] >= abs(s_fit[b, 2]) - slack
    print("largest residual %.3g (RESIDUAL = %.3g), most iterations %d" % (worst, RESIDUAL, it.max()))
    assert it.max() <= hff.hff_max_iter() // 2


def _matrices():
    rng = np.random.default_rng(20261018)
    edge = [(n, a) for n, a in fe.EDGE_A]
    rand = [("rand%d" % i, rng.standard_normal((3, 3)) * 10.0 ** rng.uniform(-3, 2)) for i in range(300)]
    return edge + rand


def test_full_matrices_round_trip(hff):
    """A -> M = U diag(mean_Q(s)) V^T in fp64 -> fit.  A_fit against A entrywise at 4 fp32 ulps of s0 plus the s gate propagated through
    U, V: |dA_ij| <= sum_k |U_ik| |V_jk| |ds_k| <= 3 max_k |ds_k| <= 3 RESIDUAL / lambda_min(H_ref).  U and V are not unique where
    singular values repeat, so A is compared and not the factors."""
    items = _matrices()
    A = np.stack([a for _, a in items])
    U, s, V = fe.proper_svd64(A)
    M = np.stack([U[b] @ np.diag(fe.mean_Q(s[b])) @ V[b].T for b in range(len(A))])
    A_fit, s_fit, H, it, st = fit(hff, M, cap=CAP_ROUND_TRIP)
    worst = 0.0
    for b, (name, a) in enumerate(items):
        lam = lambda_min_ref(s[b])
        tol = 4 * EPS32 * s[b, 0] + 3 * RESIDUAL / lam
        err = np.abs(A_fit[b] - a).max()
        worst = max(worst, err / tol)
        assert st[b] == 0, (name, st[b])
        assert err <= tol, (name, err, tol, s[b])
    print("worst |A_fit - A| / tolerance = %.3g over %d matrices, most iterations %d" % (worst, len(items), it.max()))


def test_fit_is_a_maximiser(hff):
    """l(A) = tr(A^T M) - log c(A) by the reference: l(A_fit) >= l(A_fit + delta) for fixed perturbations of relative size 1e-3 and 1e-2
    (18 single entries, both signs), up to the 1e-12 the reference's log_c resolves."""
    names = ("rank2_rot", "diag441", "diag51m1", "signed_perm", "rand32_0", "2rot")
    for name in names:
        a = fe.EDGE_STACK[fe.EDGE_NAMES.index(name)]
        U, s, V = fe.proper_svd64(a)
        M = U[0] @ np.diag(fe.mean_Q(s[0])) @ V[0].T
        A_fit = fit(hff, M)[0][0]

        def ell(x):
            return float((x * M).sum() - fe.log_c(fe.proper_svd64(x)[1][0]))
        base = ell(A_fit)
        for scale in (1e-3, 1e-2):
            for k in range(9):
                for sign in (1.0, -1.0):
                    d = np.zeros(9)
                    d[k] = sign * scale * s[0, 0]
                    assert base >= ell(A_fit + d.reshape(3, 3)) - 1e-12 * max(1.0, abs(base)), (name, scale, k, sign)


def test_status_bits(hff):
    eps = 1e-12
    s, H, it, st = solve(hff, [(1.0, 1.0, 1.0), (1.0 - eps, -(1.0 - eps), -(1.0 - eps)), (1.0, 0.0, 0.0)])
    assert (st == CAPPED).all(), st
    assert np.isfinite(s).all() and np.isfinite(H).all()
    assert (np.abs(s).max(-1) == 1e4).all(), s
    assert np.array_equal(s[0], [1e4, 1e4, 1e4]) and s[1, 0] == 1e4 and s[1, 1] < 0 and s[1, 2] < 0
    with np.errstate(all="ignore"):
        s, H, it, st = solve(hff, [(1.2, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.5, np.inf, 0.0)])
    assert (st == INPUT).all() and np.isnan(s).all() and np.isnan(H).all()
    A, s, H, it, st = fit(hff, np.zeros((1, 3, 3)))
    assert st[0] == 0 and it[0] == 0 and (A == 0).all() and (s == 0).all()
    with np.errstate(all="ignore"):
        A, s, H, it, st = fit(hff, np.stack([np.full((3, 3), np.nan), 1.2 * np.eye(3)]))
    assert (st == INPUT).all() and np.isnan(A).all()
    # one rotation as the moment (a single sample): capped, finite, A = cap * R
    R = fe.uniform_rotations64(1, seed=5)[0]
    A, s, H, it, st = fit(hff, R[None])
    assert st[0] == CAPPED and np.isfinite(A).all() and np.abs(A[0] - 1e4 * R).max() <= 1e-6
    # an iteration cap of 1 is not enough from the start point for a generic moment
    d = fe.mean_Q((5.0, 3.0, 1.0))
    s1, _, it1, st1 = solve(hff, [d], max_iter=1)
    assert st1[0] == NOT_CONVERGED and it1[0] == 1 and np.isfinite(s1).all()
    # the default cap: a maximiser beyond it is capped at it, ordered
    s2, _, _, st2 = solve(hff, [fe.mean_Q((3e4, 2e4, 1e4))])
    assert st2[0] == CAPPED and s2[0, 0] == 1e4 and s2[0, 0] >= s2[0, 1] >= abs(s2[0, 2])


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_fisher_fit.cpp (its own main: round trips, full matrices, every status path) built with
    the host-side address and undefined-behaviour sanitizers (-Xarch_host: host code only, nothing for the GPU) and run as a process of
    its own: no report, exit code 0."""
    exe = str(tmp_path / "sanitize_fisher_fit")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_fisher_fit.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)
