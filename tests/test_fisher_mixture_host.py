"""CPU: the host build of csrc/fisher_mixture.h -- EM for mixtures of matrix-Fishers, adding in the order of the device kernels --
against the numpy reference of one EM step in tests/fisher_mixture.py (its docstring derives SUM_TOL, L_TOL, H_TOL and OFFSET_GATE), and
the properties EM must have: K = 1 is the moment + fit path bit for bit, a monotone likelihood, stationarity at convergence, chaining,
empty components, grouping, NaN groups, the C ABI's refusals and the four-symmetric-modes density of
tests/test_gpu_grid_modes.py::test_four_symmetric_modes_share_the_mass on a CPU-generated level-3 grid.

The checks are written as functions of a ``fit`` callable with the signature of ``host_fit`` so that tests/test_gpu_fisher_mixture.py
runs the same checks on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rotationnormflow_amd import _lib, synth
from tests import fisher_exact as fe
from tests import fisher_mixture as fm
from tests.test_fisher_fit_host import CAPPED, INPUT, RESIDUAL

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_fisher_mixture.cpp")
OUT = os.path.join(HERE, "csrc", "_host_fisher_mixture.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f)
        for f in ("fisher_mixture.h", "fisher_fit.h", "fisher_exact.h", "fisher_math.h")]
EMPTY = 8


def _host_lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    return C.CDLL(OUT)


@pytest.fixture(scope="module")
def hfm():
    return _host_lib()


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_fit(R, lw, A_init, log_pi_init=None, iterations=1, tol=0.0, cap=1e4, log_resp=True):
    """R [G,n,3,3], or [n,3,3] shared by the G rows of lw [G,n] (lw None: G groups with w = 1/n); A_init [G,K,3,3] ->
    dict(A [G,K,3,3] f32, log_pi [G,K], s [G,K,3], loglik [G,T+1], weight_entropy [G], log_resp [G,K,n] f32, status [G,K], iterations [G])"""
    h = _host_lib()
    R = np.ascontiguousarray(R, np.float32)
    lw = None if lw is None else np.ascontiguousarray(np.atleast_2d(lw), np.float32)
    shared = R.ndim == 3 and lw is not None
    R4 = R if R.ndim == 4 else R[None]
    G, n = (lw.shape[0] if shared else R4.shape[0]), R4.shape[1]
    A_init = np.ascontiguousarray(A_init, np.float32).reshape(G, -1, 3, 3)
    K = A_init.shape[1]
    lp0 = None if log_pi_init is None else np.ascontiguousarray(log_pi_init, np.float64).reshape(G, K)
    out = dict(A=np.empty((G, K, 3, 3), np.float32), log_pi=np.empty((G, K)), s=np.empty((G, K, 3)), loglik=np.empty((G, iterations + 1)),
               weight_entropy=np.empty(G), log_resp=np.empty((G, K, n), np.float32) if log_resp else None,
               status=np.empty((G, K), np.int32), iterations=np.empty(G, np.int32))
    h.hfm_fit(G, int(shared), K, ptr(R4), ptr(lw), C.c_longlong(n), int(iterations), C.c_double(tol), C.c_double(cap), ptr(A_init), ptr(lp0),
              ptr(out["A"]), ptr(out["log_pi"]), ptr(out["s"]), ptr(out["loglik"]), ptr(out["weight_entropy"]), ptr(out["log_resp"]),
              ptr(out["status"]), ptr(out["iterations"]))
    return out


def host_sums(hfm, R, lw, A, log_pi):
    """One group's E-step on the host: (c [K], W [K] = Wu / Z, S [K,3,3] = Su / Z, L, weight_entropy as the kernel forms them)."""
    R = np.ascontiguousarray(R, np.float32)
    A = np.ascontiguousarray(A, np.float32)
    K, n = A.shape[0], R.shape[0]
    lw = None if lw is None else np.ascontiguousarray(lw, np.float32)
    c, sums = np.empty(K), np.empty(10 * K + 3)
    hfm.hfm_sums(K, ptr(R), ptr(lw), C.c_longlong(n), ptr(A), ptr(np.ascontiguousarray(log_pi, np.float64)), ptr(c), ptr(sums), None)
    per, Z = sums[:10 * K].reshape(K, 10), sums[10 * K]
    went = np.log(Z) - (sums[10 * K + 2] / Z if lw is not None else 0.0)
    return c, per[:, 9] / Z, per[:, :9].reshape(K, 3, 3) / Z, sums[10 * K + 1] / Z, went


# ---- cases -----------------------------------------------------------------------------------------------------------------------------

def make_case(n, K, seed, G=1, sigma=0.3):
    """Uniform rotations [G,n,3,3] (fp32), log-weights of a known K-component mixture per group, and a perturbed start."""
    rng = np.random.default_rng(1000 * seed + 10 * n + K)
    R = synth.uniform_rotations(G * n, seed=seed + n).astype(np.float32).reshape(G, n, 3, 3)
    rot = fe.uniform_rotations64(G * K, seed=seed + 7).reshape(G, K, 3, 3)
    A_true = rng.uniform(2.0, 12.0, (G, K, 1, 1)) * rot
    pi_true = rng.dirichlet(np.full(K, 4.0), G)
    lw = np.stack([fm.mixture_log_weights(R[g], A_true[g], pi_true[g]) for g in range(G)])
    A_init = (A_true + sigma * rng.standard_normal((G, K, 3, 3))).astype(np.float32)
    log_pi_init = np.log(rng.dirichlet(np.full(K, 4.0), G))
    return dict(R=R, lw=lw, A_true=A_true, pi_true=pi_true, A_init=A_init, log_pi_init=log_pi_init)


def fitted_mean(M, s):
    """U diag(mean_Q(s)) V^T with U, V of the reference's proper SVD of the moment M and the fp64 s a fit returned."""
    U, _, V = fe.proper_svd64(M)
    return U[0] @ np.diag(fe.mean_Q(s)) @ V[0].T


def host_c(A):
    """c of fp32 parameter matrices [K,3,3] by the host build of the kernels' rule (proper singular values, 64 lane sums, butterfly)."""
    A = np.ascontiguousarray(A, np.float32).reshape(-1, 3, 3)
    c = np.empty(len(A))
    _host_lib().hfm_c(ptr(A), len(A), ptr(c))
    return c


def check_one_step(fit, n, K, sums=None):
    """One EM iteration of one group against the numpy reference, on the gates of tests/fisher_mixture.py.  The rule's c is held to
    ``fe.log_c`` at OFFSET_GATE on its own; the reference E-step is then evaluated AT the rule's c (the host build's; the device's differs
    from it by fma contraction only, a few EPS |c|, inside the 41 LAM EPS counted for l), so W, S, L and -E are held to the counted
    rounding bounds alone and the fit to RESIDUAL.  ``sums``: None, or a callable (R, lw, A, log_pi) -> (c, W, S, L, weight_entropy)
    exposing the E-step sums themselves (the host build)."""
    case = make_case(n, K, seed=3)
    R, lw, A0, lp0 = case["R"][0], case["lw"][0], case["A_init"][0], case["log_pi_init"][0]
    c0, log_c0 = host_c(A0), fm.log_c_of(A0)
    assert np.abs(c0 - log_c0).max() <= fm.offset_gate(log_c0)
    ref = fm.e_step(R, lw, A0, lp0, c=c0)
    lam = fm.lam_of(A0, lp0, c0)
    tol_sum, tol_L = fm.sum_tol(K, lam), fm.l_tol(K, lam)
    d = lw.astype(np.float64) - float(lw.max())
    tol_H = fm.h_tol(n, float(np.abs(d[np.isfinite(d)]).max()))
    if sums is not None:
        c, W, S, L, went = sums(R, lw, A0, lp0)
        print("n %d K %d: |c - log_c| %.3g (gate %.3g), |W - ref| %.3g, |S - ref| %.3g (gate %.3g), |L - ref| %.3g (gate %.3g), |H - ref| %.3g "
              "(gate %.3g)" % (n, K, np.abs(c - log_c0).max(), fm.offset_gate(log_c0), np.abs(W - ref["W"]).max(), np.abs(S - ref["S"]).max(),
                               tol_sum, abs(L - ref["L"]), tol_L, abs(went - ref["weight_entropy"]), tol_H))
        assert np.array_equal(c, c0)
        assert np.abs(W - ref["W"]).max() <= tol_sum and np.abs(S - ref["S"]).max() <= tol_sum
        assert abs(L - ref["L"]) <= tol_L and abs(went - ref["weight_entropy"]) <= tol_H
    out = fit(R[None], lw[None], A0[None], lp0[None], iterations=1)
    assert out["iterations"][0] == 1 and np.isfinite(out["loglik"][0]).all()
    assert abs(out["loglik"][0, 0] - ref["L"]) <= tol_L and abs(out["weight_entropy"][0] - ref["weight_entropy"]) <= tol_H
    # log_pi_out = log(W_k): d(log W) = dW / W, and the log itself rounds (4 ulps)
    assert (np.abs(out["log_pi"][0] - np.log(ref["W"])) <= tol_sum / ref["W"] + 8 * fm.EPS * np.maximum(1.0, np.abs(np.log(ref["W"])))).all()
    worst = 0.0
    for k in range(K):
        st, s = out["status"][0, k], out["s"][0, k]
        if st & CAPPED:
            assert st == CAPPED and np.abs(s).max() == 1e4
            continue
        assert st == 0, (k, st)
        res = np.abs(fitted_mean(ref["M"][k], s) - ref["M"][k]).max()
        worst = max(worst, res)
        assert res <= RESIDUAL, (k, res)
        # and A (fp32) is U diag(s) V^T rounded, |dA_ij| <= 2^-24 s0: its singular values move by at most |dA|_F <= 3 x 2^-24 s0 (Weyl;
        # twice that where the sign of a vanishing s2 flips), its mean rotation by sum_kl |Cov(R_ij, R_kl)| |dA_kl| <= 9 x 2^-24 s0
        A64, s0 = out["A"][0, k].astype(np.float64), max(1.0, np.abs(s).max())
        assert np.abs(fe.proper_svd64(A64)[1][0] - s).max() <= 6 * 2.0 ** -24 * s0
        assert np.abs(fm.mean_rotation(A64) - ref["M"][k]).max() <= 9 * 2.0 ** -24 * s0 + RESIDUAL
    print("n %d K %d: largest |U diag(mean_Q(s_k)) V^T - M_k| %.3g (RESIDUAL %.3g)" % (n, K, worst, RESIDUAL))
    # the final pass: L under the new parameters and the log-responsibilities, against the reference on the outputs at the rule's c
    c1 = host_c(out["A"][0])
    new = fm.e_step(R, lw, out["A"][0], out["log_pi"][0], c=c1)
    assert abs(out["loglik"][0, 1] - new["L"]) <= fm.l_tol(K, fm.lam_of(out["A"][0], out["log_pi"][0], c1))
    if out["log_resp"] is not None:                                     # fp32 outputs of fp64 values
        lr, want = out["log_resp"][0].T.astype(np.float64), new["log_resp"]
        assert (np.abs(lr - want) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want))).all()


def check_k1(fit, moments_fit, n, weighted):
    """K = 1, one iteration: A, s and status of the moment + fit path, bit for bit; log_pi = 0, every log-responsibility 0."""
    case = make_case(n, 1, seed=5)
    R, lw = case["R"][0], case["lw"][0] if weighted else None
    out = fit(R[None], None if lw is None else lw[None], case["A_init"], None, iterations=1)
    A, s, st = moments_fit(R, lw)
    assert np.array_equal(out["A"][0, 0], A) and np.array_equal(out["s"][0, 0], s) and out["status"][0, 0] == st
    assert out["log_pi"][0, 0] == 0.0 and (out["log_resp"][0] == 0.0).all() and out["iterations"][0] == 1


def three_component_case(n=1500):
    case = make_case(n, 3, seed=11, sigma=1.0)
    return case["R"][0], case["lw"][0], case["A_init"][0], case["log_pi_init"][0]


def two_cluster_case(m=100):
    """m copies each of two rotations 120 degrees apart: both components collapse onto a point and are capped."""
    r = fe.uniform_rotations64(1, seed=21)[0]
    turn = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    R = np.concatenate([np.repeat(r[None], m, 0), np.repeat((r @ turn)[None], m, 0)]).astype(np.float32)
    A0 = np.stack([3.0 * r, 3.0 * r @ turn]).astype(np.float32)
    return R, None, A0, None


def check_monotone(fit):
    T = 30
    R, lw, A0, lp0 = three_component_case()
    out = fit(R[None], lw[None], A0[None], lp0[None], iterations=T, tol=0.0)
    L = out["loglik"][0]
    assert out["iterations"][0] == T and np.isfinite(L).all()
    assert (L[1:] >= L[:-1] - 1e-12 * np.maximum(1.0, np.abs(L[:-1]))).all(), np.diff(L)
    assert L[-1] > L[0]
    R, lw, A0, lp0 = two_cluster_case()
    out = fit(R[None], None, A0[None], None, iterations=T, tol=0.0)
    L = out["loglik"][0]
    assert np.isfinite(L).all() and (L[1:] >= L[:-1] - 1e-12 * np.maximum(1.0, np.abs(L[:-1]))).all(), np.diff(L)
    assert (out["status"][0] == CAPPED).all() and np.isfinite(out["A"]).all() and np.isfinite(out["s"]).all()
    assert (np.abs(out["s"][0]).max(-1) == 1e4).all()
    # a responsibility that underflows is an exact zero: each component owns its cluster's weight exactly, 100 / 200
    assert np.array_equal(out["log_pi"][0], np.log([0.5, 0.5]))
    lr = out["log_resp"][0].astype(np.float64)
    m = R.shape[0] // 2
    assert (lr[0, :m] == 0).all() and (lr[1, m:] == 0).all() and np.isfinite(lr).all()
    assert (np.exp(lr[0, m:]) == 0).all() and (np.exp(lr[1, :m]) == 0).all()


def separated_case(n=3000):
    """Three sharp components (concentration 40) about rotations >= 90 degrees apart, uniform rows weighted by the mixture's density."""
    base = fe.uniform_rotations64(1, seed=33)[0]
    turns = [np.eye(3), np.diag([1.0, -1.0, -1.0]), np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])]
    A_true = np.stack([40.0 * base @ t for t in turns])
    R = synth.uniform_rotations(n, seed=34).astype(np.float32)
    lw = fm.mixture_log_weights(R, A_true, [0.5, 0.3, 0.2])
    A0 = (0.5 * A_true).astype(np.float32)
    return R, lw, A0, np.log([1 / 3, 1 / 3, 1 / 3])


def check_stationarity(fit):
    """At reported convergence (tol = 1e-12): with M_k the moments the last M-step fitted (reference E-step on the parameters before
    that M-step) and M_k' those of a reference E-step on the outputs, |E_{A_k}[R] - M_k'|_inf <= RESIDUAL + |M_k' - M_k|_inf and
    |M_k' - M_k|_inf <= 1e-8.  E_{A_k}[R] = U diag(mean_Q(s_k)) V^T with the fp64 s_k of the outputs and U, V of M_k (the fp32 A_k itself
    is 4 ulps of s0 away from that, which moves E[R] by more than RESIDUAL)."""
    R, lw, A0, lp0 = separated_case()
    out = fit(R[None], lw[None], A0[None], lp0[None], iterations=256, tol=1e-12)
    T = int(out["iterations"][0])
    L = out["loglik"][0]
    print("converged after %d iterations, last gains %s" % (T, np.diff(L[max(0, T - 3):T + 1])))
    assert 2 <= T < 256 and np.isfinite(L[:T + 1]).all() and np.isnan(L[T + 1:]).all()
    assert 0 <= L[T] - L[T - 1] <= 1e-12 and (out["status"][0] == 0).all()
    # the run stopped at iteration T without an M-step there: its outputs are the parameters after T M-steps (iterations 0..T-1), and
    # the last of them fitted the E-step sums under the parameters after T - 1 M-steps, i.e. the outputs of a run of T - 1 iterations
    before = fit(R[None], lw[None], A0[None], lp0[None], iterations=T - 1, tol=0.0)
    prev = fm.e_step(R, lw, before["A"][0], before["log_pi"][0])["M"]
    new = fm.e_step(R, lw, out["A"][0], out["log_pi"][0])["M"]
    for k in range(3):
        change = np.abs(new[k] - prev[k]).max()
        gap = np.abs(fitted_mean(prev[k], out["s"][0, k]) - new[k]).max()
        print("component %d: change of M over the last iteration %.3g, |E[R] - M'| %.3g" % (k, change, gap))
        assert change <= 1e-8 and gap <= RESIDUAL + change


def check_chaining(fit, n=700, T=5):
    case = make_case(n, 3, seed=13, sigma=1.0)
    R, lw, A, lp = case["R"], case["lw"], case["A_init"], case["log_pi_init"]
    whole = fit(R, lw, A, lp, iterations=T, tol=0.0)
    trace = []
    for t in range(T):
        one = fit(R, lw, A, lp, iterations=1, tol=0.0)
        A, lp = one["A"], one["log_pi"]
        trace.append(one["loglik"][0, 0])
    trace.append(one["loglik"][0, 1])
    for k in ("A", "log_pi", "s", "status", "log_resp", "weight_entropy"):
        assert np.array_equal(whole[k], one[k]), k
    assert np.array_equal(whole["loglik"][0], np.array(trace))


def check_empty(fit, n=600, T=4):
    case = make_case(n, 3, seed=17, sigma=1.0)
    R, lw, A, lp = case["R"], case["lw"], case["A_init"], case["log_pi_init"].copy()
    lp[0, 1] = -np.inf
    three = fit(R, lw, A, lp, iterations=T, tol=0.0)
    live = [0, 2]
    two = fit(R, lw, A[:, live], lp[:, live], iterations=T, tol=0.0)
    for k in ("A", "log_pi", "s", "status", "log_resp"):
        assert np.array_equal(three[k][:, live], two[k]), k
    assert np.array_equal(three["loglik"], two["loglik"]) and np.array_equal(three["weight_entropy"], two["weight_entropy"])
    assert three["status"][0, 1] == EMPTY and three["log_pi"][0, 1] == -np.inf and np.array_equal(three["A"][0, 1], A[0, 1])
    assert (three["log_resp"][0, 1] == -np.inf).all()


def check_grouping(fit, n, T=2):
    G = 3
    case = make_case(n, 2, seed=19, G=G, sigma=1.0)
    R, lw, A, lp = case["R"], case["lw"], case["A_init"], case["log_pi_init"]
    keys = ("A", "log_pi", "s", "status", "log_resp", "loglik", "weight_entropy", "iterations")
    together = fit(R, lw, A, lp, iterations=T)
    for g in range(G):
        alone = fit(R[g:g + 1], lw[g:g + 1], A[g:g + 1], lp[g:g + 1], iterations=T)
        for k in keys:
            assert np.array_equal(together[k][g:g + 1], alone[k]), (k, g)
    plain = fit(R, None, A, lp, iterations=T)
    alone = fit(R[1:2], None, A[1:2], lp[1:2], iterations=T)
    for k in keys:
        assert np.array_equal(plain[k][1:2], alone[k]), k
    shared = fit(R[0], lw, A, lp, iterations=T)
    copied = fit(np.repeat(R[:1], G, 0), lw, A, lp, iterations=T)
    for k in keys:
        assert np.array_equal(shared[k], copied[k]), k


def check_nan_groups(fit, n):
    G, K = 3, 2
    case = make_case(n, K, seed=23, G=G)
    R, lw, A, lp = case["R"], case["lw"], case["A_init"], case["log_pi_init"]
    good = fit(R, lw, A, lp, iterations=2)
    keys = ("A", "log_pi", "s", "loglik", "weight_entropy", "log_resp")

    def only_group_is_nan(out, g):
        for k in keys:
            assert np.isnan(out[k][g]).all(), (k, g)
        assert (out["status"][g] == INPUT).all()
        for h in range(G):
            if h != g:
                for k in keys + ("status", "iterations"):
                    assert np.array_equal(out[k][h], good[k][h]), (k, h)

    dead = lw.copy()
    dead[2] = -np.inf
    only_group_is_nan(fit(R, dead, A, lp, iterations=2), 2)
    bad = R.copy()
    bad[0, n - 1, 1, 1] = np.nan
    with np.errstate(invalid="ignore"):
        only_group_is_nan(fit(bad, lw, A, lp, iterations=2), 0)
    none = lp.copy()
    none[1] = -np.inf
    only_group_is_nan(fit(R, lw, A, none, iterations=2), 1)


# ---- the tests -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 255, 257, 4097])
def test_one_step_against_the_reference(hfm, n, K):
    """n = 1, either side of the 256-row tile and across a chunk boundary; K = 1, 2, 3 and the largest, 8."""
    check_one_step(host_fit, n, K, sums=lambda *a: host_sums(hfm, *a))


def test_singular_values_are_those_of_proper_svd3_bit_for_bit(hfm):
    """proper_singular_values3 (selects instead of indexed loads) against proper_svd3's s on the edge list, 2000 random matrices at scales
    1e-3..1e4 and their fp32 roundings."""
    rng = np.random.default_rng(7)
    A = np.concatenate([fe.EDGE_STACK, rng.standard_normal((2000, 3, 3)) * 10.0 ** rng.uniform(-3, 4, (2000, 1, 1))])
    A = np.ascontiguousarray(np.concatenate([A, A.astype(np.float32).astype(np.float64)]))
    s, want = np.empty((len(A), 3)), np.empty((len(A), 3))
    hfm.hfm_singular_values(ptr(A), len(A), ptr(s), ptr(want))
    assert np.array_equal(s, want)


def host_moments_fit(R, lw, cap=1e4):
    h = _host_lib()
    R = np.ascontiguousarray(R, np.float32)
    lw = None if lw is None else np.ascontiguousarray(lw, np.float32)
    M, A, s, st = np.empty(9), np.empty((3, 3), np.float32), np.empty(3), np.empty(1, np.int32)
    h.hfm_moments_fit(ptr(R), ptr(lw), C.c_longlong(R.shape[0]), C.c_double(cap), ptr(M), ptr(A), ptr(s), ptr(st))
    return A, s, int(st[0])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 4097])
def test_one_component_is_the_moment_and_fit_path_bit_for_bit(hfm, n, weighted):
    check_k1(host_fit, host_moments_fit, n, weighted)


def test_likelihood_is_monotone(hfm):
    check_monotone(host_fit)


def test_stationarity_at_convergence(hfm):
    check_stationarity(host_fit)


def test_iterations_chain(hfm):
    check_chaining(host_fit)


def test_an_empty_component_changes_nothing(hfm):
    check_empty(host_fit)


def test_grouping_does_not_matter(hfm):
    check_grouping(host_fit, 257)


def test_nan_groups(hfm):
    check_nan_groups(host_fit, 257)


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20


def _args(**kw):
    base = dict(rotations=_FAKE, log_weights=_FAKE, n=4608, G=3, shared_rotations=1, K=4, A_init=_FAKE, iterations=8, tol=1e-9,
                max_concentration=1e4, A_out=_FAKE, log_pi_out=_FAKE, loglik_out=_FAKE, status_out=_FAKE, iterations_out=_FAKE)
    base.update(kw)
    a = _lib.FisherMixtureFit(**base)
    a.workspace, a.workspace_bytes = _FAKE, _lib.lib().rnf_fisher_mixture_fit_workspace_bytes(C.byref(a))
    return a


def _refused(a, word):
    L = _lib.lib()
    assert L.rnf_fisher_mixture_fit(C.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def test_c_abi_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    a = _args()
    assert a.workspace_bytes == 8 * (3 * 2 * (10 * 4 + 14) + 3 * 4 + 3)
    _refused(_args(K=0), "K=")
    _refused(_args(K=9), "K=")
    _refused(_args(iterations=0), "iterations")
    _refused(_args(iterations=257), "iterations")
    _refused(_args(G=0), "G=")
    _refused(_args(n=0), "n=")
    _refused(_args(tol=-1.0), "tol")
    _refused(_args(max_concentration=0.0), "max_concentration")
    _refused(_args(max_concentration=3.1e4), "max_concentration")
    _refused(_args(A_init=None), "null")
    _refused(_args(log_weights=None), "shared_rotations")
    a = _args()
    a.workspace_bytes -= 1
    _refused(a, "workspace")
    a = _args()
    a.struct_bytes += 8
    _refused(a, "struct_bytes")
    assert L.rnf_fisher_mixture_fit_workspace_bytes(C.byref(a)) == 0
    for bad in (dict(K=0), dict(K=9), dict(iterations=0)):
        assert L.rnf_fisher_mixture_fit_workspace_bytes(C.byref(_lib.FisherMixtureFit(n=10, G=1, **{**dict(K=1, iterations=1), **bad}))) == 0
    assert L.rnf_fisher_mixture_log_prob(_FAKE, _FAKE, 0, _FAKE, 10, _FAKE, None, None) != 0
    assert L.rnf_fisher_mixture_log_prob(_FAKE, _FAKE, 9, _FAKE, 10, _FAKE, None, None) != 0


def test_header_declares_the_struct_the_binding_mirrors():
    import re
    header = open(os.path.join(os.path.dirname(HERE), "include", "rnf_hip.h")).read()
    body = header[header.index("typedef struct RnfFisherMixtureFit {") + 36:header.index("} RnfFisherMixtureFit;")]
    names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
    assert names == [f for f, _ in _lib.FisherMixtureFit._fields_], names
    assert {"rnf_fisher_mixture_fit", "rnf_fisher_mixture_fit_workspace_bytes", "rnf_fisher_mixture_log_prob"} <= set(_lib.EXPORTS)


# ---- four symmetric modes ----------------------------------------------------------------------------------------------------------------

SYM = np.stack([np.eye(3), np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])])


def four_mode_case(grid32):
    """The density 1/4 sum_j MF(16 G_j) of tests/test_gpu_grid_modes.py::test_four_symmetric_modes_share_the_mass on the rows grid32:
    (log-weights fp32, the truth's A [4,3,3] fp32 and log_pi, log_norm = log mean_i p(R_i))."""
    A = (16.0 * SYM).astype(np.float32)
    lp = fm.log_prob(grid32, A, np.log(np.full(4, 0.25)))
    lw = lp.astype(np.float32)
    log_norm = float(np.log(np.mean(np.exp(lw.astype(np.longdouble)))))
    return lw, A, np.log(np.full(4, 0.25)), log_norm


def kl_of(out, Q):
    """kl = log Q - weight_entropy - L of the last used entry, per group."""
    L = np.array([out["loglik"][g, out["iterations"][g]] for g in range(len(out["iterations"]))])
    return np.log(Q) - out["weight_entropy"] - L


def modes_init(grid32, lw, K, separation_deg):
    """The start of MatrixFisherMixture.fit from the numpy restatement of rnf_grid_modes: A_k = kappa0 R_k, kappa0 = 2 / separation^2,
    log_pi_k = log of the normalised mode mass."""
    from tests.test_grid_modes_host import grid_modes_fp64
    sep = float(np.deg2rad(separation_deg))
    modes = grid_modes_fp64(lw, grid32, K, sep)
    idx, mass = modes["index"][0], modes["mass"][0]
    A = (2.0 / sep ** 2 * grid32[np.maximum(idx, 0)].astype(np.float64)).astype(np.float32)
    with np.errstate(divide="ignore"):
        lp = np.where(idx >= 0, np.log(mass / mass[idx >= 0].sum()), -np.inf)
    return A, lp


# K = 1 on this density: the grid moment is 0 up to rounding, so A ~ 0, L ~ 0 and kl = log Q - weight_entropy, the negative entropy of
# the grid posterior w.r.t. Haar; tests/fisher_mixture.py computes 3.89892 nats for it on the level-3 grid.
FOUR_MODE_K1_KL = 3.89892
# measured on the host build: the run started from the modes ends exactly 0.0 nats above the run started at the truth (both reach the
# same fp32 A and the same log_pi).  Twice that is 0, so the gate is what kl = log Q - H - L itself resolves in fp64: 8 EPS of the
# three terms' magnitudes (log Q = 10.5, H = 6.6, |L| = 3.9)
FOUR_MODE_EXCESS = 0.0


@pytest.fixture(scope="module")
def level3():
    from tests.test_so3_grid import healpix_grid_fp64
    grid = healpix_grid_fp64(3).astype(np.float32)
    assert grid.shape == (36864, 3, 3)
    return (grid,) + four_mode_case(grid)


def check_four_modes_from_truth(fit, level3):
    grid, lw, A, lp, log_norm = level3
    out = fit(grid, lw[None], A[None], lp[None], iterations=64, tol=1e-10, log_resp=False)
    kl = kl_of(out, len(grid))[0]
    print("four modes from the truth: %d iterations, kl %.6g, the truth's own kl %.6g, weights %s" % (out["iterations"][0], kl, -log_norm,
                                                                                                   np.exp(out["log_pi"][0])))
    assert kl <= -log_norm + 1e-12
    assert np.abs(np.exp(out["log_pi"][0]) - 0.25).max() <= 1e-3
    return kl


def test_four_symmetric_modes_from_the_truth_and_from_the_modes(hfm, level3):
    """Started at the truth (tol = 1e-10) EM can only raise L, so kl <= the truth's own kl = -log_norm (+1e-12), weights within 1e-3 of
    1/4.  Started from the grid's modes (separation 15 degrees, kappa0 = 29.2) it reaches the same optimum in 3 iterations: measured
    excess over the run from the truth 0.0 nats on the host build (kl 0.0280076867 both ways, against the truth's own 0.0284301), gated at
    twice that plus the fp64 resolution of kl (FOUR_MODE_EXCESS above)."""
    grid, lw, A, lp, log_norm = level3
    kl_truth = check_four_modes_from_truth(host_fit, level3)
    A0, lp0 = modes_init(grid, lw, 4, 15.0)
    out = host_fit(grid, lw[None], A0[None], lp0[None], iterations=64, tol=1e-10, log_resp=False)
    kl = kl_of(out, len(grid))[0]
    print("from the modes: %d iterations, kl %.12g, excess over the run from the truth %.3g" % (out["iterations"][0], kl, kl - kl_truth))
    assert kl - kl_truth <= 2 * FOUR_MODE_EXCESS + 8 * fm.EPS * (np.log(len(grid)) + abs(out["weight_entropy"][0]) + abs(out["loglik"][0, out["iterations"][0]]))
    assert np.abs(np.exp(out["log_pi"][0]) - 0.25).max() <= 1e-3


def test_one_component_cannot_describe_four_modes(hfm, level3):
    grid, lw, A, lp, log_norm = level3
    one = host_fit(grid, lw[None], np.zeros((1, 1, 3, 3), np.float32), None, iterations=4, tol=1e-10, log_resp=False)
    four = host_fit(grid, lw[None], A[None], lp[None], iterations=4, tol=1e-10, log_resp=False)
    kl1, kl4 = kl_of(one, len(grid))[0], kl_of(four, len(grid))[0]
    entropy = -fm.e_step(grid, lw, np.zeros((1, 3, 3)), np.zeros(1))["weight_entropy"] + np.log(len(grid))
    print("kl with one component %.6g (the posterior's negative entropy by the reference: %.6g), with four %.6g" % (kl1, entropy, kl4))
    assert np.abs(one["A"]).max() <= 1e-4 and abs(kl1 - entropy) <= 1e-6 and abs(entropy - FOUR_MODE_K1_KL) <= 1e-5
    assert kl1 >= kl4 + 1.0


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_fisher_mixture.cpp (its own main: EM runs over every status path) built with the host-side address and
    undefined-behaviour sanitizers (-Xarch_host: host code only, nothing for the GPU) and run as a process of its own."""
    exe = str(tmp_path / "sanitize_fisher_mixture")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_fisher_mixture.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)
