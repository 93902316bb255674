"""numpy fp64 / long-double reference of one EM step of a mixture of matrix-Fishers (csrc/fisher_mixture.h), built on tests/fisher_exact.py
(``log_c``, ``proper_svd64``, ``mean_Q``) only: there is no solver in here.  The M-step is therefore checked as a property
(E_{A_k}[R] = M_k) and not re-run.

Model, w.r.t. the Haar probability measure:   log p(R) = logsumexp_k( log_pi_k + tr(A_k^T R) - c(A_k) ).

Gates (EPS = 2^-53; LAM = max_k(|A_k|_1 + |log_pi_k| + |c_k|) bounds every term of l_ik, |R| <= 1):
  * C_GATE(c) = 1e-10 max(1, |c|) is what tests/test_fisher_exact_host.py allows between the 224-node rule and ``fe.log_c``;
    OFFSET_GATE = 2 C_GATE is the gate on the offset of l_ik (the kernel's c against the reference's).
  * A responsibility r_ik = exp(l_ik - lse_i): l_ik takes 9 products and 9 additions for the trace and 2 more additions, each within
    EPS LAM: 20 EPS LAM.  lse = m + log(sum_k exp(l_ik - m)): K subtractions (EPS LAM each, one per term), K exp at 4 ulps = 8 EPS, K - 1
    additions, a log at 8 EPS |log K| and one addition EPS LAM: d(lse) <= (21 LAM + 9 K + 8 log K + 1) EPS.  r adds a subtraction (EPS
    |log r|, and r |log r| <= 1/e) and an exp (8 EPS): relative to 1, d(r) <= d(l) + d(lse) + 9 EPS = RHO = (41 LAM + 9 K + 8 log K + 10) EPS.
  * A sum over rows in the kernel's order, n <= 64 x 4096 (tests/test_gpu_fisher_fit.py's MOMENT_TOL count): 32 additions, the products
    u r and (u r) R, the exp behind u at 8 EPS: 42 EPS relative to the weight sum, 40 EPS for the denominator Z, one division: 83 EPS.
    The reference evaluates l, lse and r in fp64 too (its sums are long double), so RHO enters twice:
        SUM_TOL = (83 + 2 RHO / EPS) EPS = (103 + 82 LAM + 18 K + 16 log K) EPS.
    The tests hold the rule's c to ``fe.log_c`` at OFFSET_GATE in a check of its own and evaluate this reference AT the rule's c
    (``e_step(..., c=)``), so the sums W_k, S_k (|.| <= 1) are gated at SUM_TOL alone.
  * L = sum_i w_i lse_i, |lse| <= LAM + log K: 83 EPS relative plus d(lse) twice: L_TOL = (125 LAM + 18 K + 100 log K + 2) EPS.
  * -E = -sum_i w_i log w_i = log Z - sum_i u_i d_i / Z, d_i = lw_i - max lw: H_TOL = 128 EPS (1 + log n + max |d_i| over u_i > 0).
"""
import numpy as np

from tests import fisher_exact as fe

EPS = 2.0 ** -53


def c_gate(c):
    return 1e-10 * np.maximum(1.0, np.abs(c))


def offset_gate(c):
    return 2.0 * float(np.max(c_gate(c)))


def log_c_of(A):
    """[K,3,3] -> c [K] by fe.log_c on the fp64 proper singular values."""
    s = fe.proper_svd64(np.asarray(A, np.float64))[1]
    return np.array([fe.log_c(x) for x in s])


def lam_of(A, log_pi, c):
    live = np.isfinite(log_pi)
    A = np.asarray(A, np.float64).reshape(-1, 9)
    return float((np.abs(A).sum(-1) + np.abs(np.where(live, log_pi, 0.0)) + np.abs(c))[live].max())


def sum_tol(K, lam):
    return (103 + 82 * lam + 18 * K + 16 * np.log(K)) * EPS


def l_tol(K, lam):
    return (125 * lam + 18 * K + 100 * np.log(K) + 2) * EPS


def h_tol(n, dmax):
    return 128 * EPS * (1 + np.log(n) + dmax)


def weights(lw32, n):
    """Normalised weights in long double: softmax of the fp32 log-weights, or 1/n."""
    if lw32 is None:
        return np.full(n, 1.0, np.longdouble) / n
    lw = np.asarray(lw32).astype(np.longdouble)
    with np.errstate(invalid="ignore"):
        u = np.exp(lw - lw.max())
    return u / u.sum()


def log_terms(R32, A32, log_pi, c=None):
    """l [n,K] (empty components -inf), lse [n] and log r [n,K] in fp64; c defaults to fe.log_c of the fp32 matrices."""
    R = np.asarray(R32).astype(np.float64).reshape(-1, 9)
    A = np.asarray(A32).astype(np.float64).reshape(-1, 9)
    log_pi = np.asarray(log_pi, np.float64)
    c = log_c_of(A.reshape(-1, 3, 3)) if c is None else np.asarray(c, np.float64)
    live = log_pi != -np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        l = np.where(live[None], (log_pi[None] + R @ A.T) - c[None], -np.inf)
        m = l.max(-1, keepdims=True)
        lse = (m + np.log(np.exp(l - m).sum(-1, keepdims=True)))[:, 0]
        return l, lse, l - lse[:, None]


def e_step(R32, lw32, A32, log_pi, c=None):
    """One E-step: dict(W [K], S [K,3,3], M [K,3,3] = S / W, L, weight_entropy, c [K], log_resp [n,K]) with long-double sums."""
    R = np.asarray(R32).astype(np.longdouble).reshape(-1, 3, 3)
    n = len(R)
    w = weights(lw32, n)
    A = np.asarray(A32).astype(np.float64).reshape(-1, 3, 3)
    c = log_c_of(A) if c is None else np.asarray(c, np.float64)
    l, lse, log_r = log_terms(R32, A32, log_pi, c)
    r = np.exp(log_r).astype(np.longdouble)
    wr = w[:, None] * r
    W = wr.sum(0)
    S = np.einsum("nk,nab->kab", wr, R)
    with np.errstate(invalid="ignore", divide="ignore"):
        M = S / W[:, None, None]
    pos = w > 0
    return dict(W=W.astype(np.float64), S=S.astype(np.float64), M=M.astype(np.float64), L=float((w[pos] * lse[pos].astype(np.longdouble)).sum()),
                weight_entropy=float(-(w[pos] * np.log(w[pos])).sum()), c=c, log_resp=log_r)


def log_prob(R32, A32, log_pi, c=None):
    return log_terms(R32, A32, log_pi, c)[1]


def mean_rotation(A):
    """E_A[R] = U diag(mean_Q(s)) V^T of one fp64 parameter matrix."""
    U, s, V = fe.proper_svd64(np.asarray(A, np.float64))
    return U[0] @ np.diag(fe.mean_Q(s[0])) @ V[0].T


def mixture_log_weights(R32, A, pi):
    """float32 log-density of sum_k pi_k MF(A_k) on the rows R32: the log-weights of 'a known mixture'."""
    return log_terms(R32, np.asarray(A, np.float64), np.log(np.asarray(pi, np.float64)))[1].astype(np.float32)
