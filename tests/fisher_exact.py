"""Exact fp64 references for the matrix-Fisher distribution MF(A), density exp(tr(A^T R)) / c(A) w.r.t. the Haar probability measure on
SO(3), built from numpy / scipy only (nothing here follows the sampler's or the kernels' algorithms).

With the proper SVD A = U diag(s) V^T (U, V in SO(3), s0 >= s1 >= |s2|, s2 carrying the sign of det A) and R = U Q V^T, tr(A^T R) = tr(S Q),
so everything is a function of s:
    c(S)      = int_SO(3) exp(tr(S Q)) dQ
              = int_{-1}^{1} 1/2 I0(1/2 (s_i - s_j)(1 - u)) I0(1/2 (s_i + s_j)(1 + u)) exp(s_k u) du      for any permutation (i, j, k)
    E[Q]      = diag(d log c / d s)           (off-diagonal entries vanish by symmetry),  E[R] = U diag(E[Q]) V^T
    Var_unif[exp(tr(A^T R))] = c(2S) - c(S)^2 (the variance of the norm_type-2 Monte-Carlo normaliser, per draw)
The exponential scale of the Bessel functions is factored out (scipy.special.ive), so log c stays finite and accurate to |s| ~ 1e4.
The two closed-form normalisers of the reference (norm_type 0 and 1) are restated in fp64 for the kernels' targets; norm_type 1 is the
Laplace limit of log c (log c - c_type1 = O(1/s)).
"""
import numpy as np
from numpy.polynomial.legendre import leggauss
from scipy.special import ive

# Gauss-Legendre panels on [-1, 1], graded geometrically towards both endpoints: at |s| ~ 1e4 the integrand is a boundary layer of
# width ~1e-4 at one end, elsewhere it is smooth (entire functions of u)
_T = 10.0 ** -np.arange(1, 10)
_EDGES = np.unique(np.concatenate([[-1.0, 0.0, 1.0], -1.0 + _T, 1.0 - _T]))
_X, _W = leggauss(48)
_NODES = np.concatenate([0.5 * (b - a) * _X + 0.5 * (a + b) for a, b in zip(_EDGES[:-1], _EDGES[1:])])
_WEIGHTS = np.concatenate([0.5 * (b - a) * _W for a, b in zip(_EDGES[:-1], _EDGES[1:])])

PERMS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))


def _parts(s, perm):
    """(M, a(u), b(u), exp(E(u) - M)) for the integrand of c with the exponential scales exp(|a| + |b| + s_k u) = exp(E(u)) pulled out;
    E is linear in u, so its maximum M over [-1, 1] sits at an endpoint."""
    s = np.asarray(s, np.float64)
    i, j, k = perm
    u = _NODES
    a = 0.5 * (s[i] - s[j]) * (1.0 - u)
    b = 0.5 * (s[i] + s[j]) * (1.0 + u)
    E = np.abs(a) + np.abs(b) + s[k] * u
    M = max(abs(s[i] + s[j]) + s[k], abs(s[i] - s[j]) - s[k])
    return M, a, b, np.exp(E - M)


def log_c(s, perm=(0, 1, 2)):
    """log c(S), S = diag(s): the exact log-normaliser of MF w.r.t. the Haar probability measure (log_c(0) = 0)."""
    M, a, b, e = _parts(s, perm)
    return M + np.log(np.dot(_WEIGHTS, 0.5 * ive(0, a) * ive(0, b) * e))


def mean_Q(s):
    """E[Q] diagonal = d log c / d s, analytically (I0' = I1, d a / d s_i = (1 - u)/2, d b / d s_i = (1 + u)/2) with permutation (i, j, k)."""
    s = np.asarray(s, np.float64)
    out = np.empty(3)
    for i in range(3):
        perm = (i, (i + 1) % 3, (i + 2) % 3)
        M, a, b, e = _parts(s, perm)
        i0a, i0b = ive(0, a), ive(0, b)
        c = np.dot(_WEIGHTS, 0.5 * i0a * i0b * e)
        dc = np.dot(_WEIGHTS, 0.5 * (0.5 * (1.0 - _NODES) * ive(1, a) * i0b + 0.5 * (1.0 + _NODES) * i0a * ive(1, b)) * e)
        out[i] = dc / c
    return out


def mean_Q_by_u(s):
    """The same derivative along s_k (the exp(s_k u) factor): E[Q_kk] = int u f / int f -- a second route for checking mean_Q."""
    out = np.empty(3)
    for k in range(3):
        _, a, b, e = _parts(s, ((k + 1) % 3, (k + 2) % 3, k))
        f = 0.5 * ive(0, a) * ive(0, b) * e
        out[k] = np.dot(_WEIGHTS, _NODES * f) / np.dot(_WEIGHTS, f)
    return out


def mc_rel_std(s):
    """Relative standard deviation of exp(tr(S Q)) under uniform Q, per draw: sqrt((c(2S) - c(S)^2) / c(S)^2)."""
    return float(np.sqrt(np.expm1(log_c(2.0 * np.asarray(s, np.float64)) - 2.0 * log_c(s))))


def proper_svd64(A):
    """[B,3,3] -> (U, s, V) in fp64 by LAPACK with the reference's sign rule: det U = det V = +1, s2 signed by det U det V."""
    A = np.asarray(A, np.float64).reshape(-1, 3, 3)
    U, s, Vh = np.linalg.svd(A)
    V = np.swapaxes(Vh, -1, -2).copy()
    U, s = U.copy(), s.copy()
    du, dv = np.linalg.det(U), np.linalg.det(V)
    U[:, :, 2] *= du[:, None]
    V[:, :, 2] *= dv[:, None]
    s[:, 2] *= du * dv
    return U, s, V


def log_const_t1(s):
    """norm_type 1: c = sum s - 1/2 log(8 pi (s0+s1)(s1+s2)(s0+s2)), [B,3] -> [B] (+inf where a pair sum is 0, nan where negative)."""
    s = np.asarray(s, np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s.sum(-1) - 0.5 * np.log(8.0 * np.pi * (s[:, 0] + s[:, 1]) * (s[:, 1] + s[:, 2]) * (s[:, 0] + s[:, 2]))


def dlog_const_t1(U, s, V):
    """d c_type1 / dA = U diag(f) V^T, f = d c / d s."""
    s = np.asarray(s, np.float64).reshape(-1, 3)
    p01, p12, p02 = s[:, 0] + s[:, 1], s[:, 1] + s[:, 2], s[:, 0] + s[:, 2]
    f = np.stack([1 - 0.5 * (1 / p01 + 1 / p02), 1 - 0.5 * (1 / p01 + 1 / p12), 1 - 0.5 * (1 / p12 + 1 / p02)], -1)
    return np.einsum("bik,bk,bjk->bij", U, f, V)


def log_const_t0(A):
    """norm_type 0 with the reference's batch-global Q = sum_b |A_b|_F^2: c_b = log(1 + Q/6 + det(A_b)/6), [B,3,3] -> [B]."""
    A = np.asarray(A, np.float64).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore"):
        return np.log(1.0 + (A ** 2).sum() / 6.0 + np.linalg.det(A) / 6.0)


def uniform_rotations64(n, seed):
    """[n,3,3] Haar-uniform rotations in fp64 (normalised Gaussian quaternions)."""
    q = np.random.default_rng(seed).standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)


def _edge_a():
    r = uniform_rotations64(6, seed=91)
    rng = np.random.default_rng(92)
    d321 = r[2] @ np.diag([3.0, 2.0, 1.0]) @ r[3].T
    signed_perm = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])     # det -1; A^T A diagonal: Jacobi exits at once
    out = [
        ("zero", np.zeros((3, 3))),
        ("diag500", np.diag([5.0, 0.0, 0.0])),
        ("rank1", np.outer(rng.standard_normal(3), rng.standard_normal(3)) * 2.0),
        ("rank2_rot", r[0] @ np.diag([5.0, 3.0, 0.0]) @ r[1].T),
        ("2I", 2.0 * np.eye(3)),
        ("2rot", 2.0 * r[4]),
        ("diag441", np.diag([4.0, 4.0, 1.0])),
        ("diag522", np.diag([5.0, 2.0, 2.0])),
        ("diag51m1", np.diag([5.0, 1.0, -1.0])),
        ("diag51m0999", np.diag([5.0, 1.0, -0.999])),
        ("minus3I", -3.0 * np.eye(3)),
        ("diag153", np.diag([1.0, 5.0, 3.0])),
        ("signed_perm", signed_perm @ np.diag([1.0, 4.0, 2.0])),
        ("tiny", 1e-4 * d321),
        ("big1e3", 1e3 * d321),
        ("big1e4", 1e4 * d321 / 3.0),
        ("aniso", r[5] @ np.diag([1e4, 1.0, 1e-3]) @ r[0].T),
    ]
    for t in range(3):
        out.append((f"rand32_{t}", (rng.standard_normal((3, 3)) * 3.0).astype(np.float32).astype(np.float64)))
    return out


# one shared list of parameter matrices at the edges of the proper SVD and the normalisers (fp64, exactly structured)
EDGE_A = _edge_a()
EDGE_NAMES = [n for n, _ in EDGE_A]
EDGE_STACK = np.stack([a for _, a in EDGE_A])
# exact proper singular values with a pair sum of 0: the type-1 normaliser is infinite in the reference (c = +inf)
INF_T1 = {"zero", "diag500", "rank1", "diag51m1", "minus3I"}
# the same, but with the zero pair sum exact in floating point too (the general rank-1 product has it only up to rounding)
INF_T1_EXACT = {"zero", "diag500", "diag51m1", "minus3I"}
