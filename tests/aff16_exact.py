"""fp64 reference for the per-sample 4x4 layer Condition16Trans (csrc/so3_math.h cond16_apply, csrc/so3_grad.h cond16_backward), the inputs
on which every sample is judged, the figures, and the LAPACK fp32 yardstick.  No GPU, no pytest.

The layer (flow/squeezetrans.py:33-55), restated from the rule:  q = quat(R) (pytorch3d's four-candidate rule),  t = A q with A = M on the
forward and A = M^-1 on the inverse pass,  R' = rot(t / |t|),  ldj = log|det A| - 4 log|t|.  Both results are of degree 0 in M.

How far rounding may move them is set by the matrix: a perturbation eps |M| of M turns t / |t| by about eps cond(M) in either pass, and
moves log|det M| - 4 log|t| by as much.  An fp32 routine has eps ~ 2^-23, so every figure is an error divided by 2^-23 kappa,
kappa = cond_2(M); |R' R'^T - I| is NOT divided: a rotation is a rotation whatever made it.  Tests gate each figure at twice what
LAPACK's own fp32 route (`lapack32`) shows on the same batch.

GATED DOMAIN (a condition on the input, never a measurement of the routine): finite matrices with cond(M) <= 1e3 whose largest entry
lies in [2^-70, 2^70].  Every batch of `random_batch` lies inside completely (a draw outside is drawn again; the share drawn again is
returned and the tests assert it is under 2 %), and so does every EDGE_M entry not named in OUT_OF_DOMAIN; asserted at the bottom.
"""
import numpy as np
import torch

from oracle import flow_oracle as orc

U23 = 2.0 ** -23
COND_MAX = 1e3
ENTRY_LO, ENTRY_HI = 2.0 ** -70, 2.0 ** 70


def _as64(M, d=4):
    return np.asarray(M, np.float64).reshape(-1, d, d)


def svals(M):
    return np.linalg.svd(_as64(M), compute_uv=False)


def cond(M):
    s = svals(M)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s[:, 0] / s[:, -1]


def in_domain(M):
    M = _as64(M)
    fin = np.isfinite(M).all((-1, -2))
    out = np.zeros(len(M), bool)
    amax = np.abs(M[fin]).max((-1, -2))
    with np.errstate(divide="ignore", invalid="ignore"):
        out[fin] = (cond(M[fin]) <= COND_MAX) & (amax >= ENTRY_LO) & (amax <= ENTRY_HI)
    return out


# ---- the layer in fp64 ---------------------------------------------------------------------------------------------------------------------

def quat64(R):
    """pytorch3d.transforms.matrix_to_quaternion (0.7.5): sqrt(max(0, 1 +- r00 +- r11 +- r22)), the row of the largest, denominators floored
    at 0.1.  Real part first.  [n,4] fp64."""
    r = _as64(R, 3)
    r00, r11, r22 = r[:, 0, 0], r[:, 1, 1], r[:, 2, 2]
    a = np.sqrt(np.maximum(np.stack([1 + r00 + r11 + r22, 1 + r00 - r11 - r22, 1 - r00 + r11 - r22, 1 - r00 - r11 + r22], 1), 0.0))
    s01, s02, s03 = r[:, 2, 1] - r[:, 1, 2], r[:, 0, 2] - r[:, 2, 0], r[:, 1, 0] - r[:, 0, 1]
    p12, p13, p23 = r[:, 1, 0] + r[:, 0, 1], r[:, 0, 2] + r[:, 2, 0], r[:, 1, 2] + r[:, 2, 1]
    sq = a * a
    cand = np.stack([np.stack([sq[:, 0], s01, s02, s03], 1), np.stack([s01, sq[:, 1], p12, p13], 1),
                     np.stack([s02, p12, sq[:, 2], p23], 1), np.stack([s03, p13, p23, sq[:, 3]], 1)], 1)
    best = a.argmax(1)
    i = np.arange(len(r))
    return cand[i, best] / (2 * np.maximum(a[i, best], 0.1))[:, None]


def rot64(t):
    """pytorch3d.transforms.quaternion_to_matrix of a quaternion of any length: [n,3,3]."""
    w, x, y, z = t.T
    s2 = 2.0 / (t * t).sum(1)
    return np.stack([1 - s2 * (y * y + z * z), s2 * (x * y - z * w), s2 * (x * z + y * w),
                     s2 * (x * y + z * w), 1 - s2 * (x * x + z * z), s2 * (y * z - x * w),
                     s2 * (x * z - y * w), s2 * (y * z + x * w), 1 - s2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def layer64(M, R, inverse=False):
    """(R' [n,3,3], ldj [n]) in fp64, numpy.linalg for M^-1 and log|det M|."""
    M = _as64(M)
    with np.errstate(all="ignore"):
        A = np.linalg.inv(M) if inverse else M
        lad = np.linalg.slogdet(M)[1] * (-1.0 if inverse else 1.0)
        t = np.einsum("nij,nj->ni", A, quat64(R))
        return rot64(t), lad - 4 * np.log(np.linalg.norm(t, axis=1))


def log_terms(M, R, inverse=False):
    """|log|det Ms|| + 4 |log|As q|| with Ms = M 2^-e, e the exponent of M's largest entry: the magnitudes of the two logarithms the routine
    adds (it works on Ms; the sum does not depend on e, each term does).  From fp64, not from the code under test."""
    M = _as64(M)
    Ms = M * 2.0 ** -np.floor(np.log2(np.abs(M).max((-1, -2))))[:, None, None]
    A = np.linalg.inv(Ms) if inverse else Ms
    return np.abs(np.linalg.slogdet(Ms)[1]) + 4 * np.abs(np.log(np.linalg.norm(np.einsum("nij,nj->ni", A, quat64(R)), axis=1)))


def _t(a, d):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1, d, d))


def quat_torch(Rt):
    """quat64 on a torch tensor.  The square root is taken of the chosen candidate only: autograd through the oracle's form, which takes all
    four and then selects, returns NaN (0 x inf) wherever one of the three others is clamped at 0."""
    r = Rt.reshape(-1, 3, 3)
    r00, r11, r22 = r[:, 0, 0], r[:, 1, 1], r[:, 2, 2]
    u = torch.stack([1 + r00 + r11 + r22, 1 + r00 - r11 - r22, 1 - r00 + r11 - r22, 1 - r00 - r11 + r22], 1)
    best = u.argmax(1)
    i = torch.arange(len(r))
    a = torch.sqrt(u[i, best])                             # the largest of the four is at least 1
    s01, s02, s03 = r[:, 2, 1] - r[:, 1, 2], r[:, 0, 2] - r[:, 2, 0], r[:, 1, 0] - r[:, 0, 1]
    p12, p13, p23 = r[:, 1, 0] + r[:, 0, 1], r[:, 0, 2] + r[:, 2, 0], r[:, 1, 2] + r[:, 2, 1]
    sq = a * a
    cand = torch.stack([torch.stack([sq, s01, s02, s03], 1), torch.stack([s01, sq, p12, p13], 1),
                        torch.stack([s02, p12, sq, p23], 1), torch.stack([s03, p13, p23, sq], 1)], 1)
    return cand[i, best] / (2 * a)[:, None]


def layer_torch(Mt, Rt, inverse):
    """The same layer on fp64 torch tensors, for autograd (torch.linalg for M^-1 and the determinant)."""
    A = torch.linalg.inv(Mt) if inverse else Mt
    t = (A @ quat_torch(Rt).reshape(-1, 4, 1)).reshape(-1, 4)
    lad = torch.linalg.slogdet(Mt)[1] * (-1.0 if inverse else 1.0)
    return orc.quaternion_to_matrix(t), lad - 4 * torch.log(t.norm(dim=-1))


def layer_grad64(M, R, gR, gl, inverse=False, at=None):
    """(dL/dM [n,4,4], dL/dR [n,3,3]) of L = <gR, R'> + <gl, ldj> by fp64 autograd.  `at`: evaluate at this matrix in place of M."""
    Mt = _t(M if at is None else at, 4).requires_grad_(True)
    Rt = _t(R, 3).requires_grad_(True)
    Ro, l = layer_torch(Mt, Rt, inverse)
    ((Ro * _t(gR, 3)).sum() + (l * torch.from_numpy(np.asarray(gl, np.float64))).sum()).backward()
    return Mt.grad.numpy(), Rt.grad.numpy()


# ---- figures, per sample; inf where the result is not finite -------------------------------------------------------------------------------

def _maxabs(d):
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(d).reshape(len(d), -1).max(-1)
    return np.where(np.isnan(e), np.inf, e)


def orth_err(Q):
    Q = _as64(Q, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(np.einsum("nij,nkj->nik", Q, Q) - np.eye(3)).max((-1, -2))
    return np.where(np.isnan(e), np.inf, e)


def rot_error(Q, want):
    return _maxabs(_as64(Q, 3) - want)


def ldj_error(l, want):
    return _maxabs(np.asarray(l, np.float64) - want)


def rot_figure(Q, want, k):
    """max|R' - want| / (2^-23 kappa)"""
    return rot_error(Q, want) / (U23 * k)


def ldj_figure(l, want, k):
    """|ldj - want| / (2^-23 kappa)"""
    return ldj_error(l, want) / (U23 * k)


def grad_figure(g, want, k):
    """max|g - want| / max|want| / (2^-23 kappa)"""
    return _maxabs(_as64(g) - _as64(want)) / _maxabs(_as64(want)) / (U23 * k)


def tangent(R, g):
    """The part of dL/dR a rotation can feel: vee(R^T g - g^T R), [n,3]."""
    A = np.einsum("nki,nkj->nij", _as64(R, 3), _as64(g, 3))
    A = A - A.transpose(0, 2, 1)
    return np.stack([A[:, 2, 1], A[:, 0, 2], A[:, 1, 0]], 1)


def tangent_figure(R, g, want, k):
    a, b = tangent(R, g), tangent(R, want)
    return _maxabs(a - b) / _maxabs(b) / (U23 * k)


# ---- the yardstick: LAPACK in fp32 ------------------------------------------------------------------------------------------------------

def lapack32(M, R, inverse=False):
    """The layer by torch.linalg.inv / torch.linalg.slogdet / a matrix-vector product, all fp32, on the fp64 quaternion of R rounded once.
    Returns (R' fp32, ldj fp32)."""
    Mt = torch.from_numpy(np.array(M, dtype=np.float32).reshape(-1, 4, 4))
    q = torch.from_numpy(quat64(R).astype(np.float32))
    A = torch.linalg.inv(Mt) if inverse else Mt
    t = (A @ q[:, :, None])[:, :, 0]
    lad = torch.linalg.slogdet(Mt)[1] * (-1.0 if inverse else 1.0)
    return orc.quaternion_to_matrix(t).numpy(), (lad - 4 * torch.log(t.norm(dim=-1))).numpy()


def recomposed(M):
    """The fp64 matrix whose EXACT factors are LAPACK's fp32 ones: P L U of torch.linalg.lu in fp32 (the factorisation both inv and slogdet
    go through).  fp64 autograd evaluated there is what fp32 factors cost a gradient."""
    P, L, U = torch.linalg.lu(torch.from_numpy(np.array(M, dtype=np.float32).reshape(-1, 4, 4)))
    return (P.double() @ L.double() @ U.double()).numpy()


# ---- random inputs -------------------------------------------------------------------------------------------------------------------------

KINDS = ("near_identity", "identity_plus_spread", "normal", "normal_negdet", "singular_values")
REALISTIC = (-2.0, 3.0)
RANGE = (-12.0, 12.0)
WINDOWS = {"realistic": REALISTIC, "range": RANGE}


def _draw(kind, n, rng):
    N = rng.standard_normal((n, 4, 4))
    if kind == "near_identity":
        return np.eye(4) + 0.2 * N
    if kind == "identity_plus_spread":
        return np.eye(4) + 10.0 ** rng.uniform(-2, 3, (n, 1, 1)) * N
    if kind == "normal":
        return N
    if kind == "normal_negdet":
        N[:, 0] *= -np.sign(np.linalg.det(N))[:, None]
        return N
    if kind == "singular_values":                          # U diag(1, c^-t1, c^-t2, 1/c) V^T, c = 10^U(0,3), t ~ U(0,1)
        c = 10.0 ** rng.uniform(0, 3, n)
        t1, t2 = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
        U, _ = np.linalg.qr(N)
        V, _ = np.linalg.qr(rng.standard_normal((n, 4, 4)))
        return np.einsum("nik,nk,njk->nij", U, np.stack([np.ones(n), c ** -t1, c ** -t2, 1 / c], 1), V)
    raise ValueError(kind)


def random_batch(kind, n, seed, window=REALISTIC):
    """([n,4,4] fp32, share of first draws inside the domain).  Every sample is multiplied by its own scale 10^U(window) before the one
    rounding to fp32; a sample whose fp32 matrix has cond > 1e3 is drawn again, so the batch lies in the gated domain completely."""
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    M = _draw(kind, n, rng)
    scale = 10.0 ** rng.uniform(window[0], window[1], (n, 1, 1))
    out = (M * scale).astype(np.float32)
    keep = None
    for _ in range(64):
        bad = ~in_domain(out)
        keep = 1.0 - bad.mean() if keep is None else keep
        if not bad.any():
            return out, keep
        out[bad] = (_draw(kind, int(bad.sum()), rng) * scale[bad]).astype(np.float32)
    raise AssertionError("random_batch: redraw did not converge")


# ---- named edge matrices -------------------------------------------------------------------------------------------------------------------

OUT_OF_DOMAIN = ("rank3", "rank1", "zero", "one_nan", "one_inf")
POW2_EXPONENTS = (-60, -40, 40, 60)


def _edges():
    rng = np.random.default_rng(16)
    N = lambda *s: rng.standard_normal(s)  # noqa: E731
    qr = lambda: np.linalg.qr(N(4, 4))[0]  # noqa: E731
    Q1, Q2 = qr(), qr()
    rot = Q1 * np.sign(np.linalg.det(Q1))
    sv = lambda *s: Q1 @ np.diag(s) @ Q2.T  # noqa: E731
    base = np.eye(4) + 0.2 * N(4, 4)
    e = 1.00001e-3                                           # 1e3 less 1e-5 of it: the rounding to fp32 must not leave the domain
    out = [
        ("identity", np.eye(4)),
        ("rotation4", rot),
        ("reflection", rot @ np.diag([1.0, 1.0, 1.0, -1.0])),
        ("cond_1e3_one_small", sv(1.0, 1.0, 1.0, e)),
        ("cond_1e3_two_small", sv(1.0, 1.0, e, e)),
        ("cond_1e3_three_small", sv(1.0, e, e, e)),
        ("identity_plus_500N", np.eye(4) + 500.0 * N(4, 4)),
    ]
    for k in POW2_EXPONENTS:
        out.append((f"pow2_{k}", np.ldexp(base, k)))
    nan, inf = base.copy(), base.copy()
    nan[1, 2] = np.nan
    inf[2, 0] = np.inf
    out += [
        ("rank3", sv(3.0, 1.5, 1.0, 0.0)),
        ("rank1", np.outer([1.0, -2.0, 0.5, 4.0], [2.0, 1.0, -0.25, 0.5])),       # small dyadic entries: exactly rank 1 in fp32 as well
        ("zero", np.zeros((4, 4))),
        ("one_nan", nan),
        ("one_inf", inf),
    ]
    return [(name, m.astype(np.float32)) for name, m in out]


EDGE_M = _edges()
EDGE_NAMES = [name for name, _ in EDGE_M]
EDGE_STACK = np.stack([m for _, m in EDGE_M])
EDGE_IN = np.array([name not in OUT_OF_DOMAIN for name in EDGE_NAMES])

assert len(set(EDGE_NAMES)) == len(EDGE_NAMES) and set(OUT_OF_DOMAIN) <= set(EDGE_NAMES)
assert np.array_equal(in_domain(EDGE_STACK), EDGE_IN), [n for n, a, b in zip(EDGE_NAMES, in_domain(EDGE_STACK), EDGE_IN) if a != b]
