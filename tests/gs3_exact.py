"""fp64 references for the per-sample 3x3 Gram-Schmidt layers (csrc/so3_math.h smith3 and cond_gs9_apply, csrc/so3_grad.h cond9_backward for
RNF_KIND_COND9_GS / _SMITH), the figures every sample is judged by, and the LAPACK fp32 yardstick.  No GPU, no pytest.  The inputs (KINDS,
WINDOWS, in_domain, EDGE_M, OUT_OF_DOMAIN) are those of tests/polar3_exact.py, imported, not copied.

How far rounding may move a Gram-Schmidt factor is set by the matrix: a perturbation eps |A| of A = Q U turns Q by about eps cond(A).  An
fp32 routine has eps ~ 2^-23, so every figure is an error divided by 2^-23 kappa:
    Smith (Q of the first two columns of M):           kappa2 = s1 / s2 of the 3x2 matrix M[:, :2]
    calculate_9 (R', ldj of M R or M^-1 R):            kappa  = cond(M), in both passes
    |Q Q^T - I|:                                       NOT divided by kappa: a rotation is a rotation whatever made it
Tests gate each figure at twice what LAPACK's fp32 QR shows on the same batch (`lapack_gs32`).
"""
import numpy as np
import torch

from oracle import flow_oracle as orc
from tests.polar3_exact import U23, _as64, cond, orth_err  # noqa: F401  (re-exported for the tests)


def kappa2(M):
    s = np.linalg.svd(_as64(M)[:, :, :2], compute_uv=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s[:, 0] / s[:, 1]


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1, 3, 3))


_EYE = torch.eye(3, dtype=torch.float64)[None]


# ---- the references: the oracle's own functions in fp64 ---------------------------------------------------------------------------------

def _smith(Mt):
    return orc.smithr9(Mt, _EYE.expand(Mt.shape[0], 3, 3))[0]


def _gs9(Mt, Rt, inverse):
    return orc.gs9(torch.linalg.inv(Mt) if inverse else Mt, Rt)


def smith64(M):
    """Gram-Schmidt rotation of the columns of M: oracle.smithr9 with R = I, fp64, [n,3,3]."""
    with np.errstate(all="ignore"):
        return _smith(_t(M)).numpy()


def gs9_64(M, R, inverse=False):
    """(R', ldj) of oracle.gs9 in fp64; the inverse pass applies torch.linalg.inv(M) in fp64 (squeezetrans.py:245)."""
    Ro, l = _gs9(_t(M), _t(R), inverse)
    return Ro.numpy(), l.numpy()


def layer64(name, Mt, Rt, inverse):
    """The whole layer on torch tensors: "gs9" (Condition9Trans: R' = Gram-Schmidt of M R or M^-1 R, with its ldj) or "smith"
    (Condition9RotRSmith: R' = R N or R N^T, N = smith64(M), ldj = 0)."""
    return _gs9(Mt, Rt, inverse) if name == "gs9" else orc.smithr9(Mt, Rt, inverse)


def layer_grad64(name, M, R, gR, gl, inverse=False, at=None):
    """(dL/dM, dL/dR) of L = <gR, R'> + <gl, ldj> by fp64 autograd of layer64.  `at`: evaluate at this matrix in place of M."""
    Mt = _t(M if at is None else at).requires_grad_(True)
    Rt = _t(R).requires_grad_(True)
    Ro, l = layer64(name, Mt, Rt, inverse)
    ((Ro * _t(gR)).sum() + (l * torch.from_numpy(np.asarray(gl, np.float64))).sum()).backward()
    return Mt.grad.numpy(), Rt.grad.numpy()


# ---- figures, per sample; inf where the result is not finite -------------------------------------------------------------------------------

def _maxabs(d):
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(d).reshape(len(d), -1).max(-1)
    return np.where(np.isnan(e), np.inf, e)


def rot_figure(Q, want, k):
    """max|Q - want| / (2^-23 k)"""
    return _maxabs(_as64(Q) - want) / (U23 * k)


def ldj_figure(l, want, k):
    """|ldj - want| / (2^-23 k)"""
    return _maxabs(np.asarray(l, np.float64) - want) / (U23 * k)


def grad_figure(g, want, k):
    """max|g - want| / max|want| / (2^-23 k)"""
    return _maxabs(_as64(g) - _as64(want)) / _maxabs(_as64(want)) / (U23 * k)


def tangent(R, g):
    """The part of dL/dR a rotation can feel: vee(R^T g - g^T R), [n,3]."""
    A = np.einsum("nki,nkj->nij", _as64(R), _as64(g))
    A = A - A.transpose(0, 2, 1)
    return np.stack([A[:, 2, 1], A[:, 0, 2], A[:, 1, 0]], 1)


def tangent_figure(R, g, want, k):
    """max|tangent(g) - tangent(want)| / max|tangent(want)| / (2^-23 k)"""
    a, b = tangent(R, g), tangent(R, want)
    return _maxabs(a - b) / _maxabs(b) / (U23 * k)


# ---- the yardstick: LAPACK's fp32 QR --------------------------------------------------------------------------------------------------------

def lapack_gs32(X32):
    """Householder QR of the fp32 matrices X32 [n,3,3] by torch.linalg.qr in fp32, brought to the layer's convention: signs fixed so that the
    triangular factor's diagonal is positive, then the third column replaced by the cross product of the first two (and the last row of the
    triangular factor by its sign).  Returns (Q [n,3,3] fp32, ldj [n] fp32 = 2 log|u22| - 2 log u00, U [n,3,3] fp32)."""
    X = torch.from_numpy(np.array(X32, dtype=np.float32).reshape(-1, 3, 3))
    Q, U = torch.linalg.qr(X)
    d = torch.sign(torch.diagonal(U, dim1=-2, dim2=-1))
    Q, U = Q * d[:, None, :], U * d[:, :, None]
    q2 = torch.linalg.cross(Q[..., 0], Q[..., 1])
    s = torch.sign((q2 * Q[..., 2]).sum(-1))
    Q = torch.stack([Q[..., 0], Q[..., 1], q2], -1)
    U = torch.cat([U[:, :2], U[:, 2:] * s[:, None, None]], 1)
    ldj = 2 * torch.log(U[:, 2, 2].abs()) - 2 * torch.log(U[:, 0, 0])
    return Q.numpy(), ldj.numpy(), U.numpy()


def gs9_input32(M, R, inverse):
    """The fp32 matrix the yardstick factors: fl(M R), or torch.linalg.inv(M) @ R in fp32."""
    Mt = torch.from_numpy(np.array(M, dtype=np.float32).reshape(-1, 3, 3))
    Rt = torch.from_numpy(np.array(R, dtype=np.float32).reshape(-1, 3, 3))
    return ((torch.linalg.inv(Mt) if inverse else Mt) @ Rt).numpy()


def recomposed(Q32, U32, R=None, inverse=False):
    """The fp64 matrix whose EXACT factors are the yardstick's fp32 ones: Q U for Smith; (Q U) R^-1 or R (Q U)^-1 for calculate_9.  fp64
    autograd evaluated there is what fp32 factors cost a gradient."""
    X = _as64(Q32) @ _as64(U32)
    if R is None:
        return X
    return _as64(R) @ np.linalg.inv(X) if inverse else X @ np.linalg.inv(_as64(R))
