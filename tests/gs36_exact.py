"""fp64 references for the per-sample 6x6 layer Condition36Trans (csrc/so3_math.h cond_gs36_apply, csrc/so3_grad.h cond_gs36_backward),
the figures every sample is judged by, the inputs, and the fp32 yardsticks.  No GPU, no pytest.

The layer (flow/squeezetrans.py:293-361):  v = (r0; r1), the first two columns of R as a 6-vector;  (a0; a1) = X v with X = M on the forward
and X = M^-1 on the inverse pass;  R' = Gram-Schmidt [t0 t1 t0 x t1] of A = [a0 a1];  ldj = log|det J|, J the 3x3 matrix of the images of
three tangent directions G_k R.  The references are the oracle's own functions in fp64: orc.gs36(M, R) and orc.gs36(torch.linalg.inv(M), R).

FIGURES, per sample, from the fp64 inputs alone and never from the code under test.  On the forward pass a perturbation eps |M| of M
moves A = M v by eps |M| |v| = sqrt(2) eps |M|_2 and turns its Gram-Schmidt factor by that over s2(A), the smaller singular value of the
3x2 matrix A.  On the inverse pass the routine solves M x = v by pivoted elimination, which is backward stable: the computed x solves
(M + E) x = v with |E| ~ eps |M|, so x moves by eps cond(M) |x|, RELATIVE TO ITS OWN LENGTH |x| = |A|_F and not to |M^-1|_2 |v|.  That
is the tighter kappa the four-vector solve earns over  sqrt(2) |M^-1|_2 / s2(A) * cond(M)  (|A|_F <= sqrt(2) |M^-1|_2, so it is never
larger; it is equal for M = I); a product with a computed inverse, the yardstick's route, does not earn it, and the tests assert that the
yardstick's figures stay O(1) under it all the same.  An fp32 routine has eps ~ 2^-23, so
    kappa = sqrt(2) |M|_2 / s2(A)                 (forward),          kappa = cond(M) |A|_F / s2(A)                (inverse)
    rotation figure   max|R' - R'64| / (2^-23 kappa)
    |R' R'^T - I|     in units of 2^-23, NOT divided: a rotation is a rotation whatever made it
    ldj figure        |ldj - ldj64| / (2^-23 kappa cond(J)):  the logarithm of a determinant has the conditioning of J on top of that of
                      its entries (d log|det J| = tr(J^-1 dJ)).  J is rebuilt here in fp64 from the forward-mode tangent images, and
                      `jacobian64` asserts that log|det J| is the oracle's ldj to 1e-8.

YARDSTICKS, computed by the tests on the same batch, never stored.  Rotation and |Q Q^T - I|: LAPACK's fp32 QR (gs3_exact.lapack_gs32) of
the fp32 matrix [a0 a1 a0 x a1], formed with fp32 torch as M32 @ v32 or torch.linalg.inv(M32) @ v32.  ldj: the oracle itself in fp32
torch (torch.linalg.inv in fp32 on the inverse pass): the arithmetic the reference program trains in.

GATED DOMAIN (a condition on the input): finite matrices with cond(M) <= 1e3 as the routine sees them (the fp32 matrix), at every scale.
"""
import numpy as np
import torch

from oracle import flow_oracle as orc
from tests.gs3_exact import _maxabs, lapack_gs32  # noqa: F401  (re-exported for the tests)
from tests.polar3_exact import U23, orth_err  # noqa: F401

COND_MAX = 1e3
LDJ_VACUOUS = 2.0 ** -4                                    # where 2^-23 kappa cond(J) exceeds this the ldj gate says nothing


def _as64(M, d=6):
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
    with np.errstate(divide="ignore", invalid="ignore"):
        out[fin] = cond(M[fin]) <= COND_MAX
    return out


def _t(a, d):
    return torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1, d, d))


# ---- the references: the oracle's own functions in fp64 ---------------------------------------------------------------------------------

def layer_torch(Mt, Rt, inverse):
    return orc.gs36(torch.linalg.inv(Mt) if inverse else Mt, Rt)


def gs36_64(M, R, inverse=False):
    """(R' [n,3,3], ldj [n]) of oracle.gs36 in fp64; the inverse pass applies torch.linalg.inv(M) in fp64 (squeezetrans.py:345)."""
    with np.errstate(all="ignore"):
        Ro, l = layer_torch(_t(M, 6), _t(R, 3), inverse)
    return Ro.numpy(), l.numpy()


# ---- what the figures are divided by, from the fp64 inputs alone ----------------------------------------------------------------------------

_GEN = np.array([[[0., 1, 0], [-1, 0, 0], [0, 0, 0]], [[0, 0, 1], [0, 0, 0], [-1, 0, 0]], [[0, 0, 0], [0, 0, 1], [0, -1, 0]]])


def applied(M, inverse):
    """X [n,6,6] fp64: M, or its fp64 inverse."""
    M = _as64(M)
    with np.errstate(all="ignore"):
        return np.linalg.inv(M) if inverse else M


def images(M, R, inverse):
    """(a [n,6], da [3,n,6]): X v and X (G_k R)[:, :2] stacked, in fp64."""
    X, R = applied(M, inverse), _as64(R, 3)
    dR = np.einsum("kab,nbc->knac", _GEN, R)
    v = np.concatenate([R[..., 0], R[..., 1]], -1)
    dv = np.concatenate([dR[..., 0], dR[..., 1]], -1)
    return np.einsum("nab,nb->na", X, v), np.einsum("nab,knb->kna", X, dv)


def kappa_forward_form(M, R, inverse=False):
    """sqrt(2) |X|_2 / s2(A): kappa of the forward pass, and on the inverse pass the size of what a perturbation of X itself does."""
    X = applied(M, inverse)
    a, _ = images(M, R, inverse)
    A = np.stack([a[:, :3], a[:, 3:]], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(2.0) * np.linalg.svd(X, compute_uv=False)[:, 0] / np.linalg.svd(A, compute_uv=False)[:, -1]


def kappa(M, R, inverse=False):
    """sqrt(2) |M|_2 / s2(A) on the forward pass, cond(M) |A|_F / s2(A) on the inverse pass (module docstring)."""
    if not inverse:
        return kappa_forward_form(M, R)
    a, _ = images(M, R, True)
    A = np.stack([a[:, :3], a[:, 3:]], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return cond(M) * np.linalg.norm(a, axis=-1) / np.linalg.svd(A, compute_uv=False)[:, -1]


def jacobian64(M, R, inverse=False, check=True):
    """J [n,3,3] fp64, rows = the three tangent images vee(dR' R'^T), rebuilt from the forward-mode rule (normalise / project / normalise /
    cross); log|det J| is asserted to be the oracle's ldj to 1e-8 (relative to 1 + |ldj|)."""
    a, da = images(M, R, inverse)
    a0, a1, da0, da1 = a[:, :3], a[:, 3:], da[..., :3], da[..., 3:]

    def normalize(x, dx):
        n = np.linalg.norm(x, axis=-1, keepdims=True)
        t = x / n
        return t, (dx - t * (t * dx).sum(-1, keepdims=True)) / n
    t0, dt0 = normalize(a0, da0)
    dot = (t0 * a1).sum(-1, keepdims=True)
    ddot = (dt0 * a1).sum(-1, keepdims=True) + (t0 * da1).sum(-1, keepdims=True)
    t1, dt1 = normalize(a1 - dot * t0, da1 - ddot * t0 - dot * dt0)
    t2 = np.cross(t0, t1)
    dt2 = np.cross(dt0, t1[None]) + np.cross(t0[None], dt1)
    Rt = np.stack([t0, t1, t2], -1)
    dRt = np.stack([dt0, dt1, dt2], -1)
    delta = dRt @ Rt.transpose(0, 2, 1)[None]
    J = np.stack([delta[..., 0, 1], delta[..., 0, 2], delta[..., 1, 2]], -1).transpose(1, 0, 2)
    if check:
        want = gs36_64(M, R, inverse)[1]
        got = np.log(np.abs(np.linalg.det(J)))
        assert np.abs(got - want).max() <= 1e-8 * (1 + np.abs(want).max()), np.abs(got - want).max()
    return J


def cond_J(M, R, inverse=False):
    s = np.linalg.svd(jacobian64(M, R, inverse), compute_uv=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s[:, 0] / s[:, -1]


# ---- figures, per sample; inf where the result is not finite -------------------------------------------------------------------------------

def rot_figure(Q, want, k):
    """max|Q - want| / (2^-23 k)"""
    return _maxabs(np.asarray(Q, np.float64) - want) / (U23 * k)


def ldj_figure(l, want, kj):
    """|ldj - want| / (2^-23 kappa cond(J)); kj = kappa cond(J)"""
    return _maxabs(np.asarray(l, np.float64) - want) / (U23 * kj)


# ---- the reverse step: reference, conditioning, figures -----------------------------------------------------------------------------------

def layer_grad64(M, R, gR, gl, inverse=False, at=None):
    """(dL/dM [n,6,6], dL/dR [n,3,3]) of L = <gR, R'> + <gl, ldj> by fp64 autograd of the oracle's layer.  `at`: evaluate at this matrix in
    place of M."""
    Mt = _t(M if at is None else at, 6).requires_grad_(True)
    Rt = _t(R, 3).requires_grad_(True)
    Ro, l = layer_torch(Mt, Rt, inverse)
    ((Ro * _t(gR, 3)).sum() + (l * torch.from_numpy(np.asarray(gl, np.float64))).sum()).backward()
    return Mt.grad.numpy(), Rt.grad.numpy()


def rho(M, R, inverse=False):
    """|j0| |j1| |j2| / |det J| >= 1 (Hadamard), J = jacobian64: how far the rows of J are from orthogonal, whatever their lengths."""
    J = jacobian64(M, R, inverse, check=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.linalg.norm(J, axis=-1).prod(-1) / np.abs(np.linalg.det(J))


def grad_conditioning(M, R, inverse=False):
    """(k, kl): what a relative perturbation eps of M does to the two parts of a gradient, relative to the part's own size.

    L = <gR, R'> + gl ldj, so a gradient is the sum of a part linear in gR and a part linear in gl, and fp64 autograd gives each exactly
    (gl = 0, and the difference).  Both are derivatives of functions of A = X v (and of the tangent images X dv_k), X = M or M^-1.

    Rotation part.  R' is the Gram-Schmidt factor of A; eps |M| in M turns it by eps kappa (kappa of the module docstring: through
    sqrt(2) |M|_2 / s2(A) forward, through the backward-stable solve cond(M) |A|_F / s2(A) inverse).  Its derivative g -> (g - t (t.g)) / |a|
    is made of the same unit vectors and inverse lengths, each of which moves by the same relative eps kappa, so
        d(part) <= c eps kappa |part|:                                  k = kappa.
    ldj part.  ldj = log|det J|, its gradient is grad(det J) / det J = sum_k <row k of adj(J)^T, D j_k> / det J, j_k the rows of J.  A row
    is a tangent image X dv_k pushed through the same normalisations as R' (j ~ P da / |a|, without dimension).  eps |M| in M moves da_k
    by eps |M| |dv_k| whatever |da_k| itself is, so a row moves by eps kappa ABSOLUTELY (through da_k) and by eps kappa |j_k| (through
    the frame and the lengths):  |dj_k| <= eps kappa (1 + |j_k|).  The rows have lengths of their own (dv_k may lie along a small singular
    direction of X: |J|_2 ~ 1e-2 occurs at cond(M) ~ 500), so the absolute part cannot be dropped.  Two things move:
      * 1 / det J, by tr(J^-1 dJ).  Norm-wise |J^-1 dJ| <= |J^-1|_2 |dJ| <= eps kappa sqrt(3) |J^-1|_2 (1 + |J|_2), which is the forward's
        cond(J) where |J|_2 >= 1.  Row-wise, column k of J^-1 is (j_l x j_m) / det J, so |J^-1 dJ| <= sum_k |j_l| |j_m| |dj_k| / |det J|
        <= 3 eps kappa rho (1 + 1 / min|j_k|) with rho = |j0| |j1| |j2| / |det J|.  Either holds; neither implies the other (rows of unequal
        length: the second is smaller; three nearly parallel rows: rho ~ cond(J)^2).
      * the cofactors j_l x j_m, by eps kappa (1 + 1 / min|j|) |j_l| |j_m| against |j_l x j_m| >= |det J| / |j_k|: the row-wise form again.
    The first is bounded by the smaller of the two forms, the second by the row-wise one; a figure that must be O(1) for every sample takes
        kl = kappa (|J^-1|_2 (1 + |J|_2) + rho (1 + 1 / min|j_k|)),
    the sum standing for both terms.  Next to a fold (det J -> 0 inside the domain) both grow without bound while kappa stays
    O(1): that is the conditioning the rotation figure does not carry.
    The derivation is checked in tests/test_gs36_host.py: fp64 autograd at M (1 + 2^-23 U(-1, 1)) shows figures of O(1) in all 20 cells."""
    k = kappa(M, R, inverse)
    J = jacobian64(M, R, inverse, check=False)
    with np.errstate(all="ignore"):
        sv = np.linalg.svd(J, compute_uv=False)
        rows = np.linalg.norm(J, axis=-1)
        return k, k * ((1 + sv[:, 0]) / sv[:, -1] + rho(M, R, inverse) * (1 + 1 / rows.min(-1)))


def tangent(R, g):
    """The part of dL/dR a rotation can feel: vee(R^T g - g^T R), [n,3]."""
    A = np.einsum("nki,nkj->nij", _as64(R, 3), _as64(g, 3))
    A = A - A.transpose(0, 2, 1)
    return np.stack([A[:, 2, 1], A[:, 0, 2], A[:, 1, 0]], 1)


def grad_figure(g, want, want_rot, k, kl):
    """max|g - want| / (2^-23 (k max|want_rot| + kl max|want - want_rot|)): want_rot is the gradient with g_ldj = 0 (the rotation part),
    want - want_rot the ldj part; each is measured in its own conditioning (grad_conditioning).  With g_ldj = 0 this is
    max|g - want| / max|want| / (2^-23 kappa), the figure of tests/gs3_exact.py."""
    d = _as64(g).shape[-1]
    want, want_rot = _as64(want, d), _as64(want_rot, d)
    return _maxabs(_as64(g, d) - want) / (U23 * (k * _maxabs(want_rot) + kl * _maxabs(want - want_rot)))


def tangent_figure(R, g, want, want_rot, k, kl):
    """grad_figure of the tangent parts of dL/dR."""
    a, b, br = tangent(R, g), tangent(R, want), tangent(R, want_rot)
    return _maxabs(a - b) / (U23 * (k * _maxabs(br) + kl * _maxabs(b - br)))


def product_terms(M, R, gR, gl, inverse=False):
    """(terms of dL/dM, terms of dL/dR): the sizes of what the reverse step MULTIPLIES, per sample, from the fp64 inputs alone.  An fp32
    product of terms rounds to 2^-23 of its terms, however small the sum comes out (tests/test_gs3_host.py backward_gates); restated for
    this layer, whose reverse step is so3_grad.h cond_gs36_backward (the closed form ldj = log|u.(p x q)| - 2 log|a0| - log|b1|):
      * the reverse of normalising, g -> (g - t (t.g)) / |a|, rounds the 3-term product t.g to 2^-23 c (c = the largest cotangent entry,
        of R' or of ldj) and divides by |a0| or |b1|, both >= s2(A): dL/dA carries c / s2(A); the two logarithms of lengths add
        |gl| (2 / |a0| + 1 / |b1|) <= 3 c / s2(A).
      * the determinant D = u.(p x q): dL/du = gl (p x q) / D and its like have the sizes gl |p| |q| / |D|, gl |q| |u| / |D|,
        gl |u| |p| / |D|, and reach dL/dX as outer products with unit vectors: S = |gl| (|p||q| + |q||u| + |u||p|) / |D|.  On their way back
        to t1, t2 they are multiplied by X (terms |X|_2 S, without dimension as a cotangent of a unit vector is), which the division by
        |b1|, |a0| in the reverse of normalising turns into |X|_2 S / s2(A) at most.
      so dL/dX is made of terms T = 4 c / s2(A) + S (1 + |X|_2 / s2(A)), of the dimension 1 / X as dL/dX is.
      * forward pass: dL/dM = dL/dX.  Inverse pass: dL/dM = -X^T (dL/dX) X^T, every term times |X|_2^2.
      * dL/dR = X^T dL/dA + (cross products of c, e, f = X^T t with the cotangents of p, q, u): terms |X|_2 T."""
    X = applied(M, inverse)
    a, _ = images(M, R, inverse)
    a0, a1 = a[:, :3], a[:, 3:]
    R = _as64(R, 3)
    r0, r1 = R[..., 0], R[..., 1]
    with np.errstate(all="ignore"):
        t0 = a0 / np.linalg.norm(a0, axis=-1, keepdims=True)
        b1 = a1 - t0 * (t0 * a1).sum(-1, keepdims=True)
        t1 = b1 / np.linalg.norm(b1, axis=-1, keepdims=True)
        t2 = np.cross(t0, t1)
        z = np.zeros_like(t2)
        xt = lambda top, bot: np.einsum("nba,nb->na", X, np.concatenate([top, bot], -1))  # noqa: E731
        c, e, f = xt(t2, z), xt(t1, z), xt(z, t2)
        row = lambda w: np.cross(r0, w[:, :3]) + np.cross(r1, w[:, 3:])  # noqa: E731
        p, q, u = row(c), row(e), row(f)
        D = np.abs((u * np.cross(p, q)).sum(-1))
        n = lambda w: np.linalg.norm(w, axis=-1)  # noqa: E731
        S = np.abs(np.asarray(gl, np.float64)) * (n(p) * n(q) + n(q) * n(u) + n(u) * n(p)) / D
        A = np.stack([a0, a1], -1)
        s2 = np.linalg.svd(A, compute_uv=False)[:, -1]
        x2 = np.linalg.svd(X, compute_uv=False)[:, 0]
        cmax = np.maximum(np.abs(_as64(gR, 3)).reshape(len(R), -1).max(-1), np.abs(gl))
        T = 4 * cmax / s2 + S * (1 + x2 / s2)
        return T * (x2 ** 2 if inverse else 1.0), x2 * T


def perturbed(M, seed=0):
    """M (1 + 2^-23 U(-1, 1)) entry by entry, in fp64: what one rounding of every entry would do."""
    M = _as64(M)
    return M * (1 + U23 * np.random.default_rng(seed).uniform(-1, 1, M.shape))


def recomposed32(M):
    """The fp64 product Q R of LAPACK's fp32 QR factors of the fp32 matrix M: a matrix one backward-stable fp32 step away from M.  fp64
    autograd evaluated there is what such a step costs a gradient: the yardstick of the reverse step, independent of the code under test."""
    Q, U = torch.linalg.qr(_t32(M, 6))
    return (Q.double() @ U.double()).numpy()


# ---- the yardsticks -------------------------------------------------------------------------------------------------------------------------

def _t32(a, d):
    return torch.from_numpy(np.array(a, dtype=np.float32).reshape(-1, d, d))


def lapack_rot32(M, R, inverse=False):
    """LAPACK's fp32 QR of the fp32 matrix [a0 a1 a0 x a1], (a0; a1) = M32 @ v32 or torch.linalg.inv(M32) @ v32 in fp32 torch, in the
    layer's convention (gs3_exact.lapack_gs32).  Q [n,3,3] fp32."""
    Mt, Rt = _t32(M, 6), _t32(R, 3)
    v = torch.cat([Rt[..., 0], Rt[..., 1]], -1)
    a = ((torch.linalg.inv(Mt) if inverse else Mt) @ v[:, :, None])[:, :, 0]
    a0, a1 = a[:, :3], a[:, 3:]
    X = torch.stack([a0, a1, torch.linalg.cross(a0, a1)], -1)
    return lapack_gs32(X.numpy())[0]


def oracle32(M, R, inverse=False):
    """The oracle's layer in fp32 torch: (R' fp32, ldj fp32)."""
    with np.errstate(all="ignore"):
        Mt = _t32(M, 6)
        Ro, l = orc.gs36(torch.linalg.inv(Mt) if inverse else Mt, _t32(R, 3))
    return Ro.numpy(), l.numpy()


# ---- random inputs: the families of tests/polar3_exact.py restated for 6x6 ---------------------------------------------------------------------

KINDS = ("near_identity", "identity_plus_spread", "normal", "normal_negdet", "singular_values")
REALISTIC = (-2.0, 3.0)
RANGE = (-12.0, 12.0)
WINDOWS = {"realistic": REALISTIC, "range": RANGE}


def _draw(kind, n, rng):
    N = rng.standard_normal((n, 6, 6))
    if kind == "near_identity":
        return np.eye(6) + 0.2 * N
    if kind == "identity_plus_spread":
        return np.eye(6) + 10.0 ** rng.uniform(-2, 3, (n, 1, 1)) * N
    if kind == "normal":
        return N
    if kind == "normal_negdet":
        N[:, 0] *= -np.sign(np.linalg.det(N))[:, None]
        return N
    if kind == "singular_values":                          # U diag(1, c^-t1 .. c^-t4, 1/c) V^T, c = 10^U(0,3), t ~ U(0,1)
        c = 10.0 ** rng.uniform(0, 3, n)
        t = rng.uniform(0, 1, (n, 4))
        U, _ = np.linalg.qr(N)
        V, _ = np.linalg.qr(rng.standard_normal((n, 6, 6)))
        s = np.concatenate([np.ones((n, 1)), c[:, None] ** -t, 1 / c[:, None]], 1)
        return np.einsum("nik,nk,njk->nij", U, s, V)
    raise ValueError(kind)


def random_batch(kind, n, seed, window=REALISTIC):
    """([n,6,6] fp32, share of first draws inside the domain).  Every sample is multiplied by its own scale 10^U(window) before the one
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


# ---- named edges.  Some are defined against the rotation they meet and against the pass, so they come with their R -----------------------------

POW2_EXPONENTS = (-60, -40, 40, 60)
ASKED_NAN = ("zero", "a1_equals_a0", "a0_zero", "one_nan", "one_inf")            # and "two_equal_rows" on the inverse pass
EXTREME_SCALES = (10.0 ** 19.5, 10.0 ** -19.5, 1e21, 1e30, 1e-30)


def _rot_from(rng):
    Q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    return Q * np.sign(np.linalg.det(Q))


def edges(inverse):
    """(names, M [k,6,6] fp32, R [k,3,3] fp32, in_domain mask).  In the domain: the identity, a block-diagonal pair of rotations, the
    permutation that swaps the two 3-blocks, 2^+-40 and 2^+-60 times I + 0.2 N, and cond 1e3 with the small singular direction of the
    APPLIED matrix X along v (so that A is the small image: `cond_1e3_small_in_A`) or the large one along v (`.._away_from_A`).
    Out of the domain: zero; lower rows equal to upper rows (a1 = a0); a0 = 0 exactly for R = I (rows 0..2 of X have zeros in columns
    0 and 4; X a permutation, so that the inverse pass meets it exactly as well); two equal rows; cond 1e5 and 1e7; one NaN, one inf."""
    rng = np.random.default_rng(36)
    Rg = _rot_from(rng).astype(np.float32)                   # the rotation the R-dependent edges are built against
    v = np.concatenate([Rg[:, 0], Rg[:, 1]]).astype(np.float64)
    base = np.eye(6) + 0.2 * rng.standard_normal((6, 6))
    Ra, Rb = _rot_from(rng), _rot_from(rng)
    blk = np.zeros((6, 6))
    blk[:3, :3], blk[3:, 3:] = Ra, Rb
    swap = np.zeros((6, 6))
    swap[:3, 3:], swap[3:, :3] = np.eye(3), np.eye(3)

    def with_v(col, s):                                      # X = U diag(s) V^T with V[:, col] = v / |v|
        V = np.linalg.qr(np.concatenate([v[:, None], rng.standard_normal((6, 5))], 1))[0]
        V = np.roll(V, col, axis=1) if col else V
        X = np.linalg.qr(rng.standard_normal((6, 6)))[0] @ np.diag(s) @ V.T
        return np.linalg.inv(X) if inverse else X
    e = 1.00001e-3
    s = np.array([1.0, 0.5, 0.2, 0.1, 0.05, e])
    eye3 = np.eye(3, dtype=np.float32)
    out = [("identity", np.eye(6), Rg), ("block_rotations", blk, Rg), ("swap_blocks", swap, Rg),
           ("cond_1e3_small_in_A", with_v(5, s), Rg), ("cond_1e3_away_from_A", with_v(0, s), Rg)]
    out += [(f"pow2_{k}", np.ldexp(base, k), Rg) for k in POW2_EXPONENTS]
    n_in = len(out)
    twin = base.copy()
    twin[3:] = twin[:3]
    perm = np.eye(6)[[1, 2, 3, 0, 4, 5]]                     # rows 0..2 read entries 1, 2, 3 of v = (1, 0, 0, 0, 1, 0): a0 = 0 exactly
    rows2 = base.copy()
    rows2[4] = rows2[1]
    sv = lambda c: np.linalg.qr(rng.standard_normal((6, 6)))[0] @ np.diag([1.0, 0.7, 0.5, 0.3, 0.2, 1 / c]) @ np.linalg.qr(rng.standard_normal((6, 6)))[0]  # noqa: E731
    nan, inf = base.copy(), base.copy()
    nan[1, 2], inf[4, 0] = np.nan, np.inf
    out += [("zero", np.zeros((6, 6)), Rg), ("a1_equals_a0", twin, Rg), ("a0_zero", perm.T if inverse else perm, eye3),
            ("two_equal_rows", rows2, Rg), ("cond_1e5", sv(1e5), Rg), ("cond_1e7", sv(1e7), Rg), ("one_nan", nan, Rg), ("one_inf", inf, Rg)]
    names = [n for n, _, _ in out]
    M = np.stack([m for _, m, _ in out]).astype(np.float32)
    R = np.stack([r for _, _, r in out]).astype(np.float32)
    mask = np.arange(len(out)) < n_in
    dom = in_domain(M)
    dom[names.index("a0_zero")] = False                      # a permutation, cond 1: outside because of the rotation it meets (s2(A) = 0)
    assert np.array_equal(dom, mask), [n for n, a, b in zip(names, dom, mask) if a != b]
    return names, M, R, mask


for _inv in (False, True):                                   # the definitions hold what they name
    _n, _M, _R, _in = edges(_inv)
    jacobian64(_M[_in], _R[_in], _inv)
    _a = images(_M[_n.index("a0_zero")][None], _R[_n.index("a0_zero")][None], _inv)[0][0]
    assert (_a[:3] == 0).all() and np.abs(_a[3:]).max() == 1, _a
    _k = kappa_forward_form(_M[_in], _R[_in], _inv)
    assert _k[_n.index("cond_1e3_small_in_A")] > 30 * _k[_n.index("cond_1e3_away_from_A")]
