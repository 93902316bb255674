"""CPU: the per-sample 6x6 layer Condition36Trans (csrc/so3_math.h cond_gs36_apply: exactly what cond36_finish calls; csrc/so3_grad.h
cond_gs36_backward: exactly what the training kernels' rare_gs36 calls), host build without contraction, EVERY sample against fp64
(tests/gs36_exact.py) over the whole gated domain: cond(M) <= 1e3 at every scale, det < 0 included, both passes.

The yardsticks are computed inside the tests on the same batch: LAPACK's fp32 QR of the fp32 matrix [a0 a1 a0 x a1] for the rotation and
|Q Q^T - I|, the oracle's own layer in fp32 torch for ldj.  The header may show twice the yardstick's batch
maximum of the same figure in the same cell (family x window x pass).  Figures: tests/gs36_exact.py.  The measured tables (header /
yardstick per cell), the vacuous-gate shares and what the routine this replaces shows in the same tests: DESIGN.md section 3.7d.

The reverse step is judged the same way (second half of the file): dL/dM and the tangent part of dL/dR per sample against fp64 autograd of
the oracle's layer, in the conditioning gs36_exact.grad_conditioning derives; the yardstick is fp64 autograd at the fp64 product of
LAPACK's fp32 QR factors of M, a matrix one backward-stable fp32 step away, computed here on the same batch.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from rotationnormflow_amd import synth
from tests import gs36_exact as gx
from tests.test_host_grad import f32, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_gs36.cpp")
OUT = os.path.join(HERE, "csrc", "_host_gs36.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", h) for h in ("so3_math.h", "so3_grad.h")]

U23 = gx.U23
ORTH_NAN = 16 * U23                                          # kPolar3Orth: what the header itself accepts as a rotation
N_BATCH = 20000
CASES = [(k, w) for w in gx.WINDOWS for k in gx.KINDS]
PASSES = [False, True]
VACUOUS_MAX = 0.12                                           # the largest share of a cell whose ldj gate may say nothing


@pytest.fixture(scope="module")
def h36():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    return C.CDLL(OUT)


def apply36(h36, M, R, inverse):
    A, r = f32(np.asarray(M).reshape(-1, 36)), f32(np.asarray(R).reshape(-1, 9))
    Ro, l = np.empty_like(r), np.empty(len(A), np.float32)
    h36.h36_apply(ptr(A), ptr(r), int(inverse), len(A), ptr(Ro), ptr(l))
    return Ro.reshape(-1, 3, 3), l


@functools.lru_cache(maxsize=None)
def batch(kind, window, n=N_BATCH):
    M, kept = gx.random_batch(kind, n, 1, gx.WINDOWS[window])
    assert kept >= 0.98 and gx.in_domain(M).all(), (kind, window, kept)          # a condition on the input; nothing is left out of a gate
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def rotations(n=N_BATCH):
    R = synth.uniform_rotations(n, seed=36).astype(np.float32)
    R.setflags(write=False)
    return R


# ---- the yardsticks, computed once per cell and shared ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def yardstick(inverse, kind, window, n=N_BATCH):
    """Batch maxima of the forward figures of the two fp32 yardsticks on batch(kind, window), with the fp64 references, kappa and
    kappa cond(J) themselves (read-only)."""
    M, R = batch(kind, window, n), rotations(n)
    k = gx.kappa(M, R, inverse)
    kj = k * gx.cond_J(M, R, inverse)
    want, want_l = gx.gs36_64(M, R, inverse)
    Q32 = gx.lapack_rot32(M, R, inverse)
    l32 = gx.oracle32(M, R, inverse)[1]
    for a in (k, kj, want, want_l):
        a.setflags(write=False)
    return {"rot": gx.rot_figure(Q32, want, k).max(), "orth": gx.orth_err(Q32).max(), "ldj": gx.ldj_figure(l32, want_l, kj).max(),
            "vacuous": float(np.mean(U23 * kj > gx.LDJ_VACUOUS)), "k": k, "kj": kj, "want": want, "want_ldj": want_l}


def strictest(inverse, key):
    """The smallest of the cells' yardsticks: the gate of inputs that belong to no batch (the named edges)."""
    return min(yardstick(inverse, k, w)[key] for k, w in CASES)


# ---- the references and the yardsticks themselves -----------------------------------------------------------------------------------------------

def test_reference_functions_hold_what_they_name():
    n = 2000
    M, R = batch("singular_values", "realistic", n).astype(np.float64), rotations(n).astype(np.float64)
    for inverse in PASSES:
        Ro, l = gx.gs36_64(M, R, inverse)
        a, _ = gx.images(M, R, inverse)
        assert gx.orth_err(Ro).max() < 1e-12 and np.allclose(np.linalg.det(Ro), 1.0)
        # R' is the Gram-Schmidt factor of [a0 a1]: t0 along a0, a1 in the span of t0, t1 with a positive t1 part
        assert np.abs(np.cross(Ro[:, :, 0], a[:, :3])).max() < 1e-9 * np.abs(a).max() and ((Ro[:, :, 0] * a[:, :3]).sum(-1) > 0).all()
        assert (np.abs((Ro[:, :, 2] * a[:, 3:]).sum(-1)) < 1e-9 * np.linalg.norm(a[:, 3:], axis=-1)).all() and ((Ro[:, :, 1] * a[:, 3:]).sum(-1) > 0).all()
        gx.jacobian64(M, R, inverse)                                               # asserts log|det J| = ldj to 1e-8
        for c in (2.0 ** -40, 3.0):                                                 # R' and ldj do not depend on the scale of M
            Rc, lc = gx.gs36_64(c * M, R, inverse)
            assert np.abs(Rc - Ro).max() < 1e-9 and np.abs(lc - l).max() < 1e-8
        k = gx.kappa(M, R, inverse)
        assert (k >= (gx.cond(M) if inverse else 1.0) * (1 - 1e-12)).all()        # |A|_F >= s2(A); |M v| <= sqrt(2) |M|_2
        assert (k <= gx.kappa_forward_form(M, R, inverse) * (gx.cond(M) if inverse else 1.0) * (1 + 1e-12)).all()
    # figures: off by d in one entry reads d / (2^-23 kappa); a NaN reads inf
    Q, _ = gx.gs36_64(M, R)
    k = gx.kappa(M, R)
    Qb = Q.copy()
    Qb[5, 1, 2] += 3 * U23 * k[5]
    Qb[6, 0, 0] = np.nan
    f = gx.rot_figure(Qb, Q, k)
    assert abs(f[5] - 3) < 1e-6 and np.isinf(f[6]) and f[7] == 0


@pytest.mark.parametrize("kind", gx.KINDS)
def test_the_yardsticks_are_order_one_in_the_conditioned_measure(kind):
    """The yardsticks' own figures.  Householder QR is backward stable with a constant of a few tens for a 3x3 (tests/test_gs3_host.py: under
    36), and the 6-term products (or the 6x6 LU solve) that form A before it double the count of roundings: under 72, Q orthogonal to 36
    units.  The fp32 oracle takes no second projection, so its ldj carries the loss of orthogonality on top: it is asked to stay under
    4 x 72 in units of 2^-23 kappa cond(J).  The share of samples whose ldj gate says nothing (2^-23 kappa cond(J) > 2^-4) is reported per
    cell and must not exceed 0.12."""
    for window in gx.WINDOWS:
        for inverse in PASSES:
            y = yardstick(inverse, kind, window)
            print(f"{kind}, {window}, inverse {inverse}: LAPACK fp32 rotation {y['rot']:.2f}, |QQ^T - I| {y['orth'] / U23:.2f} units; fp32 oracle ldj {y['ldj']:.2f}, "
                  f"vacuous ldj gates {y['vacuous']:.4f}; kappa median {np.median(y['k']):.3g} max {y['k'].max():.3g}")
            assert y["rot"] < 72 and y["orth"] < 36 * U23 and y["ldj"] < 288
            assert y["vacuous"] <= VACUOUS_MAX


# ---- forward: every sample ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,window", CASES)
@pytest.mark.parametrize("inverse", PASSES)
def test_every_sample_is_the_fp64_rotation(h36, inverse, kind, window):
    """All 20 000 matrices of each family and scale window, both passes: rotation figure within 2x LAPACK fp32's batch maximum, orthogonal
    within 2x LAPACK's, ldj figure within 2x the fp32 oracle's, det = +1.  No sample is left out of any of the three."""
    M, R, y = batch(kind, window), rotations(), yardstick(inverse, kind, window)
    Q, l = apply36(h36, M, R, inverse)
    f, o, fl = gx.rot_figure(Q, y["want"], y["k"]), gx.orth_err(Q), gx.ldj_figure(l, y["want_ldj"], y["kj"])
    print(f"inverse {inverse}, {kind}, {window}: header / yardstick: rotation {f.max():.2f} / {y['rot']:.2f}, ldj {fl.max():.2f} / {y['ldj']:.2f}, "
          f"|QQ^T - I| {o.max() / U23:.2f} / {y['orth'] / U23:.2f} units; vacuous ldj gates {y['vacuous']:.4f}")
    assert f.max() <= 2 * y["rot"], (f.max(), y["rot"], int(f.argmax()), int((f > 2 * y["rot"]).sum()))
    assert o.max() <= 2 * y["orth"], (o.max() / U23, y["orth"] / U23, int(o.argmax()), int((o > 2 * y["orth"]).sum()))
    assert fl.max() <= 2 * y["ldj"], (fl.max(), y["ldj"], int(fl.argmax()), int((fl > 2 * y["ldj"]).sum()))
    assert (np.linalg.det(Q.astype(np.float64)) > 0.5).all()
    assert y["vacuous"] <= VACUOUS_MAX


@pytest.mark.parametrize("inverse", PASSES)
def test_in_domain_edges(h36, inverse):
    names, M, R, inside = gx.edges(inverse)
    names, M, R = np.array(names)[inside], M[inside], R[inside]
    k = gx.kappa(M, R, inverse)
    kj = k * gx.cond_J(M, R, inverse)
    want, want_l = gx.gs36_64(M, R, inverse)
    Q, l = apply36(h36, M, R, inverse)
    f, o, fl = gx.rot_figure(Q, want, k), gx.orth_err(Q), gx.ldj_figure(l, want_l, kj)
    gate = {key: 2 * strictest(inverse, key) for key in ("rot", "orth", "ldj")}
    print(f"inverse {inverse}, in-domain edges, rotation figure:", dict(zip(names, np.round(f, 2))), "gate", gate["rot"])
    print("  ldj figure:", dict(zip(names, np.round(fl, 2))), "gate", gate["ldj"])
    print("  |QQ^T - I| in units:", dict(zip(names, np.round(o / U23, 2))), "gate", gate["orth"] / U23)
    assert (f <= gate["rot"]).all(), [(n, v) for n, v in zip(names, f) if v > gate["rot"]]
    assert (o <= gate["orth"]).all(), [(n, v) for n, v in zip(names, o) if v > gate["orth"]]
    assert (fl <= gate["ldj"]).all(), [(n, v) for n, v in zip(names, fl) if v > gate["ldj"]]
    assert (np.linalg.det(Q.astype(np.float64)) > 0.5).all()


# ---- out of the domain: a rotation or NaN ---------------------------------------------------------------------------------------------------

def check_nan_or_rotation(Q, l, tag):
    """R' all NaN beside a non-finite ldj, or finite and orthogonal to 16 units (what the header itself accepts) beside a finite ldj."""
    o = gx.orth_err(Q)
    nan = np.isnan(Q).all((-1, -2)) & ~np.isfinite(l)
    rot = np.isfinite(Q).all((-1, -2)) & (o <= ORTH_NAN) & np.isfinite(l)
    print(f"{tag}: {int(nan.sum())} of {len(Q)} NaN, the rest orthogonal to {o[~nan].max() / U23 if (~nan).any() else 0:.1f} units")
    assert (nan | rot).all(), (tag, int((~(nan | rot)).sum()), Q[~(nan | rot)][:2], l[~(nan | rot)][:2])
    return nan


@pytest.mark.parametrize("inverse", PASSES)
def test_out_of_domain_is_nan_or_a_rotation(h36, inverse):
    """The named cases outside the domain; 2 000 random matrices each of cond 1e4 .. 1e8 and of exact rank 5, at scales 10^U(-12,12); 2 000
    with the lower rows within 1e-5 .. 1e-7 of the upper rows; and the ends of the fp32 range, 10^+-19.5, 1e21, 1e+-30 times I + 0.2 N, which
    are asked to give the rotation of the matrix itself within the in-domain gate."""
    names, M, R, inside = gx.edges(inverse)
    names, M, R = np.array(names)[~inside], M[~inside], R[~inside]
    Q, l = apply36(h36, M, R, inverse)
    nan = check_nan_or_rotation(Q, l, f"inverse {inverse}, edges")
    print("  NaN:", list(names[nan]))
    for n in gx.ASKED_NAN + (("two_equal_rows",) if inverse else ()):
        assert nan[list(names).index(n)], n
    rng = np.random.default_rng(12)
    n = 2000
    Rn = rotations(n)
    U, V = np.linalg.qr(rng.standard_normal((n, 6, 6)))[0], np.linalg.qr(rng.standard_normal((n, 6, 6)))[0]
    for c in (1e4, 1e5, 1e6, 1e7, 1e8, np.inf):
        s = np.concatenate([np.ones((n, 1)), 10.0 ** rng.uniform(-3, 0, (n, 4)), np.full((n, 1), 1 / c)], 1) * 10.0 ** rng.uniform(-12, 12, (n, 1))
        Mc = np.einsum("nik,nk,njk->nij", U, s, V).astype(np.float32)
        check_nan_or_rotation(*apply36(h36, Mc, Rn, inverse), f"inverse {inverse}, cond {c:g}")
    base = np.eye(6) + 0.2 * rng.standard_normal((n, 6, 6))
    for eps in (1e-5, 1e-6, 1e-7):
        Mt = base.copy()
        Mt[:, 3:] = Mt[:, :3] * (1 + eps * rng.standard_normal((n, 3, 6)))
        check_nan_or_rotation(*apply36(h36, Mt.astype(np.float32), Rn, inverse), f"inverse {inverse}, lower rows within {eps:g} of the upper")
    for scale in gx.EXTREME_SCALES:
        Ms = (base * scale).astype(np.float32)
        Q, l = apply36(h36, Ms, Rn, inverse)
        nan = check_nan_or_rotation(Q, l, f"inverse {inverse}, scale {scale:g}")
        good = gx.in_domain(Ms)
        f = gx.rot_figure(Q, gx.gs36_64(Ms, Rn, inverse)[0], gx.kappa(Ms, Rn, inverse))
        assert good.mean() > 0.9 and not nan[good].any() and (f[good] <= 2 * strictest(inverse, "rot")).all(), (scale, int(nan[good].sum()), f[good].max())


# ---- scale covariance --------------------------------------------------------------------------------------------------------------------------

def test_power_of_two_scaling_changes_no_bit(h36):
    """f(2^k M) is bit-equal to f(M) for rotation and ldj, k = +-30, +-60."""
    n = 2000
    R = rotations(n)
    for kind in ("near_identity", "singular_values"):
        M = batch(kind, "realistic")[:n]
        for inverse in PASSES:
            Q, l = apply36(h36, M, R, inverse)
            assert np.isfinite(Q).all() and np.isfinite(l).all()
            for k in (-60, -30, 30, 60):
                Qk, lk = apply36(h36, np.ldexp(M, k), R, inverse)
                assert np.array_equal(Qk, Q) and np.array_equal(lk, l), (kind, inverse, k, int((Qk != Q).any((-1, -2)).sum()))


# ---- what the layer does to a rotation when M = I (the allowance of tests/test_gpu_gs36.py) ---------------------------------------------------

GS36_IDENTITY_UNITS = 5                                       # max|gs36(I, R) - R| over 20 000 fp32 rotations: 4.00 units of 2^-23 measured, and one
GS36_IDENTITY_LDJ_UNITS = 13                                  # max|ldj| there (the logarithm of a determinant 1 +- rounding): 12.00 units measured, and one


def test_gs36_of_identity_moves_a_rotation_by_rounding_only(h36):
    """cond_gs36_apply(I, R) re-normalises R (and replaces its third column by the cross product of the first two), so a device run with
    M = I does not return its input bit for bit.  How far it moves an fp32 rotation is measured here; tests/test_gpu_gs36.py adds these two
    numbers of units to its gates for that reason and no other."""
    R = rotations()
    I = np.broadcast_to(np.eye(6, dtype=np.float32), (len(R), 6, 6))
    for inverse in PASSES:
        Ro, l = apply36(h36, I, R, inverse)
        d = np.abs(Ro.astype(np.float64) - R).max() / U23
        print(f"gs36(I, R), inverse {inverse}: max|R' - R| = {d:.2f} units, max|ldj| = {np.abs(l).max() / U23:.2f} units")
        assert d <= GS36_IDENTITY_UNITS and np.abs(l).max() <= GS36_IDENTITY_LDJ_UNITS * U23


# ================================================================================================================================================
# the reverse step: so3_grad.h cond_gs36_backward
# ================================================================================================================================================

def backward36(h36, M, R, gR, gl, inverse):
    n = len(M)
    gM, gRin = np.zeros((n, 36), np.float32), np.zeros((n, 9), np.float32)
    h36.h36_backward(ptr(f32(np.asarray(M).reshape(n, 36))), ptr(f32(np.asarray(R).reshape(n, 9))), ptr(f32(np.asarray(gR).reshape(n, 9))),
                     ptr(f32(gl)), int(inverse), n, ptr(gM), ptr(gRin))
    return gM.reshape(-1, 6, 6), gRin.reshape(-1, 3, 3)


@functools.lru_cache(maxsize=None)
def cotangents(n=N_BATCH):
    rng = np.random.default_rng(78)
    gR, gl = rng.standard_normal((n, 3, 3)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    gR.setflags(write=False)
    gl.setflags(write=False)
    return gR, gl


COTANGENT_SETS = ("rot", "all")                              # g_ldj = 0, and random g_ldj beside the same gR


def references_grad(M, R, gR, gl, inverse, at=None):
    """fp64 autograd for both cotangent sets at once: {"rot": (dL/dM, dL/dR) with g_ldj = 0, "all": with g_ldj = gl}."""
    return {"rot": gx.layer_grad64(M, R, gR, np.zeros_like(gl), inverse, at=at), "all": gx.layer_grad64(M, R, gR, gl, inverse, at=at)}


def figures_grad(R, got, want, k, kl):
    """{set: (dL/dM figure, dL/dR tangent figure)} of `got` against `want` (both as references_grad returns them)."""
    return {s: (gx.grad_figure(got[s][0], want[s][0], want["rot"][0], k, kl), gx.tangent_figure(R, got[s][1], want[s][1], want["rot"][1], k, kl))
            for s in COTANGENT_SETS}


@functools.lru_cache(maxsize=None)
def yardstick_grad(inverse, kind, window, n=N_BATCH):
    """The backward yardstick on batch(kind, window): the batch maxima of the figures of fp64 autograd evaluated at the matrix recomposed
    from LAPACK's fp32 QR factors (gx.recomposed32), for both cotangent sets; and the fp64 gradients and conditionings themselves."""
    M, R = batch(kind, window, n), rotations(n)
    gR, gl = cotangents(n)
    k, kl = gx.grad_conditioning(M, R, inverse)
    want = references_grad(M, R, gR, gl, inverse)
    fig = figures_grad(R, references_grad(M, R, gR, gl, inverse, at=gx.recomposed32(M)), want, k, kl)
    vac = U23 * yardstick(inverse, kind, window, n)["kj"] > gx.LDJ_VACUOUS
    for a in (k, kl, vac) + tuple(x for s in COTANGENT_SETS for x in want[s]):
        a.setflags(write=False)
    return {"grad": {s: fig[s][0].max() for s in COTANGENT_SETS}, "tan": {s: fig[s][1].max() for s in COTANGENT_SETS},
            "want": want, "k": k, "kl": kl, "vacuous": vac}


def strictest_grad(inverse, key, cset):
    return min(yardstick_grad(inverse, k, w)[key][cset] for k, w in CASES)


def backward_gates(inverse, M, R, gR, gl, want, want_rot, k, kl, y_grad, y_tan):
    """Per-sample ABSOLUTE gates of dL/dM and of the tangent part of dL/dR: twice the yardstick's figure, turned back into an error
    (x 2^-23 (k max|rotation part| + kl max|ldj part|), the denominators of gx.grad_figure), plus 4 x 2^-23 times the size of the terms of
    the fp32 products the header forms.

    Why the second part (the argument of tests/test_gs3_host.py backward_gates).  The yardstick is fp64 autograd at a matrix 2^-23 away:
    it carries the conditioning of the gradient and none of the roundings an fp32 evaluation makes on the way.  Those are absolute errors
    of the size of what is multiplied, not of the result.  Where the reference gradient is small by cancellation (a cotangent nearly
    normal to what the layer can move) the figure alone, which divides by max|reference|, would hold the header to a relative accuracy no
    fp32 evaluation has.  The sizes of this layer's terms are derived in gx.product_terms."""
    tM, tR = gx.product_terms(M, R, gR, gl, inverse)
    den_M = k * gx._maxabs(want_rot[0]) + kl * gx._maxabs(want[0] - want_rot[0])
    den_R = k * gx._maxabs(gx.tangent(R, want_rot[1])) + kl * gx._maxabs(gx.tangent(R, want[1]) - gx.tangent(R, want_rot[1]))
    return 2 * y_grad * U23 * den_M + 4 * U23 * tM, 2 * y_tan * U23 * den_R + 4 * U23 * tR


def backward_errors(R, got, want):
    return gx._maxabs(got[0].astype(np.float64) - want[0]), gx._maxabs(gx.tangent(R, got[1]) - gx.tangent(R, want[1]))


@pytest.mark.parametrize("kind", gx.KINDS)
def test_gradient_conditioning_is_checked_by_a_perturbation(kind):
    """gx.grad_conditioning's derivation, checked: fp64 autograd at M (1 + 2^-23 U(-1, 1)), one rounding of every entry, shows figures of
    O(1) in both cotangent sets, both windows, both passes.  Thirty-six entries perturbed by 2^-23 |M_ij| make |E|_2 <= 2^-23 |M|_F <=
    sqrt(6) 2^-23 |M|_2, and the derivation's constants are 1 (rotation part) and 3 + 3 (ldj part): under 6 sqrt(6) < 15.  The figures
    divide by the size of the reference gradient itself, which a cotangent nearly normal to what the layer can move (three directions
    of nine) makes small by cancellation without making the perturbation's effect small: a tail no conditioning of the input removes
    (tests/test_gs3_host.py counts the same samples as "over twice"; the gates carry them by their product terms).  So the bound is
    asked of the 99.9th percentile of each cell and the maximum is printed.  The conditioning is a product of worst cases (cond(M) for a
    solve, cond(J) + rho for a determinant), which a random perturbation rarely meets, so the medians are small (down to 0.003 on the
    inverse pass); what is asked from below is that the worst sample of each cell comes within a factor ten of the bound, so that it is
    not an over-estimate by orders of magnitude in any cell.  The yardstick's own maxima are printed beside them."""
    for window in gx.WINDOWS:
        for inverse in PASSES:
            M, R, y = batch(kind, window), rotations(), yardstick_grad(inverse, kind, window)
            gR, gl = cotangents()
            fig = figures_grad(R, references_grad(M, R, gR, gl, inverse, at=gx.perturbed(M)), y["want"], y["k"], y["kl"])
            for s in COTANGENT_SETS:
                q = [np.quantile(f, 0.999) for f in fig[s]]
                md = [np.median(f) for f in fig[s]]
                print(f"{kind}, {window}, inverse {inverse}, cotangents {s}: figure of a 2^-23 perturbation, median / 99.9th percentile / max: dL/dM {md[0]:.3f} / {q[0]:.2f} / "
                      f"{fig[s][0].max():.2f}, dL/dR tangent {md[1]:.3f} / {q[1]:.2f} / {fig[s][1].max():.2f}; the yardstick's maxima {y['grad'][s]:.2f}, {y['tan'][s]:.2f}")
                assert q[0] < 15 and q[1] < 15 and fig[s][0].max() > 0.1 and fig[s][1].max() > 0.1, (window, inverse, s, q, md)
                assert np.isfinite(y["grad"][s]) and np.isfinite(y["tan"][s])


def test_gradient_reference_agrees_with_a_finite_difference():
    M, R = batch("singular_values", "realistic")[:4].astype(np.float64), rotations()[:4].astype(np.float64)
    gR, gl = (a[:4] for a in cotangents())
    E = np.random.default_rng(4).standard_normal((4, 6, 6))
    for inverse in PASSES:
        g = gx.layer_grad64(M, R, gR, gl, inverse)[0]

        def loss(A):
            Ro, l = gx.gs36_64(A, R, inverse)
            return (Ro * gR).sum((-1, -2)) + l * gl
        h = 1e-6 * np.abs(M).max((-1, -2), keepdims=True)
        fd = (loss(M + h * E) - loss(M - h * E)) / (2 * h[:, 0, 0])
        assert (np.abs(fd - (g * E).sum((-1, -2))) < 1e-4 * np.abs(g * E).sum((-1, -2))).all(), (inverse, fd, (g * E).sum((-1, -2)))


@pytest.mark.parametrize("kind,window", CASES)
@pytest.mark.parametrize("inverse", PASSES)
def test_every_sample_backward_is_the_fp64_gradient(h36, inverse, kind, window):
    """cond_gs36_backward, all 20 000 matrices of each family and scale window, both passes, uniform rotations, random normal cotangents,
    two sets: g_ldj = 0 and random g_ldj.  dL/dM and the tangent part of dL/dR per sample against fp64 autograd of the oracle's layer, each
    within 2x the figure fp64 autograd shows at the matrix recomposed from LAPACK fp32's QR factors, plus the 4 x 2^-23 of the fp32
    products (backward_gates).  No sample is left out of either set (the issue allows leaving the vacuous-ldj samples out of the second;
    the gates hold with them in); the share of samples whose forward ldj gate is vacuous is printed and must not exceed 0.12.  The
    gradient is finite on every sample: the forward returns a rotation on all of them."""
    M, R, y = batch(kind, window), rotations(), yardstick_grad(inverse, kind, window)
    gR, gl = cotangents()
    got = {"rot": backward36(h36, M, R, gR, np.zeros_like(gl), inverse), "all": backward36(h36, M, R, gR, gl, inverse)}
    fig = figures_grad(R, got, y["want"], y["k"], y["kl"])
    share = float(y["vacuous"].mean())
    for s in COTANGENT_SETS:
        eM, eR = backward_errors(R, got[s], y["want"][s])
        gate_M, gate_R = backward_gates(inverse, M, R, gR, gl if s == "all" else np.zeros_like(gl), y["want"][s], y["want"]["rot"], y["k"], y["kl"],
                                        y["grad"][s], y["tan"][s])
        g, t = fig[s]
        print(f"inverse {inverse}, {kind}, {window}, cotangents {s}: header / yardstick: dL/dM {g.max():.2f} / {y['grad'][s]:.2f} ({int((g > 2 * y['grad'][s]).sum())} over twice), "
              f"dL/dR tangent {t.max():.2f} / {y['tan'][s]:.2f} ({int((t > 2 * y['tan'][s]).sum())} over twice); error / gate max {np.max(eM / gate_M):.3f}, {np.max(eR / gate_R):.3f}; "
              f"vacuous ldj gates {share:.4f}")
        assert np.isfinite(got[s][0]).all() and np.isfinite(got[s][1]).all()
        assert (eM <= gate_M).all(), (s, int(np.argmax(eM / gate_M)), np.max(eM / gate_M), int((eM > gate_M).sum()))
        assert (eR <= gate_R).all(), (s, int(np.argmax(eR / gate_R)), np.max(eR / gate_R), int((eR > gate_R).sum()))
    assert share <= VACUOUS_MAX


@pytest.mark.parametrize("inverse", PASSES)
def test_in_domain_edges_backward(h36, inverse):
    """The named in-domain edges against the strictest yardstick of the twenty cells, both cotangent sets."""
    names, M, R, inside = gx.edges(inverse)
    names, M, R = np.array(names)[inside], M[inside], R[inside]
    n = len(M)
    gR, gl = (a[:n] for a in cotangents())
    k, kl = gx.grad_conditioning(M, R, inverse)
    want = references_grad(M, R, gR, gl, inverse)
    got = {"rot": backward36(h36, M, R, gR, np.zeros_like(gl), inverse), "all": backward36(h36, M, R, gR, gl, inverse)}
    for s in COTANGENT_SETS:
        eM, eR = backward_errors(R, got[s], want[s])
        gate_M, gate_R = backward_gates(inverse, M, R, gR, gl if s == "all" else np.zeros_like(gl), want[s], want["rot"], k, kl,
                                        strictest_grad(inverse, "grad", s), strictest_grad(inverse, "tan", s))
        print(f"inverse {inverse}, in-domain edges, cotangents {s}, dL/dM error / gate:", dict(zip(names, np.round(eM / gate_M, 3))))
        print("  dL/dR tangent error / gate:", dict(zip(names, np.round(eR / gate_R, 3))))
        assert (eM <= gate_M).all(), [(n_, v) for n_, v in zip(names, eM / gate_M) if not v <= 1]
        assert (eR <= gate_R).all(), [(n_, v) for n_, v in zip(names, eR / gate_R) if not v <= 1]


def test_backward_power_of_two_scaling_is_exact(h36):
    """dL/dM(2^k M) = 2^-k dL/dM(M) bit for bit and dL/dR unchanged, k = +-30, +-60, both passes, random g_ldj."""
    n = 2000
    R = rotations(n)
    gR, gl = (a[:n] for a in cotangents())
    for kind in ("near_identity", "singular_values"):
        M = batch(kind, "realistic")[:n]
        for inverse in PASSES:
            gM, gRin = backward36(h36, M, R, gR, gl, inverse)
            assert np.isfinite(gM).all() and np.isfinite(gRin).all()
            for k in (-60, -30, 30, 60):
                gMk, gRink = backward36(h36, np.ldexp(M, k), R, gR, gl, inverse)
                assert np.array_equal(gMk, np.ldexp(gM, -k)) and np.array_equal(gRink, gRin), (kind, inverse, k, int((gMk != np.ldexp(gM, -k)).any((-1, -2)).sum()))


@pytest.mark.parametrize("inverse", PASSES)
def test_backward_refuses_where_the_forward_refuses(h36, inverse):
    """A finite gradient never stands beside a NaN forward.  The named out-of-domain rows among in-domain rows: the rows asked to be NaN
    (gx.ASKED_NAN; two equal rows on the inverse pass) have NaN in ALL of gM and gRin, every other row is bit-equal to what it is in a
    batch without them.  Then 2 000 random matrices each of cond 1e4 .. 1e8 and of exact rank 5 at scales 10^U(-12,12), and 2 000 each
    with the lower rows within 1e-5 .. 1e-7 of the upper rows: gM and gRin are NaN throughout exactly on the rows whose forward is NaN,
    and hold no NaN elsewhere.  Last the ends of the fp32 range (gx.EXTREME_SCALES): inside the strictest in-domain gate."""
    names, M, R, inside = gx.edges(inverse)
    n = len(M)
    gR, gl = (a[:n] for a in cotangents())
    gM, gRin = backward36(h36, M, R, gR, gl, inverse)
    Q, l = apply36(h36, M, R, inverse)
    fwd_nan = np.isnan(Q).all((-1, -2)) & np.isnan(l)
    all_nan = np.isnan(gM).all((-1, -2)) & np.isnan(gRin).all((-1, -2))
    any_nan = np.isnan(gM).any((-1, -2)) | np.isnan(gRin).any((-1, -2))
    print(f"inverse {inverse}: NaN gradient rows:", [nm for nm, b in zip(names, all_nan) if b])
    for nm in gx.ASKED_NAN + (("two_equal_rows",) if inverse else ()):
        assert all_nan[names.index(nm)], nm
    assert np.array_equal(all_nan, fwd_nan) and np.array_equal(any_nan, all_nan), (list(zip(names, fwd_nan, all_nan, any_nan)))
    gM_in, gRin_in = backward36(h36, M[inside], R[inside], gR[inside], gl[inside], inverse)
    assert np.array_equal(gM[inside], gM_in) and np.array_equal(gRin[inside], gRin_in) and np.isfinite(gM_in).all() and np.isfinite(gRin_in).all()
    rng = np.random.default_rng(12)
    n = 2000
    Rn = rotations(n)
    gR, gl = (a[:n] for a in cotangents())

    def same_rows(Mc, tag):
        Q, l = apply36(h36, Mc, Rn, inverse)
        gM, gRin = backward36(h36, Mc, Rn, gR, gl, inverse)
        fwd_nan = np.isnan(Q).all((-1, -2)) & np.isnan(l)
        all_nan = np.isnan(gM).all((-1, -2)) & np.isnan(gRin).all((-1, -2))
        any_nan = np.isnan(gM).any((-1, -2)) | np.isnan(gRin).any((-1, -2))
        print(f"inverse {inverse}, {tag}: forward NaN on {int(fwd_nan.sum())} of {n}, gradient NaN on {int(all_nan.sum())}")
        assert np.array_equal(all_nan, fwd_nan) and np.array_equal(any_nan, all_nan), (tag, int((all_nan != fwd_nan).sum()), int((any_nan != all_nan).sum()))
    U, V = np.linalg.qr(rng.standard_normal((n, 6, 6)))[0], np.linalg.qr(rng.standard_normal((n, 6, 6)))[0]
    for c in (1e4, 1e5, 1e6, 1e7, 1e8, np.inf):
        s = np.concatenate([np.ones((n, 1)), 10.0 ** rng.uniform(-3, 0, (n, 4)), np.full((n, 1), 1 / c)], 1) * 10.0 ** rng.uniform(-12, 12, (n, 1))
        same_rows(np.einsum("nik,nk,njk->nij", U, s, V).astype(np.float32), f"cond {c:g}")
    base = np.eye(6) + 0.2 * rng.standard_normal((n, 6, 6))
    for eps in (1e-5, 1e-6, 1e-7):
        Mt = base.copy()
        Mt[:, 3:] = Mt[:, :3] * (1 + eps * rng.standard_normal((n, 3, 6)))
        same_rows(Mt.astype(np.float32), f"lower rows within {eps:g} of the upper")
    for scale in gx.EXTREME_SCALES:
        Ms = (base * scale).astype(np.float32)
        good = gx.in_domain(Ms)
        Mg, Rg, gRg, glg = Ms[good], Rn[good], gR[good], gl[good]
        k, kl = gx.grad_conditioning(Mg, Rg, inverse)
        want = references_grad(Mg, Rg, gRg, glg, inverse)
        got = backward36(h36, Mg, Rg, gRg, glg, inverse)
        eM, eR = backward_errors(Rg, got, want["all"])
        gate_M, gate_R = backward_gates(inverse, Mg, Rg, gRg, glg, want["all"], want["rot"], k, kl, strictest_grad(inverse, "grad", "all"),
                                        strictest_grad(inverse, "tan", "all"))
        print(f"inverse {inverse}, scale {scale:g}: error / gate max {np.max(eM / gate_M):.3f}, {np.max(eR / gate_R):.3f}")
        assert good.mean() > 0.9 and np.isfinite(got[0]).all() and (eM <= gate_M).all() and (eR <= gate_R).all(), (scale, np.max(eM / gate_M), np.max(eR / gate_R))
