"""CPU: the per-sample 4x4 layer Condition16Trans (csrc/so3_math.h cond16_apply = power-of-two prescale, a triangular factorisation for
log|det M| and for the solve M t = q of the inverse pass, calculate_16; csrc/so3_grad.h cond16_backward, which takes M^-1 from a pivoted
Gauss-Jordan elimination as inv4 does), host build without contraction,
EVERY sample against fp64 (tests/aff16_exact.py) over the whole gated domain: cond(M) <= 1e3 at every scale, det < 0 included.

The yardstick of every gate is LAPACK's own fp32 route on the same batch, computed inside the test (aff16_exact.lapack32:
torch.linalg.inv, torch.linalg.slogdet and the matrix-vector product in fp32 on the fp64 quaternion rounded once).  Per sample:
    |R' - R'64|    <= 2 x (yardstick's batch maximum) x 2^-23 kappa + 4 x 2^-23            (the 4-term products t = M q)
    |ldj - ldj64|  <= 2 x (yardstick's batch maximum) x 2^-23 kappa + 2^-24 x (|log|det Ms|| + 4 |log|t||)   (the logarithms the routine adds)
    |R'R'^T - I|   <= 2 x the yardstick's own;  det R' > 0.5
with kappa = cond_2(M) in both passes.  The measured table (header / LAPACK fp32 per kind, window and pass) and the parent's figures:
DESIGN.md section 3.7c.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import flow_oracle as orc
from rotationnormflow_amd import synth
from tests import aff16_exact as ax
from tests.test_host_math import f32, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_aff16.cpp")
OUT = os.path.join(HERE, "csrc", "_host_aff16.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", h) for h in ("so3_math.h", "so3_grad.h")]

U23 = ax.U23
N_BATCH = 20000
ORTH_NAN = 16 * U23                                          # what "a rotation" means outside the domain (kPolar3Orth of the 3x3 siblings)
CASES = [(k, w) for w in ax.WINDOWS for k in ax.KINDS]
PASSES = (False, True)


@pytest.fixture(scope="module")
def ha():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    return C.CDLL(OUT)


def cond16(ha, M, R, inverse):
    A, r = f32(np.asarray(M).reshape(-1, 16)), f32(np.asarray(R).reshape(-1, 9))
    Ro, l = np.empty_like(r), np.empty(len(A), np.float32)
    ha.ha_cond16(ptr(A), ptr(r), int(inverse), len(A), ptr(Ro), ptr(l))
    return Ro.reshape(-1, 3, 3), l


def cond16_backward(ha, M, R, inverse, gR, gl):
    n = len(M)
    gM, gRin = np.zeros((n, 16), np.float32), np.zeros((n, 9), np.float32)
    ha.ha_cond16_backward(ptr(f32(np.asarray(M).reshape(-1, 16))), ptr(f32(np.asarray(R).reshape(-1, 9))), int(inverse),
                          ptr(f32(np.asarray(gR).reshape(-1, 9))), ptr(f32(gl)), n, ptr(gM), ptr(gRin))
    return gM.reshape(-1, 4, 4), gRin.reshape(-1, 3, 3)


@functools.lru_cache(maxsize=None)
def batch(kind, window, n=N_BATCH):
    M, keep = ax.random_batch(kind, n, 1, ax.WINDOWS[window])
    assert keep >= 0.98, (kind, window, keep)                 # the domain keeps at least 0.98 of what was drawn; nothing of a batch is left out
    assert ax.in_domain(M).all()
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def rotations(n=N_BATCH):
    R = synth.uniform_rotations(n, seed=23).astype(np.float32)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def cotangents(n=N_BATCH):
    rng = np.random.default_rng(79)
    gR, gl = rng.standard_normal((n, 3, 3)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    gR.setflags(write=False)
    gl.setflags(write=False)
    return gR, gl


# ---- the yardstick: LAPACK fp32 on the same matrices, computed once per batch and shared ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def yardstick(inverse, kind, window, n=N_BATCH):
    M, R = batch(kind, window, n), rotations(n)
    k = ax.cond(M)
    want, want_l = ax.layer64(M, R, inverse)
    Q32, l32 = ax.lapack32(M, R, inverse)
    for a in (want, want_l):
        a.setflags(write=False)
    return {"rot": ax.rot_figure(Q32, want, k).max(), "ldj": ax.ldj_figure(l32, want_l, k).max(), "orth": ax.orth_err(Q32).max(),
            "want": want, "want_ldj": want_l, "kappa": k, "log_terms": ax.log_terms(M, R, inverse)}


@functools.lru_cache(maxsize=None)
def yardstick_grad(inverse, kind, window, n=N_BATCH):
    """What fp32 factors cost a gradient: the batch maxima of the figures of fp64 autograd evaluated at the matrix recomposed from LAPACK's
    fp32 LU factors; and the fp64 gradients themselves (read-only)."""
    M, R = batch(kind, window, n), rotations(n)
    gR, gl = cotangents(n)
    k = ax.cond(M)
    gM, gRin = ax.layer_grad64(M, R, gR, gl, inverse)
    gM32, gRin32 = ax.layer_grad64(M, R, gR, gl, inverse, at=ax.recomposed(M))
    gM.setflags(write=False)
    gRin.setflags(write=False)
    return {"grad": ax.grad_figure(gM32, gM, k).max(), "tan": ax.tangent_figure(R, gRin32, gRin, k).max(), "gM": gM, "gRin": gRin}


def strictest(inverse, key):
    """The smallest of the batch yardsticks: the gate of inputs that belong to no batch (the named edges)."""
    fn = yardstick_grad if key in ("grad", "tan") else yardstick
    return min(fn(inverse, k, w)[key] for k, w in CASES)


def forward_gates(y_rot, y_ldj, k, log_terms):
    return 2 * y_rot * U23 * k + 4 * U23, 2 * y_ldj * U23 * k + 0.5 * U23 * log_terms


# ---- the reference and the yardstick themselves ------------------------------------------------------------------------------------------

def test_reference_is_the_oracles_layer():
    """aff16_exact.layer64 (numpy, restated from the rule) against oracle.affine16 (pinned to the reference) in fp64, both passes; the torch
    restatement used for autograd against both; degree 0 in M; a finite difference against the fp64 gradient; the figure helpers."""
    M, R = batch("singular_values", "realistic", 2000).astype(np.float64), rotations(2000).astype(np.float64)
    gR, gl = (a[:2000] for a in cotangents())
    for inverse in PASSES:
        Ro, l = ax.layer64(M, R, inverse)
        A = torch.from_numpy(np.linalg.inv(M) if inverse else M)
        Rw, lw = orc.affine16(A, torch.from_numpy(R))
        assert np.abs(Ro - Rw.numpy()).max() < 1e-9 and np.abs(l - lw.numpy()).max() < 1e-8
        Rt, lt = ax.layer_torch(torch.from_numpy(M), torch.from_numpy(R), inverse)
        assert np.abs(Ro - Rt.numpy()).max() < 1e-9 and np.abs(l - lt.numpy()).max() < 1e-9
        assert ax.orth_err(Ro).max() < 1e-12 and np.allclose(np.linalg.det(Ro), 1.0)
        for c in (2.0 ** -40, 3.0):
            Rc, lc = ax.layer64(c * M, R, inverse)
            assert np.abs(Rc - Ro).max() < 1e-9 and np.abs(lc - l).max() < 1e-9
        g = ax.layer_grad64(M[:1], R[:1], gR[:1], gl[:1], inverse)[0]
        E = np.random.default_rng(4).standard_normal((1, 4, 4))

        def loss(X):
            Ro_, l_ = ax.layer64(X, R[:1], inverse)
            return float((Ro_ * gR[:1]).sum() + (l_ * gl[:1]).sum())
        h = 1e-6 * np.abs(M[0]).max()
        fd = (loss(M[:1] + h * E) - loss(M[:1] - h * E)) / (2 * h)
        assert abs(fd - (g * E).sum()) < 1e-5 * np.abs(g).max(), (inverse, fd, (g * E).sum())
    k = ax.cond(M)
    Ro, _ = ax.layer64(M, R)
    Qb = Ro.copy()
    Qb[5, 1, 2] += 3 * U23 * k[5]
    Qb[6, 0, 0] = np.nan
    f = ax.rot_figure(Qb, Ro, k)
    assert abs(f[5] - 3) < 1e-6 and np.isinf(f[6]) and f[7] == 0
    s = np.linalg.svd(M, compute_uv=False)
    assert np.allclose(k, s[:, 0] / s[:, 3])


@pytest.mark.parametrize("kind", ax.KINDS)
def test_lapack_fp32_is_order_one_in_the_conditioned_measure(kind):
    """The yardstick's own figures.  LU with partial pivoting of a 4x4 is backward stable with a constant of a few tens of 2^-24, so the
    rotation figure lies between 1/4 and 36 and R' is orthogonal to 36 units.  LAPACK's ldj adds log|det M| and 4 log|t| at the scale of M
    itself: each is rounded to 2^-24 of its own size, whatever kappa, so its figure is bounded by 36 + the largest such sum in units."""
    for window in ax.WINDOWS:
        for inverse in PASSES:
            y = {**yardstick(inverse, kind, window), **yardstick_grad(inverse, kind, window)}
            M, R = batch(kind, window), rotations()
            A = np.linalg.inv(M.astype(np.float64)) if inverse else M.astype(np.float64)
            logs = np.abs(np.linalg.slogdet(M.astype(np.float64))[1]) + 4 * np.abs(np.log(np.linalg.norm(np.einsum("nij,nj->ni", A, ax.quat64(R)), axis=1)))
            print(f"{kind}, {window}, inverse {inverse}: LAPACK fp32 rotation {y['rot']:.2f}, ldj {y['ldj']:.2f}, |R'R'^T - I| {y['orth'] / U23:.2f} units, "
                  f"dL/dM {y['grad']:.2f}, dL/dR tangent {y['tan']:.2f}")
            assert 0.25 < y["rot"] < 36 and y["ldj"] < 36 + 0.5 * logs.max() and y["orth"] < 36 * U23 and 0.25 < y["grad"] < 144 and y["tan"] < 144


# ---- forward: every sample ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,window", CASES)
@pytest.mark.parametrize("inverse", PASSES)
def test_every_sample_is_the_fp64_layer(ha, inverse, kind, window):
    """All 20 000 matrices of each kind and scale window, both passes: the gates of the module docstring."""
    M, R, y = batch(kind, window), rotations(), yardstick(inverse, kind, window)
    k = y["kappa"]
    Q, l = cond16(ha, M, R, inverse)
    eR, el, o = ax.rot_error(Q, y["want"]), ax.ldj_error(l, y["want_ldj"]), ax.orth_err(Q)
    gate_R, gate_l = forward_gates(y["rot"], y["ldj"], k, y["log_terms"])
    print(f"inverse {inverse}, {kind}, {window}: header / LAPACK fp32: rotation {(eR / (U23 * k)).max():.2f} / {y['rot']:.2f}, "
          f"ldj {(el / (U23 * k)).max():.2f} / {y['ldj']:.2f}, |R'R'^T - I| {o.max() / U23:.2f} / {y['orth'] / U23:.2f} units; "
          f"error / gate max {np.max(eR / gate_R):.3f}, {np.max(el / gate_l):.3f}; non-finite rows {int((~np.isfinite(eR + el)).sum())}")
    assert (eR <= gate_R).all(), (int(np.argmax(eR / gate_R)), np.max(eR / gate_R), int((eR > gate_R).sum()))
    assert (el <= gate_l).all(), (int(np.argmax(el / gate_l)), np.max(el / gate_l), int((el > gate_l).sum()))
    assert o.max() <= 2 * y["orth"], (o.max() / U23, y["orth"] / U23, int((o > 2 * y["orth"]).sum()))
    assert (np.linalg.det(Q.astype(np.float64)) > 0.5).all()


@pytest.mark.parametrize("inverse", PASSES)
def test_in_domain_edges(ha, inverse):
    M, names = ax.EDGE_STACK[ax.EDGE_IN], np.array(ax.EDGE_NAMES)[ax.EDGE_IN]
    R = rotations(len(M))
    k = ax.cond(M)
    want, want_l = ax.layer64(M, R, inverse)
    Q, l = cond16(ha, M, R, inverse)
    eR, el, o = ax.rot_error(Q, want), ax.ldj_error(l, want_l), ax.orth_err(Q)
    gate_R, gate_l = forward_gates(strictest(inverse, "rot"), strictest(inverse, "ldj"), k, ax.log_terms(M, R, inverse))
    gate_o = 2 * strictest(inverse, "orth")
    print(f"inverse {inverse}, in-domain edges, rotation error / gate:", dict(zip(names, np.round(eR / gate_R, 3))))
    print("  ldj error / gate:", dict(zip(names, np.round(el / gate_l, 3))))
    print("  |R'R'^T - I| in units:", dict(zip(names, np.round(o / U23, 2))), "gate", gate_o / U23)
    assert (eR <= gate_R).all(), [(n, v) for n, v in zip(names, eR / gate_R) if v > 1]
    assert (el <= gate_l).all(), [(n, v) for n, v in zip(names, el / gate_l) if v > 1]
    assert (o <= gate_o).all(), [(n, v / U23) for n, v in zip(names, o) if v > gate_o]
    assert (np.linalg.det(Q.astype(np.float64)) > 0.5).all()


def check_nan_or_rotation(Q, l, tag):
    """Out of the domain: R' all NaN, or finite and orthogonal to 16 units; ldj finite beside a rotation and nowhere else."""
    o = ax.orth_err(Q)
    nan = np.isnan(Q).all((-1, -2))
    rot = np.isfinite(Q).all((-1, -2)) & (o <= ORTH_NAN)
    print(f"{tag}: {int(nan.sum())} of {len(Q)} NaN, the rest orthogonal to {o[~nan].max() / U23 if (~nan).any() else 0:.1f} units")
    assert (nan | rot).all(), (tag, int((~(nan | rot)).sum()), Q[~(nan | rot)][:2])
    assert np.array_equal(np.isfinite(l), rot), tag
    return nan


@pytest.mark.parametrize("inverse", PASSES)
def test_out_of_domain_is_nan_or_a_rotation(ha, inverse):
    """Rank 3, rank 1, zero, one NaN entry, one infinite entry; M q = 0 exactly; 2000 random matrices each of cond 1e4 .. 1e12 and of exact
    rank 3, at scales 10^U(-12,12); and the ends of the fp32 range, 10^+-19.5, 1e21, 1e-20, 1e30, 1e-30 times (I + 0.3 N), where the parent
    returned R' = I (|M q|^2 overflowing) or a finite wrong ldj."""
    M, names = ax.EDGE_STACK[~ax.EDGE_IN], np.array(ax.EDGE_NAMES)[~ax.EDGE_IN]
    Q, l = cond16(ha, M, rotations(len(M)), inverse)
    nan = check_nan_or_rotation(Q, l, f"inverse {inverse}, edges")
    print("  NaN:", list(names[nan]))
    for n in ("zero", "rank1", "one_nan", "one_inf"):                               # rank3 is of rank 3 only up to its rounding to fp32
        assert nan[list(names).index(n)], n
    # M q = 0 on the forward pass: rows of M normal to q (dyadic q = (1, 0, 0, 0) from R = I)
    Z = np.array([[0, 1, 2, 3], [0, -1, 0.5, 2], [0, 4, 1, 1], [0, 2, 2, -1]], np.float32)[None]
    Q, l = cond16(ha, Z, np.eye(3, dtype=np.float32)[None], False)
    assert np.isnan(Q).all() and not np.isfinite(l).any()
    rng = np.random.default_rng(12)
    n = 2000
    R = rotations(n)
    U, V = np.linalg.qr(rng.standard_normal((n, 4, 4)))[0], np.linalg.qr(rng.standard_normal((n, 4, 4)))[0]
    for c in (1e4, 1e6, 1e8, 1e12, np.inf):
        s = np.stack([np.ones(n), 10.0 ** rng.uniform(-3, 0, n), 10.0 ** rng.uniform(-3, 0, n), np.full(n, 1 / c)], 1) * 10.0 ** rng.uniform(-12, 12, (n, 1))
        Mc = np.einsum("nik,nk,njk->nij", U, s, V).astype(np.float32)
        Q, l = cond16(ha, Mc, R, inverse)
        check_nan_or_rotation(Q, l, f"inverse {inverse}, cond {c:g}")
    base = np.eye(4) + 0.3 * rng.standard_normal((n, 4, 4))
    for scale in (10.0 ** 19.5, 10.0 ** -19.5, 1e21, 1e-20, 1e30, 1e-30, 1e13, 1e-13):
        Ms = (base * scale).astype(np.float32)
        Q, l = cond16(ha, Ms, R, inverse)
        nan = check_nan_or_rotation(Q, l, f"inverse {inverse}, scale {scale:g}")
        good = ax.cond(Ms) <= ax.COND_MAX                                           # in the domain but for the scale: the layer's answer, not a NaN
        k = ax.cond(Ms)
        want, want_l = ax.layer64(Ms, R, inverse)
        gate_R, gate_l = forward_gates(strictest(inverse, "rot"), strictest(inverse, "ldj"), k, ax.log_terms(Ms, R, inverse))
        eR, el = ax.rot_error(Q, want), ax.ldj_error(l, want_l)
        assert not nan[good].any() and (eR[good] <= gate_R[good]).all() and (el[good] <= gate_l[good]).all(), (scale, int(nan[good].sum()))


# ---- scale covariance ----------------------------------------------------------------------------------------------------------------------

def test_power_of_two_scaling_changes_no_bit(ha):
    """f(2^k M) is bit-equal to f(M) for R' and ldj, k = +-30, +-60; dL/dM(2^k M) = 2^-k dL/dM(M) bit for bit, dL/dR unchanged."""
    n = 2000
    R = rotations(n)
    gR, gl = (a[:n] for a in cotangents())
    for kind in ("near_identity", "singular_values", "normal_negdet"):
        M = batch(kind, "realistic", n)
        for inverse in PASSES:
            Q, l = cond16(ha, M, R, inverse)
            gM, gRin = cond16_backward(ha, M, R, inverse, gR, gl)
            assert np.isfinite(Q).all() and np.isfinite(l).all() and np.isfinite(gM).all() and np.isfinite(gRin).all()
            for k in (-60, -30, 30, 60):
                Mk = np.ldexp(M, k)
                Qk, lk = cond16(ha, Mk, R, inverse)
                assert np.array_equal(Qk, Q) and np.array_equal(lk, l), (kind, inverse, k, int((Qk != Q).any((-1, -2)).sum()))
                gMk, gRink = cond16_backward(ha, Mk, R, inverse, gR, gl)
                assert np.array_equal(gMk, np.ldexp(gM, -k)) and np.array_equal(gRink, gRin), (kind, inverse, k)


# ---- the other callers of the 4x4 inverse ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", list(ax.WINDOWS))
def test_inv4_over_the_domain(ha, window):
    """inv4 (Condition16TransLU's side matrices, the constant affine layer's inverse in training, affine_logdet_grad_kernel) at the scale of M:
    max|inv4(M) - M^-1| / max|M^-1| per sample within twice torch.linalg.inv's fp32 figure on the same batch, in units of 2^-23 kappa, and
    det(M) to 2^-23 kappa-free relative accuracy x 16 where it is inside the fp32 range."""
    M = batch("singular_values", window)
    k = ax.cond(M)
    A = f32(M.reshape(-1, 16))
    Mi, det = np.empty_like(A), np.empty(len(A), np.float32)
    ha.ha_inv4(ptr(A), len(A), ptr(Mi), ptr(det))
    want = np.linalg.inv(M.astype(np.float64))
    y = ax.grad_figure(torch.linalg.inv(torch.from_numpy(M.copy())).numpy(), want, k).max()
    f = ax.grad_figure(Mi.reshape(-1, 4, 4), want, k)
    sign, lad = np.linalg.slogdet(M.astype(np.float64))
    inside = np.abs(lad) < 80                                                        # e^+-80: inside the fp32 normal range
    print(f"inv4, {window}: header / LAPACK fp32 {f.max():.2f} / {y:.2f}; det checked on {int(inside.sum())} of {len(M)}")
    assert f.max() <= 2 * y, (f.max(), y, int((f > 2 * y).sum()))
    assert (np.abs(det[inside] / (sign * np.exp(lad))[inside] - 1) <= 16 * U23 * k[inside]).all()


# ---- backward: every sample ----------------------------------------------------------------------------------------------------------------

def backward_gates(inverse, M, gR, gl, want_M, want_R, R, y_grad, y_tan):
    """Per-sample ABSOLUTE gates of dL/dM and of the tangent part of dL/dR: twice the yardstick's figure, turned back into an error
    (x 2^-23 kappa max|reference|), plus 4 x 2^-23 times the size of the terms of the 4-term fp32 products the header forms.

    The terms.  With c_R = max|gR'|, c_l = |g_ldj|, c = max(c_R, c_l), s_min the smallest singular value of M and |q| = 1:
      * R' = I + (2 / |t|^2) Q(t), Q quadratic with coefficients 1 and 2 (so3_grad.h affine16_backward_t), so
        dL/dt = (2 / |t|^2) (sum of gR' x 2 t) - (gR' . Q) (2 / |t|^4) 2 t - (2 g_ldj / |t|^2) 2 t is a sum of terms of size up to 4 c / |t|,
        each rounded to 2^-23 of itself however small the sum comes out.
      * forward pass, |t| >= s_min:  dL/dM = (dL/dt) q^T + g_ldj M^-T.  The first has terms 4 c / s_min.  The second is formed from the
        COMPUTED inverse, whose entries are off by 2^-23 kappa |M^-1| = 2^-23 kappa / s_min however the sum cancels: c_l kappa / s_min.
      * inverse pass, t = M^-1 q, |t| >= 1 / s_max:  dL/dq = M^-T dL/dt with terms (1 / s_min)(4 c / |t|), and
        dL/dM = -(dL/dq) t^T - g_ldj M^-T: terms 4 c / s_min, formed from the computed inverse and the computed t (each 2^-23 kappa off):
        4 c kappa / s_min.
      * dL/dR goes through dL/dq = A^T dL/dt: terms |A| 4 c / |t| <= 4 kappa c in both passes; the quaternion's reverse step divides by
        2 max(a, 0.1) >= 2 and adds nothing larger.
    Where the reference gradient is small by cancellation the figure alone, which divides by max|reference|, would hold the header to a
    relative accuracy no fp32 evaluation has; the test prints how many samples exceed twice the yardstick without this term.

    What the gate amounts to.  The terms that carry kappa / s_min scale as the main term does (max|reference| ~ c / s_min on the forward,
    c kappa / s_min at most on the inverse pass), so for a sample without cancellation the gate is (2 y + 4 x 4) / y yardsticks on the
    inverse pass, about 4 to 6 with y = 4 .. 7, not 2; on the forward pass the kappa-carrying share is g_ldj's alone.  The test prints
    error / gate (at most 0.53 on the host build), and the count of samples over twice the yardstick alone, for that reason."""
    k = ax.cond(M)
    s_min = ax.svals(M)[:, -1]
    c_R, c_l = np.abs(gR).reshape(len(M), -1).max(-1), np.abs(gl)
    c = np.maximum(c_R, c_l)
    terms_M = 4 * c * k / s_min if inverse else (4 * c + c_l * k) / s_min
    terms_R = 4 * c * k
    gate_M = 2 * y_grad * U23 * k * ax._maxabs(want_M) + 4 * U23 * terms_M
    gate_R = 2 * y_tan * U23 * k * ax._maxabs(ax.tangent(R, want_R)) + 4 * U23 * terms_R
    return gate_M, gate_R


def backward_errors(R, gM, gRin, want_M, want_R):
    return ax._maxabs(gM.astype(np.float64) - want_M), ax._maxabs(ax.tangent(R, gRin) - ax.tangent(R, want_R))


@pytest.mark.parametrize("kind,window", CASES)
@pytest.mark.parametrize("inverse", PASSES)
def test_every_sample_backward_is_the_fp64_gradient(ha, inverse, kind, window):
    """cond16_backward, forward and inverse pass, uniform rotations, random normal cotangents of R' and ldj: dL/dM and the tangent part of
    dL/dR per sample against fp64 autograd of the fp64 layer, each within 2x the figure fp64 autograd shows at the matrix recomposed from
    LAPACK fp32's LU factors, plus the 4 x 2^-23 of the fp32 products (backward_gates)."""
    M, R, y = batch(kind, window), rotations(), yardstick_grad(inverse, kind, window)
    gR, gl = cotangents()
    k = ax.cond(M)
    gM, gRin = cond16_backward(ha, M, R, inverse, gR, gl)
    g, t = ax.grad_figure(gM, y["gM"], k), ax.tangent_figure(R, gRin, y["gRin"], k)
    eM, eR = backward_errors(R, gM, gRin, y["gM"], y["gRin"])
    gate_M, gate_R = backward_gates(inverse, M, gR, gl, y["gM"], y["gRin"], R, y["grad"], y["tan"])
    print(f"inverse {inverse}, {kind}, {window}: header / LAPACK fp32: dL/dM {g.max():.2f} / {y['grad']:.2f} ({int((g > 2 * y['grad']).sum())} over twice), "
          f"dL/dR tangent {t.max():.2f} / {y['tan']:.2f} ({int((t > 2 * y['tan']).sum())} over twice); error / gate max {np.max(eM / gate_M):.3f}, {np.max(eR / gate_R):.3f}")
    assert (eM <= gate_M).all(), (int(np.argmax(eM / gate_M)), np.max(eM / gate_M), int((eM > gate_M).sum()))
    assert (eR <= gate_R).all(), (int(np.argmax(eR / gate_R)), np.max(eR / gate_R), int((eR > gate_R).sum()))


@pytest.mark.parametrize("inverse", PASSES)
def test_in_domain_edges_backward(ha, inverse):
    M, names = ax.EDGE_STACK[ax.EDGE_IN], np.array(ax.EDGE_NAMES)[ax.EDGE_IN]
    n = len(M)
    R = rotations(n)
    gR, gl = (a[:n] for a in cotangents())
    wM, wR = ax.layer_grad64(M, R, gR, gl, inverse)
    gM, gRin = cond16_backward(ha, M, R, inverse, gR, gl)
    eM, eR = backward_errors(R, gM, gRin, wM, wR)
    gate_M, gate_R = backward_gates(inverse, M, gR, gl, wM, wR, R, strictest(inverse, "grad"), strictest(inverse, "tan"))
    print(f"inverse {inverse}, in-domain edges, dL/dM error / gate:", dict(zip(names, np.round(eM / gate_M, 3))))
    print("  dL/dR tangent error / gate:", dict(zip(names, np.round(eR / gate_R, 3))))
    assert (eM <= gate_M).all(), [(n_, v) for n_, v in zip(names, eM / gate_M) if v > 1]
    assert (eR <= gate_R).all(), [(n_, v) for n_, v in zip(names, eR / gate_R) if v > 1]


# ---- what the layer does to a rotation when M = I (the allowance of tests/test_gpu_aff16.py) -------------------------------------------------

AFF16_IDENTITY_UNITS = 4                                      # max|cond16(I, R) - R| over 20 000 fp32 rotations: 4.00 units of 2^-23 measured
AFF16_IDENTITY_LDJ_UNITS = 7                                  # max|ldj| there (-2 log of |quat(R)|^2 = 1 +- rounding): 6.00 units and a hair measured, rounded up


def test_identity_moves_a_rotation_by_rounding_only(ha):
    """cond16_apply(I, R) = rot(quat(R)) re-normalises R, so a device run with M = I does not return its input bit for bit.  How far it
    moves an fp32 rotation is measured here; tests/test_gpu_aff16.py adds these two numbers of units to its gates for that reason only."""
    R = rotations()
    I = np.broadcast_to(np.eye(4, dtype=np.float32), (len(R), 4, 4))
    for inverse in PASSES:
        Ro, l = cond16(ha, I, R, inverse)
        d = np.abs(Ro.astype(np.float64) - R).max() / U23
        print(f"cond16(I, R), inverse {inverse}: max|R' - R| = {d:.2f} units, max|ldj| = {np.abs(l).max() / U23:.2f} units")
        assert d <= AFF16_IDENTITY_UNITS and np.abs(l).max() <= AFF16_IDENTITY_LDJ_UNITS * U23
