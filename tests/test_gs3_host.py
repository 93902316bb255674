"""CPU: the per-sample 3x3 Gram-Schmidt layers (csrc/so3_math.h smith3 and cond_gs9_apply, csrc/so3_grad.h cond9_backward for
RNF_KIND_COND9_GS / _SMITH), host build without contraction, EVERY sample against fp64 (tests/gs3_exact.py) over the whole gated domain of
tests/polar3_exact.py: cond(M) <= 1e3 at every scale, det < 0 included.

The yardstick of every gate is LAPACK's own fp32 route on the same matrices, computed inside the test: ``torch.linalg.qr`` in fp32 of M
(Smith), of fl(M R) (calculate_9 forward) and of ``torch.linalg.inv(M) @ R`` (calculate_9 inverse), signs fixed and the third column replaced by
the cross product.  The header may show twice the yardstick's batch maximum of the same figure.  Figures are in units of 2^-23 kappa
(kappa2 = s1 / s2 of M[:, :2] for Smith, cond(M) for calculate_9); |Q Q^T - I| is in units of 2^-23 and not divided.
The measured table (header / LAPACK fp32, per kind and window) and the parent's figures: DESIGN.md section 3.7b.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from rotationnormflow_amd import synth
from tests import gs3_exact as gx
from tests import polar3_exact as px
from tests.test_host_grad import f32, hg, ptr  # noqa: F401  (hg: the host build of so3_grad.h with hg_cond9, a fixture)
from tests.test_polar3_host import CASES, N_BATCH, batch

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_gs3.cpp")
OUT = os.path.join(HERE, "csrc", "_host_gs3.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", "so3_math.h")]

U23 = px.U23
ORTH_NAN = 16 * U23                                          # kPolar3Orth: what the header itself accepts as a rotation
LAYERS = {"gs9": 6, "smith": 7}                              # RNF_KIND_COND9_GS, RNF_KIND_COND9_SMITH
PASSES = [("gs9", False), ("gs9", True), ("smith", False), ("smith", True)]


@pytest.fixture(scope="module")
def hs():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    return C.CDLL(OUT)


def smith3(hs, M):
    A = f32(np.asarray(M).reshape(-1, 9))
    Q = np.empty_like(A)
    hs.hs_smith3(ptr(A), ptr(Q), len(A))
    return Q.reshape(-1, 3, 3)


def gs9(hs, M, R, inverse):
    A, r = f32(np.asarray(M).reshape(-1, 9)), f32(np.asarray(R).reshape(-1, 9))
    Ro, l = np.empty_like(A), np.empty(len(A), np.float32)
    hs.hs_gs9(ptr(A), ptr(r), int(inverse), len(A), ptr(Ro), ptr(l))
    return Ro.reshape(-1, 3, 3), l


def cond9(hg, name, inverse, M, R, gR, gl):
    n = len(M)
    gM, gRin = np.zeros((n, 9), np.float32), np.zeros((n, 9), np.float32)
    hg.hg_cond9(LAYERS[name], int(inverse), ptr(f32(M)), ptr(f32(R)), ptr(f32(gR)), ptr(f32(gl)), n, ptr(gM), ptr(gRin))
    return gM.reshape(-1, 3, 3), gRin.reshape(-1, 3, 3)


@functools.lru_cache(maxsize=None)
def rotations(n=N_BATCH):
    R = synth.uniform_rotations(n, seed=21).astype(np.float32)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def cotangents(n=N_BATCH):
    rng = np.random.default_rng(78)
    gR, gl = rng.standard_normal((n, 3, 3)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    gR.setflags(write=False)
    gl.setflags(write=False)
    return gR, gl


def layer_kappa(name, M):
    return gx.kappa2(M) if name == "smith" else gx.cond(M)


# ---- the yardstick: LAPACK fp32 on the same matrices, computed once per batch and shared ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def yardstick(name, inverse, kind, window, n=N_BATCH):
    """LAPACK fp32's batch maxima of the forward figures on batch(kind, window), the fp64 references themselves (read-only) and the fp64
    matrix recomposed from LAPACK's fp32 factors.  Smith's rotation does not depend on the pass (the inverse pass transposes it)."""
    M, R = batch(kind, window, n), rotations(n)
    assert px.in_domain(M).mean() >= 0.98 and px.in_domain(M).all()          # a condition on the input; nothing is left out of a gate
    k = layer_kappa(name, M)
    if name == "smith":
        Q32, l32, U32 = gx.lapack_gs32(M)
        want, want_l = gx.smith64(M), np.zeros(n)
        at = gx.recomposed(Q32, U32)
    else:
        Q32, l32, U32 = gx.lapack_gs32(gx.gs9_input32(M, R, inverse))
        want, want_l = gx.gs9_64(M, R, inverse)
        at = gx.recomposed(Q32, U32, R, inverse)
    for a in (want, want_l, at):
        a.setflags(write=False)
    return {"rot": gx.rot_figure(Q32, want, k).max(), "ldj": gx.ldj_figure(l32, want_l, k).max() if name == "gs9" else 0.0,
            "orth": px.orth_err(Q32).max(), "want": want, "want_ldj": want_l, "at": at}


@functools.lru_cache(maxsize=None)
def yardstick_grad(name, inverse, kind, window, n=N_BATCH):
    """The backward yardstick: what fp32 factors cost a gradient, i.e. the batch maxima of the figures of fp64 autograd evaluated at the
    matrix recomposed from LAPACK's fp32 factors; and the fp64 gradients themselves (read-only)."""
    M, R = batch(kind, window, n), rotations(n)
    gR, gl = cotangents(n)
    k = layer_kappa(name, M)
    gM, gRin = gx.layer_grad64(name, M, R, gR, gl, inverse)
    gM32, gRin32 = gx.layer_grad64(name, M, R, gR, gl, inverse, at=yardstick(name, inverse, kind, window, n)["at"])
    gM.setflags(write=False)
    gRin.setflags(write=False)
    return {"grad": gx.grad_figure(gM32, gM, k).max(), "tan": gx.tangent_figure(R, gRin32, gRin, k).max(), "gM": gM, "gRin": gRin}


def strictest(name, inverse, key):
    """The smallest of the batch yardsticks: the gate of inputs that belong to no batch (the named edges)."""
    fn = yardstick_grad if key in ("grad", "tan") else yardstick
    return min(fn(name, inverse, k, w)[key] for k, w in CASES)


def forward(hs, name, inverse, M, R):
    """(rotation the figure judges, ldj): smith3's N, or calculate_9's R'."""
    if name == "smith":
        return smith3(hs, M), np.zeros(len(M), np.float32)
    return gs9(hs, M, R, inverse)


# ---- the references and the yardstick themselves ----------------------------------------------------------------------------------------------

def test_reference_functions_hold_what_they_name():
    M, R = batch("singular_values", "realistic", 2000).astype(np.float64), rotations(2000).astype(np.float64)
    Q = gx.smith64(M)
    U = np.einsum("nki,nkj->nij", Q, M)                                            # Q^T M: upper triangular in its first two columns, u00, u11 > 0
    assert px.orth_err(Q).max() < 1e-12 and np.allclose(np.linalg.det(Q), 1.0)
    assert np.abs(U[:, 1:, 0]).max() < 1e-12 * np.abs(U).max() and np.abs(U[:, 2, 1]).max() < 1e-12 * np.abs(U).max() and (U[:, 0, 0] > 0).all() and (U[:, 1, 1] > 0).all()
    for inverse in (False, True):
        Ro, l = gx.gs9_64(M, R, inverse)
        X = (np.linalg.inv(M) if inverse else M) @ R
        U = np.einsum("nki,nkj->nij", Ro, X)
        assert px.orth_err(Ro).max() < 1e-12 and np.allclose(np.linalg.det(Ro), 1.0) and np.abs(np.tril(U, -1)).max() < 1e-9 * np.abs(U).max()
        assert np.allclose(l, 2 * np.log(np.abs(U[:, 2, 2])) - 2 * np.log(U[:, 0, 0]), rtol=0, atol=1e-9)      # the closed form the header uses
        for c in (2.0 ** -40, 3.0):                                                 # R' and ldj do not depend on the scale of M
            Rc, lc = gx.gs9_64(c * M, R, inverse)
            assert np.abs(Rc - Ro).max() < 1e-9 and np.abs(lc - l).max() < 1e-9
    s = np.linalg.svd(M, compute_uv=False)
    assert np.allclose(gx.cond(M), s[:, 0] / s[:, 2]) and (gx.kappa2(M) <= gx.cond(M) * (1 + 1e-12)).all() and (gx.kappa2(M) >= 1).all()
    # a finite difference agrees with the fp64 gradient
    gR, gl = cotangents(2000)
    E = np.random.default_rng(4).standard_normal((1, 3, 3))
    for name, inverse in PASSES:
        g = gx.layer_grad64(name, M[:1], R[:1], gR[:1], gl[:1], inverse)[0]
        def loss(A):
            Ro, l = gx.layer64(name, gx._t(A), gx._t(R[:1]), inverse)
            return float((Ro.numpy() * gR[:1]).sum() + (l.numpy() * gl[:1]).sum())
        h = 1e-6 * np.abs(M[0]).max()
        fd = (loss(M[:1] + h * E) - loss(M[:1] - h * E)) / (2 * h)
        assert abs(fd - (g * E).sum()) < 1e-6 * np.abs(g).max() * 10, (name, inverse, fd, (g * E).sum())
    # figures: off by d in one entry reads d / (2^-23 kappa); a NaN reads inf
    k = gx.kappa2(M)
    Qb = Q.copy()
    Qb[5, 1, 2] += 3 * U23 * k[5]
    Qb[6, 0, 0] = np.nan
    f = gx.rot_figure(Qb, Q, k)
    assert abs(f[5] - 3) < 1e-6 and np.isinf(f[6]) and f[7] == 0


@pytest.mark.parametrize("kind", px.KINDS)
def test_lapack_fp32_is_order_one_in_the_conditioned_measure(kind):
    """The yardstick's own figures.  Householder QR is backward stable: |E| <= c 2^-24 |X| with c of a few tens for a 3x3 (two reflections of
    about ten roundings each, and for calculate_9 the product or the inverse before them), so the conditioned figures are between 1/4 and 36 as
    the SVD's are (tests/test_polar3_host.py), Q is orthogonal to 36 units, and a gradient through four such factors stays under 144."""
    for window in px.WINDOWS:
        for name, inverse in PASSES:
            y = {**yardstick(name, inverse, kind, window), **yardstick_grad(name, inverse, kind, window)}
            print(f"{kind}, {window}, {name}, inverse {inverse}: LAPACK fp32 rotation {y['rot']:.2f}, ldj {y['ldj']:.2f}, |QQ^T - I| {y['orth'] / U23:.2f} units, "
                  f"dL/dM {y['grad']:.2f}, dL/dR tangent {y['tan']:.2f}")
            assert 0.25 < y["rot"] < 36 and y["ldj"] < 36 and y["orth"] < 36 * U23 and 0.25 < y["grad"] < 144 and y["tan"] < 144


# ---- forward: every sample ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,window", CASES)
@pytest.mark.parametrize("name,inverse", PASSES[:3])
def test_every_sample_is_the_fp64_rotation(hs, name, inverse, kind, window):
    """All 20 000 matrices of each kind and scale window, smith3 and both passes of calculate_9: rotation and ldj figures within 2x LAPACK
    fp32's batch maxima, orthogonal within 2x LAPACK's, det = +1 (q2 is a cross product: also where det M < 0, as in the reference)."""
    M, R, y = batch(kind, window), rotations(), yardstick(name, inverse, kind, window)
    k = layer_kappa(name, M)
    Q, l = forward(hs, name, inverse, M, R)
    f, o, fl = gx.rot_figure(Q, y["want"], k), px.orth_err(Q), gx.ldj_figure(l, y["want_ldj"], k)
    print(f"{name}, inverse {inverse}, {kind}, {window}: header / LAPACK fp32: rotation {f.max():.2f} / {y['rot']:.2f}, ldj {fl.max():.2f} / {y['ldj']:.2f}, "
          f"|QQ^T - I| {o.max() / U23:.2f} / {y['orth'] / U23:.2f} units")
    assert f.max() <= 2 * y["rot"], (f.max(), y["rot"], int(f.argmax()), int((f > 2 * y["rot"]).sum()))
    assert o.max() <= 2 * y["orth"], (o.max() / U23, y["orth"] / U23, int(o.argmax()), int((o > 2 * y["orth"]).sum()))
    assert fl.max() <= 2 * y["ldj"], (fl.max(), y["ldj"], int(fl.argmax()), int((fl > 2 * y["ldj"]).sum()))
    assert (np.linalg.det(Q.astype(np.float64)) > 0.5).all()


@pytest.mark.parametrize("name,inverse", PASSES[:3])
def test_in_domain_edges(hs, name, inverse):
    M, names = px.EDGE_STACK[px.EDGE_IN], np.array(px.EDGE_NAMES)[px.EDGE_IN]
    R = rotations(len(M))
    k = layer_kappa(name, M)
    want, want_l = (gx.smith64(M), np.zeros(len(M))) if name == "smith" else gx.gs9_64(M, R, inverse)
    Q, l = forward(hs, name, inverse, M, R)
    f, o, fl = gx.rot_figure(Q, want, k), px.orth_err(Q), gx.ldj_figure(l, want_l, k)
    gate = {key: 2 * strictest(name, inverse, key) for key in ("rot", "orth", "ldj")}
    print(f"{name}, inverse {inverse}, in-domain edges, rotation figure:", dict(zip(names, np.round(f, 2))), "gate", gate["rot"])
    print("  ldj figure:", dict(zip(names, np.round(fl, 2))), "gate", gate["ldj"])
    print("  |QQ^T - I| in units:", dict(zip(names, np.round(o / U23, 2))), "gate", gate["orth"] / U23)
    assert (f <= gate["rot"]).all(), [(n, v) for n, v in zip(names, f) if v > gate["rot"]]
    assert (o <= gate["orth"]).all(), [(n, v) for n, v in zip(names, o) if v > gate["orth"]]
    assert (fl <= gate["ldj"]).all(), [(n, v) for n, v in zip(names, fl) if v > gate["ldj"]]
    assert (np.linalg.det(Q.astype(np.float64)) > 0.5).all()
    if name == "smith":
        i = list(names).index("identity")
        assert np.array_equal(Q[i], M[i])                                          # M = I passes the layer's input through bit for bit


def check_nan_or_rotation(Q, l, tag):
    """Out of the domain: R' all NaN, or finite and orthogonal to 16 units (what the header itself accepts); ldj finite only beside a rotation
    (l = None for Smith, whose ldj is 0 by definition and never computed)."""
    o = px.orth_err(Q)
    nan = np.isnan(Q).all((-1, -2))
    rot = np.isfinite(Q).all((-1, -2)) & (o <= ORTH_NAN)
    print(f"{tag}: {int(nan.sum())} of {len(Q)} NaN, the rest orthogonal to {o[~nan].max() / U23 if (~nan).any() else 0:.1f} units")
    assert (nan | rot).all(), (tag, int((~(nan | rot)).sum()), Q[~(nan | rot)][:2])
    assert l is None or not (np.isfinite(l) & ~rot).any(), tag
    return nan


@pytest.mark.parametrize("name,inverse", PASSES[:3])
def test_out_of_domain_is_nan_or_a_rotation(hs, name, inverse):
    """Rank 2, rank 1, zero, cond 1e5 and 1e7, one NaN entry, one infinite entry; 2000 random matrices each of cond 1e4 .. 1e8 and of exact
    rank 2, at scales 10^U(-12,12); and the ends of the fp32 range, 10^+-19.5, 1e21, 1e-20, 1e30, 1e-30 times (I + 0.3 N)."""
    M, names = px.EDGE_STACK[~px.EDGE_IN], np.array(px.EDGE_NAMES)[~px.EDGE_IN]
    Q, l = forward(hs, name, inverse, M, rotations(len(M)))
    ldj = lambda l: None if name == "smith" else l  # noqa: E731
    nan = check_nan_or_rotation(Q, ldj(l), f"{name}, inverse {inverse}, edges")
    print("  NaN:", list(names[nan]))
    for n in ("zero", "rank1", "one_inf") + (("one_nan", "rank2") if name == "gs9" else ()):       # Smith does not read the third column
        assert nan[list(names).index(n)], n
    rng = np.random.default_rng(12)
    n = 2000
    R = rotations(n)
    U, V = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0], np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    for c in (1e4, 1e5, 1e6, 1e7, 1e8, np.inf):
        s = np.stack([np.ones(n), 10.0 ** rng.uniform(-3, 0, n), np.full(n, 1 / c)], 1) * 10.0 ** rng.uniform(-12, 12, (n, 1))
        Mc = np.einsum("nik,nk,njk->nij", U, s, V).astype(np.float32)
        Q, l = forward(hs, name, inverse, Mc, R)
        check_nan_or_rotation(Q, ldj(l), f"{name}, inverse {inverse}, cond {c:g}")
    base = np.eye(3) + 0.3 * rng.standard_normal((n, 3, 3))
    for scale in (10.0 ** 19.5, 10.0 ** -19.5, 1e21, 1e-20, 1e30, 1e-30, 1e13, 1e-13):
        Ms = (base * scale).astype(np.float32)
        Q, l = forward(hs, name, inverse, Ms, R)
        nan = check_nan_or_rotation(Q, ldj(l), f"{name}, inverse {inverse}, scale {scale:g}")
        good = gx.cond(Ms) <= px.COND_MAX                                          # in the domain but for the scale: the rotation of M, not a NaN
        k = layer_kappa(name, Ms)
        want = gx.smith64(Ms) if name == "smith" else gx.gs9_64(Ms, R, inverse)[0]
        f = gx.rot_figure(Q, want, k)
        assert not nan[good].any() and (f[good] <= 2 * strictest(name, inverse, "rot")).all(), (scale, int(nan[good].sum()), f[good].max())


# ---- scale covariance --------------------------------------------------------------------------------------------------------------------------

def test_power_of_two_scaling_changes_no_bit(hs, hg):
    """f(2^k M) is bit-equal to f(M) for rotation and ldj, k = +-30, +-60; dL/dM(2^k M) = 2^-k dL/dM(M) bit for bit, dL/dR unchanged."""
    n = 2000
    R = rotations(n)
    gR, gl = (a[:n] for a in cotangents())
    for kind in ("near_identity", "singular_values"):
        M = batch(kind, "realistic", n)
        for name, inverse in PASSES:
            Q, l = forward(hs, name, inverse, M, R)
            gM, gRin = cond9(hg, name, inverse, M, R, gR, gl)
            assert np.isfinite(Q).all() and np.isfinite(l).all() and np.isfinite(gM).all() and np.isfinite(gRin).all()
            for k in (-60, -30, 30, 60):
                Mk = np.ldexp(M, k)
                Qk, lk = forward(hs, name, inverse, Mk, R)
                assert np.array_equal(Qk, Q) and np.array_equal(lk, l), (kind, name, inverse, k, int((Qk != Q).any((-1, -2)).sum()))
                gMk, gRink = cond9(hg, name, inverse, Mk, R, gR, gl)
                assert np.array_equal(gMk, np.ldexp(gM, -k)) and np.array_equal(gRink, gRin), (kind, name, inverse, k)


# ---- backward: every sample, the whole layer ---------------------------------------------------------------------------------------------------

def backward_gates(name, inverse, M, gR, gl, want_M, want_R, R, y_grad, y_tan):
    """Per-sample ABSOLUTE gates of dL/dM and of the tangent part of dL/dR: twice the yardstick's figure, turned back into an error
    (x 2^-23 kappa max|reference|), plus 4 x 2^-23 times the size of the terms of the 3-term fp32 products the header forms.

    Why the second part.  The yardstick is fp64 autograd at a matrix 2^-23 away: it carries the conditioning of the gradient and none of
    the roundings an fp32 evaluation makes on the way.  Those are absolute errors of the size of what is multiplied, not of the result: the
    reverse of normalising, g -> (g - q (q . g)) / |b|, rounds the 3-term product q . g to 2^-23 c (c = the largest cotangent entry) and
    divides by |b| >= s_min, so dL/dM carries 2^-23 c / s_min however small dL/dM itself comes out, with s_min the smallest singular value
    of what is factored (M[:, :2] for Smith, M for calculate_9; the inverse pass maps a cotangent of M^-1 to one of M, another factor cond).
    dL/dR = gR' N^T (Smith) has terms of size c; dL/dR = M^T gX (calculate_9) has terms of size |M| c / s_min = cond c.
    Where the reference gradient is small by cancellation (a cotangent nearly normal to what the layer can move) the figure alone,
    which divides by max|reference|, would hold the header to a relative accuracy no fp32 evaluation has: without this term 1 to 13 of
    20 000 samples exceed twice the yardstick in 17 of the 40 cells (the test prints the count of every cell)."""
    k = layer_kappa(name, M)
    A = M.astype(np.float64)
    s_min = np.linalg.svd(A[:, :, :2] if name == "smith" else A, compute_uv=False)[:, -1]
    c = np.abs(gR).reshape(len(M), -1).max(-1)
    if name == "gs9":
        c = np.maximum(c, np.abs(gl))
    terms_M = c / s_min * (k if name == "gs9" and inverse else 1.0)
    terms_R = c * (k if name == "gs9" else 1.0)
    gate_M = 2 * y_grad * U23 * k * gx._maxabs(want_M) + 4 * U23 * terms_M
    gate_R = 2 * y_tan * U23 * k * gx._maxabs(gx.tangent(R, want_R)) + 4 * U23 * terms_R
    return gate_M, gate_R


def backward_errors(R, gM, gRin, want_M, want_R):
    return gx._maxabs(gM.astype(np.float64) - want_M), gx._maxabs(gx.tangent(R, gRin) - gx.tangent(R, want_R))


@pytest.mark.parametrize("kind,window", CASES)
@pytest.mark.parametrize("name,inverse", PASSES)
def test_every_sample_backward_is_the_fp64_gradient(hg, name, inverse, kind, window):
    """cond9_backward for RNF_KIND_COND9_GS / _SMITH, forward and inverse pass, uniform rotations, random normal cotangents of R' and ldj:
    dL/dM and the tangent part of dL/dR per sample against fp64 autograd of the oracle's layer, each within 2x the figure fp64 autograd
    shows at the matrix recomposed from LAPACK fp32's factors, plus the 4 x 2^-23 of the fp32 products (backward_gates)."""
    M, R, y = batch(kind, window), rotations(), yardstick_grad(name, inverse, kind, window)
    gR, gl = cotangents()
    k = layer_kappa(name, M)
    gM, gRin = cond9(hg, name, inverse, M, R, gR, gl)
    g, t = gx.grad_figure(gM, y["gM"], k), gx.tangent_figure(R, gRin, y["gRin"], k)
    eM, eR = backward_errors(R, gM, gRin, y["gM"], y["gRin"])
    gate_M, gate_R = backward_gates(name, inverse, M, gR, gl, y["gM"], y["gRin"], R, y["grad"], y["tan"])
    print(f"{name}, inverse {inverse}, {kind}, {window}: header / LAPACK fp32: dL/dM {g.max():.2f} / {y['grad']:.2f} ({int((g > 2 * y['grad']).sum())} over twice), "
          f"dL/dR tangent {t.max():.2f} / {y['tan']:.2f} ({int((t > 2 * y['tan']).sum())} over twice); error / gate max {np.max(eM / gate_M):.3f}, {np.max(eR / gate_R):.3f}")
    assert (eM <= gate_M).all(), (int(np.argmax(eM / gate_M)), np.max(eM / gate_M), int((eM > gate_M).sum()))
    assert (eR <= gate_R).all(), (int(np.argmax(eR / gate_R)), np.max(eR / gate_R), int((eR > gate_R).sum()))


@pytest.mark.parametrize("name,inverse", PASSES)
def test_in_domain_edges_backward(hg, name, inverse):
    M, names = px.EDGE_STACK[px.EDGE_IN], np.array(px.EDGE_NAMES)[px.EDGE_IN]
    n = len(M)
    R = rotations(n)
    gR, gl = (a[:n] for a in cotangents())
    wM, wR = gx.layer_grad64(name, M, R, gR, gl, inverse)
    gM, gRin = cond9(hg, name, inverse, M, R, gR, gl)
    eM, eR = backward_errors(R, gM, gRin, wM, wR)
    gate_M, gate_R = backward_gates(name, inverse, M, gR, gl, wM, wR, R, strictest(name, inverse, "grad"), strictest(name, inverse, "tan"))
    print(f"{name}, inverse {inverse}, in-domain edges, dL/dM error / gate:", dict(zip(names, np.round(eM / gate_M, 3))))
    print("  dL/dR tangent error / gate:", dict(zip(names, np.round(eR / gate_R, 3))))
    assert (eM <= gate_M).all(), [(n_, v) for n_, v in zip(names, eM / gate_M) if v > 1]
    assert (eR <= gate_R).all(), [(n_, v) for n_, v in zip(names, eR / gate_R) if v > 1]


# ---- what calculate_9 does to a rotation when M = I (the allowance of tests/test_gpu_gs3.py) -------------------------------------------------

GS9_IDENTITY_UNITS = 4                                        # max|gs9(I, R) - R| over 20 000 fp32 rotations: 3.50 units of 2^-23 measured, rounded up
GS9_IDENTITY_LDJ_UNITS = 8                                    # max|ldj| there (the logarithm of two lengths 1 +- rounding): 7.00 units measured


def test_gs9_of_identity_moves_a_rotation_by_rounding_only(hs):
    """cond_gs9_apply(I, R) re-normalises R, so a device run with M = I does not return its input bit for bit as Smith's does.  How far it
    moves an fp32 rotation is measured here; tests/test_gpu_gs3.py adds these two numbers of units to its gates for that reason and no other."""
    R = rotations()
    I = np.broadcast_to(np.eye(3, dtype=np.float32), R.shape)
    for inverse in (False, True):
        Ro, l = gs9(hs, I, R, inverse)
        d = np.abs(Ro.astype(np.float64) - R).max() / U23
        print(f"gs9(I, R), inverse {inverse}: max|R' - R| = {d:.2f} units, max|ldj| = {np.abs(l).max() / U23:.2f} units")
        assert d <= GS9_IDENTITY_UNITS and np.abs(l).max() <= GS9_IDENTITY_LDJ_UNITS * U23
