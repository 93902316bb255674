"""CPU: polar3 (csrc/so3_math.h) and polar3_backward (csrc/so3_grad.h), host build without contraction, EVERY sample against fp64
(tests/polar3_exact.py) over the whole gated domain: cond(M) <= 1e3 at every scale, det < 0 included.

The yardstick of every gate is LAPACK's own fp32 route on the same matrices, ``torch.linalg.svd`` in fp32 and U @ Vh, judged by the same
fp64 functions inside the test; the header may show twice its batch maximum (the standing margin between two correct routines,
tests/test_gpu_condrot_svd.py).  Figures are in units of 2^-23 kappa(M), kappa = s0 / (s1 + s2).

Measured (host build, 20 000 matrices per kind and window; header / LAPACK fp32):
    kind, window                         rotation figure   |QQ^T - I| / 2^-23   backward figure
    near_identity, realistic             1.99 /  9.45       2.50 / 11.99         27.96 /  44.38
    identity_plus_spread, realistic      2.10 /  9.91       2.19 / 11.46         16.43 /  32.23
    normal, realistic                    1.97 /  7.32       2.20 / 11.89         12.88 / 113.88
    normal_negdet, realistic             1.74 /  6.65       2.09 / 13.48         18.08 /  25.51
    singular_values, realistic           2.52 /  7.98       2.00 / 12.15         17.53 / 125.32
    near_identity, range                 1.97 /  8.87       2.20 / 11.86         37.04 /  41.07
    identity_plus_spread, range          2.11 / 11.96       2.14 / 12.34         19.54 /  32.28
    normal, range                        2.16 /  6.81       2.25 / 13.75         18.05 / 107.20
    normal_negdet, range                 1.83 /  6.69       2.28 / 12.74         15.57 /  33.55
    singular_values, range               2.70 /  9.68       2.51 / 13.72         21.38 / 141.66
Whole layer (2 000 per kind, both sides, both passes): dL/dM figure <= 33.8, dL/dR tangent error <= 0.05 of its gate.
The unscaled ten-step iteration this replaced shows rotation figures of 8.5e6 .. 1.9e10 in the realistic window (3 800 - 8 200 of 20 000
samples per batch over the gate) and 2e16 .. inf in the range window, and fails 38 of these 45 tests.
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
from tests import polar3_exact as px
from tests.test_host_grad import f32, hg, ptr, tangent  # noqa: F401  (hg: the host build of so3_grad.h with hg_cond9, a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_polar3.cpp")
OUT = os.path.join(HERE, "csrc", "_host_polar3.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f) for f in ("so3_grad.h", "so3_math.h")]

N_BATCH = 20000
CASES = [(k, w) for w in px.WINDOWS for k in px.KINDS]


@pytest.fixture(scope="module")
def hp():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    return C.CDLL(OUT)


def polar3(hp, M):
    A = f32(np.asarray(M).reshape(-1, 9))
    Q = np.empty_like(A)
    hp.hp_polar3(ptr(A), ptr(Q), len(A))
    return Q.reshape(-1, 3, 3)


def polar3_backward(hp, M, G):
    A, g = f32(np.asarray(M).reshape(-1, 9)), f32(np.asarray(G).reshape(-1, 9))
    out = np.empty_like(A)
    hp.hp_polar3_backward(ptr(A), ptr(g), ptr(out), len(A))
    return out.reshape(-1, 3, 3)


# ---- the yardstick: LAPACK fp32 on the same matrices, computed once per batch and shared -------------------------------------------------

def lapack32(M):
    """(U @ Vh, U, S, Vh) of torch.linalg.svd in fp32."""
    U, S, Vh = torch.linalg.svd(torch.from_numpy(np.array(M, dtype=np.float32)))
    return (U @ Vh).numpy(), U.numpy(), S.numpy(), Vh.numpy()


@functools.lru_cache(maxsize=None)
def batch(kind, window, n=N_BATCH):
    M = px.random_batch(kind, n, 1, px.WINDOWS[window])
    assert px.in_domain(M).all()                               # nothing of a batch is left out of a gate
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def normal_G(n=N_BATCH):
    G = np.random.default_rng(77).standard_normal((n, 3, 3)).astype(np.float32)
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=None)
def yardstick(kind, window, n=N_BATCH):
    """LAPACK fp32's batch maxima on batch(kind, window): rotation figure, orthogonality, and the backward figure of fp64 autograd evaluated
    at the matrix U32 diag(S32) Vh32 of its fp32 factors (what fp32 factors cost a gradient).  Also the fp64 gradient itself."""
    M = batch(kind, window, n)
    Q, U, S, Vh = lapack32(M)
    want = px.polar_grad64(M, normal_G(n))
    M32 = np.einsum("nik,nk,nkj->nij", U.astype(np.float64), S.astype(np.float64), Vh.astype(np.float64))
    g = px.grad_figure(px.polar_grad64(M32, normal_G(n)), want, M)
    want.setflags(write=False)
    return {"rot": px.rot_figure(Q, M).max(), "orth": px.orth_err(Q).max(), "grad": g.max(), "want": want}


def strictest(key):
    """The smallest of the batch yardsticks: the gate of inputs that belong to no batch (the named edges)."""
    return min(yardstick(k, w)[key] for k, w in CASES)


# ---- the reference itself ----------------------------------------------------------------------------------------------------------------

def test_reference_functions_hold_what_they_name():
    M = batch("singular_values", "realistic", 2000)
    s = px.svals(M)
    assert np.allclose(px.kappa(M), s[:, 0] / (s[:, 1] + s[:, 2])) and np.allclose(px.cond(M), s[:, 0] / s[:, 2])
    Q = px.polar64(M)
    assert px.orth_err(Q).max() < 1e-14 and (np.sign(np.linalg.det(Q)) == np.sign(np.linalg.det(M.astype(np.float64)))).all()
    H = np.einsum("nki,nkj->nij", Q, M.astype(np.float64))                        # Q^T M is symmetric positive definite
    assert np.abs(H - H.transpose(0, 2, 1)).max() < 1e-12 * np.abs(H).max() and (np.linalg.eigvalsh((H + H.transpose(0, 2, 1)) / 2) > 0).all()
    # the two fp64 derivatives agree where the SVD's own derivative exists, and a finite difference agrees with both
    G = normal_G(2000)
    a, b = px.polar_grad64(M, G), px.polar_grad_closed64(M, G)
    assert (np.abs(a - b).max((-1, -2)) <= 1e-9 * np.abs(a).max((-1, -2))).all()
    M1 = np.eye(3) + 0.3 * np.random.default_rng(3).standard_normal((1, 3, 3))
    E = np.random.default_rng(4).standard_normal((1, 3, 3))
    fd = ((px.polar64(M1 + 1e-6 * E) - px.polar64(M1 - 1e-6 * E)) / 2e-6 * G[:1]).sum()
    assert abs(fd - (px.polar_grad64(M1, G[:1]) * E).sum()) < 1e-8
    # figures: a rotation off by d in one entry reads d / (2^-23 kappa); a NaN reads inf
    Qb = Q.copy()
    Qb[5, 1, 2] += 3 * px.U23 * px.kappa(M)[5]
    Qb[6, 0, 0] = np.nan
    f = px.rot_figure(Qb, M)
    assert abs(f[5] - 3) < 1e-6 and np.isinf(f[6]) and f[7] == 0 and np.isinf(px.orth_err(Qb)[6])


def test_edge_list_holds_what_it_names():
    by = dict(px.EDGE_M)
    s = {n: px.svals(m)[0] for n, m in by.items() if np.isfinite(m).all()}
    assert 999.9 <= s["cond_1e3_two_large"][0] / s["cond_1e3_two_large"][2] <= 1e3 and s["cond_1e3_two_large"][1] > 0.99 * s["cond_1e3_two_large"][0]
    assert 999.9 <= s["cond_1e3_two_small"][0] / s["cond_1e3_two_small"][2] <= 1e3 and s["cond_1e3_two_small"][1] < 1.01 * s["cond_1e3_two_small"][2]
    assert abs(s["rotated_diag_2_2_1"][0] - s["rotated_diag_2_2_1"][1]) < 1e-6 and abs(s["rotated_diag_2_1_1"][1] - s["rotated_diag_2_1_1"][2]) < 1e-6
    assert s["rank1"][1] < 1e-15 * s["rank1"][0] and s["rank2"][2] < 1e-6 * s["rank2"][0] < s["rank2"][1] and s["zero"][0] == 0
    assert 0.5e5 < s["cond_1e5"][0] / s["cond_1e5"][2] < 2e5 and 0.3e7 < s["cond_1e7"][0] / s["cond_1e7"][2] < 3e7
    assert np.linalg.det(by["reflection"].astype(np.float64)) < 0 < np.linalg.det(by["rotation"].astype(np.float64))
    assert px.orth_err(by["rotation"]).max() < 1e-6 and px.orth_err(by["reflection"]).max() < 1e-6
    assert s["identity_plus_500N"][0] > 300
    for e in px.HOLLOW_EXPONENTS:
        h = by[f"hollow_1e{e}"]
        assert (np.diag(h) == 0).all() and 0.1 * 10.0 ** e < np.abs(h).max() < 10 * 10.0 ** e
    for k in px.POW2_EXPONENTS:
        assert np.array_equal(np.ldexp(by[f"pow2_{k}"], -k), np.ldexp(by["pow2_40"], -40))
    assert np.isnan(by["one_nan"]).sum() == 1 and np.isinf(by["one_inf"]).sum() == 1
    for kind in px.KINDS:                                          # kinds hold what they name
        M = batch(kind, "range", 2000).astype(np.float64)
        assert (np.linalg.det(M) < 0).all() == (kind == "normal_negdet")
    amax = np.abs(batch("normal", "range")).max((-1, -2))
    assert amax.min() < 1e-11 and amax.max() > 1e11 and np.abs(batch("near_identity", "realistic")).max() > 500


@pytest.mark.parametrize("kind", px.KINDS)
def test_lapack_fp32_is_order_one_in_the_conditioned_measure(kind):
    """The yardstick's own figures.  A backward-stable 3x3 SVD has |E| <= p(3) 2^-24 |M| with p a low-degree polynomial (9 roundings each
    for the bidiagonalisation and the sweeps, U and V both entering U Vh): 36 units is the most it can show, and a product of two
    orthogonal fp32 factors is orthogonal to about 3 + 3 roundings per entry on each side.  The gradient U [(B - B^T)_ij / (s_i + s_j)] Vh
    takes the error of U, of Vh, of B = U^T G V and of the divisor, each of the size of the rotation's: four times its bound.
    (Measured: 7 - 12 units, 11 - 13 units, 30 - 115 units.)"""
    for window in px.WINDOWS:
        y = yardstick(kind, window)
        print(f"{kind}, {window}: LAPACK fp32 rotation figure max {y['rot']:.2f}, |QQ^T - I| max {y['orth'] / px.U23:.2f} units, backward figure max {y['grad']:.2f}")
        assert 0.5 < y["rot"] < 36 and y["orth"] < 36 * px.U23 and 0.5 < y["grad"] < 144


# ---- forward: every sample ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,window", CASES)
def test_every_sample_is_the_fp64_polar_factor(hp, kind, window):
    """All 20 000 matrices of each kind and scale window: figure within 2x LAPACK fp32's batch maximum, orthogonal within 2x LAPACK's,
    the sign of det M kept.  `realistic` has scales 10^U(-2,3), `range` 10^U(-12,12)."""
    M, y = batch(kind, window), yardstick(kind, window)
    Q = polar3(hp, M)
    f, o = px.rot_figure(Q, M), px.orth_err(Q)
    print(f"{kind}, {window}: figure max {f.max():.2f} (LAPACK fp32 {y['rot']:.2f}), |QQ^T - I| max {o.max() / px.U23:.2f} units (LAPACK fp32 {y['orth'] / px.U23:.2f})")
    assert f.max() <= 2 * y["rot"], (f.max(), y["rot"], int(f.argmax()), int((f > 2 * y["rot"]).sum()))
    assert o.max() <= 2 * y["orth"], (o.max(), y["orth"], int(o.argmax()))
    with np.errstate(invalid="ignore"):
        assert (np.sign(np.linalg.det(Q.astype(np.float64))) == np.sign(np.linalg.det(M.astype(np.float64)))).all()


def test_in_domain_edges(hp):
    M, names = px.EDGE_STACK[px.EDGE_IN], np.array(px.EDGE_NAMES)[px.EDGE_IN]
    Q = polar3(hp, M)
    f, o = px.rot_figure(Q, M), px.orth_err(Q)
    print("in-domain edges, figure:", dict(zip(names, np.round(f, 2))), "gate", 2 * strictest("rot"))
    print("in-domain edges, |QQ^T - I| in units:", dict(zip(names, np.round(o / px.U23, 2))), "gate", 2 * strictest("orth") / px.U23)
    assert (f <= 2 * strictest("rot")).all(), [(n, v) for n, v in zip(names, f) if v > 2 * strictest("rot")]
    assert (o <= 2 * strictest("orth")).all(), [(n, v) for n, v in zip(names, o) if v > 2 * strictest("orth")]
    assert (np.sign(np.linalg.det(Q.astype(np.float64))) == np.sign(np.linalg.det(M.astype(np.float64)))).all()
    for name in ("identity", "minus_identity"):
        assert np.array_equal(Q[list(names).index(name)], M[list(names).index(name)])


def check_nan_or_rotation(Q, M, names):
    """Out of the domain: all-NaN, or finite and orthogonal to the in-domain bound; a NaN or infinite entry gives NaN."""
    o = px.orth_err(Q)
    report = {n: ("NaN" if np.isnan(q).all() else f"orthogonal to {e / px.U23:.1f} units") for n, q, e in zip(names, Q, o)}
    print("out of domain:", report)
    for n, q, e, m in zip(names, Q, o, M):
        assert np.isnan(q).all() or (np.isfinite(q).all() and e <= 2 * strictest("orth")), (n, q)
        if not np.isfinite(m).all():
            assert np.isnan(q).all(), n
    return report


def test_out_of_domain_is_nan_or_a_rotation(hp):
    """Rank 2, rank 1, zero, cond 1e5 and 1e7, one NaN entry, one infinite entry; and 2000 random matrices each of cond 1e4 .. 1e8 and of
    exact rank 2.  (The header gives: rank1, zero, one_nan, one_inf NaN; rank2, cond_1e5, cond_1e7 and
    every one of the 12 000 random matrices orthogonal to <= 2.2 units.)"""
    M, names = px.EDGE_STACK[~px.EDGE_IN], np.array(px.EDGE_NAMES)[~px.EDGE_IN]
    check_nan_or_rotation(polar3(hp, M), M, names)
    rng = np.random.default_rng(12)
    n = 2000
    U, V = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0], np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    for c in (1e4, 1e5, 1e6, 1e7, 1e8, np.inf):
        s = np.stack([np.ones(n), 10.0 ** rng.uniform(-3, 0, n), np.full(n, 1 / c)], 1) * 10.0 ** rng.uniform(-12, 12, (n, 1))
        Mc = np.einsum("nik,nk,njk->nij", U, s, V).astype(np.float32)
        Q = polar3(hp, Mc)
        o = px.orth_err(Q)
        nan = np.isnan(Q).all((-1, -2))
        print(f"cond {c:g}: {int(nan.sum())} of {n} NaN, the rest orthogonal to {o[~nan].max() / px.U23 if (~nan).any() else 0:.1f} units")
        assert (nan | (np.isfinite(Q).all((-1, -2)) & (o <= 2 * strictest("orth")))).all(), c


def test_power_of_two_scaling_changes_no_bit(hp):
    """polar3(2^k M) is bit-equal to polar3(M), and gM(2^k M) to 2^-k gM(M): the normalisation is a power of two."""
    for kind in ("near_identity", "singular_values"):
        M, G = batch(kind, "realistic", 2000), normal_G(2000)
        Q, g = polar3(hp, M), polar3_backward(hp, M, G)
        assert np.isfinite(Q).all() and np.isfinite(g).all()
        for k in (-40, -10, -1, 1, 10, 40):
            Mk = np.ldexp(M, k)
            assert np.array_equal(polar3(hp, Mk), Q), (kind, k, int((polar3(hp, Mk) != Q).any((-1, -2)).sum()))
            assert np.array_equal(polar3_backward(hp, Mk, G), np.ldexp(g, -k)), (kind, k)


@pytest.mark.parametrize("kind,window", CASES)
def test_transpose(hp, kind, window):
    """The inverse pass feeds M^T and relies on polar(M^T) = polar(M)^T: the two results differ by no more than their own errors."""
    M = batch(kind, window)
    Mt = np.ascontiguousarray(M.transpose(0, 2, 1))
    Q, Qt = polar3(hp, M), polar3(hp, Mt)
    want = px.polar64(M)
    ea, eb = np.abs(Q - want).max((-1, -2)), np.abs(Qt - want.transpose(0, 2, 1)).max((-1, -2))
    d = np.abs(Q.astype(np.float64) - Qt.transpose(0, 2, 1)).max((-1, -2))
    assert np.isfinite(d).all() and (d <= ea + eb).all()
    assert px.rot_figure(Qt, Mt).max() <= 2 * yardstick(kind, window)["rot"]


# ---- backward: every sample -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,window", CASES)
def test_every_sample_backward_is_the_fp64_gradient(hp, kind, window):
    """polar3 then polar3_backward against fp64 autograd through torch.linalg.svd, random normal G, per sample, within 2x the figure fp64
    autograd shows at LAPACK fp32's factors.  And a G with Q^T G symmetric, whose gradient is zero: |gM| within the absolute error bound
    of the general case."""
    M, y, G = batch(kind, window), yardstick(kind, window), normal_G()
    gM = polar3_backward(hp, M, G)
    g = px.grad_figure(gM, y["want"], M)
    print(f"{kind}, {window}: backward figure max {g.max():.2f} (fp64 autograd at LAPACK fp32's factors {y['grad']:.2f})")
    assert g.max() <= 2 * y["grad"], (g.max(), y["grad"], int(g.argmax()), int((g > 2 * y["grad"]).sum()))
    A = G.astype(np.float64) + G.transpose(0, 2, 1)
    Gs = (px.polar64(M) @ A * 0.5).astype(np.float32)                              # Q^T Gs = (G + G^T) / 2 up to the rounding of Gs
    bound = 2 * y["grad"] * px.U23 * px.kappa(M) * np.abs(y["want"]).max((-1, -2))
    z = np.abs(polar3_backward(hp, M, Gs)).max((-1, -2))
    print(f"{kind}, {window}: zero-gradient direction, max |gM| / bound {np.max(z / bound):.3f}")
    assert np.isfinite(z).all() and (z <= bound).all(), (int(np.argmax(z / bound)), np.max(z / bound))


def test_in_domain_edges_backward(hp):
    """The named edges, repeated singular values included (the polar factor is smooth there, unlike U^T V of the 4x4 layer).  Where two
    singular values are EXACTLY equal torch's SVD derivative divides by zero, so the edges are judged by the closed form that
    test_reference_functions_hold_what_they_name ties to it."""
    M, names = px.EDGE_STACK[px.EDGE_IN], np.array(px.EDGE_NAMES)[px.EDGE_IN]
    G = normal_G(len(M))
    g = px.grad_figure(polar3_backward(hp, M, G), px.polar_grad_closed64(M, G), M)
    print("in-domain edges, backward figure:", dict(zip(names, np.round(g, 2))), "gate", 2 * strictest("grad"))
    assert (g <= 2 * strictest("grad")).all(), [(n, v) for n, v in zip(names, g) if v > 2 * strictest("grad")]


# ---- the whole layer --------------------------------------------------------------------------------------------------------------------------

LAYER_N = 2000


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("kind_id,name", [(8, "csvdl9"), (9, "csvdr9")])
def test_whole_layer_backward_per_sample(hg, kind_id, name, inverse):
    """cond9_backward for RNF_KIND_COND9_POLAR_L / _R, forward and inverse pass, uniform rotations, every kind of matrix at realistic scales:
    dL/dM per sample against fp64 autograd of the oracle's layer with the backward figure; dL/dR on the tangent space per sample.

    dL/dR = Q^T gR' (or gR' Q^T) carries Q's own error: per entry of the tangent 2 x 3 products, so the gate is
    6 max|gR'| (2 x LAPACK's rotation figure x 2^-23 kappa + 4 x 2^-23 for the fp32 products), relative to the sample's own reference
    magnitude with a floor of 1e-3 of the batch median."""
    for kind in px.KINDS:
        M = batch(kind, "realistic", LAYER_N)
        y = yardstick(kind, "realistic")
        rng = np.random.default_rng(kind_id + 10 * inverse)
        R = synth.uniform_rotations(LAYER_N, seed=kind_id).astype(np.float64)
        gR, gl = rng.standard_normal((LAYER_N, 3, 3)), rng.standard_normal(LAYER_N)
        Mt = torch.from_numpy(M.astype(np.float64)).requires_grad_(True)
        Rt = torch.from_numpy(R).requires_grad_(True)
        fn = orc.svdl9 if name == "csvdl9" else orc.svdr9
        Ro, l = fn(Mt.transpose(-1, -2) if inverse else Mt, Rt)
        ((Ro * torch.from_numpy(gR)).sum() + (l * torch.from_numpy(gl)).sum()).backward()
        gM, gRin = np.zeros((LAYER_N, 9), np.float32), np.zeros((LAYER_N, 9), np.float32)
        hg.hg_cond9(kind_id, int(inverse), ptr(f32(M)), ptr(f32(R)), ptr(f32(gR)), ptr(f32(gl)), LAYER_N, ptr(gM), ptr(gRin))
        g = px.grad_figure(gM, Mt.grad.numpy(), M)
        got_t, want_t = tangent(R, gRin.reshape(-1, 3, 3).astype(np.float64)), tangent(R, Rt.grad.numpy())
        mag = np.abs(want_t).max((-1, -2))
        mag = np.maximum(mag, 1e-3 * np.median(mag))
        et = np.abs(got_t - want_t).max((-1, -2)) / mag
        gate_t = 6 * np.abs(gR).max((-1, -2)) * (2 * y["rot"] * px.U23 * px.kappa(M) + 4 * px.U23) / mag
        print(f"{name}, inverse {inverse}, {kind}: dL/dM figure max {g.max():.2f} (gate {2 * y['grad']:.2f}), dL/dR tangent error / gate max {np.max(et / gate_t):.3f}")
        assert g.max() <= 2 * y["grad"], (kind, g.max(), int(g.argmax()))
        assert np.isfinite(et).all() and (et <= gate_t).all(), (kind, int(np.argmax(et / gate_t)), np.max(et / gate_t))
