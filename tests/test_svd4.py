"""CPU: csrc/svd4_lapack.h (the dense-SVD path of LAPACK restated for 4x4, run per sample on the device by ConditionRot) reproduces
``torch.svd``'s SIGN conventions: U^T V -- which is not a function of the matrix alone (flow/rottrans.py:37-66) -- equals the reference's.

Beside the agreement with LAPACK's signs (>= 99.7 % of the matrices), EVERY sample is judged against fp64 (tests/svd4_exact.py): its
rotation must lie in one of the 8 sign classes of the true U^T V, as closely as the matrix's conditioning allows an fp32 routine, and its
factors must be a singular value decomposition.  The yardstick of every such gate is LAPACK's own fp32 routine (``torch.svd``) on the same
input, judged by the same fp64 function inside the test: the header may show twice LAPACK's figure, the room between two correct
implementations of one algorithm.  The host build here is compiled without contraction; tests/test_gpu_condrot_svd.py asks the same of
the device build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import svd4_exact as sx

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_svd4.cpp")
OUT = os.path.join(HERE, "csrc", "_host_svd4.so")
HDR = os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", "svd4_lapack.h")


@pytest.fixture(scope="module")
def hs():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC], check=True)
    return C.CDLL(OUT)


def _utv(hs, M):
    A = np.ascontiguousarray(M.reshape(-1, 16), dtype=np.float32)
    rot = np.empty_like(A)
    sv = np.empty((A.shape[0], 4), np.float32)
    bad = hs.hs_utv(A.ctypes.data_as(C.c_void_p), rot.ctypes.data_as(C.c_void_p), sv.ctypes.data_as(C.c_void_p), A.shape[0])
    return rot.reshape(-1, 4, 4), sv, bad


@pytest.mark.parametrize("spread", [0.05, 0.5, 3.0])
def test_utv_has_lapacks_signs(hs, spread):
    """I + spread * N(0,1): near-identity (the layer at initialisation), the trained-like regime of the fixtures, and far from identity."""
    torch.manual_seed(int(spread * 100))
    M = (torch.eye(4) + spread * torch.randn(20000, 4, 4)).float()
    U, S, V = torch.svd(M)
    want = (U.transpose(1, 2) @ V).numpy()
    got, sv, bad = _utv(hs, M.numpy())
    assert bad == 0
    assert np.abs(sv - S.numpy()).max() < 2e-5 * max(1.0, float(S.max()))
    err = np.abs(got - want).reshape(len(got), -1).max(1)
    # Identical rotation for >= 99.7 % of the matrices (measured 99.8 - 99.9 %).  The rest are razor-edge decisions of the QR iteration
    # (sweep direction, deflation and shift tests compare quantities that differ by rounding between two implementations of the same
    # algorithm -- MKL against netlib against this header, each pair ~0.1 % apart): another, equally valid sign pattern, as between the
    # reference's own fp32 and fp64 runs.
    assert np.mean(err < 1e-4) > 0.997, np.mean(err < 1e-4)
    # orthogonality of the result
    assert np.abs(np.einsum("nij,nkj->nik", got, got) - np.eye(4)).max() < 1e-5


def test_utv_on_degenerate_inputs(hs):
    """Identity, a diagonal matrix with a negative entry, a rank-deficient matrix: finite, orthogonal, LAPACK's answer where it is unique."""
    M = np.stack([np.eye(4), np.diag([2.0, -1.0, 0.5, 3.0]), np.diag([1.0, 1.0, 0.0, 2.0]) + 0 * np.eye(4)]).astype(np.float32)
    got, sv, bad = _utv(hs, M)
    assert bad == 0 and np.isfinite(got).all()
    U, S, V = torch.svd(torch.from_numpy(M))
    want = (U.transpose(1, 2) @ V).numpy()
    assert np.abs(got[:2] - want[:2]).max() < 1e-6
    assert np.abs(np.einsum("nij,nkj->nik", got, got) - np.eye(4)).max() < 1e-5


# ---- the fp64 reference itself ---------------------------------------------------------------------------------------------------------

def _lapack32(M):
    """torch.svd in fp32 (LAPACK sgesdd): (U^T V, U, S, V^T) as numpy."""
    U, S, V = torch.svd(torch.from_numpy(np.ascontiguousarray(M, dtype=np.float32)))
    return (U.transpose(-1, -2) @ V).numpy(), U.numpy(), S.numpy(), V.transpose(-1, -2).numpy()


def test_sign_class_error_is_zero_on_the_8_classes_and_order_one_elsewhere():
    M = sx.random_batch(0.5, 500)
    want, S = sx.utv64(M)
    assert sx.SIGNS.shape == (8, 4) and len({tuple(d) for d in np.concatenate([sx.SIGNS, -sx.SIGNS])}) == 16
    for k, D in enumerate(sx.SIGNS):
        for sgn in (1.0, -1.0):                                     # D and -D: the same class
            err, which = sx.sign_class(D[:, None] * sgn * want * sgn * D[None, :], M)
            assert err.max() == 0.0 and (which == k).all()
    # a sign pattern that is NOT of the form D rot D (one sign on one side only) is far from every class for a generic rotation
    err = sx.sign_class_error(want * np.array([1.0, 1.0, 1.0, -1.0]), M)
    assert np.median(err) > 0.3 and err.min() > 1e-3, (np.median(err), err.min())
    # a non-finite rotation is infinitely far, never "closest to NaN"
    bad = want.copy()
    bad[3, 1, 2] = np.nan
    assert np.isinf(sx.sign_class_error(bad, M)[3]) and sx.sign_class_error(bad, M)[4] == 0.0
    # conditioned: err * gap / s_max / 2^-24
    S = np.array([[4.0, 3.0, 2.5, 1.0]])
    assert sx.conditioned(np.array([2.0 ** -20]), S)[0] == 16 * 0.5 / 4.0


@pytest.mark.parametrize("spread", sx.SPREADS)
def test_lapack_fp32_is_order_one_in_the_conditioned_measure(spread):
    """The yardstick's own figure.  First-order perturbation theory: a backward error E turns the singular vectors by <= ~ |E| / gap, and
    LAPACK's bound on |E| / |A| is a low-degree polynomial p(n) of the dimension times 2^-24.  n^2 = 16 roundings each for the two-sided
    bidiagonalisation and for the QR sweeps, and U and V both enter U^T V: p = 64 is the most a backward-stable 4x4 routine can show.
    (Measured: 0.88, 5.0, 8.5.)"""
    M = sx.random_batch(spread)
    _, S64 = sx.utv64(M)
    c = sx.conditioned(sx.sign_class_error(_lapack32(M)[0], M), S64)
    print(f"spread {spread}: LAPACK fp32 conditioned sign-class error max {c.max():.3f}")
    assert c.max() < 64.0, c.max()


def test_factor_checks_see_a_wrong_factor():
    M = sx.random_batch(0.5, 50)
    _, U, S, VT = _lapack32(M)
    good = sx.factor_checks(M, U, S, VT)
    assert all(good[k].max() < sx.FACTOR_FLOOR for k in sx.FACTOR_KEYS) and good["ordered"].all()
    U2 = U.copy()
    U2[7, :, 2] *= -1.0                                             # one left vector's sign alone: still orthogonal, no longer a factorisation
    f = sx.factor_checks(M, U2, S, VT)
    assert f["residual"][7] > 1e-2 and f["u_orth"][7] < sx.FACTOR_FLOOR and np.delete(f["residual"], 7).max() < sx.FACTOR_FLOOR
    S2 = S.copy()
    S2[9] = S2[9, ::-1]
    assert not sx.factor_checks(M, U, S2, VT)["ordered"][9]
    assert sx.factor_checks(M, U, S * np.float32(1.001), VT)["values"].min() > 1e-4


def test_edge_list_holds_what_it_names():
    assert len(set(sx.EDGE_NAMES)) == len(sx.EDGE_NAMES) == 23
    S = np.linalg.svd(sx.EDGE_STACK[sx.EDGE_FINITE].astype(np.float64), compute_uv=False)
    by = dict(zip(np.array(sx.EDGE_NAMES)[sx.EDGE_FINITE], S))
    assert (by["rank1"][1:] < 1e-15 * by["rank1"][0]).all()                        # exactly rank 1 in fp32
    assert by["rank2"][2] < 1e-6 * by["rank2"][0] < by["rank2"][1] and by["rank3"][3] < 1e-6 * by["rank3"][0] < by["rank3"][2]
    assert np.abs(by["orthogonal"] - 1).max() < 1e-6
    for e in sx.SCALE_EXPONENTS:
        assert 0.3 * 10.0 ** e < by[f"scale_1e{e}"][0] < 10 * 10.0 ** e
    assert [n for n, f in zip(sx.EDGE_NAMES, sx.EDGE_FINITE) if not f] == ["one_nan", "one_inf"]
    assert np.isnan(sx.EDGE_STACK[-2]).sum() == 1 and np.isinf(sx.EDGE_STACK[-1]).sum() == 1


# ---- the host build: every sample ------------------------------------------------------------------------------------------------------

def _svd(hs, M):
    """(rot, U, S, VT, flag per sample) of the host build."""
    A = np.ascontiguousarray(np.asarray(M, dtype=np.float32).reshape(-1, 16))
    n = A.shape[0]
    rot, U, VT = np.empty_like(A), np.empty_like(A), np.empty_like(A)
    S, flag = np.empty((n, 4), np.float32), np.empty(n, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert hs.hs_svd(p(A), p(rot), p(U), p(S), p(VT), p(flag), n) == flag.sum()
    return rot.reshape(n, 4, 4), U.reshape(n, 4, 4), S, VT.reshape(n, 4, 4), flag


def _orth(rot):
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(np.einsum("nij,nkj->nik", rot.astype(np.float64), rot.astype(np.float64)) - np.eye(4)).max((-1, -2))
    return np.where(np.isnan(e), np.inf, e)


def check_batch_against_lapack(M, rot, U, S, VT, what):
    """Every sample of a batch of generic matrices: conditioned sign-class error and factor checks within 2x LAPACK fp32's batch maximum."""
    _, S64 = sx.utv64(M)
    lrot, lU, lS, lVT = _lapack32(M)
    got = sx.conditioned(sx.sign_class_error(rot, M), S64)
    ref = sx.conditioned(sx.sign_class_error(lrot, M), S64)
    print(f"{what}: conditioned sign-class error max {got.max():.3f}, LAPACK fp32 {ref.max():.3f}")
    assert got.max() <= 2 * ref.max(), (what, got.max(), ref.max(), int(got.argmax()))
    f, lf = sx.factor_checks(M, U, S, VT), sx.factor_checks(M, lU, lS, lVT)
    for k in sx.FACTOR_KEYS:
        print(f"{what}: {k} max {f[k].max():.3e}, LAPACK fp32 {lf[k].max():.3e}")
        assert f[k].max() <= 2 * lf[k].max(), (what, k, f[k].max(), lf[k].max(), int(f[k].argmax()))
    assert f["ordered"].all(), what
    return got.max(), ref.max()


@pytest.mark.parametrize("spread", sx.SPREADS)
def test_every_random_sample_lies_in_a_sign_class_of_the_fp64_rotation(hs, spread):
    """All 20 000 matrices of each batch, none left out.  (Measured, header / LAPACK: 0.84 / 0.88, 4.2 / 5.0, 7.1 / 8.5.)"""
    M = sx.random_batch(spread)
    rot, U, S, VT, flag = _svd(hs, M)
    assert flag.sum() == 0
    assert np.array_equal(rot, _utv(hs, M)[0])                      # the two shim entries run one routine
    check_batch_against_lapack(M, rot, U, S, VT, f"host build, spread {spread}")


def check_edges(M, rot, U, S, VT, flag, names):
    """EDGE_M (or the part of it a caller can feed): the flag exactly on the non-finite matrices, NaN throughout beside it; every finite
    matrix gives an orthogonal rot and a factorisation; where U^T V is unique, a sign class of the fp64 rotation (2x LAPACK's maximum over
    those matrices, like a random batch).

    The factor checks are gated per matrix at 2x LAPACK's figure on that matrix, with a floor of 16 * 2^-24 (4 roundings per entry of a
    4-term dot product) under the gate: on the matrices LAPACK factorises exactly the gate would otherwise be 0, and below the floor the
    ratio of two correct routines' rounding errors on ONE matrix says nothing (on the random batches the header shows more than twice
    LAPACK's residual on 7 % of the matrices and LAPACK more than twice the header's on 9 %, while 0.1 % of either lie above the floor)."""
    fin = np.isfinite(M).all((-1, -2))
    assert [n for n, b in zip(names, flag) if b] == [n for n, b in zip(names, fin) if not b]
    assert all(np.isnan(x[~fin]).all() for x in (rot, U, S, VT))   # the defined result of a failed sample
    M, rot, U, S, VT, names = M[fin], rot[fin], U[fin], S[fin], VT[fin], np.array(names)[fin]
    assert np.isfinite(rot).all() and _orth(rot).max() < 1e-5, dict(zip(names, _orth(rot)))
    lrot, lU, lS, lVT = _lapack32(M)
    f, lf = sx.factor_checks(M, U, S, VT), sx.factor_checks(M, lU, lS, lVT)
    for k in sx.FACTOR_KEYS:
        gate = np.maximum(2 * lf[k], sx.FACTOR_FLOOR)
        print(f"edges, {k}: max {f[k].max():.3e} ({names[f[k].argmax()]}), LAPACK fp32 max {lf[k].max():.3e}, exactly 0 on {int((lf[k] == 0).sum())}")
        assert (f[k] <= gate).all(), (k, [(n, a, b) for n, a, b, g in zip(names, f[k], lf[k], gate) if a > g])
    assert f["ordered"].all()
    uniq = sx.unique_utv(M)
    assert all(uniq[list(names).index(f"scale_1e{e}")] for e in sx.SCALE_EXPONENTS if f"scale_1e{e}" in names)
    assert uniq[list(names).index("diag_2_-1_0.5_3")] and not uniq[list(names).index("identity")]
    _, S64 = sx.utv64(M)
    got = sx.conditioned(sx.sign_class_error(rot, M), S64)[uniq]
    ref = sx.conditioned(sx.sign_class_error(lrot, M), S64)[uniq]
    print("edges with a unique U^T V:", dict(zip(names[uniq], np.round(got, 3))), "LAPACK fp32", np.round(ref, 3))
    assert got.max() <= 2 * ref.max(), (got.max(), ref.max(), names[uniq][got.argmax()])


def test_edge_matrices_flag_or_factorise(hs):
    rot, U, S, VT, flag = _svd(hs, sx.EDGE_STACK)
    check_edges(sx.EDGE_STACK, rot, U, S, VT, flag, sx.EDGE_NAMES)
    rot2, _, bad = _utv(hs, sx.EDGE_STACK)
    assert bad == 2 and np.array_equal(rot2, rot, equal_nan=True)


@pytest.mark.parametrize("e", [-30, -20, -16, -12, 12, 16, 18, 19, 20, 25, 30])
def test_every_scale_flags_or_returns_a_rotation(hs, e):
    """(I + 0.5 N(0,1)) * 10^e, 2000 matrices: a rot beside a clear flag is orthogonal -- and with the scaling step no finite matrix is
    flagged, and every one lands in a sign class of the fp64 rotation like the unit-scale batches.  (Without the step: from 1e19 the fp32
    squares overflow, infinite singular values and |R R^T - I| = 1 beside flag 0; from 1e-16 down they underflow.)"""
    torch.manual_seed(1000 + e)
    M = ((torch.eye(4) + 0.5 * torch.randn(2000, 4, 4)).double() * 10.0 ** e).float().numpy()
    rot, U, S, VT, flag = _svd(hs, M)
    orth = _orth(rot)
    print(f"1e{e}: flagged {int(flag.sum())}, non-finite rot {int((~np.isfinite(rot).all((-1, -2))).sum())}, not orthogonal {int((orth > 1e-4).sum())}")
    assert (orth[flag == 0] < 1e-5).all(), (e, int((orth[flag == 0] >= 1e-5).sum()))
    assert flag.sum() == 0
    check_batch_against_lapack(M, rot, U, S, VT, f"host build, scale 1e{e}")


def test_power_of_two_scaling_changes_no_bit_of_the_rotation(hs):
    """Scaling by 2^k is exact in fp32 while nothing under- or overflows, and the routine's decisions compare quantities of equal degree,
    so U^T V must not change by a bit, whether the matrix takes the path untouched (k = 0), is brought back by the scaling step (+-30,
    +-60), or is a flow's healthy matrix."""
    M = sx.random_batch(0.5)
    rot, _, S, _, flag = _svd(hs, M)
    assert flag.sum() == 0
    for k in (-60, -30, 30, 60):
        r, _, s, _, fl = _svd(hs, np.ldexp(M, k))
        assert fl.sum() == 0 and np.array_equal(r, rot), (k, int((r != rot).any((-1, -2)).sum()))
        assert np.abs(np.ldexp(s.astype(np.float64), -k) - S).max() < 4 * sx.EPS32 * S.max()
