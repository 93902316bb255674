"""fp64 reference for rot = U^T V of the SVD of a 4x4 matrix (csrc/svd4_lapack.h, ConditionRot), numpy only: it judges EVERY sample,
also those on which two fp32 routines pick different signs.

With distinct non-zero singular values the pairs (u_i, v_i) are defined up to one common sign each, so U^T V is defined up to
rot -> D rot D, D = diag(+-1): 16 sign patterns, D and -D giving the same matrix, hence 8 candidates.  "Equal up to the routine's sign
convention" is: rot lies (to rounding) on one of the 8.  How far rounding may move it is set by the matrix: singular vectors of a matrix
perturbed by eps |A| turn by about eps s_max / gap, gap = the smallest difference of adjacent singular values.  `conditioned` divides that
out, so its value is O(1) for a backward-stable fp32 routine whatever the matrix, and a test can gate it at a small multiple of what
LAPACK's own fp32 routine shows on the same input.
"""
import itertools

import numpy as np

EPS32 = 2.0 ** -24

# the 8 sign classes: D = diag(1, +-1, +-1, +-1) (D and -D give the same D rot D)
SIGNS = np.array([(1.0,) + t for t in itertools.product((1.0, -1.0), repeat=3)])


def _as64(M):
    return np.asarray(M, np.float64).reshape(-1, 4, 4)


def utv64(M):
    """(U^T V [n,4,4], singular values [n,4]) of numpy.linalg.svd in fp64."""
    U, S, VT = np.linalg.svd(_as64(M))
    return np.einsum("nki,njk->nij", U, VT), S


def sign_class(rot, M):
    """Per sample: (the smallest max|rot - D utv64(M) D| over the 8 sign classes, the index into SIGNS of the D that attains it)."""
    want, _ = utv64(M)
    cand = SIGNS[None, :, :, None] * want[:, None] * SIGNS[None, :, None, :]              # [n, 8, 4, 4]
    err = np.abs(_as64(rot)[:, None] - cand).max((-1, -2))                                # [n, 8]; NaN where rot is not finite
    err = np.where(np.isnan(err), np.inf, err)
    return err.min(1), err.argmin(1)


def sign_class_error(rot, M):
    return sign_class(rot, M)[0]


def rel_gap(S):
    """Smallest difference of adjacent singular values over the largest (0 for the zero matrix)."""
    S = np.asarray(S, np.float64).reshape(-1, 4)
    smax = S[:, 0]
    return np.where(smax > 0, (S[:, :-1] - S[:, 1:]).min(1) / np.where(smax > 0, smax, 1.0), 0.0)


def conditioned(err, S):
    """err * gap / s_max in units of 2^-24."""
    return np.asarray(err, np.float64) * rel_gap(S) / EPS32


def factor_checks(M, U, S, VT):
    """What holds for the factors of EVERY finite matrix, degenerate ones included; per sample, all but `ordered` are max-abs errors:
    residual |U diag(S) VT - M| / s_max, u_orth |U^T U - I|, v_orth |VT VT^T - I|, values |S - S64| / s_max, ordered (S >= 0, non-increasing).
    s_max is fp64's; for the zero matrix the two relative figures are the absolute ones."""
    M, U, VT = _as64(M), _as64(U), _as64(VT)
    S = np.asarray(S, np.float64).reshape(-1, 4)
    S64 = np.linalg.svd(M, compute_uv=False)
    smax = np.where(S64[:, 0] > 0, S64[:, 0], 1.0)
    eye = np.eye(4)
    with np.errstate(invalid="ignore", over="ignore"):
        out = {
            "residual": np.abs(np.einsum("nik,nk,nkj->nij", U, S, VT) - M).max((-1, -2)) / smax,
            "u_orth": np.abs(np.einsum("nki,nkj->nij", U, U) - eye).max((-1, -2)),
            "v_orth": np.abs(np.einsum("nik,njk->nij", VT, VT) - eye).max((-1, -2)),
            "values": np.abs(S - S64).max(1) / smax,
        }
    out = {k: np.where(np.isnan(v), np.inf, v) for k, v in out.items()}
    out["ordered"] = (S[:, -1] >= 0) & (S[:, :-1] >= S[:, 1:]).all(1)
    return out


FACTOR_KEYS = ("residual", "u_orth", "v_orth", "values")
FACTOR_FLOOR = 16 * EPS32          # 4 roundings per entry of a 4-term dot product: the gate where LAPACK's own figure is exactly 0


def unique_utv(M, rel=1e-5):
    """True where U^T V is a function of the matrix up to the sign classes: singular values distinct and non-zero, by `rel` of s_max (at
    1e-5 an fp32 routine still resolves the class to ~ 2^-24 / 1e-5 = 6e-3; below, the smallest values are fp32 rounding of the input)."""
    S = np.linalg.svd(_as64(M), compute_uv=False)
    return (rel_gap(S) > rel) & (S[:, -1] > rel * S[:, 0])


def random_batch(spread, n=20000):
    """I + spread N(0,1) as fp32: near the identity (the layer at initialisation), the regime of the trained-like fixtures, far from it.
    (The batches tests/test_svd4.py has always used.)"""
    import torch
    torch.manual_seed(int(spread * 100))
    return (torch.eye(4) + spread * torch.randn(n, 4, 4)).float().numpy()


SPREADS = (0.05, 0.5, 3.0)
SCALE_EXPONENTS = (-30, -20, -16, -12, 12, 16, 18, 19, 20, 30)


def _edges():
    rng = np.random.default_rng(4)
    N = lambda *s: rng.standard_normal(s)
    Q, _ = np.linalg.qr(N(4, 4))
    Q2, _ = np.linalg.qr(N(4, 4))
    rank = lambda k: (Q[:, :k] * np.array([3.0, 1.5, 0.5])[:k]) @ Q2[:, :k].T
    out = [
        ("zero", np.zeros((4, 4))),
        ("identity", np.eye(4)),
        ("minus_identity", -np.eye(4)),
        ("permutation", np.eye(4)[[2, 0, 3, 1]]),
        ("diag_2211", np.diag([2.0, 2.0, 1.0, 1.0])),
        ("diag_2_-1_0.5_3", np.diag([2.0, -1.0, 0.5, 3.0])),
        ("rank1", np.outer([1.0, -2.0, 0.5, 3.0], [2.0, 1.0, -1.0, 0.25])),        # small dyadic entries: exactly rank 1 in fp32 as well
        ("rank2", rank(2)),
        ("rank3", rank(3)),
        ("orthogonal", Q),
        ("identity_plus_1e-7", np.eye(4) + 1e-7 * N(4, 4)),
    ]
    for e in SCALE_EXPONENTS:
        out.append((f"scale_1e{e}", (np.eye(4) + 0.5 * N(4, 4)) * 10.0 ** e))
    bad = np.eye(4) + 0.5 * N(4, 4)
    nan, inf = bad.copy(), bad.copy()
    nan[1, 2] = np.nan
    inf[2, 0] = np.inf
    out += [("one_nan", nan), ("one_inf", inf)]
    return [(name, m.astype(np.float32)) for name, m in out]


EDGE_M = _edges()                                        # [(name, fp32 4x4)]
EDGE_NAMES = [name for name, _ in EDGE_M]
EDGE_STACK = np.stack([m for _, m in EDGE_M])
EDGE_FINITE = np.isfinite(EDGE_STACK).all((-1, -2))
