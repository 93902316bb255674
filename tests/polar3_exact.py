"""fp64 reference for the orthogonal polar factor Q = U V^T of a 3x3 matrix (csrc/so3_math.h polar3, Condition9RotL / Condition9RotR) and for
its derivative (csrc/so3_grad.h polar3_backward), with the inputs on which every sample is judged.  No GPU, no pytest.

How far rounding may move Q is set by the matrix: a perturbation E of M turns the polar factor by about |E| / (s1 + s2), the two SMALLEST
singular values (Q is smooth where singular values meet and singular only where s1 + s2 = 0).  An fp32 routine has |E| ~ 2^-23 s0, so

    kappa(M) = s0 / (s1 + s2)

is the conditioning of the polar factor relative to |M|_2, and  max|Q - polar64(M)| / (2^-23 kappa(M))  is O(1) for a backward-stable
fp32 routine whatever the matrix.  Tests gate it at twice what LAPACK's own fp32 SVD shows on the same batch.

GATED DOMAIN (a condition on the input, never a measurement of the routine): finite matrices with cond(M) = s0 / s2 <= 1e3 whose largest
entry lies in [2^-70, 2^70] (the named edges at 2^+-60 times an entry above 1, and the hollow matrix at 1e-20 = 2^-66, must lie inside).
Every kind of `random_batch` lies inside completely, by construction (a draw outside is drawn again), and so does every EDGE_M entry
that is not named in OUT_OF_DOMAIN; both are asserted at the bottom of this module.
"""
import numpy as np

U23 = 2.0 ** -23                                          # the unit of every figure
COND_MAX = 1e3
ENTRY_LO, ENTRY_HI = 2.0 ** -70, 2.0 ** 70


def _as64(M):
    return np.asarray(M, np.float64).reshape(-1, 3, 3)


def svals(M):
    return np.linalg.svd(_as64(M), compute_uv=False)


def polar64(M):
    """U @ Vh of numpy.linalg.svd in fp64 of the (fp32) matrix, [n,3,3]."""
    U, _, Vh = np.linalg.svd(_as64(M))
    return U @ Vh


def kappa(M):
    s = svals(M)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s[:, 0] / (s[:, 1] + s[:, 2])


def cond(M):
    s = svals(M)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s[:, 0] / s[:, 2]


def in_domain(M):
    M = np.asarray(M, np.float64).reshape(-1, 3, 3)
    fin = np.isfinite(M).all((-1, -2))
    out = np.zeros(len(M), bool)
    amax = np.abs(M[fin]).max((-1, -2))
    with np.errstate(divide="ignore", invalid="ignore"):
        out[fin] = (cond(M[fin]) <= COND_MAX) & (amax >= ENTRY_LO) & (amax <= ENTRY_HI)
    return out


def polar_grad64(M, G):
    """d<G, U Vh>/dM by fp64 torch.autograd through torch.linalg.svd: how the reference differentiates the layer (rottrans.py:69-78).
    Singular where two singular values are EQUAL (the SVD's own derivative is, though the polar factor's is not); see polar_grad_closed64."""
    import torch
    Mt = torch.from_numpy(_as64(M).copy()).requires_grad_(True)
    U, _, Vh = torch.linalg.svd(Mt)
    ((U @ Vh) * torch.from_numpy(_as64(G))).sum().backward()
    return Mt.grad.numpy()


def polar_grad_closed64(M, G):
    """The same derivative in closed form, fp64: with M = U diag(s) Vh and B = U^T G V,  dL/dM = U [(B_ij - B_ji) / (s_i + s_j)] Vh.
    Smooth at repeated singular values, where torch's SVD derivative divides by zero; equal to polar_grad64 to ~1e-10 elsewhere
    (tests/test_polar3_host.py checks that), and used only for the EDGE_M entries with exactly repeated singular values."""
    U, s, Vh = np.linalg.svd(_as64(M))
    B = np.einsum("nki,nkl,njl->nij", U, _as64(G), Vh)
    X = (B - B.transpose(0, 2, 1)) / (s[:, :, None] + s[:, None, :])
    return U @ X @ Vh


def orth_err(Q):
    """max|Q Q^T - I| per sample in fp64; inf where Q is not finite."""
    Q = _as64(Q)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(np.einsum("nij,nkj->nik", Q, Q) - np.eye(3)).max((-1, -2))
    return np.where(np.isnan(e), np.inf, e)


def rot_figure(Q, M):
    """f = max|Q - polar64(M)| / (2^-23 kappa(M)) per sample; inf where Q is not finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(_as64(Q) - polar64(M)).max((-1, -2))
    return np.where(np.isnan(e), np.inf, e) / (U23 * kappa(M))


def grad_figure(gM, want, M):
    """g = max|gM - want| / max|want| / (2^-23 kappa(M)) per sample."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(_as64(gM) - _as64(want)).max((-1, -2))
    return np.where(np.isnan(e), np.inf, e) / np.abs(_as64(want)).max((-1, -2)) / (U23 * kappa(M))


# ---- random inputs -------------------------------------------------------------------------------------------------------------------

KINDS = ("near_identity", "identity_plus_spread", "normal", "normal_negdet", "singular_values")
REALISTIC = (-2.0, 3.0)                                    # per-sample scale 10^U(lo, hi): what a trained conditioner produces
RANGE = (-12.0, 12.0)                                      # the fp32 range the routine is asked to cover
WINDOWS = {"realistic": REALISTIC, "range": RANGE}


def _draw(kind, n, rng):
    N = rng.standard_normal((n, 3, 3))
    if kind == "near_identity":
        return np.eye(3) + 0.2 * N
    if kind == "identity_plus_spread":
        return np.eye(3) + 10.0 ** rng.uniform(-2, 3, (n, 1, 1)) * N
    if kind == "normal":
        return N
    if kind == "normal_negdet":
        N[:, 0] *= -np.sign(np.linalg.det(N))[:, None]
        return N
    if kind == "singular_values":                          # U diag(1, c^-t, 1/c) V^T, c = 10^U(0,3), t ~ U(0,1): two small values included
        c = 10.0 ** rng.uniform(0, 3, n)
        t = rng.uniform(0, 1, n)
        U, _ = np.linalg.qr(N)
        V, _ = np.linalg.qr(rng.standard_normal((n, 3, 3)))
        return np.einsum("nik,nk,njk->nij", U, np.stack([np.ones(n), c ** -t, 1 / c], 1), V)
    raise ValueError(kind)


def random_batch(kind, n, seed, window=REALISTIC):
    """[n,3,3] fp32 of one kind, every sample multiplied by its own scale 10^U(window) before the one rounding to fp32.  A sample whose
    fp32 matrix has cond > 1e3 is drawn again (about 2 % of the Gaussian kinds), so the batch lies in the gated domain completely."""
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    M = _draw(kind, n, rng)
    scale = 10.0 ** rng.uniform(window[0], window[1], (n, 1, 1))
    out = (M * scale).astype(np.float32)
    for _ in range(64):
        bad = ~in_domain(out)
        if not bad.any():
            return out
        out[bad] = (_draw(kind, int(bad.sum()), rng) * scale[bad]).astype(np.float32)
    raise AssertionError("random_batch: redraw did not converge")


# ---- named edge matrices ---------------------------------------------------------------------------------------------------------------

OUT_OF_DOMAIN = ("rank2", "rank1", "zero", "cond_1e5", "cond_1e7", "one_nan", "one_inf")
POW2_EXPONENTS = (-60, -40, 40, 60)
HOLLOW_EXPONENTS = (-6, -12, -20)


def _edges():
    rng = np.random.default_rng(9)
    N = lambda *s: rng.standard_normal(s)
    qr = lambda: np.linalg.qr(N(3, 3))[0]
    Q1, Q2 = qr(), qr()
    rot = Q1 * np.sign(np.linalg.det(Q1))
    sv = lambda *s: Q1 @ np.diag(s) @ Q2.T
    base = np.eye(3) + 0.2 * N(3, 3)
    out = [
        ("identity", np.eye(3)),
        ("minus_identity", -np.eye(3)),
        ("rotation", rot),
        ("reflection", rot @ np.diag([1.0, 1.0, -1.0])),
        ("diag_5_1_-1", np.diag([5.0, 1.0, -1.0])),
        ("rotated_diag_2_2_1", sv(2.0, 2.0, 1.0)),
        ("rotated_diag_2_1_1", sv(2.0, 1.0, 1.0)),
        ("cond_1e3_two_large", sv(1.0, 1.0, 1.00001e-3)),            # 1e3 less 1e-5 of it: the rounding to fp32 must not leave the domain
        ("cond_1e3_two_small", sv(1.0, 1.00001e-3, 1.00001e-3)),
        ("identity_plus_500N", np.eye(3) + 500.0 * N(3, 3)),
    ]
    for e in HOLLOW_EXPONENTS:                               # what net = -I + tiny gives: zero diagonal, everything else ~10^e
        H = N(3, 3) * 10.0 ** e
        np.fill_diagonal(H, 0.0)
        out.append((f"hollow_1e{e}", H))
    for k in POW2_EXPONENTS:
        out.append((f"pow2_{k}", np.ldexp(base, k)))
    nan, inf = base.copy(), base.copy()
    nan[1, 2] = np.nan
    inf[2, 0] = np.inf
    out += [
        ("rank2", sv(3.0, 1.5, 0.0)),
        ("rank1", np.outer([1.0, -2.0, 0.5], [2.0, 1.0, -0.25])),     # small dyadic entries: exactly rank 1 in fp32 as well
        ("zero", np.zeros((3, 3))),
        ("cond_1e5", sv(1.0, 0.3, 1e-5)),
        ("cond_1e7", sv(1.0, 0.3, 1e-7)),
        ("one_nan", nan),
        ("one_inf", inf),
    ]
    return [(name, m.astype(np.float32)) for name, m in out]


EDGE_M = _edges()                                            # [(name, fp32 3x3)]
EDGE_NAMES = [name for name, _ in EDGE_M]
EDGE_STACK = np.stack([m for _, m in EDGE_M])
EDGE_IN = np.array([name not in OUT_OF_DOMAIN for name in EDGE_NAMES])

# the domain is a condition on the inputs: checked here, once, for everything a test will gate
assert len(set(EDGE_NAMES)) == len(EDGE_NAMES) and set(OUT_OF_DOMAIN) <= set(EDGE_NAMES)
assert np.array_equal(in_domain(EDGE_STACK), EDGE_IN), [n for n, a, b in zip(EDGE_NAMES, in_domain(EDGE_STACK), EDGE_IN) if a != b]
for _kind in KINDS:
    for _w in WINDOWS.values():
        assert in_domain(random_batch(_kind, 512, 0, _w)).all(), (_kind, _w)
