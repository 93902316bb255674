"""Fitting matrix-Fisher distributions on the device: rnf_rotation_moments (fp64 weighted moments in one fixed order) and rnf_fisher_fit
(the maximum-likelihood A of a moment matrix, csrc/fisher_fit.h) against the fp64 references of tests/fisher_exact.py, and the layers
above them: ``MatrixFisherN.fit``, ``harness.grid_pose_fisher``, graph capture.  RESIDUAL and the gate |s_fit - s| <= RESIDUAL /
lambda_min(H_ref) are those of tests/test_fisher_fit_host.py; statistical gates use 5 standard errors and seeded streams."""
import numpy as np
import pytest
import torch
from scipy.special import ive
from scipy.stats import chi2

from rotationnormflow_amd import grid_pose, harness, synth
from rotationnormflow_amd.utils import fisher, sd
from rotationnormflow_amd.utils.fisher import MatrixFisherN
from tests import fisher_exact as fe
from tests.test_fisher_fit_host import CAPPED, EPS32, INPUT, RESIDUAL, full

pytestmark = pytest.mark.gpu

CAP = 3e4              # the largest cap the C ABI takes: EDGE_A reaches s0 = 1e4, the default cap


def mean_Q_batch(S):
    """fe.mean_Q for a batch [B,3] at once (the same formulas on fe's nodes, broadcast over rows; checked against fe.mean_Q below)."""
    S = np.asarray(S, np.float64).reshape(-1, 3)
    u, w = fe._NODES[None], fe._WEIGHTS[None]
    out = np.empty_like(S)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        a = 0.5 * (S[:, i] - S[:, j])[:, None] * (1.0 - u)
        b = 0.5 * (S[:, i] + S[:, j])[:, None] * (1.0 + u)
        E = np.abs(a) + np.abs(b) + S[:, k][:, None] * u
        M = np.maximum(np.abs(S[:, i] + S[:, j]) + S[:, k], np.abs(S[:, i] - S[:, j]) - S[:, k])[:, None]
        e = np.exp(E - M)
        i0a, i0b = ive(0, a), ive(0, b)
        c = (w * 0.5 * i0a * i0b * e).sum(-1)
        dc = (w * 0.5 * (0.5 * (1.0 - u) * ive(1, a) * i0b + 0.5 * (1.0 + u) * i0a * ive(1, b)) * e).sum(-1)
        out[:, i] = dc / c
    return out


def lambda_min_batch(S):
    """Smallest eigenvalue of the reference Hessian per row: central differences of mean_Q with steps 1e-3 max(1, |s_j|), symmetrised."""
    S = np.asarray(S, np.float64).reshape(-1, 3)
    H = np.empty((len(S), 3, 3))
    for j in range(3):
        h = 1e-3 * np.maximum(1.0, np.abs(S[:, j]))
        e = np.zeros_like(S)
        e[:, j] = h
        H[:, :, j] = (mean_Q_batch(S + e) - mean_Q_batch(S - e)) / (2 * h)[:, None]
    return np.linalg.eigvalsh(0.5 * (H + H.transpose(0, 2, 1))).min(-1)


def _fit(M, cap=1e4, max_iterations=0):
    out = fisher.fit_matrix_fisher(torch.from_numpy(np.ascontiguousarray(M, np.float64)).cuda(), cap, max_iterations)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def fit_batch():
    """The edge list plus 509 random parameter matrices at scales 1e-3..1e2 (B = 529 = 4 * 132 + 1: the last workgroup holds one wave),
    their exact moments M = U diag(mean_Q(s)) V^T in fp64 and the references' lambda_min, computed once."""
    rng = np.random.default_rng(20261019)
    A = np.concatenate([fe.EDGE_STACK, rng.standard_normal((509, 3, 3)) * 10.0 ** rng.uniform(-3, 2, (509, 1, 1))])
    U, s, V = fe.proper_svd64(A)
    d = mean_Q_batch(s)
    for b in (0, 3, 14, 16, 100):
        assert np.abs(d[b] - fe.mean_Q(s[b])).max() <= 1e-14
    M = np.einsum("bik,bk,bjk->bij", U, d, V)
    return dict(A=A, U=U, s=s, V=V, d=d, M=M, lam=lambda_min_batch(s))


def test_fit_against_the_references(fit_batch):
    """rnf_fisher_fit on 529 moments: |mean_Q(s_fit) - d|_inf <= RESIDUAL, |s_fit - s|_inf <= RESIDUAL / lambda_min(H_ref), A against the
    original matrix at 4 fp32 ulps of s0 plus 3 x the s gate (as on the host), H's smallest eigenvalue within 1% of the reference's."""
    ref = fit_batch
    got = _fit(ref["M"], CAP)
    B = len(ref["M"])
    assert B % 4 == 1 and (got["status"] == 0).all(), np.nonzero(got["status"])[0]
    res = np.abs(mean_Q_batch(got["s"]) - ref["d"]).max(-1)
    ds = np.abs(got["s"] - ref["s"]).max(-1)
    dA = np.abs(got["A"].astype(np.float64) - ref["A"]).max((-1, -2))
    print("largest residual %.3g (gate %.3g), largest |ds| lambda_min / RESIDUAL %.3g, most iterations %d"
          % (res.max(), RESIDUAL, (ds * ref["lam"] / RESIDUAL).max(), got["iterations"].max()))
    assert (res <= RESIDUAL).all(), (res.argmax(), res.max())
    assert (ds <= RESIDUAL / ref["lam"]).all(), (ds * ref["lam"]).argmax()
    assert (dA <= 4 * EPS32 * ref["s"][:, 0] + 3 * RESIDUAL / ref["lam"]).all()
    assert (got["s"][:, 0] >= got["s"][:, 1] - 1e-13 * np.maximum(1, got["s"][:, 0])).all()
    lam_dev = np.array([np.linalg.eigvalsh(full(h)).min() for h in got["hessian"]])
    assert (np.abs(lam_dev / ref["lam"] - 1.0) <= 1e-2).all()         # a sanity check: the reference differences are good to ~1e-6


def test_a_row_does_not_depend_on_its_batch(fit_batch):
    """Bit-identical outputs for a row fitted in the whole batch, alone, at another position (the batch reversed) and in a batch of 7."""
    M = fit_batch["M"]
    whole, rev, seven = _fit(M, CAP), _fit(M[::-1], CAP), _fit(M[3:10], CAP)
    for k in ("A", "s", "hessian", "iterations", "status"):
        assert np.array_equal(whole[k], rev[k][::-1]), k
        assert np.array_equal(whole[k][3:10], seven[k]), k
    for b in (0, 14, 528):
        alone = _fit(M[b:b + 1], CAP)
        for k in ("A", "s", "hessian", "iterations", "status"):
            assert np.array_equal(whole[k][b:b + 1], alone[k]), (k, b)


def test_status_bits_on_the_device():
    R = fe.uniform_rotations64(1, seed=5)[0]
    eps = 1e-12
    M = np.stack([np.eye(3), np.diag([1.0, -1.0, -1.0]) * (1 - eps), R, np.diag([1.2, 0.0, 0.0]), np.full((3, 3), np.nan), np.zeros((3, 3))])
    got = _fit(M)
    assert list(got["status"]) == [CAPPED, CAPPED, CAPPED, INPUT, INPUT, 0]
    assert np.isfinite(got["A"][:3]).all() and (np.abs(got["s"][:3]).max(-1) == 1e4).all()
    assert np.abs(got["A"][2] - 1e4 * R).max() <= 4 * EPS32 * 1e4
    assert np.isnan(got["A"][3:5]).all() and np.isnan(got["s"][3:5]).all() and np.isnan(got["hessian"][3:5]).all()
    assert (got["A"][5] == 0).all() and (got["s"][5] == 0).all() and got["iterations"][5] == 0
    d = fe.mean_Q((5.0, 3.0, 1.0))
    one = _fit(np.diag(d)[None], max_iterations=1)
    assert one["status"][0] == 2 and one["iterations"][0] == 1 and np.isfinite(one["A"]).all()


# ---- rnf_rotation_moments ---------------------------------------------------------------------------------------------------------

# Bound on |M_dev - M_exact| per entry, |M| <= 1, for n <= 8192 (two chunks): a term passes through at most 16 additions in its thread
# (4096-row chunk / 256 threads), 6 butterfly steps, 3 wave additions, 1 chunk addition and 6 more butterfly steps = 32 additions, each
# rounding by at most 2^-53 of a partial sum <= W (the weight sum); the product w R rounds once more, and the fp64 exp behind w may differ
# from the long-double one by 4 ulps = 8 x 2^-53.  That is 41 x 2^-53 relative to W in the numerator and 40 x 2^-53 in the denominator,
# plus one rounding of the division: 82 x 2^-53, taken as 128 x 2^-53 = 1.4e-14.
MOMENT_TOL = 128 * 2.0 ** -53


def _moments_ref(R32, lw32=None):
    """Long-double reference on the same fp32 inputs: R32 [G,n,3,3] or [n,3,3], lw32 [G,n] or None -> [G,3,3] float64."""
    R = R32.astype(np.longdouble)
    if lw32 is None:
        return (R.sum(-3) / R.shape[-3]).astype(np.float64).reshape(-1, 3, 3)
    lw = lw32.astype(np.longdouble)
    with np.errstate(invalid="ignore"):
        w = np.exp(lw - lw.max(-1, keepdims=True))
    R = R if R.ndim == 4 else R[None]
    return ((w[..., None, None] * R).sum(1) / w.sum(-1)[:, None, None]).astype(np.float64)


def _moments_dev(R32, lw32=None):
    lw = None if lw32 is None else torch.from_numpy(lw32).cuda()
    return fisher.rotation_moments(torch.from_numpy(R32).cuda(), lw).cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_moments_against_long_double(n):
    """n at 1, around the wave size and across a chunk boundary (4097 = one full chunk and one row, so partials of two chunks add up);
    n = 63 and 65 make groups 1.. start off the 16-byte boundary (36 n bytes), which takes the dword loads."""
    rng = np.random.default_rng(n)
    for G in (1, 3, 5):
        R = synth.uniform_rotations(G * n, seed=n + G).astype(np.float32).reshape(G, n, 3, 3)
        lw = (rng.standard_normal((G, n)) * 3.0).astype(np.float32)
        cases = [(R, None), (R, lw), (R[0], lw)]                       # plain mean, weighted, shared rotations
        if G == 1:
            cases.append((R[0], None))                                  # the [n,3,3] form
        for Rc, lwc in cases:
            got, want = _moments_dev(Rc, lwc), _moments_ref(Rc, lwc)
            assert got.shape == want.shape == (G, 3, 3) and got.dtype == np.float64
            assert np.abs(got - want).max() <= MOMENT_TOL, (n, G, np.abs(got - want).max())
        if n > 1:                                                       # a -inf row contributes nothing: the same as leaving it out
            cut = lw.copy()
            cut[:, n // 2] = -np.inf
            keep = np.arange(n) != n // 2
            got = _moments_dev(R, cut)
            assert np.abs(got - _moments_ref(R[:, keep], lw[:, keep])).max() <= MOMENT_TOL
        dead = lw.copy()                                                # an all -inf group is NaN, and only that group
        dead[G - 1] = -np.inf
        got = _moments_dev(R, dead)
        assert np.isnan(got[G - 1]).all() and np.isfinite(got[:G - 1]).all()
        bad = R.copy()                                                  # a NaN rotation: that group is NaN
        bad[0, n - 1, 1, 1] = np.nan
        got = _moments_dev(bad, lw)
        assert np.isnan(got[0]).any() and np.isfinite(got[1:]).all()


@pytest.mark.parametrize("n", [65, 4097])
def test_moments_are_bit_identical_however_grouped(n):
    G = 5
    R = synth.uniform_rotations(G * n, seed=3).astype(np.float32).reshape(G, n, 3, 3)
    lw = (np.random.default_rng(4).standard_normal((G, n)) * 2.0).astype(np.float32)
    for Rc, lwc, one in ((R, lw, lambda g: (R[g:g + 1], lw[g:g + 1])), (R, None, lambda g: (R[g:g + 1], None)),
                         (R[0], lw, lambda g: (R[0], lw[g:g + 1]))):
        together = _moments_dev(Rc, lwc)
        for g in range(G):
            assert np.array_equal(together[g:g + 1], _moments_dev(*one(g))), (n, g)


# ---- sampler -> fit ----------------------------------------------------------------------------------------------------------------

def _sampler_cases():
    r = fe.uniform_rotations64(2, seed=31)
    return [("diag531", np.diag([5.0, 3.0, 1.0])), ("rot302010", r[0] @ np.diag([30.0, 20.0, 10.0]) @ r[1].T),
            ("diag51m1", np.diag([5.0, 1.0, -1.0])), ("zero", np.zeros((3, 3)))]


@pytest.mark.parametrize("name,A", _sampler_cases(), ids=[n for n, _ in _sampler_cases()])
def test_sample_then_fit_recovers_A(name, A):
    """n = 2^16 draws of MF(A) from the device sampler, fitted: |s_hat - s| <= 5 sqrt(diag(H_ref^-1) / n) (the MLE's asymptotic standard
    error, H the Fisher information of s), and the likelihood-ratio statistic 2 n (l(A_hat) - l(A)) in [-eps, q]: l(X) = tr(X^T M) -
    log c(X) by the reference on the device's moment M, q the chi-square(9) quantile at tail 1e-6 (A has 9 free parameters), eps = 4 n x
    1e-10 max(1, log c): the reference's log_c is gated at 1e-10 relative and enters twice."""
    n = 1 << 16
    torch.manual_seed(1234)
    R = MatrixFisherN(torch.from_numpy(A.astype(np.float32)).cuda().reshape(1, 3, 3))._sample(n)[0]
    fisher.sampler_failures()
    M = fisher.rotation_moments(R)
    fit = fisher.fit_matrix_fisher(M)
    assert int(fit["status"][0]) == 0
    s_hat, A_hat, M = fit["s"][0].cpu().numpy(), fit["A"][0].cpu().double().numpy(), M[0].cpu().numpy()
    s = fe.proper_svd64(A)[1][0]
    H = np.empty((3, 3))
    for j in range(3):
        e = np.zeros(3)
        e[j] = 1e-3 * max(1.0, abs(s[j]))
        H[:, j] = (fe.mean_Q(s + e) - fe.mean_Q(s - e)) / (2 * e[j])
    se = np.sqrt(np.diag(np.linalg.inv(0.5 * (H + H.T))) / n)
    print(name, "s_hat", s_hat, "s", s, "|s_hat - s| / se", np.abs(s_hat - s) / se)
    assert (np.abs(s_hat - s) <= 5 * se).all()

    def ell(X):
        return float((X * M).sum() - fe.log_c(fe.proper_svd64(X)[1][0]))
    lr = 2 * n * (ell(A_hat) - ell(A))
    q = chi2.isf(1e-6, 9)
    eps = 4 * n * 1e-10 * max(1.0, fe.log_c(s))
    print(name, "likelihood ratio statistic %.3f in [-%.3g, %.3f]" % (lr, eps, q))
    assert -eps <= lr <= q


# ---- MatrixFisherN.fit ---------------------------------------------------------------------------------------------------------------

def test_fit_classmethod_shapes_and_the_grid_density():
    """The three accepted shapes; and a known Fisher's own log-density on the level-2 grid (4608 rows) as log-weights: the fitted A has
    E[R] = the grid moment, whatever the grid resolution -- |U diag(mean_Q(s_fit)) V^T - M|_inf <= RESIDUAL with U, V of the reference's
    SVD of M and the fp64 s the fit returns; A (fp32) is U diag(s) V^T at 4 fp32 ulps of s0; ``mean_rotation()`` (fp32 in, fp32 out)
    meets M at 9 x 2^-24 s0 + 2^-23: dE[R]_ij = sum_kl Cov(R_ij, R_kl) dA_kl with |Cov| <= 1 and |dA_kl| <= 2^-24 s0 for the rounded A,
    plus the rounding of its own fp32 output."""
    n, G = 300, 3
    R = torch.from_numpy(synth.uniform_rotations(G * n, seed=12).astype(np.float32)).cuda().reshape(G, n, 3, 3)
    lw = torch.from_numpy(np.random.default_rng(13).standard_normal((G, n)).astype(np.float32)).cuda()
    one, many, shared = MatrixFisherN.fit(R[0]), MatrixFisherN.fit(R), MatrixFisherN.fit(R[0], lw)
    for dist, rows in ((one, 1), (many, G), (shared, G)):
        assert dist.norm_type == "exact" and dist.A.shape == (rows, 3, 3) and dist.A.is_cuda
        assert dist.fit_status.shape == (rows,) and dist.fit_status.dtype == torch.int32 and not bool(dist.fit_status.any())
        assert dist.log_const().shape == (rows,)
    assert torch.equal(one.A, many.A[:1])
    with pytest.raises(NotImplementedError):
        MatrixFisherN.fit(R[0], norm_type=1)
    with pytest.raises(ValueError):
        MatrixFisherN.fit(R, lw[:2])

    r = fe.uniform_rotations64(2, seed=14)
    A = (r[0] @ np.diag([5.0, 3.0, 1.0]) @ r[1].T).astype(np.float32)
    grid = sd.generate_healpix_grid(2, device=torch.device("cuda"))
    assert grid.shape[0] == 4608
    known = MatrixFisherN(torch.from_numpy(A).cuda().reshape(1, 3, 3), "exact")
    logp = known._log_prob(grid).reshape(1, -1)
    dist = MatrixFisherN.fit(grid, logp)
    M = fisher.rotation_moments(grid, logp)[0].cpu().numpy()
    assert np.abs(M - _moments_ref(grid.cpu().numpy(), logp.cpu().numpy())[0]).max() <= MOMENT_TOL
    U, d, V = fe.proper_svd64(M)
    s_fit = dist.fit_s[0].cpu().numpy()
    assert int(dist.fit_status[0]) == 0
    assert np.abs(U[0] @ np.diag(fe.mean_Q(s_fit)) @ V[0].T - M).max() <= RESIDUAL
    assert np.abs(dist.A[0].cpu().double().numpy() - U[0] @ np.diag(s_fit) @ V[0].T).max() <= 4 * EPS32 * s_fit[0]
    assert np.abs(dist.mean_rotation()[0].cpu().double().numpy() - M).max() <= 9 * 2.0 ** -24 * s_fit[0] + 2.0 ** -23


# ---- harness.grid_pose_fisher ----------------------------------------------------------------------------------------------------------

def test_grid_pose_fisher():
    from tests.test_gpu_grid_pose import _flow, _offset
    _, _, fl = _flow()
    B = 3
    feat = torch.from_numpy(synth.features(B, 32, seed=21)).cuda()
    O = _offset()
    a = harness.grid_pose_fisher(fl, feat, recursion_level=2, offset=O, images_per_launch=1)
    b = harness.grid_pose_fisher(fl, feat, recursion_level=2, offset=O, images_per_launch=3)
    for k in ("A", "mean_rotation", "mode", "s", "entropy", "status", "moments"):
        assert torch.equal(a[k], b[k]), k
    assert a["A"].shape == (B, 3, 3) and a["s"].shape == (B, 3) and a["s"].dtype == torch.float64
    assert not bool(a["status"].any())
    mode = a["mode"].double()
    assert (mode @ mode.transpose(-1, -2) - torch.eye(3, device="cuda", dtype=torch.float64)).abs().max().item() <= 1e-6
    assert (torch.linalg.det(mode) - 1.0).abs().max().item() <= 1e-6
    assert bool((a["entropy"] <= 0).all())
    # the moment from the grid search's own log-densities, in long double
    grid = sd.generate_healpix_grid(2, device=feat.device, offset=O)
    with torch.no_grad():
        lp = torch.cat([x[3] for x in grid_pose._grid_launches(fl, feat, grid, B, None, None, None, "test")])
    est, best, index, _ = harness.grid_estimate_rotations(fl, feat, recursion_level=2, offset=O)
    assert torch.equal(lp.max(-1).values, best)
    want = _moments_ref(grid.cpu().numpy(), lp.cpu().numpy())
    assert np.abs(a["moments"].cpu().numpy() - want).max() <= MOMENT_TOL
    U, d, V = fe.proper_svd64(want)
    s = a["s"].cpu().numpy()
    fitted = np.einsum("bik,bk,bjk->bij", U, mean_Q_batch(s), V)
    assert np.abs(fitted - want).max() <= RESIDUAL
    coupled = type("Coupled", (torch.nn.Module,), {"_rnf_batch_coupled": True})()
    fl.add_module("_test_coupled", coupled)
    try:
        with pytest.raises(ValueError):
            harness.grid_pose_fisher(fl, feat, recursion_level=2, offset=O)
    finally:
        del fl._modules["_test_coupled"]


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------

def test_graph_capture_of_moments_and_fit():
    """Both entries captured in one graph; two replays with new inputs copied into the captured buffers are bit-equal to eager runs."""
    n, G = 4097, 3
    data = []
    for seed in (51, 52, 53):
        R = torch.from_numpy(synth.uniform_rotations(n, seed=seed).astype(np.float32)).cuda()
        lw = torch.from_numpy((np.random.default_rng(seed).standard_normal((G, n)) * 2).astype(np.float32)).cuda()
        data.append((R, lw))

    def step(R, lw):
        M = fisher.rotation_moments(R, lw)
        fit = fisher.fit_matrix_fisher(M)
        return M, fit["A"], fit["s"], fit["hessian"], fit["iterations"], fit["status"]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [[x.clone() for x in step(R, lw)] for R, lw in data]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    R_in, lw_in = data[0][0].clone(), data[0][1].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(R_in, lw_in)
    for (R, lw), want in zip(data[1:], eager[1:]):
        R_in.copy_(R)
        lw_in.copy_(lw)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, want):
            assert torch.equal(x, y)
