"""GPU (-m gpu): the exact matrix-Fisher normaliser on the device (rnf_fisher_exact, norm_type="exact") against the independent fp64
references of tests/fisher_exact.py: the log-constant on degenerate, extreme and random A, its independence of the batch, the C ABI's
argument handling, the mean rotation and the entropy, the gradient w.r.t. A (closed form, through a linear head, and as a score that
vanishes at the truth), the normalisation of the density (which the Laplace form, norm_type 1, misses), the fused flow path and graph
capture.

Gates that rest on statistics alone use 5 standard errors (exact ones from fe.mc_rel_std, or the samples' own); every stream is seeded."""
import numpy as np
import pytest
import torch

from oracle import flow_oracle as orc
from rotationnormflow_amd import _lib, make_config, synth
from rotationnormflow_amd.utils.fisher import MatrixFisherN, matrix_fisher_norm_N, sampler_failures
from tests import fisher_exact as fe
from tests.gpu_helpers import product_flow

pytestmark = pytest.mark.gpu

EDGE = dict(fe.EDGE_A)


def _f32(A):
    """fp32 copy of A (what the kernels see) and its exact fp64 value (what the references use)."""
    A32 = np.ascontiguousarray(np.asarray(A, np.float64).reshape(-1, 3, 3).astype(np.float32))
    return A32, A32.astype(np.float64)


def _random_A(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3, 3)) * 10.0 ** rng.uniform(-4, 4, (n, 1, 1))


def _rot(seed):
    return fe.uniform_rotations64(1, seed)[0]


def _mean_want(A64):
    """(U diag(mean_Q) V^T, s, mean_Q) per row in fp64."""
    U, s, V = fe.proper_svd64(A64)
    m = np.stack([fe.mean_Q(x) for x in s])
    return np.einsum("bik,bk,bjk->bij", U, m, V), s, m


@pytest.fixture(scope="module")
def big_batch():
    """EDGE_STACK + 4099 random matrices at scales 1e-4 .. 1e4 (B = 4119), with the exact log c of every row."""
    A32, A64 = _f32(np.concatenate([fe.EDGE_STACK, _random_A(4099, seed=45)]))
    _, s, _ = fe.proper_svd64(A64)
    want = np.array([fe.log_c(x) for x in s])
    return A32, A64, want


def _exact(A32, c=True, mean=True):
    """rnf_fisher_exact through the C ABI on a device copy of A32 -> (c, mean) tensors (None where not asked for)."""
    A = torch.from_numpy(A32).cuda()
    B = A.shape[0]
    co = torch.empty(B, dtype=torch.float32, device="cuda") if c else None
    mo = torch.empty(B, 3, 3, dtype=torch.float32, device="cuda") if mean else None
    _lib.check(_lib.lib().rnf_fisher_exact(A.data_ptr(), B, co.data_ptr() if c else None, mo.data_ptr() if mean else None,
                                           torch.cuda.current_stream().cuda_stream))
    return co, mo


def test_log_const_against_the_exact_reference(big_batch):
    A32, _, want = big_batch
    c = MatrixFisherN(torch.from_numpy(A32).cuda(), "exact").log_const().cpu().double().numpy()
    assert c.shape == want.shape and np.isfinite(c).all()
    rel = np.abs(c - want) / np.maximum(1.0, np.abs(want))
    print("worst |c - log_c| / max(1, |log_c|) = %.3g at row %d" % (rel.max(), rel.argmax()))
    assert (rel <= 3e-7).all(), (rel.max(), rel.argmax())


def test_a_row_does_not_depend_on_the_batch(big_batch):
    A32 = big_batch[0]
    row = A32[len(fe.EDGE_NAMES) + 7:len(fe.EDGE_NAMES) + 8]
    c1, m1 = _exact(row)
    for B in (63, 64, 65, 4119):
        batch = np.ascontiguousarray(np.concatenate([A32[:B - 1], row]))
        c, m = _exact(batch)
        assert torch.equal(c[-1:], c1) and torch.equal(m[-1:], m1), B
    assert torch.equal(MatrixFisherN(torch.from_numpy(row).cuda(), "exact").log_const(), c1)


def test_c_abi_argument_handling():
    L = _lib.lib()
    err = lambda: L.rnf_last_error().decode()      # noqa: E731
    A32, A64 = _f32(fe.EDGE_STACK)
    A = torch.from_numpy(A32).cuda()
    B = A.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    assert L.rnf_fisher_exact(A.data_ptr(), B, None, None, st) != 0 and "null" in err()
    assert L.rnf_fisher_exact(A.data_ptr(), 0, A.data_ptr(), None, st) == 0
    assert L.rnf_fisher_exact(A.data_ptr(), -1, A.data_ptr(), None, st) != 0
    c_both, m_both = _exact(A32)
    c_only, _ = _exact(A32, mean=False)
    _, m_only = _exact(A32, c=False)
    assert torch.equal(c_both, c_only) and torch.equal(m_both, m_only)
    # the same constants through the norm_type entry point; type 2 stays refused there
    c_nt = torch.empty(B, dtype=torch.float32, device="cuda")
    assert L.rnf_fisher_log_const_nt(A.data_ptr(), B, _lib.FISHER_NORM_EXACT, None, 0, c_nt.data_ptr(), st) == 0
    assert torch.equal(c_nt, c_both)
    assert L.rnf_fisher_log_const_nt(A.data_ptr(), B, 2, None, 0, c_nt.data_ptr(), st) != 0 and "norm_type" in err()
    assert L.rnf_abi_version() == 8
    # Python: integer 3 stays refused and points to "exact"; a host A is refused
    with pytest.raises(NotImplementedError, match="exact"):
        MatrixFisherN(A, 3)
    with pytest.raises(NotImplementedError, match="exact"):
        matrix_fisher_norm_N(A, 3)
    with pytest.raises(RuntimeError):
        MatrixFisherN(torch.from_numpy(A32), "exact")
    # .norm = exp(c - sum s), also through the module-level helper
    _, s, _ = fe.proper_svd64(A64)
    log_c = np.array([fe.log_c(x) for x in s])
    want = np.exp(log_c - s.sum(-1))
    for got in (MatrixFisherN(A, "exact").norm, matrix_fisher_norm_N(A, "exact")):
        got = got.cpu().double().numpy()                            # c carries 3e-7 max(1, |c|); the fp32 result another rounding
        assert (np.abs(got - want) <= (3e-7 * np.maximum(1.0, np.abs(log_c)) + 2e-7) * want).all()


def test_mean_rotation_and_entropy_on_edge_matrices():
    A32, A64 = _f32(fe.EDGE_STACK)
    want, s, m = _mean_want(A64)
    h_want = np.array([fe.log_c(x) for x in s]) - (s * m).sum(-1)
    for norm_type in ("exact", 1):                                  # always from the exact kernel, whatever the instance's norm_type
        dist = MatrixFisherN(torch.from_numpy(A32).cuda(), norm_type)
        got = dist.mean_rotation().cpu().double().numpy()
        h = dist.entropy().cpu().double().numpy()
        assert got.shape == (len(A32), 3, 3) and h.shape == (len(A32),)
        for b, name in enumerate(fe.EDGE_NAMES):
            tol = 2e-6 * max(1.0, np.abs(want[b]).max())
            if s[b, 1] < 1e-6 * s[b, 0]:                            # free singular vectors: compare what is determined
                assert abs(np.linalg.norm(got[b]) - np.linalg.norm(want[b])) <= tol, name
                tr_want = (A64[b] * want[b]).sum()
                assert abs((A64[b] * got[b]).sum() - tr_want) <= 2e-6 * max(1.0, abs(tr_want)), name
            else:
                assert np.abs(got[b] - want[b]).max() <= tol, (name, np.abs(got[b] - want[b]).max())
            assert abs(h[b] - h_want[b]) <= 2e-6 * max(1.0, abs(h_want[b])), (name, h[b], h_want[b])


GRAD_ROWS = ["2I", "2rot", "diag441", "big1e3", "rand32_0", "zero", "minus3I", "diag51m1", "tiny", "aniso"]


def test_gradient_wrt_A_against_the_closed_form():
    """d/dA sum_i g_i log p(R_i) = T - G E[R] with T = sum g_i R_i, G = sum g_i, also on the rows the Laplace form cannot serve."""
    A32, A64 = _f32(np.stack([EDGE[k] for k in GRAD_ROWS]))
    B, per = len(GRAD_ROWS), 1024
    R = torch.from_numpy(fe.uniform_rotations64(B * per, 93).astype(np.float32)).cuda()
    g = torch.from_numpy(np.random.default_rng(94).standard_normal(B * per).astype(np.float32)).cuda()
    R64 = R.cpu().double().numpy().reshape(B, per, 3, 3)
    g64 = g.cpu().double().numpy().reshape(B, per)
    T = np.einsum("bn,bnij->bij", g64, R64)
    G = g64.sum(1)
    want = T - G[:, None, None] * _mean_want(A64)[0]
    A = torch.from_numpy(A32).cuda().requires_grad_(True)
    lp = MatrixFisherN(A, "exact")._log_prob(R)
    (gA,) = torch.autograd.grad((lp * g).sum(), A)
    assert torch.isfinite(gA).all()
    err = np.abs(gA.cpu().double().numpy() - want).max((1, 2))
    scale = np.maximum(1.0, np.abs(want).max((1, 2)))
    print("gradient error / scale per row:", dict(zip(GRAD_ROWS, (err / scale).round(10))))
    assert (err <= 2e-6 * scale).all(), (err, scale)


def test_gradient_reaches_a_linear_head():
    """feature @ W + b -> A (B = 256, four rotations per row): the gradient that arrives at A passes the closed-form check row by row, and
    W and b receive its chain rule (an fp32 product over 256 rows: 1e-5 of the largest entry)."""
    B, per, F = 256, 4, 16
    rng = np.random.default_rng(95)
    feat = torch.from_numpy(rng.standard_normal((B, F)).astype(np.float32)).cuda()
    W = torch.from_numpy((rng.standard_normal((F, 9)) * 0.5).astype(np.float32)).cuda().requires_grad_(True)
    bias = torch.from_numpy(rng.standard_normal(9).astype(np.float32)).cuda().requires_grad_(True)
    R = torch.from_numpy(fe.uniform_rotations64(B * per, 96).astype(np.float32)).cuda()
    g = torch.from_numpy(rng.standard_normal(B * per).astype(np.float32)).cuda()
    A = (feat @ W + bias).reshape(B, 3, 3)
    lp = MatrixFisherN(A, "exact")._log_prob(R)
    gW, gb, gA = torch.autograd.grad((lp * g).sum(), (W, bias, A))
    A64 = A.detach().cpu().double().numpy()
    g64 = g.cpu().double().numpy().reshape(B, per)
    T = np.einsum("bn,bnij->bij", g64, R.cpu().double().numpy().reshape(B, per, 3, 3))
    want = T - g64.sum(1)[:, None, None] * _mean_want(A64)[0]
    err = np.abs(gA.cpu().double().numpy() - want).max((1, 2))
    assert (err <= 2e-6 * np.maximum(1.0, np.abs(want).max((1, 2)))).all(), err.max()
    gA64 = gA.cpu().double().numpy().reshape(B, 9)
    gW_want, gb_want = feat.cpu().double().numpy().T @ gA64, gA64.sum(0)
    assert np.abs(gW.cpu().double().numpy() - gW_want).max() <= 1e-5 * max(1.0, np.abs(gW_want).max())
    assert np.abs(gb.cpu().double().numpy() - gb_want).max() <= 1e-5 * max(1.0, np.abs(gb_want).max())
    assert float(gW.abs().max()) > 0.0


NORMALISED = [("rot1p5m3", _rot(101) @ np.diag([1.0, 0.5, -0.3]) @ _rot(102).T), ("2rot", EDGE["2rot"]), ("diag51m1", EDGE["diag51m1"]),
              ("rand32_0", EDGE["rand32_0"])]


@pytest.fixture(scope="module")
def uniform_2p20():
    return torch.from_numpy(fe.uniform_rotations64(1 << 20, 103).astype(np.float32)).cuda()


@pytest.mark.parametrize("name,A", NORMALISED)
def test_density_integrates_to_one(name, A, uniform_2p20):
    """mean of exp(log p(R)) over 2^20 Haar-uniform rotations is 1 within 5 exact standard errors; with the Laplace normaliser
    (norm_type 1) on the small first matrix it is not -- the reason the exact one exists."""
    A32, A64 = _f32(A)
    s = fe.proper_svd64(A64)[1][0]
    n = uniform_2p20.shape[0]
    band = 5.0 * fe.mc_rel_std(s) / np.sqrt(n) + 1e-6              # + fp32 rounding of log p
    At = torch.from_numpy(A32).cuda()
    with torch.no_grad():
        got = MatrixFisherN(At, "exact")._log_prob(uniform_2p20).double().exp().mean().item()
    print(name, "mean density %.6f, band %.2g" % (got, band))
    assert abs(got - 1.0) <= band, (name, got, band)
    if name == "rot1p5m3":
        with torch.no_grad():
            laplace = MatrixFisherN(At, 1)._log_prob(uniform_2p20).double().exp().mean().item()
        assert abs(laplace - 1.0) > band, (laplace, band)


@pytest.mark.parametrize("name,A", [
    ("rot531", _rot(51) @ np.diag([5.0, 3.0, 1.0]) @ _rot(52).T),
    ("negdet", _rot(53) @ np.diag([4.0, 2.0, -1.5]) @ _rot(54).T),
    ("aniso", EDGE["aniso"]),
])
def test_score_vanishes_at_the_truth(name, A):
    """E_{R ~ MF(A)} d log p(R) / dA = E[R] - dc/dA = 0: the autograd gradient of mean(log p) over 2^18 samples of the exact sampler is
    within 5 standard errors (of the samples' own mean) of 0 per entry, plus 1e-6."""
    n = 1 << 18
    A32, _ = _f32(A)
    torch.manual_seed(111)
    At = torch.from_numpy(A32).cuda().requires_grad_(True)
    R = MatrixFisherN(At.detach())._sample(n)[0]
    sampler_failures()
    (gA,) = torch.autograd.grad(MatrixFisherN(At, "exact")._log_prob(R).mean(), At)
    sem = (R.double().std(0) / np.sqrt(n)).cpu().numpy()
    got = gA[0].cpu().double().numpy()
    assert (np.abs(got) <= 5.0 * sem + 1e-6).all(), (name, got, sem)


@pytest.mark.parametrize("B", [1, 512])
def test_fused_flow_log_prob_shifts_by_the_constant(B):
    """Flow.log_prob with an exact base and with a type-1 base of the same A differ by c1 - c_exact per row, nothing else."""
    cfg = make_config("C1")
    fl = product_flow(cfg, synth.fill_state_dict(orc.state_shapes(cfg), seed=3, regime="trained"))
    n = 512
    R = torch.from_numpy(synth.uniform_rotations(n, seed=121)).cuda()
    rng = np.random.default_rng(122)
    A32, _ = _f32(np.stack([_rot(130 + b) @ np.diag(np.sort(rng.uniform(0.5, 6.0, 3))[::-1]) @ _rot(700 + b).T for b in range(B)]))
    At = torch.from_numpy(A32).cuda()
    exact, laplace = MatrixFisherN(At, "exact"), MatrixFisherN(At, 1)
    with torch.no_grad():
        le = fl.log_prob(R, base=exact)["logp"].double()
        l1 = fl.log_prob(R, base=laplace)["logp"].double()
    shift = (laplace.log_const().double() - exact.log_const().double()).repeat_interleave(n // B)
    assert torch.isfinite(le).all() and shift.abs().max().item() > 1e-2
    tol = 1e-5 * torch.maximum(torch.ones_like(le), torch.maximum(le.abs(), l1.abs()))
    assert ((le - l1 - shift).abs() <= tol).all(), (le - l1 - shift).abs().max().item()


def test_graph_capture_of_constant_log_prob_and_backward():
    """MatrixFisherN(A, "exact"), _log_prob and the backward w.r.t. A captured in one graph: two replays are bit-equal to the eager run."""
    B, per = 65, 8
    A32, _ = _f32(np.concatenate([fe.EDGE_STACK, _random_A(B - len(fe.EDGE_NAMES), seed=141)]))
    A = torch.from_numpy(A32).cuda().requires_grad_(True)
    R = torch.from_numpy(fe.uniform_rotations64(B * per, 142).astype(np.float32)).cuda()
    g = torch.from_numpy(np.random.default_rng(143).standard_normal(B * per).astype(np.float32)).cuda()

    def step():
        dist = MatrixFisherN(A, "exact")
        lp = dist._log_prob(R)
        (gA,) = torch.autograd.grad((lp * g).sum(), A)
        return dist.log_const(), lp.detach(), gA

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [x.clone() for x in step()]
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(2):
        for x in out:
            x.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, eager):
            assert torch.equal(x, y)
