"""GPU (-m gpu): the matrix-Fisher device kernels against the exact fp64 references of tests/fisher_exact.py at degenerate and extreme A.

rnf_fisher_proper_svd (rotations, reconstruction, signs, Bingham parameters), rnf_fisher_log_const_nt (closed forms 0 / 1),
rnf_fisher_log_const_mc (norm_type 2 against the exact log c), rnf_fisher_sample (moments of the exact distribution, the uniform law at
A = 0, multi-row and grid-stride launches), rnf_matrix_to_quaternion (all four branches and their signs), rnf_fisher_log_prob at
concentrated A and rnf_fisher_log_prob_backward_param at repeated singular values.

Tolerances that rest on the statistics alone: the sampler's moments (5 standard errors of the sample itself, plus 1e-6 for fp32 rounding;
for tr(A^T R) plus 3e-7 sum|s| for the fp32 rounding of U and V), the A = 0 angle law (KS p > 1e-4) and the norm_type-2 normaliser (6 exact
relative standard deviations of the Monte-Carlo mean, plus 2e-5 for fp32).  Every random stream is seeded, so every gate is deterministic.
"""
import numpy as np
import pytest
import torch
from scipy import stats

from oracle import flow_oracle as orc
from rotationnormflow_amd import _lib
from rotationnormflow_amd.utils.fisher import MatrixFisherN, device_proper_svd, sampler_failures
from tests import fisher_exact as fe

pytestmark = pytest.mark.gpu

N_MOM = 1 << 18


def _f32(A):
    """fp32 copy of A (what the kernels see) and its exact fp64 value (what the references use)."""
    A32 = np.ascontiguousarray(np.asarray(A, np.float64).reshape(-1, 3, 3).astype(np.float32))
    return A32, A32.astype(np.float64)


def _random_A(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3, 3)) * 10.0 ** rng.uniform(-4, 4, (n, 1, 1))


def _sample(A32, n, seed):
    torch.manual_seed(seed)
    R = MatrixFisherN(torch.from_numpy(A32).cuda())._sample(n)
    sampler_failures()                                              # no rejection loop ran out of proposals
    return R


def _check_moments(R, a64, what):
    """R [n,3,3] (device) ~ MF(a64): rotations; E[R] = U diag(E[Q]) V^T and E[tr(A^T R)] = sum s_i E[Q_ii], within 5 standard errors."""
    n = R.shape[0]
    Rd = R.double()
    eye = torch.eye(3, dtype=torch.float64, device=R.device)
    assert (Rd @ Rd.transpose(-1, -2) - eye).abs().max().item() < 1e-5, what
    assert (torch.linalg.det(Rd) - 1).abs().max().item() < 1e-5, what
    U, s, V = fe.proper_svd64(a64)
    m = fe.mean_Q(s[0])
    ER = U[0] @ np.diag(m) @ V[0].T
    mean, sem = Rd.mean(0).cpu().numpy(), (Rd.std(0) / np.sqrt(n)).cpu().numpy()
    assert (np.abs(mean - ER) < 5 * sem + 1e-6).all(), (what, mean, ER, sem)
    t = (Rd * torch.from_numpy(a64[0]).to(R.device)).sum((-1, -2))
    t_mean, t_sem = t.mean().item(), t.std().item() / np.sqrt(n)
    assert abs(t_mean - float((s[0] * m).sum())) < 5 * t_sem + 3e-7 * np.abs(s[0]).sum() + 1e-6, (what, t_mean, (s[0] * m).sum(), t_sem)


# ---- proper SVD and the closed-form normalisers ----------------------------------------------------------------------------------------

def test_proper_svd_on_edge_and_random_matrices():
    A32, A64 = _f32(np.concatenate([fe.EDGE_STACK, _random_A(4099, seed=41)]))          # B = 4119: not a multiple of the 64-thread block
    U, V, s, lam = (x.cpu().double().numpy() for x in device_proper_svd(torch.from_numpy(A32).cuda()))
    _, s_ref, _ = fe.proper_svd64(A64)
    s0 = s_ref[:, 0]
    eye = np.eye(3)
    for M in (U, V):
        assert np.abs(np.einsum("bki,bkj->bij", M, M) - eye).max() < 1e-6
        assert np.abs(np.linalg.det(M) - 1.0).max() < 1e-6
    assert (np.abs(np.einsum("bik,bk,bjk->bij", U, s, V) - A64).max((1, 2)) <= 2e-6 * s0).all()
    assert (np.abs(s - s_ref).max(1) <= 1e-6 * s0).all()
    assert (s[:, 0] >= s[:, 1]).all() and (s[:, 1] >= np.abs(s[:, 2]) - 1e-6 * s0).all()
    signed = np.abs(s_ref[:, 1] * s_ref[:, 2]) > 1e-6 * s0 ** 2                        # det A clearly away from 0
    assert (np.sign(s[signed, 2]) == np.sign(np.linalg.det(A64[signed]))).all()
    assert (lam[:, 0] == 0).all()
    s32 = s.astype(np.float32).astype(np.float64)
    want = 2.0 * np.stack([s32[:, 1] + s32[:, 2], s32[:, 0] + s32[:, 2], s32[:, 0] + s32[:, 1]], -1)
    assert (np.abs(lam[:, 1:] - want).max(1) <= 1e-6 * s0).all()
    assert (lam[:, 1:] >= -1e-6 * s0[:, None]).all()                                      # Bingham parameters are >= 0 (s1 >= |s2|)


def _log_const(A32, norm_type):
    return MatrixFisherN(torch.from_numpy(A32).cuda(), norm_type).log_const().cpu().double().numpy()


def test_log_const_type1_against_closed_form():
    A32, A64 = _f32(np.concatenate([fe.EDGE_STACK, _random_A(4099, seed=42)]))
    c = _log_const(A32, 1)
    _, s_ref, _ = fe.proper_svd64(A64)
    want = fe.log_const_t1(s_ref)
    names = fe.EDGE_NAMES + ["random"] * 4099
    pair = np.minimum(np.minimum(s_ref[:, 0] + s_ref[:, 1], s_ref[:, 1] + s_ref[:, 2]), s_ref[:, 0] + s_ref[:, 2])
    for b, name in enumerate(names):
        if name in fe.INF_T1_EXACT:
            assert c[b] == np.inf, name
        elif name not in fe.INF_T1 and pair[b] > 1e-3 * s_ref[b, 0]:                     # a well-conditioned closed form
            assert abs(c[b] - want[b]) <= 3e-7 * max(1.0, abs(want[b])), (name, c[b], want[b])


def test_log_const_type0_against_closed_form_and_batch_coupling():
    """Type 0 couples the rows through Q = sum_b |A_b|_F^2: a zero row still gets log(1 + Q/6); a lone zero matrix gets 0."""
    rng = np.random.default_rng(43)
    for A in (fe.EDGE_STACK, np.stack([np.diag([5.0, 3.0, 1.0]), np.zeros((3, 3)), 0.5 * rng.standard_normal((3, 3)), fe.EDGE_A[8][1]]),
              np.zeros((1, 3, 3)), 0.3 * rng.standard_normal((257, 3, 3))):
        A32, A64 = _f32(A)
        c = _log_const(A32, 0)
        want = fe.log_const_t0(A64)
        assert np.abs(c - want).max() <= 3e-7 * max(1.0, np.abs(want).max()), (c, want)
    assert _log_const(np.zeros((1, 3, 3), np.float32), 0)[0] == 0.0


@pytest.mark.parametrize("name,A", [
    ("rot531", fe.uniform_rotations64(1, 51)[0] @ np.diag([5.0, 3.0, 1.0]) @ fe.uniform_rotations64(1, 52)[0].T),
    ("negdet", fe.uniform_rotations64(1, 53)[0] @ np.diag([4.0, 2.0, -1.5]) @ fe.uniform_rotations64(1, 54)[0].T),
    ("2rot", 2.0 * fe.uniform_rotations64(1, 55)[0]),
    ("rep331", fe.uniform_rotations64(1, 56)[0] @ np.diag([3.0, 3.0, 0.5]) @ fe.uniform_rotations64(1, 57)[0].T),
])
def test_mc_normaliser_against_exact_log_c(name, A):
    """norm_type 2 (Monte-Carlo over approx_num uniform rotations) against the exact log c; tolerance 6 exact standard deviations."""
    n_mc = 1 << 24
    A32, A64 = _f32(A)
    torch.manual_seed(61)
    c = MatrixFisherN(torch.from_numpy(A32).cuda(), 2, approx_num=n_mc).log_const().item()
    s = fe.proper_svd64(A64)[1][0]
    want = fe.log_c(s)
    tol = 6.0 * fe.mc_rel_std(s) / np.sqrt(n_mc) + 2e-5
    assert abs(c - want) < tol, (name, c, want, tol)


# ---- the sampler against the exact distribution ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", fe.EDGE_NAMES)
def test_sampler_moments_on_edge_matrices(name):
    A32, A64 = _f32(dict(fe.EDGE_A)[name])
    R = _sample(A32, N_MOM, seed=71)
    _check_moments(R[0], A64, name)


def test_sampler_at_zero_is_uniform():
    """A = 0: MF(0) is the Haar measure -- rotation angle with CDF (theta - sin theta) / pi, E[R_ij R_kl] = delta_ik delta_jl / 3."""
    R = _sample(np.zeros((1, 3, 3), np.float32), N_MOM, seed=72)[0].double()
    eye = torch.eye(3, dtype=torch.float64, device=R.device)
    assert (R @ R.transpose(-1, -2) - eye).abs().max().item() < 1e-5
    assert (torch.linalg.det(R) - 1).abs().max().item() < 1e-5
    cos = ((R.diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2).clamp(-1, 1)
    theta = torch.arccos(cos).cpu().numpy()
    assert stats.kstest(theta, lambda x: (x - np.sin(x)) / np.pi).pvalue > 1e-4
    n = R.shape[0]
    prod = torch.einsum("nij,nkl->nijkl", R, R).reshape(n, 81)
    mean, sem = prod.mean(0).cpu().numpy(), (prod.std(0) / np.sqrt(n)).cpu().numpy()
    want = np.einsum("ik,jl->ijkl", np.eye(3), np.eye(3)).reshape(81) / 3.0
    assert (np.abs(mean - want) < 5 * sem + 1e-6).all()
    m1, sem1 = R.mean(0).cpu().numpy(), (R.std(0) / np.sqrt(n)).cpu().numpy()
    assert (np.abs(m1) < 5 * sem1 + 1e-6).all()


def test_sampler_moments_all_edge_rows_in_one_launch():
    A32, A64 = _f32(fe.EDGE_STACK)
    R = _sample(A32, N_MOM, seed=73)
    assert R.shape == (len(fe.EDGE_NAMES), N_MOM, 3, 3)
    for b, name in enumerate(fe.EDGE_NAMES):
        _check_moments(R[b], A64[b:b + 1], name)


def test_sampler_moments_grid_stride():
    """B * n = 3 * 2^20 exceeds the launch's 8192 x 256 threads: the grid-stride loop serves the rest."""
    names = ["rand32_0", "diag441", "big1e4"]
    A32, A64 = _f32(np.stack([dict(fe.EDGE_A)[k] for k in names]))
    R = _sample(A32, 1 << 20, seed=74)
    for b, name in enumerate(names):
        _check_moments(R[b], A64[b:b + 1], name)


def test_sampler_many_rows_one_sample_each():
    """65536 rows of one A at n = 1: every row draws from its own stream, and together they follow MF(A)."""
    a = dict(fe.EDGE_A)["rand32_1"]
    A32, A64 = _f32(np.broadcast_to(a, (1 << 16, 3, 3)))
    R = _sample(A32, 1, seed=75)
    assert R.shape == (1 << 16, 1, 3, 3)
    _check_moments(R[:, 0], A64[:1], "rows")


# ---- matrix_to_quaternion: every branch of the pytorch3d rule ----------------------------------------------------------------------------

def _axis_angle(axis, angle):
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    K = np.zeros(axis.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -axis[..., 2], axis[..., 1], -axis[..., 0]
    K = K - np.swapaxes(K, -1, -2)
    s, c = np.sin(angle)[..., None, None], np.cos(angle)[..., None, None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def _signed_permutations():
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            M = np.zeros((3, 3))
            M[range(3), p] = sg
            if np.linalg.det(M) > 0:
                out.append(M)
    return np.stack(out)


def test_matrix_to_quaternion_branches_and_signs():
    rng = np.random.default_rng(81)
    ax = rng.standard_normal((4096, 3))
    sets = [fe.uniform_rotations64(65536, seed=82),
            np.stack([np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])]),   # pi about the axes
            _axis_angle(ax, np.full(4096, np.pi)),                                                        # pi about random axes
            _axis_angle(ax, np.pi - 10.0 ** rng.uniform(-6, -1, 4096)),                                   # near pi
            np.eye(3)[None], _axis_angle(ax, 10.0 ** rng.uniform(-7, -1, 4096)),                          # identity and near it
            _signed_permutations()]
    R32 = np.ascontiguousarray(np.concatenate(sets).astype(np.float32))
    n = R32.shape[0]
    Rt = torch.from_numpy(R32).cuda()
    q = torch.empty(n, 4, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().rnf_matrix_to_quaternion(Rt.data_ptr(), n, q.data_ptr(), torch.cuda.current_stream().cuda_stream))
    q = q.cpu().double().numpy()
    R64 = R32.astype(np.float64)
    want = orc.matrix_to_quaternion(torch.from_numpy(R64)).numpy()
    m = R64.reshape(n, 9)
    qa = np.sqrt(np.maximum(np.stack([1 + m[:, 0] + m[:, 4] + m[:, 8], 1 + m[:, 0] - m[:, 4] - m[:, 8], 1 - m[:, 0] + m[:, 4] - m[:, 8],
                                      1 - m[:, 0] - m[:, 4] + m[:, 8]], -1), 0.0))
    top = np.sort(qa, -1)
    clear = top[:, 3] - top[:, 2] > 1e-5
    branch = qa.argmax(-1)
    for k in range(4):                                                                    # every branch, with both signs of its entries
        sel = clear & (branch == k)
        assert sel.sum() >= 100, k
        assert ((want[sel] > 1e-3).any(0) & (want[sel] < -1e-3).any(0)).sum() >= 3, k
    err = np.abs(q - want).max(-1)
    assert err[clear].max() < 2e-6                                                        # same branch, same sign
    err_pm = np.minimum(err, np.abs(q + want).max(-1))
    assert err_pm.max() < 2e-6                                                            # ties: the same rotation, up to q -> -q
    assert np.abs(np.linalg.norm(q, axis=-1) - 1).max() < 2e-6
    back = orc.quaternion_to_matrix(torch.from_numpy(q)).numpy()
    assert np.abs(back - R64).max() < 2e-6


# ---- log-density and its parameter gradient -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["big1e3", "big1e4", "aniso", "diag51m0999", "rand32_2"])
def test_log_prob_at_concentrated_A(name):
    """rnf_fisher_log_prob where tr(A^T R) and c nearly cancel (|s| up to 1e4): its error against fp64 is at most twice the fp32 error of
    the oracle's own restatement of the reference."""
    A32, A64 = _f32(dict(fe.EDGE_A)[name])
    R = torch.cat([_sample(A32, 8192, seed=91)[0], torch.from_numpy(fe.uniform_rotations64(1024, 92).astype(np.float32)).cuda()])
    got = MatrixFisherN(torch.from_numpy(A32).cuda())._log_prob(R).cpu().double().numpy()
    Rc = R.cpu()
    want = orc.fisher_log_prob(Rc.double(), torch.from_numpy(A64), torch.float64).numpy()
    o32 = orc.fisher_log_prob(Rc, torch.from_numpy(A32), torch.float32).double().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 2.0 * np.abs(o32 - want).max() + 1e-6, (np.abs(got - want).max(), np.abs(o32 - want).max())


def test_log_prob_backward_param_at_repeated_and_large_singular_values():
    """d log p / dA through rnf_fisher_log_prob_backward_param against the fp64 closed form: sum_i g_i R_i - G dc/dA with
    dc/dA = U diag(f) V^T (type 1) or cofactor / (6 D) plus the batch coupling through Q (type 0)."""
    names = ["2I", "2rot", "diag441", "diag522", "big1e3", "rand32_0"]
    A32, A64 = _f32(np.stack([dict(fe.EDGE_A)[k] for k in names]))
    B, per = len(names), 1024
    R = torch.from_numpy(fe.uniform_rotations64(B * per, 93).astype(np.float32)).cuda()
    g = torch.from_numpy(np.random.default_rng(94).standard_normal(B * per).astype(np.float32)).cuda()
    R64 = R.cpu().double().numpy().reshape(B, per, 3, 3)
    g64 = g.cpu().double().numpy().reshape(B, per)
    T = np.einsum("bn,bnij->bij", g64, R64)
    G = g64.sum(1)
    U, s, V = fe.proper_svd64(A64)
    D = 1.0 + (A64 ** 2).sum() / 6.0 + np.linalg.det(A64) / 6.0
    cof = np.linalg.det(A64)[:, None, None] * np.swapaxes(np.linalg.inv(A64), -1, -2)
    want = {1: T - G[:, None, None] * fe.dlog_const_t1(U, s, V),
            0: T - G[:, None, None] * cof / (6.0 * D[:, None, None]) - (G / D).sum() * A64 / 3.0}
    for norm_type in (1, 0):
        A = torch.from_numpy(A32).cuda().requires_grad_(True)
        lp = MatrixFisherN(A, norm_type)._log_prob(R)
        (gA,) = torch.autograd.grad((lp * g).sum(), A)
        err = np.abs(gA.cpu().double().numpy() - want[norm_type]).max((1, 2))
        scale = np.maximum(1.0, np.abs(want[norm_type]).max((1, 2)))
        assert (err <= 2e-6 * scale).all(), (norm_type, err, scale)
