"""GPU (-m gpu): condrot_utv_kernel (rnf_condrot_svd / rnf_condrot_matrices, one thread per sample through csrc/svd4_lapack.h) on its own,
every sample against fp64 (tests/svd4_exact.py) with LAPACK's fp32 routine on the same input as the yardstick, like tests/test_svd4.py
does for the host build of the same header.  The device build is compiled with -O3 and default contraction (FMAs where the host test
has none), so it is a different rounding of the same algorithm and is judged on its own.

The kernel adds I to its input.  Every test passes fp32(M - I), formed in fp64 and rounded once, and judges against the matrix the kernel
sees, fp32(input) + I in fp32 arithmetic (one exact-rounded add per diagonal entry, which contraction cannot change).
"""
import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib
from tests import svd4_exact as sx
from tests.test_svd4 import _lapack32, _svd, check_batch_against_lapack, check_edges, hs  # noqa: F401  (hs: the host build, a fixture)

pytestmark = pytest.mark.gpu

GUARD = 16                     # rows behind row n-1 of every output buffer that no launch may touch
SENTINEL = -12345.0
EYE32 = np.eye(4, dtype=np.float32)


def _as_input(M):
    """(the kernel's input [n,16] fp32, the matrix the kernel sees [n,4,4] fp32)."""
    M = np.asarray(M).reshape(-1, 4, 4)
    with np.errstate(invalid="ignore"):
        inp = (M.astype(np.float64) - np.eye(4)).astype(np.float32)
        return np.ascontiguousarray(inp.reshape(-1, 16)), inp + EYE32


def _device(inp, n=None, factors=True):
    """Run the first n rows of inp [N,16] (numpy fp32 or a device tensor).  Returns numpy (rot [n,4,4], U, S, VT, flag); U = S = VT = None
    for rnf_condrot_matrices.  Every output buffer carries GUARD sentinel rows behind row n-1, checked here."""
    x = inp if torch.is_tensor(inp) else torch.from_numpy(inp).cuda()
    n = x.shape[0] if n is None else n
    bufs = [torch.full((n + GUARD, w), SENTINEL, dtype=torch.float32, device="cuda") for w in ((16, 16, 4, 16) if factors else (16,))]
    flag = torch.zeros(1 + GUARD, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if factors:
        rot, U, S, VT = bufs
        _lib.check(_lib.lib().rnf_condrot_svd(x.data_ptr(), n, rot.data_ptr(), U.data_ptr(), S.data_ptr(), VT.data_ptr(), flag.data_ptr(), stream))
    else:
        _lib.check(_lib.lib().rnf_condrot_matrices(x.data_ptr(), n, bufs[0].data_ptr(), flag.data_ptr(), stream))
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[n:] == SENTINEL).all()), ("written past row n-1", n, tuple(b.shape))
    assert int(flag[1:].abs().max()) == 0
    out = [b[:n].cpu().numpy() for b in bufs]
    out = [o.reshape(n, 4, 4) if o.shape[1] == 16 else o for o in out] + [None] * (4 - len(bufs))
    return (*out, int(flag[0]))


def _dot_gate(U, VT):
    """|fl32(u . v) - u . v| for a 4-term fp32 dot product, contracted or not: <= 4 * 2^-24 |u| |v| (gamma_4), the norms being 1 up to the
    factors' own orthogonality error."""
    return 4 * sx.EPS32 * (1 + max(np.abs(np.einsum("nki,nki->ni", U, U) - 1).max(), np.abs(np.einsum("nik,nik->ni", VT, VT) - 1).max())) / (1 - 4 * sx.EPS32)


# ---- every sample of the random batches ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spread", sx.SPREADS)
def test_every_random_sample_on_the_device(hs, spread):
    """All 20 000 matrices of each batch of tests/test_svd4.py through rnf_condrot_svd: sign class of the fp64 rotation and factor checks
    within 2x LAPACK fp32's batch maximum, rot = U^T V of the returned factors, LAPACK's exact signs on >= 99.7 %; and against the HOST
    build of the same header: the share of bit-equal rotations is reported, not gated (it measures what contraction changes), and every
    sample that differs passes the fp64 gate like the rest.

    Measured on an MI355X, spread 0.05 / 0.5 / 3.0: conditioned sign-class error max 0.78 / 4.4 / 6.8 (LAPACK fp32 on the same input 0.97 /
    4.5 / 8.0), LAPACK's exact signs on 99.81 / 99.89 / 99.92 %.  NO rotation is bit-equal to the host build's (share 0.0000 in all three
    batches: with FMAs in the Householder updates every sample differs in some last bit), and on 32 / 16 / 24 of the 20 000 samples the
    two builds of one header land in different sign classes (max |device - host| 0.18 / 1.4 / 1.9), as any two LAPACK builds do; every
    one of them passes the fp64 gate."""
    inp, M = _as_input(sx.random_batch(spread))
    rot, U, S, VT, flag = _device(inp)
    assert flag == 0
    got, ref = check_batch_against_lapack(M, rot, U, S, VT, f"device build, spread {spread}")
    # rot against U^T V of the returned factors in fp64
    utv = np.einsum("nki,njk->nij", U.astype(np.float64), VT.astype(np.float64))
    assert np.abs(rot - utv).max() <= _dot_gate(U.astype(np.float64), VT.astype(np.float64)), np.abs(rot - utv).max()
    # LAPACK's exact signs
    share = np.mean(np.abs(rot - _lapack32(M)[0]).reshape(len(M), -1).max(1) < 1e-4)
    print(f"device build, spread {spread}: LAPACK's exact signs on {share:.5f} of the batch")
    assert share > 0.997, share
    # device build against host build
    hrot = _svd(hs, M)[0]
    differs = (rot != hrot).any((-1, -2))
    _, S64 = sx.utv64(M)
    cond = sx.conditioned(sx.sign_class_error(rot, M), S64)
    other_class = sx.sign_class(rot, M)[1] != sx.sign_class(hrot, M)[1]
    print(f"device build, spread {spread}: rot bit-equal to the host build's on {1 - differs.mean():.5f} of the batch, max |device - host| "
          f"{np.abs(rot - hrot).max():.3e}, another sign class on {int(other_class.sum())} samples")
    assert differs.sum() == 0 or cond[differs].max() <= 2 * ref


# ---- edge matrices and the flag ----------------------------------------------------------------------------------------------------------

# EDGE_M entries that do not survive the kernel's "+ I": fp32(fp32(M - I) + I) != M.  The small scales lose their diagonal (-1 + 1e-12 is -1
# in fp32); the two matrices with generic diagonal entries below 1/2 lose those entries' last bits.
NOT_FEEDABLE = ["rank2", "orthogonal", "scale_1e-30", "scale_1e-20", "scale_1e-16", "scale_1e-12"]


def _hollow(e):
    """What a caller CAN feed at a small scale: the conditioner's output -I plus something tiny off the diagonal.  Zero diagonal, N(0,1) *
    10^e elsewhere; survives the round trip exactly."""
    M = np.random.default_rng(100 - e).standard_normal((4, 4)) * 10.0 ** e
    np.fill_diagonal(M, 0.0)
    return M.astype(np.float32)


def test_edge_matrices_on_the_device():
    """EDGE_M through the kernel under the conditions of the host test (tests/test_svd4.py check_edges), without the NOT_FEEDABLE entries and
    with three kinds of extras that are feedable: `rank2` and `orthogonal` as the round trip leaves them (still degenerate to 1e-7), and
    hollow matrices at the scales 1e-30 .. 1e-12 for the scaled-up path."""
    inp, seen = _as_input(sx.EDGE_STACK)
    same = np.array([np.array_equal(a, b) for a, b in zip(seen, sx.EDGE_STACK)])
    assert [n for n, ok, fin in zip(sx.EDGE_NAMES, same, sx.EDGE_FINITE) if fin and not ok] == NOT_FEEDABLE
    keep = same | ~sx.EDGE_FINITE                                   # a NaN / inf entry stays one, whatever the rest rounds to
    names = [n for n, k in zip(sx.EDGE_NAMES, keep) if k]
    mats = [seen[keep]]
    for name in ("rank2", "orthogonal"):
        mats.append(seen[sx.EDGE_NAMES.index(name)][None])
        names.append(name + "_as_rounded")
    for e in (-30, -20, -16, -12):
        mats.append(_hollow(e)[None])
        names.append(f"hollow_1e{e}")
    inp, seen2 = _as_input(np.concatenate(mats))
    fin = np.isfinite(seen2).all((-1, -2))
    assert np.array_equal(seen2[fin], np.concatenate(mats)[fin])    # everything in the list is what the kernel sees
    rot, U, S, VT, flag = _device(inp)
    assert flag == 1                                                # the list holds the NaN and the inf matrix
    per_sample = (~fin).astype(np.int32)
    # the flag is one word per launch; which samples raised it: NaN throughout exactly there (check_edges asserts it from `per_sample`)
    assert np.array_equal(np.isnan(rot).any((-1, -2)), ~fin)
    check_edges(seen2, rot, U, S, VT, per_sample, names)
    # the finite ones alone: a clear flag
    assert _device(inp[fin])[4] == 0
    U_s = sx.unique_utv(seen2[fin])
    assert all(U_s[[n for n, f in zip(names, fin) if f].index(f"hollow_1e{e}")] for e in (-30, -20, -16, -12))


def test_one_bad_sample_raises_the_flag_and_touches_no_other_row():
    inp, _ = _as_input(sx.random_batch(0.5, 1001))
    clean = _device(inp)
    assert clean[4] == 0
    bad = inp.copy()
    bad[417, 6] = np.nan
    got = _device(bad)
    assert got[4] == 1
    rest = np.arange(1001) != 417
    for a, b in zip(got[:4], clean[:4]):
        assert np.array_equal(a[rest], b[rest]) and np.isnan(a[417]).all()
    rot_only = _device(bad, factors=False)
    assert rot_only[4] == 1 and np.array_equal(rot_only[0], got[0], equal_nan=True)


def test_the_layer_reports_a_flagged_call_one_call_later():
    """condrot_failures() raises after a ConditionRot evaluation (either mode) that met a NaN matrix, and not after clean ones."""
    from rotationnormflow_amd.flow.rottrans import ConditionRot, _CondRotFn, condrot_failures
    inp, _ = _as_input(sx.random_batch(0.5, 1001))
    good = torch.from_numpy(inp).cuda()
    bad = good.clone()
    bad[5, 0] = float("nan")
    layer = ConditionRot(8)
    feature = torch.zeros(1001, 8, device="cuda")
    condrot_failures()                                              # nothing pending from earlier tests
    for out, fails in ((good, False), (bad, True), (good, False)):
        layer._net = lambda f, out=out: out                         # the conditioner's output, prescribed
        for grad in (False, True):
            rot = layer._rnf_side(feature, grad=grad)
            assert rot.shape == (1001, 16)
            if fails:
                with pytest.raises(RuntimeError, match="ConditionRot"):
                    condrot_failures()
                assert bool(torch.isnan(rot[5]).all()) and bool(torch.isfinite(rot[:5]).all()) and bool(torch.isfinite(rot[6:]).all())
            else:
                condrot_failures()
                assert bool(torch.isfinite(rot).all())
    assert _CondRotFn.apply(good[:0]).shape == (0, 16)
    condrot_failures()


# ---- launch shapes -------------------------------------------------------------------------------------------------------------------------

def test_a_row_is_the_same_in_every_launch_size():
    """n = 0, 1, 63, 64, 65, 4097 and 2^20 (64-thread blocks): row i is bit-equal whatever n it travels in, rnf_condrot_matrices and
    rnf_condrot_svd give bit-equal rot, and nothing is written past row n-1 (guard rows in every output buffer, checked in _device)."""
    N = 1 << 20
    torch.manual_seed(11)
    x = (0.5 * torch.randn(N, 16)).cuda()
    full = _device(x)
    assert full[4] == 0
    # the big launch against fp64, every row: orthogonal and in a sign class (the batch gates need LAPACK on 2^20 matrices; the small
    # launches below are judged through bit-equality with these rows and the random-batch tests judge the routine)
    M = x.cpu().numpy().reshape(N, 4, 4) + EYE32
    head = slice(0, 20000)
    check_batch_against_lapack(M[head], *(a[head] for a in full[:4]), "device build, first 20000 rows of 2^20")
    tail = slice(N - 20000, N)
    check_batch_against_lapack(M[tail], *(a[tail] for a in full[:4]), "device build, last 20000 rows of 2^20")
    assert np.array_equal(_device(x, factors=False)[0], full[0])
    for n in (0, 1, 63, 64, 65, 4097):
        part = _device(x, n)
        assert part[4] == 0
        for a, b in zip(part[:4], full[:4]):
            assert a.shape[0] == n and np.array_equal(a, b[:n]), n
        assert np.array_equal(_device(x, n, factors=False)[0], full[0][:n]), n


# ---- the analytic backward on device factors ---------------------------------------------------------------------------------------------

GRAD_DEVICE = "cuda"


def _grad_figure(rot, U, S, VT, G, M):
    """condrot_grad in fp32 on given fp32 factors against fp64 autograd of torch.linalg.svd on the same matrices, per sample:
    max|got - want| / max|want| * relative gap / 2^-24.  The routine's sign class D (rot = D rot64 D) is taken from sign_class; with it
    <G, rot> = <D G D, rot64>, which fp64 autograd differentiates.  The gradient is ~ |G| / gap and every factor entering it is off by
    ~ 2^-24 / relative gap, so the figure is O(1) like `conditioned`."""
    from rotationnormflow_amd.flow.rottrans import condrot_grad
    n = len(M)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(n, -1).to(GRAD_DEVICE)
    got = condrot_grad(t(rot), t(U), t(S), t(VT), t(G)).cpu().double().numpy()      # fp32 torch ops on the device, as the layer runs them
    D = sx.SIGNS[sx.sign_class(rot, M)[1]]
    M64 = torch.from_numpy(M.astype(np.float64)).requires_grad_(True)
    U64, _, VT64 = torch.linalg.svd(M64)
    rot64 = U64.transpose(-1, -2) @ VT64.transpose(-1, -2)
    DGD = torch.from_numpy(D[:, :, None] * G.astype(np.float64) * D[:, None, :])
    (rot64 * DGD).sum().backward()
    want = M64.grad.numpy().reshape(n, 16)
    _, S64 = sx.utv64(M)
    return np.abs(got - want).max(1) / np.abs(want).max(1) * sx.rel_gap(S64) / sx.EPS32, sx.rel_gap(S64)


def test_condrot_grad_on_device_factors_against_fp64_autograd():
    """The backward ConditionRot trains through, fed with the DEVICE routine's factors, against fp64 autograd of the SVD.  Samples with a
    relative gap below 1e-2 are left out (the derivative blows up where singular values meet); for I + 0.5 N(0,1) that is well under
    25 % of the batch, asserted on the input alone.  Yardstick as everywhere: the same figure from LAPACK fp32's factors, gate 2x its
    maximum.  At M = I exactly (the layer at zero-initialised last weights) the derivative does not exist: finite is all that is asked."""
    from rotationnormflow_amd.flow.rottrans import condrot_grad
    n = 4000
    inp, M = _as_input(sx.random_batch(0.5, n))
    G = np.random.default_rng(7).standard_normal((n, 4, 4)).astype(np.float32)
    rot, U, S, VT, flag = _device(inp)
    assert flag == 0
    fig, gap = _grad_figure(rot, U, S, VT, G, M)
    lrot, lU, lS, lVT = _lapack32(M)
    lfig, _ = _grad_figure(lrot, lU, lS, lVT, G, M)
    use = gap >= 1e-2
    assert 1 - use.mean() < 0.25, 1 - use.mean()
    print(f"condrot_grad on device factors: figure max {fig[use].max():.3f}, on LAPACK fp32 factors {lfig[use].max():.3f}, left out {1 - use.mean():.4f}")
    assert fig[use].max() <= 2 * lfig[use].max(), (fig[use].max(), lfig[use].max(), int(np.where(use)[0][fig[use].argmax()]))
    # M = I exactly
    z = torch.zeros(3, 16, device="cuda")
    r1, U1, S1, VT1, f1 = _device(z)
    assert f1 == 0 and np.array_equal(r1, np.broadcast_to(EYE32, (3, 4, 4))) and np.array_equal(S1, np.ones((3, 4), np.float32))
    g1 = condrot_grad(*(torch.from_numpy(a).reshape(3, -1).cuda() for a in (r1, U1, S1, VT1)), torch.randn(3, 16, device="cuda"))
    assert bool(torch.isfinite(g1).all())
