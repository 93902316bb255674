"""GPU (-m gpu): polar3 (csrc/so3_math.h) inside the kernels that inline it, every sample against fp64 (tests/polar3_exact.py) with the gates of
tests/test_polar3_host.py: LAPACK fp32's batch maximum on the same kind of matrix, times two.

The matrix reaches polar3 from the conditioner's registers, so chosen matrices are fed through a STEERING NETWORK: on the 3x3 layer's net
every hidden layer is zero, fc_first copies feature i into hidden unit i (i < 18) and fc_last takes unit i minus unit 9 + i.  With
D = M - I and the features [max(D, 0), max(-D, 0), 0 ...] the net returns D with no rounding at all (ReLU of non-negative numbers, products
with 0 and +-1; asserted on the CPU against the fp32 oracle), and the kernel sees M32 = fl(I + D).

The layer is isolated by the flow's own arithmetic: the Moebius layer of the flow ignores the features (their columns of its fc_first are
zero, the rest are the recipe weights), and the 3x3 layer is the LAST layer applied (forward: [mobius, 3x3]; inverse pass: the flow
[3x3, mobius] run backwards).  A second run with zero features has M = I, for which polar3 returns I and the 3x3 product returns its
input bit for bit: that run gives the rotation R that entered the layer, and the first run must give polar(M) R (R polar(M)) to the
layer's own error, 2 x LAPACK's figure x 2^-23 kappa(M) for the rotation plus 4 x 2^-23 for the 3-term fp32 products.
"""
import functools

import numpy as np
import pytest
import torch

import rotationnormflow_amd as rnf
from oracle import flow_oracle as orc
from rotationnormflow_amd import make_config, runtime, synth
from tests import polar3_exact as px
from tests.gpu_helpers import product_flow
from tests.test_polar3_host import hp, polar3 as host_polar3, strictest, yardstick  # noqa: F401  (hp: the host build, a fixture)

pytestmark = pytest.mark.gpu

EYE32 = np.eye(3, dtype=np.float32)
FD = 24
SIDES = ["L", "R"]


def as_features(M):
    """(features [n,24] fp32, the matrix the kernel sees [n,3,3] fp32 = fl(I + D), D = fl(M - I) formed in fp64 and rounded once)."""
    M = np.asarray(M).reshape(-1, 3, 3)
    with np.errstate(invalid="ignore"):
        D = (M.astype(np.float64) - np.eye(3)).astype(np.float32).reshape(-1, 9)
    feat = np.zeros((len(D), FD), np.float32)
    with np.errstate(invalid="ignore"):
        feat[:, :9] = np.where(D > 0, D, 0)
        feat[:, 9:18] = np.where(D < 0, -D, 0)
    bad = ~np.isfinite(D)
    feat[:, :9][bad] = D[bad]                                  # a NaN / inf entry travels as itself
    return feat, D.reshape(-1, 3, 3) + EYE32


@functools.lru_cache(maxsize=None)
def steering_net(rot, kind, inverse):
    """(cfg, weights, index of the 3x3 layer) of the steering flow whose 3x3 layer is `kind` (make_config's rot=`rot`).  inverse: the flow
    whose INVERSE pass applies the 3x3 layer last.  Shared with tests/test_gpu_gs3.py."""
    extra = dict(last_affine=1, first_affine=0) if inverse else {}
    cfg = make_config(layers=1, segments=16, condition=1, feature_dim=FD, rot=rot, **extra)
    kinds = orc.layer_kinds(cfg)
    assert kinds == ([kind, "mobius"] if inverse else ["mobius", kind])
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=31, regime="trained")
    i9, im = (0, 1) if inverse else (1, 0)
    pre = f"layers.{i9}.net"
    for k in w:
        if k.startswith(pre + "."):
            w[k] = np.zeros_like(w[k])
    for i in range(18):
        w[f"{pre}.fc_first.weight"][i, i] = 1.0
    for i in range(9):
        w[f"{pre}.fc_last.weight"][i, i] = 1.0
        w[f"{pre}.fc_last.weight"][i, 9 + i] = -1.0
    w[f"layers.{im}.conditioner.fc_first.weight"][:, 3:] = 0.0            # the Moebius layer does not see the features
    return cfg, w, i9


def steering(side, inverse):
    """(cfg, weights, index of the 3x3 layer).  inverse: the flow whose INVERSE pass applies the 3x3 layer last."""
    return steering_net("9TransLSVD" if side == "L" else "9TransRSVD", "csvdl9" if side == "L" else "csvdr9", inverse)


def assert_net_returns_D(side, inverse, feat, seen):
    cfg, w, i9 = steering(side, inverse)
    p = {k: torch.from_numpy(v) for k, v in w.items()}
    got = orc.cond9_matrix(torch.from_numpy(feat), p, f"layers.{i9}.net").numpy()
    assert np.array_equal(got, seen, equal_nan=True)


@functools.lru_cache(maxsize=None)
def flow_of(side, inverse):
    cfg, w, _ = steering(side, inverse)
    return product_flow(cfg, w)


GUARD = 16                     # rows behind row n-1 of both output buffers that no launch may touch
SENTINEL = -12345.0


def run(side, inverse, R, feat, fl=None):
    """(R' [n,3,3], ldj [n]) numpy fp32 of the flow (its inverse pass) on the device.  The launch is the one Flow.forward / Flow.inverse make
    (runtime.run_flow: the packed flow through runtime._flow_pass), but into buffers of this test, which carry GUARD sentinel rows behind
    row n-1: every run of every test here checks that nothing is written past the batch."""
    fl = flow_of(side, inverse) if fl is None else fl
    Rd, fd = torch.from_numpy(np.ascontiguousarray(R)).cuda(), torch.from_numpy(np.ascontiguousarray(feat)).cuda()
    packed = fl._packed(Rd.device, fd)
    rot, f = runtime._check_inputs(Rd, fd, packed, None)
    n = rot.shape[0]
    out = torch.full((n + GUARD, 3, 3), SENTINEL, dtype=torch.float32, device=Rd.device)
    ldj = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=Rd.device)
    with torch.no_grad():
        runtime._flow_pass(fl, packed, rot, f, fd, 0, inverse, rotation_out=out.data_ptr(), ldj_out=ldj.data_ptr())
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all()) and bool((ldj[n:] == SENTINEL).all()), ("written past row n-1", n)
    return out[:n].cpu().numpy(), ldj[:n].cpu().numpy()


def layer_alone(side, inverse, R, feat):
    """(R' of the run, the rotation that entered the 3x3 layer = R' of the run with M = I, ldj of both)."""
    out, l = run(side, inverse, R, feat)
    base, l0 = run(side, inverse, R, np.zeros_like(feat))
    return out, base, l, l0


def device_Q(side, inverse, out, base):
    """polar3's own result, recovered in fp64 from R' = Q R (L) or R Q (R); the inverse pass applies Q(M^T) = Q^T."""
    o, b = out.astype(np.float64), base.astype(np.float64)
    Q = o @ b.transpose(0, 2, 1) if side == "L" else b.transpose(0, 2, 1) @ o
    return Q.transpose(0, 2, 1) if inverse else Q


def want_out(side, inverse, seen, base):
    Q = px.polar64(seen)
    Q = Q.transpose(0, 2, 1) if inverse else Q
    return Q @ base.astype(np.float64) if side == "L" else base.astype(np.float64) @ Q


@functools.lru_cache(maxsize=None)
def realistic_table(per_kind=820, dmax=None):
    """(seen [n,3,3], features, per-sample LAPACK rotation figure of the sample's kind, LAPACK orthogonality figure).  Realistic window,
    every kind; dmax: only matrices with |D| <= dmax (drawn 8 x as many and cut: a condition on the input)."""
    seen, feat, yr, yo = [], [], [], []
    for kind in px.KINDS:
        M = px.random_batch(kind, per_kind * (8 if dmax else 1), 5)
        f, s = as_features(M)
        keep = px.in_domain(s)
        if dmax:
            keep &= np.abs(s - EYE32).max((-1, -2)) <= dmax
        assert keep.sum() >= (per_kind if dmax else 0.98 * per_kind), (kind, keep.sum())
        f, s = f[keep][:per_kind], s[keep][:per_kind]
        y = yardstick(kind, "realistic")
        seen.append(s); feat.append(f); yr.append(np.full(len(s), y["rot"])); yo.append(np.full(len(s), y["orth"]))
    return tuple(np.concatenate(a) for a in (seen, feat, yr, yo))


def device():
    """The device the flows run on, named as the tensors name it (runtime.fallback_fired keys its workspaces by that name)."""
    return torch.device("cuda", torch.cuda.current_device())


def rotations(n, seed):
    return synth.uniform_rotations(n, seed=seed)


def check_layer(side, inverse, seen, feat, yr, yo, what, extra=0.0):
    """Every sample: R' against polar64(M) R within the gate, R' orthogonal, ldj untouched by the layer."""
    n = len(seen)
    R = rotations(n, 3)
    out, base, l, l0 = layer_alone(side, inverse, R, feat)
    k = px.kappa(seen)
    gate = (2 * yr + extra) * px.U23 * k + 4 * px.U23
    err = np.abs(out - want_out(side, inverse, seen, base)).max((-1, -2))
    o = px.orth_err(out)
    print(f"{what}: max error / gate {np.max(err / gate):.3f}, rotation figure max {np.max(err / (px.U23 * k)):.2f}, |R'R'^T - I| max {o.max() / px.U23:.2f} units "
          f"(input rotations {px.orth_err(base).max() / px.U23:.2f})")
    assert np.isfinite(out).all() and (err <= gate).all(), (what, int(np.argmax(err / gate)), np.max(err / gate))
    assert (o <= 2 * yo + px.orth_err(base) + 4 * px.U23).all(), (what, o.max())
    assert np.array_equal(l, l0), what                             # ldj exactly 0 from the layer
    return out, base


# ---- forward and inverse, both kinds, per sample ---------------------------------------------------------------------------------------------

@pytest.fixture
def fp32():
    old = rnf.get_precision()
    rnf.set_precision("fp32")
    yield
    rnf.set_precision(old)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("side", SIDES)
def test_every_sample_fp32(fp32, side, inverse):
    """Under set_precision("fp32") the matrix arrives exactly at any scale: every kind at realistic scales 10^U(-2,3) (4 100 samples), and
    the `range` window as far as fp32 features carry it, 10^U(0,12) (below 1 the sum I + D keeps the identity's digits, not M's; the
    hollow edges cover small matrices)."""
    seen, feat, yr, yo = realistic_table()
    assert_net_returns_D(side, inverse, feat, seen)
    check_layer(side, inverse, seen, feat, yr, yo, f"fp32, {side}, inverse {inverse}, realistic")
    big = []
    for kind in px.KINDS:
        f, s = as_features(px.random_batch(kind, 400, 6, (0.0, 12.0)))
        keep = px.in_domain(s)
        assert keep.mean() > 0.98
        y = yardstick(kind, "range")
        big.append((s[keep], f[keep], np.full(keep.sum(), y["rot"]), np.full(keep.sum(), y["orth"])))
    seen, feat, yr, yo = (np.concatenate(a) for a in zip(*big))
    assert_net_returns_D(side, inverse, feat, seen)
    check_layer(side, inverse, seen, feat, yr, yo, f"fp32, {side}, inverse {inverse}, scales up to 1e12")


# EDGE_M entries that do not survive I + (M - I) in fp32: generic entries below 1/2 in magnitude lose their last bits against the identity,
# and the small power-of-two scales lose their diagonal altogether (-1 + 2^-40 is -1).  They are fed as the round trip leaves them where
# that is still inside the domain; the hollow matrices (zero diagonal) are what a caller CAN feed at a small scale.
NOT_FEEDABLE = ["rotation", "reflection", "cond_1e3_two_large", "cond_1e3_two_small", "pow2_-60", "pow2_-40"]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("side", SIDES)
def test_in_domain_edges_fp32(fp32, side, inverse):
    feat, seen = as_features(px.EDGE_STACK)
    same = np.array([np.array_equal(a, b) for a, b in zip(seen, px.EDGE_STACK)])
    assert [n for n, ok, dom in zip(px.EDGE_NAMES, same, px.EDGE_IN) if dom and not ok] == NOT_FEEDABLE
    keep = px.EDGE_IN & (same | px.in_domain(seen))                # what is not fed exactly is fed as rounded where that is still in the domain
    names = [n + ("" if s else "_as_rounded") for n, s, k in zip(px.EDGE_NAMES, same, keep) if k]
    print("edges fed:", names)
    seen, feat = seen[keep], feat[keep]
    assert_net_returns_D(side, inverse, feat, seen)
    n = len(seen)
    check_layer(side, inverse, seen, feat, np.full(n, strictest("rot")), np.full(n, strictest("orth")), f"fp32, {side}, inverse {inverse}, edges")


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("side", SIDES)
def test_every_sample_split_precision(side, inverse, precision):
    """The default arithmetic and bf16x3, realistic window with |D| <= 30.  M is the fp32 oracle conditioner's output; the kernel's D carries
    the arithmetic's documented resolution (an fp16 pair holds 22 significant bits of an operand x while |x| >= 2^-3 and
    resolves 2^-25 absolutely below; the equalisation puts the hidden units of this net, whose rms is 1 by the packer's estimate, at a
    power-of-two factor in (1/4, 1/2], so D carries 2^-22 |D_ij| for |D_ij| >= 1/2 and at most 2^-23 absolutely below).  Either way an
    entry of the error E is at most 2^-22 max(1, max|D|) and max|D| <= max|M| + 1 <= s0 + 1, so |E|_2 <= 3 max|E_ij| <= 3 x 2^-22 (s0 + 1).  It turns Q by |E|_2 / (s1 + s2) = (|E|_2 / s0) kappa:
    one more term of 6 (1 + 1 / s0) units in the gate, from the format, not from the kernel.  (On an MI355X: f16x2 shows rotation figures
    up to 175 units on the samples with s0 ~ 1e-2, at most 0.37 of this gate; bf16x3 at most 2.6 units, 0.07 of it.)"""
    old = rnf.get_precision()
    rnf.set_precision(precision)
    try:
        seen, feat, yr, yo = realistic_table(dmax=30.0)
        assert_net_returns_D(side, inverse, feat, seen)
        extra = 6 * (1 + 1 / px.svals(seen)[:, 0])
        check_layer(side, inverse, seen, feat, yr, yo, f"{precision}, {side}, inverse {inverse}", extra=extra)
        assert not runtime.fallback_fired(device())
    finally:
        rnf.set_precision(old)


# ---- launch shape -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("side", SIDES)
def test_a_row_is_the_same_in_every_launch_size(fp32, side, inverse):
    """n = 1, 31, 32, 33, 65 and 4 097: row i is bit-equal whatever n it travels in, and nothing is written past row n-1 (sentinel rows
    behind both outputs, checked in run); a scale-500 matrix sits in the last (ragged) row of each size and in lanes 0 and 63 of a wave."""
    seen, feat, yr, yo = realistic_table()
    big = as_features(px.EDGE_STACK[px.EDGE_NAMES.index("identity_plus_500N")][None])[0][0]
    N = 4097
    feat = np.ascontiguousarray(np.resize(feat, (N, FD)))
    for row in (0, 30, 31, 32, 63, 64, 127, N - 1):
        feat[row] = big
    R = rotations(N, 8)
    full, lfull = run(side, inverse, R, feat)
    assert np.isfinite(full).all() and full.shape[0] == N
    for n in (1, 31, 32, 33, 65):
        part, lpart = run(side, inverse, R[:n], feat[:n])
        assert part.shape[0] == n and np.array_equal(part, full[:n]) and np.array_equal(lpart, lfull[:n]), n


# ---- out of the domain ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("side", SIDES)
def test_bad_rows_are_nan_or_rotations_and_touch_no_other_row(fp32, side, inverse):
    """A rank-1 matrix, the zero matrix and one with a NaN entry among clean ones (finite arithmetic on registers): the clean rows are
    bit-equal to the all-clean run; the singular rows are NaN throughout or orthogonal.  The NaN entry reaches the kernel as a NaN FEATURE,
    which the conditioner stage itself poisons before polar3 runs (a NaN x0 marks the sample's outputs, tests/test_gpu_guard.py): that row
    is asked to be non-finite, as every such sample is.  (On an MI355X: rank1 and zero NaN throughout, one_nan NaN in R'[0][0].)"""
    seen, feat, yr, yo = realistic_table()
    n = 1000
    feat = feat[:n].copy()
    R = rotations(n, 9)
    clean, lclean = run(side, inverse, R, feat)
    efeat, _ = as_features(px.EDGE_STACK)
    rows = {17: "rank1", 500: "one_nan", 999: "zero"}
    for r, name in rows.items():
        feat[r] = efeat[px.EDGE_NAMES.index(name)]
    got, l = run(side, inverse, R, feat)
    rest = np.array([i not in rows for i in range(n)])
    assert np.array_equal(got[rest], clean[rest]) and np.array_equal(l[rest], lclean[rest])
    for r, name in rows.items():
        print(f"{name}: {'NaN' if np.isnan(got[r]).all() else got[r]}")
        if name == "one_nan":
            assert not np.isfinite(got[r]).all(), got[r]
        else:
            assert np.isnan(got[r]).all() or px.orth_err(got[r][None])[0] <= 2 * strictest("orth") + 8 * px.U23, (name, got[r])


def test_a_nan_row_fires_the_guard_like_any_non_finite_rotation():
    """Default arithmetic, guard on.  A rotation that polar3 returns as NaN is reported as every non-finite R' is: the launch is re-run on
    the strict kernels (runtime.fallback_fired), the row stays NaN there, and every other row is finite.  The row that makes polar3 return
    NaN is M = 0 (D = -I: with the feature scale set to 1 the features 0 and 1 pass the split-precision conditioner without rounding, so the
    matrix arrives exactly singular; the flow is this test's own, so the setting touches no other test).
    The rank-1 matrix need not arrive exactly singular in this arithmetic (its D carries the format's 2^-22 rounding): it is out of the
    domain and asked to be NaN or a rotation, as everywhere.  The NaN feature row is non-finite as in test_bad_rows_are_nan_or_rotations.
    (On an MI355X: the guard fires and all three rows are NaN throughout.)"""
    old = rnf.get_precision()
    rnf.set_precision("f16x2")                                   # only the split-precision kernels are guarded
    try:
        _guard_body()
    finally:
        rnf.set_precision(old)


def _guard_body():
    seen, feat, yr, yo = realistic_table(dmax=30.0)
    n = 1000
    feat = feat[:n].copy()
    R = rotations(n, 10)
    cfg, w, _ = steering("L", False)
    fl = product_flow(cfg, w)
    fl.set_feature_scale(1.0)
    run("L", False, R, feat, fl)
    assert not runtime.fallback_fired(device())
    efeat, _ = as_features(px.EDGE_STACK)
    rows = {123: "zero", 300: "rank1", 600: "one_nan"}
    for r, name in rows.items():
        feat[r] = efeat[px.EDGE_NAMES.index(name)]
    got, l = run("L", False, R, feat, fl)
    fired = runtime.fallback_fired(device())
    for r, name in rows.items():
        print(f"guard fired {fired}; {name}: {'NaN' if np.isnan(got[r]).all() else got[r]}")
    assert fired
    rest = np.array([i not in rows for i in range(n)])
    assert np.isfinite(got[rest]).all() and np.isfinite(l[rest]).all()
    assert np.isnan(got[123]).all()
    assert np.isnan(got[300]).all() or px.orth_err(got[300][None])[0] <= 2 * strictest("orth") + 8 * px.U23, got[300]
    assert not np.isfinite(got[600]).all()
    # the zero matrix alone: polar3's NaN is what fires the guard
    run("L", False, R[:200], feat[:200], fl)
    assert runtime.fallback_fired(device())


# ---- training backward ---------------------------------------------------------------------------------------------------------------------------

DMAX_TRAIN = 3000.0            # 500 x a six-sigma normal entry: the features stay far inside the half range (65504) the activations travel in


@functools.lru_cache(maxsize=None)
def training_table(n=512):
    """(seen [n,3,3], features, per-sample LAPACK backward / rotation figure of the sample's kind): every kind, scales 10^U(-2, 2.7), no
    exact zero in D (so every entry of dL/dD is readable from one of the two feature gradients); four times as many are drawn and the first
    n / 5 of each kind that are inside the domain as the kernel sees them, with |D| <= DMAX_TRAIN, are kept (a condition on the input)."""
    per = -(-n // len(px.KINDS))
    seen, feat, yg, yr = [], [], [], []
    for kind in px.KINDS:
        f, s = as_features(px.random_batch(kind, 4 * per, 7, (-2.0, 2.7)))
        keep = px.in_domain(s) & ((s - EYE32) != 0).all((-1, -2)) & (np.abs(s - EYE32).max((-1, -2)) <= DMAX_TRAIN)
        assert keep.sum() >= per, (kind, keep.sum())
        y = yardstick(kind, "realistic")
        seen.append(s[keep][:per]); feat.append(f[keep][:per]); yg.append(np.full(per, y["grad"])); yr.append(np.full(per, y["rot"]))
    return tuple(np.concatenate(a)[:n] for a in (seen, feat, yg, yr))


def _train_pass(fl, inverse, R, feat):
    Rd = torch.from_numpy(np.ascontiguousarray(R)).cuda().requires_grad_(True)
    fd = torch.from_numpy(np.ascontiguousarray(feat)).cuda().requires_grad_(True)
    Ro, l = fl.inverse(Rd, fd) if inverse else fl(Rd, fd)
    return Rd, fd, Ro, l


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("side", SIDES)
def test_training_backward_per_sample(side, inverse):
    """.train(), default arithmetic, n = 512: cond9_backward (polar3, polar3_backward) inside the training kernels.

    dL/dM per sample is read from the feature gradient (gfeat[i] = gD[i] where D[i] > 0, gfeat[9 + i] = -gD[i] where D[i] < 0: the
    steering net's ReLUs and +-1 weights pass it unchanged, the Moebius layer does not see the features) and judged with the backward
    figure of tests/test_polar3_host.py against fp64 autograd of the oracle's layer, fed with the rotation that entered the layer on the
    device (the training forward with zero features, M = I).  Gate: 2 x the LAPACK yardstick of the sample's kind, plus what the
    arithmetic's resolution of D allows, which is not the kernel's doing: the forward's E with |E|_2 <= 3 x 2^-22 (s0 + 1)
    (test_every_sample_split_precision) moves Q twice (Q^T gQ and Q hat(z)) and T = tr(S) I - S by 2 |E|, each relative change
    |E|_2 / (s1 + s2) = (|E|_2 / s0) kappa, and max-entry against 2-norm of the result costs another factor 3:
    4 x 3 x 6 (1 + 1 / s0) units; and 4 units for the 2^-22 resolution of gD itself on its way through the net's backward.
    gR' is scaled per sample by min(1, s1 + s2), so that |gM| ~ |gR'| / (s1 + s2) stays of order one, inside the half range the backward's
    activations travel in: the overflow report must stay quiet.

    dL/dR on the tangent space, per sample, against fp64 autograd of the whole oracle flow: the Moebius layer's share at the training
    tests' REL = 2e-4 of the batch maximum (tests/test_gpu_grad.py), the 3x3 layer's share (Q^T gR', 2 x 3 products per tangent entry) at
    6 max|gR'| ((2 x LAPACK's rotation figure + the forward's format term) 2^-23 kappa + 4 x 2^-23).  fc_last.bias.grad = sum_n gD_n to
    2e-4 of its maximum.

    Measured on an MI355X (L / R, forward and inverse pass): dL/dM figure max 6.7 .. 15.4 units (LAPACK yardsticks 25 .. 125; at most 0.054
    of the gate, whose format term this batch does not use up: with features up to 2 800 the launch runs on the strict kernels),
    max |gM| 4.0 .. 4.6, fc_last.bias.grad within 1.9e-7 .. 6.6e-7 of its maximum, dL/dR tangent error at most 0.002 of its gate."""
    from tests.test_gpu_grad import REL, tangent
    seen, feat, yg, yr = training_table()
    n = len(seen)
    assert n == 512
    assert_net_returns_D(side, inverse, feat, seen)
    s = px.svals(seen)
    rng = np.random.default_rng(40 + 2 * (side == "R") + inverse)
    gR = (rng.standard_normal((n, 3, 3)) * np.minimum(1.0, s[:, 1] + s[:, 2])[:, None, None]).astype(np.float32)
    gl = rng.standard_normal(n).astype(np.float32)
    R = rotations(n, 11)
    cfg, w, i9 = steering(side, inverse)
    fl = product_flow(cfg, w).train()
    # the rotation that enters the 3x3 layer: the same training forward with M = I
    _, _, base, _ = _train_pass(fl, inverse, R, np.zeros_like(feat))
    base = base.detach().cpu().numpy().astype(np.float64)
    Rd, fd, Ro, l = _train_pass(fl, inverse, R, feat)
    ((Ro * torch.from_numpy(gR).cuda()).sum() + (l * torch.from_numpy(gl).cuda()).sum()).backward()
    torch.cuda.synchronize()
    gfeat = fd.grad.cpu().numpy().astype(np.float64)
    D = (seen - EYE32).reshape(n, 9)
    gD = np.where(D > 0, gfeat[:, :9], -gfeat[:, 9:18]).reshape(n, 3, 3)
    assert np.isfinite(Ro.detach().cpu().numpy()).all() and np.isfinite(gD).all()
    # fp64 autograd of the oracle's layer on the device's input rotation
    Mt = torch.from_numpy(seen.astype(np.float64)).requires_grad_(True)
    layer = orc.svdl9 if side == "L" else orc.svdr9
    Ro64, l64 = layer(Mt.transpose(-1, -2) if inverse else Mt, torch.from_numpy(base))
    ((Ro64 * torch.from_numpy(gR).double()).sum() + (l64 * torch.from_numpy(gl).double()).sum()).backward()
    want = Mt.grad.numpy()
    k = px.kappa(seen)
    fmt = 6 * (1 + 1 / s[:, 0])
    g = px.grad_figure(gD, want, seen)
    gate = 2 * yg + 12 * fmt + 4
    print(f"train, {side}, inverse {inverse}: dL/dM figure max {g.max():.2f}, figure / gate max {np.max(g / gate):.3f}, max |gM| {np.abs(gD).max():.2f}")
    assert (g <= gate).all(), (int(np.argmax(g / gate)), np.max(g / gate), g.max())
    # fc_last.bias.grad = sum_n gD_n
    gb = dict(fl.named_parameters())[f"layers.{i9}.net.fc_last.bias"].grad.cpu().numpy().astype(np.float64)
    wb = want.reshape(n, 9).sum(0)
    print(f"train, {side}, inverse {inverse}: fc_last.bias.grad error / max {np.abs(gb - wb).max() / np.abs(wb).max():.2e}")
    assert np.abs(gb - wb).max() <= REL * np.abs(wb).max()
    # dL/dR on the tangent space against the whole oracle flow in fp64
    p = {kk: torch.from_numpy(v).double() for kk, v in w.items()}
    Rt = torch.from_numpy(R).double().requires_grad_(True)
    fn = orc.flow_inverse if inverse else orc.flow_forward
    Rw, lw = fn(cfg, p, Rt, torch.from_numpy(feat).double(), dtype=torch.float64, grad=True)
    ((Rw * torch.from_numpy(gR).double()).sum() + (lw * torch.from_numpy(gl).double()).sum()).backward()
    tg, tw = tangent(R.astype(np.float64), Rd.grad.cpu().numpy().astype(np.float64)), tangent(R.astype(np.float64), Rt.grad.numpy())
    et = np.abs(tg - tw).max((-1, -2))
    gate_t = REL * np.abs(tw).max() + 6 * np.abs(gR).max((-1, -2)) * ((2 * yr + fmt) * px.U23 * k + 4 * px.U23)
    print(f"train, {side}, inverse {inverse}: dL/dR tangent error / gate max {np.max(et / gate_t):.3f}")
    assert np.isfinite(et).all() and (et <= gate_t).all(), (int(np.argmax(et / gate_t)), np.max(et / gate_t))
    # the half-range overflow report (one call later, tests/test_gpu_grad.py test_half_range_overflow_is_reported) stays quiet
    _train_pass(fl, inverse, R, feat)
    torch.cuda.synchronize()
    _train_pass(fl, inverse, R, feat)
    torch.cuda.synchronize()


# ---- device build against host build ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", SIDES)
def test_device_build_against_host_build(fp32, hp, side):
    """The device's polar3 (recovered from R' R^T in fp64) against the host build of the same header on the same M32: the share of rotations
    equal to within the recovery's own rounding is reported, not gated (device code contracts to FMAs, the host build does not); the
    difference is gated at the sum of both sides' error bounds."""
    seen, feat, yr, yo = realistic_table()
    R = rotations(len(seen), 3)
    out, base, _, _ = layer_alone(side, False, R, feat)
    Qd, Qh = device_Q(side, False, out, base), host_polar3(hp, seen).astype(np.float64)
    d = np.abs(Qd - Qh).max((-1, -2))
    bound = 2 * (2 * yr * px.U23 * px.kappa(seen)) + 4 * px.U23 + 3 * px.orth_err(base)
    print(f"{side}: device polar3 within 4 x 2^-23 of the host build's on {np.mean(d <= 4 * px.U23):.4f} of the batch, max difference / bound {np.max(d / bound):.3f}")
    assert (d <= bound).all(), (int(np.argmax(d / bound)), np.max(d / bound))
