"""GPU (-m gpu): the per-sample 3x3 Gram-Schmidt layers (csrc/so3_math.h smith3 and cond_gs9_apply; Condition9RotRSmith and Condition9Trans) inside the
kernels that inline them, every sample against fp64 (tests/gs3_exact.py) with the gates of tests/test_gs3_host.py: LAPACK fp32's batch maximum
on the same kind of matrix, times two.

The chosen matrices reach the layer through the steering network of tests/test_gpu_polar3.py (the net returns D = M - I with no rounding, the
Moebius layer does not see the features, the 3x3 layer is the last one applied), and the layer is isolated by a second run with zero
features, M = I:
    Smith:        smith3(I) = I and R I returns R bit for bit, so the second run IS the rotation R that entered the layer, and the first
                  must give R N (R N^T) to 2 x LAPACK's figure x 2^-23 kappa2(M) plus 4 x 2^-23 for the 3-term fp32 products.
    calculate_9:  the second run gives B = gs9(I, R), R re-normalised: R = B T with T upper triangular, 2^-23-close to I.  Gram-Schmidt of
                  M R = (M B) T is Gram-Schmidt of M B, and ldj(M R) = ldj(M B) + ldj(T) with ldj(T) the second run's own: in exact
                  arithmetic the first run is gs9_64(M, B) and its ldj less the second run's is ldj64(M, B).  What is left is B's own
                  rounding, measured on the host build (tests/test_gs3_host.py: 4 units for the rotation, 8 for ldj); it acts on R as any
                  perturbation does, so these numbers of units are ADDED to the gates' figures, for that reason and no other.  The two ldj
                  also carry the Moebius layer's ldj, summed in fp32: half an ulp of each total, 2^-24 (|ldj| + |ldj0|), not the layer's doing.
"""
import functools

import numpy as np
import pytest
import torch

import rotationnormflow_amd as rnf
from rotationnormflow_amd import runtime
from tests import gs3_exact as gx
from tests import polar3_exact as px
from tests.gpu_helpers import product_flow
from tests.test_gpu_polar3 import EYE32, FD, as_features, device, rotations, run, steering_net, training_table
from tests.test_gs3_host import (GS9_IDENTITY_LDJ_UNITS, GS9_IDENTITY_UNITS, backward_gates, layer_kappa, strictest, yardstick,
                                 yardstick_grad)
from oracle import flow_oracle as orc

pytestmark = pytest.mark.gpu

U23 = px.U23
LAYER = {"gs9": ("9TransLSmith", "cgs9"), "smith": ("9TransRSmith", "csmithr9")}      # make_config's rot, the oracle's layer kind
NAMES = ["gs9", "smith"]


def steering(name, inverse):
    return steering_net(*LAYER[name], inverse)


@functools.lru_cache(maxsize=None)
def flow_of(name, inverse):
    cfg, w, _ = steering(name, inverse)
    return product_flow(cfg, w)


def assert_net_returns_D(name, inverse, feat, seen):
    cfg, w, i9 = steering(name, inverse)
    p = {k: torch.from_numpy(v) for k, v in w.items()}
    got = orc.cond9_matrix(torch.from_numpy(feat), p, f"layers.{i9}.net").numpy()
    assert np.array_equal(got, seen, equal_nan=True)


def layer_alone(name, inverse, R, feat, fl=None):
    """(R' of the run, R' of the run with M = I, ldj of both)."""
    fl = flow_of(name, inverse) if fl is None else fl
    out, l = run(None, inverse, R, feat, fl)
    base, l0 = run(None, inverse, R, np.zeros_like(feat), fl)
    return out, base, l, l0


def want_out(name, inverse, seen, base):
    """(R', the layer's own ldj) in fp64, from the rotation the M = I run returned."""
    b = base.astype(np.float64)
    if name == "smith":
        N = gx.smith64(seen)
        return b @ (N.transpose(0, 2, 1) if inverse else N), np.zeros(len(seen))
    return gx.gs9_64(seen, b, inverse)


@functools.lru_cache(maxsize=None)
def table(name, inverse, window="realistic", per_kind=820, seed=5, lo_hi=None, dmax=None):
    """(seen [n,3,3], features, per-sample LAPACK rotation / ldj / orthogonality figures of the sample's kind).  Every kind; dmax: only
    matrices with |D| <= dmax (drawn 8 x as many and cut: a condition on the input)."""
    cols = [[] for _ in range(5)]
    for kind in px.KINDS:
        M = px.random_batch(kind, per_kind * (8 if dmax else 1), seed, lo_hi or px.WINDOWS[window])
        f, s = as_features(M)
        keep = px.in_domain(s)
        if dmax:
            keep &= np.abs(s - EYE32).max((-1, -2)) <= dmax
        assert keep.sum() >= (per_kind if dmax else 0.98 * per_kind), (kind, keep.sum())
        f, s = f[keep][:per_kind], s[keep][:per_kind]
        y = yardstick(name, inverse, kind, window)
        for c, v in zip(cols, (s, f, np.full(len(s), y["rot"]), np.full(len(s), y["ldj"]), np.full(len(s), y["orth"]))):
            c.append(v)
    return tuple(np.concatenate(c) for c in cols)


def check_layer(name, inverse, seen, feat, yr, yl, yo, what, extra=0.0, fl=None):
    """Every sample: R' and the layer's ldj against fp64 within the gates, R' orthogonal."""
    n = len(seen)
    R = rotations(n, 3)
    out, base, l, l0 = layer_alone(name, inverse, R, feat, fl)
    k = layer_kappa(name, seen)
    want, want_l = want_out(name, inverse, seen, base)
    moved = GS9_IDENTITY_UNITS if name == "gs9" else 0
    gate = (2 * yr + extra + moved) * U23 * k + 4 * U23
    err = np.abs(out - want).max((-1, -2))
    o = px.orth_err(out)
    print(f"{what}: max error / gate {np.max(err / gate):.3f}, rotation figure max {np.max(err / (U23 * k)):.2f}, |R'R'^T - I| max {o.max() / U23:.2f} units "
          f"(input rotations {px.orth_err(base).max() / U23:.2f})")
    assert np.isfinite(out).all() and (err <= gate).all(), (what, int(np.argmax(err / gate)), np.max(err / gate))
    if name == "smith":                                                # R' = R N: as orthogonal as R and N are, and three products
        assert (o <= 2 * yo + px.orth_err(base) + 4 * U23).all(), (what, o.max() / U23)
        assert np.array_equal(l, l0), what                             # ldj exactly 0 from the layer
    else:                                                              # R' is the layer's own Gram-Schmidt factor
        assert (o <= 2 * yo).all(), (what, o.max() / U23)
        el = np.abs(l.astype(np.float64) - l0 - want_l)
        gate_l = (2 * yl + extra + GS9_IDENTITY_LDJ_UNITS) * U23 * k + 2.0 ** -24 * (np.abs(l) + np.abs(l0))
        print(f"{what}: ldj error / gate max {np.max(el / gate_l):.3f}, ldj figure max {np.max(el / (U23 * k)):.2f}")
        assert np.isfinite(l).all() and (el <= gate_l).all(), (what, int(np.argmax(el / gate_l)), np.max(el / gate_l))
    assert (np.linalg.det(out.astype(np.float64)) > 0.5).all()
    return out, base


@pytest.fixture
def fp32():
    old = rnf.get_precision()
    rnf.set_precision("fp32")
    yield
    rnf.set_precision(old)


# ---- forward and inverse, both layers, per sample ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_every_sample_fp32(fp32, name, inverse):
    """Under set_precision("fp32") the matrix arrives exactly at any scale: every kind at realistic scales 10^U(-2,3) (4 100 samples), and
    the `range` window as far as fp32 features carry it, 10^U(0,12), 2 000 samples (below 1 the sum I + D keeps the identity's digits, not
    M's; the hollow edges cover small matrices)."""
    seen, feat, yr, yl, yo = table(name, inverse)
    assert_net_returns_D(name, inverse, feat, seen)
    check_layer(name, inverse, seen, feat, yr, yl, yo, f"fp32, {name}, inverse {inverse}, realistic")
    seen, feat, yr, yl, yo = table(name, inverse, "range", 400, 6, (0.0, 12.0))
    assert_net_returns_D(name, inverse, feat, seen)
    check_layer(name, inverse, seen, feat, yr, yl, yo, f"fp32, {name}, inverse {inverse}, scales up to 1e12")


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_in_domain_edges_fp32(fp32, name, inverse):
    """The named edges as tests/test_gpu_polar3.py feeds them: exactly where I + (M - I) keeps them, as rounded where that is still inside the
    domain."""
    feat, seen = as_features(px.EDGE_STACK)
    same = np.array([np.array_equal(a, b) for a, b in zip(seen, px.EDGE_STACK)])
    keep = px.EDGE_IN & (same | px.in_domain(seen))
    print("edges fed:", [n + ("" if s else "_as_rounded") for n, s, k in zip(px.EDGE_NAMES, same, keep) if k])
    seen, feat = seen[keep], feat[keep]
    assert_net_returns_D(name, inverse, feat, seen)
    n = len(seen)
    gates = [np.full(n, strictest(name, inverse, key)) for key in ("rot", "ldj", "orth")]
    check_layer(name, inverse, seen, feat, *gates, f"fp32, {name}, inverse {inverse}, edges")


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_every_sample_split_precision(name, inverse, precision):
    """The default arithmetic and bf16x3, realistic window with |D| <= 30, with the format allowance tests/test_gpu_polar3.py documents and no
    wider: the kernel's D carries an error E with max|E_ij| <= 2^-22 max(1, max|D|) <= 2^-22 (s0(M) + 1), |E|_2 <= 3 max|E_ij|, which is not
    the kernel's doing.  It turns a Gram-Schmidt factor of A by |E|_2 / s_min(A) = (|E|_2 / s0(A)) kappa: 6 (s0(M) + 1) / s0(A) more units in
    the figures' gates, with A the matrix that is factored (M for calculate_9, where this is polar3's 6 (1 + 1 / s0); M[:, :2] for Smith)."""
    old = rnf.get_precision()
    rnf.set_precision(precision)
    try:
        seen, feat, yr, yl, yo = table(name, inverse, dmax=30.0)
        assert_net_returns_D(name, inverse, feat, seen)
        A = seen.astype(np.float64)
        s0 = np.linalg.svd(A, compute_uv=False)[:, 0]
        s0A = np.linalg.svd(A[:, :, :2], compute_uv=False)[:, 0] if name == "smith" else s0
        check_layer(name, inverse, seen, feat, yr, yl, yo, f"{precision}, {name}, inverse {inverse}", extra=6 * (s0 + 1) / s0A)
        assert not runtime.fallback_fired(device())
    finally:
        rnf.set_precision(old)


# ---- launch shape -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_a_row_is_the_same_in_every_launch_size(fp32, name, inverse):
    """n = 1, 63, 64, 65, 257 and 4 097: row i is bit-equal whatever n it travels in, and nothing is written past row n-1 (sentinel rows
    behind both outputs, checked in run); a scale-500 matrix sits in the last (ragged) row of each size and in lanes 0 and 63 of a wave."""
    seen, feat, yr, yl, yo = table(name, inverse)
    big = as_features(px.EDGE_STACK[px.EDGE_NAMES.index("identity_plus_500N")][None])[0][0]
    N = 4097
    feat = np.ascontiguousarray(np.resize(feat, (N, FD)))
    for row in (0, 62, 63, 64, 127, 256, N - 1):
        feat[row] = big
    R = rotations(N, 8)
    fl = flow_of(name, inverse)
    full, lfull = run(None, inverse, R, feat, fl)
    assert np.isfinite(full).all() and np.isfinite(lfull).all() and full.shape[0] == N
    for n in (1, 63, 64, 65, 257):
        part, lpart = run(None, inverse, R[:n], feat[:n], fl)
        assert part.shape[0] == n and np.array_equal(part, full[:n]) and np.array_equal(lpart, lfull[:n]), n


# ---- out of the domain ------------------------------------------------------------------------------------------------------------------------

def bad_features():
    """Feature rows of matrices the layers must refuse: rank 1 and zero (EDGE_M), and I + 0.2 N with a NaN / an infinite entry in its FIRST
    column (Smith does not read the third, where EDGE_M's one_nan has it)."""
    efeat, _ = as_features(px.EDGE_STACK)
    base = px.EDGE_STACK[px.EDGE_NAMES.index("pow2_40")].astype(np.float64) * 2.0 ** -40
    nan, inf = base.copy(), base.copy()
    nan[1, 0] = np.nan
    inf[2, 0] = np.inf
    return {"rank1": efeat[px.EDGE_NAMES.index("rank1")], "zero": efeat[px.EDGE_NAMES.index("zero")],
            "nan_in_column_0": as_features(nan[None])[0][0], "inf_in_column_0": as_features(inf[None])[0][0]}


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_bad_rows_are_nan_and_touch_no_other_row(fp32, name, inverse):
    """Rank-1, zero, NaN and infinite matrices among clean ones, exact arithmetic on the way in: the clean rows are bit-equal to the all-clean
    run, the bad rows are not finite (R' NaN throughout for the singular matrices, which only the layer itself can notice; ldj not finite
    beside it for calculate_9)."""
    seen, feat, yr, yl, yo = table(name, inverse)
    n = 1000
    feat = feat[:n].copy()
    R = rotations(n, 9)
    fl = flow_of(name, inverse)
    clean, lclean = run(None, inverse, R, feat, fl)
    assert np.isfinite(clean).all() and np.isfinite(lclean).all()
    rows = dict(zip((17, 500, 63, 999), bad_features().items()))
    for r, (_, f) in rows.items():
        feat[r] = f
    got, l = run(None, inverse, R, feat, fl)
    rest = np.array([i not in rows for i in range(n)])
    assert np.array_equal(got[rest], clean[rest]) and np.array_equal(l[rest], lclean[rest])
    for r, (what, _) in rows.items():
        print(f"{name}, inverse {inverse}, {what}: {'NaN' if np.isnan(got[r]).all() else got[r]}, ldj {l[r]}")
        assert not np.isfinite(got[r]).any() if what in ("rank1", "zero") else not np.isfinite(got[r]).all(), (what, got[r])
        if what in ("rank1", "zero"):
            assert np.isnan(got[r]).all(), (what, got[r])
            assert name == "smith" or not np.isfinite(l[r]), (what, l[r])


@pytest.mark.parametrize("name", NAMES)
def test_a_nan_row_fires_the_guard_like_any_non_finite_rotation(name):
    """Default arithmetic, guard on, as tests/test_gpu_polar3.py: a rotation the layer returns as NaN is reported as every non-finite R' is
    (runtime.fallback_fired), the row stays NaN on the strict kernels, and every other row is finite.  With the feature scale set to 1 the
    zero matrix (D = -I) and the rank-1 matrix (D of a few dyadic digits, |D| <= 4) pass the split-precision conditioner without rounding."""
    old = rnf.get_precision()
    rnf.set_precision("f16x2")                                   # only the split-precision kernels are guarded
    try:
        seen, feat, yr, yl, yo = table(name, False, dmax=30.0)
        n = 1000
        feat = feat[:n].copy()
        R = rotations(n, 10)
        cfg, w, _ = steering(name, False)
        fl = product_flow(cfg, w)
        fl.set_feature_scale(1.0)
        run(None, False, R, feat, fl)
        assert not runtime.fallback_fired(device())
        rows = dict(zip((123, 300, 600, 777), bad_features().items()))
        for r, (_, f) in rows.items():
            feat[r] = f
        got, l = run(None, False, R, feat, fl)
        fired = runtime.fallback_fired(device())
        for r, (what, _) in rows.items():
            print(f"{name}: guard fired {fired}; {what}: {'NaN' if np.isnan(got[r]).all() else got[r]}")
        assert fired
        rest = np.array([i not in rows for i in range(n)])
        assert np.isfinite(got[rest]).all() and np.isfinite(l[rest]).all()
        for r, (what, _) in rows.items():
            assert not np.isfinite(got[r]).all(), what
        # the singular matrices alone, one at a time: the layer's own NaN is what fires the guard
        for r in (123, 300):
            one = feat[:200].copy()
            one[5] = feat[r]
            got, _ = run(None, False, R[:200], one, fl)
            assert np.isnan(got[5]).all() and runtime.fallback_fired(device()), rows[r][0]
    finally:
        rnf.set_precision(old)


# ---- training backward ---------------------------------------------------------------------------------------------------------------------------

def _train_pass(fl, inverse, R, feat):
    Rd = torch.from_numpy(np.ascontiguousarray(R)).cuda().requires_grad_(True)
    fd = torch.from_numpy(np.ascontiguousarray(feat)).cuda().requires_grad_(True)
    Ro, l = fl.inverse(Rd, fd) if inverse else fl(Rd, fd)
    return Rd, fd, Ro, l


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_training_backward_per_sample(name, inverse):
    """.train(), default arithmetic, n = 512, scales 10^U(-2, 2.7): cond9_backward for RNF_KIND_COND9_GS / _SMITH inside the training kernels.

    dL/dM per sample is read from the feature gradient as tests/test_gpu_polar3.py reads it and judged against fp64 autograd of the
    oracle's layer, fed with the rotation the training forward returns for M = I (zero features; for calculate_9 that is the re-normalised
    input, which gives the same R' and an ldj that differs by a term without M: see the module docstring).  Gate per sample: the host test's
    (backward_gates: 2 x the LAPACK yardstick of the sample's kind, plus 4 x 2^-23 of the fp32 products), plus, in the figure, what is not the
    kernel's doing: GS9_IDENTITY_UNITS for the rounding of the M = I run (calculate_9), 4 units for the 2^-22 resolution of gD on its way
    through the net's backward, and 4 x 3 x the forward's format term 6 (s0(M) + 1) / s0(A) (test_every_sample_split_precision): the
    arithmetic's error E of D moves the two divisors |x0|, |b1| and, twice, the factor Q, each by (|E|_2 / s0) kappa relatively, and
    max-entry against 2-norm costs a factor 3 (the count of tests/test_gpu_polar3.py).
    The cotangents are scaled per sample by min(1, s_min / cond^inverse) so that |dL/dM| ~ |cotangent| cond^inverse / s_min stays of order
    one, inside the half range the backward's activations travel in.  fc_last.bias.grad = sum_n gD_n to the training tests' REL = 2e-4 of
    its maximum against the fp64 sum."""
    from tests.test_gpu_grad import REL
    seen, feat, _, _ = training_table()
    n = len(seen)
    assert n == 512
    per = -(-n // len(px.KINDS))
    kind_of = np.repeat(np.arange(len(px.KINDS)), per)[:n]
    assert_net_returns_D(name, inverse, feat, seen)
    A = seen.astype(np.float64)
    s = np.linalg.svd(A, compute_uv=False)
    sA = np.linalg.svd(A[:, :, :2], compute_uv=False) if name == "smith" else s
    k = layer_kappa(name, seen)
    rng = np.random.default_rng(50 + 2 * (name == "smith") + inverse)
    damp = np.minimum(1.0, sA[:, -1] / (k if name == "gs9" and inverse else 1.0))
    gR = (rng.standard_normal((n, 3, 3)) * damp[:, None, None]).astype(np.float32)
    gl = (rng.standard_normal(n) * damp).astype(np.float32)
    R = rotations(n, 11)
    cfg, w, i9 = steering(name, inverse)
    fl = product_flow(cfg, w).train()
    _, _, base, _ = _train_pass(fl, inverse, R, np.zeros_like(feat))          # the rotation that enters the 3x3 layer (re-normalised by calculate_9)
    base = base.detach().cpu().numpy()
    Rd, fd, Ro, l = _train_pass(fl, inverse, R, feat)
    ((Ro * torch.from_numpy(gR).cuda()).sum() + (l * torch.from_numpy(gl).cuda()).sum()).backward()
    torch.cuda.synchronize()
    gfeat = fd.grad.cpu().numpy().astype(np.float64)
    D = (seen - EYE32).reshape(n, 9)
    gD = np.where(D > 0, gfeat[:, :9], -gfeat[:, 9:18]).reshape(n, 3, 3)
    assert np.isfinite(Ro.detach().cpu().numpy()).all() and np.isfinite(gD).all()
    want, want_R = gx.layer_grad64(name, seen, base, gR, gl, inverse)
    yg = np.array([yardstick_grad(name, inverse, kd, "realistic")["grad"] for kd in px.KINDS])[kind_of]
    gate, _ = backward_gates(name, inverse, seen, gR, gl, want, want_R, base, yg, 0.0)
    fmt = 6 * (s[:, 0] + 1) / sA[:, 0]
    gate = gate + (12 * fmt + 4 + (GS9_IDENTITY_UNITS if name == "gs9" else 0)) * U23 * k * gx._maxabs(want)
    err = gx._maxabs(gD - want)
    print(f"train, {name}, inverse {inverse}: dL/dM figure max {gx.grad_figure(gD, want, k).max():.2f}, error / gate max {np.max(err / gate):.3f}, "
          f"max |gM| {np.abs(gD).max():.2f}")
    assert (err <= gate).all(), (int(np.argmax(err / gate)), np.max(err / gate))
    gb = dict(fl.named_parameters())[f"layers.{i9}.net.fc_last.bias"].grad.cpu().numpy().astype(np.float64)
    wb = want.reshape(n, 9).sum(0)
    print(f"train, {name}, inverse {inverse}: fc_last.bias.grad error / max {np.abs(gb - wb).max() / np.abs(wb).max():.2e}")
    assert np.abs(gb - wb).max() <= REL * np.abs(wb).max()
