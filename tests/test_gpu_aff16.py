"""GPU (-m gpu): the per-sample 4x4 layer Condition16Trans (csrc/so3_math.h cond16_apply, csrc/so3_grad.h cond16_backward) inside the kernels that
inline it, every sample against fp64 (tests/aff16_exact.py) with the gates of tests/test_aff16_host.py: LAPACK fp32's batch maximum on the
same kind of matrix, times two.

The chosen matrices reach the layer through a STEERING NETWORK (the idea of tests/test_gpu_polar3.py, for sixteen outputs): on the 4x4
layer's net every hidden layer is zero, fc_first copies feature i into hidden unit i (i < 32) and fc_last row i takes unit i minus unit
16 + i.  With D = M - I and the features [max(D, 0), max(-D, 0), 0 ...] the net returns D with no rounding (asserted on the CPU against
the fp32 oracle), and the kernel sees M32 = fl(I + D).  The Moebius layer of the flow does not see the features, and the 4x4 layer is the
LAST layer applied (forward: [mobius, cond16]; inverse pass: the flow [cond16, mobius] run backwards).

The layer is isolated by a second run with zero features, M = I.  It returns B = rot(quat(R)), the re-normalised input, and
l0 = (the Moebius layer's ldj) - 4 log|quat(R)|.  In exact arithmetic quat(B) = quat(R) / |quat(R)|, so the first run is the fp64 layer at
(M, B) and its ldj less l0 is that layer's ldj.  What is left is B's own rounding, measured on the host build (tests/test_aff16_host.py:
AFF16_IDENTITY_UNITS for the rotation, AFF16_IDENTITY_LDJ_UNITS for ldj); it acts on R as any perturbation does, so these numbers of units
are ADDED to the gates' figures, for that reason and no other.  The two ldj also carry the Moebius layer's ldj, summed in fp32: half an
ulp of each total, 2^-24 (|ldj| + |ldj0|), not the layer's doing.

Measured on an MI355X: see the docstrings of the tests and DESIGN.md section 3.7c.
"""
import functools

import numpy as np
import pytest
import torch

import rotationnormflow_amd as rnf
from oracle import flow_oracle as orc
from rotationnormflow_amd import make_config, runtime, synth
from tests import aff16_exact as ax
from tests.gpu_helpers import product_flow
from tests.test_aff16_host import (AFF16_IDENTITY_LDJ_UNITS, AFF16_IDENTITY_UNITS, backward_gates, cond16 as host_cond16, forward_gates,
                                   ha, strictest, yardstick, yardstick_grad)  # noqa: F401  (ha: the host build, a fixture)
from tests.test_gpu_polar3 import device, rotations, run

pytestmark = pytest.mark.gpu

U23 = ax.U23
EYE32 = np.eye(4, dtype=np.float32)
FD = 40
PASSES = [False, True]


def as_features(M):
    """(features [n,40] fp32, the matrix the kernel sees [n,4,4] fp32 = fl(I + D), D = fl(M - I) formed in fp64 and rounded once)."""
    M = np.asarray(M).reshape(-1, 4, 4)
    with np.errstate(invalid="ignore"):
        D = (M.astype(np.float64) - np.eye(4)).astype(np.float32).reshape(-1, 16)
    feat = np.zeros((len(D), FD), np.float32)
    with np.errstate(invalid="ignore"):
        feat[:, :16] = np.where(D > 0, D, 0)
        feat[:, 16:32] = np.where(D < 0, -D, 0)
    bad = ~np.isfinite(D)
    feat[:, :16][bad] = D[bad]                                 # a NaN / inf entry travels as itself
    return feat, D.reshape(-1, 4, 4) + EYE32


@functools.lru_cache(maxsize=None)
def steering(inverse):
    """(cfg, weights, index of the 4x4 layer).  inverse: the flow whose INVERSE pass applies the 4x4 layer last."""
    extra = dict(last_affine=1, first_affine=0) if inverse else {}
    cfg = make_config(layers=1, segments=16, condition=1, feature_dim=FD, rot="16Trans", **extra)
    assert orc.layer_kinds(cfg) == (["cond16", "mobius"] if inverse else ["mobius", "cond16"])
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=33, regime="trained")
    i16, im = (0, 1) if inverse else (1, 0)
    pre = f"layers.{i16}.net"
    for k in w:
        if k.startswith(pre + "."):
            w[k] = np.zeros_like(w[k])
    for i in range(32):
        w[f"{pre}.fc_first.weight"][i, i] = 1.0
    for i in range(16):
        w[f"{pre}.fc_last.weight"][i, i] = 1.0
        w[f"{pre}.fc_last.weight"][i, 16 + i] = -1.0
    w[f"layers.{im}.conditioner.fc_first.weight"][:, 3:] = 0.0             # the Moebius layer does not see the features
    return cfg, w, i16


@functools.lru_cache(maxsize=None)
def flow_of(inverse):
    cfg, w, _ = steering(inverse)
    return product_flow(cfg, w)


def assert_net_returns_D(inverse, feat, seen):
    cfg, w, i16 = steering(inverse)
    p = {k: torch.from_numpy(v) for k, v in w.items()}
    got = orc.cond16_matrix(torch.from_numpy(feat), p, f"layers.{i16}.net").numpy()
    assert np.array_equal(got, seen, equal_nan=True)


def layer_alone(inverse, R, feat, fl=None):
    """(R' of the run, R' of the run with M = I, ldj of both)."""
    fl = flow_of(inverse) if fl is None else fl
    out, l = run(None, inverse, R, feat, fl)
    base, l0 = run(None, inverse, R, np.zeros_like(feat), fl)
    return out, base, l, l0


@functools.lru_cache(maxsize=None)
def table(inverse, window="realistic", per_kind=820, seed=5, lo_hi=None, dmax=None):
    """(seen [n,4,4], features, per-sample LAPACK rotation / ldj / orthogonality figures of the sample's kind).  Every kind; dmax: only
    matrices with |D| <= dmax (drawn 8 x as many and cut: a condition on the input)."""
    cols = [[] for _ in range(5)]
    for kind in ax.KINDS:
        M, _ = ax.random_batch(kind, per_kind * (8 if dmax else 1), seed, lo_hi or ax.WINDOWS[window])
        f, s = as_features(M)
        keep = ax.in_domain(s)
        if dmax:
            keep &= np.abs(s - EYE32).max((-1, -2)) <= dmax
        assert keep.sum() >= (per_kind if dmax else 0.98 * per_kind), (kind, keep.sum())
        f, s = f[keep][:per_kind], s[keep][:per_kind]
        y = yardstick(inverse, kind, window)
        for c, v in zip(cols, (s, f, np.full(len(s), y["rot"]), np.full(len(s), y["ldj"]), np.full(len(s), y["orth"]))):
            c.append(v)
    return tuple(np.concatenate(c) for c in cols)


def check_layer(inverse, seen, feat, yr, yl, yo, what, extra=0.0, fl=None):
    """Every sample: R' and the layer's ldj against fp64 within the gates, R' orthogonal.  extra: the format's units for the rotation
    figure (eight times as many for ldj, test_every_sample_split_precision)."""
    n = len(seen)
    R = rotations(n, 3)
    out, base, l, l0 = layer_alone(inverse, R, feat, fl)
    k = ax.cond(seen)
    want, want_l = ax.layer64(seen, base, inverse)
    gate, gate_l = forward_gates(yr + 0.5 * (extra + AFF16_IDENTITY_UNITS), yl + 0.5 * (8 * extra + AFF16_IDENTITY_LDJ_UNITS), k,
                                 ax.log_terms(seen, base, inverse))
    gate_l = gate_l + 2.0 ** -24 * (np.abs(l) + np.abs(l0))
    err, o = ax.rot_error(out, want), ax.orth_err(out)
    el = np.abs(l.astype(np.float64) - l0 - want_l)
    used = np.max((err - 4 * U23) / (U23 * k) - 2 * yr - AFF16_IDENTITY_UNITS) if np.ndim(extra) else 0.0
    print(f"{what}: max error / gate {np.max(err / gate):.3f}, rotation figure max {np.max(err / (U23 * k)):.2f}, |R'R'^T - I| max {o.max() / U23:.2f} units; "
          f"ldj error / gate max {np.max(el / gate_l):.3f}, ldj figure max {np.max(el / (U23 * k)):.2f}"
          + (f"; of the format term's units at most {max(used, 0.0):.2f} are used (the term: {np.min(extra):.1f} .. {np.max(extra):.1f})" if np.ndim(extra) else ""))
    assert np.isfinite(out).all() and (err <= gate).all(), (what, int(np.argmax(err / gate)), np.max(err / gate))
    assert np.isfinite(l).all() and (el <= gate_l).all(), (what, int(np.argmax(el / gate_l)), np.max(el / gate_l))
    assert (o <= 2 * yo).all(), (what, o.max() / U23)
    assert (np.linalg.det(out.astype(np.float64)) > 0.5).all()
    return out, base


@pytest.fixture
def fp32():
    old = rnf.get_precision()
    rnf.set_precision("fp32")
    yield
    rnf.set_precision(old)


# ---- forward and inverse, per sample ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", PASSES)
def test_every_sample_fp32(fp32, inverse):
    """Under set_precision("fp32") the matrix arrives exactly at any scale: every kind at realistic scales 10^U(-2,3) (4 100 samples), and
    the `range` window as far as fp32 features carry it, 10^U(0,12), 2 000 samples (below 1 the sum I + D keeps the identity's digits, not
    M's).  Measured on an MI355X: rotation figure at most 5.52, ldj figure at most 18.98, |R'R'^T - I| at most 4.95 units; at most 0.40 of
    the rotation gate and 0.37 of the ldj gate."""
    seen, feat, yr, yl, yo = table(inverse)
    assert_net_returns_D(inverse, feat, seen)
    check_layer(inverse, seen, feat, yr, yl, yo, f"fp32, inverse {inverse}, realistic")
    seen, feat, yr, yl, yo = table(inverse, "range", 400, 6, (0.0, 12.0))
    assert_net_returns_D(inverse, feat, seen)
    check_layer(inverse, seen, feat, yr, yl, yo, f"fp32, inverse {inverse}, scales up to 1e12")


@pytest.mark.parametrize("inverse", PASSES)
def test_in_domain_edges_fp32(fp32, inverse):
    """The named edges: exactly where I + (M - I) keeps them, as rounded where that is still inside the domain (the 4-D rotation, the
    reflection and the cond-1e3 matrices lose their last bits against the identity; 2^-40 and 2^-60 times a matrix lose their diagonal
    altogether and are not fed)."""
    feat, seen = as_features(ax.EDGE_STACK)
    same = np.array([np.array_equal(a, b) for a, b in zip(seen, ax.EDGE_STACK)])
    keep = ax.EDGE_IN & (same | ax.in_domain(seen))
    names = [n + ("" if s else "_as_rounded") for n, s, k in zip(ax.EDGE_NAMES, same, keep) if k]
    print("edges fed:", names)
    assert {"identity", "identity_plus_500N", "pow2_40", "pow2_60"} <= set(names) and len(names) >= 9
    seen, feat = seen[keep], feat[keep]
    assert_net_returns_D(inverse, feat, seen)
    gates = [np.full(len(seen), strictest(inverse, key)) for key in ("rot", "ldj", "orth")]
    check_layer(inverse, seen, feat, *gates, f"fp32, inverse {inverse}, edges")


def format_units(seen):
    """The split formats' resolution of D, in units of the rotation figure.  The kernel's D carries an error E with
    max|E_ij| <= 2^-22 max(1, max|D|) <= 2^-22 (s0(M) + 1) (tests/test_gpu_polar3.py test_every_sample_split_precision), which
    is not the kernel's doing, and |E|_2 <= 4 max|E_ij| for a 4x4.  It turns t / |t| by |E|_2 / s_min(M) = (|E|_2 / s0) kappa in either pass:
    8 (1 + 1 / s0) units of 2^-23 kappa.  ldj moves by |tr(M^-1 E)| + 4 |E|_2 / s_min <= 8 |E|_2 / s_min: eight times as many units."""
    return 8 * (1 + 1 / ax.svals(seen)[:, 0])


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("inverse", PASSES)
def test_every_sample_split_precision(inverse, precision):
    """The default arithmetic and bf16x3, realistic window with |D| <= 30, with the format allowance of format_units and no wider.
    Measured on an MI355X: f16x2 shows rotation figures up to 209 and ldj figures up to 403 on the samples with s0 ~ 1e-2 and uses at
    most 195 of the term's 8 .. 808 units (0.37 of the gate); bf16x3 at most 5.16 and 11.46 and none of the term."""
    old = rnf.get_precision()
    rnf.set_precision(precision)
    try:
        seen, feat, yr, yl, yo = table(inverse, dmax=30.0)
        assert_net_returns_D(inverse, feat, seen)
        check_layer(inverse, seen, feat, yr, yl, yo, f"{precision}, inverse {inverse}", extra=format_units(seen))
        assert not runtime.fallback_fired(device())
    finally:
        rnf.set_precision(old)


# ---- launch shape ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", PASSES)
def test_a_row_is_the_same_in_every_launch_size(fp32, inverse):
    """n = 1, 31, 32, 33, 65, 255, 256, 257 and 4 097 (cond16_finish pairs lanes j and j + 32, a tile is 256 rotations): row i is bit-equal
    whatever n it travels in, and nothing is written past row n-1 (sentinel rows behind both outputs, checked in run); a scale-500 matrix
    sits in lanes 0, 31, 32 and 63 of a wave and in the last (ragged) row of each size."""
    seen, feat, yr, yl, yo = table(inverse)
    big = as_features(ax.EDGE_STACK[ax.EDGE_NAMES.index("identity_plus_500N")][None])[0][0]
    N = 4097
    feat = np.ascontiguousarray(np.resize(feat, (N, FD)))
    for row in (0, 30, 31, 32, 63, 64, 254, 255, 256, N - 1):
        feat[row] = big
    R = rotations(N, 8)
    fl = flow_of(inverse)
    full, lfull = run(None, inverse, R, feat, fl)
    assert np.isfinite(full).all() and np.isfinite(lfull).all() and full.shape[0] == N
    for n in (1, 31, 32, 33, 65, 255, 256, 257):
        part, lpart = run(None, inverse, R[:n], feat[:n], fl)
        assert part.shape[0] == n and np.array_equal(part, full[:n]) and np.array_equal(lpart, lfull[:n]), n


# ---- out of the domain -----------------------------------------------------------------------------------------------------------------------

def bad_rows():
    efeat, _ = as_features(ax.EDGE_STACK)
    return {name: efeat[ax.EDGE_NAMES.index(name)] for name in ("rank1", "zero", "one_nan")}


def nan_or_rotation(Ro, l):
    """R' all NaN with a non-finite ldj, or a rotation to the host test's 16 units."""
    if np.isfinite(Ro).all():
        return ax.orth_err(Ro[None])[0] <= 16 * U23
    return bool(np.isnan(Ro).all()) and not np.isfinite(l)


@pytest.mark.parametrize("inverse", PASSES)
def test_bad_rows_touch_no_other_row(fp32, inverse):
    """A rank-1 matrix, the zero matrix and one with a NaN entry among clean ones, exact arithmetic on the way in: the clean rows are
    bit-equal to the all-clean run; the bad rows are NaN throughout with a non-finite ldj, or rotations (tests/test_aff16_host.py: no finite
    wrong answer).  The zero matrix is NaN in both passes (M q = 0; a zero pivot).  The NaN entry reaches the kernel as a NaN FEATURE,
    which the conditioner stage itself poisons: that row is asked to be non-finite, as every such sample is."""
    seen, feat, yr, yl, yo = table(inverse)
    n = 1000
    feat = feat[:n].copy()
    R = rotations(n, 9)
    fl = flow_of(inverse)
    clean, lclean = run(None, inverse, R, feat, fl)
    assert np.isfinite(clean).all() and np.isfinite(lclean).all()
    rows = dict(zip((17, 500, 999), bad_rows().items()))
    for r, (_, f) in rows.items():
        feat[r] = f
    got, l = run(None, inverse, R, feat, fl)
    rest = np.array([i not in rows for i in range(n)])
    assert np.array_equal(got[rest], clean[rest]) and np.array_equal(l[rest], lclean[rest])
    for r, (what, _) in rows.items():
        print(f"inverse {inverse}, {what}: {'NaN' if np.isnan(got[r]).all() else got[r]}, ldj {l[r]}")
        if what == "one_nan":
            assert not np.isfinite(got[r]).all(), got[r]
        else:
            assert nan_or_rotation(got[r], l[r]), (what, got[r], l[r])
        if what == "zero":
            assert np.isnan(got[r]).all() and not np.isfinite(l[r])


def test_the_zero_matrix_fires_the_guard_on_the_inverse_pass():
    """Default arithmetic, guard on, inverse pass: M = 0 (D = -I; with the feature scale set to 1 the features 0 and 1 pass the
    split-precision conditioner without rounding, so the matrix arrives exactly singular) has no inverse.  The layer returns NaN, which is
    reported as every non-finite R' is (runtime.fallback_fired); every other row stays finite."""
    old = rnf.get_precision()
    rnf.set_precision("f16x2")                                   # only the split-precision kernels are guarded
    try:
        seen, feat, yr, yl, yo = table(True, dmax=30.0)
        n = 1000
        feat = feat[:n].copy()
        R = rotations(n, 10)
        cfg, w, _ = steering(True)
        fl = product_flow(cfg, w)
        fl.set_feature_scale(1.0)
        run(None, True, R, feat, fl)
        assert not runtime.fallback_fired(device())
        feat[123] = bad_rows()["zero"]
        got, l = run(None, True, R, feat, fl)
        fired = runtime.fallback_fired(device())
        print(f"guard fired {fired}; zero: {'NaN' if np.isnan(got[123]).all() else got[123]}, ldj {l[123]}")
        assert fired
        rest = np.arange(n) != 123
        assert np.isfinite(got[rest]).all() and np.isfinite(l[rest]).all()
        assert np.isnan(got[123]).all() and not np.isfinite(l[123])
    finally:
        rnf.set_precision(old)


# ---- training backward -------------------------------------------------------------------------------------------------------------------------

DMAX_TRAIN = 3000.0            # 500 x a six-sigma normal entry: the features stay far inside the half range (65504) the activations travel in


@functools.lru_cache(maxsize=None)
def training_table(n):
    """(seen [n,4,4], features, kind index): every kind, scales 10^U(-2, 2.7), no exact zero in D (so every entry of dL/dD is readable
    from one of the two feature gradients); four times as many are drawn and the first n / 5 of each kind that are inside the domain as the
    kernel sees them, with |D| <= DMAX_TRAIN, are kept (a condition on the input)."""
    per = -(-n // len(ax.KINDS))
    seen, feat = [], []
    for kind in ax.KINDS:
        f, s = as_features(ax.random_batch(kind, 4 * per, 7, (-2.0, 2.7))[0])
        keep = ax.in_domain(s) & ((s - EYE32) != 0).all((-1, -2)) & (np.abs(s - EYE32).max((-1, -2)) <= DMAX_TRAIN)
        assert keep.sum() >= per, (kind, keep.sum())
        seen.append(s[keep][:per]); feat.append(f[keep][:per])
    return np.concatenate(seen)[:n], np.concatenate(feat)[:n], np.repeat(np.arange(len(ax.KINDS)), per)[:n]


def _train_pass(fl, inverse, R, feat):
    Rd = torch.from_numpy(np.ascontiguousarray(R)).cuda().requires_grad_(True)
    fd = torch.from_numpy(np.ascontiguousarray(feat)).cuda().requires_grad_(True)
    Ro, l = fl.inverse(Rd, fd) if inverse else fl(Rd, fd)
    return Rd, fd, Ro, l


@pytest.mark.parametrize("n", [512, 6400])
@pytest.mark.parametrize("inverse", PASSES)
def test_training_backward_per_sample(inverse, n):
    """.train(), default arithmetic: cond16_backward inside the training kernels, n = 512 (train_block16.h) and n = 6 400 (train_kernels.h;
    the sweep switches at 6 144 rotations, so both are selected by size).

    dL/dM per sample is read from the feature gradient (gfeat[i] = gD[i] where D[i] > 0, gfeat[16 + i] = -gD[i] where D[i] < 0: the
    steering net's ReLUs and +-1 weights pass it unchanged, the Moebius layer does not see the features) and judged against fp64 autograd
    of the fp64 layer, fed with the rotation the training forward returns for M = I (zero features: the re-normalised input, which gives
    the same R' and an ldj that differs by a term without M: see the module docstring).  Gate per sample: the host test's (backward_gates:
    2 x the LAPACK yardstick of the sample's kind, plus 4 x 2^-23 of the fp32 products), plus, in the figure, what is not the kernel's
    doing: AFF16_IDENTITY_UNITS for the rounding of the M = I run, 4 units for the 2^-22 resolution of gD on its way through the net's
    backward, and 4 x 3 x the forward's format term (format_units): the arithmetic's error E of D moves t, |t|^2 (twice) and M^-1, each by
    (|E|_2 / s0) kappa relatively, and max-entry against 2-norm costs a factor 3 (the count of tests/test_gpu_polar3.py).
    The cotangents are scaled per sample by min(1, s_min) so that |dL/dM| ~ |cotangent| / s_min stays of order one, inside the half range
    the backward's activations travel in: the overflow report must stay quiet.  fc_last.bias.grad = sum_n gD_n to the training tests'
    REL = 2e-4 of its maximum against the fp64 sum.  dL/dR on the tangent space against fp64 autograd of the whole oracle flow: REL of the
    batch maximum (the Moebius layer's share, tests/test_gpu_grad.py) plus the host gate of the 4x4 layer's own dL/dR with the same
    additions.  Measured on an MI355X (n = 512 / 6 400, forward and inverse pass): dL/dM figure max 2.5 .. 10.5, at most 0.058 of the
    gate (none of the format term is used: the whole batch is inside the gate without it), max |gM| 5.9 .. 8.7, fc_last.bias.grad within 3.8e-7 .. 2.0e-6 of
    its maximum, dL/dR tangent error at most 0.43 of its gate."""
    from tests.test_gpu_grad import REL, tangent
    seen, feat, kind_of = training_table(n)
    assert len(seen) == n
    assert_net_returns_D(inverse, feat, seen)
    s = ax.svals(seen)
    k = s[:, 0] / s[:, -1]
    rng = np.random.default_rng(60 + inverse)
    damp = np.minimum(1.0, s[:, -1])
    gR = (rng.standard_normal((n, 3, 3)) * damp[:, None, None]).astype(np.float32)
    gl = (rng.standard_normal(n) * damp).astype(np.float32)
    R = rotations(n, 11)
    cfg, w, i16 = steering(inverse)
    fl = product_flow(cfg, w).train()
    _, _, base, _ = _train_pass(fl, inverse, R, np.zeros_like(feat))          # the rotation that enters the 4x4 layer, re-normalised
    base = base.detach().cpu().numpy()
    Rd, fd, Ro, l = _train_pass(fl, inverse, R, feat)
    ((Ro * torch.from_numpy(gR).cuda()).sum() + (l * torch.from_numpy(gl).cuda()).sum()).backward()
    torch.cuda.synchronize()
    gfeat = fd.grad.cpu().numpy().astype(np.float64)
    D = (seen - EYE32).reshape(n, 16)
    gD = np.where(D > 0, gfeat[:, :16], -gfeat[:, 16:32]).reshape(n, 4, 4)
    assert np.isfinite(Ro.detach().cpu().numpy()).all() and np.isfinite(gD).all()
    want, want_R = ax.layer_grad64(seen, base, gR, gl, inverse)
    yg = np.array([yardstick_grad(inverse, kd, "realistic")["grad"] for kd in ax.KINDS])[kind_of]
    yt = np.array([yardstick_grad(inverse, kd, "realistic")["tan"] for kd in ax.KINDS])[kind_of]
    gate, gate_R = backward_gates(inverse, seen, gR, gl, want, want_R, base, yg, yt)
    more = (12 * format_units(seen) + 4 + AFF16_IDENTITY_UNITS) * U23 * k
    gate = gate + more * ax._maxabs(want)
    err = ax._maxabs(gD - want)
    host_gate = gate - 12 * format_units(seen) * U23 * k * ax._maxabs(want)            # everything but the format term
    used = np.maximum(err - host_gate, 0.0) / (U23 * k * ax._maxabs(want))
    print(f"train, n {n}, inverse {inverse}: dL/dM figure max {ax.grad_figure(gD, want, k).max():.2f}, error / gate max {np.max(err / gate):.3f}, "
          f"max |gM| {np.abs(gD).max():.2f}; of the format term's units at most {used.max():.2f} are used (the term: "
          f"{12 * format_units(seen).min():.0f} .. {12 * format_units(seen).max():.0f}), {np.mean(err <= host_gate):.4f} of the batch is inside the gate without it")
    assert (err <= gate).all(), (int(np.argmax(err / gate)), np.max(err / gate))
    gb = dict(fl.named_parameters())[f"layers.{i16}.net.fc_last.bias"].grad.cpu().numpy().astype(np.float64)
    wb = want.reshape(n, 16).sum(0)
    print(f"train, n {n}, inverse {inverse}: fc_last.bias.grad error / max {np.abs(gb - wb).max() / np.abs(wb).max():.2e}")
    assert np.abs(gb - wb).max() <= REL * np.abs(wb).max()
    # dL/dR on the tangent space against the whole oracle flow in fp64
    p = {kk: torch.from_numpy(v).double() for kk, v in w.items()}
    Rt = torch.from_numpy(R).double().requires_grad_(True)
    fn = orc.flow_inverse if inverse else orc.flow_forward
    Rw, lw = fn(cfg, p, Rt, torch.from_numpy(feat).double(), dtype=torch.float64, grad=True)
    ((Rw * torch.from_numpy(gR).double()).sum() + (lw * torch.from_numpy(gl).double()).sum()).backward()
    tg, tw = tangent(R.astype(np.float64), Rd.grad.cpu().numpy().astype(np.float64)), tangent(R.astype(np.float64), Rt.grad.numpy())
    et = np.abs(tg - tw).reshape(n, -1).max(-1)
    gate_t = REL * np.abs(tw).max() + gate_R + more * ax._maxabs(ax.tangent(base, want_R))
    print(f"train, n {n}, inverse {inverse}: dL/dR tangent error / gate max {np.max(et / gate_t):.3f}")
    assert np.isfinite(et).all() and (et <= gate_t).all(), (int(np.argmax(et / gate_t)), np.max(et / gate_t))
    # The half-range overflow report stays quiet.  An overflow of the backward's half-range activations is reported one call LATER, as
    # runtime.HalfRangeError from the next pass (tests/test_gpu_grad.py test_half_range_overflow_is_reported): these two passes are the
    # check, not left-over code.
    try:
        for _ in range(2):
            _train_pass(fl, inverse, R, feat)
            torch.cuda.synchronize()
    except runtime.HalfRangeError as e:
        pytest.fail(f"the backward left the half range: {e}")


# ---- device build against host build -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", PASSES)
def test_device_build_against_host_build(fp32, ha, inverse):
    """The device's layer against the host build of the same headers on the same (M32, B): the share of rotations equal to within
    4 x 2^-23 is reported, not gated (device code contracts to FMAs and takes 1 / x and the square roots from the hardware, the host build
    does not); the difference is gated at the sum of both sides' error bounds.  Measured on an MI355X: 0.993 (forward) and 0.935
    (inverse) of the batch within 4 x 2^-23, the difference at most 0.23 of the bound (ldj 0.26)."""
    seen, feat, yr, yl, yo = table(inverse)
    R = rotations(len(seen), 3)
    out, base, l, l0 = layer_alone(inverse, R, feat)
    Rh, lh = host_cond16(ha, seen, base, inverse)
    k = ax.cond(seen)
    gh, glh = forward_gates(yr, yl, k, ax.log_terms(seen, base, inverse))
    gd, gld = forward_gates(yr + 0.5 * AFF16_IDENTITY_UNITS, yl + 0.5 * AFF16_IDENTITY_LDJ_UNITS, k, ax.log_terms(seen, base, inverse))
    d = ax._maxabs(out.astype(np.float64) - Rh)
    dl = np.abs(l.astype(np.float64) - l0 - lh)
    bound, bound_l = gh + gd, glh + gld + 2.0 ** -24 * (np.abs(l) + np.abs(l0))
    print(f"inverse {inverse}: device R' within 4 x 2^-23 of the host build's on {np.mean(d <= 4 * U23):.4f} of the batch, max difference / bound "
          f"{np.max(d / bound):.3f}; ldj {np.max(dl / bound_l):.3f}")
    assert (d <= bound).all() and (dl <= bound_l).all(), (int(np.argmax(d / bound)), np.max(d / bound), np.max(dl / bound_l))
