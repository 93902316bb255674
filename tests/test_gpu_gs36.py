"""GPU (-m gpu): the per-sample 6x6 layer Condition36Trans (csrc/so3_math.h cond_gs36_apply) inside the stack kernels that inline it
(flow_kernels.h cond36_finish: the only user of a second fc_last tile, with lane-half shuffles of 36 outputs), every sample against fp64
(tests/gs36_exact.py) with the gates of tests/test_gs36_host.py: the yardstick's maximum over the same family of the batch that was fed, times two.

The chosen matrices reach the layer through a STEERING NETWORK (the scheme of tests/test_gpu_aff16.py, for 36 outputs).  The hidden width is
64, the +-split of all 36 entries would need 72 units, so ten entries travel on ONE unit each: the off-diagonal entries of row 0 and of
column 0 of D = M - I (ONE).  The other 26 (SIGNED, the diagonal among them) take two units each, max(D, 0) and max(-D, 0): 62 units in all.
Every hidden layer of the 6x6 layer's net is zero, fc_first copies feature j into unit j (j < 62) and every fc_last row has at most two
non-zero weights of which one is active, so the net returns D with no rounding (asserted on the CPU against the fp32 oracle, bit for bit) and
the kernel sees M32 = fl(I + D).  A one-unit entry must be non-negative (the unit is a ReLU): the random families are made so by
M -> S1 M S2 with S1, S2 diagonal +-1 (`sign_fix`; exact; singular values and cond unchanged; the sign of det M is NOT preserved, so the
share of det < 0 that arrives is reported and asserted instead).  The feature width is 64, the Moebius layer's fc_first does not see the
features, and the 6x6 layer is the LAST layer applied in each pass.

The layer is isolated by a second run with zero features, M = I.  It returns B = [t0 t1 t0 x t1] of the incoming rotation's first two
columns, and the Moebius layer's ldj plus the layer's own at M = I.  The first run is then the fp64 layer at (M, B) up to B's own rounding,
measured on the host build (tests/test_gs36_host.py: GS36_IDENTITY_UNITS, GS36_IDENTITY_LDJ_UNITS): these numbers of units are ADDED to the
gates' figures, for that reason and no other.  The two ldj also carry the Moebius layer's ldj, summed in fp32: 2^-24 (|ldj| + |ldj0|).

The training kernels' reverse step (csrc/so3_grad.h cond_gs36_backward) is judged per sample at the end of the file, on both block sizes.

Measured on an MI355X: see the docstrings of the tests and DESIGN.md section 3.7d.
"""
import functools

import numpy as np
import pytest
import torch

import rotationnormflow_amd as rnf
from oracle import flow_oracle as orc
from rotationnormflow_amd import make_config, runtime, synth
from tests import gs36_exact as gx
from tests.gpu_helpers import product_flow
from tests.test_gpu_polar3 import device, rotations, run
from tests.test_gpu_grad import train_block  # noqa: F401  (a fixture: rnf_set_train_block)
from tests.test_gs36_host import (GS36_IDENTITY_LDJ_UNITS, GS36_IDENTITY_UNITS, apply36, backward_gates, h36, references_grad, strictest,  # noqa: F401  (h36: a fixture)
                                  yardstick_grad)

pytestmark = pytest.mark.gpu

U23 = gx.U23
EYE32 = np.eye(6, dtype=np.float32)
FD = 64
PASSES = [False, True]
ONE = np.array([1, 2, 3, 4, 5, 6, 12, 18, 24, 30])           # row 0 and column 0 of D without the corner: one hidden unit each
SIGNED = np.array([i for i in range(36) if i not in set(ONE.tolist())])
NOT_FEEDABLE = ["cond_1e3_small_in_A", "cond_1e3_away_from_A", "pow2_-60", "pow2_-40"]
# the two cond-1e3 edges are defined against the rotation they meet, which on the device is the Moebius layer's output; 2^-40 and 2^-60
# times a matrix lose every digit against the identity in I + D.  They stay host-only (tests/test_gs36_host.py).


def sign_fix(M):
    """S1 M S2 with the ten one-unit entries non-negative: S2[0] = S1[0] = +1, S1[i] = sign M[i,0], S2[j] = sign M[0,j]."""
    M = np.array(M, dtype=np.float64).reshape(-1, 6, 6)
    s1 = np.where(M[:, :, 0] < 0, -1.0, 1.0)
    s2 = np.where(M[:, 0, :] < 0, -1.0, 1.0)
    s1[:, 0], s2[:, 0] = 1.0, 1.0
    return M * s1[:, :, None] * s2[:, None, :]


def as_features(M):
    """(features [n,64] fp32, the matrix the kernel sees [n,6,6] fp32 = fl(I + D), D = fl(M - I) formed in fp64 and rounded once)."""
    M = np.asarray(M).reshape(-1, 6, 6)
    with np.errstate(invalid="ignore"):
        D = (M.astype(np.float64) - np.eye(6)).astype(np.float32).reshape(-1, 36)
        assert not (D[:, ONE] < 0).any(), "a one-unit entry must be non-negative: sign_fix first"
        feat = np.zeros((len(D), FD), np.float32)
        feat[:, :10] = D[:, ONE]                                # NaN / inf travel as themselves
        Ds = D[:, SIGNED]
        feat[:, 10:36] = np.where(Ds > 0, Ds, 0)
        feat[:, 36:62] = np.where(Ds < 0, -Ds, 0)
        bad = ~np.isfinite(Ds)
        feat[:, 10:36][bad] = Ds[bad]
    return feat, D.reshape(-1, 6, 6) + EYE32


@functools.lru_cache(maxsize=None)
def steering(inverse):
    """(cfg, weights, index of the 6x6 layer).  inverse: the flow whose INVERSE pass applies the 6x6 layer last."""
    extra = dict(last_affine=1, first_affine=0) if inverse else {}
    cfg = make_config(layers=1, segments=16, condition=1, feature_dim=FD, rot="36Trans", **extra)
    assert orc.layer_kinds(cfg) == (["cgs36", "mobius"] if inverse else ["mobius", "cgs36"])
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=36, regime="trained")
    i36, im = (0, 1) if inverse else (1, 0)
    pre = f"layers.{i36}.net"
    for k in w:
        if k.startswith(pre + "."):
            w[k] = np.zeros_like(w[k])
    assert w[f"{pre}.fc_first.weight"].shape == (64, FD) and w[f"{pre}.fc_last.weight"].shape == (36, 64)
    for j in range(62):
        w[f"{pre}.fc_first.weight"][j, j] = 1.0
    for p, e in enumerate(ONE):
        w[f"{pre}.fc_last.weight"][e, p] = 1.0
    for q, e in enumerate(SIGNED):
        w[f"{pre}.fc_last.weight"][e, 10 + q] = 1.0
        w[f"{pre}.fc_last.weight"][e, 36 + q] = -1.0
    w[f"layers.{im}.conditioner.fc_first.weight"][:, 3:] = 0.0             # the Moebius layer does not see the features
    return cfg, w, i36


@functools.lru_cache(maxsize=None)
def flow_of(inverse):
    cfg, w, _ = steering(inverse)
    return product_flow(cfg, w)


def assert_net_returns_D(inverse, feat, seen):
    cfg, w, i36 = steering(inverse)
    p = {k: torch.from_numpy(v) for k, v in w.items()}
    got = orc.cond36_matrix(torch.from_numpy(feat), p, f"layers.{i36}.net").numpy()
    assert np.array_equal(got, seen, equal_nan=True)


def layer_alone(inverse, R, feat, fl=None):
    """(R' of the run, R' of the run with M = I, ldj of both)."""
    fl = flow_of(inverse) if fl is None else fl
    out, l = run(None, inverse, R, feat, fl)
    base, l0 = run(None, inverse, R, np.zeros_like(feat), fl)
    return out, base, l, l0


@functools.lru_cache(maxsize=None)
def table(inverse, window="realistic", per_kind=800, seed=5, lo_hi=None, dmax=None):
    """(seen [n,6,6], features, index of the sample's family).  Every family, sign-fixed; kept are the matrices inside the domain as the
    kernel sees them, and with dmax those with |D| <= dmax (drawn 8 x as many and cut): conditions on the input."""
    seen, feat, kind_of = [], [], []
    for i, kind in enumerate(gx.KINDS):
        M, _ = gx.random_batch(kind, per_kind * (8 if dmax else 1), seed, lo_hi or gx.WINDOWS[window])
        f, s = as_features(sign_fix(M))
        keep = gx.in_domain(s)
        if dmax:
            keep &= np.abs(s - EYE32).max((-1, -2)) <= dmax
        assert keep.sum() >= (per_kind if dmax else 0.98 * per_kind), (kind, keep.sum())
        seen.append(s[keep][:per_kind]); feat.append(f[keep][:per_kind]); kind_of.append(np.full(len(seen[-1]), i))
    out = tuple(np.concatenate(c) for c in (seen, feat, kind_of))
    assert (np.linalg.det(out[0].astype(np.float64)) < 0).mean() > 0.2          # det < 0 does arrive (sign_fix does not keep the sign)
    return out


def yardsticks_here(seen, base, inverse, kind_of, want, want_l, k, kj):
    """The two fp32 yardsticks on THIS batch, (seen, base): per sample the maximum of its family's figures (rotation, ldj, |QQ^T - I|)."""
    fr = gx.rot_figure(gx.lapack_rot32(seen, base, inverse), want, k)
    fo = gx.orth_err(gx.lapack_rot32(seen, base, inverse))
    fl = gx.ldj_figure(gx.oracle32(seen, base, inverse)[1], want_l, kj)
    yr, yl, yo = np.empty(len(seen)), np.empty(len(seen)), np.empty(len(seen))
    for i in np.unique(kind_of):
        m = kind_of == i
        yr[m], yl[m], yo[m] = fr[m].max(), fl[m].max(), fo[m].max()
    return yr, yl, yo


def gates(k, kj, yr, yl, extra=0.0):
    """Per-sample absolute gates of the rotation and of the layer's ldj: 2 x the yardstick plus the identity run's units (and the
    format's, twelve times as many for ldj: format_units), as figures."""
    return U23 * k * (2 * yr + GS36_IDENTITY_UNITS + extra), U23 * kj * (2 * yl + GS36_IDENTITY_LDJ_UNITS + 12 * extra)


def check_layer(inverse, seen, feat, kind_of, what, extra=0.0, fl=None, fixed=None):
    """Every sample: R' and the layer's ldj against fp64 within the gates, R' orthogonal.  The yardsticks are computed here, on the batch
    that was fed and the rotations that entered the layer; fixed = (rot, ldj, orth): given figures instead (the named edges)."""
    n = len(seen)
    R = rotations(n, 3)
    out, base, l, l0 = layer_alone(inverse, R, feat, fl)
    want, want_l = gx.gs36_64(seen, base, inverse)
    k = gx.kappa(seen, base, inverse)
    kj = k * gx.cond_J(seen, base, inverse)
    yr, yl, yo = fixed if fixed is not None else yardsticks_here(seen, base, inverse, kind_of, want, want_l, k, kj)
    gate, gate_l = gates(k, kj, yr, yl, extra)
    gate_l = gate_l + 2.0 ** -24 * (np.abs(l) + np.abs(l0))
    err, o = gx._maxabs(out.astype(np.float64) - want), gx.orth_err(out)
    el = np.abs(l.astype(np.float64) - l0 - want_l)
    used = np.max(err / (U23 * k) - 2 * yr - GS36_IDENTITY_UNITS) if np.ndim(extra) else 0.0
    used_l = np.max(el / (U23 * kj) - 2 * yl - GS36_IDENTITY_LDJ_UNITS) if np.ndim(extra) else 0.0
    print(f"{what}: max error / gate {np.max(err / gate):.3f}, rotation figure max {np.max(err / (U23 * k)):.2f} (yardstick {np.max(yr):.2f}), |R'R'^T - I| max {o.max() / U23:.2f} units "
          f"(yardstick {np.max(yo) / U23:.2f}); ldj error / gate max {np.max(el / gate_l):.3f}, ldj figure max {np.max(el / (U23 * kj)):.2f} (yardstick {np.max(yl):.2f}); "
          f"vacuous ldj gates {np.mean(U23 * kj > gx.LDJ_VACUOUS):.4f}"
          + (f"; of the format term's units at most {max(used, 0.0):.2f} (rotation) and {max(used_l, 0.0):.2f} (ldj) are used (the term: {np.min(extra):.1f} .. {np.max(extra):.1f}, x 12 for ldj)" if np.ndim(extra) else ""))
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
    """Under set_precision("fp32") the matrix arrives exactly at any scale: every family at realistic scales 10^U(-2,3) (about 800 each),
    and the `range` window as far as fp32 features carry it, 10^U(0,12), 400 per family (below 1 the sum I + D keeps the identity's digits,
    not M's).  Measured on an MI355X (forward / inverse pass): rotation figure at most 0.87 / 1.38 beside a yardstick of 1.59 / 1.70 on
    the same batch, at most 0.113 / 0.200 of the gate, |R'R'^T - I| at most 3.18 / 3.10 units, ldj figure at most 4.90 / 3.43, at most
    0.269 / 0.171 of its gate; 0.0010 / 0.0145 of the samples have a vacuous ldj gate."""
    seen, feat, kind_of = table(inverse)
    assert_net_returns_D(inverse, feat, seen)
    check_layer(inverse, seen, feat, kind_of, f"fp32, inverse {inverse}, realistic")
    seen, feat, kind_of = table(inverse, "range", 400, 6, (0.0, 12.0))
    assert_net_returns_D(inverse, feat, seen)
    check_layer(inverse, seen, feat, kind_of, f"fp32, inverse {inverse}, scales up to 1e12")


@pytest.mark.parametrize("inverse", PASSES)
def test_in_domain_edges_fp32(fp32, inverse):
    """The feedable named edges (sign-fixed; as rounded by I + (M - I) where that is still inside the domain), at the strictest gate.
    Measured on an MI355X: at most 0.081 of the rotation gate and 0.025 of the ldj gate."""
    names, M, _, inside = gx.edges(inverse)
    keep = [i for i, n in enumerate(names) if inside[i] and n not in NOT_FEEDABLE]
    feat, seen = as_features(sign_fix(M[keep]))
    assert gx.in_domain(seen).all() and np.array_equal(seen[0], EYE32)
    print("edges fed:", [names[i] for i in keep])
    assert {"identity", "block_rotations", "swap_blocks", "pow2_40", "pow2_60"} == {names[i] for i in keep}
    assert_net_returns_D(inverse, feat, seen)
    g = tuple(np.full(len(seen), strictest(inverse, key)) for key in ("rot", "ldj", "orth"))
    check_layer(inverse, seen, feat, None, f"fp32, inverse {inverse}, edges", fixed=g)


DMAX = 30.0


def format_units(seen):
    """The split formats' resolution of D, in units of the rotation figure.  The kernel's D carries an error E with
    max|E_ij| <= 2^-22 max(1, max|D|) <= 2^-22 (s0(M) + 1) (tests/test_gpu_polar3.py test_every_sample_split_precision), which
    is not the kernel's doing, and |E|_2 <= 6 max|E_ij| for a 6x6.  Forward pass: A = M v moves by |E|_2 |v| = sqrt(2) |E|_2, its
    Gram-Schmidt factor by that over s2(A) = (|E|_2 / s0) kappa.  Inverse pass: x = M^-1 v moves by cond(M) (|E|_2 / s0) |x|, the factor
    by that over s2(A) = (|E|_2 / s0) kappa again.  |E|_2 / s0 <= 6 x 2^-22 (1 + 1 / s0) = 12 (1 + 1 / s0) units of 2^-23.
    ldj = log|det J|: d ldj = tr(J^-1 dJ) has three terms of at most cond(J) |dJ| / |J| each, and an entry of J (a tangent image
    (da - t (t . da)) / |a| turned into the frame t0, t1, t2) feels the same relative perturbation through four factors (the direction
    of a, its length, da, and the frame), so ldj gets 3 x 4 = twelve times as many units of 2^-23 kappa cond(J) (gates)."""
    return 12 * (1 + 1 / gx.svals(seen)[:, 0])


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("inverse", PASSES)
def test_every_sample_split_precision(inverse, precision):
    """The default arithmetic and bf16x3, realistic window with |D| <= 30, with the format allowance of format_units and no wider; how
    much of it is used is printed.  Measured on an MI355X (forward / inverse pass): f16x2 shows rotation figures up to 137 / 100 and ldj
    figures up to 190 / 136 and uses at most 129 / 90 (rotation) and 173 / 118 (ldj) of the term's 12 .. 1 200 units, 0.140 / 0.127 of the
    rotation gate; bf16x3 shows 0.90 / 1.11 and 5.53 / 4.18 and uses none of the term."""
    old = rnf.get_precision()
    rnf.set_precision(precision)
    try:
        seen, feat, kind_of = table(inverse, dmax=DMAX)
        assert_net_returns_D(inverse, feat, seen)
        check_layer(inverse, seen, feat, kind_of, f"{precision}, inverse {inverse}", extra=format_units(seen))
        assert not runtime.fallback_fired(device())
    finally:
        rnf.set_precision(old)


# ---- launch shape ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", PASSES)
def test_a_row_is_the_same_in_every_launch_size(fp32, inverse):
    """n = 1, 63, 64, 65, 257 and 4 097 (cond36_finish pairs lanes j and j + 32 and reads rows 32..35 from a second fc_last tile; a wave is
    64 lanes, a tile 256 rotations): row i is bit-equal whatever n it travels in, and nothing is written past row n-1 (sentinel rows behind
    both outputs, checked in run)."""
    seen, feat, _ = table(inverse)
    N = 4097
    feat = np.ascontiguousarray(np.resize(feat, (N, FD)))
    R = rotations(N, 8)
    fl = flow_of(inverse)
    full, lfull = run(None, inverse, R, feat, fl)
    assert np.isfinite(full).all() and np.isfinite(lfull).all() and full.shape[0] == N
    for n in (1, 63, 64, 65, 257):
        part, lpart = run(None, inverse, R[:n], feat[:n], fl)
        assert part.shape[0] == n and np.array_equal(part, full[:n]) and np.array_equal(lpart, lfull[:n]), n


# ---- out of the domain -----------------------------------------------------------------------------------------------------------------------

def bad_rows():
    """Features of: the zero matrix; lower rows equal to upper rows (a1 = a0); two equal rows (singular on the inverse pass); one NaN entry.
    The matrices are made of multiples of 2^-6 below 4, so that M - I and I + D are exact and the kernel sees exactly these."""
    rng = np.random.default_rng(3)
    base = sign_fix(np.round((np.eye(6) + 0.2 * rng.standard_normal((6, 6))) * 64) / 64)[0]
    twin, rows2, nan = base.copy(), base.copy(), base.copy()
    twin[3:] = twin[:3]
    rows2[4] = rows2[1]
    nan[1, 2] = np.nan
    M = np.stack([np.zeros((6, 6)), twin, rows2, nan])
    feat, seen = as_features(M)
    assert np.array_equal(seen[:3], M[:3].astype(np.float32))
    return dict(zip(("zero", "a1_equals_a0", "two_equal_rows", "one_nan"), feat))


@pytest.mark.parametrize("inverse", PASSES)
def test_bad_rows_touch_no_other_row(fp32, inverse):
    """The zero matrix, a1 = a0, two equal rows and a NaN feature among 1 000 clean rows, exact arithmetic on the way in: the clean rows
    are bit-equal to the all-clean run, the bad rows are NaN throughout with a non-finite ldj (two equal rows: on the inverse pass; on the
    forward pass NaN or a rotation to 16 units beside a finite ldj).  The NaN entry reaches the kernel as a NaN FEATURE, which the
    kernel's feature stage reports by its own convention, not the layer's: the ReLU drops the NaN, the layer sees a finite matrix, and the
    row is marked with a NaN in R' and a NaN ldj on the way out (as in tests/test_gpu_aff16.py).  That row is asked for exactly that."""
    seen, feat, _ = table(inverse)
    n = 1000
    feat = feat[:n].copy()
    R = rotations(n, 9)
    fl = flow_of(inverse)
    clean, lclean = run(None, inverse, R, feat, fl)
    assert np.isfinite(clean).all() and np.isfinite(lclean).all()
    rows = dict(zip((17, 95, 500, 999), bad_rows().items()))
    for r, (_, f) in rows.items():
        feat[r] = f
    got, l = run(None, inverse, R, feat, fl)
    rest = np.array([i not in rows for i in range(n)])
    assert np.array_equal(got[rest], clean[rest]) and np.array_equal(l[rest], lclean[rest])
    for r, (what, _) in rows.items():
        nan = bool(np.isnan(got[r]).all()) and not np.isfinite(l[r])
        print(f"inverse {inverse}, {what}: {'NaN' if nan else got[r]}, ldj {l[r]}")
        if what == "one_nan":
            assert np.isnan(got[r]).any() and np.isnan(l[r]), (what, got[r], l[r])
        elif what == "two_equal_rows" and not inverse:
            assert nan or (np.isfinite(got[r]).all() and gx.orth_err(got[r][None])[0] <= 16 * U23 and np.isfinite(l[r])), (what, got[r], l[r])
        else:
            assert nan, (what, got[r], l[r])


def test_a_singular_matrix_fires_the_guard_on_the_inverse_pass():
    """Default arithmetic, guard on, inverse pass: M = 0 (D = -I; with the feature scale set to 1 the features 0 and 1 pass the
    split-precision conditioner without rounding, so the matrix arrives exactly singular) has no inverse.  The layer returns NaN, which is
    reported as every non-finite R' is (runtime.fallback_fired); every other row stays finite."""
    old = rnf.get_precision()
    rnf.set_precision("f16x2")                                   # only the split-precision kernels are guarded
    try:
        seen, feat, _ = table(True, dmax=DMAX)
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


# ---- device build against host build -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", PASSES)
def test_device_build_against_host_build(fp32, h36, inverse):
    """The device's layer against the host build of the same headers on the same (M32, B): the share of rotations equal to within
    4 x 2^-23 is reported, not gated (device code contracts to FMAs and takes 1 / x and the square roots from the hardware, the host build
    does not); the difference is gated at the sum of both sides' error bounds.  Measured on an MI355X: 0.9915 (forward) and 0.9590
    (inverse) of the batch within 4 x 2^-23, the difference at most 0.185 of the bound (ldj 0.194)."""
    seen, feat, kind_of = table(inverse)
    R = rotations(len(seen), 3)
    out, base, l, l0 = layer_alone(inverse, R, feat)
    Rh, lh = apply36(h36, seen, base, inverse)
    want, want_l = gx.gs36_64(seen, base, inverse)
    k = gx.kappa(seen, base, inverse)
    kj = k * gx.cond_J(seen, base, inverse)
    yr, yl, _ = yardsticks_here(seen, base, inverse, kind_of, want, want_l, k, kj)
    gd, gld = gates(k, kj, yr, yl)
    gh, glh = U23 * k * 2 * yr, U23 * kj * 2 * yl
    d = gx._maxabs(out.astype(np.float64) - Rh)
    dl = np.abs(l.astype(np.float64) - l0 - lh)
    bound, bound_l = gh + gd, glh + gld + 2.0 ** -24 * (np.abs(l) + np.abs(l0))
    print(f"inverse {inverse}: device R' within 4 x 2^-23 of the host build's on {np.mean(d <= 4 * U23):.4f} of the batch, max difference / bound "
          f"{np.max(d / bound):.3f}; ldj {np.max(dl / bound_l):.3f}")
    assert (d <= bound).all() and (dl <= bound_l).all(), (int(np.argmax(d / bound)), np.max(d / bound), np.max(dl / bound_l))


# ---- training backward: so3_grad.h cond_gs36_backward inside both training kernels ---------------------------------------------------------

DMAX_TRAIN = 3000.0            # the features stay far inside the half range (65504) the activations travel in
N_TRAIN = 512
RAGGED = 65                    # a multiple of neither 16 nor 64


@functools.lru_cache(maxsize=None)
def training_table():
    """(seen [512,6,6], features, kind index): every family, sign-fixed, scales 10^U(-2, 2.7), no exact zero in D (so every entry of dL/dD
    is readable from a feature gradient); four times as many are drawn and the first 103 of each family that are inside the domain as
    the kernel sees them, with |D| <= DMAX_TRAIN, are kept (a condition on the input)."""
    per = -(-N_TRAIN // len(gx.KINDS))
    seen, feat = [], []
    for kind in gx.KINDS:
        f, s = as_features(sign_fix(gx.random_batch(kind, 4 * per, 7, (-2.0, 2.7))[0]))
        keep = gx.in_domain(s) & ((s - EYE32) != 0).all((-1, -2)) & (np.abs(s - EYE32).max((-1, -2)) <= DMAX_TRAIN)
        assert keep.sum() >= per, (kind, keep.sum())
        seen.append(s[keep][:per]); feat.append(f[keep][:per])
    return np.concatenate(seen)[:N_TRAIN], np.concatenate(feat)[:N_TRAIN], np.repeat(np.arange(len(gx.KINDS)), per)[:N_TRAIN]


def _train_pass(fl, inverse, R, feat):
    Rd = torch.from_numpy(np.ascontiguousarray(R)).cuda().requires_grad_(True)
    fd = torch.from_numpy(np.ascontiguousarray(feat)).cuda().requires_grad_(True)
    Ro, l = fl.inverse(Rd, fd) if inverse else fl(Rd, fd)
    return Rd, fd, Ro, l


def feature_grad_to_gD(gfeat, seen):
    """dL/dD [n,6,6] from the feature gradient: the steering net's ReLUs and +-1 weights pass it unchanged.  ONE entries from gfeat[:, :10],
    SIGNED entries from gfeat[:, 10:36] where D > 0 and from -gfeat[:, 36:62] where D < 0."""
    n = len(seen)
    D = (seen - EYE32).reshape(n, 36)
    gD = np.empty((n, 36))
    gD[:, ONE] = gfeat[:, :10]
    gD[:, SIGNED] = np.where(D[:, SIGNED] > 0, gfeat[:, 10:36], -gfeat[:, 36:62])
    return gD.reshape(n, 6, 6)


@pytest.mark.parametrize("n", [N_TRAIN, RAGGED])
@pytest.mark.parametrize("block", [16, 64])
@pytest.mark.parametrize("inverse", PASSES)
def test_training_backward_per_sample(inverse, block, n, train_block):
    """.train(), default arithmetic: cond_gs36_backward inside the training kernels, the block forced to 16 (train_block16.h) and to 64
    (train_kernels.h; the same binary that serves large batches), n = 512 and a ragged n = 65 (every eighth row of the same table).

    dL/dM per sample is read from the feature gradient (feature_grad_to_gD; the Moebius layer does not see the features) and judged
    against fp64 autograd of the fp64 layer, fed with the rotation the training forward returns for M = I (zero features: the
    re-normalised input, module docstring).  Gate per sample: the host test's (tests/test_gs36_host.py backward_gates: 2 x the yardstick
    of the sample's family at realistic scales, plus 4 x 2^-23 of the fp32 products), plus, in the figure, what is not the kernel's
    doing: GS36_IDENTITY_UNITS for the rounding of the M = I run, 4 units for the 2^-22 resolution of gD on its way through the net's
    backward, and 12 x the forward's format term (format_units): the arithmetic's error E of D moves a, its two lengths, the frame and
    the solve, each by (|E|_2 / s0) kappa relatively, and max-entry against 2-norm costs a factor 3 (the count of tests/test_gpu_aff16.py).
    How much of the format term is used is printed.
    The cotangents are damped per sample by min(1, 1 / max|dL/dM of the undamped cotangents|) (fp64; the gradient is linear in them), so
    that |dL/dM| stays of order one, inside the half range the backward's activations travel in: the overflow report must stay quiet.
    The share of samples whose forward ldj gate is vacuous is printed and must not exceed 0.12; no sample is left out.
    fc_last.bias.grad = sum_n gD_n to the training tests' REL = 2e-4 of its maximum against the fp64 sum.  dL/dR on the tangent space
    against fp64 autograd of the whole oracle flow: REL of the batch maximum (the Moebius layer's share, tests/test_gpu_grad.py) plus the
    host gate of the 6x6 layer's own dL/dR with the same additions.  Measured figures: DESIGN.md section 3.7d."""
    from tests.test_gpu_grad import REL, tangent
    seen, feat, kind_of = training_table()
    if n != N_TRAIN:
        pick = np.arange(n) * (N_TRAIN // n)
        seen, feat, kind_of = seen[pick], feat[pick], kind_of[pick]
    assert len(seen) == n and len(np.unique(kind_of)) == len(gx.KINDS)
    assert_net_returns_D(inverse, feat, seen)
    train_block(block)
    R = rotations(n, 11)
    cfg, w, i36 = steering(inverse)
    fl = product_flow(cfg, w).train()
    _, _, base, _ = _train_pass(fl, inverse, R, np.zeros_like(feat))          # the rotation that enters the 6x6 layer, re-normalised
    base = base.detach().cpu().numpy()
    rng = np.random.default_rng(60 + inverse)
    gR1, gl1 = rng.standard_normal((n, 3, 3)), rng.standard_normal(n)
    damp = np.minimum(1.0, 1.0 / gx._maxabs(gx.layer_grad64(seen, base, gR1, gl1, inverse)[0]))
    gR, gl = (gR1 * damp[:, None, None]).astype(np.float32), (gl1 * damp).astype(np.float32)
    Rd, fd, Ro, l = _train_pass(fl, inverse, R, feat)
    ((Ro * torch.from_numpy(gR).cuda()).sum() + (l * torch.from_numpy(gl).cuda()).sum()).backward()
    torch.cuda.synchronize()
    gD = feature_grad_to_gD(fd.grad.cpu().numpy().astype(np.float64), seen)
    assert np.isfinite(Ro.detach().cpu().numpy()).all() and np.isfinite(gD).all()
    k, kl = gx.grad_conditioning(seen, base, inverse)
    want = references_grad(seen, base, gR, gl, inverse)
    yg = np.array([yardstick_grad(inverse, kd, "realistic")["grad"]["all"] for kd in gx.KINDS])[kind_of]
    yt = np.array([yardstick_grad(inverse, kd, "realistic")["tan"]["all"] for kd in gx.KINDS])[kind_of]
    gate, gate_R = backward_gates(inverse, seen, base, gR, gl, want["all"], want["rot"], k, kl, yg, yt)
    den_M = k * gx._maxabs(want["rot"][0]) + kl * gx._maxabs(want["all"][0] - want["rot"][0])
    den_R = k * gx._maxabs(gx.tangent(base, want["rot"][1])) + kl * gx._maxabs(gx.tangent(base, want["all"][1]) - gx.tangent(base, want["rot"][1]))
    fmt = 12 * format_units(seen)
    host_gate = gate + (4 + GS36_IDENTITY_UNITS) * U23 * den_M                      # everything but the format term
    gate = host_gate + fmt * U23 * den_M
    err = gx._maxabs(gD - want["all"][0])
    used = np.maximum(err - host_gate, 0.0) / (U23 * den_M)
    vac = float(np.mean(U23 * k * gx.cond_J(seen, base, inverse) > gx.LDJ_VACUOUS))
    print(f"train, block {block}, n {n}, inverse {inverse}: dL/dM figure max {gx.grad_figure(gD, want['all'][0], want['rot'][0], k, kl).max():.2f}, error / gate max {np.max(err / gate):.3f}, "
          f"max |gM| {np.abs(gD).max():.2f}; of the format term's units at most {used.max():.2f} are used (the term: {fmt.min():.0f} .. {fmt.max():.0f}), "
          f"{np.mean(err <= host_gate):.4f} of the batch is inside the gate without it; vacuous ldj gates {vac:.4f}")
    assert (err <= gate).all(), (int(np.argmax(err / gate)), np.max(err / gate))
    assert vac <= 0.12
    gb = dict(fl.named_parameters())[f"layers.{i36}.net.fc_last.bias"].grad.cpu().numpy().astype(np.float64)
    wb = want["all"][0].reshape(n, 36).sum(0)
    print(f"train, block {block}, n {n}, inverse {inverse}: fc_last.bias.grad error / max {np.abs(gb - wb).max() / np.abs(wb).max():.2e}")
    assert np.abs(gb - wb).max() <= REL * np.abs(wb).max()
    # dL/dR on the tangent space against the whole oracle flow in fp64
    p = {kk: torch.from_numpy(v).double() for kk, v in w.items()}
    Rt = torch.from_numpy(R).double().requires_grad_(True)
    fn = orc.flow_inverse if inverse else orc.flow_forward
    Rw, lw = fn(cfg, p, Rt, torch.from_numpy(feat).double(), dtype=torch.float64, grad=True)
    ((Rw * torch.from_numpy(gR).double()).sum() + (lw * torch.from_numpy(gl).double()).sum()).backward()
    tg, tw = tangent(R.astype(np.float64), Rd.grad.cpu().numpy().astype(np.float64)), tangent(R.astype(np.float64), Rt.grad.numpy())
    et = np.abs(tg - tw).reshape(n, -1).max(-1)
    gate_t = REL * np.abs(tw).max() + gate_R + (fmt + 4 + GS36_IDENTITY_UNITS) * U23 * den_R
    print(f"train, block {block}, n {n}, inverse {inverse}: dL/dR tangent error / gate max {np.max(et / gate_t):.3f}")
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


@pytest.mark.parametrize("block", [16, 64])
@pytest.mark.parametrize("inverse", PASSES)
def test_a_refused_row_gets_a_nan_feature_gradient_and_no_other_row_does(fp32, inverse, block, train_block):
    """A row the forward refuses (the zero matrix, a1 = a0, and on the inverse pass two equal rows; exact on the way in) among 97 clean
    rows of the training table, a ragged batch: R' of that row is NaN, its feature gradient is NaN on every unit the matrix keeps active
    and holds no finite non-zero entry, and every other row's feature gradient is finite and bit-equal to the all-clean run's."""
    seen, feat, _ = training_table()
    n = 97
    pick = np.arange(n) * (N_TRAIN // n)
    feat = feat[pick].copy()
    train_block(block)
    R = rotations(n, 12)
    cfg, w, _ = steering(inverse)
    rng = np.random.default_rng(70)
    gR, gl = rng.standard_normal((n, 3, 3)).astype(np.float32) * 1e-3, rng.standard_normal(n).astype(np.float32) * 1e-3

    def grads(f):
        fl = product_flow(cfg, w).train()
        Rd, fd, Ro, l = _train_pass(fl, inverse, R, f)
        ((Ro * torch.from_numpy(gR).cuda()).sum() + (l * torch.from_numpy(gl).cuda()).sum()).backward()
        torch.cuda.synchronize()
        return Ro.detach().cpu().numpy(), fd.grad.cpu().numpy(), Rd.grad.cpu().numpy()
    Rc, gc, gRc = grads(feat)
    assert np.isfinite(Rc).all() and np.isfinite(gc).all() and np.isfinite(gRc).all()
    bad = bad_rows()
    rows = {5: "zero", 40: "a1_equals_a0"}
    if inverse:
        rows[96] = "two_equal_rows"
    for r, what in rows.items():
        feat[r] = bad[what]
    Rb, gb, gRb = grads(feat)
    rest = np.array([i not in rows for i in range(n)])
    assert np.array_equal(Rb[rest], Rc[rest]) and np.array_equal(gb[rest], gc[rest]) and np.array_equal(gRb[rest], gRc[rest])
    for r, what in rows.items():
        active = feat[r, :62] > 0
        print(f"block {block}, inverse {inverse}, {what}: R' {'NaN' if np.isnan(Rb[r]).all() else Rb[r]}, feature gradient NaN on {int(np.isnan(gb[r, :62][active]).sum())} of {int(active.sum())} active units")
        assert np.isnan(Rb[r]).all(), (what, Rb[r])
        assert active.any() and np.isnan(gb[r, :62][active]).all(), (what, gb[r, :62])
        assert not (np.isfinite(gb[r]) & (gb[r] != 0)).any(), (what, gb[r])
