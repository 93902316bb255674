"""Credible sets and HPD levels on the SO(3) grid (rnf_grid_credible, harness.grid_credible / grid_pose_credible) on the device: the
reduction against the fp64 checker and the checking function of tests/test_grid_credible_host.py on its synthetic rows, monotonicity,
consistency with rnf_grid_modes, hand cases, determinism and grouping, the flow end to end with ground truths, calibration of a known
density, and the NaN / empty edge cases."""
import numpy as np
import pytest
import torch

from rotationnormflow_amd import grid_pose, harness, runtime, synth
from rotationnormflow_amd.utils import sd
from rotationnormflow_amd.utils.fisher import MatrixFisherN
from tests.test_gpu_grid_pose import _fisher_rows, _flow, _offset
from tests.test_grid_credible_host import (FULL_GRID_CASES, LEVELS3, LEVELS8, case_seed, check_against_reference, check_credible, eps_for,
                                           grid_credible_fp64, numpy_grid, set_mass, synthetic_logp, synthetic_queries)

pytestmark = pytest.mark.gpu


def _same(a, b):
    """bit-equal, NaN where NaN"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


def _np(got):
    return tuple(t.cpu().numpy() if t is not None else None for t in got)


def _rows(level, g, rows=None, seed=None):
    """synthetic log p [g,Q] on the level's grid (the numpy grid up to level 3, the device's above), or on its first ``rows`` rows"""
    grid = numpy_grid(level) if level <= 3 else sd.generate_healpix_grid(level, device="cuda").cpu().numpy()
    return synthetic_logp(grid[:rows] if rows is not None else grid, g, seed=case_seed(level, g) if seed is None else seed)


# (level, g, levels, G, rows): rows < Q takes a prefix of the grid, so that Q is a multiple of neither the 256-row tile nor the 8192 rows of
# a block; level 5 has 288 blocks per image (the merge of block histograms) and nearly every row in one bin of the first digit
@pytest.mark.parametrize("level,g,levels,G,rows", [(2, 1, (0.9,), 0, None), (2, 5, LEVELS8, 16, None), (3, 1, LEVELS8, 0, None),
                                                   (3, 5, LEVELS8, 16, None), (3, 5, (0.5,), 16, None), (2, 1, LEVELS8, 16, 1),
                                                   (2, 5, LEVELS8, 0, 1000), (3, 5, LEVELS8, 16, 30001), (3, 1, (0.95,), 16, 30001),
                                                   (5, 1, LEVELS3, 16, None), (5, 5, LEVELS3, 0, None)])
def test_reduction_passes_the_checking_function(level, g, levels, G, rows):
    lp = _rows(level, g, rows)
    qs = synthetic_queries(lp, G, seed=level + g) if G else None
    got = _np(harness.grid_credible(torch.from_numpy(lp).cuda(), levels, torch.from_numpy(qs).cuda() if G else None))
    full = rows is None and (level, g) in FULL_GRID_CASES and len(levels) == 8     # asserted exact in nine of ten on the CPU too
    check_against_reference(lp, levels, got, qs, min_exact=0.9 if full else None)
    thr, cnt, mass = got[:3]
    assert np.all(np.diff(thr, axis=1) <= 0) and np.all(np.diff(cnt, axis=1) >= 0) and np.all(np.diff(mass, axis=1) >= 0)


def test_monotone_in_the_level():
    lp = _rows(3, 3, seed=77)
    levels = tuple(np.linspace(0.02, 0.98, 8))
    thr, cnt, mass = _np(harness.grid_credible(torch.from_numpy(lp).cuda(), levels))[:3]
    assert np.all(np.diff(thr, axis=1) <= 0) and np.all(np.diff(cnt, axis=1) >= 0) and np.all(np.diff(mass, axis=1) >= 0)
    assert np.all(mass >= np.asarray(levels, np.float32)[None] - eps_for(lp.shape[1])) and np.all(cnt >= 1)


def test_consistent_with_the_modes_reduction_and_with_itself():
    grid = sd.generate_healpix_grid(3, device="cuda")
    lp = torch.from_numpy(_rows(3, 4, seed=31)).cuda()
    lp[1, 100:5000] = float("-inf")                              # cells without mass
    lp = lp + torch.tensor([0.0, 3.5, -7.25, 1.0], device="cuda")[:, None]      # unnormalised rows: log_norm follows
    qs = torch.stack([lp.max(dim=1).values, torch.full((4,), float("-inf"), device="cuda")], dim=1)
    thr, cnt, mass, log_norm, qm, qc = harness.grid_credible(lp, LEVELS3, qs)
    want = harness.grid_modes(lp, grid, 1, np.deg2rad(10.0))[3]
    assert float((log_norm - want).abs().max()) <= 1e-6
    assert bool((qm[:, 0] == 0).all()) and bool((qc[:, 0] == 0).all())         # nothing is denser than the maximum
    assert bool((qm[:, 1] == 1).all())                                           # every finite cell is above -inf: all of T
    assert torch.equal(qc[:, 1], torch.isfinite(lp).sum(dim=1))
    assert int(qc[1, 1]) == lp.shape[1] - 4900 and bool((cnt[1] <= qc[1, 1]).all())


def test_hand_cases_on_the_device():
    Q = 4608
    const = torch.full((1, Q), -2.5, device="cuda")
    thr, cnt, mass, log_norm, _, _ = harness.grid_credible(const, LEVELS8)
    assert bool((cnt == Q).all()) and bool((mass == 1).all()) and bool((thr == -2.5).all()) and abs(float(log_norm[0]) + 2.5) <= 1e-6
    two = torch.full((1, 20), float(-np.log(9.0)), device="cuda")              # 2 cells of weight 1 and 18 of weight 1/9: half the mass each
    two[0, [3, 11]] = 0.0
    thr, cnt, mass, log_norm, qm, qc = harness.grid_credible(two, (0.2, 0.3, 0.7, 0.99), torch.tensor([[0.0, -1.0, -5.0]], device="cuda"))
    low = float(np.float32(-np.log(9.0)))
    assert cnt[0].tolist() == [2, 2, 20, 20] and thr[0].tolist() == [0.0, 0.0, low, low]
    assert np.allclose(mass[0].cpu().numpy(), [0.5, 0.5, 1.0, 1.0], atol=1e-6) and abs(float(log_norm[0]) - np.log(4.0 / 20)) <= 1e-6
    assert qc[0].tolist() == [0, 2, 20] and np.allclose(qm[0].cpu().numpy(), [0.0, 0.5, 1.0], atol=1e-6)
    zeros = torch.tensor([[-1.0, -0.0, 0.0, -2.0, 0.0, -0.0]], device="cuda")   # zeros of either sign tie
    thr, cnt, mass, _, qm, qc = harness.grid_credible(zeros, (0.1, 0.8), torch.tensor([[0.0, -0.0]], device="cuda"))
    assert cnt[0].tolist() == [4, 4] and thr[0].tolist() == [0.0, 0.0] and qc[0].tolist() == [0, 0]
    one = harness.grid_credible(torch.tensor([[-3.25]], device="cuda"), (0.01, 0.99), torch.tensor([[-3.25, -4.0]], device="cuda"))
    assert one[1][0].tolist() == [1, 1] and one[0][0].tolist() == [-3.25, -3.25] and one[2][0].tolist() == [1.0, 1.0]
    assert one[5][0].tolist() == [0, 1] and one[4][0].tolist() == [0.0, 1.0] and float(one[3][0]) == -3.25


def test_deterministic_and_independent_of_the_grouping():
    lp = torch.from_numpy(_rows(3, 5, rows=30001, seed=55)).cuda()
    qs = torch.from_numpy(synthetic_queries(lp.cpu().numpy(), 16, seed=3)).cuda()
    a, b = harness.grid_credible(lp, LEVELS8, qs), harness.grid_credible(lp, LEVELS8, qs)
    for x, y in zip(a, b):
        assert _same(x, y)
    for i in range(lp.shape[0]):
        for x, y in zip(a, harness.grid_credible(lp[i:i + 1], LEVELS8, qs[i:i + 1])):
            assert _same(x[i:i + 1], y), i
    _, _, fl = _flow(seed=13)
    B = 6
    feat = torch.from_numpy(synth.features(B, 32, seed=8)).cuda()
    gt = torch.from_numpy(synth.uniform_rotations(B * 2, seed=9)).cuda().reshape(B, 2, 3, 3)
    kw = dict(levels=LEVELS3, recursion_level=3, offset=_offset(6), base=_fisher_rows(B, seed=5), gt_rotation=gt)
    runs = [harness.grid_pose_credible(fl, feat, **kw), harness.grid_pose_credible(fl, feat, images_per_launch=1, **kw),
            harness.grid_pose_credible(fl, feat, images_per_launch=4, **kw)]
    for r in runs[1:]:
        for key in ("threshold", "count", "volume", "mass", "log_norm", "gt_log_prob", "gt_level", "gt_inside"):
            assert _same(r[key].float(), runs[0][key].float()), key


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("precision", ["f16x2", "fp32", "bf16x3"])
def test_pose_credible_equals_the_reduction_of_the_materialised_density(precision, with_base):
    old = runtime.get_precision()
    runtime.set_precision(precision)
    try:
        _, _, fl = _flow()
        B = 8
        feat = torch.from_numpy(synth.features(B, 32, seed=2)).cuda()
        base = _fisher_rows(B) if with_base else None
        est, best, index, O = harness.grid_estimate_rotations(fl, feat, recursion_level=2, offset=_offset(), base=base)
        out = harness.grid_pose_credible(fl, feat, recursion_level=2, offset=O, base=base, gt_rotation=est)
        grid = sd.generate_healpix_grid(2, device="cuda", offset=O)
        Q = grid.shape[0]
        with torch.no_grad():
            lp = fl.log_prob(grid.repeat(B, 1, 1), feat, base=base, feature_repeat=Q)["logp"].reshape(B, Q)
        thr, cnt, mass, log_norm, qm, _ = harness.grid_credible(lp, (0.5, 0.9, 0.95), best[:, None])
        assert torch.equal(out["threshold"], thr) and torch.equal(out["count"], cnt) and torch.equal(out["mass"], mass)
        assert torch.equal(out["log_norm"], log_norm) and torch.equal(out["volume"], cnt.float() / Q) and torch.equal(out["offset"], O)
        # the ground truth at the grid's own arg-max: its density is the maximum, nothing is denser, every set holds it
        assert torch.equal(out["gt_log_prob"], best) and bool((out["gt_level"] == 0).all()) and bool(out["gt_inside"].all())
        assert out["gt_inside"].shape == (B, 3) and out["gt_inside"].dtype == torch.bool
    finally:
        runtime.set_precision(old)


def test_pose_credible_ground_truth_statistics_match_the_checker():
    _, _, fl = _flow(seed=17)
    B, K = 6, 3
    feat = torch.from_numpy(synth.features(B, 32, seed=12)).cuda()
    gt = torch.from_numpy(synth.uniform_rotations(B * K, seed=13)).cuda().reshape(B, K, 3, 3)
    base = _fisher_rows(B, seed=14, scale=1.0)                   # broad: random ground truths land inside and outside the sets
    out = harness.grid_pose_credible(fl, feat, levels=LEVELS8, recursion_level=2, offset=_offset(10), base=base, gt_rotation=gt)
    grid = sd.generate_healpix_grid(2, device="cuda", offset=out["offset"])
    Q = grid.shape[0]
    with torch.no_grad():
        lp = fl.log_prob(grid.repeat(B, 1, 1), feat, base=base, feature_repeat=Q)["logp"].reshape(B, Q)
        at = fl.log_prob(gt.reshape(-1, 3, 3), feat, base=base, feature_repeat=K)["logp"].reshape(B, K).max(dim=1).values
    # the densest of the K.  Rows of K = 3 run on another kernel family than rows of 32 (csrc/flow_plan.h); each is within 1.5e-4 of the
    # fp64 density on trained-like weights (the smoke test's bound), so they are within 3e-4 of each other
    assert float((out["gt_log_prob"] - at).abs().max()) < 3e-4
    gt_lp = out["gt_log_prob"].cpu().numpy()
    ref = grid_credible_fp64(lp.cpu().numpy(), LEVELS8, gt_lp[:, None])
    # grid_pose_credible does not return the query count: the checker's own stands in for it
    got = (out["threshold"], out["count"], out["mass"], out["log_norm"], out["gt_level"][:, None], torch.from_numpy(ref["query_count"]))
    check_against_reference(lp.cpu().numpy(), LEVELS8, _np(got), gt_lp[:, None])
    inside = gt_lp.astype(np.float64)[:, None] >= out["threshold"].cpu().numpy().astype(np.float64)
    assert np.array_equal(out["gt_inside"].cpu().numpy(), inside)
    exact = np.array([[abs(set_mass(lp[b].cpu().numpy(), float(ref["threshold"][b, j]))[0] - a) > eps_for(Q) for j, a in enumerate(LEVELS8)]
                      for b in range(B)])
    assert np.array_equal(inside[exact], (gt_lp.astype(np.float64)[:, None] >= ref["threshold"])[exact])
    assert np.abs(out["gt_level"].cpu().numpy().astype(np.float64) - ref["query_mass"][:, 0]).max() <= eps_for(Q)


def test_ground_truth_far_from_a_concentrated_mode_is_outside():
    _, _, fl = _flow(seed=2, layers=3)                           # unconditional: one image per base row
    B = 3
    R = synth.uniform_rotations(B, seed=21).astype(np.float64)
    base = MatrixFisherN(torch.from_numpy((60.0 * R).astype(np.float32)).cuda())
    O = _offset(3)
    est = harness.grid_estimate_rotations(fl, None, recursion_level=3, offset=O, base=base)[0]
    flip = torch.diag(torch.tensor([1.0, -1.0, -1.0], device="cuda"))         # 180 degrees about x
    far = est @ flip
    out = harness.grid_pose_credible(fl, None, levels=(0.5, 0.9, 0.95), recursion_level=3, offset=O, base=base, gt_rotation=far)
    assert bool((out["gt_level"] > 0.99).all()) and not bool(out["gt_inside"].any())
    both = harness.grid_pose_credible(fl, None, levels=(0.5, 0.9, 0.95), recursion_level=3, offset=O, base=base,
                                      gt_rotation=torch.stack([far, est, far], dim=1))           # K = 3: the densest counts
    near = harness.grid_pose_credible(fl, None, levels=(0.5, 0.9, 0.95), recursion_level=3, offset=O, base=base, gt_rotation=est)
    assert torch.equal(both["gt_log_prob"], near["gt_log_prob"]) and bool((both["gt_level"] == 0).all()) and bool(both["gt_inside"].all())
    assert bool((both["gt_log_prob"] > out["gt_log_prob"]).all())


def test_side_layer_flow_gathers_the_chunks_of_one_image():
    _, _, fl = _flow(seed=5, layers=2, condition=1, feature_dim=16, lu=1)          # Condition16TransLU: side layers, one image per launch
    B = 2
    feat = torch.from_numpy(synth.features(B, 16, seed=6)).cuda()
    O = _offset(4).cuda()
    Q = sd.grid_size(4)
    assert Q > grid_pose.GRID_SIDE_LAUNCH_ROWS
    out = harness.grid_pose_credible(fl, feat, recursion_level=4, offset=O)
    grid = sd.generate_healpix_grid(4, device="cuda", offset=O)
    lp = torch.empty(B, Q, device="cuda")
    chunks = 0
    with torch.no_grad():
        for b0, b1, lo, part in grid_pose._grid_launches(fl, feat, grid, B, None, None, None, "test"):
            lp[b0:b1, lo:lo + part.shape[1]] = part
            chunks += 1
    assert chunks == 2 * B
    thr, cnt, mass, log_norm, _, _ = harness.grid_credible(lp, (0.5, 0.9, 0.95))
    assert torch.equal(out["threshold"], thr) and torch.equal(out["count"], cnt) and torch.equal(out["mass"], mass)
    assert torch.equal(out["log_norm"], log_norm)
    for b in range(B):
        check_credible(lp[b].cpu().numpy(), 0.9, float(thr[b, 1]), int(cnt[b, 1]), float(mass[b, 1]))


def test_coverage_of_a_known_density():
    """B = 512 matrix-Fisher densities with singular values in [2, 8], one ground truth drawn from each: the HPD level of the ground truth
    is uniform, so the alpha-set holds it in a fraction alpha of the images, within 5 sqrt(alpha (1 - alpha) / B)."""
    B, level = 512, 3
    rng = np.random.default_rng(2024)
    U, V = synth.uniform_rotations(B, seed=61).astype(np.float64), synth.uniform_rotations(B, seed=62).astype(np.float64)
    s = np.sort(rng.uniform(2.0, 8.0, (B, 3)), axis=1)[:, ::-1]
    base = MatrixFisherN(torch.from_numpy((U * s[:, None, :] @ np.swapaxes(V, 1, 2)).astype(np.float32)).cuda())
    torch.manual_seed(7)
    gt = base._sample(1).reshape(B, 3, 3)
    grid = sd.generate_healpix_grid(level, device="cuda", offset=_offset(9).cuda())
    Q = grid.shape[0]
    levels = (0.5, 0.9)
    with torch.no_grad():
        gt_lp = base._log_prob(gt)
        lp = torch.cat([MatrixFisherN(base.A[b:b + 64])._log_prob(grid.repeat(min(64, B - b), 1, 1)).reshape(-1, Q) for b in range(0, B, 64)])
    thr, cnt, mass, _, gt_level, _ = harness.grid_credible(lp, levels, gt_lp[:, None])
    inside = (gt_lp[:, None] >= thr).cpu().numpy()
    ref = grid_credible_fp64(lp.cpu().numpy(), levels, gt_lp.cpu().numpy()[:, None])
    want = gt_lp.cpu().numpy().astype(np.float64)[:, None] >= ref["threshold"]
    assert np.array_equal(inside, want)
    assert np.abs(gt_level.cpu().numpy()[:, 0].astype(np.float64) - ref["query_mass"][:, 0]).max() <= eps_for(Q)
    for j, a in enumerate(levels):
        assert abs(want[:, j].mean() - a) <= 5 * np.sqrt(a * (1 - a) / B), (a, want[:, j].mean())
    assert abs((ref["query_mass"][:, 0] < 0.5).mean() - want[:, 0].mean()) <= 2 / B      # the level below alpha IS being inside the alpha-set


def test_nan_inf_and_empty_images_leave_the_others_alone():
    good = torch.from_numpy(_rows(2, 3, seed=91)).cuda()
    Q = good.shape[1]
    lp = torch.cat([good[:1], good[:1], good[1:2], good[:1], good[2:], torch.full((1, Q), float("-inf"), device="cuda")])
    lp[1, 700] = float("nan")
    lp[3, 4000] = float("inf")
    qs = torch.from_numpy(synthetic_queries(lp.cpu().numpy(), 3, seed=4)).cuda()
    qs[:, 2] = float("nan")
    out = harness.grid_credible(lp, LEVELS3, qs)
    thr, cnt, mass, log_norm, qm, qc = out
    for b in (1, 3, 5):
        assert bool(torch.isnan(thr[b]).all()) and bool((cnt[b] == -1).all()) and bool(torch.isnan(mass[b]).all())
        assert bool(torch.isnan(qm[b]).all()) and bool((qc[b] == -1).all())
    assert bool(torch.isnan(log_norm[1])) and bool(torch.isnan(log_norm[3])) and float(log_norm[5]) == float("-inf")
    keep = [0, 2, 4]
    alone = harness.grid_credible(lp[keep].contiguous(), LEVELS3, qs[keep].contiguous())
    for x, y in zip(out, alone):
        assert _same(x[keep], y)
    assert bool(torch.isnan(qm[keep, 2]).all()) and bool((qc[keep, 2] == -1).all())            # a NaN query
    assert bool(torch.isfinite(qm[keep, :2]).all()) and bool((qc[keep, :2] >= 0).all())
    F = set_mass(lp[0].cpu().numpy(), float(thr[0, 1]))[0]
    assert abs(float(mass[0, 1]) - F) <= eps_for(Q)
