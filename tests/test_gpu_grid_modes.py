"""Top-k pose modes with probability mass on the SO(3) grid (rnf_grid_modes, harness.grid_pose_modes) on the device: k = 1 against the
existing grid search, the reduction against the fp64 checker of tests/test_grid_modes_host.py, a density with a known four-mode answer,
the meaning of log_norm, determinism and grouping, the chunked level-6 path, pose_accuracy(top_k) and the NaN / separation edge cases."""
import numpy as np
import pytest
import torch

from rotationnormflow_amd import grid_pose, harness, runtime, synth
from rotationnormflow_amd.utils import sd
from rotationnormflow_amd.utils.fisher import MatrixFisherN
from tests.test_gpu_grid_pose import _fisher_rows, _flow, _offset
from tests.test_grid_modes_host import grid_modes_fp64

pytestmark = pytest.mark.gpu


def _same(a, b):
    """bit-equal, NaN where NaN"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


def _check_against_fp64(got, want, lp):
    index, log_prob, mass, log_norm, spread = (t.cpu() if t is not None else None for t in got)
    assert np.array_equal(index.numpy(), want["index"]), (index, want["index"])
    assert np.array_equal(log_prob.double().numpy(), np.where(want["index"] >= 0, lp[np.arange(lp.shape[0])[:, None], want["index"]],
                                                               -np.inf))
    assert np.abs(mass.double().numpy() - want["mass"]).max() <= 1e-6
    assert np.abs(log_norm.double().numpy() - want["log_norm"]).max() <= 1e-6
    if want["spread"] is not None:
        assert np.abs(spread.double().numpy() - want["spread"]).max() <= 1e-4


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("precision", ["f16x2", "fp32", "bf16x3"])
def test_k1_equals_the_grid_search(precision, with_base):
    old = runtime.get_precision()
    runtime.set_precision(precision)
    try:
        _, _, fl = _flow()
        B = 8
        feat = torch.from_numpy(synth.features(B, 32, seed=2)).cuda()
        base = _fisher_rows(B) if with_base else None
        est, best, index, O = harness.grid_estimate_rotations(fl, feat, recursion_level=2, offset=_offset(), base=base)
        m = harness.grid_pose_modes(fl, feat, top_k=1, recursion_level=2, offset=O, base=base)
        assert torch.equal(m["index"][:, 0], index) and torch.equal(m["log_prob"][:, 0], best) and torch.equal(m["est"][:, 0], est)
        assert torch.equal(m["offset"], O) and m["est"].shape == (B, 1, 3, 3) and bool((m["mass"] > 0).all())
    finally:
        runtime.set_precision(old)


# (level, g, k, rows): rows < Q takes a prefix of the grid, so that Q is not a multiple of the 256-row tile nor of 2048 rows per block
@pytest.mark.parametrize("level,g,k,rows", [(2, 1, 1, None), (2, 5, 2, None), (2, 5, 16, None), (3, 1, 4, None), (3, 5, 16, None),
                                            (3, 5, 4, 30001), (2, 1, 16, 1000), (5, 1, 1, None), (5, 1, 4, None), (5, 5, 2, None)])
def test_reduction_matches_the_fp64_checker(level, g, k, rows):
    _, _, fl = _flow(seed=12)
    grid = sd.generate_healpix_grid(level, device="cuda", offset=_offset(level + 20))
    if rows is not None:
        grid = grid[:rows]
    Q = grid.shape[0]
    feat = torch.from_numpy(synth.features(g, 32, seed=level + k)).cuda()
    gt = torch.from_numpy(synth.uniform_rotations(g * 3, seed=k)).cuda().reshape(g, 3, 3, 3)
    with torch.no_grad():
        lp = fl.log_prob(grid.repeat(g, 1, 1), feat, feature_repeat=Q)["logp"].reshape(g, Q)
    sep = np.deg2rad(12.0)
    got = harness.grid_modes(lp, grid, k, sep, gt)
    want = grid_modes_fp64(lp.cpu().numpy(), grid.cpu().numpy(), k, sep, gt.cpu().numpy())
    _check_against_fp64(got, want, lp.cpu().double().numpy())


def _rot(axis):
    R = -np.eye(3)
    R[axis, axis] = 1.0
    return R                                                    # a 180-degree rotation about the axis


def test_four_symmetric_modes_share_the_mass():
    G = np.stack([np.eye(3), _rot(0), _rot(1), _rot(2)])       # pairwise 180 degrees apart
    Gt = torch.from_numpy(G.astype(np.float32)).cuda()
    grid = sd.generate_healpix_grid(4, device="cuda", offset=_offset(31))
    Q = grid.shape[0]
    c = MatrixFisherN(64.0 * Gt[:1]).log_const()[0]
    tr = torch.einsum("qij,gij->qg", grid.double(), 64.0 * Gt.double())
    lp = (torch.logsumexp(tr, dim=1) - np.log(4.0) - c.double()).float()[None]
    got = harness.grid_modes(lp, grid, 5, np.deg2rad(30.0), Gt[None])
    index, log_prob, mass, log_norm, spread = got
    want = grid_modes_fp64(lp.cpu().numpy(), grid.cpu().numpy(), 5, np.deg2rad(30.0), G[None])
    _check_against_fp64(got, want, lp.cpu().double().numpy())
    R = grid.cpu().double().numpy().reshape(Q, 9)
    nearest = [int(np.argmax(R @ g.reshape(9))) for g in G]     # the grid point closest to each G_j
    chosen = index[0, :4].cpu().numpy()
    for g, n in zip(G, nearest):
        ang = np.arccos(np.clip((R[chosen] @ g.reshape(9) - 1) / 2, -1, 1)).min()
        assert ang <= np.arccos(np.clip((R[n] @ g.reshape(9) - 1) / 2, -1, 1)) + 1e-3, (ang, n, chosen)
    assert np.abs(mass[0, :4].cpu().numpy() - 0.25).max() < 0.01
    assert float(mass[0, 4]) < 0.01 and int(index[0, 4]) >= 0


def test_log_norm_converges_with_the_grid_level():
    A = torch.from_numpy((4.0 * synth.uniform_rotations(1, seed=3)[0].astype(np.float64) @ np.diag([3.0, 2.0, 1.0])).astype(np.float32))
    base = MatrixFisherN(A.cuda())
    norms = []
    for level in (4, 5):
        grid = sd.generate_healpix_grid(level, device="cuda", offset=_offset(41))
        with torch.no_grad():
            lp = base._log_prob(grid).reshape(1, -1)
        norms.append(float(harness.grid_modes(lp, grid, 1, np.deg2rad(10.0))[3][0]))
    assert abs(norms[0] - norms[1]) < 2e-3, norms


def test_deterministic_and_independent_of_the_grouping():
    _, _, fl = _flow(seed=13)
    B = 6
    feat = torch.from_numpy(synth.features(B, 32, seed=8)).cuda()
    gt = torch.from_numpy(synth.uniform_rotations(B * 2, seed=9)).cuda().reshape(B, 2, 3, 3)
    base = _fisher_rows(B, seed=5)
    kw = dict(top_k=4, separation_deg=20.0, recursion_level=3, offset=_offset(6), base=base, gt_rotation=gt)
    runs = [harness.grid_pose_modes(fl, feat, **kw), harness.grid_pose_modes(fl, feat, **kw),
            harness.grid_pose_modes(fl, feat, images_per_launch=1, **kw), harness.grid_pose_modes(fl, feat, images_per_launch=4, **kw)]
    for r in runs[1:]:
        for key in ("est", "log_prob", "index", "mass", "log_norm", "spread_deg"):
            assert _same(r[key], runs[0][key]), key


def test_level6_gathers_the_chunks_of_one_image():
    _, _, fl = _flow(seed=14)
    feat = torch.from_numpy(synth.features(1, 32, seed=10)).cuda()
    O = _offset(7)
    est, best, index, _ = harness.grid_estimate_rotations(fl, feat, recursion_level=6, offset=O)
    m = harness.grid_pose_modes(fl, feat, top_k=2, recursion_level=6, offset=O)
    assert sd.grid_size(6) > grid_pose.GRID_MAX_LAUNCH_ROWS
    assert torch.equal(m["index"][:, 0], index) and torch.equal(m["log_prob"][:, 0], best) and torch.equal(m["est"][:, 0], est)
    assert int(m["index"][0, 1]) >= 0 and bool(torch.isfinite(m["log_norm"]).all()) and float(m["mass"].sum()) <= 1 + 1e-6


def test_pose_accuracy_best_of_k():
    _, _, fl = _flow(seed=9)
    B, k = 4, 4
    feat = torch.from_numpy(synth.features(B, 32, seed=5)).cuda()
    gt = torch.from_numpy(synth.uniform_rotations(B, seed=6)).cuda()
    O = _offset(1)
    one = harness.pose_accuracy(fl, feat, gt, method="log_pdf", offset=O)
    four = harness.pose_accuracy(fl, feat, gt, method="log_pdf", offset=O, top_k=k)
    modes = harness.grid_pose_modes(fl, feat, top_k=k, number_queries=500, offset=O)
    assert four["est_rotation"].shape == (B, k, 3, 3) and _same(four["est_rotation"], modes["est"])
    valid = modes["index"] >= 0
    err = harness.min_geodesic_distance(modes["est"].reshape(-1, 3, 3), gt.repeat_interleave(k, 0)).reshape(B, k)
    want = torch.rad2deg(torch.where(valid, err, torch.full_like(err, float("inf"))).min(-1).values)
    assert torch.equal(four["err_deg"], want) and bool((four["err_deg"] <= one["err_deg"]).all())
    own = harness.pose_accuracy(fl, feat, modes["est"][:, 0], method="log_pdf", offset=O, top_k=k)
    assert float(own["err_deg"].max()) < 0.05             # 0 up to the fp32 trace of a rotation with itself (at most 1 ulp below 3)
    got = harness.pose_accuracy(fl, feat, gt, method="nll_grad", offset=O, top_k=k, refine_steps=3)
    ok = valid.reshape(-1)
    ref = harness.refine_rotations(fl, feat.repeat_interleave(k, 0)[ok], modes["est"].reshape(-1, 3, 3)[ok], steps=3, lr=1e-4, base=None)
    assert torch.allclose(got["est_rotation"].reshape(-1, 3, 3)[ok], ref, atol=1e-6)
    assert not torch.equal(got["est_rotation"].reshape(-1, 3, 3)[ok], modes["est"].reshape(-1, 3, 3)[ok])


def test_nan_image_and_full_separation():
    old = runtime.get_precision()
    runtime.set_precision("fp32")                                # no range guard: a NaN row cannot make the launch re-run
    try:
        _, _, fl = _flow(seed=15)
        B = 4
        feat = torch.from_numpy(synth.features(B, 32, seed=11)).cuda()
        bad = feat.clone()
        bad[2] = float("nan")
        kw = dict(top_k=3, separation_deg=20.0, recursion_level=2, offset=_offset(8))
        clean, hit = harness.grid_pose_modes(fl, feat, **kw), harness.grid_pose_modes(fl, bad, **kw)
        assert bool(torch.isnan(hit["log_norm"][2])) and bool(torch.isnan(hit["mass"][2]).all())
        assert bool((hit["index"][2, 1:] == -1).all()) and bool(torch.isnan(hit["log_prob"][2, 0]))
        for key in ("est", "log_prob", "index", "mass", "log_norm"):
            for b in (0, 1, 3):
                assert _same(hit[key][b], clean[key][b]), (key, b)
        full = harness.grid_pose_modes(fl, feat, top_k=3, separation_deg=180.0, recursion_level=2, offset=_offset(8))
        assert bool((full["index"][:, 0] >= 0).all()) and bool((full["index"][:, 1:] == -1).all())
        assert bool(torch.isnan(full["est"][:, 1:]).all()) and bool((full["mass"][:, 1:] == 0).all())
        assert torch.allclose(full["mass"][:, 0], torch.ones(B, device="cuda"), atol=1e-6)
    finally:
        runtime.set_precision(old)
