"""Grid-search pose estimation (eval.py:403-480 ``log_pdf`` / ``nll_grad``): the device HEALPix grid against the fp64 checker of
tests/test_so3_grid.py, and harness.grid_estimate_rotations against the materialised density path, the fp64 oracle, its own grouping, and
its memory bound."""
import numpy as np
import pytest
import torch

from oracle import flow_oracle as orc
from rotationnormflow_amd import grid_pose, harness, make_config, runtime, synth
from rotationnormflow_amd.utils import sd
from rotationnormflow_amd.utils.fisher import MatrixFisherN
from tests.gpu_helpers import product_flow
from tests.test_so3_grid import healpix_grid_fp64

pytestmark = pytest.mark.gpu

C4_LIKE = dict(layers=4, condition=1, feature_dim=32, rot="16UnTrans", frequent_permute=1, last_affine=1, first_affine=0)


def _offset(seed=5):
    return torch.from_numpy(synth.uniform_rotations(1, seed=seed)[0])


def _flow(seed=3, **kw):
    cfg = make_config(**(kw or C4_LIKE))
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=seed, regime="trained")
    return cfg, w, product_flow(cfg, w)


def _fisher_rows(B, seed=7, scale=4.0):
    """B distinct, peaked matrix-Fisher parameters: A_b = scale * R_b diag(3, 2, 1)."""
    R = synth.uniform_rotations(B, seed=seed).astype(np.float64)
    return MatrixFisherN(torch.from_numpy((scale * R @ np.diag([3.0, 2.0, 1.0])).astype(np.float32)).cuda())


def _materialised(fl, grid, feature, base, B):
    """The reference's shape of the computation: every image's [Q] rotations explicit in one [B*Q] batch, then torch.argmax per image."""
    Q = grid.shape[0]
    with torch.no_grad():
        lp = fl.log_prob(grid.repeat(B, 1, 1), feature, base=base, feature_repeat=Q if feature is not None else None)["logp"]
    lp = lp.reshape(B, Q)
    idx = torch.argmax(lp, dim=-1)
    return idx, lp.gather(1, idx[:, None])[:, 0]


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4, 5])
def test_device_grid_matches_the_fp64_checker(level):
    rows = None if level < 5 else np.sort(np.random.default_rng(level).choice(sd.grid_size(level), 10_000, replace=False))
    want = healpix_grid_fp64(level, rows)
    grid = sd.generate_healpix_grid(level, device="cuda")
    assert grid.dtype == torch.float32 and grid.is_cuda and grid.shape == (sd.grid_size(level), 3, 3)
    got = grid.cpu().double().numpy()
    got = got if rows is None else got[rows]
    assert np.abs(got - want).max() < 1e-6
    assert np.abs(got @ np.swapaxes(got, 1, 2) - np.eye(3)).max() < 1e-6
    assert np.abs(np.linalg.det(got) - 1).max() < 1e-6
    O = _offset(level)
    moved = sd.generate_healpix_grid(level, device="cuda", offset=O.cuda()).cpu().double().numpy()
    moved = moved if rows is None else moved[rows]
    assert np.abs(moved - want @ O.double().numpy()).max() < 1e-6
    assert np.abs(moved - got @ O.double().numpy()).max() < 1e-6


def test_grid_api_defaults_cache_and_limits():
    cpu = sd.generate_healpix_grid(size=600)                  # the reference's default: a CPU tensor; size 600 -> level 1
    assert cpu.device.type == "cpu" and cpu.shape == (576, 3, 3)
    assert torch.equal(cpu, sd.generate_healpix_grid(1, device="cuda").cpu())
    q = sd.generate_queries(500, mode="grid")
    assert q is sd.get_closest_available_grid(500) and torch.equal(q, cpu)
    g = sd.get_closest_available_grid(500, device="cuda")
    assert g.is_cuda and g is sd.generate_queries(400, mode="grid", device="cuda")
    torch.manual_seed(0)
    r = sd.generate_queries(1000, mode="random")
    assert r.shape == (1000, 3, 3) and torch.allclose(r @ r.transpose(1, 2), torch.eye(3).expand(1000, 3, 3), atol=1e-5)
    with pytest.raises(ValueError):
        sd.generate_healpix_grid(9, device="cuda")
    with pytest.raises(ValueError):
        sd.generate_queries(10, mode="spiral")


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("precision", ["f16x2", "fp32", "bf16x3"])
def test_grid_search_equals_the_materialised_path(precision, with_base):
    old = runtime.get_precision()
    runtime.set_precision(precision)
    try:
        _, _, fl = _flow()
        B = 8
        feat = torch.from_numpy(synth.features(B, 32, seed=2)).cuda()
        base = _fisher_rows(B) if with_base else None
        est, best, index, O = harness.grid_estimate_rotations(fl, feat, recursion_level=2, offset=_offset(), base=base)
        grid = sd.generate_healpix_grid(2, device="cuda", offset=O)
        idx, val = _materialised(fl, grid, feat, base, B)
        assert torch.equal(index, idx) and torch.equal(best, val)
        assert torch.equal(est, grid[idx])
        assert fl._packed(feat.device).precision == precision
    finally:
        runtime.set_precision(old)


def test_grid_search_agrees_with_the_fp64_oracle():
    cfg = make_config(layers=3, condition=1, feature_dim=16, rot="16Trans")          # tests/test_harness.py's flow
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=4, regime="default")
    fl = product_flow(cfg, w)
    B = 4
    feat = synth.features(B, 16, seed=1)
    est, best, index, O = harness.grid_estimate_rotations(fl, torch.from_numpy(feat).cuda(), recursion_level=1, offset=_offset(9))
    grid = sd.generate_healpix_grid(1, offset=O).numpy()
    Q = grid.shape[0]
    lp, _ = orc.log_prob(cfg, w, np.tile(grid, (B, 1, 1)), np.repeat(feat, Q, axis=0), None, torch.float64)
    lp = lp.reshape(B, Q)
    chosen = lp.gather(1, index.cpu()[:, None])[:, 0]
    assert (lp.max(-1).values - chosen).max().item() < 1e-3
    assert (chosen - best.cpu().double()).abs().max().item() < 1e-3
    assert np.array_equal(est.cpu().numpy(), grid[index.cpu().numpy()])


def test_grouping_and_chunking_do_not_change_the_result(monkeypatch):
    _, _, fl = _flow(seed=6)
    B = 8
    feat = torch.from_numpy(synth.features(B, 32, seed=3)).cuda()
    base = _fisher_rows(B, seed=11)
    runs = [harness.grid_estimate_rotations(fl, feat, recursion_level=2, offset=_offset(2), base=base, images_per_launch=g)
            for g in (1, 3, B, None)]
    with monkeypatch.context() as m:
        m.setattr(grid_pose, "GRID_MAX_LAUNCH_ROWS", 1000)            # one image's 4608 rotations in five ragged chunks
        runs.append(harness.grid_estimate_rotations(fl, feat, recursion_level=2, offset=_offset(2), base=base, images_per_launch=1))
        assert _chunks(fl, feat, 2, B) == 5 * B                       # the patch reaches the launch loop
    est0, best0, index0, _ = runs[0]
    for est, best, index, _ in runs[1:]:
        assert torch.equal(index, index0) and torch.equal(best, best0) and torch.equal(est, est0)
    one = MatrixFisherN(base.A[:1])                                   # a one-row base is shared by every image
    e1, b1, i1, O = harness.grid_estimate_rotations(fl, feat, recursion_level=2, offset=_offset(2), base=one)
    idx, val = _materialised(fl, sd.generate_healpix_grid(2, device="cuda", offset=O), feat, one, B)
    assert torch.equal(i1, idx) and torch.equal(b1, val)


def _chunks(fl, feat, level, B, images_per_launch=1):
    """How many launches ``_grid_launches`` makes for B images on the level's grid."""
    grid = sd.generate_healpix_grid(level, device="cuda", offset=_offset(2).cuda())
    with torch.no_grad():
        return sum(1 for _ in grid_pose._grid_launches(fl, feat, grid, B, None, None, images_per_launch, "test"))


def _same_bits(a, b):
    """torch.equal, with NaNs equal where both have one."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 0, a), torch.where(b.isnan(), 0, b))


def test_every_whole_image_analysis_gathers_ragged_chunks(monkeypatch):
    """Each analysis that reduces whole images, on one image per launch in five ragged chunks (4608 rows, 1000 per launch) against the
    three images in one launch: the same bits in every returned tensor."""
    _, _, fl = _flow(seed=6)
    B = 3
    feat = torch.from_numpy(synth.features(B, 32, seed=3)).cuda()
    gt = torch.from_numpy(synth.uniform_rotations(B, seed=12)).cuda()
    O = _offset(2)

    def analyses(g):
        return dict(modes=harness.grid_pose_modes(fl, feat, top_k=4, recursion_level=2, offset=O, images_per_launch=g),
                    credible=harness.grid_pose_credible(fl, feat, recursion_level=2, offset=O, gt_rotation=gt, images_per_launch=g),
                    fisher=harness.grid_pose_fisher(fl, feat, recursion_level=2, offset=O, images_per_launch=g),
                    mixture=harness.grid_pose_mixture(fl, feat, components=2, iterations=8, recursion_level=2, offset=O, images_per_launch=g),
                    beam=dict(zip(("est", "max_log_prob", "index", "offset"),
                                  harness.grid_beam_estimate_rotations(fl, feat, recursion_level=3, start_level=2, beam=16, offset=O,
                                                                       images_per_launch=g))))

    want = analyses(None)
    assert _chunks(fl, feat, 2, B, None) == 1
    with monkeypatch.context() as m:
        m.setattr(grid_pose, "GRID_MAX_LAUNCH_ROWS", 1000)
        got = analyses(1)
        assert _chunks(fl, feat, 2, B) == 5 * B
    for name, out in want.items():
        assert set(got[name]) == set(out)
        for key, value in out.items():
            assert _same_bits(got[name][key], value), (name, key)


def test_unconditional_flow_uses_one_image_per_base_row():
    _, _, fl = _flow(seed=2, layers=3)
    base = _fisher_rows(3, seed=4, scale=10.0)
    est, best, index, O = harness.grid_estimate_rotations(fl, None, recursion_level=2, offset=_offset(3), base=base)
    assert est.shape == (3, 3, 3) and len(set(index.tolist())) == 3
    idx, val = _materialised(fl, sd.generate_healpix_grid(2, device="cuda", offset=O), None, base, 3)
    assert torch.equal(index, idx) and torch.equal(best, val)
    est, best, index, O = harness.grid_estimate_rotations(fl, recursion_level=1, offset=_offset(3))
    assert est.shape == (1, 3, 3) and best.shape == (1,)
    idx, val = _materialised(fl, sd.generate_healpix_grid(1, device="cuda", offset=O), None, None, 1)
    assert torch.equal(index, idx) and torch.equal(best, val)


def test_batch_coupled_flow_evaluates_one_image_per_launch():
    _, _, fl = _flow(seed=5, layers=2, condition=1, feature_dim=16, lu=1)          # Condition16TransLU
    B = 3
    feat = torch.from_numpy(synth.features(B, 16, seed=6)).cuda()
    est, best, index, O = harness.grid_estimate_rotations(fl, feat, recursion_level=1, offset=_offset(4))
    grid = sd.generate_healpix_grid(1, device="cuda", offset=O)
    for b in range(B):
        idx, val = _materialised(fl, grid, feat[b:b + 1], None, 1)
        assert int(index[b]) == int(idx[0]) and torch.equal(best[b:b + 1], val)
    with pytest.raises(ValueError):
        harness.grid_estimate_rotations(fl, feat, recursion_level=1, images_per_launch=2)


def test_level5_search_does_not_materialise_the_batch():
    _, _, fl = _flow(seed=8)
    B = 16
    feat = torch.from_numpy(synth.features(B, 32, seed=4)).cuda()
    harness.grid_estimate_rotations(fl, feat, recursion_level=0, offset=_offset())             # pack and workspaces outside the window
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    est, best, index, _ = harness.grid_estimate_rotations(fl, feat, recursion_level=5, offset=_offset())
    torch.cuda.synchronize()
    Q = sd.grid_size(5)
    grew = torch.cuda.max_memory_allocated() - before
    assert grew < Q * 48 + Q * 36 + (64 << 20), grew               # one launch's rows + the grid + 64 MB; [B*Q] would be 1.36 GB
    assert est.shape == (B, 3, 3) and bool(torch.isfinite(best).all()) and int(index.max()) < Q


def test_pose_accuracy_methods():
    _, _, fl = _flow(seed=9)
    B = 4
    feat = torch.from_numpy(synth.features(B, 32, seed=5)).cuda()
    gt = torch.from_numpy(synth.uniform_rotations(B, seed=6)).cuda()
    O = _offset(1)
    est0 = harness.grid_estimate_rotations(fl, feat, number_queries=500, offset=O)[0]
    pdf = harness.pose_accuracy(fl, feat, gt, method="log_pdf", offset=O)
    assert torch.equal(pdf["est_rotation"], est0)
    got = harness.pose_accuracy(fl, feat, gt, method="nll_grad", offset=O, refine_steps=3)
    want = harness.refine_rotations(fl, feat, est0, steps=3, lr=1e-4, base=None)
    assert torch.allclose(got["est_rotation"], want, atol=1e-6)
    assert not torch.equal(got["est_rotation"], est0)
    # the default is the inverse-sampling estimate, unchanged
    queries = torch.from_numpy(synth.uniform_rotations(300, seed=8)).cuda()
    a = harness.pose_accuracy(fl, feat, gt, queries=queries)
    b = harness.pose_accuracy(fl, feat, gt, queries=queries, method="log_inv")
    est, _ = harness.estimate_rotations(fl, feat, queries=queries)
    assert torch.equal(a["est_rotation"], est) and torch.equal(b["est_rotation"], est) and a["acc"] == b["acc"]
    with pytest.raises(ValueError):
        harness.pose_accuracy(fl, feat, gt, method="sample")


def test_offset_is_drawn_from_torch_and_returned():
    _, _, fl = _flow(seed=10)
    feat = torch.from_numpy(synth.features(2, 32, seed=7)).cuda()
    torch.manual_seed(123)
    est, best, index, O = harness.grid_estimate_rotations(fl, feat, recursion_level=1)
    assert torch.allclose(O @ O.T, torch.eye(3, device=O.device), atol=1e-5) and abs(float(torch.det(O)) - 1) < 1e-5
    again = harness.grid_estimate_rotations(fl, feat, recursion_level=1, offset=O)
    assert torch.equal(again[2], index) and torch.equal(again[1], best) and torch.equal(again[0], est)
    torch.manual_seed(123)
    assert torch.equal(harness.grid_estimate_rotations(fl, feat, recursion_level=1)[3], O)
