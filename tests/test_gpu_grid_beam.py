"""Coarse-to-fine beam search over the HEALPix SO(3) grid hierarchy (rnf_so3_grid_children, rnf_grid_beam_select,
harness.grid_beam_estimate_rotations) on the device: children against the numpy rule of tests/test_so3_hierarchy_host.py and, bit for
bit, against the full grid's rows; the selection against a torch restatement; beams that cover every row equal to the full search bit for
bit; consistency with the full grid at level 4; agreement with the full search on trained weights; limits and pose_accuracy."""
import numpy as np
import pytest
import torch

from rotationnormflow_amd import harness, runtime, synth
from rotationnormflow_amd.utils import sd
from tests.test_gpu_grid_pose import _fisher_rows, _flow, _offset
from tests.test_so3_hierarchy_host import children as children_np
from tests.trained_helpers import load_trained

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("with_offset", [False, True])
def test_children_are_the_rows_of_the_full_grid(level, with_offset):
    Q = sd.grid_size(level)
    rng = np.random.default_rng(level)
    parents = np.arange(Q) if Q <= 4608 else np.sort(rng.choice(Q, 3000, replace=False))
    parents = np.concatenate([parents, [-1, Q]])                          # outside the level: children -1
    O = _offset(level + 30).cuda() if with_offset else None
    rows, rot = harness.grid_children(torch.from_numpy(parents).cuda().reshape(1, -1), level, O)
    rows, rot = rows.reshape(-1, 12), rot.reshape(-1, 12, 3, 3)
    want = children_np(level, parents[:-2])
    assert np.array_equal(rows[:-2].cpu().numpy(), want)
    assert bool((rows[-2:] == -1).all())
    full = sd.generate_healpix_grid(level + 1, device="cuda", offset=O)
    assert torch.equal(rot[:-2], full[rows[:-2]])
    assert torch.equal(rot[-2:], full[0].expand(2, 12, 3, 3))           # a missing child carries row 0's rotation
    no_rot, none = harness.grid_children(torch.from_numpy(parents).cuda(), level, O, rotations=False)
    assert none is None and torch.equal(no_rot.reshape(-1, 12), rows)


def test_children_at_level_5_with_offset():
    rng = np.random.default_rng(5)
    parents = rng.choice(sd.grid_size(5), 20000, replace=False)
    O = _offset(17).cuda()
    rows, rot = harness.grid_children(torch.from_numpy(parents).cuda(), 5, O)
    assert np.array_equal(rows.reshape(-1, 12).cpu().numpy(), children_np(5, parents))
    full = sd.generate_healpix_grid(6, device="cuda", offset=O)            # 18.9M rows, 680 MB
    assert torch.equal(rot, full[rows])
    del full


def _select_torch(lp, rows, beam):
    """Restatement: sort every image's candidates by (log p descending with a NaN first, row ascending), keep the first of each row."""
    g, M = lp.shape
    out_r = torch.full((g, beam), -1, dtype=torch.int64)
    out_v = torch.full((g, beam), float("-inf"))
    for b in range(g):
        v, r = lp[b].double(), rows[b]
        ok = r >= 0
        v, r = v[ok], r[ok]
        order = sorted(range(r.numel()), key=lambda i: (0, 0.0, int(r[i])) if torch.isnan(v[i]) else (1, -float(v[i]), int(r[i])))
        seen, k = set(), 0
        for i in order:
            if int(r[i]) in seen:
                continue
            seen.add(int(r[i]))
            out_r[b, k], out_v[b, k] = r[i], lp[b][ok][i]
            k += 1
            if k == beam:
                break
    return out_r, out_v


def _same(a, b):
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


@pytest.mark.parametrize("g,M,beam,implicit", [(3, 50, 8, False), (2, 5000, 16, False), (2, 9000, 64, True), (1, 300, 1, False),
                                               (4, 12, 16, False), (2, 20000, 100, False), (1, 40, 40, True)])
def test_selection_matches_the_torch_restatement(g, M, beam, implicit):
    gen = torch.Generator().manual_seed(g * 1000 + M + beam)
    lp = torch.randn(g, M, generator=gen).round(decimals=1)              # many exact ties
    if implicit:
        rows = torch.arange(M).expand(g, M).contiguous()
    else:
        rows = torch.randint(0, max(2, M // 3), (g, M), generator=gen)   # duplicates, some with different values
        rows[:, ::11] = -1                                               # no candidate
    lp[0, ::13] = float("-inf")
    if M > 20:
        lp[0, 5] = float("nan")
        lp[-1, 17] = float("inf")
    lp = lp.float()
    got_r, got_v = harness.grid_beam_select(lp.cuda(), beam, None if implicit else rows.cuda())
    want_r, want_v = _select_torch(lp, rows, beam)
    assert torch.equal(got_r.cpu(), want_r), (got_r, want_r)
    assert _same(got_v.cpu(), want_v)
    again = harness.grid_beam_select(lp.cuda(), beam, None if implicit else rows.cuda())
    assert torch.equal(again[0], got_r) and _same(again[1], got_v)


def test_selection_of_a_level_4_grid_and_fewer_distinct_rows_than_the_beam():
    Q = sd.grid_size(4)
    gen = torch.Generator().manual_seed(4)
    lp = torch.randn(3, Q, generator=gen)
    lp[1, 100:200] = 10.0                                                # 100-way tie: rows ascending
    for beam in (1, 16, 1024):
        r, v = harness.grid_beam_select(lp.cuda(), beam)
        ref_v, ref_i = torch.sort(-lp.double(), dim=1, stable=True)
        assert torch.equal(r.cpu(), ref_i[:, :beam]) and torch.equal(v.cpu(), lp.gather(1, ref_i[:, :beam]))
    rows = torch.tensor([[5, 5, 3, -1, 3, 9]])
    r, v = harness.grid_beam_select(torch.tensor([[1.0, 2.0, 0.5, 9.0, 0.5, float("-inf")]]).cuda(), 6, rows.cuda())
    assert r.tolist() == [[5, 3, 9, -1, -1, -1]] and v.tolist() == [[2.0, 0.5, float("-inf")] + [float("-inf")] * 3]


def _check_exhaustive(fl, feat, base, L, S, beam, **kw):
    O = _offset(L + 40)
    est, best, index, off = harness.grid_beam_estimate_rotations(fl, feat, recursion_level=L, start_level=S, beam=beam, offset=O,
                                                                 base=base, **kw)
    e0, b0, i0, _ = harness.grid_estimate_rotations(fl, feat, recursion_level=L, offset=O, base=base)
    assert torch.equal(index, i0) and torch.equal(best, b0) and torch.equal(est, e0), (index, i0, best, b0)
    assert torch.equal(off, O.cuda())
    return index


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("precision", ["f16x2", "fp32", "bf16x3"])
def test_exhaustive_beams_equal_the_full_search(precision, with_base):
    old = runtime.get_precision()
    runtime.set_precision(precision)
    try:
        _, _, fl = _flow()
        B = 6
        feat = torch.from_numpy(synth.features(B, 32, seed=12)).cuda()
        base = _fisher_rows(B, seed=13) if with_base else None
        _check_exhaustive(fl, feat, base, 1, 0, 72)                      # every level-0 row kept: children cover level 1
        _check_exhaustive(fl, feat, base, 2, 1, 576)                     # every level-1 row kept: children cover level 2
        assert fl._packed(feat.device).precision == precision
    finally:
        runtime.set_precision(old)


def test_exhaustive_beams_equal_the_full_search_unconditional():
    _, _, fl = _flow(seed=2, layers=3)
    base = _fisher_rows(3, seed=4, scale=10.0)
    _check_exhaustive(fl, None, base, 1, 0, 72)
    _check_exhaustive(fl, None, base, 2, 1, 576)
    _check_exhaustive(fl, None, None, 2, 1, 576)


def test_start_level_equal_to_the_level_is_the_full_search():
    _, _, fl = _flow(seed=4)
    feat = torch.from_numpy(synth.features(3, 32, seed=1)).cuda()
    _check_exhaustive(fl, feat, None, 2, 2, 4)


def test_level_4_estimate_is_a_row_of_the_full_grid_and_does_not_depend_on_grouping():
    _, _, fl = _flow(seed=6)
    B = 5
    feat = torch.from_numpy(synth.features(B, 32, seed=3)).cuda()
    base = _fisher_rows(B, seed=11)
    O = _offset(8)
    runs = [harness.grid_beam_estimate_rotations(fl, feat, recursion_level=4, start_level=2, beam=16, offset=O, base=base,
                                                 images_per_launch=g) for g in (None, 1, 2)]
    est, best, index, _ = runs[0]
    for e, b, i, _ in runs[1:]:
        assert torch.equal(i, index) and torch.equal(b, best) and torch.equal(e, est)
    grid = sd.generate_healpix_grid(4, device="cuda", offset=O)
    with torch.no_grad():
        lp = fl.log_prob(grid.repeat(B, 1, 1), feat, base=base, feature_repeat=grid.shape[0])["logp"].reshape(B, -1)
    assert torch.equal(best, lp.gather(1, index[:, None])[:, 0])
    assert bool((best <= lp.max(-1).values).all())
    assert torch.equal(est, grid[index])


def _trained_rates(name, n_img, L=4, S=2, beam=16):
    cfg, ckpt, w, fx, spec = load_trained(name)
    flow = harness.build_flow_from_checkpoint(cfg, ckpt)
    feat = torch.from_numpy(fx["test_feat"][:n_img]).cuda()
    gt = torch.from_numpy(fx["test_rot"][:n_img]).cuda()
    O = _offset(3)
    e_b, b_b, i_b, _ = harness.grid_beam_estimate_rotations(flow, feat, recursion_level=L, start_level=S, beam=beam, offset=O)
    e_f, b_f, i_f, _ = harness.grid_estimate_rotations(flow, feat, recursion_level=L, offset=O)
    agree = float((i_b == i_f).double().mean())
    err_b = torch.rad2deg(harness.min_geodesic_distance(e_b, gt))
    err_f = torch.rad2deg(harness.min_geodesic_distance(e_f, gt))
    print(f"{name} L={L} start={S} beam={beam}: agreement {agree:.4f} over {n_img} images; median error beam {err_b.median():.2f} deg, "
          f"full {err_f.median():.2f} deg; within 15 deg beam {(err_b <= 15).double().mean():.4f}, full {(err_f <= 15).double().mean():.4f}")
    assert bool((b_b <= b_f).all())
    return agree, err_b, err_f


# measured on one MI355X at L = 4, start 2, beam 16: trained_c4 63 of 64 images (0.984), trained_cond4 256 of 256
@pytest.mark.parametrize("name,n_img,gate", [("trained_c4", 64, 0.95), ("trained_cond4", 256, 0.99)])
def test_trained_weights_agree_with_the_full_search(name, n_img, gate):
    agree, err_b, err_f = _trained_rates(name, n_img)
    assert agree >= gate, agree
    assert (err_b <= 15).double().mean() >= (err_f <= 15).double().mean() - (1 - gate)


def test_limits_and_refusals():
    _, _, fl = _flow(seed=9)
    feat = torch.from_numpy(synth.features(2, 32, seed=5)).cuda()
    bad = [dict(recursion_level=5, start_level=5 + 1), dict(recursion_level=6, start_level=5), dict(recursion_level=9, start_level=2),
           dict(recursion_level=3, start_level=-1), dict(recursion_level=3, beam=0), dict(recursion_level=3, beam=1025),
           dict(recursion_level=2, start_level=3), dict(recursion_level=3, images_per_launch=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            harness.grid_beam_estimate_rotations(fl, feat, **kw)
    _, _, lu = _flow(seed=5, layers=2, condition=1, feature_dim=16, lu=1)            # Condition16TransLU: batch-coupled
    with pytest.raises(ValueError):
        harness.grid_beam_estimate_rotations(lu, torch.from_numpy(synth.features(2, 16, seed=6)).cuda(), recursion_level=2, start_level=1)
    gt = torch.from_numpy(synth.uniform_rotations(2, seed=6)).cuda()
    with pytest.raises(ValueError):
        harness.pose_accuracy(fl, feat, gt, method="log_inv", beam=4)
    with pytest.raises(ValueError):
        harness.pose_accuracy(fl, feat, gt, method="log_pdf", beam=4, top_k=2)


def test_pose_accuracy_with_a_beam():
    _, _, fl = _flow(seed=9)
    B = 4
    feat = torch.from_numpy(synth.features(B, 32, seed=5)).cuda()
    gt = torch.from_numpy(synth.uniform_rotations(B, seed=6)).cuda()
    O = _offset(1)
    est = harness.grid_beam_estimate_rotations(fl, feat, recursion_level=3, start_level=1, beam=8, offset=O)[0]
    pdf = harness.pose_accuracy(fl, feat, gt, method="log_pdf", recursion_level=3, offset=O, beam=8, start_level=1)
    assert torch.equal(pdf["est_rotation"], est)
    assert torch.allclose(pdf["err_deg"], torch.rad2deg(harness.min_geodesic_distance(est, gt)))
    got = harness.pose_accuracy(fl, feat, gt, method="nll_grad", recursion_level=3, offset=O, beam=8, start_level=1, refine_steps=3)
    want = harness.refine_rotations(fl, feat, est, steps=3, lr=1e-4, base=None)
    assert torch.allclose(got["est_rotation"], want, atol=1e-6)
    # without a beam: the whole grid, as before
    full = harness.pose_accuracy(fl, feat, gt, method="log_pdf", recursion_level=3, offset=O)
    assert torch.equal(full["est_rotation"], harness.grid_estimate_rotations(fl, feat, recursion_level=3, offset=O)[0])
