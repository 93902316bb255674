"""GPU: draws from SO(3) grid posteriors (rnf_so3_grid_cell_points, rnf_grid_sample; sd.grid_cell_points, harness.grid_sample /
grid_pose_sample) against the restatements, the host build, the brackets and the cases of tests/test_grid_sample_host.py."""
import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib, harness, synth
from rotationnormflow_amd.utils import sd
from tests.test_gpu_grid_pose import _fisher_rows, _flow
from tests.test_grid_sample_host import (CENTRE_GATE, MARGIN, MAX_SKIPPED, chart_rows_case, check_degenerate, check_draws, check_located,
                                         degenerate_case, density_case, host_cell_points, host_sample, shift_of)
from tests.test_so3_locate_host import grid_locate_fp64

pytestmark = pytest.mark.gpu


def _offset(seed):
    return synth.uniform_rotations(1, seed=seed)[0].astype(np.float32)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_sample(lp, n, level=-1, method="systematic", jitter=True, seed=1, offset=None, draw_base=0, draws_total=None, image_base=0):
    """rnf_grid_sample with every argument and output (the Python entry point always draws one whole set) -> host_sample's dict"""
    lp = _cuda(np.atleast_2d(lp).astype(np.float32)) if not isinstance(lp, torch.Tensor) else lp
    g, Q = lp.shape
    index = torch.full((g, n), -7, dtype=torch.int64, device="cuda")
    target, total = torch.full((g, n), -7, dtype=torch.int64, device="cuda"), torch.full((g,), -7, dtype=torch.int64, device="cuda")
    rot = torch.full((g, n, 3, 3), -7.0, dtype=torch.float32, device="cuda") if level >= 0 else None
    off = _cuda(None if offset is None else np.asarray(offset, np.float32).reshape(9))
    args = _lib.GridSample(logp=lp.data_ptr(), Q=Q, g=g, level=level, draws=n, draw_base=draw_base, draws_total=n if draws_total is None else draws_total,
                           image_base=image_base, method=_lib.GRID_SAMPLE_METHODS[method], jitter=int(jitter), seed=seed,
                           offset=off.data_ptr() if off is not None else None, index_out=index.data_ptr(), target_out=target.data_ptr(),
                           total_out=total.data_ptr(), rot_out=rot.data_ptr() if rot is not None else None)
    _lib.call("grid_sample", args, lp.device)
    return dict(index=index.cpu().numpy(), target=target.cpu().numpy().view(np.uint64), total=total.cpu().numpy().view(np.uint64),
                rot=None if rot is None else rot.cpu().numpy())


def _same(a, b, keys=("index", "target", "total", "rot")):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("level", [0, 1, 2, 3, 6])
def test_device_chart_locates_to_its_row_and_agrees_with_the_host_build(level):
    rows, u = chart_rows_case(level, 70 + level)
    for O in (None, _offset(80 + level)):
        off = _cuda(O)
        rot = sd.grid_cell_points(_cuda(rows), _cuda(u), level, off)
        assert rot.shape == (len(rows), 3, 3) and rot.dtype == torch.float32
        back = sd.grid_index(rot, level, off).cpu().numpy()
        check_located(level, rows, rot.cpu().numpy(), O, (level, O is None))               # the restatement's cells, the margin rule
        _, margin = grid_locate_fp64(level, rot.cpu().numpy(), O)
        safe = margin >= MARGIN
        assert 1.0 - safe.mean() <= MAX_SKIPPED and np.array_equal(back[safe], rows[safe])  # and the device's own
        assert np.abs(rot.cpu().numpy().astype(np.float64) - host_cell_points(level, rows, u, O)).max() <= CENTRE_GATE
    half = torch.full((len(rows), 3), 0.5, device="cuda")
    grid = sd.generate_healpix_grid(level, device="cuda")[_cuda(rows)]
    assert (sd.grid_cell_points(_cuda(rows), half, level) - grid).abs().max().item() <= CENTRE_GATE
    bad = sd.grid_cell_points(_cuda(np.array([-1, sd.grid_size(level), 0, 0], np.int64)),
                              _cuda(np.float32([[.5, .5, .5], [.5, .5, .5], [np.nan, .5, .5], [.5, 1.5, .5]])), level)
    assert torch.isnan(bad).all()
    assert sd.grid_cell_points(torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, 3, device="cuda"), level).shape == (0, 3, 3)


@pytest.mark.parametrize("method", ["systematic", "multinomial"])
def test_device_draws_lie_in_the_bracket_with_exact_targets(method):
    lp = density_case(2, 3, 11)
    seed = 0xC0FFEE1234567
    got = device_sample(lp, 6000, level=2, method=method, seed=seed, image_base=7)
    share, single = check_draws(lp, got, method, seed, 6000, image_base=7, what=method)
    assert share > 0.99
    host = host_sample(lp, 6000, level=2, method=method, seed=seed, image_base=7)
    # the host's expf may differ from the device's in the last place: the totals, hence the targets, need not be equal; the rows are
    # compared where the bracket of the device's target is one row and the host's target has the same bracket
    _, host_single = check_draws(lp, host, method, seed, 6000, image_base=7, what="host")
    both = single & host_single
    if np.array_equal(host["total"], got["total"]):
        assert np.array_equal(host["index"][both], got["index"][both])
    else:
        assert np.mean(host["index"][both] == got["index"][both]) > 0.999


def test_exact_cases_on_the_device():
    for seed in (1, 2 ** 63 + 12345):
        Q = 576
        got = device_sample(np.zeros((1, Q), np.float32), 3 * Q, level=1, seed=seed)
        assert np.array_equal(np.bincount(got["index"][0], minlength=Q), np.full(Q, 3)) and int(got["total"][0]) == Q << shift_of(Q)
        holes = np.zeros((1, Q), np.float32)
        holes[0, 1::2] = -np.inf
        count = np.bincount(device_sample(holes, 3 * (Q // 2), level=1, seed=seed)["index"][0], minlength=Q)
        assert (count[0::2] == 3).all() and (count[1::2] == 0).all()
        one = np.full((1, Q), -np.inf, np.float32)
        one[0, 123] = -4.5
        assert (device_sample(one, 500, level=1, seed=seed, method="multinomial")["index"] == 123).all()
    Q = 3 * 8192 + 17                                       # many blocks, a ragged last chunk
    got = device_sample(np.full((1, Q), 2.5, np.float32), 3 * Q, seed=5)
    assert np.array_equal(np.bincount(got["index"][0], minlength=Q), np.full(Q, 3))
    Q = (1 << 24) + 4099                                    # rows beyond fp32's integers and torch.multinomial's categories
    lp = torch.full((1, Q), -float("inf"), device="cuda")
    lp[0, Q - 5000:] = 1.0
    got = device_sample(lp, 15_000, seed=8)
    assert np.array_equal(np.bincount(got["index"][0] - (Q - 5000), minlength=5000), np.full(5000, 3))
    multi = device_sample(lp, 4000, seed=8, method="multinomial")["index"][0]
    assert multi.min() >= Q - 5000 and multi.max() < Q and len(np.unique(multi)) > 2000


@pytest.mark.parametrize("method", ["systematic", "multinomial"])
def test_device_draws_are_deterministic_and_tile(method):
    lp = _cuda(np.array(density_case(1, 5, 3)))
    O, n = _offset(14), 1000
    whole = device_sample(lp, n, level=1, method=method, seed=77, offset=O)
    assert _same(whole, device_sample(lp, n, level=1, method=method, seed=77, offset=O))              # two runs
    for b0, b1 in ((0, 1), (1, 2), (2, 5)):                                                            # 1 + 1 + 3 images
        part = device_sample(lp[b0:b1], n, level=1, method=method, seed=77, offset=O, image_base=b0)
        assert all(np.array_equal(part[k], whole[k][b0:b1]) for k in ("index", "target", "total", "rot")), (b0, b1)
    for k0, k1 in ((0, 1), (1, 640), (640, 1000)):                                                     # draws in three calls
        part = device_sample(lp, k1 - k0, level=1, method=method, seed=77, offset=O, draw_base=k0, draws_total=n)
        assert all(np.array_equal(part[k], whole[k][:, k0:k1]) for k in ("index", "target", "rot")), (k0, k1)
    plain = device_sample(lp, n, level=1, method=method, seed=77, offset=O, jitter=False)
    grid = sd.generate_healpix_grid(1, device="cuda", offset=_cuda(O)).cpu().numpy()
    assert np.array_equal(plain["index"], whole["index"]) and np.array_equal(plain["rot"], grid[plain["index"]])   # the grid's rows, bit for bit
    back = sd.grid_index(_cuda(whole["rot"]), 1, _cuda(O)).cpu().numpy()
    assert np.mean(back == whole["index"]) >= 1.0 - MAX_SKIPPED


def test_degenerate_images_on_the_device():
    lp = degenerate_case()
    for method in ("systematic", "multinomial"):
        got = device_sample(lp, 300, level=1, method=method, seed=31)
        check_degenerate(lp, got)
        for b in (0, 4):
            alone = device_sample(lp[b:b + 1], 300, level=1, method=method, seed=31, image_base=b)
            assert all(np.array_equal(alone[k][0], got[k][b]) for k in ("index", "target", "total", "rot"))
    out = harness.grid_sample(_cuda(lp), 300, recursion_level=1, seed=31)
    assert (out["index"][1:4] == -1).all() and torch.isnan(out["log_prob"][1:4]).all() and torch.isnan(out["rotations"][1:4]).all()
    assert torch.isfinite(out["log_prob"][0]).all()


def test_python_entry_point_returns_what_the_library_drew():
    lp = density_case(2, 3, 11)
    O = _offset(6)
    dl = _cuda(np.array(lp))
    out = harness.grid_sample(dl, 5000, recursion_level=2, method="multinomial", offset=_cuda(O), seed=123)
    raw = device_sample(lp, 5000, level=2, method="multinomial", seed=123, offset=O)
    assert np.array_equal(out["index"].cpu().numpy(), raw["index"]) and np.array_equal(out["rotations"].cpu().numpy(), raw["rot"])
    assert np.array_equal(out["target"].cpu().numpy().view(np.uint64), raw["target"])
    log_norm = torch.logsumexp(dl.double(), 1, keepdim=True) - np.log(lp.shape[1])
    assert torch.allclose(out["log_prob"].double(), dl.gather(1, out["index"]).double() - log_norm, rtol=2e-7, atol=1e-6)   # the fp32 store
    rows_only = harness.grid_sample(dl, 100, seed=123, method="multinomial")
    assert rows_only["rotations"] is None and torch.equal(rows_only["index"], out["index"][:, :100])
    torch.manual_seed(9)
    a = harness.grid_sample(dl, 64, recursion_level=2)
    torch.manual_seed(9)
    b = harness.grid_sample(dl, 64, recursion_level=2)
    assert torch.equal(a["index"], b["index"]) and torch.equal(a["rotations"], b["rotations"])
    assert not torch.equal(harness.grid_sample(dl, 64, recursion_level=2)["target"], a["target"])       # the generator has moved on


@pytest.mark.parametrize("conditional", [True, False])
def test_grid_pose_sample_equals_grid_sample_of_the_materialised_rows(conditional):
    B, level, n = 3, 2, 500
    if conditional:
        _, _, fl = _flow()
        feat, base = torch.from_numpy(synth.features(B, 32, seed=2)).cuda(), None
    else:
        _, _, fl = _flow(seed=2, layers=3)                   # unconditional: one image per base row
        feat, base = None, _fisher_rows(B)
    O = torch.from_numpy(_offset(5))
    grid = sd.generate_healpix_grid(level, device="cuda", offset=O.cuda())
    Q = grid.shape[0]
    with torch.no_grad():
        lp = fl.log_prob(grid.repeat(B, 1, 1), feat, base=base, feature_repeat=Q if feat is not None else None)["logp"].reshape(B, Q)
    for temperature, method in ((1.0, "systematic"), (2.5, "multinomial")):
        got = harness.grid_pose_sample(fl, feat, n, recursion_level=level, temperature=temperature, method=method, offset=O, base=base, seed=41)
        want = harness.grid_sample(lp / temperature, n, recursion_level=level, method=method, offset=O, seed=41)
        assert all(torch.equal(got[k], want[k]) for k in ("index", "rotations", "target")) and torch.equal(got["offset"], O.cuda())
        assert torch.equal(got["log_prob"], want["log_prob"])
        one = harness.grid_pose_sample(fl, feat, n, recursion_level=level, temperature=temperature, method=method, offset=O, base=base, seed=41,
                                       images_per_launch=1)
        assert all(torch.equal(got[k], one[k]) for k in ("index", "rotations", "target"))
    default = harness.grid_pose_sample(fl, feat, n, recursion_level=level, offset=O, base=base, seed=41)
    unit = harness.grid_pose_sample(fl, feat, n, recursion_level=level, offset=O, base=base, seed=41, temperature=1)
    assert all(torch.equal(default[k], unit[k]) for k in ("index", "rotations", "target", "log_prob"))


def test_jittered_draws_of_a_known_density_fit_it():
    """2^18 jittered multinomial draws of a smooth density at level 1 (455 per cell on average, no cell below 40): binned back into the
    cells they are the multinomial sample of the density the statistic assumes, so z is a standard normal; Haar-uniform rotations against
    the same density are far outside."""
    level, n = 1, 1 << 18
    O = _cuda(_offset(8))
    grid = sd.generate_healpix_grid(level, device="cuda", offset=O)
    A = _cuda((synth.uniform_rotations(1, seed=71)[0].astype(np.float64) @ np.diag([1.0, 0.6, 0.3])).astype(np.float32))
    lp = (grid * A).sum(dim=(1, 2)).reshape(1, -1)          # tr(A^T R): within +-1.9
    out = harness.grid_sample(lp, n, recursion_level=level, method="multinomial", jitter=True, offset=O, seed=2024)
    own = harness.grid_fit(lp, sd.grid_histogram(out["rotations"], level, O))
    uni = harness.grid_fit(lp, sd.grid_histogram(sd.random_rotations(n, device="cuda"), level, O))
    print(f"own: z {float(own['z']):.2f}, kl {float(own['kl']):.5f}; uniform: z {float(uni['z']):.1f}, kl {float(uni['kl']):.5f}")
    assert int(own["n"]) == n and abs(float(own["z"])) < 5
    assert float(uni["z"]) > 100
    counts = torch.bincount(out["index"][0], minlength=grid.shape[0])
    moved = (sd.grid_histogram(out["rotations"], level, O)[0] - counts).abs().sum().item()
    assert moved <= 2 * MAX_SKIPPED * n                     # the jitter keeps a draw in its cell (up to boundary rounding)
