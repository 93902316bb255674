"""From rotations back to the cells of the SO(3) grid (rnf_so3_grid_locate: sd.grid_index / grid_histogram) and the fit of a histogram
against a grid density (rnf_grid_fit: harness.grid_fit / grid_pose_fit) on the device: round trips through the device's own grid and its
hierarchy, the fp64 restatements of tests/test_so3_locate_host.py, the poles and non-finite rows, the histogram's arithmetic, the fit's
tolerances and edge cases, determinism and grouping, the flow end to end, and the statistics on a known density and a trained flow."""
import functools

import numpy as np
import pytest
import torch

from rotationnormflow_amd import grid_pose, harness, synth
from rotationnormflow_amd.utils import sd
from rotationnormflow_amd.utils.fisher import MatrixFisherN
from tests.test_gpu_grid_pose import _fisher_rows, _flow, _offset
from tests.test_grid_credible_host import case_seed, numpy_grid, synthetic_logp
from tests.test_so3_locate_host import fit_edge_rows, grid_fit_fp64, grid_locate_fp64, multinomial_counts, pole_cases
from tests.trained_helpers import load_trained

pytestmark = pytest.mark.gpu

FLOATS = ("log_norm", "log_likelihood", "grid_log_likelihood", "g_stat", "chi2", "kl", "z")
MARGIN = 1e-9                                         # of the restatement: a million times the rounding of its fp64 arithmetic


def _same(a, b):
    """bit-equal, NaN where NaN"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


def _same_fit(a, b, rows=slice(None)):
    return all(_same(a[k][rows], b[k]) for k in FLOATS + ("n", "occupied")) and a["dof"] == b["dof"]


@functools.lru_cache(maxsize=None)
def _random_rotations(n, seed):
    return synth.uniform_rotations(n, seed=seed).astype(np.float32)


# ---- locate -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
def test_every_row_of_the_device_grid_is_located_in_its_own_cell(level):
    want = torch.arange(sd.grid_size(level), device="cuda")
    assert torch.equal(sd.grid_index(sd.generate_healpix_grid(level, device="cuda"), level), want)
    O = _offset(level + 1).cuda()
    rows = sd.grid_index(sd.generate_healpix_grid(level, device="cuda", offset=O), level, O)
    assert rows.dtype == torch.int64 and torch.equal(rows, want)


@pytest.mark.parametrize("level", [4, 5, 6, 7])
def test_children_are_located_one_level_down(level):
    rng = np.random.default_rng(level)
    parents = torch.from_numpy(rng.integers(0, sd.grid_size(level), 3000)).cuda()
    O = _offset(level + 2).cuda()
    rows, rot = harness.grid_children(parents, level, O)
    assert rows.shape == (36000,) and torch.equal(sd.grid_index(rot, level + 1, O), rows)


@pytest.mark.parametrize("level", [0, 3, 8])
def test_rows_of_random_rotations_equal_the_restatement(level):
    R = _random_rotations(1 << 18, 101)
    O = _offset(level + 3)
    want, margin = grid_locate_fp64(level, R, O)
    got = sd.grid_index(torch.from_numpy(R).cuda(), level, O.cuda()).cpu().numpy()
    keep = margin >= MARGIN
    print(f"level {level}: smallest margin {margin.min():.2e}, {int((~keep).sum())} of {R.shape[0]} rows left out, "
          f"{int((got != want).sum())} rows differ")
    assert (~keep).mean() <= 1e-5
    assert np.array_equal(got[keep], want[keep])
    assert got.min() >= 0 and got.max() < sd.grid_size(level)
    shaped = sd.grid_index(torch.from_numpy(R[:60]).cuda().reshape(3, 4, 5, 3, 3), level, O.cuda())           # [...] in, [...] out
    assert shaped.shape == (3, 4, 5) and np.array_equal(shaped.reshape(-1).cpu().numpy(), got[:60])


@pytest.mark.parametrize("level", [0, 1, 3])
def test_poles_and_non_finite_rows(level):
    cases = pole_cases()
    R = torch.from_numpy(np.stack([c[1] for c in cases]).astype(np.float32)).cuda()
    assert sd.grid_index(R, level).tolist() == [c[2](level) for c in cases]
    bad = torch.from_numpy(_random_rotations(6, 7).copy()).cuda()
    bad[1, 2, 1] = float("nan")
    bad[3, 0, 0] = float("inf")
    bad[4, 1, 2] = float("-inf")
    rows = sd.grid_index(bad, level, _offset(2).cuda())
    assert rows[[1, 3, 4]].tolist() == [-1, -1, -1] and bool((rows[[0, 2, 5]] >= 0).all())
    assert sd.grid_index(torch.empty(0, 3, 3, device="cuda"), level).shape == (0,)
    assert int(sd.grid_histogram(torch.empty(2, 0, 3, 3, device="cuda"), level).sum()) == 0


# ---- histogram ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 3])
def test_histogram_equals_the_bincount_of_the_restatement(level):
    g, n, Q = 3, 50_000, sd.grid_size(level)
    R = _random_rotations(g * n, 202).reshape(g, n, 3, 3).copy()
    R[1, 17, 0, 0] = np.nan                                # rows of -1 are not counted
    R[2, 40_000, 2, 2] = np.inf
    O = _offset(level + 4)
    want, margin = grid_locate_fp64(level, R.reshape(-1, 3, 3), O)
    assert margin.min() >= MARGIN                          # of the restatement alone: none of these rows is in doubt
    want = want.reshape(g, n)
    ref = np.stack([np.bincount(want[b][want[b] >= 0], minlength=Q) for b in range(g)])
    Rd = torch.from_numpy(R).cuda()
    counts = sd.grid_histogram(Rd, level, O.cuda())
    assert counts.dtype == torch.int32 and counts.shape == (g, Q) and np.array_equal(counts.cpu().numpy(), ref)
    assert counts.sum(1).tolist() == [n, n - 1, n - 1]
    assert torch.equal(sd.grid_histogram(Rd, level, O.cuda()), counts)                        # two runs, bit-equal
    out = counts.clone()
    assert sd.grid_histogram(Rd, level, O.cuda(), out=out) is out and torch.equal(out, 2 * counts)
    one = sd.grid_histogram(Rd[2], level, O.cuda())                                           # [n,3,3]: one image
    assert one.shape == (1, Q) and torch.equal(one[0], counts[2])
    with pytest.raises(ValueError, match="out"):
        sd.grid_histogram(Rd, level, O.cuda(), out=torch.zeros(g, Q, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        sd.grid_histogram(Rd, level, O.cuda(), out=torch.zeros(g, Q + 1, dtype=torch.int32, device="cuda"))


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fit_case(level, g):
    """(lp float32 [2g,Q], counts int32 [2g,Q]): g synthetic rows with multinomial counts of n = 10 Q from the row's own masses, then the
    same rows with counts from flat masses."""
    lp = synthetic_logp(numpy_grid(level), g, seed=case_seed(level, g))
    Q = lp.shape[1]
    rng = np.random.default_rng(case_seed(level, g) + 1)
    own = np.stack([multinomial_counts(lp[b], 10 * Q, rng) for b in range(g)])
    flat = np.stack([multinomial_counts(np.zeros(Q), 10 * Q, rng) for b in range(g)])
    return np.concatenate([lp, lp]), np.concatenate([own, flat])


def _check_fit(got, ref, rows):
    """The tolerances that the one fp32 step allows: expf to 2^-20 relative (as eps_for of tests/test_grid_credible_host.py) moves log Z,
    hence log_norm and every log p_i, by at most 2^-19 absolute -- 2e-6 with the fp64 rounding of the sums; g_stat = 2 sum c_i (...)
    then by at most n 2^-18; every term of chi2 + n = sum c_i^2 / (n p_i) by at most 2^-18 relative."""
    n = ref["n"][rows].astype(np.float64)
    for k in ("log_norm", "log_likelihood", "grid_log_likelihood"):
        err = np.abs(got[k].cpu().numpy()[rows] - ref[k][rows]).max()
        print(f"{k}: max abs error {err:.2e}")
        assert err <= 2e-6, k
    g_err = np.abs(got["g_stat"].cpu().numpy()[rows] - ref["g_stat"][rows]) / n
    c_err = np.abs(got["chi2"].cpu().numpy()[rows] - ref["chi2"][rows]) / (ref["chi2"][rows] + n)
    print(f"g_stat: max error / n {g_err.max():.2e} (bound {2.0 ** -18:.2e}); chi2 + n: max relative error {c_err.max():.2e}")
    assert np.all(g_err <= 2.0 ** -18) and np.all(c_err <= 2.0 ** -18)
    assert np.array_equal(got["n"].cpu().numpy()[rows], ref["n"][rows]) and np.array_equal(got["occupied"].cpu().numpy()[rows], ref["occupied"][rows])


@pytest.mark.parametrize("level,g", [(1, 5), (2, 3), (3, 2)])
def test_fit_equals_the_restatement(level, g):
    lp, counts = _fit_case(level, g)
    Q = lp.shape[1]
    lpd, cd = torch.from_numpy(lp).cuda(), torch.from_numpy(counts).cuda()
    got = harness.grid_fit(lpd, cd)
    ref = grid_fit_fp64(lp, counts)
    assert all(got[k].dtype == torch.float64 and got[k].shape == (2 * g,) for k in FLOATS)
    assert got["n"].dtype == torch.int64 and got["occupied"].dtype == torch.int64 and got["dof"] == Q - 1
    _check_fit(got, ref, np.arange(2 * g))
    assert bool((got["n"] == 10 * Q).all())
    assert torch.equal(got["kl"], got["g_stat"] / (2.0 * got["n"].double())) and torch.equal(got["z"], (got["g_stat"] - (Q - 1)) / np.sqrt(2.0 * (Q - 1)))
    # counts drawn from the row's own masses fit it, flat ones do not.  (These rows are peaked: most cells expect far less than one sample,
    # so kl lies below (Q - 1) / (2 n) and z reads nothing here -- the chi-square limit needs a few samples per cell.)
    print(f"kl: own masses {got['kl'][:g].tolist()}, flat masses {got['kl'][g:].tolist()}")
    assert bool((got["kl"][:g] < 0.05).all()) and bool((got["kl"][g:] > 1).all())
    grid = sd.generate_healpix_grid(level, device="cuda")
    assert float((got["log_norm"] - harness.grid_modes(lpd, grid, 1, np.pi)[3].double()).abs().max()) <= 1e-6
    again = harness.grid_fit(lpd, cd)                                                          # run to run, and g = 1 per call
    assert _same_fit(got, again)
    for b in range(2 * g):
        assert _same_fit(got, harness.grid_fit(lpd[b:b + 1], cd[b:b + 1]), slice(b, b + 1)), b


def test_fit_on_ragged_sizes_and_many_blocks():
    """Q a multiple of neither the 256-row tile nor a block's 8192 rows, one cell, and level 5's 288 blocks per image."""
    rng = np.random.default_rng(12)
    for Q, g in [(1, 2), (255, 3), (30001, 2), (sd.grid_size(5), 1)]:
        lp = (rng.standard_normal((g, Q)) * 2.0).astype(np.float32)
        counts = np.stack([multinomial_counts(lp[b], 4 * Q + 3, rng) for b in range(g)])
        got = harness.grid_fit(torch.from_numpy(lp).cuda(), torch.from_numpy(counts).cuda())
        _check_fit(got, grid_fit_fp64(lp, counts), np.arange(g))


def test_fit_edge_cases_on_the_device():
    lp, c = fit_edge_rows()
    lp = np.concatenate([lp, np.full((1, 8), -np.inf)])
    c = np.concatenate([c, c[:1]])
    got = harness.grid_fit(torch.from_numpy(lp.astype(np.float32)).cuda(), torch.from_numpy(c.astype(np.int32)).cuda())
    r = {k: v.cpu().numpy() for k, v in got.items() if k != "dof"}
    ref = grid_fit_fp64(lp.astype(np.float32), c)
    _check_fit(got, ref, np.array([0]))                    # a -inf cell without samples contributes nothing
    for b in (1, 2):                                       # a sample in a -inf cell, and in one whose weight underflowed
        assert r["log_likelihood"][b] == -np.inf and r["grid_log_likelihood"][b] == -np.inf
        assert r["g_stat"][b] == np.inf and r["chi2"][b] == np.inf and r["kl"][b] == np.inf and r["z"][b] == np.inf
        assert abs(r["log_norm"][b] - ref["log_norm"][b]) <= 2e-6
    for b in (3, 4):                                       # a NaN, a +inf maximum
        assert all(np.isnan(r[k][b]) for k in FLOATS) and r["n"][b] == 22 and r["occupied"][b] == 7
    assert abs(r["log_norm"][5] - ref["log_norm"][5]) <= 2e-6 and r["n"][5] == 0 and r["occupied"][5] == 0      # no samples
    assert all(np.isnan(r[k][5]) for k in FLOATS[1:])
    assert r["log_norm"][6] == -np.inf and r["log_likelihood"][6] == -np.inf and r["g_stat"][6] == np.inf and r["chi2"][6] == np.inf
    alone = harness.grid_fit(torch.from_numpy(lp[:1].astype(np.float32)).cuda(), torch.from_numpy(c[:1].astype(np.int32)).cuda())
    assert _same_fit(got, alone, slice(0, 1))              # the bad images leave the good one alone


# ---- the flow end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conditional,with_base", [(True, False), (True, True), (False, False), (False, True)])
def test_pose_fit_equals_the_fit_of_the_materialised_density(conditional, with_base):
    level, n = 2, 3000
    Q = sd.grid_size(level)
    if conditional:
        _, _, fl = _flow()
        B = 4
        feat = torch.from_numpy(synth.features(B, 32, seed=2)).cuda()
    else:
        _, _, fl = _flow(seed=2, layers=3)
        B, feat = (3 if with_base else 1), None
    base = _fisher_rows(B, seed=4) if with_base else None
    samples = torch.from_numpy(_random_rotations(B * n, 303).reshape(B, n, 3, 3)).cuda()
    if B == 1:
        samples = samples[0]                                # [n,3,3] for one image
    O = _offset(6).cuda()
    out = harness.grid_pose_fit(fl, feat, samples=samples, recursion_level=level, offset=O, base=base)
    grid = sd.generate_healpix_grid(level, device="cuda", offset=O)
    with torch.no_grad():
        lp = fl.log_prob(grid.repeat(B, 1, 1), feat, base=base, feature_repeat=Q if feat is not None else None)["logp"].reshape(B, Q)
    counts = sd.grid_histogram(samples, level, O)
    want = harness.grid_fit(lp, counts)
    assert _same_fit(out, want) and torch.equal(out["counts"], counts) and torch.equal(out["offset"], O)
    assert bool((out["n"] == n).all()) and bool(torch.isfinite(out["kl"]).all())
    for ipl in (1, 3):
        assert _same_fit(out, harness.grid_pose_fit(fl, feat, samples=samples, recursion_level=level, offset=O, base=base,
                                                    images_per_launch=ipl)), ipl
    with pytest.raises(ValueError, match="images"):
        harness.grid_pose_fit(fl, feat, samples=torch.zeros(B + 1, 5, 3, 3, device="cuda"), recursion_level=level)


def test_pose_fit_draws_the_flows_own_samples_in_budgeted_launches(monkeypatch):
    _, _, fl = _flow()
    B, n = 3, 5000
    feat = torch.from_numpy(synth.features(B, 32, seed=2)).cuda()
    monkeypatch.setattr(grid_pose, "GRID_LAUNCH_ROWS", 4608)                                  # 1536 samples per image and launch: 4 launches
    torch.manual_seed(3)
    for base in (None, _fisher_rows(B, seed=4), _fisher_rows(1, seed=4)):
        out = harness.grid_pose_fit(fl, feat, n_samples=n, recursion_level=1, offset=_offset(6), base=base)
        assert out["counts"].shape == (B, 576) and out["counts"].sum(1).tolist() == [n] * B and out["n"].tolist() == [n] * B
        uniform = harness.grid_pose_fit(fl, feat, samples=sd.random_rotations(B * n, device="cuda").reshape(B, n, 3, 3), recursion_level=1,
                                        offset=out["offset"], base=base)
        assert _same(out["log_norm"], uniform["log_norm"])
        if base is not None:                                # a peaked base: the flow's own samples fit its density, uniform ones do not
            assert bool((out["kl"] < uniform["kl"]).all())
    _, _, lu = _flow(seed=5, layers=2, condition=1, feature_dim=16, lu=1)                     # batch-coupled: one image per launch
    feat = torch.from_numpy(synth.features(2, 16, seed=6)).cuda()
    out = harness.grid_pose_fit(lu, feat, n_samples=2000, recursion_level=1, offset=_offset(4))
    assert out["counts"].sum(1).tolist() == [2000, 2000]
    with pytest.raises(ValueError):
        harness.grid_pose_fit(lu, feat, n_samples=100, recursion_level=1, images_per_launch=2)


# ---- statistics: conditions, not measured gates ---------------------------------------------------------------------------------------------
def test_samples_of_a_known_density_fit_it_better_than_others():
    """An exact matrix-Fisher with proper singular values (3, 2, 1) at level 2, n = 2^20: its own samples against Haar-uniform ones and
    against samples of the same Fisher turned by 30 degrees.  The sampling floor of kl is (Q - 1) / (2 n) = 0.0022 nats."""
    level, n = 2, 1 << 20
    U, V = synth.uniform_rotations(2, seed=71).astype(np.float64)
    A = torch.from_numpy((U @ np.diag([3.0, 2.0, 1.0]) @ V.T).astype(np.float32)).cuda()[None]
    mf = MatrixFisherN(A, "exact")
    O = _offset(8).cuda()
    grid = sd.generate_healpix_grid(level, device="cuda", offset=O)
    torch.manual_seed(11)
    own = mf.sample(n)[0]
    a = np.deg2rad(30.0)
    turn = torch.tensor([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device="cuda")
    with torch.no_grad():
        lp = mf.log_prob(grid).reshape(1, -1)
    fits = {name: harness.grid_fit(lp, sd.grid_histogram(R, level, O))
            for name, R in (("own", own), ("uniform", sd.random_rotations(n, device="cuda")), ("turned", turn @ own))}
    for name, f in fits.items():
        print(f"{name}: kl {float(f['kl']):.5f} nats, z {float(f['z']):.2f}, grid_log_likelihood {float(f['grid_log_likelihood']):.5f}, "
              f"log_norm {float(f['log_norm']):.2e}, occupied {int(f['occupied'])}")
    assert float(fits["own"]["kl"]) < float(fits["turned"]["kl"]) and float(fits["own"]["kl"]) < float(fits["uniform"]["kl"])
    assert int(fits["own"]["n"]) == n and abs(float(fits["own"]["log_norm"])) < 0.05


def test_a_trained_flows_samples_fit_its_density_better_than_uniform_ones():
    cfg, ckpt, _, _, _ = load_trained("trained_c1")
    fl = harness.build_flow_from_checkpoint(cfg, ckpt)
    torch.manual_seed(5)
    own = harness.grid_pose_fit(fl, None, n_samples=1 << 18, recursion_level=2, offset=_offset(9))
    uni = harness.grid_pose_fit(fl, None, samples=sd.random_rotations(1 << 18, device="cuda"), recursion_level=2, offset=own["offset"])
    for name, f in (("own", own), ("uniform", uni)):
        print(f"trained_c1 {name}: kl {float(f['kl']):.5f} nats, z {float(f['z']):.2f}, grid_log_likelihood "
              f"{float(f['grid_log_likelihood']):.5f}, log_norm {float(f['log_norm']):.4f}, occupied {int(f['occupied'])}")
    assert int(own["n"]) == 1 << 18 and _same(own["log_norm"], uni["log_norm"])
    assert float(own["kl"]) < float(uni["kl"]) and float(own["grid_log_likelihood"]) > float(uni["grid_log_likelihood"])
