"""GPU: rnf_so3_kernel_moments and what is built on it (utils/kde.py so3_kernel_moments, SO3KernelDensity.log_prob with its gradient,
score, mean_shift, modes, sample; harness.kde_modes; grid_pose.grid_modes_refine) against the fp64 restatements, the cases and the gates
of tests/test_so3_moments_host.py (its docstring derives the gates), at the smallest shapes at which the tiles of 64, the chunks of
4096, the blocks of 256 queries and the finalise can go wrong.

Measured on the MI355X: the worst fraction of each gate over test_accuracy_against_the_restatement was 0.28 (log_density), 0.101
(mean), 0.084 (msd, dlogp_dkappa); R.grad used 0.011 of kappa gate_mean; the mean-shift endpoints were at most 0.0216 degrees from the
fp64 restatement's (at most 25 steps; the estimate from the contraction rate of about 0.66 per step is 0.002 degrees, the rest is the
fp32 resolution of an angle near 0); the refined grid modes at most 0.012 degrees from R0.  DESIGN.md 3.3e."""
import functools

import numpy as np
import pytest
import torch

from rotationnormflow_amd import harness
from rotationnormflow_amd.utils import kde, sd
from tests import test_so3_moments_host as hm
from tests.test_gpu_so3_kde import two_mode_log_density, two_mode_sets

pytestmark = pytest.mark.gpu
DEV = "cuda"
KAPPAS = (4.0, 64.0, 16384.0)
SENTINEL = 12345.0


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def gpu_kernel_moments(centres, queries, kappa, log_weights=None, group_queries=False, project=True, **kw):
    """The signature of hm.host_kernel_moments on the device -> dict of numpy arrays with a leading G"""
    lw = dev(log_weights)
    out = kde.so3_kernel_moments(dev(centres), dev(queries), kappa, lw if lw is None or lw.dim() == 2 else lw[None], project=project,
                                 group_queries=group_queries, **kw)
    lead = lw is not None or group_queries
    return {k: (v if lead else v[None]).cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 4095, 4096, 4097, 9000])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("weighted", [False, True])
def test_accuracy_against_the_restatement(n, kind, weighted):
    for m in (1, 65, 1000):
        for kappa in KAPPAS:
            hm.check_case(gpu_kernel_moments, n, m, kind, weighted, kappa, False, "device", KAPPAS)
    for kappa in KAPPAS:
        hm.check_case(gpu_kernel_moments, n, 65, kind, weighted, kappa, True, "device", KAPPAS)
    print("worst fractions of the gates so far:", {k[1]: round(v, 4) for k, v in hm.WORST.items() if k[0] == "device"})


def test_the_library_writes_no_row_behind_the_last():
    """The C entry point on output buffers with sentinel rows behind the last row of every output, at a ragged size"""
    from rotationnormflow_amd import _lib
    Cn, Qr, lw = (dev(x) for x in hm.make_case(4097, 65, "clustered", True))
    G, m = 3, 65
    bufs = {k: torch.full((G * m + 4,) + ((9,) if k in ("mean", "rotation") else ()), SENTINEL, device=DEV) for k in hm.OUTPUTS}
    args = _lib.So3KernelMoments(centres=Cn.data_ptr(), queries=Qr.data_ptr(), log_weights=lw.data_ptr(), n=4097, m=m, G=G, kappa=64.0,
                                 **{k: v.data_ptr() for k, v in bufs.items()})
    _lib.call("so3_kernel_moments", args, Cn.device)
    torch.cuda.synchronize()
    want = kde.so3_kernel_moments(Cn, Qr, 64.0, lw, project=True)
    for k, v in bufs.items():
        assert (v[G * m:] == SENTINEL).all(), k
        assert torch.equal(torch.nan_to_num(v[:G * m].reshape(want[k].shape)), torch.nan_to_num(want[k])), k


def test_log_density_is_the_kernel_sums_bit_for_bit():
    for n, m, kind, weighted in ((4097, 1000, "clustered", True), (9000, 65, "uniform", False), (63, 1, "uniform", True)):
        Cn, Qr, lw = (dev(x) for x in hm.make_case(n, m, kind, weighted))
        for kappa in (0.0,) + KAPPAS:
            assert torch.equal(kde.so3_kernel_moments(Cn, Qr, kappa, lw)["log_density"], kde.so3_kernel_log_density(Cn, Qr, kappa, lw)), (n, kappa)


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in hm.OUTPUTS + ("dlogp_dkappa",))


def test_bit_identical_from_run_to_run_and_however_the_call_is_tiled():
    Cn, Qr, lw = hm.make_case(4097, 1000, "clustered", True)
    whole = gpu_kernel_moments(Cn, Qr, 64.0, lw)
    assert same(whole, gpu_kernel_moments(Cn, Qr, 64.0, lw))
    for step in (64, 937):
        parts = [gpu_kernel_moments(Cn, Qr[i:i + step], 64.0, lw) for i in range(0, 1000, step)]
        assert same(whole, {k: np.concatenate([p[k] for p in parts], axis=1) for k in whole}), step
    assert same({k: v[:, ::-1] for k, v in whole.items()}, gpu_kernel_moments(Cn, Qr[::-1], 64.0, lw))
    assert same({k: v[2:] for k, v in whole.items()}, gpu_kernel_moments(Cn, Qr, 64.0, lw[2:]))      # group 2 of G = 3 in a call of its own
    assert same(whole, gpu_kernel_moments(Cn, np.stack([Qr] * 3), 64.0, lw, True))                   # the same queries given per group
    rolled = gpu_kernel_moments(Cn, hm.group_sets(Qr, 3), 64.0, lw, True)
    for g in range(3):
        assert all(np.array_equal(np.roll(whole[k][g], 7 * g, axis=0), rolled[k][g], equal_nan=True) for k in hm.OUTPUTS), g
    # the Python tiling, forced by a small cap: queries in tiles, then groups too; shared queries and queries per group
    for cap in (1 << 20, 1 << 12):
        assert same(whole, gpu_kernel_moments(Cn, Qr, 64.0, lw, workspace_cap=cap)), cap
        assert same(rolled, gpu_kernel_moments(Cn, hm.group_sets(Qr, 3), 64.0, lw, True, workspace_cap=cap)), cap


def test_blocks_of_one_wave_and_of_four_give_the_same_bits():
    """The pairwise pass runs blocks of 64 threads while blocks of 256 would number fewer than 1024 (csrc/so3_kernel_moments.h
    block_for), which covers every other case of this file: here 70,001 queries x 4 groups make 274 x 4 = 1096 blocks of 256, and the
    same queries in calls of 9,000 (36 x 4 blocks) take the other path.  The large call is also held to the restatement."""
    Cn, _, _ = hm.make_case(65, 1, "clustered", False)
    Qr = hm.draw("clustered", 70001, 31)
    lw = (2.0 * np.random.default_rng(32).standard_normal((4, 65))).astype(np.float32)
    whole = gpu_kernel_moments(Cn, Qr, 64.0, lw)
    parts = [gpu_kernel_moments(Cn, Qr[i:i + 9000], 64.0, lw) for i in range(0, 70001, 9000)]
    assert same(whole, {k: np.concatenate([p[k] for p in parts], axis=1) for k in whole})
    ref = hm.kernel_moments_fp64(Cn, Qr, 64.0, lw)
    assert (np.abs(whole["mean"] - ref["mean"]).max(axis=(2, 3)) <= ref["gate_mean"]).all()
    assert (np.abs(whole["msd"] - ref["msd"]) <= ref["gate_msd"]).all()
    assert (np.abs(whole["log_density"] - ref["log_density"]) <= hm.gate(ref["E"])).all()


def test_edge_cases():
    hm.check_edge_cases(gpu_kernel_moments)
    Cn = dev(hm.draw("uniform", 5, 1))
    out = kde.so3_kernel_moments(Cn, torch.empty(0, 3, 3, device=DEV), 4.0, project=True)           # m = 0 is a no-op
    assert tuple(out["mean"].shape) == (0, 3, 3) and tuple(out["step"].shape) == (0,) and out["dlogp_dkappa"].dtype == torch.float64
    with pytest.raises(ValueError, match="queries"):
        kde.so3_kernel_moments(Cn, Cn[None].expand(2, 5, 3, 3), 4.0)     # queries per group without group_queries
    with pytest.raises(ValueError, match="groups"):
        kde.so3_kernel_moments(Cn, Cn[None].expand(2, 5, 3, 3).contiguous(), 4.0, torch.zeros(3, 5, device=DEV), group_queries=True)


def test_output_ranks_follow_the_log_weights():
    Cn, Qr, lw = (dev(x) for x in hm.make_case(70, 33, "uniform", True))
    f = kde.so3_kernel_moments
    full = f(Cn, Qr, 64.0, lw, project=True)
    assert {k: tuple(v.shape) for k, v in full.items()} == dict(log_density=(3, 33), mean=(3, 33, 3, 3), msd=(3, 33), rotation=(3, 33, 3, 3),
                                                                step=(3, 33), dlogp_dkappa=(3, 33))
    one = f(Cn, Qr, 64.0, lw[2], project=True)
    assert all(torch.equal(torch.nan_to_num(one[k]), torch.nan_to_num(full[k][2])) for k in full)
    assert set(f(Cn, Qr, 64.0)) == {"log_density", "mean", "msd", "dlogp_dkappa"} and tuple(f(Cn, Qr, 64.0)["mean"].shape) == (33, 3, 3)


def test_graph_capture_replays_the_eager_result():
    Cn, Qr, lw = (dev(x) for x in hm.make_case(4097, 300, "clustered", True))

    def step():
        out = kde.so3_kernel_moments(Cn, Qr, 64.0, lw, project=True)
        return [out[k] for k in hm.OUTPUTS]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(2):
        for t in out:
            t.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) for a, b in zip(out, eager))


# ---- the estimate ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kappa", [4.0, 64.0, 16384.0])
def test_log_prob_carries_its_gradient_and_the_score(kappa):
    (Cn, Qr, lw), refs = hm.references(4097, 65, "clustered", True, KAPPAS, False)
    ref = refs[kappa]
    est = kde.SO3KernelDensity(dev(Cn), kappa, dev(lw[0]))
    plain = est.log_prob(dev(Qr))
    R = dev(Qr).reshape(5, 13, 3, 3).requires_grad_(True)
    lp = est.log_prob(R)
    assert lp.requires_grad and tuple(lp.shape) == (5, 13) and torch.equal(lp.detach().reshape(-1), plain)       # the same bits
    with torch.no_grad():
        assert not est.log_prob(R).requires_grad
    coef = torch.linspace(0.5, 2.0, 65, device=DEV).reshape(5, 13)
    (lp * coef).sum().backward()
    want = kappa * (ref["mean"][0] - Qr.astype(np.float64))              # the restatement's gradient
    got = (R.grad / coef[..., None, None]).reshape(65, 3, 3).double().cpu().numpy()
    frac = np.abs(got - want).max(axis=(1, 2)) / (kappa * ref["gate_mean"][0])
    print("kappa %g: worst |R.grad - kappa (M - R)| as a fraction of kappa gate_mean %.3f" % (kappa, frac.max()))
    assert tuple(R.grad.shape) == (5, 13, 3, 3) and (frac <= 1.0).all()
    amb = est.score(dev(Qr).reshape(5, 13, 3, 3), frame="ambient")
    assert tuple(amb.shape) == (5, 13, 3, 3) and amb.dtype == torch.float32 and not amb.requires_grad
    assert (np.abs(amb.reshape(65, 3, 3).double().cpu().numpy() - want).max(axis=(1, 2)) <= kappa * ref["gate_mean"][0]).all()
    A = np.swapaxes(Qr.astype(np.float64), 1, 2) @ want
    A = A - np.swapaxes(A, 1, 2)                                         # R^T M - M^T R, times kappa: |entries| of R <= 1, three terms, twice
    body = est.score(dev(Qr), frame="body")
    assert tuple(body.shape) == (65, 3)
    assert (np.abs(body.double().cpu().numpy() - np.stack([A[:, 2, 1], A[:, 0, 2], A[:, 1, 0]], axis=1)).max(axis=1) <= 6 * kappa * ref["gate_mean"][0]).all()
    with pytest.raises(ValueError, match="frame"):
        est.score(dev(Qr), frame="world")


@functools.lru_cache(maxsize=1)
def two_mode_estimate():
    train, _, _, _ = hm.two_mode_reference()
    return kde.SO3KernelDensity(dev(train), 32.0)


def test_mean_shift_reaches_the_restatements_endpoints():
    train, ends, _, _ = hm.two_mode_reference()
    est = two_mode_estimate()
    starts = dev(train[:256])
    rot, lp, converged, taken = est.mean_shift(starts)
    assert tuple(rot.shape) == (256, 3, 3) and converged.dtype == torch.bool and taken.dtype == torch.int32
    assert bool(converged.all()) and int(taken.max()) < 200
    off = hm.angle_deg(rot.double().cpu().numpy(), ends)
    print("mean shift: at most %d steps, worst angle to the fp64 endpoint %.5f degrees" % (int(taken.max()), off.max()))
    assert (off <= 0.05).all()
    assert torch.equal(lp, est.log_prob(rot))
    halves = [est.mean_shift(starts[:128]), est.mean_shift(starts[128:])]            # bit-identical whatever other starts share the call
    for k in range(4):
        assert torch.equal(torch.cat([h[k] for h in halves]), (rot, lp, converged, taken)[k]), k
    again = est.mean_shift(starts, check_every=1)                        # and however often the host looks
    assert torch.equal(again[0], rot) and torch.equal(again[3], taken)
    sharp = kde.SO3KernelDensity(dev(train), 128.0).mean_shift(starts, kappa=32.0)   # the kernel of the search is an argument
    assert torch.equal(sharp[0], rot) and torch.equal(sharp[1], lp)


def test_modes_of_the_two_mode_set():
    train, ends, _, _ = hm.two_mode_reference()
    est = two_mode_estimate()
    out = est.modes(top_k=4, starts=dev(train[:256]))
    got, mass = out["est"].double().cpu().numpy(), out["mass"].double().cpu().numpy()
    assert tuple(out["est"].shape) == (4, 3, 3) and tuple(out["log_prob"].shape) == (4,) and out["converged_fraction"] == 1.0
    assert np.isfinite(got[:2]).all() and np.isnan(got[2:]).all() and (mass[2:] == 0).all() and bool(torch.isnan(out["log_prob"][2:]).all())
    off = [float(hm.angle_deg(got[:2], M).min()) for M in hm.TWO_MODES]
    centres, label = hm.cluster(ends)
    share = np.array([(label == int(np.argmin(hm.angle_deg(centres, g)))).mean() for g in got[:2]])  # the restatement's share of the starts
    print("modes: %.3f and %.3f degrees from the true modes, masses %s (fp64 shares %s)" % (off[0], off[1], mass[:2], share))
    assert max(off) <= 2.0 and abs(mass.sum() - 1.0) <= 1e-6 and (np.abs(mass[:2] - share) <= 1e-6).all()
    assert float(out["log_prob"][0]) >= float(out["log_prob"][1])
    own = est.modes(top_k=2)                                             # 1024 of its own rotations at a stride of 4
    assert np.isfinite(own["est"].cpu().numpy()).all() and abs(float(own["mass"].sum()) - 1.0) <= 1e-6
    assert max(float(hm.angle_deg(own["est"].double().cpu().numpy(), M).min()) for M in hm.TWO_MODES) <= 2.0
    wrapped = harness.kde_modes(dev(train), 32.0, top_k=2)
    assert all(torch.equal(wrapped[k], own[k]) for k in ("est", "log_prob", "mass"))


def test_samples_follow_the_estimate():
    train, test = two_mode_sets()
    est = kde.SO3KernelDensity(dev(train), 128.0)
    torch.manual_seed(5)
    S = est.sample(4096)
    torch.manual_seed(5)
    assert torch.equal(S, est.sample(4096))                              # the same seed, the same bits
    R = S.double().cpu().numpy()
    assert tuple(S.shape) == (4096, 3, 3) and S.dtype == torch.float32
    assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= 16 * 2.0 ** -23 and (np.linalg.det(R) > 0).all()
    drawn, held = float(two_mode_log_density(R).mean()), float(two_mode_log_density(test).mean())
    print("mean true log-density: %.4f over the samples, %.4f over the held-out draws" % (drawn, held))
    assert abs(drawn - held) <= 0.15
    lw = torch.full((4096,), -float("inf"), device=DEV)
    lw[7] = 0.0                                                          # all of the mass on one centre: every sample is near it
    near = kde.SO3KernelDensity(dev(train), 128.0, lw).sample(64).double().cpu().numpy()
    assert (hm.angle_deg(near, train[7]) <= 25.0).all()                  # 7 standard deviations of MF(128 I)'s angle per axis


# ---- modes off the grid ------------------------------------------------------------------------------------------------------------------

def test_grid_modes_are_refined_off_the_grid():
    """A level-3 grid posterior 0.6 MF(20 R0) + 0.4 MF(20 R0 Rz(180)) for four R0: the grid arg-max is a grid row, degrees away from R0;
    mean shift on the kernel-smoothed grid posterior at the default kappa brings mode 0 within 0.5 degrees (fp64: 0.33 at most for
    kappa <= 40).  Through the public grid_modes + grid_modes_refine path, which is what grid_pose_modes_refined runs per launch."""
    grid = sd.generate_healpix_grid(recursion_level=3, device=DEV)
    Q = grid.shape[0]
    g64 = grid.double().cpu().numpy()
    R0 = hm.draw("uniform", 4, 5).astype(np.float64)
    R1 = R0 @ np.diag([-1.0, -1.0, 1.0])
    t0 = 20.0 * (np.einsum("qij,bij->bq", g64, R0) - 3.0)
    t1 = 20.0 * (np.einsum("qij,bij->bq", g64, R1) - 3.0)
    logp = dev(np.logaddexp(np.log(0.6) + t0, np.log(0.4) + t1).astype(np.float32))
    index, _, _, _, _ = harness.grid_modes(logp, grid, 3, float(np.deg2rad(15.0)))
    start = grid[index.clamp(min=0)]
    start[index < 0] = float("nan")
    start[1, 2] = float("nan")                                           # a mode that does not exist
    refined, converged = harness.grid_modes_refine(logp, grid, start)
    assert tuple(refined.shape) == (4, 3, 3, 3) and tuple(converged.shape) == (4, 3) and converged.dtype == torch.bool
    before = hm.angle_deg(start[:, 0].double().cpu().numpy(), R0)
    after = hm.angle_deg(refined[:, 0].double().cpu().numpy(), R0)
    second = hm.angle_deg(refined[:, 1].double().cpu().numpy(), R1)
    kappa = 0.5 / (8 * np.pi ** 2 / Q) ** (2.0 / 3.0)
    print("level 3, default kappa %.2f: arg-max %s degrees from R0, refined %s; mode 1 refined %s from R0 Rz(180)" % (kappa, before, after, second))
    assert (before >= 2.0).all() and (after <= 0.5).all() and bool(converged[:, :2].all())
    assert bool(torch.isnan(refined[1, 2]).all()) and not bool(converged[1, 2])
    same_kappa = harness.grid_modes_refine(logp, grid, start, kappa=kappa)
    assert torch.equal(torch.nan_to_num(same_kappa[0]), torch.nan_to_num(refined))
    alone = harness.grid_modes_refine(logp[2:3], grid, start[2:3])       # an image's modes do not depend on the batch
    assert torch.equal(torch.nan_to_num(alone[0]), torch.nan_to_num(refined[2:3]))


def test_grid_pose_modes_refined_runs_the_launches_of_grid_pose_modes():
    """On a flow: the dict of grid_pose_modes bit for bit, plus the refinement of exactly those modes, whatever the images per launch"""
    from rotationnormflow_amd import synth
    from tests.test_gpu_grid_pose import _flow, _offset
    _, _, fl = _flow(seed=13)
    feat = torch.from_numpy(synth.features(3, 32, seed=8)).cuda()
    kw = dict(top_k=4, separation_deg=20.0, recursion_level=2, offset=_offset(6))
    plain = harness.grid_pose_modes(fl, feat, **kw)
    out = harness.grid_pose_modes_refined(fl, feat, **kw)
    assert set(out) == set(plain) | {"refined", "converged"}
    for k, v in plain.items():
        assert torch.equal(torch.nan_to_num(out[k]), torch.nan_to_num(v)), k
    assert tuple(out["refined"].shape) == (3, 4, 3, 3) and tuple(out["converged"].shape) == (3, 4)
    missing = out["index"] < 0
    assert bool(torch.isnan(out["refined"][missing]).all()) and bool(torch.isfinite(out["refined"][~missing]).all())
    assert bool(out["converged"][~missing].all()) and not bool(out["converged"][missing].any())
    R = out["refined"][~missing].double()
    assert float((R.transpose(1, 2) @ R - torch.eye(3, device=DEV, dtype=torch.float64)).abs().max()) <= 2 * hm.ORTH
    one = harness.grid_pose_modes_refined(fl, feat, images_per_launch=1, **kw)
    assert torch.equal(torch.nan_to_num(one["refined"]), torch.nan_to_num(out["refined"])) and torch.equal(one["converged"], out["converged"])
    with pytest.raises(ValueError, match="top_k"):
        harness.grid_pose_modes_refined(fl, feat, top_k=17)
