"""GPU: rnf_so3_angle_cdf and what is built on it (utils/angles.py so3_angle_cdf and so3_angle_quantile; grid_pose.grid_error,
grid_pose_error, grid_ball_estimate, grid_pose_ball_estimate) against the fp64 restatement, the cases and the gates of
tests/test_so3_angles_host.py (its docstring states the gates), at the smallest shapes at which the tiles of 64, the chunks of 4096, the
blocks of one wave and of 256 queries, the kernels of 0, 1, 2, 4 and 8 threshold slots and the finalise can go wrong.

Measured on the MI355X: the worst fraction of each gate over test_accuracy_against_the_restatement (n <= 9000, m <= 1000) was 0.996
for the mass (a pair inside the band on the other side: the error is that pair's weight) and 0.102 of 4e-6 ref + 2^-23 beyond the band,
0.343 for mean_angle and 0.343 for mean_sq_angle; per-query thresholds 0.015, 0.059, 0.055.  DESIGN.md 3.3f."""
import numpy as np
import pytest
import torch

from rotationnormflow_amd import harness
from rotationnormflow_amd.utils import angles, sd
from tests import test_so3_angles_host as ha

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.0


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def gpu_angle_cdf(centres, queries, log_weights=None, group_queries=False, thresholds=None, query_tau=None, moments=True, **kw):
    """The signature of ha.host_angle_cdf on the device -> dict of numpy arrays with a leading G"""
    lw = dev(log_weights)
    lead = lw is not None or group_queries
    qt = None
    if query_tau is not None:
        qt = dev(np.asarray(query_tau, np.float32))
        qt = qt if lead else qt[0]
    th = None if thresholds is None else [float(t) for t in np.atleast_1d(thresholds)]
    out = angles.so3_angle_cdf(dev(centres), dev(queries), th, qt, lw if lw is None or lw.dim() == 2 else lw[None], group_queries=group_queries,
                               moments=moments, **kw)
    return {k: (v if lead else v[None]).cpu().numpy() for k, v in out.items() if k != "rms_angle"}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 4095, 4096, 4097, 9000])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("weighted", [False, True])
def test_accuracy_against_the_restatement(n, kind, weighted):
    for m in (1, 65, 1000):
        ha.check_case(gpu_angle_cdf, n, m, kind, weighted, False, "device")
    ha.check_case(gpu_angle_cdf, n, 65, kind, weighted, True, "device")
    print("worst fractions of the gates so far:", {k[1]: round(v, 4) for k, v in ha.WORST.items() if k[0] == "device"})


def test_thresholds_per_query():
    ha.check_query_tau(gpu_angle_cdf, "device")


def test_edge_cases():
    ha.check_edge_cases(gpu_angle_cdf)
    Cn = dev(ha.draw("uniform", 5, 1))
    out = angles.so3_angle_cdf(Cn, torch.empty(0, 3, 3, device=DEV), [0.3, 0.5])                      # m = 0 is a no-op
    assert tuple(out["mass"].shape) == (2, 0) and tuple(out["mean_angle"].shape) == (0,) and tuple(out["rms_angle"].shape) == (0,)
    with pytest.raises(ValueError, match="queries"):
        angles.so3_angle_cdf(Cn, Cn[None].expand(2, 5, 3, 3), [0.3])     # queries per group without group_queries
    with pytest.raises(ValueError, match="groups"):
        angles.so3_angle_cdf(Cn, Cn[None].expand(2, 5, 3, 3).contiguous(), [0.3], None, torch.zeros(3, 5, device=DEV), group_queries=True)
    with pytest.raises(ValueError, match="both"):
        angles.so3_angle_cdf(Cn, Cn, [0.3], torch.zeros(1, 5, device=DEV))
    with pytest.raises(ValueError, match="thresholds"):
        angles.so3_angle_cdf(Cn, Cn, [0.1] * 9)
    with pytest.raises(ValueError, match="threshold 4"):
        angles.so3_angle_cdf(Cn, Cn, [4.0])
    with pytest.raises(ValueError, match="query_tau"):
        angles.so3_angle_cdf(Cn, Cn, None, torch.zeros(1, 4, device=DEV))
    with pytest.raises(ValueError, match="nothing"):
        angles.so3_angle_cdf(Cn, Cn, moments=False)
    with pytest.raises(ValueError, match="workspace_cap"):
        angles.so3_angle_cdf(Cn, Cn, [0.3], workspace_cap=16)
    with pytest.raises(ValueError, match="level"):
        angles.so3_angle_quantile(Cn, Cn, [0.5, 1.0])
    with pytest.raises(ValueError, match="tol"):
        angles.so3_angle_quantile(Cn, Cn, [0.5], tol=0.0)


def test_output_ranks_follow_the_log_weights():
    Cn, Qr, lw = (dev(x) for x in ha.make_case(70, 33, "uniform", True))
    f = angles.so3_angle_cdf
    full = f(Cn, Qr, [0.3, 1.0, 2.0], None, lw)
    assert {k: tuple(v.shape) for k, v in full.items()} == dict(mass=(3, 3, 33), mean_angle=(3, 33), mean_sq_angle=(3, 33), rms_angle=(3, 33))
    one = f(Cn, Qr, [0.3, 1.0, 2.0], None, lw[2])
    assert all(torch.equal(one[k], full[k][2]) for k in full) and tuple(f(Cn, Qr, 0.3)["mass"].shape) == (1, 33)
    assert torch.equal(full["rms_angle"], torch.sqrt(full["mean_sq_angle"])) and set(f(Cn, Qr, 0.3, moments=False)) == {"mass"}
    q = angles.so3_angle_quantile(Cn, Qr, [0.5, 0.9], lw)
    assert {k: tuple(v.shape) for k, v in q.items()} == dict(radius=(3, 2, 33), lo=(3, 2, 33), mass_lo=(3, 2, 33), mass_hi=(3, 2, 33))
    assert q["radius"].dtype == torch.float64 and tuple(angles.so3_angle_quantile(Cn, Qr, 0.5)["radius"].shape) == (1, 33)


def test_the_library_writes_no_row_behind_the_last():
    """The C entry point on output buffers with sentinel rows behind the last row of every output, at a ragged size"""
    import ctypes as C

    from rotationnormflow_amd import _lib
    Cn, Qr, lw = (dev(x) for x in ha.make_case(4097, 65, "clustered", True))
    G, m, T = 3, 65, 5
    th = (C.c_double * T)(*np.deg2rad([5.0, 15.0, 30.0, 90.0, 180.0]))
    bufs = dict(mass=torch.full((G * T * m + 7,), SENTINEL, device=DEV), mean_angle=torch.full((G * m + 7,), SENTINEL, device=DEV),
                mean_sq_angle=torch.full((G * m + 7,), SENTINEL, device=DEV))
    args = _lib.So3AngleCdf(centres=Cn.data_ptr(), queries=Qr.data_ptr(), log_weights=lw.data_ptr(), n=4097, m=m, G=G, T=T,
                            thresholds=C.addressof(th), **{k: v.data_ptr() for k, v in bufs.items()})
    _lib.call("so3_angle_cdf", args, Cn.device)
    torch.cuda.synchronize()
    want = angles.so3_angle_cdf(Cn, Qr, list(th), None, lw)
    for k, v in bufs.items():
        assert (v[-7:] == SENTINEL).all(), k
        assert torch.equal(v[:-7].reshape(want[k].shape), want[k]), k


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ha.OUTPUTS)


def test_bit_identical_from_run_to_run_and_however_the_call_is_tiled():
    Cn, Qr, lw = ha.make_case(4097, 1000, "clustered", True)
    th = np.deg2rad(ha.THRESHOLDS_DEG)
    whole = gpu_angle_cdf(Cn, Qr, lw, thresholds=th)
    assert same(whole, gpu_angle_cdf(Cn, Qr, lw, thresholds=th))
    for step in (64, 937):
        parts = [gpu_angle_cdf(Cn, Qr[i:i + step], lw, thresholds=th) for i in range(0, 1000, step)]
        assert same(whole, {k: np.concatenate([p[k] for p in parts], axis=-1) for k in whole}), step
    assert same({k: v[..., ::-1] for k, v in whole.items()}, gpu_angle_cdf(Cn, Qr[::-1], lw, thresholds=th))
    assert same({k: v[2:] for k, v in whole.items()}, gpu_angle_cdf(Cn, Qr, lw[2:], thresholds=th))      # group 2 of G = 3 in a call of its own
    assert same(whole, gpu_angle_cdf(Cn, np.stack([Qr] * 3), lw, True, thresholds=th))                   # the same queries given per group
    rolled = gpu_angle_cdf(Cn, ha.group_sets(Qr, 3), lw, True, thresholds=th)
    for g in range(3):
        assert all(np.array_equal(np.roll(whole[k][g], 7 * g, axis=-1), rolled[k][g]) for k in ha.OUTPUTS), g
    # however the thresholds are split over calls, shared or per query, with or without the moments
    for a, b in ((0, 1), (1, 3), (3, 8), (0, 4)):
        assert np.array_equal(gpu_angle_cdf(Cn, Qr, lw, thresholds=th[a:b], moments=False)["mass"], whole["mass"][:, a:b]), (a, b)
    tau = np.broadcast_to(ha.tau_of(th)[None, :, None], (3, 8, 1000))
    assert same(whole, gpu_angle_cdf(Cn, Qr, lw, query_tau=tau))
    # the Python tiling, forced by a small cap: queries in tiles, then groups too; shared queries and queries per group
    for cap in (1 << 20, 1 << 12):
        assert same(whole, gpu_angle_cdf(Cn, Qr, lw, thresholds=th, workspace_cap=cap)), cap
        assert same(rolled, gpu_angle_cdf(Cn, ha.group_sets(Qr, 3), lw, True, thresholds=th, workspace_cap=cap)), cap
        assert same(whole, gpu_angle_cdf(Cn, Qr, lw, query_tau=tau, workspace_cap=cap)), cap


def test_blocks_of_one_wave_and_of_four_give_the_same_bits():
    """The pairwise pass runs blocks of 64 threads while blocks of 256 would number fewer than 1024 (csrc/so3_angle_cdf.h block_for),
    which covers every other case of this file.  Queries per group: 70,001 queries x 4 groups make 274 x 4 = 1096 blocks of 256, the
    same queries in calls of 9,000 (36 x 4 blocks) take the other path.  Shared queries and thresholds put the four groups into one
    thread (274 blocks: one wave each), and 262,145 shared queries make 1025 blocks of 256 for that kernel, against calls of 65,536.
    The first call is also held to the restatement."""
    Cn, _, _ = ha.make_case(65, 1, "clustered", False)
    Qr = ha.draw("clustered", 70001, 31)
    lw = (2.0 * np.random.default_rng(32).standard_normal((4, 65))).astype(np.float32)
    th = np.deg2rad([5.2, 15.2, 180.0])
    per = gpu_angle_cdf(Cn, np.broadcast_to(Qr, (4,) + Qr.shape), lw, True, thresholds=th)
    parts = [gpu_angle_cdf(Cn, np.broadcast_to(Qr[i:i + 9000], (4,) + Qr[i:i + 9000].shape), lw, True, thresholds=th) for i in range(0, 70001, 9000)]
    assert same(per, {k: np.concatenate([p[k] for p in parts], axis=-1) for k in per})
    assert same(per, gpu_angle_cdf(Cn, Qr, lw, thresholds=th))                                       # four groups per thread, one wave per block
    big = np.concatenate([Qr, Qr, Qr, Qr[:52142]])                                                   # 262,145 shared queries
    whole = gpu_angle_cdf(Cn, big, lw, thresholds=th)
    assert same({k: v[..., :70001] for k, v in whole.items()}, per)
    parts = [gpu_angle_cdf(Cn, big[i:i + 65536], lw, thresholds=th) for i in range(0, len(big), 65536)]
    assert same(whole, {k: np.concatenate([p[k] for p in parts], axis=-1) for k in whole})
    deg, ref = ha.settle((5.2, 15.2, 180.0), lambda d: ha.angle_cdf_fp64(Cn, Qr, ha.tau_of(np.deg2rad(d)), lw), "n 65 m 70001 x 4 groups")
    ha.check_against(gpu_angle_cdf(Cn, Qr, lw, thresholds=np.deg2rad(deg)), ref, deg, "device-large", "n 65 m 70001 x 4 groups")


def gpu_quantile(Cn, Qr, lw, group_queries=False, **kw):
    def quantile(levels, tol):
        out = angles.so3_angle_quantile(dev(Cn), dev(Qr), list(levels), dev(lw), group_queries=group_queries, tol=tol, **kw)
        return {k: v.cpu().numpy() for k, v in out.items()}
    return quantile


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_quantile_brackets_the_level(kind):
    Cn, Qr, lw = ha.make_case(4097, 65, kind, True)
    out = ha.check_quantile(gpu_quantile(Cn, Qr, lw), ha.restatement_at_angles(Cn, Qr, lw))
    assert out["radius"].shape == (3, 2, 65) and (out["radius"][:, 1] >= out["radius"][:, 0]).all()
    for cap in (1 << 12, None):                                          # tiling gives the same bits, and so does a call of a part
        tiled = gpu_quantile(Cn, Qr, lw, workspace_cap=cap)((0.5, 0.9), 1e-3) if cap else gpu_quantile(Cn, Qr[:16], lw)((0.5, 0.9), 1e-3)
        assert all(np.array_equal(tiled[k], out[k] if cap else out[k][..., :16]) for k in out), cap
    Qg = ha.group_sets(Qr, 3)
    per = ha.check_quantile(gpu_quantile(Cn, Qg, lw, True), ha.restatement_at_angles(Cn, Qg, lw, True))
    assert np.array_equal(per["radius"][0], out["radius"][0]) and np.array_equal(np.roll(out["radius"][2], 14, axis=-1), per["radius"][2])


def test_quantile_is_zero_where_the_query_is_a_centre_that_heavy():
    Cn, Qr, _ = ha.make_case(255, 8, "uniform", False)
    lw = np.zeros((1, 255), np.float32)
    lw[0, 17] = np.log(254.0 * 1.5)                                      # centre 17 carries 0.6 of the mass
    Qr = Qr.copy()
    Qr[3] = Cn[17]
    out = ha.check_quantile(gpu_quantile(Cn, Qr, lw), ha.restatement_at_angles(Cn, Qr, lw))
    assert out["radius"][0, 0, 3] == 0.0 and out["lo"][0, 0, 3] == 0.0 and abs(out["mass_hi"][0, 0, 3] - 0.6) <= 1e-6
    assert out["radius"][0, 1, 3] > 0.0 and (np.delete(out["radius"][0, 0], 3) > 0.0).all()
    Qn = Qr.copy()
    Qn[5, 1, 1] = np.nan                                                 # a query that is not finite has no radius
    bad = gpu_quantile(Cn, Qn, lw)((0.5,), 1e-3)
    assert np.isnan(bad["radius"][0, 0, 5]) and np.isnan(bad["mass_hi"][0, 0, 5]) and np.array_equal(np.delete(bad["radius"][0, 0], 5), np.delete(out["radius"][0, 0], 5))


# ---- grid posteriors ---------------------------------------------------------------------------------------------------------------------

def two_mode_posterior(level, R0, w0=0.6, kappa=20.0):
    """(grid [Q,3,3] on the device, logp [b,Q] float32 numpy, R1): w0 MF(kappa R0) + (1 - w0) MF(kappa R0 Rz(180)) on the level's grid, up
    to the normaliser -- the posterior of tests/test_gpu_so3_moments.py's refinement test"""
    grid = sd.generate_healpix_grid(recursion_level=level, device=DEV)
    g64 = grid.double().cpu().numpy()
    R1 = R0 @ np.diag([-1.0, -1.0, 1.0])
    t0 = kappa * (np.einsum("qij,bij->bq", g64, R0) - 3.0)
    t1 = kappa * (np.einsum("qij,bij->bq", g64, R1) - 3.0)
    return grid, np.logaddexp(np.log(w0) + t0, np.log(1.0 - w0) + t1).astype(np.float32), R1


def test_grid_error_on_a_two_mode_posterior():
    R0 = ha.draw("uniform", 2, 5).astype(np.float64)
    grid, logp, R1 = two_mode_posterior(2, R0)
    gn = grid.cpu().numpy()
    lp = dev(logp)
    index, _, _, _, _ = harness.grid_modes(lp, grid, 2, float(np.deg2rad(40.0)))
    est = torch.cat([grid[index], torch.full((2, 1, 3, 3), float("nan"), device=DEV)], dim=1)       # two modes, and one that does not exist
    en = est[:, :2].cpu().numpy()
    assert (ha.angle_deg(en[:, 0], R0) <= 12.0).all() and (ha.angle_deg(en[:, 1], R1) <= 12.0).all()
    # the thresholds: the level-2 grid has rows exactly 15 and 30 degrees apart (its tilts), so those two move off them by the rule of
    # tests/test_so3_angles_host.py; 180 degrees stays
    deg, ref = ha.settle((15.0, 30.0, 180.0), lambda d: ha.angle_cdf_fp64(gn, en, ha.tau_of(np.deg2rad(d)), logp, True), "grid_error")
    assert all(abs(a - b) < 0.5 for a, b in zip(deg, (15.0, 30.0, 180.0)))
    gt = dev(R0.astype(np.float32))
    out = harness.grid_error(lp, grid, est, thresholds_deg=tuple(deg), levels=(0.5, 0.9), gt=gt)
    assert {k: tuple(v.shape) for k, v in out.items()} == dict(acc=(2, 3, 3), expected_deg=(2, 3), rms_deg=(2, 3), radius_deg=(2, 3, 2),
                                                              error_deg=(2, 3), pit=(2, 3))
    assert all(bool(torch.isnan(v[:, 2]).all()) for v in out.values())                              # the missing mode: NaN rows
    got = dict(mass=out["acc"][:, :2].permute(0, 2, 1).cpu().numpy(), mean_angle=np.deg2rad(out["expected_deg"][:, :2].double().cpu().numpy()),
               mean_sq_angle=np.deg2rad(out["rms_deg"][:, :2].double().cpu().numpy()) ** 2)
    # the restatement first: what the 0.6 / 0.4 split implies
    assert (np.abs(ref["mass"][:, 2] - 1.0) <= 1e-12).all() and ((ref["mass"][:, 1, 0] > 0.5) & (ref["mass"][:, 1, 0] < 0.7)).all()
    assert (np.abs(got["mass"][:, 2] - 1.0) <= 4e-6).all() and ((got["mass"][:, 1, 0] > 0.5) & (got["mass"][:, 1, 0] < 0.7)).all()
    assert ((got["mass"][:, 1, 1] > 0.3) & (got["mass"][:, 1, 1] < 0.5)).all()                      # and 0.4 about mode 1
    err = np.abs(got["mass"] - ref["mass"])
    assert (ref["U"][:, :2] <= ha.U_CAP).all() and (err <= np.where(np.arange(3)[None, :, None] == 2, 0.0, ref["U"]) + 4e-6 * ref["mass"] + 2.0 ** -23).all()
    assert (np.abs(got["mean_angle"] - ref["mean_angle"]) <= ref["gate_mean"] + 1e-7 * ref["mean_angle"]).all()     # + the rounding of degrees
    assert (np.abs(got["mean_sq_angle"] - ref["mean_sq_angle"]) <= ref["gate_sq"] + 4e-7 * ref["mean_sq_angle"]).all()
    # the radii: the restatement's distribution function at the returned brackets, then what the split implies
    q = angles.so3_angle_quantile(grid, est[:, :2], [0.5, 0.9], lp, group_queries=True, tol=float(np.deg2rad(0.05)))
    assert torch.equal(torch.rad2deg(q["radius"]).permute(0, 2, 1).float(), out["radius_deg"][:, :2])
    ha.check_quantile(lambda levels, tol: {k: v.cpu().numpy() for k, v in q.items()}, ha.restatement_at_angles(gn, en, logp, True),
                      tol=float(np.deg2rad(0.05)))
    radius = out["radius_deg"].cpu().numpy()
    assert (radius[:, 0, 1] > 150.0).all() and (radius[:, 0, 0] < 45.0).all() and (radius[:, 1, 0] > 90.0).all()
    # the realised error and its PIT: the mass of the ball about the estimate that just reaches the truth
    want = ha.angle_deg(en, R0[:, None])
    assert (np.abs(out["error_deg"][:, :2].double().cpu().numpy() - want) <= 1e-4).all()
    d2 = ((en.astype(np.float64) - R0[:, None].astype(np.float32).astype(np.float64)) ** 2).sum(axis=(2, 3))
    pit = ha.angle_cdf_fp64(gn, en, d2.astype(np.float32)[:, None, :], logp, True)
    got_pit = out["pit"][:, :2].double().cpu().numpy()
    print("grid_error: acc %s, radius %s, error %s, pit %s (restatement %s, undecided %s)" % (
        got["mass"][:, :, 0], radius[:, 0], want[:, 0], got_pit[:, 0], pit["mass"][:, 0, 0], pit["U"][:, 0, 0]))
    assert (np.abs(got_pit - pit["mass"][:, 0]) <= pit["U"][:, 0] + 4e-6 * pit["mass"][:, 0] + 2.0 ** -23).all()
    assert ((got_pit >= 0) & (got_pit <= 1)).all() and (got_pit[:, 1] > 0.4).all()                  # the ball about mode 1 that reaches the truth holds mode 1's own 0.4
    alone = harness.grid_error(lp[1:], grid, est[1:], thresholds_deg=tuple(deg), gt=gt[1:])          # an image does not depend on the batch
    assert all(torch.equal(torch.nan_to_num(alone[k]), torch.nan_to_num(out[k][1:])) for k in out)
    with pytest.raises(ValueError, match="symmetric"):
        harness.grid_error(lp, grid, est, gt=torch.stack([gt, gt], dim=1))


def test_expected_error_about_a_ground_truth_is_the_spread():
    """expected_deg about a ground truth against IPDF's spread of grid_modes on the same rows: each is held to the fp64 restatement"""
    R0 = ha.draw("uniform", 2, 6).astype(np.float64)
    grid, logp, _ = two_mode_posterior(2, R0)
    lp, gt = dev(logp), dev(R0.astype(np.float32))
    ref = ha.angle_cdf_fp64(grid.cpu().numpy(), gt.cpu().numpy()[:, None], None, logp, True)
    spread = harness.grid_modes(lp, grid, 1, float(np.deg2rad(15.0)), gt[:, None])[4].double().cpu().numpy()
    out = harness.grid_error(lp, grid, gt[:, None], thresholds_deg=(), levels=())
    assert tuple(out["acc"].shape) == (2, 1, 0) and tuple(out["radius_deg"].shape) == (2, 1, 0)
    expected = np.deg2rad(out["expected_deg"][:, 0].double().cpu().numpy())
    print("expected %s rad, spread %s rad, restatement %s" % (expected, spread, ref["mean_angle"][:, 0]))
    assert (np.abs(expected - ref["mean_angle"][:, 0]) <= ref["gate_mean"][:, 0] + 1e-7 * ref["mean_angle"][:, 0]).all()
    assert (np.abs(spread - ref["mean_angle"][:, 0]) <= 1e-4).all()      # the tolerance of tests/test_gpu_grid_modes.py


def test_grid_ball_estimate_prefers_the_broad_mode_to_the_spike():
    """A spike of 3 % of the mass on one grid row plus a broad mode MF(3 R) with the rest, 120 degrees away, as cell masses on the grid
    (a spike narrower than a cell is one row's mass): the arg-max is the spike's row -- the densest row of the broad mode carries about
    1.5 % -- while the ball of 20 degrees with the most mass sits in the broad mode"""
    grid = sd.generate_healpix_grid(recursion_level=2, device=DEV)
    gn = grid.double().cpu().numpy()
    Q = len(gn)
    spike = np.array([100, 2000])
    Rs = gn[spike]
    Rb = Rs @ ha.rodrigues(np.deg2rad(120.0) * np.array([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0]]))
    w = np.exp(3.0 * (np.einsum("qij,bij->bq", gn, Rb) - 3.0))
    w *= 0.97 / w.sum(axis=1, keepdims=True)
    w[np.arange(2), spike] += 0.03
    logp = np.log(w).astype(np.float32)
    lp = dev(logp)
    radius = 20.2
    out = harness.grid_ball_estimate(lp, grid, radius, candidates=256)
    assert {k: tuple(v.shape) for k, v in out.items()} == dict(est=(2, 3, 3), index=(2,), mass=(2,), argmax_index=(2,), argmax_mass=(2,))
    index, top = out["index"].cpu().numpy(), out["argmax_index"].cpu().numpy()
    assert np.array_equal(top, spike) and np.array_equal(top, logp.argmax(axis=1)) and torch.equal(out["est"], grid[out["index"]])
    assert (ha.angle_deg(gn[index], Rb) <= 20.0).all() and (ha.angle_deg(gn[index], Rs) >= 90.0).all()       # a row in the broad mode
    rows = torch.topk(lp, 256, dim=1).indices.cpu().numpy()
    ref = ha.angle_cdf_fp64(gn, np.stack([gn[np.concatenate([[top[b]], rows[b]])] for b in range(2)]), ha.tau_of(np.deg2rad([radius])), logp, True)
    mass, U = ref["mass"][:, 0], ref["U"][:, 0]
    gate = U + 4e-6 * mass + 2.0 ** -23
    assert (U <= ha.U_CAP).all()
    for b in range(2):
        at = 1 + int(np.flatnonzero(rows[b] == index[b])[0])
        assert abs(float(out["mass"][b]) - mass[b, at]) <= gate[b, at] and abs(float(out["argmax_mass"][b]) - mass[b, 0]) <= gate[b, 0]
        assert (mass[b, 1:] - gate[b, 1:] <= mass[b, at] + gate[b, at]).all()          # no candidate's ball is heavier, as far as fp32 can tell
        assert mass[b, at] > 2.0 * mass[b, 0]
    print("grid_ball_estimate: ball mass %s about rows %s, %s about the arg-max rows %s" % (out["mass"].cpu().numpy(), index, out["argmax_mass"].cpu().numpy(), top))
    every, all_rows = harness.grid_ball_estimate(lp, grid, radius, candidates=None), harness.grid_ball_estimate(lp, grid, radius, candidates=Q)
    assert all(torch.equal(every[k], all_rows[k]) for k in every)                          # bit for bit
    assert bool((every["mass"] >= out["mass"]).all()) and torch.equal(every["argmax_mass"], out["argmax_mass"])
    lpn = lp.clone()
    lpn[1, 7] = float("nan")                                             # an image without a posterior has no estimate
    bad = harness.grid_ball_estimate(lpn, grid, radius, candidates=256)
    assert int(bad["index"][1]) == -1 and bool(torch.isnan(bad["est"][1]).all()) and bool(torch.isnan(bad["mass"][1]))
    assert int(bad["index"][0]) == int(index[0]) and torch.equal(bad["mass"][0], out["mass"][0])


def test_grid_pose_error_and_ball_estimate_run_the_launches_of_grid_estimate_rotations():
    from rotationnormflow_amd import synth
    from tests.test_gpu_grid_pose import _flow, _offset
    _, _, fl = _flow(seed=13)
    feat = torch.from_numpy(synth.features(2, 32, seed=8)).cuda()
    kw = dict(recursion_level=1, offset=_offset(6))
    est, best, index, offset = harness.grid_estimate_rotations(fl, feat, **kw)
    gt = dev(ha.draw("uniform", 2, 9))
    out = harness.grid_pose_error(fl, feat, gt_rotation=gt, **kw)
    assert {k: tuple(v.shape) for k, v in out.items()} == dict(acc=(2, 1, 2), expected_deg=(2, 1), rms_deg=(2, 1), radius_deg=(2, 1, 2),
                                                              error_deg=(2, 1), pit=(2, 1), est=(2, 1, 3, 3), index=(2,), log_norm=(2,), offset=(3, 3))
    assert torch.equal(out["index"], index) and torch.equal(out["est"][:, 0], est)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    assert bool(((out["acc"] >= 0) & (out["acc"] <= 1)).all()) and bool((out["acc"][..., 1] >= out["acc"][..., 0]).all())
    assert bool((out["radius_deg"][..., 1] >= out["radius_deg"][..., 0]).all()) and bool((out["rms_deg"] >= out["expected_deg"]).all())
    assert bool(((out["pit"] >= 0) & (out["pit"] <= 1)).all())
    assert (np.abs(out["error_deg"][:, 0].double().cpu().numpy() - ha.angle_deg(est.cpu().numpy(), gt.cpu().numpy())) <= 1e-4).all()
    one = harness.grid_pose_error(fl, feat, gt_rotation=gt, images_per_launch=1, **kw)
    assert all(torch.equal(one[k], out[k]) for k in out)
    modes = harness.grid_pose_modes(fl, feat, top_k=3, separation_deg=60.0, **kw)
    many = harness.grid_pose_error(fl, feat, est=modes["est"], thresholds_deg=(30.0,), levels=(0.5,), **kw)
    assert tuple(many["acc"].shape) == (2, 3, 1) and "pit" not in many and torch.equal(many["acc"][:, 0], harness.grid_pose_error(
        fl, feat, thresholds_deg=(30.0,), levels=(0.5,), **kw)["acc"][:, 0])
    ball = harness.grid_pose_ball_estimate(fl, feat, radius_deg=30.0, candidates=64, **kw)
    assert {k: tuple(v.shape) for k, v in ball.items()} == dict(est=(2, 3, 3), index=(2,), mass=(2,), argmax_index=(2,), argmax_mass=(2,), offset=(3, 3))
    assert torch.equal(ball["argmax_index"], index) and bool((ball["mass"] >= ball["argmax_mass"]).all()) and bool((ball["index"] >= 0).all())
    assert torch.equal(ball["argmax_mass"], many["acc"][:, 0, 0])                                    # the same ball about the same row
    with pytest.raises(ValueError, match="symmetric"):
        harness.grid_pose_error(fl, feat, gt_rotation=torch.stack([gt, gt], dim=1), **kw)
