"""GPU: rnf_so3_set_angle_cdf and what is built on it (utils/angles.py so3_set_angle_cdf and so3_set_angle_quantile; grid_pose.grid_set_error,
grid_error_symmetric, grid_pose_error_symmetric) against the fp64 restatement, the cases and the gates of
tests/test_so3_set_angles_host.py (its docstring states the gates), at the smallest shapes at which the tiles of 64, the chunks of 4096,
the blocks of one wave and of 256 sets, the kernels of 0, 1, 2, 4 and 8 threshold slots, the groups per thread and the finalise can go
wrong, on both kernels: a wave per set for few sets, a thread per set otherwise (csrc/so3_set_angle_cdf.h wave_per_set).  n <= 9000
throughout.

Measured on the MI355X: the worst fraction of each gate over test_accuracy_against_the_restatement_and_the_host_build was 0.076 for the
mass, 0.300 for mean_angle and 0.167 for mean_sq_angle; the largest undecided weight of a case 2.9e-5.  DESIGN.md 3.3g."""
import numpy as np
import pytest
import torch

from rotationnormflow_amd import harness
from rotationnormflow_amd.utils import angles, sd, symmetry
from tests import test_so3_angles_host as ha
from tests import test_so3_set_angles_host as hs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)


def gpu_set_angle_cdf(centres, sets, log_weights=None, group_queries=False, thresholds=None, query_tau=None, moments=True, **kw):
    """The signature of hs.host_set_angle_cdf on the device -> dict of numpy arrays with a leading G"""
    lw = dev(log_weights)
    lead = lw is not None or group_queries
    qt = None
    if query_tau is not None:
        qt = dev(np.asarray(query_tau, np.float32))
        qt = qt if lead else qt[0]
    th = None if thresholds is None else [float(t) for t in np.atleast_1d(thresholds)]
    out = angles.so3_set_angle_cdf(dev(centres), dev(sets), th, qt, lw if lw is None or lw.dim() == 2 else lw[None], group_queries=group_queries,
                                   moments=moments, **kw)
    return {k: (v if lead else v[None]).cpu().numpy() for k, v in out.items() if k != "rms_angle"}


def gpu_single_angle_cdf(centres, queries, log_weights=None, group_queries=False, thresholds=None, query_tau=None, moments=True):
    """rnf_so3_angle_cdf with the same signature"""
    lw = dev(log_weights)
    lead = lw is not None or group_queries
    qt = None
    if query_tau is not None:
        qt = dev(np.asarray(query_tau, np.float32))
        qt = qt if lead else qt[0]
    th = None if thresholds is None else [float(t) for t in np.atleast_1d(thresholds)]
    out = angles.so3_angle_cdf(dev(centres), dev(queries), th, qt, lw, group_queries=group_queries, moments=moments)
    return {k: (v if lead else v[None]).cpu().numpy() for k, v in out.items() if k != "rms_angle"}


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("case", hs.CASES + [(9000, 65, 12, 3, 8, False, False, True)], ids=lambda c: "n%d-m%d-K%d-G%d-T%d-%d%d%d" % c)
def test_accuracy_against_the_restatement_and_the_host_build(case):
    got = hs.check_set_case(gpu_set_angle_cdf, case, "device")
    # the host build makes the same comparisons on the same fp32 d2: every indicator agrees, so the masses differ by the rounding of the
    # weights alone -- the gate without its band of undecided pairs
    (Cn, sets, lw, grouped), deg, tau, ref, label = hs.set_reference(*case)
    host = hs.host_set_angle_cdf(Cn, sets, lw, grouped, thresholds=np.deg2rad(deg) if deg else None, query_tau=tau, moments=case[7])
    assert (np.abs(got["mass"].astype(np.float64) - host["mass"]) <= 4e-6 * ref["mass"] + 2.0 ** -23).all(), label
    if lw is None and case[4]:                                           # uniform weights: the counts of the indicators themselves
        assert np.array_equal(np.rint(got["mass"].astype(np.float64) * case[0]), np.rint(host["mass"].astype(np.float64) * case[0])), label
    print("worst fractions of the gates so far:", {k[1]: round(v, 4) for k, v in hs.WORST.items() if k[0] == "device"})


def test_bit_identities():
    """K = 1 is rnf_so3_angle_cdf bit for bit (one group and several, with and without moments, shared and per-query thresholds);
    padding, the order of the members, the split of the thresholds, the group's and the set's position, shared against per-group sets"""
    hs.check_set_bit_identities(gpu_set_angle_cdf, gpu_single_angle_cdf)
    Cn, sets, _ = hs.make_set_case(4097, 70, 1, 1)
    lw4 = (2.0 * np.random.default_rng(4).standard_normal((4, 4097))).astype(np.float32)
    for th in (np.deg2rad([15.0, 30.0]), np.deg2rad(ha.THRESHOLDS_DEG), None):
        for lw in (None, lw4[:1], lw4):
            for mom in (True, False):
                if th is None and not mom:
                    continue
                a = gpu_set_angle_cdf(Cn, sets, lw, False, thresholds=th, moments=mom)
                assert same(a, gpu_single_angle_cdf(Cn, sets[:, 0], lw, False, thresholds=th, moments=mom)), (th, lw is None, mom)


@pytest.mark.parametrize("per_query", [False, True], ids=["shared-thresholds", "query-tau"])
def test_sets_of_one_member_are_the_queries_bit_for_bit_through_the_shared_tiling(per_query):
    """so3_set_angle_cdf on [m,1,3,3] against so3_angle_cdf on [m,3,3], which share the thresholds, the tiling and the copy-back of
    utils/angles.py: n = 4097 is two chunks, the second a single ragged tile; [G,n] log-weights, T = 3, the moments.  Under the default cap
    (one call) and under a cap of two queries' partial sums (8 bytes x 5 slots x 2 chunks each), which tiles the queries in twos and the
    groups in ones and copies every tile back."""
    n, m, G, T = 4097, 5, 3, 3
    Cn, sets, lw = hs.make_set_case(n, m, 1, G)
    Cn, sets, lw = dev(Cn), dev(sets), dev(lw)
    th = [float(t) for t in np.deg2rad([15.0, 30.0, 120.0])]
    tau = dev(np.broadcast_to(ha.tau_of(np.asarray(th))[None, :, None], (G, T, m)).copy()) * torch.linspace(0.5, 1.5, m, device=DEV)
    kw = dict(query_tau=tau) if per_query else dict(thresholds=th)
    per_query_bytes = angles.SLOT_BYTES * (T + 2) * 2
    outs = []
    for cap in (None, 2 * per_query_bytes):
        a = angles.so3_set_angle_cdf(Cn, sets, log_weights=lw, workspace_cap=cap, **kw)
        b = angles.so3_angle_cdf(Cn, sets[:, 0], log_weights=lw, workspace_cap=cap, **kw)
        assert a.keys() == b.keys() == {"mass", "mean_angle", "mean_sq_angle", "rms_angle"} and tuple(a["mass"].shape) == (G, T, m)
        assert all(torch.equal(a[k], b[k]) and torch.isfinite(a[k]).all() for k in a), (per_query, cap)
        outs.append(a)
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])
    assert (outs[0]["mass"][:, 1:] >= outs[0]["mass"][:, :-1]).all()     # the thresholds of a query increase with the slot


def test_edge_cases():
    hs.check_set_edge_cases(gpu_set_angle_cdf)
    Cn = dev(ha.draw("uniform", 5, 1))
    out = angles.so3_set_angle_cdf(Cn, torch.empty(0, 3, 3, 3, device=DEV), [0.3, 0.5])             # m = 0 is a no-op
    assert tuple(out["mass"].shape) == (2, 0) and tuple(out["mean_angle"].shape) == (0,) and tuple(out["rms_angle"].shape) == (0,)
    sets = Cn[:, None].expand(5, 2, 3, 3).contiguous()
    with pytest.raises(ValueError, match="query_sets"):
        angles.so3_set_angle_cdf(Cn, sets[None], [0.3])                  # sets per group without group_queries
    with pytest.raises(ValueError, match="both"):
        angles.so3_set_angle_cdf(Cn, sets, [0.3], torch.zeros(1, 5, device=DEV))
    with pytest.raises(ValueError, match="thresholds"):
        angles.so3_set_angle_cdf(Cn, sets, [0.1] * 9)
    with pytest.raises(ValueError, match="query_tau"):
        angles.so3_set_angle_cdf(Cn, sets, None, torch.zeros(1, 4, device=DEV))
    with pytest.raises(ValueError, match="nothing"):
        angles.so3_set_angle_cdf(Cn, sets, moments=False)
    with pytest.raises(ValueError, match="workspace_cap"):
        angles.so3_set_angle_cdf(Cn, sets, [0.3], workspace_cap=16)
    with pytest.raises(ValueError, match="level"):
        angles.so3_set_angle_quantile(Cn, sets, [0.5, 1.0])
    full = angles.so3_set_angle_cdf(Cn, sets, [0.3, 1.0], None, torch.zeros(3, 5, device=DEV))
    assert {k: tuple(v.shape) for k, v in full.items()} == dict(mass=(3, 2, 5), mean_angle=(3, 5), mean_sq_angle=(3, 5), rms_angle=(3, 5))
    assert torch.equal(full["rms_angle"], torch.sqrt(full["mean_sq_angle"]))


def test_mass_orderings():
    hs.check_set_mass_orderings(gpu_set_angle_cdf)


def test_bit_identical_from_run_to_run_and_however_the_call_is_tiled():
    Cn, sets, lw = hs.make_set_case(4097, 1000, 2, 3)
    th = np.deg2rad(ha.THRESHOLDS_DEG)
    whole = gpu_set_angle_cdf(Cn, sets, lw, thresholds=th)
    assert same(whole, gpu_set_angle_cdf(Cn, sets, lw, thresholds=th))
    for step in (64, 937):
        parts = [gpu_set_angle_cdf(Cn, sets[i:i + step], lw, thresholds=th) for i in range(0, 1000, step)]
        assert same(whole, {k: np.concatenate([p[k] for p in parts], axis=-1) for k in whole}), step
    rolled = gpu_set_angle_cdf(Cn, hs.per_group_sets(sets, 3), lw, True, thresholds=th)
    for g in range(3):
        assert all(np.array_equal(np.roll(whole[k][g], 2 * g, axis=-1), rolled[k][g]) for k in ha.OUTPUTS), g
    tau = np.broadcast_to(ha.tau_of(th)[None, :, None], (3, 8, 1000))
    assert same(whole, gpu_set_angle_cdf(Cn, np.stack([sets] * 3), lw, True, query_tau=tau))
    # the Python tiling, forced by a small cap: sets in tiles, then groups too; shared sets and sets per group
    for cap in (1 << 20, 1 << 12):
        assert same(whole, gpu_set_angle_cdf(Cn, sets, lw, thresholds=th, workspace_cap=cap)), cap
        assert same(rolled, gpu_set_angle_cdf(Cn, hs.per_group_sets(sets, 3), lw, True, thresholds=th, workspace_cap=cap)), cap
        assert same(whole, gpu_set_angle_cdf(Cn, np.stack([sets] * 3), lw, True, query_tau=tau, workspace_cap=cap)), cap
    # the bracket search on top of it
    q = {k: v.cpu().numpy() for k, v in angles.so3_set_angle_quantile(dev(Cn), dev(sets[:65]), [0.5, 0.9], dev(lw)).items()}
    tiled = {k: v.cpu().numpy() for k, v in angles.so3_set_angle_quantile(dev(Cn), dev(sets[:65]), [0.5, 0.9], dev(lw), workspace_cap=1 << 12).items()}
    assert same(q, tiled) and q["radius"].shape == (3, 2, 65) and (q["radius"][:, 1] >= q["radius"][:, 0]).all()

    def cdf64(theta):
        t = np.where(theta >= np.pi, np.float32(ha.FLT_MAX), (8.0 * np.sin(0.5 * theta) ** 2).astype(np.float32))[:, None, :].astype(np.float32)
        ref = hs.set_angle_cdf_fp64(Cn, np.stack([sets[:65]] * 3), t, lw, True)
        return ref["mass"][:, 0], ref["U"][:, 0]
    ha.check_quantile(lambda levels, tol: q, cdf64)


def test_a_wave_per_set_and_a_thread_per_set_give_the_same_bits():
    """Few sets of K >= 8 members run a wave per (group, set, chunk), csrc/so3_set_angle_cdf.h wave_per_set: at most 4096 of them.
    2100 sets x 2 chunks, and 1400 sets x 2 chunks x 3 groups per-set thresholds, take a thread per set; the same sets in calls of
    64 and of 600 take a wave per set.  Ragged last tile (4097 = 64 x 64 + 1), padding members, all three kernel forms."""
    Cn, sets, lw = hs.make_set_case(4097, 2100, 12, 3)
    sets = sets.copy()
    sets[5, 3:] = np.nan                                                 # sets of 3 and of 11 live members
    sets[6, 7, 0, 1] = np.inf
    th = np.deg2rad(ha.THRESHOLDS_DEG)
    for lwk, mom in ((None, True), (None, False), (lw, True)):           # one group; three groups that share the minima
        whole = gpu_set_angle_cdf(Cn, sets, lwk, thresholds=th, moments=mom)
        for step in (64, 600):
            parts = [gpu_set_angle_cdf(Cn, sets[i:i + step], lwk, thresholds=th, moments=mom) for i in range(0, 2100, step)]
            assert same(whole, {k: np.concatenate([p[k] for p in parts], axis=-1) for k in whole}), (lwk is None, mom, step)
    tau = ha.tau_of(np.random.default_rng(2).uniform(0.02, np.pi - 0.02, 3 * 3 * 1400)).reshape(3, 3, 1400)
    per = np.stack([sets[:1400]] * 3)
    whole = gpu_set_angle_cdf(Cn, per, lw, True, query_tau=tau)
    parts = [gpu_set_angle_cdf(Cn, per[:, i:i + 350], lw, True, query_tau=tau[:, :, i:i + 350]) for i in range(0, 1400, 350)]
    assert same(whole, {k: np.concatenate([p[k] for p in parts], axis=-1) for k in whole})
    host = hs.host_set_angle_cdf(Cn, sets[:70], lw, thresholds=th)       # and both hold the host build's indicator bits
    ref = hs.set_angle_cdf_fp64(Cn, sets[:70], ha.tau_of(th), lw)
    for got in (gpu_set_angle_cdf(Cn, sets[:70], lw, thresholds=th), {k: v[..., :70] for k, v in gpu_set_angle_cdf(Cn, sets, lw, thresholds=th).items()}):
        assert (np.abs(got["mass"].astype(np.float64) - host["mass"]) <= 4e-6 * ref["mass"] + 2.0 ** -23).all()


def test_blocks_of_one_wave_and_of_four_give_the_same_bits():
    """The pairwise pass runs blocks of 64 threads while blocks of 256 would number fewer than 1024 (ac::block_for), which covers every
    other case of this file.  Sets per group: 70,001 sets x 4 groups make 274 x 4 = 1096 blocks of 256; the same sets in calls of
    9,000 take the other path.  Shared sets and thresholds put the four groups into one thread (274 blocks: one wave each), and 262,145
    shared sets make 1025 blocks of 256 for that kernel, against calls of 65,536."""
    Cn, _, _ = hs.make_set_case(65, 1, 2, 1)
    Er = ha.draw("clustered", 70001, 31)
    sets = (Er.astype(np.float64)[:, None] @ hs.group_of(2).astype(np.float64)[None]).astype(np.float32)
    lw = (2.0 * np.random.default_rng(32).standard_normal((4, 65))).astype(np.float32)
    th = np.deg2rad([5.2, 15.2, 180.0])
    per = gpu_set_angle_cdf(Cn, np.broadcast_to(sets, (4,) + sets.shape), lw, True, thresholds=th)
    parts = [gpu_set_angle_cdf(Cn, np.broadcast_to(sets[i:i + 9000], (4,) + sets[i:i + 9000].shape), lw, True, thresholds=th) for i in range(0, 70001, 9000)]
    assert same(per, {k: np.concatenate([p[k] for p in parts], axis=-1) for k in per})
    assert same(per, gpu_set_angle_cdf(Cn, sets, lw, thresholds=th))                                 # four groups per thread, one wave per block
    big = np.concatenate([sets, sets, sets, sets[:52142]])                                           # 262,145 shared sets
    whole = gpu_set_angle_cdf(Cn, big, lw, thresholds=th)
    assert same({k: v[..., :70001] for k, v in whole.items()}, per)
    parts = [gpu_set_angle_cdf(Cn, big[i:i + 65536], lw, thresholds=th) for i in range(0, len(big), 65536)]
    assert same(whole, {k: np.concatenate([p[k] for p in parts], axis=-1) for k in whole})


def test_the_library_writes_no_row_behind_the_last():
    import ctypes as C

    from rotationnormflow_amd import _lib
    SENTINEL = 12345.0
    Cn, sets, lw = (dev(x) for x in hs.make_set_case(4097, 65, 12, 3))
    G, m, T = 3, 65, 5
    th = (C.c_double * T)(*np.deg2rad([5.0, 15.0, 30.0, 90.0, 180.0]))
    bufs = dict(mass=torch.full((G * T * m + 7,), SENTINEL, device=DEV), mean_angle=torch.full((G * m + 7,), SENTINEL, device=DEV),
                mean_sq_angle=torch.full((G * m + 7,), SENTINEL, device=DEV))
    args = _lib.So3SetAngleCdf(centres=Cn.data_ptr(), queries=sets.data_ptr(), log_weights=lw.data_ptr(), n=4097, m=m, K=12, G=G, T=T,
                               thresholds=C.addressof(th), **{k: v.data_ptr() for k, v in bufs.items()})
    _lib.call("so3_set_angle_cdf", args, Cn.device)
    torch.cuda.synchronize()
    want = angles.so3_set_angle_cdf(Cn, sets, list(th), None, lw)
    for k, v in bufs.items():
        assert (v[-7:] == SENTINEL).all(), k
        assert torch.equal(v[:-7].reshape(want[k].shape), want[k]), k


def test_capture_in_a_graph_and_replay():
    Cn, sets, lw = (dev(x) for x in hs.make_set_case(4097, 65, 12, 3))
    tau = dev(np.broadcast_to(ha.tau_of(np.deg2rad([15.0, 30.0, 90.0]))[None, :, None], (3, 3, 65)).copy())
    sets_g = torch.stack([sets] * 3)

    def step():
        a = angles.so3_set_angle_cdf(Cn, sets, [0.3, 1.0, 2.0], None, lw)
        b = angles.so3_set_angle_cdf(Cn, sets_g, None, tau, lw, group_queries=True, moments=False)
        return [a["mass"], a["mean_angle"], a["mean_sq_angle"], b["mass"]]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [x.clone() for x in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(2):
        for x in out:
            x.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, eager):
            assert torch.equal(x, y)


# ---- grid posteriors ---------------------------------------------------------------------------------------------------------------------

def symmetric_posterior(level, R0, S, kappa=20.0):
    """(grid [Q,3,3] on the device, logp [b,Q] float32 numpy): the mixture of MF(kappa R0 S_s) over the group S, up to the normaliser"""
    grid = sd.generate_healpix_grid(recursion_level=level, device=DEV)
    g64 = grid.double().cpu().numpy()
    modes = R0[:, None] @ S.astype(np.float64)[None]                     # [b,K,3,3]
    t = kappa * (np.einsum("qij,bkij->bkq", g64, modes) - 3.0)
    return grid, np.logaddexp.reduce(t, axis=1).astype(np.float32)


def acos_tolerance_deg(theta_deg):
    """The tolerance of an angle that goes through an fp32 trace and acosf (rnf_min_geodesic): nine fused products of entries <= 1
    each round at half an ulp of a partial sum below 4, 9 x 2^-23 in all, halved by (tr - 1) / 2: dx <= 5.4e-7, and d theta = dx /
    sin theta; acosf itself and the fp32 result add 2 ulp of an angle below pi, 4.8e-7; plus 1e-5 degrees for the fp32 degrees"""
    return np.degrees(5.4e-7 / np.sin(np.radians(theta_deg)) + 4.8e-7) + 1e-5


def test_grid_error_symmetric_on_a_tetrahedral_posterior():
    S = symmetry.point_group("T", device=DEV)
    Sn = S.cpu().numpy()
    R0 = ha.draw("uniform", 2, 5).astype(np.float64)
    grid, logp = symmetric_posterior(2, R0, Sn)
    gn, lp = grid.cpu().numpy(), dev(logp)
    est = dev(R0.astype(np.float32))[:, None]                            # [2,1,3,3]
    orb = symmetry.orbit(est, S)                                         # [2,1,12,3,3]: the sets the call sees
    on = orb.cpu().numpy()
    # the grid has rows at exactly 15 and 30 degrees from one another: the thresholds move by the rule of tests/test_so3_angles_host.py
    deg, ref = ha.settle((15.0, 30.0, 180.0), lambda d: hs.set_angle_cdf_fp64(gn, on, ha.tau_of(np.deg2rad(d)), logp, True), "grid_error_symmetric")
    assert all(abs(a - b) < 0.5 for a, b in zip(deg, (15.0, 30.0, 180.0)))
    truth = ha.draw("uniform", 2, 15).astype(np.float32)
    gts = symmetry.orbit(dev(truth), S)                                  # [2,12,3,3]: the 12 equivalent truths
    out = harness.grid_error_symmetric(lp, grid, est, S, thresholds_deg=tuple(deg), levels=(0.5, 0.9), gt=gts)
    assert {k: tuple(v.shape) for k, v in out.items()} == dict(acc=(2, 1, 3), expected_deg=(2, 1), rms_deg=(2, 1), radius_deg=(2, 1, 2),
                                                              error_deg=(2, 1), pit=(2, 1))
    got = dict(mass=out["acc"].permute(0, 2, 1).cpu().numpy(), mean_angle=np.deg2rad(out["expected_deg"].double().cpu().numpy()),
               mean_sq_angle=np.deg2rad(out["rms_deg"].double().cpu().numpy()) ** 2)
    err = np.abs(got["mass"] - ref["mass"])
    assert (ref["U"][:, :2] <= ha.U_CAP).all() and (err <= np.where(np.arange(3)[None, :, None] == 2, 0.0, ref["U"]) + 4e-6 * ref["mass"] + 2.0 ** -23).all()
    assert (np.abs(got["mean_angle"] - ref["mean_angle"]) <= ref["gate_mean"] + 1e-7 * ref["mean_angle"]).all()     # + the rounding of degrees
    assert (np.abs(got["mean_sq_angle"] - ref["mean_sq_angle"]) <= ref["gate_sq"] + 4e-7 * ref["mean_sq_angle"]).all()
    # the twelve balls of 30 degrees about the orbit are disjoint (the members are 120 degrees apart or more): their union holds what
    # the twelve hold one by one, 12 times the one about R0 up to the grid's asymmetry -- well above grid_error's value
    single = harness.grid_error(lp, grid, orb[:, 0], thresholds_deg=tuple(deg), levels=())["acc"]    # [2,12,3]: each member alone
    acc = out["acc"][:, 0]
    print("grid_error_symmetric: acc %s, one member %s, the members' sum %s" % (acc.cpu().numpy(), single[:, 0].cpu().numpy(), single.sum(1).cpu().numpy()))
    assert bool((acc[:, 1] >= single[:, :, 1].sum(1) - 1e-5).all()) and bool((acc[:, :2] <= single[:, :, :2].sum(1) + 1e-5).all())
    assert bool((acc[:, 1] > 3.0 * single[:, 0, 1]).all()) and bool((acc[:, 1] > 0.5).all()) and bool((single[:, 0, 1] < 0.2).all())
    assert bool((out["expected_deg"] < 30.0).all())                      # every mode is near a member; about one estimate it is ~ 100
    assert bool((harness.grid_error(lp, grid, est, levels=())["expected_deg"] > 60.0).all())
    # each of the 12 equivalent truths gives the same error and the same pit; the group recovered from the truths does too
    want = torch.rad2deg(harness.min_geodesic_distance(est[:, 0], gts)).double().cpu().numpy()
    exact = ha.angle_deg(on[:, 0], truth[:, None]).min(axis=1)
    assert ((exact > 5.0) & (exact < 175.0)).all()
    tol = acos_tolerance_deg(exact)
    assert (np.abs(out["error_deg"][:, 0].double().cpu().numpy() - want) <= tol).all() and (np.abs(want - exact) <= tol).all()
    for s in range(12):
        one = harness.grid_error_symmetric(lp, grid, est, S, thresholds_deg=(), levels=(), gt=gts[:, s])
        # the threshold is min_s |est S_s - gt|^2 of another rounding of the same pose: it moves by parts in 1e7, and the pit by the
        # weight of a grid row in that band, of which this posterior has none
        assert (one["error_deg"] - out["error_deg"]).abs().max() <= 1e-4 and (one["pit"] - out["pit"]).abs().max() <= 1e-6, s
    rolled = harness.grid_error_symmetric(lp, grid, est, None, thresholds_deg=tuple(deg), levels=(0.5, 0.9), gt=gts.roll(5, dims=1))
    assert (rolled["acc"] - out["acc"]).abs().max() <= 1e-5 and (rolled["error_deg"] - out["error_deg"]).abs().max() <= 1e-4
    assert (rolled["radius_deg"] - out["radius_deg"]).abs().max() <= 0.06 and (rolled["pit"] - out["pit"]).abs().max() <= 1e-5
    d2 = ((on[:, 0].astype(np.float64) - truth[:, None].astype(np.float64)) ** 2).sum(axis=(2, 3)).min(axis=1)
    pit = hs.set_angle_cdf_fp64(gn, on, d2.astype(np.float32)[:, None, None], logp, True)
    assert (np.abs(out["pit"].double().cpu().numpy() - pit["mass"][:, 0]) <= pit["U"][:, 0] + 4e-6 * pit["mass"][:, 0] + 2.0 ** -23).all()
    per_image = harness.grid_error_symmetric(lp, grid, est, torch.stack([S, S]), thresholds_deg=tuple(deg), gt=gts)      # one group per image
    assert all(torch.equal(per_image[k], out[k]) for k in out)
    alone = harness.grid_error_symmetric(lp[1:], grid, est[1:], S, thresholds_deg=tuple(deg), gt=gts[1:])              # an image does not depend on the batch
    assert all(torch.equal(alone[k], out[k][1:]) for k in out)


def test_expected_error_about_an_orbit_of_truths_is_the_spread():
    """expected_deg about a truth's orbit against the spread of grid_modes for the same K <= 16 truths: two kernels, one definition;
    the tolerance is the one tests/test_gpu_so3_angles.py records for K = 1"""
    S = symmetry.point_group("T", device=DEV)
    R0 = ha.draw("uniform", 2, 6).astype(np.float64)
    grid, logp = symmetric_posterior(2, R0, S.cpu().numpy())
    lp = dev(logp)
    truth = dev(R0.astype(np.float32))
    gts = symmetry.orbit(truth, S)                                       # [2,12,3,3]
    spread = harness.grid_modes(lp, grid, 1, float(np.deg2rad(15.0)), gts)[4].double().cpu().numpy()
    out = harness.grid_error_symmetric(lp, grid, truth[:, None], S, thresholds_deg=(), levels=())
    assert tuple(out["acc"].shape) == (2, 1, 0) and tuple(out["radius_deg"].shape) == (2, 1, 0)
    expected = np.deg2rad(out["expected_deg"][:, 0].double().cpu().numpy())
    ref = hs.set_angle_cdf_fp64(grid.cpu().numpy(), gts.cpu().numpy()[:, None], None, logp, True)
    print("expected %s rad, spread %s rad, restatement %s" % (expected, spread, ref["mean_angle"][:, 0]))
    assert (np.abs(expected - ref["mean_angle"][:, 0]) <= ref["gate_mean"][:, 0] + 1e-7 * ref["mean_angle"][:, 0] + 2e-7).all()
    assert (np.abs(spread - ref["mean_angle"][:, 0]) <= 1e-4).all() and (np.abs(spread - expected) <= 1e-4).all()


def test_grid_set_error_on_top_k_modes():
    S = symmetry.point_group("D2").numpy()                               # four modes, 180 degrees apart
    R0 = ha.draw("uniform", 2, 7).astype(np.float64)
    grid, logp = symmetric_posterior(2, R0, S)
    lp = dev(logp)
    index = harness.grid_modes(lp, grid, 3, float(np.deg2rad(40.0)))[0]
    est = torch.cat([grid[index], torch.full((2, 1, 3, 3), float("nan"), device=DEV)], dim=1)       # three modes and one that does not exist
    each = harness.grid_error(lp, grid, est[:, :3], thresholds_deg=(15.2, 30.2), levels=(0.5,))
    best = harness.grid_set_error(lp, grid, est[:, None], thresholds_deg=(15.2, 30.2), levels=(0.5,))       # the modes as ONE set; NaN is padding
    assert {k: tuple(v.shape) for k, v in best.items()} == dict(acc=(2, 1, 2), expected_deg=(2, 1), rms_deg=(2, 1), radius_deg=(2, 1, 1))
    assert all(bool(torch.isfinite(v).all()) for v in best.values())
    assert bool((best["acc"][:, 0] >= each["acc"].max(dim=1).values).all()) and bool((best["acc"][:, 0] <= each["acc"].sum(dim=1) + 1e-5).all())
    assert bool((best["acc"][:, 0, 1] > 1.5 * each["acc"][..., 1].max(dim=1).values).all())          # three of four equal modes against one
    assert bool((best["expected_deg"][:, 0] <= each["expected_deg"].min(dim=1).values).all())
    assert bool((best["radius_deg"][:, 0, 0] <= each["radius_deg"][:, :, 0].min(dim=1).values + 0.05).all())
    assert torch.equal(best["acc"], harness.grid_set_error(lp, grid, est[:, [3, 1, 0, 2]][:, None], thresholds_deg=(15.2, 30.2), levels=(0.5,))["acc"])
    one = harness.grid_set_error(lp, grid, est[:, :1, None], thresholds_deg=(15.2, 30.2), levels=(0.5, 0.9))           # k = 1: grid_error's bits
    ref = harness.grid_error(lp, grid, est[:, :1], thresholds_deg=(15.2, 30.2), levels=(0.5, 0.9))
    assert all(torch.equal(one[k], ref[k]) for k in one)
    none = harness.grid_set_error(lp, grid, est[:, 3:, None], levels=(0.5,))                         # a set of padding only
    assert all(bool(torch.isnan(v).all()) for v in none.values())


def test_grid_pose_error_symmetric_runs_the_launches_of_grid_estimate_rotations():
    from rotationnormflow_amd import synth
    from tests.test_gpu_grid_pose import _flow, _offset
    _, _, fl = _flow(seed=13)
    feat = torch.from_numpy(synth.features(2, 32, seed=8)).cuda()
    kw = dict(recursion_level=1, offset=_offset(6))
    est, best, index, offset = harness.grid_estimate_rotations(fl, feat, **kw)
    S = symmetry.point_group("D2", device=DEV)
    gts = symmetry.orbit(dev(ha.draw("uniform", 2, 9)), S)               # [2,4,3,3]
    out = harness.grid_pose_error_symmetric(fl, feat, S, gt_rotation=gts, **kw)
    assert {k: tuple(v.shape) for k, v in out.items()} == dict(acc=(2, 1, 2), expected_deg=(2, 1), rms_deg=(2, 1), radius_deg=(2, 1, 2),
                                                              error_deg=(2, 1), pit=(2, 1), est=(2, 1, 3, 3), index=(2,), log_norm=(2,), offset=(3, 3))
    assert torch.equal(out["index"], index) and torch.equal(out["est"][:, 0], est)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    assert bool(((out["acc"] >= 0) & (out["acc"] <= 1)).all()) and bool((out["acc"][..., 1] >= out["acc"][..., 0]).all())
    assert bool((out["radius_deg"][..., 1] >= out["radius_deg"][..., 0]).all()) and bool((out["rms_deg"] >= out["expected_deg"]).all())
    assert bool(((out["pit"] >= 0) & (out["pit"] <= 1)).all())
    plain = harness.grid_pose_error(fl, feat, gt_rotation=gts[:, 0], **kw)
    assert bool((out["acc"] >= plain["acc"]).all()) and bool((out["expected_deg"] <= plain["expected_deg"]).all())
    assert bool((out["error_deg"] <= plain["error_deg"] + 1e-4).all())
    want = torch.rad2deg(harness.min_geodesic_distance(est, gts)).double().cpu().numpy()
    exact = ha.angle_deg(est.cpu().numpy()[:, None], gts.cpu().numpy()).min(axis=1)
    tol = acos_tolerance_deg(np.clip(exact, 1.0, 179.0))
    assert (np.abs(out["error_deg"][:, 0].double().cpu().numpy() - exact) <= tol).all() and (np.abs(want - exact) <= tol).all()
    one = harness.grid_pose_error_symmetric(fl, feat, S, gt_rotation=gts, images_per_launch=1, **kw)
    assert all(torch.equal(one[k], out[k]) for k in out)
    recovered = harness.grid_pose_error_symmetric(fl, feat, None, gt_rotation=gts, **kw)             # the group from the truths
    assert (recovered["acc"] - out["acc"]).abs().max() <= 1e-5 and (recovered["error_deg"] - out["error_deg"]).abs().max() <= 1e-4
    trivial = harness.grid_pose_error_symmetric(fl, feat, symmetry.point_group("C1", device=DEV), gt_rotation=gts[:, 0], **kw)
    assert all(torch.equal(trivial[k], plain[k]) for k in ("acc", "expected_deg", "rms_deg", "radius_deg", "pit", "index", "log_norm"))
    modes = harness.grid_pose_modes(fl, feat, top_k=3, separation_deg=60.0, **kw)
    many = harness.grid_pose_error_symmetric(fl, feat, torch.stack([S, S]), est=modes["est"], thresholds_deg=(30.0,), levels=(0.5,), **kw)
    assert tuple(many["acc"].shape) == (2, 3, 1) and "pit" not in many
    with pytest.raises(ValueError, match="symmetric"):                   # grid_pose_error keeps its refusal
        harness.grid_pose_error(fl, feat, gt_rotation=gts, **kw)
