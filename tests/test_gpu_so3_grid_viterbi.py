"""GPU: the max-plus pass over the SO(3) grid's neighbourhoods (rnf_so3_grid_local_max) against the fp64 bracket of
tests/test_so3_grid_viterbi_host.py, its bit-level invariances, and the two recursions built on the neighbour-limited passes:
grid_viterbi (the most probable joint path) and grid_smooth (fixed-interval smoothing), with grid_pose_smooth on top.

The bracket here is the same brute force over ALL Q rows, in torch fp64 on the device from the whole matrix of distances."""
import math
import time

import numpy as np
import pytest
import torch

from oracle import flow_oracle as orc
from rotationnormflow_amd import harness, make_config, synth
from rotationnormflow_amd.utils import kde
from tests import test_gpu_so3_grid_local as gl
from tests import test_so3_grid_local_host as hl
from tests import test_so3_grid_viterbi_host as hv
from tests.gpu_helpers import product_flow
from tests.test_so3_kde_host import gate, log_normaliser

pytestmark = pytest.mark.gpu
DEV = "cuda"
dev = gl.dev


def device_local_max(level, grid, queries, kappa, cut, lw, off):
    out, arg, count = kde.so3_grid_local_log_max(grid, level, kappa, d2_cut=cut, queries=queries, log_weights=lw, offset=off, return_count=True)
    assert out.dtype == torch.float32 and arg.dtype == torch.int64 and count.dtype == torch.int32 and out.shape == arg.shape
    return out.reshape(-1, queries.shape[0]), arg.reshape(-1, queries.shape[0]), count


def numpy_fn(level, grid, queries, kappa, cut, lw, off):
    out, arg, count = device_local_max(level, dev(grid), dev(queries), kappa, cut, dev(lw), dev(off))
    return out.cpu().numpy(), arg.cpu().numpy(), count.cpu().numpy()


def check_max_device(out, arg, count, d2, kappa, cut, lw, what):
    """hv.check_max in torch on the device: out, arg [G,m], count [m] against the bracket from the fp64 distances d2 [m,Q]"""
    m, Q = d2.shape
    lw64 = torch.zeros(1, Q, dtype=torch.float64, device=d2.device) if lw is None else lw.double()
    l_kappa, delta = float(log_normaliser(kappa)), hl.delta_of(cut)
    excl, incl = d2 <= cut - delta, d2 <= cut + delta
    assert bool((excl.sum(1) <= count).all()) and bool((count <= incl.sum(1)).all()), (what, "count")
    rows, worst, ninf = torch.arange(m, device=d2.device), 0.0, torch.full_like(d2, -math.inf)
    for g, w in enumerate(lw64):
        got = out[g].double()
        term = w[None, :] - 0.5 * kappa * d2 - l_kappa
        E_all = 0.5 * kappa * d2 + torch.nan_to_num(w, posinf=0.0, neginf=0.0).abs()[None, :]
        lo, alo = torch.where(excl, term, ninf).max(dim=1)
        hi, ahi = torch.where(incl, term, ninf).max(dim=1)
        zero = torch.zeros_like(lo)
        E = torch.maximum(torch.where(torch.isfinite(lo), E_all[rows, alo], zero), torch.where(torch.isfinite(hi), E_all[rows, ahi], zero))
        gt = gate(E)
        assert not bool(torch.isnan(got).any()), what
        assert bool((got >= lo - gt).all()), (what, g, "below the bracket", float((lo - got - gt).max()))
        assert bool((got <= hi + gt).all()), (what, g, "above the bracket", float((got - hi - gt).max()))
        live = torch.isfinite(got)
        assert bool(((arg[g] >= 0) == live).all()) and bool((arg[g][~live] == -1).all()) and bool((arg[g] < Q).all()), (what, g, "arg")
        a = torch.where(live, arg[g], torch.zeros_like(arg[g]))
        assert bool(incl[rows, a][live].all()), (what, g, "arg is no member")
        own_err = (term[rows, a] - got).abs() / gate(torch.maximum(E, E_all[rows, a]))
        assert bool((own_err[live] <= 1.0).all()), (what, g, "arg's own term", float(own_err[live].max()))
        fin = live & torch.isfinite(lo)
        if bool(fin.any()):
            worst = max(worst, float((torch.maximum(lo - got, got - hi) / gt)[fin].max()))
    return worst


# ---- the device against the bracket --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level,kind,m", [(1, "none", 0), (1, "fixed", 0), (2, "none", 0), (2, "fixed", 0), (3, "fixed", 2048), (3, "none", 2048),
                                          (4, "fixed", 512), (4, "none", 512)])
def test_device_max_lies_in_the_bracket(level, kind, m):
    """Every grid row and the special queries at levels 1 and 2 with every cut of the sum's file; 2 048 queries at level 3 and 512 at level
    4 with the cuts 0, one spacing, 15 degrees and 8.  G = 5, 3 and 1 (the last two give the first's bits) and no weights."""
    grid, off, queries = gl.sampled_case(level, kind, m)
    Q = grid.shape[0]
    lw5 = dev(hl.log_weights_of(Q, 5, 20 + level))
    d2 = gl.dense_d2(grid, queries)
    nearest = float(d2[Q:].min()) if m == 0 else 1e-4                       # of the off-grid queries
    cuts = hl.cuts_of(level, nearest) if level <= 2 else (0.0, hl.chord2(hl.spacing_deg(level)), hl.chord2(15.0), 8.0)
    worst = 0.0
    for cut in cuts:
        for kappa in hl.KAPPAS:
            out5, arg5, count = device_local_max(level, grid, queries, kappa, cut, lw5, off)
            worst = max(worst, check_max_device(out5, arg5, count, d2, kappa, cut, lw5, (level, kind, cut, kappa, "G=5")))
            out3, arg3, count3 = device_local_max(level, grid, queries, kappa, cut, lw5[:3], off)
            out1, arg1, count1 = device_local_max(level, grid, queries, kappa, cut, lw5[4:], off)
            assert torch.equal(_bits(out3), _bits(out5[:3])) and torch.equal(_bits(out1), _bits(out5[4:]))
            assert torch.equal(arg3, arg5[:3]) and torch.equal(arg1, arg5[4:]) and torch.equal(count, count3) and torch.equal(count, count1)
            out0, arg0, count0 = device_local_max(level, grid, queries, kappa, cut, None, off)
            worst = max(worst, check_max_device(out0, arg0, count0, d2, kappa, cut, None, (level, kind, cut, kappa, "no weights")))
            assert torch.equal(count, count0)
            if cut == 8.0:
                assert bool((count == Q).all())
    print("level %d offset %s: %d queries, worst distance beyond the bracket / gate %.3f" % (level, kind, queries.shape[0], worst))


def test_device_max_ties_and_sentinels():
    hv.check_max_ties(numpy_fn)
    hv.check_max_ties(numpy_fn, 2, "none")
    hv.check_max_sentinels(numpy_fn)
    grid, off = gl.device_grid(1, "fixed")
    out, arg = kde.so3_grid_local_log_max(grid, 1, 4.0, queries=grid[:0], offset=off)           # m = 0 is a no-op
    assert tuple(out.shape) == (0,) and tuple(arg.shape) == (0,)


# ---- bit equality ----------------------------------------------------------------------------------------------------------------------

def _bits(x):
    return x.contiguous().view(torch.int32)


def test_device_gives_the_host_builds_bits_at_level_2():
    grid, off = gl.device_grid(2, "fixed")
    g_host, o_host = grid.cpu().numpy(), off.cpu().numpy()
    lw = hl.log_weights_of(len(g_host), 2, 4)
    for kappa, cut in ((64.0, hl.chord2(30.0)), (1e4, hl.chord2(15.0)), (4.0, 8.0)):
        want, warg, wcount = hv.host_local_max(2, g_host, None, kappa, cut, lw, o_host)
        got, arg, count = kde.so3_grid_local_log_max(grid, 2, kappa, d2_cut=cut, log_weights=dev(lw), offset=off, return_count=True)
        assert np.array_equal(count.cpu().numpy(), wcount)
        same = got.cpu().numpy().view(np.int32) == want.view(np.int32)
        same_arg = arg.cpu().numpy() == warg
        print("kappa %g cut %.4f: %d of %d outputs and %d args differ from the host build" % (kappa, cut, int((~same).sum()), same.size, int((~same_arg).sum())))
        assert same.all() and same_arg.all()


def test_a_max_does_not_depend_on_the_call(monkeypatch):
    level = 3
    grid, off, queries = gl.sampled_case(level, "fixed", 2048)
    Q = grid.shape[0]
    lw = dev(hl.log_weights_of(Q, 3, 3))
    kappa, cut = 264.0, hl.chord2(15.0)
    call = lambda q, w: kde.so3_grid_local_log_max(grid, level, kappa, d2_cut=cut, queries=q, log_weights=w, offset=off, return_count=True)  # noqa: E731
    whole, arg, count = call(queries[:937], lw)
    again, arg2, _ = call(queries[:937], lw)
    assert torch.equal(_bits(whole), _bits(again)) and torch.equal(arg, arg2)                  # from run to run
    scount = kde.so3_grid_local_log_sum(grid, level, kappa, d2_cut=cut, queries=queries[:937], log_weights=lw, offset=off, return_count=True)[1]
    assert torch.equal(scount, count)                                                          # the sum's membership
    for i in (0, 5, 936):
        one, a1, c1 = call(queries[i:i + 1], lw)                                               # alone
        assert torch.equal(_bits(one[:, 0]), _bits(whole[:, i])) and torch.equal(a1[:, 0], arg[:, i]) and c1[0] == count[i]
    part, a64, c64 = call(queries[100:164], lw)
    assert torch.equal(_bits(part), _bits(whole[:, 100:164])) and torch.equal(a64, arg[:, 100:164]) and torch.equal(c64, count[100:164])
    rev, arev, crev = call(queries[:937].flip(0).contiguous(), lw)
    assert torch.equal(_bits(rev.flip(1)), _bits(whole)) and torch.equal(arev.flip(1), arg) and torch.equal(crev.flip(0), count)
    g1, ag1, _ = call(queries[:937], lw[1:2])                                                  # G = 3 against G = 1, and the group's position
    assert torch.equal(_bits(g1[0]), _bits(whole[1])) and torch.equal(ag1[0], arg[1])
    swapped, aswapped, _ = call(queries[:937], lw.flip(0).contiguous())
    assert torch.equal(_bits(swapped.flip(0)), _bits(whole)) and torch.equal(aswapped.flip(0), arg)
    monkeypatch.setattr(kde, "LOCAL_QUERY_TILE", 100)                                          # the Python tiling forced small
    monkeypatch.setattr(kde, "LOCAL_GROUP_TILE", 2)
    tiled, atiled, ctiled = call(queries[:937], lw)
    assert torch.equal(_bits(tiled), _bits(whole)) and torch.equal(atiled, arg) and torch.equal(ctiled, count)
    rows, arows = kde.so3_grid_local_log_max(grid, level, kappa, d2_cut=cut, log_weights=lw[0], offset=off)      # the grid rows, tiled
    monkeypatch.undo()
    rows1, arows1 = kde.so3_grid_local_log_max(grid, level, kappa, d2_cut=cut, log_weights=lw[0], offset=off)    # .. and by the null pointer
    assert rows.shape == (Q,) and torch.equal(_bits(rows), _bits(rows1)) and torch.equal(arows, arows1)


def test_graph_capture_replays_the_eager_max():
    grid, off, queries = gl.sampled_case(3, "fixed", 2048)
    lw = dev(hl.log_weights_of(grid.shape[0], 3, 6))

    def step():
        return kde.so3_grid_local_log_max(grid, 3, 264.0, queries=queries, log_weights=lw, offset=off, return_count=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager, earg, ecount = (x.clone() for x in step())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                           # a host read-back would fail the capture
        out, arg, count = step()
    for _ in range(2):
        out.fill_(float("nan"))
        arg.fill_(-7)
        count.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager)) and torch.equal(arg, earg) and torch.equal(count, ecount)


# ---- the recursions --------------------------------------------------------------------------------------------------------------------

T, B, KAPPA = hv.T_FRAMES, hv.B_SEQ, hv.KAPPA
RECURSIONS = [(level, radius, kind) for level, radius in hv.RECURSION_CASES for kind in ("none", "fixed")]


def prior_of(level, kind):
    """A broad bump about the first trajectory's start, fp32 [Q]"""
    return hv.bumps(hl.grid_of(level, kind), [hv.trajectory(100)[0]], [1.0], 4.0)


@pytest.mark.parametrize("level,radius,kind", RECURSIONS)
def test_grid_viterbi_reaches_the_fp64_optimum(level, radius, kind):
    """The fp64 joint of the returned path against the dense fp64 Viterbi optimum, within T (gate(E) + 3 2^-24 W): T max passes, each
    within its gate, and T stored fp32 deltas; W the largest magnitude the recursion stores in fp32, from the reference.  Measured: every
    path is the reference's own (shortfall 0), log_joint within 0.0005 of the bound."""
    grid, off = gl.device_grid(level, kind)
    model, ll = hv.model_of(level, kind, radius), hv.sequences(level, kind)
    for prior in (None, prior_of(level, kind)):
        res = harness.grid_viterbi(dev(ll), grid, level, KAPPA, radius_deg=radius, offset=off, log_prior=dev(prior))
        assert tuple(res["index"].shape) == (B, T) and res["index"].dtype == torch.int64 and tuple(res["est"].shape) == (B, T, 3, 3)
        assert tuple(res["log_joint"].shape) == (B,) and res["log_joint"].dtype == torch.float64
        assert torch.equal(res["est"], grid[res["index"]])
        path = res["index"].cpu().numpy()
        ref = hv.viterbi_fp64(model, ll, prior)
        joint, worst_d2 = hv.joint_fp64(model, ll, path, prior)
        tol = hv.recursion_tolerance(model, ref["W"], T, T)
        short = ref["score"] - joint
        off_by = np.abs(res["log_joint"].cpu().numpy() - joint)
        print("level %d radius %g offset %s prior %s: optimum - joint of the path %s, |log_joint - joint| %s, tolerance %.3g (W %.1f): %.4f and %.4f of it; "
              "%d of %d rows as the reference's" % (level, radius, kind, prior is not None, short, off_by, tol, ref["W"], short.max() / tol,
                                                   off_by.max() / tol, int((path == ref["path"]).sum()), path.size))
        assert np.isfinite(joint).all() and worst_d2 <= model.cut            # every step of every path within the cut, in fp64
        assert (short <= tol).all() and (off_by <= tol).all()
        # T = 1: the arg-max of pi_0 l_0
        one = harness.grid_viterbi(dev(ll[:, :1]), grid, level, KAPPA, radius_deg=radius, offset=off, log_prior=dev(prior))
        first = dev(ll[:, 0]).double()
        if prior is not None:
            first = first + harness.grid_diffuse_local(dev(prior)[None], grid, level, KAPPA, radius, off).double()
        assert torch.equal(one["index"][:, 0], torch.argmax(first, dim=1)) and tuple(one["index"].shape) == (B, 1)
        # the sequences are independent: B split over calls, and a sequence without the B axis
        for b in range(B):
            alone = harness.grid_viterbi(dev(ll[b:b + 1]), grid, level, KAPPA, radius_deg=radius, offset=off, log_prior=dev(prior))
            assert torch.equal(alone["index"], res["index"][b:b + 1]) and torch.equal(alone["log_joint"], res["log_joint"][b:b + 1])
        flat = harness.grid_viterbi(dev(ll[0]), grid, level, KAPPA, radius_deg=radius, offset=off, log_prior=dev(prior))
        assert tuple(flat["index"].shape) == (T,) and torch.equal(flat["index"], res["index"][0]) and tuple(flat["est"].shape) == (T, 3, 3)


@pytest.mark.parametrize("level,radius", [(2, 25.0), (2, 40.0)])
def test_grid_viterbi_stays_on_one_branch_of_a_symmetric_object_where_the_filter_hops(level, radius):
    """The point of the feature.  Bumps at R_t and R_t Rz(180) with weights alternating about one half: the fp64 filter's per-frame
    arg-max jumps beyond the radius (asserted on the reference); the path of grid_viterbi has no such jump and stays within the grid
    spacing plus the bump width of one of the two branches throughout."""
    kind = "fixed"
    grid, off = gl.device_grid(level, kind)
    g_host = hl.grid_of(level, kind)
    model = hv.model_of(level, kind, radius)
    ll, branches = hv.symmetric_sequence(level, kind)
    top = hv.forward_backward_fp64(model, ll)["filtered"][0].argmax(axis=1)
    hops = hv.angle_deg(g_host[top][1:], g_host[top][:-1])
    assert (hops > radius).sum() >= 1                                       # the precondition, on the reference
    res = harness.grid_viterbi(dev(ll), grid, level, KAPPA, radius_deg=radius, offset=off)
    est = res["est"][0].cpu().numpy()
    steps = hv.angle_deg(est[1:], est[:-1])
    filt = harness.grid_smooth(dev(ll), grid, level, KAPPA, radius_deg=radius, offset=off)["filtered"][0].argmax(dim=1).cpu().numpy()
    print("steps in degrees: fp64 filter %s, device filter %s, grid_viterbi %s; beyond the allowance of either branch by %s" % (
        np.round(hops, 1), np.round(hv.angle_deg(g_host[filt][1:], g_host[filt][:-1]), 1), np.round(steps, 1),
        np.round(hv.branch_distance(est, branches, level), 1)))
    assert (steps <= radius).all()
    assert hv.branch_distance(est, branches, level).min() <= 0.0


@pytest.mark.parametrize("level,radius,kind", RECURSIONS)
def test_grid_smooth_is_the_fp64_forward_backward_recursion(level, radius, kind):
    """filtered is the grid_filter_step chain bit for bit, the last smoothed frame the last filtered one; every smoothed frame has unit
    mass; filtered + backward has unit mass before it is renormalised, and smoothed agrees with the fp64 recursion on every row that
    carries more than 1e-6 of its frame -- both within the gates of the chained sums feeding the frame plus 3 2^-24 W per stored fp32
    intermediate (hv.recursion_tolerance).  Measured: 0.0002 and 0.0006 of the bound."""
    grid, off = gl.device_grid(level, kind)
    Q = grid.shape[0]
    model, ll = hv.model_of(level, kind, radius), hv.sequences(level, kind)
    for prior in (None, prior_of(level, kind)):
        lld = dev(ll)
        res = harness.grid_smooth(lld, grid, level, KAPPA, radius_deg=radius, offset=off, log_prior=dev(prior))
        assert set(res) == {"smoothed", "filtered", "log_evidence", "backward", "index", "est"}
        assert tuple(res["smoothed"].shape) == (B, T, Q) and res["smoothed"].dtype == torch.float32 and res["filtered"].dtype == torch.float32
        assert tuple(res["log_evidence"].shape) == (B, T) and res["log_evidence"].dtype == torch.float64
        post = None if prior is None else dev(prior)[None].expand(B, Q).contiguous()
        for t in range(T):                                                  # the chain by hand
            if post is None:
                ev = torch.logsumexp(lld[:, 0].double(), dim=1) - math.log(Q)
                post = (lld[:, 0].double() - ev[:, None]).float()
            else:
                step = harness.grid_filter_step(post, lld[:, t], grid, level, KAPPA, radius, off)
                post, ev = step["posterior"], step["log_evidence"]
            assert torch.equal(_bits(res["filtered"][:, t]), _bits(post)) and torch.equal(res["log_evidence"][:, t], ev)
        assert torch.equal(_bits(res["smoothed"][:, T - 1]), _bits(res["filtered"][:, T - 1]))
        assert torch.equal(res["index"], res["smoothed"].argmax(dim=2)) and torch.equal(res["est"], grid[res["index"]])
        mass = (torch.logsumexp(res["smoothed"].double(), dim=2) - math.log(Q)).abs().max().item()
        assert mass <= 2e-6
        ref = hv.forward_backward_fp64(model, ll, prior)
        raw = (torch.logsumexp(res["filtered"].double() + res["backward"].double(), dim=2) - math.log(Q)).abs().cpu().numpy()    # [B,T]
        err = np.abs(res["smoothed"].double().cpu().numpy() - ref["smoothed"])
        err = np.where(ref["smoothed"] - math.log(Q) > math.log(1e-6), err, 0.0).max(axis=2)                                       # [B,T]
        # frame t is fed by t forward sums (one more with a prior) and T - 1 - t backward ones, plus the Z sum; each forward step stores
        # its log-weights and its posterior, each backward step its log-weights and b, then the smoothed frame itself
        forward = np.arange(T) + (prior is not None)
        backward = T - 1 - np.arange(T)
        tol = np.array([hv.recursion_tolerance(model, ref["W"], f + b + 1, 2 * f + 2 * b + 2) for f, b in zip(forward, backward)])
        print("level %d radius %g offset %s prior %s: |log mass| %.2e; worst over frames of |log mass of filtered + b| / tolerance %.4f, of "
              "|smoothed - fp64| / tolerance %.4f (tolerance %.3g .. %.3g, W %.1f)" % (
                  level, radius, kind, prior is not None, mass, (raw / tol).max(), (err / tol).max(), tol.min(), tol.max(), ref["W"]))
        assert (raw <= tol).all() and (err <= tol).all()
        assert np.abs(res["log_evidence"].cpu().numpy() - ref["evidence"]).max() <= tol.max()


def test_level_4_smoke_of_both_recursions():
    """2 sequences of 3 frames at level 4 with the default radius: finite outputs, paths within the radius, unit mass, a few seconds"""
    level, kappa = 4, 264.1
    grid, off = gl.device_grid(level, "fixed")
    Q = grid.shape[0]
    cut = kde.local_default_d2_cut(kappa)
    centres = dev(np.stack([hv.trajectory(300 + b, 3, 3.0) for b in range(2)]).astype(np.float32))      # 3 degrees per frame
    ll = -0.5 * 200.0 * ((grid[None, None] - centres[:, :, None]) ** 2).sum(dim=(3, 4))                  # [2,3,Q]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    path = harness.grid_viterbi(ll, grid, level, kappa, offset=off)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    smooth = harness.grid_smooth(ll, grid, level, kappa, offset=off)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print("level 4, 2 sequences of 3 frames: grid_viterbi %.2f s, grid_smooth %.2f s" % (t1 - t0, t2 - t1))
    assert t1 - t0 <= 5.0 and t2 - t1 <= 5.0
    assert torch.isfinite(path["log_joint"]).all() and torch.isfinite(path["est"]).all() and tuple(path["index"].shape) == (2, 3)
    step_d2 = ((path["est"][:, 1:].double() - path["est"][:, :-1].double()) ** 2).sum(dim=(2, 3))
    assert bool((step_d2 <= cut + hl.delta_of(cut)).all())
    assert bool((hv_angle(path["est"], centres) <= 2.0 * 360.0 / (6 * 2 ** level)).all())              # on the trajectory, to two grid spacings
    assert torch.isfinite(smooth["smoothed"]).all() and torch.isfinite(smooth["log_evidence"]).all()
    assert (torch.logsumexp(smooth["smoothed"].double(), dim=2) - math.log(Q)).abs().max().item() <= 2e-6
    assert (torch.logsumexp(smooth["filtered"].double(), dim=2) - math.log(Q)).abs().max().item() <= 2e-6


def hv_angle(a, b):
    return torch.from_numpy(hv.angle_deg(a.cpu().numpy(), b.cpu().numpy()))


def test_grid_pose_smooth_on_a_small_conditional_flow():
    cfg = make_config(layers=3, condition=1, feature_dim=16, rot="16Trans")
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=4, regime="default")
    fl = product_flow(cfg, w)
    frames, level = 3, 2
    feat = torch.from_numpy(synth.features(frames, 16, seed=1)).cuda()
    O = torch.from_numpy(synth.uniform_rotations(1, seed=9)[0])
    res = harness.grid_pose_smooth(fl, feat, 64.0, recursion_level=level, offset=O)
    Q = 72 * 8 ** level
    assert set(res) == {"est_smoothed", "index_smoothed", "est_path", "index_path", "log_evidence", "log_joint", "smoothed", "grid", "offset"}
    for name in ("est_smoothed", "est_path"):
        assert tuple(res[name].shape) == (frames, 3, 3) and torch.isfinite(res[name]).all()
    assert tuple(res["index_smoothed"].shape) == (frames,) and tuple(res["index_path"].shape) == (frames,) and tuple(res["smoothed"].shape) == (frames, Q)
    assert tuple(res["log_evidence"].shape) == (frames,) and res["log_joint"].dim() == 0 and torch.isfinite(res["log_joint"])
    assert torch.equal(res["est_path"], res["grid"][res["index_path"]]) and torch.equal(res["est_smoothed"], res["grid"][res["index_smoothed"]])
    cut = kde.local_default_d2_cut(64.0)
    step_d2 = ((res["est_path"][1:].double() - res["est_path"][:-1].double()) ** 2).sum(dim=(1, 2))
    assert bool((step_d2 <= cut + hl.delta_of(cut)).all())
    filt = harness.grid_pose_filter(fl, feat, 64.0, recursion_level=level, offset=O)          # the same forward chain: its last frame is the smoother's
    assert torch.equal(filt["log_evidence"], res["log_evidence"]) and int(filt["index"][-1]) == int(res["index_smoothed"][-1])
    assert torch.equal(_bits(filt["posterior"]), _bits(res["smoothed"][-1]))
    cfg = make_config(layers=2, condition=1, feature_dim=16, lu=1)          # Condition16TransLU: batch-coupled
    coupled = product_flow(cfg, synth.fill_state_dict(orc.state_shapes(cfg), seed=5, regime="trained"))
    with pytest.raises(ValueError, match="batch-coupled"):
        harness.grid_pose_smooth(coupled, feat, 64.0, recursion_level=1)
