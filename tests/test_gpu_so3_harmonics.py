"""Harmonic analysis on SO(3) on the device (rnf_so3_wigner, rnf_so3_fourier, rnf_so3_fourier_eval; utils/harmonics.py; the grid_*
functions built on them): the cases, the restatement and the gates of tests/test_so3_harmonics_host.py, device against host build,
bit-identity under tiling, graph capture, and the grid functions against the restatement.

Device against host build.  The entry records are formed in fp64 and are the same bits; the quaternion is formed in fp64.  The fp32
terms are not promised to be the same bits: the device build contracts a product that feeds an addition (u + v of the seeds, the
power tables) into an fma, which the host build (-ffp-contract=off) does not.  So the device is GATED against the host build with the
gates of the restatement, and the measured differences are printed.

The worst fractions of the gates measured on the MI355X (each test prints its own, run with -s; DESIGN.md 3.3i has them beside the
host build's): matrices 0.248, D^1 0.25 of 2^-23, orthogonality 0.072, products 0.059, analysis 0.130, chunk boundary 0.246, synthesis
0.083, grid_diffuse_spectral at level 1 0.924 (the flat posterior, where the output's own rounding is half of the gate), grid_spectrum's
power 0.017 of its propagated bound, grid_compose below 0.01.  In these runs the device's outputs had the host build's bits (0 of
1 309 000 matrix entries differ), which is measured, not promised.

grid_compose has no gate in the host file; its gate here is the synthesis gate on the coefficients the device hands to the synthesis,
plus what the analysis gate allows the composed coefficients to be off by: |F^l|_F <= sqrt(2l+1) (a mean of orthogonal matrices),
|dF^l|_F <= (2l+1) g_l with g_l = C_ENTRY (l+1) 2^-23 per entry, so |d(F_a^l F_b^l)|_F <= 2 sqrt(2l+1) (2l+1) g_l, and a degree adds at
most (2l+1) h_l |dC^l|_F |D^l|_F = 2 (2l+1)^3 h_l g_l to a value."""
import numpy as np
import pytest
import torch

from rotationnormflow_amd import grid_pose, harness, synth
from rotationnormflow_amd.utils import harmonics, sd
from tests import test_so3_harmonics_host as hh
from tests.test_gpu_grid_pose import _flow, _offset

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.0


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def dev_wigner(R, L):
    return harmonics.wigner_matrices(dev(np.asarray(R, np.float32).reshape(-1, 3, 3)), L).cpu().numpy()


def dev_fourier(Cn, L, lw=None, **kw):
    out = harmonics.so3_fourier(dev(np.asarray(Cn, np.float32).reshape(-1, 3, 3)), L, log_weights=dev(lw), **kw)
    return out.cpu().numpy().reshape(-1, hh.count(L))


def raw_multiplier(L):
    """h_l = 1 / (2l+1): so3_fourier_density's factor (2l+1) h_l is then 1 to within 2^-52, and the fp32 coefficients times it, rounded
    to fp32, reach the kernel as they are"""
    return [1.0 / (2 * l + 1) for l in range(L + 1)]


def dev_density(c, Q, L, group_queries=False):
    out = harmonics.so3_fourier_density(dev(np.asarray(c, np.float32).reshape(-1, hh.count(L))), dev(np.asarray(Q, np.float32)), L,
                                        multiplier=raw_multiplier(L), group_queries=group_queries)
    return out.cpu().numpy()


def test_raw_multiplier_is_exactly_one():
    scale = harmonics._degree_scale(raw_multiplier(16), 16, "test", torch.device(DEV))
    assert bool((scale.to(torch.float32) == 1.0).all()) and bool(((scale - 1.0).abs() < 1e-15).all())


def test_device_matrices_against_the_restatement_and_the_host_build():
    hh.check_matrices(dev_wigner, "MI355X ")
    rows = hh.matrix_rows()
    d, h = dev_wigner(rows, hh.LMAX), hh.host_wigner(rows, hh.LMAX)
    f = hh.worst(np.abs(d.astype(np.float64) - h), hh.entry_gate(hh.LMAX)[None])
    print(f"device against host build, matrices: {f:.3f} of the gate, {int((d != h).sum())} of {d.size} entries differ in bits")
    assert f <= 1.0
    bad = rows[:3].copy()
    bad[1, 0, 2] = np.nan
    out = dev_wigner(bad, 3)
    assert np.isnan(out[1]).all() and np.array_equal(out[[0, 2]], dev_wigner(rows[[0, 2]], 3))
    assert np.array_equal(dev_wigner(rows[:9], 5), d[:9, :hh.count(5)])   # bits do not depend on L


def test_device_analysis_against_the_restatement_and_the_host_build():
    hh.check_analysis(dev_fourier, "MI355X ")
    f = 0.0
    for n, G, L in hh.ANALYSIS_CASES:
        Cn, lw, _ = hh.analysis_reference(n, G, L)
        f = max(f, hh.worst(np.abs(dev_fourier(Cn, L, lw).astype(np.float64) - hh.host_fourier(Cn, L, lw)), hh.entry_gate(L)[None]))
    print(f"device against host build, analysis: {f:.3f} of the gate")
    assert f <= 1.0


def test_device_chunk_boundary_against_the_character_sum():
    hh.check_chunk_boundary(dev_fourier, dev_density, "MI355X ")


def test_device_synthesis_against_the_restatement_and_the_host_build():
    hh.check_synthesis(dev_density, "MI355X ")
    f = 0.0
    for m, G, gq in hh.SYNTHESIS_CASES:
        c, Q, ref = hh.synthesis_reference(m, G, gq)
        diff = np.abs(dev_density(c, Q, hh.SYNTHESIS_L, gq).astype(np.float64) - hh.host_density(c, Q, hh.SYNTHESIS_L, gq))
        f = max(f, hh.worst(diff, hh.synthesis_gate(c, ref, hh.SYNTHESIS_L)))
    print(f"device against host build, synthesis: {f:.3f} of the gate")
    assert f <= 1.0


def test_device_edge_cases():
    Cn, Q = hh.analysis_centres().copy(), hh.synthesis_queries()[0, :6].copy()
    lw = hh.weight_rows(5, 65, 91)
    lw[1, 7] = -np.inf
    Cn[7, 1, 1] = np.nan
    lw[4] = -np.inf
    F = dev_fourier(Cn, 8, lw)
    assert np.isfinite(F[1]).all() and np.isnan(F[[0, 2, 3, 4]]).all()
    keep = np.delete(np.arange(65), 7)
    ref = hh.fourier_fp64(hh.analysis_centres()[keep], 8, lw[1:2, keep])
    assert hh.worst(np.abs(F[1:2] - ref), hh.entry_gate(8)[None]) <= 1.0
    lwn = hh.weight_rows(2, 65, 92)
    lwn[0, 64] = np.nan
    Fn = dev_fourier(hh.analysis_centres(), 8, lwn)
    assert np.isnan(Fn[0]).all() and np.isfinite(Fn[1]).all()
    Q[2, 0, 0] = np.inf
    c = hh.synthesis_coefficients()[:3, :hh.count(8)].copy()
    c[1, 5] = np.nan
    f = dev_density(c, Q, 8)
    assert np.isnan(f[:, 2]).all() and np.isnan(f[1]).all() and np.isfinite(np.delete(f[[0, 2]], 2, axis=1)).all()
    assert tuple(harmonics.wigner_matrices(torch.zeros(0, 3, 3, device=DEV), 3).shape) == (0, 84)
    assert tuple(harmonics.so3_fourier_density(dev(c[0]), torch.zeros(0, 3, 3, device=DEV), 8).shape) == (0,)


def test_bit_identity_under_tiling():
    Cn, lw = hh.uniform_rotations(4099, 111), hh.weight_rows(5, 4099, 112)
    full = dev_fourier(Cn, 16, lw)
    per_group = 8 * 2 * (6545 + 2) + 4 * 4099 + 8
    assert np.array_equal(dev_fourier(Cn, 16, lw, workspace_cap=per_group), full)          # one group per call
    assert np.array_equal(dev_fourier(Cn, 16, lw, workspace_cap=2 * per_group + 1), full)   # two per call: GB = 2 blocks, the last alone
    assert np.array_equal(dev_fourier(Cn, 16, lw[3]), full[3:4])
    assert np.array_equal(dev_fourier(Cn, 7, lw), full[:, :hh.count(7)])                    # the other kernel instance, GB = 4
    with pytest.raises(ValueError, match="workspace_cap"):
        dev_fourier(Cn, 16, lw, workspace_cap=per_group - 1)
    c, Q = hh.synthesis_coefficients(), hh.synthesis_queries()
    whole = dev_density(c, Q[0], hh.SYNTHESIS_L)                                             # 5 groups: blocks of 4 and 1
    assert np.array_equal(dev_density(c[2:3], Q[0, 100:130], hh.SYNTHESIS_L)[0], whole[2, 100:130])      # a small block, GB = 1
    assert np.array_equal(dev_density(c[1:], Q[0, 250:], hh.SYNTHESIS_L), whole[1:, 250:])
    assert np.array_equal(dev_density(c, np.broadcast_to(Q[0], Q.shape).copy(), hh.SYNTHESIS_L, True), whole)
    many = np.tile(Q[0], (5, 1, 1))                                       # 1285 queries: blocks of 256 threads
    assert np.array_equal(dev_density(c, many, hh.SYNTHESIS_L)[:, 257:514], whole)


def test_graph_capture_replays_the_eager_result():
    Cn, lw, Q = dev(hh.uniform_rotations(4099, 121)), dev(hh.weight_rows(3, 4099, 122)), dev(hh.uniform_rotations(300, 123))
    h = harmonics.fisher_multipliers(4.0, 8).to(DEV)

    def step():
        F = harmonics.so3_fourier(Cn, 8, log_weights=lw)
        return [F, harmonics.so3_fourier_density(F, Q, 8, multiplier=h)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                           # a linear chain: no parallel branches
        out = step()
    for _ in range(2):
        for t in out:
            t.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))


# ---- the grid functions ------------------------------------------------------------------------------------------------------------------

def level1_posteriors():
    """(grid [576,3,3] on the device, logp [3,576] float32 numpy): one Fisher mode with kappa = 8 about an off-grid rotation, two modes,
    uniform"""
    grid = sd.generate_healpix_grid(1, device=DEV, offset=_offset(21).to(DEV))
    g = grid.cpu().numpy().astype(np.float64)
    M = hh.project(hh.uniform_rotations(2, 131))
    tr = lambda R: np.einsum("ab,qab->q", R, g)                           # noqa: E731
    lp = np.stack([8.0 * tr(M[0]), np.logaddexp(8.0 * tr(M[0]) + 0.3, 12.0 * tr(M[1])), np.zeros(len(g))])
    return grid, lp.astype(np.float32)


def test_grid_spectrum_and_diffuse_spectral_against_the_character_sums():
    grid, lp = level1_posteriors()
    g32, L = grid.cpu().numpy(), 8
    spec = harness.grid_spectrum(dev(lp), grid, L)
    w = hh.softmax_rows(lp.astype(np.float64), np.ones(576, bool))[0]
    P = hh.project(g32)
    chi = hh.characters((np.einsum("iab,jab->ij", P, P) - 1) / 2, L) * (2 * np.arange(L + 1) + 1)
    power = np.einsum("gi,gj,ijl->gl", w, w, chi)
    gl = hh.C_ENTRY * (np.arange(L + 1) + 1) * hh.EPS * (2 * np.arange(L + 1) + 1)           # |dF^l|_F
    bound = (2 * np.arange(L + 1) + 1) * (2 * np.sqrt(np.maximum(power, 0.0) / (2 * np.arange(L + 1) + 1)) * gl + gl * gl)
    got = spec["power"].cpu().numpy()
    print("grid_spectrum: power against the character sums, worst fraction of its bound", float((np.abs(got - power) / bound).max()))
    assert tuple(spec["coefficients"].shape) == (3, 969) and spec["power"].dtype == torch.float64 and (np.abs(got - power) <= bound).all()
    assert torch.equal(spec["collision"], spec["power"].sum(-1)) and torch.equal(spec["tail"], spec["power"][:, L] / spec["collision"])
    norms = np.sqrt(got[2] / (2 * np.arange(L + 1) + 1))                  # |mean_q D^l(R_q)|_F: the grid's quadrature error, not gated
    print("level 1, uniform weights: |F^l|_F =", " ".join(f"{v:.2g}" for v in norms), f"collision {float(spec['collision'][2]):.4f}")

    out = harness.grid_diffuse_spectral(dev(lp), grid, kappa=2.0, lmax=L)
    h = harmonics.fisher_multipliers(2.0, L).numpy()
    ref = hh.character_density(g32, lp, g32, h)
    c = hh.scaled(out["coefficients"].cpu().numpy().astype(np.float64), h, L).astype(np.float32)
    dens = out["density"].cpu().numpy().astype(np.float64)
    f = hh.worst(np.abs(dens - ref), hh.synthesis_gate(c, ref, L))
    print(f"grid_diffuse_spectral: {f:.3f} of the synthesis gate; negative_mass {out['negative_mass'].cpu().numpy()}, truncation {out['truncation']:.3g}")
    assert f <= 1.0 and out["density"].dtype == torch.float32 and tuple(out["density"].shape) == (3, 576)
    assert bool((out["negative_mass"] >= -1e-3).all()) and out["truncation"] == float(17 * h[8])
    assert torch.equal(out["log_density"], torch.log(out["density"].clamp(min=float(np.finfo(np.float32).tiny))))
    assert torch.equal(out["coefficients"], spec["coefficients"])
    heat = harness.grid_diffuse_spectral(dev(lp), grid, t=0.2, lmax=L)
    refh = hh.character_density(g32, lp, g32, harmonics.heat_multipliers(0.2, L).numpy())
    ch = hh.scaled(heat["coefficients"].cpu().numpy().astype(np.float64), harmonics.heat_multipliers(0.2, L).numpy(), L).astype(np.float32)
    assert hh.worst(np.abs(heat["density"].cpu().numpy() - refh), hh.synthesis_gate(ch, refh, L)) <= 1.0
    with pytest.raises(ValueError, match="grid_diffuse_local"):
        harness.grid_diffuse_spectral(dev(lp), grid, kappa=200.0, lmax=L)
    modes = harness.grid_modes(out["log_density"], grid, 2, float(np.deg2rad(30.0)))         # the result feeds the other grid functions
    assert int(modes[0][0, 0]) == int(np.argmax(dens[0]))


def test_grid_compose_against_the_restatement():
    grid, lp = level1_posteriors()
    g32, L = grid.cpu().numpy(), 8
    Fa = hh.fourier_fp64(g32, L, lp[:2])
    Fb = hh.fourier_fp64(g32, L, lp[1:2])
    D = hh.wigner_fp64(hh.project(g32), L)
    odd = 2 * np.arange(L + 1) + 1
    for invert, kappa in ((False, None), (True, None), (False, 1.5)):
        out = harness.grid_compose(dev(lp[:2]), dev(lp[1:2]), grid, lmax=L, invert_a=invert, smooth_kappa=kappa)
        h = np.ones(L + 1) if kappa is None else harmonics.fisher_multipliers(kappa, L).numpy()
        comp = np.concatenate([((hh.block(Fa, l).transpose(0, 2, 1) if invert else hh.block(Fa, l)) @ hh.block(Fb, l)).reshape(2, -1)
                               for l in range(L + 1)], axis=1)
        ref = hh.scaled(comp, h, L) @ D.T
        c = hh.scaled(out["coefficients"].cpu().numpy().astype(np.float64), h, L).astype(np.float32)
        extra = float((2.0 * odd ** 3 * h * hh.C_ENTRY * (np.arange(L + 1) + 1) * hh.EPS).sum())
        f = hh.worst(np.abs(out["density"].cpu().numpy() - ref), hh.synthesis_gate(c, ref, L) + extra)
        print(f"grid_compose(invert_a={invert}, smooth_kappa={kappa}): {f:.3f} of the gate; truncation {out['truncation']:.3g}, "
              f"negative_mass {out['negative_mass'].cpu().numpy()}")
        assert f <= 1.0 and tuple(out["density"].shape) == (2, 576)
        assert out["truncation"] == (17.0 if kappa is None else float(17 * h[8]))


def test_rotate_equals_the_analysis_of_the_shifted_set():
    L = 8
    Cn, S = hh.uniform_rotations(9, 141), hh.uniform_rotations(1, 142)[0]
    lw = hh.weight_rows(3, 9, 143)
    F = harmonics.so3_fourier(dev(Cn), L, log_weights=dev(lw))
    P, Sp = hh.project(Cn), hh.project(S[None])[0]
    gate = hh.entry_gate(L) * (2 * hh.degree_of_entry(L) + 1) * 2         # a product of two gated factors over 2l+1 terms
    left = harmonics.rotate(F, dev(S), L, side="left").cpu().numpy()
    assert (np.abs(left - hh.fourier_fp64(Sp @ P, L, lw)) <= gate).all()
    right = harmonics.rotate(F, dev(S), L, side="right").cpu().numpy()
    assert (np.abs(right - hh.fourier_fp64(P @ Sp, L, lw)) <= gate).all()


def test_grid_pose_spectrum_equals_the_spectrum_of_the_materialised_density():
    _, _, fl = _flow()
    B = 4
    feat = torch.from_numpy(synth.features(B, 32, seed=2)).cuda()
    out = harness.grid_pose_spectrum(fl, feat, lmax=8, recursion_level=1, offset=_offset())
    grid = sd.generate_healpix_grid(1, device=DEV, offset=out["offset"])
    Q = grid.shape[0]
    with torch.no_grad():
        lp = fl.log_prob(grid.repeat(B, 1, 1), feat, feature_repeat=Q)["logp"].reshape(B, Q)
    ref = harness.grid_spectrum(lp, grid, 8)
    for key in ("coefficients", "power", "collision", "tail"):
        assert torch.equal(out[key], ref[key]), key
    one = harness.grid_pose_spectrum(fl, feat, lmax=8, recursion_level=1, offset=out["offset"], images_per_launch=1)
    assert torch.equal(one["coefficients"], out["coefficients"])
    assert grid_pose.grid_pose_spectrum is harness.grid_pose_spectrum


def test_difference_to_grid_diffuse_at_level_2_is_recorded():
    """Not asserted beyond being finite: the difference is the grid's quadrature error plus the truncation."""
    grid = sd.generate_healpix_grid(2, device=DEV, offset=_offset(21).to(DEV))
    M = torch.from_numpy(hh.project(hh.uniform_rotations(1, 131))[0]).to(DEV, torch.float32)
    lp = (8.0 * (grid * M).sum(dim=(1, 2)))[None]
    dense = harness.grid_diffuse(lp, grid, 2.0).exp()
    spectral = harness.grid_diffuse_spectral(lp, grid, kappa=2.0, lmax=8)["density"]
    diff = float((dense - spectral).abs().max())
    print(f"level 2, kappa 2, L = 8: max |grid_diffuse - grid_diffuse_spectral| = {diff:.4g} at a peak density of {float(dense.max()):.4g}")
    assert np.isfinite(diff)
