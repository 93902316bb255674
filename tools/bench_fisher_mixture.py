#!/usr/bin/env python3
"""Time of the matrix-Fisher mixture fit: one EM iteration of rnf_fisher_mixture_fit at K = 1 and K = 4 for `--images` groups on the
shared level-`--level` grid (default 16 x 36,864 rows), beside rnf_rotation_moments + rnf_fisher_fit on the same inputs (the path a K = 1
iteration reproduces bit for bit), and a whole fit of `--iterations` iterations.  An iteration is the difference between a call with
T + 1 and one with 1 iterations, divided by T: a call also carries the prepare launch and the final pass.  With `--pose`, the whole
`harness.grid_pose_mixture` beside `harness.grid_pose_fisher` on the small conditional flow of the grid-search tests.  Device events
around `--launches` back-to-back calls after a warm-up, best and median of `--repeats` windows, one JSON line per case.
python tools/bench_fisher_mixture.py [--launches 10] [--level 3] [--images 16] [--pose]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rotationnormflow_amd import harness  # noqa: E402
from rotationnormflow_amd.utils import fisher, sd  # noqa: E402


def window(fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / launches            # microseconds per call


def four_mode_logp(grid, G):
    """G images' log-densities on the grid: four sharp modes 180 degrees apart about a per-image rotation (the SYMSOL-like case)."""
    sym = torch.tensor([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], device=grid.device, dtype=torch.float64)
    rot = sd.random_rotations(G).to(grid.device).double()
    A = 16.0 * rot[:, None] @ torch.diag_embed(sym)[None]                      # [G,4,3,3]
    tr = torch.einsum("qij,gkij->gqk", grid.double(), A)
    return torch.logsumexp(tr, -1).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=16, help="T of the many-iteration calls")
    ap.add_argument("--pose", action="store_true", help="also time harness.grid_pose_mixture beside harness.grid_pose_fisher")
    a = ap.parse_args()
    device = torch.cuda.get_device_name(0)
    torch.manual_seed(1)
    grid = sd.generate_healpix_grid(a.level, device=torch.device("cuda"))
    Q, G, T = grid.shape[0], a.images, a.iterations
    logp = four_mode_logp(grid, G)
    sep = float(np.deg2rad(15.0))
    starts = {}
    for K in (1, 4):
        index, _, mass, _, _ = harness.grid_modes(logp, grid, K, sep)
        starts[K] = fisher.mixture_init_from_modes(grid, index, mass, sep)

    def mixture(K, iterations):
        return lambda: fisher.fit_matrix_fisher_mixture(grid, logp, *starts[K], iterations=iterations, tol=0.0)

    cases = {
        "rotation_moments + fit_matrix_fisher": (lambda: fisher.fit_matrix_fisher(fisher.rotation_moments(grid, logp)), {}),
        "mixture K=1, 1 iteration": (mixture(1, 1), {}),
        "mixture K=1, T+1 iterations": (mixture(1, T + 1), dict(T=T)),
        "mixture K=4, 1 iteration": (mixture(4, 1), {}),
        "mixture K=4, T+1 iterations": (mixture(4, T + 1), dict(T=T)),
    }
    if a.pose:
        import contextlib
        import io
        from rotationnormflow_amd import make_config, synth
        from rotationnormflow_amd.flow.flow import Flow
        cfg = make_config(layers=4, condition=1, feature_dim=32, rot="16UnTrans", frequent_permute=1, last_affine=1, first_affine=0)
        with contextlib.redirect_stdout(io.StringIO()):
            fl = Flow(cfg)
        shapes = {k: tuple(v.shape) for k, v in fl.state_dict().items()}
        fl.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed=3, regime="trained").items()})
        fl = fl.cuda().eval()
        feat = torch.from_numpy(synth.features(G, 32, seed=21)).cuda()
        O = torch.eye(3)
        cases["grid_pose_fisher"] = (lambda: harness.grid_pose_fisher(fl, feat, recursion_level=a.level, offset=O), {})
        cases["grid_pose_mixture K=4"] = (lambda: harness.grid_pose_mixture(fl, feat, components=4, recursion_level=a.level, offset=O), {})
    med = {}
    for name, (fn, extra) in cases.items():
        window(fn, a.launches)                                  # warm-up
        us = sorted(window(fn, a.launches) for _ in range(a.repeats))
        med[name] = us[len(us) // 2]
        print(json.dumps(dict(metric="us per call", case=name, best=round(us[0], 2), median=round(us[len(us) // 2], 2), launches=a.launches,
                              repeats=a.repeats, rows=Q, images=G, device=device, **extra)), flush=True)
    for K in (1, 4):
        per = (med[f"mixture K={K}, T+1 iterations"] - med[f"mixture K={K}, 1 iteration"]) / T
        print(json.dumps(dict(metric="us per EM iteration (median of T+1 minus median of 1, over T)", case=f"mixture K={K}", value=round(per, 2),
                              T=T, rows=Q, images=G, device=device)), flush=True)


if __name__ == "__main__":
    main()
