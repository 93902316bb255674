#!/usr/bin/env python3
"""Credible sets with a ground truth (harness.grid_pose_credible, three levels) against the plain grid search
(harness.grid_estimate_rotations) on the workloads of tools/bench_grid_pose.py, in one process, the calls alternating step by step, median.
One JSON line per workload:

  symsol    21 layers, F = 512, 16UnTrans, 128 images on the 576-point grid
  modelnet  24 layers, F = 2048, 16Trans, 128 images on the 576-point grid
  c4_l5     C4 on the 2.4 M-point level-5 evaluation grid, 16 images

    python tools/bench_grid_credible.py [--steps 5] [--only symsol,modelnet,c4_l5]

The reduction's kernel-only times come from a separate trace of the credible call alone (no timing of its own):

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_grid_credible.py --trace-only --steps 3"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_grid_modes import setup  # noqa: E402
from bench_grid_pose import WORKLOADS  # noqa: E402
from rotationnormflow_amd import harness, synth  # noqa: E402
from rotationnormflow_amd.utils import sd  # noqa: E402

LEVELS = (0.5, 0.9, 0.95)


def ground_truths(B):
    return torch.from_numpy(synth.uniform_rotations(B, seed=5)).cuda()


def run(name, cfg, B, level, steps):
    fl, feat, O = setup(cfg, B)
    gt = ground_truths(B)
    calls = {"search": lambda: harness.grid_estimate_rotations(fl, feat, recursion_level=level, offset=O),
             "credible": lambda: harness.grid_pose_credible(fl, feat, levels=LEVELS, recursion_level=level, offset=O, gt_rotation=gt),
             "modes_k4": lambda: harness.grid_pose_modes(fl, feat, top_k=4, recursion_level=level, offset=O)}
    times = {k: [] for k in calls}
    out = {}
    with torch.no_grad():
        for fn in calls.values():                       # warm-up: packing, workspaces, code objects
            fn()
        for _ in range(steps):
            for key, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[key] = fn()
                torch.cuda.synchronize()
                times[key].append(time.perf_counter() - t0)
    ms = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
    cr = out["credible"]
    return dict(metric="credible sets and ground-truth HPD level on the SO(3) grid", workload=name, layers=cfg.layers,
                feature_dim=cfg.feature_dim, images=B, level=level, grid_rows=sd.grid_size(level), steps=steps, levels=LEVELS,
                search_ms=ms["search"], credible_ms=ms["credible"], modes_k4_ms=ms["modes_k4"],
                credible_vs_search=ms["credible"] / ms["search"], credible_vs_modes_k4=ms["credible"] / ms["modes_k4"],
                log_norm_same_as_modes=bool(float((cr["log_norm"] - out["modes_k4"]["log_norm"]).abs().max()) <= 1e-6),
                mean_volume=[round(float(x), 6) for x in cr["volume"].mean(0)], mean_mass=[round(float(x), 6) for x in cr["mass"].mean(0)],
                mean_gt_level=float(cr["gt_level"].mean()), coverage=[round(float(x), 4) for x in cr["gt_inside"].float().mean(0)])


def trace_only(name, cfg, B, level, steps):
    fl, feat, O = setup(cfg, B)
    gt = ground_truths(B)
    with torch.no_grad():
        for _ in range(steps + 1):
            harness.grid_pose_credible(fl, feat, levels=LEVELS, recursion_level=level, offset=O, gt_rotation=gt)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--trace-only", action="store_true", help="run only grid_pose_credible, for a kernel trace")
    a = ap.parse_args()
    for name in a.only.split(","):
        cfg, B, level = WORKLOADS[name]
        if a.trace_only:
            trace_only(name, cfg, B, level, a.steps)
        else:
            print(json.dumps(run(name, cfg, B, level, a.steps)), flush=True)


if __name__ == "__main__":
    main()
