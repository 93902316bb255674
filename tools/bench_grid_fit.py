#!/usr/bin/env python3
"""Samples against the density on the SO(3) grid (harness.grid_pose_fit with one ground truth per image) against the plain grid search
(harness.grid_estimate_rotations) on workloads of tools/bench_grid_pose.py, and the locate + histogram of 2^20 rotations, in one process,
the calls alternating step by step, median.  One JSON line for the histogram, then one per workload:

  symsol    21 layers, F = 512, 16UnTrans, 128 images on the 576-point grid
  c4_l5     C4 on the 2.4 M-point level-5 evaluation grid, 16 images

    python tools/bench_grid_fit.py [--steps 5] [--only symsol,c4_l5]

The kernel-only times of the locate kernel and of the fit reduction (next to the modes and credible reductions on the same rows) come
from a separate trace of those calls alone (no timing of its own):

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_grid_fit.py --trace-only --steps 3"""
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

HISTOGRAM_ROTATIONS = 1 << 20
HISTOGRAM_LEVELS = (2, 5)
TRACE_LEVEL, TRACE_IMAGES = 5, 16


def median_ms(calls, steps):
    times = {k: [] for k in calls}
    out = {}
    with torch.no_grad():
        for fn in calls.values():                           # warm-up: packing, workspaces, code objects
            fn()
        for _ in range(steps):
            for key, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[key] = fn()
                torch.cuda.synchronize()
                times[key].append(time.perf_counter() - t0)
    return {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}, out


def histogram(steps):
    R = torch.from_numpy(synth.uniform_rotations(HISTOGRAM_ROTATIONS, seed=6)).cuda()
    O = torch.from_numpy(synth.uniform_rotations(1, seed=4)[0]).cuda()
    calls = {}
    for level in HISTOGRAM_LEVELS:
        calls[f"index_l{level}"] = lambda level=level: sd.grid_index(R, level, O)
        calls[f"histogram_l{level}"] = lambda level=level: sd.grid_histogram(R, level, O)
    ms, out = median_ms(calls, steps)
    return dict(metric="locate and histogram of rotations on the SO(3) grid", rotations=HISTOGRAM_ROTATIONS, steps=steps,
                occupied={k: int((v > 0).sum()) for k, v in out.items() if k.startswith("histogram")},
                **{k + "_ms": v for k, v in ms.items()})


def run(name, cfg, B, level, steps):
    fl, feat, O = setup(cfg, B)
    gt = torch.from_numpy(synth.uniform_rotations(B, seed=5)).cuda().reshape(B, 1, 3, 3)
    calls = {"search": lambda: harness.grid_estimate_rotations(fl, feat, recursion_level=level, offset=O),
             "fit": lambda: harness.grid_pose_fit(fl, feat, samples=gt, recursion_level=level, offset=O),
             "credible": lambda: harness.grid_pose_credible(fl, feat, recursion_level=level, offset=O, gt_rotation=gt[:, 0])}
    ms, out = median_ms(calls, steps)
    return dict(metric="ground truths against the density on the SO(3) grid", workload=name, layers=cfg.layers, feature_dim=cfg.feature_dim,
                images=B, level=level, grid_rows=sd.grid_size(level), steps=steps, search_ms=ms["search"], fit_ms=ms["fit"],
                credible_ms=ms["credible"], fit_vs_search=ms["fit"] / ms["search"],
                log_norm_same_as_credible=bool(float((out["fit"]["log_norm"] - out["credible"]["log_norm"].double()).abs().max()) <= 1e-6),
                mean_grid_log_likelihood=float(out["fit"]["grid_log_likelihood"].mean()))


def trace_only(steps):
    """The reductions alone, on rows at hand: locate + histogram of 2^20 rotations, and fit, modes (k = 1) and credible on 16 level-5 rows."""
    R = torch.from_numpy(synth.uniform_rotations(HISTOGRAM_ROTATIONS, seed=6)).cuda()
    O = torch.from_numpy(synth.uniform_rotations(1, seed=4)[0]).cuda()
    grid = sd.generate_healpix_grid(TRACE_LEVEL, device="cuda", offset=O)
    torch.manual_seed(0)
    lp = torch.randn(TRACE_IMAGES, grid.shape[0], device="cuda")
    for _ in range(steps + 1):
        for level in HISTOGRAM_LEVELS:
            sd.grid_histogram(R, level, O)
        counts = sd.grid_histogram(R[None].expand(TRACE_IMAGES, -1, -1, -1), TRACE_LEVEL, O)
        harness.grid_fit(lp, counts)
        harness.grid_modes(lp, grid, 1, 0.25)
        harness.grid_credible(lp, (0.5, 0.9, 0.95))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="symsol,c4_l5")
    ap.add_argument("--trace-only", action="store_true", help="run only the reductions, for a kernel trace")
    a = ap.parse_args()
    if a.trace_only:
        trace_only(a.steps)
        return
    print(json.dumps(histogram(a.steps)), flush=True)
    for name in a.only.split(","):
        cfg, B, level = WORKLOADS[name]
        print(json.dumps(run(name, cfg, B, level, a.steps)), flush=True)


if __name__ == "__main__":
    main()
