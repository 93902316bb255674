#!/usr/bin/env python3
"""Top-k pose modes (harness.grid_pose_modes) against the plain grid search (harness.grid_estimate_rotations) on the workloads of
tools/bench_grid_pose.py, in one process, the three calls alternating step by step.  One JSON line per workload:

  symsol    21 layers, F = 512, 16UnTrans, 128 images on the 576-point grid
  modelnet  24 layers, F = 2048, 16Trans, 128 images on the 576-point grid
  c4_l5     C4 on the 2.4 M-point level-5 evaluation grid, 16 images

    python tools/bench_grid_modes.py [--steps 5] [--only symsol,modelnet,c4_l5]

The reduction's kernel-only time comes from a separate trace of the modes call alone (no timing of its own):

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_grid_modes.py --trace-only --steps 3"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_grid_pose import WORKLOADS  # noqa: E402
from rotationnormflow_amd import harness, synth  # noqa: E402
from rotationnormflow_amd.flow.flow import Flow  # noqa: E402
from rotationnormflow_amd.utils import sd  # noqa: E402


def setup(cfg, B):
    with contextlib.redirect_stdout(io.StringIO()):
        fl = Flow(cfg)
    shapes = {k: tuple(v.shape) for k, v in fl.state_dict().items()}
    fl.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed=1, regime="trained").items()})
    fl = fl.cuda().eval()
    feat = torch.from_numpy(synth.features(B, fl.feature_dim, seed=3)).cuda()
    O = torch.from_numpy(synth.uniform_rotations(1, seed=4)[0]).cuda()
    return fl, feat, O


def run(name, cfg, B, level, steps):
    fl, feat, O = setup(cfg, B)
    calls = {"search": lambda: harness.grid_estimate_rotations(fl, feat, recursion_level=level, offset=O),
             "modes_k1": lambda: harness.grid_pose_modes(fl, feat, top_k=1, recursion_level=level, offset=O),
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
    search, m4 = out["search"], out["modes_k4"]
    same = bool(torch.equal(search[2], m4["index"][:, 0]) and torch.equal(search[1], m4["log_prob"][:, 0]))
    return dict(metric="top-k pose modes on the SO(3) grid", workload=name, layers=cfg.layers, feature_dim=cfg.feature_dim, images=B,
                level=level, grid_rows=sd.grid_size(level), steps=steps, search_ms=ms["search"], modes_k1_ms=ms["modes_k1"],
                modes_k4_ms=ms["modes_k4"], k1_vs_search=ms["modes_k1"] / ms["search"], k4_vs_search=ms["modes_k4"] / ms["search"],
                mode0_same_as_search=same, mean_mass_k4=[round(float(x), 4) for x in m4["mass"].mean(0)],
                mean_log_norm=float(m4["log_norm"].mean()))


def trace_only(name, cfg, B, level, steps):
    fl, feat, O = setup(cfg, B)
    with torch.no_grad():
        for _ in range(steps + 1):
            harness.grid_pose_modes(fl, feat, top_k=4, recursion_level=level, offset=O)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--trace-only", action="store_true", help="run only grid_pose_modes(top_k=4), for a kernel trace")
    a = ap.parse_args()
    for name in a.only.split(","):
        cfg, B, level = WORKLOADS[name]
        if a.trace_only:
            trace_only(name, cfg, B, level, a.steps)
        else:
            print(json.dumps(run(name, cfg, B, level, a.steps)), flush=True)


if __name__ == "__main__":
    main()
