#!/usr/bin/env python3
"""Coarse-to-fine beam search (harness.grid_beam_estimate_rotations) against the full grid search (harness.grid_estimate_rotations) at
the same level, in one process, the two calls alternating step by step.  One JSON line per workload: median ms of each, rows evaluated
per image, and the share of images whose beam estimate is the full search's arg-max (same row):

  c4_l5      C4 (24 layers, F = 256), 16 images, level 5 (2.4 M rows per image)
  c4_l6      C4, 16 images, level 6 (18.9 M rows per image)
  symsol_l5  the SYMSOL shape (21 layers, F = 512), 128 images, level 5
  trained_c4_l5  C4 with the weights of tests/golden/trained_c4.pth (the reference's own training), its first 16 test features, level 5

The synthetic workloads' weights (synth.fill_state_dict) give rough, many-moded densities; trained_c4_l5 is the concentrated density the
beam search is meant for.

    python tools/bench_grid_beam.py [--steps 3] [--only c4_l5,c4_l6,symsol_l5] [--start 2] [--beam 16]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_grid_modes import setup  # noqa: E402
from bench_grid_pose import SYMSOL  # noqa: E402
from rotationnormflow_amd import harness, make_config, synth  # noqa: E402
from rotationnormflow_amd.utils import sd  # noqa: E402

WORKLOADS = {
    "c4_l5": (make_config("C4"), 16, 5),
    "c4_l6": (make_config("C4"), 16, 6),
    "symsol_l5": (make_config(**SYMSOL), 128, 5),
    "trained_c4_l5": (make_config("C4"), 16, 5),
}


def trained(name, B):
    from tests.trained_helpers import load_trained
    cfg, ckpt, _, fx, _ = load_trained(name)
    fl = harness.build_flow_from_checkpoint(cfg, ckpt)
    O = torch.from_numpy(synth.uniform_rotations(1, seed=4)[0]).cuda()
    return fl, torch.from_numpy(fx["test_feat"][:B]).cuda(), O


def run(name, cfg, B, level, start, beam, steps):
    fl, feat, O = trained("trained_c4", B) if name.startswith("trained_c4") else setup(cfg, B)
    calls = {"full": lambda: harness.grid_estimate_rotations(fl, feat, recursion_level=level, offset=O),
             "beam": lambda: harness.grid_beam_estimate_rotations(fl, feat, recursion_level=level, start_level=start, beam=beam, offset=O)}
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
    full, bm = out["full"], out["beam"]
    rows_beam = sd.grid_size(start) + beam * 12 * (level - start)
    return dict(metric="coarse-to-fine beam search on the SO(3) grid", workload=name, layers=cfg.layers, feature_dim=cfg.feature_dim,
                images=B, level=level, start_level=start, beam=beam, steps=steps, full_ms=ms["full"], beam_ms=ms["beam"],
                speedup=ms["full"] / ms["beam"], rows_per_image_full=sd.grid_size(level), rows_per_image_beam=rows_beam,
                agreement=float((bm[2] == full[2]).double().mean()), beam_le_full=bool((bm[1] <= full[1]).all()),
                mean_logp_gap=float((full[1] - bm[1]).double().mean()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--start", type=int, default=2)
    ap.add_argument("--beam", type=int, default=16)
    a = ap.parse_args()
    for name in a.only.split(","):
        cfg, B, level = WORKLOADS[name]
        print(json.dumps(run(name, cfg, B, level, a.start, a.beam, a.steps)), flush=True)


if __name__ == "__main__":
    main()
