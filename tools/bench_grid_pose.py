#!/usr/bin/env python3
"""Grid-search pose estimation (eval.py:403-462, ``log_pdf``): harness.grid_estimate_rotations on the HEALPix SO(3) grid against the plain
``flow.log_prob(..., feature_repeat=Q)`` on the same rotations materialised as one [B*Q] batch, in the same process.  One JSON line per
workload:

  symsol    settings/symsol.yml's flow (21 layers, F = 512, 16UnTrans), a batch of 128 images, number_queries 500 -> the 576-point grid
  modelnet  settings/modelnet_uni.yml's flow without the category embedding (24 layers, F = 2048, 16Trans), 128 images, 576 points
  c4_l5     C4 (24 layers, F = 256, 16UnTrans) on the 2.4 M-point level-5 evaluation grid, 16 images

    python tools/bench_grid_pose.py [--steps 5] [--only symsol,modelnet,c4_l5]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rotationnormflow_amd import harness, make_config, synth  # noqa: E402
from rotationnormflow_amd.flow.flow import Flow  # noqa: E402
from rotationnormflow_amd.utils import sd  # noqa: E402

SYMSOL = dict(layers=21, condition=1, feature_dim=512, rot="16UnTrans", frequent_permute=1, last_affine=1, first_affine=0)
MODELNET = dict(layers=24, condition=1, feature_dim=2048, rot="16Trans")
WORKLOADS = {
    "symsol": (make_config(**SYMSOL), 128, sd.closest_grid_level(500)),
    "modelnet": (make_config(**MODELNET), 128, sd.closest_grid_level(500)),
    "c4_l5": (make_config("C4"), 16, 5),
}


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, out


def run(name, cfg, B, level, steps):
    with contextlib.redirect_stdout(io.StringIO()):
        fl = Flow(cfg)
    shapes = {k: tuple(v.shape) for k, v in fl.state_dict().items()}
    fl.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_state_dict(shapes, seed=1, regime="trained").items()})
    fl = fl.cuda().eval()
    feat = torch.from_numpy(synth.features(B, fl.feature_dim, seed=3)).cuda()
    O = torch.from_numpy(synth.uniform_rotations(1, seed=4)[0]).cuda()
    Q = sd.grid_size(level)
    with torch.no_grad():
        t_grid, grid = timed(lambda: sd.generate_healpix_grid(level, device="cuda", offset=O), steps)
        t_search, (_, best, index, _) = timed(lambda: harness.grid_estimate_rotations(fl, feat, recursion_level=level, offset=O), steps)
        rows = grid.repeat(B, 1, 1)
        t_plain, res = timed(lambda: fl.log_prob(rows, feat, feature_repeat=Q), steps)
        lp = res["logp"].reshape(B, Q)
        same = bool(torch.equal(torch.argmax(lp, -1), index) and torch.equal(lp.max(-1).values, best))
    del rows, res, lp
    torch.cuda.empty_cache()
    n = B * Q
    return dict(metric="grid-search pose estimate (log_pdf)", workload=name, layers=cfg.layers, feature_dim=cfg.feature_dim, rot=cfg.rot,
                images=B, level=level, grid_rows=Q, rotations=n, grid_ms=t_grid * 1e3, search_ms=t_search * 1e3,
                ms_per_image=t_search * 1e3 / B, rot_per_s=n / t_search, plain_log_prob_ms=t_plain * 1e3, plain_rot_per_s=n / t_plain,
                rate_vs_plain=t_plain / t_search, grid_share_of_one_image=t_grid / (t_search / B), same_as_plain=same)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    a = ap.parse_args()
    for name in a.only.split(","):
        cfg, B, level = WORKLOADS[name]
        print(json.dumps(run(name, cfg, B, level, a.steps)), flush=True)


if __name__ == "__main__":
    main()
