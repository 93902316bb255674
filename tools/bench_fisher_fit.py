#!/usr/bin/env python3
"""Time of the matrix-Fisher fitting kernels: rnf_rotation_moments on the level-5 shared grid (2,359,296 rows, 16 images' log-densities)
beside the torch expression that computes the same moments without it, `(softmax(logp, -1)[..., None, None].double() * grid.double()).sum(1)`,
and rnf_fisher_fit at B = 4096.  Device events around `--launches` back-to-back calls after a warm-up, best and median of `--repeats`
windows, one JSON line per case; the moment kernel's line carries the bytes it has to read and the fraction of `--hbm-gbs` that is.
python tools/bench_fisher_fit.py [--launches 10] [--level 5] [--images 16]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rotationnormflow_amd.utils import fisher, sd  # noqa: E402


def window(fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / launches            # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--level", type=int, default=5)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the fraction is taken of (MI355X: 8 TB/s)")
    a = ap.parse_args()
    device = torch.cuda.get_device_name(0)
    grid = sd.generate_healpix_grid(a.level, device=torch.device("cuda"))
    Q, G = grid.shape[0], a.images
    gen = torch.Generator(device="cuda").manual_seed(1)
    logp = torch.randn(G, Q, device="cuda", generator=gen) * 3.0
    # every image reads its own log-densities once; the grid is shared and has to come from memory at least once
    least = 4 * G * Q + 36 * Q
    most = 4 * G * Q * 2 + 36 * Q * G                            # the maximum pass reads logp again; each image's blocks read the grid

    def torch_moments():
        return (torch.softmax(logp, -1)[..., None, None].double() * grid.double()).sum(1)

    err = (fisher.rotation_moments(grid, logp) - torch_moments()).abs().max().item()
    M = fisher.rotation_moments(torch.from_numpy(np.random.default_rng(2).standard_normal((4096, 64, 3, 3)).astype(np.float32)).cuda() * 0.2)
    cases = {
        "rnf_rotation_moments": (lambda: fisher.rotation_moments(grid, logp), dict(rows=Q, images=G)),
        "torch softmax * grid": (torch_moments, dict(rows=Q, images=G)),
        "rnf_fisher_fit": (lambda: fisher.fit_matrix_fisher(M), dict(B=4096)),
    }
    for name, (fn, extra) in cases.items():
        window(fn, a.launches)                                  # warm-up
        us = sorted(window(fn, a.launches) for _ in range(a.repeats))
        rec = dict(metric="us per call", case=name, best=round(us[0], 2), median=round(us[len(us) // 2], 2), launches=a.launches,
                   repeats=a.repeats, device=device, **extra)
        if name == "rnf_rotation_moments":
            med = us[len(us) // 2] * 1e-6
            rec.update(max_abs_diff_to_torch=err, bytes_least=least, bytes_requested=most,
                       hbm_fraction_least=round(least / med / (a.hbm_gbs * 1e9), 4), gbs_requested=round(most / med / 1e9, 1))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
