#!/usr/bin/env python3
"""Draws from SO(3) grid posteriors (harness.grid_sample) against the torch expression they replace,

    pick = torch.multinomial(torch.softmax(logp, 1), n, True);  rotations = grid[pick]

(rows only: no jitter, no log_prob, and no more than 2^24 grid rows), in one process, the calls alternating step by step, median of
--steps runs after a warm-up.  16 images of a two-peaked density at levels 3 and 5 with n = 4096 and n = 2^20 draws per image, then one
image at level 6 (18.9 M rows), where the torch expression cannot run.  One JSON line per case:

    python tools/time_grid_sample.py [--steps 7] [--only l3,l5,l6]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rotationnormflow_amd import harness, synth  # noqa: E402
from rotationnormflow_amd.utils import sd  # noqa: E402

CASES = {"l3": (3, 16), "l5": (5, 16), "l6": (6, 1)}       # level, images
DRAWS = (4096, 1 << 20)
TORCH_MAX_ROWS = 1 << 24


def median_ms(calls, steps):
    times = {k: [] for k in calls}
    with torch.no_grad():
        for fn in calls.values():                           # warm-up: workspaces, code objects
            fn()
        for _ in range(steps):
            for key, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[key].append(time.perf_counter() - t0)
    return {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}


def density(grid, g):
    """g rows of log(0.6 exp(12 (tr(A^T R) - 3)) + 0.4 exp(6 (tr(B^T R) - 3)) + 1e-6) on the grid's rows -> float32 [g,Q]"""
    R = torch.from_numpy(synth.uniform_rotations(2 * g, seed=12)).cuda().reshape(2, g, 9)
    flat = grid.reshape(-1, 9)
    a, b = flat @ R[0].T - 3.0, flat @ R[1].T - 3.0        # [Q,g]
    return torch.log(0.6 * torch.exp(12.0 * a) + 0.4 * torch.exp(6.0 * b) + 1e-6).T.contiguous()


def torch_draws(lp, grid, n):
    pick = torch.multinomial(torch.softmax(lp, 1), n, True)
    return grid[pick]


def run(name, steps):
    level, g = CASES[name]
    grid = sd.generate_healpix_grid(level, device="cuda")
    lp = density(grid, g)
    Q = grid.shape[0]
    rows = []
    for n in DRAWS:
        calls = {"systematic_jitter": lambda: harness.grid_sample(lp, n, recursion_level=level, seed=1),
                 "multinomial_jitter": lambda: harness.grid_sample(lp, n, recursion_level=level, method="multinomial", seed=1),
                 "multinomial_rows": lambda: harness.grid_sample(lp, n, recursion_level=level, method="multinomial", jitter=False, seed=1)}
        if Q <= TORCH_MAX_ROWS:
            calls["torch_multinomial"] = lambda: torch_draws(lp, grid, n)
        ms = median_ms(calls, steps)
        rows.append(dict(metric="draws from SO(3) grid posteriors", case=name, level=level, grid_rows=Q, images=g, draws_per_image=n, steps=steps,
                         **{k + "_ms": round(v, 4) for k, v in ms.items()},
                         torch_vs_multinomial_rows=round(ms["torch_multinomial"] / ms["multinomial_rows"], 3) if "torch_multinomial" in ms else None))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--only", default="l3,l5,l6")
    a = ap.parse_args()
    for name in a.only.split(","):
        for row in run(name, a.steps):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
