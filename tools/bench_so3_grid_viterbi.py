#!/usr/bin/env python3
"""One frame of the two recursions on the SO(3) grid (grid_pose.grid_viterbi, grid_pose.grid_smooth) next to one frame of the filter
(grid_pose.grid_filter_step), on the same box.  One process, the arms alternating step by step, median.  One JSON line per case:

  level3, level4, level5   4 sequences, kappa = 264.1 (default radius 15 degrees): a grid_viterbi step (log-weights delta - log Z in fp64,
                           the max-plus pass rnf_so3_grid_local_max, the likelihood, re-centring, the back-pointers), a grid_smooth
                           backward step (log-weights l + b in fp64, the sum pass, - log Z - log Q - log evidence), the two passes alone,
                           and grid_filter_step.  log Z is precomputed for the two recursions as they do once per sequence;
                           grid_filter_step recomputes it every step, so its time holds two sum passes.
  level3 also              a chunked dense torch max-plus over all Q^2 pairs (fp32, 2 048 queries per chunk): what the step would cost
                           without the neighbourhoods, and whether it picks the same predecessors.

    python tools/bench_so3_grid_viterbi.py [--steps 5] [--only level3,level4,level5]

What is reported is what was measured here, nothing else: in particular the share of a sum pass that a max pass costs (expected about 29
of 53 issue slots per row looked at, DESIGN.md 3.3h, never measured before) is the ratio of the two ``*_pass_ms`` figures."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_so3_kde import median_ms  # noqa: E402
from rotationnormflow_amd import harness  # noqa: E402
from rotationnormflow_amd.utils import kde, sd  # noqa: E402

KAPPA, SEQUENCES = 264.1, 4


def frames(grid, seed):
    """Two frames' log-likelihoods [SEQUENCES, 2, Q]: a sharp bump per sequence that moves a few degrees, on a floor"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    Q = grid.shape[0]
    modes = grid[torch.randint(0, Q, (SEQUENCES,), device="cuda", generator=gen)]
    small = torch.linalg.matrix_exp(0.05 * torch.tensor([[0.0, -1.0, 0.5], [1.0, 0.0, -0.3], [-0.5, 0.3, 0.0]], device="cuda"))
    both = torch.stack([modes, modes @ small], dim=1)                                              # [S,2,3,3]
    tr = torch.einsum("qij,stij->stq", grid, both)
    return torch.log(torch.exp(100.0 * (tr - 3.0)) + 1e-6)


def dense_max_plus(grid, lw, kappa, chunk=2048):
    """max_j (lw[g][j] - (kappa/2) d^2(G_j, G_i)) and its arg over ALL rows, in fp32 torch, chunked over the queries"""
    G9 = grid.reshape(-1, 9)
    best, arg = [], []
    for i0 in range(0, G9.shape[0], chunk):
        d2 = (6.0 - 2.0 * G9[i0:i0 + chunk] @ G9.T).clamp_min(0.0)                                 # |a - b|^2 = 6 - 2 tr(a^T b) for rotations
        v, a = (lw[:, None, :] - 0.5 * kappa * d2[None]).max(dim=2)
        best.append(v)
        arg.append(a)
    return torch.cat(best, dim=1), torch.cat(arg, dim=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="level3,level4,level5")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_so3_grid_viterbi: no GPU; there is nothing to measure on a CPU")
    for name in a.only.split(","):
        level = int(name[-1])
        grid = sd.generate_healpix_grid(level, device="cuda")
        Q = grid.shape[0]
        log_q = math.log(Q)
        ll = frames(grid, level)
        lz = kde.so3_grid_local_log_sum(grid, level, KAPPA).double() - log_q                       # log Z_j, once per sequence
        first = harness.grid_filter_step(torch.zeros(SEQUENCES, Q, device="cuda"), ll[:, 0], grid, level, KAPPA)
        post, ev = first["posterior"], first["log_evidence"]
        delta = post                                                                               # a re-centred delta looks like a posterior
        b_next = torch.zeros(SEQUENCES, Q, device="cuda")
        lw_fixed = (delta.double() - lz).float()

        def viterbi_step():
            lw = (delta.double() - lz).float()
            best, arg = kde.so3_grid_local_log_max(grid, level, KAPPA, log_weights=lw)
            d = ll[:, 1].double() + best.double() - log_q
            top = d.max(dim=1).values
            return (d - top[:, None]).float(), arg.to(torch.int32), top

        def smooth_backward_step():
            lw = (ll[:, 1].double() + b_next.double()).float()
            s = kde.so3_grid_local_log_sum(grid, level, KAPPA, log_weights=lw)
            return (s.double() - lz - log_q - ev[:, None]).float()

        calls = {"viterbi_step": viterbi_step, "smooth_backward_step": smooth_backward_step,
                 "filter_step": lambda: harness.grid_filter_step(post, ll[:, 1], grid, level, KAPPA)["posterior"],
                 "max_pass": lambda: kde.so3_grid_local_log_max(grid, level, KAPPA, log_weights=lw_fixed),
                 "sum_pass": lambda: kde.so3_grid_local_log_sum(grid, level, KAPPA, log_weights=lw_fixed)}
        if level == 3:
            calls["dense_torch_max_plus"] = lambda: dense_max_plus(grid, lw_fixed, KAPPA)
        ms, out = median_ms(calls, a.steps)
        count = kde.so3_grid_local_log_sum(grid, level, KAPPA, return_count=True)[1]
        line = dict(metric="one frame of the recursions on the SO(3) grid", case=name, level=level, rows=Q, sequences=SEQUENCES, kappa=KAPPA,
                    radius_deg=math.degrees(math.acos(1.0 - kde.local_default_d2_cut(KAPPA) / 4.0)), steps=a.steps,
                    mean_neighbours=float(count.double().mean()), viterbi_step_ms=ms["viterbi_step"],
                    smooth_backward_step_ms=ms["smooth_backward_step"], filter_step_ms=ms["filter_step"], max_pass_ms=ms["max_pass"],
                    sum_pass_ms=ms["sum_pass"], max_over_sum_pass=ms["max_pass"] / ms["sum_pass"])
        if level == 3:
            arg = out["max_pass"][1]
            same = (out["dense_torch_max_plus"][1] == arg)[arg >= 0].double().mean()
            line.update(dense_torch_max_plus_ms=ms["dense_torch_max_plus"], dense_over_max_pass=ms["dense_torch_max_plus"] / ms["max_pass"],
                        dense_picks_the_same_predecessor=float(same))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
