#!/usr/bin/env python3
"""The moments of the pairwise matrix-Fisher kernel sum (rnf_so3_kernel_moments: utils/kde.py so3_kernel_moments, mean shift,
grid_pose.grid_modes_refine) against torch autograd through the chunked eager difference-form expression -- the only thing a user could
run before it, kept in this tool and on no product path -- in one process, the calls alternating step by step, median.  One JSON line
per case:

  moments     2^20 queries against 2^14 centres: log-density and the responsibility-weighted mean (1.7e10 pairs)
  mean_shift  32 mean-shift steps of 1024 starts on 2^16 centres (2.1e9 pairs)
  refine      32 mean-shift steps of the 4 grid modes of 16 images at level 3 (36,864 rows, one set of queries per image: 7.5e7 pairs)

    python tools/bench_so3_moments.py [--steps 5] [--only moments,mean_shift,refine] [--clock-seconds 3]

The eager arm gets the mean from the gradient, M = Q + grad / kappa, and projects with torch.linalg.svd.  Each line carries pairs/s of
both arms and the issue bound of the kernel: ISSUE_SLOTS vector-issue slots per pair over 256 CUs x 4 SIMDs x 32 lanes per cycle at the
shader clock observed while the HIP arm alone runs back to back (tools/bench_so3_kde.py observed_clock_ghz).  Kernel-only times come
from a separate trace of the HIP arm alone:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_so3_moments.py --trace-only --steps 3"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_so3_kde import LANES, TORCH_TILE, clustered, median_ms, observed_clock_ghz  # noqa: E402
from rotationnormflow_amd import harness  # noqa: E402
from rotationnormflow_amd.utils import kde, sd  # noqa: E402

# Vector-issue slots per pair of so3_kernel_moments_kernel, both sweeps, from its gfx950 disassembly.  First sweep (ks::tile_pass): 9 v_sub
# + 9 v_fma + 1 v_min for d2, 1 v_fma for the exponent, 1/2 v_max3: 20.5.  Second sweep: the same 19 for d2, then v_fma, v_sub, v_exp_f32
# (counted as 4, as tools/bench_so3_kde.py counts it), v_add for sum e, 1 v_fma for sum e d2 and 9 v_fma with the centre's entries as
# scalar operands: 36.  With log-weights each sweep adds 1 v_mul.
ISSUE_SLOTS = 20.5 + 36.0


def torch_moments(Cn, Qr, kappa, lw=None):
    """log-density [m] and mean [m,3,3] by autograd through the chunked eager expression: M = Q + grad / kappa"""
    n, m = Cn.shape[0], Qr.shape[0]
    c9 = Cn.reshape(n, 9)
    log_w = torch.log_softmax((torch.zeros(n, device=Cn.device) if lw is None else lw).double(), dim=0).float()
    k2 = torch.tensor(2.0 * kappa, dtype=torch.float64)
    l = float(torch.log(torch.special.i0e(k2) - torch.special.i1e(k2))) if kappa > 0 else 0.0
    lp, mean = torch.empty(m, device=Cn.device), torch.empty(m, 9, device=Cn.device)
    step = max(1, TORCH_TILE // n)
    with torch.enable_grad():
        for i0 in range(0, m, step):
            q = Qr.reshape(m, 9)[i0:i0 + step].detach().clone().requires_grad_(True)
            d2 = torch.zeros(q.shape[0], n, device=Cn.device)
            for k in range(9):
                d2 = d2 + (q[:, k, None] - c9[None, :, k]) ** 2
            r = torch.logsumexp(log_w[None, :] - (0.5 * kappa) * d2, dim=1) - l
            (g,) = torch.autograd.grad(r.sum(), q)
            lp[i0:i0 + step] = r.detach()
            mean[i0:i0 + step] = q.detach() + g / kappa
    return lp, mean.reshape(m, 3, 3)


def torch_mean_shift(Cn, starts, kappa, steps, lw=None):
    cur = starts.clone()
    for _ in range(steps):
        _, M = torch_moments(Cn, cur, kappa, lw)
        U, _, Vh = torch.linalg.svd(M)
        cur = U @ Vh
    return cur


def hip_refine(logp, grid, start, kappa, steps):
    return harness.grid_modes_refine(logp, grid, start, kappa=kappa, tol=1e-30, max_steps=steps, check_every=steps)[0]


def torch_refine(logp, grid, start, kappa, steps):
    return torch.stack([torch_mean_shift(grid, start[b], kappa, steps, logp[b]) for b in range(logp.shape[0])])


def cases():
    C14, Q20 = clustered(1 << 14, 2), clustered(1 << 20, 3)
    C16 = clustered(1 << 16, 1)
    S = C16[::64].contiguous()
    est = kde.SO3KernelDensity(C16, 32.0)
    grid = sd.generate_healpix_grid(3, device="cuda")
    torch.manual_seed(3)
    logp = 3.0 * torch.randn(16, grid.shape[0], device="cuda")
    index = harness.grid_modes(logp, grid, 4, 0.2618)[0]
    start = grid[index.clamp(min=0)].contiguous()
    kr = 0.5 / (8.0 * 3.141592653589793 ** 2 / grid.shape[0]) ** (2.0 / 3.0)
    return {
        "moments": dict(pairs=float(1 << 34), hip=lambda: kde.so3_kernel_moments(C14, Q20, 64.0)["mean"],
                        eager=lambda: torch_moments(C14, Q20, 64.0)[1]),
        "mean_shift": dict(pairs=32.0 * 1024 * (1 << 16),
                           hip=lambda: est.mean_shift(S, tol=1e-30, max_steps=32, check_every=32)[0],
                           eager=lambda: torch_mean_shift(C16, S, 32.0, 32)),
        "refine": dict(pairs=32.0 * 16 * 4 * grid.shape[0], slots=ISSUE_SLOTS + 2.0, hip=lambda: hip_refine(logp, grid, start, kr, 32),
                       eager=lambda: torch_refine(logp, grid, start, kr, 32)),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="moments,mean_shift,refine")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="stands in where the clock cannot be observed")
    ap.add_argument("--clock-seconds", type=float, default=3.0, help="how long the HIP arm runs for the clock samples (0: skip)")
    ap.add_argument("--trace-only", action="store_true", help="run only the HIP arm, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_so3_moments: no GPU; there is nothing to measure on a CPU")
    all_cases = cases()
    for name in a.only.split(","):
        case = all_cases[name]
        if a.trace_only:
            for _ in range(a.steps + 1):
                case["hip"]()
            torch.cuda.synchronize()
            continue
        ms, out = median_ms({"hip": case["hip"], "eager": case["eager"]}, a.steps)
        diff = (out["hip"].double() - out["eager"].double()).abs()
        clock = observed_clock_ghz(case["hip"], a.clock_seconds) if a.clock_seconds > 0 else None
        slots = case.get("slots", ISSUE_SLOTS)
        bound = LANES * (clock or a.clock_ghz) * 1e9 / slots
        print(json.dumps(dict(metric="moments of the pairwise matrix-Fisher kernel sum on SO(3)", case=name, steps=a.steps, pairs=case["pairs"],
                              hip_ms=ms["hip"], eager_ms=ms["eager"], eager_over_hip=ms["eager"] / ms["hip"],
                              hip_pairs_per_s=case["pairs"] / ms["hip"] * 1e3, eager_pairs_per_s=case["pairs"] / ms["eager"] * 1e3,
                              issue_slots_per_pair=slots, clock_ghz=clock or a.clock_ghz, clock_observed=clock is not None,
                              issue_bound_pairs_per_s=bound, hip_share_of_issue_bound=case["pairs"] / ms["hip"] * 1e3 / bound,
                              max_abs_difference=float(diff[torch.isfinite(diff)].max()))), flush=True)


if __name__ == "__main__":
    main()
