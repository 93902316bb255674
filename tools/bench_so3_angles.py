#!/usr/bin/env python3
"""The distribution function of the geodesic angle (rnf_so3_angle_cdf: utils/angles.py so3_angle_cdf and so3_angle_quantile,
grid_pose.grid_error, grid_pose.grid_ball_estimate) against the chunked torch-eager difference-form expression with ``<=`` and a weighted
sum -- the only thing a user could run before it, kept in this tool and on no product path -- in one process, the calls alternating
step by step, median.  One JSON line per case:

  mass        2^20 queries against 2^14 centres, 8 thresholds, masses only (1.7e10 pairs)
  moments     the same with the mean and mean squared angle
  grid_error  16 images x 4 estimates at level 3 (36,864 rows): 2 thresholds, the moments, 2 error radii to 0.05 degrees
  ball        grid_ball_estimate of 16 images, 4096 candidates, level 3 (2.4e9 pairs)

    python tools/bench_so3_angles.py [--steps 5] [--only mass,moments,grid_error,ball] [--clock-seconds 3]

The eager arm of grid_error takes the radii the way one would in torch: sort each estimate's angles, accumulate the weights, search
the level.  Each line carries pairs/s of both arms and the issue bound of the kernel: vector-issue slots per pair over 256 CUs x 4 SIMDs
x 32 lanes per cycle at the shader clock observed while the HIP arm alone runs back to back (tools/bench_so3_kde.py
observed_clock_ghz).  Kernel-only times come from a separate trace of the HIP arm alone:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_so3_angles.py --trace-only --steps 3"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_so3_kde import LANES, TORCH_TILE, clustered, median_ms, observed_clock_ghz  # noqa: E402
from rotationnormflow_amd import harness  # noqa: E402
from rotationnormflow_amd.utils import angles, sd  # noqa: E402


def issue_slots(T, moments, groups=1):
    """Vector-issue slots per pair of so3_angle_cdf_kernel<TT, MOM, GB, PERQ> from its gfx950 disassembly: 9 v_sub + 9 v_fma + 1 v_min
    for d2; per threshold 1 v_cmp + 1 v_cndmask, and 1 v_fmac per group; with the moments 40 more for theta (the correctly rounded
    sqrt around 2 v_sqrt_f32, the two branches of asinf as selects, theta^2) and its two sums, the v_sqrt_f32 counted as 4 each like
    tools/bench_so3_kde.py's v_exp_f32, and 2 v_fmac per further group."""
    return 19 + T * (2 + groups) + ((40 + 6 + 2 * (groups - 1)) if moments else 0)


def torch_cdf(Cn, Qr, taus, lw=None, moments=True):
    """mass [T,m] (and mean_angle, mean_sq_angle [m]) by the chunked eager expression; ``taus`` float32 [T]"""
    n, m = Cn.shape[0], Qr.shape[0]
    c9, q9 = Cn.reshape(n, 9), Qr.reshape(m, 9)
    w = torch.softmax((torch.zeros(n, device=Cn.device) if lw is None else lw).double(), dim=0).float()
    mass = torch.empty(len(taus), m, device=Cn.device)
    mean, sq = torch.empty(m, device=Cn.device), torch.empty(m, device=Cn.device)
    step = max(1, TORCH_TILE // n)
    for i0 in range(0, m, step):
        q = q9[i0:i0 + step]
        d2 = torch.zeros(q.shape[0], n, device=Cn.device)
        for k in range(9):
            d2 += (q[:, k, None] - c9[None, :, k]) ** 2
        for t, tau in enumerate(taus):
            mass[t, i0:i0 + step] = ((d2 <= tau) * w[None, :]).sum(dim=1)
        if moments:
            th = 2.0 * torch.asin(torch.sqrt(d2 * 0.125).clamp_(max=1.0))
            mean[i0:i0 + step] = th @ w
            sq[i0:i0 + step] = (th * th) @ w
    return mass, mean, sq


def torch_grid_error(logp, grid, est, taus, levels):
    """acc [g,k,T], expected and rms [g,k], radius [g,k,L] (radians) per image by the eager expression and a sort"""
    acc, exp, rms, rad = [], [], [], []
    for b in range(logp.shape[0]):
        n = grid.shape[0]
        d2 = ((est[b].reshape(-1, 1, 9) - grid.reshape(1, n, 9)) ** 2).sum(dim=2)
        w = torch.softmax(logp[b].double(), dim=0).float()
        th = 2.0 * torch.asin(torch.sqrt(d2 * 0.125).clamp_(max=1.0))
        acc.append(torch.stack([((d2 <= tau) * w[None]).sum(dim=1) for tau in taus], dim=1))
        exp.append(th @ w)
        rms.append(torch.sqrt((th * th) @ w))
        srt, order = torch.sort(th, dim=1)
        cum = torch.cumsum(w[order], dim=1)
        at = torch.searchsorted(cum, torch.tensor(levels, device=cum.device).expand(cum.shape[0], -1).contiguous()).clamp_(max=n - 1)
        rad.append(srt.gather(1, at))
    return torch.stack(acc), torch.stack(exp), torch.stack(rms), torch.stack(rad)


def torch_ball(logp, grid, tau, candidates):
    """the row among each image's ``candidates`` densest whose ball carries the most mass -> (index [g], mass [g])"""
    index, best = [], []
    for b in range(logp.shape[0]):
        rows = torch.topk(logp[b], candidates).indices
        mass = torch_cdf(grid, grid[rows], [tau], logp[b], moments=False)[0][0]
        at = torch.argmax(mass)
        index.append(rows[at])
        best.append(mass[at])
    return torch.stack(index), torch.stack(best)


def cases():
    C14, Q20 = clustered(1 << 14, 2), clustered(1 << 20, 3)
    th8 = [math.radians(d) for d in (5.0, 15.0, 30.0, 60.0, 90.0, 120.0, 150.0, 180.0)]
    tau8 = [3.0e38 if t >= math.pi else 8.0 * math.sin(0.5 * t) ** 2 for t in th8]
    grid = sd.generate_healpix_grid(3, device="cuda")
    Q = grid.shape[0]
    torch.manual_seed(3)
    logp = 3.0 * torch.randn(16, Q, device="cuda")
    index = harness.grid_modes(logp, grid, 4, 0.2618)[0]
    est = grid[index.clamp(min=0)].contiguous()
    th2 = [math.radians(15.2), math.radians(30.2)]                       # off the grid's own 15 degrees between tilts
    tau2 = [8.0 * math.sin(0.5 * t) ** 2 for t in th2]
    passes = math.ceil(math.log(math.pi / math.radians(0.05)) / math.log(9.0))
    return {
        "mass": dict(pairs=float(1 << 34), slots=issue_slots(8, False), hip=lambda: angles.so3_angle_cdf(C14, Q20, th8, moments=False)["mass"],
                     eager=lambda: torch_cdf(C14, Q20, tau8, moments=False)[0]),
        "moments": dict(pairs=float(1 << 34), slots=issue_slots(8, True), hip=lambda: angles.so3_angle_cdf(C14, Q20, th8)["mean_angle"],
                        eager=lambda: torch_cdf(C14, Q20, tau8)[1]),
        # pairs of the HIP arm: one pass with 2 thresholds and the moments, then the 4 estimates once per level at tau = 0 and in
        # `passes` passes of 8 thresholds
        "grid_error": dict(pairs=float(16 * 4 * Q) * (1 + 2 * (1 + passes)), slots=issue_slots(8, False),
                           hip=lambda: harness.grid_error(logp, grid, est, (15.2, 30.2), (0.5, 0.9))["radius_deg"],
                           eager=lambda: torch.rad2deg(torch_grid_error(logp, grid, est, tau2, [0.5, 0.9])[3])),
        "ball": dict(pairs=float(16 * 4097 * Q), slots=issue_slots(1, False),
                     hip=lambda: harness.grid_ball_estimate(logp, grid, 15.2, 4096)["mass"],
                     eager=lambda: torch_ball(logp, grid, tau2[0], 4096)[1]),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="mass,moments,grid_error,ball")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="stands in where the clock cannot be observed")
    ap.add_argument("--clock-seconds", type=float, default=3.0, help="how long the HIP arm runs for the clock samples (0: skip)")
    ap.add_argument("--trace-only", action="store_true", help="run only the HIP arm, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_so3_angles: no GPU; there is nothing to measure on a CPU")
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
        bound = LANES * (clock or a.clock_ghz) * 1e9 / case["slots"]
        print(json.dumps(dict(metric="distribution function of the geodesic angle on SO(3)", case=name, steps=a.steps, pairs=case["pairs"],
                              hip_ms=ms["hip"], eager_ms=ms["eager"], eager_over_hip=ms["eager"] / ms["hip"],
                              hip_pairs_per_s=case["pairs"] / ms["hip"] * 1e3, issue_slots_per_pair=case["slots"], clock_ghz=clock or a.clock_ghz,
                              clock_observed=clock is not None, issue_bound_pairs_per_s=bound,
                              hip_share_of_issue_bound=case["pairs"] / ms["hip"] * 1e3 / bound,
                              max_abs_difference=float(diff[torch.isfinite(diff)].max()))), flush=True)


if __name__ == "__main__":
    main()
