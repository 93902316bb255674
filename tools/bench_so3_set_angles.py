#!/usr/bin/env python3
"""The distribution function of the angle to the nearest member of a set (rnf_so3_set_angle_cdf: utils/angles.py so3_set_angle_cdf,
grid_pose.grid_error_symmetric) against the chunked torch-eager expression -- difference-form d2, ``amin`` over the members, ``<=``, a
weighted sum: the only thing a user could run before it, kept in this tool and on no product path -- in one process, the calls
alternating step by step, median.  One JSON line per case:

  mass        2^16 sets of K = 12 against 2^14 centres, 8 thresholds, masses only (1.3e10 pair-members)
  moments     the same with the mean and mean squared angle
  symmetric   grid_error_symmetric of 16 images x 4 estimates at level 3 (36,864 rows) under point_group("I"), K = 60: 2 thresholds,
              the moments, 2 error radii to 0.05 degrees
  cylinder    the same for 16 images x 1 estimate under point_group("D360"), K = 720

    python tools/bench_so3_set_angles.py [--steps 5] [--only mass,moments,symmetric,cylinder] [--clock-seconds 3]

The two grid cases are few sets and run the wave-per-set kernel (csrc/so3_set_angle_cdf.h wave_per_set); their issue bound is still
the thread-per-set kernel's census, the least work the pass needs.  Each line carries pair-members/s of both arms and the issue bound of the kernel: vector-issue slots per pair over 256 CUs x 4 SIMDs x
32 lanes per cycle at the shader clock observed while the HIP arm alone runs back to back (tools/bench_so3_kde.py observed_clock_ghz).
Kernel-only times come from a separate trace of the HIP arm alone:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_so3_set_angles.py --trace-only --steps 3"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import bench_so3_angles  # noqa: E402
from bench_so3_kde import LANES, TORCH_TILE, clustered, median_ms, observed_clock_ghz  # noqa: E402
from rotationnormflow_amd import harness  # noqa: E402
from rotationnormflow_amd.utils import angles, sd, symmetry  # noqa: E402

MEMBER_SLOTS = 1226.0 / 64.0                         # per pair-member, from the member loop's 64 centres in the gfx950 disassembly


def issue_slots(K, T, moments, groups=1):
    """Vector-issue slots per (centre, set) pair of so3_set_angle_cdf_kernel<TT, MOM, GB, PERQ> from its gfx950 disassembly: per member 9
    v_sub + 8 v_fmac + 1 v_fma for the squared distance, 1 v_min3 for the cap and the running minimum, and the member's 9 v_mov
    shared by the tile's 64 centres; once per pair what tools/bench_so3_angles.py counts past its own d2 (19)"""
    return MEMBER_SLOTS * K + bench_so3_angles.issue_slots(T, moments, groups) - 19


def torch_set_cdf(Cn, sets, taus, lw=None, moments=True):
    """mass [T,m] (and mean_angle, mean_sq_angle [m]) by the chunked eager expression; ``sets`` [m,K,3,3], ``taus`` float32 [T]"""
    n, m, K = Cn.shape[0], sets.shape[0], sets.shape[1]
    c9, q9 = Cn.reshape(n, 9), sets.reshape(m, K, 9)
    w = torch.softmax((torch.zeros(n, device=Cn.device) if lw is None else lw).double(), dim=0).float()
    mass = torch.empty(len(taus), m, device=Cn.device)
    mean, sq = torch.empty(m, device=Cn.device), torch.empty(m, device=Cn.device)
    step = max(1, TORCH_TILE // (n * K))
    for i0 in range(0, m, step):
        q = q9[i0:i0 + step]
        d2 = torch.zeros(q.shape[0], K, n, device=Cn.device)
        for k in range(9):
            d2 += (q[:, :, k, None] - c9[None, None, :, k]) ** 2
        d2 = d2.amin(dim=1)
        for t, tau in enumerate(taus):
            mass[t, i0:i0 + step] = ((d2 <= tau) * w[None, :]).sum(dim=1)
        if moments:
            th = 2.0 * torch.asin(torch.sqrt(d2 * 0.125).clamp_(max=1.0))
            mean[i0:i0 + step] = th @ w
            sq[i0:i0 + step] = (th * th) @ w
    return mass, mean, sq


def torch_grid_error_symmetric(logp, grid, est, S, taus, levels):
    """acc [g,k,T], expected and rms [g,k], radius [g,k,L] (radians) per image by the eager expression, ``amin`` and a sort"""
    acc, exp, rms, rad = [], [], [], []
    n = grid.shape[0]
    for b in range(logp.shape[0]):
        members = (est[b][:, None] @ S[None]).reshape(-1, S.shape[0], 1, 9)
        d2 = ((members - grid.reshape(1, 1, n, 9)) ** 2).sum(dim=3).amin(dim=1)
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


def cases():
    C14, E16 = clustered(1 << 14, 2), clustered(1 << 16, 3)
    sets = symmetry.orbit(E16, symmetry.point_group("T", device="cuda")).contiguous()     # [2^16,12,3,3]
    th8 = [math.radians(d) for d in (5.0, 15.0, 30.0, 60.0, 90.0, 120.0, 150.0, 180.0)]
    tau8 = [3.0e38 if t >= math.pi else 8.0 * math.sin(0.5 * t) ** 2 for t in th8]
    grid = sd.generate_healpix_grid(3, device="cuda")
    Q = grid.shape[0]
    torch.manual_seed(3)
    logp = 3.0 * torch.randn(16, Q, device="cuda")
    index = harness.grid_modes(logp, grid, 4, 0.2618)[0]
    est = grid[index.clamp(min=0)].contiguous()
    ico, cyl = symmetry.point_group("I", device="cuda"), symmetry.point_group("D360", device="cuda")
    th2 = [math.radians(15.2), math.radians(30.2)]                       # off the grid's own 15 degrees between tilts
    tau2 = [8.0 * math.sin(0.5 * t) ** 2 for t in th2]
    passes = math.ceil(math.log(math.pi / math.radians(0.05)) / math.log(9.0))
    calls = 1 + 2 * (1 + passes)            # one pass with 2 thresholds and the moments, then per level tau = 0 and `passes` passes of 8
    pm = float(1 << 30) * 12
    return {
        "mass": dict(pair_members=pm, K=12, slots=issue_slots(12, 8, False),
                     hip=lambda: angles.so3_set_angle_cdf(C14, sets, th8, moments=False)["mass"],
                     eager=lambda: torch_set_cdf(C14, sets, tau8, moments=False)[0]),
        "moments": dict(pair_members=pm, K=12, slots=issue_slots(12, 8, True), hip=lambda: angles.so3_set_angle_cdf(C14, sets, th8)["mean_angle"],
                        eager=lambda: torch_set_cdf(C14, sets, tau8)[1]),
        "symmetric": dict(pair_members=float(16 * 4 * Q * 60) * calls, K=60, slots=issue_slots(60, 8, False),
                          hip=lambda: harness.grid_error_symmetric(logp, grid, est, ico, (15.2, 30.2), (0.5, 0.9))["radius_deg"],
                          eager=lambda: torch.rad2deg(torch_grid_error_symmetric(logp, grid, est, ico, tau2, [0.5, 0.9])[3])),
        "cylinder": dict(pair_members=float(16 * Q * 720) * calls, K=720, slots=issue_slots(720, 8, False),
                         hip=lambda: harness.grid_error_symmetric(logp, grid, est[:, :1], cyl, (15.2, 30.2), (0.5, 0.9))["radius_deg"],
                         eager=lambda: torch.rad2deg(torch_grid_error_symmetric(logp, grid, est[:, :1], cyl, tau2, [0.5, 0.9])[3])),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="mass,moments,symmetric,cylinder")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="stands in where the clock cannot be observed")
    ap.add_argument("--clock-seconds", type=float, default=3.0, help="how long the HIP arm runs for the clock samples (0: skip)")
    ap.add_argument("--trace-only", action="store_true", help="run only the HIP arm, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_so3_set_angles: no GPU; there is nothing to measure on a CPU")
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
        pairs = case["pair_members"] / case["K"]
        bound = LANES * (clock or a.clock_ghz) * 1e9 / case["slots"]     # pairs per second
        print(json.dumps(dict(metric="distribution function of the angle to the nearest member of a set on SO(3)", case=name, steps=a.steps,
                              K=case["K"], pair_members=case["pair_members"], hip_ms=ms["hip"], eager_ms=ms["eager"],
                              eager_over_hip=ms["eager"] / ms["hip"], hip_pair_members_per_s=case["pair_members"] / ms["hip"] * 1e3,
                              issue_slots_per_pair=case["slots"], clock_ghz=clock or a.clock_ghz, clock_observed=clock is not None,
                              issue_bound_pair_members_per_s=bound * case["K"], hip_share_of_issue_bound=pairs / ms["hip"] * 1e3 / bound,
                              max_abs_difference=float(diff[torch.isfinite(diff)].max()))), flush=True)


if __name__ == "__main__":
    main()
