#!/usr/bin/env python3
"""The pairwise matrix-Fisher kernel sum (rnf_so3_kernel_sum: utils/kde.py, grid_pose.grid_diffuse) against the chunked torch-eager
expression -- the only thing a user could run before it, kept in this tool and on no product path -- in one process, the calls
alternating step by step, median.  One JSON line per case:

  fit        leave-one-out scores of 8 bandwidths at n = 2^16 (4.3e9 pairs)
  log_prob   2^20 queries against 2^14 centres, one bandwidth (1.7e10 pairs)
  diffuse_l2 grid_diffuse of 16 images at level 2 (4,608 rows: 2.1e7 pairs for log Z, then 16 groups on the same pairs)
  diffuse_l3 the same at level 3 (36,864 rows: 1.4e9 pairs)

    python tools/bench_so3_kde.py [--steps 5] [--only fit,log_prob,diffuse_l2,diffuse_l3] [--clock-seconds 3]

Each line carries pairs/s of both arms (a pair is one (centre, query) distance, however many bandwidths and groups share it) and the
issue bound of the kernel: issue_slots() vector-issue slots per pair over 256 CUs x 4 SIMDs x 32 lanes per cycle at the shader clock
observed while the HIP arm alone runs back to back for --clock-seconds (the median of read-only `rocm-smi --showclocks` samples, the
first second dropped; "clock_observed" is false and --clock-ghz stands in where no sample could be read).  The kernel-only times come
from a separate trace of the HIP arm alone (no timing of its own):

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_so3_kde.py --trace-only --steps 3"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rotationnormflow_amd import harness, synth  # noqa: E402
from rotationnormflow_amd.utils import kde, sd  # noqa: E402

LANES = 256 * 4 * 32                                 # a SIMD issues a wave64 VALU instruction over 2 cycles: 32 lanes per cycle


def issue_slots(J, groups=1, weighted=False):
    """Vector-issue slots per pair of the hot kernel, both sweeps together, from the gfx950 disassembly of
    so3_kernel_sum_kernel<J, GB, LOO>: per pair and sweep 9 v_sub + 9 v_fma + 1 v_min for d2 (+ 1 v_mul per group with log-weights); per
    slot (bandwidth x group) the first sweep issues 1 v_fma + 1/2 v_max3, the second 1 v_fma + 1 v_sub + 1 v_exp_f32 + 1 v_add, the
    v_exp_f32 counted as 4: profiles/r1/mfma_valu_coissue_microbench.txt has it at 8.0 cycles per instruction against 2.0 for v_fma_f32
    (slopes of the one-wave rows).  Leave-one-out adds nothing outside the tiles of a block's own queries."""
    return 2 * (19 + (groups if weighted else 0)) + J * groups * (1.5 + 7.0)


def observed_clock_ghz(fn, seconds):
    """The median shader clock (GHz) while ``fn`` runs back to back for ``seconds``, or None; a query only, nothing is set."""
    import re
    import subprocess
    import threading
    samples, stop = [], threading.Event()

    def poll():
        t0 = time.perf_counter()
        while not stop.is_set():
            try:
                out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=10).stdout
            except (OSError, subprocess.SubprocessError):
                return
            m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
            if m and time.perf_counter() - t0 > 1.0:
                samples.append(float(m.group(1)))
            time.sleep(0.2)

    th = threading.Thread(target=poll)
    th.start()
    t0 = time.perf_counter()
    with torch.no_grad():
        while time.perf_counter() - t0 < seconds:
            fn()
            torch.cuda.synchronize()
    stop.set()
    th.join()
    return sorted(samples)[len(samples) // 2] * 1e-3 if samples else None


FIT_KAPPAS = [2.0 ** k for k in range(3, 11)]
TORCH_TILE = 1 << 24                                # elements of the [queries, centres] tiles of the eager arm


def torch_kernel_sum(Cn, Qr, kappas, lw=None, leave_one_out=False):
    """The chunked eager expression, in difference form: [G,J,m] from [m_tile, n] tiles."""
    n = Cn.shape[0]
    Q = Cn if Qr is None else Qr
    m = Q.shape[0]
    c9, q9 = Cn.reshape(n, 9), Q.reshape(m, 9)
    lw = torch.zeros(1, n, device=Cn.device) if lw is None else lw.reshape(-1, n)
    log_w = torch.log_softmax(lw.double(), dim=1).float()
    l = [float(torch.log(torch.special.i0e(torch.tensor(2.0 * k, dtype=torch.float64)) - torch.special.i1e(torch.tensor(2.0 * k, dtype=torch.float64))))
         if k > 0 else 0.0 for k in kappas]
    out = torch.empty(lw.shape[0], len(kappas), m, device=Cn.device)
    step = max(1, TORCH_TILE // n)
    for i0 in range(0, m, step):
        q = q9[i0:i0 + step]
        d2 = torch.zeros(q.shape[0], n, device=Cn.device)
        for k in range(9):
            d2 += (q[:, k, None] - c9[None, :, k]) ** 2
        if leave_one_out:
            idx = torch.arange(i0, i0 + q.shape[0], device=Cn.device)
            d2[torch.arange(q.shape[0], device=Cn.device), idx] = float("inf")
        for g in range(lw.shape[0]):
            for a, kappa in enumerate(kappas):
                r = torch.logsumexp(log_w[g][None, :] - (0.5 * kappa) * d2, dim=1) - l[a]
                if leave_one_out:
                    r = r - torch.log1p(-torch.exp(log_w[g][i0:i0 + q.shape[0]]))
                out[g, a, i0:i0 + q.shape[0]] = r
    return out


def torch_grid_diffuse(logp, grid, kappa):
    lz = torch_kernel_sum(grid, grid, [kappa])[0, 0]
    lw = torch.log_softmax(logp, dim=1) - lz
    return torch_kernel_sum(grid, grid, [kappa], lw)[:, 0] + torch.logsumexp(lw, dim=1, keepdim=True)


def median_ms(calls, steps):
    times = {k: [] for k in calls}
    out = {}
    with torch.no_grad():
        for key, fn in calls.items():                       # warm-up: workspaces, code objects
            out[key] = fn()
        for _ in range(steps):
            for key, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out[key] = fn()
                torch.cuda.synchronize()
                times[key].append(time.perf_counter() - t0)
    return {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}, out


def clustered(n, seed):
    """Rotations around three modes (a flow's samples are not uniform): uniform modes times small uniform-axis rotations"""
    R = torch.from_numpy(synth.uniform_rotations(n, seed=seed)).cuda().reshape(n, 3, 3)
    modes = torch.from_numpy(synth.uniform_rotations(3, seed=seed + 1)).cuda().reshape(3, 3, 3)
    small = torch.linalg.matrix_exp(0.15 * (R - R.transpose(1, 2)))
    return (modes[torch.arange(n, device="cuda") % 3] @ small).contiguous()


def cases():
    fit_R = clustered(1 << 16, 1)
    lp_C, lp_Q = clustered(1 << 14, 2), clustered(1 << 20, 3)
    out = {"fit": dict(pairs=float(1 << 32), slots=issue_slots(8),
                       hip=lambda: kde.so3_kernel_log_density(fit_R, None, FIT_KAPPAS, leave_one_out=True),
                       eager=lambda: torch_kernel_sum(fit_R, None, FIT_KAPPAS, leave_one_out=True)[0]),
           "log_prob": dict(pairs=float(1 << 34), slots=issue_slots(1),
                            hip=lambda: kde.so3_kernel_log_density(lp_C, lp_Q, 64.0),
                            eager=lambda: torch_kernel_sum(lp_C, lp_Q, [64.0])[0, 0])}
    for level in (2, 3):
        grid = sd.generate_healpix_grid(level, device="cuda")
        Q = grid.shape[0]
        torch.manual_seed(level)
        logp = 3.0 * torch.randn(16, Q, device="cuda")
        # pairs: the log Z call and the 16-group call walk the same Q^2 pairs once each (4 groups share a pair's d2: 4 passes)
        out[f"diffuse_l{level}"] = dict(pairs=float(Q) * Q * 2, slots=(issue_slots(1) + 4 * issue_slots(1, 4, True)) / 2,
                                        hip=lambda logp=logp, grid=grid: harness.grid_diffuse(logp, grid, 64.0),
                                        eager=lambda logp=logp, grid=grid: torch_grid_diffuse(logp, grid, 64.0))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="fit,log_prob,diffuse_l2,diffuse_l3")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="stands in where the clock cannot be observed")
    ap.add_argument("--clock-seconds", type=float, default=3.0, help="how long the HIP arm runs for the clock samples (0: skip)")
    ap.add_argument("--trace-only", action="store_true", help="run only the HIP arm, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_so3_kde: no GPU; there is nothing to measure on a CPU")
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
        print(json.dumps(dict(metric="pairwise matrix-Fisher kernel sum on SO(3)", case=name, steps=a.steps, pairs=case["pairs"],
                              hip_ms=ms["hip"], eager_ms=ms["eager"], eager_over_hip=ms["eager"] / ms["hip"],
                              hip_pairs_per_s=case["pairs"] / ms["hip"] * 1e3, eager_pairs_per_s=case["pairs"] / ms["eager"] * 1e3,
                              issue_slots_per_pair=case["slots"], clock_ghz=clock or a.clock_ghz, clock_observed=clock is not None, issue_bound_pairs_per_s=bound,
                              hip_share_of_issue_bound=case["pairs"] / ms["hip"] * 1e3 / bound,
                              max_abs_difference=float(diff[torch.isfinite(diff)].max()))), flush=True)


if __name__ == "__main__":
    main()
