#!/usr/bin/env python3
"""The neighbour-limited diffusion on the SO(3) grid (rnf_so3_grid_local_sum: utils/kde.py so3_grid_local_log_sum,
grid_pose.grid_diffuse_local) -- against the dense grid_diffuse (rnf_so3_kernel_sum, Q^2 pairs per image) where the dense form can run,
and alone where it cannot.  One process, the arms alternating step by step, median.  One JSON line per case:

  level3_r15, level3_r30   16 images at level 3 (36 864 rows), kappa whose default radius ((kappa/2) d^2 = 18 nats) is 15 and 30 degrees:
                           grid_diffuse_local against grid_diffuse
  level4, level5           grid_diffuse_local alone, 4 images, default radius 15 degrees (294 912 and 2 359 296 rows): its time, the time
                           of its unweighted pass (log Z) alone, terms per second, the share of enumerated rows that pass the membership
                           test (from the host build's census of 256 queries) and the unweighted pass's share of its issue bound
  level4_fisher            the anisotropic pass (rnf_so3_grid_local_fisher, concentration=V diag(s) V^T with s2 + s3 = 2 kappa) against the
                           isotropic pass of the same build at the same cut, level 4, 15 degrees: unweighted, 4 images as groups, and the
                           max-plus pass; the arms alternate, median

    python tools/bench_so3_grid_local.py [--steps 5] [--only level3_r15,level3_r30,level4,level5,level4_fisher] [--clock-seconds 3]

A term is one (query, member, image) of a sum.  The issue bound of the unweighted pass: vector-issue slots over 256 CUs x 4 SIMDs x 32 lanes
per cycle at the shader clock observed while the pass runs back to back (tools/bench_so3_kde.py observed_clock_ghz); from the gfx950
disassembly of so3_grid_local_kernel<1, false> a row the enumeration looks at costs 29 slots in the first sweep and 24 in the second (9 v_sub
+ 9 v_fma + v_min + the compare, the address and the loop), a member 18 more in the second (the polynomial exp2 and its add)."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_so3_kde import LANES, median_ms, observed_clock_ghz  # noqa: E402
from rotationnormflow_amd import harness  # noqa: E402
from rotationnormflow_amd.utils import kde, sd  # noqa: E402

VISITED_SLOTS, MEMBER_SLOTS = 29.0 + 24.0, 18.0


def kappa_for_radius(deg):
    return 2.0 * kde.LOCAL_NATS / kde.local_radius_to_d2_cut(deg)


def posterior(grid, images, seed):
    """A few sharp modes per image on a floor, as a flow's grid posterior is: log-densities [images, Q]"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    Q = grid.shape[0]
    modes = grid[torch.randint(0, Q, (images, 3), device="cuda", generator=gen)]                   # [images,3,3,3]
    tr = torch.einsum("qij,bkij->bkq", grid, modes)
    return torch.logsumexp(40.0 * (tr - 3.0), dim=1) + torch.log1p(1e-3 * torch.rand(images, Q, device="cuda", generator=gen))


def visited_share(grid, level, kappa, samples=256):
    """members / rows looked at over ``samples`` grid rows, from the host build of the kernel's row functions (None if it cannot be built)"""
    try:
        from tests.test_so3_grid_local_host import host_local_sum
        g = grid.cpu().numpy()
        pick = np.arange(0, len(g), max(1, len(g) // samples))[:samples]
        _, count, seen = host_local_sum(level, g, g[pick], kappa, kde.local_default_d2_cut(kappa), visited=True)
        return float(count.sum()) / float(seen.sum())
    except (OSError, ImportError, RuntimeError) as e:
        print("bench_so3_grid_local: no host census (%s)" % e, file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only", default="level3_r15,level3_r30,level4,level5,level4_fisher")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="stands in where the clock cannot be observed")
    ap.add_argument("--clock-seconds", type=float, default=3.0, help="how long the unweighted pass runs for the clock samples (0: skip)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_so3_grid_local: no GPU; there is nothing to measure on a CPU")
    for name in a.only.split(","):
        if name.startswith("level3"):
            radius = 15.0 if name.endswith("r15") else 30.0
            kappa, level, images = kappa_for_radius(radius), 3, 16
            grid = sd.generate_healpix_grid(level, device="cuda")
            logp = posterior(grid, images, 3)
            ms, out = median_ms({"local": lambda: harness.grid_diffuse_local(logp, grid, level, kappa),
                                 "dense": lambda: harness.grid_diffuse(logp, grid, kappa)}, a.steps)
            count = kde.so3_grid_local_log_sum(grid, level, kappa, return_count=True)[1]
            diff = (out["local"].double() - out["dense"].double()).abs()          # largest in the tails, where the truncated tail of the kernel is all there is
            tv = 0.5 * (torch.softmax(out["local"].double(), 1) - torch.softmax(out["dense"].double(), 1)).abs().sum(dim=1).max()
            print(json.dumps(dict(metric="diffusion of grid posteriors on SO(3)", case=name, level=level, rows=grid.shape[0], images=images,
                                  kappa=kappa, radius_deg=radius, steps=a.steps, local_ms=ms["local"], dense_ms=ms["dense"],
                                  dense_over_local=ms["dense"] / ms["local"], mean_neighbours=float(count.double().mean()),
                                  max_abs_log_difference=float(diff[torch.isfinite(diff)].max()), max_total_variation=float(tv))), flush=True)
            continue
        if name == "level4_fisher":
            level, images, radius = 4, 4, 15.0
            kappa, cut = kappa_for_radius(radius), kde.local_radius_to_d2_cut(radius)
            axes = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1)))[0].numpy()
            K = (axes * np.array([4.0 * kappa, 1.5 * kappa, 0.5 * kappa])) @ axes.T                  # the same loosest-axis bound: s2 + s3 = 2 kappa
            K = 0.5 * (K + K.T)
            grid = sd.generate_healpix_grid(level, device="cuda")
            lw = torch.log_softmax(posterior(grid, images, level), dim=1)
            arms = {"iso_unweighted": lambda: kde.so3_grid_local_log_sum(grid, level, kappa, d2_cut=cut),
                    "fisher_unweighted": lambda: kde.so3_grid_local_log_sum(grid, level, concentration=K, d2_cut=cut),
                    "iso_weighted": lambda: kde.so3_grid_local_log_sum(grid, level, kappa, d2_cut=cut, log_weights=lw),
                    "fisher_weighted": lambda: kde.so3_grid_local_log_sum(grid, level, concentration=K, d2_cut=cut, log_weights=lw),
                    "iso_max": lambda: kde.so3_grid_local_log_max(grid, level, kappa, d2_cut=cut, log_weights=lw),
                    "fisher_max": lambda: kde.so3_grid_local_log_max(grid, level, concentration=K, d2_cut=cut, log_weights=lw)}
            ms, _ = median_ms(arms, a.steps)
            count = kde.so3_grid_local_log_sum(grid, level, kappa, d2_cut=cut, return_count=True)[1]
            line = dict(metric="anisotropic against isotropic neighbour-limited pass on SO(3)", case=name, level=level, rows=grid.shape[0],
                        images=images, kappa=kappa, radius_deg=radius, steps=a.steps, mean_neighbours=float(count.double().mean()))
            line.update({k + "_ms": v for k, v in ms.items()})
            line.update({"fisher_over_iso_" + k: ms["fisher_" + k] / ms["iso_" + k] for k in ("unweighted", "weighted", "max")})
            print(json.dumps(line), flush=True)
            continue
        level, images, radius = int(name[-1]), 4, 15.0
        kappa = kappa_for_radius(radius)
        grid = sd.generate_healpix_grid(level, device="cuda")
        logp = posterior(grid, images, level)
        unweighted = lambda: kde.so3_grid_local_log_sum(grid, level, kappa)                                       # noqa: E731
        ms, _ = median_ms({"diffuse": lambda: harness.grid_diffuse_local(logp, grid, level, kappa), "unweighted": unweighted}, a.steps)
        count = kde.so3_grid_local_log_sum(grid, level, kappa, return_count=True)[1]
        terms = float(count.double().sum())
        share = visited_share(grid, level, kappa)
        clock = observed_clock_ghz(unweighted, a.clock_seconds) if a.clock_seconds > 0 else None
        line = dict(metric="neighbour-limited diffusion of grid posteriors on SO(3)", case=name, level=level, rows=grid.shape[0], images=images,
                    kappa=kappa, radius_deg=radius, steps=a.steps, diffuse_ms=ms["diffuse"], unweighted_ms=ms["unweighted"],
                    mean_neighbours=terms / grid.shape[0], diffuse_terms=terms * (1 + images),
                    diffuse_terms_per_s=terms * (1 + images) / ms["diffuse"] * 1e3, unweighted_terms_per_s=terms / ms["unweighted"] * 1e3,
                    members_over_rows_looked_at=share, clock_ghz=clock or a.clock_ghz, clock_observed=clock is not None)
        if share:
            slots = VISITED_SLOTS * terms / share + MEMBER_SLOTS * terms
            bound_ms = slots / (LANES * (clock or a.clock_ghz) * 1e9) * 1e3
            line.update(unweighted_issue_slots=slots, unweighted_issue_bound_ms=bound_ms, unweighted_share_of_issue_bound=bound_ms / ms["unweighted"])
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
