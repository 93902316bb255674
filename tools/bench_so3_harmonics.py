#!/usr/bin/env python3
"""Harmonic analysis on SO(3) (rnf_so3_fourier, rnf_so3_fourier_eval: utils/harmonics.py, grid_pose.grid_spectrum /
grid_diffuse_spectral) timed as whole calls for 16 images, median of --steps, one JSON line per case:

  spectrum_l{3,5}_L{8,16}   grid_spectrum (the analysis and the power per degree)
  spectral_l{3,5}_L{8,16}   grid_diffuse_spectral (analysis and synthesis on the grid rows) with the heat kernel whose truncation
                            (2L+1) h_L is 1e-3: a kernel as sharp as the degree resolves
  dense_l3                  grid_diffuse_spectral against grid_diffuse (Q^2 pairs) at level 3 for the same kappa = 8, L = 16, with the
                            maximum absolute difference of the two densities
  local_l{4,5}              grid_diffuse_spectral against grid_diffuse_local (one call) at levels 4 and 5 for kappa = 8, whose local
                            radius (where (kappa/2) d^2 = 18 nats) is 97 degrees, L = 16, with the same difference.  The level-5 local
                            arm walks about 6e12 pair terms and takes minutes: it runs only when named (--only local5)

    python tools/bench_so3_harmonics.py [--steps 3] [--only spectrum,spectral,dense,local4,local5] [--images 16]

The two diffusions differ by construction: grid_diffuse renormalises its operator on the grid, the spectral form carries the grid's
quadrature error and its truncation."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rotationnormflow_amd import harness, synth  # noqa: E402
from rotationnormflow_amd.utils import sd  # noqa: E402

WIDE_KAPPA, WIDE_L = 8.0, 16                          # 18 nats at d^2 = 4.5: a local radius of 97 degrees; (2L+1) a_L = 9e-3 at L = 16


def median_ms(fn, steps):
    with torch.no_grad():
        out = fn()                                       # warm-up: workspaces, code objects
        times = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
    return sorted(times)[len(times) // 2] * 1e3, out


def once_ms(fn):
    """One call, no warm-up: for the arms that take seconds to minutes"""
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def posteriors(grid, images, seed):
    """Two-mode matrix-Fisher posteriors on the grid rows: [images, Q] log-densities"""
    M = torch.from_numpy(synth.uniform_rotations(2 * images, seed=seed)).cuda().reshape(images, 2, 3, 3)
    tr = torch.einsum("bkij,qij->bkq", M, grid)
    return torch.logaddexp(12.0 * tr[:, 0], 8.0 * tr[:, 1] + 1.0).contiguous()


def emit(**kw):
    print(json.dumps(dict(metric="harmonic analysis on SO(3)", **kw)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--only", default="spectrum,spectral,dense,local4")
    ap.add_argument("--images", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_so3_harmonics: no GPU; there is nothing to measure on a CPU")
    only = a.only.split(",")
    grids = {}

    def level(k):
        if k not in grids:
            g = sd.generate_healpix_grid(k, device="cuda")
            grids[k] = (g, posteriors(g, a.images, k))
        return grids[k]

    for lv in (3, 5):
        for L in (8, 16):
            grid, logp = level(lv)
            if "spectrum" in only:
                ms, _ = median_ms(lambda: harness.grid_spectrum(logp, grid, L), a.steps)
                emit(case=f"spectrum_l{lv}_L{L}", images=a.images, rows=grid.shape[0], lmax=L, steps=a.steps, ms=ms)
            if "spectral" in only:
                t = math.log((2 * L + 1) / 1e-3) / (L * (L + 1))
                ms, out = median_ms(lambda: harness.grid_diffuse_spectral(logp, grid, t=t, lmax=L), a.steps)
                emit(case=f"spectral_l{lv}_L{L}", images=a.images, rows=grid.shape[0], lmax=L, steps=a.steps, heat_t=t, ms=ms,
                     truncation=out["truncation"], negative_mass=float(out["negative_mass"].min()))
    if "dense" in only:
        grid, logp = level(3)
        ms_s, out = median_ms(lambda: harness.grid_diffuse_spectral(logp, grid, kappa=WIDE_KAPPA, lmax=WIDE_L), a.steps)
        ms_d, dense = median_ms(lambda: harness.grid_diffuse(logp, grid, WIDE_KAPPA), a.steps)
        emit(case="dense_l3", images=a.images, rows=grid.shape[0], lmax=WIDE_L, kappa=WIDE_KAPPA, steps=a.steps, spectral_ms=ms_s, dense_ms=ms_d,
             dense_over_spectral=ms_d / ms_s, truncation=out["truncation"], peak_density=float(dense.max().exp()),
             max_abs_difference=float((dense.exp() - out["density"]).abs().max()))
    for lv in (4, 5):
        if f"local{lv}" in only:
            grid, logp = level(lv)
            ms_s, out = median_ms(lambda: harness.grid_diffuse_spectral(logp, grid, kappa=WIDE_KAPPA, lmax=WIDE_L), a.steps)
            ms_l, local = once_ms(lambda: harness.grid_diffuse_local(logp, grid, lv, WIDE_KAPPA))
            emit(case=f"local_l{lv}", images=a.images, rows=grid.shape[0], lmax=WIDE_L, kappa=WIDE_KAPPA, steps=a.steps, spectral_ms=ms_s, local_ms=ms_l,
                 local_over_spectral=ms_l / ms_s, truncation=out["truncation"], peak_density=float(local.max().exp()),
                 max_abs_difference=float((local.exp() - out["density"]).abs().max()))


if __name__ == "__main__":
    main()
