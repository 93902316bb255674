"""The grid analyses: evaluate a flow's log-density on the HEALPix grid over SO(3) (``utils.sd``) and reduce each image's row on the
device -- the arg-max of ``eval.py``'s ``log_pdf`` mode (``grid_estimate_rotations``), top-k modes with their mass (``grid_pose_modes``),
highest-density credible sets (``grid_pose_credible``), samples against the density (``grid_pose_fit``), draws from it
(``grid_pose_sample``), matrix-Fisher and mixture fits (``grid_pose_fisher``, ``grid_pose_mixture``), the error distribution of point estimates and the Acc@theta-optimal estimate
(``grid_pose_error``, ``grid_pose_ball_estimate``) and the coarse-to-fine beam search (``grid_beam_estimate_rotations``).  They share one path
from (flow, feature, base) to log-density rows (``_GridFlow``); ``grid_modes``, ``grid_credible``, ``grid_fit``, ``grid_sample``, ``grid_children``
and ``grid_beam_select`` are the reductions' entry points of the library on rows already at hand.  ``harness`` re-exports the public functions.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, runtime
from .flow.flow import Flow
from .utils import fisher, sd


# Rotations per launch of the grid search: images are grouped up to about 2^21 rotations (the regime the shared-row kernels are measured
# in); a single image's grid larger than GRID_MAX_LAUNCH_ROWS is evaluated in chunks of that size.  Flows with side layers take one feature
# row per rotation (runtime.expand_shared_rows), so their launches are kept to GRID_SIDE_LAUNCH_ROWS to bound the expanded features.
GRID_LAUNCH_ROWS = 1 << 21
GRID_MAX_LAUNCH_ROWS = 1 << 24
GRID_SIDE_LAUNCH_ROWS = 1 << 18


def _batch_coupled(flow: Flow) -> list:
    """Names of ``flow``'s layer classes whose matrices come from the first rows of a launch."""
    return sorted({type(m).__name__ for m in flow.modules() if getattr(m, "_rnf_batch_coupled", False)})


def _refuse_batch_coupled(flow: Flow, who: str, consequence: str = ""):
    coupled = _batch_coupled(flow)
    if coupled:
        raise ValueError(f"{who}: batch-coupled layers ({', '.join(coupled)}) take their matrices from a launch's first rows{consequence}; "
                         "use grid_estimate_rotations")


class _GridFlow:
    """The one path from (flow, feature rows, base rows) to log-density rows: B images' feature [B,F] (or None) and base (A [1|B,3,3], c)
    (or None, None), the flow's packed image and what bounds a launch.  Call its methods under no_grad."""

    def __init__(self, flow: Flow, feature, B, A, c, dev):
        self.flow, self.feature, self.B, self.A, self.c, self.dev = flow, feature, B, A, c, dev
        self.packed = flow._packed(dev, feature)
        self.coupled = bool(_batch_coupled(flow))

    @property
    def budget(self):
        """Rotations per launch (the module's constants, read at call time)."""
        return GRID_SIDE_LAUNCH_ROWS if self.packed.side_layers else GRID_LAUNCH_ROWS

    def log_prob(self, rot, b0, b1, repeat):
        """log p [(b1 - b0) * repeat] of ``rot`` [(b1 - b0) * repeat,3,3]: ``repeat`` consecutive rotations per image b0..b1-1, which share the
        image's feature row and base row."""
        feat = self.feature[b0:b1] if self.feature is not None else None
        rows = (self.A, self.c) if self.A is None or self.A.shape[0] == 1 else (self.A[b0:b1], self.c[b0:b1])
        return runtime.run_log_prob(self.flow, self.packed, rot, feat, *rows, feature_repeat=repeat)["logp"]

    def launches(self, grid, images_per_launch, who: str):
        """Evaluate the images' log-density on ``grid`` [Q,3,3] in launches of about GRID_LAUNCH_ROWS shared-row rotations.
        Yields (b0, b1, lo, logp [b1 - b0, rows]) per launch: images b0..b1-1 on grid rows lo..lo+rows-1 -- whole images (lo = 0, rows = Q)
        when several share a launch, consecutive chunks of one image otherwise."""
        Q, B = grid.shape[0], self.B
        if images_per_launch is None:
            images_per_launch = 1 if self.coupled else max(1, self.budget // Q)
        g = min(int(images_per_launch), B)
        if g < 1 or (self.coupled and g > 1):
            raise ValueError(f"{who}: images_per_launch={images_per_launch}" + (" (batch-coupled layers: 1)" if self.coupled else ""))
        if g > 1 and g * Q > GRID_MAX_LAUNCH_ROWS:
            raise ValueError(f"{who}: {g} images of {Q} rotations exceed {GRID_MAX_LAUNCH_ROWS} rotations per launch")
        chunk = Q if g > 1 else min(Q, GRID_SIDE_LAUNCH_ROWS if self.packed.side_layers else GRID_MAX_LAUNCH_ROWS)
        rep = grid.repeat(g, 1, 1) if g > 1 else grid          # one image per launch: the grid itself, no copy
        for b0 in range(0, B, g):
            b1 = min(B, b0 + g)
            if g > 1:
                yield b0, b1, 0, self.log_prob(rep[:(b1 - b0) * Q], b0, b1, Q).reshape(b1 - b0, Q)
                continue
            for lo in range(0, Q, chunk):
                part = grid[lo:lo + chunk]
                yield b0, b1, lo, self.log_prob(part, b0, b1, part.shape[0]).reshape(1, -1)

    def images(self, grid, images_per_launch, who: str):
        """``launches`` by whole images: yields (b0, b1, logp [b1 - b0, Q]).  An image evaluated in chunks has them gathered into one [1,Q]
        float32 buffer, which the next such image overwrites (in stream order): reduce it before asking for the next."""
        Q, whole = grid.shape[0], None
        for b0, b1, lo, lp in self.launches(grid, images_per_launch, who):
            if lp.shape[1] < Q:                                 # one image in chunks: gather them first
                if whole is None:
                    whole = torch.empty(1, Q, dtype=torch.float32, device=self.dev)
                whole[:, lo:lo + lp.shape[1]] = lp
                if lo + lp.shape[1] < Q:
                    continue
                lp = whole
            yield b0, b1, lp


def _grid_inputs(flow: Flow, feature, number_queries, recursion_level, offset, base, who: str):
    """The common arguments of the grid searches -> (_GridFlow of the B images, level, offset [3,3])."""
    if not flow.condition:
        feature = None
    if feature is not None:
        dev, B = feature.device, feature.shape[0]
    else:
        dev = base.A.device if base is not None else torch.device("cuda", torch.cuda.current_device())
        B = base.A.reshape(-1, 3, 3).shape[0] if base is not None else 1
    if dev.type != "cuda":
        raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    level = int(recursion_level) if recursion_level is not None else sd.closest_grid_level(500 if number_queries is None else number_queries)
    if offset is None:
        offset = sd.random_rotations(1)[0]
    offset = offset.reshape(3, 3).to(device=dev, dtype=torch.float32)
    A = c = None
    if base is not None:
        A = base.A.detach().reshape(-1, 3, 3).to(device=dev, dtype=torch.float32)
        c = base.log_const().reshape(-1).to(device=dev, dtype=torch.float32)
        if A.shape[0] not in (1, B):
            raise ValueError(f"{who}: the base has {A.shape[0]} rows for {B} images (1 or {B})")
    return _GridFlow(flow, feature, B, A, c, dev), level, offset


def _grid_launches(flow: Flow, feature, grid, B, A, c, images_per_launch, who: str):
    """``_GridFlow.launches`` for B images given as their feature [B,F] (or None) and base rows (A, c) (or None, None)."""
    return _GridFlow(flow, feature, B, A, c, grid.device).launches(grid, images_per_launch, who)


def grid_estimate_rotations(flow: Flow, feature: torch.Tensor = None, number_queries: int = None, recursion_level: int = None, offset=None,
                            base=None, images_per_launch: int = None):
    """Grid-search pose estimate of ``eval.py``'s ``log_pdf`` mode (eval.py:437-462): evaluate each image's log-density on the HEALPix grid
    over SO(3) (``utils.sd``; level ``recursion_level``, or the one closest to ``number_queries``, default 500, in log space) multiplied on
    the right by ``offset`` [3,3] (None: one Haar-uniform rotation drawn from torch's generator, as ``trans.random_rotation()``), and keep
    the grid point of largest log p (``torch.argmax``: the first on a tie).

    feature [B,F] (None for an unconditional flow: B = the base's rows, or 1).  ``base``: None (uniform) or a ``MatrixFisherN`` with one row
    (shared by every image) or B rows (row b scores image b's grid; its log-constants are sliced, never recomputed on a slice).
    ``images_per_launch``: images evaluated per launch (default: as many as fit in about 2^21 rotations; 1 for flows with batch-coupled
    layers, whose matrices come from the first rows of a launch, as in the reference's per-image chunks).
    Returns (est [B,3,3], max_log_prob [B], index [B] into the grid, offset [3,3])."""
    gf, level, offset = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, "grid_estimate_rotations")
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        bests, indices = [], []
        for b0, b1, lo, lp in gf.launches(grid, images_per_launch, "grid_estimate_rotations"):
            if b1 - b0 > 1:
                idx = torch.argmax(lp, dim=-1)
                bests.append(lp.gather(1, idx[:, None])[:, 0])
                indices.append(idx)
                continue
            lp = lp[0]                                          # the first chunk's maximum wins a tie, a NaN wins as in torch.argmax
            idx = torch.argmax(lp)
            val = lp[idx]
            if lo == 0:
                v, i = val, idx
            else:
                take = (val > v) | (val.isnan() & ~v.isnan())
                v, i = torch.where(take, val, v), torch.where(take, idx + lo, i)
            if lo + lp.shape[0] == grid.shape[0]:
                bests.append(v.reshape(1))
                indices.append(i.reshape(1))
        best, index = (bests[0], indices[0]) if len(bests) == 1 else (torch.cat(bests), torch.cat(indices))
        est = grid[index]
    return est, best, index, offset


def grid_modes(logp: torch.Tensor, grid: torch.Tensor, top_k: int, separation_rad: float, gt: torch.Tensor = None):
    """``rnf_grid_modes`` on g images' log-densities ``logp`` [g,Q] (float32, on the device) over ``grid`` [Q,3,3]: the top-k modes
    separated by ``separation_rad`` and the mass each carries (include/rnf_hip.h).  ``gt``: None or [g,K,3,3] ground truths for the spread.
    -> (index [g,k] int64, log_prob [g,k], mass [g,k], log_norm [g], spread [g] in radians or None)"""
    g, Q = logp.shape
    dev = logp.device
    lp = logp.to(torch.float32).contiguous()
    grid = grid.reshape(Q, 9).to(torch.float32).contiguous()
    gt = None if gt is None else gt.reshape(g, -1, 9).to(device=dev, dtype=torch.float32).contiguous()
    index = torch.empty(g, top_k, dtype=torch.int64, device=dev)
    log_prob = torch.empty(g, top_k, dtype=torch.float32, device=dev)
    mass = torch.empty(g, top_k, dtype=torch.float32, device=dev)
    log_norm = torch.empty(g, dtype=torch.float32, device=dev)
    spread = torch.empty(g, dtype=torch.float32, device=dev) if gt is not None else None
    args = _lib.GridModes(logp=lp.data_ptr(), grid=grid.data_ptr(), Q=Q, g=g, top_k=int(top_k), separation_rad=float(separation_rad),
                          gt=gt.data_ptr() if gt is not None else None, n_gt=gt.shape[1] if gt is not None else 0,
                          index_out=index.data_ptr(), logp_out=log_prob.data_ptr(), mass_out=mass.data_ptr(),
                          log_norm_out=log_norm.data_ptr(), spread_out=spread.data_ptr() if spread is not None else None)
    _lib.call("grid_modes", args, dev)
    return index, log_prob, mass, log_norm, spread


def grid_pose_modes(flow: Flow, feature: torch.Tensor = None, top_k: int = 4, separation_deg: float = 15.0, number_queries: int = None,
                    recursion_level: int = None, offset=None, base=None, gt_rotation=None, images_per_launch: int = None) -> dict:
    """The ``top_k`` pose modes of each image's density on the grid of ``grid_estimate_rotations`` (same inputs, same launches), at least
    ``separation_deg`` apart, with the probability mass of each.  Grid cells have equal Haar volume and the flow's density is relative to the
    normalised Haar measure, so exp(log p_i) / Q is cell i's mass; ``log_norm`` = log(sum_i exp(log p_i) / Q) tends to 0 as the grid level
    grows.  Mode 0 is ``grid_estimate_rotations``'s estimate; mode j the first arg-max among the points at least ``separation_deg`` from
    modes 0..j-1, its mass that of the points within ``separation_deg`` of it and of no earlier mode (``rnf_grid_modes``,
    include/rnf_hip.h).  Modes that do not exist have index -1, log p -inf, mass 0 and NaN rotations.  ``gt_rotation`` [B,K,3,3] or
    [B,3,3] adds IPDF's spread: the expected angle (degrees) to the closest ground truth under the grid-normalised mass.
    An image whose grid is evaluated in chunks (more than 2^24 rows, level >= 6; 2^18 with side layers) has its chunks gathered into one
    [Q] float32 buffer (4 bytes per grid row) before the reduction.
    -> dict(est [B,k,3,3], log_prob [B,k], index [B,k] int64, mass [B,k], log_norm [B], spread_deg [B] (with gt_rotation), offset [3,3])"""
    if not 1 <= int(top_k) <= 16:
        raise ValueError(f"grid_pose_modes: top_k={top_k} outside 1..16")
    if not 0.0 < float(separation_deg) <= 180.0:
        raise ValueError(f"grid_pose_modes: separation_deg={separation_deg} outside (0, 180]")
    k, sep = int(top_k), float(np.deg2rad(np.float64(separation_deg)))
    gf, level, offset = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, "grid_pose_modes")
    gt = None
    if gt_rotation is not None:
        gt = gt_rotation.reshape(gf.B, -1, 3, 3).to(device=gf.dev, dtype=torch.float32)
        if gt.shape[1] > 128:
            raise ValueError(f"grid_pose_modes: {gt.shape[1]} ground truths per image (at most 128)")
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        outs = []
        for b0, b1, lp in gf.images(grid, images_per_launch, "grid_pose_modes"):
            outs.append(grid_modes(lp, grid, k, sep, gt[b0:b1] if gt is not None else None))
        index, log_prob, mass, log_norm, spread = (torch.cat(t) if t[0] is not None else None for t in zip(*outs))
        est = grid[index.clamp(min=0)]
        est[index < 0] = float("nan")
    out = dict(est=est, log_prob=log_prob, index=index, mass=mass, log_norm=log_norm, offset=offset)
    if gt is not None:
        out["spread_deg"] = torch.rad2deg(spread)
    return out


def grid_modes_refine(logp: torch.Tensor, grid: torch.Tensor, est: torch.Tensor, kappa: float = None, tol: float = 1e-5, max_steps: int = 200,
                      check_every: int = 8):
    """Mean shift of grid modes off the grid: image b's modes ``est`` [g,k,3,3] (grid rows, e.g. ``grid[index]`` of ``grid_modes``) climb
    the kernel-smoothed grid posterior sum_i softmax(logp_b)_i k_kappa(R_i, .) (``utils.kde.so3_kernel_moments`` with the grid as
    centres, ``logp`` [g,Q] as log-weights and one set of queries per image).  ``kappa`` defaults to 0.5 / s^2 with s = (8 pi^2 / Q)^(1/3)
    rad, the grid spacing.  A NaN mode stays NaN.  -> (refined [g,k,3,3], converged [g,k] bool)"""
    from .utils.kde import _kappas, _mean_shift
    who = "grid_modes_refine"
    if not (isinstance(logp, torch.Tensor) and logp.dim() == 2 and isinstance(grid, torch.Tensor) and tuple(grid.shape) == (logp.shape[1], 3, 3)):
        raise ValueError(f"{who}: logp {tuple(getattr(logp, 'shape', ()))} and grid {tuple(getattr(grid, 'shape', ()))}, expected [g,Q] and [Q,3,3]")
    if not (isinstance(est, torch.Tensor) and est.dim() == 4 and est.shape[0] == logp.shape[0] and tuple(est.shape[2:]) == (3, 3)):
        raise ValueError(f"{who}: est {tuple(getattr(est, 'shape', ()))}, expected [{logp.shape[0]},k,3,3]")
    if not (logp.is_cuda and grid.is_cuda and est.is_cuda):
        raise ValueError(f"{who}: logp, grid and est must be on the GPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    Q = grid.shape[0]
    k = 0.5 / (8.0 * np.pi ** 2 / Q) ** (2.0 / 3.0) if kappa is None else float(kappa)
    (k,), _ = _kappas(min(k, 1e6) if kappa is None else k, who)
    refined, converged, _ = _mean_shift(grid, est, k, logp, True, float(tol), max_steps, check_every)
    return refined, converged


def grid_pose_modes_refined(flow: Flow, feature: torch.Tensor = None, top_k: int = 4, separation_deg: float = 15.0, kappa: float = None,
                            number_queries: int = None, recursion_level: int = None, offset=None, base=None, gt_rotation=None,
                            images_per_launch: int = None, tol: float = 1e-5, max_steps: int = 200, check_every: int = 8) -> dict:
    """``grid_pose_modes`` (same inputs, same launches), then each mode is taken off the grid by mean shift on the kernel-smoothed grid
    posterior (``grid_modes_refine``; ``kappa`` defaults to 0.5 / s^2, s the grid spacing in radians).
    -> the dict of ``grid_pose_modes`` plus ``refined`` [B,k,3,3] and ``converged`` [B,k]; modes that do not exist stay NaN.
    What it is and is not: ``refined`` is the mode of the SMOOTHED posterior, and it helps only where the density is wider than the grid
    spacing.  An fp64 run at level 3 on a 0.6 MF(20 R0) + 0.4 MF(20 R0 Rz(180)) posterior gave a mean error of 3.78 degrees for the
    arg-max and 0.02 to 0.05 degrees for kappa = 10..40; the same run with concentration 200 gave no gain at any kappa, and level 1
    gave none."""
    if not 1 <= int(top_k) <= 16:
        raise ValueError(f"grid_pose_modes_refined: top_k={top_k} outside 1..16")
    if not 0.0 < float(separation_deg) <= 180.0:
        raise ValueError(f"grid_pose_modes_refined: separation_deg={separation_deg} outside (0, 180]")
    k, sep = int(top_k), float(np.deg2rad(np.float64(separation_deg)))
    gf, level, offset = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, "grid_pose_modes_refined")
    gt = None
    if gt_rotation is not None:
        gt = gt_rotation.reshape(gf.B, -1, 3, 3).to(device=gf.dev, dtype=torch.float32)
        if gt.shape[1] > 128:
            raise ValueError(f"grid_pose_modes_refined: {gt.shape[1]} ground truths per image (at most 128)")
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        outs, refs = [], []
        for b0, b1, lp in gf.images(grid, images_per_launch, "grid_pose_modes_refined"):
            res = grid_modes(lp, grid, k, sep, gt[b0:b1] if gt is not None else None)
            start = grid[res[0].clamp(min=0)]
            start[res[0] < 0] = float("nan")
            outs.append(res)
            refs.append((start,) + grid_modes_refine(lp, grid, start, kappa, tol, max_steps, check_every))
        index, log_prob, mass, log_norm, spread = (torch.cat(t) if t[0] is not None else None for t in zip(*outs))
        est, refined, converged = (torch.cat(t) for t in zip(*refs))
    out = dict(est=est, log_prob=log_prob, index=index, mass=mass, log_norm=log_norm, offset=offset, refined=refined, converged=converged)
    if gt is not None:
        out["spread_deg"] = torch.rad2deg(spread)
    return out


def _error_args(logp, grid, who: str):
    if not (isinstance(logp, torch.Tensor) and logp.dim() == 2 and isinstance(grid, torch.Tensor) and tuple(grid.shape) == (logp.shape[1], 3, 3)):
        raise ValueError(f"{who}: logp {tuple(getattr(logp, 'shape', ()))} and grid {tuple(getattr(grid, 'shape', ()))}, expected [g,Q] and [Q,3,3]")
    if not 1 <= logp.shape[0] <= 65535:
        raise ValueError(f"{who}: logp holds {logp.shape[0]} images (1 to 65535)")


def _chord2(a, b):
    """|a - b|_F^2 of rotations [...,3,3] in fp64 (8 sin^2 of half the angle between them)"""
    d = a.to(torch.float64) - b.to(torch.float64)
    return (d * d).sum(dim=(-2, -1))


def grid_error(logp: torch.Tensor, grid: torch.Tensor, est: torch.Tensor, thresholds_deg=(15.0, 30.0), levels=(0.5, 0.9), gt: torch.Tensor = None,
               tol_deg: float = 0.05) -> dict:
    """The posterior distribution of the error of point estimates, in the units of Acc@theta and the median error: with image b's grid
    posterior softmax(``logp``[b]) over ``grid`` [Q,3,3] and its estimates ``est`` [g,k,3,3] (any rotations: grid rows, refined modes,
    another method's output), the distribution function of the geodesic angle from each estimate to the posterior
    (``utils.angles.so3_angle_cdf`` with the grid as centres, ``logp`` [g,Q] as log-weights and one set of queries per image) gives
    ``acc`` [g,k,T], the mass within each of ``thresholds_deg`` (up to 8, in [0, 180]) -- the predicted Acc@theta of that estimate;
    ``expected_deg`` and ``rms_deg`` [g,k], the mean and root-mean-square angle; and ``radius_deg`` [g,k,L], for each of ``levels`` in
    (0, 1) the radius at which the ball about the estimate reaches that mass (``so3_angle_quantile``, to ``tol_deg``): level 0.5 is the
    predicted median error.  A NaN estimate, such as a missing mode of ``grid_pose_modes``, gives NaN.
    ``gt`` [g,3,3], one ground truth per image, adds ``error_deg`` [g,k], the realised angle, and ``pit`` [g,k] = F(error): the mass of
    the ball about the estimate that just reaches the truth (one call with the squared chordal distance |est - gt|_F^2 as the query's
    threshold).  It is uniform on [0, 1] for a calibrated model: the radial counterpart of ``grid_pose_credible``'s HPD level.  A set of
    several symmetric truths per image is refused: the error about one estimate under a symmetric posterior needs a convention for
    the closest mode, which ``grid_error_symmetric`` and ``grid_set_error`` supply.  All float32 on the device; no host synchronisation."""
    from .utils.angles import so3_angle_cdf, so3_angle_quantile
    who = "grid_error"
    _error_args(logp, grid, who)
    if not (isinstance(est, torch.Tensor) and est.dim() == 4 and est.shape[0] == logp.shape[0] and tuple(est.shape[2:]) == (3, 3)):
        raise ValueError(f"{who}: est {tuple(getattr(est, 'shape', ()))}, expected [{logp.shape[0]},k,3,3]")
    th = [float(t) for t in (thresholds_deg if isinstance(thresholds_deg, (tuple, list)) else [thresholds_deg])]
    if len(th) > 8 or not all(0.0 <= t <= 180.0 for t in th):
        raise ValueError(f"{who}: thresholds_deg={tuple(th)}: up to 8 angles in 0..180 degrees")
    lv = [float(a) for a in (levels if isinstance(levels, (tuple, list)) else [levels])]
    if not all(0.0 < a < 1.0 for a in lv):
        raise ValueError(f"{who}: level outside (0, 1) in levels={tuple(lv)}")
    if not 0.0 < float(tol_deg) <= 180.0:
        raise ValueError(f"{who}: tol_deg={tol_deg} outside (0, 180]")
    if gt is not None:
        if isinstance(gt, torch.Tensor) and gt.dim() == 4 and gt.shape[1] > 1:
            raise ValueError(f"{who}: gt holds {gt.shape[1]} symmetric ground truths per image; the error about one estimate is defined for one")
        if not (isinstance(gt, torch.Tensor) and gt.numel() == logp.shape[0] * 9):
            raise ValueError(f"{who}: gt {tuple(getattr(gt, 'shape', ()))}, expected [{logp.shape[0]},3,3]")
    if not (logp.is_cuda and grid.is_cuda and est.is_cuda and (gt is None or gt.is_cuda)):
        raise ValueError(f"{who}: logp, grid, est and gt must be on the GPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    g, k = est.shape[:2]
    rad = [float(np.pi) if t >= 180.0 else float(np.deg2rad(np.float64(t))) for t in th]
    cdf = so3_angle_cdf(grid, est, rad if rad else None, None, logp, group_queries=True)
    out = dict(acc=cdf["mass"].permute(0, 2, 1).contiguous(), expected_deg=torch.rad2deg(cdf["mean_angle"]), rms_deg=torch.rad2deg(cdf["rms_angle"]))
    if lv:
        q = so3_angle_quantile(grid, est, lv, logp, group_queries=True, tol=float(np.deg2rad(np.float64(tol_deg))))
        out["radius_deg"] = torch.rad2deg(q["radius"]).permute(0, 2, 1).to(torch.float32).contiguous()
    else:
        out["radius_deg"] = torch.empty(g, k, 0, dtype=torch.float32, device=logp.device)
    if gt is not None:
        d2 = _chord2(est, gt.reshape(g, 1, 3, 3).to(est.device))                           # [g,k] fp64; NaN where the estimate is
        out["error_deg"] = torch.rad2deg(2.0 * torch.asin(torch.sqrt(d2 / 8.0).clamp(max=1.0))).to(torch.float32)
        tau = d2.to(torch.float32)[:, None, :]                                              # rounded once: the threshold of the one call
        out["pit"] = so3_angle_cdf(grid, est, None, tau, logp, group_queries=True, moments=False)["mass"][:, 0]
    return out


def grid_pose_error(flow: Flow, feature: torch.Tensor = None, est: torch.Tensor = None, thresholds_deg=(15.0, 30.0), levels=(0.5, 0.9),
                    number_queries: int = None, recursion_level: int = None, offset=None, base=None, gt_rotation=None,
                    images_per_launch: int = None) -> dict:
    """``grid_error`` of each image's density on the grid of ``grid_estimate_rotations`` (same inputs, same launches, the chunk gathering of
    ``grid_pose_modes``).  ``est`` [B,k,3,3] or [B,3,3]: the estimates to judge; None: each image's grid arg-max, the rotation
    ``grid_estimate_rotations`` returns (k = 1).  ``gt_rotation`` [B,3,3]: one ground truth per image, for ``error_deg`` and ``pit``.
    -> the dict of ``grid_error`` (every entry with a leading B) plus ``est`` [B,k,3,3], ``index`` [B] int64 (the grid arg-max, as
    ``grid_estimate_rotations``), ``log_norm`` [B] = log(sum_i exp(log p_i) / Q) and ``offset`` [3,3]."""
    who = "grid_pose_error"
    gf, level, offset = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, who)
    B = gf.B
    if est is not None:
        if not (isinstance(est, torch.Tensor) and est.dim() in (3, 4) and est.shape[0] == B and tuple(est.shape[-2:]) == (3, 3)):
            raise ValueError(f"{who}: est {tuple(getattr(est, 'shape', ()))}, expected [{B},k,3,3] or [{B},3,3]")
        est = est.reshape(B, -1, 3, 3).to(device=gf.dev, dtype=torch.float32)
    gt = None
    if gt_rotation is not None:
        if gt_rotation.dim() == 4 and gt_rotation.shape[1] > 1:
            raise ValueError(f"{who}: gt_rotation holds {gt_rotation.shape[1]} symmetric ground truths per image; the error about one "
                             "estimate is defined for one")
        gt = gt_rotation.reshape(B, 3, 3).to(device=gf.dev, dtype=torch.float32)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        Q = grid.shape[0]
        outs = []
        for b0, b1, lp in gf.images(grid, images_per_launch, who):
            index = torch.argmax(lp, dim=1)
            e = est[b0:b1] if est is not None else grid[index][:, None]
            res = grid_error(lp, grid, e, thresholds_deg, levels, gt[b0:b1] if gt is not None else None)
            res.update(est=e, index=index, log_norm=(torch.logsumexp(lp.to(torch.float64), dim=1) - float(np.log(Q))).to(torch.float32))
            outs.append(res)
    out = outs[0] if len(outs) == 1 else {key: torch.cat([o[key] for o in outs]) for key in outs[0]}
    out["offset"] = offset
    return out


def _error_options(thresholds_deg, levels, tol_deg, who: str):
    """-> (thresholds in radians, levels) of the error functions, checked"""
    th = [float(t) for t in (thresholds_deg if isinstance(thresholds_deg, (tuple, list)) else [thresholds_deg])]
    if len(th) > 8 or not all(0.0 <= t <= 180.0 for t in th):
        raise ValueError(f"{who}: thresholds_deg={tuple(th)}: up to 8 angles in 0..180 degrees")
    lv = [float(a) for a in (levels if isinstance(levels, (tuple, list)) else [levels])]
    if not all(0.0 < a < 1.0 for a in lv):
        raise ValueError(f"{who}: level outside (0, 1) in levels={tuple(lv)}")
    if not 0.0 < float(tol_deg) <= 180.0:
        raise ValueError(f"{who}: tol_deg={tol_deg} outside (0, 180]")
    return [float(np.pi) if t >= 180.0 else float(np.deg2rad(np.float64(t))) for t in th], lv


def grid_set_error(logp: torch.Tensor, grid: torch.Tensor, sets: torch.Tensor, thresholds_deg=(15.0, 30.0), levels=(0.5, 0.9),
                   tol_deg: float = 0.05) -> dict:
    """``grid_error`` with a SET of rotations in place of each estimate: the posterior distribution of the angle to the nearest member
    (``utils.angles.so3_set_angle_cdf``).  ``sets`` [g,k,K,3,3]: k sets of K members per image; a member with a non-finite entry is
    padding and is skipped, a set of padding only gives NaN.  -> ``acc`` [g,k,T], the mass of the union of the balls of each threshold
    about the members; ``expected_deg``, ``rms_deg`` [g,k] and ``radius_deg`` [g,k,L] of the angle to the nearest member.
    With ``sets = modes["est"][:, None]`` -- the k modes of ``grid_pose_modes`` taken as ONE set, missing (NaN) modes counting
    as padding -- ``acc`` is the predicted best-of-k Acc@theta, the counterpart of ``pose_accuracy(top_k=k)``; with the orbit of an
    estimate under a symmetry group it is ``grid_error_symmetric``.  All float32 on the device; no host synchronisation."""
    from .utils.angles import so3_set_angle_cdf, so3_set_angle_quantile
    who = "grid_set_error"
    _error_args(logp, grid, who)
    if not (isinstance(sets, torch.Tensor) and sets.dim() == 5 and sets.shape[0] == logp.shape[0] and tuple(sets.shape[3:]) == (3, 3)):
        raise ValueError(f"{who}: sets {tuple(getattr(sets, 'shape', ()))}, expected [{logp.shape[0]},k,K,3,3]")
    if not 1 <= sets.shape[2] <= 4096:
        raise ValueError(f"{who}: sets of {sets.shape[2]} members (1 to 4096)")
    rad, lv = _error_options(thresholds_deg, levels, tol_deg, who)
    if not (logp.is_cuda and grid.is_cuda and sets.is_cuda):
        raise ValueError(f"{who}: logp, grid and sets must be on the GPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    g, k = sets.shape[:2]
    cdf = so3_set_angle_cdf(grid, sets, rad if rad else None, None, logp, group_queries=True)
    out = dict(acc=cdf["mass"].permute(0, 2, 1).contiguous(), expected_deg=torch.rad2deg(cdf["mean_angle"]), rms_deg=torch.rad2deg(cdf["rms_angle"]))
    if lv:
        q = so3_set_angle_quantile(grid, sets, lv, logp, group_queries=True, tol=float(np.deg2rad(np.float64(tol_deg))))
        out["radius_deg"] = torch.rad2deg(q["radius"]).permute(0, 2, 1).to(torch.float32).contiguous()
    else:
        out["radius_deg"] = torch.empty(g, k, 0, dtype=torch.float32, device=logp.device)
    return out


def grid_error_symmetric(logp: torch.Tensor, grid: torch.Tensor, est: torch.Tensor, symmetry: torch.Tensor = None, thresholds_deg=(15.0, 30.0),
                         levels=(0.5, 0.9), gt: torch.Tensor = None, tol_deg: float = 0.05) -> dict:
    """``grid_error`` for a symmetric object: the error of an estimate E is the angle to the nearest of the equivalent poses E S_s, S
    the object's symmetry group acting in the body frame (``utils.symmetry``), which is how SYMSOL scores (the angle to the nearest of a
    set of equivalent ground truths).  ``est`` [g,k,3,3]; ``symmetry`` [K,3,3] (``point_group``) or [g,K,3,3], one group per image, NaN
    members as padding; None with ``gt`` [g,K',3,3]: the group recovered from the truths (``symmetry_from_truths``).
    -> ``acc``, ``expected_deg``, ``rms_deg``, ``radius_deg`` as ``grid_set_error`` with ``orbit(est, symmetry)`` as its sets.
    ``gt`` [g,3,3] or [g,K',3,3] (equivalent truths, the first is used) adds ``error_deg`` [g,k], the least angle from a member of the
    orbit to the truth -- ``min_geodesic_distance(est, gt)`` when ``gt`` is the truth's orbit under the same group -- and ``pit`` [g,k]
    = F(error), from one call with the threshold min_s |est S_s - gt_0|_F^2 formed in fp64 and rounded once."""
    from .utils.angles import so3_set_angle_cdf
    from .utils.symmetry import orbit, symmetry_from_truths
    who = "grid_error_symmetric"
    _error_args(logp, grid, who)
    g = logp.shape[0]
    if not (isinstance(est, torch.Tensor) and est.dim() == 4 and est.shape[0] == g and tuple(est.shape[2:]) == (3, 3)):
        raise ValueError(f"{who}: est {tuple(getattr(est, 'shape', ()))}, expected [{g},k,3,3]")
    if gt is not None and not (isinstance(gt, torch.Tensor) and ((gt.dim() == 3 and tuple(gt.shape) == (g, 3, 3)) or (
            gt.dim() == 4 and gt.shape[0] == g and gt.shape[1] >= 1 and tuple(gt.shape[2:]) == (3, 3)))):
        raise ValueError(f"{who}: gt {tuple(getattr(gt, 'shape', ()))}, expected [{g},3,3] or [{g},K,3,3]")
    if symmetry is None:
        if gt is None or gt.dim() != 4:
            raise ValueError(f"{who}: symmetry=None needs gt [{g},K,3,3], a set of equivalent truths per image to recover the group from")
        symmetry = symmetry_from_truths(gt.to(device=est.device, dtype=torch.float32))
    if not (isinstance(symmetry, torch.Tensor) and symmetry.dim() in (3, 4) and tuple(symmetry.shape[-2:]) == (3, 3) and (
            symmetry.dim() == 3 or symmetry.shape[0] == g)):
        raise ValueError(f"{who}: symmetry {tuple(getattr(symmetry, 'shape', ()))}, expected [K,3,3] or [{g},K,3,3]")
    if not (logp.is_cuda and grid.is_cuda and est.is_cuda and symmetry.is_cuda and (gt is None or gt.is_cuda)):
        raise ValueError(f"{who}: logp, grid, est, symmetry and gt must be on the GPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    sym = symmetry.to(device=est.device, dtype=torch.float32)
    sets = orbit(est.to(torch.float32), sym if sym.dim() == 3 else sym[:, None]).contiguous()    # [g,k,K,3,3]
    out = grid_set_error(logp, grid, sets, thresholds_deg, levels, tol_deg)
    if gt is not None:
        gt0 = gt.reshape(g, -1, 3, 3)[:, 0].to(est.device)
        d2s = _chord2(sets, gt0[:, None, None])                                             # [g,k,K] fp64; NaN for padding members
        dead = torch.isnan(d2s)
        d2 = torch.where(dead, torch.full_like(d2s, float("inf")), d2s).amin(dim=2)
        d2 = torch.where(dead.all(dim=2), torch.full_like(d2, float("nan")), d2)            # NaN where the estimate or the truth is
        out["error_deg"] = torch.rad2deg(2.0 * torch.asin(torch.sqrt(d2 / 8.0).clamp(max=1.0))).to(torch.float32)
        tau = d2.to(torch.float32)[:, None, :]                                              # rounded once: the threshold of the one call
        out["pit"] = so3_set_angle_cdf(grid, sets, None, tau, logp, group_queries=True, moments=False)["mass"][:, 0]
    return out


def grid_pose_error_symmetric(flow: Flow, feature: torch.Tensor = None, symmetry: torch.Tensor = None, est: torch.Tensor = None,
                              gt_rotation: torch.Tensor = None, thresholds_deg=(15.0, 30.0), levels=(0.5, 0.9), number_queries: int = None,
                              recursion_level: int = None, offset=None, base=None, images_per_launch: int = None) -> dict:
    """``grid_error_symmetric`` of each image's density on the grid of ``grid_estimate_rotations`` (same inputs, same launches, the chunk
    gathering of ``grid_pose_modes``), as ``grid_pose_error`` is to ``grid_error``.  ``symmetry`` [K,3,3] or [B,K,3,3]; None: recovered
    from ``gt_rotation`` [B,K,3,3].  ``est`` [B,k,3,3] or [B,3,3]; None: each image's grid arg-max.  ``gt_rotation`` [B,3,3] or
    [B,K,3,3] for ``error_deg`` and ``pit``.
    -> the dict of ``grid_error_symmetric`` (every entry with a leading B) plus ``est``, ``index``, ``log_norm`` and ``offset``."""
    who = "grid_pose_error_symmetric"
    gf, level, offset = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, who)
    B = gf.B
    if est is not None:
        if not (isinstance(est, torch.Tensor) and est.dim() in (3, 4) and est.shape[0] == B and tuple(est.shape[-2:]) == (3, 3)):
            raise ValueError(f"{who}: est {tuple(getattr(est, 'shape', ()))}, expected [{B},k,3,3] or [{B},3,3]")
        est = est.reshape(B, -1, 3, 3).to(device=gf.dev, dtype=torch.float32)
    gt = None
    if gt_rotation is not None:
        if not (isinstance(gt_rotation, torch.Tensor) and gt_rotation.dim() in (3, 4) and gt_rotation.shape[0] == B):
            raise ValueError(f"{who}: gt_rotation {tuple(getattr(gt_rotation, 'shape', ()))}, expected [{B},3,3] or [{B},K,3,3]")
        gt = gt_rotation.to(device=gf.dev, dtype=torch.float32)
    if symmetry is not None:
        if not (isinstance(symmetry, torch.Tensor) and symmetry.dim() in (3, 4) and (symmetry.dim() == 3 or symmetry.shape[0] == B)):
            raise ValueError(f"{who}: symmetry {tuple(getattr(symmetry, 'shape', ()))}, expected [K,3,3] or [{B},K,3,3]")
        symmetry = symmetry.to(device=gf.dev, dtype=torch.float32)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        Q = grid.shape[0]
        outs = []
        for b0, b1, lp in gf.images(grid, images_per_launch, who):
            index = torch.argmax(lp, dim=1)
            e = est[b0:b1] if est is not None else grid[index][:, None]
            sym = symmetry[b0:b1] if symmetry is not None and symmetry.dim() == 4 else symmetry
            res = grid_error_symmetric(lp, grid, e, sym, thresholds_deg, levels, gt[b0:b1] if gt is not None else None)
            res.update(est=e, index=index, log_norm=(torch.logsumexp(lp.to(torch.float64), dim=1) - float(np.log(Q))).to(torch.float32))
            outs.append(res)
    out = outs[0] if len(outs) == 1 else {key: torch.cat([o[key] for o in outs]) for key in outs[0]}
    out["offset"] = offset
    return out


def grid_ball_estimate(logp: torch.Tensor, grid: torch.Tensor, radius_deg: float = 15.0, candidates: int = 4096) -> dict:
    """The point estimate to report when scored by Acc@theta and not by density: among each image's ``candidates`` densest grid rows
    (``torch.topk``; None: every grid row), the one whose ball of ``radius_deg`` carries the most mass under softmax(``logp``[b])
    (``utils.angles.so3_angle_cdf`` with the candidates as per-image queries).  A tie goes to the denser row, then to the lower index --
    the first in the candidates' order.  The maximiser over the candidates need not be the maximiser over SO(3): the ball's centre is
    restricted to grid rows, and with ``candidates`` below Q to the densest of them; a broad mode whose rows are all less dense than
    ``candidates`` rows elsewhere is not seen.  Cost: Q x candidates pairs per image.
    -> dict(est [g,3,3], index [g] int64 (-1 and NaN where the image's masses are NaN), mass [g], argmax_index [g] int64 and
    argmax_mass [g]: the densest row and its own ball mass, for comparison)"""
    from .utils.angles import so3_angle_cdf
    who = "grid_ball_estimate"
    _error_args(logp, grid, who)
    if not 0.0 < float(radius_deg) <= 180.0:
        raise ValueError(f"{who}: radius_deg={radius_deg} outside (0, 180]")
    g, Q = logp.shape
    if candidates is not None and not 1 <= int(candidates):
        raise ValueError(f"{who}: candidates={candidates} (at least 1, or None for every grid row)")
    if not (logp.is_cuda and grid.is_cuda):
        raise ValueError(f"{who}: logp and grid must be on the GPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    rad = float(np.pi) if float(radius_deg) >= 180.0 else float(np.deg2rad(np.float64(radius_deg)))
    lp = logp.detach().to(torch.float32)
    top = torch.argmax(lp, dim=1)                                                            # [g]
    if candidates is None:
        rows = torch.arange(Q, device=lp.device)[None].expand(g, Q)
        mass = so3_angle_cdf(grid, grid, [rad], None, lp, moments=False)["mass"][:, 0]       # [g,Q]: shared queries
        top_mass = mass.gather(1, top[:, None])[:, 0]
    else:
        rows = torch.topk(lp, min(int(candidates), Q), dim=1).indices                        # [g,c]
        queries = torch.cat([grid[top][:, None], grid[rows]], dim=1)                         # the arg-max first: its mass with its own bits
        mass = so3_angle_cdf(grid, queries, [rad], None, lp, group_queries=True, moments=False)["mass"][:, 0]
        top_mass, mass = mass[:, 0], mass[:, 1:]
    dens = lp.gather(1, rows)
    best = torch.where(torch.isnan(mass), torch.full_like(mass, -1.0), mass).max(dim=1, keepdim=True).values
    tied = mass == best
    dens_best = torch.where(tied, dens, torch.full_like(dens, -float("inf"))).max(dim=1, keepdim=True).values
    index = torch.where(tied & (dens == dens_best), rows, torch.full_like(rows, Q)).min(dim=1).values
    none = index == Q
    index = torch.where(none, torch.full_like(index, -1), index)
    est = grid[index.clamp(min=0)].clone()
    est[none] = float("nan")
    return dict(est=est, index=index, mass=torch.where(none, torch.full_like(best[:, 0], float("nan")), best[:, 0]), argmax_index=top,
                argmax_mass=top_mass)


def grid_pose_ball_estimate(flow: Flow, feature: torch.Tensor = None, radius_deg: float = 15.0, candidates: int = 4096,
                            number_queries: int = None, recursion_level: int = None, offset=None, base=None,
                            images_per_launch: int = None) -> dict:
    """``grid_ball_estimate`` of each image's density on the grid of ``grid_estimate_rotations`` (same inputs, same launches, the chunk
    gathering of ``grid_pose_modes``): the Acc@``radius_deg``-optimal grid row among each image's ``candidates`` densest.
    -> the dict of ``grid_ball_estimate`` (every entry with a leading B) plus ``offset`` [3,3]"""
    who = "grid_pose_ball_estimate"
    if not 0.0 < float(radius_deg) <= 180.0:
        raise ValueError(f"{who}: radius_deg={radius_deg} outside (0, 180]")
    gf, level, offset = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, who)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        outs = [grid_ball_estimate(lp, grid, radius_deg, candidates) for _, _, lp in gf.images(grid, images_per_launch, who)]
    out = outs[0] if len(outs) == 1 else {key: torch.cat([o[key] for o in outs]) for key in outs[0]}
    out["offset"] = offset
    return out


GRID_CREDIBLE_MAX_ROWS = 1 << 26                  # rnf_grid_credible's fixed point (include/rnf_hip.h): level 6 fits
GRID_CREDIBLE_MAX_LEVELS = 8
GRID_CREDIBLE_MAX_QUERIES = 16
GRID_GT_ROW = 32                                    # the shortest shared row on the fast shared-row kernels (csrc/flow_plan.h)


def _credible_levels(levels, who: str):
    lv = [float(a) for a in (levels if isinstance(levels, (tuple, list)) else np.asarray(levels, np.float64).reshape(-1))]
    if not 1 <= len(lv) <= GRID_CREDIBLE_MAX_LEVELS:
        raise ValueError(f"{who}: {len(lv)} levels (1 to {GRID_CREDIBLE_MAX_LEVELS})")
    for a in lv:
        if not 0.0 < a < 1.0:
            raise ValueError(f"{who}: level {a} outside (0, 1)")
    return lv


def grid_credible(logp: torch.Tensor, levels, queries: torch.Tensor = None):
    """``rnf_grid_credible`` on g images' log-densities ``logp`` [g,Q] (float32, on the device): per level alpha the highest-density
    credible set {log p >= threshold}, the smallest such set of grid cells with mass >= alpha, and per query log-density v [g,G] the mass
    and number of the cells with log p > v (include/rnf_hip.h).
    -> (threshold [g,J], count [g,J] int64, mass [g,J], log_norm [g], query_mass [g,G] or None, query_count [g,G] int64 or None)"""
    lv = _credible_levels(levels, "grid_credible")
    g, Q = logp.shape
    if Q > GRID_CREDIBLE_MAX_ROWS:
        raise ValueError(f"grid_credible: {Q} grid rows (at most 2^26)")
    dev = logp.device
    lp = logp.to(torch.float32).contiguous()
    J, G = len(lv), 0
    if queries is not None:
        queries = queries.reshape(g, -1).to(device=dev, dtype=torch.float32).contiguous()
        G = queries.shape[1]
        if not 1 <= G <= GRID_CREDIBLE_MAX_QUERIES:
            raise ValueError(f"grid_credible: {G} queries per image (at most {GRID_CREDIBLE_MAX_QUERIES})")
    threshold = torch.empty(g, J, dtype=torch.float32, device=dev)
    count = torch.empty(g, J, dtype=torch.int64, device=dev)
    mass = torch.empty(g, J, dtype=torch.float32, device=dev)
    log_norm = torch.empty(g, dtype=torch.float32, device=dev)
    query_mass = torch.empty(g, G, dtype=torch.float32, device=dev) if G else None
    query_count = torch.empty(g, G, dtype=torch.int64, device=dev) if G else None
    host_levels = (C.c_double * J)(*lv)
    args = _lib.GridCredible(logp=lp.data_ptr(), Q=Q, g=g, levels=C.addressof(host_levels), n_levels=J,
                             queries=queries.data_ptr() if G else None, n_queries=G, threshold_out=threshold.data_ptr(),
                             count_out=count.data_ptr(), mass_out=mass.data_ptr(), log_norm_out=log_norm.data_ptr(),
                             query_mass_out=query_mass.data_ptr() if G else None, query_count_out=query_count.data_ptr() if G else None)
    _lib.call("grid_credible", args, dev)
    return threshold, count, mass, log_norm, query_mass, query_count


def grid_pose_credible(flow: Flow, feature: torch.Tensor = None, levels=(0.5, 0.9, 0.95), number_queries: int = None,
                       recursion_level: int = None, offset=None, base=None, gt_rotation=None, images_per_launch: int = None) -> dict:
    """Highest-density credible sets of each image's density on the grid of ``grid_estimate_rotations`` (same inputs, same launches, the
    chunk gathering of ``grid_pose_modes``): per level alpha the smallest set of grid cells {log p >= threshold} that carries mass alpha
    under the grid-normalised density, its number of cells ``count`` and its ``volume`` = count / Q as a fraction of SO(3).  Cell masses
    are fixed-point integers, so the sets are exact order statistics, bit-identical from run to run and for any grouping; a reported mass is
    within Q 2^-(S+1), S = 62 - ceil(log2 Q), of the real-valued one (``rnf_grid_credible``, include/rnf_hip.h; 1.1e-6 at level 5).
    ``gt_rotation`` [B,3,3] or [B,K,3,3] (K <= 16 symmetric ground truths) adds the calibration statistics: the flow's log-density at the
    ground truths themselves (the densest of an image's K), evaluated like a grid row -- a ground truth that is a grid row gets that row's
    log p bit for bit, except in flows with batch-coupled layers, whose matrices come from the first rows of a launch: there the ground
    truths' own launch (one per image) builds them from the ground truths, not from the grid's first rows; ``gt_level`` = the mass of the
    cells denser than it, its HPD level, uniform on [0, 1] for a calibrated model; and ``gt_inside`` [B,J] = gt_log_prob >= threshold.
    ``gt_inside.float().mean(0)`` is the coverage curve: the fraction of images whose alpha-set holds the ground truth, alpha when
    calibrated.  Grids above 2^26 rows (level 7) are refused.
    -> dict(threshold [B,J], count [B,J] int64, volume [B,J], mass [B,J], log_norm [B], offset [3,3]; with gt_rotation: gt_log_prob [B],
    gt_level [B], gt_inside [B,J] bool)"""
    lv = _credible_levels(levels, "grid_pose_credible")
    level = int(recursion_level) if recursion_level is not None else sd.closest_grid_level(500 if number_queries is None else number_queries)
    if sd.grid_size(level) > GRID_CREDIBLE_MAX_ROWS:
        raise ValueError(f"grid_pose_credible: level {level} has {sd.grid_size(level)} grid rows (at most 2^26)")
    if gt_rotation is not None and gt_rotation.dim() == 4 and gt_rotation.shape[1] > GRID_CREDIBLE_MAX_QUERIES:
        raise ValueError(f"grid_pose_credible: {gt_rotation.shape[1]} ground truths per image (at most {GRID_CREDIBLE_MAX_QUERIES})")
    gf, level, offset = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, "grid_pose_credible")
    B = gf.B
    gt = None
    if gt_rotation is not None:
        gt = gt_rotation.reshape(B, -1, 3, 3).to(device=gf.dev, dtype=torch.float32).contiguous()
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        Q = grid.shape[0]
        gt_log_prob = None
        if gt is not None:
            # The images at their ground truths: shared rows through run_log_prob, each image's K padded with its first one to GRID_GT_ROW
            # rotations -- rows that long run on the kernels the grid's rows run on (csrc/flow_plan.h), so a ground truth that is a grid row
            # gets that row's log p bit for bit.  Launches hold the rows the grid's launches may; batch-coupled flows take one image per
            # launch, as their grids do (their matrices then come from the ground truths: see the docstring).
            K = gt.shape[1]
            step = 1 if gf.coupled else max(1, gf.budget // GRID_GT_ROW)
            pad = torch.cat([gt, gt[:, :1].expand(-1, GRID_GT_ROW - K, -1, -1)], dim=1)
            parts = []
            for b0 in range(0, B, step):
                b1 = min(B, b0 + step)
                at = gf.log_prob(pad[b0:b1].reshape(-1, 3, 3), b0, b1, GRID_GT_ROW)
                parts.append(at.reshape(b1 - b0, GRID_GT_ROW)[:, :K].max(dim=1).values)
            gt_log_prob = parts[0] if len(parts) == 1 else torch.cat(parts)
        outs = []
        for b0, b1, lp in gf.images(grid, images_per_launch, "grid_pose_credible"):
            outs.append(grid_credible(lp, lv, gt_log_prob[b0:b1, None] if gt is not None else None)[:5])
        threshold, count, mass, log_norm, gt_level = (torch.cat(t) if t[0] is not None else None for t in zip(*outs))
    volume = torch.where(count < 0, float("nan"), count.to(torch.float32) / Q)
    out = dict(threshold=threshold, count=count, volume=volume, mass=mass, log_norm=log_norm, offset=offset)
    if gt is not None:
        out.update(gt_log_prob=gt_log_prob, gt_level=gt_level[:, 0], gt_inside=gt_log_prob[:, None] >= threshold)
    return out


GRID_FIT_MAX_ROWS = 1 << 26                        # rnf_grid_fit's and the histogram's limit (include/rnf_hip.h): level 6 fits


def grid_fit(logp: torch.Tensor, counts: torch.Tensor) -> dict:
    """``rnf_grid_fit`` on g images: how well the histogram ``counts`` [g,Q] (int32, ``sd.grid_histogram``) of n samples fits the density
    ``logp`` [g,Q] (float32) on the same grid, both on the device (include/rnf_hip.h).  With p_i = softmax(logp)_i, the density at cell
    i's grid rotation normalised over the grid -- a midpoint value of the density, not the cell's exact mass:
    ``log_norm`` = log(sum_i exp(lp_i) / Q); ``log_likelihood`` = the mean log p at the grid rotations of the samples' cells;
    ``grid_log_likelihood`` = log_likelihood - log_norm, the mean of log(p_i Q) (IPDF's metric); ``g_stat`` = 2 sum c_i log(c_i / (n p_i))
    and ``chi2`` = sum (c_i - n p_i)^2 / (n p_i); ``n``, ``occupied`` (cells with a sample; both int64, exact); ``kl`` = g_stat / (2 n),
    the KL divergence from the empirical histogram to the grid density in nats (its sampling floor is (Q - 1) / (2 n)); ``dof`` = Q - 1 and
    ``z`` = (g_stat - dof) / sqrt(2 dof).  ``z`` reads as a standard normal under "the samples come from p" only when the chi-square
    limit holds, i.e. with n / Q of a few or more samples per cell, and only as far as the midpoint values stand for the cells' masses.
    Deterministic: bit-identical from run to run and whatever g.
    -> dict(log_norm, log_likelihood, grid_log_likelihood, g_stat, chi2, kl, z: float64 [g]; n, occupied: int64 [g]; dof: int)"""
    if logp.dim() != 2 or counts.dim() != 2 or logp.shape != counts.shape:
        raise ValueError(f"grid_fit: logp {tuple(logp.shape)} and counts {tuple(counts.shape)} (want [g,Q] both)")
    g, Q = logp.shape
    if not 1 <= Q <= GRID_FIT_MAX_ROWS:
        raise ValueError(f"grid_fit: {Q} grid rows (1 to 2^26)")
    if not 1 <= g <= 65535:
        raise ValueError(f"grid_fit: {g} images (1 to 65535)")
    if counts.dtype != torch.int32:
        raise ValueError(f"grid_fit: counts of dtype {counts.dtype} (want int32, as grid_histogram returns)")
    if not logp.is_cuda or not counts.is_cuda:
        raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    dev = logp.device
    lp = logp.detach().to(torch.float32).contiguous()
    cn = counts.to(dev).contiguous()
    stats = torch.empty(g, len(_lib.GRID_FIT_STATS), dtype=torch.float64, device=dev)
    _lib.call("grid_fit", _lib.GridFit(logp=lp.data_ptr(), counts=cn.data_ptr(), Q=Q, g=g, stats_out=stats.data_ptr()), dev)
    out = {name: stats[:, i] for i, name in enumerate(_lib.GRID_FIT_STATS)}
    n = out["n"]
    out["kl"] = out["g_stat"] / (2.0 * n)
    out["dof"] = Q - 1
    out["z"] = (out["g_stat"] - (Q - 1)) / float(np.sqrt(2.0 * (Q - 1))) if Q > 1 else torch.full_like(n, float("nan"))
    out["n"], out["occupied"] = n.to(torch.int64), out["occupied"].to(torch.int64)
    return out


GRID_SAMPLE_MAX_ROWS = 1 << 26                     # rnf_grid_sample's limits (include/rnf_hip.h): level 6 fits; draws per image
GRID_SAMPLE_MAX_DRAWS = 1 << 30
GRID_SAMPLE_MAX_LEVEL = 6


def _sample_seed(seed) -> int:
    """The Philox key: ``seed``, or one drawn from torch's default generator (``MatrixFisherN._sample``'s rule), so that
    ``torch.manual_seed`` reproduces the draws."""
    if seed is None:
        return int(torch.randint(0, 2 ** 62, (1,)).item())
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"grid_sample: seed={seed} outside 0..2^64-1")
    return seed


def _sample_options(n, recursion_level, method, who: str):
    """Argument checks shared by ``grid_sample`` and ``grid_pose_sample`` -> (n, level or -1, the method's number)."""
    n = int(n)
    if not 1 <= n <= GRID_SAMPLE_MAX_DRAWS:
        raise ValueError(f"{who}: n={n} draws per image (1 to 2^30)")
    if method not in _lib.GRID_SAMPLE_METHODS:
        raise ValueError(f"{who}: method must be 'systematic' or 'multinomial', got {method!r}")
    level = -1 if recursion_level is None else int(recursion_level)
    if recursion_level is not None and not 0 <= level <= GRID_SAMPLE_MAX_LEVEL:
        raise ValueError(f"{who}: recursion_level={recursion_level} outside 0..{GRID_SAMPLE_MAX_LEVEL} (at most 2^26 grid rows)")
    return n, level, _lib.GRID_SAMPLE_METHODS[method]


def _grid_sample(lp, n, level, method, jitter, off, seed, image_base):
    """``rnf_grid_sample`` on the checked arguments: lp float32 [g,Q] contiguous on the device, off [9] or None."""
    g, Q = lp.shape
    dev = lp.device
    index = torch.empty(g, n, dtype=torch.int64, device=dev)
    target = torch.empty(g, n, dtype=torch.int64, device=dev)      # uint64 values below 2^62: the same bits as int64
    total = torch.empty(g, dtype=torch.int64, device=dev)
    rot = torch.empty(g, n, 3, 3, dtype=torch.float32, device=dev) if level >= 0 else None
    args = _lib.GridSample(logp=lp.data_ptr(), Q=Q, g=g, level=level, draws=n, draw_base=0, draws_total=n, image_base=image_base, method=method,
                           jitter=1 if jitter else 0, seed=seed, offset=off.data_ptr() if off is not None else None,
                           index_out=index.data_ptr(), target_out=target.data_ptr(), total_out=total.data_ptr(),
                           rot_out=rot.data_ptr() if rot is not None else None)
    _lib.call("grid_sample", args, dev)
    # log(sum exp(lp) / Q) from the sum the draws were made from, T = sum rint(exp(lp - m) 2^S): within 2^-23 + Q / T of the real one, and
    # no fp64 copy of the rows
    S = 62 - max(Q - 1, 0).bit_length()
    log_norm = lp.max(dim=1).values.to(torch.float64) + torch.log(total.to(torch.float64)) - (S * float(np.log(2.0)) + float(np.log(Q)))
    picked = lp.gather(1, index.clamp(min=0)).to(torch.float64) - log_norm[:, None]
    log_prob = torch.where(index >= 0, picked, torch.full_like(picked, float("nan"))).to(torch.float32)
    return dict(index=index, rotations=rot, log_prob=log_prob, target=target)


def grid_sample(logp: torch.Tensor, n: int, recursion_level: int = None, method: str = "systematic", jitter: bool = True, offset=None,
                seed: int = None) -> dict:
    """``rnf_grid_sample``: ``n`` draws per image from the posteriors ``logp`` [g,Q] (float32, any normalisation, on the device) on grid
    rows -- a filtered, diffused, tempered or multiplied posterior as well as a flow's.  Row i is drawn with probability
    softmax(logp)_i (in 62-bit fixed point: the masses of ``grid_credible``; a row at -inf, or more than about 26 nats below the
    maximum at level 6, is never drawn).  ``method``: 'multinomial', independent draws, or 'systematic', one random offset and n evenly
    spaced targets -- every row is drawn floor(n p_i) or ceil(n p_i) times and the draws come in ascending row order (shuffle them if the
    order matters).  With ``recursion_level`` (0..6, Q = 72 * 8^level, the grid of ``offset``) the draws are rotations: ``jitter`` places
    each uniformly (Haar) inside its drawn cell (``sd.grid_cell_points``), so they follow the piecewise-constant density and
    ``sd.grid_index`` gives the drawn row back; without it they are the grid's own rows, bit for bit.  ``recursion_level`` None: any
    Q <= 2^26, rows only.  ``seed`` None: the key comes from torch's default generator, so ``torch.manual_seed`` reproduces the draws;
    draw k of image b depends on (seed, k, b) alone.  An image with a NaN, a +inf or no finite value has index -1 and NaN elsewhere.
    -> dict(index int64 [g,n], rotations float32 [g,n,3,3] or None, log_prob float32 [g,n] = logp[index] - log(sum exp(logp) / Q), the
    piecewise-constant posterior's density at the draw in the measure of ``logp``, target int64 [g,n] the integers that were inverted)"""
    who = "grid_sample"
    if not isinstance(logp, torch.Tensor) or logp.dim() != 2:
        raise ValueError(f"{who}: logp {tuple(getattr(logp, 'shape', ()))} (want [g,Q])")
    n, level, method = _sample_options(n, recursion_level, method, who)
    g, Q = logp.shape
    if not 1 <= Q <= GRID_SAMPLE_MAX_ROWS:
        raise ValueError(f"{who}: {Q} grid rows (1 to 2^26)")
    if not 1 <= g <= 65535:
        raise ValueError(f"{who}: {g} images (1 to 65535)")
    if level >= 0 and Q != sd.grid_size(level):
        raise ValueError(f"{who}: {Q} rows are not the {sd.grid_size(level)} of level {level}")
    if offset is not None and (level < 0 or offset.numel() != 9):
        raise ValueError(f"{who}: offset of shape {tuple(offset.shape)} (want [3, 3], with a recursion_level)")
    if seed is not None:
        seed = _sample_seed(seed)
    if not logp.is_cuda:
        raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    seed = _sample_seed(seed)
    lp = logp.detach().to(torch.float32).contiguous()
    off = offset.detach().reshape(9).to(device=lp.device, dtype=torch.float32).contiguous() if offset is not None else None
    return _grid_sample(lp, n, level, method, jitter, off, seed, 0)


def grid_pose_sample(flow: Flow, feature: torch.Tensor = None, n: int = 1, recursion_level: int = 3, temperature: float = 1.0,
                     method: str = "systematic", jitter: bool = True, offset=None, base=None, images_per_launch: int = None,
                     seed: int = None) -> dict:
    """``grid_sample`` of the flow's density on the grid of ``grid_estimate_rotations`` (same inputs, same launches): ``n`` rotations per
    image from softmax(log p / ``temperature``) over the level's cells -- temperature 1 the flow's posterior as the grid sees it, above 1
    flatter, below 1 sharper (none of which ``flow.inverse`` can draw).  Image b of the batch is global image b of the stream, so the
    result equals ``grid_sample`` of the materialised rows whatever ``images_per_launch``.  Flows with batch-coupled layers are refused.
    -> ``grid_sample``'s dict (every entry [B,n,...]; ``log_prob`` is of the tempered rows) plus offset [3,3]"""
    who = "grid_pose_sample"
    n, level, method = _sample_options(n, recursion_level, method, who)
    if level < 0:
        raise ValueError(f"{who}: recursion_level is required (0..{GRID_SAMPLE_MAX_LEVEL})")
    temperature = float(temperature)
    if not 0.0 < temperature < float("inf"):
        raise ValueError(f"{who}: temperature={temperature} (a positive number)")
    _refuse_batch_coupled(flow, who, ", so an image's density would depend on the launch")
    gf, level, offset = _grid_inputs(flow, feature, None, level, offset, base, who)
    seed = _sample_seed(seed)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        off = offset.reshape(9).contiguous()
        parts = []
        for b0, b1, lp in gf.images(grid, images_per_launch, who):
            if b1 - b0 > 65535:
                raise ValueError(f"{who}: {b1 - b0} images in one launch (at most 65535)")
            parts.append(_grid_sample((lp / temperature).contiguous(), n, level, method, jitter, off, seed, b0))
    out = parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    out["offset"] = offset
    return out


def grid_diffuse(logp: torch.Tensor, grid: torch.Tensor, kappa: float) -> torch.Tensor:
    """The prediction step of a Bayes filter on the SO(3) grid: each image's grid posterior diffused by an isotropic matrix-Fisher motion
    kernel of concentration ``kappa`` (0..1e6).  ``logp`` [B,Q] log-densities on the rows of ``grid`` [Q,3,3] (any normalisation), both
    on the device.  With p_b = softmax(logp_b), k the kernel of ``utils.kde.so3_kernel_log_density`` and Z_j = (1/Q) sum_i k(R_j, R_i),
        out[b][i] = log sum_j p_bj k(R_j, R_i) / Z_j:
    dividing by Z_j makes the operator a Markov kernel ON THE GRID, so that sum_i exp(out[b][i]) / Q = 1 whatever kappa -- a kernel
    sharper than a cell would otherwise leak or gain mass (1.69 at level 2 with kappa = 64).  Two calls of the pairwise kernel sum:
    log Z, then the sum with the log-weights log p_b - log Z_j (whose softmax normaliser is added back).  kappa -> infinity returns
    log_softmax(logp) + log Q; the cost is Q^2 pairs per image, meant for levels <= 3.
    -> float32 [B,Q], a log-density w.r.t. Haar on the grid rows, ready for grid_modes, grid_credible and the others."""
    from .utils.kde import so3_kernel_log_density
    if not isinstance(logp, torch.Tensor) or logp.dim() != 2:
        raise ValueError(f"grid_diffuse: logp {tuple(getattr(logp, 'shape', ()))} (want [B,Q])")
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3 or tuple(grid.shape) != (logp.shape[1], 3, 3):
        raise ValueError(f"grid_diffuse: grid {tuple(getattr(grid, 'shape', ()))} for logp {tuple(logp.shape)} (want [Q,3,3])")
    if not 1 <= logp.shape[0] <= 65535:
        raise ValueError(f"grid_diffuse: logp holds {logp.shape[0]} images (1 to 65535)")
    if not logp.is_cuda or not grid.is_cuda:
        raise ValueError("grid_diffuse: logp and grid must be on the GPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    kappa = float(kappa)
    lz = so3_kernel_log_density(grid, grid, kappa)                                         # [Q]: log Z_j (k is symmetric)
    # log(p_bj / Z_j), formed in fp64 and rounded once: these are the numbers the second call sees
    lw = (torch.log_softmax(logp.detach().to(torch.float64), dim=1) - lz.to(torch.float64)).to(torch.float32)
    out = so3_kernel_log_density(grid, grid, kappa, log_weights=lw)                        # weights softmax(lw): normalised to 1 ..
    return (out.to(torch.float64) + torch.logsumexp(lw.to(torch.float64), dim=1, keepdim=True)).to(torch.float32)   # .. so their normaliser comes back


def _local_args(logp, grid, who: str, name: str = "logp"):
    if not isinstance(logp, torch.Tensor) or logp.dim() != 2:
        raise ValueError(f"{who}: {name} {tuple(getattr(logp, 'shape', ()))} (want [B,Q])")
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3 or tuple(grid.shape) != (logp.shape[1], 3, 3):
        raise ValueError(f"{who}: grid {tuple(getattr(grid, 'shape', ()))} for {name} {tuple(logp.shape)} (want [Q,3,3])")
    if logp.shape[0] < 1:
        raise ValueError(f"{who}: {name} holds no image")
    if not logp.is_cuda or not grid.is_cuda:
        raise ValueError(f"{who}: {name} and grid must be on the GPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")


def _right_multiply(x: torch.Tensor, D) -> torch.Tensor:
    """x [...,3,3] @ D for a host matrix D [3,3] in x's precision, from Python scalars: no host-to-device copy, so it can be captured"""
    return torch.stack([x[..., 0] * float(D[0, c]) + x[..., 1] * float(D[1, c]) + x[..., 2] * float(D[2, c]) for c in range(3)], dim=-1)


def _isotropic(A):
    """kappa where the host matrix A [3,3] is exactly kappa I with kappa >= 0 (the isotropic model, no drift), else None"""
    k = float(A[0, 0])
    return k if k >= 0.0 and np.array_equal(A, k * np.eye(3)) else None


DRIFT_RESOLUTION = 1e-7                             # a drift closer to the identity than fp32 resolves in a rotation's entries is none


def _motion_cut(A, level, radius_deg, who):
    """The host side of one motion matrix, from the arguments alone (no device work): -> (drift, K, whether the fp32 drift differs from
    the identity, the cut).  Refuses what the entry point would refuse of K, and an explicit radius under the floor of a drifting model."""
    from .utils import kde
    drift, K, sv = kde.motion_factors(A)
    kde._concentration(K, who)
    drifting = bool(np.abs(drift - np.eye(3)).max() > DRIFT_RESOLUTION)
    if radius_deg is None:
        return drift, K, drifting, kde.local_default_d2_cut_fisher(sv, level, drifting)
    cut = kde.local_radius_to_d2_cut(radius_deg)
    if drifting and cut < kde.local_floor_d2_cut(level):
        raise ValueError(f"{who}: radius_deg={radius_deg} is below {kde.LOCAL_FLOOR_SPACINGS} grid spacings of level {level} "
                         f"({kde.LOCAL_FLOOR_SPACINGS * 360.0 / (6 * 2 ** int(level)):.3f} degrees): a drifted row may find no neighbour")
    return drift, K, drifting, cut


class _MotionStep:
    """One matrix-Fisher motion model A = Delta K on one grid: the shifted rows C = grid Delta in fp32, formed once,
    their offset O Delta, the cut, and the four passes.  ``rows`` is ``grid`` itself where the fp32 drift is the identity."""

    def __init__(self, A, grid, level, radius_deg, offset, who):
        self.A = A
        drift, self.K, self.drifting, self.cut = _motion_cut(A, level, radius_deg, who)
        self.level, self.grid = int(level), grid
        self.offset = offset
        self.rows, self.rows_offset = grid, offset
        if self.drifting:
            g32 = grid.detach().to(torch.float32)
            self.rows = _right_multiply(g32, drift).contiguous()
            off = torch.eye(3, dtype=torch.float64, device=grid.device) if offset is None else offset.detach().to(
                device=grid.device, dtype=torch.float64).reshape(3, 3)
            self.rows_offset = _right_multiply(off, drift).to(torch.float32)
        self._lzq = None

    def _queries(self, side):
        return None if not self.drifting else side

    def log_zq(self):
        """log Z_j + log Q, float64 [Q]: rows G, queries C_j; -inf where the neighbourhood of C_j is empty"""
        from .utils.kde import so3_grid_local_log_sum
        if self._lzq is None:
            self._lzq = so3_grid_local_log_sum(self.grid, self.level, concentration=self.K, d2_cut=self.cut, queries=self._queries(self.rows),
                                               offset=self.offset).to(torch.float64)
        return self._lzq

    def minus_log_z(self, x64, log_q: float):
        """x - log Z_j in fp64 rounded once; -inf where Z_j = 0: such a source row's mass is dropped"""
        lzq = self.log_zq()
        return torch.where(torch.isneginf(lzq), torch.full_like(x64, -float("inf")), x64 - (lzq - log_q)).to(torch.float32)

    def predict(self, lw):
        """log sum_j exp(lw_j) k(C_j, G_i): rows C (offset O Delta), queries G"""
        from .utils.kde import so3_grid_local_log_sum
        return so3_grid_local_log_sum(self.rows, self.level, concentration=self.K, d2_cut=self.cut, queries=self._queries(self.grid),
                                      log_weights=lw, offset=self.rows_offset)

    def best(self, lw):
        """max_j and arg max_j of lw_j + log k(C_j, G_i): the max-plus pass in the predict orientation; arg is the source row j"""
        from .utils.kde import so3_grid_local_log_max
        return so3_grid_local_log_max(self.rows, self.level, concentration=self.K, d2_cut=self.cut, queries=self._queries(self.grid),
                                      log_weights=lw, offset=self.rows_offset)

    def backward(self, lw):
        """log sum_i exp(lw_i) k(C_j, G_i): rows G (offset O), queries C"""
        from .utils.kde import so3_grid_local_log_sum
        return so3_grid_local_log_sum(self.grid, self.level, concentration=self.K, d2_cut=self.cut, queries=self._queries(self.rows),
                                      log_weights=lw, offset=self.offset)


class _Motions:
    """The motion models of one call: one matrix, or one per step; a step whose matrix equals the one built last reuses it (its rows C
    and its Z).  Only the last one built is kept."""

    def __init__(self, A, steps, grid, level, radius_deg, offset, who, built=None):
        self.A, self.args, self.last, self.last_A = A, (grid, level, radius_deg, offset, who), built, None if built is None else built.A

    def step(self, t):
        """the model of the step t -> t + 1 (t = 0: also the one a ``log_prior`` is taken through)"""
        a = self.A if self.A.ndim == 2 else self.A[t]
        if self.last is None or not np.array_equal(a, self.last_A):
            self.last, self.last_A = _MotionStep(a, *self.args), a
        return self.last


def _motion_host(kappa, motion, steps, level, radius_deg, who):
    """The checks of ``kappa`` / ``motion`` that need no device, first in every function that takes them: exactly one of the two; the
    shape ([3,3]; with ``steps`` not None also [steps,3,3], one matrix per step); finite entries; each matrix's concentration and, for an
    explicit radius, the floor.  -> (kappa, None) on the isotropic path (``motion`` exactly kappa I in every step IS that path: the same
    bits), else (None, A float64 numpy) -- or the _MotionStep / _Motions a caller hands down."""
    if (kappa is None) == (motion is None):
        raise ValueError(f"{who}: give exactly one of kappa and motion")
    if motion is None or isinstance(motion, (_MotionStep, _Motions)):
        return kappa, motion
    if isinstance(motion, torch.Tensor):
        motion = motion.detach().cpu().to(torch.float64).numpy()               # a GPU tensor is read back
    A = np.asarray(motion, dtype=np.float64)
    if A.shape != (3, 3) and (steps is None or A.shape != (steps, 3, 3)):
        want = "[3,3]" if steps is None else f"[3,3] or [{steps},3,3] (one matrix per step)"
        raise ValueError(f"{who}: motion {tuple(A.shape)}, expected {want}")
    if not np.isfinite(A).all():
        raise ValueError(f"{who}: motion holds a non-finite entry")
    flat = A.reshape(-1, 3, 3)
    if len(flat) and all(np.array_equal(a, flat[0]) for a in flat) and _isotropic(flat[0]) is not None:
        return _isotropic(flat[0]), None
    for t, a in enumerate(flat):
        if t == 0 or not np.array_equal(a, flat[t - 1]):
            _motion_cut(a, level, radius_deg, who)
    return None, A


def _motion_plan(A, grid, level, radius_deg, offset, who):
    """The device side of ``_motion_host``'s second result, once the other arguments are checked"""
    if A is None or isinstance(A, (_MotionStep, _Motions)):
        return A
    return _MotionStep(A, grid, level, radius_deg, offset, who) if A.ndim == 2 else _Motions(A, len(A), grid, level, radius_deg, offset, who)


def _steps_of(log_likelihood):
    """T - 1 of a [T,Q] or [B,T,Q] tensor (else 0: the shape is refused further on)"""
    ok = isinstance(log_likelihood, torch.Tensor) and log_likelihood.dim() in (2, 3)
    return max(int(log_likelihood.shape[-2]) - 1, 0) if ok else 0


def grid_diffuse_local(logp: torch.Tensor, grid: torch.Tensor, level: int, kappa: float = None, radius_deg: float = None, offset=None,
                       motion=None) -> torch.Tensor:
    """``grid_diffuse``'s operator on the TRUNCATED motion kernel, for the levels where Q^2 pairs cannot run: each image's grid posterior
    diffused by the isotropic matrix-Fisher kernel of concentration ``kappa`` cut off at ``radius_deg`` (default: where (kappa/2) d^2 = 18
    nats, capped at 180 degrees; ``utils.kde.so3_grid_local_log_sum``).  ``logp`` [B,Q] on the rows of ``grid`` [Q,3,3] =
    ``sd.generate_healpix_grid(level, offset=offset)``.  With N(j) the rows within the radius of row j, p_b = softmax(logp_b) and
    Z_j = (1/Q) sum_{i in N(j)} k(R_j, R_i),
        out[b][i] = log sum_{j in N(i)} p_bj k(R_j, R_i) / Z_j.
    The neighbourhoods are symmetric (membership is one bit-symmetric fp32 distance), so this is a Markov kernel on the grid:
    sum_i exp(out[b][i]) / Q = 1 whatever kappa and radius.  Two calls of the neighbour-limited sum: Z without weights, then the sum with
    the log-weights log_softmax(logp) - log Z, formed in fp64 and rounded once.  The cost is Q |N| terms per image, not Q^2.
    -> float32 [B,Q], a log-density w.r.t. Haar on the grid rows.  At radius 180 it is ``grid_diffuse`` (which stays the dense form).
    ``motion`` [3,3] in place of ``kappa`` (exactly one of the two): a general matrix-Fisher step x' = x E, E ~ MF(A), A = Delta K
    (``utils.kde.motion_factors``, ``utils.kde.motion_matrix``): the drift Delta shifts the source rows to C_j = R_j Delta (formed once in
    fp32; they are the grid of offset O Delta), the symmetric K is a per-axis concentration, and k(C_j, R_i) = exp(-1/2 tr((R_i - C_j) K
    (R_i - C_j)^T) - l(K)) (``rnf_so3_grid_local_fisher``).  N(j) is the ball of ``radius_deg`` about C_j -- by default where the loosest
    axis reaches 18 nats, and with a drift not below 1.25 grid spacings: a smaller explicit radius is refused -- Z_j sums over it, and
    the same stored C serves both orientations, so membership and term are bit-symmetric and the operator stays a Markov kernel.  A
    source row whose neighbourhood is nevertheless empty (Z_j = 0) gets the log-weight -inf: its mass is dropped.  ``motion`` = kappa I
    gives the bits of ``kappa``."""
    from .utils.kde import so3_grid_local_log_sum
    who = "grid_diffuse_local"
    kappa, mo = _motion_host(kappa, motion, None, level, radius_deg, who)
    _local_args(logp, grid, who)
    Q = grid.shape[0]
    mo = _motion_plan(mo, grid, level, radius_deg, offset, who)
    if mo is not None:
        return mo.predict(mo.minus_log_z(torch.log_softmax(logp.detach().to(torch.float64), dim=1), float(np.log(Q))))
    lz = so3_grid_local_log_sum(grid, level, kappa, radius_deg=radius_deg, offset=offset).to(torch.float64) - float(np.log(Q))   # log Z_j
    lw = (torch.log_softmax(logp.detach().to(torch.float64), dim=1) - lz).to(torch.float32)
    return so3_grid_local_log_sum(grid, level, kappa, radius_deg=radius_deg, log_weights=lw, offset=offset)


def grid_filter_step(log_prior: torch.Tensor, log_likelihood: torch.Tensor, grid: torch.Tensor, level: int, kappa: float = None,
                     radius_deg: float = None, offset=None, motion=None) -> dict:
    """One step of a Bayes filter on the SO(3) grid: predict with ``grid_diffuse_local`` (motion kernel ``kappa``, ``radius_deg``), multiply
    by the likelihood, normalise.  ``log_prior`` [B,Q] (any normalisation) and ``log_likelihood`` [B,Q] (log of the observation's density
    at each grid rotation) on the rows of ``grid`` [Q,3,3] of ``level`` and ``offset``.
    -> dict(posterior [B,Q] float32 with sum_i exp(posterior) / Q = 1, log_evidence [B] float64 = log (1/Q) sum_i predicted_i
    likelihood_i, the log predictive density of the observation, predicted [B,Q] float32, the diffused prior).  The product and its
    normaliser are formed in fp64 and rounded once.  ``motion`` [3,3] in place of ``kappa``: the drifting, anisotropic model of
    ``grid_diffuse_local``."""
    who = "grid_filter_step"
    kappa, motion = _motion_host(kappa, motion, None, level, radius_deg, who)
    if not isinstance(log_likelihood, torch.Tensor) or tuple(log_likelihood.shape) != tuple(getattr(log_prior, "shape", ())):
        raise ValueError(f"{who}: log_likelihood {tuple(getattr(log_likelihood, 'shape', ()))} for log_prior "
                         f"{tuple(getattr(log_prior, 'shape', ()))} (want the same shape)")
    _local_args(log_prior, grid, who, "log_prior")
    if not log_likelihood.is_cuda:
        raise ValueError(f"{who}: log_likelihood must be on the GPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    predicted = grid_diffuse_local(log_prior, grid, level, kappa, radius_deg, offset, _motion_plan(motion, grid, level, radius_deg, offset, who))
    joint = predicted.to(torch.float64) + log_likelihood.detach().to(torch.float64)
    log_evidence = torch.logsumexp(joint, dim=1) - float(np.log(grid.shape[0]))
    return dict(posterior=(joint - log_evidence[:, None]).to(torch.float32), log_evidence=log_evidence, predicted=predicted)


def grid_pose_filter(flow: Flow, features: torch.Tensor = None, kappa: float = None, recursion_level: int = 4, radius_deg: float = None, offset=None,
                     base=None, images_per_launch: int = None, log_prior: torch.Tensor = None, motion=None) -> dict:
    """A Bayes filter over a SEQUENCE of frames of one object: ``features`` [T,F], one row per frame (for an unconditional flow, the T rows
    of ``base``).  Each frame's log-density on the level-``recursion_level`` grid -- the launches of ``grid_estimate_rotations`` -- is the
    frame's likelihood; between frames the posterior is diffused by the motion kernel ``kappa`` (``grid_filter_step``).  Frame 0 starts
    from ``log_prior`` [Q] (None: uniform, and no diffusion before it: its posterior is its normalised likelihood, its estimate that of
    ``grid_estimate_rotations``).  ``offset`` as ``grid_estimate_rotations``.  Flows with batch-coupled layers are refused.
    -> dict(est [T,3,3] the posterior's arg-max rotation per frame, index [T], log_evidence [T] float64 (the log predictive density of
    each frame given the earlier ones), posterior [Q] float32 after the last frame (sum exp / Q = 1), grid [Q,3,3], offset [3,3]).
    ``motion`` in place of ``kappa`` (exactly one of the two): one matrix [3,3] (``grid_diffuse_local``), or [T-1,3,3], one per frame
    after the first -- the step into frame t uses ``motion[t-1]``; a ``log_prior`` is taken through ``motion[0]``."""
    who = "grid_pose_filter"
    if kappa is None and motion is None:
        raise ValueError(f"{who}: kappa is required")
    if kappa is not None and motion is not None:
        raise ValueError(f"{who}: give exactly one of kappa and motion")
    _refuse_batch_coupled(flow, who, ", so a frame's likelihood would depend on the frames that share its launch")
    gf, level, offset = _grid_inputs(flow, features, None, recursion_level, offset, base, who)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        Q = grid.shape[0]
        kappa, mo = _motion_host(kappa, motion, gf.B - 1, level, radius_deg, who)
        mo = _motion_plan(mo, grid, level, radius_deg, offset, who)
        if isinstance(mo, _MotionStep):
            mo = _Motions(mo.A, 0, grid, level, radius_deg, offset, who, mo)
        if mo is not None and log_prior is not None and gf.B == 1 and mo.A.ndim == 3:
            raise ValueError(f"{who}: a log_prior is taken through motion[0], but motion holds no matrix")
        post = None
        if log_prior is not None:
            if not isinstance(log_prior, torch.Tensor) or tuple(log_prior.shape) != (Q,):
                raise ValueError(f"{who}: log_prior {tuple(getattr(log_prior, 'shape', ()))}, expected [{Q}]")
            post = log_prior.detach().to(device=gf.dev, dtype=torch.float32)[None]
        indices, evidences = [], []
        for b0, b1, lp in gf.images(grid, images_per_launch, who):
            for k in range(b1 - b0):
                ll = lp[k:k + 1]
                if post is None:                                            # a uniform prior: nothing to diffuse
                    ll64 = ll.to(torch.float64)
                    ev = torch.logsumexp(ll64, dim=1) - float(np.log(Q))
                    post = (ll64 - ev[:, None]).to(torch.float32)
                else:
                    step = grid_filter_step(post, ll, grid, level, kappa, radius_deg, offset,
                                            None if mo is None else mo.step(max(b0 + k - 1, 0)))
                    post, ev = step["posterior"], step["log_evidence"]
                indices.append(torch.argmax(post[0]).reshape(1))
                evidences.append(ev)
        index = torch.cat(indices)
    return dict(est=grid[index], index=index, log_evidence=torch.cat(evidences), posterior=post[0], grid=grid, offset=offset)


def _sequence_args(log_likelihood, grid, level, log_prior, who: str):
    """-> (log-likelihoods [B,T,Q] float32, whether the caller gave the B axis, log_prior [B,Q] float32 or None)"""
    ll = log_likelihood
    if not isinstance(ll, torch.Tensor) or ll.dim() not in (2, 3):
        raise ValueError(f"{who}: log_likelihood {tuple(getattr(ll, 'shape', ()))} (want [T,Q] or [B,T,Q])")
    batched = ll.dim() == 3
    ll = ll if batched else ll[None]
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3 or tuple(grid.shape) != (ll.shape[2], 3, 3):
        raise ValueError(f"{who}: grid {tuple(getattr(grid, 'shape', ()))} for log_likelihood {tuple(log_likelihood.shape)} (want [Q,3,3])")
    if grid.shape[0] != 72 * 8 ** int(level):
        raise ValueError(f"{who}: grid holds {grid.shape[0]} rows, level {level} has {72 * 8 ** int(level)}")
    B, T, Q = ll.shape
    if T < 1 or not 1 <= B <= 65535:
        raise ValueError(f"{who}: log_likelihood holds {B} sequences of {T} frames (1 to 65535 sequences, at least one frame)")
    if not ll.is_cuda or not grid.is_cuda:
        raise ValueError(f"{who}: log_likelihood and grid must be on the GPU; rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    prior = None
    if log_prior is not None:
        if not isinstance(log_prior, torch.Tensor) or tuple(log_prior.shape) not in ((Q,), (B, Q)):
            raise ValueError(f"{who}: log_prior {tuple(getattr(log_prior, 'shape', ()))}, expected [{Q}] or [{B},{Q}]")
        prior = log_prior.detach().to(device=ll.device, dtype=torch.float32).reshape(-1, Q).expand(B, Q).contiguous()
    return ll.detach().to(torch.float32), batched, prior


def _recentre(delta):
    """delta [B,Q] float64 -> (delta - its row maximum as float32, the maxima [B] float64; 0 where a row holds no finite number)"""
    top = delta.max(dim=1).values
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    return (delta - top[:, None]).to(torch.float32), top


def grid_viterbi(log_likelihood: torch.Tensor, grid: torch.Tensor, level: int, kappa: float = None, radius_deg: float = None, offset=None,
                 log_prior: torch.Tensor = None, motion=None) -> dict:
    """The most probable JOINT sequence of grid rows under the model ``grid_pose_filter`` implies (Viterbi): per-frame arg-maxes are not
    a path -- on a symmetric object they hop between equivalent modes -- this is one.  ``log_likelihood`` [T,Q] or [B,T,Q]: each frame's
    log-likelihood on the rows of ``grid`` [Q,3,3] of ``level`` and ``offset``.  The model: a step j -> i has the mass
    k(R_j, R_i) / (Z_j Q) on the neighbourhood N(j) of ``grid_diffuse_local`` (``kappa``, ``radius_deg``, its per-row Z_j); the initial
    density pi_0 is uniform (``log_prior`` None) or ``grid_diffuse_local(log_prior)`` ([Q] or [B,Q]), the filter's predicted density of
    frame 0; p(x, y) = pi_0(x_0)/Q  prod_t k(x_{t-1}, x_t) / (Z Q)  prod_t l_t(x_t).  The recursion
        delta_0(i) = log pi_0(i) - log Q + l_0(i),    delta_t(i) = l_t(i) + max_{j in N(i)} [delta_{t-1}(j) - log Z_j + log k(R_j, R_i)] - log Q
    runs on the max-plus pass ``utils.kde.so3_grid_local_log_max`` with the B sequences as its groups (neighbourhoods are symmetric, so
    the backward operator is the forward one).  Its log-weights delta - log Z are formed in fp64 and rounded once; delta is re-centred on
    its maximum every frame and the offsets are summed in fp64.  Ties go to the smallest row.  The back-pointers are kept as int32
    [T,B,Q] -- 4 T B Q bytes, 9.4 MB per frame and sequence at level 5 -- and followed by T device-side gathers: no host synchronisation.
    -> dict(index [B,T] int64 the path's rows, est [B,T,3,3] its rotations, log_joint [B] float64 = log p(path, y)); without the B
    axis where ``log_likelihood`` came without it.  T = 1 gives the arg-max of pi_0 l_0.
    ``motion`` in place of ``kappa`` (exactly one of the two): one matrix [3,3] (``grid_diffuse_local``) or [T-1,3,3], the step t-1 -> t
    using ``motion[t-1]`` (a ``log_prior`` is taken through ``motion[0]``).  The step j -> i then has the mass k(C_j, R_i) / (Z_j Q) with the
    shifted rows C_j = R_j Delta, the max-plus pass runs over the rows C with the grid rows as queries, and its arg is the source row j."""
    from .utils.kde import so3_grid_local_log_max, so3_grid_local_log_sum
    who = "grid_viterbi"
    kappa, mo = _motion_host(kappa, motion, _steps_of(log_likelihood), level, radius_deg, who)
    ll, batched, prior = _sequence_args(log_likelihood, grid, level, log_prior, who)
    B, T, Q = ll.shape
    log_q = float(np.log(Q))
    mo = _motion_plan(mo, grid, level, radius_deg, offset, who)
    if isinstance(mo, _MotionStep):
        mo = _Motions(mo.A, 0, grid, level, radius_deg, offset, who, mo)
    if mo is not None and prior is not None and T == 1 and mo.A.ndim == 3:
        raise ValueError(f"{who}: a log_prior is taken through motion[0], but motion holds no matrix")
    with torch.no_grad():
        delta = ll[:, 0].to(torch.float64) - log_q
        if prior is not None:
            delta = delta + grid_diffuse_local(prior, grid, level, kappa, radius_deg, offset, None if mo is None else mo.step(0)).to(torch.float64)
        delta, log_joint = _recentre(delta)
        back = torch.empty(T, B, Q, dtype=torch.int32, device=ll.device)
        if T > 1 and mo is None:
            lz = so3_grid_local_log_sum(grid, level, kappa, radius_deg=radius_deg, offset=offset).to(torch.float64) - log_q    # log Z_j
        for t in range(1, T):
            if mo is not None:
                step = mo.step(t - 1)
                best, arg = step.best(step.minus_log_z(delta.to(torch.float64), log_q))
            else:
                lw = (delta.to(torch.float64) - lz).to(torch.float32)
                best, arg = so3_grid_local_log_max(grid, level, kappa, radius_deg=radius_deg, log_weights=lw, offset=offset)
            back[t] = arg
            delta, top = _recentre(ll[:, t].to(torch.float64) + best.to(torch.float64) - log_q)
            log_joint = log_joint + top
        index = torch.empty(B, T, dtype=torch.int64, device=ll.device)
        index[:, T - 1] = torch.argmax(delta, dim=1)
        log_joint = log_joint + delta.max(dim=1).values.to(torch.float64)        # 0 after re-centring, -inf where no path has mass
        for t in range(T - 1, 0, -1):
            index[:, t - 1] = back[t].gather(1, index[:, t, None])[:, 0].to(torch.int64).clamp_min(0)    # -1: no predecessor with mass
        est = grid[index]
    if not batched:
        index, est, log_joint = index[0], est[0], log_joint[0]
    return dict(index=index, est=est, log_joint=log_joint)


def grid_smooth(log_likelihood: torch.Tensor, grid: torch.Tensor, level: int, kappa: float = None, radius_deg: float = None, offset=None,
                log_prior: torch.Tensor = None, motion=None) -> dict:
    """Fixed-interval smoothing on the SO(3) grid: every frame of a recorded sequence judged with all of it, p(x_t | y_0..T-1), by the
    forward-backward recursion on the model of ``grid_viterbi`` (same arguments).  Forward: the ``grid_filter_step`` chain itself, frame 0
    from ``log_prior`` (None: uniform, and as in ``grid_pose_filter`` nothing is diffused before it: its posterior is its normalised
    likelihood).  Backward, with b_{T-1} = 0 and the existing neighbour-limited sum (the neighbourhoods and the kernel are symmetric, so
    the backward operator is the forward one, scaled by the per-row Z_j of ``grid_diffuse_local``):
        b_t(j) = log sum_{i in N(j)} k(R_j, R_i) l_{t+1}(i) exp b_{t+1}(i) - log Z_j - log Q - log_evidence_{t+1},
    log-weights and result formed in fp64 and rounded once.  smoothed_t = filtered_t + b_t, renormalised in fp64 (the last frame, where
    b = 0 exactly, is the filtered one bit for bit).
    -> dict(smoothed [B,T,Q] and filtered [B,T,Q] float32 log-densities with sum exp / Q = 1, log_evidence [B,T] float64 as
    ``grid_filter_step``'s, backward [B,T,Q] float32 the b_t, index [B,T] and est [B,T,3,3] the smoothed arg-max); without the B axis
    where ``log_likelihood`` came without it.  Three [B,T,Q] float32 arrays are kept.
    ``motion`` in place of ``kappa`` (exactly one of the two): as in ``grid_viterbi``.  The backward step of t uses ``motion[t]``:
        b_t(j) = log sum_{i in N(j)} k(C_j, R_i) l_{t+1}(i) exp b_{t+1}(i) - log Z_j - log Q - log_evidence_{t+1},
    the sum over the grid rows with the shifted rows C as queries; a source row with Z_j = 0 has b = -inf.  A time-varying motion
    rebuilds each distinct matrix's rows and Z on the way back."""
    from .utils.kde import so3_grid_local_log_sum
    who = "grid_smooth"
    kappa, mo = _motion_host(kappa, motion, _steps_of(log_likelihood), level, radius_deg, who)
    ll, batched, prior = _sequence_args(log_likelihood, grid, level, log_prior, who)
    B, T, Q = ll.shape
    log_q = float(np.log(Q))
    mo = _motion_plan(mo, grid, level, radius_deg, offset, who)
    if isinstance(mo, _MotionStep):
        mo = _Motions(mo.A, 0, grid, level, radius_deg, offset, who, mo)
    if mo is not None and prior is not None and T == 1 and mo.A.ndim == 3:
        raise ValueError(f"{who}: a log_prior is taken through motion[0], but motion holds no matrix")
    with torch.no_grad():
        filtered = torch.empty(B, T, Q, dtype=torch.float32, device=ll.device)
        evidence = torch.empty(B, T, dtype=torch.float64, device=ll.device)
        post = prior
        for t in range(T):
            if post is None:                                                # a uniform prior: nothing to diffuse
                ll64 = ll[:, 0].to(torch.float64)
                ev = torch.logsumexp(ll64, dim=1) - log_q
                post = (ll64 - ev[:, None]).to(torch.float32)
            else:
                step = grid_filter_step(post, ll[:, t], grid, level, kappa, radius_deg, offset, None if mo is None else mo.step(max(t - 1, 0)))
                post, ev = step["posterior"], step["log_evidence"]
            filtered[:, t], evidence[:, t] = post, ev
        backward = torch.zeros(B, T, Q, dtype=torch.float32, device=ll.device)
        smoothed = torch.empty_like(filtered)
        smoothed[:, T - 1] = filtered[:, T - 1]
        if T > 1 and mo is None:
            lz = so3_grid_local_log_sum(grid, level, kappa, radius_deg=radius_deg, offset=offset).to(torch.float64)    # log Z_j + log Q
        for t in range(T - 2, -1, -1):
            lw = (ll[:, t + 1].to(torch.float64) + backward[:, t + 1].to(torch.float64)).to(torch.float32)
            if mo is not None:
                step = mo.step(t)
                s, lzq = step.backward(lw).to(torch.float64), step.log_zq()
                b = torch.where(torch.isneginf(lzq), torch.full_like(s, -float("inf")), s - lzq - evidence[:, t + 1, None])
                backward[:, t] = b.to(torch.float32)
            else:
                s = so3_grid_local_log_sum(grid, level, kappa, radius_deg=radius_deg, log_weights=lw, offset=offset)
                backward[:, t] = (s.to(torch.float64) - lz - evidence[:, t + 1, None]).to(torch.float32)
            both = filtered[:, t].to(torch.float64) + backward[:, t].to(torch.float64)
            smoothed[:, t] = (both - (torch.logsumexp(both, dim=1, keepdim=True) - log_q)).to(torch.float32)
        index = torch.argmax(smoothed, dim=2)
        est = grid[index]
    res = dict(smoothed=smoothed, filtered=filtered, log_evidence=evidence, backward=backward, index=index, est=est)
    return res if batched else {k: v[0] for k, v in res.items()}


def grid_pose_smooth(flow: Flow, features: torch.Tensor = None, kappa: float = None, recursion_level: int = 4, radius_deg: float = None, offset=None,
                     base=None, images_per_launch: int = None, log_prior: torch.Tensor = None, motion=None) -> dict:
    """``grid_pose_filter`` for a RECORDED sequence: the frames' grid log-densities -- collected on the launches of
    ``grid_estimate_rotations``, one row per frame of ``features`` [T,F] -- are judged together, by ``grid_smooth`` (each frame's marginal
    given the whole clip) and by ``grid_viterbi`` (the most probable joint path; on a symmetric object it stays on one branch where the
    per-frame arg-max hops).  Arguments as ``grid_pose_filter``; ``log_prior`` [Q] or None.  T Q floats are kept for the likelihoods, and
    what the two recursions keep.  Flows with batch-coupled layers are refused.
    -> dict(est_smoothed [T,3,3], index_smoothed [T], est_path [T,3,3], index_path [T], log_evidence [T] float64, log_joint float64 [],
    smoothed [T,Q], grid [Q,3,3], offset [3,3]).  ``motion`` in place of ``kappa``: [3,3] or [T-1,3,3], as in ``grid_pose_filter``."""
    who = "grid_pose_smooth"
    if kappa is None and motion is None:
        raise ValueError(f"{who}: kappa is required")
    if kappa is not None and motion is not None:
        raise ValueError(f"{who}: give exactly one of kappa and motion")
    _refuse_batch_coupled(flow, who, ", so a frame's likelihood would depend on the frames that share its launch")
    gf, level, offset = _grid_inputs(flow, features, None, recursion_level, offset, base, who)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        ll = torch.cat([lp.to(torch.float32).clone() for _, _, lp in gf.images(grid, images_per_launch, who)])
        kappa, mo = _motion_host(kappa, motion, ll.shape[0] - 1, level, radius_deg, who)
        mo = _motion_plan(mo, grid, level, radius_deg, offset, who)             # built once: both recursions share the rows C and Z
        if isinstance(mo, _MotionStep):
            mo = _Motions(mo.A, 0, grid, level, radius_deg, offset, who, mo)
        smooth = grid_smooth(ll, grid, level, kappa, radius_deg, offset, log_prior, mo)
        path = grid_viterbi(ll, grid, level, kappa, radius_deg, offset, log_prior, mo)
    return dict(est_smoothed=smooth["est"], index_smoothed=smooth["index"], est_path=path["est"], index_path=path["index"],
                log_evidence=smooth["log_evidence"], log_joint=path["log_joint"], smoothed=smooth["smoothed"], grid=grid, offset=offset)


SPECTRAL_TRUNCATION = 1e-2                        # the largest (2L+1) h_L the spectral passes accept


def _spectral_multiplier(kappa, t, lmax: int, who: str, required: bool = True):
    """-> (multipliers [L+1] float64 or None, truncation = (2L+1) h_L); raises where the kernel is too sharp for lmax"""
    from .utils import harmonics
    if kappa is not None and t is not None:
        raise ValueError(f"{who}: both kappa and t are given; pass one of the two")
    if kappa is None and t is None:
        if required:
            raise ValueError(f"{who}: one of kappa (matrix-Fisher kernel) and t (heat kernel) is required")
        return None, float(2 * lmax + 1)
    h = harmonics.fisher_multipliers(kappa, lmax) if kappa is not None else harmonics.heat_multipliers(t, lmax)
    truncation = float((2 * lmax + 1) * h[lmax])
    if truncation > SPECTRAL_TRUNCATION:
        what = f"kappa={float(kappa)}" if kappa is not None else f"t={float(t)}"
        raise ValueError(f"{who}: {what} is too sharp for lmax={lmax}: the first degree left out would still carry (2L+1) h_L = "
                         f"{truncation:.3g} > {SPECTRAL_TRUNCATION}; raise lmax, or use grid_diffuse_local, which is made for sharp kernels")
    return h, truncation


def _spectral_density(coeffs, grid, lmax: int, h, truncation: float) -> dict:
    from .utils import harmonics
    density = harmonics.so3_fourier_density(coeffs, grid, lmax, multiplier=h)
    tiny = float(np.finfo(np.float32).tiny)
    negative = density.to(torch.float64).clamp(max=0.0).sum(dim=1) / grid.shape[0]
    return dict(density=density, log_density=torch.log(density.clamp(min=tiny)), negative_mass=negative, truncation=truncation,
                coefficients=coeffs)


def _spectrum_of(coeffs, lmax: int) -> dict:
    from .utils import harmonics
    power = harmonics.power_spectrum(coeffs.to(torch.float64), lmax)
    collision = power.sum(dim=-1)
    return dict(coefficients=coeffs, power=power, collision=collision, tail=power[..., lmax] / collision)


def grid_spectrum(logp: torch.Tensor, grid: torch.Tensor, lmax: int = 8) -> dict:
    """The SO(3) Fourier coefficients of each image's grid posterior and their power per degree: a sharpness measure that does not
    depend on a resolution.  ``logp`` [B,Q] log-densities on the rows of ``grid`` [Q,3,3] (any normalisation); p_b = softmax(logp_b).
    -> dict(coefficients [B,C_L] float32 = F_b^l = sum_q p_bq D^l(R_q) (``utils.harmonics.so3_fourier``), power [B,lmax+1] float64 =
    (2l+1) |F^l|_F^2, collision [B] = sum_l power, which tends to the integral of p^2 (1 for the uniform density), tail [B] =
    power[lmax] / collision: a tail that is not small says that lmax is too low for this posterior).  The analysis is of the discrete
    measure on the grid rows, so it carries the grid's quadrature error."""
    from .utils import harmonics
    who = "grid_spectrum"
    _local_args(logp, grid, who)
    _error_args(logp, grid, who)
    return _spectrum_of(harmonics.so3_fourier(grid, lmax, log_weights=logp), lmax)


def grid_diffuse_spectral(logp: torch.Tensor, grid: torch.Tensor, kappa: float = None, t: float = None, lmax: int = 8) -> dict:
    """Each image's grid posterior convolved with a WIDE zonal kernel, in the harmonic domain: the isotropic matrix-Fisher kernel of
    concentration ``kappa`` (the kernel of ``grid_diffuse``) or the heat kernel at time ``t``, evaluated on the grid rows.  The
    counterpart of ``grid_diffuse_local``: a sharp kernel stays local, a wide one needs few degrees and costs Q C_L per image whatever
    its width.  ``logp`` [B,Q] on the rows of ``grid`` [Q,3,3]; p_b = softmax(logp_b), F_b = ``so3_fourier`` of it,
        density[b][i] = sum_l (2l+1) h_l <F_b^l, D^l(R_i)>.
    -> dict(density [B,Q] float32 relative to Haar (uniform = 1), log_density = log max(density, tiny), negative_mass [B] float64 =
    sum_q min(density, 0) / Q, truncation = (2L+1) h_L, coefficients [B,C_L] of the posterior).  Raises ValueError where the kernel is
    so sharp that ``truncation`` exceeds 1e-3: use ``grid_diffuse_local`` there.  Unlike ``grid_diffuse`` the operator is not
    renormalised on the grid: it differs from it by the grid's quadrature error plus the truncation.  ``log_density`` feeds
    ``grid_modes``, ``grid_credible``, ``grid_sample`` and ``grid_filter_step``."""
    from .utils import harmonics
    who = "grid_diffuse_spectral"
    _local_args(logp, grid, who)
    _error_args(logp, grid, who)
    lmax = harmonics._lmax(lmax, who)
    h, truncation = _spectral_multiplier(kappa, t, lmax, who)
    return _spectral_density(harmonics.so3_fourier(grid, lmax, log_weights=logp), grid, lmax, h, truncation)


def grid_compose(logp_a: torch.Tensor, logp_b: torch.Tensor, grid: torch.Tensor, lmax: int = 8, invert_a: bool = False,
                 smooth_kappa: float = None) -> dict:
    """The density of R_a R_b (``invert_a``: of R_a^T R_b, the relative rotation) for independent R_a ~ softmax(logp_a), R_b ~
    softmax(logp_b) on the rows of ``grid`` [Q,3,3], evaluated on the same rows: blocks F_a^l F_b^l (``utils.harmonics.compose``) in
    place of a Q^2 gather.  ``logp_a``, ``logp_b`` [B,Q] (one may hold a single row shared by the other's images).  ``smooth_kappa``:
    the product is also convolved with the matrix-Fisher kernel of that concentration (None: band limiting alone, which rings where
    the product is sharper than lmax resolves; ``truncation`` is then 2 lmax + 1).  -> the dict of ``grid_diffuse_spectral``."""
    from .utils import harmonics
    who = "grid_compose"
    _local_args(logp_a, grid, who, "logp_a")
    _local_args(logp_b, grid, who, "logp_b")
    _error_args(logp_a, grid, who)
    _error_args(logp_b, grid, who)
    if logp_a.shape[0] != logp_b.shape[0] and 1 not in (logp_a.shape[0], logp_b.shape[0]):
        raise ValueError(f"{who}: logp_a holds {logp_a.shape[0]} images, logp_b {logp_b.shape[0]} (the same number, or one of them 1)")
    lmax = harmonics._lmax(lmax, who)
    h, truncation = _spectral_multiplier(smooth_kappa, None, lmax, who, required=False)
    Fa, Fb = harmonics.so3_fourier(grid, lmax, log_weights=logp_a), harmonics.so3_fourier(grid, lmax, log_weights=logp_b)
    return _spectral_density(harmonics.compose(Fa, Fb, lmax, invert_a=invert_a).contiguous(), grid, lmax, h, truncation)


def grid_pose_spectrum(flow: Flow, feature: torch.Tensor = None, lmax: int = 8, number_queries: int = None, recursion_level: int = None,
                       offset=None, base=None, images_per_launch: int = None) -> dict:
    """``grid_spectrum`` of each image's density on the grid of ``grid_estimate_rotations`` (same inputs, same launches; a group's
    coefficients do not depend on the launch that held it).  Flows with batch-coupled layers are refused as in ``grid_pose_fisher``.
    -> the dict of ``grid_spectrum`` plus offset [3,3]."""
    from .utils import harmonics
    who = "grid_pose_spectrum"
    lmax = harmonics._lmax(lmax, who)
    _refuse_batch_coupled(flow, who, ", so an image's density would depend on the launch")
    gf, level, offset = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, who)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        parts = [harmonics.so3_fourier(grid, lmax, log_weights=lp) for b0, b1, lp in gf.images(grid, images_per_launch, who)]
        out = _spectrum_of(parts[0] if len(parts) == 1 else torch.cat(parts), lmax)
    out["offset"] = offset
    return out


def grid_pose_fit(flow: Flow, feature: torch.Tensor = None, samples: torch.Tensor = None, n_samples: int = 1 << 18, recursion_level: int = 2,
                  offset=None, base=None, images_per_launch: int = None) -> dict:
    """Samples against the flow's density, on the grid of ``grid_estimate_rotations`` (same inputs, same launches, the chunk gathering of
    ``grid_pose_modes``): each image's ``samples`` are binned into the grid's cells (``sd.grid_histogram`` at the offset the density is
    evaluated at) and the histogram is held against the image's log-density row (``grid_fit``, whose statistics are returned).
    ``samples`` [B,n,3,3], or [n,3,3] for one image or an unconditional flow without a B-row base: ground truths (one, or all symmetric
    ones of an image: ``grid_log_likelihood`` is then IPDF's log-likelihood of the ground truth's cell), rotations of a dataset (``kl``:
    data against model), samples of another model.  ``samples`` None: ``n_samples`` per image are drawn from the flow itself --
    ``base.sample`` (``sd.random_rotations`` without a base) through ``flow.inverse`` with the image's feature row, in launches of at
    most the module's launch budget, accumulated into one histogram -- so ``kl`` and ``z`` say whether the sampler and the density agree
    (``kl`` against its floor (Q - 1) / (2 n)).  Flows with batch-coupled layers take one image per launch, as in ``grid_pose_credible``.
    Limits (ValueError before any launch): recursion_level 0..6 (Q <= 2^26), n_samples >= 1.
    -> ``grid_fit``'s dict (every entry [B]; ``log_norm`` is the grid's) plus counts [B,Q] int32 and offset [3,3]"""
    who = "grid_pose_fit"
    level = int(recursion_level)
    if not 0 <= level <= sd.MAX_LEVEL or sd.grid_size(level) > GRID_FIT_MAX_ROWS:
        raise ValueError(f"{who}: recursion_level={recursion_level} outside 0..6 (at most 2^26 grid rows)")
    if samples is None and int(n_samples) < 1:
        raise ValueError(f"{who}: n_samples={n_samples} (at least 1)")
    if samples is not None and (samples.dim() not in (3, 4) or tuple(samples.shape[-2:]) != (3, 3)):
        raise ValueError(f"{who}: samples of shape {tuple(samples.shape)} (want [B,n,3,3] or [n,3,3])")
    if images_per_launch is not None and int(images_per_launch) < 1:
        raise ValueError(f"{who}: images_per_launch={images_per_launch}")
    gf, level, offset = _grid_inputs(flow, feature, None, level, offset, base, who)
    B, dev = gf.B, gf.dev
    if B > 65535:
        raise ValueError(f"{who}: {B} images (at most 65535)")
    if samples is not None:
        if samples.dim() == 3:
            samples = samples[None]
        if samples.shape[0] != B:
            raise ValueError(f"{who}: samples for {samples.shape[0]} images, {B} images")
        samples = samples.to(device=dev, dtype=torch.float32)
    Q = sd.grid_size(level)
    with torch.no_grad():
        if samples is not None:
            counts = sd.grid_histogram(samples, level, offset)
        else:
            counts = torch.zeros(B, Q, dtype=torch.int32, device=dev)
            total = int(n_samples)
            step = 1 if gf.coupled else min(B, gf.budget)               # images per sampling launch
            for b0 in range(0, B, step):
                b1 = min(B, b0 + step)
                k = b1 - b0
                mf = None
                if gf.A is not None:                                    # the images' base rows; a single row serves them all
                    mf = fisher.MatrixFisherN(gf.A if gf.A.shape[0] == 1 else gf.A[b0:b1])
                per = max(1, gf.budget // k)
                for s0 in range(0, total, per):
                    m = min(per, total - s0)
                    if mf is None:
                        z = sd.random_rotations(k * m, device=dev)
                    else:
                        z = mf.sample(k * m if gf.A.shape[0] == 1 else m).reshape(k * m, 3, 3)
                    feat = gf.feature[b0:b1] if gf.feature is not None else None
                    x = flow.inverse(z, feat, feature_repeat=m if feat is not None else None)[0]
                    sd.grid_histogram(x.reshape(k, m, 3, 3), level, offset, out=counts[b0:b1])
        grid = sd.generate_healpix_grid(level, device=dev, offset=offset)
        fits = []
        for b0, b1, lp in gf.images(grid, images_per_launch, who):
            fits.append(grid_fit(lp, counts[b0:b1]))
    out = fits[0] if len(fits) == 1 else {k: (torch.cat([f[k] for f in fits]) if k != "dof" else Q - 1) for k in fits[0]}
    out.update(counts=counts, offset=offset)
    return out


def grid_pose_fisher(flow: Flow, feature: torch.Tensor = None, number_queries: int = None, recursion_level: int = None, offset=None, base=None,
                     images_per_launch: int = None) -> dict:
    """The matrix-Fisher distribution that matches each image's density on the grid of ``grid_estimate_rotations`` (same inputs, same
    launches): the grid moment M_b = sum_i softmax(log p_b)_i R_i in fp64 (``rnf_rotation_moments`` on the shared grid) and its
    maximum-likelihood A_b (``rnf_fisher_fit``), i.e. the Fisher with E[R] = M_b -- the moment projection of the grid posterior.
    ``mode`` = U V^T of A's proper SVD is its most likely rotation, ``s`` its three concentrations; ``mean_rotation`` and ``entropy`` come
    from the exact kernel on the fitted A.  ``status`` [B] int32 as ``fit_matrix_fisher`` (1: capped at the default max_concentration 1e4,
    e.g. all mass on one grid point).  Flows with batch-coupled layers are refused as in ``grid_beam_estimate_rotations``.
    -> dict(A [B,3,3], mean_rotation [B,3,3], mode [B,3,3], s [B,3] fp64, entropy [B], status [B], moments [B,3,3] fp64, offset [3,3])"""
    who = "grid_pose_fisher"
    _refuse_batch_coupled(flow, who, ", so an image's density would depend on the launch")
    gf, level, offset = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, who)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        moments = []
        for b0, b1, lp in gf.images(grid, images_per_launch, who):
            moments.append(fisher.rotation_moments(grid, lp))
        moments = moments[0] if len(moments) == 1 else torch.cat(moments)
        fit = fisher.fit_matrix_fisher(moments)
        U, V, _, _ = fisher.device_proper_svd(fit["A"])
        mf = fisher.MatrixFisherN(fit["A"], "exact")
        return dict(A=fit["A"], mean_rotation=mf.mean_rotation(), mode=U @ V.transpose(-1, -2), s=fit["s"], entropy=mf.entropy(),
                    status=fit["status"], moments=moments, offset=offset)


def grid_pose_mixture(flow: Flow, feature: torch.Tensor = None, components: int = 4, separation_deg: float = 15.0, iterations: int = 64,
                      tol: float = 1e-9, number_queries: int = None, recursion_level: int = None, offset=None, base=None,
                      images_per_launch: int = None, max_concentration: float = 1e4) -> dict:
    """A ``components``-component mixture of matrix-Fishers for each image's density on the grid of ``grid_estimate_rotations`` (same
    inputs, same launches as ``grid_pose_fisher``): EM on the shared grid with the image's log-densities as log-weights
    (``rnf_fisher_mixture_fit``), started from the image's ``grid_modes`` (``fisher.mixture_init_from_modes``: component k on mode k,
    weight = the mode's share of the mass; a mode that does not exist is an empty component, status 8, weight 0).  ``kl`` = log Q -
    weight_entropy - log_likelihood is the KL divergence from the grid-normalised posterior (mass softmax(log p)_i on cell i, i.e. density
    Q softmax(log p)_i w.r.t. Haar) to the mixture: >= 0 up to rounding, the smaller the better the summary; with ``components=1`` it is
    the same quantity for the single Fisher of ``grid_pose_fisher``, whose A, s and status that call reproduces bit for bit.
    ``mode`` = U V^T of each A's proper SVD.  Flows with batch-coupled layers are refused as in ``grid_pose_fisher``.
    -> dict(A [B,K,3,3], weight [B,K] fp64, mode [B,K,3,3], s [B,K,3] fp64, log_likelihood [B] fp64, kl [B] fp64, status [B,K],
    iterations [B], loglik [B,iterations+1] fp64 (the trace: entry t before iteration t, NaN after the last used one), offset [3,3])"""
    who = "grid_pose_mixture"
    if not 1 <= int(components) <= 8:
        raise ValueError(f"{who}: components={components} outside 1..8")
    if not 0.0 < float(separation_deg) <= 180.0:
        raise ValueError(f"{who}: separation_deg={separation_deg} outside (0, 180]")
    _refuse_batch_coupled(flow, who, ", so an image's density would depend on the launch")
    K, sep = int(components), float(np.deg2rad(np.float64(separation_deg)))
    gf, level, offset = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, who)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=gf.dev, offset=offset)
        B, Q = gf.B, grid.shape[0]
        fits = []
        for b0, b1, lp in gf.images(grid, images_per_launch, who):
            index, _, mass, _, _ = grid_modes(lp, grid, K, sep)
            A0, lp0 = fisher.mixture_init_from_modes(grid, index, mass, sep)
            fits.append(fisher.fit_matrix_fisher_mixture(grid, lp, A0, lp0, iterations, tol, max_concentration))
        fit = fits[0] if len(fits) == 1 else {k: torch.cat([f[k] for f in fits]) for k in fits[0]}
        U, V, _, _ = fisher.device_proper_svd(fit["A"])
        L = fit["loglik"].gather(1, fit["iterations"].long()[:, None])[:, 0]
        return dict(A=fit["A"], weight=fit["log_pi"].exp(), mode=(U @ V.transpose(-1, -2)).reshape(B, K, 3, 3), s=fit["s"], log_likelihood=L,
                    kl=float(np.log(Q)) - fit["weight_entropy"] - L, status=fit["status"], iterations=fit["iterations"], loglik=fit["loglik"],
                    offset=offset)


def grid_children(parents: torch.Tensor, level: int, offset=None, rotations: bool = True):
    """``rnf_so3_grid_children``: the 12 level-(``level`` + 1) children of each level-``level`` grid row in ``parents`` [..., m] (int64, on
    the device; a row outside the level, e.g. -1, has children -1) -> (rows [..., m * 12] int64, rotations [..., m * 12, 3, 3] or None).
    The rotations are bit-identical to the rows of ``utils.sd.generate_healpix_grid(level + 1, offset=offset)`` (include/rnf_hip.h)."""
    dev = parents.device
    par = parents.to(torch.int64).contiguous()
    shape = par.shape[:-1] + (par.shape[-1] * 12,)
    rows = torch.empty(shape, dtype=torch.int64, device=dev)
    rot = torch.empty(shape + (3, 3), dtype=torch.float32, device=dev) if rotations else None
    off = offset.reshape(9).to(device=dev, dtype=torch.float32).contiguous() if offset is not None else None
    _lib.call("so3_grid_children", _lib.GridChildren(level=int(level), parents=par.data_ptr(), n=par.numel(),
                                                     offset=off.data_ptr() if off is not None else None, rows_out=rows.data_ptr(),
                                                     rot_out=rot.data_ptr() if rot is not None else None), dev)
    return rows, rot


def grid_beam_select(logp: torch.Tensor, beam: int, rows: torch.Tensor = None):
    """``rnf_grid_beam_select``: per image (row of ``logp`` [g,M], float32 on the device), the ``beam`` best distinct candidate rows --
    log p descending (a NaN first), then row ascending; ``rows`` [g,M] int64 the candidates' grid rows (None: candidate i is row i; a row
    < 0 is no candidate).  Past the distinct rows: row -1, log p -inf.  -> (rows [g,beam] int64, log_prob [g,beam])"""
    g, M = logp.shape
    dev = logp.device
    lp = logp.to(torch.float32).contiguous()
    rw = rows.reshape(g, M).to(torch.int64).contiguous() if rows is not None else None
    rows_out = torch.empty(g, int(beam), dtype=torch.int64, device=dev)
    logp_out = torch.empty(g, int(beam), dtype=torch.float32, device=dev)
    args = _lib.GridBeamSelect(logp=lp.data_ptr(), rows=rw.data_ptr() if rw is not None else None, M=M, g=g, beam=int(beam),
                               rows_out=rows_out.data_ptr(), logp_out=logp_out.data_ptr())
    _lib.call("grid_beam_select", args, dev)
    return rows_out, logp_out


GRID_BEAM_MAX = 1024
GRID_BEAM_MAX_START = 4


def grid_beam_estimate_rotations(flow: Flow, feature: torch.Tensor = None, recursion_level: int = 5, start_level: int = 2, beam: int = 16,
                                 offset=None, base=None, images_per_launch: int = None):
    """Coarse-to-fine beam search for ``grid_estimate_rotations``'s estimate at level ``recursion_level``: evaluate the whole level
    ``start_level`` grid, keep each image's ``beam`` best distinct rows (``rnf_grid_beam_select``), then at every level up to
    ``recursion_level`` evaluate the 12 children of each kept row (``rnf_so3_grid_children``: the four NESTED sub-pixels times the tilts
    2t - 1, 2t, 2t + 1) and select again; the last level keeps the best row.  Every evaluated row is a row of the full level-L grid (same
    rotation bits, same log p), so ``index`` is in the full grid's row order and, when the beams cover every row, the result is
    ``grid_estimate_rotations(recursion_level=L)``'s.  About beam * 12 * (L - start_level) rows per image instead of 72 * 8^L.
    No host synchronisation between levels.

    Inputs as ``grid_estimate_rotations`` (feature [B,F] or None, ``offset``, ``base`` with 1 or B rows); ``images_per_launch`` groups the
    start level as there and the refinement launches up to about 2^21 rows (beam * 12 per image).  Limits (ValueError before any launch):
    0 <= start_level <= min(recursion_level, 4), recursion_level <= 8, 1 <= beam <= 1024; flows with batch-coupled layers are refused
    (their matrices come from a launch's first rows, so a candidate set would change the density).  start_level == recursion_level is
    ``grid_estimate_rotations`` itself.  Returns (est [B,3,3], max_log_prob [B], index [B] into the level-L grid, offset [3,3])."""
    who = "grid_beam_estimate_rotations"
    L, S, beam = int(recursion_level), int(start_level), int(beam)
    if not 0 <= L <= sd.MAX_LEVEL:
        raise ValueError(f"{who}: recursion_level={recursion_level} outside 0..{sd.MAX_LEVEL}")
    if not 0 <= S <= min(L, GRID_BEAM_MAX_START):
        raise ValueError(f"{who}: start_level={start_level} outside 0..min(recursion_level, {GRID_BEAM_MAX_START})")
    if not 1 <= beam <= GRID_BEAM_MAX:
        raise ValueError(f"{who}: beam={beam} outside 1..{GRID_BEAM_MAX}")
    if images_per_launch is not None and int(images_per_launch) < 1:
        raise ValueError(f"{who}: images_per_launch={images_per_launch}")
    _refuse_batch_coupled(flow, who)
    if S == L:
        return grid_estimate_rotations(flow, feature, recursion_level=L, offset=offset, base=base, images_per_launch=images_per_launch)
    gf, _, offset = _grid_inputs(flow, feature, None, L, offset, base, who)
    B, dev = gf.B, gf.dev
    with torch.no_grad():
        # the start level: the whole grid, in grid_estimate_rotations' launches; an image evaluated in chunks is gathered first
        grid = sd.generate_healpix_grid(S, device=dev, offset=offset)
        kept = torch.empty(B, beam, dtype=torch.int64, device=dev)
        for b0, b1, lp in gf.images(grid, images_per_launch, who):
            kept[b0:b1] = grid_beam_select(lp, beam)[0]
        del grid
        # the refinement levels: each image's beam * 12 children in one shared-row launch group of about 2^21 rows
        M = beam * 12
        g = int(images_per_launch) if images_per_launch is not None else max(1, gf.budget // M)
        g = max(1, min(g, B, 65535))
        est = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
        best = torch.empty(B, dtype=torch.float32, device=dev)
        index = torch.empty(B, dtype=torch.int64, device=dev)
        for level in range(S, L):
            last = level + 1 == L
            nxt = torch.empty(B, beam, dtype=torch.int64, device=dev) if not last else None
            for b0 in range(0, B, g):
                b1 = min(B, b0 + g)
                rows, rot = grid_children(kept[b0:b1], level, offset)
                lp = gf.log_prob(rot.reshape(-1, 3, 3), b0, b1, M).reshape(b1 - b0, M)
                sel = grid_beam_select(lp, 1 if last else beam, rows)[0]
                if not last:
                    nxt[b0:b1] = sel
                    continue
                pos = torch.argmax((rows == sel).to(torch.int32), dim=-1)          # the first candidate of the chosen row
                ar = torch.arange(b1 - b0, device=dev)
                est[b0:b1], best[b0:b1], index[b0:b1] = rot[ar, pos], lp[ar, pos], sel[:, 0]     # log p with its own bits
            kept = nxt
    return est, best, index, offset
