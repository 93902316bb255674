"""Minimal evaluation harness for the hot path (SURVEY 8(f) "next", rank 1): load a checkpoint written by the reference's
``Agent.save_ckpt`` (agent.py:111-153: ``torch.save({"clock", "flow_state_dict", "optimizer_flow_state_dict", ...})``), read a
``raw`` dataset file (dataset/dataset_raw.py:13: ``{data_dir}/raw/{category}_{phase}.npy``, float32 ``[M,3,3]``) and reproduce the
statistic ``eval_uncondition.py:31-45`` prints: the mean over the whole test set of the per-sample log-likelihood
``ldj + base_log_prob`` (agent.py:226-229).  Everything numerical runs through the HIP path (Flow.log_prob).

    python -m rotationnormflow_amd.harness --ckpt exps/.../ckpt_iteration50000.pth --data data/raw/peak_test.npy \\
           [--config settings/raw.yml] [--batch-size 1048576]

``train_uncondition`` is the matching minimal training loop (train_uncondition.py:37-90 + agent.py:75-92 for the unconditional
``raw`` recipe): Adam on ``mean(-ldj)`` over shuffled mini-batches, periodic test log-likelihood, checkpoints in the reference's
format so that ``Agent.load_ckpt`` (agent.py:171-198) and this module read them back.

    python -m rotationnormflow_amd.harness --train data/raw/peak_train.npy --data data/raw/peak_test.npy --ckpt out.pth \\
           [--config settings/raw.yml] [--iterations 50000] [--train-batch 1024] [--lr 1e-4]
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import io
import os

import numpy as np
import torch

from .configs import load_yaml_config, make_config
from . import runtime
from .flow.flow import Flow


def load_reference_checkpoint(path, map_location="cpu") -> dict:
    """-> the flow's state dict from a reference checkpoint (or from a bare state-dict file).  Strips a DataParallel
    ``module.`` prefix if present (agent.py:133 saves ``flow.module.state_dict()``, older dumps may not)."""
    obj = torch.load(path, map_location=map_location, weights_only=False)
    sd = obj.get("flow_state_dict", obj) if isinstance(obj, dict) else obj
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


FEATURE_SCALE_SUFFIX = ".rnf.json"


def read_sidecar(ckpt_path) -> dict:
    """``<ckpt>.rnf.json`` as a dictionary ({} when there is none): "feature_mean_square" (the equalisation's calibration input) and, round 6,
    "rootfinder_first_order" (3 | 4, ``Flow.set_rootfinder_order``).  The reference's checkpoint layout (agent.py:132-146) has no place for
    either and must stay loadable by the reference, hence a file NEXT to the checkpoint."""
    import json
    side = str(ckpt_path) + FEATURE_SCALE_SUFFIX
    if not os.path.exists(side):
        return {}
    with open(side) as fh:
        return dict(json.load(fh))


def read_feature_scale(ckpt_path):
    """The calibration a checkpoint's sidecar carries (``<ckpt>.rnf.json``: {"feature_mean_square": m_f}), or None."""
    value = read_sidecar(ckpt_path).get("feature_mean_square")
    return None if value is None else float(value)


def write_rootfinder_order(ckpt_path, order: int) -> None:
    """Record the root finder's first-pass order (3 | 4) in the checkpoint's sidecar, beside whatever it already holds."""
    import json
    if order not in (3, 4):
        raise ValueError(f"root-finder first-pass order must be 3 or 4, got {order!r}")
    side = read_sidecar(ckpt_path)
    side["rootfinder_first_order"] = int(order)
    with open(str(ckpt_path) + FEATURE_SCALE_SUFFIX, "w") as fh:
        json.dump(side, fh)


def write_feature_scale(ckpt_path, flow_or_value, features=None) -> float:
    """Write the sidecar: the flow's fixed calibration (``Flow.set_feature_scale`` / ``calibrate_feature_scale``), a number, or -- with
    ``features`` -- the mean square measured on that batch.  Conditional flows whose features are not of unit scale want one, so that every
    process that loads the checkpoint packs the same images without seeing data first."""
    import json
    if features is not None:
        value = runtime.feature_mean_square(features)
    elif isinstance(flow_or_value, (int, float)):
        value = runtime.quantise_feature_ms(float(flow_or_value))
    else:
        value = getattr(flow_or_value, "_feature_ms_fixed", None)
        if value is None:
            raise ValueError("the flow has no fixed feature scale: call flow.calibrate_feature_scale(features) first, or pass features=")
    side = read_sidecar(ckpt_path)
    side["feature_mean_square"] = float(value)
    with open(str(ckpt_path) + FEATURE_SCALE_SUFFIX, "w") as fh:
        json.dump(side, fh)
    return float(value)


def build_flow_from_checkpoint(config, ckpt_path, device="cuda") -> Flow:
    with contextlib.redirect_stdout(io.StringIO()):
        flow = Flow(config)
    missing = flow.load_state_dict(load_reference_checkpoint(ckpt_path), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    flow = flow.to(device).eval()
    side = read_sidecar(ckpt_path)
    ms = side.get("feature_mean_square") if getattr(config, "condition", 0) else None
    if ms is not None:
        flow.set_feature_scale(float(ms))
    if side.get("rootfinder_first_order") is not None:
        flow.set_rootfinder_order(int(side["rootfinder_first_order"]))
    return flow


def load_raw_rotations(path) -> torch.Tensor:
    data = np.load(path)
    if data.ndim != 3 or data.shape[1:] != (3, 3):
        raise ValueError(f"{path}: expected a [M,3,3] array of rotation matrices, got {data.shape}")
    return torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32))


def mean_log_likelihood(flow: Flow, rotations: torch.Tensor, base=None, batch_size: int = 1 << 20, device="cuda") -> float:
    """eval_uncondition.py:31-45: np.mean over the test set of (ldj + base log-prob).  fp64 accumulation on the device."""
    total = torch.zeros(2, dtype=torch.float64, device=device)
    with torch.no_grad():
        for lo in range(0, rotations.shape[0], batch_size):
            total += flow.log_prob(rotations[lo:lo + batch_size].to(device), base=base)["sum"]
    return float(total[0] / total[1])


def expand_optimizer_state(flow: Flow, state: dict) -> dict:
    """Optimizer state of a FLATTENED flow in its in-memory form (one entry) -> the layout the reference's ``optim.Adam(flow.parameters())``
    has (one entry per parameter tensor, agent.py:23,143).  ``optimizer.state_dict()`` of an optimizer built over a flattened flow already
    returns that layout (rotationnormflow_amd/flatopt.py hooks it); such a state is returned unchanged."""
    if not flow.is_flat:
        return state
    from . import flatopt
    return flatopt.expand_state([{"params": [flow._parameters["_flat"]]}], state)


def flatten_optimizer_state(flow: Flow, state: dict) -> dict:
    """The inverse: an optimizer state in the reference's per-tensor layout (a checkpoint ``Agent.save_ckpt`` wrote) -> the one-entry
    state of an optimizer over the flattened flow's parameter (what ``optimizer.load_state_dict`` does by itself through flatopt)."""
    if not flow.is_flat:
        return state
    from . import flatopt
    n = len(flow._flat_slots)
    if len(state["param_groups"]) != 1 or len(state["param_groups"][0]["params"]) not in (1, n):
        raise ValueError(f"optimizer state covers {[len(g['params']) for g in state['param_groups']]} parameters, the flow has {n} tensors")
    return flatopt.flatten_state([{"params": [flow._parameters["_flat"]]}], state)


def save_reference_checkpoint(path, flow: Flow, optimizer, epoch: int, minibatch: int, iteration: int):
    """The dictionary ``Agent.save_ckpt`` writes for an unconditional flow (agent.py:132-151; clock: utils/utils.py:36-45).  The optimizer
    state of a flattened flow is written in the reference's per-tensor layout (``optimizer.state_dict()`` returns it: flatopt)."""
    torch.save({
        "clock": {"epoch": epoch, "minibatch": minibatch, "iteration": iteration},
        "flow_state_dict": {k: v.detach().cpu() for k, v in flow.state_dict().items()},
        "optimizer_flow_state_dict": expand_optimizer_state(flow, optimizer.state_dict()),
    }, path)


def host_preprocess_layers(flow) -> list:
    """Names of the layer classes of ``flow`` whose training tensors go through host-side linear algebra (rot='16Rot' / '16UnRot',
    '9TransLSVD' / '9TransRSVD' / '9TransRSmith'): such flows cannot be captured into a HIP graph."""
    return sorted({type(l).__name__ for l in flow.layers if getattr(l, "_rnf_host_preprocess", False) or getattr(l, "_rnf_no_graph", False)})


class GraphedTrainStep:
    """One training iteration (agent.py:75-92: forward, loss, zero_grad, backward, optimizer step) captured ONCE as a HIP graph and
    replayed: the iteration is launch-bound on the host (264 parameter tensors go through autograd and the optimizer one by one), the
    graph replays the same dozen device launches without any of it.

        step = GraphedTrainStep(flow, optimizer, rotation_shape=(1024, 3, 3))          # optimizer: Adam(..., capturable=True)
        loss = step(batch)                                                             # device tensor, valid until the next call

    Static shapes: every batch must have ``rotation_shape`` (and ``feature_shape``).  ``base``: optional MatrixFisherN with a frozen A
    (its term is added to the loss as in agent.py:58-65)."""

    def __init__(self, flow: Flow, optimizer, rotation_shape, feature_shape=None, base=None, warmup: int = 3, device="cuda"):
        from . import runtime
        blockers = host_preprocess_layers(flow)
        if blockers:
            raise RuntimeError(f"GraphedTrainStep: {', '.join(blockers)} build their training tensors on the host (a 4x4 / 3x3 SVD or "
                               "Gram-Schmidt per iteration: a device->host copy, illegal during stream capture); train this flow eagerly "
                               "(train_uncondition(..., graph=False))")
        self._runtime = runtime
        self.flow, self.optimizer, self.base = flow, optimizer, base
        self.rotation = torch.eye(3, device=device).expand(*rotation_shape).contiguous()
        self.feature = torch.zeros(feature_shape, device=device) if feature_shape is not None else None
        # The warm-up iterations torch.cuda.graphs needs (lazy optimizer state, allocator pools) run on placeholder data, so the
        # parameters and the optimizer state are put back IN PLACE afterwards (the graph must keep seeing the same tensors).
        params = [p for g in optimizer.param_groups for p in g["params"]]
        saved_params = [p.detach().clone() for p in params]
        saved_state = {id(p): {k: v.clone() for k, v in optimizer.state.get(p, {}).items() if torch.is_tensor(v)} for p in params}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # off the default stream, as torch.cuda.graphs requires
            for _ in range(warmup):
                optimizer.zero_grad(set_to_none=True)
                self._loss().backward()
                optimizer.step()
            with torch.no_grad():
                for p, old in zip(params, saved_params):
                    p.copy_(old)
                    for k, v in optimizer.state.get(p, {}).items():
                        if torch.is_tensor(v):
                            before = saved_state[id(p)].get(k)
                            v.copy_(before) if before is not None else v.zero_()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        with torch.cuda.graph(self.graph):
            self.loss = self._loss()
            self.loss.backward()
            optimizer.step()

    def _loss(self):
        rot, ldj = self.flow(self.rotation, self.feature)
        loss = (-ldj).mean()
        if self.base is not None:
            loss = loss - self.base._log_prob(rot).mean()
        return loss

    def __call__(self, rotation, feature=None):
        self.rotation.copy_(rotation)
        if self.feature is not None:
            self.feature.copy_(feature)
        self.graph.replay()
        self._runtime.note_training_step()                  # parameters changed: host-packed blobs of the eval path are stale
        return self.loss


def train_uncondition(flow: Flow, train_rotations: torch.Tensor, iterations: int, batch_size: int = 1024, lr: float = 1e-4,
                      seed: int = 42, test_rotations: torch.Tensor = None, val_every: int = 0, ckpt_path=None, save_every: int = 0,
                      base=None, device="cuda", log=print, graph: bool = True, data_parallel=None):
    """Maximum-likelihood training of an unconditional flow on a ``raw`` rotation set.  One iteration = the reference's
    ``Agent.train_func`` (agent.py:75-92): loss = mean(-ldj) (- mean base log-prob if ``base`` is given), zero_grad, backward, Adam
    step -- here three HIP launches (device packer, fused forward, fused backward) plus the optimizer; with ``graph`` (default) the
    whole iteration is captured once as a HIP graph and replayed (GraphedTrainStep), which removes the per-tensor host work.
    Returns the list of (iteration, train loss) pairs sampled every 100 iterations and the final test log-likelihood (or None)."""
    flow = flow.to(device).train()
    gen = torch.Generator().manual_seed(seed)
    data = train_rotations.to(device)
    n = data.shape[0]
    # data parallel: every rank draws the SAME global mini-batch (same seed) and trains on its own contiguous slice of it; the
    # gradient blob is averaged over the ranks by one all-reduce inside backward (dist.data_parallel_training), so each rank takes
    # the optimizer step of the global batch and the replicas stay identical.  Over RCCL the all-reduce is captured into the HIP
    # graph of the iteration like any other launch (stream-ordered); over gloo (host collectives) the iteration runs eagerly.
    import torch.distributed as tdist
    world = tdist.get_world_size() if (tdist.is_available() and tdist.is_initialized()) else 1
    rank = tdist.get_rank() if world > 1 else 0
    from .dist import collectives_are_capturable, data_parallel_training, shard_bounds
    if world > 1 or data_parallel:                       # data_parallel=True forces the gradient all-reduce on a one-rank group too
        data_parallel_training(flow, even_alone=bool(data_parallel) and world == 1)
        if graph and not collectives_are_capturable():    # RCCL collectives are stream-ordered and captured with the rest of the
            graph = False                                 # iteration; gloo's run on the host: eager iterations then
    if graph and host_preprocess_layers(flow):
        log(f"train_uncondition: {', '.join(host_preprocess_layers(flow))} need host-side linear algebra every iteration; training eagerly "
            "(no HIP graph)")
        graph = False
    opt = torch.optim.Adam(flow.parameters(), lr=lr, fused=True, capturable=graph)   # one launch instead of a dozen foreach kernels
    batch_size = min(batch_size, n)
    if graph and world > 1 and batch_size % world:        # the graph has static shapes: every rank's slice must have the same size
        raise ValueError(f"train_uncondition: batch_size {batch_size} must be a multiple of the world size {world} for graphed "
                         "data-parallel training (or pass graph=False)")
    gstep = GraphedTrainStep(flow, opt, (batch_size // world, 3, 3), base=base, device=device) if graph else None
    history, it, epoch = [], 0, 0
    while it < iterations:
        perm = torch.randperm(n, generator=gen).to(device)
        for mb, lo in enumerate(range(0, n - batch_size + 1, batch_size)):
            batch = data[perm[lo:lo + batch_size]]
            if world > 1:
                b0, b1 = shard_bounds(batch.shape[0], rank, world)
                batch = batch[b0:b1]
            if gstep is not None:
                loss = gstep(batch)
            else:
                rot, ldj = flow(batch)
                loss = (-ldj).mean()
                if base is not None:
                    loss = loss - base._log_prob(rot).mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
            it += 1
            if it % 100 == 0 or it == iterations:
                history.append((it, float(loss.detach())))
            if val_every and test_rotations is not None and it % val_every == 0:
                log(f"iteration {it}: train loss {float(loss.detach()):.6f}  test log-likelihood "
                    f"{mean_log_likelihood(flow, test_rotations, base=base, device=device):.6f}")
                flow.train()
            if ckpt_path and save_every and it % save_every == 0:
                save_reference_checkpoint(ckpt_path, flow, opt, epoch, mb + 1, it)
            if it >= iterations:
                break
        epoch += 1
    if ckpt_path:
        save_reference_checkpoint(ckpt_path, flow, opt, epoch, 0, it)
    final = mean_log_likelihood(flow, test_rotations, base=base, device=device) if test_rotations is not None else None
    return history, final


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", required=True, help="checkpoint to evaluate, or (with --train) to write")
    ap.add_argument("--data", required=True, help="raw test set, [M,3,3] float32 .npy")
    ap.add_argument("--train", help="raw training set: train an unconditional flow first, then evaluate it on --data")
    ap.add_argument("--iterations", type=int, default=50000)
    ap.add_argument("--train-batch", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--config", action="append", default=[], help="settings/*.yml file(s); later files override earlier ones")
    ap.add_argument("--layers", type=int)
    ap.add_argument("--segments", type=int)
    ap.add_argument("--rot")
    ap.add_argument("--batch-size", type=int, default=1 << 20)
    args = ap.parse_args(argv)
    over = {k: v for k, v in (("layers", args.layers), ("segments", args.segments), ("rot", args.rot)) if v is not None}
    config = load_yaml_config(*args.config, **over) if args.config else make_config(**over)
    if args.train:
        torch.manual_seed(args.seed)
        with contextlib.redirect_stdout(io.StringIO()):
            flow = Flow(config)
        _, final = train_uncondition(flow, load_raw_rotations(args.train), args.iterations, args.train_batch, args.lr, args.seed,
                                     test_rotations=load_raw_rotations(args.data), val_every=1000, ckpt_path=args.ckpt, save_every=5000)
        print(final)
        return
    flow = build_flow_from_checkpoint(config, args.ckpt)
    print(mean_log_likelihood(flow, load_raw_rotations(args.data), batch_size=args.batch_size))


def estimate_rotations(flow: Flow, feature: torch.Tensor, queries: torch.Tensor = None, base=None, number_queries: int = 500):
    """Pose estimate per feature row, as ``Agent.eval_acc`` does (agent.py:238-283): push ``number_queries`` base samples per row
    through ``Flow.inverse`` and keep the sample with the largest ``-ldj + base_log_prob``.

    feature [B,F] (cuda); queries [Q,3,3] shared by all rows (the reference's ``sd.generate_queries``), or ``base`` = a
    ``MatrixFisherN`` with B rows to draw them from (``pretrain_fisher``).  Returns (est_rotation [B,3,3], log_prob [B,Q])."""
    B = feature.shape[0]
    with torch.no_grad():
        if base is not None:
            sample = base._sample(number_queries).reshape(-1, 3, 3)                     # agent.py:248-251
            base_ll = base._log_prob(sample).reshape(B, -1)
            Q = number_queries
        else:
            Q = queries.shape[0]
            sample = queries[None].expand(B, Q, 3, 3).reshape(-1, 3, 3).contiguous()    # agent.py:253-258
            base_ll = torch.zeros(B, Q, device=feature.device)
        # agent.py:240-244 repeats every feature row Q times; here the rows are shared inside the kernels (one projection per image)
        samples, ldj = flow.inverse(sample, feature, feature_repeat=Q)
        log_prob = -ldj.reshape(B, Q) + base_ll                                         # agent.py:262-263
        best = torch.argmax(log_prob, dim=-1)
        est = samples.reshape(B, Q, 3, 3)[torch.arange(B, device=best.device), best]
    return est, log_prob


# Rotations per launch of the grid search: images are grouped up to about 2^21 rotations (the regime the shared-row kernels are measured
# in); a single image's grid larger than GRID_MAX_LAUNCH_ROWS is evaluated in chunks of that size.  Flows with side layers take one feature
# row per rotation (runtime.expand_shared_rows), so their launches are kept to GRID_SIDE_LAUNCH_ROWS to bound the expanded features.
GRID_LAUNCH_ROWS = 1 << 21
GRID_MAX_LAUNCH_ROWS = 1 << 24
GRID_SIDE_LAUNCH_ROWS = 1 << 18


def _grid_inputs(flow: Flow, feature, number_queries, recursion_level, offset, base, who: str):
    """The common arguments of the grid searches -> (feature or None, device, B images, level, offset [3,3], base A [1|B,3,3], c)."""
    from .utils import sd
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
    return feature, dev, B, level, offset, A, c


def _grid_launches(flow: Flow, feature, grid, B, A, c, images_per_launch, who: str):
    """Evaluate B images' log-density on ``grid`` [Q,3,3] in launches of about GRID_LAUNCH_ROWS shared-row rotations (call under no_grad).
    Yields (b0, b1, lo, logp [b1 - b0, rows]) per launch: images b0..b1-1 on grid rows lo..lo+rows-1 -- whole images (lo = 0, rows = Q)
    when several share a launch, consecutive chunks of one image otherwise."""
    Q = grid.shape[0]
    coupled = any(getattr(m, "_rnf_batch_coupled", False) for m in flow.modules())
    packed = flow._packed(grid.device, feature)
    budget = GRID_SIDE_LAUNCH_ROWS if packed.side_layers else GRID_LAUNCH_ROWS
    if images_per_launch is None:
        images_per_launch = 1 if coupled else max(1, budget // Q)
    g = min(int(images_per_launch), B)
    if g < 1 or (coupled and g > 1):
        raise ValueError(f"{who}: images_per_launch={images_per_launch}" + (" (batch-coupled layers: 1)" if coupled else ""))
    if g > 1 and g * Q > GRID_MAX_LAUNCH_ROWS:
        raise ValueError(f"{who}: {g} images of {Q} rotations exceed {GRID_MAX_LAUNCH_ROWS} rotations per launch")
    chunk = Q if g > 1 else min(Q, GRID_SIDE_LAUNCH_ROWS if packed.side_layers else GRID_MAX_LAUNCH_ROWS)

    def log_prob(rot, b0, b1):
        feat = feature[b0:b1] if feature is not None else None
        rows = (A, c) if A is None or A.shape[0] == 1 else (A[b0:b1], c[b0:b1])
        return runtime.run_log_prob(flow, packed, rot, feat, *rows, feature_repeat=rot.shape[0] // (b1 - b0))["logp"]

    rep = grid.repeat(g, 1, 1) if g > 1 else grid          # one image per launch: the grid itself, no copy
    for b0 in range(0, B, g):
        b1 = min(B, b0 + g)
        if g > 1:
            yield b0, b1, 0, log_prob(rep[:(b1 - b0) * Q], b0, b1).reshape(b1 - b0, Q)
            continue
        for lo in range(0, Q, chunk):
            yield b0, b1, lo, log_prob(grid[lo:lo + chunk], b0, b1).reshape(1, -1)


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
    from .utils import sd
    feature, dev, B, level, offset, A, c = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base,
                                                        "grid_estimate_rotations")
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=dev, offset=offset)
        bests, indices = [], []
        for b0, b1, lo, lp in _grid_launches(flow, feature, grid, B, A, c, images_per_launch, "grid_estimate_rotations"):
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
    from . import _lib
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
    L = _lib.lib()
    need = L.rnf_grid_modes_workspace_bytes(C.byref(args))
    if need == 0:
        _lib.check(1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    args.workspace, args.workspace_bytes = ws.data_ptr(), need
    with torch.cuda.device(dev):
        args.stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.rnf_grid_modes(C.byref(args)))
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
    from .utils import sd
    if not 1 <= int(top_k) <= 16:
        raise ValueError(f"grid_pose_modes: top_k={top_k} outside 1..16")
    if not 0.0 < float(separation_deg) <= 180.0:
        raise ValueError(f"grid_pose_modes: separation_deg={separation_deg} outside (0, 180]")
    k, sep = int(top_k), float(np.deg2rad(np.float64(separation_deg)))
    feature, dev, B, level, offset, A, c = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, "grid_pose_modes")
    gt = None
    if gt_rotation is not None:
        gt = gt_rotation.reshape(B, -1, 3, 3).to(device=dev, dtype=torch.float32)
        if gt.shape[1] > 128:
            raise ValueError(f"grid_pose_modes: {gt.shape[1]} ground truths per image (at most 128)")
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=dev, offset=offset)
        Q = grid.shape[0]
        outs, whole = [], None
        for b0, b1, lo, lp in _grid_launches(flow, feature, grid, B, A, c, images_per_launch, "grid_pose_modes"):
            if lp.shape[1] < Q:                                 # one image in chunks: gather them first
                if whole is None:
                    whole = torch.empty(1, Q, dtype=torch.float32, device=dev)
                whole[:, lo:lo + lp.shape[1]] = lp
                if lo + lp.shape[1] < Q:
                    continue
                lp = whole
            outs.append(grid_modes(lp, grid, k, sep, gt[b0:b1] if gt is not None else None))
        index, log_prob, mass, log_norm, spread = (torch.cat(t) if t[0] is not None else None for t in zip(*outs))
        est = grid[index.clamp(min=0)]
        est[index < 0] = float("nan")
    out = dict(est=est, log_prob=log_prob, index=index, mass=mass, log_norm=log_norm, offset=offset)
    if gt is not None:
        out["spread_deg"] = torch.rad2deg(spread)
    return out


GRID_CREDIBLE_MAX_ROWS = 1 << 26                   # rnf_grid_credible's fixed point (include/rnf_hip.h): level 6 fits
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
    from . import _lib
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
    L = _lib.lib()
    need = L.rnf_grid_credible_workspace_bytes(C.byref(args))
    if need == 0:
        _lib.check(1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    args.workspace, args.workspace_bytes = ws.data_ptr(), need
    with torch.cuda.device(dev):
        args.stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.rnf_grid_credible(C.byref(args)))
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
    from .utils import sd
    lv = _credible_levels(levels, "grid_pose_credible")
    level = int(recursion_level) if recursion_level is not None else sd.closest_grid_level(500 if number_queries is None else number_queries)
    if sd.grid_size(level) > GRID_CREDIBLE_MAX_ROWS:
        raise ValueError(f"grid_pose_credible: level {level} has {sd.grid_size(level)} grid rows (at most 2^26)")
    if gt_rotation is not None and gt_rotation.dim() == 4 and gt_rotation.shape[1] > GRID_CREDIBLE_MAX_QUERIES:
        raise ValueError(f"grid_pose_credible: {gt_rotation.shape[1]} ground truths per image (at most {GRID_CREDIBLE_MAX_QUERIES})")
    feature, dev, B, level, offset, A, c = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, "grid_pose_credible")
    gt = None
    if gt_rotation is not None:
        gt = gt_rotation.reshape(B, -1, 3, 3).to(device=dev, dtype=torch.float32).contiguous()
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=dev, offset=offset)
        Q = grid.shape[0]
        gt_log_prob = None
        if gt is not None:
            # The images at their ground truths: shared rows through run_log_prob, each image's K padded with its first one to GRID_GT_ROW
            # rotations -- rows that long run on the kernels the grid's rows run on (csrc/flow_plan.h), so a ground truth that is a grid row
            # gets that row's log p bit for bit.  Launches hold the rows _grid_launches allows; batch-coupled flows take one image per
            # launch, as their grids do (their matrices then come from the ground truths: see the docstring).
            K = gt.shape[1]
            packed = flow._packed(dev, feature)
            coupled = any(getattr(m, "_rnf_batch_coupled", False) for m in flow.modules())
            step = 1 if coupled else max(1, (GRID_SIDE_LAUNCH_ROWS if packed.side_layers else GRID_LAUNCH_ROWS) // GRID_GT_ROW)
            pad = torch.cat([gt, gt[:, :1].expand(-1, GRID_GT_ROW - K, -1, -1)], dim=1)
            parts = []
            for b0 in range(0, B, step):
                b1 = min(B, b0 + step)
                rows = (A, c) if A is None or A.shape[0] == 1 else (A[b0:b1], c[b0:b1])
                at = runtime.run_log_prob(flow, packed, pad[b0:b1].reshape(-1, 3, 3), feature[b0:b1] if feature is not None else None,
                                          *rows, feature_repeat=GRID_GT_ROW)["logp"]
                parts.append(at.reshape(b1 - b0, GRID_GT_ROW)[:, :K].max(dim=1).values)
            gt_log_prob = parts[0] if len(parts) == 1 else torch.cat(parts)
        outs, whole = [], None
        for b0, b1, lo, lp in _grid_launches(flow, feature, grid, B, A, c, images_per_launch, "grid_pose_credible"):
            if lp.shape[1] < Q:                                 # one image in chunks: gather them first
                if whole is None:
                    whole = torch.empty(1, Q, dtype=torch.float32, device=dev)
                whole[:, lo:lo + lp.shape[1]] = lp
                if lo + lp.shape[1] < Q:
                    continue
                lp = whole
            outs.append(grid_credible(lp, lv, gt_log_prob[b0:b1, None] if gt is not None else None)[:5])
        threshold, count, mass, log_norm, gt_level = (torch.cat(t) if t[0] is not None else None for t in zip(*outs))
    volume = torch.where(count < 0, float("nan"), count.to(torch.float32) / Q)
    out = dict(threshold=threshold, count=count, volume=volume, mass=mass, log_norm=log_norm, offset=offset)
    if gt is not None:
        out.update(gt_log_prob=gt_log_prob, gt_level=gt_level[:, 0], gt_inside=gt_log_prob[:, None] >= threshold)
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
    from .utils import sd
    from .utils import fisher
    who = "grid_pose_fisher"
    coupled = sorted({type(m).__name__ for m in flow.modules() if getattr(m, "_rnf_batch_coupled", False)})
    if coupled:
        raise ValueError(f"{who}: batch-coupled layers ({', '.join(coupled)}) take their matrices from a launch's first rows, so an image's "
                         "density would depend on the launch; use grid_estimate_rotations")
    feature, dev, B, level, offset, A, c = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, who)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=dev, offset=offset)
        Q = grid.shape[0]
        moments, whole = [], None
        for b0, b1, lo, lp in _grid_launches(flow, feature, grid, B, A, c, images_per_launch, who):
            if lp.shape[1] < Q:                                 # one image in chunks: gather them first
                if whole is None:
                    whole = torch.empty(1, Q, dtype=torch.float32, device=dev)
                whole[:, lo:lo + lp.shape[1]] = lp
                if lo + lp.shape[1] < Q:
                    continue
                lp = whole
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
    from .utils import sd
    from .utils import fisher
    who = "grid_pose_mixture"
    if not 1 <= int(components) <= 8:
        raise ValueError(f"{who}: components={components} outside 1..8")
    if not 0.0 < float(separation_deg) <= 180.0:
        raise ValueError(f"{who}: separation_deg={separation_deg} outside (0, 180]")
    coupled = sorted({type(m).__name__ for m in flow.modules() if getattr(m, "_rnf_batch_coupled", False)})
    if coupled:
        raise ValueError(f"{who}: batch-coupled layers ({', '.join(coupled)}) take their matrices from a launch's first rows, so an image's "
                         "density would depend on the launch; use grid_estimate_rotations")
    K, sep = int(components), float(np.deg2rad(np.float64(separation_deg)))
    feature, dev, B, level, offset, A, c = _grid_inputs(flow, feature, number_queries, recursion_level, offset, base, who)
    with torch.no_grad():
        grid = sd.generate_healpix_grid(level, device=dev, offset=offset)
        Q = grid.shape[0]
        fits, whole = [], None
        for b0, b1, lo, lp in _grid_launches(flow, feature, grid, B, A, c, images_per_launch, who):
            if lp.shape[1] < Q:                                 # one image in chunks: gather them first
                if whole is None:
                    whole = torch.empty(1, Q, dtype=torch.float32, device=dev)
                whole[:, lo:lo + lp.shape[1]] = lp
                if lo + lp.shape[1] < Q:
                    continue
                lp = whole
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
    from . import _lib
    dev = parents.device
    par = parents.to(torch.int64).contiguous()
    shape = par.shape[:-1] + (par.shape[-1] * 12,)
    rows = torch.empty(shape, dtype=torch.int64, device=dev)
    rot = torch.empty(shape + (3, 3), dtype=torch.float32, device=dev) if rotations else None
    off = offset.reshape(9).to(device=dev, dtype=torch.float32).contiguous() if offset is not None else None
    with torch.cuda.device(dev):
        args = _lib.GridChildren(level=int(level), parents=par.data_ptr(), n=par.numel(), offset=off.data_ptr() if off is not None else None,
                                 rows_out=rows.data_ptr(), rot_out=rot.data_ptr() if rot is not None else None,
                                 stream=torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.lib().rnf_so3_grid_children(C.byref(args)))
    return rows, rot


def grid_beam_select(logp: torch.Tensor, beam: int, rows: torch.Tensor = None):
    """``rnf_grid_beam_select``: per image (row of ``logp`` [g,M], float32 on the device), the ``beam`` best distinct candidate rows --
    log p descending (a NaN first), then row ascending; ``rows`` [g,M] int64 the candidates' grid rows (None: candidate i is row i; a row
    < 0 is no candidate).  Past the distinct rows: row -1, log p -inf.  -> (rows [g,beam] int64, log_prob [g,beam])"""
    from . import _lib
    g, M = logp.shape
    dev = logp.device
    lp = logp.to(torch.float32).contiguous()
    rw = rows.reshape(g, M).to(torch.int64).contiguous() if rows is not None else None
    rows_out = torch.empty(g, int(beam), dtype=torch.int64, device=dev)
    logp_out = torch.empty(g, int(beam), dtype=torch.float32, device=dev)
    args = _lib.GridBeamSelect(logp=lp.data_ptr(), rows=rw.data_ptr() if rw is not None else None, M=M, g=g, beam=int(beam),
                               rows_out=rows_out.data_ptr(), logp_out=logp_out.data_ptr())
    L = _lib.lib()
    need = L.rnf_grid_beam_select_workspace_bytes(C.byref(args))
    if need == 0:
        _lib.check(1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    args.workspace, args.workspace_bytes = ws.data_ptr(), need
    with torch.cuda.device(dev):
        args.stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.rnf_grid_beam_select(C.byref(args)))
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
    from .utils import sd
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
    coupled = sorted({type(m).__name__ for m in flow.modules() if getattr(m, "_rnf_batch_coupled", False)})
    if coupled:
        raise ValueError(f"{who}: batch-coupled layers ({', '.join(coupled)}) take their matrices from a launch's first rows; "
                         "use grid_estimate_rotations")
    if S == L:
        return grid_estimate_rotations(flow, feature, recursion_level=L, offset=offset, base=base, images_per_launch=images_per_launch)
    feature, dev, B, _, offset, A, c = _grid_inputs(flow, feature, None, L, offset, base, who)
    with torch.no_grad():
        # the start level: the whole grid, in grid_estimate_rotations' launches; an image evaluated in chunks is gathered first
        grid = sd.generate_healpix_grid(S, device=dev, offset=offset)
        Q = grid.shape[0]
        kept = torch.empty(B, beam, dtype=torch.int64, device=dev)
        whole = None
        for b0, b1, lo, lp in _grid_launches(flow, feature, grid, B, A, c, images_per_launch, who):
            if lp.shape[1] < Q:
                if whole is None:
                    whole = torch.empty(1, Q, dtype=torch.float32, device=dev)
                whole[:, lo:lo + lp.shape[1]] = lp
                if lo + lp.shape[1] < Q:
                    continue
                lp = whole
            kept[b0:b1] = grid_beam_select(lp, beam)[0]
        del grid, whole
        # the refinement levels: each image's beam * 12 children in one shared-row launch group of about 2^21 rows
        packed = flow._packed(dev, feature)
        M = beam * 12
        budget = GRID_SIDE_LAUNCH_ROWS if packed.side_layers else GRID_LAUNCH_ROWS
        g = int(images_per_launch) if images_per_launch is not None else max(1, budget // M)
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
                feat = feature[b0:b1] if feature is not None else None
                fisher = (A, c) if A is None or A.shape[0] == 1 else (A[b0:b1], c[b0:b1])
                lp = runtime.run_log_prob(flow, packed, rot.reshape(-1, 3, 3), feat, *fisher, feature_repeat=M)["logp"]
                lp = lp.reshape(b1 - b0, M)
                sel = grid_beam_select(lp, 1 if last else beam, rows)[0]
                if not last:
                    nxt[b0:b1] = sel
                    continue
                pos = torch.argmax((rows == sel).to(torch.int32), dim=-1)          # the first candidate of the chosen row
                ar = torch.arange(b1 - b0, device=dev)
                est[b0:b1], best[b0:b1], index[b0:b1] = rot[ar, pos], lp[ar, pos], sel[:, 0]     # log p with its own bits
            kept = nxt
    return est, best, index, offset


def matrix_to_quaternion(R: torch.Tensor) -> torch.Tensor:
    """[B,3,3] rotations -> unit quaternions [B,4] (real part first), largest-component branch per row."""
    m = R.reshape(-1, 3, 3)
    m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
    cand = torch.stack([
        torch.stack([1 + m00 + m11 + m22, m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]], -1),
        torch.stack([m[:, 2, 1] - m[:, 1, 2], 1 + m00 - m11 - m22, m[:, 0, 1] + m[:, 1, 0], m[:, 0, 2] + m[:, 2, 0]], -1),
        torch.stack([m[:, 0, 2] - m[:, 2, 0], m[:, 0, 1] + m[:, 1, 0], 1 - m00 + m11 - m22, m[:, 1, 2] + m[:, 2, 1]], -1),
        torch.stack([m[:, 1, 0] - m[:, 0, 1], m[:, 0, 2] + m[:, 2, 0], m[:, 1, 2] + m[:, 2, 1], 1 - m00 - m11 + m22], -1)], 1)
    best = torch.argmax(torch.stack([cand[:, i, i] for i in range(4)], -1), -1)
    q = cand[torch.arange(m.shape[0], device=m.device), best]
    return q / q.norm(dim=-1, keepdim=True)


def refine_rotations(flow: Flow, feature, rotations: torch.Tensor, steps: int = 100, lr: float = 1e-4, base=None):
    """Pose refinement of ``eval.py``'s ``nll_grad`` mode (eval.py:464-480): gradient ascent of the log-density over the query
    rotation, parameterised by a quaternion; every step is the FIRST step of a fresh Adam (eval.py:470-471 re-creates the optimizer
    inside the loop), i.e. q <- q - lr * g / (|g| + 1e-8), followed by renormalisation.  The gradient w.r.t. the rotation comes from
    the backward sweep with the parameter gradients switched off (the flow's parameters are frozen for the duration).
    rotations [B,3,3], feature [B,F] or None.  Returns the refined rotations [B,3,3]."""
    from .utils.fisher import quaternion_to_matrix
    flags = [p.requires_grad for p in flow.parameters()]
    for p in flow.parameters():
        p.requires_grad_(False)
    try:
        q = matrix_to_quaternion(rotations.detach()).to(torch.float32)
        for _ in range(steps):
            q = q.detach().requires_grad_(True)
            with torch.enable_grad():
                rot, ldj = flow(quaternion_to_matrix(q), feature)
                loss = -ldj.mean()
                if base is not None:
                    loss = loss - base._log_prob(rot).mean()
                (g,) = torch.autograd.grad(loss, q)
            q = q.detach() - lr * g / (g.abs() + 1e-8)
            q = q / q.norm(dim=-1, keepdim=True)
        return quaternion_to_matrix(q.detach())
    finally:
        for p, f in zip(flow.parameters(), flags):
            p.requires_grad_(f)


def min_geodesic_distance(est_rotation: torch.Tensor, gt_rotation: torch.Tensor) -> torch.Tensor:
    """utils/utils.py:231-235: angle (radians) between each estimate [B,3,3] and the closest of its ground truths [B,K,3,3] (or [B,3,3])."""
    from . import _lib
    est = est_rotation.reshape(-1, 3, 3).to(torch.float32).contiguous()
    n = est.shape[0]
    gt = gt_rotation.reshape(n, -1, 3, 3).to(device=est.device, dtype=torch.float32).contiguous()
    if not est.is_cuda:
        raise RuntimeError("rotationnormflow_amd runs on the GPU only (no CPU fallback)")
    out = torch.empty(n, dtype=torch.float32, device=est.device)
    with torch.cuda.device(est.device):
        _lib.check(_lib.lib().rnf_min_geodesic(est.data_ptr(), gt.data_ptr(), n, gt.shape[1], out.data_ptr(),
                                               torch.cuda.current_stream(est.device).cuda_stream))
    return out


def pose_accuracy(flow: Flow, feature, gt_rotation, queries=None, base=None, number_queries: int = 500, thresholds_deg=(15.0, 30.0),
                  method: str = "log_inv", recursion_level: int = None, offset=None, refine_steps: int = 100, top_k: int = 1,
                  separation_deg: float = 15.0, beam: int = None, start_level: int = 2):
    """What ``Agent.eval_acc`` + ``eval.py`` report per batch (agent.py:238-283, utils/utils.py:208-209): arg-max pose estimate, geodesic
    error in degrees against the (possibly several) ground truths, accuracy at the thresholds.  -> dict(err_deg, est_rotation, acc)

    ``method`` (eval.py:36-44): "log_inv" (default) pushes base samples through the inverse (``estimate_rotations``); "log_pdf" is the
    grid search (``grid_estimate_rotations`` with ``number_queries`` / ``recursion_level`` / ``offset`` / ``base``); "nll_grad" refines the
    grid estimate with ``refine_steps`` gradient steps at lr 1e-4 without a base term (eval.py:464-480).

    ``top_k`` > 1 (grid methods only; the commented-out ``for top_k in [1, 2, 4]`` of eval.py:243,297,406): the estimates are the modes of
    ``grid_pose_modes`` (``separation_deg`` apart; "nll_grad" refines every valid one, each with its image's feature row), ``est_rotation``
    is [B,k,3,3] (NaN for a missing mode) and an image's error is the smallest over its valid modes (best of k).

    ``beam`` (grid methods with top_k = 1 only): the grid estimate is ``grid_beam_estimate_rotations``'s coarse-to-fine search from
    ``start_level`` to the level above, keeping ``beam`` rows per image ("nll_grad" refines it); None (default) searches the whole grid."""
    if method not in ("log_inv", "log_pdf", "nll_grad"):
        raise ValueError(f"pose_accuracy: method must be 'log_inv', 'log_pdf' or 'nll_grad', got {method!r}")
    if int(top_k) < 1 or (int(top_k) > 1 and method == "log_inv"):
        raise ValueError(f"pose_accuracy: top_k={top_k} needs a grid method (log_inv's samples are not equivolumetric and carry no mass)")
    if beam is not None and (method == "log_inv" or int(top_k) > 1):
        raise ValueError(f"pose_accuracy: beam={beam} needs a grid method and top_k = 1 (modes and masses need the whole grid)")
    if top_k > 1:
        return _pose_accuracy_top_k(flow, feature, gt_rotation, base, number_queries, thresholds_deg, method, recursion_level, offset,
                                    refine_steps, int(top_k), separation_deg)
    if method == "log_inv":
        est, _ = estimate_rotations(flow, feature, queries=queries, base=base, number_queries=number_queries)
    elif beam is not None:
        from .utils import sd
        level = recursion_level if recursion_level is not None else sd.closest_grid_level(number_queries)
        est = grid_beam_estimate_rotations(flow, feature, recursion_level=level, start_level=start_level, beam=beam, offset=offset,
                                           base=base)[0]
    else:
        est = grid_estimate_rotations(flow, feature, number_queries=number_queries, recursion_level=recursion_level, offset=offset,
                                      base=base)[0]
    if method == "nll_grad":
        est = refine_rotations(flow, feature, est, steps=refine_steps, lr=1e-4, base=None)
    err_deg = torch.rad2deg(min_geodesic_distance(est, gt_rotation))
    return dict(err_deg=err_deg, est_rotation=est, acc={t: float((err_deg <= t).float().mean()) for t in thresholds_deg})


def _pose_accuracy_top_k(flow, feature, gt_rotation, base, number_queries, thresholds_deg, method, recursion_level, offset, refine_steps,
                         k, separation_deg):
    modes = grid_pose_modes(flow, feature, top_k=k, separation_deg=separation_deg, number_queries=number_queries,
                            recursion_level=recursion_level, offset=offset, base=base)
    est, valid = modes["est"], modes["index"] >= 0
    B = est.shape[0]
    if method == "nll_grad":
        flat, ok = est.reshape(B * k, 3, 3).clone(), valid.reshape(-1)
        feat = feature if feature is not None and flow.condition else None
        rows = feat.repeat_interleave(k, 0)[ok] if feat is not None else None
        flat[ok] = refine_rotations(flow, rows, flat[ok], steps=refine_steps, lr=1e-4, base=None)
        est = flat.reshape(B, k, 3, 3)
    gt = gt_rotation.reshape(B, -1, 3, 3).to(device=est.device)
    err = min_geodesic_distance(est.reshape(B * k, 3, 3), gt.repeat_interleave(k, 0)).reshape(B, k)
    err_deg = torch.rad2deg(torch.where(valid, err, torch.full_like(err, float("inf"))).min(-1).values)
    return dict(err_deg=err_deg, est_rotation=est, acc={t: float((err_deg <= t).float().mean()) for t in thresholds_deg})

if __name__ == "__main__":
    main()
