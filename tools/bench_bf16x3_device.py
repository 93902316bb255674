#!/usr/bin/env python3
"""bf16x3 on the device-packed paths: what a training-mode module (or an nn.DataParallel replica) costs under no_grad against the same flow
in eval mode (host-packed, cached), in the same process.  One JSON line per workload, all times in ms:

  pack_ms         one rnf_pack_flow_device launch (bf16x3 images of every layer)
  eval_ms         eval mode, bf16x3 (the blob is cached: the call is the flow pass alone)
  train_ms        training mode under no_grad, bf16x3 (device pack + the same flow pass)
  train_fp32_ms   training mode under no_grad with set_precision("fp32"): the exact-fp32 kernels, the arithmetic these paths ran under
                  bf16x3 before the device packer built bf16x3 images

  C2    24 unconditional layers, K = 64, log p with a matrix-Fisher base, 2^20 rotations
  C4q   C4 (24 layers, F = 256, 16UnTrans), 2048 images x 512 queries (feature_repeat), log p, 2^20 rotations

    python tools/bench_bf16x3_device.py [--steps 10] [--only C2,C4q]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from oracle import flow_oracle as orc  # noqa: E402
from rotationnormflow_amd import autograd, make_config, runtime, synth  # noqa: E402
from rotationnormflow_amd.utils.fisher import MatrixFisherN  # noqa: E402
from tests.gpu_helpers import product_flow  # noqa: E402

N = 1 << 20
Q = 512


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def workload(name):
    if name == "C2":
        cfg = make_config("C2")
        w = synth.fill_state_dict(orc.state_shapes(cfg), seed=4, regime="trained")
        fl = product_flow(cfg, w)
        R = torch.from_numpy(synth.uniform_rotations(N, seed=46)).cuda()
        base = MatrixFisherN(torch.from_numpy(synth.fisher_A("tilted")).cuda())
        return fl, (lambda f: f.log_prob(R, base=base))
    cfg = make_config("C4")
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=6, regime="trained")
    fl = product_flow(cfg, w)
    R = torch.from_numpy(synth.uniform_rotations(N, seed=48)).cuda()
    rows = torch.from_numpy(synth.features(N // Q, orc.feature_dim_of(cfg), seed=50)).cuda()
    return fl, (lambda f: f.log_prob(R, rows, feature_repeat=Q))


def run(name, steps):
    fl, call = workload(name)
    out = dict(workload=name, n=N, steps=steps)
    with torch.no_grad():
        runtime.set_precision("fp32")
        fl.train()
        out["train_fp32_ms"] = timed(lambda: call(fl), steps)
        runtime.set_precision("bf16x3")
        fl.eval()
        fl.invalidate()
        out["eval_ms"] = timed(lambda: call(fl), steps)
        fl.train()
        out["train_ms"] = timed(lambda: call(fl), steps)
        plan = fl._rnf_train_plan[1]
        assert plan.precision == "bf16x3"
        plain = torch.cat([t.detach().reshape(-1) for t in autograd.train_tensors(list(fl.layers))])
        stream = torch.cuda.current_stream().cuda_stream
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        plan.pack(plain, stream)
        reps = 50
        start.record()
        for _ in range(reps):
            plan.pack(plain, stream)
        end.record()
        torch.cuda.synchronize()
        out["pack_ms"] = start.elapsed_time(end) / reps
    fl.eval()
    out["train_over_eval"] = out["train_ms"] / out["eval_ms"]
    out["fp32_over_train"] = out["train_fp32_ms"] / out["train_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", default="C2,C4q")
    args = ap.parse_args()
    old = runtime.get_precision()
    try:
        for name in args.only.split(","):
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in run(name, args.steps).items()}), flush=True)
    finally:
        runtime.set_precision(old)


if __name__ == "__main__":
    main()
