#!/usr/bin/env python3
"""Time of the exact matrix-Fisher normaliser kernel (rnf_fisher_exact: c alone, c + mean rotation) beside the closed-form type-1 constant
(rnf_fisher_log_const_nt) at the same B: device events around `--launches` back-to-back launches after a warm-up, best and median of
`--repeats` windows, one JSON line per case.   python tools/bench_fisher_exact.py [--launches 50]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rotationnormflow_amd import _lib  # noqa: E402


def window(fn, launches):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / launches            # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    L = _lib.lib()
    device = torch.cuda.get_device_name(0)
    for B in (1, 1024, 65536):
        rng = np.random.default_rng(B)
        A = torch.from_numpy((rng.standard_normal((B, 3, 3)) * 10.0 ** rng.uniform(-4, 4, (B, 1, 1))).astype(np.float32)).cuda()
        c = torch.empty(B, dtype=torch.float32, device="cuda")
        mean = torch.empty(B, 3, 3, dtype=torch.float32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        cases = {
            "exact c": lambda: _lib.check(L.rnf_fisher_exact(A.data_ptr(), B, c.data_ptr(), None, st)),
            "exact c + mean": lambda: _lib.check(L.rnf_fisher_exact(A.data_ptr(), B, c.data_ptr(), mean.data_ptr(), st)),
            "type 1 c": lambda: _lib.check(L.rnf_fisher_log_const_nt(A.data_ptr(), B, 1, None, 0, c.data_ptr(), st)),
        }
        for name, fn in cases.items():
            window(fn, a.launches)                              # warm-up
            us = sorted(window(fn, a.launches) for _ in range(a.repeats))
            print(json.dumps(dict(metric="us per launch", case=name, B=B, best=round(us[0], 2), median=round(us[len(us) // 2], 2),
                                  launches=a.launches, repeats=a.repeats, device=device)), flush=True)


if __name__ == "__main__":
    main()
