"""CPU: the operand construction of the split-fp16 fc_first step (csrc/fc_first.h), compiled for the host into a stand-alone program
(tests/csrc/host_fc_first.cpp: both lane halves' A and B operands for random rows and columns, the 16-term sum of one
v_mfma_f32_32x32x16_f16 in fp32, against the fp64 product).

Gate: every case within 2^-21 of  m = sum_k |W_ik y_k| + |b_i|  -- the bound of the three-term split (hi.hi + hi.lo + lo.hi of two
11-bit roundings per factor), derived in the program's header, not measured.  It is asserted as it stands on weights and biases of
magnitude 2^-3 .. 2^3 (log-uniform, random signs; conditioning columns on the unit sphere), the domain in which every `lo` term the
derivation speaks of is a normal fp16 number or its factor is small.  Normal draws at three scales, which include values whose `lo` is an
fp16 subnormal, are gated by the same bound with that floor written out: 2^-21 m + 2^-25 (sum_k (|W_ik| + |y_k|) + 1).

Measured over 200 000 cases each (max error / gate): band 0.88; normal draws 0.61 / 0.71 / 0.77 at scales 0.25 / 1 / 8."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_fc_first.cpp")
OUT = os.path.join(HERE, "csrc", "_host_fc_first")
HDR = os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", "fc_first.h")


@pytest.fixture(scope="module")
def program():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-mf16c", "-o", OUT, SRC], check=True)
    return OUT


def _run(program, mode, scale):
    run = subprocess.run([program, "7", "200000", mode, str(scale)], capture_output=True, text=True)
    print(run.stdout.strip())
    return run, json.loads(run.stdout)


def test_split_product_is_within_the_three_term_bound(program):
    run, res = _run(program, "band", 1.0)
    assert res["shape_ok"] == 1 and res["range_ok"] == 1
    assert res["nonfinite"] == 0 and res["over"] == 0 and res["max_rel"] <= 2.0 ** -21, res
    assert run.returncode == 0


@pytest.mark.parametrize("scale", [0.25, 1.0, 8.0])
def test_small_values_keep_the_bound_plus_the_subnormal_floor(program, scale):
    run, res = _run(program, "normal", scale)
    assert res["nonfinite"] == 0 and res["over"] == 0 and res["max_err_over_gate"] <= 1.0, res
    assert run.returncode == 0
