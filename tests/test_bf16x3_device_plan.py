"""CPU: the device-packed paths keep the selected bf16x3 arithmetic, and the training layer table lays out bf16x3 records exactly where the
host packers put them (no GPU needed: the host packers and the layer table are host code)."""
import contextlib
import io

import numpy as np
import pytest
import torch

from oracle import flow_oracle as orc
from rotationnormflow_amd import _lib, autograd, runtime, synth
from rotationnormflow_amd.flow.flow import Flow


@contextlib.contextmanager
def _precision(name):
    old = runtime.get_precision()
    runtime.set_precision(name)
    try:
        yield
    finally:
        runtime.set_precision(old)


def test_device_precision_is_the_selected_precision():
    old = runtime.get_precision()
    for name in ("bf16x3", "fp32", "f16x2"):
        with _precision(name):
            assert runtime.device_precision() == name
    assert runtime.get_precision() == old


CASES = {
    "uncond_k64": dict(layers=3, segments=64),
    "uncond_k20": dict(layers=2, segments=20),
    "cond_f256": dict(layers=2, segments=16, condition=1, feature_dim=256),
    "cond_f20_first_affine": dict(layers=2, segments=16, condition=1, feature_dim=20, last_affine=1),
    "cond9": dict(layers=2, segments=16, condition=1, feature_dim=24, rot="9TransLSmith"),
    "cond36": dict(layers=2, segments=16, condition=1, feature_dim=24, rot="36Trans", last_affine=1),
    "lu": dict(layers=2, segments=16, lu=1),
    "rot": dict(layers=2, segments=16, rot="UnRot"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_train_plan_lays_out_bf16x3_records_like_the_host_packer(name):
    cfg = orc.make_config(**CASES[name])
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=7, regime="trained")
    with contextlib.redirect_stdout(io.StringIO()):
        fl = Flow(cfg)
    fl.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    layers, rows = list(fl.layers), fl._forward_rows()
    host = runtime.pack_layers(layers, rows, "cpu", "bf16x3")
    plan = autograd.TrainPlan(layers, rows, torch.device("cpu"), "bf16x3")
    assert plan.prec == _lib.PREC_BF16X3
    assert np.array_equal(plan.desc[:, :6], host.desc[:, :6])          # same record offsets, same precision column
    assert plan.blob_floats == host.blob.numel()
    # no fallback images behind a bf16x3 blob (the range guard belongs to f16x2)
    assert np.array_equal(autograd.desc_with_fallback(plan), plan.desc)
