"""CPU: the reference's checkpoint path through the DEFAULT drop-in (``get_flow`` flattens the parameters).

Every reference entry point that loads a checkpoint (eval.py:23, eval_uncondition.py:21, train.py:49, train_uncondition.py:28) calls
``Agent.load_ckpt`` (agent.py:155-198), which loads the weights and then, unconditionally, the Adam state into a fresh
``optim.Adam(self.flow.parameters())``.  tests/agent_replay.py replays those statements.  Covered here, both directions:
  (a) a checkpoint the REFERENCE wrote (tests/golden/traj_c1_step10.pth: its own Flow + Adam, per-tensor optimizer state, written by
      make_trained.py with Agent.save_ckpt's statements) loads into the drop-in agent and is written back entry for entry;
  (b) a checkpoint the DROP-IN agent writes loads into a per-tensor implementation -- this repo's ``Flow(config)``, and a module laid out
      as the reference's own ``flow.flow.Flow`` (its ``get_flow`` is ``Flow(config)``): the parameter and state-dict names, order and
      shapes recorded from it in tests/golden/param_order.json -- and the next Adam step is the same arithmetic on both sides.
"""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from rotationnormflow_amd.configs import make_config
from rotationnormflow_amd.flow.flow import Flow, get_flow
from tests.agent_replay import ReplayedAgent
from tests.golden.trained_cases import TRAJ

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_CKPT = os.path.join(GOLDEN, "traj_c1_step10.pth")


def quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


def quiet_get_flow(cfg):
    return quiet(get_flow, cfg)


def classic_get_flow(cfg):
    return quiet(Flow, cfg)


def reference_get_flow():
    """A ``get_flow`` whose module has the reference Flow's per-tensor layout for the trajectory structure: every parameter under its
    dotted name, in the order the reference registers them (tests/golden/param_order.json, written by make_param_order.py from the
    reference's own ``Flow``).  The checkpoint path never runs the flow, so names, order and shapes are all of the reference it touches."""
    with open(os.path.join(GOLDEN, "param_order.json")) as fh:
        layout = json.load(fh)["traj_c1"]
    assert layout["cfg"] == TRAJ["traj_c1"]["cfg"]

    def build(cfg):
        root = torch.nn.Module()
        for name, shape in layout["parameters"]:
            *path, leaf = name.split(".")
            mod = root
            for part in path:
                if part not in mod._modules:
                    mod.add_module(part, torch.nn.Module())
                mod = mod._modules[part]
            mod.register_parameter(leaf, torch.nn.Parameter(torch.zeros(shape)))
        assert [[k, list(p.shape)] for k, p in root.named_parameters()] == layout["parameters"]
        assert [[k, list(v.shape)] for k, v in root.state_dict().items()] == layout["state_dict"]
        return root
    return build


def cfg_traj():
    return make_config(**TRAJ["traj_c1"]["cfg"])


def fake_gradient_step(agent, seed):
    """One optimizer step on seeded gradients (the kernels do not run on CPU): per state-dict key the same values on every implementation."""
    g = torch.Generator().manual_seed(seed)
    mod = agent.flow.module
    grads = {k: torch.randn(v.shape, generator=g) * 1e-2 for k, v in sorted(mod.state_dict().items())}
    if getattr(mod, "is_flat", False):
        flat = mod._parameters["_flat"]
        flat.grad = torch.zeros_like(flat)
        for k, view in mod.named_parameter_gradients().items():
            view.copy_(grads[k])
    else:
        for k, p in mod.named_parameters():
            p.grad = grads[k].clone()
    agent.optimizer_flow.step()


def test_reference_written_checkpoint_loads_through_the_default_dropin(tmp_path):
    ck = torch.load(REF_CKPT, map_location="cpu", weights_only=True)
    n_tensors = len(ck["flow_state_dict"])
    assert len(ck["optimizer_flow_state_dict"]["state"]) == n_tensors == len(ck["optimizer_flow_state_dict"]["param_groups"][0]["params"])
    agent = ReplayedAgent(cfg_traj(), quiet_get_flow, "cpu")
    assert agent.flow.module.is_flat and len(list(agent.flow.parameters())) == 1           # the default: ONE parameter
    agent.load_ckpt(REF_CKPT)                                                             # round 4: ValueError (parameter group size)
    assert agent.clock["iteration"] == 10
    # weights arrived, and the in-memory optimizer state is the concatenation of the reference's per-tensor entries
    sd = agent.flow.module.state_dict()
    for k, v in ck["flow_state_dict"].items():
        assert torch.equal(sd[k], v), k
    flat = agent.flow.module._parameters["_flat"]
    st = agent.optimizer_flow.state[flat]
    layout = agent.flow.module._flat_layout()
    order = [k for k, _, _ in layout]
    ref_state = ck["optimizer_flow_state_dict"]["state"]
    ref_keys = list(ck["flow_state_dict"].keys())                                           # parameters() order = state-dict order (no buffers here)
    assert order == ref_keys
    for name in ("exp_avg", "exp_avg_sq"):
        for i, (key, off, shape) in enumerate(layout):                                      # entry i of the reference = slice of tensor i
            assert tuple(ref_state[i][name].shape) == shape
            assert torch.equal(st[name][off:off + ref_state[i][name].numel()], ref_state[i][name].reshape(-1)), (key, name)
    assert float(st["step"]) == 10.0
    # ... and save_ckpt writes it back entry for entry (same keys, shapes, values, param_groups)
    agent.save_ckpt(tmp_path / "again.pth")
    again = torch.load(tmp_path / "again.pth", map_location="cpu", weights_only=True)
    a, b = again["optimizer_flow_state_dict"], ck["optimizer_flow_state_dict"]
    assert a["param_groups"][0]["params"] == b["param_groups"][0]["params"] == list(range(n_tensors))
    assert {k: v for k, v in a["param_groups"][0].items() if k != "params"} == {k: v for k, v in b["param_groups"][0].items() if k != "params"}
    for i in range(n_tensors):
        assert set(a["state"][i]) == set(b["state"][i])
        for name, v in b["state"][i].items():
            assert a["state"][i][name].shape == v.shape and torch.equal(a["state"][i][name], v), (i, name)
    assert list(again["flow_state_dict"]) == ref_keys


@pytest.mark.parametrize("target", ["classic", "reference"])
def test_dropin_written_checkpoint_resumes_in_a_per_tensor_implementation(tmp_path, target):
    other = classic_get_flow if target == "classic" else reference_get_flow()
    cfg = cfg_traj()
    src = ReplayedAgent(cfg, quiet_get_flow, "cpu")
    src.load_ckpt(REF_CKPT)
    fake_gradient_step(src, seed=5)                                                       # state the drop-in itself produced (step 11)
    src.clock["iteration"] += 1
    src.save_ckpt(tmp_path / "dropin.pth")
    dst = ReplayedAgent(cfg, other, "cpu")
    assert len(list(dst.flow.parameters())) == len(src.flow.module._flat_slots) > 1
    dst.load_ckpt(tmp_path / "dropin.pth")                                                # agent.py:171-198 on the other implementation
    assert dst.clock["iteration"] == 11
    # the NEXT step: flat Adam on one tensor == per-tensor Adam on its slices, bit for bit
    fake_gradient_step(src, seed=6)
    fake_gradient_step(dst, seed=6)
    a, b = src.flow.module.state_dict(), dst.flow.module.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    sa, sb = src.optimizer_flow.state_dict(), dst.optimizer_flow.state_dict()
    assert sa["param_groups"] == sb["param_groups"]
    for i in sb["state"]:
        for name, v in sb["state"][i].items():
            assert torch.equal(sa["state"][i][name], v), (i, name)
    # ... and the same checkpoint goes back into a drop-in agent (drop-in -> drop-in)
    back = ReplayedAgent(cfg, quiet_get_flow, "cpu")
    back.load_ckpt(tmp_path / "dropin.pth")
    fake_gradient_step(back, seed=6)
    for k, v in back.flow.module.state_dict().items():
        assert torch.equal(v, a[k]), k


def test_bridge_handles_fresh_optimizers_other_parameters_and_amsgrad(tmp_path):
    from rotationnormflow_amd import flatopt
    fl = quiet_get_flow(make_config(None, layers=2, segments=16))
    n = len(fl._flat_slots)
    # a fresh optimizer (no state yet): still the per-tensor numbering (agent.py:143 right after construction)
    opt = torch.optim.Adam(fl.parameters(), 1e-3)
    sd = opt.state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["params"] == list(range(n))
    torch.optim.Adam(fl.parameters(), 1e-3).load_state_dict(sd)
    # other parameters beside the flat one, two groups, amsgrad (a third per-element state tensor)
    extra, extra2 = torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 2))
    opt = torch.optim.Adam([{"params": [extra, fl._flat]}, {"params": [extra2], "lr": 1e-2}], 1e-3, amsgrad=True)
    for p in (extra, fl._flat, extra2):
        p.grad = torch.randn_like(p)
    opt.step()
    sd = opt.state_dict()
    assert sd["param_groups"][0]["params"] == list(range(n + 1)) and sd["param_groups"][1]["params"] == [n + 1]
    assert sd["state"][0]["exp_avg"].shape == (5,) and sd["state"][n + 1]["exp_avg"].shape == (2, 2)
    key0, off0, shape0 = fl._flat_layout()[0]
    assert sd["state"][1]["max_exp_avg_sq"].shape == shape0
    opt2 = torch.optim.Adam([{"params": [extra, fl._flat]}, {"params": [extra2], "lr": 1e-2}], 1e-3, amsgrad=True)
    opt2.load_state_dict(sd)
    for name in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        assert torch.equal(opt2.state[fl._flat][name], opt.state[fl._flat][name])
        assert torch.equal(opt2.state[extra2][name], opt.state[extra2][name])
    # named parameters (torch >= 2.6 keeps param_names in the state): the flat entry expands to the state-dict keys
    optn = torch.optim.SGD(fl.named_parameters(), 1e-3, momentum=0.9)
    fl._flat.grad = torch.randn_like(fl._flat)
    optn.step()
    sdn = optn.state_dict()
    assert sdn["param_groups"][0]["param_names"] == [k for k, _, _ in fl._flat_layout()]
    optn2 = torch.optim.SGD(fl.named_parameters(), 1e-3, momentum=0.9)
    optn2.load_state_dict(sdn)
    assert torch.equal(optn2.state[fl._flat]["momentum_buffer"], optn.state[fl._flat]["momentum_buffer"])
    # a state whose per-tensor step counters differ cannot ride on one tensor: refused with the way out named
    bad = opt.state_dict()
    bad["state"][3]["step"] = bad["state"][3]["step"] + 1
    with pytest.raises(ValueError, match="RNF_FLAT_PARAMS=0"):
        opt2.load_state_dict(bad)
    # a wrong-sized state is still torch's own error
    with pytest.raises(ValueError, match="parameter group"):
        torch.optim.Adam(fl.parameters(), 1e-3).load_state_dict(torch.optim.Adam([extra, extra2], 1e-3).state_dict())
    # copies of the module are tagged again (deepcopy builds new Parameter objects), optimizers over them are bridged too
    import copy
    clone = copy.deepcopy(fl)
    assert flatopt.layout_of(clone._flat) == flatopt.layout_of(fl._flat)
    assert torch.optim.Adam(clone.parameters(), 1e-3).state_dict()["param_groups"][0]["params"] == list(range(n))
    # RNF_FLAT_PARAMS=0 keeps per-tensor parameters and needs no bridge
    os.environ["RNF_FLAT_PARAMS"] = "0"
    try:
        plain = quiet_get_flow(make_config(None, layers=2, segments=16))
    finally:
        del os.environ["RNF_FLAT_PARAMS"]
    assert not plain.is_flat and len(list(plain.parameters())) == n
