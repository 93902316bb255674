"""GPU (-m gpu): fc_first of the lean forward split-precision kernels on ONE split-fp16 matrix step (csrc/fc_first.h,
csrc/flow_kernels.h Mlp<1>::first_tile_h), for x0 and for the residual, at every launch width.

Flows: the trained-like synthetic weights (synth.fill_state_dict, regime "trained"; 6 Moebius + 6 constant-affine layers, K = 64, the
stack of tests/test_gpu_lean_columns.py) and the reference-trained checkpoint tests/golden/trained_c2.pth (24 + 24 layers, K = 64: C2).  Launches of 65 rows (ragged, the 4-wave instantiation),
40 000 rows (8 waves) and 65 536 + 32 rows (16 waves, one ragged tile on a 256-CU device).  The fp64 oracle and its own fp32 run are
evaluated once per flow on 1 121 rows -- the first 65, the last 512 of the 40 000 and the last 544 of the large launch (its ragged tile
included) -- read from the LARGE launch; the small launches are held to those rows bit for bit (width independence).

Gates: tests/test_gpu_lean_columns.py::_forward_gates, unchanged, for the log-det and for log p with the matrix-Fisher base, and that
file's rotation gate; and the mean abs error of each quantity within the mean error of the oracle's fp32 run on the same rows.

Measured on these rows (abs error against the fp64 oracle: mean / p99 / max; profiles/r8/parity_fc_first.jsonl):
    flow, quantity        parent build                    this build                      oracle's own fp32 run
    synthetic6 rotation   1.43e-7 / 5.49e-7 / 1.35e-6     1.50e-7 / 5.77e-7 / 1.07e-6     2.97e-7 / 1.28e-6 / 2.07e-6
    synthetic6 log-det    5.88e-7 / 1.87e-6 / 3.00e-6     5.86e-7 / 2.04e-6 / 3.16e-6     8.56e-7 / 2.91e-6 / 5.47e-6
    synthetic6 log p      1.01e-6 / 3.99e-6 / 5.91e-6     1.05e-6 / 3.91e-6 / 5.97e-6     2.01e-6 / 7.75e-6 / 1.18e-5
    trained_c2 rotation   1.19e-7 / 6.97e-7 / 2.35e-6     1.23e-7 / 7.29e-7 / 3.00e-6     5.23e-7 / 3.41e-6 / 1.44e-5
    trained_c2 log-det    1.02e-6 / 3.37e-6 / 2.00e-5     1.01e-6 / 3.42e-6 / 2.38e-5     2.81e-6 / 1.42e-5 / 2.34e-5
    trained_c2 log p      1.16e-6 / 4.24e-6 / 2.48e-5     1.16e-6 / 5.05e-6 / 3.06e-5     3.70e-6 / 1.90e-5 / 5.00e-5
Both builds pass the gates on both flows.  (The synthetic weights on the 24 + 24-layer C2 stack are NOT a case of this file: there the
parent build itself misses the last clause of _forward_gates for log p -- p99 |got - fp32 oracle| 9.2e-5 against 8.2e-5 + 1e-5, this build
9.9e-5 -- because that clause allows the kernel 1e-5 of its own while both builds' p99 error against fp64 is 2 - 3e-5 on that stack, a
third of the fp32 oracle's 8.2e-5.  Its figures are in profiles/r8/parity_fc_first.jsonl: log p mean 2.78e-6 / 2.73e-6 / oracle fp32 7.69e-6.)

Range: one fc_first weight of 7e4 (splits into (inf, -inf); Mlp<1>::range_probe turns hidden layer 0's tested accumulator NaN) and one NaN rotation entry in the
column the first layer transforms (a NaN in the column it REWRITES is overwritten by a cross product, here as in the reference) -- the guard fires and the call
returns what the strict re-run arithmetic returns when asked for directly, as in tests/test_gpu_guard.py.  The packer's equalisation
and audit are switched off for the weight case (as test_gpu_guard.py's `unequalised` does): equalised, the row would be rescaled into
range before it reaches the kernel.  Both cases run at a 4-wave size and at 65 536 + 32 rows, the 16-wave instantiation."""
import functools

import numpy as np
import pytest
import torch

import rotationnormflow_amd as rnf
from oracle import flow_oracle as orc
from rotationnormflow_amd import make_config, runtime, synth
from rotationnormflow_amd.utils.fisher import MatrixFisherN
from tests.gpu_helpers import product_flow
from tests.test_gpu_lean_columns import _forward_gates

pytestmark = pytest.mark.gpu

N_BIG = 65_536 + 32
N_MID = 40_000
N_SMALL = 65
FISHER = "diag531"
ROWS = np.r_[0:N_SMALL, N_MID - 512:N_MID, N_BIG - 544:N_BIG]
FLOWS = ("synthetic6", "trained_c2")


def weights_of(name):
    if name == "synthetic6":
        cfg = make_config(None, layers=6, segments=64)
        return cfg, synth.fill_state_dict(orc.state_shapes(cfg), seed=2024, regime="trained")
    from tests.trained_helpers import load_trained
    cfg, _, w, _, _ = load_trained(name)
    return cfg, w


@functools.lru_cache(maxsize=None)
def rotations():
    R = synth.uniform_rotations(N_BIG, seed=77)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def reference(name):
    """fp64 and fp32 oracle on ROWS: (rotation, log-det, log p) each, read-only."""
    cfg, w = weights_of(name)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        Rw, lw = orc.flow_forward(cfg, w, rotations()[ROWS], None, dtype)
        fw = orc.fisher_log_prob(Rw, synth.fisher_A(FISHER), dtype)
        ref[dtype] = tuple(a.double().numpy() for a in (Rw, lw, lw + fw))
        for a in ref[dtype]:
            a.setflags(write=False)
    return ref


def launches(name):
    """{n: (rotation, log-det, log p)} on the CPU for the three launch sizes, with the library that is loaded now."""
    cfg, w = weights_of(name)
    fl = product_flow(cfg, w)
    R = torch.from_numpy(rotations().copy()).cuda()
    base = MatrixFisherN(torch.from_numpy(synth.fisher_A(FISHER)))
    out = {}
    with torch.no_grad():
        for n in (N_BIG, N_MID, N_SMALL):
            Rn = R[:n].contiguous()
            Rt, ldj = fl(Rn)
            lp = fl.log_prob(Rn, base=base)["logp"]
            out[n] = (Rt.cpu(), ldj.cpu(), lp.cpu())
    torch.cuda.synchronize()
    assert not runtime.fallback_fired(R.device)
    return out


def error_stats(name, out):
    """Per quantity: abs error of the large launch's ROWS against the fp64 oracle, and the oracle's own fp32 error."""
    ref = reference(name)
    stats = {}
    for i, q in enumerate(("rotation", "ldj", "logp")):
        got = out[N_BIG][i].double().numpy()[ROWS]
        err, noise = np.abs(got - ref[torch.float64][i]), np.abs(ref[torch.float32][i] - ref[torch.float64][i])
        stats[q] = {"mean": float(err.mean()), "p99": float(np.quantile(err, 0.99)), "max": float(err.max()),
                    "ref32_mean": float(noise.mean()), "ref32_p99": float(np.quantile(noise, 0.99)), "ref32_max": float(noise.max())}
    return stats


@pytest.fixture(scope="module", params=FLOWS)
def evaluated(request):
    return request.param, launches(request.param)


def test_log_det_and_rotation_match_the_oracle(evaluated):
    name, out = evaluated
    ref, st = reference(name), error_stats(name, out)
    print(name, st)
    Rt, ldj = out[N_BIG][0].double().numpy()[ROWS], out[N_BIG][1].double().numpy()[ROWS]
    R64, l64, _ = ref[torch.float64]
    R32, l32, _ = ref[torch.float32]
    _forward_gates(ldj, l64, l32)
    assert np.abs(Rt - R64).max() <= 4 * np.abs(R32 - R64).max() + 1e-5
    assert np.abs(np.einsum("nij,nkj->nik", Rt, Rt) - np.eye(3)).max() < 1e-5
    assert np.abs(np.linalg.det(Rt) - 1).max() < 1e-5
    assert st["ldj"]["mean"] <= st["ldj"]["ref32_mean"], st["ldj"]
    assert st["rotation"]["mean"] <= st["rotation"]["ref32_mean"], st["rotation"]


def test_log_prob_with_the_fisher_base_matches_the_oracle(evaluated):
    name, out = evaluated
    ref, st = reference(name), error_stats(name, out)
    _forward_gates(out[N_BIG][2].double().numpy()[ROWS], ref[torch.float64][2], ref[torch.float32][2])
    assert st["logp"]["mean"] <= st["logp"]["ref32_mean"], st["logp"]


@pytest.mark.parametrize("n", (N_SMALL, N_MID))
def test_a_rotation_does_not_depend_on_the_launch_width(evaluated, n):
    out = evaluated[1]
    for small, big in zip(out[n], out[N_BIG]):
        assert small.shape[0] == n and torch.equal(small, big[:n])


# ---- range ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def unequalised():
    from rotationnormflow_amd import _lib
    L = _lib.lib()
    eq, au = L.rnf_set_equalize(0), L.rnf_set_pack_audit(0)
    yield
    L.rnf_set_equalize(eq)
    L.rnf_set_pack_audit(au)


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _guarded_equals_strict(fl, R):
    assert rnf.get_precision() == "f16x2"
    with torch.no_grad():
        Rt, ldj = fl(R)
    assert fl._packed(R.device).precision == "f16x2"
    assert runtime.fallback_fired(R.device)
    rnf.set_precision(runtime._fallback_precision)
    try:
        with torch.no_grad():
            Rs, ls = fl(R)
    finally:
        rnf.set_precision("f16x2")
    assert _same(ldj, ls) and _same(Rt, Rs)
    return Rt, ldj


@pytest.mark.parametrize("n", (N_SMALL, 3000, N_BIG))
def test_an_fc_first_weight_beyond_the_fp16_range_falls_back(unequalised, n):
    cfg = make_config(layers=3, segments=16)
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=5, regime="trained")
    key = sorted(k for k in w if k.endswith("conditioner.fc_first.weight"))[1]
    v = w[key].copy()
    v[17, 1] = 7.0e4
    w[key] = v
    R = torch.from_numpy(synth.uniform_rotations(n, seed=11)).cuda()
    Rt, ldj = _guarded_equals_strict(product_flow(cfg, w), R)
    assert torch.isfinite(ldj).all() and torch.isfinite(Rt).all()
    _, lw = orc.flow_forward(cfg, w, R.cpu().numpy(), None, dtype=torch.float64)
    err = np.abs(ldj.cpu().double().numpy() - lw.numpy())
    assert np.median(err) < 1e-4 and np.quantile(err, 0.99) < 2e-2, (np.median(err), err.max())


@pytest.mark.parametrize("n", (3000, N_BIG))
def test_a_nan_rotation_falls_back_and_stays_with_its_own_sample(n):
    cfg = make_config(layers=3, segments=16)
    w = synth.fill_state_dict(orc.state_shapes(cfg), seed=5, regime="trained")
    Rn = synth.uniform_rotations(n, seed=11).copy()
    Rn[41, 1, 0] = np.nan
    R = torch.from_numpy(Rn).cuda()
    Rt, ldj = _guarded_equals_strict(product_flow(cfg, w), R)
    bad = torch.zeros(n, dtype=torch.bool, device="cuda")
    bad[41] = True
    assert torch.isnan(ldj[bad]).all() and torch.isfinite(ldj[~bad]).all() and torch.isfinite(Rt[~bad]).all()
