"""Top-k pose modes on the SO(3) grid (rnf_grid_modes, harness.grid_pose_modes), CPU part: an fp64 numpy restatement of the reduction
that tests/test_gpu_grid_modes.py checks the device against, pinned here on hand-built inputs; the C ABI's refusals, which happen before
any launch; and the argument checks of the Python entry points."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib, harness, make_config
from rotationnormflow_amd.flow.flow import Flow
from tests.test_so3_grid import healpix_grid_fp64


def grid_modes_fp64(lp, grid, k, sep, gt=None):
    """fp64 restatement of rnf_grid_modes (include/rnf_hip.h).  lp [g,Q] (or [Q]), grid [Q,3,3] (the float32 rows the device reads),
    sep in radians, gt [g,K,3,3] or None.  -> dict(index [g,k], log_prob [g,k], mass [g,k], log_norm [g], spread [g] or None)"""
    lp = np.atleast_2d(np.asarray(lp, np.float64))
    g, Q = lp.shape
    R = np.asarray(grid, np.float64).reshape(Q, 9)
    thr = -np.inf if sep >= np.pi else float(np.float32(1.0 + 2.0 * np.cos(sep)))
    out = dict(index=np.full((g, k), -1, np.int64), log_prob=np.full((g, k), -np.inf), mass=np.zeros((g, k)), log_norm=np.zeros(g),
               spread=None if gt is None else np.zeros(g))
    for b in range(g):
        row = lp[b]
        region = np.full(Q, -1)                           # the first mode a row is within sep of
        i0 = int(np.argmax(row))                          # numpy, like torch: the first maximum, a NaN wins
        modes = [i0]
        if not np.isnan(row[i0]):
            for j in range(1, k):
                region[(region < 0) & (R @ R[modes[-1]] > thr)] = j - 1
                free = np.flatnonzero(region < 0)
                if free.size == 0:
                    break
                modes.append(int(free[np.argmax(row[free])]))
            if len(modes) == k:
                region[(region < 0) & (R @ R[modes[-1]] > thr)] = k - 1
        out["index"][b, :len(modes)] = modes
        out["log_prob"][b, :len(modes)] = row[modes]
        M = row[i0]
        if np.isnan(M):
            out["mass"][b] = np.nan
            out["log_norm"][b] = np.nan
            if gt is not None:
                out["spread"][b] = np.nan
            continue
        w = np.zeros(Q) if M == -np.inf else np.exp(row - M)
        S = w.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            out["log_norm"][b] = M + np.log(S) - np.log(Q)
            for j in range(len(modes)):
                out["mass"][b, j] = w[region == j].sum() / S
            if gt is not None:
                G = np.asarray(gt[b], np.float64).reshape(-1, 9)
                ang = np.arccos(np.clip(((R @ G.T).max(1) - 1) / 2, -1, 1))
                out["spread"][b] = (w * ang).sum() / S
    return out


def _grid(level=1, seed=0):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    O = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return healpix_grid_fp64(level, offset=O).astype(np.float32)


def _geodesic(a, b):
    return np.arccos(np.clip((np.einsum("ij,ij", a.astype(np.float64), b.astype(np.float64)) - 1) / 2, -1, 1))


def test_ties_resolve_to_the_first_index():
    grid = _grid()
    lp = np.zeros(grid.shape[0])
    lp[[17, 40, 300]] = 2.0
    r = grid_modes_fp64(lp, grid, 3, np.deg2rad(1.0))
    assert r["index"][0, 0] == 17 and r["index"][0, 1] == 40 and r["index"][0, 2] == 300
    assert np.all(r["log_prob"][0] == 2.0)
    flat = grid_modes_fp64(np.zeros(grid.shape[0]), grid, 1, np.deg2rad(10.0))
    assert flat["index"][0, 0] == 0 and abs(flat["log_norm"][0]) < 1e-12


def test_minus_infinity_entries_carry_no_mass():
    grid = _grid()
    Q = grid.shape[0]
    lp = np.full(Q, -np.inf)
    lp[[5, 200]] = [1.0, 0.5]
    r = grid_modes_fp64(lp, grid, 4, np.deg2rad(5.0))
    assert list(r["index"][0, :2]) == [5, 200]
    assert np.isclose(r["log_norm"][0], np.log((np.e + np.exp(0.5)) / Q))
    assert np.isclose(r["mass"][0, :2].sum(), 1.0) and np.isclose(r["mass"][0, 0], np.e / (np.e + np.exp(0.5)))
    assert np.all(r["log_prob"][0, 2:] == -np.inf) and np.all(r["mass"][0, 2:] == 0)   # -inf rows still qualify as modes
    assert np.all(r["index"][0, 2:] >= 0)
    none = grid_modes_fp64(np.full(Q, -np.inf), grid, 2, np.deg2rad(5.0))              # no finite value: -inf, NaN masses
    assert none["index"][0, 0] == 0 and none["log_norm"][0] == -np.inf and np.isnan(none["mass"][0]).all()


def test_a_nan_row_gives_the_nan_semantics():
    grid = _grid()
    Q = grid.shape[0]
    gt = grid[None, None, :1]
    lp = np.linspace(0, 1, Q)
    lp[[30, 90]] = np.nan
    r = grid_modes_fp64(lp, grid, 3, np.deg2rad(10.0), gt=gt)
    assert r["index"][0, 0] == 30 and np.isnan(r["log_prob"][0, 0])
    assert list(r["index"][0, 1:]) == [-1, -1] and np.all(r["log_prob"][0, 1:] == -np.inf)
    assert np.isnan(r["mass"][0]).all() and np.isnan(r["log_norm"][0]) and np.isnan(r["spread"][0])


def test_separation_pi_leaves_only_mode_zero():
    grid = _grid(seed=3)
    lp = np.random.default_rng(1).normal(size=grid.shape[0])
    r = grid_modes_fp64(lp, grid, 4, np.pi)
    assert r["index"][0, 0] == np.argmax(lp) and list(r["index"][0, 1:]) == [-1, -1, -1]
    assert np.isclose(r["mass"][0, 0], 1.0) and np.all(r["mass"][0, 1:] == 0)


def test_two_peak_masses_add_up_to_the_peaks():
    grid = _grid(level=2, seed=4)
    Q = grid.shape[0]
    R = grid.reshape(Q, 9).astype(np.float64)
    a, b = 100, int(np.argmin(R @ R[100]))                 # two grid points about 180 degrees apart
    lp = np.log(0.7 * np.exp(40 * (R @ R[a] - 3)) + 0.3 * np.exp(40 * (R @ R[b] - 3)) + 1e-30)
    sep = np.deg2rad(60.0)
    r = grid_modes_fp64(lp, grid, 3, sep, gt=np.stack([grid[a], grid[b]])[None])
    assert list(r["index"][0, :2]) == [a, b]
    w = np.exp(lp - lp.max())
    near = lambda i: R @ R[i] > 1 + 2 * np.cos(sep)        # noqa: E731
    assert np.isclose(r["mass"][0, 0], w[near(a)].sum() / w.sum()) and np.isclose(r["mass"][0, 1], w[near(b)].sum() / w.sum())
    assert np.isclose(r["mass"][0, :2].sum(), w[near(a) | near(b)].sum() / w.sum())
    assert r["mass"][0, :2].sum() > 0.99 and r["mass"][0, 2] < 0.01 and r["mass"][0].sum() <= 1 + 1e-12
    assert abs(r["mass"][0, 0] - 0.7) < 0.02 and abs(r["mass"][0, 1] - 0.3) < 0.02
    ang = np.array([min(_geodesic(grid[i], grid[a]), _geodesic(grid[i], grid[b])) for i in range(Q)])
    assert np.isclose(r["spread"][0], (w * ang).sum() / w.sum())


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20                                          # a 16-byte-aligned address that is never read


def _args(**kw):
    base = dict(logp=_FAKE, grid=_FAKE, Q=4608, g=3, top_k=4, separation_rad=0.25, index_out=_FAKE, logp_out=_FAKE, mass_out=_FAKE,
                log_norm_out=_FAKE)
    base.update(kw)
    a = _lib.GridModes(**base)
    need = _lib.lib().rnf_grid_modes_workspace_bytes(ctypes.byref(a))
    a.workspace, a.workspace_bytes = _FAKE, need
    return a


def _refused(a, word):
    L = _lib.lib()
    assert L.rnf_grid_modes(ctypes.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def test_workspace_follows_the_documented_rule():
    L = _lib.lib()
    for Q, g, k in [(1, 1, 1), (576, 128, 4), (2047, 2, 16), (2049, 5, 2), (72 * 8 ** 5, 16, 4), (72 * 8 ** 6, 1, 2), (72 * 8 ** 8, 1, 16)]:
        a = _lib.GridModes(Q=Q, g=g, top_k=k)
        want = g * min(-(-Q // 2048), 2048) * 8 * (k + 2)
        assert L.rnf_grid_modes_workspace_bytes(ctypes.byref(a)) == want, (Q, g, k)
    assert L.rnf_grid_modes_workspace_bytes(ctypes.byref(_lib.GridModes(Q=10, g=1, top_k=17))) == 0
    assert L.rnf_grid_modes_workspace_bytes(ctypes.byref(_lib.GridModes(Q=0, g=1, top_k=1))) == 0
    assert L.rnf_grid_modes_workspace_bytes(ctypes.byref(_lib.GridModes(Q=10, g=0, top_k=1))) == 0
    bad = _lib.GridModes(Q=10, g=1, top_k=1)
    bad.struct_bytes -= 8
    assert L.rnf_grid_modes_workspace_bytes(ctypes.byref(bad)) == 0


def test_c_abi_refuses_bad_arguments_before_any_launch():
    _refused(_args(top_k=0), "top_k")
    _refused(_args(top_k=17), "top_k")
    _refused(_args(separation_rad=0.0), "separation_rad")
    _refused(_args(separation_rad=-0.1), "separation_rad")
    _refused(_args(separation_rad=np.pi + 1e-9), "separation_rad")
    _refused(_args(Q=0), "Q=")
    _refused(_args(g=0), "g=")
    _refused(_args(logp=None), "null")
    _refused(_args(mass_out=None), "null")
    _refused(_args(grid=_FAKE + 4), "aligned")
    _refused(_args(gt=_FAKE, n_gt=0, spread_out=_FAKE), "n_gt")
    _refused(_args(gt=_FAKE, n_gt=129, spread_out=_FAKE), "n_gt")
    _refused(_args(gt=_FAKE, n_gt=2), "spread_out")
    a = _args()
    a.workspace_bytes -= 1
    _refused(a, "workspace")
    a = _args()
    a.workspace = None
    _refused(a, "workspace")
    a = _args()
    a.struct_bytes += 8
    _refused(a, "struct_bytes")


def test_header_declares_the_struct_the_binding_mirrors():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    body = header[header.index("typedef struct RnfGridModes {") + 29:header.index("} RnfGridModes;")]
    names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
    assert names == [f for f, _ in _lib.GridModes._fields_], names
    assert {"rnf_grid_modes", "rnf_grid_modes_workspace_bytes"} <= set(_lib.EXPORTS)


# ---- Python entry points: argument checks run before anything touches a device ----------------------------------------------------------
def _cpu_flow():
    with contextlib.redirect_stdout(io.StringIO()):
        return Flow(make_config(layers=2, condition=1, feature_dim=16, rot="16Trans"))


def test_python_entry_points_validate_their_arguments():
    fl = _cpu_flow()
    feat = torch.zeros(2, 16)
    gt = torch.eye(3).expand(2, 3, 3)
    with pytest.raises(ValueError, match="top_k"):
        harness.pose_accuracy(fl, feat, gt, method="log_inv", top_k=2)
    with pytest.raises(ValueError, match="top_k"):
        harness.pose_accuracy(fl, feat, gt, method="log_pdf", top_k=0)
    with pytest.raises(ValueError, match="separation_deg"):
        harness.grid_pose_modes(fl, feat, separation_deg=0)
    with pytest.raises(ValueError, match="separation_deg"):
        harness.grid_pose_modes(fl, feat, separation_deg=181)
    with pytest.raises(ValueError, match="top_k"):
        harness.grid_pose_modes(fl, feat, top_k=17)
    with pytest.raises(RuntimeError, match="GPU only"):                 # valid arguments on CPU tensors: no CPU fallback
        harness.grid_pose_modes(fl, feat, top_k=2, recursion_level=0)
