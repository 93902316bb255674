"""Credible sets on the SO(3) grid (rnf_grid_credible, harness.grid_pose_credible), CPU part: an fp64 numpy restatement with real-valued
weights (sort, cumulative sum, no fixed point), pinned here on hand-built rows; the checking function and the seeded generator of synthetic
log p rows that tests/test_gpu_grid_credible.py shares; the C ABI's refusals, which happen before any launch; and the argument checks of
the Python entry points."""
import contextlib
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib, harness, make_config
from rotationnormflow_amd.flow.flow import Flow
from tests.test_so3_grid import healpix_grid_fp64

LEVELS3 = (0.5, 0.9, 0.95)
LEVELS8 = (0.05, 0.1, 0.25, 0.5, 0.68, 0.9, 0.95, 0.99)
FULL_GRID_CASES = [(2, 5), (3, 1), (3, 5)]            # (level, images) of the full-grid cases the device is held to 90 % exact on


def eps_fix(Q):
    """The fixed point's bound on any reported mass fraction: Q 2^-(S+1) with S = 62 - ceil(log2 Q) (include/rnf_hip.h)."""
    S = 62 - int(np.ceil(np.log2(Q))) if Q > 1 else 62
    return Q * 2.0 ** -(S + 1)


def eps_for(Q):
    """eps_fix(Q) + 2^-20: the second term covers the fp32 exponential and the rounding of the fp32 outputs (derived, not measured)."""
    return eps_fix(Q) + 2.0 ** -20


def _weights(row):
    """(w [Q] fp64 relative to the maximum, kind): kind 'nan' (a NaN, or a +inf maximum), 'empty' (no finite value) or 'ok'."""
    row = np.asarray(row, np.float64)
    if np.isnan(row).any() or row.max() == np.inf:
        return None, "nan"
    if row.max() == -np.inf:
        return None, "empty"
    return np.exp(row - row.max()), "ok"


def grid_credible_fp64(lp, levels, queries=None):
    """fp64 restatement of rnf_grid_credible with true real-valued weights.  lp [g,Q] (or [Q]), levels [J], queries [g,G] or None.
    -> dict(threshold [g,J], count [g,J] int64, mass [g,J], log_norm [g], query_mass [g,G], query_count [g,G] int64 (None without queries))"""
    lp = np.atleast_2d(np.asarray(lp, np.float64))
    g, Q = lp.shape
    J = len(levels)
    qs = None if queries is None else np.asarray(queries, np.float64).reshape(g, -1)
    out = dict(threshold=np.full((g, J), np.nan), count=np.full((g, J), -1, np.int64), mass=np.full((g, J), np.nan),
               log_norm=np.full(g, np.nan), query_mass=None if qs is None else np.full(qs.shape, np.nan),
               query_count=None if qs is None else np.full(qs.shape, -1, np.int64))
    for b in range(g):
        row = lp[b]
        w, kind = _weights(row)
        if kind != "ok":
            out["log_norm"][b] = np.nan if kind == "nan" else -np.inf
            continue
        order = np.argsort(-row, kind="stable")
        v, cw = row[order], np.cumsum(w[order])
        ends = np.flatnonzero(np.r_[v[1:] != v[:-1], True])        # the last cell of every group of tied values (-0 == +0)
        F = cw[ends] / cw[-1]
        out["log_norm"][b] = row.max() + np.log(cw[-1]) - np.log(Q)
        for j, a in enumerate(levels):
            k = int(np.searchsorted(F, a, side="left"))            # the first (largest) value whose set reaches alpha
            out["threshold"][b, j] = v[ends[k]] + 0.0              # a zero threshold is +0
            out["count"][b, j] = ends[k] + 1
            out["mass"][b, j] = F[k]
        if qs is not None:
            for q, x in enumerate(qs[b]):
                if not np.isnan(x):
                    out["query_mass"][b, q] = w[row > x].sum() / cw[-1]
                    out["query_count"][b, q] = int((row > x).sum())
    return out


def set_mass(row, tau):
    """(F(tau), F+(tau)) = the mass fractions of {lp >= tau} and {lp > tau}, in fp64 with real-valued weights."""
    row = np.asarray(row, np.float64)
    w, kind = _weights(row)
    assert kind == "ok"
    return w[row >= tau].sum() / w.sum(), w[row > tau].sum() / w.sum()


def check_credible(row, alpha, tau, n, mu, eps=None):
    """What a device result (tau, n, mu) for one image and level must satisfy."""
    row32 = np.asarray(row, np.float32)
    eps = eps_for(row32.size) if eps is None else eps
    tau = np.float32(tau)
    canon = (row32 + np.float32(0)).view(np.uint32)                # -0 -> +0: a zero threshold is reported as +0
    assert np.float32(tau).view(np.uint32) in canon, f"threshold {tau!r} is not one of the image's values"
    F, Fp = set_mass(row32, float(tau))
    assert int(n) == int((row32 >= tau).sum()), (int(n), int((row32 >= tau).sum()))
    assert F >= alpha - eps, (F, alpha)
    assert Fp < alpha + eps, (Fp, alpha)
    assert abs(float(mu) - F) <= eps, (float(mu), F)


def check_query(row, v, query_mass, query_count, eps=None):
    row32 = np.asarray(row, np.float32)
    eps = eps_for(row32.size) if eps is None else eps
    Fp = set_mass(row32, float(np.float32(v)))[1]
    assert int(query_count) == int((row32 > np.float32(v)).sum())
    assert abs(float(query_mass) - Fp) <= eps, (float(query_mass), Fp)


def is_exact(row, alpha, tau_ref, eps=None):
    """The checker's own threshold is at least eps away from the level on both sides: the device must then return the same value."""
    eps = eps_for(np.asarray(row).size) if eps is None else eps
    F, Fp = set_mass(np.asarray(row, np.float32), float(tau_ref))
    return abs(F - alpha) > eps and abs(Fp - alpha) > eps


def check_against_reference(lp, levels, got, queries=None, min_exact=None):
    """Every (image, level) of the device outputs ``got`` (the tuple of harness.grid_credible, as numpy) passes check_credible, the exact
    cases are bit-equal to the checker's threshold, and at least ``min_exact`` of the cases are exact.  Returns the exact fraction."""
    lp = np.atleast_2d(np.asarray(lp, np.float32))
    ref = grid_credible_fp64(lp, levels, queries)
    thr, cnt, mass, log_norm, qm, qc = got
    exact = 0
    for b in range(lp.shape[0]):
        for j, a in enumerate(levels):
            check_credible(lp[b], a, thr[b, j], cnt[b, j], mass[b, j])
            if is_exact(lp[b], a, ref["threshold"][b, j]):
                exact += 1
                assert np.float32(thr[b, j]).view(np.uint32) == np.float32(ref["threshold"][b, j]).view(np.uint32), (b, j)
                assert int(cnt[b, j]) == int(ref["count"][b, j]), (b, j)
        if queries is not None:
            for q in range(np.asarray(queries).reshape(lp.shape[0], -1).shape[1]):
                check_query(lp[b], np.asarray(queries).reshape(lp.shape[0], -1)[b, q], qm[b, q], qc[b, q])
    assert np.abs(np.asarray(log_norm, np.float64) - ref["log_norm"]).max() < 2e-6
    frac = exact / (lp.shape[0] * len(levels))
    if min_exact is not None:
        assert frac >= min_exact, frac
    return frac


@functools.lru_cache(maxsize=None)
def numpy_grid(level):
    return healpix_grid_fp64(level).astype(np.float32)


def synthetic_logp(grid, g, seed):
    """g seeded rows of a two-component Fisher-like log-density on ``grid`` [Q,3,3] plus noise, normalised so that log_norm is about 0.
    -> float32 [g,Q]"""
    rng = np.random.default_rng(seed)
    R = np.asarray(grid, np.float64).reshape(-1, 9)
    Q = R.shape[0]
    out = np.empty((g, Q), np.float32)
    for b in range(g):
        a, c = rng.integers(0, Q, 2)
        k1, k2 = rng.uniform(10.0, 30.0, 2)            # peaks sharp enough that the 0.99 set ends where cells still weigh > eps
        mix = rng.uniform(0.3, 0.7)
        dens = mix * np.exp(k1 * (R @ R[a] - 3.0)) + (1 - mix) * np.exp(k2 * (R @ R[c] - 3.0)) + 1e-30
        lp = np.log(dens) + 0.05 * rng.standard_normal(Q)
        out[b] = (lp - np.log(np.exp(lp).mean())).astype(np.float32)
    return out


def synthetic_queries(lp, G, seed):
    """G query values per image: the image's maximum, -inf, some of its own values and values between them.  -> float32 [g,G]"""
    rng = np.random.default_rng(seed)
    g, Q = lp.shape
    q = np.empty((g, G), np.float32)
    for b in range(g):
        own = lp[b, rng.integers(0, Q, G)]
        q[b] = np.where(rng.random(G) < 0.5, own, own + np.float32(0.01) * rng.standard_normal(G).astype(np.float32))
        q[b, 0] = lp[b].max()
        if G > 1:
            q[b, 1] = -np.inf
    return q


# ---- the checker on hand-built rows -------------------------------------------------------------------------------------------------------
def test_a_constant_row_is_one_set():
    r = grid_credible_fp64(np.full(37, 1.5), LEVELS8, queries=[[1.5, 1.0]])
    assert np.all(r["count"] == 37) and np.all(r["mass"] == 1.0) and np.all(r["threshold"] == 1.5)
    assert np.isclose(r["log_norm"][0], 1.5)
    assert r["query_mass"][0, 0] == 0 and r["query_count"][0, 0] == 0
    assert r["query_mass"][0, 1] == 1 and r["query_count"][0, 1] == 37


def test_two_valued_row_by_hand():
    n1, Q = 2, 20                                           # 2 cells of weight 1, 18 of weight 1/9: the dense cells hold half the mass
    lp = np.full(Q, -np.log(9.0))
    lp[[3, 11]] = 0.0
    r = grid_credible_fp64(lp, (0.2, 0.3, 0.7, 0.99))
    assert list(r["count"][0]) == [n1, n1, Q, Q]
    assert list(r["threshold"][0]) == [0.0, 0.0, -np.log(9.0), -np.log(9.0)]
    assert np.allclose(r["mass"][0], [0.5, 0.5, 1.0, 1.0])
    assert np.isclose(r["log_norm"][0], np.log(4.0 / Q))
    edge = float(r["mass"][0, 0])                           # a level exactly on the boundary: the dense cells suffice, one ulp more needs all
    on = grid_credible_fp64(lp, (edge, np.nextafter(edge, 1.0)))
    assert list(on["count"][0]) == [n1, Q] and list(on["threshold"][0]) == [0.0, -np.log(9.0)]
    q = grid_credible_fp64(lp, (0.5,), queries=[[0.0, -1.0, -np.log(9.0), -5.0]])
    assert list(q["query_count"][0]) == [0, n1, n1, Q]
    assert np.allclose(q["query_mass"][0], [0.0, 0.5, 0.5, 1.0])


def test_a_single_cell():
    r = grid_credible_fp64(np.array([-3.25]), (0.01, 0.5, 0.99), queries=[[-3.25, -4.0]])
    assert np.all(r["count"] == 1) and np.all(r["mass"] == 1.0) and np.all(r["threshold"] == -3.25)
    assert r["log_norm"][0] == -3.25
    assert list(r["query_count"][0]) == [0, 1] and list(r["query_mass"][0]) == [0.0, 1.0]


def test_minus_infinity_cells_are_never_inside():
    lp = np.full(50, -np.inf)
    lp[[4, 9, 30]] = [0.0, np.log(0.5), np.log(0.25)]
    r = grid_credible_fp64(lp, (0.5, 0.6, 0.9, 0.999), queries=[[-np.inf, np.log(0.25)]])
    assert list(r["count"][0]) == [1, 2, 3, 3]
    assert np.allclose(r["mass"][0], [4 / 7, 6 / 7, 1.0, 1.0])
    assert r["threshold"][0, 3] == np.log(0.25)
    assert r["query_count"][0, 0] == 3 and r["query_mass"][0, 0] == 1.0
    assert r["query_count"][0, 1] == 2 and np.isclose(r["query_mass"][0, 1], 6 / 7)


def test_zeros_of_either_sign_tie():
    lp = np.array([-1.0, -0.0, 0.0, -2.0, 0.0, -0.0])
    r = grid_credible_fp64(lp, (0.1, 0.8), queries=[[0.0, -0.0]])
    assert r["count"][0, 0] == 4 and r["threshold"][0, 0] == 0.0 and not np.signbit(r["threshold"][0, 0])
    assert list(r["query_count"][0]) == [0, 0]
    check_credible(lp, 0.1, 0.0, 4, r["mass"][0, 0])


def test_nan_and_empty_rows():
    lp = np.linspace(-3, 0, 40)
    bad = lp.copy()
    bad[7] = np.nan
    inf = lp.copy()
    inf[2] = np.inf
    r = grid_credible_fp64(np.stack([lp, bad, inf, np.full(40, -np.inf)]), LEVELS3, queries=np.zeros((4, 2)))
    assert np.all(r["count"][0] > 0) and np.isfinite(r["log_norm"][0])
    for b in (1, 2, 3):
        assert np.all(r["count"][b] == -1) and np.isnan(r["mass"][b]).all() and np.isnan(r["threshold"][b]).all()
        assert np.isnan(r["query_mass"][b]).all() and np.all(r["query_count"][b] == -1)
    assert np.isnan(r["log_norm"][1]) and np.isnan(r["log_norm"][2]) and r["log_norm"][3] == -np.inf
    q = grid_credible_fp64(lp, LEVELS3, queries=[[np.nan, -1.0]])
    assert np.isnan(q["query_mass"][0, 0]) and q["query_count"][0, 0] == -1 and q["query_count"][0, 1] > 0


def test_checker_results_pass_the_checking_function():
    lp = synthetic_logp(numpy_grid(1), 3, seed=5)
    qs = synthetic_queries(lp, 4, seed=6)
    r = grid_credible_fp64(lp, LEVELS8, qs)
    got = (r["threshold"], r["count"], r["mass"], r["log_norm"], r["query_mass"], r["query_count"])
    assert check_against_reference(lp, LEVELS8, got, qs) > 0.9
    assert np.all(np.diff(r["threshold"], axis=1) <= 0) and np.all(np.diff(r["count"], axis=1) >= 0)
    with pytest.raises(AssertionError):                     # one cell too many is caught
        check_credible(lp[0], 0.5, r["threshold"][0, 2], r["count"][0, 2] + 1, r["mass"][0, 2])
    with pytest.raises(AssertionError):                     # and so is the next value down
        nxt = np.sort(lp[0][lp[0] < np.float32(r["threshold"][0, 2])])[-1]
        F = set_mass(lp[0], float(nxt))[0]
        check_credible(lp[0], 0.5, nxt, (lp[0] >= nxt).sum(), F)


def case_seed(level, g):
    return level * 100 + g


@pytest.mark.parametrize("level,g", FULL_GRID_CASES)
def test_the_generator_makes_nine_cases_in_ten_exact(level, g):
    lp = synthetic_logp(numpy_grid(level), g, seed=case_seed(level, g))
    ref = grid_credible_fp64(lp, LEVELS8)
    exact = [is_exact(lp[b], a, ref["threshold"][b, j]) for b in range(g) for j, a in enumerate(LEVELS8)]
    assert np.mean(exact) >= 0.9
    assert np.abs(ref["log_norm"]).max() < 1e-3


def test_fixed_point_bound_values():
    assert eps_fix(72 * 8 ** 5) == 72 * 8 ** 5 * 2.0 ** -41 and 1.0e-6 < eps_fix(72 * 8 ** 5) < 1.9e-6      # level 5: S = 40
    assert eps_fix(72 * 8 ** 6) == 72 * 8 ** 6 * 2.0 ** -38 and 6.0e-5 < eps_fix(72 * 8 ** 6) < 1.2e-4      # level 6: S = 37
    assert eps_fix(1) == 2.0 ** -63 and eps_fix(2) == 2.0 ** -61 and eps_fix(3) == 3 * 2.0 ** -61


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20                                          # an aligned address that is never read


def _args(levels=LEVELS3, **kw):
    host = (ctypes.c_double * max(len(levels), 1))(*levels)
    base = dict(logp=_FAKE, Q=4608, g=3, levels=ctypes.addressof(host), n_levels=len(levels), threshold_out=_FAKE, count_out=_FAKE,
                mass_out=_FAKE, log_norm_out=_FAKE)
    base.update(kw)
    a = _lib.GridCredible(**base)
    a._keep = host
    need = _lib.lib().rnf_grid_credible_workspace_bytes(ctypes.byref(a))
    a.workspace, a.workspace_bytes = _FAKE, need
    return a


def _refused(a, word):
    L = _lib.lib()
    assert L.rnf_grid_credible(ctypes.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def test_workspace_follows_the_documented_rule():
    L = _lib.lib()
    for Q, g, J, G in [(1, 1, 1, 0), (4608, 5, 8, 16), (8193, 2, 3, 1), (72 * 8 ** 5, 16, 3, 1), (72 * 8 ** 6, 1, 8, 16), (1 << 26, 1, 1, 0)]:
        nb = min(-(-Q // 8192), 512)
        want = g * (16 * min(-(-Q // 2048), 2048) + 20 + 128 * J + nb * (3072 * J + 12 * G))
        want = (want + 15) // 16 * 16
        a = _lib.GridCredible(Q=Q, g=g, n_levels=J, n_queries=G)
        assert L.rnf_grid_credible_workspace_bytes(ctypes.byref(a)) == want, (Q, g, J, G)
    for bad in (dict(Q=0), dict(Q=(1 << 26) + 1), dict(g=0), dict(g=65536), dict(n_levels=0), dict(n_levels=9), dict(n_queries=-1),
                dict(n_queries=17)):
        kw = dict(Q=10, g=1, n_levels=1, n_queries=0)
        kw.update(bad)
        assert L.rnf_grid_credible_workspace_bytes(ctypes.byref(_lib.GridCredible(**kw))) == 0, bad
    short = _lib.GridCredible(Q=10, g=1, n_levels=1)
    short.struct_bytes -= 8
    assert L.rnf_grid_credible_workspace_bytes(ctypes.byref(short)) == 0


def test_c_abi_refuses_bad_arguments_before_any_launch():
    _refused(_args(g=0), "g=")
    _refused(_args(g=65536), "g=")
    _refused(_args(Q=0), "Q=")
    _refused(_args(Q=(1 << 26) + 1), "Q=")
    _refused(_args(levels=()), "n_levels")
    _refused(_args(levels=(0.5,) * 9), "n_levels")
    _refused(_args(levels=(0.5, 0.0)), "levels[1]")
    _refused(_args(levels=(1.0,)), "levels[0]")
    _refused(_args(levels=(0.5, 0.9, float("nan"))), "levels[2]")
    _refused(_args(levels=(-0.1,)), "levels[0]")
    _refused(_args(n_queries=-1), "n_queries")
    _refused(_args(n_queries=17, queries=_FAKE, query_mass_out=_FAKE, query_count_out=_FAKE), "n_queries")
    _refused(_args(logp=None), "null")
    _refused(_args(levels=LEVELS3, threshold_out=None), "null")
    _refused(_args(count_out=None), "null")
    _refused(_args(mass_out=None), "null")
    _refused(_args(log_norm_out=None), "null")
    _refused(_args(n_queries=2, query_mass_out=_FAKE, query_count_out=_FAKE), "queries")
    _refused(_args(n_queries=2, queries=_FAKE, query_count_out=_FAKE), "query_mass_out")
    _refused(_args(n_queries=2, queries=_FAKE, query_mass_out=_FAKE), "query_count_out")
    a = _args()
    a.levels = None
    _refused(a, "levels")
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
    body = header[header.index("typedef struct RnfGridCredible {") + 32:header.index("} RnfGridCredible;")]
    names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
    assert names == [f for f, _ in _lib.GridCredible._fields_], names
    assert {"rnf_grid_credible", "rnf_grid_credible_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "Q 2^-(S + 1)" in header and "S = 62 - ceil(log2 Q)" in header        # the rule and its bound are stated


# ---- Python entry points: argument checks run before anything touches a device ----------------------------------------------------------
def _cpu_flow():
    with contextlib.redirect_stdout(io.StringIO()):
        return Flow(make_config(layers=2, condition=1, feature_dim=16, rot="16Trans"))


def test_python_entry_points_validate_their_arguments():
    fl = _cpu_flow()
    feat = torch.zeros(2, 16)
    for bad in ((0.0,), (1.0,), (0.5, 1.5), (float("nan"),), (), (0.5,) * 9):
        with pytest.raises(ValueError, match="level"):
            harness.grid_pose_credible(fl, feat, levels=bad, recursion_level=0)
        with pytest.raises(ValueError, match="level"):
            harness.grid_credible(torch.zeros(2, 8), bad)
    with pytest.raises(ValueError, match="ground truths"):
        harness.grid_pose_credible(fl, feat, recursion_level=0, gt_rotation=torch.eye(3).expand(2, 17, 3, 3))
    with pytest.raises(ValueError, match="queries"):
        harness.grid_credible(torch.zeros(2, 8), (0.5,), queries=torch.zeros(2, 17))
    with pytest.raises(ValueError, match="grid rows"):
        harness.grid_pose_credible(fl, feat, recursion_level=7)
    with pytest.raises(RuntimeError, match="GPU only"):                 # valid arguments on CPU tensors: no CPU fallback
        harness.grid_pose_credible(fl, feat, recursion_level=0)
