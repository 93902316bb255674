"""From a rotation back to its cell of the SO(3) grid (rnf_so3_grid_locate, sd.grid_index / grid_histogram) and the fit of a histogram
against a grid density (rnf_grid_fit, harness.grid_fit / grid_pose_fit), CPU part: fp64 numpy restatements of both, which
tests/test_gpu_grid_locate.py shares; the locate restatement against the grid checker of tests/test_so3_grid.py (round trip), on
Haar-uniform rotations (equal volume) and at the poles; the fit restatement on hand-built rows; the C ABI's refusals, which happen before
any launch; and the argument checks of the Python entry points."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib, harness, make_config, synth
from rotationnormflow_amd.flow.flow import Flow
from rotationnormflow_amd.utils import sd
from tests.test_so3_grid import _rx, _rz, healpix_grid_fp64


def grid_locate_fp64(level, R, offset=None):
    """fp64 restatement of rnf_so3_grid_locate (include/rnf_hip.h).  R [n,3,3] (the fp32 values the device reads, as any float type),
    offset [3,3] or None -> (rows int64 [n], margin fp64 [n]).  margin: the smallest distance of any floor or rint argument from the
    value at which it switches, and of |z| from 2/3 scaled by nside: a rotation whose margin is far above the rounding of the fp64
    arithmetic (1e-9 is a million times that) has the same row however the arithmetic is ordered."""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    n = R.shape[0]
    bad = ~np.isfinite(R).all(axis=(1, 2))
    A = np.where(bad[:, None, None], np.eye(3), R)
    if offset is not None:
        A = A @ np.asarray(offset, np.float64).reshape(3, 3).T
    nside = 2 ** level
    npix, ncap, nl4, tilts = 12 * nside * nside, 2 * nside * (nside - 1), 4 * nside, 6 * nside
    z = np.clip(A[:, 0, 0], -1.0, 1.0)
    za = np.abs(z)
    sth = np.hypot(A[:, 1, 0], A[:, 2, 0])
    pole = (A[:, 1, 0] == 0) & (A[:, 2, 0] == 0)
    phi = np.where(pole, 0.0, np.arctan2(A[:, 2, 0], A[:, 1, 0]))
    tau = np.where(pole, np.where(z > 0, np.arctan2(A[:, 2, 1], A[:, 1, 1]), np.arctan2(A[:, 2, 1], A[:, 2, 2])),
                   np.arctan2(A[:, 0, 2], -A[:, 0, 1]))
    tt = phi * (2.0 / np.pi)
    tt = np.where(tt < 0, tt + 4.0, tt)
    tt = np.where(tt >= 4.0, tt - 4.0, tt)

    def off_int(x):                                        # distance of a floor argument from the closest integer
        return np.abs(x - np.rint(x))

    margin = np.abs(za - 2.0 / 3.0) * nside
    # the belt
    t1, t2 = nside * (0.5 + tt), nside * z * 0.75
    jp, jm = np.floor(t1 - t2).astype(np.int64), np.floor(t1 + t2).astype(np.int64)
    ir = np.clip(nside + 1 + jp - jm, 1, 2 * nside + 1)
    kshift = 1 - (ir & 1)
    ip = ((jp + jm - nside + kshift + 1 + 2 * nl4) >> 1) & (nl4 - 1)
    p_belt = ncap + (ir - 1) * nl4 + ip
    m_belt = np.minimum(off_int(t1 - t2), off_int(t1 + t2))
    # the caps
    tp = tt - np.floor(tt)
    tmp = np.minimum(nside * sth / np.sqrt((1.0 + za) / 3.0), float(nside))
    cjp, cjm = np.floor(tp * tmp).astype(np.int64), np.floor((1.0 - tp) * tmp).astype(np.int64)
    cir = np.clip(cjp + cjm + 1, 1, nside)
    cip = np.clip(np.floor(tt * cir).astype(np.int64), 0, 4 * cir - 1)
    p_cap = np.where(z > 0, 2 * cir * (cir - 1) + cip, npix - 2 * cir * (cir + 1) + cip)
    m_cap = np.minimum(np.minimum(off_int(tp * tmp), off_int((1.0 - tp) * tmp)), off_int(tt * cir))
    belt = za <= 2.0 / 3.0
    p = np.clip(np.where(belt, p_belt, p_cap), 0, npix - 1)
    margin = np.minimum(margin, np.where(belt, m_belt, m_cap))
    u = tau / (2.0 * np.pi / tilts)
    k = np.rint(u).astype(np.int64)
    margin = np.minimum(margin, 0.5 - np.abs(u - k))      # rint switches at the half-integers
    rows = (k % tilts) * npix + p
    rows[bad] = -1
    margin = np.where(bad, np.inf, margin)
    assert rows.shape == (n,)
    return rows, margin


def grid_fit_fp64(lp, counts):
    """fp64 restatement of rnf_grid_fit with real-valued fp64 weights.  lp [g,Q] (or [Q]), counts int [g,Q]
    -> dict(log_norm, log_likelihood, grid_log_likelihood, g_stat, chi2: fp64 [g]; n, occupied: int64 [g])"""
    lp = np.atleast_2d(np.asarray(lp, np.float64))
    counts = np.atleast_2d(np.asarray(counts, np.int64))
    g, Q = lp.shape
    out = {k: np.full(g, np.nan) for k in ("log_norm", "log_likelihood", "grid_log_likelihood", "g_stat", "chi2")}
    out["n"], out["occupied"] = np.zeros(g, np.int64), np.zeros(g, np.int64)
    for b in range(g):
        row, c = lp[b], np.maximum(counts[b], 0)
        occ = c > 0
        n = int(c.sum())
        out["n"][b], out["occupied"][b] = n, int(occ.sum())
        if np.isnan(row).any() or row.max() == np.inf:
            continue
        M = row.max()
        with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
            w = np.zeros(Q) if M == -np.inf else np.exp(row - M)
            Z = w.sum()
            out["log_norm"][b] = M + np.log(Z) - np.log(Q)
            if n == 0:
                continue
            if (w[occ] == 0).any():                        # a sample in a cell without mass
                out["log_likelihood"][b] = -np.inf
                out["grid_log_likelihood"][b] = -np.inf - out["log_norm"][b]
                out["g_stat"][b] = out["chi2"][b] = np.inf
                continue
            cf = c[occ].astype(np.float64)
            p = w[occ] / Z
            out["log_likelihood"][b] = (cf * row[occ]).sum() / n
            out["grid_log_likelihood"][b] = out["log_likelihood"][b] - out["log_norm"][b]
            out["g_stat"][b] = 2.0 * (cf * (np.log(cf / n) - np.log(p))).sum()
            pa = w / Z                                       # Pearson's statistic over every cell, as defined
            out["chi2"][b] = ((c[pa > 0] - n * pa[pa > 0]) ** 2 / (n * pa[pa > 0])).sum()
    return out


def multinomial_counts(lp_row, n, rng):
    """n samples over the cells with the row's own masses softmax(lp) -> int32 [Q]"""
    w = np.exp(np.asarray(lp_row, np.float64) - np.max(lp_row))
    return rng.multinomial(n, w / w.sum()).astype(np.int32)


def _offset(seed):
    return synth.uniform_rotations(1, seed=seed)[0].astype(np.float32)


# ---- locate: the restatement against the grid checker ------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1, 2, 3, 4])
def test_every_grid_row_is_located_in_its_own_cell(level):
    Q = sd.grid_size(level)
    rows, margin = grid_locate_fp64(level, healpix_grid_fp64(level).astype(np.float32))
    assert np.array_equal(rows, np.arange(Q))
    # ring nside has its centres at z = 2/3 exactly, where the belt's and the caps' formulas meet (and agree): no margin there
    away = np.abs(np.abs(healpix_grid_fp64(level)[:, 0, 0]) - 2.0 / 3.0) > 1e-3
    assert margin[away].min() > 1e-6                       # elsewhere a cell's centre is far from every switching point
    O = _offset(level + 20)
    moved = healpix_grid_fp64(level, offset=O.astype(np.float64)).astype(np.float32)
    assert np.array_equal(grid_locate_fp64(level, moved, O)[0], np.arange(Q))
    if level <= 2:                                         # and not merely by luck: without the offset the rows differ
        assert not np.array_equal(grid_locate_fp64(level, moved)[0], np.arange(Q))


@pytest.mark.parametrize("level", [5, 6, 7, 8])
def test_random_rows_of_the_fine_levels_are_located(level):
    rng = np.random.default_rng(level)
    want = rng.integers(0, sd.grid_size(level), 20_000)
    O = _offset(level + 30)
    assert np.array_equal(grid_locate_fp64(level, healpix_grid_fp64(level, want).astype(np.float32))[0], want)
    assert np.array_equal(grid_locate_fp64(level, healpix_grid_fp64(level, want, O.astype(np.float64)).astype(np.float32), O)[0], want)


@pytest.mark.parametrize("level", [0, 1, 2])
def test_cells_have_equal_volume(level):
    """200 Q Haar-uniform rotations: the cell counts are multinomial with equal masses, so Pearson's chi^2 against Q - 1 degrees of
    freedom is within 5 standard deviations of its mean."""
    Q = sd.grid_size(level)
    R = synth.uniform_rotations(200 * Q, seed=40 + level)
    rows, _ = grid_locate_fp64(level, R, _offset(50 + level))
    c = np.bincount(rows, minlength=Q)
    assert c.shape == (Q,) and c.sum() == 200 * Q
    chi2 = ((c - 200.0) ** 2 / 200.0).sum()
    z = (chi2 - (Q - 1)) / np.sqrt(2.0 * (Q - 1))
    assert abs(z) < 5, z


def pole_cases():
    """(name, R fp64 [3,3], level -> expected row) of the pole rule: at z = +1 the rotation is Rx(a) and a is all tilt; at z = -1 it is
    Rz(pi) Rx(a).  The north pole lies in pixel 0, the south pole in pixel npix - 4 (phi = 0: the first of the last ring)."""
    def north(a):
        return lambda level: int(np.rint(a / (2 * np.pi / (6 * 2 ** level)))) % (6 * 2 ** level) * 12 * 4 ** level

    def south(a):
        return lambda level: north(a)(level) + 12 * 4 ** level - 4

    cases = [("I", np.eye(3), north(0.0)), ("diag(1,-1,-1)", np.diag([1.0, -1.0, -1.0]), north(np.pi)),
             ("diag(-1,-1,1)", np.diag([-1.0, -1.0, 1.0]), south(0.0)), ("diag(-1,1,-1)", np.diag([-1.0, 1.0, -1.0]), south(np.pi))]
    for a in (0.3, 1.0, 2.5, -0.7, -3.0):
        cases.append((f"Rx({a})", _rx(np.float64(a)), north(a)))
        cases.append((f"Rz(pi)Rx({a})", np.diag([-1.0, -1.0, 1.0]) @ _rx(np.float64(a)), south(a)))
    return cases


@pytest.mark.parametrize("level", [0, 1, 3])
def test_pole_rule(level):
    for name, R, want in pole_cases():
        R32 = R.astype(np.float32)
        assert R32[1, 0] == 0 and R32[2, 0] == 0, name
        assert grid_locate_fp64(level, R32[None])[0][0] == want(level), name


def test_pole_rows_are_what_the_grid_generates():
    """Rz(pi) Rx(a) = Rx(0) Rz(pi) Rx(a): the south pole with tilt a; diag(-1,1,-1) = Rz(pi) Rx(pi)."""
    np.testing.assert_allclose(_rz(np.float64(np.pi)) @ _rx(np.float64(np.pi)), np.diag([-1.0, 1.0, -1.0]), atol=1e-15)
    np.testing.assert_allclose(_rz(np.float64(np.pi)), np.diag([-1.0, -1.0, 1.0]), atol=1e-15)


def test_non_finite_rotations_have_no_cell():
    R = synth.uniform_rotations(4, seed=3).astype(np.float32)
    R[1, 2, 1] = np.nan
    R[3, 0, 0] = np.inf
    rows, margin = grid_locate_fp64(2, R)
    assert rows[1] == -1 and rows[3] == -1 and rows[0] >= 0 and rows[2] >= 0 and np.isinf(margin[[1, 3]]).all()


def test_margin_of_random_rotations_is_far_above_rounding():
    R = synth.uniform_rotations(200_000, seed=11)
    for level in (0, 3, 8):
        assert grid_locate_fp64(level, R, _offset(level))[1].min() > 1e-9


# ---- the fit restatement on hand-built rows ----------------------------------------------------------------------------------------------
def test_counts_proportional_to_the_masses_fit_exactly():
    lp = np.log(np.array([1.0, 2.0, 3.0, 4.0, 0.5, 0.5]) / 11.0 * 6.0)          # masses k / 11, log_norm 0
    r = grid_fit_fp64(lp, np.array([2, 4, 6, 8, 1, 1]) * 5)
    assert abs(r["g_stat"][0]) < 1e-12 and abs(r["chi2"][0]) < 1e-12 and abs(r["log_norm"][0]) < 1e-15
    assert r["n"][0] == 110 and r["occupied"][0] == 6
    r = grid_fit_fp64(lp, np.array([2, 4, 6, 8, 1, 2]) * 5)
    assert r["g_stat"][0] > 0 and r["chi2"][0] > 0


def test_flat_row_with_flat_counts():
    r = grid_fit_fp64(np.full(72, -1.25), np.full(72, 3))
    assert r["log_norm"][0] == -1.25 and r["log_likelihood"][0] == -1.25 and r["grid_log_likelihood"][0] == 0
    assert abs(r["g_stat"][0]) < 1e-12 and abs(r["chi2"][0]) < 1e-12 and r["n"][0] == 216 and r["occupied"][0] == 72


def test_one_sample_in_the_arg_max_cell():
    rng = np.random.default_rng(1)
    lp = rng.standard_normal(50)
    c = np.zeros(50, np.int64)
    c[np.argmax(lp)] = 1
    r = grid_fit_fp64(lp, c)
    assert r["log_likelihood"][0] == lp.max() and r["n"][0] == 1 and r["occupied"][0] == 1
    p = np.exp(lp.max()) / np.exp(lp).sum()
    assert np.isclose(r["g_stat"][0], -2 * np.log(p)) and np.isclose(r["chi2"][0], 1 / p - 1)
    assert np.isclose(r["grid_log_likelihood"][0], np.log(p * 50))


def fit_edge_rows():
    """(lp [6,8], counts [6,8]) of the edge cases of include/rnf_hip.h, one per row."""
    base = np.array([0.0, -1.0, -2.0, -0.5, -3.0, -1.5, -0.25, -2.5])
    lp = np.tile(base, (6, 1))
    c = np.tile(np.array([5, 3, 1, 4, 0, 2, 6, 1]), (6, 1))
    lp[0, 4] = -np.inf                                      # a -inf cell without samples contributes nothing
    lp[1, 2] = -np.inf                                      # a -inf cell with a sample
    lp[2, 5] = -800.0                                       # a cell whose weight underflows (in fp32 and in fp64), with samples
    lp[3, 1] = np.nan
    lp[4, 6] = np.inf
    c[5] = 0                                                # no samples
    return lp, c


def test_edge_cases_of_the_fit():
    lp, c = fit_edge_rows()
    r = grid_fit_fp64(lp, c)
    fin = lp[0][np.isfinite(lp[0])]
    assert np.isclose(r["log_norm"][0], np.log(np.exp(fin).sum() / 8)) and np.isfinite(r["g_stat"][0]) and np.isfinite(r["chi2"][0])
    assert np.isclose(r["log_likelihood"][0], (c[0] * np.where(c[0] > 0, lp[0], 0)).sum() / 22)
    for b in (1, 2):
        assert r["log_likelihood"][b] == -np.inf and r["grid_log_likelihood"][b] == -np.inf
        assert r["g_stat"][b] == np.inf and r["chi2"][b] == np.inf and np.isfinite(r["log_norm"][b])
    for b in (3, 4):
        assert all(np.isnan(r[k][b]) for k in ("log_norm", "log_likelihood", "grid_log_likelihood", "g_stat", "chi2"))
        assert r["n"][b] == 22 and r["occupied"][b] == 7
    assert np.isfinite(r["log_norm"][5]) and r["n"][5] == 0 and r["occupied"][5] == 0
    assert all(np.isnan(r[k][5]) for k in ("log_likelihood", "grid_log_likelihood", "g_stat", "chi2"))
    empty = grid_fit_fp64(np.full(8, -np.inf), c[0])
    assert empty["log_norm"][0] == -np.inf and empty["log_likelihood"][0] == -np.inf and empty["g_stat"][0] == np.inf


def test_multinomial_counts_from_the_rows_own_masses_fit():
    from tests.test_grid_credible_host import numpy_grid, synthetic_logp
    lp = synthetic_logp(numpy_grid(1), 2, seed=9)
    Q = lp.shape[1]
    rng = np.random.default_rng(4)
    own = np.stack([multinomial_counts(lp[b], 10 * Q, rng) for b in range(2)])
    flat = np.stack([multinomial_counts(np.zeros(Q), 10 * Q, rng) for b in range(2)])
    r, f = grid_fit_fp64(lp, own), grid_fit_fp64(lp, flat)
    assert np.all(r["n"] == 10 * Q) and np.all(r["g_stat"] / (2 * r["n"]) < f["g_stat"] / (2 * f["n"]))
    assert np.all(r["grid_log_likelihood"] > f["grid_log_likelihood"])


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20


def _locate(**kw):
    base = dict(level=2, rotations=_FAKE, n=10, g=1, rows_out=_FAKE)
    base.update(kw)
    return _lib.GridLocate(**base)


def _fit(**kw):
    base = dict(logp=_FAKE, counts=_FAKE, Q=4608, g=3, stats_out=_FAKE)
    base.update(kw)
    a = _lib.GridFit(**base)
    a.workspace, a.workspace_bytes = _FAKE, _lib.lib().rnf_grid_fit_workspace_bytes(ctypes.byref(a))
    return a


def _refused(fn, a, word):
    L = _lib.lib()
    assert getattr(L, fn)(ctypes.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def test_locate_refuses_bad_arguments_before_any_launch():
    fn = "rnf_so3_grid_locate"
    _refused(fn, _locate(level=-1), "level=")
    _refused(fn, _locate(level=9), "level=")
    _refused(fn, _locate(g=0), "g=")
    _refused(fn, _locate(g=65536), "g=")
    _refused(fn, _locate(n=-1), "n=")
    _refused(fn, _locate(rows_out=None), "at least one output")
    _refused(fn, _locate(rows_out=None, counts=_FAKE, level=7), "2^26")
    _refused(fn, _locate(counts=_FAKE, level=8), "2^26")
    _refused(fn, _locate(rotations=None), "null rotations")
    a = _locate()
    a.struct_bytes += 8
    _refused(fn, a, "struct_bytes")
    assert _lib.lib().rnf_so3_grid_locate(ctypes.byref(_locate(n=0, rotations=None))) == 0          # nothing to do, nothing launched
    assert _lib.lib().rnf_so3_grid_locate(ctypes.byref(_locate(n=0, level=8))) == 0


def test_fit_refuses_bad_arguments_before_any_launch():
    fn = "rnf_grid_fit"
    _refused(fn, _fit(g=0), "g=")
    _refused(fn, _fit(g=65536), "g=")
    _refused(fn, _fit(Q=0), "Q=")
    _refused(fn, _fit(Q=(1 << 26) + 1), "Q=")
    _refused(fn, _fit(logp=None), "null")
    _refused(fn, _fit(counts=None), "null")
    _refused(fn, _fit(stats_out=None), "null")
    a = _fit()
    a.workspace_bytes -= 1
    _refused(fn, a, "workspace")
    a = _fit()
    a.workspace = None
    _refused(fn, a, "workspace")
    a = _fit()
    a.workspace = _FAKE + 4
    _refused(fn, a, "aligned")
    a = _fit()
    a.struct_bytes += 8
    _refused(fn, a, "struct_bytes")


def test_fit_workspace_follows_the_documented_rule():
    L = _lib.lib()
    for Q, g in [(1, 1), (4608, 5), (8193, 2), (72 * 8 ** 5, 16), (72 * 8 ** 6, 1), (1 << 26, 3)]:
        want = g * (16 * min(-(-Q // 2048), 2048) + 48 * min(-(-Q // 8192), 512) + 12)
        want = (want + 15) // 16 * 16
        assert L.rnf_grid_fit_workspace_bytes(ctypes.byref(_lib.GridFit(Q=Q, g=g))) == want, (Q, g)
    for bad in (dict(Q=0), dict(Q=(1 << 26) + 1), dict(g=0), dict(g=65536)):
        kw = dict(Q=10, g=1)
        kw.update(bad)
        assert L.rnf_grid_fit_workspace_bytes(ctypes.byref(_lib.GridFit(**kw))) == 0, bad
    short = _lib.GridFit(Q=10, g=1)
    short.struct_bytes -= 8
    assert L.rnf_grid_fit_workspace_bytes(ctypes.byref(short)) == 0


def test_header_declares_the_structs_the_binding_mirrors():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    for name, cls in (("RnfGridLocate", _lib.GridLocate), ("RnfGridFit", _lib.GridFit)):
        body = header[header.index("typedef struct %s {" % name) + len("typedef struct %s {" % name):header.index("} %s;" % name)]
        names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
        assert names == [f for f, _ in cls._fields_], names
    assert {"rnf_so3_grid_locate", "rnf_grid_fit", "rnf_grid_fit_workspace_bytes"} <= set(_lib.EXPORTS)
    stats = re.findall(r"#define RNF_GRID_FIT_(\w+) (\d+)", header)
    assert [s.lower() for s, _ in stats[:-1]] == [s.replace("g_stat", "g") for s in _lib.GRID_FIT_STATS]
    assert [int(v) for _, v in stats] == list(range(len(_lib.GRID_FIT_STATS) + 1)) and stats[-1][0] == "STATS"
    assert "Voronoi" in header and "equal Haar" in header          # what a cell is and is not is stated
    assert _lib.lib().rnf_abi_version() == 8                       # the additions leave the ABI version alone


# ---- Python entry points: argument checks run before anything touches a device ----------------------------------------------------------
def _cpu_flow():
    with contextlib.redirect_stdout(io.StringIO()):
        return Flow(make_config(layers=2, condition=1, feature_dim=16, rot="16Trans"))


def test_python_entry_points_validate_their_arguments():
    R = torch.eye(3).expand(5, 3, 3)
    for fn in (sd.grid_index, sd.grid_histogram):
        with pytest.raises(ValueError, match="level"):
            fn(R, 9)
        with pytest.raises(ValueError, match="level"):
            fn(R, -1)
        with pytest.raises(ValueError, match="rotations"):
            fn(torch.zeros(5, 9), 1)
        with pytest.raises(ValueError, match="offset"):
            fn(R, 1, offset=torch.zeros(4))
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(R, 1)
    with pytest.raises(ValueError, match="grid rows"):
        sd.grid_histogram(R, 7)
    with pytest.raises(ValueError, match="rotations"):
        sd.grid_histogram(torch.zeros(2, 2, 5, 3, 3), 1)
    with pytest.raises(ValueError, match="want"):
        harness.grid_fit(torch.zeros(2, 8), torch.zeros(2, 9, dtype=torch.int32))
    with pytest.raises(ValueError, match="want"):
        harness.grid_fit(torch.zeros(8), torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        harness.grid_fit(torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="grid rows"):
        harness.grid_fit(torch.zeros(1, 0), torch.zeros(1, 0, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        harness.grid_fit(torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int32))
    fl = _cpu_flow()
    feat = torch.zeros(2, 16)
    for bad in (dict(recursion_level=7), dict(recursion_level=-1), dict(n_samples=0), dict(samples=torch.zeros(2, 9)),
                dict(samples=torch.zeros(1, 2, 2, 3, 3)), dict(images_per_launch=0)):
        with pytest.raises(ValueError):
            harness.grid_pose_fit(fl, feat, **bad)
    with pytest.raises(RuntimeError, match="GPU only"):                 # valid arguments on CPU tensors: no CPU fallback
        harness.grid_pose_fit(fl, feat, samples=R.expand(2, 5, 3, 3), recursion_level=0)
