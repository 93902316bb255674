"""CPU: draws from SO(3) grid posteriors (csrc/grid_sample.h: rnf_so3_grid_cell_points, rnf_grid_sample; sd.grid_cell_points,
harness.grid_sample / grid_pose_sample).  The host build of the header (tests/csrc/host_grid_sample.cpp: the functions the kernels call,
with the host's expf) is held to numpy restatements which tests/test_gpu_grid_sample.py shares: a numpy Philox4x32-10, the targets in
Python integers, the masses rint(exp(lp - m) 2^S) from the fp64 exponential and their uint64 np.cumsum.

The bracket of a draw.  The library's mass is W_i = rint(e_i 2^S) with e_i the fp32 expf of the fp32 difference lp_i - m; the restatement's
is W'_i = rint(exp(lp_i - m) 2^S) from the same fp32 difference.  An expf within one unit in the last place of fp32 (the bound of the
device's and of the host's library) has |e_i - exp| <= 2^-23 exp, and each rint moves a mass by at most 1/2, so the prefix sums obey
|C_i - C'_i| <= 2^-23 C'_i + (i + 1).  The drawn row has C_{i-1} <= v < C_i, hence
    first j with C'_j > (v - Q)(1 - DELTA)  <=  i  <=  first j with C'_j > (v + Q)(1 + DELTA),      DELTA = 2^-22 = 2.4e-7
(2^-23 to first order, doubled for the division by 1 -+ 2^-23; Q is the integer roundings' share, Q 2^-S <= 2^-10 of one row's mass at
the very worst and 2^-37 of it at level 2).  No draw is left out of this check.
"""
import contextlib
import ctypes as C
import functools
import io
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib, grid_pose, harness, make_config, synth
from rotationnormflow_amd.flow.flow import Flow
from rotationnormflow_amd.utils import sd
from tests.test_grid_credible_host import numpy_grid, synthetic_logp
from tests.test_so3_grid import healpix_grid_fp64
from tests.test_so3_kde_host import ptr
from tests.test_so3_locate_host import grid_fit_fp64, grid_locate_fp64

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_grid_sample.cpp")
OUT = os.path.join(HERE, "csrc", "_host_grid_sample.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f) for f in ("grid_sample.h", "grid_mass.h", "philox.h", "so3_grid.h")]
DELTA = 2.0 ** -22                                         # the module's docstring
MARGIN = 1e-5                                              # charts are compared with their cell where the located point is this far inside
MAX_SKIPPED = 5e-4                                         # .. and at most this share of them is not
CENTRE_GATE = 2.0 ** -23                                   # a chart centre against the fp64 grid: the fp32 store rounds an entry of size <= 1
#                                                            by 2^-24 = 6e-8; the fp64 arithmetic before it adds 1e-15.  Twice the store.
METHODS = {"multinomial": 0, "systematic": 1}


def _host_lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    return C.CDLL(OUT)


def _off9(offset):
    return None if offset is None else np.ascontiguousarray(offset, np.float32).reshape(9)


def host_cell_points(level, rows, u, offset=None):
    """The host build of the chart: rows int64 [n], u [n,3] -> float32 [n,3,3]"""
    rows = np.ascontiguousarray(rows, np.int64)
    u = np.ascontiguousarray(u, np.float32).reshape(len(rows), 3)
    rot = np.empty((len(rows), 3, 3), np.float32)
    _host_lib().hgs_cell_points(int(level), ptr(_off9(offset)), ptr(rows), ptr(u), C.c_longlong(len(rows)), ptr(rot))
    return rot


def host_grid_rows(level, rows, offset=None):
    """The host build of the grid's own row function (so3_grid.h's grid_row) -> float32 [n,3,3]"""
    rows = np.ascontiguousarray(rows, np.int64)
    rot = np.empty((len(rows), 3, 3), np.float32)
    _host_lib().hgs_grid_rows(int(level), ptr(_off9(offset)), ptr(rows), C.c_longlong(len(rows)), ptr(rot))
    return rot


def host_sample(logp, n, level=-1, method="systematic", jitter=True, seed=1, offset=None, draw_base=0, draws_total=None, image_base=0):
    """The host build of rnf_grid_sample -> dict(index int64 [g,n], target uint64 [g,n], total uint64 [g], rot float32 [g,n,3,3] or None)"""
    lp = np.ascontiguousarray(np.atleast_2d(logp), np.float32)
    g, Q = lp.shape
    index, target, total = np.empty((g, n), np.int64), np.empty((g, n), np.uint64), np.empty(g, np.uint64)
    rot = np.empty((g, n, 3, 3), np.float32) if level >= 0 else None
    _host_lib().hgs_sample(ptr(lp), C.c_longlong(Q), g, int(level), C.c_longlong(n), C.c_longlong(draw_base),
                           C.c_longlong(n if draws_total is None else draws_total), C.c_longlong(image_base), METHODS[method], int(bool(jitter)),
                           C.c_ulonglong(seed), ptr(_off9(offset)), ptr(index), ptr(target), ptr(total), ptr(rot))
    return dict(index=index, target=target, total=total, rot=rot)


# ---- the restatements --------------------------------------------------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)


def philox_np(seed, draw, image, stream):
    """Philox4x32-10 with key (seed low, seed high) on the counters (draw, image low, image high, stream) -> uint64 [n,4] (32-bit words)"""
    draw = np.atleast_1d(np.asarray(draw, np.uint64))
    c = [draw & _M32, np.full_like(draw, int(image) & 0xFFFFFFFF), np.full_like(draw, (int(image) >> 32) & 0xFFFFFFFF),
         np.full_like(draw, int(stream))]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=1)


def r64_np(seed, draw, image, stream=0):
    """-> a list of Python integers below 2^64"""
    w = philox_np(seed, draw, image, stream)
    return [(int(a) << 32) | int(b) for a, b in zip(w[:, 0], w[:, 1])]


def targets_ref(method, seed, image, draws, N, T):
    """The targets of the global draws ``draws`` of global image ``image`` in Python integers -> uint64 [n]"""
    T = int(T)
    if method == "multinomial":
        return np.array([(r * T) >> 64 for r in r64_np(seed, draws, image)], np.uint64)
    a = (r64_np(seed, [0], image)[0] * T) >> 64
    return np.array([(int(k) * T + a) // int(N) for k in draws], np.uint64)


def jitter_ref(seed, image, draws):
    """The three jitter uniforms of the draws -> float64 [n,3] in (0, 1)"""
    return (philox_np(seed, draws, image, 1)[:, :3].astype(np.float64) + 0.5) / 4294967296.0


def shift_of(Q):
    c = 0
    while (1 << c) < Q:
        c += 1
    return 62 - c


def prefix_ref(row):
    """The restatement's masses of one image: rint(exp(lp - m) 2^S) from the fp64 exponential of the fp32 difference
    -> (W uint64 [Q], C uint64 [Q] inclusive)"""
    row = np.asarray(row, np.float32)
    with np.errstate(invalid="ignore"):
        d = (row - row.max()).astype(np.float64)           # the fp32 subtraction, as the library forms it
    W = np.rint(np.exp(d) * 2.0 ** shift_of(len(row))).astype(np.uint64)
    return W, np.cumsum(W, dtype=np.uint64)


def bracket_of(Cref, v):
    """The rows a draw of target v may land on -> (lo, hi) int64 [n], inclusive"""
    Q = len(Cref)
    v = np.asarray(v, np.float64)                          # 2^-53 relative: far inside DELTA
    Cf = Cref.astype(np.float64)
    lo = np.searchsorted(Cf, (v - Q) * (1.0 - DELTA), side="right")
    hi = np.searchsorted(Cf, (v + Q) * (1.0 + DELTA), side="right")
    return lo, np.minimum(hi, Q - 1)


def check_draws(lp, got, method, seed, N, image_base=0, draw_base=0, what=""):
    """Every image of ``got`` (host_sample's dict, or the device's as numpy) against the restatement: targets exactly, rows in the bracket,
    no row without mass.  -> the share of draws whose bracket is a single row"""
    lp = np.atleast_2d(lp)
    single = []
    for b in range(lp.shape[0]):
        W, Cref = prefix_ref(lp[b])
        T, n = int(got["total"][b]), got["index"].shape[1]
        assert abs(T - int(Cref[-1])) <= DELTA * int(Cref[-1]) + len(W), (what, b, T, int(Cref[-1]))
        want = targets_ref(method, seed, image_base + b, np.arange(draw_base, draw_base + n), N, T)
        assert np.array_equal(got["target"][b].astype(np.uint64), want), (what, b, "targets")
        assert (want < np.uint64(T)).all(), (what, b)
        lo, hi = bracket_of(Cref, want)
        idx = got["index"][b]
        assert ((lo <= idx) & (idx <= hi)).all(), (what, b, "outside the bracket", int(np.abs(idx - np.clip(idx, lo, hi)).max()))
        assert (np.exp(lp[b][idx].astype(np.float64) - lp[b].max()) > 0).all(), (what, b, "a row without mass was drawn")
        single.append(lo == hi)
    return float(np.mean(single)), np.stack(single)


def _offset(seed):
    return synth.uniform_rotations(1, seed=seed)[0].astype(np.float32)


@functools.lru_cache(maxsize=4)
def density_case(level, g, seed):
    """synthetic_logp on the level's grid -> float32 [g,Q] (read-only)"""
    lp = synthetic_logp(numpy_grid(level), g, seed)
    lp.setflags(write=False)
    return lp


def chart_rows_case(level, seed):
    """The rows and uniforms the chart is located on: every row of levels 0..3 once, 10^5 random rows of level 6"""
    rng = np.random.default_rng(seed)
    Q = sd.grid_size(level)
    rows = np.arange(Q, dtype=np.int64) if level <= 3 else rng.integers(0, Q, 100_000)
    return rows, rng.random((len(rows), 3), dtype=np.float32)


def check_located(level, rows, rot, offset, what):
    """The charts ``rot`` of ``rows`` lie in their own cells (grid_locate_fp64), up to the MARGIN rule"""
    got, margin = grid_locate_fp64(level, rot, offset)
    safe = margin >= MARGIN
    assert 1.0 - safe.mean() <= MAX_SKIPPED, (what, 1.0 - safe.mean())
    assert np.array_equal(got[safe], rows[safe]), (what, int((got[safe] != rows[safe]).sum()))


# ---- Philox and the targets -----------------------------------------------------------------------------------------------------------------

def test_numpy_philox_is_philox4x32_10_and_the_host_build_agrees():
    # known answers of Random123 (kat_vectors): zero counter and key; all ones
    assert [hex(int(w)) for w in philox_np(0, [0], 0, 0)[0]] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    ones = philox_np(0xFFFFFFFFFFFFFFFF, [0xFFFFFFFF], 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF)[0]
    assert [hex(int(w)) for w in ones] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]
    h = _host_lib()
    rng = np.random.default_rng(0)
    for _ in range(50):
        seed, draw, image, stream = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 30)), int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2))
        words = (C.c_uint * 4)()
        h.hgs_philox(C.c_ulonglong(seed), C.c_longlong(draw), C.c_longlong(image), C.c_uint(stream), words)
        assert list(words) == [int(w) for w in philox_np(seed, [draw], image, stream)[0]]


def test_systematic_targets_are_the_floor_of_the_exact_quotient():
    """k q + (k r + a) / N in 64 bits against floor((k T + a) / N) in Python integers, at the largest T and N"""
    lp = np.zeros((1, 1 << 20), np.float32)
    lp[0, ::3] = -0.3
    for N, base, n in ((1 << 30, (1 << 30) - 1000, 1000), (999_983, 0, 1000), (7, 0, 7)):
        got = host_sample(lp, n, method="systematic", seed=99, draw_base=base, draws_total=N, image_base=5)
        assert int(got["total"][0]) > 2 ** 61
        want = targets_ref("systematic", 99, 5, np.arange(base, base + n), N, got["total"][0])
        assert np.array_equal(got["target"][0], want) and (np.diff(got["index"][0]) >= 0).all()


# ---- the chart ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_chart_centre_is_the_grid_row(level):
    Q = sd.grid_size(level)
    rows = np.arange(Q, dtype=np.int64)
    half = np.full((Q, 3), 0.5, np.float32)
    for O in (None, _offset(60 + level)):
        ref = healpix_grid_fp64(level, offset=None if O is None else O.astype(np.float64))
        err = np.abs(host_cell_points(level, rows, half, O).astype(np.float64) - ref).max()
        assert err <= CENTRE_GATE, (level, err)
        assert np.abs(host_grid_rows(level, rows, O).astype(np.float64) - ref).max() <= CENTRE_GATE     # the host build of grid_row itself


@pytest.mark.parametrize("level", [0, 1, 2, 3, 6])
def test_charts_locate_to_their_own_row(level):
    rows, u = chart_rows_case(level, 70 + level)
    for O in (None, _offset(80 + level)):
        rot = host_cell_points(level, rows, u, O)
        assert np.isfinite(rot).all()
        check_located(level, rows, rot, O, (level, O is None))


def test_chart_corners_edges_and_the_poles_are_rotations():
    """u on the boundary of [0, 1]^3, the poles among them (the far corner of a polar face): finite, orthonormal, determinant 1"""
    for level in (0, 2, 6):
        Q = sd.grid_size(level)
        rows = np.concatenate([np.arange(min(Q, 600)), np.arange(Q - min(Q, 600), Q)]).astype(np.int64)
        for corner in np.ndindex(2, 2, 2):
            rot = host_cell_points(level, rows, np.tile(np.float32(corner), (len(rows), 1))).astype(np.float64)
            assert np.abs(rot @ rot.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and np.abs(np.linalg.det(rot) - 1).max() < 1e-6
    north = host_cell_points(0, [0, 1, 2, 3], np.float32([[1, 1, 0.5]] * 4))          # faces 0..3 at nside 1: the pole is their corner
    assert np.allclose(north[:, 0, 0], 1.0) and np.allclose(north[:, 1, 0], 0.0) and np.allclose(north[:, 2, 0], 0.0)
    south = host_cell_points(0, [8, 9, 10, 11], np.float32([[0, 0, 0.5]] * 4))
    assert np.allclose(south[:, 0, 0], -1.0)


def test_chart_refuses_rows_and_uniforms_outside_their_range_with_nans():
    rows = np.array([-1, 72, 1 << 40, 5, 5, 5, 5, 5], np.int64)
    u = np.full((8, 3), 0.5, np.float32)
    u[3, 0], u[4, 1], u[5, 2], u[6, 0] = np.nan, np.inf, -1e-3, 1.0001
    rot = host_cell_points(0, rows, u)
    assert np.isnan(rot[:7]).all() and np.isfinite(rot[7]).all()


def test_uniform_charts_are_haar_uniform():
    """Uniform rows of level 1 with uniform u, located two levels down: Pearson's chi^2 per degree of freedom within 0.05 of 1 (its
    standard deviation at 36863 degrees of freedom is 0.007)."""
    rng = np.random.default_rng(2024)
    Q3, n = sd.grid_size(3), 30 * sd.grid_size(3)
    rows = rng.integers(0, sd.grid_size(1), n)
    O = _offset(91)
    fine, _ = grid_locate_fp64(3, host_cell_points(1, rows, rng.random((n, 3), dtype=np.float32), O), O)
    c = np.bincount(fine, minlength=Q3)
    chi2 = ((c - n / Q3) ** 2 / (n / Q3)).sum() / (Q3 - 1)
    assert abs(chi2 - 1.0) < 0.05, chi2
    coarse, margin = grid_locate_fp64(1, host_cell_points(1, rows[:100_000], rng.random((100_000, 3), dtype=np.float32), O), O)
    assert np.array_equal(coarse[margin >= MARGIN], rows[:100_000][margin >= MARGIN])


# ---- the draws -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["systematic", "multinomial"])
def test_draws_lie_in_the_bracket_and_targets_are_exact(method):
    lp = density_case(2, 3, 11)
    got = host_sample(lp, 6000, level=2, method=method, seed=0xC0FFEE1234567, image_base=7)
    share, _ = check_draws(lp, got, method, 0xC0FFEE1234567, 6000, image_base=7, what=method)
    assert share > 0.99, share                             # and the bracket is nearly always one row: the check has teeth


@pytest.mark.parametrize("seed", [1, 2 ** 63 + 12345])
def test_flat_rows_are_drawn_exactly_three_times_each(seed):
    Q = 576
    flat = np.zeros((1, Q), np.float32)
    got = host_sample(flat, 3 * Q, level=1, seed=seed)
    assert np.array_equal(np.bincount(got["index"][0], minlength=Q), np.full(Q, 3)) and int(got["total"][0]) == Q << shift_of(Q)
    holes = flat.copy()
    holes[0, 1::2] = -np.inf
    got = host_sample(holes, 3 * (Q // 2), level=1, seed=seed)
    want = np.zeros(Q, np.int64)
    want[0::2] = 3
    assert np.array_equal(np.bincount(got["index"][0], minlength=Q), want)
    one = np.full((1, Q), -np.inf, np.float32)
    one[0, 123] = -4.5
    for method in METHODS:
        assert (host_sample(one, 500, level=1, seed=seed, method=method)["index"] == 123).all()


def test_many_blocks_and_a_ragged_last_chunk():
    Q = 3 * 8192 + 17
    got = host_sample(np.full((1, Q), 2.5, np.float32), 3 * Q, level=-1, seed=5)
    assert np.array_equal(np.bincount(got["index"][0], minlength=Q), np.full(Q, 3)) and got["rot"] is None


def test_rows_beyond_2_to_the_24():
    Q = (1 << 24) + 4099
    lp = np.full((1, Q), -np.inf, np.float32)
    lp[0, Q - 5000:] = 1.0
    got = host_sample(lp, 15_000, level=-1, seed=8)
    assert np.array_equal(np.bincount(got["index"][0] - (Q - 5000), minlength=5000), np.full(5000, 3))
    multi = host_sample(lp, 4000, level=-1, seed=8, method="multinomial")["index"][0]
    assert multi.min() >= Q - 5000 and multi.max() < Q and len(np.unique(multi)) > 2000


def test_systematic_counts_are_within_one_of_their_expectation():
    lp = density_case(2, 3, 11)
    n = 200_000
    got = host_sample(lp, n, level=2, seed=17)
    for b in range(lp.shape[0]):
        W, Cref = prefix_ref(lp[b])
        p = W.astype(np.float64) / float(Cref[-1])
        count = np.bincount(got["index"][b], minlength=lp.shape[1])
        assert np.abs(count - n * p).max() < 1.0 + 2.0 * n * DELTA, np.abs(count - n * p).max()
        assert (np.diff(got["index"][b]) >= 0).all()


def test_multinomial_counts_pass_the_likelihood_ratio_test():
    """A smooth density whose every cell expects tens of draws, so that the chi-square limit of the G statistic holds"""
    Q = sd.grid_size(1)
    lp = np.random.default_rng(3).uniform(-1.5, 1.5, (2, Q)).astype(np.float32)
    n = 200 * Q
    got = host_sample(lp, n, level=1, method="multinomial", seed=23)
    counts = np.stack([np.bincount(got["index"][b], minlength=Q) for b in range(2)])
    fit = grid_fit_fp64(lp, counts)
    z = (fit["g_stat"] - (Q - 1)) / np.sqrt(2.0 * (Q - 1))
    assert (np.abs(z) < 5).all(), z
    flat = grid_fit_fp64(np.zeros_like(lp), counts)        # and the statistic can tell: the same counts against a flat density
    assert ((flat["g_stat"] - (Q - 1)) / np.sqrt(2.0 * (Q - 1)) > 50).all()


def degenerate_case(level=1):
    """A regular image between a NaN one, a +inf one and one without a finite value -> float32 [5,Q]"""
    lp = np.array(density_case(level, 2, 5)).repeat(3, axis=0)[:5].copy()
    lp[1, 17] = np.nan
    lp[2, 40] = np.inf
    lp[3, :] = -np.inf
    return lp


def check_degenerate(lp, got):
    for b in (1, 2, 3):
        assert (got["index"][b] == -1).all() and np.isnan(got["rot"][b]).all() and int(got["total"][b]) == 0 and (got["target"][b] == 0).all()
    for b in (0, 4):
        assert (got["index"][b] >= 0).all() and np.isfinite(got["rot"][b]).all() and int(got["total"][b]) > 0


@pytest.mark.parametrize("method", ["systematic", "multinomial"])
def test_degenerate_images_have_no_draws_and_leave_the_others_alone(method):
    lp = degenerate_case()
    got = host_sample(lp, 300, level=1, method=method, seed=31)
    check_degenerate(lp, got)
    for b in (0, 4):
        alone = host_sample(lp[b:b + 1], 300, level=1, method=method, seed=31, image_base=b)
        assert all(np.array_equal(alone[k][0], got[k][b]) for k in ("index", "target", "total", "rot"))


@pytest.mark.parametrize("method", ["systematic", "multinomial"])
def test_tiling_over_images_and_draws_is_bit_identical(method):
    lp = density_case(1, 5, 3)
    O = _offset(14)
    n = 1000
    whole = host_sample(lp, n, level=1, method=method, seed=77, offset=O)
    for b0, b1 in ((0, 1), (1, 2), (2, 5)):
        part = host_sample(lp[b0:b1], n, level=1, method=method, seed=77, offset=O, image_base=b0)
        assert all(np.array_equal(part[k], whole[k][b0:b1]) for k in ("index", "target", "total", "rot")), (b0, b1)
    for k0, k1 in ((0, 1), (1, 640), (640, 1000)):
        part = host_sample(lp, k1 - k0, level=1, method=method, seed=77, offset=O, draw_base=k0, draws_total=n)
        assert all(np.array_equal(part[k], whole[k][:, k0:k1]) for k in ("index", "target", "rot")), (k0, k1)
    assert not np.array_equal(host_sample(lp, n, level=1, method=method, seed=78, offset=O)["target"], whole["target"])


def test_rotations_are_the_grid_rows_without_jitter_and_in_their_cell_with_it():
    lp = density_case(2, 2, 21)
    O = _offset(15)
    plain = host_sample(lp, 2000, level=2, jitter=False, seed=3, offset=O, method="multinomial")
    assert np.array_equal(plain["rot"].reshape(-1, 3, 3), host_grid_rows(2, plain["index"].reshape(-1), O))       # bit for bit
    moved = host_sample(lp, 2000, level=2, jitter=True, seed=3, offset=O, method="multinomial")
    assert np.array_equal(moved["index"], plain["index"])
    check_located(2, moved["index"].reshape(-1), moved["rot"].reshape(-1, 3, 3), O, "jittered draws")
    for b in range(2):                                     # and the jitter is the documented stream through the documented chart
        u = jitter_ref(3, b, np.arange(2000))
        assert u.min() > 0 and u.max() < 1
        ref = host_cell_points(2, moved["index"][b], u.astype(np.float32), O)
        assert np.abs(ref.astype(np.float64) - moved["rot"][b]).max() < 1e-6     # u rounded to fp32 moves a point by under 6e-8 of a cell


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20


def _sample(**kw):
    base = dict(logp=_FAKE, Q=4608, g=3, level=2, draws=100, draw_base=0, draws_total=100, image_base=0, method=1, jitter=1, seed=1,
                index_out=_FAKE, target_out=_FAKE, total_out=_FAKE, rot_out=_FAKE)
    base.update(kw)
    a = _lib.GridSample(**base)
    a.workspace, a.workspace_bytes = _FAKE, _lib.lib().rnf_grid_sample_workspace_bytes(C.byref(a))
    return a


def _points(**kw):
    base = dict(level=2, rows=_FAKE, u=_FAKE, n=10, rot_out=_FAKE)
    base.update(kw)
    return _lib.GridCellPoints(**base)


def _refused(fn, a, word):
    L = _lib.lib()
    assert getattr(L, fn)(C.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def test_sample_refuses_bad_arguments_before_any_launch():
    fn = "rnf_grid_sample"
    for bad, word in ((dict(g=0), "g="), (dict(g=65536), "g="), (dict(Q=0), "Q="), (dict(Q=(1 << 26) + 1), "Q="), (dict(Q=4607), "level 2"),
                      (dict(level=7, Q=72 * 8 ** 7), "Q="), (dict(level=7), "level="), (dict(level=-2), "level="),
                      (dict(level=-1), "rot_out"), (dict(method=2), "method="), (dict(method=-1), "method="),
                      (dict(draws_total=0), "draws_total="), (dict(draws_total=(1 << 30) + 1, draws=1), "draws_total="),
                      (dict(draw_base=1), "outside"), (dict(draws=101), "outside"), (dict(draws=-1), "outside"), (dict(draw_base=-1), "outside"),
                      (dict(draw_base=1 << 62, draws=1 << 62), "outside"), (dict(image_base=-1), "image_base="), (dict(logp=None), "null logp"),
                      (dict(index_out=None), "null index_out")):
        _refused(fn, _sample(**bad), word)
    a = _sample()
    a.workspace_bytes -= 1
    _refused(fn, a, "workspace")
    a = _sample()
    a.workspace = None
    _refused(fn, a, "workspace")
    a = _sample()
    a.workspace = _FAKE + 4
    _refused(fn, a, "aligned")
    a = _sample()
    a.struct_bytes += 8
    _refused(fn, a, "struct_bytes")


def test_cell_points_refuses_bad_arguments_before_any_launch():
    fn = "rnf_so3_grid_cell_points"
    for bad, word in ((dict(level=-1), "level="), (dict(level=7), "level="), (dict(n=-1), "n="), (dict(rows=None), "null"), (dict(u=None), "null"),
                      (dict(rot_out=None), "null")):
        _refused(fn, _points(**bad), word)
    a = _points()
    a.struct_bytes -= 8
    _refused(fn, a, "struct_bytes")
    assert _lib.lib().rnf_so3_grid_cell_points(C.byref(_points(n=0, rows=None))) == 0            # nothing to do, nothing launched


def test_sample_workspace_follows_the_documented_rule():
    L = _lib.lib()
    for Q, g in [(1, 1), (4608, 5), (3 * 8192 + 17, 2), (72 * 8 ** 5, 16), (72 * 8 ** 6, 1), (1 << 26, 3)]:
        want = g * (16 * min(-(-Q // 2048), 2048) + 8 * -(-Q // 64) + 20)
        want = (want + 15) // 16 * 16
        assert L.rnf_grid_sample_workspace_bytes(C.byref(_lib.GridSample(Q=Q, g=g))) == want, (Q, g)
    assert 8 * -(-(1 << 26) // 64) == 8 << 20              # the prefix: 8 MiB per image at the most, 1/32 of the image
    for bad in (dict(Q=0), dict(Q=(1 << 26) + 1), dict(g=0), dict(g=65536)):
        kw = dict(Q=10, g=1)
        kw.update(bad)
        assert L.rnf_grid_sample_workspace_bytes(C.byref(_lib.GridSample(**kw))) == 0, bad
    short = _lib.GridSample(Q=10, g=1)
    short.struct_bytes -= 8
    assert L.rnf_grid_sample_workspace_bytes(C.byref(short)) == 0


def test_header_declares_the_structs_the_binding_mirrors():
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    for name, cls in (("RnfGridCellPoints", _lib.GridCellPoints), ("RnfGridSample", _lib.GridSample)):
        body = header[header.index("typedef struct %s {" % name) + len("typedef struct %s {" % name):header.index("} %s;" % name)]
        names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
        assert names == [f for f, _ in cls._fields_], names
    assert {"rnf_so3_grid_cell_points", "rnf_grid_sample", "rnf_grid_sample_workspace_bytes"} <= set(_lib.EXPORTS)
    methods = dict(re.findall(r"#define RNF_GRID_SAMPLE_(\w+) (\d+)", header))
    assert {k.lower(): int(v) for k, v in methods.items()} == _lib.GRID_SAMPLE_METHODS == METHODS
    assert "#define RNF_ABI_VERSION 8" in header and _lib.lib().rnf_abi_version() == 8         # the additions leave the ABI version alone
    csrc = os.path.join(root, "rotationnormflow_amd", "csrc")
    assert open(os.path.join(csrc, "grid_credible.h")).read().count("fixed_mass(") == 2          # its two uses; the one definition ..
    assert "u64 fixed_mass(" in open(os.path.join(csrc, "grid_mass.h")).read()                   # .. is shared with grid_sample.h
    assert "struct Philox" not in open(os.path.join(csrc, "sampler_kernel.h")).read()
    assert _host_lib().hgs_shift(C.c_longlong(72 * 8 ** 6)) == shift_of(72 * 8 ** 6) == 37


# ---- Python entry points: argument checks run before anything touches a device ----------------------------------------------------------
def _cpu_flow(**kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return Flow(make_config(layers=2, condition=1, feature_dim=16, rot="16Trans", **kw))


def test_python_entry_points_validate_their_arguments():
    assert harness.grid_sample is grid_pose.grid_sample and harness.grid_pose_sample is grid_pose.grid_pose_sample
    lp = torch.zeros(2, 576)
    for bad, word in ((dict(logp=torch.zeros(576)), "want"), (dict(n=0), "draws"), (dict(n=(1 << 30) + 1), "draws"), (dict(method="stratified"), "method"),
                      (dict(recursion_level=7), "recursion_level"), (dict(recursion_level=2), "rows"), (dict(offset=torch.eye(3)), "offset"),
                      (dict(recursion_level=1, offset=torch.zeros(4)), "offset"), (dict(logp=torch.zeros(1, 0)), "grid rows"),
                      (dict(seed=-1), "seed")):
        kw = dict(logp=lp, n=10)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            harness.grid_sample(**kw)
    with pytest.raises(RuntimeError, match="GPU only"):
        harness.grid_sample(lp, 10, recursion_level=1)
    idx, u = torch.zeros(5, dtype=torch.int64), torch.zeros(5, 3)
    for bad, word in ((dict(recursion_level=7), "level"), (dict(recursion_level=-1), "level"), (dict(index=idx.to(torch.int32)), "int64"),
                      (dict(u=torch.zeros(5, 2)), "u of shape"), (dict(u=torch.zeros(4, 3)), "u of shape"), (dict(offset=torch.zeros(4)), "offset")):
        kw = dict(index=idx, u=u, recursion_level=1)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            sd.grid_cell_points(**kw)
    with pytest.raises(RuntimeError, match="GPU only"):
        sd.grid_cell_points(idx, u, 1)
    fl, feat = _cpu_flow(), torch.zeros(2, 16)
    for bad in (dict(n=0), dict(recursion_level=7), dict(recursion_level=None), dict(temperature=0.0), dict(temperature=float("nan")),
                dict(method="residual")):
        kw = dict(n=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            harness.grid_pose_sample(fl, feat, **kw)
    with pytest.raises(RuntimeError, match="GPU only"):                 # valid arguments on CPU tensors: no CPU fallback
        harness.grid_pose_sample(fl, feat, 4, recursion_level=0)


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_grid_sample.cpp (its own main: the exact cases of this file, the poles, row 0 and row Q - 1, every degenerate
    image) built with the host-side address and undefined-behaviour sanitizers (-Xarch_host: host code only, nothing for the GPU) and
    run as a process of its own."""
    exe = str(tmp_path / "sanitize_grid_sample")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_grid_sample.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)
