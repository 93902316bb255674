"""CPU: the neighbour-limited kernel sum over the SO(3) grid (csrc/so3_grid_local.h, rnf_so3_grid_local_sum) and what is built on it.

``local_sum_fp64`` is the numpy fp64 restatement of the definition: brute force over ALL Q rows with the mask d^2 <= cut, from the same
fp32 inputs; tests/test_gpu_so3_grid_local.py imports it, the cases and the checks.  The fp32 membership test of the kernel and the fp64
d^2 of the restatement can disagree for pairs within delta = 4e-6 max(1, d2_cut) of the cut (twelve fp32 roundings of a d^2 up to 8), so
the restatement gives a BRACKET, not an exclusion: with the sets excl = {d^2 <= cut - delta} and incl = {d^2 <= cut + delta},
    count_excl <= count <= count_incl,    sum_excl - gate <= out <= sum_incl + gate,
gate = 1e-6 E + 4e-6 with E = (kappa/2) d^2 + |lw| of the largest term (the kernel sum's gate, tests/test_so3_kde_host.py).  No case is
left out.  Here the host build of the header (the kernel's row functions in the kernel's order) is held to the bracket at levels 0, 1
and 2, with and without an offset; symmetry of the neighbourhoods, the sentinels, the C ABI's refusals, the struct against its binding,
the Python argument checks and a sanitizer program are exercised without a device."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from rotationnormflow_amd import _lib, synth
from tests.test_so3_grid import _rx, _rz, healpix_grid_fp64
from tests.test_so3_kde_host import gate, log_normaliser, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_so3_grid_local.cpp")
OUT = os.path.join(HERE, "csrc", "_host_so3_grid_local.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f)
        for f in ("so3_grid_local.h", "so3_kernel_sum.h", "fisher_exact.h", "fisher_math.h")]
KAPPAS = (0.0, 4.0, 64.0, 1e4)
LEVELS = (0, 1, 2)


def _host_lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    return C.CDLL(OUT)


def host_local_sum(level, grid, queries, kappa, d2_cut, log_weights=None, offset=None, visited=False):
    """The host build of the kernel's arithmetic -> (float32 [G,m], int32 [m]); with ``visited`` also int32 [m], the rows each query's
    enumeration looked at"""
    h = _host_lib()
    Gr = np.ascontiguousarray(grid, np.float32).reshape(-1, 9)
    Qr = None if queries is None else np.ascontiguousarray(queries, np.float32).reshape(-1, 9)
    m = len(Gr) if Qr is None else len(Qr)
    lw = None if log_weights is None else np.ascontiguousarray(log_weights, np.float32).reshape(-1, len(Gr))
    G = 1 if lw is None else len(lw)
    off = None if offset is None else np.ascontiguousarray(offset, np.float32).reshape(9)
    out, count = np.empty((G, m), np.float32), np.empty(m, np.int32)
    seen = np.empty(m, np.int32) if visited else None
    h.hsgl_local_sum(int(level), ptr(off), ptr(Gr), ptr(Qr), ptr(lw), C.c_longlong(m), G, C.c_double(kappa), C.c_double(d2_cut), ptr(out), ptr(count),
                     ptr(seen))
    return (out, count, seen) if visited else (out, count)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def chord2(deg):
    """The squared chordal distance 4 (1 - cos omega) of a rotation angle in degrees"""
    return 4.0 * (1.0 - math.cos(math.radians(deg)))


def dist2_fp64(grid, queries, chunk=256):
    """|G_j - Q_i|_F^2 [m,Q] in fp64 from the fp32 entries (the squares of the nine differences)"""
    Gr = np.asarray(grid, np.float32).reshape(-1, 9).astype(np.float64)
    Qr = np.asarray(queries, np.float32).reshape(-1, 9).astype(np.float64)
    d2 = np.empty((len(Qr), len(Gr)))
    for i in range(0, len(Qr), chunk):
        diff = Qr[i:i + chunk, None, :] - Gr[None, :, :]
        d2[i:i + chunk] = np.einsum("ijk,ijk->ij", diff, diff)
    return d2


def delta_of(d2_cut):
    return 4e-6 * max(1.0, d2_cut)


def local_sum_fp64(d2, kappa, d2_cut, log_weights=None):
    """The bracket of out[g][i] = log sum_{j: d2 <= cut} exp(lw_gj) k_kappa from the fp64 distances d2 [m,Q]
    -> dict(lo, hi [G,m], count_lo, count_hi [m], E [G,m]): lo over d2 <= cut - delta, hi over d2 <= cut + delta; -inf where a set is empty or
    massless, NaN where a NaN log-weight lies inside; E = (kappa/2) d^2 + |lw| of hi's largest term."""
    m, Q = d2.shape
    lw = np.zeros((1, Q)) if log_weights is None else np.asarray(log_weights, np.float32).reshape(-1, Q).astype(np.float64)
    l_kappa, delta = float(log_normaliser(kappa)), delta_of(d2_cut)
    res = {}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for name, mask in (("lo", d2 <= d2_cut - delta), ("hi", d2 <= d2_cut + delta)):
            res["count_" + name] = mask.sum(axis=1)
            vals, Es = [], []
            for g in range(len(lw)):
                t = np.where(mask, lw[g][None, :] - 0.5 * kappa * d2, -np.inf)
                nan = (mask & np.isnan(lw[g])[None, :]).any(axis=1)
                t = np.where(np.isnan(t), -np.inf, t)
                top, at = t.max(axis=1), t.argmax(axis=1)
                safe = np.where(np.isfinite(top), top, 0.0)
                v = safe + np.log(np.exp(t - safe[:, None]).sum(axis=1)) - l_kappa
                v = np.where(np.isfinite(top), v, -np.inf)
                vals.append(np.where(nan, np.nan, v))
                Es.append(np.where(np.isfinite(top), 0.5 * kappa * d2[np.arange(m), at] + np.abs(np.nan_to_num(lw[g][at], posinf=0.0, neginf=0.0)), 0.0))
            res[name], res["E_" + name] = np.stack(vals), np.stack(Es)
    res["E"] = np.maximum(res["E_lo"], res["E_hi"])
    return res


def check_bracket(got, count, ref, what, missed_only=False):
    """out [G,m] and count [m] against the bracket; ``missed_only``: only that nothing is missed relative to brute force"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref["lo"].shape and count.shape == ref["count_lo"].shape, what
    assert (ref["count_lo"] <= count).all(), (what, "a neighbour is missed", int((ref["count_lo"] - count).max()))
    g = gate(ref["E"])
    with np.errstate(invalid="ignore"):
        below = got < ref["lo"] - g
    assert not np.isnan(got).any() and not below.any(), (what, "below the bracket", float(np.nanmax(np.where(below, ref["lo"] - got, 0.0))))
    if missed_only:
        return
    assert (count <= ref["count_hi"]).all(), (what, "a row beyond the cut is counted", int((count - ref["count_hi"]).max()))
    with np.errstate(invalid="ignore"):
        above = got > ref["hi"] + g
    assert not above.any(), (what, "above the bracket", float(np.nanmax(np.where(above, got - ref["hi"], 0.0))))
    empty = ref["count_hi"] == 0
    assert (count[empty] == 0).all() and np.isneginf(got[:, empty]).all(), what
    with np.errstate(invalid="ignore"):
        slack = np.where(np.isfinite(ref["lo"]) & np.isfinite(got), np.maximum(ref["lo"] - got, got - ref["hi"]) / g, -np.inf)
    return float(slack.max())


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

def offset_of(kind):
    """None, or a fixed non-trivial rotation [3,3] fp32"""
    return None if kind == "none" else synth.uniform_rotations(1, seed=41).astype(np.float32).reshape(3, 3)


@functools.lru_cache(maxsize=8)
def grid_of(level, kind):
    g = healpix_grid_fp64(level, offset=None if kind == "none" else offset_of(kind).astype(np.float64)).astype(np.float32)
    g.setflags(write=False)
    return g


def spacing_deg(level):
    return 360.0 / (6 * 2 ** level)


def cuts_of(level, nearest_d2):
    """0, below the nearest row, one grid spacing, 15, 60 and 180 degrees, and 8 (everything)"""
    return (0.0, 0.5 * nearest_d2, chord2(spacing_deg(level)), chord2(15.0), chord2(60.0), chord2(180.0), 8.0)


def special_queries(level, kind, n_random=24, seed=0):
    """Off-grid rotations [k,3,3] fp32 for the level and offset: the two poles exactly (Q O^T e_x = +-e_x) at several tilts, discs that
    cross phi = 0, discs that straddle the cap/belt boundaries (z = +-2/3), tilts next to 0 (a tilt window that wraps), and random ones.
    -> (queries, index of the first random one)"""
    O = np.eye(3) if kind == "none" else offset_of(kind).astype(np.float64)
    a = lambda *v: np.asarray(v, np.float64)                                # noqa: E731
    rows = []
    for tilt in (0.0, 0.3, 3.0):
        rows += [_rx(a(tilt))[0], (_rz(a(np.pi)) @ _rx(a(tilt)))[0]]         # the poles: Rz(pi) e_x = -e_x
    for theta in (0.4, np.arccos(2.0 / 3.0), 1.5, np.arccos(-2.0 / 3.0) + 0.02, 2.9):
        for phi in (0.004, -0.004 + 2 * np.pi):
            rows.append((_rx(a(phi)) @ _rz(a(theta)) @ _rx(a(1.0)))[0])      # across phi = 0, at and off the cap boundaries
        for tau in (0.003, 2 * np.pi - 0.003):
            rows.append((_rx(a(2.0)) @ _rz(a(theta)) @ _rx(a(tau)))[0])      # the tilt window wraps
    special = np.stack(rows) @ O
    rand = synth.uniform_rotations(n_random, seed=50 + seed + level).astype(np.float64).reshape(-1, 3, 3)
    return np.concatenate([special, rand]).astype(np.float32), len(special)


def log_weights_of(Q, G, seed):
    rng = np.random.default_rng(seed)
    lw = (2.0 * rng.standard_normal((G, Q))).astype(np.float32)
    if G > 1:
        lw[1, rng.permutation(Q)[:Q // 2]] = -np.inf
    return lw


@functools.lru_cache(maxsize=6)
def case(level, kind):
    """(grid, queries = every grid row then the special ones, fp64 distances [m,Q], index of the first off-grid query)"""
    grid = grid_of(level, kind)
    extra, _ = special_queries(level, kind)
    queries = np.concatenate([grid, extra])
    d2 = dist2_fp64(grid, queries)
    for x in (queries, d2):
        x.setflags(write=False)
    return grid, queries, d2, len(grid)


def check_level(fn, level, kind, kappas=KAPPAS, pick=None):
    """``fn(level, grid, queries, kappa, d2_cut, log_weights, offset)`` -> (out, count) against the bracket for every cut and kappa;
    ``pick``: indices into the case's queries (default: all)."""
    grid, queries, d2, n_grid = case(level, kind)
    if pick is not None:
        queries, d2 = queries[pick], d2[pick]
        off_grid = np.asarray(pick) >= n_grid
    else:
        off_grid = np.arange(len(queries)) >= n_grid
    nearest = float(d2[off_grid].min()) if off_grid.any() else 1e-3
    lw = log_weights_of(len(grid), 2, level)[1:]                           # one row, half of its entries -inf
    worst = 0.0
    for cut in cuts_of(level, nearest):
        for kappa in kappas:
            for w in (None, lw):
                out, count = fn(level, grid, queries, kappa, cut, w, offset_of(kind))
                ref = local_sum_fp64(d2, kappa, cut, w)
                worst = max(worst, check_bracket(out, count, ref, (level, kind, cut, kappa, w is not None)))
                if cut == 0.0:
                    assert (count[~off_grid] >= 1).all() and (count[off_grid] == 0).all()
                if cut == 8.0:                                          # everything, rows at 180 degrees whose fp32 d^2 rounds above 8 included
                    assert (count == len(grid)).all()
    print("level %d offset %s: worst distance beyond the bracket / gate %.3f" % (level, kind, worst))


def check_near_rotation(fn, level, kind):
    """Matrices that are rotations only to 1e-3: nothing is missed relative to brute force"""
    grid = grid_of(level, kind)
    rng = np.random.default_rng(7 + level)
    base, _ = special_queries(level, kind, n_random=16, seed=3)
    queries = (base.astype(np.float64) + 1e-3 * rng.uniform(-1, 1, base.shape)).astype(np.float32)
    d2 = dist2_fp64(grid, queries)
    for cut in cuts_of(level, float(d2.min())):
        for kappa in (4.0, 1e4):
            out, count = fn(level, grid, queries, kappa, cut, None, offset_of(kind))
            check_bracket(out, count, local_sum_fp64(d2, kappa, cut), (level, kind, cut, kappa, "near-rotation"), missed_only=True)


def check_sentinels(fn, level=1, kind="fixed"):
    grid = grid_of(level, kind)
    Q = len(grid)
    queries, _ = special_queries(level, kind)
    d2 = dist2_fp64(grid, queries)
    cut, delta = chord2(40.0), delta_of(chord2(40.0))
    assert not ((d2 > cut - delta) & (d2 <= cut + delta)).any()             # no pair at the cut: the sets are exact
    inside = d2 <= cut
    off = offset_of(kind)
    lw = np.zeros((3, Q), np.float32)
    lw[0, inside[0]] = -np.inf                                              # query 0: a massless neighbourhood
    lw[1, np.flatnonzero(inside[1])[0]] = np.nan                            # query 1: a NaN inside
    lw[2, np.flatnonzero(inside[2])[::2]] = -np.inf                         # query 2: half of its rows drop out
    out, count = fn(level, grid, queries, 16.0, cut, lw, off)
    assert np.array_equal(count, inside.sum(axis=1))
    assert np.isneginf(out[0, 0]) and np.isnan(out[1, 1])
    nan_free = ~inside[:, np.isnan(lw[1])].any(axis=1)
    assert np.isfinite(out[1, nan_free]).all() and np.isnan(out[1, ~nan_free]).all()    # NaN only where it lies inside
    ref = local_sum_fp64(d2, 16.0, cut, lw)
    ok = ~np.isnan(ref["hi"])
    assert np.array_equal(np.isnan(out), ~ok)
    fin = ok & np.isfinite(ref["hi"])
    assert (np.abs(out[fin] - ref["hi"][fin]) <= gate(ref["E"][fin])).all() and np.array_equal(np.isneginf(out), ok & np.isneginf(ref["hi"]))
    bad = queries.copy()
    bad[3, 1, 1], bad[5, 0, 2] = np.nan, np.inf
    bad[7] *= 4.0                                                           # finite, further than any cut from every rotation
    out, count = fn(level, grid, bad, 16.0, cut, None, off)
    assert np.isnan(out[0, [3, 5]]).all() and (count[[3, 5]] == 0).all()
    assert np.isneginf(out[0, 7]) and count[7] == 0
    rest = np.delete(np.arange(len(bad)), [3, 5, 7])
    assert np.isfinite(out[0, rest]).all() and np.array_equal(count[rest], inside.sum(axis=1)[rest])
    holes = grid.copy()
    holes[np.flatnonzero(inside[4])[0], 2] = np.nan                         # a grid row with a NaN entry is no member
    out2, count2 = fn(level, holes, queries, 16.0, cut, None, off)
    assert count2[4] == count[4] - 1 and np.isfinite(out2[0, 4])


# ---- tests -------------------------------------------------------------------------------------------------------------------------------

def test_soft_exp2_is_accurate_and_exact_at_zero():
    h = _host_lib()
    x = np.concatenate([-np.abs(np.random.default_rng(0).standard_normal(20000) * 30.0), [0.0, -0.5, -1.0, -124.99, -125.5, -1e30, -np.inf, np.nan]])
    x = x.astype(np.float32)
    y = np.empty_like(x)
    h.hsgl_exp2_soft(ptr(x), C.c_longlong(len(x)), ptr(y))
    want = np.exp2(x.astype(np.float64))
    live = x >= -125.0
    assert (np.abs(y[live] / want[live] - 1.0) <= 1.5e-7).all()
    assert y[len(x) - 8] == 1.0 and y[len(x) - 6] == 0.5 and (y[-4:-1] == 0.0).all() and np.isnan(y[-1])


def thinned(level, kind, stride=8):
    """Every ``stride``-th grid row and every off-grid query of the case"""
    _, queries, _, n_grid = case(level, kind)
    return np.concatenate([np.arange(0, n_grid, stride), np.arange(n_grid, len(queries))])


@pytest.mark.parametrize("kind", ["none", "fixed"])
@pytest.mark.parametrize("level", LEVELS)
def test_host_build_lies_in_the_bracket_for_every_cut_and_kappa(level, kind):
    """Every cut, every kappa, with and without log-weights; the queries are every grid row and the special ones.  At level 2 (4 658
    queries against 4 608 rows) every query runs every cut at kappa = 64, and every eighth grid row and every special query runs the
    full product: the restatement costs 1 s per combination on all of them."""
    if level < 2:
        check_level(host_local_sum, level, kind)
    else:
        check_level(host_local_sum, level, kind, kappas=(64.0,))
        check_level(host_local_sum, level, kind, pick=thinned(level, kind))


@pytest.mark.parametrize("kind", ["none", "fixed"])
@pytest.mark.parametrize("level", LEVELS)
def test_host_near_rotations_miss_nothing(level, kind):
    check_near_rotation(host_local_sum, level, kind)


def test_host_enumeration_is_a_superset_that_looks_at_each_row_once():
    """visited >= count, never more than Q (a row is looked at once however the windows overlap), and all of Q where the cut is 8"""
    for level in (0, 2):
        grid, queries, _, _ = case(level, "fixed")
        for cut in (0.0, chord2(spacing_deg(level)), chord2(60.0), 8.0):
            _, count, seen = host_local_sum(level, grid, queries[::5], 4.0, cut, None, offset_of("fixed"), visited=True)
            assert (seen >= count).all() and (seen <= len(grid)).all()
            if cut == 8.0:
                assert (seen == len(grid)).all()


def test_host_null_queries_are_the_grid_rows():
    grid = grid_of(1, "fixed")
    lw = log_weights_of(len(grid), 2, 5)
    a = host_local_sum(1, grid, None, 64.0, chord2(30.0), lw, offset_of("fixed"))
    b = host_local_sum(1, grid, grid, 64.0, chord2(30.0), lw, offset_of("fixed"))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("deg", [30.0, 15.0, 60.0])
def test_host_neighbourhoods_are_symmetric_at_level_1(deg):
    """j in N(i) <=> i in N(j): group j carries weight on row j alone, so that out[j][i] is finite exactly where j is in N(i)"""
    grid = grid_of(1, "fixed")
    Q = len(grid)
    lw = np.full((Q, Q), -np.inf, np.float32)
    lw[np.arange(Q), np.arange(Q)] = 0.0
    out, count = host_local_sum(1, grid, None, 0.0, chord2(deg), lw, offset_of("fixed"))
    member = np.isfinite(out)
    assert np.array_equal(member, member.T) and np.array_equal(member.sum(axis=0), count) and member.diagonal().all()


def test_host_sentinels():
    check_sentinels(host_local_sum)


def test_host_result_does_not_depend_on_the_batch():
    grid, queries, _, _ = case(2, "fixed")
    lw = log_weights_of(len(grid), 3, 9)
    pick = np.arange(0, len(queries), 7)
    whole, count = host_local_sum(2, grid, queries[pick], 64.0, chord2(15.0), lw, offset_of("fixed"))
    part, pcount = host_local_sum(2, grid, queries[pick][::-1][:100], 64.0, chord2(15.0), lw[2:], offset_of("fixed"))
    assert np.array_equal(whole[2:, ::-1][:, :100], part) and np.array_equal(count[::-1][:100], pcount)


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20


def _args(**kw):
    base = dict(level=2, offset=_FAKE, grid=_FAKE, queries=_FAKE * 2, log_weights=_FAKE, m=1000, G=3, kappa=64.0, d2_cut=0.5, out=_FAKE, count=_FAKE)
    base.update(kw)
    return _lib.So3GridLocalSum(**base)


def _refused(a, word):
    L = _lib.lib()
    assert L.rnf_so3_grid_local_sum(C.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def test_c_abi_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.rnf_abi_version() == 8
    for bad, word in ((dict(level=-1), "level="), (dict(level=7), "level="), (dict(G=0), "G="), (dict(G=65536), "G="), (dict(m=-1), "m="),
                      (dict(m=1 << 31), "m="), (dict(kappa=-1.0), "kappa="), (dict(kappa=1.0000001e6), "kappa="), (dict(kappa=float("nan")), "kappa="),
                      (dict(d2_cut=-1e-9), "d2_cut="), (dict(d2_cut=8.0000001), "d2_cut="), (dict(d2_cut=float("nan")), "d2_cut="),
                      (dict(d2_cut=float("inf")), "d2_cut="), (dict(grid=_FAKE + 4), "aligned"), (dict(queries=_FAKE + 8), "aligned"),
                      (dict(out=_FAKE + 2), "aligned"), (dict(log_weights=_FAKE + 1), "aligned"), (dict(count=_FAKE + 2), "aligned"),
                      (dict(offset=_FAKE + 3), "aligned"), (dict(queries=None), "null queries"), (dict(grid=None), "null"), (dict(out=None), "null")):
        _refused(_args(**bad), word)
    a = _args()
    a.struct_bytes += 8
    _refused(a, "struct_bytes")
    assert L.rnf_so3_grid_local_sum(C.byref(_args(m=0, out=None, grid=None))) == 0          # m = 0 is a no-op


def test_header_declares_the_struct_the_binding_mirrors():
    import re
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    body = header[header.index("typedef struct RnfSo3GridLocalSum {") + 34:header.index("} RnfSo3GridLocalSum;")]
    names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
    assert names == [f for f, _ in _lib.So3GridLocalSum._fields_], names
    assert "rnf_so3_grid_local_sum" in _lib.EXPORTS and "#define RNF_ABI_VERSION 8" in header
    device = open(os.path.join(root, "rotationnormflow_amd", "csrc", "so3_grid_local.h")).read()
    assert "bit-identical from" in device and "bit-identical from" in header and "NOT normalised" in header  # stated where callers read
    assert "__host__ __device__" in open(os.path.join(root, "rotationnormflow_amd", "csrc", "fisher_math.h")).read()   # RNF_FM_HD: the row functions


def test_python_entry_points_validate_their_arguments():
    from rotationnormflow_amd import grid_pose, harness
    from rotationnormflow_amd.utils import kde
    assert harness.grid_diffuse_local is grid_pose.grid_diffuse_local and harness.grid_filter_step is grid_pose.grid_filter_step
    assert harness.grid_pose_filter is grid_pose.grid_pose_filter and harness.so3_grid_local_log_sum is kde.so3_grid_local_log_sum
    grid = torch.zeros(72, 3, 3)
    with pytest.raises(ValueError, match="GPU"):
        kde.so3_grid_local_log_sum(grid, 0, 4.0)
    with pytest.raises(ValueError, match="grid"):
        kde.so3_grid_local_log_sum(torch.zeros(72, 9), 0, 4.0)
    with pytest.raises(ValueError, match="GPU"):
        grid_pose.grid_diffuse_local(torch.zeros(2, 72), grid, 0, 4.0)
    with pytest.raises(ValueError, match="grid"):
        grid_pose.grid_diffuse_local(torch.zeros(2, 72), torch.zeros(71, 3, 3), 0, 4.0)
    with pytest.raises(ValueError, match="log_likelihood"):
        grid_pose.grid_filter_step(torch.zeros(2, 72), torch.zeros(3, 72), grid, 0, 4.0)
    # the default radius: (kappa/2) d^2 = 18 nats, capped at 180 degrees
    assert kde.local_default_d2_cut(4.0) == 8.0 and kde.local_default_d2_cut(0.0) == 8.0
    assert abs(kde.local_default_d2_cut(64.0) - 36.0 / 64.0) < 1e-15
    assert abs(kde.local_radius_to_d2_cut(15.0) - chord2(15.0)) < 1e-15 and kde.local_radius_to_d2_cut(180.0) == 8.0
    for bad in (-1.0, 181.0, float("nan")):
        with pytest.raises(ValueError, match="radius_deg"):
            kde.local_radius_to_d2_cut(bad)


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_so3_grid_local.cpp (its own main: level 0 to 2 enumerations at every cut of this file, the poles and cut 8
    among them) built with the host-side address and undefined-behaviour sanitizers (-Xarch_host: host code only, nothing for the GPU)
    and run as a process of its own."""
    exe = str(tmp_path / "sanitize_so3_grid_local")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_so3_grid_local.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)
