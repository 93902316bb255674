"""CPU: the pairwise matrix-Fisher kernel sum (csrc/so3_kernel_sum.h, rnf_so3_kernel_sum) and what is built on it.

``kernel_sum_fp64`` is the numpy fp64 restatement of the definition -- difference form, explicit log-sum-exp, leave-one-out -- from
the same fp32 inputs; tests/test_gpu_so3_kde.py imports it, the cases and the gate.  Here the host build of the header (the same
arithmetic in the kernels' order) is held to it at the GPU gate, the normaliser l(kappa) to the Haar integral over the rotation angle,
and the edge cases, the C ABI's refusals, the workspace rule, the struct against its binding and the Python argument checks are
exercised without a device.

The gate, per output: |got - ref| <= 1e-6 E + 4e-6 with E = (kappa/2) d^2 + |lw| of the restatement's largest term.  The exponent takes
at most 12 fp32 roundings (9 subtractions, the squares and their sum of non-negative terms, the scaling): 12 * 2^-24 E = 7.2e-7 E; the
rest covers the fp32 exponential, the sums (fp32 over at most 64 terms of which the largest is 1, fp64 above) and the one rounding of
the output."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy import integrate, special

from rotationnormflow_amd import _lib, synth

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_so3_kernel_sum.cpp")
OUT = os.path.join(HERE, "csrc", "_host_so3_kernel_sum.so")
HDRS = [os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc", f) for f in ("so3_kernel_sum.h", "fisher_exact.h", "fisher_math.h")]
KAPPAS8 = tuple(2.0 ** k for k in range(0, 15, 2))                      # 1, 4, .. 16384
KAPPA1 = (64.0,)


def _host_lib():
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < newest:
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", OUT, SRC],
                       check=True)
    h = C.CDLL(OUT)
    h.hks_workspace_bytes.restype = C.c_ulonglong
    return h


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def log_normaliser(kappa):
    """l(kappa) = log(i0e(2 kappa) - i1e(2 kappa)), l(0) = 0 (scipy's Bessel functions)"""
    kappa = np.asarray(kappa, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(kappa == 0.0, 0.0, np.log(special.i0e(2 * kappa) - special.i1e(2 * kappa)))


def kernel_sum_fp64(centres, queries, kappas, log_weights=None, leave_one_out=False):
    """out[g][a][i] = log sum_j w_gj k_a(C_j, Q_i) (leave-one-out: j != i, minus log1p(-w_gi)) in fp64 from the fp32 inputs, with the
    edge cases of include/rnf_hip.h -> (out [G,J,m], E [G,J,m]): E = (kappa/2) d^2 + |lw| of each output's largest term."""
    Cn = np.asarray(centres, np.float32).reshape(-1, 9).astype(np.float64)
    Qr = Cn if queries is None else np.asarray(queries, np.float32).reshape(-1, 9).astype(np.float64)
    n, m = len(Cn), len(Qr)
    lw = np.zeros((1, n)) if log_weights is None else np.asarray(log_weights, np.float32).reshape(-1, n).astype(np.float64)
    G, J = len(lw), len(kappas)
    out, E = np.full((G, J, m), np.nan), np.zeros((G, J, m))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        diff = Qr[:, None, :] - Cn[None, :, :]
        d2 = np.einsum("ijk,ijk->ij", diff, diff)                        # [m,n]: squares of the nine differences
        del diff
        q_ok = np.isfinite(Qr).all(axis=1)
        c_ok = np.isfinite(Cn).all(axis=1)
        for g in range(G):
            live = lw[g] != -np.inf
            if np.isnan(lw[g]).any() or (live & ~c_ok).any() or not live.any() or np.isposinf(lw[g]).any():
                continue
            mx = lw[g][live].max()
            log_z = mx + np.log(np.exp(lw[g][live] - mx).sum())
            for a, kappa in enumerate(kappas):
                t = np.where(live[None, :], lw[g][None, :] - 0.5 * kappa * np.where(live[None, :], d2, 0.0), -np.inf)
                if leave_one_out:
                    t[np.arange(n), np.arange(n)] = -np.inf
                top = t.max(axis=1)
                at = t.argmax(axis=1)
                safe = np.where(np.isfinite(top), top, 0.0)
                lse = safe + np.log(np.exp(t - safe[:, None]).sum(axis=1))
                r = lse - log_z - float(log_normaliser(kappa))
                if leave_one_out:
                    w = np.exp(lw[g] - log_z)
                    r = np.where(w < 1.0, r - np.log1p(-np.minimum(w, 1.0)), np.nan)
                r = np.where(np.isfinite(top) & q_ok, r, np.nan)
                out[g, a] = r
                E[g, a] = 0.5 * kappa * np.where(live[at], d2[np.arange(m), at], 0.0) + np.abs(np.where(live[at], lw[g][at], 0.0))
    return out, np.nan_to_num(E, nan=0.0, posinf=0.0)


def gate(E):
    return 1e-6 * E + 4e-6


def host_kernel_sum(centres, queries, kappas, log_weights=None, leave_one_out=False):
    """The host build of the kernels' arithmetic -> float32 [G,J,m]"""
    h = _host_lib()
    Cn = np.ascontiguousarray(centres, np.float32).reshape(-1, 9)
    Qr = None if queries is None else np.ascontiguousarray(queries, np.float32).reshape(-1, 9)
    n, m = len(Cn), len(Cn) if Qr is None else len(Qr)
    lw = None if log_weights is None else np.ascontiguousarray(log_weights, np.float32).reshape(-1, n)
    G = 1 if lw is None else len(lw)
    kap = np.ascontiguousarray(kappas, np.float64)
    out = np.empty((G, len(kap), m), np.float32)
    h.hks_kernel_sum(ptr(Cn), ptr(Qr), ptr(lw), C.c_longlong(n), C.c_longlong(m), G, ptr(kap), len(kap), int(leave_one_out), ptr(out))
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

def rodrigues(v):
    """Rotation vectors [k,3] -> rotations [k,3,3] (fp64)"""
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v, axis=1)
    ax = v / np.where(th > 0, th, 1.0)[:, None]
    K = np.zeros((len(v), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    return np.eye(3) + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)


def draw(kind, k, seed):
    """k rotations [k,3,3] fp32: "uniform" (synth.uniform_rotations) or "clustered" (three fixed modes times Rodrigues rotations with
    N(0, 0.05^2) rotation vectors)"""
    if kind == "uniform":
        return synth.uniform_rotations(k, seed=seed).astype(np.float32).reshape(k, 3, 3)
    rng = np.random.default_rng(seed)
    modes = synth.uniform_rotations(3, seed=77).astype(np.float64).reshape(3, 3, 3)
    return (modes[rng.integers(0, 3, k)] @ rodrigues(0.05 * rng.standard_normal((k, 3)))).astype(np.float32)


def make_case(n, m, kind, weighted, seed=0):
    """Centres [n,3,3] of ``kind``; queries [m,3,3], half drawn the same way and half uniform; log-weights None or [3,n] whose row 1 has
    half its entries -inf."""
    Cn = draw(kind, n, 100 + seed + n)
    Qr = np.concatenate([draw(kind, m // 2, 200 + seed + m), draw("uniform", m - m // 2, 300 + seed + m)])
    lw = None
    if weighted:
        rng = np.random.default_rng(400 + seed + n)
        lw = (2.0 * rng.standard_normal((3, n))).astype(np.float32)
        lw[1, rng.permutation(n)[:n // 2]] = -np.inf
    return Cn, Qr, lw


@functools.lru_cache(maxsize=4)
def reference(n, m, kind, weighted):
    """(case, restatement for KAPPAS8, its E): computed once per case, shared by the J = 8 and the J = 1 checks"""
    case = make_case(n, m, kind, weighted)
    ref, E = kernel_sum_fp64(case[0], case[1], KAPPAS8, case[2])
    for a in (ref, E) + tuple(x for x in case if x is not None):
        a.setflags(write=False)
    return case, ref, E


def check_case(fn, n, m, kind, weighted):
    """``fn(centres, queries, kappas, log_weights, leave_one_out)`` -> [G,J,m] against the restatement on the gate, J = 8 and J = 1."""
    (Cn, Qr, lw), ref, E = reference(n, m, kind, weighted)
    pick = KAPPAS8.index(KAPPA1[0])
    for kappas, r, e in ((KAPPAS8, ref, E), (KAPPA1, ref[:, pick:pick + 1], E[:, pick:pick + 1])):
        got = np.asarray(fn(Cn, Qr, kappas, lw, False), np.float64)
        assert got.shape == r.shape and np.isfinite(r).all() and np.isfinite(got).all()
        err = np.abs(got - r)
        print("n %d m %d %s weighted %d J %d: worst |got - ref| / gate %.3f (|err| %.3g, E up to %.3g)" % (
            n, m, kind, weighted, len(kappas), (err / gate(e)).max(), err.max(), e.max()))
        assert (err <= gate(e)).all()


def check_leave_one_out(fn, n):
    Cn = draw("clustered", n, 500 + n)
    if n > 9:
        Cn[9] = Cn[5]                                                    # a duplicate at another index counts
    rng = np.random.default_rng(n)
    kappas = KAPPAS8 if n <= 65 else (4.0, KAPPAS8[-1])                  # the pairs grow as n^2: two bandwidths past one chunk
    for lw in (None, (2.0 * rng.standard_normal((2 if n <= 65 else 1, n))).astype(np.float32)):
        got = np.asarray(fn(Cn, None, kappas, lw, True), np.float64)
        ref, E = kernel_sum_fp64(Cn, None, kappas, lw, True)
        if n == 1:
            assert np.isnan(got).all() and np.isnan(ref).all()
            continue
        assert np.isfinite(got).all() and (np.abs(got - ref) <= gate(E)).all()
        if n > 9 and lw is None:                                         # the twin at distance 0 alone gives exp(-l) / (n - 1)
            want = -float(log_normaliser(KAPPAS8[-1])) - np.log(n - 1)
            assert got[0, -1, 5] >= want - 1e-4 and got[0, -1, 9] >= want - 1e-4


def check_edge_cases(fn):
    n, m = 130, 70
    Cn, Qr, lw = make_case(n, m, "uniform", True)
    dead = lw[1] == -np.inf
    bad = Cn.copy()
    bad[dead, 1, 1] = np.nan                                             # NaN entries where group 1 has no weight: groups 0 and 2 hold them
    got = fn(bad, Qr, KAPPA1, lw, False)
    ref, E = kernel_sum_fp64(bad, Qr, KAPPA1, lw)
    assert np.isnan(got[0]).all() and np.isnan(got[2]).all() and np.isfinite(got[1]).all()
    assert (np.abs(got[1] - ref[1]) <= gate(E[1])).all()
    clean, _ = kernel_sum_fp64(Cn, Qr, KAPPA1, lw)
    assert np.array_equal(ref[1], clean[1])                              # left out whatever its entries
    lwn = lw.copy()
    lwn[2, 129] = np.nan
    got = fn(Cn, Qr, KAPPA1, lwn, False)
    assert np.isnan(got[2]).all() and np.isfinite(got[:2]).all()
    lwd = lw.copy()
    lwd[0] = -np.inf
    got = fn(Cn, Qr, KAPPA1, lwd, False)
    assert np.isnan(got[0]).all() and np.isfinite(got[1:]).all()
    Qb = Qr.copy()
    Qb[3, 0, 2], Qb[69, 2, 2] = np.inf, np.nan
    got = fn(Cn, Qb, KAPPAS8, None, False)
    assert np.isnan(got[0, :, [3, 69]]).all() and np.isfinite(np.delete(got, [3, 69], axis=2)).all()
    one = np.full((1, n), -np.inf, np.float32)
    one[0, 17] = 0.25                                                    # all of the mass on one centre
    got = fn(Cn, None, KAPPA1, one, True)
    assert np.isnan(got[0, 0, 17]) and np.isfinite(np.delete(got[0, 0], 17)).all()
    got = fn(Cn, Qr, (0.0,), None, False)                                # kappa = 0: the uniform density
    assert np.abs(got).max() <= 4e-6


def check_far_queries(fn):
    """Centres within 3 degrees of the identity, a query 180 degrees away, kappa = 1e4: about -4e4, finite, on the gate."""
    rng = np.random.default_rng(5)
    v = rng.standard_normal((200, 3))
    v *= (np.deg2rad(3.0) * rng.uniform(0, 1, 200) / np.linalg.norm(v, axis=1))[:, None]
    Cn = rodrigues(v).astype(np.float32)
    Qr = np.diag([1.0, -1.0, -1.0]).astype(np.float32)[None]
    got = fn(Cn, Qr, (1e4,), None, False)
    ref, E = kernel_sum_fp64(Cn, Qr, (1e4,))
    assert np.isfinite(got).all() and -4.1e4 < got[0, 0, 0] < -3.9e4 and (np.abs(got - ref) <= gate(E)).all()


# ---- tests -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kappa", [0.0, 0.5, 3.0, 50.0, 1e3, 1e4])
def test_normaliser_is_the_integral_over_the_rotation_angle(kappa):
    """exp(l) = int_0^pi exp(2 kappa (cos t - 1)) (1 - cos t) / pi dt, the Haar integral of exp(kappa (tr R - 3))"""
    h = _host_lib()
    l = np.empty(1)
    h.hks_log_normaliser(ptr(np.array([kappa])), 1, ptr(l))
    f = lambda t: np.exp(-4.0 * kappa * np.sin(0.5 * t) ** 2) * 2.0 * np.sin(0.5 * t) ** 2 / np.pi     # noqa: E731
    cut = min(np.pi, 12.0 / np.sqrt(max(kappa, 1.0)))
    val = integrate.quad(f, 0.0, cut, epsabs=0.0, epsrel=1e-13, limit=400)[0]
    if cut < np.pi:
        val += integrate.quad(f, cut, np.pi, epsabs=0.0, epsrel=1e-13, limit=400)[0]
    assert abs(l[0] - np.log(val)) <= 1e-10 and abs(float(log_normaliser(kappa)) - np.log(val)) <= 1e-10
    if kappa == 0.0:
        assert l[0] == 0.0


@pytest.mark.parametrize("n,m", [(1, 1), (63, 65), (65, 65), (4097, 65)])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
@pytest.mark.parametrize("weighted", [False, True])
def test_host_build_against_the_restatement(n, m, kind, weighted):
    check_case(host_kernel_sum, n, m, kind, weighted)


@pytest.mark.parametrize("n", [1, 2, 65, 4097])
def test_host_leave_one_out(n):
    check_leave_one_out(host_kernel_sum, n)


def test_host_edge_cases():
    check_edge_cases(host_kernel_sum)


def test_host_far_queries_stay_finite():
    check_far_queries(host_kernel_sum)


def test_host_result_does_not_depend_on_the_batch():
    Cn, Qr, lw = make_case(4097, 300, "clustered", True)
    whole = host_kernel_sum(Cn, Qr, KAPPAS8, lw)
    assert np.array_equal(whole[:, :, 256:], host_kernel_sum(Cn, Qr[256:], KAPPAS8, lw))
    assert np.array_equal(whole[2:], host_kernel_sum(Cn, Qr, KAPPAS8, lw[2:]))
    assert np.array_equal(whole[:, 3:4], host_kernel_sum(Cn, Qr, KAPPAS8[3:4], lw))


# ---- the C ABI: every refusal below happens before a launch (the pointers are never dereferenced) ----------------------------------------
_FAKE = 1 << 20
_KAPPAS = (C.c_double * 8)(*KAPPAS8)


def _args(**kw):
    base = dict(centres=_FAKE, queries=_FAKE * 2, log_weights=_FAKE, n=4608, m=1000, G=3, kappas=C.cast(_KAPPAS, C.c_void_p), J=8, out=_FAKE)
    base.update(kw)
    a = _lib.So3KernelSum(**base)
    a.workspace, a.workspace_bytes = _FAKE, _lib.lib().rnf_so3_kernel_sum_workspace_bytes(C.byref(a))
    return a


def _refused(a, word):
    L = _lib.lib()
    assert L.rnf_so3_kernel_sum(C.byref(a)) != 0
    msg = L.rnf_last_error().decode()
    assert word in msg, msg


def test_c_abi_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.rnf_abi_version() == 8
    a = _args()
    assert a.workspace_bytes == (12 * 3 * 8 * 2 * 1000 + 16 * 3 * 2 + 8 * 3 + 15) // 16 * 16        # the rule of include/rnf_hip.h
    assert a.workspace_bytes == _host_lib().hks_workspace_bytes(C.c_longlong(4608), C.c_longlong(1000), 3, 8)
    for bad, word in ((dict(J=0), "J="), (dict(J=9), "J="), (dict(G=0), "G="), (dict(G=65536), "G="), (dict(n=0), "n="),
                      (dict(n=(1 << 24) + 1), "n="), (dict(m=-1), "m="), (dict(m=1 << 31), "m=")):
        _refused(_args(**bad), word)
        assert L.rnf_so3_kernel_sum_workspace_bytes(C.byref(_lib.So3KernelSum(**{**dict(n=10, m=10, G=1, J=1), **bad}))) == 0
    for k in (-1.0, 1.0000001e6, float("nan"), float("inf")):
        _refused(_args(kappas=C.cast((C.c_double * 8)(1.0, k, *KAPPAS8[2:]), C.c_void_p)), "kappas[1]")
    _refused(_args(kappas=None), "kappas")
    _refused(_args(centres=_FAKE + 4), "aligned")
    _refused(_args(queries=_FAKE + 8), "aligned")
    _refused(_args(leave_one_out=1), "leave_one_out")                    # m != n and other queries
    _refused(_args(leave_one_out=1, m=4608), "leave_one_out")            # other queries
    _refused(_args(leave_one_out=1, queries=None), "leave_one_out")      # m != n
    _refused(_args(queries=None), "null queries")
    _refused(_args(centres=None), "null")
    _refused(_args(out=None), "null")
    _refused(_args(G=65535, n=1 << 24, m=(1 << 31) - 1), "tile")         # a workspace no size_t holds
    a = _args()
    a.workspace_bytes -= 1
    _refused(a, "workspace")
    a = _args()
    a.workspace += 4
    _refused(a, "workspace")
    a = _args()
    a.struct_bytes += 8
    _refused(a, "struct_bytes")
    assert L.rnf_so3_kernel_sum_workspace_bytes(C.byref(a)) == 0
    assert L.rnf_so3_kernel_sum(C.byref(_args(m=0, out=None))) == 0       # m = 0 is a no-op
    assert L.rnf_so3_kernel_sum_workspace_bytes(C.byref(_args(m=0))) == (16 * 3 * 2 + 8 * 3 + 15) // 16 * 16


def test_header_declares_the_struct_the_binding_mirrors():
    import re
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "rnf_hip.h")).read()
    body = header[header.index("typedef struct RnfSo3KernelSum {") + 31:header.index("} RnfSo3KernelSum;")]
    names = [decl.split()[-1].lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")[:-1]]
    assert names == [f for f, _ in _lib.So3KernelSum._fields_], names
    assert {"rnf_so3_kernel_sum", "rnf_so3_kernel_sum_workspace_bytes"} <= set(_lib.EXPORTS)
    assert "#define RNF_ABI_VERSION 8" in header
    device = open(os.path.join(root, "rotationnormflow_amd", "csrc", "so3_kernel_sum.h")).read()
    assert "bit-identical from run to run" in device and "bit-identical from" in header      # the invariance is stated


def test_python_entry_points_validate_their_arguments():
    from rotationnormflow_amd import grid_pose, harness
    from rotationnormflow_amd.utils import kde
    R = torch.eye(3).expand(5, 3, 3).contiguous()
    with pytest.raises(ValueError, match="centres"):
        kde.so3_kernel_log_density(R, None, 4.0)                         # on the CPU
    with pytest.raises(ValueError, match="centres"):
        kde.so3_kernel_log_density(torch.zeros(5, 9), None, 4.0)
    with pytest.raises(ValueError, match="rotations"):
        kde.SO3KernelDensity.fit(R)
    with pytest.raises(ValueError, match="rotations"):
        kde.SO3KernelDensity(R, 4.0)
    with pytest.raises(ValueError, match="kappa"):
        kde.SO3KernelDensity.fit(R, kappas=[4.0, 2e6])
    with pytest.raises(ValueError, match="rotations"):
        harness.kde_baseline(R, R)
    with pytest.raises(ValueError, match="grid"):
        harness.grid_diffuse(torch.zeros(2, 72), torch.zeros(71, 3, 3), 4.0)
    with pytest.raises(ValueError, match="GPU"):
        grid_pose.grid_diffuse(torch.zeros(2, 72), torch.zeros(72, 3, 3), 4.0)
    assert harness.grid_diffuse is grid_pose.grid_diffuse and len(kde.DEFAULT_KAPPAS) == 25
    assert kde.DEFAULT_KAPPAS[0] == 4.0 and kde.DEFAULT_KAPPAS[-1] == 16384.0


def test_stand_alone_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/csrc/sanitize_so3_kernel_sum.cpp (its own main: ragged sizes, -inf weights, NaN rows, leave-one-out with n = 1) built with
    the host-side address and undefined-behaviour sanitizers (-Xarch_host: host code only, nothing for the GPU) and run as a process of
    its own."""
    exe = str(tmp_path / "sanitize_so3_kernel_sum")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O1", "-g", "-ffp-contract=off"] + san
                   + ["-o", exe, os.path.join(HERE, "csrc", "sanitize_so3_kernel_sum.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", (run.stdout, run.stderr)
