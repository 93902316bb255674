"""CPU: the launch plan of rnf_flow_pass (csrc/flow_plan.h, compiled for the host) against what the library launched BEFORE the plan
existed.

tests/golden/flow_plan_parent.json is a kernel trace (rocprofv3 --kernel-trace) of the commit named in the file, taken by
tools/record_flow_plan.py on the compute-unit count named in the file: per call of rnf_flow_pass the descriptor, the fields of the pass
struct, and the ordered launches -- kernel name (= the instantiation), workgroup size, grid size.  The planner must reproduce every one of
them.  The trace's LDS column holds the STATIC group segment only (0 for every kernel with dynamic LDS), so the dynamic LDS bytes are
pinned by ``test_dynamic_lds_bytes`` from the layout arithmetic of csrc/layout.h written out by hand.

The stated invariants are checked over the recorded calls and a sweep of n, segments and switches around them."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from rotationnormflow_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "host_flow_plan.cpp")
OUT = os.path.join(HERE, "csrc", "_host_flow_plan.so")
CSRC = os.path.join(os.path.dirname(HERE), "rotationnormflow_amd", "csrc")
HDRS = [os.path.join(CSRC, "flow_plan.h"), os.path.join(CSRC, "layout.h"), os.path.join(os.path.dirname(HERE), "include", "rnf_hip.h")]
RECORD = json.load(open(os.path.join(HERE, "golden", "flow_plan_parent.json")))
CUS = RECORD["cus"]

ROW, MEMSET, PROJECTION, STACK, FINALIZE = 16, 0, 1, 2, 3
FILL = "__amd_rocclr_fillBufferAligned"                  # what hipMemsetAsync of the guard words shows as
PROJ_NAMES = ["rnf::featproj_ksplit_kernel(rnf::FeatProjArgs)", "void rnf::featproj_kernel<8, 1, true>(rnf::FeatProjArgs)",     # enum ProjKernel
              "void rnf::featproj_kernel<8, 1, false>(rnf::FeatProjArgs)", "void rnf::featproj_kernel<8, 0, false>(rnf::FeatProjArgs)"]
FINALIZE_NAME = "rnf::nll_finalize_kernel(double const*, int, double, double*, int, double const*, int, int const*)"
SUMMARY = ("family", "ext", "rows", "prec", "fb_prec", "guarded", "pipe", "fused", "ws_need", "kt_inv", "rf_first4", "n_slots")
SWITCH_ENV = {"RNF_WIDE": "wide", "RNF_STAGING": "staging_dma", "RNF_GUARD": "guard", "RNF_LEAN": "lean", "RNF_FAIR": "fair"}
DEFAULT_SWITCHES = dict(wide=1, staging_dma=1, guard=1, lean=1, fused=0, fair=1, rf_first=0)


@pytest.fixture(scope="module")
def fpl():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", OUT, SRC], check=True)
    return C.CDLL(OUT)


def key_name(k):
    b = ("false", "true")
    return (f"void rnf::flow_stack_kernel<{k[0]}, {k[1]}, {k[2]}, {b[k[3]]}, {k[4]}, {b[k[5]]}, {k[6]}, {b[k[7]]}, {b[k[8]]}>"
            "(rnf::FlowArgs)")


def switches_of(case, call):
    sw = dict(DEFAULT_SWITCHES, fused=call["fused"])
    for name in case["env"]:
        sw[SWITCH_ENV[name]] = 0                          # the recorded groups flip one switch each: "0", or RNF_STAGING=sync
    return sw


def plan(fpl, desc, call, sw, cus=CUS):
    """-> (launch rows, summary dict) or the refusal text"""
    d = np.ascontiguousarray(desc, np.int32)
    fields = np.array([call["dir"], call["n"], call["n_layers"], call["segments"], call["feature_dim"], call["feature_div"], call["feature"],
                       call["side"], call["states"], call["sum_out"], call["workspace"], call["workspace_bytes"], call["in_place"]], np.int64)
    s = np.array([sw[k] for k in ("wide", "staging_dma", "guard", "lean", "fused", "fair", "rf_first")], np.int32)
    rows = np.zeros((256, ROW), np.int64)
    summary = np.zeros(len(SUMMARY), np.int64)
    err = C.create_string_buffer(512)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    count = fpl.fp_plan(p(d), p(fields), cus, p(s), p(rows), len(rows), p(summary), err, len(err))
    if count < 0:
        return err.value.decode()
    return rows[:count], dict(zip(SUMMARY, summary.tolist()))


def as_trace(rows):
    """planner rows -> what the kernel trace shows: [name, workgroup size, grid size in work-items, static LDS bytes]"""
    out = []
    for r in rows.tolist():
        if r[0] == MEMSET:
            out.append([FILL])
        elif r[0] == PROJECTION:
            out.append([PROJ_NAMES[r[2]], r[11], r[11] * r[12], 0])
        elif r[0] == FINALIZE:
            out.append([FINALIZE_NAME, 256, 256, 2048])   # 256 doubles of static LDS
        else:
            assert r[0] == STACK, "the planner emitted a key the dispatcher does not hold"
            out.append([key_name(r[2:11]), r[11], r[11] * r[12], 0])
    return out


def recorded_calls():
    for case in RECORD["cases"]:
        for i, call in enumerate(case["calls"]):
            yield case, i, call


def test_record_says_where_it_comes_from():
    assert RECORD["commit"] and RECORD["cus"] > 0 and str(RECORD["cus"]) in RECORD["about"] and RECORD["commit"] in RECORD["about"]
    assert len(RECORD["cases"]) > 300 and not [c["case"] for c in RECORD["cases"] if c.get("error")]


def test_planner_reproduces_every_recorded_launch(fpl):
    bad = []
    for case, i, call in recorded_calls():
        got = plan(fpl, RECORD["descs"][call["desc"]], call, switches_of(case, call))
        assert not isinstance(got, str), (case["case"], got)
        mine = as_trace(got[0])
        theirs = [[l[0]] if l[0] == FILL else l for l in call["launches"]]       # (the fill kernel's geometry is the runtime's business)
        if mine != theirs:
            bad.append((case["case"], i, [m for m, t in zip(mine, theirs) if m != t][:2], [t for m, t in zip(mine, theirs) if m != t][:2],
                        len(mine), len(theirs)))
    assert not bad, f"{len(bad)} calls differ, first: {bad[:3]}"


def test_dynamic_lds_bytes(fpl):
    """layout.h by hand: a K = 64 f16x2 layer image is 12736 + 8 * 2080 = 29376 floats = 117504 bytes; + 64 bytes of governor words on
    the forward pass; + two affine blocks of 112 floats (896 bytes).  The bf16x3 re-run: three ring regions of 4 * (3072 + 32) floats
    (148992 bytes) + 896.  FUSED: + one projection out tile of 16 * 512 + 32 floats (32896 bytes).  Projections: two DMA buffers of
    16 k-steps x 512 floats (65536 bytes) in split precision, F / 8 * 256 floats in exact fp32, and the K-split's 2 x 64 KiB weights +
    2 x 16 KiB exchange slots (163840 bytes)."""
    by_name = {c["case"]: c for c in RECORD["cases"]}

    def lds(name):
        case = by_name[name]
        rows, _ = plan(fpl, RECORD["descs"][case["calls"][0]["desc"]], case["calls"][0], switches_of(case, case["calls"][0]))
        return [(int(r[0]), int(r[1]), int(r[13])) for r in rows.tolist() if r[0] in (PROJECTION, STACK)]

    assert lds("C2/fwd/n1024") == [(STACK, 0, 117504 + 64 + 896), (STACK, 1, 148992 + 896)]
    assert lds("C2/inv/n1024") == [(STACK, 0, 117504 + 896), (STACK, 1, 148992 + 896)]
    assert lds("C2/fp32/fwd/n4096") == [(STACK, 0, 117504 + 896)]
    assert lds("C2/bf16x3/fwd/n4096") == [(STACK, 0, 148992 + 896)]
    assert lds("C4/fwd/n1024") == [(PROJECTION, 0, 65536), (STACK, 0, 118464), (PROJECTION, 1, 256 // 8 * 256 * 4), (STACK, 1, 149888)]
    assert lds("C5/fwd/n1024")[0] == (PROJECTION, 0, 163840) and lds("C5/fwd/n1024")[2] == (PROJECTION, 1, 32768)
    assert lds("fused/C4/fwd/n4096")[0] == (STACK, 0, 118464 + 32896)
    assert lds("K96/inv/n4096")[0] == (STACK, 0, 117504)          # 8 of 12 tiles resident, synchronous staging: no affine blocks
    # fewer segments: 12736 + KT * 2080 floats with KT = 1, 2, 4 tiles resident, + 896 (inverse: no governor words)
    assert lds("K8/inv/n4096") == [(STACK, 0, (12736 + 2080) * 4 + 896), (STACK, 1, 148992 + 896)]
    assert lds("K16/inv/n4096")[0] == (STACK, 0, (12736 + 2 * 2080) * 4 + 896)
    assert lds("K32/inv/n4096")[0] == (STACK, 0, (12736 + 4 * 2080) * 4 + 896)
    assert lds("K12/fwd/n4096")[0] == (STACK, 0, (12736 + 2 * 2080) * 4 + 64 + 896)
    # the extended and the shared-row kernels share the K = 64 layout; the exact-fp32 re-run of a device-packed flow shares the primary's
    assert lds("cond9/f16x2/fwd/n4096")[1] == (STACK, 0, 118464) and lds("cond36/f16x2/inv/n4096")[1] == (STACK, 0, 118400)
    assert lds("C4/f16x2/rows512/fwd/n4096") == [(PROJECTION, 0, 65536), (STACK, 0, 118464), (PROJECTION, 1, 32768), (STACK, 1, 149888)]
    assert lds("C4/f16x2/rows512/inv/n4096")[1] == (STACK, 0, 118400) and lds("C4/f16x2/rows16/fwd/n4096")[1] == (STACK, 0, 118464)
    assert lds("C4/f16x2/device-packed/fwd/n4096")[1::2] == [(STACK, 0, 118464), (STACK, 1, 118464)]
    assert lds("F1024/f16x2/fwd/n4096")[0] == (PROJECTION, 0, 65536) and lds("F1024/fp32/fwd/n4096")[0] == (PROJECTION, 0, 32768)
    assert lds("K96/cond9/fp32/inv/n4096")[1] == (STACK, 0, 117504) and lds("K200/inv/n4096")[0] == (STACK, 0, 117504)
    # a 6x6 conditional layer keeps its TWO fc_last tiles resident even where the Moebius layers have one (K = 8)
    case = by_name["cond36/f16x2/fwd/n4096"]
    rows, _ = plan(fpl, RECORD["descs"][case["calls"][0]["desc"]], dict(case["calls"][0], segments=8), switches_of(case, case["calls"][0]))
    assert [int(r[13]) for r in rows.tolist() if r[0] == STACK][0] == (12736 + 2 * 2080) * 4 + 64 + 896
    # no conditioner at all would be 256 bytes (the block partials of a 16-wave workgroup); a training forward (general family, governor on)
    assert lds("C2/training/fwd/n16384") == [(STACK, 0, 118464)]


def sweep_sizes(div):
    ns = {1, 2, 31, 32, 33, 1000, 50001, (1 << 22)}
    for e in range(5, 23):
        ns |= {(1 << e) - 1, 1 << e, (1 << e) + 1}
    for t in (CUS * 4 * 32, CUS * 8 * 32, 1 << 18):
        ns |= {t - 1, t, t + 1, 2 * t + 5}
    if div:
        ns = {max(1, n // div) * div for n in ns}
    return sorted(n for n in ns if n <= (1 << 22))


def test_invariants_and_coverage_of_the_built_instantiations(fpl):
    """Family, ext, rows mode, precisions and `guarded` are fixed by the flow and the call, never by n or the chunk; only the width and the
    grids move.  The workspace the plan asks for is what rnf_flow_pass_workspace_bytes answers.  Every key the planner emits is in the
    dispatcher's list, and every listed instantiation is reached."""
    L = _lib.lib()
    keys = np.zeros((4096, 9), np.int64)
    n_built = fpl.fp_built_keys(keys.ctypes.data_as(C.c_void_p))
    assert n_built == 80                                   # the library's flow_stack_kernel count (nm -C librnf_hip.so | grep __device_stub__)
    built = {tuple(k) for k in keys[:n_built].tolist()}
    seen = set()
    configs = {}
    for case, i, call in recorded_calls():
        sw = switches_of(case, call)
        fixed = {k: v for k, v in call.items() if k not in ("n", "launches", "workspace_bytes")}
        configs.setdefault(json.dumps([fixed, sw], sort_keys=True), (fixed, sw))
    assert len(configs) > 60
    for fixed, sw in configs.values():
        desc = RECORD["descs"][fixed["desc"]]
        table = np.ascontiguousarray(desc, np.int32)
        variants = [(fixed["segments"], sw)]
        # the plan does not read the blob, so the same descriptor stands for the flow with other segment counts and staging modes
        variants += [(K, dict(sw, staging_dma=st)) for K in (8, 16, 32, 64, 96) for st in (0, 1) if (K, st) != (fixed["segments"], sw["staging_dma"])]
        for K, sw_v in variants:
            stable = None
            for n in sweep_sizes(fixed["feature_div"]):
                call = dict(fixed, n=n, segments=K, workspace_bytes=1 << 60)
                got = plan(fpl, desc, call, sw_v)
                assert not isinstance(got, str), (fixed, K, n, got)
                rows, summary = got
                assert all(r[0] != -1 for r in rows.tolist()), (fixed, K, n)
                seen |= {tuple(r[2:11]) for r in rows.tolist() if r[0] == STACK}
                if K == fixed["segments"]:
                    q = _lib.FlowPass(dir=call["dir"], n=n, feature_div=call["feature_div"], desc=table.ctypes.data,
                                      n_layers=call["n_layers"], segments=K)
                    assert L.rnf_flow_pass_workspace_bytes(q) == summary["ws_need"], (fixed, n)
                now = {k: summary[k] for k in ("family", "ext", "rows", "prec", "fb_prec", "guarded", "pipe", "fused", "kt_inv")}
                stable = stable or now
                assert now == stable, (fixed, K, n, now, stable)
                chunks = {}
                for r in rows.tolist():                    # ... nor by the chunk: one key per (primary / fallback) up to the width
                    if r[0] == STACK:
                        chunks.setdefault(r[1], set()).add(tuple(r[2:4] + r[5:11]))
                assert all(len(v) == 1 for v in chunks.values()), (fixed, K, n)
    assert seen <= built
    assert seen == built, f"never emitted: {sorted(built - seen)}"
