#!/usr/bin/env python3
"""Record what rnf_flow_pass launches, case by case (tests/golden/flow_plan_parent.json; tests/test_flow_plan.py replays the record through the
host-built planner of csrc/flow_plan.h).

    python tools/record_flow_plan.py record OUT.json      one rocprofv3 --kernel-trace run per case group (a fresh child process each: the
                                                          library reads its environment switches once), merged into OUT.json
    python tools/record_flow_plan.py compare A.json B.json   launches and output CRCs of two records, case by case; exit 1 on a difference
    python tools/record_flow_plan.py run GROUP CALLS.json    (what `record` starts under the profiler)

Per call of rnf_flow_pass the record holds the fields of RnfFlowPass the launch plan depends on, the descriptor table, and the ordered
kernel launches of the trace between two marker launches: kernel name, workgroup size, grid size (work-items) and LDS bytes.  Per case it
holds a CRC of the outputs, so that a second recording also shows whether the same bits came out.  Flows are built from configs.py presets
and synth weights only."""
import contextlib
import csv
import glob
import io
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARKER = "matrix_to_quaternion_kernel"          # launched before and after every rnf_flow_pass: the trace is cut at these
# environment switches, each read once by the library (and RNF_GUARD by the runtime): one child process per group
GROUPS = {"default": {}, "wide0": {"RNF_WIDE": "0"}, "sync": {"RNF_STAGING": "sync"}, "guard0": {"RNF_GUARD": "0"}, "lean0": {"RNF_LEAN": "0"},
          "fair0": {"RNF_FAIR": "0"}}
SIZES = (1 << 10, 1 << 15, (1 << 15) + 1, 1 << 16, (1 << 16) + 1, 1 << 20, 50001)
SMALL_LARGE = (4096, 1 << 17)


# ---- the cases ------------------------------------------------------------------------------------------------------
def run_group(group, out_path):
    import numpy as np
    import torch

    from rotationnormflow_amd import _lib, make_config, runtime, synth
    from rotationnormflow_amd.flow.flow import Flow

    dev = torch.device("cuda", 0)
    L = _lib.lib()
    calls, descs, cases = [], [], []
    mark_in = torch.from_numpy(synth.uniform_rotations(1, seed=3)).to(dev)
    mark_out = torch.empty(4, device=dev)

    def marker():
        _lib.check(L.rnf_matrix_to_quaternion(mark_in.data_ptr(), 1, mark_out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))

    real_pass = L.rnf_flow_pass

    def traced_pass(p):
        q = p._obj if hasattr(p, "_obj") else p
        table = np.ctypeslib.as_array((_lib.C.c_int32 * (q.n_layers * runtime.DESC_STRIDE)).from_address(q.desc)).tolist()
        if table not in descs:
            descs.append(table)
        calls.append(dict(dir=q.dir, n=q.n, n_layers=q.n_layers, segments=q.segments, feature_dim=q.feature_dim, feature_div=q.feature_div,
                          feature=bool(q.feature), side=bool(q.side), states=bool(q.states), sum_out=bool(q.sum_out), workspace=bool(q.workspace),
                          workspace_bytes=q.workspace_bytes, in_place=bool(q.rotation_out) and q.rotation_out == q.rotation,
                          fused=fused_now[0], desc=descs.index(table)))
        marker()
        rc = real_pass(p)
        marker()
        return rc

    L.rnf_flow_pass = traced_pass
    fused_now = [0]

    gen = torch.Generator(device=dev)
    rot_all = torch.from_numpy(synth.uniform_rotations(1 << 20, seed=2)).to(dev)

    def feats(rows, F):
        gen.manual_seed(1000 + F)
        return torch.randn((rows, F), generator=gen, device=dev, dtype=torch.float32)

    flows = {}

    def flow(preset=None, precision="f16x2", **over):
        key = (preset, precision, tuple(sorted(over.items())))
        if key not in flows:
            flows.clear()                                  # one flow resident at a time
            cfg = make_config(preset, **over)
            runtime.set_precision(precision)
            with contextlib.redirect_stdout(io.StringIO()):
                fl = Flow(cfg)
            w = synth.fill_state_dict({k: tuple(v.shape) for k, v in fl.state_dict().items()}, seed=1, regime="default")
            fl.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
            flows[key] = fl.to(dev).eval()
        runtime.set_precision(precision)
        return flows[key]

    def crc(t):
        return None if t is None else zlib.crc32(t.detach().cpu().numpy().tobytes())

    def case(name, fn):
        first = len(calls)
        try:
            outs = fn()
            torch.cuda.synchronize()
            result = dict(crc=[crc(t) for t in outs])
        except (RuntimeError, NotImplementedError) as e:
            # a refusal of the library or of the packers is part of the record; anything the HIP runtime reports ends the run
            if "failed:" in str(e) or "HIP" in str(e):
                raise
            result = dict(crc=None, error=str(e)[:200])
        cases.append(dict(case=name, calls=list(range(first, len(calls))), **result))
        print(name, flush=True)

    def evaluate(fl, n, inverse=False, repeat=None, logp=False):
        R = rot_all[:n]
        f = feats(n // (repeat or 1), fl.feature_dim) if fl.condition else None
        with torch.no_grad():
            if logp:
                r = fl.log_prob(R, f, return_rotation=True, feature_repeat=repeat)
                return r["rotation"], r["logp"], r["sum"]
            return fl.inverse(R, f, feature_repeat=repeat) if inverse else fl(R, f, feature_repeat=repeat)

    def in_place(fl, n):                                   # rotation_out == rotation: the C ABI directly (the Python layer never aliases)
        R = rot_all[:n].clone()
        f = feats(n, fl.feature_dim) if fl.condition else None
        packed = fl._packed(dev, f)
        ldj = torch.empty(n, device=dev)
        p = _lib.FlowPass(dir=0, rotation=R.data_ptr(), feature=f.data_ptr() if f is not None else None, n=n, feature_dim=packed.feat_padded,
                          blob=packed.blob.data_ptr(), desc=packed.desc.ctypes.data, n_layers=packed.n_layers, segments=packed.segments,
                          rotation_out=R.data_ptr(), ldj_out=ldj.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        ws = runtime.workspace(dev, L.rnf_flow_pass_workspace_bytes(p))
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
        _lib.check(L.rnf_flow_pass(p))
        return R, ldj

    def training(fl, n, inverse=False):                    # grad mode: the pass saves the per-layer states
        fl.train()
        try:
            R = rot_all[:n]
            f = feats(n, fl.feature_dim) if fl.condition else None
            out = fl.inverse(R, f) if inverse else fl(R, f)
        finally:
            fl.eval()
        return [t.detach() for t in out]

    def device_packed(fl, n, inverse=False):               # training mode without a gradient: images packed on the device
        fl.train()
        try:
            return evaluate(fl, n, inverse)
        finally:
            fl.eval()

    if group != "default":                                 # one switch flipped: the two headline presets, small and large
        for preset in ("C2", "C4"):
            for inverse in (False, True):
                for n in (1 << 10, 1 << 17):
                    case(f"{group}/{preset}/{'inv' if inverse else 'fwd'}/n{n}", lambda: evaluate(flow(preset), n, inverse))
            case(f"{group}/{preset}/logp/n4096", lambda: evaluate(flow(preset), 4096, logp=True))
    else:
        for preset in ("C1", "C2", "C4", "C5", "C5u"):
            for inverse in (False, True):
                for n in SIZES:
                    case(f"{preset}/{'inv' if inverse else 'fwd'}/n{n}", lambda: evaluate(flow(preset), n, inverse))
        for preset in ("C2", "C4"):
            for n in SMALL_LARGE + ((1 << 18) + 5,):
                case(f"{preset}/logp/n{n}", lambda: evaluate(flow(preset), n, logp=True))
            for precision in ("fp32", "bf16x3"):
                for inverse in (False, True):
                    for n in SMALL_LARGE:
                        case(f"{preset}/{precision}/{'inv' if inverse else 'fwd'}/n{n}", lambda: evaluate(flow(preset, precision), n, inverse))
            for precision in ("f16x2", "fp32", "bf16x3"):
                for inverse in (False, True):
                    for n in SMALL_LARGE:
                        case(f"{preset}/{precision}/device-packed/{'inv' if inverse else 'fwd'}/n{n}",
                             lambda: device_packed(flow(preset, precision), n, inverse))
            for n in SMALL_LARGE:
                case(f"{preset}/in-place/n{n}", lambda: in_place(flow(preset), n))
            for inverse in (False, True):
                for n in (1 << 14, 1 << 17):
                    case(f"{preset}/training/{'inv' if inverse else 'fwd'}/n{n}", lambda: training(flow(preset), n, inverse))
        # shared feature rows: the extended kernel (16 rotations per row) and the ROWS kernels (512 per row)
        for preset, precision in (("C4", "f16x2"), ("C5", "f16x2"), ("C4", "fp32"), ("C4", "bf16x3")):
            for repeat in (16, 512):
                for inverse in (False, True):
                    for n in (1 << 12, 1 << 18):
                        case(f"{preset}/{precision}/rows{repeat}/{'inv' if inverse else 'fwd'}/n{n}",
                             lambda: evaluate(flow(preset, precision), n, inverse, repeat))
                case(f"{preset}/{precision}/rows{repeat}/logp/n{1 << 12}", lambda: evaluate(flow(preset, precision), 1 << 12, repeat=repeat, logp=True))
        # layer kinds of the extended instantiation: conditional 3x3 and 6x6, side matrices; the unconditional 3x3 / 6x6 of the general one
        small = dict(layers=4, feature_dim=64)
        for tag, over in (("cond9", dict(condition=1, rot="9TransLSmith", **small)), ("cond36", dict(condition=1, rot="36Trans", **small)),
                          ("side16rot", dict(condition=1, rot="16Rot", **small)), ("side16lu", dict(condition=1, rot="16Trans", lu=1, **small)),
                          ("gs9", dict(rot="9TransLSmith", layers=4)), ("gs36", dict(rot="36Trans", layers=4))):
            for precision in ("f16x2", "fp32", "bf16x3"):
                for inverse in (False, True):
                    for n in SMALL_LARGE:
                        case(f"{tag}/{precision}/{'inv' if inverse else 'fwd'}/n{n}", lambda: evaluate(flow(None, precision, **over), n, inverse))
        for tag, over in (("cond9", dict(condition=1, rot="9TransLSmith", **small)), ("cond36", dict(condition=1, rot="36Trans", **small))):
            for inverse in (False, True):
                case(f"{tag}/rows512/{'inv' if inverse else 'fwd'}/n4096", lambda: evaluate(flow(None, **over), 4096, inverse, 512))
        # segments: kt_inv 1 .. 16 and the stash of the inverse, synchronous staging of the forward above 64
        for K in (8, 12, 16, 32, 64, 96, 128, 200):
            for n in SMALL_LARGE:
                case(f"K{K}/inv/n{n}", lambda: evaluate(flow(None, layers=4, segments=K), n, True))
            case(f"K{K}/fwd/n4096", lambda: evaluate(flow(None, layers=4, segments=K), 4096))
        for K in (8, 96, 200):
            for precision in ("f16x2", "fp32", "bf16x3"):
                for tag, over in (("cond16", dict(condition=1, rot="16Trans", **small)), ("cond9", dict(condition=1, rot="9TransLSmith", **small))):
                    for inverse in (False, True):
                        case(f"K{K}/{tag}/{precision}/{'inv' if inverse else 'fwd'}/n4096",
                             lambda: evaluate(flow(None, precision, segments=K, **over), 4096, inverse))
            if K <= 128:                                   # (the stash of K > 128 is not built for shared rows)
                case(f"K{K}/cond16/rows512/inv/n4096", lambda: evaluate(flow(None, segments=K, condition=1, rot="16Trans", **small), 4096, True, 512))
        # feature widths: one pass, K split over wave pairs, K-chunks through the scratch
        for F in (256, 512, 1024, 2048):
            for precision in ("f16x2", "fp32"):
                for n in (4096, (1 << 18) + 4096):
                    case(f"F{F}/{precision}/fwd/n{n}",
                         lambda: evaluate(flow(None, precision, layers=2, condition=1, rot="16UnTrans", feature_dim=F, last_affine=1, first_affine=0), n))
        # FUSED (opt-in): projection inside the stack kernel
        fused_now[0] = 1
        L.rnf_set_fused(1)
        for n in (4096, 1 << 17, 1 << 20):
            case(f"fused/C4/fwd/n{n}", lambda: evaluate(flow("C4"), n))
        case("fused/C4/inv/n4096", lambda: evaluate(flow("C4"), 4096, True))
        case("fused/C2/fwd/n4096", lambda: evaluate(flow("C2"), 4096))
        L.rnf_set_fused(0)
        fused_now[0] = 0

    props = torch.cuda.get_device_properties(0)
    with open(out_path, "w") as fh:
        json.dump(dict(group=group, env=GROUPS[group], cus=props.multi_processor_count, descs=descs, calls=calls, cases=cases), fh)


# ---- trace -> record ------------------------------------------------------------------------------------------------
def read_trace(trace_dir):
    """-> the launches between the (2k)th and (2k+1)th marker, for every k"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"{trace_dir}: expected one kernel trace, found {files}")
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Dispatch_Id"]))
    out, current, markers = [], None, 0
    for r in rows:
        if MARKER in r["Kernel_Name"]:
            markers += 1
            if current is None:
                current = []
            else:
                out.append(current)
                current = None
        elif current is not None:
            wg = int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"])
            grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
            current.append([r["Kernel_Name"], wg, grid, int(r["LDS_Block_Size"])])
    if markers % 2:
        raise SystemExit(f"{files[0]}: odd number of marker launches")
    return out


def record(out_path, commit):
    work = out_path + ".work"
    os.makedirs(work, exist_ok=True)
    merged = dict(commit=commit, cus=None, descs=[], cases=[])
    for group, env in GROUPS.items():
        calls_path, trace_dir = os.path.join(work, f"calls_{group}.json"), os.path.join(work, f"trace_{group}")
        # the profiled program is a fresh child; a failure or a time limit ends the recording (nothing more is started on the GPU)
        subprocess.run(["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "-o", "run", "--", sys.executable,
                        os.path.abspath(__file__), "run", group, calls_path], env=dict(os.environ, **env), check=True,
                       stdout=open(os.path.join(work, f"log_{group}.txt"), "w"), stderr=subprocess.STDOUT)
        part = json.load(open(calls_path))
        launches = read_trace(trace_dir)
        if len(launches) != len(part["calls"]):
            raise SystemExit(f"{group}: {len(part['calls'])} calls but {len(launches)} marked spans in the trace")
        merged["cus"] = part["cus"]
        remap = []
        for table in part["descs"]:
            if table not in merged["descs"]:
                merged["descs"].append(table)
            remap.append(merged["descs"].index(table))
        for c in part["cases"]:
            calls = []
            for i in c["calls"]:
                call = dict(part["calls"][i], launches=launches[i])
                call["desc"] = remap[call["desc"]]
                calls.append(call)
            merged["cases"].append(dict(case=c["case"], env=env, crc=c["crc"], calls=calls))
        print(f"{group}: {len(part['cases'])} cases, {len(launches)} calls", flush=True)
    with open(out_path, "w") as fh:
        fh.write("{\n")
        fh.write(f' "about": "kernel launches of rnf_flow_pass per case (tools/record_flow_plan.py), recorded at commit {commit} on '
                 f'{merged["cus"]} compute units",\n')
        fh.write(f' "commit": {json.dumps(commit)}, "cus": {merged["cus"]},\n')
        fh.write(' "descs": [\n' + ",\n".join("  " + json.dumps(d, separators=(",", ":")) for d in merged["descs"]) + "\n ],\n")
        fh.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in merged["cases"]) + "\n ]\n}\n")


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = 0
    if a["cus"] != b["cus"]:
        print(f"compute units differ: {a['cus']} / {b['cus']}")
        bad += 1
    by_name = {c["case"]: c for c in b["cases"]}
    for ca in a["cases"]:
        cb = by_name.pop(ca["case"], None)
        if cb is None:
            print(f"{ca['case']}: missing in {b_path}")
            bad += 1
            continue
        la, lb = [c["launches"] for c in ca["calls"]], [c["launches"] for c in cb["calls"]]
        if la != lb:
            print(f"{ca['case']}: launches differ\n  {la}\n  {lb}")
            bad += 1
        if ca["crc"] != cb["crc"]:
            print(f"{ca['case']}: output CRCs differ {ca['crc']} / {cb['crc']}")
            bad += 1
    for name in by_name:
        print(f"{name}: missing in {a_path}")
        bad += 1
    print(f"{len(a['cases'])} cases compared, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "run":
        run_group(sys.argv[2], sys.argv[3])
    elif len(sys.argv) >= 3 and sys.argv[1] == "record":
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        record(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else (head or "unknown"))
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
