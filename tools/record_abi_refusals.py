#!/usr/bin/env python3
"""Record what the struct entry points of the C ABI say when they refuse their arguments (tests/golden/abi_refusals_parent.json;
tests/test_abi_refusals.py replays the list on the current build and compares the strings).

    python tools/record_abi_refusals.py record OUT.json [COMMIT]    every case below on the built library -> OUT.json
    python tools/record_abi_refusals.py compare A.json B.json       two records case by case; exit 1 on a difference

Every case is refused before any launch, so no GPU is needed and no pointer is dereferenced: device pointers are fake non-null
addresses, only the arrays the library reads on the host (thresholds, kappas, levels) are real.  Per entry: a wrong struct_bytes, the
ranges of its counts (g / G of 0 and 65536 among them), its null and alignment refusals, a workspace one byte short and a misaligned
one.  A case that is not refused ends the recording: its launch would follow."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAKE = 1 << 20                                       # a 16-byte aligned address that is never read
_TH = (C.c_double * 8)(*[math.radians(d) for d in (5.0, 10.0, 15.0, 30.0, 45.0, 60.0, 90.0, 180.0)])
_KAPPAS = (C.c_double * 2)(1.0, 200.0)
_LEVELS = (C.c_double * 2)(0.5, 0.9)
_HOST = []                                           # host arrays of the cases, kept alive
# rnf_flow_pass_workspace_bytes reads the descriptor table once struct_bytes is right: only that case asks it.  Three entries do not
# check the alignment of their workspace: with a misaligned one they would launch.
READS_ITS_ARGUMENTS = ("flow_pass",)
ANY_ALIGNMENT = ("flow_pass", "grid_beam_select", "grid_modes")


def host(*values):
    a = (C.c_double * len(values))(*values)
    _HOST.append(a)
    return C.addressof(a)


def _angle(extra):
    walk = [("G=0", dict(G=0)), ("G=65536", dict(G=65536)), ("n=0", dict(n=0)), ("n=2^24+1", dict(n=(1 << 24) + 1)), ("m=-1", dict(m=-1)),
            ("m=2^31", dict(m=1 << 31)), ("T=-1", dict(T=-1)), ("T=9", dict(T=9)),
            ("T=0 without moments", dict(T=0, thresholds=None, mean_angle=None, mean_sq_angle=None)), ("T=0 with thresholds", dict(T=0)),
            ("thresholds and query_tau", dict(query_tau=FAKE)), ("neither thresholds nor query_tau", dict(thresholds=None)),
            ("thresholds[0]<0", dict(thresholds=host(-1e-9, *_TH[1:]))),
            ("thresholds[1]>pi", dict(thresholds=host(_TH[0], math.pi * (1 + 1e-15), *_TH[2:]))),
            ("thresholds[2] NaN", dict(thresholds=host(_TH[0], _TH[1], float("nan"), *_TH[3:]))),
            ("thresholds[3] inf", dict(thresholds=host(_TH[0], _TH[1], _TH[2], float("inf"), *_TH[4:]))),
            ("centres misaligned", dict(centres=FAKE + 4)), ("queries misaligned", dict(queries=2 * FAKE + 8)), ("null centres", dict(centres=None)),
            ("null queries", dict(queries=None)), ("does not fit", dict(G=65535, n=1 << 24, m=(1 << 31) - 1))]
    return walk + extra


def entries():
    """-> [(entry, struct class, arguments that pass every check, [(case, changed arguments)])]"""
    from rotationnormflow_amd import _lib as B
    g_range = [("g=0", dict(g=0)), ("g=65536", dict(g=65536))]
    G_range = [("G=0", dict(G=0)), ("G=65536", dict(G=65536))]
    pair = dict(centres=FAKE, queries=2 * FAKE, n=4608, m=1000, G=3)
    angle = dict(pair, log_weights=FAKE, T=8, thresholds=C.addressof(_TH), mass=FAKE, mean_angle=FAKE, mean_sq_angle=FAKE)
    return [
        ("flow_pass", B.FlowPass, dict(rotation=FAKE, n=16, blob=FAKE, segments=8, rotation_out=FAKE, ldj_out=FAKE),
         [("dir=2", dict(dir=2)), ("fisher_A without fisher_c", dict(fisher_A=FAKE)), ("feature_div=-1", dict(feature_div=-1))]),
        ("flow_backward_pass", B.FlowBackward, dict(states=FAKE, n=16), []),
        ("so3_grid_children", B.GridChildren, dict(level=1, parents=FAKE, n=10, rows_out=FAKE),
         [("level=-1", dict(level=-1)), ("level=99", dict(level=99)), ("n=-1", dict(n=-1)), ("null parents", dict(parents=None))]),
        ("grid_beam_select", B.GridBeamSelect, dict(logp=FAKE, M=100000, g=3, beam=8, rows_out=FAKE, logp_out=FAKE),
         g_range + [("M=0", dict(M=0)), ("beam=0", dict(beam=0)), ("beam=2^20", dict(beam=1 << 20)), ("null logp", dict(logp=None))]),
        ("grid_modes", B.GridModes,
         dict(logp=FAKE, grid=FAKE, Q=4608, g=3, top_k=2, separation_rad=0.5, index_out=FAKE, logp_out=FAKE, mass_out=FAKE, log_norm_out=FAKE),
         g_range + [("Q=0", dict(Q=0)), ("top_k=0", dict(top_k=0)), ("top_k=2^20", dict(top_k=1 << 20)),
                    ("separation_rad=0", dict(separation_rad=0.0)), ("separation_rad=4", dict(separation_rad=4.0)), ("null logp", dict(logp=None)), ("grid misaligned", dict(grid=FAKE + 4)),
                    ("n_gt=0", dict(gt=FAKE, n_gt=0)), ("gt without spread_out", dict(gt=FAKE, n_gt=1))]),
        ("grid_credible", B.GridCredible,
         dict(logp=FAKE, Q=4608, g=3, levels=C.addressof(_LEVELS), n_levels=2, threshold_out=FAKE, count_out=FAKE, mass_out=FAKE, log_norm_out=FAKE),
         g_range + [("Q=0", dict(Q=0)), ("Q=2^26+1", dict(Q=(1 << 26) + 1)), ("n_levels=0", dict(n_levels=0)), ("n_levels=1000", dict(n_levels=1000)),
                    ("n_queries=-1", dict(n_queries=-1)), ("n_queries=1000", dict(n_queries=1000)), ("null levels", dict(levels=None)),
                    ("levels[1]=1", dict(levels=host(0.5, 1.0))), ("null logp", dict(logp=None)), ("n_queries without queries", dict(n_queries=1))]),
        ("so3_grid_locate", B.GridLocate, dict(level=1, rotations=FAKE, n=10, g=1, rows_out=FAKE),
         g_range + [("level=-1", dict(level=-1)), ("level=99", dict(level=99)), ("n=-1", dict(n=-1)), ("no output", dict(rows_out=None)),
                    ("counts at level 7", dict(level=7, counts=FAKE)), ("null rotations", dict(rotations=None))]),
        ("grid_fit", B.GridFit, dict(logp=FAKE, counts=FAKE, Q=4608, g=3, stats_out=FAKE),
         g_range + [("Q=0", dict(Q=0)), ("Q=2^26+1", dict(Q=(1 << 26) + 1)), ("null logp", dict(logp=None))]),
        ("so3_grid_cell_points", B.GridCellPoints, dict(level=1, rows=FAKE, u=FAKE, n=10, rot_out=FAKE),
         [("level=-1", dict(level=-1)), ("level=99", dict(level=99)), ("n=-1", dict(n=-1)), ("null rows", dict(rows=None))]),
        ("grid_sample", B.GridSample, dict(logp=FAKE, Q=4608, g=3, level=2, draws=10, draws_total=10, index_out=FAKE),
         g_range + [("Q=0", dict(Q=0)), ("Q=2^26+1", dict(Q=(1 << 26) + 1)), ("level=-2", dict(level=-2)), ("level=99", dict(level=99)),
                    ("Q of another level", dict(level=1)), ("rot_out without a level", dict(level=-1, rot_out=FAKE)), ("method=7", dict(method=7)),
                    ("draws_total=0", dict(draws_total=0)), ("draws beyond the total", dict(draws=11)), ("image_base=-1", dict(image_base=-1)),
                    ("null logp", dict(logp=None)), ("null index_out", dict(index_out=None))]),
        ("so3_kernel_sum", B.So3KernelSum, dict(pair, kappas=C.addressof(_KAPPAS), J=2, out=FAKE),
         G_range + [("J=0", dict(J=0)), ("J=99", dict(J=99)), ("n=0", dict(n=0)), ("n=2^24+1", dict(n=(1 << 24) + 1)), ("m=-1", dict(m=-1)),
                    ("m=2^31", dict(m=1 << 31)), ("does not fit", dict(G=65535, n=1 << 24, m=(1 << 31) - 1)), ("null kappas", dict(kappas=None)),
                    ("kappas[1]<0", dict(kappas=host(1.0, -1.0))), ("centres misaligned", dict(centres=FAKE + 4)),
                    ("queries misaligned", dict(queries=2 * FAKE + 8)), ("leave_one_out with m != n", dict(leave_one_out=1)),
                    ("null queries with m != n", dict(queries=None)), ("null centres", dict(centres=None))]),
        ("so3_kernel_moments", B.So3KernelMoments, dict(pair, kappa=2.0, log_density=FAKE),
         G_range + [("n=0", dict(n=0)), ("n=2^24+1", dict(n=(1 << 24) + 1)), ("m=-1", dict(m=-1)), ("m=2^31", dict(m=1 << 31)),
                    ("does not fit", dict(G=65535, n=1 << 24, m=(1 << 31) - 1)), ("kappa=-1", dict(kappa=-1.0)),
                    ("centres misaligned", dict(centres=FAKE + 4)), ("queries misaligned", dict(queries=2 * FAKE + 8)),
                    ("step without rotation", dict(step=FAKE)), ("null centres", dict(centres=None))]),
        ("so3_angle_cdf", B.So3AngleCdf, angle, _angle([])),
        ("so3_set_angle_cdf", B.So3SetAngleCdf, dict(angle, K=60), _angle([("K=0", dict(K=0)), ("K=4097", dict(K=4097)), ("K=-3", dict(K=-3))])),
        ("so3_grid_local_sum", B.So3GridLocalSum, dict(level=2, grid=FAKE, queries=2 * FAKE, m=100, G=1, kappa=1.0, d2_cut=1.0, out=FAKE),
         G_range + [("level=-1", dict(level=-1)), ("level=99", dict(level=99)), ("m=-1", dict(m=-1)), ("kappa=-1", dict(kappa=-1.0)),
                    ("d2_cut=9", dict(d2_cut=9.0)), ("grid misaligned", dict(grid=FAKE + 4)), ("queries misaligned", dict(queries=2 * FAKE + 8)),
                    ("offset misaligned", dict(offset=FAKE + 2)), ("null queries with m != Q", dict(queries=None)), ("null grid", dict(grid=None))]),
        ("so3_wigner", B.So3Wigner, dict(rotations=FAKE, n=10, lmax=2, out=FAKE),
         [("lmax=-1", dict(lmax=-1)), ("lmax=17", dict(lmax=17)), ("n=-1", dict(n=-1)), ("n=2^24+1", dict(n=(1 << 24) + 1)),
          ("null rotations", dict(rotations=None))]),
        ("so3_fourier", B.So3Fourier, dict(centres=FAKE, n=4608, G=3, lmax=2, out=FAKE),
         G_range + [("lmax=-1", dict(lmax=-1)), ("lmax=17", dict(lmax=17)), ("n=0", dict(n=0)), ("n=2^24+1", dict(n=(1 << 24) + 1)),
                    ("null centres", dict(centres=None))]),
        ("so3_fourier_eval", B.So3FourierEval, dict(coeffs=FAKE, queries=FAKE, m=10, G=1, lmax=2, out=FAKE),
         G_range + [("lmax=-1", dict(lmax=-1)), ("lmax=17", dict(lmax=17)), ("m=-1", dict(m=-1)), ("null coeffs", dict(coeffs=None))]),
        ("rotation_moments", B.RotationMoments, dict(rotations=FAKE, n=10000, G=3, moments_out=FAKE),
         [("G=0", dict(G=0)), ("n=0", dict(n=0)), ("n=2^40+1", dict(n=(1 << 40) + 1)), ("more than one launch", dict(G=1 << 31, n=1 << 20)),
          ("null rotations", dict(rotations=None)), ("shared_rotations without log_weights", dict(shared_rotations=1))]),
        ("fisher_fit", B.FisherFit, dict(moments=FAKE, B=10, max_concentration=100.0, A_out=FAKE),
         [("B=-1", dict(B=-1)), ("max_concentration=0", dict(max_concentration=0.0)), ("max_iterations=-1", dict(max_iterations=-1)),
          ("null moments", dict(moments=None)), ("more than one launch", dict(B=1 << 34))]),
        ("fisher_mixture_fit", B.FisherMixtureFit,
         dict(rotations=FAKE, n=10000, G=3, K=2, A_init=FAKE, iterations=5, tol=1e-6, max_concentration=100.0, A_out=FAKE, log_pi_out=FAKE,
              loglik_out=FAKE, status_out=FAKE, iterations_out=FAKE),
         [("G=0", dict(G=0)), ("G=2^31", dict(G=1 << 31)), ("n=0", dict(n=0)), ("K=0", dict(K=0)), ("K=99", dict(K=99)),
          ("iterations=0", dict(iterations=0)),
          ("null rotations", dict(rotations=None)), ("shared_rotations without log_weights", dict(shared_rotations=1)), ("tol=-1", dict(tol=-1.0)),
          ("max_concentration=0", dict(max_concentration=0.0))]),
    ]


def replay(L=None):
    """Every case on the library ``L`` (default: the built one) -> [dict(entry, case, error, workspace_error)]: the message of the
    refusal, and that of ``rnf_<entry>_workspace_bytes`` where the entry has one and it refuses too (else None)"""
    from rotationnormflow_amd import _lib as B
    L = L or B.lib()
    out = []
    for entry, struct, good, bad in entries():
        sizer = getattr(L, f"rnf_{entry}_workspace_bytes", None) if f"rnf_{entry}_workspace_bytes" in B.EXPORTS else None

        def build(changed):
            a = struct(**dict(good, **changed))
            if sizer is not None and entry not in READS_ITS_ARGUMENTS:
                a.workspace, a.workspace_bytes = FAKE, sizer(C.byref(a))
            return a

        cases = [("struct_bytes", lambda: build({}), lambda a: setattr(a, "struct_bytes", a.struct_bytes + 8))]
        cases += [(name, lambda changed=changed: build(changed), None) for name, changed in bad]
        if sizer is not None and entry not in READS_ITS_ARGUMENTS:
            cases.append(("workspace one byte short", lambda: build({}), lambda a: setattr(a, "workspace_bytes", a.workspace_bytes - 1)))
        if sizer is not None and entry not in ANY_ALIGNMENT:
            cases.append(("workspace misaligned", lambda: build({}), lambda a: setattr(a, "workspace", a.workspace + 4)))
        for name, make, change in cases:
            a = make()
            if change:
                change(a)
            ws_error = None
            if sizer is not None and (entry not in READS_ITS_ARGUMENTS or name == "struct_bytes") and sizer(C.byref(a)) == 0:
                ws_error = L.rnf_last_error().decode()
            rc = getattr(L, "rnf_" + entry)(C.byref(a))
            error = L.rnf_last_error().decode()
            if rc == 0 or "failed:" in error:
                raise SystemExit(f"rnf_{entry}, case {name!r}: not refused before the launch (rc={rc}, {error!r})")
            out.append(dict(entry=entry, case=name, error=error, workspace_error=ws_error))
    return out


def record(out_path, commit):
    cases = replay()
    with open(out_path, "w") as fh:
        fh.write("{\n")
        fh.write(f' "about": "what the struct entry points answer to arguments they refuse before any launch (tools/record_abi_refusals.py), '
                 f'recorded at commit {commit}",\n')
        fh.write(f' "commit": {json.dumps(commit)},\n')
        fh.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c) for c in cases) + "\n ]\n}\n")
    print(f"{len(cases)} refusals of {len({c['entry'] for c in cases})} entry points -> {out_path}")


def compare(a_path, b_path):
    a, b = json.load(open(a_path))["cases"], json.load(open(b_path))["cases"]
    bad = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    for x, y in zip(a, b):
        if x != y:
            print(f"{x}\n{y}\n")
    print(f"{len(a)} / {len(b)} cases, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "record":
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        record(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else (head or "unknown"))
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
