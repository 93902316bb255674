"""CPU: the struct entry points of the C ABI refuse bad arguments with the texts the parent of the check helpers printed.

tests/golden/abi_refusals_parent.json is tools/record_abi_refusals.py's record of that parent's build: per entry a wrong struct_bytes,
its ranges, its null and alignment refusals, a short and a misaligned workspace, and for the two angle entries the T, K, threshold and
"does not fit; tile" cases.  Every case is refused before any launch (fake pointers, no GPU).  The replay on the current build must
give the same strings, case by case, from the entry and from its *_workspace_bytes."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_abi_refusals", os.path.join(ROOT, "tools", "record_abi_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_refusals_are_the_recorded_ones():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_refusals_parent.json")))["cases"]
    got = _tool().replay()
    assert [(c["entry"], c["case"]) for c in got] == [(c["entry"], c["case"]) for c in want]
    for g, w in zip(got, want):
        assert g == w, (g, w)
    entries = {c["entry"] for c in want}
    assert len(want) >= 200 and {"so3_angle_cdf", "so3_set_angle_cdf", "grid_credible", "fisher_mixture_fit", "flow_pass"} <= entries
    for entry in ("so3_angle_cdf", "so3_set_angle_cdf"):
        said = " ".join(c["error"] for c in want if c["entry"] == entry)
        for word in ("struct_bytes", "G=0", "G=65536", ".T=9", "T=0 requires", "thresholds[2]", "16-byte aligned", "8-byte aligned", "smaller than",
                     "does not fit; tile the " + ("sets" if "set" in entry else "queries")):
            assert word in said, (entry, word)
