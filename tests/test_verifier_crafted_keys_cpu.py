"""Crafted verification keys whose input accumulator reaches its edge cases (tests/verify_crafted.py: acc at infinity from IC[0], from P + (-P) and from full-width
inputs; doublings at IC[0] and inside the sum; IC points at infinity; zero inputs; 1, 5 and 16 inputs): the host verifier (what verify*proof falls back to, and what
decides a record the GPU hands back) and the oracle give libsnark's verdict on every case.  libsnark is asked on the spot where oracle/_ref/ref_harness exists; its
stored answers (tests/golden/verify_crafted_keys.json) are used, and checked against it, everywhere."""
import json, os
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import verify_crafted as vc
import verify_mutations as vm

HARNESS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "ref_harness")

def test_crafted_keys_are_decided_like_libsnark(golden_dir, tmp_path):
    stored = json.load(open(os.path.join(golden_dir, "verify_crafted_keys.json"))); want = stored["verdicts"]
    keys = vc.write_keys(tmp_path); cases = vc.labelled(keys)
    assert vc.cases_sha256(keys) == stored["cases_sha256"] and sorted(want) == sorted(c[0] for c in cases) and len(cases) == len(want)
    if os.path.exists(HARNESS):
        for path, label, cs in keys: assert vm.reference_verdicts(HARNESS, path, cs, tmp_path) == [want[label + " / " + cl] for cl, _, _ in cs], label
    for label, path, h, x in cases:
        assert int(e.verify(path, h, x)) == want[label], ("host", label)
        assert int(o.verify(o.parse_vk(path), x, o.proof_words_from_hex(h))) == want[label], ("oracle", label)
    # what the set covers: every key accepts one case and rejects another; a valid proof under a wrong input is rejected; the edges of the issue's table
    for path, label, cs in keys:
        v = [want[label + " / " + cl] for cl, _, _ in cs]; assert 1 in v and 0 in v, label
    assert sum(1 for c in cases if "valid, input 0 + 1" in c[0] and want[c[0]] == 0) >= 10
    assert {len(x) for _, _, _, x in cases} >= {0, 1, 2, 5, 16}
    for key, verdict in (("ic=[P] / valid", 1), ("ic=[O] / valid", 1), ("ic=[O], gt of the control / valid", 0), ("ic=[P,-P] / valid x=1", 1), ("ic=[P,-P] / valid x=2", 0),
                         ("ic=[P,P] / valid x=1", 1), ("ic=[P,P], gt of the control / valid x=1", 0), ("ic=[P,O] / valid x=12345", 1), ("ic=[P,P], x=r-1 / valid x=r-1", 1)):
        assert want[key] == verdict, key
