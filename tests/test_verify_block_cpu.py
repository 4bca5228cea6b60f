"""The randomized block check's host model (zkgpu_test_verify_rlc_host: the equation of DESIGN.md "Block verification" computed with pairing_host, no device)
on the committed mutation corpora, and the drop-in header zk_block.h."""
import json, os, random
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import verify_mutations as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_block_header_declares_verify_block_only():
    from test_abi_exports import declared_symbols
    import ctypes
    assert declared_symbols("zk_block.h") == ["verifyBlock"]
    assert hasattr(ctypes.CDLL(os.path.join(ROOT, "blockmaze_amd", "libzkgpu.so")), "verifyBlock")

def weights(rng, n): return [rng.randrange(1, 1 << 128) for _ in range(n)]

@pytest.mark.parametrize("name", ["groth16_small", "groth16_step"])
def test_equation_holds_on_valid_records_and_fails_with_any_bad_one(golden_dir, name):
    """three random weight vectors: one equation over the corpus's accepted records holds; adding one rejected record (a verdict 0, or an encoding on which the
    assert-enabled reference aborts) either makes it fail or leaves the left-hand side unchanged — the record did not pass the screen and is not in the equation;
    at least 40 records make it fail"""
    vk = os.path.join(golden_dir, name, "vk.txt"); ni = json.load(open(os.path.join(golden_dir, name, "meta.json")))["n_inputs"]
    cases = [c for c in vm.read_golden(os.path.join(golden_dir, "verify_mutations_%s.txt" % name)) if len(c[2]) == ni]
    good = [c for c in cases if c[3] == 1]; bad = [c for c in cases if c[3] != 1]; assert len(good) >= 20 and len(bad) >= 40
    rng = random.Random(0x5EED + len(name)); failed = 0
    for t in range(3):
        base = rng.sample(good, 12); w = weights(rng, len(base) + 1)
        holds, gt = e.verify_rlc_equation(vk, [c[1] for c in base], [c[2] for c in base], w[:-1]); assert holds
        for c in (bad if t == 0 else rng.sample(bad, 15)):
            h2, gt2 = e.verify_rlc_equation(vk, [x[1] for x in base] + [c[1]], [x[2] for x in base] + [c[2]], w)
            assert not h2 or gt2 == gt, c[0]
            failed += not h2
    assert failed >= 40

def test_weights_matter_for_opposite_shifts(golden_dir):
    """two valid proofs with C1 + D and C2 - D for a random G1 point D: all weights 1 let the shifts cancel and the equation holds; random weights expose them"""
    d = os.path.join(golden_dir, "groth16_small"); vk = os.path.join(d, "vk.txt"); meta = json.load(open(os.path.join(d, "meta.json")))
    cases = [c for c in vm.read_golden(os.path.join(golden_dir, "verify_mutations_groth16_small.txt")) if c[3] == 1 and len(c[2]) == meta["n_inputs"]]
    (_, p1, x1, _), (_, p2, x2, _) = cases[0], cases[-1]
    D = o.g1_op("mul", o.g1_gen(), k=random.Random(7).randrange(1, o.R_MOD))
    def shift(h, P):
        A, B, C = vm.points(vm.coords(h)); return vm.to_hex(vm.from_points(A, B, o.g1_op("add", C, P)))
    recs = [shift(p1, D), shift(p2, vm.g1_neg(D))]; ins = [x1, x2]
    assert not e.verify(vk, recs[0], x1) and not e.verify(vk, recs[1], x2)
    assert e.verify_rlc_equation(vk, recs, ins, [1, 1])[0]
    rng = random.Random(11)
    for _ in range(3): assert not e.verify_rlc_equation(vk, recs, ins, weights(rng, 2))[0]
