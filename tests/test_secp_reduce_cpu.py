"""The paths of reduce512 (csrc/secp256k1.cuh) on Python integers, no GPU: secp_model.fold_trace restates the three folds and says which carries a product takes; the
constructors beside it deliver operands for every path that can be taken, and the paths that cannot are shown empty.  Mutants of the restatement, which live only
in this file, show that the constructed operands catch a dropped carry where the operand set of tests/test_gpu_senders.py cannot.  The same operands go to the
device in tests/test_gpu_senders.py."""
import random
import pytest
import secp_model as m

P, N = m.P, m.N
W = 1 << 256

def edge_operands():
    """operands() of tests/test_gpu_senders.py, restated: that module is marked gpu as a whole"""
    rng = random.Random(11)
    edge = [0, 1, 2, P - 1, P - 2, N - 1, N, 2**256 - 1, P, P + 1, N + 1, 2**255] + [0xFFFFFFFF << (32 * k) for k in range(8)] + [1 << (32 * k) for k in range(1, 8)]
    return edge + [rng.getrandbits(256) for _ in range(64)]
EDGE_PAIRS = [(a, b) for a in edge_operands() for b in edge_operands()]

@pytest.mark.parametrize("modulus", [N, P], ids=["N", "p"])
def test_fold_trace_agrees_with_the_remainder(modulus):
    """(fold_trace asserts its residue against % itself; here it is compared once more from outside) on the 8,281 edge pairs and 20,000 random pairs"""
    assert len(EDGE_PAIRS) == 8281; rng = random.Random(modulus); seen = {}
    for a, b in EDGE_PAIRS + [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(20000)]:
        r, rec = m.fold_trace(a, b, modulus); assert r == a * b % modulus; seen[rec[:2]] = seen.get(rec[:2], 0) + 1
    print("mod %s: records (fold-2 carry, fold-3 carry) on the edge and random pairs: %s" % ("N" if modulus == N else "p", sorted(seen.items())))
    assert all(rec[1] == 0 for rec in seen)                                                          # what the old operands never reach

@pytest.mark.parametrize("name", list(m.REDUCE_CLASSES))
def test_constructors_deliver_every_class_and_the_unreachable_ones_stay_empty(name):
    """At least 64 cases a class, each with the wanted record by the model alone, canonical operands except where the class says a = 2^256 - 1.  Every constructor
    looks at 20,000 candidates, and none of them, whatever its recipe, leaves the bounds: C^2 < 1.62 x 2^256 for N (C < 2^128.35), and what fold 1 hands on is at most
    C (lo + hi C < 2^256 (1 + C)), so fold 2's sum is below 2^256 + C^2 < 2.62 x 2^256: its carry is at most 2.  Where it is 2 the low words are below 0.62 x 2^256
    and adding 2 C cannot carry: no (2, 1).  For p, C^2 < 2^67 and fold 2's sum is below 2^256 + 2^67: a carry of at most 1, and then low words below 2^67, to
    which fold 3 adds C < 2^34: no fold-3 carry."""
    modulus, recipe, want = m.REDUCE_CLASSES[name]; C = W - modulus; cases, seen = m.reduce_cases(name, tries=20000)
    print("%s: %d cases kept, records over 20,000 candidates: %s" % (name, len(cases), sorted(seen.items())))
    assert len(cases) >= 64 and sum(seen.values()) == 20000
    for a, b in cases:
        assert m.record_wanted(m.fold_trace(a, b, modulus)[1], want) and b < modulus and (a < modulus or (recipe == "fold3 max" and a == W - 1))
    if modulus == N: assert C * C * 100 < 162 * W and all(c2 <= 2 and (c2, c3) != (2, 1) and (c3 == 0 or c2 == 1) for c2, c3 in seen)
    else: assert C * C < 1 << 67 and all(c2 <= 1 and c3 == 0 for c2, c3 in seen)

# ---- mutants: wrong restatements of reduce512, here only ----------------------------------------------------------------------------------------------------------
def mutant_reduce(a, b, modulus, mutant):
    """fold_trace's arithmetic with one step broken: "no +C" drops the + C after a fold-3 carry, "no over2" ignores what fold 2 hands on above its low eight words,
    "no sub" skips the final subtraction.  (Read by the letter, "the second word fold 2 hands on" would be the second 32-bit word of that carry; the carry is at
    most 2, so that word is always zero and a mutant that drops it is no mutant.  The one here drops the words fold 2 hands on beside its low eight.)"""
    C = W - modulus; t = a * b; s1 = t % W + t // W * C; s2 = s1 % W + s1 // W * C
    over2 = 0 if mutant == "no over2" else s2 // W
    s3 = s2 % W + over2 * C; r = s3 % W + (C if s3 // W and mutant != "no +C" else 0)
    return r - modulus if r >= modulus and mutant != "no sub" else r

AIMED = {"no +C": ["N (1,1)", "N (1,1) a = 2^256 - 1"], "no over2": ["N (1,0)", "N (2,0)", "N (1,1)", "N sub, fold-2 carry 1", "p (1,0)", "p sqr (1,0)"],
         "no sub": ["N sub", "N sub, fold-2 carry 1", "p sub", "p sqr sub"]}

@pytest.mark.parametrize("mutant", list(AIMED))
def test_each_mutant_is_wrong_on_its_whole_class_and_right_on_the_old_operands(mutant):
    for modulus in (N, P):                                                                            # the unbroken restatement first: it is fold_trace
        assert all(mutant_reduce(a, b, modulus, None) == a * b % modulus for a, b in EDGE_PAIRS[::7])
    for name in AIMED[mutant]:
        modulus = m.REDUCE_CLASSES[name][0]; cases = m.reduce_cases(name, tries=20000)[0]; wrong = sum(mutant_reduce(a, b, modulus, mutant) != a * b % modulus for a, b in cases)
        print("mutant %r on class %s: wrong on %d of %d" % (mutant, name, wrong, len(cases))); assert wrong == len(cases) >= 64
    for modulus in (N, P):
        bad = [(a, b) for a, b in EDGE_PAIRS if mutant_reduce(a, b, modulus, mutant) != a * b % modulus]
        print("mutant %r mod %s on the 8,281 edge pairs: wrong on %d" % (mutant, "N" if modulus == N else "p", len(bad)))
        if mutant == "no +C": assert not bad                                                          # the old operands cannot see this one at all
        if mutant == "no over2" and modulus == P: assert len(bad) <= 3                                # fold 2 carries for 3 of the edge pairs
        assert len(bad) < len(EDGE_PAIRS)

# ---- the crafted signatures ---------------------------------------------------------------------------------------------------------------------------------------
def test_crafted_signatures_take_their_paths_and_the_model_accepts_them():
    """64 lines of each kind; the products of the recovery, s / r and m / r, take the path the kind names; the model's verdict is ok on at least 9 of 10, so that the
    device test cannot pass by refusing them"""
    lines = m.crafted_signatures(); want = m.crafted_expected(); by_kind = {}
    for (kind, hs, h, sig), exp in zip(lines, want):
        r = int.from_bytes(sig[:32], "big"); s = int.from_bytes(sig[32:64], "big"); mm = int.from_bytes(h, "big"); rinv = pow(r, -1, N); by_kind.setdefault(kind, []).append(exp[0])
        assert hs == m.CRAFTED_KINDS[kind] and 1 <= s <= (N // 2 if hs else N - 1) and sig[64] in (0, 1)
        cls = m.REDUCE_CLASSES["N (1,1)" if kind.startswith("fold3") else "N sub"][2]
        if kind.endswith(("u2", "both")): assert m.record_wanted(m.fold_trace(s, rinv, N)[1], cls)
        if kind.endswith(("u1", "both")): assert mm < N and m.record_wanted(m.fold_trace(mm, rinv, N)[1], cls)
    for kind, oks in by_kind.items(): print("crafted %s: %d lines, the model accepts %d" % (kind, len(oks), sum(oks))); assert len(oks) == 64 and 10 * sum(oks) >= 9 * len(oks)
    assert set(by_kind) == set(m.CRAFTED_KINDS)

def test_a_low_s_cannot_reach_the_fold_3_carry():
    """Why "fold3 u2" and "fold3 both" carry a high s.  The fold-3 carry needs fold 2 to carry with its low words within C of 2^256: over1 C > 2^256 - C, over1 being
    what fold 1 hands on, at most hi C / 2^256 + 1.  So hi > 2^512 / C^2 - 2 x 2^256 / C > 0.61 x 2^256 - 2^129, and with s <= N / 2 the product's high half stays
    below 2^255.  The bound in integers, then 20,000 low s by the recipe."""
    C = W - N; assert W * W // (C * C) - 2 * (W // C) - 2 > W // 2
    rng = random.Random(3)
    for _ in range(20000):
        r = rng.randrange(1, N); s = (2 * C - rng.randrange(1, C + 1)) * r % N
        if s <= N // 2: assert m.fold_trace(s, pow(r, -1, N), N)[1][1] == 0
