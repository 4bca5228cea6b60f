"""Crafted verification keys whose input accumulator acc = IC[0] + sum_j x_j IC[j+1] meets its edge cases, with proofs to decide on them (TEST INFRASTRUCTURE).

Every key has gamma = delta = G2 and IC points that are known multiples s_j G1 (s = 0: the point at infinity), so acc = a G1 with a = s_0 + sum_j x_j s_{j+1} mod r.
The proof (5 G1, 7 G2, 3 G1) satisfies e(A, B) = alpha_g1_beta_g2 e(acc, gamma) e(C, delta) exactly when alpha_g1_beta_g2 = e((32 - a) G1, G2): a key's GT value is
made for a DESIGNED accumulator, and a case is accepted iff the accumulator its inputs give is that one (or its proof compensates in C).  The edge cases:
acc = O (from IC[0] = O, from P + (-P), from a full-width input), doublings (at IC[0] and inside the accumulation), IC points at infinity, zero inputs, and 1, 5 and
16 inputs (16: the most BatchVerifier takes; with 5 and 16 inputs there are more than 64 (input, window) pairs, so the accumulation's quads take two each).
Who decides the right verdict is libsnark (oracle/_ref/ref_harness verifymany; tests/golden/verify_crafted_keys.json holds its answers).

Also the key-file writer the crafted-key tests share, and the random-curve-point batch of the GPU verifier tests."""
import os
from oracle import pyoracle as o

R = o.R_MOD

def g1_bytes(P):
    """compressed key-file encoding (alt_bn128_g1.cpp:404-418 under BINARY_OUTPUT / MONTGOMERY_OUTPUT): '0'|'1' is_zero, 32 bytes of Montgomery X (LE), '0'|'1' lsb of canonical Y"""
    if P is None: return b"1" + bytes(32) + b"1"
    return b"0" + o.to_mont(o.FQ, [P[0]])[0].to_bytes(32, "little") + (b"1" if P[1] & 1 else b"0")
def g2_bytes(Q):
    if Q is None: return b"1" + bytes(64) + b"1"
    (x0, x1), (y0, y1) = Q; m = o.to_mont(o.FQ, [x0, x1]); return b"0" + m[0].to_bytes(32, "little") + m[1].to_bytes(32, "little") + (b"1" if y0 & 1 else b"0")
def write_vk(path, gt12, gamma, delta, ic):
    """r1cs_gg_ppzksnark.tcc:100-108 + accumulation_vector.tcc:63-69"""
    n = len(ic) - 1; b = " ".join(str(c) for c in gt12).encode() + b"\n" + g2_bytes(gamma) + b"\n" + g2_bytes(delta) + b"\n" + g1_bytes(ic[0]) + b"\n"
    b += b"%d\n%d\n" % (n, n) + b"".join(b"%d\n" % i for i in range(n)) + b"%d\n" % n + b"".join(g1_bytes(p) + b"\n" for p in ic[1:]) + b"\n\n"
    open(path, "wb").write(b)
def proof_hex(A, B, C): return o.proof_hex(o.to_arr([A[0], A[1], B[0][0], B[0][1], B[1][0], B[1][1], C[0], C[1]]).reshape(-1))

# ---- the crafted keys --------------------------------------------------------------------------------------------------------------------------------------------
P = 11                                                   # the scalar of "P" in the table of the issue that asked for these cases
AB, C0 = 35, 3                                           # the valid proof (5 G1, 7 G2, 3 G1)

def acc_of(ic, x):
    assert len(x) == len(ic) - 1; return (ic[0] + sum(a * b for a, b in zip(x, ic[1:]))) % R

def _keys():
    """[(label, IC scalars, the accumulator the GT value is made for, [(case label, inputs)])]: every input vector is decided with the valid proof; the helper adds
    the other proofs"""
    g = o.SplitMix64(0xC4AF7ED); rnd = lambda: 1 + g.next() % (R - 1); full = R - 1
    keys = [
        ("ic=[P]", [P], P, [("", [])]),                                                                     # control
        ("ic=[O]", [0], 0, [("", [])]),                                                                     # acc = O: accepted as if e(O, gamma) = 1
        ("ic=[O], gt of the control", [0], P, [("", [])]),                                                  # ... and that value is not any other's
        ("ic=[P,-P]", [P, R - P], 0, [("x=1", [1]), ("x=2", [2])]),                                          # P + (-P) = O; -P
        ("ic=[P,P]", [P, P], 2 * P, [("x=1", [1]), ("x=0", [0])]),                                          # doubling at IC[0]
        ("ic=[P,P], gt of the control", [P, P], P, [("x=1", [1]), ("x=0", [0])]),
        ("ic=[P,O]", [P, 0], P, [("x=12345", [12345]), ("x=0", [0]), ("x=r-1", [full])]),                 # an IC point at infinity: the input does not matter
        ("ic=[P,P], x=r-1", [P, P], 0, [("x=r-1", [full]), ("x=r-2", [R - 2])]),                           # acc = O from a full-width input (every byte non-zero)
        ("ic=[O,P,P]", [0, P, P], 2 * P, [("x=(1,1)", [1, 1]), ("x=(1,2)", [1, 2]), ("x=(2,0)", [2, 0])]),   # a doubling inside the accumulation
        ("ic=[O,P,-P]", [0, P, R - P], 0, [("x=(1,1)", [1, 1]), ("x=(5,5)", [5, 5]), ("x=(1,0)", [1, 0])]),  # acc = O inside the accumulation
        ("ic=[Q,P,256P], doubling of windows", [77, P, 256 * P], 77 + 2 * 256 * P, [("x=(256,1)", [256, 1]), ("x=(1,256)", [1, 256])]),   # window 1 of x_0 meets window 0 of x_1
    ]
    # 5 inputs: random multiples of G1, random full-width inputs, all-zero inputs (acc = IC[0]), an input of r - 1
    ic5 = [rnd() for _ in range(6)]; x5 = [rnd() for _ in range(5)]
    keys.append(("5 inputs", ic5, acc_of(ic5, x5), [("random", x5), ("zeros", [0] * 5), ("x_4 = r-1", x5[:4] + [full])]))
    keys.append(("5 inputs, zero inputs", ic5, ic5[0], [("zeros", [0] * 5), ("random", x5)]))
    # 5 inputs whose accumulator is O with full-width inputs: the last input solves the sum
    ic5o = [rnd() for _ in range(6)]; x5o = [rnd() for _ in range(4)]; x5o.append((-(ic5o[0] + sum(a * b for a, b in zip(x5o, ic5o[1:5]))) * pow(ic5o[5], -1, R)) % R)
    assert acc_of(ic5o, x5o) == 0
    keys.append(("5 inputs, acc = O", ic5o, 0, [("solved", x5o), ("solved, x_0 + 1", [(x5o[0] + 1) % R] + x5o[1:])]))
    # 16 inputs (the maximum): random; acc = O from sixteen full-width inputs; inputs 7 and 8 equal with equal IC points (a doubling deep in the sum); IC points at infinity
    ic16 = [rnd() for _ in range(17)]; x16 = [rnd() for _ in range(16)]
    keys.append(("16 inputs", ic16, acc_of(ic16, x16), [("random", x16), ("all r-1", [full] * 16), ("zeros", [0] * 16)]))
    ic16o = [rnd() for _ in range(17)]; x16o = [rnd() for _ in range(15)]
    x16o.append((-(ic16o[0] + sum(a * b for a, b in zip(x16o, ic16o[1:16]))) * pow(ic16o[16], -1, R)) % R); assert acc_of(ic16o, x16o) == 0
    keys.append(("16 inputs, acc = O", ic16o, 0, [("solved", x16o), ("solved, x_15 - 1", x16o[:15] + [(x16o[15] - 1) % R])]))
    ic16d = [rnd() for _ in range(17)]; ic16d[8] = ic16d[9]; ic16d[3] = 0; ic16d[0] = 0; x16d = [rnd() for _ in range(16)]; x16d[8] = x16d[7]
    keys.append(("16 inputs, equal terms, IC at infinity", ic16d, acc_of(ic16d, x16d), [("x_7 = x_8", x16d), ("x_7 = x_8, x_2 changed", x16d[:2] + [rnd()] + x16d[3:]), ("x_7 = x_8 = 1, rest 0", [0] * 7 + [1, 1] + [0] * 7)]))
    return keys

def cases():
    """[(key label, IC scalars, designed accumulator, [(case label, proof hex, inputs)])]: per key, for every input vector, the valid proof, the same with A and B
    re-balanced, a proof with a wrong C, and (for keys with inputs) a proof whose C compensates input 0 + 1 under that input; plus a valid proof under input 0 + 1"""
    G1, G2 = o.g1_gen(), o.g2_gen(); m1 = lambda k: o.g1_op("mul", G1, k=k % R); m2 = lambda k: o.g2_op("mul", G2, k=k % R); out = []
    valid, rebal, wrong_c = proof_hex(m1(5), m2(7), m1(C0)), proof_hex(m1(7), m2(5), m1(C0)), proof_hex(m1(5), m2(7), m1(C0 + 1))
    for label, ic, design, xs in _keys():
        assert (AB - C0 - design) % R, label                                   # (the GT value is never the identity: e(O, .) has no encoding here)
        cs = []
        for xl, x in xs:
            t = (" " + xl) if xl else ""
            cs += [("valid" + t, valid, x), ("re-balanced" + t, rebal, x), ("wrong C" + t, wrong_c, x)]
        cc = (C0 + design - acc_of(ic, xs[0][1])) % R                               # a C that makes up for an accumulator other than the designed one
        if cc not in (0, C0): cs.append(("C compensating the accumulator", proof_hex(m1(5), m2(7), m1(cc)), xs[0][1]))
        if len(ic) > 1:
            x = list(xs[0][1]); bad = [(x[0] + 1) % R] + x[1:]; shift = ic[1]          # input 0 + 1 moves acc by IC[1]
            cs.append(("valid, input 0 + 1", valid, bad))
            if (C0 - shift) % R: cs.append(("C compensating input 0 + 1", proof_hex(m1(5), m2(7), m1(C0 - shift)), bad))
        out.append((label, ic, design, cs))
    return out

def gt_for(design):
    """alpha_g1_beta_g2 under which the valid proof is accepted iff acc = design G1"""
    return o.pairing(o.g1_op("mul", o.g1_gen(), k=(AB - C0 - design) % R), o.g2_gen())

def write_keys(directory):
    """writes one vk file per crafted key -> [(vk path, key label, [(case label, proof hex, inputs)])]"""
    G1, G2 = o.g1_gen(), o.g2_gen(); out = []
    for i, (label, ic, design, cs) in enumerate(cases()):
        path = os.path.join(str(directory), "crafted_vk_%02d.txt" % i)
        write_vk(path, gt_for(design), G2, G2, [o.g1_op("mul", G1, k=s) if s else None for s in ic]); out.append((path, label, cs))
    return out

def labelled(keys):
    """[(key label + ' / ' + case label, vk path, proof hex, inputs)] in a fixed order"""
    return [(label + " / " + cl, path, h, x) for path, label, cs in keys for cl, h, x in cs]

# ---- random curve points -----------------------------------------------------------------------------------------------------------------------------------------
def random_curve_batch(good, inputs, seed=2903):
    """what a prover never produces: 120 "proofs" made of random multiples of the generators (on the curve, so that the whole pairing runs on arbitrary field values)
    under random or genuine public inputs, and 40 valid proofs under random public inputs, shuffled among the valid proofs `good` (24) -> (proofs, inputs)"""
    g = o.SplitMix64(seed); G1, G2 = o.g1_gen(), o.g2_gen(); rnd = lambda: 1 + g.next() % (o.R_MOD - 1)
    cs = [(pr, inputs) for pr in good]
    for _ in range(120): cs.append((proof_hex(o.g1_op("mul", G1, k=rnd()), o.g2_op("mul", G2, k=rnd()), o.g1_op("mul", G1, k=rnd())), [rnd() for _ in inputs] if g.next() & 1 else inputs))
    for _ in range(40): cs.append((good[g.next() % len(good)], [rnd() for _ in inputs]))            # a valid proof under random inputs
    order = list(range(len(cs)))
    for i in range(len(order) - 1, 0, -1): j = g.next() % (i + 1); order[i], order[j] = order[j], order[i]
    cs = [cs[i] for i in order]; return [c[0] for c in cs], [c[1] for c in cs]

# ---- a mixed batch ---------------------------------------------------------------------------------------------------------------------------------------------------
def mixed_batch(good, inputs):
    """the valid proofs `good`, then tampered proofs (one flipped hex digit in each of the 8 coordinates), wrong public inputs, all-zero inputs, the all-zero record,
    a record that is not hex and a proof spliced from two valid ones -> (proofs, inputs); only the first len(good) are valid"""
    proofs, ins = [], []
    for g in good: proofs.append(g); ins.append(inputs)
    for k in range(8):                                                                   # one flipped hex digit in each of the 8 coordinates
        g = good[k % len(good)]; pos = 64 * k + 37; proofs.append(g[:pos] + ("0" if g[pos] != "0" else "1") + g[pos + 1:]); ins.append(inputs)
    for j in range(len(inputs)): bad = list(inputs); bad[j] = (bad[j] + 1) % o.R_MOD; proofs.append(good[0]); ins.append(bad)
    proofs.append(good[1]); ins.append([0] * len(inputs))
    proofs.append("0" * 512); ins.append(inputs)                                          # all-zero record: (0,0) is off-curve
    proofs.append("zz" + good[0][2:]); ins.append(inputs)                                 # not hex
    proofs.append(good[2][:128] + good[3][128:]); ins.append(inputs)                      # A of one valid proof with B, C of another
    return proofs, ins

def reference_answers(harness, directory):
    """{case label: libsnark's verdict} (ref_harness verifymany, one call per key): what tests/golden/verify_crafted_keys.json stores"""
    import verify_mutations as vm
    keys = write_keys(directory); out = {}
    for path, label, cs in keys:
        for (cl, _, _), v in zip(cs, vm.reference_verdicts(harness, path, cs, directory)): out[label + " / " + cl] = v
    return keys, out

def cases_sha256(keys):
    import hashlib; return hashlib.sha256(repr([(label, h, x) for label, _, h, x in labelled(keys)]).encode()).hexdigest()

if __name__ == "__main__":           # python tests/verify_crafted.py <ref_harness> <output json>: the fixture, from the reference binary
    import json, sys, tempfile
    with tempfile.TemporaryDirectory() as d:
        keys, v = reference_answers(sys.argv[1], d)
        json.dump({"cases_sha256": cases_sha256(keys), "verdicts": v}, open(sys.argv[2], "w"), indent=0, sort_keys=True)
