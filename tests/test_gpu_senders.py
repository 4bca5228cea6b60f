"""Senders from signatures on the device (include/zk_senders.h; DESIGN.md "Senders from signatures"): the raw field and scalar operations of csrc/secp256k1.cuh at
the edges of their contract, the resident table of G, the walk u1 G + u2 P with every exceptional branch of its point addition taken, and zkRecoverSenders against
every line of tests/golden/ecrecover_cases.txt — verdicts and keys from the reference's own libsecp256k1 (tools/make_senders_golden.py).  Python integers
(tests/secp_model.py) are the reference of everything else.  Every test here fails on a library without the feature: the entries do not exist."""
import os, random, subprocess, sys, threading
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import secp_model as m

pytestmark = pytest.mark.gpu
P, N = m.P, m.N
ARG, NO_DEVICE = -2, -1

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    engine.init(); return engine

def fixture_lines():
    out = []
    for l in open(os.path.join(ROOT, "tests", "golden", "ecrecover_cases.txt")):
        f = l.split(); out.append((bytes.fromhex(f[0]), bytes.fromhex(f[1]), int(f[2]), f[3] == "1", bytes.fromhex(f[4]) if f[3] == "1" else bytes(64), bytes.fromhex(f[5]) if f[3] == "1" else bytes(20)))
    return out
LINES = fixture_lines()

# ---- raw operations -------------------------------------------------------------------------------------------------------------------------------------------------
def operands():
    rng = random.Random(11)
    edge = [0, 1, 2, P - 1, P - 2, N - 1, N, 2**256 - 1, P, P + 1, N + 1, 2**255] + [0xFFFFFFFF << (32 * k) for k in range(8)] + [1 << (32 * k) for k in range(1, 8)]
    return edge + [rng.getrandbits(256) for _ in range(64)]

def test_raw_field_and_scalar_operations_at_the_contract_edges(e):
    """secp256k1.cuh's contract, line by line.  mul, sqr and reduce take ANY 256-bit value (2^256 - 1, every limb 0xFFFFFFFF, is among the operands) and return the
    canonical result; add, sub, neg, inv and sqrt take canonical values.  There is no lazy bound to probe: every routine returns a value below its modulus, which is
    what each comparison with Python's % checks.  All pairs of the operand set, one lane a pair."""
    vals = operands(); pairs = [(a, b) for a in vals for b in vals]; A = [a for a, _ in pairs]; B = [b for _, b in pairs]
    assert e.secp_ops("fq_mul", A, B) == [a * b % P for a, b in pairs]
    assert e.secp_ops("n_mul", A, B) == [a * b % N for a, b in pairs]
    assert e.secp_ops("fq_sqr", vals) == [a * a % P for a in vals]
    assert e.secp_ops("fq_reduce", vals) == [a % P for a in vals] and e.secp_ops("n_reduce", vals) == [a % N for a in vals]
    canon = [(a, b) for a, b in pairs if a < P and b < P]; A = [a for a, _ in canon]; B = [b for _, b in canon]
    assert e.secp_ops("fq_add", A, B) == [(a + b) % P for a, b in canon]
    assert e.secp_ops("fq_sub", A, B) == [(a - b) % P for a, b in canon]
    fq = [a for a in vals if a < P]; fn = [a for a in vals if a < N]
    assert e.secp_ops("fq_neg", fq) == [-a % P for a in fq]
    assert e.secp_ops("fq_inv", fq) == [pow(a, P - 2, P) for a in fq]                                  # inv(0) = 0
    assert e.secp_ops("fq_sqrt", fq) == [pow(a, (P + 1) // 4, P) for a in fq]
    assert e.secp_ops("n_inv", fn) == [pow(a, N - 2, N) for a in fn]

def test_raw_products_on_every_path_of_the_reduction(e):
    """reduce512's carries, reached on purpose (tests/secp_model.py fold_trace and reduce_cases; tests/test_secp_reduce_cpu.py shows on the CPU that every class is
    delivered and that a dropped carry is wrong on all of it): the fold-2 carries 0, 1, 2 and the fold-3 carry modulo N, also with a = 2^256 - 1; the fold-2 carry
    modulo p; the final subtraction after a product with a non-zero high half, both moduli.  Every case of every class goes to both products, one call an operation;
    the squares a^2 = C + d and a^2 = epsilon go to fq_sqr."""
    cases = [ab for name in m.REDUCE_CLASSES for ab in m.reduce_cases(name)[0]]; assert len(cases) == 64 * len(m.REDUCE_CLASSES) == 768
    A = [a for a, _ in cases]; B = [b for _, b in cases]
    assert e.secp_ops("n_mul", A, B) == [a * b % N for a, b in cases]
    assert e.secp_ops("fq_mul", A, B) == [a * b % P for a, b in cases]
    sq = [a for name in ("p sqr (1,0)", "p sqr sub") for a, _ in m.reduce_cases(name)[0]]; assert len(sq) == 128
    assert e.secp_ops("fq_sqr", sq) == [a * a % P for a in sq]

def test_crafted_signatures_take_the_reduction_carries_inside_the_recovery(e):
    """zkRecoverSenders on signatures whose u1 = -m / r, u2 = s / r or both take the fold-3 carry, or the final subtraction after a non-zero high half
    (secp_model.crafted_signatures: 64 of each of five kinds).  A dropped carry changes u1 or u2 by C and gives another key.  The lines with a low s go in one call
    with homestead on; the fold-3 carry in u2 needs s above N / 2 (test_secp_reduce_cpu.py: test_a_low_s_cannot_reach_the_fold_3_carry), so those go in one
    call with homestead off.  Both again without pubs.  ok, keys and addresses against the model on every line."""
    lines = m.crafted_signatures(); want = m.crafted_expected(); z = e.Zk(); assert len(lines) == 320 and 10 * sum(w[0] for w in want) >= 9 * len(want)
    for hs in (True, False):
        idx = [i for i, l in enumerate(lines) if l[1] == hs]; assert len(idx) >= 128
        froms, pubs, ok = z.RecoverSenders([lines[i][2] for i in idx], [lines[i][3] for i in idx], homestead=hs)
        assert ok == [want[i][0] for i in idx]
        assert pubs == [want[i][1].to_bytes(32, "big") + want[i][2].to_bytes(32, "big") for i in idx] and froms == [want[i][3] for i in idx]
        froms2, none, ok2 = z.RecoverSenders([lines[i][2] for i in idx], [lines[i][3] for i in idx], homestead=hs, want_pubs=False)
        assert none is None and (froms2, ok2) == (froms, ok)

def test_resident_table_of_g(e):
    assert e.secp_gtable() == [m.mul(k, m.G) for k in range(1, 16)]

# ---- the walk -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_walk_small_family_single_digits_random_and_every_exceptional_branch(e):
    """u1 G + u2 P through the recovery's own launches.  u1, u2 in {0, +-1 ... +-9} (negatives mod N) with P = k G for k in {1, 2, 16, N - 1}: 1,444 cases.  With
    P = +-G or 2 G the walk meets its own table entries: (1, 1, G) adds G to G (equal operands), (1, 1, -G) adds -G to G (opposite operands, result at infinity), and
    every case with a non-zero digit starts from the running sum at infinity.  Then one non-zero 4-bit digit at every one of the 64 window positions, and 64 random
    cases.  One call; afterwards the counters of that call show each of the four branches taken."""
    rng = random.Random(5); small = [0] + [s * j % N for j in range(1, 10) for s in (1, -1)]; u1 = []; u2 = []; pts = []; want = []
    mult = {}                                                                                       # j (k G) for the small family, by addition
    for k in (1, 2, 16, N - 1):
        base = m.mul(k, m.G); acc = None
        for j in range(0, 10): mult[(k, j)] = acc; mult[(k, -j % N)] = m.neg(acc); acc = m.add(acc, base)
    for k in (1, 2, 16, N - 1):
        base = m.mul(k, m.G)
        for a in small:
            for b in small: u1.append(a); u2.append(b); pts.append(base); want.append(m.add(mult[(1, a)], mult[(k, b)]))
    assert len(u1) == 1444 and None in want
    for w in range(64):
        a = rng.randrange(1, 16) << (4 * w); b = rng.randrange(1, 16) << (4 * (63 - w)); base = m.mul(rng.randrange(1, N), m.G)
        u1.append(a); u2.append(b); pts.append(base); want.append(m.lincomb(a, b, base))
    for _ in range(64):
        a = rng.randrange(N); b = rng.randrange(N); base = m.mul(rng.randrange(1, N), m.G); u1.append(a); u2.append(b); pts.append(base); want.append(m.lincomb(a, b, base))
    assert e.secp_lincomb(u1, u2, pts) == want
    c = e.senders_counters(); assert all(c[k] >= 1 for k in ("equal", "opposite", "at_infinity", "to_infinity")), c

# ---- the call -------------------------------------------------------------------------------------------------------------------------------------------------------
def by_flag(hs): return [l for l in LINES if l[2] == hs]

def test_every_fixture_line(e):
    """ok, pubs and froms of every line equal the reference library's verdict and key and the address of that key; the outputs are zero where ok = 0"""
    z = e.Zk(); seen = 0
    for hs in (0, 1):
        lines = by_flag(hs); froms, pubs, ok = z.RecoverSenders([l[0] for l in lines], [l[1] for l in lines], homestead=bool(hs)); seen += len(lines)
        assert ok == [l[3] for l in lines] and pubs == [l[4] for l in lines] and froms == [l[5] for l in lines]
        assert all(p == bytes(64) and f == bytes(20) for p, f, o in zip(pubs, froms, ok) if not o)
    assert seen == len(LINES) and sum(l[3] for l in LINES) >= 300 and sum(not l[3] for l in LINES) >= 90

@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_counts_around_the_wave_and_workgroup_sizes(e, n):
    """n lines cut from the fixture's homestead-off lines, taken round and round from an offset so that accepted and refused lines alternate as the fixture has them;
    with and without pubs"""
    lines = by_flag(0); picked = [lines[(7 * n + i) % len(lines)] for i in range(n)]; z = e.Zk()
    froms, pubs, ok = z.RecoverSenders([l[0] for l in picked], [l[1] for l in picked], homestead=False)
    assert ok == [l[3] for l in picked] and pubs == [l[4] for l in picked] and froms == [l[5] for l in picked]
    froms2, none, ok2 = z.RecoverSenders([l[0] for l in picked], [l[1] for l in picked], homestead=False, want_pubs=False)           # pubs = NULL
    assert none is None and (froms2, ok2) == (froms, ok)
    if n >= 63: assert True in ok and False in ok

def test_bad_arguments_leave_the_outputs_as_the_header_says(e):
    import ctypes
    L = e.lib(); lines = by_flag(1)[:3]; hb = np.frombuffer(b"".join(l[0] for l in lines), dtype=np.uint8).copy(); sb = np.frombuffer(b"".join(l[1] for l in lines), dtype=np.uint8).copy()
    def fresh(): return np.full(60, 0xA5, dtype=np.uint8), np.full(192, 0xA5, dtype=np.uint8), np.full(3, 0xA5, dtype=np.uint8)
    def ptr(a): return a.ctypes.data_as(ctypes.c_void_p)
    for fn, bad in ((L.zkgpu_recover_senders, ARG), (L.zkRecoverSenders, -1)):
        fn.restype = ctypes.c_int
        fr, pb, ok = fresh(); assert fn(ptr(hb), ptr(sb), -1, 1, ptr(fr), ptr(pb), ptr(ok)) == bad and set(fr) | set(pb) | set(ok) == {0xA5}       # n < 0: nothing to zero
        fr, pb, ok = fresh(); assert fn(None, ptr(sb), 3, 1, ptr(fr), ptr(pb), ptr(ok)) == bad and not fr.any() and not pb.any() and not ok.any()  # no hashes
        fr, pb, ok = fresh(); assert fn(ptr(hb), None, 3, 1, ptr(fr), ptr(pb), ptr(ok)) == bad and not fr.any() and not pb.any() and not ok.any()  # no signatures
        fr, pb, ok = fresh(); assert fn(ptr(hb), ptr(sb), 3, 1, None, ptr(pb), ptr(ok)) == bad and not pb.any() and not ok.any()                   # no froms
        fr, pb, ok = fresh(); assert fn(ptr(hb), ptr(sb), 3, 1, ptr(fr), ptr(pb), None) == bad and not fr.any() and not pb.any()                   # no ok
        fr, pb, ok = fresh(); assert fn(ptr(hb), ptr(sb), 0, 1, ptr(fr), ptr(pb), ptr(ok)) == 0 and set(fr) | set(pb) | set(ok) == {0xA5}          # n = 0: nothing queued, nothing written
        fr, pb, ok = fresh(); assert fn(ptr(hb), ptr(sb), 3, 1, ptr(fr), ptr(pb), ptr(ok)) == sum(l[3] for l in lines) and bytes(pb) == b"".join(l[4] for l in lines)

def test_two_threads_get_the_answers_of_one(e):
    z = e.Zk(); lines = by_flag(0); parts = (lines[:150], lines[100:]); got = [None, None]
    def run(k):
        for _ in range(3): got[k] = z.RecoverSenders([l[0] for l in parts[k]], [l[1] for l in parts[k]], homestead=False)
    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts: t.start()
    for t in ts: t.join()
    for k in range(2): assert got[k] == ([l[5] for l in parts[k]], [l[4] for l in parts[k]], [l[3] for l in parts[k]])

# ---- into the chain call --------------------------------------------------------------------------------------------------------------------------------------------
def leg_chain(tmp):
    """Three mint proofs in two blocks at the tree depth of tests/test_gpu_chain_accounts.py (its proofs and states are locals of its leg, so only DEPTH and the
    helpers it imports can be shared; the proofs here are made the same way).  Every record's sender is the address of a seeded key; a hash per record is signed with
    the model; the froms that zkRecoverSenders gives go into verifyChainAccounts, and the answer — return value, verdicts, anchors, the filled records, the sizes,
    the table's log — must be what the call gives with the addresses the model computes."""
    import workload as w
    from blockmaze_amd import engine as e
    from test_gpu_block_accounts import ZERO, with_old
    from test_gpu_chain_accounts import DEPTH
    e.keygen("mint", os.path.join(tmp, "mintpk.txt"), os.path.join(tmp, "mintvk.txt"), seed=0x5EED); z = e.Zk(); rng = random.Random(17)
    def mint_of(d): p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("mint", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    items = [mint_of(w.mint_instance(20 + i)) for i in range(3)]; first = [0, 1, 3]; keys = [rng.randrange(1, N) for _ in items]; hashes = [rng.getrandbits(256).to_bytes(32, "big") for _ in items]
    sigs = [m.sign(h, k, rng.randrange(1, N)) for h, k in zip(hashes, keys)]; model = [m.address(m.mul(k, m.G)) for k in keys]
    froms, pubs, ok = z.RecoverSenders(hashes, sigs); assert ok == [True] * 3 and len(set(model)) == 3
    tree = e.Tree(DEPTH); leaves = w.deposit_instance(1, 8)["leaves"]; assert z.TreeAppend(tree.h, leaves) == 8; answers = []
    for road in (froms, model):
        a = e.AccountTable(); assert z.AcctsSet(a, list(model), [it[2][0] for it in items]) == 0; s = e.SpentSet(bytes(20))   # (the state belongs to the real senders on both roads)
        got = z.VerifyChainAccounts(None, e.records_from_items([with_old(it, ZERO) for it in items]), list(road), first, a, tree.h, [8], 8, s.h)
        answers.append((got[:3], got[3].tobytes(), got[4:], a.read_log(), s.read_log(), tree.size())); a.close(); s.close(); assert z.TreeRewind(tree.h, 8) == 8
    assert answers[0] == answers[1] and answers[0][0] == (2, [True] * 3, [-1] * 3), answers[0][0]          # the two roads first: a wrong sender shows here as a record not accepted
    assert froms == model
    tree.close()

def test_recovered_senders_into_verify_chain_accounts(tmp_path):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chain", str(tmp_path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path)))
    assert r.returncode == 0 and "LEG OK chain" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])

if __name__ == "__main__":
    {"chain": leg_chain}[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
