"""Two keys a record on the device (SpentSet::spend_pairs in blockmaze_amd/csrc/gpu_snset.hip; include/zkgpu.h, include/zk_spent_pk.h) against the Python model of
tests/test_snset_pairs_cpu.py and the library's host model (zkgpu_test_snset_host_pairs).  After every mutating step the table read back from the device must satisfy
the invariants of check_table.  Every leg runs in a process of its own under a time limit: `python tests/test_gpu_snset_pairs.py <leg> <scratch dir>` is what each
test starts."""
import os, random, subprocess, sys, threading
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
from test_snset_cpu import model_spend, universe
from test_snset_pairs_cpu import chain, model_pairs

pytestmark = pytest.mark.gpu
TOMB = 0xFFFFFFFF

def check_table(e, s, log):
    """every live log index exactly once and no tentative value; each entry reachable from its home slot (computed here from the documented mix and the seed) without
    crossing an empty slot; the tombstone count is the host's; the load factor holds; size and log are the model's"""
    t, seed, tombs = s.slots(); n = len(log); N = len(t); assert N >= 16 and N & (N - 1) == 0
    live = t[(t != 0) & (t != TOMB)]; assert sorted(live.tolist()) == list(range(1, n + 1)), (n, sorted(live.tolist())[:10])
    assert int((t == TOMB).sum()) == tombs and 2 * (n + tombs) <= N, (n, tombs, N)
    assert s.size() == n and s.read_log() == log
    pos = {int(v): i for i, v in enumerate(t.tolist()) if v not in (0, TOMB)}
    for idx, key in enumerate(log):
        j = e.snset_home(key, seed, N); p = pos[idx + 1]
        while j != p: assert t[j] != 0, (idx, j); j = (j + 1) % N
    return t, tombs

class Checked:
    """a device set and the model's log side by side: every call is compared with the Python model and with the host model, every mutation checks the table"""
    def __init__(self, e, exempt=None, log2_slots=None, seed=0): self.e = e; self.exempt = exempt; self.s = e.SpentSet(exempt, log2_slots, seed); self.log = []
    def spend_pairs(self, pairs, commit=True):
        want, log = model_pairs(self.log, self.exempt, pairs, commit); host, app = self.e.snset_host_pairs(self.log, self.exempt, pairs, commit)
        assert host == want and app == log[len(self.log):]
        got, size = self.s.spend_pairs(pairs, commit); assert got == want and size == len(log), ([i for i in range(len(pairs)) if got[i] != want[i]][:8], size, len(log))
        self.log = log; check_table(self.e, self.s, self.log); return got
    def rewind(self, m): self.s.rewind(m); del self.log[m:]; check_table(self.e, self.s, self.log)
    def query_all(self, size, keys):
        at = {k: i for i, k in enumerate(self.log)}; assert self.s.query(size, keys) == [at[k] if k in at and at[k] < size else None for k in keys], size

def random_pairs(rng, U, n): return [None if r < 0.1 else (rng.choice(U),) if r < 0.4 else (rng.choice(U), rng.choice(U)) for r in (rng.random() for _ in range(n))]

# ---- the legs (each in a fresh process) ------------------------------------------------------------------------------------------------------------------------
def leg_differential(tmp):
    from blockmaze_amd import engine as e
    rng = random.Random(71); seen = set(); r0 = e.snset_rounds()
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000):
        U = universe(max(4, n // 2), 700 + n); c = Checked(e, U[0], 4, 0xD1FF + n); c.spend_pairs([(k,) for k in U[1:1 + len(U) // 4]])   # an alphabet so small that most records collide; a quarter of it resident
        if n in (65, 257): c.s.round_cap(1)                                                                # these two: the host finishes whatever the first round leaves open
        for rep in range(3):
            batch = random_pairs(rng, U, n); a = c.spend_pairs(batch, False); b = c.spend_pairs(batch, True); assert a == b; seen |= set(b)
            c.query_all(len(c.log), U)
    A, B, C, D = universe(4, 72); c = Checked(e, C, 4, 5)
    assert c.spend_pairs([(C, A), (C,), (B, C), (A, A), (B, B), (B,), None, (D, A), (D,)]) == [0, 0, 1, 2, 2, 0, 0, 2, 0] and c.log == [A, B, D]   # the exempt key first and second; k1 == k2; a rejected record inserts nothing
    r1 = e.snset_rounds(); print("rounds", r1[0] - r0[0], "host finishes", r1[1] - r0[1]); assert seen == {0, 1, 2}

def leg_check_only(tmp):
    from blockmaze_amd import engine as e
    U = universe(400, 33); rng = random.Random(34)
    for log2, resident, batch in ((None, U[:50], random_pairs(rng, U[30:90], 60)), (4, U[:5], random_pairs(rng, U[:60], 40)),      # (the last two need a larger table than the set's: the call
                                  (10, U[:300], random_pairs(rng, U[100:399], 300))):                                              #  runs on a rebuilt copy)
        c = Checked(e, None, log2, 99); c.s.spend(resident); c.log = list(resident); t0, seed0, tombs0 = c.s.slots(); log0 = c.s.read_log(); assert log2 is None or 2 * (len(resident) + 2 * len(batch)) > len(t0)
        a = c.spend_pairs(batch, False); t1, seed1, tombs1 = c.s.slots()
        assert t0.tobytes() == t1.tobytes() and (seed0, tombs0) == (seed1, tombs1) and c.s.read_log() == log0 and c.s.size() == len(resident), log2
        assert 1 in a and 2 in a and 0 in a and c.spend_pairs(batch, True) == a, log2

def leg_single_key(tmp):
    from blockmaze_amd import engine as e
    U = universe(300, 44); rng = random.Random(45); a = e.SpentSet(U[0], 4, 77); b = e.SpentSet(U[0], 4, 77); log = []
    for n in (1, 5, 64, 257, 700):
        keys = [rng.choice(U) for _ in range(n)]; mask = [rng.random() < 0.8 for _ in range(n)]; commit = n != 64
        want, log = model_spend(log, U[0], keys, mask, commit); got_a = a.spend(keys, mask, commit); got_b = b.spend_pairs([(k,) if m else None for k, m in zip(keys, mask)], commit)
        assert got_a == got_b == (want, len(log)) and a.read_log() == b.read_log() == log, n
        check_table(e, a, log); check_table(e, b, log); assert b.slots()[2] == 0                                               # one key a record: no rejected record holds a slot, no tombstone

def leg_chain(tmp):
    from blockmaze_amd import engine as e
    U = universe(100, 55)
    for L in (12, 13):
        pairs = chain(L, U); want, log = model_pairs([], None, pairs, True); assert want == [i % 2 * 2 for i in range(L)]
        a = Checked(e, None, 4, L); r0, h0 = e.snset_rounds(); assert a.spend_pairs(pairs) == want; r1, h1 = e.snset_rounds(); assert (r1 - r0, h1 - h0) == ((L + 1) // 2, 0), (L, r1 - r0, h1 - h0)
        b = Checked(e, None, 4, L); b.s.round_cap(2); assert b.spend_pairs(pairs) == want; r2, h2 = e.snset_rounds(); assert (r2 - r1, h2 - h1) == (2, 1), (L, r2 - r1, h2 - h1)
        assert a.log == b.log == log
        b.s.round_cap(2); assert b.spend_pairs(pairs, False) == [1] * L and e.snset_rounds() == (r2 + 1, h2)              # everything resident: decided in the first round
        b.s.round_cap(0); pairs2 = chain(L, U[50:]); r3, h3 = e.snset_rounds(); b.spend_pairs(pairs2); assert e.snset_rounds() == (r3 + (L + 1) // 2, h3)   # 0: the default cap again

def leg_launches(tmp):
    from blockmaze_amd import engine as e
    U = universe(26000, 77); s = e.SpentSet(); s.spend(U[:20000]); assert len(s.slots()[0]) == 65536                     # room for what follows: no rebuild is due
    pair = lambda i: (U[20000 + 2 * i], U[20001 + 2 * i]) if i % 2 else (U[20000 + 2 * i],)
    k0 = e.snset_launches(); r0 = e.snset_rounds(); got, size = s.spend_pairs([pair(0)]); k1 = e.snset_launches(); r1 = e.snset_rounds(); assert got == [0] and size == 20001
    batch = [pair(i) for i in range(1, 1001)]; got, size = s.spend_pairs(batch); k2 = e.snset_launches(); r2 = e.snset_rounds()
    assert k1 - k0 == k2 - k1 <= 4 and got == [0] * 1000 and size == 20001 + 1500 and len(s.slots()[0]) == 65536, (k0, k1, k2)
    assert (r1[0] - r0[0], r2[0] - r1[0]) == (1, 1) and r2[1] == r0[1]                                                 # no conflict among the batch's own keys: one round
    got, size = s.spend_pairs(batch + [(U[0], U[25999])], False); assert got == [1] * 1001 and e.snset_launches() - k2 == k1 - k0   # resident keys are no conflict inside the batch either
    check_table(e, s, U[:20001] + [k for p in batch for k in p])

def leg_rewind(tmp):
    from blockmaze_amd import engine as e
    U = universe(100, 88); c = Checked(e, None, 4, 3); pairs = [(U[2 * i], U[2 * i + 1]) for i in range(20)]; assert c.spend_pairs(pairs) == [0] * 20 and c.log == U[:40]
    c.rewind(21); assert c.s.slots()[2] == 19 and c.log == U[:21]                                                       # between k1 and k2 of record 10
    c.query_all(21, U[:44]); assert c.s.query(21, [U[20], U[21]]) == [20, None]
    assert c.spend_pairs([(U[20], U[21]), (U[21], U[22]), (U[50], U[20]), (U[23],)]) == [1, 0, 1, 0] and c.log == U[:21] + [U[21], U[22], U[23]]   # k1 stayed, k2 went
    for m in (0, 1, 21, 22, 24): c.query_all(m, U[:44])
    c.rewind(0); assert c.spend_pairs(pairs[::-1]) == [0] * 20

def leg_threads(tmp):
    from blockmaze_amd import engine as e
    U = universe(6000, 99); shared = U[:2000]; own = [U[2000:4000], U[4000:6000]]; s = e.SpentSet(); codes = [[], []]; errs = []
    def worker(j):
        try:
            for b in range(40):
                pairs = [(own[j][50 * b + 2 * t], own[j][50 * b + 2 * t + 1]) for t in range(25)] + [(shared[50 * b + 2 * t], shared[50 * b + 2 * t + 1]) for t in range(25)]
                if j: pairs.reverse()
                got, size = s.spend_pairs(pairs); codes[j].append(dict(zip(pairs, got)))
        except BaseException as x: errs.append(x)
    th = [threading.Thread(target=worker, args=(j,)) for j in range(2)]
    for x in th: x.start()
    for x in th: x.join()
    assert not errs, errs
    log = s.read_log(); assert len(log) == len(set(log)) == 6000 and set(log) == set(U)                # every key once
    for b in range(40):
        for t in range(25):
            p = (shared[50 * b + 2 * t], shared[50 * b + 2 * t + 1]); assert sorted((codes[0][b][p], codes[1][b][p])) == [0, 1], b   # a serial order: a shared pair was fresh in exactly one call
            for j in range(2): assert codes[j][b][(own[j][50 * b + 2 * t], own[j][50 * b + 2 * t + 1])] == 0
    at = {k: i for i, k in enumerate(log)}
    for j in range(2):
        for k in range(0, 2000, 2): assert at[own[j][k + 1]] == at[own[j][k]] + 1                       # k2 directly after k1
    check_table(e, s, log)

def leg_block(tmp):
    from blockmaze_amd import engine as e
    import workload as w
    for i, kind in enumerate(("send", "mint", "redeem", "deposit")): e.keygen(kind, os.path.join(tmp, kind + "pk.txt"), os.path.join(tmp, kind + "vk.txt"), seed=0xB10C4A2E + 7 * i)
    z = e.Zk()
    def mint(i): d = w.mint_instance(i); p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("mint", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    def redeem(i): d = w.mint_instance(i, redeem=True); p = z.GenRedeemProof(*w.mint_args(d)); assert z.VerifyRedeemProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("redeem", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    def send(i): d = w.send_instance(i); p = z.GenSendProof(*w.send_args(d)); a = [d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]; assert z.VerifySendProof(p, *a); return ("send", p, a, 0)
    def deposit(i, pk=None):
        """a valid deposit; pk: the one-time address of another deposit instead of its own (the note cmtS, its leaf and the root follow)"""
        d = w.deposit_instance(i, 16)
        if pk is not None:
            d["pk_recv"] = pk; d["cmtS"] = w.cmts(d["value_s"], pk, d["r_s"], d["sn_A_old"]); d["leaves"][d["index"]] = d["cmtS"]; d["rt"], _ = w.merkle_root_and_path(d["leaves"], d["index"])
        p = z.GenDepositProof(*w.deposit_args(d), d["leaves"], d["rt"], d["sk"]); a = [d["rt"], d["pk_recv"], d["cmtB_old"], d["sn_old"], d["cmtB"], d["sn_s"]]
        assert z.VerifyDepositProof(p, *a); return ("deposit", p, a, 0), d["leaves"]
    pad = lambda pk: bytes(12) + pk; flip = lambda b: bytes([b[0] ^ 1]) + b[1:]
    M1, M2, R1, S1 = mint(1), mint(2), redeem(1), send(1)
    (D1, l1), (D3, l3), (D4, l4) = deposit(1), deposit(3), deposit(4); (D2, l2) = deposit(2, D1[2][1]); (D5, l5) = deposit(5, D4[2][1])
    D1bad = ("deposit", D1[1], D1[2][:4] + [flip(D1[2][4])] + D1[2][5:], 0)
    sn = lambda it: it[2][3 if it[0] == "deposit" else 1]; pk = lambda it: pad(it[2][1])
    assert len(set(sn(x) for x in (D1, D2, D3, D4, D5))) == 5 and pk(D2) == pk(D1) and pk(D5) == pk(D4) and len(set(pk(x) for x in (D1, D3, D4))) == 3
    items = [M1, D1, S1, D2, D3, R1, D4, D5, M1, M2, D1bad]; recs = e.records_from_items(items); leaves = l1 + l2 + l3 + l4 + l5; lists = [(16 * j, 16) for j in range(5)]
    list_of = [-1, 0, -1, 1, 2, -1, 3, 4, -1, -1, 0]
    plain = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    # D2: its pk is D1's -> goes, and its serial number is not burnt.  D3: its pk is in the set.  D4: its serial number is in the set -> goes, and frees its pk for D5.  M1 twice.
    state = [1, 1, 1, 0, 0, 1, 0, 1, 0, 1, 0]
    rc0, ok0 = z.VerifyBlockRecordsRoots(recs, leaves, lists, list_of); assert (rc0, [int(x) for x in ok0]) == (sum(plain), plain)
    assert z.VerifyBlockState(None, recs, leaves, lists, list_of, None, True) == (rc0, ok0, None)          # no set: verifyBlockRecordsRoots
    def fresh():
        s = z.SnSetNew(bytes(32)); assert s and z.SnSetSpend(s, [pk(D3), sn(D4)]) == (2, [False, False]); return s
    s = fresh()
    rc, ok, size = z.VerifyBlockState(None, recs, leaves, lists, list_of, s, False); assert (rc, [int(x) for x in ok], size) == (sum(state), state, 2) and z.SnSetSize(s) == 2   # the pool's check changes nothing
    rc, ok, size = z.VerifyBlockState(None, recs, leaves, lists, list_of, s, True); assert (rc, [int(x) for x in ok], size) == (sum(state), state, 2 + 4 + 2 * 2) and z.SnSetSize(s) == 10   # an accepted deposit: two keys
    assert z.SnSetContains(s, [sn(D2), sn(D3), sn(D1), pk(D1), sn(D5), pk(D4), sn(D4)]) == [False, False, True, True, True, True, True]   # a rejected deposit has not burnt its serial number
    assert z.SnSetContains(s, [sn(M1), sn(D1), pk(D1), sn(S1)], 5) == [True, True, True, False]             # the log: the two keys of fresh(), M1, D1's serial number and then its pk, S1, ...
    assert z.VerifyBlockState(None, recs, leaves, lists, list_of, s, True) == (0, [False] * 11, 10)
    # the drop-in pairs call on the same keys
    t = fresh(); assert z.SnSetSpendPairs(t, [sn(x) for x in items[:10]], [pk(x) if x[0] == "deposit" else None for x in items[:10]]) == (10, [not x for x in state[:10]])
    assert z.SnSetSpendPairs(t, [sn(D2), bytes(32)], [bytes(32), pk(D2)], False) == (10, [False, True]) and z.SnSetSpendPairs(t, [sn(D2)], None) == (11, [False]); z.SnSetFree(t)
    # a block without deposits: verifyBlockFull's verdicts and size
    nd = [M1, S1, R1, M1, M2, S1]; a, b = fresh(), fresh()
    assert z.VerifyBlockState(None, nd, None, None, None, a, True) == z.VerifyBlockFull(nd, None, None, None, b, True) == (4, [True, True, True, False, True, False], 6); z.SnSetFree(a); z.SnSetFree(b)
    # behind a proof cache: the second pass over the block finds its proofs there, and decides the same
    c = e.ProofCache(64); u = fresh(); first = z.VerifyBlockState(c, recs, leaves, lists, list_of, u, False); h1 = c.stats(); second = z.VerifyBlockState(c, recs, leaves, lists, list_of, u, True); h2 = c.stats()
    assert first == (sum(state), [bool(x) for x in state], 2) and second == (sum(state), [bool(x) for x in state], 10) and h1[0] == 0 and h2[0] - h1[0] >= 9, (h1, h2)   # nine distinct valid records
    z.SnSetFree(u); z.SnSetFree(s)

LEGS = {"differential": leg_differential, "check_only": leg_check_only, "single_key": leg_single_key, "chain": leg_chain, "launches": leg_launches, "rewind": leg_rewind, "threads": leg_threads,
        "block": leg_block}

def run_leg(name, tmp_path, timeout=300):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path)))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

def test_differential_against_the_model(tmp_path): print(run_leg("differential", tmp_path))
def test_check_only_leaves_table_and_log_bit_for_bit(tmp_path): run_leg("check_only", tmp_path)
def test_single_key_batches_equal_spend(tmp_path): run_leg("single_key", tmp_path)
def test_alternating_chain_rounds_and_host_finish(tmp_path): run_leg("chain", tmp_path)
def test_no_internal_conflict_one_round_whatever_n(tmp_path): run_leg("launches", tmp_path)
def test_rewind_into_the_middle_of_a_pair(tmp_path): run_leg("rewind", tmp_path)
def test_two_threads_on_one_set(tmp_path): run_leg("threads", tmp_path)
def test_verify_block_state(tmp_path): run_leg("block", tmp_path, 600)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
