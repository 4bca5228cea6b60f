"""The resident set of spent serial numbers (blockmaze_amd/csrc/gpu_snset.hip; include/zkgpu.h, include/zk_spent.h) against the Python model of
tests/test_snset_cpu.py and the library's host model (zkgpu_test_snset_host).  After every mutating step the table read back from the device must satisfy the
invariants of check_table.  Every leg runs in a process of its own under a time limit: `python tests/test_gpu_snset.py <leg> <scratch dir>` is what each test starts."""
import ctypes, os, random, subprocess, sys, threading
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
from test_snset_cpu import model_spend, universe

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
    """a device set and the model's log side by side: every spend is compared with the Python model and with the host model, every mutation checks the table"""
    def __init__(self, e, exempt=None, log2_slots=None, seed=0): self.e = e; self.exempt = exempt; self.s = e.SpentSet(exempt, log2_slots, seed); self.log = []
    def spend(self, keys, mask=None, commit=True):
        want, log = model_spend(self.log, self.exempt, keys, mask, commit); host, app = self.e.snset_host(self.log, self.exempt, keys, mask, commit)
        assert host == want and app == log[len(self.log):]
        got, size = self.s.spend(keys, mask, commit); assert got == want and size == len(log), ([i for i in range(len(keys)) if got[i] != want[i]][:8], size, len(log))
        self.log = log; check_table(self.e, self.s, self.log); return got
    def rewind(self, m): self.s.rewind(m); del self.log[m:]; check_table(self.e, self.s, self.log)
    def query_all(self, size, keys):
        at = {k: i for i, k in enumerate(self.log)}; assert self.s.query(size, keys) == [at[k] if k in at and at[k] < size else None for k in keys], size

def keys_with_home(e, seed, n_slots, home, count, start):
    out = []; c = start
    while len(out) < count:
        k = c.to_bytes(20, "big"); c += 1
        if e.snset_home(k, seed, n_slots) == home: out.append(k)
    return out

# ---- the legs (each in a fresh process) ------------------------------------------------------------------------------------------------------------------------
def leg_chains(tmp):
    from blockmaze_amd import engine as e
    seed = 0x5EED5EED1234; A = keys_with_home(e, seed, 16, 5, 3, 1); Wr = keys_with_home(e, seed, 16, 15, 3, 1000); keys = A + Wr
    absent = keys_with_home(e, seed, 16, 6, 1, 5000) + keys_with_home(e, seed, 16, 0, 1, 6000) + keys_with_home(e, seed, 16, 10, 1, 7000) + keys_with_home(e, seed, 16, 15, 1, 8000)
    c = Checked(e, None, 4, seed)
    for k in keys: assert c.spend([k]) == [0]
    t, _ = check_table(e, c.s, keys); assert len(t) == 16 and [int(t[i]) for i in (5, 6, 7, 15, 0, 1)] == [1, 2, 3, 4, 5, 6] and int((t != 0).sum()) == 6   # three share slot 5's chain; one chain wraps past slot 15 to 0
    c.query_all(6, keys + absent); assert c.s.query(6, absent) == [None] * 4
    for m in range(7): c.query_all(m, keys + absent)
    d = Checked(e, None, 4, seed); assert d.spend(keys) == [0] * 6; t, _ = check_table(e, d.s, keys); assert len(t) == 16 and sorted(np.nonzero(t)[0].tolist()) == [0, 1, 5, 6, 7, 15]
    d.query_all(6, keys + absent); assert d.spend(keys + absent[:1]) == [1] * 6 + [0]

def leg_repeats(tmp):
    from blockmaze_amd import engine as e
    U = universe(700, 21); EX = U[699]; c = Checked(e, EX)
    for r in (2, 3, 70): assert c.spend([U[r]] * r) == [0] + [2] * (r - 1)                              # 70: more than a wave
    assert len(c.log) == 3
    keys = list(U[100:700 - 1]) + [U[98]]; assert len(keys) == 600; X = U[99]; keys[0] = keys[300] = keys[599] = X; mask = [1] * 600; mask[0] = 0
    got = c.spend(keys, mask); assert got[0] == 0 and got[300] == 0 and got[599] == 2 and sum(got) == 2 and c.log[3:] == [k for i, k in enumerate(keys) if i not in (0, 599)]
    assert c.spend([U[2], X, U[2], U[150], X]) == [1] * 5                                              # resident, repeated: 1 every time
    n = len(c.log); assert c.spend([EX] * 5) == [0] * 5 and c.spend([EX, U[1], EX, U[1]]) == [0, 0, 0, 2] and len(c.log) == n + 1
    assert c.s.query(len(c.log), [EX]) == [None]

def leg_check_only(tmp):
    from blockmaze_amd import engine as e
    U = universe(400, 33)
    for log2, resident, batch in ((None, U[:50], U[40:60] + U[55:70] + [U[300]] * 3 + U[:5]), (4, U[:5], U[3:40] + U[10:12]), (10, U[:300], U[100:399] + U[390:395])):   # (the last two need a larger table than the set's: the call runs on a rebuilt copy)
        c = Checked(e, None, log2, 99); c.spend(resident); t0, seed0, tombs0 = c.s.slots(); log0 = c.s.read_log(); launches = e.snset_launches()
        a = c.spend(batch, None, False); t1, seed1, tombs1 = c.s.slots()
        assert t0.tobytes() == t1.tobytes() and (seed0, tombs0) == (seed1, tombs1) and c.s.read_log() == log0 and c.s.size() == len(resident), log2
        mask = [i % 3 != 0 for i in range(len(batch))]; c.spend(batch, mask, False); assert c.s.slots()[0].tobytes() == t0.tobytes()
        assert 1 in a and 2 in a and 0 in a and c.spend(batch, None, True) == a, log2

def leg_growth(tmp):
    from blockmaze_amd import engine as e
    U = universe(400, 44); c = Checked(e, None, 4, 7); at = 0; sizes = [len(c.s.slots()[0])]; assert sizes == [16]
    for k in (5, 9, 40, 300):
        due = 2 * (at + k) > sizes[-1]; c.spend(U[at:at + k]); at += k; sizes.append(len(c.s.slots()[0])); assert (sizes[-1] > sizes[-2]) == due, sizes   # each rebuild: a larger slots array
        c.query_all(at, U); assert c.log == U[:at]
    assert sizes == [16, 16, 32, 128, 1024] and c.spend(U[:at]) == [1] * at                              # (5 keys fit the first 16 slots; 14, 54 and 354 need 32, 128 and 1,024)

def leg_rewind(tmp):
    from blockmaze_amd import engine as e
    U = universe(400, 55); c = Checked(e, None, 4, 3)
    for b in range(5): c.spend(U[40 * b:40 * b + 40])
    for m in (0, 40, 80, 120, 160, 200, 1, 95, 161): c.query_all(m, U[:230])
    c.rewind(120); assert c.s.slots()[2] == 80; c.query_all(120, U[:230]); assert c.s.query(120, U[120:200]) == [None] * 80
    again = U[199:119:-1] + U[200:230]; assert c.spend(again) == [0] * 110 and c.log == U[:120] + again
    k0 = e.snset_launches(); c.rewind(len(c.log)); assert e.snset_launches() == k0                        # rewind to the current size: nothing happens
    L = e.lib(); t0 = c.s.slots()[0].tobytes(); rc = L.zkgpu_snset_rewind(ctypes.c_void_p(c.s.h), ctypes.c_uint64(len(c.log) + 1)); assert rc == -2
    out = (ctypes.c_uint64 * 1)(77); assert L.zkgpu_snset_query(ctypes.c_void_p(c.s.h), ctypes.c_uint64(len(c.log) + 1), U[0], ctypes.c_size_t(1), out) == -2 and out[0] == 77
    buf = ctypes.create_string_buffer(b"\x07" * 40, 40); assert L.zkgpu_snset_read_log(ctypes.c_void_p(c.s.h), ctypes.c_uint64(len(c.log)), ctypes.c_uint64(1), buf) == -2 and buf.raw == b"\x07" * 40
    assert L.zkgpu_snset_spend(ctypes.c_void_p(c.s.h), None, None, ctypes.c_size_t(2), 1, buf, None) == -2 and L.zkgpu_snset_spend(ctypes.c_void_p(c.s.h), U[0] + U[1], None, ctypes.c_size_t(2), 1, None, None) == -2
    assert buf.raw == b"\x07" * 40 and c.s.slots()[0].tobytes() == t0 and e.snset_launches() == k0; check_table(e, c.s, c.log)
    c.rewind(0); t, _, tombs = c.s.slots(); assert not t.any() and tombs == 0 and c.s.query(0, U[:3]) == [None] * 3
    assert c.spend(U[:10]) == [0] * 10
    # tombstones force a rebuild: a small table, four keys, and rounds of "rewind to 2, add 2 new keys"
    d = Checked(e, None, 4, 12); d.spend(U[300:304]); at = 304; rebuilt = 0; seen = []
    for _ in range(8):
        d.rewind(2); before = d.s.slots()[2]; d.spend(U[at:at + 2]); at += 2; after = d.s.slots()[2]; seen.append((before, after)); rebuilt += after == 0 and before > 0
    assert rebuilt >= 2 and max(b for b, a in seen) >= 4 and len(d.s.slots()[0]) == 16, seen

def leg_differential(tmp):
    from blockmaze_amd import engine as e
    U = universe(64, 66); rng = random.Random(67); c = Checked(e, U[63], 4, 0xD1FF); ops = {"spend": 0, "check": 0, "query": 0, "rewind": 0}
    for step in range(300):
        r = rng.random()
        if r < 0.55:
            n = rng.choice([1, 2, 3, 5, 9, 20]); keys = [rng.choice(U) for _ in range(n)]; mask = None if rng.random() < 0.4 else [rng.random() < 0.75 for _ in range(n)]
            commit = rng.random() < 0.6; c.spend(keys, mask, commit); ops["spend" if commit else "check"] += 1
        elif r < 0.8: c.query_all(rng.randrange(len(c.log) + 1), U); ops["query"] += 1
        else: c.rewind(rng.randrange(len(c.log) + 1) if rng.random() < 0.8 else len(c.log)); ops["rewind"] += 1
    print(ops, "final size", len(c.log)); assert min(ops.values()) >= 20

def leg_launches(tmp):
    from blockmaze_amd import engine as e
    U = universe(26000, 77); s = e.SpentSet(); s.spend(U[:20000]); assert len(s.slots()[0]) == 65536                     # room for what follows: no rebuild is due
    k0 = e.snset_launches(); s.spend(U[20000:20001]); k1 = e.snset_launches(); got, size = s.spend(U[21000:26000]); k2 = e.snset_launches()
    assert k1 - k0 == k2 - k1 <= 3 and got == [0] * 5000 and size == 25001 and len(s.slots()[0]) == 65536, (k0, k1, k2)
    s.spend(U[:1], None, False); assert e.snset_launches() - k2 == k1 - k0
    t = e.SpentSet(None, 4, 1); t.spend(U[:3]); k3 = e.snset_launches(); t.spend(U[3:103]); k4 = e.snset_launches(); assert k4 - k3 == (k1 - k0) + 1 and len(t.slots()[0]) > 16   # a rebuild is due: one more
    check_table(e, s, U[:20001] + U[21000:26000])

def leg_threads(tmp):
    from blockmaze_amd import engine as e
    U = universe(3000, 88); shared = U[:1000]; own = [U[1000:2000], U[2000:3000]]; s = e.SpentSet(); codes = [[], []]; errs = []
    def worker(j):
        try:
            for b in range(40):
                keys = own[j][25 * b:25 * b + 25] + shared[25 * b:25 * b + 25]
                if j: keys.reverse()
                got, size = s.spend(keys); codes[j].append(dict(zip(keys, got)))
        except BaseException as x: errs.append(x)
    th = [threading.Thread(target=worker, args=(j,)) for j in range(2)]
    for x in th: x.start()
    for x in th: x.join()
    assert not errs, errs
    log = s.read_log(); assert len(log) == len(set(log)) == 3000 and set(log) == set(U)                # every key once
    for b in range(40):
        for k in shared[25 * b:25 * b + 25]: assert sorted((codes[0][b][k], codes[1][b][k])) == [0, 1], b   # a serial order: a shared key was fresh in exactly one call
        for j in range(2): assert all(codes[j][b][k] == 0 for k in own[j][25 * b:25 * b + 25])
    check_table(e, s, log)

def leg_block(tmp):
    from blockmaze_amd import engine as e
    import workload as w
    for i, kind in enumerate(("send", "mint", "redeem", "deposit")): e.keygen(kind, os.path.join(tmp, kind + "pk.txt"), os.path.join(tmp, kind + "vk.txt"), seed=0xB10C4A2E + 7 * i)
    z = e.Zk()
    def mint(i): d = w.mint_instance(i); p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("mint", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    def redeem(i): d = w.mint_instance(i, redeem=True); p = z.GenRedeemProof(*w.mint_args(d)); assert z.VerifyRedeemProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("redeem", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    def send(i): d = w.send_instance(i); p = z.GenSendProof(*w.send_args(d)); a = [d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]; assert z.VerifySendProof(p, *a); return ("send", p, a, 0)
    def deposit(i):
        d = w.deposit_instance(i, 16); p = z.GenDepositProof(*w.deposit_args(d), d["leaves"], d["rt"], d["sk"]); a = [d["rt"], d["pk_recv"], d["cmtB_old"], d["sn_old"], d["cmtB"], d["sn_s"]]
        assert z.VerifyDepositProof(p, *a); return ("deposit", p, a, 0), d["leaves"]
    M1, M2, M3, R1, R2, S1, S2 = mint(1), mint(2), mint(3), redeem(1), redeem(2), send(1), send(2); D1, leaves = deposit(1)
    flip = lambda b: bytes([b[0] ^ 1]) + b[1:]
    S2bad = ("send", S2[1], [S2[2][0], S2[2][1], flip(S2[2][2]), S2[2][3]], 0); M3bad = ("mint", M3[1], M3[2], M3[3] ^ 1); D1bad = ("deposit", D1[1], D1[2][:4] + [flip(D1[2][4])] + D1[2][5:], 0)
    for bad, good in ((S2bad, S2), (M3bad, M3), (D1bad, D1)): assert bad[2][3 if bad[0] == "deposit" else 1] == good[2][3 if bad[0] == "deposit" else 1]   # a twin spends the same serial number
    items = [M1, S1, D1, R1, S1, S2bad, S2, M2, D1bad, R2, M3bad, M3]; recs = e.records_from_items(items); assert len(recs) == 12 and sorted(set(int(k) for k in recs["kind"])) == [0, 1, 2, 3]
    list_of = [-1, -1, 0, -1, -1, -1, -1, -1, 0, -1, -1, -1]; lists = [(0, 16)]
    plain = [1, 1, 1, 1, 1, 0, 1, 1, 0, 1, 0, 1]; full = [1, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1]          # the valid record twice: the second goes; the valid original after its rejected twin stays
    rc0, ok0 = z.VerifyBlockRecordsRoots(recs, leaves, lists, list_of); assert (rc0, [int(x) for x in ok0]) == (sum(plain), plain)
    assert z.VerifyBlockFull(recs, leaves, lists, list_of, None, True) == (rc0, ok0, None)               # no set: verifyBlockRecordsRoots, byte for byte
    assert z.VerifyBlockFull(recs, None, None, None, None, False)[:2] == z.VerifyBlockRecordsRoots(recs, None, None, [-1] * 12)
    s = z.SnSetNew(bytes(32)); assert s and z.SnSetSize(s) == 0
    rc, ok, size = z.VerifyBlockFull(recs, leaves, lists, list_of, s, False); assert (rc, [int(x) for x in ok], size) == (sum(full), full, 0) and z.SnSetSize(s) == 0   # the pool's check changes nothing
    rc, ok, size = z.VerifyBlockFull(recs, leaves, lists, list_of, s, True); assert (rc, [int(x) for x in ok], size) == (sum(full), full, 8) and z.SnSetSize(s) == 8
    for commit in (False, True): assert z.VerifyBlockFull(recs, leaves, lists, list_of, s, commit) == (0, [False] * 12, 8)   # the same block again: every record spent
    sn = [e.record_sn(r) for r in recs]; assert sn[2] == D1[2][3] and sn[1] == S1[2][1] and sn[0] == M1[2][1] and sn[3] == R1[2][1]
    assert z.SnSetSpend(s, [sn[2], sn[1], D1[2][1] + bytes(12), bytes(32)], False) == (8, [True, True, False, False])   # deposit: args[3]; send: args[1]; not deposit's pk; the exempt value
    assert z.SnSetContains(s, sn) == [True] * 12 and z.SnSetContains(s, sn, 0) == [False] * 12 and z.SnSetContains(s, sn, 9) is None
    assert z.SnSetRewind(s, 3) == 3 and z.SnSetRewind(s, 4) == -1 and z.SnSetContains(s, sn[:4]) == [True, True, True, False]
    rc, ok, size = z.VerifyBlockFull(recs, leaves, lists, list_of, s, True); assert [int(x) for x in ok] == [0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1] and size == 8 and rc == 5
    z.SnSetFree(s)

LEGS = {"chains": leg_chains, "repeats": leg_repeats, "check_only": leg_check_only, "growth": leg_growth, "rewind": leg_rewind, "differential": leg_differential, "launches": leg_launches,
        "threads": leg_threads, "block": leg_block}

def run_leg(name, tmp_path, timeout=300):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path)))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

def test_chains_sharing_a_home_slot_and_wrapping(tmp_path): run_leg("chains", tmp_path)
def test_repeats_inside_one_call(tmp_path): run_leg("repeats", tmp_path)
def test_check_only_leaves_table_and_log_bit_for_bit(tmp_path): run_leg("check_only", tmp_path)
def test_growth_from_a_small_table(tmp_path): run_leg("growth", tmp_path)
def test_rewind_requery_and_tombstone_rebuild(tmp_path): run_leg("rewind", tmp_path)
def test_differential_against_the_model(tmp_path): print(run_leg("differential", tmp_path))
def test_launch_count_does_not_grow_with_n(tmp_path): run_leg("launches", tmp_path)
def test_two_threads_on_one_set(tmp_path): run_leg("threads", tmp_path)
def test_verify_block_full(tmp_path): run_leg("block", tmp_path, 600)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
