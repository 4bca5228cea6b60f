"""The account table on the device (blockmaze_amd/csrc/gpu_accounts.hip; include/zkgpu.h "the account table") against the Python model of
tests/test_accounts_cpu.py.  After every mutating step the log read back must be the model's, prev words included, and the index must satisfy check_table: one slot
an address, holding the address's latest entry, reachable from its home slot."""
import ctypes, os, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
from test_accounts_cpu import Model, random_records, addr_of, ZERO, OLD_ARG

pytestmark = pytest.mark.gpu
TOMB = 0xFFFFFFFF
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000]

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    engine.init(); return engine

def check_table(e, t, m):
    """the log is the model's, prev included; every address has exactly one slot and it holds its latest entry; no other value but tombstones, as many as the host
    counts; the load factor holds; each slot is reachable from the address's home (the documented mix) without crossing an empty slot"""
    log = t.read_log(); assert t.size() == m.size() and [(a, v) for a, v, _ in log] == m.log and [p for _, _, p in log] == m.prevs()
    slots, seed, tombs = t.slots(); N = len(slots); assert N >= 16 and N & (N - 1) == 0
    latest = {}
    for i, (a, _) in enumerate(m.log): latest[a] = i + 1
    live = slots[(slots != 0) & (slots != TOMB)]; assert sorted(live.tolist()) == sorted(latest.values()), (len(live), len(latest))
    assert int((slots == TOMB).sum()) == tombs and 2 * (m.size() + tombs) <= N, (m.size(), tombs, N)
    pos = {int(v): i for i, v in enumerate(slots.tolist()) if v not in (0, TOMB)}
    for a, idx in latest.items():
        j = e.snset_home(a, seed, N); p = pos[idx]
        while j != p: assert slots[j] != 0, (idx, j); j = (j + 1) % N
    return slots, tombs

class Checked:
    """a device table and the model side by side"""
    def __init__(self, e, log2_slots=None, seed=0): self.e = e; self.t = e.AccountTable(log2_slots, seed); self.m = Model()
    def set(self, addrs, values): self.t.set(addrs, values); self.m.set(addrs, values); return check_table(self.e, self.t, self.m)
    def rewind(self, size): self.t.rewind(size); self.m.rewind(size); return check_table(self.e, self.t, self.m)
    def get_all(self, addrs, size=-1): got = self.t.get(addrs, size); assert got == [self.m.value(a, size) for a in addrs], size
    def fill_both(self, froms, recs):
        before = self.t.slots()[0].copy()
        for chained in (False, True):
            got = self.t.fill(froms, recs, chained); want = self.m.fill(froms, recs, chained); assert got.tobytes() == want.tobytes(), (chained, [i for i in range(len(recs)) if got[i].tobytes() != want[i].tobytes()][:8])
        assert np.array_equal(self.t.slots()[0], before); check_table(self.e, self.t, self.m)                   # a fill leaves the index bit for bit
    def commit(self, froms, recs): self.t.commit_chain(froms, recs); self.m.commit_chain(froms, recs); return check_table(self.e, self.t, self.m)
    def close(self): self.t.close()

def senders(mix, n, salt):
    rng = np.random.RandomState(1000 + n + 7 * salt)
    if mix == "distinct": return [addr_of(10 * n + i, salt) for i in range(n)]
    if mix == "three": return [addr_of(int(k), 200) for k in rng.randint(0, 3, n)]
    return [addr_of(77, 201)] * n
def values(n, seed): rng = np.random.RandomState(seed); return [rng.bytes(32) for _ in range(n)]
def kinds(n, seed): rng = np.random.RandomState(seed); k = rng.randint(0, 4, n); k[rng.rand(n) < 0.1] = 7; return k

@pytest.mark.parametrize("mix", ["distinct", "three", "equal"])
def test_set_get_fill_commit_at_every_size(e, mix):
    """n = 0 .. 1000 on one growing table: set, get (resident and absent addresses), both fills over all four kinds and kind 7, commit_chain — the whole 720 bytes of
    every record against the model's; the table of 2^10 slots is rebuilt on the way"""
    c = Checked(e); absent = [addr_of(i, 250) for i in range(3)]; n_slots = []
    for n in SIZES:
        a = senders(mix, n, 1); was = len(c.t.slots()[0]); l0, h0 = e.accts_launches(); c.set(a, values(n, n)); l1, h1 = e.accts_launches(); n_slots.append(len(c.t.slots()[0]))
        over = int(max([a.count(x) for x in set(a)] + [0]) > 256)                                                # a sender with more than 256 records: the host's search, and the third launch again
        assert (l1 - l0, h1 - h0) == ((0, 0) if n == 0 else (3 + int(n_slots[-1] != was) + over, over)), (n, l1 - l0, h1 - h0)   # probe, pred, write, and at most one rebuild: whatever n is
        c.get_all(sorted(set(a)) + absent); assert c.t.get(absent) == [ZERO] * 3
        f = senders(mix, n, 2) if mix == "distinct" else a; recs = random_records(kinds(n, 50 + n), 60 + n); c.fill_both(f, recs); c.commit(f, recs); c.get_all(sorted(set(f)) + absent)
    assert n_slots[0] == 1 << 10 and n_slots[-1] > 1 << 10
    c.close()

def test_small_table_rebuilds_probe_chains_and_tombstones(e):
    """2^4 slots: the table grows by rebuilds, addresses share probe chains, rewinds leave tombstones that later calls walk over, and a rebuild drops them"""
    c = Checked(e, 4, 0x5EED5EED1234); A = [addr_of(i, 9) for i in range(40)]
    slots, _ = c.set(A[:6], values(6, 1)); assert len(slots) == 16
    slots, _ = c.set(A[:3] + A[6:8], values(5, 2)); assert len(slots) == 32                                  # 11 entries + 5: 2^5
    c.get_all(A[:10]); slots, tombs = c.rewind(8); assert tombs == 2 and len(slots) == 32                       # A[6] and A[7] have no entry below 8, A[2] goes back to its first
    slots, tombs = c.rewind(4); assert tombs == 4; c.get_all(A[:10]); c.get_all(A[:10], 2)                      # A[4], A[5] are gone as well: four tombstones
    recs = random_records([0, 1, 2, 3, 7, 1], 3); c.fill_both([A[4], A[0], A[4], A[9], A[1], A[0]], recs)     # claims beside tombstones, released again
    slots, tombs = c.commit([A[4], A[0], A[4], A[9], A[1], A[0]], recs); assert tombs == 4 and len(slots) == 32
    slots, tombs = c.set(A[10:24], values(14, 4)); assert tombs == 0 and len(slots) == 64                      # 2 x (9 + 4 + 14) > 32: rebuilt, the tombstones are gone
    c.get_all(A); c.rewind(0); assert not c.t.slots()[0].any(); c.get_all(A[:4]); c.set(A[:2], values(2, 5)); c.get_all(A[:4]); c.close()

def test_rewind_to_every_size_and_past_states(e):
    """a log of 40 entries over 5 addresses: rewind to every size; after each, get at every past size for resident and absent addresses; regrow and compare again"""
    rng = np.random.RandomState(40); A = [addr_of(i, 11) for i in range(5)]; absent = [addr_of(i, 12) for i in range(2)]
    who = [A[int(k)] for k in rng.randint(0, 5, 40)]; who[20] = who[23] = A[2]; who[21] = who[22] = A[3]; vals = values(40, 41)
    for m in range(41):
        c = Checked(e, 4, 7 + m); c.set(who[:25], vals[:25]); c.set(who[25:], vals[25:]); c.rewind(m)
        for size in list(range(m + 1)) + [-1]: c.get_all(A + absent, size)
        assert c.t.get(absent, m) == [ZERO] * 2
        c.set(who[m:][::-1], vals[m:]); assert c.m.size() == 40                                                  # regrown, in another order
        for size in (0, m // 2, m, (m + 40) // 2, 40, -1): c.get_all(A + absent, size)
        c.close()
    c = Checked(e); c.set(who, vals); c.rewind(22); assert c.m.value(A[2]) == vals[20] and c.m.value(A[3]) == vals[21]; c.get_all(A)   # between two entries of one address
    for m in range(22, -1, -1): c.rewind(m); c.get_all(A + absent)                                               # and step by step down to the empty table
    c.close()

def test_fill_touches_the_old_slot_only(e):
    c = Checked(e); X, Y, Z = addr_of(1, 13), addr_of(2, 13), addr_of(3, 13); c.set([X, Y], values(2, 70))
    recs = random_records([0, 1, 7, 2, 3, 1, 2, 0], 71); froms = [X, X, X, Z, Y, Z, X, Y]
    for chained in (False, True):
        got = c.t.fill(froms, recs, chained); assert got.tobytes() == c.m.fill(froms, recs, chained).tobytes()
        for i in range(len(recs)):
            k = int(recs["kind"][i]); probe = got[i:i + 1].copy()
            if k > 3: assert got[i].tobytes() == recs[i].tobytes(); continue
            probe["args"][0][OLD_ARG[k]] = recs["args"][i][OLD_ARG[k]]; assert probe.tobytes() == recs[i].tobytes(), i
    flat = c.t.fill(froms, recs, False); ch = c.t.fill(froms, recs, True)
    assert bytes(flat["args"][1][0]) == c.m.value(X) and bytes(ch["args"][1][0]) == bytes(recs["args"][0][2]) and bytes(ch["args"][6][2]) == bytes(recs["args"][1][3])   # X: mint -> send -> (kind 7 skipped) -> deposit
    assert bytes(ch["args"][3][2]) == ZERO and bytes(ch["args"][5][0]) == bytes(recs["args"][3][4]) and bytes(flat["args"][5][0]) == ZERO                              # Z is absent: zero, then its own deposit
    c.close()

def test_host_finish_beyond_the_chain_cap(e):
    """with a cap of 4 list steps the all-equal and the 3-address batches go to the host's predecessor search and give the same bytes; the launch counters show the
    road; with the default cap distinct addresses never do"""
    for mix in ("equal", "three"):
        c = Checked(e, 12, 21); c.t.chain_cap(4)                                                                 # (2^12 slots: no rebuild among the launches counted below)
        for n in (2, 63, 257):
            a = senders(mix, n, 3); recs = random_records(np.arange(n) % 4, 81 + n); (l0, h0) = e.accts_launches(); c.set(a, values(n, n)); (l1, h1) = e.accts_launches()
            assert (l1 - l0, h1 - h0) == ((3, 0) if n == 2 else (4, 1)), (mix, n, l1 - l0, h1 - h0)             # the third launch twice
            c.fill_both(a, recs); (l2, h2) = e.accts_launches(); assert h2 - h1 == (0 if n == 2 else 1) and l2 - l1 == 1 + (3 if n == 2 else 4)   # one flat fill, one chained
            c.commit(a, recs); c.get_all(sorted(set(a)))
        c.t.chain_cap(0); a = senders(mix, 257, 4); (l0, h0) = e.accts_launches(); c.set(a, values(257, 9)); (l1, h1) = e.accts_launches()
        assert h1 == h0 if mix == "three" else h1 == h0 + 1; c.close()                                           # default cap 256: 257 equal addresses are one step too many
    c = Checked(e)
    for n in SIZES[1:]:
        (l0, h0) = e.accts_launches(); c.set(senders("distinct", n, 5), values(n, n)); assert e.accts_launches()[1] == h0
    c.close()

def test_bad_arguments_change_nothing(e):
    c = Checked(e, 4, 3); A = [addr_of(i, 14) for i in range(5)]; c.set(A + A[:1] + [addr_of(9, 14)], values(7, 90)); c.rewind(6)   # (the last address goes: one tombstone)
    L = e.lib(); h = ctypes.c_void_p(c.t.h); ARG = -2; out = ctypes.create_string_buffer(b"\x07" * 64, 64); recs = random_records([0, 1], 91); keep = recs.tobytes(); ptr = recs.ctypes.data_as(ctypes.c_void_p)
    before = (c.t.read_log(), c.t.slots()[0].copy(), c.t.slots()[2]); ab = b"".join(A[:2])
    assert L.zkgpu_accts_set(h, None, bytes(64), ctypes.c_size_t(2)) == ARG and L.zkgpu_accts_set(h, ab, None, ctypes.c_size_t(2)) == ARG
    assert L.zkgpu_accts_get(h, None, ctypes.c_size_t(2), ctypes.c_int64(-1), out) == ARG and L.zkgpu_accts_get(h, ab, ctypes.c_size_t(2), ctypes.c_int64(-1), None) == ARG
    assert L.zkgpu_accts_get(h, ab, ctypes.c_size_t(2), ctypes.c_int64(7), out) == ARG and L.zkgpu_accts_get(h, ab, ctypes.c_size_t(2), ctypes.c_int64(-2), out) == ARG and out.raw == b"\x07" * 64
    assert L.zkgpu_accts_fill(h, None, ptr, ctypes.c_size_t(2), 1) == ARG and L.zkgpu_accts_fill(h, ab, None, ctypes.c_size_t(2), 0) == ARG and recs.tobytes() == keep
    assert L.zkgpu_accts_commit_chain(h, None, ptr, ctypes.c_size_t(2)) == ARG and L.zkgpu_accts_commit_chain(h, ab, None, ctypes.c_size_t(2)) == ARG
    assert L.zkgpu_accts_rewind(h, ctypes.c_uint64(7)) == ARG and L.zkgpu_accts_read_log(h, ctypes.c_uint64(5), ctypes.c_uint64(2), out) == ARG and L.zkgpu_accts_read_log(h, ctypes.c_uint64(0), ctypes.c_uint64(1), None) == ARG
    assert L.zkgpu_accts_size(h, None) == ARG and L.zkgpu_accts_set(None, ab, bytes(64), ctypes.c_size_t(2)) == ARG
    after = (c.t.read_log(), c.t.slots()[0], c.t.slots()[2]); assert after[0] == before[0] and np.array_equal(after[1], before[1]) and after[2] == before[2] == 1
    assert L.zkgpu_accts_set(h, None, None, ctypes.c_size_t(0)) == 0 and L.zkgpu_accts_get(h, None, ctypes.c_size_t(0), ctypes.c_int64(6), None) == 0 and L.zkgpu_accts_rewind(h, ctypes.c_uint64(6)) == 0
    check_table(e, c.t, c.m); c.get_all(A, 6); c.close()
    z = e.Zk(); t = z.AcctsNew(); assert t and z.AcctsSize(t) == 0 and z.AcctsSet(t, A[:2], values(2, 92)) == 0 and z.AcctsSize(t) == 2 and z.AcctsGet(t, A[:3]) == values(2, 92) + [ZERO]
    assert z.AcctsGet(t, A[:1], 3) is None and z.AcctsRewind(t, 3) == -1 and z.AcctsRewind(t, -1) == -1 and z.AcctsGet(t, A[:2], 1) == [values(2, 92)[0], ZERO] and z.AcctsRewind(t, 1) == 0 and z.AcctsSize(t) == 1
    rc, filled = z.AcctsFillRecords(t, A[:2], recs, False); assert rc == 0 and bytes(filled["args"][0][0]) == values(2, 92)[0] and bytes(filled["args"][1][0]) == ZERO; z.AcctsFree(t)
