"""The account table's segment entries on the device (blockmaze_amd/csrc/gpu_accounts.hip, k_acct_probe_tiled and k_acct_pred_tiled; DESIGN.md "A stretch of the chain
with accounts"): fill_segment and commit_segment against the Python model of tests/test_accounts_cpu.py and against the older road — fill(chained = 1) and commit_chain
— on a twin table.  Compared: the logs (address, value, prev), get at past sizes, and the whole 720 bytes of every filled record; never slot positions between two
tables, because which address claims which slot is a race."""
import os, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
from test_accounts_cpu import Model, random_records, addr_of
from test_gpu_accounts import check_table, senders, values, kinds

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 2, 255, 256, 257, 512, 513, 1000]

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    engine.init(); return engine

class Twins:
    """the segment road on table t, the older road on table o, and the model"""
    def __init__(self, e, log2_slots=None, seed=0): self.e = e; self.t = e.AccountTable(log2_slots, seed); self.o = e.AccountTable(log2_slots, seed + 1); self.m = Model()
    def check(self):
        check_table(self.e, self.t, self.m); assert self.o.read_log() == self.t.read_log()
    def set(self, addrs, vals): self.t.set(addrs, vals); self.o.set(addrs, vals); self.m.set(addrs, vals); self.check()
    def rewind(self, size): self.t.rewind(size); self.o.rewind(size); self.m.rewind(size); self.check()
    def fill(self, froms, recs):
        """-> (launches, host finishes) the segment fill added; the index of t is bit for bit what it was"""
        before = self.t.slots()[0].copy(); l0, h0 = self.e.accts_launches(); got = self.t.fill_segment(froms, recs); l1, h1 = self.e.accts_launches()
        old = self.o.fill(froms, recs, True); want = self.m.fill(froms, recs, True)
        assert got.tobytes() == want.tobytes(), [i for i in range(len(recs)) if got[i].tobytes() != want[i].tobytes()][:8]
        assert old.tobytes() == want.tobytes() and np.array_equal(self.t.slots()[0], before)
        return l1 - l0, h1 - h0
    def commit(self, froms, recs):
        l0, h0 = self.e.accts_launches(); self.t.commit_segment(froms, recs); l1, h1 = self.e.accts_launches()
        self.o.commit_chain(froms, recs); self.m.commit_chain(froms, recs); self.check(); return l1 - l0, h1 - h0
    def get_all(self, addrs, size=-1): assert self.t.get(addrs, size) == [self.m.value(a, size) for a in addrs], size
    def close(self): self.t.close(); self.o.close()

@pytest.mark.parametrize("mix", ["distinct", "three", "equal"])
def test_segment_fill_and_commit_at_every_size(e, mix):
    """n = 0 .. 1000 on one growing table, once with every record taking part (kinds 0 .. 3: n is the number of lanes) and once with kind 7 mixed in: the 720 bytes of
    every filled record, the index after the fill, the log after the commit; three launches and at most one rebuild whatever n and the mix are, and no host finish"""
    c = Twins(e); absent = [addr_of(i, 251) for i in range(3)]
    for n in SIZES:
        for mixed in (False, True):
            f = senders(mix, n, 3 + int(mixed)); recs = random_records(kinds(n, 150 + n) if mixed else np.arange(n) % 4, 160 + n + int(mixed)); m = int((recs["kind"] <= 3).sum())
            was = len(c.t.slots()[0]); grows = int(2 * (c.m.size() + m) > was)                                          # the batch no longer fits half of the table: rebuilt first
            assert c.fill(f, recs) == ((3 + grows, 0) if m else (0, 0)), (n, mixed)                                      # (a fill lets its rebuilt table go again)
            assert c.commit(f, recs) == ((3 + grows, 0) if m else (0, 0)) and (len(c.t.slots()[0]) != was) == bool(grows and m), (n, mixed)
            c.get_all(sorted(set(f)) + absent)
    assert len(c.t.slots()[0]) > 1 << 10
    c.close()

def test_tile_borders(e):
    """the smallest shapes at which the tiled search can go wrong, every record taking part, so the record index is the lane: a sender at records 255 and 256 only; a
    sender in tiles 0 and 3 of a four-tile batch with nothing between; a sender whose tile-first is also its tile-last; a sender that fills a whole tile; the last
    tile partly empty.  Half of the named senders are resident before the batch, half are not."""
    c = Twins(e, 13, 77); N = [addr_of(i, 240) for i in range(8)]; c.set(N[::2], values(4, 5))
    def batch(n, named, salt):
        f = [addr_of(i, salt) for i in range(n)]                                                             # everything else: distinct senders
        for a, at in named.items():
            for i in at: f[i] = a
        return f
    shapes = [(512, {N[0]: [255, 256], N[1]: [0, 511]}),
              (1024, {N[0]: [10, 3 * 256 + 5], N[1]: [255, 768], N[2]: [0, 300, 310, 1023], N[3]: [256]}),     # N[2]: alone in tile 0 and in tile 3; N[3]: alone in the batch
              (769, {N[4]: [100] + list(range(256, 512)) + [768], N[5]: [0, 255], N[1]: [512, 767]}),          # N[4] fills tile 1; the last tile holds one record, N[4]'s
              (700, {N[6]: list(range(0, 700, 7)), N[7]: [699], N[0]: [511, 512, 698]}),
              (257, {N[2]: [256], N[3]: [0, 256 - 1]})]
    for k, (n, named) in enumerate(shapes):
        f = batch(n, named, 100 + k); recs = random_records(np.arange(n) % 4, 300 + k)
        assert c.fill(f, recs) == (3, 0) and c.commit(f, recs) == (3, 0), k
        c.get_all(N)
    log = c.t.read_log(); at = [i for i, (a, _, _) in enumerate(log) if a == N[4]]; assert len(at) == 259 and [log[i][2] for i in at[1:]] == [i + 1 for i in at[:-1]]   # N[4]'s prev chain runs through the whole tile
    c.close()

def test_small_table_rebuilds_and_shared_probe_chains(e):
    """2^4 slots: the batch forces rebuilds, addresses share probe chains, rewinds leave tombstones the probe walks over; get at every past size"""
    c = Twins(e, 4, 0x5EED5EED1234); A = [addr_of(i, 19) for i in range(40)]; rng = np.random.RandomState(8)
    c.set(A[:6], values(6, 1))
    f = A[:3] + A[6:8] + A[:2]; recs = random_records([0, 1, 2, 3, 7, 1, 0], 2); assert c.fill(f, recs) == (4, 0); assert c.commit(f, recs)[0] == 4 and len(c.t.slots()[0]) == 32   # 6 + 6 entries: 2^5
    c.rewind(8); c.rewind(4)                                                                                  # tombstones
    f = [A[4], A[0], A[4], A[9], A[1], A[0]]; recs = random_records([0, 1, 2, 3, 7, 1], 3); assert c.fill(f, recs) == (3, 0) and c.commit(f, recs) == (3, 0)
    f = [A[int(k)] for k in rng.randint(0, 40, 300)]; recs = random_records(kinds(300, 4), 5); assert c.fill(f, recs)[1] == 0 and c.commit(f, recs)[1] == 0 and len(c.t.slots()[0]) >= 512
    for size in range(0, c.m.size() + 1, 13): c.get_all(A, size)
    c.rewind(20); c.get_all(A)
    f = [A[int(k)] for k in rng.randint(0, 12, 40)]; recs = random_records(np.arange(40) % 4, 6); assert c.fill(f, recs) == (3, 0) and c.commit(f, recs) == (3, 0)
    for size in range(c.m.size() + 1): c.get_all(A[:12], size)
    c.close()

def test_one_sender_with_a_thousand_records_stays_on_the_device(e):
    """the default cap: 1,000 records of one sender are four tiles, four nodes — three launches and no host finish on the segment road, one host finish on the older
    road, and the same bytes"""
    t = e.AccountTable(12, 5); o = e.AccountTable(12, 6); m = Model(); X = addr_of(1, 230); f = [X] * 1000; recs = random_records(np.arange(1000) % 4, 400)
    for x in (t, o): x.set([X], values(1, 9))
    m.set([X], values(1, 9)); want = m.fill(f, recs, True)
    l0, h0 = e.accts_launches(); got = t.fill_segment(f, recs); l1, h1 = e.accts_launches(); old = o.fill(f, recs, True); l2, h2 = e.accts_launches()
    assert (l1 - l0, h1 - h0) == (3, 0) and (l2 - l1, h2 - h1) == (4, 1) and got.tobytes() == old.tobytes() == want.tobytes()
    l0, h0 = e.accts_launches(); t.commit_segment(f, recs); l1, h1 = e.accts_launches(); o.commit_chain(f, recs); l2, h2 = e.accts_launches(); m.commit_chain(f, recs)
    assert (l1 - l0, h1 - h0) == (3, 0) and (l2 - l1, h2 - h1) == (4, 1); check_table(e, t, m); assert t.read_log() == o.read_log(); t.close(); o.close()

def test_host_finish_beyond_the_chain_cap_on_the_segment_road(e):
    """chain_cap(2): a sender in two tiles walks two nodes and stays on the device; a sender in four tiles (n = 769) takes exactly one host finish — the third launch
    twice — and the bytes are still the model's"""
    c = Twins(e, 13, 31); c.t.chain_cap(2); X, Y = addr_of(1, 231), addr_of(2, 231)
    f = [addr_of(i, 120) for i in range(769)]; f[3] = f[4] = f[300] = X; recs = random_records(np.arange(769) % 4, 500); assert c.fill(f, recs) == (3, 0) and c.commit(f, recs) == (3, 0)
    f = [addr_of(i, 121) for i in range(769)]
    for i in (7, 8, 256, 600, 768): f[i] = Y
    recs = random_records(np.arange(769) % 4, 501); assert c.fill(f, recs) == (4, 1) and c.commit(f, recs) == (4, 1)
    f = [X] * 769; recs = random_records(np.arange(769) % 4, 502); assert c.fill(f, recs) == (4, 1) and c.commit(f, recs) == (4, 1); c.get_all([X, Y])
    c.t.chain_cap(0); assert c.fill(f, recs) == (3, 0); c.close()

def test_segment_entries_refuse_bad_arguments(e):
    import ctypes
    c = Twins(e, 4, 3); A = [addr_of(i, 24) for i in range(3)]; c.set(A, values(3, 90)); L = e.lib(); h = ctypes.c_void_p(c.t.h); ARG = -2
    recs = random_records([0, 1], 91); keep = recs.tobytes(); ptr = recs.ctypes.data_as(ctypes.c_void_p); ab = b"".join(A[:2]); before = (c.t.read_log(), c.t.slots()[0].copy())
    assert L.zkgpu_accts_fill_segment(h, None, ptr, ctypes.c_size_t(2)) == ARG and L.zkgpu_accts_fill_segment(h, ab, None, ctypes.c_size_t(2)) == ARG and L.zkgpu_accts_fill_segment(None, ab, ptr, ctypes.c_size_t(2)) == ARG
    assert L.zkgpu_accts_commit_segment(h, None, ptr, ctypes.c_size_t(2)) == ARG and L.zkgpu_accts_commit_segment(h, ab, None, ctypes.c_size_t(2)) == ARG and recs.tobytes() == keep
    assert L.zkgpu_accts_fill_segment(h, None, None, ctypes.c_size_t(0)) == 0 and L.zkgpu_accts_commit_segment(h, None, None, ctypes.c_size_t(0)) == 0
    assert c.t.read_log() == before[0] and np.array_equal(c.t.slots()[0], before[1]); c.close()
