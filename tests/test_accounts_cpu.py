"""The account table without a device (include/zk_accounts.h, DESIGN.md "Account table"): the Python model the device tests compare the kernels with — a list of
(address, value) entries; value at a size; rewind; chained and unchained fill —, the argument that "chained fill, stop at the first rejection" decides what the
reference's sequential loop decides, checked on every small block and on seeded random ones, the header and the exports, every entry in a process that sees no
device, and the host half of the predecessor search under ASan and UBSan as a program of its own (tests/accounts_finish_driver.cpp)."""
import itertools, os, random, subprocess, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)

ACCTS_ENGINE = ["zkgpu_accts_create", "zkgpu_accts_destroy", "zkgpu_accts_size", "zkgpu_accts_set", "zkgpu_accts_get", "zkgpu_accts_fill", "zkgpu_accts_commit_chain", "zkgpu_accts_rewind",
                "zkgpu_accts_read_log", "zkgpu_test_accts_create", "zkgpu_test_accts_slots", "zkgpu_test_accts_chain_cap", "zkgpu_test_accts_launches"]
ACCTS_DROPIN = ["zkAcctsNew", "zkAcctsFree", "zkAcctsSize", "zkAcctsSet", "zkAcctsGet", "zkAcctsRewind", "zkAcctsFillRecords", "verifyBlockAccounts"]
OLD_ARG = {0: 0, 1: 0, 2: 2, 3: 0}; NEW_ARG = {0: 2, 1: 3, 2: 4, 3: 2}; ZERO = bytes(32)
RECORD_DTYPE = np.dtype([("kind", "u1"), ("reserved", "u1", (7,)), ("value_s", "<u8"), ("proof", "u1", (512,)), ("args", "u1", (6, 32))])

# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------------------
class Model:
    """the table as the issue defines it: state m = the first m entries of an append-only log; nothing else"""
    def __init__(self): self.log = []
    def size(self): return len(self.log)
    def value(self, addr, size=None):
        for a, v in reversed(self.log[:len(self.log) if size is None or size < 0 else size]):
            if a == addr: return v
        return ZERO
    def prevs(self):
        """prev of every entry: log index + 1 of the previous entry with the same address, or 0"""
        last = {}; out = []
        for i, (a, _) in enumerate(self.log): out.append(last.get(a, 0)); last[a] = i + 1
        return out
    def set(self, addrs, values): self.log += [(bytes(a), bytes(v)) for a, v in zip(addrs, values)]
    def rewind(self, m): assert 0 <= m <= len(self.log); del self.log[m:]
    def fill(self, addrs, recs, chained):
        out = recs.copy(); cur = {}
        for i, a in enumerate(addrs):
            k = int(recs["kind"][i])
            if k > 3: continue
            out["args"][i][OLD_ARG[k]] = np.frombuffer(cur.get(a, self.value(a)) if chained else self.value(a), dtype=np.uint8); cur[a] = bytes(recs["args"][i][NEW_ARG[k]])
        return out
    def commit_chain(self, addrs, recs):
        for i, a in enumerate(addrs):
            k = int(recs["kind"][i])
            if k <= 3: self.log.append((bytes(a), bytes(recs["args"][i][NEW_ARG[k]])))

def random_records(kinds, seed):
    rng = np.random.RandomState(seed); recs = np.zeros(len(kinds), dtype=RECORD_DTYPE); recs["kind"] = kinds
    recs["reserved"] = rng.randint(0, 256, (len(kinds), 7)); recs["value_s"] = rng.randint(0, 1 << 62, len(kinds)); recs["proof"] = rng.randint(0, 256, (len(kinds), 512)); recs["args"] = rng.randint(0, 256, (len(kinds), 6, 32))
    return recs
def addr_of(k, salt=0): return bytes([salt, k & 255, (k >> 8) & 255]) + bytes(16) + bytes([0xA5])

def test_model_value_rewind_and_fill():
    m = Model(); A, B, C = addr_of(1), addr_of(2), addr_of(3); v = [bytes([i]) * 32 for i in range(1, 8)]
    m.set([A, B, A], v[:3]); assert m.size() == 3 and m.prevs() == [0, 0, 1]
    assert [m.value(A, s) for s in range(4)] == [ZERO, v[0], v[0], v[2]] and m.value(B) == v[1] and m.value(C) == ZERO and m.value(B, 1) == ZERO and m.value(A, -1) == v[2]
    recs = random_records([0, 1, 7, 2, 3, 1], 5); froms = [A, A, A, C, A, C]
    flat = m.fill(froms, recs, False); chained = m.fill(froms, recs, True)
    for out, want in ((flat, [v[2], v[2], None, ZERO, v[2], ZERO]),
                      (chained, [v[2], bytes(recs["args"][0][2]), None, ZERO, bytes(recs["args"][1][3]), bytes(recs["args"][3][4])])):   # (the kind-7 record is no link of A's chain)
        for i, w in enumerate(want):
            k = int(recs["kind"][i]); probe = out[i:i + 1].copy()
            if w is None: assert out[i].tobytes() == recs[i].tobytes(); continue
            assert bytes(out["args"][i][OLD_ARG[k]]) == w, i
            probe["args"][0][OLD_ARG[k]] = recs["args"][i][OLD_ARG[k]]; assert probe.tobytes() == recs[i].tobytes(), i      # only the old slot differs
    m.commit_chain(froms, recs); assert m.size() == 8 and m.prevs() == [0, 0, 1, 3, 4, 0, 5, 6] and m.value(A) == bytes(recs["args"][4][2]) and m.value(C) == bytes(recs["args"][5][3])
    m.rewind(4); assert m.value(A) == bytes(recs["args"][0][2]) and m.value(C) == ZERO; m.rewind(0); assert m.value(A) == ZERO

# ---- chained fill and first rejection against the reference's sequential loop -------------------------------------------------------------------------------------
# A transaction is (sender, class, new).  Its proof holds for exactly one old value: class "C" the value its sender has after the sender's earlier transactions of
# the block (the honest wallet), class "P" the sender's value before the block (a wallet that did not chain), class "N" none.
def proves(tx, pre, block_before):
    sender, cls, _ = tx
    if cls == "N": return None
    if cls == "P": return pre.get(sender, ZERO)
    earlier = [t for t in block_before if t[0] == sender]; return earlier[-1][2] if earlier else pre.get(sender, ZERO)
def reference_loop(block, pre):
    """core/state_processor.go: old := cur[from]; accept iff the proof verifies under old; cur[from] := new.  The first failure makes the block invalid: the
    state goes back.  -> (verdicts up to and including the first failure, the old of each of them, the state after)"""
    cur = dict(pre); verdicts = []; olds = []
    for i, tx in enumerate(block):
        old = cur.get(tx[0], ZERO); ok = proves(tx, pre, block[:i]) == old; verdicts.append(ok); olds.append(old)
        if not ok: return verdicts, olds, dict(pre)
        cur[tx[0]] = tx[2]
    return verdicts, olds, cur
def chained_road(block, pre):
    """verifyBlockAccounts: the chained fill, every verdict from the filled statement, cut at the first rejection"""
    chain = {}; olds = []
    for tx in block: olds.append(chain.get(tx[0], pre.get(tx[0], ZERO))); chain[tx[0]] = tx[2]
    verdicts = [proves(tx, pre, block[:i]) == olds[i] for i, tx in enumerate(block)]
    f = verdicts.index(False) if False in verdicts else len(block)
    state = dict(pre)
    if f == len(block): state.update(chain)
    return verdicts[:f + 1], olds[:f + 1], state, f, verdicts
def check_block(block, pre, seen):
    want = reference_loop(block, pre); got = chained_road(block, pre); assert got[:3] == want, (block, pre)
    f = got[3]; seen["valid" if f == len(block) else "first" if f == 0 else "later"] += 1
    if f < len(block):
        # why the records after f are "not decided": the reference, going on WITHOUT record f, may decide them otherwise than the chained statements did
        rest = block[:f] + block[f + 1:]; again = reference_loop(rest, pre)[0]
        if again[f:] and again[f:f + 1] != got[4][f + 1:f + 2]: seen["differs_after_f"] += 1
    if any(t[1] == "P" and any(u[0] == t[0] for u in block[:i]) for i, t in enumerate(block[:f + 1])): seen["stale_old"] += 1

def test_chained_fill_decides_what_the_sequential_loop_decides():
    seen = dict(valid=0, first=0, later=0, differs_after_f=0, stale_old=0); X, Y = addr_of(1), addr_of(2); pres = [{}, {X: bytes([9]) * 32}, {X: bytes([9]) * 32, Y: bytes([8]) * 32}]
    alphabet = [(s, c) for s in (X, Y) for c in "CPN"]
    for n in range(0, 5):
        for combo in itertools.product(alphabet, repeat=n):
            block = [(s, c, bytes([16 + i]) * 32) for i, (s, c) in enumerate(combo)]
            for pre in pres: check_block(block, pre, seen)
    assert sum(seen[k] for k in ("valid", "first", "later")) == 3 * sum(6 ** n for n in range(5))
    rng = random.Random(20); senders = [addr_of(k) for k in range(5)]
    for _ in range(3000):
        pre = {s: rng.getrandbits(256).to_bytes(32, "big") for s in senders if rng.random() < 0.6}
        block = [(rng.choice(senders), rng.choices("CPN", weights=[12, 2, 1])[0], rng.getrandbits(256).to_bytes(32, "big")) for _ in range(rng.randrange(1, 24))]
        check_block(block, pre, seen)
    assert all(seen.values()), seen

# ---- the header and the exports ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

def test_python_binding_uses_the_header_layout(e):
    assert e.RECORD_DTYPE == RECORD_DTYPE and e.ACCT_OLD_ARG == OLD_ARG and e.ACCT_NEW_ARG == NEW_ARG

def test_account_symbols_exported_by_libzkgpu_only(e):
    from test_abi_exports import SYMS, declared_symbols
    from test_tree_block_cpu import defined
    L = e.lib(); have = defined(e.LIB_PATH)
    for s in ACCTS_ENGINE + ACCTS_DROPIN: getattr(L, s); assert s in have, s
    assert sorted(set(declared_symbols("zk_accounts.h")) - {"uint8_t"}) == sorted(ACCTS_DROPIN)          # ("uint8_t (*addrs)[20]" reads as a call to the helper)
    for s in ACCTS_ENGINE: assert s in declared_symbols("zkgpu.h"), s
    for lib, syms in SYMS.items():                                                                         # the four thin libraries: unchanged
        assert defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)) == sorted(syms), lib

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")])
def test_accounts_header_compiles_as_c_and_cxx_when_included_twice(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_accounts.h"\n#include "zk_accounts.h"\n'
                   'int main(void) { const uint8_t froms[1][20] = {{0}}, vals[1][32] = {{0}}; uint8_t out[1][32]; unsigned char ok[1]; int32_t of[1]; long long a = 0, s = 0, t = 0; zk_block_record rec; zk_accts *x = zkAcctsNew();\n'
                   '  rec.kind = 0; if (x) { (void)zkAcctsSet(x, froms, vals, 1); (void)zkAcctsGet(x, froms, 1, -1, out); (void)zkAcctsFillRecords(x, froms, &rec, 1, 0); (void)zkAcctsRewind(x, 0); (void)zkAcctsSize(x);\n'
                   '    (void)verifyBlockAccounts(0, &rec, froms, 1, x, 0, 0, 0, 0, 0, ok, of, &a, &s, &t); zkAcctsFree(x); } return 0; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

NO_DEVICE = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from blockmaze_amd import engine as e
L = e.lib(); assert e.device_count() == 0
L.zkgpu_accts_create.restype = ctypes.c_void_p; L.zkgpu_test_accts_create.restype = ctypes.c_void_p; L.zkAcctsNew.restype = ctypes.c_void_p; L.zkAcctsSize.restype = ctypes.c_longlong
NO_DEVICE = -1
assert L.zkgpu_accts_create() is None and b"no HIP device" in L.zkgpu_last_error() and L.zkgpu_test_accts_create(4, ctypes.c_uint64(1)) is None and L.zkAcctsNew() is None
try: e.AccountTable(); raise SystemExit("a table without a device")
except e.ZkGpuError: pass
n64 = ctypes.c_uint64(7); addrs = bytes(40); vals = bytes(64); out = ctypes.create_string_buffer(b"\x07" * 64, 64); recs = np.zeros(2, dtype=e.RECORD_DTYPE); recs["args"] = 3; keep = recs.tobytes(); ptr = recs.ctypes.data_as(ctypes.c_void_p)
assert L.zkgpu_accts_size(None, ctypes.byref(n64)) == NO_DEVICE and n64.value == 7
assert L.zkgpu_accts_set(None, addrs, vals, ctypes.c_size_t(2)) == NO_DEVICE and L.zkgpu_accts_get(None, addrs, ctypes.c_size_t(2), ctypes.c_int64(-1), out) == NO_DEVICE and out.raw == b"\x07" * 64
assert L.zkgpu_accts_fill(None, addrs, ptr, ctypes.c_size_t(2), 1) == NO_DEVICE and L.zkgpu_accts_commit_chain(None, addrs, ptr, ctypes.c_size_t(2)) == NO_DEVICE and recs.tobytes() == keep
assert L.zkgpu_accts_rewind(None, ctypes.c_uint64(0)) == NO_DEVICE and L.zkgpu_accts_read_log(None, ctypes.c_uint64(0), ctypes.c_uint64(0), None) == NO_DEVICE
assert L.zkgpu_test_accts_slots(None, None, ctypes.byref(n64), ctypes.byref(n64), ctypes.byref(n64)) == NO_DEVICE and L.zkgpu_test_accts_chain_cap(None, 4) == NO_DEVICE
assert L.zkgpu_test_accts_launches(ctypes.byref(n64), ctypes.byref(n64)) == NO_DEVICE and b"no HIP device" in L.zkgpu_last_error()
L.zkgpu_accts_destroy(None); L.zkAcctsFree(None)
z = e.Zk(); assert z.AcctsSize(None) == -1 and z.AcctsSet(None, [bytes(20)], [bytes(32)]) == -1 and z.AcctsGet(None, [bytes(20)]) is None and z.AcctsRewind(None, 0) == -1
rc, filled = z.AcctsFillRecords(None, [bytes(20)] * 2, recs, True); assert rc == -1 and filled.tobytes() == keep
got = z.VerifyBlockAccounts(None, recs, [bytes(20)] * 2, None, None, None, None, True); assert got[:3] == (-1, [False, False], [-1, -1]) and got[3].tobytes() == keep and got[4:] == (None, None, None), got
print("NO DEVICE OK")
"""

def test_entries_without_a_device(e, tmp_path):
    """a process that sees no device: no table can be made, every entry answers ZKGPU_ERR_NO_DEVICE (the drop-in level -1) and writes nothing"""
    script = tmp_path / "no_device.py"; script.write_text(NO_DEVICE); keys = tmp_path / "keys"; keys.mkdir()
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ZK_PRFKEY_DIR=str(keys)))
    assert r.returncode == 0 and "NO DEVICE OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])

def test_host_predecessor_search_under_sanitizers(tmp_path):
    """acct_pred_host (the search a batch beyond the chain cap takes) as a program of its own under ASan + UBSan, on seeded batches against the O(n^2) search"""
    exe = str(tmp_path / "accounts_finish_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "blockmaze_amd", "csrc"), os.path.join(ROOT, "tests", "accounts_finish_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ACCOUNTS FINISH OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])

def test_bench_host_comparand_agrees_with_the_model(tmp_path):
    """tools/accounts_host.cpp — the unordered_map loop that tools/accounts_bench.py times the device against — built here and compared with the model: the chained
    fill and the commit of a block in one pass, the journal's size, and the rewind"""
    import ctypes
    so = str(tmp_path / "accounts_host.so"); subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "accounts_host.cpp"), "-o", so])
    H = ctypes.CDLL(so); H.accounts_host_new.restype = ctypes.c_void_p; H.accounts_host_size.restype = ctypes.c_uint64; h = ctypes.c_void_p(H.accounts_host_new()); m = Model()
    A = [addr_of(i, 30) for i in range(6)]; vals = [bytes([i + 1]) * 32 for i in range(8)]; first = A[:5] + A[:3]
    H.accounts_host_set(h, b"".join(first), b"".join(vals), ctypes.c_size_t(8)); m.set(first, vals); assert H.accounts_host_size(h) == 8
    rng = random.Random(31); kinds = [rng.choice([0, 1, 2, 3, 7]) for _ in range(200)]; froms = [rng.choice(A) for _ in kinds]; recs = random_records(kinds, 32)
    for _ in range(2):                                                                                    # twice: the second time after the rewind
        got = recs.copy(); H.accounts_host_block(h, b"".join(froms), got.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(kinds))); want = m.fill(froms, recs, True)
        assert got.tobytes() == want.tobytes() and H.accounts_host_size(h) == 8 + sum(k <= 3 for k in kinds)
        H.accounts_host_rewind(h, ctypes.c_uint64(8)); assert H.accounts_host_size(h) == 8
    H.accounts_host_rewind(h, ctypes.c_uint64(5)); m.rewind(5); one = random_records([0] * 6, 33); got = one.copy()
    H.accounts_host_block(h, b"".join(A), got.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(6)); assert got.tobytes() == m.fill(A, one, True).tobytes()   # the values of state 5; A[5] absent: zero
    H.accounts_host_free(h)
