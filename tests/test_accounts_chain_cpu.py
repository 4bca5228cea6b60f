"""A stretch of the chain with accounts, without a device (include/zk_accounts_chain.h, DESIGN.md "A stretch of the chain with accounts"): a Python model of the
tiled predecessor search against the brute-force definition; the argument that one chained fill over the whole segment, cut at the first rejection, decides what the
loop of verifyBlockAccounts decides; the header, the exports, and every new entry in a process that sees no device."""
import itertools, os, random, subprocess, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
from test_accounts_cpu import ZERO, addr_of, chained_road, proves

SEGMENT_ENGINE = ["zkgpu_accts_fill_segment", "zkgpu_accts_commit_segment"]
CHAIN_DROPIN = ["verifyChainAccounts"]

# ---- the tiled search ----------------------------------------------------------------------------------------------------------------------------------------------
def brute(slots):
    """acct_pred_host's definition: pred[i] = 1 + the closest j < i with the same slot, or 0; succ[i] = 1 if some j > i has the same slot"""
    n = len(slots)
    pred = [max([j + 1 for j in range(i) if slots[j] == slots[i]], default=0) for i in range(n)]
    succ = [int(any(slots[j] == slots[i] for j in range(i + 1, n))) for i in range(n)]
    return pred, succ
def host(slots):
    """acct_pred_host's own loop, for the batches too long for the quadratic search"""
    last = {}; pred = []; succ = [0] * len(slots)
    for i, a in enumerate(slots):
        l = last.get(a, 0); pred.append(l)
        if l: succ[l - 1] = 1
        last[a] = i + 1
    return pred, succ

def tiled_search(slots, T, rng):
    """k_acct_probe_tiled and k_acct_pred_tiled with a tile of T records: slots[i] is where[i].  The tile-firsts push themselves on their slot's list in an order the
    device does not fix (rng).  -> (pred, succ, the longest walk in nodes)"""
    n = len(slots); UNSET = None; pred = [UNSET] * n; succ = [UNSET] * n; tlast = [UNSET] * n; link = [UNSET] * n; heads = {}; firsts = []
    for first in range(0, n, T):                                                          # launch 1: one workgroup a tile, after its barrier
        tile = slots[first:first + T]; lanes = {}
        for t, at in enumerate(tile): lanes.setdefault(at, []).append(t)
        for t, at in enumerate(tile):
            i = first + t; mine = lanes[at]; k = mine.index(t)                            # what the lane's one pass over the tile's where words leaves it with:
            lower = mine[k - 1] + 1 if k else 0; last = mine[-1]                          # the closest lower lane of its slot (+ 1), and the highest lane of its slot
            if last != t: succ[i] = 1
            if lower: pred[i] = first + lower; continue
            pred[i] = 0; tlast[i] = first + last; firsts.append(i)
    rng.shuffle(firsts)
    for i in firsts: link[i] = heads.get(slots[i], 0); heads[slots[i]] = i + 1          # link[i] = atomicExch(&heads[slot], i + 1)
    longest = 0; stores = []
    for i in range(n):                                                                    # launch 2: pred and tlast of launch 1 are read, succ words of tile-lasts are written
        if pred[i] != 0: continue
        node = heads[slots[i]]; steps = 0; best = 0; later = 0
        while node:
            steps += 1; j = node - 1
            if j < i: best = max(best, node)
            elif j > i: later = 1
            node = link[j]
        longest = max(longest, steps); stores.append((i, tlast[best - 1] + 1 if best else 0, tlast[i], later))
    for i, p, last, later in stores:
        assert succ[last] is UNSET, (slots, T, last)                                      # the word launch 1 left alone: written once, by one lane
        pred[i] = p; succ[last] = later
    return pred, succ, longest

def check_tiled(slots, T, rng):
    pred, succ, longest = tiled_search(slots, T, rng); want = host(slots); assert (pred, succ) == want, (slots, T, pred, succ)
    if len(slots) <= 64: assert want == brute(slots)
    assert longest <= -(-len(slots) // T), (slots, T, longest)                            # a walk visits at most ceil(m / T) nodes, whatever the mix of senders
    return longest

def test_tiled_search_model_against_the_brute_force_definition():
    """The model of the two tiled launches at tile sizes 2, 3, 4 and 256: every assignment of 3 senders to up to 7 records at tiles of 2 and 3, and 2,000 seeded random
    batches.  pred and succ must be the brute-force ones, every succ word written exactly once, and no walk longer than ceil(m / T) nodes.  This test pins the model
    and needs no library: it passes on a tree without the feature."""
    rng = random.Random(7); longest = 0
    for n in range(0, 8):
        for slots in itertools.product(range(3), repeat=n):
            for T in (2, 3): longest = max(longest, check_tiled(list(slots), T, rng))
    assert longest == 4                                                                   # 7 records of one sender at T = 2: four tiles, four nodes
    for k in range(2000):
        T = (2, 3, 4, 256)[k % 4]; n = rng.randrange(0, 40 if T < 256 else 1100); senders = rng.choice([1, 2, 3, 8, max(1, n)])
        check_tiled([rng.randrange(senders) for _ in range(n)], T, rng)
    assert check_tiled([0] * 1000, 256, rng) == 4 and -(-65536 // 256) == 256                 # one sender in 1,000 records: four nodes; the default cap of 256 nodes covers 65,536 records

# ---- one fill over the segment against the loop of verifyBlockAccounts --------------------------------------------------------------------------------------------------
def loop_road(blocks, pre):
    """include/zk_accounts_chain.h's specification: test_accounts_cpu.chained_road (verifyBlockAccounts with commit = 1) block after block with the state carried over;
    the first block that is not accepted whole stops it.  -> (blocks accepted, ok of every record, the old of every decided record, the state after)"""
    state = dict(pre); ok = []; olds = []; B = len(blocks)
    for b, block in enumerate(blocks):
        verdicts, old, after, f, _ = chained_road(block, state)
        if f < len(block): ok += [True] * f + [False] * (len(block) - f); olds += old; B = b; break
        ok += [True] * f; olds += old[:f]; state = after
    ok += [False] * (sum(len(b) for b in blocks) - len(ok))
    return B, ok, olds, state

def segment_road(blocks, pre):
    """verifyChainAccounts: ONE chained fill over the whole segment, every verdict from the filled statement, the first rejection, the cut to whole blocks.  What a
    proof holds for is a fact about the proof, not about the road: `pre` of its block on the chain as the wallets saw it, every earlier block applied."""
    chain = {}; olds = []; verdicts = []; seen = dict(pre); starts = []
    for block in blocks:
        starts.append(dict(seen))
        for tx in block: seen[tx[0]] = tx[2]
    for b, block in enumerate(blocks):
        for i, tx in enumerate(block):
            olds.append(chain.get(tx[0], pre.get(tx[0], ZERO))); chain[tx[0]] = tx[2]; verdicts.append(proves(tx, starts[b], block[:i]) == olds[-1])
    first = [0]
    for block in blocks: first.append(first[-1] + len(block))
    B = len(blocks); decided = len(verdicts); ok = list(verdicts)
    if False in verdicts:
        f = verdicts.index(False); B = max(b for b in range(len(blocks)) if first[b] <= f); decided = f + 1
        ok = [i < f for i in range(len(verdicts))]
    state = dict(pre)
    for block in blocks[:B]:
        for tx in block: state[tx[0]] = tx[2]
    return B, ok, olds[:decided], state

def check_chain(blocks, pre, seen):
    want = loop_road(blocks, pre); got = segment_road(blocks, pre); assert got == want, (blocks, pre, got, want)
    B = got[0]; seen["whole" if B == len(blocks) else "first_block" if B == 0 else "later_block"] += 1
    where = {}
    for b, block in enumerate(blocks[:B]):
        for tx in block:
            if where.setdefault(tx[0], b) != b: seen["crosses_a_border"] += 1; return

def test_segment_fill_decides_what_the_loop_of_block_calls_decides():
    """Every chain of up to 3 blocks of up to 2 records over 2 senders x {C, P, N}, and 2,000 seeded random chains: return value, verdicts, the old values of every
    decided record and the state after must be the loop's.  Every outcome class must occur.  This test pins the argument of DESIGN.md and needs no library: it passes
    on a tree without the feature."""
    seen = dict(whole=0, first_block=0, later_block=0, crosses_a_border=0); X, Y = addr_of(1), addr_of(2); pre = {X: bytes([9]) * 32}
    alphabet = [(s, c) for s in (X, Y) for c in "CPN"]; shapes = [combo for k in range(3) for combo in itertools.product(alphabet, repeat=k)]; total = 0
    for nb in range(0, 4):
        for chain in itertools.product(shapes, repeat=nb):
            k = 0; blocks = []
            for combo in chain: blocks.append([(s, c, bytes([16 + k + i]) * 32) for i, (s, c) in enumerate(combo)]); k += len(combo)
            check_chain(blocks, pre, seen); total += 1
    assert total == sum(43 ** nb for nb in range(4)) and all(seen.values()), seen
    rng = random.Random(21); senders = [addr_of(k) for k in range(5)]
    for _ in range(2000):
        p = {s: rng.getrandbits(256).to_bytes(32, "big") for s in senders if rng.random() < 0.6}
        blocks = [[(rng.choice(senders), rng.choices("CPN", weights=[40, 2, 1])[0], rng.getrandbits(256).to_bytes(32, "big")) for _ in range(rng.randrange(0, 9))] for _ in range(rng.randrange(0, 7))]
        check_chain(blocks, p, seen)

# ---- the header and the exports ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

def test_chain_accounts_symbols_exported_by_libzkgpu_only(e):
    from test_abi_exports import SYMS, declared_symbols
    from test_tree_block_cpu import defined
    L = e.lib(); have = defined(e.LIB_PATH)
    for s in SEGMENT_ENGINE + CHAIN_DROPIN: getattr(L, s); assert s in have, s
    assert sorted(set(declared_symbols("zk_accounts_chain.h")) - {"uint8_t"}) == CHAIN_DROPIN            # ("uint8_t (*froms)[20]" reads as a call to the helper)
    for s in SEGMENT_ENGINE: assert s in declared_symbols("zkgpu.h"), s
    for s in CHAIN_DROPIN: assert s not in declared_symbols("zk_accounts.h") and s not in declared_symbols("zk_tree_chain.h")
    for lib, syms in SYMS.items():                                                                         # the four thin libraries: unchanged
        assert defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)) == sorted(syms), lib

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")])
def test_chain_accounts_header_compiles_as_c_and_cxx_when_included_twice(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_accounts_chain.h"\n#include "zk_accounts_chain.h"\n'
                   'int main(void) { const uint8_t froms[1][20] = {{0}}; unsigned char ok[1]; int32_t of[1]; const int first[2] = {0, 1}; const long long prior[1] = {0}; long long a[1], s[1], t[1]; zk_block_record rec;\n'
                   '  rec.kind = 0; return verifyChainAccounts(0, &rec, froms, 1, first, 1, 0, 0, prior, 1, 4, 0, ok, of, a, s, t) == -1 ? 0 : 1; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

NO_DEVICE = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from blockmaze_amd import engine as e
L = e.lib(); assert e.device_count() == 0
NO_DEVICE = -1
addrs = bytes(40); recs = np.zeros(2, dtype=e.RECORD_DTYPE); recs["args"] = 3; keep = recs.tobytes(); ptr = recs.ctypes.data_as(ctypes.c_void_p)
assert L.zkgpu_accts_fill_segment(None, addrs, ptr, ctypes.c_size_t(2)) == NO_DEVICE and b"no HIP device" in L.zkgpu_last_error()
assert L.zkgpu_accts_commit_segment(None, addrs, ptr, ctypes.c_size_t(2)) == NO_DEVICE and recs.tobytes() == keep
z = e.Zk()
got = z.VerifyChainAccounts(None, recs, [bytes(20)] * 2, [0, 1, 2], None, None, [0], 4, None)
assert got[:3] == (-1, [False, False], [-1, -1]) and got[3].tobytes() == keep and got[4:] == (None, None, None), got
# the raw call with every argument in place — the handles are never looked into before the device is asked for; they point at zeroed memory here —: the refusal is
# the missing device's, the outputs are as a failure leaves them, recs and the sizes arrays are untouched
dummy = ctypes.create_string_buffer(1 << 16); handle = ctypes.c_void_p(ctypes.addressof(dummy))
ok = (ctypes.c_ubyte * 2)(7, 7); of = (ctypes.c_int32 * 2)(7, 7); first = (ctypes.c_int * 3)(0, 1, 2); prior = (ctypes.c_longlong * 1)(0); sizes = [(ctypes.c_longlong * 2)(-7, -7) for _ in range(3)]
L.verifyChainAccounts.restype = ctypes.c_int
assert L.verifyChainAccounts(None, ptr, addrs, 2, first, 2, handle, handle, prior, 1, 4, None, ok, of, *sizes) == -1 and b"no HIP device" in L.zkgpu_last_error()
assert list(ok) == [0, 0] and list(of) == [-1, -1] and recs.tobytes() == keep and all(list(s) == [-7, -7] for s in sizes)
print("NO DEVICE OK")
"""

def test_chain_accounts_entries_without_a_device(e, tmp_path):
    """a process that sees no device: verifyChainAccounts returns -1 with every ok 0 and every anchor_of -1 and leaves recs alone; the two engine entries answer
    ZKGPU_ERR_NO_DEVICE"""
    script = tmp_path / "no_device.py"; script.write_text(NO_DEVICE); keys = tmp_path / "keys"; keys.mkdir()
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ZK_PRFKEY_DIR=str(keys)))
    assert r.returncode == 0 and "NO DEVICE OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
