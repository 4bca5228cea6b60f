"""Transaction trie roots without a device (include/zk_tx_roots.h): the model (tests/trie_model.py) against the reference's own recorded values, the
claims the kernels rest on (the sorted order of the keys, the level rules) against the general model, the 0xC0 recipient, chain_bodies_roots run exhaustively over a
toy oracle, the header, the exports, and every entry in a process that sees no device."""
import hashlib, itertools, os, random, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import tx_model as t
import tx_corpus as c
import bodies_model as bm
import bodies_corpus as bc
import trie_model as tm
import tx_roots_model as rm

DROPIN = ["verifyChainBodiesRoots", "zkTxRoots"]
ENGINE = ["zkgpu_list_trie_roots", "zkgpu_tx_roots"]
sha3 = lambda b: hashlib.sha3_256(bytes(b)).digest()             # where only the SHAPE of the trie is compared, any hash function serves; this one is fast

# ---- the four pins ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_model_reproduces_the_recorded_roots_of_the_reference():
    """emptyRoot (trie_test.go TestEmptyTrie), both roots of TestInsert — the first has embedded nodes and a branch with a value —, and the TxHash in the header of the
    block that block_test.go records, over that block's one transaction of 97 bytes"""
    v = tm.vectors(); assert tm.Trie(rm.keccak).hash() == v["empty_root"] == tm.EMPTY_ROOT == tm.derive_sha([], rm.keccak) and len(v["inserts"]) == 2
    for root, kvs in v["inserts"]:
        tr = tm.Trie(rm.keccak)
        for k, val in kvs: tr.update(k, val)
        assert tr.hash() == root and tr.hash_many(lambda ms: [rm.keccak(m) for m in ms]) == root
    assert len(v["block_tx"]) == 97 and tm.derive_sha([v["block_tx"]], rm.keccak) == v["block_txhash"] == tm.level_root([v["block_tx"]], rm.keccak)

# ---- the claims the kernels rest on -------------------------------------------------------------------------------------------------------------------------------------
def test_the_sorted_order_of_the_keys():
    """the keys rlp(0) .. rlp(n - 1) sorted as byte strings are the indices 1 .. min(n - 1, 127), then 0, then 128 .. n - 1; no key is a prefix of another"""
    keys = [t.enc_int(i) for i in range(70000)]; order = sorted(range(70000), key=lambda i: keys[i])
    assert order == tm.sorted_indices(70000) and all(not keys[order[s + 1]].startswith(keys[order[s]]) for s in range(69999))
    for n in list(range(0, 300)) + [4095, 4096, 4097, 65535, 65536, 65537, 69999]:
        assert sorted(range(n), key=lambda i: keys[i]) == tm.sorted_indices(n), n

def test_the_level_rules_give_the_root_of_the_general_trie():
    """leaves from the adjacent prefixes, a branch for every run whose first and last key share exactly d nibbles, an extension where the borders leave a gap: the root
    of trie.go's insert and the hasher for every n in 0 .. 300 (Keccak-256, memoised), and at the edges of two- and three-byte indices (a stand-in hash: shape only)"""
    rng = random.Random(24); vals = [rng.randbytes(32) for _ in range(301)]
    for n in range(301): assert tm.level_root(vals[:n], rm.keccak) == tm.derive_sha(vals[:n], rm.keccak), n
    big = [i.to_bytes(4, "big") * 8 for i in range(65553)]
    for n in (600, 4095, 4096, 4097, 4098, 4111, 4112, 4113, 65535, 65536, 65537, 65538, 65553): assert tm.level_root(big[:n], sha3) == tm.derive_sha(big[:n], sha3), n
    assert tm.derive_sha(big[:700], sha3) == tm.derive_sha(big[:700], keccak_many=lambda ms: [sha3(m) for m in ms])

def test_a_0xc0_recipient_is_hashed_as_0x80():
    """the reference re-encodes the decoded transaction (derive_sha.go:38): a nil Recipient written as an empty list comes back as an empty string"""
    rng = random.Random(25); tx = bc.signed(rng, t.HOMESTEAD, 0, Code=2, Recipient=None); raw = t.encode(tx, nil_as_list=True); fixed = t.encode(tx)
    diff = [k for k in range(len(raw)) if raw[k] != fixed[k]]; assert len(raw) == len(fixed) and len(diff) == 1 and (raw[diff[0]], fixed[diff[0]]) == (0xC0, 0x80) and tm.tx_value(raw) == fixed
    roots, defined = rm.tx_roots([raw, fixed], [0, 1, 2]); assert defined == [True, True] and roots[0] == roots[1] == tm.derive_sha([fixed], rm.keccak) != tm.derive_sha([raw], rm.keccak)

def test_a_block_with_a_malformed_transaction_has_no_root():
    pool = bc.Pool(); body = pool.body("pzrrrr"); first = [0, 2, 3, 6, 6]; roots, defined = rm.tx_roots(body, first)     # r: MALFORMED, SIG, DEPOSIT_KEY, CHAIN_ID
    assert [s for s in bm.records(body, pool.signer, pool.chain_id)[5]] == [t.OK, t.OK, t.MALFORMED, t.SIG, bm.DEPOSIT_KEY, t.CHAIN_ID]
    assert defined == [True, False, True, True] and roots[1] == bytes(32) and roots[3] == tm.EMPTY_ROOT and roots[2] == tm.derive_sha(body[3:6], rm.keccak)

# ---- chain_bodies_roots, exhaustively, over a toy oracle ----------------------------------------------------------------------------------------------------------------
def test_chain_bodies_roots_on_every_assignment_of_two_blocks_of_two():
    """every assignment of {public, zk-ok, zk-rejected, bad-status} x {root right, root wrong} to up to 2 blocks x up to 2 transactions.  The toy oracle is
    verifyChainAccounts' contract on records that say themselves whether they verify; the expectation is computed from the letters alone."""
    pool = bc.Pool(); raw_of = {"p": pool.public[0], "z": pool.zk[0], "x": pool.zk[1], "r": pool.refused[1]}; rejected = bm.one(pool.zk[1], pool.signer, pool.chain_id)[4]
    assert bm.one(raw_of["r"], pool.signer, pool.chain_id)[0] == t.SIG                              # a bad status that decodes: its block has a root all the same
    state = {"size": 100}
    def oracle(recs, rec_froms, first):
        assert len(rec_froms) == len(recs) == first[-1] and first[0] == 0
        ok = [False] * len(recs); sizes = []; k = 0; size = state["size"]; stopped = False
        for b in range(len(first) - 1):
            blk = range(first[b], first[b + 1])
            if not stopped and all(recs[j] != rejected for j in blk):
                for j in blk: ok[j] = True
                k += 1; size += len(blk)
            elif not stopped:
                stopped = True
                for j in blk:
                    if recs[j] == rejected: break
                    ok[j] = True
            sizes.append(size)
        state["size"] = size
        return k, ok, [-1] * len(recs), list(recs), sizes
    classes = {"stopped by a root": 0, "stopped by a status": 0, "root and status in one block": 0, "k < B0": 0, "k = n_blocks": 0, "a wrong root behind B0": 0, "an empty block with a wrong root": 0}; runs = 0
    blocks = [""] + ["".join(w) for L in (1, 2) for w in itertools.product("pzxr", repeat=L)]
    for nb in (1, 2):
        for body in itertools.product(blocks, repeat=nb):
            letters = "".join(body); first = [0]
            for blk in body: first.append(first[-1] + len(blk))
            raws = [raw_of[ch] for ch in letters]; right, defined = rm.tx_roots(raws, first); assert all(defined)
            for wrong in itertools.product((False, True), repeat=nb):
                want = [bytes(32) if wrong[b] else right[b] for b in range(nb)]; state["size"] = 100
                k, o = rm.chain_bodies_roots(raws, first, want, pool.signer, pool.chain_id, oracle, lambda: state["size"]); runs += 1
                by_root = next((b for b in range(nb) if wrong[b]), nb); by_status = next((b for b in range(nb) if "r" in body[b]), nb); B0 = min(by_root, by_status)
                want_k = next((b for b in range(B0) if "x" in body[b]), B0); m = sum(ch in "zx" for ch in letters); decided = sum(ch in "zx" for blk in body[:B0] for ch in blk)
                assert (k, o["B0"], o["n_recs"]) == (want_k, B0, m) and o["roots"] == right and o["root_ok"] == [not w for w in wrong] and not any(o["ok"][decided:]), (body, wrong)
                accepted = sum(ch in "zx" for blk in body[:want_k] for ch in blk); assert state["size"] == 100 + accepted and o["sizes"][want_k:] == [100 + accepted] * (nb - want_k)
                if not any(wrong):                                 # with the headers' own roots the call is verifyChainBodies
                    state["size"] = 100; k2, o2 = bm.chain_bodies(raws, first, pool.signer, pool.chain_id, oracle, lambda: state["size"])
                    assert k2 == k and all(o2[key] == o[key] for key in o2)
                if B0 < nb and by_root < by_status: classes["stopped by a root"] += 1
                if B0 < nb and by_status < by_root: classes["stopped by a status"] += 1
                if B0 < nb and by_status == by_root: classes["root and status in one block"] += 1
                if want_k < B0: classes["k < B0"] += 1
                if want_k == nb: classes["k = n_blocks"] += 1
                if any(wrong[b] for b in range(B0 + 1, nb)): classes["a wrong root behind B0"] += 1
                if any(wrong[b] and not body[b] for b in range(nb)): classes["an empty block with a wrong root"] += 1
    assert runs == 2 * 21 + 4 * 21 * 21 and all(v > 0 for v in classes.values()), classes
    # a malformed transaction: its block has no root, so no header root can be right
    raws = [raw_of["z"], pool.refused[0], raw_of["z"]]; first = [0, 1, 2, 3]; roots, defined = rm.tx_roots(raws, first); assert defined == [True, False, True]
    state["size"] = 100; k, o = rm.chain_bodies_roots(raws, first, [roots[0], bytes(32), bytes(32)], pool.signer, pool.chain_id, oracle, lambda: state["size"])
    assert (k, o["B0"], o["root_ok"]) == (1, 1, [True, False, False])
    for bad_first in ([1, 2], [0, 1], [0, 2, 1, 2]):
        with pytest.raises(bm.Refused): rm.chain_bodies_roots([raw_of["p"], raw_of["z"]], bad_first, [bytes(32)] * (len(bad_first) - 1), pool.signer, pool.chain_id, oracle, lambda: 0)
    with pytest.raises(bm.Refused): rm.chain_bodies_roots([raw_of["p"]], [0, 1], [], pool.signer, pool.chain_id, oracle, lambda: 0)

# ---- the header and the exports -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

def test_roots_symbols_exported_by_libzkgpu_only(e):
    from test_abi_exports import SYMS, declared_symbols
    from test_tree_block_cpu import defined
    L = e.lib(); have = defined(e.LIB_PATH)
    for s in DROPIN + ENGINE: getattr(L, s); assert s in have, s
    assert sorted(set(declared_symbols("zk_tx_roots.h")) - {"uint8_t"}) == DROPIN                  # ("uint8_t (*roots)[32]" reads as a call to the helper)
    for s in ENGINE: assert s in declared_symbols("zkgpu.h"), s
    for lib, syms in SYMS.items():                                                                 # the four thin libraries: unchanged
        assert defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)) == sorted(syms), lib

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")])
def test_roots_header_compiles_as_c_and_cxx_when_included_twice(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_tx_roots.h"\n#include "zk_tx_roots.h"\n'
                   'int main(void) { const uint8_t tx[1] = {0xc0}; const uint64_t off[2] = {0, 1}; const int first[2] = {0, 1}; zk_block_record recs[1]; uint8_t rf[1][20], th[1][32], fr[1][20], code[1], st[1];\n'
                   '  unsigned char ok[1], def[1], rok[1]; int32_t of[1], an[1]; long long s0[1], s1[1], s2[1]; int m = 0; uint8_t roots[1][32]; const uint8_t want[1][32] = {{0}};\n'
                   '  if (zkTxRoots(tx, off, 1, first, 1, roots, def) != -1) return 1;\n'
                   '  return verifyChainBodiesRoots(0, tx, off, 1, first, 1, ZK_SIGNER_FRONTIER, 0, 0, 0, 0, 0, 0, 0, recs, rf, of, th, fr, code, st, ok, an, s0, s1, s2, &m, want, roots, rok) == -1 ? 0 : 1; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

NO_DEVICE = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from blockmaze_amd import engine as e
L = e.lib(); assert e.device_count() == 0
NO_DEVICE, ARG = -1, -2
vals = [bytes(32), bytes(33), bytes(40)]
rc, roots = e.list_trie_roots(vals, [0, 1, 3]); assert rc == NO_DEVICE and b"no HIP device" in L.zkgpu_last_error() and roots.shape == (2, 32) and not roots.any()   # handed in full of 0xA5
# bad arguments win over the missing device
rc, roots = e.list_trie_roots([bytes(32), bytes(31)], [0, 2]); assert rc == ARG and b"under 32 bytes" in L.zkgpu_last_error() and not roots.any()
for first in ([0, 2], [1, 3], [0, 2, 1, 3]):
    rc, roots = e.list_trie_roots(vals, first); assert rc == ARG and b"first" in L.zkgpu_last_error() and not roots.any(), first
assert e.list_trie_roots([], [0])[0] == 0 and e.list_trie_roots([], [0, 0])[0] == NO_DEVICE        # n_lists = 0 asks for no device; empty lists do: there is no host path
txs = [b"\xc0", b"\xc1\x80"]
rc, roots, defined = e.tx_roots(txs, [0, 1, 2]); assert rc == NO_DEVICE and not roots.any() and not defined.any()
rc, roots, defined = e.tx_roots(txs, [0, 1, 1]); assert rc == ARG and b"first" in L.zkgpu_last_error() and not roots.any() and not defined.any()
assert e.tx_roots([], [0])[0] == 0 and e.tx_roots([], [0, 0, 0])[0] == NO_DEVICE
buf = lambda n: np.full(n, 0xA5, dtype=np.uint8); ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p); off = np.array([0, 1, 3], dtype=np.uint64); dec = np.array([0, 2, 1], dtype=np.uint64)
first = np.array([0, 1, 2], dtype=np.int32); blob = buf(3); L.zkTxRoots.restype = ctypes.c_int; L.zkgpu_list_trie_roots.restype = ctypes.c_int
def roots_call(txs=blob, offs=off, n=2, first=first, nb=2, roots=True, defined=True):
    r, d = buf(64), buf(2); p = lambda a: ptr(a) if a is not None else None
    rc = L.zkTxRoots(p(txs), p(offs), n, p(first), nb, ptr(r) if roots else None, ptr(d) if defined else None); return rc, r, d, L.zkgpu_last_error()
rc, r, d, err = roots_call(); assert rc == -1 and b"no HIP device" in err and not r.any() and not d.any()
rc, r, d, err = roots_call(offs=dec); assert rc == -1 and b"decrease" in err and not r.any() and not d.any()
rc, r, d, err = roots_call(n=-1); assert rc == -1 and b"negative" in err and not r.any() and not d.any()
rc, r, d, err = roots_call(nb=-1); assert rc == -1 and b"negative" in err and set(r) == set(d) == {0xA5}                       # nothing to zero
for kw in (dict(txs=None), dict(offs=None), dict(first=None), dict(roots=False), dict(defined=False)):
    rc, r, d, err = roots_call(**kw); assert rc == -1 and b"null" in err and (not kw.get("roots", True) or not r.any()) and (not kw.get("defined", True) or not d.any()), kw
rc, r, d, err = roots_call(n=0, first=np.array([0, 0, 0], dtype=np.int32), txs=None); assert rc == -1 and b"no HIP device" in err    # empty blocks: no bytes are needed, a device is
rc, r, d, err = roots_call(n=0, nb=0, first=None, offs=None, txs=None); assert rc == 0 and set(r) == set(d) == {0xA5}               # n_blocks = 0: nothing is queued or written
r = buf(64); assert L.zkgpu_list_trie_roots(ptr(blob), ptr(off), 2, ptr(first), 2, ptr(r)) == ARG and b"under 32 bytes" in L.zkgpu_last_error() and not r.any()
r = buf(64); assert L.zkgpu_list_trie_roots(ptr(blob), ptr(off), 2, ptr(first), 2, None) == ARG and b"null" in L.zkgpu_last_error()
# the chain call: every refusal of its own comes before the device, and zeroes every output (anchor_of: -1), the roots and root_ok included
sizes = (1440, 40, 8, 64, 40, 2, 2); fake = ctypes.c_void_p(8); cid = ctypes.c_uint64(1); L.verifyChainBodiesRoots.restype = ctypes.c_int
def chain(n=2, first=first, nb=2, signer=2, accts=fake, tree=fake, n_prior=0, window=4, ok=True, m=True, want=True, roots=True, rok=True):
    outs = [buf(k) for k in sizes]; okb = buf(2); an = np.full(2, 5, dtype=np.int32); sz = [np.full(2, 5, dtype=np.int64) for _ in range(3)]; mm = ctypes.c_int(5); w, r, k = buf(64), buf(64), buf(2)
    rc = L.verifyChainBodiesRoots(None, ptr(blob), ptr(off), n, ptr(first) if first is not None else None, nb, signer, cid, accts, tree, None, n_prior, window, None, *[ptr(a) for a in outs],
                                  ptr(okb) if ok else None, ptr(an), *[ptr(x) for x in sz], ctypes.byref(mm) if m else None, ptr(w) if want else None, ptr(r) if roots else None, ptr(k) if rok else None)
    assert rc == -1 and not any(a.any() for a in outs) and (not ok or not okb.any()) and list(an) == [-1, -1] and (not m or mm.value == 0), (rc, L.zkgpu_last_error())
    assert nb < 0 or ((not roots or not r.any()) and (not rok or not k.any())) and set(w) == {0xA5}
    return L.zkgpu_last_error()
assert b"no HIP device" in chain()
assert b"signer" in chain(signer=7) and b"no tree" in chain(tree=None) and b"account table" in chain(accts=None) and b"window" in chain(window=-1) and b"prior" in chain(n_prior=1)
assert b"block_first" in chain(first=np.array([0, 1, 1], dtype=np.int32)) and b"block_first" in chain(first=np.array([1, 1, 2], dtype=np.int32)) and b"block_first" in chain(first=None)
assert b"decreases" in chain(first=np.array([0, 3, 2], dtype=np.int32)) and b"null" in chain(ok=False) and b"null" in chain(m=False) and b"negative" in chain(nb=-1)
assert b"roots" in chain(want=False) and b"roots" in chain(roots=False) and b"roots" in chain(rok=False)
z = e.Zk()
try: z.TxRoots(txs, [0, 1, 2]); raise SystemExit("no error")
except e.ZkGpuError as err: assert "no HIP device" in str(err)
assert z.TxRoots([], [0]) == ([], [])
rc, o = z.VerifyChainBodiesRoots(None, txs, [0, 1, 2], [bytes(32)] * 2, e.SIGNER_EIP155, 1, 8, 8, None, 4, None, fill=0xA5)
assert rc == -1 and o["n_recs"] == 0 and not any(np.frombuffer(a.tobytes(), dtype=np.uint8).any() for k, a in o["raw"].items() if k != "anchor_of") and set(o["raw"]["anchor_of"]) == {-1}
# verifyChainBodies itself: as ever
rc, o = z.VerifyChainBodies(None, txs, [0, 1, 2], e.SIGNER_EIP155, 1, 8, 8, None, 4, None, fill=0xA5); assert rc == -1 and o["n_recs"] == 0 and b"no HIP device" in L.zkgpu_last_error()
print("NO DEVICE OK")
"""

def test_roots_entries_without_a_device(e, tmp_path):
    """a process that sees no device: every entry returns -1 / ZKGPU_ERR_NO_DEVICE with every output zeroed, and every bad argument is reported before the device is asked for"""
    script = tmp_path / "no_device.py"; script.write_text(NO_DEVICE); keys = tmp_path / "keys"; keys.mkdir()
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ZK_PRFKEY_DIR=str(keys)))
    assert r.returncode == 0 and "NO DEVICE OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
