"""Records from the block bodies' bytes without a device (include/zk_bodies.h): the model (tests/bodies_model.py) against a pin of the record layout
that is not its own reading — engine.records_from_items on the item zktx.go builds from the decoded fields —, the deposit rule and every mutator of
tests/bodies_corpus.py held to the verdict it claims, chain_bodies run exhaustively over a toy oracle, the header, the exports, and both entries in a process that
sees no device."""
import itertools, os, random, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import secp_model as sm
import tx_model as t
import tx_corpus as c
import bodies_model as bm
import bodies_corpus as bc

DROPIN = ["verifyChainBodies", "zkTxRecords"]
ENGINE = ["zkgpu_tx_records", "zkgpu_test_bodies_gather"]

def item_of(tx, pk):
    """the verify call of zktx.go for a decoded transaction, as Zk.VerifyBlock takes it: (kind, proof, args in the symbol's order, value_s); old = 32 zero bytes"""
    code = tx["Code"]; proof = bytes(tx["ZKProof"]); old = bytes(32)
    if code == 1: return ("mint", proof, [old, tx["ZKSN"], tx["ZKCMT"]], tx["ZKValue"])                          # zktx.go:122-133: verifyMintproof(proof, cmtA_old, sn_old, cmtA, value_s)
    if code == 5: return ("redeem", proof, [old, tx["ZKSN"], tx["ZKCMT"]], tx["ZKValue"])                        # :198-210
    if code == 2: return ("send", proof, [old, tx["ZKSN"], tx["ZKCMTS"], tx["ZKCMT"]], 0)                        # :148-160: verifySendproof(proof, cmtAold, snAold, cmtS, cmtAnew)
    return ("deposit", proof, [tx["RTcmt"], pk, old, tx["ZKSN"], tx["ZKCMT"], tx["ZKSNS"]], 0)                   # :180-194: verifyDepositproof(proof, rt, pk, cmtB, snB, cmtBnew, sns)

def test_record_layout_against_records_from_items():
    """the pin that is not the model's own reading: for every ZK code, three signers and every proof length, the model's record equals the record the engine's packer
    makes from the item in zktx.go's order; a deposit's pk is secp_model.address of the signing key, which the model has to recover from the signature"""
    from blockmaze_amd import engine as e
    rng = random.Random(41); count = 0
    for signer, chain_id in ((t.FRONTIER, 0), (t.HOMESTEAD, 3), (t.EIP155, 3)):
        for code in bc.ZK_CODES:
            for L in (bc.PROOF_LENGTHS if signer == t.EIP155 else (512,)):
                key, nonce = rng.randrange(1, 2**20), rng.randrange(1, 2**20); tx = c.rand_tx(rng, Code=code, ZKProof=bc.hexproof(rng, L))
                tx = bc.sign_deposit(tx, key, nonce) if code == 3 else t.sign_tx(tx, signer, chain_id, key, nonce); raw = t.encode(tx)
                recs, rec_froms, rec_of, froms, codes, status, txhash = bm.records([raw], signer, chain_id)
                assert status == [t.OK] and codes == [code] and rec_of == [0] and len(recs[0]) == 720, (signer, code, L, status)
                want = e.records_from_items([item_of(tx, sm.address(sm.mul(key, sm.G)))]).tobytes(); assert recs[0] == want, (signer, code, L)
                assert froms[0] == rec_froms[0] == (tx["ZKAdrress"] if code == 3 else sm.address(sm.mul(key, sm.G))) and txhash[0] == t.keccak256(raw)
                assert recs[0][1:8] == bytes(7) and recs[0][16:16 + min(L, 512)] == tx["ZKProof"][:512] and recs[0][16 + min(L, 512):528] == bytes(512 - min(L, 512)); count += 1
    assert count == 4 * (1 + 1 + 6)

def test_other_codes_are_zk_tx_senders():
    """for every code other than 3 the four outputs are tx_model.sender's, record or not; codes 0, 4 and above 5 make no record"""
    rng = random.Random(42)
    for label, raw, signer, chain_id in c.valid_cases():
        st, code, th, frm, rec = bm.one(raw, signer, chain_id)
        if code != 3 or st == t.MALFORMED: assert (st, code, th, frm) == t.sender(raw, signer, chain_id), label
        assert (rec is not None) == (st == t.OK and code in (1, 2, 3, 5)), label
    for code in (0, 4, 6, 255):
        raw = t.encode(bc.signed(rng, t.HOMESTEAD, 0, Code=code)); assert bm.one(raw, t.HOMESTEAD, 0)[0] == t.OK and bm.one(raw, t.HOMESTEAD, 0)[4] is None

def test_every_case_of_the_corpus_has_the_verdict_it_claims():
    """the deposit rule under all three call signers (the refused cases: the wrong key, X or Y of 33 bytes, a high s — also under Frontier —, V = 37, V = 0x0100, R = 0,
    R of 33 bytes, and more), X and Y of 0, 1, 31 and 32 bytes, and ZKProof of 0 .. 600 characters: each case built from an accepted one"""
    seen = {}
    for label, claim, raw, signer, chain_id in bc.deposit_cases() + bc.xy_length_cases() + bc.proof_length_cases():
        st, code, th, frm, rec = bm.one(raw, signer, chain_id); assert st == claim, (label, st); seen[label.split(" / ")[0]] = seen.get(label.split(" / ")[0], 0) + 1
        tx = t.decode(raw)[0]
        if code == 3:
            assert th == t.keccak256(raw) and frm == (tx["ZKAdrress"] if st == t.OK else bytes(20)) and (rec is None) == (st != t.OK), label
            assert t.sender(raw, signer, chain_id)[0] == t.OK                                      # zkTxSenders accepts every one of them: the rule is this header's
            if st == t.OK: assert rec[528 + 32:528 + 52] == t.keccak256(tx["X"].to_bytes(32, "big") + tx["Y"].to_bytes(32, "big"))[12:] and rec[528 + 52:528 + 64] == bytes(12)
    for rule in ("valid", "the wrong key", "X of 33 bytes", "Y of 33 bytes", "a high s", "V = 37", "V = 0x0100", "R = 0", "R of 33 bytes"): assert seen[rule] == 4, rule   # FRONTIER, HOMESTEAD, EIP155 twice
    assert seen["signed over nine fields"] == 1
    for name in "XY":
        assert seen["%s of 31 bytes, accepted" % name] == 1 and seen["%s of 32 bytes" % name] == 1 and all(seen["%s of %d bytes, refused" % (name, k)] == 1 for k in (0, 1, 31))
    for L in bc.PROOF_LENGTHS:
        for code in bc.ZK_CODES: assert seen["proof %d, code %d" % (L, code)] == 1

def test_a_high_s_is_the_same_key_under_frontier():
    """what makes the Frontier leg of the rule a rule of its own: with s -> N - s and the parity flipped, the recovery with homestead = false returns the signing key"""
    label, claim, raw, signer, chain_id = [x for x in bc.deposit_cases() if x[0].startswith("a high s") and x[3] == t.FRONTIER][0]
    tx = t.decode(raw)[0]; sig = tx["R"].to_bytes(32, "big") + tx["S"].to_bytes(32, "big") + bytes([tx["V"] - 27])
    ok, x, y, addr = sm.recover(bm.six_field_hash(tx), sig, False); assert ok and (x, y) == (tx["X"], tx["Y"]) and not sm.recover(bm.six_field_hash(tx), sig, True)[0]

def test_pool_and_alignment_builders():
    pool = bc.Pool(); recs, rec_froms, rec_of, froms, code, status, txhash = bm.records(pool.body("pzrpzrpzrzr"), pool.signer, pool.chain_id)
    assert [s != t.OK for s in status] == [ch == "r" for ch in "pzrpzrpzrzr"] and [r >= 0 for r in rec_of] == [ch == "z" for ch in "pzrpzrpzrzr"]
    assert sorted(set(status)) == [t.OK, t.MALFORMED, t.CHAIN_ID, t.SIG, bm.DEPOSIT_KEY] and set(code[i] for i in range(11) if "pzrpzrpzrzr"[i] == "p") == {0, 4}
    raws = bc.alignment_cases(); st = bm.records(raws, t.HOMESTEAD, 0); assert all(s == t.OK for s in st[5]) and len(st[0]) == len(raws) // 2

# ---- chain_bodies, exhaustively, over a toy oracle ----------------------------------------------------------------------------------------------------------------------
def test_chain_bodies_on_every_assignment_of_two_blocks_of_three():
    """every assignment of {public, zk-ok, zk-rejected, bad-status} to up to 2 blocks x up to 3 transactions.  The toy oracle is verifyChainAccounts' contract on records
    that say themselves whether they verify; the expectation is computed from the letters alone."""
    pool = bc.Pool(); raw_of = {"p": pool.public[0], "z": pool.zk[0], "x": pool.zk[1], "r": pool.refused[0]}; rejected = bm.one(pool.zk[1], pool.signer, pool.chain_id)[4]
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
    classes = {"k = B0 < n_blocks": 0, "k < B0": 0, "k = n_blocks": 0, "a block of public transactions only": 0, "m = 0": 0}; runs = 0
    blocks = [""] + ["".join(w) for L in (1, 2, 3) for w in itertools.product("pzxr", repeat=L)]
    for nb in (1, 2):
        for body in itertools.product(blocks, repeat=nb):
            letters = "".join(body); first = [0]
            for blk in body: first.append(first[-1] + len(blk))
            state["size"] = 100; k, o = bm.chain_bodies([raw_of[ch] for ch in letters], first, pool.signer, pool.chain_id, oracle, lambda: state["size"]); runs += 1
            B0 = next((b for b in range(nb) if "r" in body[b]), nb); want_k = next((b for b in range(B0) if "x" in body[b]), B0)
            m = sum(ch in "zx" for ch in letters); decided = sum(ch in "zx" for blk in body[:B0] for ch in blk)
            assert (k, o["B0"], o["n_recs"]) == (want_k, B0, m) and len(o["ok"]) == len(o["recs"]) == m and not any(o["ok"][decided:]), (body, k, o["B0"])
            assert [r >= 0 for r in o["rec_of"]] == [ch in "zx" for ch in letters] and [s != t.OK for s in o["status"]] == [ch == "r" for ch in letters]
            accepted = sum(ch in "zx" for blk in body[:want_k] for ch in blk); assert state["size"] == 100 + accepted and o["sizes"][want_k:] == [100 + accepted] * (nb - want_k)
            assert all(o["ok"][:accepted]) and len(o["sizes"]) == nb
            if want_k == B0 < nb: classes["k = B0 < n_blocks"] += 1
            if want_k < B0: classes["k < B0"] += 1
            if want_k == nb: classes["k = n_blocks"] += 1
            if any(blk and set(blk) == {"p"} for blk in body): classes["a block of public transactions only"] += 1
            if m == 0: classes["m = 0"] += 1
    assert runs == 85 + 85 * 85 and all(v > 0 for v in classes.values()), classes
    for bad_first in ([1, 2], [0, 1], [0, 2, 1, 2]):
        with pytest.raises(bm.Refused): bm.chain_bodies([raw_of["p"], raw_of["z"]], bad_first, pool.signer, pool.chain_id, oracle, lambda: 0)

# ---- the header and the exports ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

def test_bodies_symbols_exported_by_libzkgpu_only(e):
    from test_abi_exports import SYMS, declared_symbols
    from test_tree_block_cpu import defined
    L = e.lib(); have = defined(e.LIB_PATH)
    for s in DROPIN + ENGINE: getattr(L, s); assert s in have, s
    assert sorted(set(declared_symbols("zk_bodies.h")) - {"uint8_t"}) == DROPIN                    # ("uint8_t (*txhash)[32]" reads as a call to the helper)
    for s in ENGINE: assert s in declared_symbols("zkgpu.h"), s
    for lib, syms in SYMS.items():                                                                 # the four thin libraries: unchanged
        assert defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)) == sorted(syms), lib

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")])
def test_bodies_header_compiles_as_c_and_cxx_when_included_twice(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_bodies.h"\n#include "zk_bodies.h"\n#include "zk_txs.h"\n'
                   'int main(void) { const uint8_t tx[1] = {0xc0}; const uint64_t off[2] = {0, 1}; const int first[2] = {0, 1}; zk_block_record recs[1]; uint8_t rf[1][20], th[1][32], fr[1][20], code[1], st[1];\n'
                   '  unsigned char ok[1]; int32_t of[1], an[1]; long long s0[1], s1[1], s2[1]; int m = 0;\n'
                   '  if (zkTxRecords(tx, off, 1, ZK_SIGNER_EIP155, 1, recs, rf, of, th, fr, code, st) != -1) return 1;\n'
                   '  return verifyChainBodies(0, tx, off, 1, first, 1, ZK_SIGNER_FRONTIER, 0, 0, 0, 0, 0, 0, 0, recs, rf, of, th, fr, code, st, ok, an, s0, s1, s2, &m) == -1 && ZK_TX_DEPOSIT_KEY == 4 ? 0 : 1; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

NO_DEVICE = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from blockmaze_amd import engine as e
L = e.lib(); assert e.device_count() == 0
NO_DEVICE, ARG = -1, -2
txs = [b"\xc0", b"\xc1\x80"]
zeroed = lambda o: not any(np.frombuffer(a.tobytes(), dtype=np.uint8).any() for a in o.values() if a is not None)
rc, o = e.tx_records(txs, e.SIGNER_EIP155, 1); assert rc == NO_DEVICE and b"no HIP device" in L.zkgpu_last_error() and zeroed(o)      # the wrapper hands 0xA5 in: every output is zeroed
rc, o = e.tx_records(txs, e.SIGNER_HOMESTEAD, 0, want_txhash=False); assert rc == NO_DEVICE and o["txhash"] is None and zeroed(o)
# bad arguments win over the missing device
rc, o = e.tx_records(txs, 3, 1); assert rc == ARG and b"signer" in L.zkgpu_last_error() and zeroed(o)
rc, o = e.tx_records(txs, e.SIGNER_EIP155, 2**62); assert rc == ARG and b"chain id" in L.zkgpu_last_error() and zeroed(o)
assert e.tx_records(txs, e.SIGNER_EIP155, 2**62 - 1)[0] == NO_DEVICE and e.tx_records([], e.SIGNER_EIP155, 1)[0] == 0                    # n = 0 returns 0 and asks for no device
buf = lambda n: np.full(n, 0xA5, dtype=np.uint8); ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p); off = np.array([0, 1, 3], dtype=np.uint64); dec = np.array([0, 2, 1], dtype=np.uint64)
blob = buf(3); L.zkTxRecords.restype = ctypes.c_int; L.verifyChainBodies.restype = ctypes.c_int; cid = ctypes.c_uint64(1)
sizes = (1440, 40, 8, 64, 40, 2, 2)                                                                # recs, rec_froms, rec_of, txhash, froms, code, status for n = 2
outs = [buf(k) for k in sizes]
assert L.zkTxRecords(ptr(blob), ptr(off), 2, 2, cid, *[ptr(a) for a in outs]) == -1 and b"no HIP device" in L.zkgpu_last_error() and not any(a.any() for a in outs)
outs = [buf(k) for k in sizes]
assert L.zkTxRecords(ptr(blob), ptr(dec), 2, 2, cid, *[ptr(a) for a in outs]) == -1 and b"decrease" in L.zkgpu_last_error() and not any(a.any() for a in outs)
outs = [buf(k) for k in sizes]
assert L.zkTxRecords(ptr(blob), ptr(off), -1, 2, cid, *[ptr(a) for a in outs]) == -1 and all(set(a) == {0xA5} for a in outs)             # n < 0: nothing to zero
for missing in (0, 1, 2, 4, 5, 6):                                                                 # a null recs, rec_froms, rec_of, froms, code or status; a null txhash is allowed
    outs = [buf(k) for k in sizes]; args = [ptr(a) for a in outs]; args[missing] = None
    assert L.zkTxRecords(ptr(blob), ptr(off), 2, 2, cid, *args) == -1 and b"null" in L.zkgpu_last_error() and not any(a.any() for k, a in enumerate(outs) if k != missing), missing
outs = [buf(k) for k in sizes]; args = [ptr(a) for a in outs]; args[3] = None
assert L.zkTxRecords(ptr(blob), ptr(off), 2, 2, cid, *args) == -1 and b"no HIP device" in L.zkgpu_last_error()
# the chain call: every refusal of its own comes before the device, and zeroes every output (anchor_of: -1)
first = np.array([0, 1, 2], dtype=np.int32); fake = ctypes.c_void_p(8)                            # (a handle that is never followed: without a device no table or tree can exist)
def chain(n=2, first=first, nb=2, signer=2, accts=fake, tree=fake, n_prior=0, window=4, ok=True, m=True):
    outs = [buf(k) for k in sizes]; okb = buf(2); an = np.full(2, 5, dtype=np.int32); sz = [np.full(2, 5, dtype=np.int64) for _ in range(3)]; mm = ctypes.c_int(5)
    rc = L.verifyChainBodies(None, ptr(blob), ptr(off), n, ptr(first) if first is not None else None, nb, signer, cid, accts, tree, None, n_prior, window, None, *[ptr(a) for a in outs],
                             ptr(okb) if ok else None, ptr(an), *[ptr(x) for x in sz], ctypes.byref(mm) if m else None)
    assert rc == -1 and not any(a.any() for a in outs) and (not ok or not okb.any()) and list(an) == [-1, -1] and (not m or mm.value == 0), (rc, L.zkgpu_last_error())
    return L.zkgpu_last_error()
assert b"no HIP device" in chain()
assert b"signer" in chain(signer=7) and b"no tree" in chain(tree=None) and b"account table" in chain(accts=None) and b"window" in chain(window=-1) and b"prior" in chain(n_prior=1)
assert b"block_first" in chain(first=np.array([0, 1, 1], dtype=np.int32)) and b"block_first" in chain(first=np.array([1, 1, 2], dtype=np.int32)) and b"block_first" in chain(first=None)
assert b"decreases" in chain(first=np.array([0, 3, 2], dtype=np.int32)) and b"null" in chain(ok=False) and b"null" in chain(m=False) and b"negative" in chain(nb=-1)
z = e.Zk()
try: z.TxRecords(txs, e.SIGNER_EIP155, 1); raise SystemExit("no error")
except e.ZkGpuError as err: assert "no HIP device" in str(err)
recs, rec_froms, rec_of, froms, txhash, code, status = z.TxRecords([], e.SIGNER_EIP155, 1); assert len(recs) == 0 and (rec_froms, rec_of, froms, txhash, code, status) == ([], [], [], [], [], [])
rc, o = z.VerifyChainBodies(None, txs, [0, 1, 2], e.SIGNER_EIP155, 1, 8, 8, None, 4, None, fill=0xA5)
assert rc == -1 and o["n_recs"] == 0 and not any(np.frombuffer(a.tobytes(), dtype=np.uint8).any() for k, a in o["raw"].items() if k != "anchor_of") and set(o["raw"]["anchor_of"]) == {-1}
print("NO DEVICE OK")
"""

def test_bodies_entries_without_a_device(e, tmp_path):
    """a process that sees no device: both entries return -1 / ZKGPU_ERR_NO_DEVICE with every output zeroed, and every bad argument is reported before the device is asked for"""
    script = tmp_path / "no_device.py"; script.write_text(NO_DEVICE); keys = tmp_path / "keys"; keys.mkdir()
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ZK_PRFKEY_DIR=str(keys)))
    assert r.returncode == 0 and "NO DEVICE OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
