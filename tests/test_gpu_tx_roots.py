"""Transaction trie roots on the device (include/zk_tx_roots.h) against tests/trie_model.py, byte for byte: the generic entry at every structural edge of
one-, two- and three-byte indices and at the value lengths where a header or a rate block changes, the refusals, Zk.TxRoots on bodies of mixed transactions, two threads,
poisoned allocations, the calls of zk_txs.h and zk_bodies.h before and after, and Zk.VerifyChainBodiesRoots on real proofs.  The model's hash function is
engine.keccak256 — the sponge that tests/test_gpu_txs.py holds against hashlib —, many messages a call, memoised across the tests."""
import ctypes, os, random, subprocess, sys, threading
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import secp_model as sm
import tx_model as t
import tx_corpus as c
import bodies_model as bm
import bodies_corpus as bc
import trie_model as tm
import tx_roots_model as rm

pytestmark = pytest.mark.gpu
OK, NO_DEVICE, ARG = 0, -1, -2

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    engine.init(); return engine
@pytest.fixture(scope="module")
def pool(): return bc.Pool()

_memo = {}
def hasher(e):
    """keccak_many for the model: the messages not seen before go through the device's sponge in one call"""
    def many(msgs):
        miss = sorted(set(bytes(m) for m in msgs if bytes(m) not in _memo))
        if miss: _memo.update(zip(miss, e.keccak256(miss)))
        return [_memo[bytes(m)] for m in msgs]
    return many
def growing_roots(values, sizes, many):
    """DeriveSha of values[:n] for every n of sizes (ascending): one trie of the general model, grown a value at a time, hashed at each size"""
    tr = tm.Trie(); out = {}; k = 0
    for n in sizes:
        while k < n: tr.update(t.enc_int(k), values[k]); k += 1
        out[n] = tr.hash_many(many)
    return out
def device_roots(e, lists, start=0):
    first = [0]
    for l in lists: first.append(first[-1] + len(l))
    rc, roots = e.list_trie_roots([v for l in lists for v in l], first, start=start); assert rc == OK, (rc, e.lib().zkgpu_last_error())
    return [bytes(r) for r in roots]

# ---- the generic entry --------------------------------------------------------------------------------------------------------------------------------------------------
def test_lists_of_0_to_600_values_in_one_call(e):
    """601 lists of 0 .. 600 values of 32 bytes, 180,300 values, an empty list after every tenth: 1 / 2 values, 16 / 17, 127 / 128 / 129 (index 0 gets a sibling),
    143 / 144 / 145 (the one-nibble extension under 81 ends), 255 .. 258, 271 / 272 / 273 (extensions of three and two nibbles), 511 / 512 / 513 all lie inside"""
    rng = random.Random(61); vals = [rng.randbytes(32) for _ in range(600)]; want = growing_roots(vals, range(601), hasher(e)); lists, sizes = [], []
    for n in range(601):
        lists.append(vals[:n]); sizes.append(n)
        if n % 10 == 9: lists.append([]); sizes.append(0)
    got = device_roots(e, lists); assert sum(sizes) == 180300 and len(got) == 661
    wrong = [n for n, r in zip(sizes, got) if r != want[n]]; assert not wrong, wrong[:20]
    assert want[0] == tm.EMPTY_ROOT and want[1] == hasher(e)([t.enc_list([b"\x82\x20\x80", t.enc_str(vals[0])])])[0]   # one value: the hash of the single leaf

@pytest.mark.parametrize("sizes", [(4095, 4096, 4097, 4098, 4113), (65535, 65536, 65537, 65538, 65553)])
def test_three_byte_indices(e, sizes):
    """the last two-byte index and the first three-byte ones: a new key length, and under it an extension of five nibbles"""
    rng = random.Random(sizes[0]); vals = [rng.randbytes(32) for _ in range(sizes[-1])]; want = growing_roots(vals, sizes, hasher(e))
    got = device_roots(e, [vals[:n] for n in sizes]); assert got == [want[n] for n in sizes], [n for n, r in zip(sizes, got) if r != want[n]]

LENGTHS = [32, 33] + list(range(50, 58)) + list(range(118, 141)) + list(range(250, 261))
BIG = list(range(65530, 65541))
@pytest.mark.parametrize("start", [0, 3])
def test_value_lengths(e, start):
    """20 values of each length where a list or string header changes its form (55 / 56, 255 / 256, 65,535 / 65,536) and where the leaf crosses a rate block with every
    prefix length; the blob at two alignments of its first byte"""
    rng = random.Random(62 + start); many = hasher(e)
    lists = [[rng.randbytes(L) for _ in range(20)] for L in LENGTHS] + [[rng.randbytes(L if k == 7 else 32) for k in range(20)] for L in BIG]
    got = device_roots(e, lists, start=start); want = [tm.derive_sha(l, keccak_many=many) for l in lists]
    assert got == want, [len(l[7]) for l, g, w in zip(lists, got, want) if g != w]

def test_the_recorded_block(e):
    """the one transaction of the block that core/types/block_test.go records: the TxHash of its header, through both entries"""
    v = tm.vectors(); assert device_roots(e, [[v["block_tx"]]]) == [v["block_txhash"]]

def test_refusals_and_the_ways_to_get_minus_one(e):
    L = e.lib(); vals = [bytes([k]) * 40 for k in range(5)]
    rc, roots = e.list_trie_roots(vals[:2] + [bytes(31)] + vals[2:], [0, 3, 6]); assert rc == ARG and b"under 32 bytes" in L.zkgpu_last_error() and not roots.any()
    for first in ([0, 4], [1, 5], [0, 3, 2, 5]):
        rc, roots = e.list_trie_roots(vals, first); assert rc == ARG and b"first" in L.zkgpu_last_error() and not roots.any(), first
    assert e.list_trie_roots([], [0])[0] == OK
    rc, roots = e.list_trie_roots([], [0, 0, 0]); assert rc == OK and [bytes(r) for r in roots] == [tm.EMPTY_ROOT] * 2
    blob, off = e._tx_blob(vals); first = np.array([0, 2, 5], dtype=np.int32); buf = lambda k: np.full(k, 0xA5, dtype=np.uint8); ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    dec = off.copy(); dec[1], dec[2] = off[2], off[1]; L.zkTxRoots.restype = ctypes.c_int; L.zkgpu_list_trie_roots.restype = ctypes.c_int
    def call(txs=blob, offs=off, n=5, first=first, nb=2, roots=True, defined=True):
        r, d = buf(64), buf(2); return L.zkTxRoots(ptr(txs), ptr(offs), n, ptr(first), nb, ptr(r) if roots else None, ptr(d) if defined else None), r, d
    rc, r, d = call(); assert rc == 0 and not r.any() and not d.any()                               # five strings that are no transactions: two blocks without a root, and no error
    rc, r, d = call(n=-1); assert rc == -1 and not r.any() and not d.any()
    rc, r, d = call(nb=-1); assert rc == -1 and set(r) == set(d) == {0xA5}                          # nothing to zero
    rc, r, d = call(offs=dec); assert rc == -1 and b"decrease" in L.zkgpu_last_error() and not r.any() and not d.any()
    for bad in ([0, 2, 4], [1, 2, 5], [0, 3, 2]):
        rc, r, d = call(first=np.array(bad, dtype=np.int32)); assert rc == -1 and b"first" in L.zkgpu_last_error() and not r.any() and not d.any(), bad
    for kw in (dict(txs=None), dict(offs=None), dict(first=None), dict(roots=False), dict(defined=False)):
        rc, r, d = call(**kw); assert rc == -1 and b"null" in L.zkgpu_last_error() and (not kw.get("roots", True) or not r.any()) and (not kw.get("defined", True) or not d.any()), kw
    rc, r, d = call(n=0, nb=0, first=None, offs=None, txs=None); assert rc == 0 and set(r) == set(d) == {0xA5}   # n_blocks = 0: nothing is queued or written
    rc, r, d = call(n=0, first=np.array([0, 0, 0], dtype=np.int32), txs=None); assert rc == 2 and r.tobytes() == tm.EMPTY_ROOT * 2 and list(d) == [1, 1]

# ---- the transaction form -----------------------------------------------------------------------------------------------------------------------------------------------
def test_tx_roots_on_bodies_of_mixed_transactions(e, pool):
    """public, ZK, refused-but-decodable and malformed transactions in blocks of 0 to 200: a root for every block without a malformed transaction, whatever the other
    statuses; a 0xC0 recipient hashed as 0x80; the valid corpus of zk_txs.h as one block a signer"""
    z = e.Zk(); many = hasher(e); rng = random.Random(63)
    body = pool.body("pzzp" * 10 + "r" * 4 + "z" * 130 + "prrrp" + "zp" * 100); first = [0, 40, 41, 42, 43, 44, 44, 174, 179, 379]   # the four refused ones alone; one of each among others
    roots, defined = z.TxRoots(body, first); want = rm.tx_roots(body, first, keccak_many=many); assert (roots, defined) == want
    status = bm.records(body, pool.signer, pool.chain_id)[5]; assert defined == [not any(status[i] == t.MALFORMED for i in range(first[b], first[b + 1])) for b in range(9)]
    assert defined == [True, False, True, True, True, True, True, False, True] and roots[1] == roots[7] == bytes(32) and roots[5] == tm.EMPTY_ROOT
    tx = bc.signed(rng, t.HOMESTEAD, 0, Code=2, Recipient=None); raw, fixed = t.encode(tx, nil_as_list=True), t.encode(tx)
    roots, defined = z.TxRoots([raw, fixed, pool.zk[0], raw], [0, 1, 2, 4]); assert defined == [True] * 3 and roots[0] == roots[1] == tm.derive_sha([fixed], keccak_many=many)
    assert roots[2] == tm.derive_sha([pool.zk[0], fixed], keccak_many=many) and roots[0] != device_roots(e, [[raw]])[0]                        # the generic entry takes the bytes as they are
    by = {}
    for label, raw, signer, chain_id in c.valid_cases(): by.setdefault((signer, chain_id), []).append(raw)
    blocks = [v for k, v in sorted(by.items())]; raws = [r for v in blocks for r in v]; first = [0]
    for v in blocks: first.append(first[-1] + len(v))
    assert z.TxRoots(raws, first) == rm.tx_roots(raws, first, keccak_many=many) and len(raws) >= 100
    v = tm.vectors(); rc, roots, defined = e.tx_roots([v["block_tx"]], [0, 1]); assert rc == 0 and not defined.any()   # nine fields: no transaction of this chain (txdata has 26)

def test_two_threads_get_the_answers_of_one(e, pool):
    rng = random.Random(64); lists = [[rng.randbytes(40) for _ in range(n)] for n in (300, 0, 17, 129)]; body = pool.body("zprz" * 50); first = [0, 3, 3, 120, 200]; got = [None, None]
    run = [lambda: device_roots(e, lists), lambda: [a.tobytes() for a in e.tx_roots(body, first)[1:]]]; want = [f() for f in run]
    def loop(k):
        for _ in range(3): got[k] = run[k]()
    ts = [threading.Thread(target=loop, args=(k,)) for k in range(2)]
    for th in ts: th.start()
    for th in ts: th.join()
    assert got == want

def test_the_calls_of_zk_txs_and_zk_bodies_give_the_same_bytes_before_and_after(e, pool):
    by = {}
    for label, raw, signer, chain_id in c.valid_cases(): by.setdefault((signer, chain_id), []).append(raw)
    body = pool.body("zprz" * 40)
    def snap(): return ([(k, [a.tobytes() for a in e.tx_senders(v, *k)[1].values()], [a.tobytes() for a in e.tx_signing_inputs(v, *k)[1].values()]) for k, v in sorted(by.items())],
                        [a.tobytes() for a in e.tx_records(body, pool.signer, pool.chain_id)[1].values()])
    before = snap(); rc, roots, defined = e.tx_roots(body, [0, 100, 160]); assert rc == 0 and not defined.any()
    rng = random.Random(65); device_roots(e, [[rng.randbytes(64) for _ in range(5000)]]); assert snap() == before

# ---- the residues of the workspace layouts ------------------------------------------------------------------------------------------------------------------------------
def cuts(rng, n, n_lists):
    """n_lists lists over n values, empty ones among them: n_lists + 1 entries from 0 to n, not decreasing"""
    return [0] + sorted(rng.randrange(n + 1) for _ in range(n_lists - 1)) + [n]

def test_every_residue_of_n_and_of_the_list_count(e, pool):
    """n = 1 .. 9 transactions in 1 .. 9 blocks: n mod 4 and mod 2, 65 n mod 4 and the block count mod 8 are where a region of the workspace or an output in the
    download moves by a padding (csrc/txs_layout.hpp); the other tests step n by wave and workgroup borders.  Every call of zk_txs.h, zk_bodies.h and zk_tx_roots.h
    against its model, byte for byte; verifyChainBodiesRoots on public transactions only — no record, so no proof and no key — on a fresh tree and account table: the
    one road to the records with the roots beside them."""
    from test_gpu_bodies import check
    DEPTH = 5
    z = e.Zk(); many = hasher(e); S, CID = pool.signer, pool.chain_id; rng = random.Random(67); tree = e.Tree(DEPTH); accts = e.AccountTable(); memo = {}
    def model(f, raw):                                                                               # the model decides each distinct transaction once
        if (f, raw) not in memo: memo[f, raw] = f(raw, S, CID)
        return memo[f, raw]
    for n in range(1, 10):
        body = pool.body(("zprzpzzrp" * 2)[n:2 * n]); public = pool.body("p" * n)[n % 3:] + pool.body("p" * n)[:n % 3]
        rc, o = e.tx_signing_inputs(body, S, CID); want = [model(t.signing_inputs, r) for r in body]; assert rc == sum(w["status"] == t.OK for w in want), n
        for got, key in (("txhash", "txhash"), ("sighash", "sighash"), ("sigs", "sig"), ("deposit_from", "deposit_from")): assert o[got].tobytes() == b"".join(w[key] for w in want), (n, got)
        assert list(o["code"]) == [w["code"] for w in want] and list(o["status"]) == [w["status"] for w in want], n
        rc, o = e.tx_senders(body, S, CID); want = [model(t.sender, r) for r in body]; assert rc == sum(w[0] == t.OK for w in want), n
        assert (list(o["status"]), list(o["code"]), o["txhash"].tobytes(), o["froms"].tobytes()) == ([w[0] for w in want], [w[1] for w in want], b"".join(w[2] for w in want), b"".join(w[3] for w in want)), n
        check(e, body, S, CID, n)
        recs, rec_froms, rec_of, froms, code, status, txhash = bm.records(public, S, CID); assert not recs and status == [t.OK] * n
        for n_lists in range(1, 10):
            first = cuts(rng, n, n_lists); assert z.TxRoots(body, first) == rm.tx_roots(body, first, keccak_many=many), (n, first)
            roots, defined = rm.tx_roots(public, first, keccak_many=many); assert all(defined)
            rc, o = z.VerifyChainBodiesRoots(None, public, first, roots, S, CID, accts, tree.h, None, 8, None, fill=0xA5); assert rc == n_lists, (n, first, rc, e.lib().zkgpu_last_error())
            assert (o["roots"], o["root_ok"], o["txhash"], o["froms"], o["code"], o["status"], o["n_recs"]) == (roots, [True] * n_lists, txhash, froms, code, status, 0), (n, first)
    assert tree.size() == 0 and accts.size() == 0; accts.close(); tree.close()

# ---- child-process legs -------------------------------------------------------------------------------------------------------------------------------------------------
def leg_poison(tmp):
    """every device allocation of this process starts full of 0xA5 bytes (ZK_DEBUG_POISON_ALLOC=1): what the kernels leave unwritten would show in the roots"""
    from blockmaze_amd import engine as e
    assert os.environ.get("ZK_DEBUG_POISON_ALLOC") == "1"; e.init(); pool = bc.Pool(); many = hasher(e); rng = random.Random(66)
    sizes = [0, 1, 2, 17, 128, 129, 145, 273, 0, 700]; vals = [rng.randbytes(33) for _ in range(700)]; want = growing_roots(vals, sorted(sizes), many)
    assert device_roots(e, [vals[:n] for n in sizes]) == [want[n] for n in sizes]
    body = pool.body("zpzzrpzpp" * 30); first = [0, 0, 4, 5, 200, 270]; z = e.Zk(); assert z.TxRoots(body, first) == rm.tx_roots(body, first, keccak_many=many)
    assert device_roots(e, [vals[:300], [], vals[:3]]) == [tm.derive_sha(vals[:300], keccak_many=many), tm.EMPTY_ROOT, tm.derive_sha(vals[:3], keccak_many=many)]   # a smaller call in the grown workspace

def leg_chain(tmp):
    """The segment of tests/test_gpu_bodies.py — three mint proofs, a public transaction and a code-4 transaction in two blocks, and a block of public transactions only —
    on twin states: with the headers' own roots VerifyChainBodiesRoots is VerifyChainBodies output for output; one wrong root in block 1 stops the import there; a wrong
    root behind a malformed transaction leaves B0 at the earlier block."""
    import workload as w
    from blockmaze_amd import engine as e
    from test_gpu_chain_accounts import DEPTH
    e.keygen("mint", os.path.join(tmp, "mintpk.txt"), os.path.join(tmp, "mintvk.txt"), seed=0x5EED); z = e.Zk(); rng = random.Random(23); SIGNER, CID = t.EIP155, 1337; many = hasher(e)
    def mint_of(d): p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return d, p
    mints = [mint_of(w.mint_instance(30 + i)) for i in range(3)]; keys = [rng.randrange(1, 2**24) for _ in range(3)]; senders = [sm.address(sm.mul(k, sm.G)) for k in keys]
    def mint_tx(j): d, p = mints[j]; return t.encode(t.sign_tx(c.rand_tx(rng, Code=1, ZKValue=d["value_s"], ZKSN=d["sn_old"], ZKCMT=d["cmtA"], ZKProof=p.encode()), SIGNER, CID, keys[j], rng.randrange(1, 2**24)))
    def other(code): return t.encode(bc.signed(rng, SIGNER, CID, Code=code))
    M = [mint_tx(j) for j in range(3)]; segment = [other(0), M[0], M[1], other(4), M[2], other(0), other(0)]; first = [0, 2, 5, 7]
    tree = e.Tree(DEPTH); leaves = w.deposit_instance(1, 8)["leaves"]; assert z.TreeAppend(tree.h, leaves) == 8
    def states(): a = e.AccountTable(); assert z.AcctsSet(a, senders, [d["cmtA_old"] for d, p in mints]) == 0; return a, e.SpentSet(bytes(20))
    def run(raws, first, want=None):
        a, s = states()
        if want is None: rc, o = z.VerifyChainBodies(None, raws, first, SIGNER, CID, a, tree.h, [8], 8, s.h, fill=0xA5)
        else: rc, o = z.VerifyChainBodiesRoots(None, raws, first, want, SIGNER, CID, a, tree.h, [8], 8, s.h, fill=0xA5)
        log = (a.read_log(), s.read_log(), tree.size()); a.close(); s.close(); assert z.TreeRewind(tree.h, 8) == 8
        return rc, {k: (v.tobytes() if k == "recs" else v) for k, v in o.items() if k != "raw"}, log
    right, defined = rm.tx_roots(segment, first, keccak_many=many); assert defined == [True] * 3 and len(set(right)) == 3
    # 1. the headers' own roots: verifyChainBodies, output for output, and the states' logs
    rc0, o0, log0 = run(segment, first); rc, o, log = run(segment, first, right); assert rc0 == 3 and o0["ok"] == [True] * 3
    assert (rc, log) == (rc0, log0) and all(o[k] == o0[k] for k in o0) and o["roots"] == right and o["root_ok"] == [True] * 3
    # 2. one wrong root in block 1: k = 1, the states as after block 0, every record made and those of blocks 1 and 2 not decided, every root written
    rc1, o1, log1 = run(segment[:2], [0, 2]); wrong = [right[0], right[2], right[2]]; rc, o, log = run(segment, first, wrong); assert rc1 == 1
    assert (rc, log) == (1, log1) and o["root_ok"] == [True, False, True] and o["roots"] == right and o["status"] == [t.OK] * 7 and o["n_recs"] == 3 and o["ok"] == [True, False, False]
    assert o["anchor_of"] == o1["anchor_of"] + [-1, -1] and o["accts_sizes"] == o1["accts_sizes"] * 3 and o["set_sizes"] == o1["set_sizes"] * 3 and o["tree_sizes"] == o1["tree_sizes"] * 3
    assert o["recs"][:720] == o1["recs"] and o["recs"][720:] == b"".join(bm.records(segment, SIGNER, CID)[0][1:])                               # not decided: the old slot stays zero
    # 3. a malformed transaction in block 1 and a wrong root in block 2: B0 is block 1, by status and by its missing root
    broken = segment[:3] + [segment[3][:-1]] + segment[4:]; rcb, ob, logb = run(broken, first); rc, o, log = run(broken, first, [right[0], right[1], bytes(32)])
    assert rcb == 1 and (rc, log) == (rcb, logb) and all(o[k] == ob[k] for k in ob) and o["root_ok"] == [True, False, False] and o["roots"] == [right[0], bytes(32), right[2]]
    # 4. a wrong root in block 0: nothing is imported
    rc, o, log = run(segment, first, [bytes(32)] + right[1:]); assert rc == 0 and o["root_ok"] == [False, True, True] and not any(o["ok"]) and log[2] == 8 and o["n_recs"] == 3
    tree.close()

def run_leg(name, tmp_path, **env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path), **env))
    assert r.returncode == 0 and "LEG OK " + name in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
def test_poisoned_allocations_come_out_equal(tmp_path): run_leg("poison", tmp_path, ZK_DEBUG_POISON_ALLOC="1")
def test_verify_chain_bodies_roots_on_real_proofs(tmp_path): run_leg("chain", tmp_path)

if __name__ == "__main__":
    {"poison": leg_poison, "chain": leg_chain}[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
