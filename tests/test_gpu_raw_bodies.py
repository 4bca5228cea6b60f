"""Block bodies from their bytes on the device (include/zk_raw_bodies.h) against tests/body_model.py, byte for byte on every output: block counts across
the scan's tile, empty and refused bodies at every place, each head form at each payload length, the pack at every residue, one long list, the corpus, cap, the ways to
get -1, two threads, poisoned allocations, the calls of §22-§25 before and after, and Zk.VerifyChainRawBodies against Zk.VerifyChainBodiesRoots on real proofs."""
import os, random, subprocess, sys, threading
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
import body_model as bdm
import body_corpus as bcp

pytestmark = pytest.mark.gpu
NO_DEVICE, ARG, RUNTIME, CAP = -1, -2, -3, -5

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    engine.init(); return engine
@pytest.fixture(scope="module")
def pool(): return bc.Pool()

def check(e, bodies, start=0, want=None):
    """the test entry on `bodies` against the model: k, n, block_first, body_status, tx_beg, tx_size, the packed bytes and the packed off; entries beyond n keep the fill"""
    s = want or bdm.split_all(bodies, start=start); rc, o = e.body_split(bodies, start=start, packed=True); n = s["n"]
    assert rc == s["k"], (rc, s["k"], e.lib().zkgpu_last_error())
    assert o["n_txs"] == n and list(o["block_first"]) == s["block_first"] and list(o["body_status"]) == s["body_status"]
    assert list(o["tx_beg"][:n]) == s["tx_beg"] and list(o["tx_size"][:n]) == s["tx_size"]
    assert o["packed"] == s["packed"] and list(o["packed_off"][:n + 1]) == s["off"]                  # the concatenation, and the running sum
    assert set(o["tx_beg"][n:].tobytes()) <= {0xA5} and set(o["tx_size"][n:].tobytes()) <= {0xA5} and set(o["packed_off"][n + 1:].tobytes()) <= {0xA5}
    rc2, o2 = e.body_split(bodies, start=start)                                                     # the entry without the pack: the same outputs
    assert rc2 == rc and all(o2[k].tobytes() == o[k].tobytes() for k in ("tx_beg", "tx_size", "block_first", "body_status")) and o2["n_txs"] == n
    return s

def tiny(rng, count):
    """a body of `count` elements of 1 .. 3 bytes: a lone byte, c1 xx, c2 xx xx"""
    return bdm.body([(b"\x05", b"\xc1\x07", b"\xc2\x01\x02")[rng.randrange(3)] for _ in range(count)])

# ---- counts -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [0, 1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_block_counts_across_the_lanes_and_the_scan_tile(e, nb):
    """bodies of 0 .. 3 tiny elements: 63 / 64 / 65 are a wave, 255 / 256 / 257 the scan's tile of 256, 4,097 seventeen tiles with a carry between them"""
    rng = random.Random(100 + nb); bodies = [tiny(rng, rng.randrange(4)) for _ in range(nb)]; s = check(e, bodies); assert s["k"] == nb

def test_empty_and_refused_bodies_at_every_place(e):
    """bodies without a transaction, malformed bodies and bodies with an uncle before, between and behind full ones and as the last: off[n] and block_first[n_blocks]
    are written whatever the last bodies are"""
    rng = random.Random(71); full = lambda: tiny(rng, 1 + rng.randrange(3)); empty = bdm.body([]); bad = b"\xc1\xc0"; uncle = bdm.body([b"\x05"], [b"\xc0"]); nothing = b""
    for tail in ([], [empty], [bad], [uncle], [nothing], [empty, bad, uncle, nothing], [empty] * 300):
        for lead in ([], [empty, bad], [uncle, nothing, empty]):
            bodies = lead + [full(), empty, full(), bad, uncle, full(), nothing, full()] + tail; s = check(e, bodies, start=rng.randrange(9)); assert s["n"] >= 4
    for only in ([empty], [bad], [uncle], [nothing], [bad, uncle, nothing, empty] * 70): s = check(e, only); assert s["n"] == 0 and s["off"] == [0]

def test_each_head_form_at_each_payload_length(e):
    forms = bcp.head_form_bodies(); assert len(forms) == 22
    for label, raw in forms: s = check(e, [raw]); assert s["k"] == 1, label
    check(e, [raw for _, raw in forms], start=5)

# ---- the pack -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_packed_word_holds_bytes_of_eight_bodies(e):
    """c3 c1 xx c0 in a row: every packed byte comes from another body, a packed word from eight; and between them bodies that give nothing"""
    for count in (9, 16, 17, 100):
        bodies = [bytes([0xC3, 0xC1, k & 0x7F, 0xC0]) for k in range(count)]; s = check(e, bodies); assert s["packed"] == bytes(k & 0x7F for k in range(count)) and s["tx_size"] == [1] * count
        mixed = []
        for k, b in enumerate(bodies): mixed += [b] + [b"\xc2\xc0\xc0", b"\xc1\xc0", b""][:k % 4]
        s = check(e, mixed, start=3); assert s["n"] == count

def test_every_residue_of_the_source_and_of_the_packed_base(e):
    """a body whose item-0 payload begins at each of the eight residues mod 8 of the upload, with the packed base at each residue: 64 pairs, each with payloads of 1 .. 20
    bytes so that a piece ends inside a word, at its end, and spans two source words"""
    rng = random.Random(72); seen = set()
    for src in range(8):
        for dst in range(8):
            # body A gives dst packed bytes; a filler body (refused: it gives nothing) of `pad` bytes moves body B's payload to residue src
            a = bdm.body([b"\x05"] * dst); assert len(a) == 3 + dst
            for pad in range(1, 9):
                if (len(a) + pad + 2) % 8 == src: break
            filler = bytes([0x80 + pad - 1]) + bytes(pad - 1) if pad > 1 else b"\x05"; assert len(filler) == pad and bdm.split(filler)[0] == bdm.MALFORMED
            for size in (1, 7, 8, 9, 20):
                b = bdm.body([bytes([0xC0 + size - 1]) + rng.randbytes(size - 1)]); assert len(b) == 3 + size
                s = check(e, [a, filler, b]); assert s["tx_beg"][-1] % 8 == src and s["off"][-2] % 8 == dst and s["tx_size"][-1] == size; seen.add((src, dst))
    assert len(seen) == 64
    # body_off[0] != 0: the upload starts at the first body, whatever stands before it in the caller's buffer
    bodies = [bdm.body([t.enc_str(rng.randbytes(1 + rng.randrange(40))) for _ in range(rng.randrange(5))]) for _ in range(20)]
    for start in (1, 2, 7, 8, 9, 1000): check(e, bodies, start=start)

def test_real_transactions_in_bodies(e, pool):
    """bodies of signed transactions, the zk ones of several hundred bytes: the extents are the transactions, the packed bytes their concatenation"""
    rng = random.Random(73); bodies = []; txs = []
    for b in range(40):
        blk = pool.body("".join(rng.choice("pzr") for _ in range(rng.randrange(6)))); blk = [x for x in blk if x != pool.refused[0]]; bodies.append(bdm.body(blk)); txs += blk
    s = check(e, bodies, start=4); assert s["txs"] == txs and s["k"] == 40

def test_one_body_of_32769_one_byte_elements(e):
    """every element a lone byte: the split is OK, every transaction is ZK_TX_MALFORMED (the walk's verdict, through zkgpu_tx_senders on the packed extents)"""
    rng = random.Random(74); elems = [bytes([rng.randrange(0x80)]) for _ in range(32769)]; raw = bdm.body(elems); s = check(e, [raw]); assert s["n"] == 32769 and s["tx_size"] == [1] * 32769
    rc, o = e.tx_senders(s["txs"], t.FRONTIER, 0); assert rc == 0 and set(o["status"]) == {t.MALFORMED}

# ---- the corpus ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_corpus_in_one_call_and_each_case_as_body_zero(e):
    cases = bcp.cases(); bodies = [x[2] for x in cases]; s = check(e, bodies, start=6); assert s["body_status"] == [x[1] for x in cases] and s["k"] == 3
    ok = cases[0][2]
    for label, claim, raw, n in cases:
        s = check(e, [raw, ok, raw]); assert s["body_status"] == [claim, bdm.OK, claim] and s["k"] == (3 if claim == bdm.OK else 0) and s["n"] == 3 + 2 * n, label

def test_cap(e):
    """cap = n is enough; cap = n - 1 is ZKGPU_ERR_CAP (zkBodySplit's -2): n_txs, block_first and body_status are valid and the per-transaction outputs zeroed; cap = 0
    serves bodies without transactions; Zk.BodySplit hands -2 through"""
    rng = random.Random(75); bodies = [tiny(rng, rng.randrange(4)) for _ in range(50)] + [b"\xc1\xc0"]; s = bdm.split_all(bodies); n = s["n"]; assert n > 10
    rc, o = e.body_split(bodies, cap=n, packed=True); assert rc == 50 and list(o["tx_beg"]) == s["tx_beg"] and list(o["tx_size"]) == s["tx_size"] and o["packed"] == s["packed"]
    for cap in (n - 1, 1, 0):
        for packed in (False, True):
            rc, o = e.body_split(bodies, cap=cap, packed=packed); assert rc == CAP and b"room for" in e.lib().zkgpu_last_error(), (cap, rc)
            assert o["n_txs"] == n and list(o["block_first"]) == s["block_first"] and list(o["body_status"]) == s["body_status"] and not o["tx_beg"].any() and not o["tx_size"].any()
            if packed: assert not any(o["packed"]) and not o["packed_off"].any()
    rc, o = e.body_split([bdm.body([]), b""], cap=0); assert rc == 1 and o["n_txs"] == 0 and list(o["block_first"]) == [0, 0, 0] and list(o["body_status"]) == [bdm.OK, bdm.MALFORMED]
    z = e.Zk(); k, d = z.BodySplit(bodies, cap=n - 1); assert k == -2 and d["n_txs"] == n and d["block_first"] == s["block_first"] and d["tx_beg"] == []
    k, d = z.BodySplit(bodies); assert k == 50 and (d["n_txs"], d["block_first"], d["body_status"], d["tx_beg"], d["tx_size"]) == (n, s["block_first"], s["body_status"], s["tx_beg"], s["tx_size"])
    k, d = z.BodySplit(bodies, start=11); assert d["tx_beg"] == [x + 11 for x in s["tx_beg"]]

def test_the_ways_to_get_minus_one(e):
    import ctypes
    L = e.lib(); buf = lambda n, dt=np.uint8: np.frombuffer(bytes([0xA5]) * (np.dtype(dt).itemsize * n), dtype=dt).copy(); ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    blob = np.frombuffer(b"\xc2\xc0\xc0\xc3\xc1\x05\xc0", dtype=np.uint8).copy(); off = np.array([0, 3, 7], dtype=np.uint64); dec = np.array([0, 4, 3], dtype=np.uint64); L.zkBodySplit.restype = ctypes.c_int
    def call(bodies=blob, offs=off, nb=2, cap=4, beg=True, size=True, first=True, status=True, n=True):
        tb, ts, bf, bs, nt = buf(4, np.uint64), buf(4, np.uint32), buf(3, np.int32), buf(2), ctypes.c_int(5)
        rc = L.zkBodySplit(ptr(bodies), ptr(offs), nb, cap, ptr(tb) if beg else None, ptr(ts) if size else None, ptr(bf) if first else None, ptr(bs) if status else None, ctypes.byref(nt) if n else None)
        return rc, (not beg or cap < 0 or not tb.any()) and (not size or cap < 0 or not ts.any()) and (not first or nb < 0 or not bf[:nb + 1].any()) and (not status or nb <= 0 or not bs.any()) and (not n or nt.value == 0), (list(bf), list(bs), nt.value, list(tb), list(ts))
    rc, clean, got = call(); assert rc == 2 and got == ([0, 0, 1], [0, 0], 1, [5] + [0xA5A5A5A5A5A5A5A5] * 3, [1] + [0xA5A5A5A5] * 3)
    for kw in (dict(offs=dec), dict(nb=-1), dict(cap=-1), dict(bodies=None), dict(offs=None), dict(beg=False), dict(size=False), dict(first=False), dict(status=False), dict(n=False)):
        rc, clean, got = call(**kw); assert rc == -1 and clean, (kw, got)
    rc, clean, got = call(nb=0, bodies=None, offs=None, status=False); assert rc == 0 and got[0][0] == 0 and got[2] == 0                            # nothing queued
    assert call()[0] == 2                                                                           # a refusal leaves the next call as it was

# ---- beside the other calls ---------------------------------------------------------------------------------------------------------------------------------------------
def test_two_threads_get_the_answers_of_one(e, pool):
    rng = random.Random(76); bodies = [tiny(rng, rng.randrange(4)) for _ in range(700)]; body = pool.body("zprz" * 50); first = [0, 3, 3, 120, 200]; got = [None, None]
    snap = lambda o: [o[1][k].tobytes() if hasattr(o[1][k], "tobytes") else o[1][k] for k in sorted(o[1])] + [o[0]]
    run = [lambda: snap(e.body_split(bodies, start=3, packed=True)), lambda: [a.tobytes() for a in e.tx_roots(body, first)[1:]]]; want = [f() for f in run]
    def loop(k):
        for _ in range(3): got[k] = run[k]()
    ts = [threading.Thread(target=loop, args=(k,)) for k in range(2)]
    for th in ts: th.start()
    for th in ts: th.join()
    assert got == want

def test_the_calls_of_the_sections_before_give_the_same_bytes_before_and_after(e, pool):
    """zk_txs.h, zk_bodies.h, zk_tx_roots.h and zk_headers.h around a split that grows the raw buffer and packs into the shared workspace"""
    import header_corpus as hc
    by = {}
    for label, raw, signer, chain_id in c.valid_cases(): by.setdefault((signer, chain_id), []).append(raw)
    body = pool.body("zprz" * 40); hdrs, parent, _ = hc.chain(hc.CHAIN_SEED, 9)
    def snap(): return ([(k, [a.tobytes() for a in e.tx_senders(v, *k)[1].values()], [a.tobytes() for a in e.tx_signing_inputs(v, *k)[1].values()]) for k, v in sorted(by.items())],
                        [a.tobytes() for a in e.tx_records(body, pool.signer, pool.chain_id)[1].values()], [a.tobytes() for a in e.tx_roots(body, [0, 100, 160])[1:]],
                        [a.tobytes() for a in e.headers(hdrs, hc.PERIOD, hc.CHAIN_EPOCH, hc.NOW, parent)[1].values()])
    before = snap(); rng = random.Random(77); check(e, [bdm.body(pool.body("zpz")) for _ in range(300)] + [tiny(rng, 3)] * 2000, start=1); assert snap() == before

# ---- child-process legs -------------------------------------------------------------------------------------------------------------------------------------------------
def leg_poison(tmp):
    """every device allocation of this process starts full of 0xA5 bytes (ZK_DEBUG_POISON_ALLOC=1): what the kernels leave unwritten would show in the outputs"""
    from blockmaze_amd import engine as e
    assert os.environ.get("ZK_DEBUG_POISON_ALLOC") == "1"; e.init(); rng = random.Random(78); pool = bc.Pool()
    check(e, [x[2] for x in bcp.cases()], start=2)
    bodies = [tiny(rng, rng.randrange(4)) for _ in range(600)] + [b"", b"\xc1\xc0"]; check(e, bodies)
    check(e, [bdm.body(pool.body("zp"))], start=1)                                                  # a smaller call in the grown buffers
    z = e.Zk(); tree = e.Tree(5); accts = e.AccountTable(); public = [bdm.body(pool.body("pp")), bdm.body([]), b"\xc1\xc0", bdm.body(pool.body("p"))]
    s = bdm.split_all(public); right, _ = rm.tx_roots(s["txs"], s["block_first"])
    rc, o = z.VerifyChainRawBodies(None, public, right, pool.signer, pool.chain_id, accts, tree.h, None, 8, None, fill=0xA5)
    assert rc == 2 and o["body_status"] == [0, 0, 1, 0] and o["root_ok"] == [True, True, False, True] and o["roots"] == [right[0], tm.EMPTY_ROOT, bytes(32), right[3]] and o["status"] == [t.OK] * 3
    accts.close(); tree.close()

def leg_chain(tmp):
    """The segment of tests/test_gpu_bodies.py — three mint proofs, a public transaction and a code-4 transaction in two blocks, and a block of public transactions only —
    wrapped into bodies, on twin states: VerifyChainRawBodies gives what VerifyChainBodiesRoots gives with caller-made off and block_first, output for output, and leaves
    the same three states; a malformed body 1, or an uncle in body 1, stops the import behind block 0; and tx_root of Zk.Headers serves as want_roots."""
    import workload as w
    import header_corpus as hc
    import header_model as hm
    from blockmaze_amd import engine as e
    from test_gpu_chain_accounts import DEPTH
    e.keygen("mint", os.path.join(tmp, "mintpk.txt"), os.path.join(tmp, "mintvk.txt"), seed=0x5EED); z = e.Zk(); rng = random.Random(23); SIGNER, CID = t.EIP155, 1337
    many = lambda msgs: e.keccak256([bytes(m) for m in msgs])
    def mint_of(d): p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return d, p
    mints = [mint_of(w.mint_instance(30 + i)) for i in range(3)]; keys = [rng.randrange(1, 2**24) for _ in range(3)]; senders = [sm.address(sm.mul(k, sm.G)) for k in keys]
    def mint_tx(j): d, p = mints[j]; return t.encode(t.sign_tx(c.rand_tx(rng, Code=1, ZKValue=d["value_s"], ZKSN=d["sn_old"], ZKCMT=d["cmtA"], ZKProof=p.encode()), SIGNER, CID, keys[j], rng.randrange(1, 2**24)))
    def other(code): return t.encode(bc.signed(rng, SIGNER, CID, Code=code))
    M = [mint_tx(j) for j in range(3)]; segment = [other(0), M[0], M[1], other(4), M[2], other(0), other(0)]; first = [0, 2, 5, 7]
    blocks = [segment[first[b]:first[b + 1]] for b in range(3)]; bodies = [bdm.body(blk) for blk in blocks]
    tree = e.Tree(DEPTH); leaves = w.deposit_instance(1, 8)["leaves"]; assert z.TreeAppend(tree.h, leaves) == 8
    def states(): a = e.AccountTable(); assert z.AcctsSet(a, senders, [d["cmtA_old"] for d, p in mints]) == 0; return a, e.SpentSet(bytes(20))
    def run(raws, first, want, raw_bodies=None, **kw):
        a, s = states()
        if raw_bodies is None: rc, o = z.VerifyChainBodiesRoots(None, raws, first, want, SIGNER, CID, a, tree.h, [8], 8, s.h, fill=0xA5)
        else: rc, o = z.VerifyChainRawBodies(None, raw_bodies, want, SIGNER, CID, a, tree.h, [8], 8, s.h, fill=0xA5, **kw)
        log = (a.read_log(), s.read_log(), tree.size()); sizes = None; a.close(); s.close(); assert z.TreeRewind(tree.h, 8) == 8
        return rc, {k: (v.tobytes() if k == "recs" else v) for k, v in o.items() if k != "raw"}, log, sizes
    right, defined = rm.tx_roots(segment, first, keccak_many=many); assert defined == [True] * 3 and len(set(right)) == 3
    # 1. the same k, the same outputs, the same three states; tx_beg and tx_size lead back into the bodies' bytes
    rc0, o0, log0, sz0 = run(segment, first, right); assert rc0 == 3 and o0["ok"] == [True] * 3
    for start, cap in ((0, None), (13, 7)):
        rc, o, log, sz = run(None, None, right, bodies, start=start, cap=cap); assert (rc, log, sz) == (rc0, log0, sz0) and all(o[k] == o0[k] for k in o0), [k for k in o0 if o[k] != o0[k]]
        blob = bytes(start) + b"".join(bodies); assert (o["n_txs"], o["block_first"], o["body_status"]) == (7, first, [0, 0, 0]) and [blob[b:b + s] for b, s in zip(o["tx_beg"], o["tx_size"])] == segment
    # 2. cap = n - 1: -2, n_txs set, nothing committed
    rc, o, log, sz = run(None, None, right, bodies, cap=6); a, s = states(); fresh = (a.read_log(), s.read_log(), 8); a.close(); s.close()
    assert rc == -2 and o["n_txs"] == 7 and log == fresh
    # 3. body 1 malformed, and an uncle in body 1: k = 1, the states those of the old call on block 0 alone; body 2's root is still written
    rc1, o1, log1, sz1 = run(segment[:2], [0, 2], right[:1]); assert rc1 == 1
    for bad, st in ((t.enc_list([t.enc_list(blocks[1] + [b"\x81\x05"]), b"\xc0"]), bdm.MALFORMED), (bdm.body(blocks[1], [b"\xc0"]), bdm.UNCLES)):
        rc, o, log, sz = run(None, None, right, [bodies[0], bad, bodies[2]]); kept = segment[:2] + segment[5:]
        assert (rc, log, sz) == (1, log1, sz1) and o["body_status"] == [0, st, 0] and o["block_first"] == [0, 2, 2, 4] and o["n_txs"] == 4
        assert o["root_ok"] == [True, False, True] and o["roots"] == [right[0], bytes(32), right[2]] and o["status"] == [t.OK] * 4 and o["n_recs"] == 1 and o["ok"] == [True]
        assert o["txhash"] == [t.keccak256(r) for r in kept] and o["recs"] == o1["recs"] and o["accts_sizes"] == o1["accts_sizes"] * 3 and o["tree_sizes"] == o1["tree_sizes"] * 3
    # 4. body 0 refused: nothing is imported
    rc, o, log, sz = run(None, None, right, [b"\xc1\xc0"] + bodies[1:]); assert rc == 0 and o["body_status"] == [1, 0, 0] and not any(o["ok"]) and log[2] == 8 and o["n_recs"] == 2
    # 5. the headers' tx_root as want_roots
    def headers_over(roots):
        parent = (rng.randbytes(32), 40, hc.T0); prev = parent; raws = []
        for b, root in enumerate(roots):
            h = hm.sign_header(hc.rand_header(rng, Number=41 + b, ParentHash=prev[0], Time=prev[2] + hc.PERIOD, TxHash=root), hc.KEYS[b], rng.randrange(1, sm.N)); raws.append(hm.encode(h))
            prev = (hm.header_hash(h), 41 + b, h["Time"])
        return raws, parent
    for roots, accepted in ((right, 3), ([right[0], right[2], right[2]], 1)):
        raws, parent = headers_over(roots); k, ho = z.Headers(raws, hc.PERIOD, 0, hc.NOW, parent); assert k == 3 and ho["tx_root"] == roots
        rc, o, log, sz = run(None, None, ho["tx_root"], bodies); assert rc == accepted and o["roots"] == right and o["root_ok"] == [r == g for r, g in zip(roots, right)]
    tree.close()

def run_leg(name, tmp_path, **env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path), **env))
    assert r.returncode == 0 and "LEG OK " + name in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
def test_poisoned_allocations_come_out_equal(tmp_path): run_leg("poison", tmp_path, ZK_DEBUG_POISON_ALLOC="1")
def test_verify_chain_raw_bodies_on_real_proofs(tmp_path): run_leg("chain", tmp_path)

if __name__ == "__main__":
    {"poison": leg_poison, "chain": leg_chain}[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
