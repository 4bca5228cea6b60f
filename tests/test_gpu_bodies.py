"""Records from the block bodies' bytes on the device (include/zk_bodies.h) against the model (tests/bodies_model.py), byte for byte on every output:
counts at the borders of a wave, a workgroup and the scan's tile, mixes of public, ZK and refused transactions, every start residue mod 8, the corpora of
tests/bodies_corpus.py and tests/tx_corpus.py, the untouched calls of zk_txs.h, poisoned allocations, two threads, the ways to get -1, and verifyChainBodies on real
proofs against zkTxSenders + records_from_items + verifyChainAccounts on twin states."""
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

pytestmark = pytest.mark.gpu
ARG = -2
SCAN_TILE = 256 * 128                                            # k_body_scan: 256 counts a tile, one count for 128 transactions

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    engine.init(); return engine
@pytest.fixture(scope="module")
def pool(): return bc.Pool()

def check(e, raws, signer, chain_id, label=""):
    """zkTxRecords against the model: m, recs[0 .. m), rec_froms (zero from m on), rec_of, froms, txhash, code, status"""
    rc, o = e.tx_records(raws, signer, chain_id); recs, rec_froms, rec_of, froms, code, status, txhash = bm.records(raws, signer, chain_id); n, m = len(raws), len(recs)
    assert rc == m, (label, rc, m, e.lib().zkgpu_last_error())
    assert list(o["status"]) == status and list(o["code"]) == code, (label, [(i, int(o["status"][i]), status[i]) for i in range(n) if o["status"][i] != status[i]][:5])
    assert list(o["rec_of"]) == rec_of, label
    assert o["froms"].tobytes() == b"".join(froms) and o["txhash"].tobytes() == b"".join(txhash), label
    assert o["rec_froms"].tobytes() == b"".join(rec_froms) + bytes(20 * (n - m)), label
    got = o["recs"].tobytes()
    if got[:720 * m] != b"".join(recs):
        j = next(j for j in range(m) if got[720 * j:720 * j + 720] != recs[j]); at = next(k for k in range(720) if got[720 * j + k] != recs[j][k])
        raise AssertionError((label, "record", j, "byte", at, got[720 * j + at], recs[j][at]))
    assert got[720 * m:] == b"\xa5" * (720 * (n - m)), label                                      # recs[m .. n) is left as it was
    return rc, o

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 257, SCAN_TILE + 1])
def test_counts_at_the_borders_of_a_wave_a_workgroup_and_the_scan(e, pool, n):
    pattern = ("zpzzrpzpp" * (n // 9 + 1))[:n]; rc, o = check(e, pool.body(pattern), pool.signer, pool.chain_id, n); assert rc == pattern.count("z")

MIXES = {"all public": "p" * 200, "all ZK": "z" * 200, "alternating": "pz" * 100, "one ZK after 300 public": "p" * 300 + "z", "refused first": "r" + "zp" * 70, "refused last": "zp" * 70 + "r",
         "refused at a workgroup border": "z" * 127 + "r" + "z" * 40, "refused behind a workgroup border": "z" * 128 + "r" + "z" * 40, "all refused": "r" * 130}
@pytest.mark.parametrize("name", sorted(MIXES))
def test_mixes(e, pool, name):
    pattern = MIXES[name]; rc, o = check(e, pool.body(pattern), pool.signer, pool.chain_id, name); assert rc == pattern.count("z")

def test_every_start_residue_mod_8_of_a_transaction_and_of_its_proof(e):
    raws = bc.alignment_cases(); rc, o = check(e, raws, t.HOMESTEAD, 0, "alignment"); assert rc == len(raws) // 2
    for shift in range(1, 8): check(e, [raws[0][:-shift]] + raws[1:], t.HOMESTEAD, 0, "alignment, shifted %d" % shift)       # (a malformed first transaction of every length mod 8 moves all the others)

def test_gather_bytewise_and_from_aligned_words_agree(e, pool):
    raws = bc.alignment_cases() + pool.body("zpz" * 50)[:149]
    try: e.bodies_gather_bytewise(True); check(e, raws, t.HOMESTEAD, 0, "bytewise")
    finally: e.bodies_gather_bytewise(False)
    check(e, raws, t.HOMESTEAD, 0, "aligned")

def grouped(cases):
    g = {}
    for x in cases: g.setdefault((x[3], x[4]), []).append(x)
    return g

def test_deposit_rule_xy_lengths_and_proof_lengths(e):
    cases = bc.deposit_cases() + bc.xy_length_cases() + bc.proof_length_cases(); seen = set()
    for (signer, chain_id), group in grouped(cases).items():
        rc, o = check(e, [x[2] for x in group], signer, chain_id, (signer, chain_id))
        for k, x in enumerate(group): assert int(o["status"][k]) == x[1], x[0]; seen.add(x[1])
    assert seen == {t.OK, bm.DEPOSIT_KEY}

def test_refusal_corpus_and_zk_tx_senders_agree_on_every_code_but_3(e):
    corpus = c.refusal_corpus(); z = e.Zk(); others = 0
    for (signer, chain_id), group in grouped([(x[0], x[1], x[2], x[3], x[4]) for x in corpus]).items():
        raws = [x[2] for x in group]; rc, o = check(e, raws, signer, chain_id, (signer, chain_id)); froms, txhash, code, status = z.TxSenders(raws, signer, chain_id)
        for k in range(len(raws)):
            assert int(o["code"][k]) == code[k] and bytes(o["txhash"][k]) == txhash[k]
            if code[k] != 3 or status[k] == t.MALFORMED: assert int(o["status"][k]) == status[k] and bytes(o["froms"][k]) == froms[k], group[k][0]; others += 1
            else: assert status[k] == t.OK and int(o["status"][k]) in (t.OK, bm.DEPOSIT_KEY)
    assert others >= 300

def test_the_calls_of_zk_txs_give_the_same_bytes_before_and_after(e, pool):
    by = {}
    for label, raw, signer, chain_id in c.valid_cases(): by.setdefault((signer, chain_id), []).append(raw)
    def snap(): return [(k, [a.tobytes() for a in e.tx_senders(v, *k)[1].values()], [a.tobytes() for a in e.tx_signing_inputs(v, *k)[1].values()]) for k, v in sorted(by.items())]
    before = snap(); check(e, pool.body("zprz" * 40), pool.signer, pool.chain_id, "between"); assert snap() == before

def test_two_threads_get_the_answers_of_one(e, pool):
    parts = [pool.body("zpzr" * 30), bc.alignment_cases()]; args = [(pool.signer, pool.chain_id), (t.HOMESTEAD, 0)]; got = [None, None]
    flat = lambda r: (r[0], [(k, v.tobytes()) for k, v in sorted(r[1].items())]); want = [flat(e.tx_records(parts[k], *args[k])) for k in range(2)]
    def run(k):
        for _ in range(3): got[k] = flat(e.tx_records(parts[k], *args[k]))
    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for th in ts: th.start()
    for th in ts: th.join()
    assert got == want and want[0][0] == 60 and want[1][0] == 16

def test_the_ways_to_get_minus_one(e, pool):
    L = e.lib(); raws = pool.body("zp"); zeroed = lambda o: not any(np.frombuffer(a.tobytes(), dtype=np.uint8).any() for a in o.values() if a is not None)
    rc, o = e.tx_records(raws, 3, 1); assert rc == ARG and b"signer" in L.zkgpu_last_error() and zeroed(o)
    rc, o = e.tx_records(raws, t.EIP155, 2**62); assert rc == ARG and b"chain id" in L.zkgpu_last_error() and zeroed(o)
    blob, off = e._tx_blob(raws); buf = lambda k: np.full(k, 0xA5, dtype=np.uint8); ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p); sizes = (1440, 40, 8, 64, 40, 2, 2); cid = ctypes.c_uint64(pool.chain_id)
    L.zkTxRecords.restype = ctypes.c_int; dec = off.copy(); dec[1], dec[2] = off[2], off[1]
    def call(txs=blob, offs=off, n=2, missing=None):
        outs = [buf(k) for k in sizes]; args = [ptr(a) for a in outs]
        if missing is not None: args[missing] = None
        return L.zkTxRecords(ptr(txs) if txs is not None else None, ptr(offs) if offs is not None else None, n, pool.signer, cid, *args), outs
    rc, outs = call(); assert rc == 1 and outs[0][:720].tobytes() == bm.one(raws[0], pool.signer, pool.chain_id)[4] and set(outs[0][720:]) == {0xA5}
    rc, outs = call(missing=3); assert rc == 1                                                      # a null txhash is allowed
    rc, outs = call(n=0); assert rc == 0 and all(set(a) == {0xA5} for a in outs)                    # n = 0: nothing is queued or written
    rc, outs = call(n=-1); assert rc == -1 and all(set(a) == {0xA5} for a in outs)
    rc, outs = call(offs=dec); assert rc == -1 and b"decrease" in L.zkgpu_last_error() and not any(a.any() for a in outs)
    for kw in (dict(txs=None), dict(offs=None)) + tuple(dict(missing=k) for k in (0, 1, 2, 4, 5, 6)):
        rc, outs = call(**kw); assert rc == -1 and b"null" in L.zkgpu_last_error() and not any(a.any() for k, a in enumerate(outs) if k != kw.get("missing")), kw

# ---- child-process legs -------------------------------------------------------------------------------------------------------------------------------------------------
def leg_poison(tmp):
    """every device allocation of this process starts full of 0xA5 bytes (ZK_DEBUG_POISON_ALLOC=1): what the kernels leave unwritten would show in the outputs"""
    from blockmaze_amd import engine as e
    assert os.environ.get("ZK_DEBUG_POISON_ALLOC") == "1"; e.init(); pool = bc.Pool()
    check(e, pool.body("zpzzrpzpp" * 30), pool.signer, pool.chain_id, "poison, mix"); check(e, pool.body("p" * 70), pool.signer, pool.chain_id, "poison, no record")
    for (signer, chain_id), group in grouped(bc.proof_length_cases() + bc.deposit_cases()[:13]).items(): check(e, [x[2] for x in group], signer, chain_id, "poison, proofs and deposits")
    check(e, bc.alignment_cases(), t.HOMESTEAD, 0, "poison, alignment")

def leg_chain(tmp):
    """Three mint proofs, a public transaction and a code-4 transaction in two blocks, and a block of public transactions only; every transaction is encoded and signed
    by the model.  verifyChainBodies on the bytes against zkTxSenders + records_from_items + verifyChainAccounts on twin states: the return value, verdicts, anchors,
    filled records, sizes and the logs of the table, the set and the tree's size."""
    import workload as w
    from blockmaze_amd import engine as e
    from test_gpu_chain_accounts import DEPTH
    e.keygen("mint", os.path.join(tmp, "mintpk.txt"), os.path.join(tmp, "mintvk.txt"), seed=0x5EED); z = e.Zk(); rng = random.Random(23); SIGNER, CID = t.EIP155, 1337
    def mint_of(d): p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return d, p
    mints = [mint_of(w.mint_instance(30 + i)) for i in range(3)]; keys = [rng.randrange(1, 2**24) for _ in range(3)]; senders = [sm.address(sm.mul(k, sm.G)) for k in keys]
    def mint_tx(j): d, p = mints[j]; return t.encode(t.sign_tx(c.rand_tx(rng, Code=1, ZKValue=d["value_s"], ZKSN=d["sn_old"], ZKCMT=d["cmtA"], ZKProof=p.encode()), SIGNER, CID, keys[j], rng.randrange(1, 2**24)))
    def other(code): return t.encode(bc.signed(rng, SIGNER, CID, Code=code))
    M = [mint_tx(j) for j in range(3)]; segment = [other(0), M[0], M[1], other(4), M[2], other(0), other(0)]; first = [0, 2, 5, 7]          # block 2: public transactions only
    tree = e.Tree(DEPTH); leaves = w.deposit_instance(1, 8)["leaves"]; assert z.TreeAppend(tree.h, leaves) == 8
    def states(): a = e.AccountTable(); assert z.AcctsSet(a, senders, [d["cmtA_old"] for d, p in mints]) == 0; return a, e.SpentSet(bytes(20))
    def comparand(raws, first):
        """the road of INTEGRATION.md before this header: the senders from the device, the records built on the host, the blocks [0, B0) into verifyChainAccounts"""
        froms, txhash, code, status = z.TxSenders(raws, SIGNER, CID); bad = [i for i, s in enumerate(status) if s != t.OK]; nb = len(first) - 1
        B0 = nb if not bad else next(b for b in range(nb) if first[b + 1] > bad[0]); items, rf, rec_first = [], [], [0]
        for b in range(B0):
            for i in range(first[b], first[b + 1]):
                if code[i] == 1: tx = t.decode(raws[i])[0]; items.append(("mint", tx["ZKProof"], [bytes(32), tx["ZKSN"], tx["ZKCMT"]], tx["ZKValue"])); rf.append(froms[i])
            rec_first.append(len(items))
        a, s = states(); got = z.VerifyChainAccounts(None, e.records_from_items(items), rf, rec_first, a, tree.h, [8], 8, s.h)
        out = (got[0], got[1], got[2], got[3].tobytes(), got[4], got[5], got[6], a.read_log(), s.read_log(), tree.size()); a.close(); s.close(); assert z.TreeRewind(tree.h, 8) == 8
        return B0, len(items), out
    def bodies(raws, first):
        a, s = states(); rc, o = z.VerifyChainBodies(None, raws, first, SIGNER, CID, a, tree.h, [8], 8, s.h, fill=0xA5); log = (a.read_log(), s.read_log(), tree.size()); a.close(); s.close()
        assert z.TreeRewind(tree.h, 8) == 8; return rc, o, log
    model = bm.records(segment, SIGNER, CID)
    # 1. the segment as it is: three blocks accepted, the third with no record
    B0, n0, want = comparand(segment, first); rc, o, log = bodies(segment, first); assert (B0, n0, want[0]) == (3, 3, 3) and want[1] == [True] * 3
    assert (rc, o["ok"], o["anchor_of"], o["recs"].tobytes(), o["accts_sizes"], o["set_sizes"], o["tree_sizes"]) + log == want, (rc, o["ok"], want[:3])
    assert o["n_recs"] == 3 and o["rec_of"] == [-1, 0, 1, -1, 2, -1, -1] == model[2] and o["rec_froms"] == senders and o["froms"] == model[3] and o["code"] == [0, 1, 1, 4, 1, 0, 0] and o["status"] == [t.OK] * 7
    assert o["txhash"] == model[6] and want[4][1] == want[4][2] and [r[:16] + r[16:528] + bytes(32) + r[560:] for r in [o["recs"].tobytes()[720 * j:720 * j + 720] for j in range(3)]] == model[0]
    # 2. a malformed transaction in block 1: k = 1 = B0, the states after block 0, the records of blocks 1 and 2 made and not decided
    broken = segment[:3] + [segment[3][:-1]] + segment[4:]; B0, n0, want = comparand(broken, first); rc, o, log = bodies(broken, first); assert (B0, n0, want[0]) == (1, 1, 1)
    assert rc == 1 and o["n_recs"] == 3 and o["status"] == [t.OK] * 3 + [t.MALFORMED] + [t.OK] * 3 and o["ok"] == [True, False, False] and o["anchor_of"] == want[2] + [-1, -1] and log == want[7:]
    assert o["recs"].tobytes()[:720] == want[3] and o["recs"].tobytes()[720:] == b"".join(bm.records(broken, SIGNER, CID)[0][1:])          # decided: filled; not decided: the old slot stays zero
    assert o["accts_sizes"] == want[4] + [want[4][0]] * 2 and o["set_sizes"] == want[5] + [want[5][0]] * 2 and o["tree_sizes"] == want[6] + [want[6][0]] * 2
    # 3. a stale mint in block 1 (mint 0 again: its old commitment is no longer the table's, its serial number is spent): k = 1 by ok, B0 = 3
    stale = segment[:3] + [segment[3], M[0]] + segment[5:]; B0, n0, want = comparand(stale, first); rc, o, log = bodies(stale, first); assert (B0, n0, want[0]) == (3, 3, 1) and want[1] == [True, True, False]
    assert (rc, o["ok"], o["anchor_of"], o["recs"].tobytes(), o["accts_sizes"], o["set_sizes"], o["tree_sizes"]) + log == want and o["status"] == [t.OK] * 7
    tree.close()

def run_leg(name, tmp_path, **env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path), **env))
    assert r.returncode == 0 and "LEG OK " + name in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
def test_poisoned_allocations_come_out_equal(tmp_path): run_leg("poison", tmp_path, ZK_DEBUG_POISON_ALLOC="1")
def test_verify_chain_bodies_on_real_proofs_against_the_three_calls(tmp_path): run_leg("chain", tmp_path)

if __name__ == "__main__":
    {"poison": leg_poison, "chain": leg_chain}[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
