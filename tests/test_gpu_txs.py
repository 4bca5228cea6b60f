"""Sender inputs from raw transactions on the device (include/zk_txs.h): the multi-block sponge against the model, zkTxSigningInputs against the model
field by field of the output on every shape the walk and the hashes distinguish, the refusal corpus of tests/tx_corpus.py, zkTxSenders on signed transactions, and
its froms inside verifyChainAccounts.  The model (tests/tx_model.py) is a restatement of the reference's Go; tests/test_txs_cpu.py pins it.  Every test here fails on
a library without the feature: the entries do not exist."""
import ctypes, os, random, subprocess, sys, threading
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import secp_model as sm
import tx_model as t
import tx_corpus as c

pytestmark = pytest.mark.gpu
ARG = -2

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    engine.init(); return engine

_MODEL = {}
def model(raw, signer, chain_id):
    """the model's signing inputs, computed once a distinct case"""
    k = (raw, signer, chain_id)
    if k not in _MODEL: _MODEL[k] = t.signing_inputs(raw, signer, chain_id)
    return _MODEL[k]
@pytest.fixture(scope="module")
def valid(): return c.valid_cases()

def check_inputs(e, cases):
    """zkTxSigningInputs on cases of one signer and chain id against the model, every output"""
    z = e.Zk(); signer, chain_id = cases[0][2], cases[0][3]; assert all(x[2:] == (signer, chain_id) for x in cases)
    txhash, sighash, sigs, dep, code, status = z.TxSigningInputs([x[1] for x in cases], signer, chain_id)
    for k, x in enumerate(cases):
        want = model(x[1], signer, chain_id); got = dict(status=status[k], code=code[k], txhash=txhash[k], sighash=sighash[k], sig=sigs[k], deposit_from=dep[k])
        assert got == want, (x[0], k, {f: (got[f], want[f]) for f in got if got[f] != want[f]})
    return status
def grouped(cases):
    g = {}
    for x in cases: g.setdefault((x[2], x[3]), []).append(x)
    return list(g.values())

# ---- the sponge -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_sponge_every_length_to_300_and_the_third_block_at_every_alignment(e):
    """one call; the strings lie end to end, so the lengths 0 .. 300 alone start at every alignment; the block edges 407 / 408 / 409 are repeated behind 0, 1, 2 and
    3 bytes of filler"""
    rng = random.Random(31); msgs = [rng.randbytes(n) for n in range(301)]
    for shift in range(4):
        for n in (135, 136, 137, 271, 272, 273, 407, 408, 409): msgs += [bytes(shift), rng.randbytes(n)]
    starts = np.cumsum([0] + [len(m) for m in msgs[:-1]]); assert {int(s) % 4 for s, m in zip(starts, msgs) if len(m) >= 407} == {0, 1, 2, 3}
    assert e.keccak256(msgs) == [t.keccak256(m) for m in msgs]
    assert e.keccak256([]) == [] and e.keccak256([b""])[0].hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"

# ---- valid transactions ---------------------------------------------------------------------------------------------------------------------------------------------
def test_every_valid_shape_field_by_field(e, valid):
    """payload lengths over the three header forms of the signing list and of the transaction, both hashes at 135 / 136 / 137 mod 136, nil recipients of both
    spellings, CMTBlock of 0 / 1 / 3, the six codes, the chain ids, the three signers, both V; protected, unprotected and wrong-id records in one EIP155 call"""
    labels = {x[0] for x in valid}; seen = set()
    for want in ["payload %d" % L for L in c.PAYLOAD_LENGTHS] + ["payload one byte", "recipient 0x80", "recipient 0xC0", "cmtblock 0", "cmtblock 1", "cmtblock 3", "sig 135 mod 136", "sig 0 mod 136",
                 "sig 1 mod 136", "tx 135 mod 136", "tx 0 mod 136", "tx 1 mod 136"] + ["code %d" % k for k in range(6)] + ["chain id %d" % i for i in c.CHAIN_IDS]: assert want in labels, want
    for group in grouped(valid):
        status = check_inputs(e, group); seen |= set(status)
        if group[0][2] == t.EIP155 and any("wrong" in x[0] for x in group): assert t.CHAIN_ID in status and t.OK in status and any("unprotected" in x[0] for x in group)
    assert seen == {t.OK, t.CHAIN_ID}
    for x in valid:
        if x[0].startswith("sig "): tx, sp = t.decode(x[1]); six = x[1][sp[1][0]: sp[6][1]] + (t.enc_int(x[3]) + b"\x80\x80" if x[2] == t.EIP155 else b""); assert len(t.head(0xC0, len(six)) + six) % 136 == {"135": 135, "0": 0, "1": 1}[x[0].split()[1]]
        if x[0].startswith("tx "): assert len(x[1]) % 136 == {"135": 135, "0": 0, "1": 1}[x[0].split()[1]]

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 300])
def test_counts_around_the_wave_and_workgroup_sizes(e, valid, n):
    pool = [x for x in valid if x[2:] == (t.EIP155, 1) and len(x[1]) < 2000]; assert len(pool) >= 10
    cases = [pool[(3 * n + i) % len(pool)] for i in range(n)]
    if n == 0: assert e.Zk().TxSigningInputs([], t.EIP155, 1) == ([], [], [], [], [], []); return
    check_inputs(e, cases)

# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(): return c.refusal_corpus()

def test_refusal_corpus_against_the_model(e, corpus):
    """at least 300 cases; every MALFORMED rule of the header for each of six bases, every status class; both calls.  A mutator that stops producing its case shows in
    the counts."""
    z = e.Zk(); rules = {}; classes = {k: 0 for k in (t.OK, t.MALFORMED, t.CHAIN_ID, t.SIG)}; assert len(corpus) >= 300
    for group in grouped([(x[0], x[2], x[3], x[4]) for x in corpus]):
        signer, chain_id = group[0][2:]; check_inputs(e, group)
        froms, txhash, code, status = z.TxSenders([x[1] for x in group], signer, chain_id)
        for k, x in enumerate(group):
            want = t.sender(x[1], signer, chain_id); assert (status[k], code[k], txhash[k], froms[k]) == want, (x[0], k, status[k], want[0]); rules[x[0]] = rules.get(x[0], 0) + 1; classes[want[0]] += 1
    names = [r for r, _ in c.malformed_mutators()]; assert len(names) >= 45 and all(rules[r] == 6 for r in names) and rules["valid"] == 6, rules
    for rule in ["V = %d" % v for v in (0, 26, 29, 34, 35, 36)] + ["V of %d bytes" % k for k in (2, 8, 9, 33)] + ["R of 33 bytes", "S of 33 bytes", "R = 0", "S above N / 2"]: assert rules[rule] == 3, rule
    assert classes[t.OK] >= 6 and classes[t.MALFORMED] >= 270 and classes[t.CHAIN_ID] >= 12 and classes[t.SIG] >= 30, classes

def test_the_ten_ways_to_get_minus_one(e, valid):
    L = e.lib(); pool = [x[1] for x in valid if x[2:] == (t.EIP155, 1)][:3]; blob = np.frombuffer(b"".join(pool), dtype=np.uint8).copy()
    off = np.array([0] + list(np.cumsum([len(p) for p in pool])), dtype=np.uint64); dec = off.copy(); dec[1], dec[2] = off[2], off[1]
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None; cid = lambda v: ctypes.c_uint64(v)
    def fresh(): return [np.full(3 * w, 0xA5, dtype=np.uint8) for w in (32, 32, 65, 20, 1, 1)]
    def zeroed(outs, skip=()): return all(not a.any() for k, a in enumerate(outs) if k not in skip)
    for fn, bad in ((L.zkgpu_tx_signing_inputs, ARG), (L.zkTxSigningInputs, -1)):
        fn.restype = ctypes.c_int
        o = fresh(); assert fn(ptr(blob), ptr(off), -1, 2, cid(1), *map(ptr, o)) == bad and all(set(a) == {0xA5} for a in o)                         # 1: n < 0, nothing to zero
        o = fresh(); assert fn(None, ptr(off), 3, 2, cid(1), *map(ptr, o)) == bad and zeroed(o)                                                       # 2: no txs
        o = fresh(); assert fn(ptr(blob), None, 3, 2, cid(1), *map(ptr, o)) == bad and zeroed(o)                                                      # 3: no off
        for k in (0, 1, 2, 4, 5):                                                                                                                    # 4-8: an output missing
            o = fresh(); args = [ptr(a) for a in o]; args[k] = None; assert fn(ptr(blob), ptr(off), 3, 2, cid(1), *args) == bad and zeroed(o, skip=(k,)), k
        o = fresh(); assert fn(ptr(blob), ptr(dec), 3, 2, cid(1), *map(ptr, o)) == bad and zeroed(o)                                                  # 9: a decreasing off
        o = fresh(); assert fn(ptr(blob), ptr(off), 3, 3, cid(1), *map(ptr, o)) == bad and zeroed(o)                                                  # 10: an unknown signer
        o = fresh(); assert fn(ptr(blob), ptr(off), 3, -1, cid(1), *map(ptr, o)) == bad and zeroed(o)
        o = fresh(); assert fn(ptr(blob), ptr(off), 3, 2, cid(2**62), *map(ptr, o)) == bad and zeroed(o)                                              # 11: chain_id >= 2^62
        o = fresh(); assert fn(ptr(blob), ptr(off), 0, 2, cid(1), *map(ptr, o)) == 0 and all(set(a) == {0xA5} for a in o)                             # n = 0: nothing queued, nothing written
        o = fresh(); args = [ptr(a) for a in o]; args[3] = None; assert fn(ptr(blob), ptr(off), 3, 2, cid(1), *args) == 3 and bytes(o[0][:32]) == t.keccak256(pool[0])   # deposit_from may be NULL
    for fn, bad in ((L.zkgpu_tx_senders, ARG), (L.zkTxSenders, -1)):
        fn.restype = ctypes.c_int
        def fresh4(): return [np.full(3 * w, 0xA5, dtype=np.uint8) for w in (32, 20, 1, 1)]
        o = fresh4(); assert fn(ptr(blob), ptr(off), -1, 2, cid(1), *map(ptr, o)) == bad and all(set(a) == {0xA5} for a in o)
        for k in (1, 2, 3):
            o = fresh4(); args = [ptr(a) for a in o]; args[k] = None; assert fn(ptr(blob), ptr(off), 3, 2, cid(1), *args) == bad and zeroed(o, skip=(k,)), k
        o = fresh4(); assert fn(ptr(blob), ptr(dec), 3, 2, cid(1), *map(ptr, o)) == bad and zeroed(o)
        o = fresh4(); assert fn(ptr(blob), ptr(off), 3, 7, cid(1), *map(ptr, o)) == bad and zeroed(o)
        o = fresh4(); assert fn(ptr(blob), ptr(off), 3, 2, cid(2**63), *map(ptr, o)) == bad and zeroed(o)
    off2 = off.copy(); off2[2] = off2[1]                                                              # an empty transaction is MALFORMED, not an error
    o = fresh(); assert L.zkTxSigningInputs(ptr(blob), ptr(off2), 3, 2, cid(1), *map(ptr, o)) == 1 and list(o[5]) == [t.OK, t.MALFORMED, t.MALFORMED] and not o[0][32:].any()

# ---- zkTxSenders ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def signed(): return c.signed_cases()

def test_senders_of_signed_transactions_deposits_and_refused_records(e, signed):
    """froms equals the keys' addresses; a deposit carries ZKAdrress whatever its V, R, S are; refused records lie between them; txhash = NULL; and the one call agrees
    byte for byte with zkTxSigningInputs followed by zkRecoverSenders"""
    z = e.Zk(); seen = {k: 0 for k in (t.OK, t.MALFORMED, t.SIG)}; deposits = 0
    for signer in c.SIGNERS:
        for chain_id in (0, 1, 1337, 2**62 - 1):
            group = [x for x in signed if x[1:3] == (signer, chain_id)]
            if not group: continue
            raws = [x[0] for x in group]; froms, txhash, code, status = z.TxSenders(raws, signer, chain_id)
            for k, x in enumerate(group):
                want = t.sender(x[0], signer, chain_id); assert (status[k], code[k], txhash[k], froms[k]) == want, k; seen[want[0]] += 1; deposits += code[k] == 3
                if x[4] is not None: assert (status[k], froms[k]) == (x[4], x[3]), k                   # the key's own address, not only the model's
            froms2, none, code2, status2 = z.TxSenders(raws, signer, chain_id, want_txhash=False); assert none is None and (froms2, code2, status2) == (froms, code, status)
            th, sh, sigs, dep, code3, st3 = z.TxSigningInputs(raws, signer, chain_id); rf, _, ok = z.RecoverSenders(sh, sigs, homestead=signer != t.FRONTIER, want_pubs=False)
            two = [dep[k] if code3[k] == 3 else (rf[k] if st3[k] == t.OK and ok[k] else bytes(20)) for k in range(len(raws))]
            assert two == froms and th == txhash and code3 == code and [t.SIG if (st3[k] == t.OK and code3[k] != 3 and not ok[k]) else st3[k] for k in range(len(raws))] == status
    assert seen[t.OK] >= 36 and seen[t.MALFORMED] >= 3 and seen[t.SIG] >= 6 and deposits >= 4, (seen, deposits)

def test_two_threads_get_the_answers_of_one(e, signed):
    z = e.Zk(); parts = [[x[0] for x in signed if x[1:3] == (t.EIP155, 1)], [x[0] for x in signed if x[1:3] == (t.HOMESTEAD, 1)]]; args = [(t.EIP155, 1), (t.HOMESTEAD, 1)]; got = [None, None]
    assert all(len(p) >= 3 for p in parts); want = [z.TxSenders(parts[k], *args[k]) for k in range(2)]
    def run(k):
        for _ in range(3): got[k] = z.TxSenders(parts[k], *args[k])
    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for th in ts: th.start()
    for th in ts: th.join()
    assert got == want and all(w[3].count(t.OK) >= 3 for w in want)

# ---- into the chain call --------------------------------------------------------------------------------------------------------------------------------------------
def leg_chain(tmp):
    """The shape of tests/test_gpu_senders.py's last test: three mint proofs in two blocks; every record's transaction is encoded and signed by the model under a
    seeded key; the froms that zkTxSenders gives go into verifyChainAccounts, and the answer — return value, verdicts, anchors, the filled records, the sizes, the
    table's log — must be what the call gives with the addresses the model computes."""
    import workload as w
    from blockmaze_amd import engine as e
    from test_gpu_block_accounts import ZERO, with_old
    from test_gpu_chain_accounts import DEPTH
    e.keygen("mint", os.path.join(tmp, "mintpk.txt"), os.path.join(tmp, "mintvk.txt"), seed=0x5EED); z = e.Zk(); rng = random.Random(17)
    def mint_of(d): p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("mint", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    items = [mint_of(w.mint_instance(20 + i)) for i in range(3)]; first = [0, 1, 3]; keys = [rng.randrange(1, 2**24) for _ in items]
    raws = [t.encode(t.sign_tx(c.rand_tx(rng, Code=1, ZKValue=int(it[3]), ZKProof=it[1].encode()), t.EIP155, 1337, k, rng.randrange(1, 2**24))) for it, k in zip(items, keys)]
    model = [sm.address(sm.mul(k, sm.G)) for k in keys]; assert [t.sender(r, t.EIP155, 1337)[3] for r in raws] == model and len(set(model)) == 3
    froms, txhash, code, status = z.TxSenders(raws, t.EIP155, 1337); assert status == [t.OK] * 3 and code == [1] * 3 and txhash == [t.keccak256(r) for r in raws]
    tree = e.Tree(DEPTH); leaves = w.deposit_instance(1, 8)["leaves"]; assert z.TreeAppend(tree.h, leaves) == 8; answers = []
    for road in (froms, model):
        a = e.AccountTable(); assert z.AcctsSet(a, list(model), [it[2][0] for it in items]) == 0; s = e.SpentSet(bytes(20))   # (the state belongs to the real senders on both roads)
        got = z.VerifyChainAccounts(None, e.records_from_items([with_old(it, ZERO) for it in items]), list(road), first, a, tree.h, [8], 8, s.h)
        answers.append((got[:3], got[3].tobytes(), got[4:], a.read_log(), s.read_log(), tree.size())); a.close(); s.close(); assert z.TreeRewind(tree.h, 8) == 8
    assert answers[0] == answers[1] and answers[0][0] == (2, [True] * 3, [-1] * 3), answers[0][0]          # the two roads first: a wrong sender shows here as a record not accepted
    assert froms == model
    tree.close()

def test_tx_senders_into_verify_chain_accounts(tmp_path):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chain", str(tmp_path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path)))
    assert r.returncode == 0 and "LEG OK chain" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])

if __name__ == "__main__":
    {"chain": leg_chain}[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
