"""Headers from their bytes on the device (include/zk_headers.h): zkHeaders against the model (tests/header_model.py) byte for byte on every output —
linked signed chains around the wave and workgroup sizes, every case of tests/header_corpus.py in one call and as header 0, every alignment of the upload, 4,097 copies of
one header, the recorded header's seal hash, poisoned allocations, two threads, the calls of zk_txs.h, zk_bodies.h and zk_tx_roots.h before and after, the ways to get
-1, and tx_root handed to verifyChainBodiesRoots on real proofs.  tests/test_headers_cpu.py pins the model.  Every test here fails on a library without the feature: the
entries do not exist."""
import ctypes, os, random, subprocess, sys, threading
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import header_corpus as c
import header_model as hm
import secp_model as sm
import tx_model as t

pytestmark = pytest.mark.gpu
ARG = -2

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    engine.init(); return engine

def rows(o, n):
    """the device's outputs as the model's dicts"""
    return [{k: (bytes(o[k][i]) if o[k].ndim == 2 else int(o[k][i])) for k in hm.ZERO} for i in range(n)]
def check(e, raws, period, epoch, now, parent, want=None, start=0):
    """zkgpu_headers against the model (or against `want`, the model's answer computed before), every output of every header, and the return value"""
    if want is None: want = hm.headers(raws, period, epoch, now, parent)
    rc, o = e.headers(raws, period, epoch, now, parent, start=start); got = rows(o, len(raws))
    for i, (g, w) in enumerate(zip(got, want)): assert g == w, (i, {f: (g[f], w[f]) for f in g if g[f] != w[f]})
    assert rc == hm.accepted(want), (rc, e.lib().zkgpu_last_error()); return want

# ---- chains ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_chain():
    """257 linked signed headers with a checkpoint every eight, and the model's answer, computed once: a prefix of the chain has the prefix of the answer"""
    raws, parent, signers = c.chain(c.CHAIN_SEED, 257); want = hm.headers(raws, c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent)
    assert hm.accepted(want) == 257 and [w["signer"] for w in want] == signers and all(w["status"] != hm.SEAL_UNDECIDED for w in want)
    return raws, parent, want

@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 127, 128, 129, 257])
def test_linked_signed_chains_around_the_wave_and_workgroup_sizes(e, long_chain, n):
    raws, parent, want = long_chain; check(e, raws[:n], c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent, want=want[:n])
    if n == 0: assert e.Zk().Headers([], c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent)[0] == 0

def test_chain_from_a_genesis_and_chains_that_break(e, long_chain):
    raws, parent, signers = c.chain(c.GENESIS_SEED, 12, first=0); assert parent is None
    want = check(e, raws, c.PERIOD, c.CHAIN_EPOCH, c.NOW, None); assert hm.accepted(want) == 12 and want[0]["signer"] == bytes(20) and [w["signer"] for w in want] == signers
    raws, parent, want = long_chain; raws = raws[:70]
    for broken in (raws[:5] + raws[6:], raws[:3] + [b"\xc0"] + raws[3:], raws[:64] + [raws[64][:-1]] + raws[65:], [b""] + raws, raws[1:]):
        got = check(e, broken, c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent); assert hm.accepted(got) < len(broken) and sum(w["status"] == hm.OK for w in got) >= 60
    late = check(e, raws, c.PERIOD, c.CHAIN_EPOCH, want[40]["time"], parent); assert hm.accepted(late) == 41 and late[41]["status"] == hm.FUTURE and late[41]["signer"] == bytes(20)
    slow = check(e, raws, c.PERIOD + 2, c.CHAIN_EPOCH, c.NOW, parent); assert hm.TIMESTAMP in {w["status"] for w in slow}
    k, o = e.Zk().Headers(raws, c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent); assert k == 70 and o["signer"] == [w["signer"] for w in want[:70]] and o["tx_root"] == [w["tx_root"] for w in want[:70]]

@pytest.mark.parametrize("start", range(8))
def test_headers_starting_at_every_residue_mod_8(e, long_chain, start):
    raws, parent, want = long_chain; check(e, raws[:9], c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent, want=want[:9], start=start)

# ---- the corpus -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(): return c.cases()

def test_the_whole_corpus_in_one_call(e, corpus):
    """every case behind its predecessor of the corpus: the standalone rules and the hashes of all of them, ANCESTOR for whatever passes them"""
    raws = [x[2] for x in corpus]; want = check(e, raws, c.PERIOD, c.EPOCH, c.NOW, corpus[0][3]); seen = {w["status"] for w in want}
    assert hm.accepted(want) == 2 and corpus[1][0] == "genesis, no parent" and hm.ANCESTOR in seen and hm.MALFORMED in seen and len(seen) >= 14

def test_every_case_of_the_corpus_as_header_0(e, corpus):
    seen = set()
    for label, claim, raw, parent, key in corpus:
        want = check(e, [raw, corpus[0][2]], c.PERIOD, c.EPOCH, c.NOW, parent); seen.add(want[0]["status"])
        if claim is not None: assert want[0]["status"] == claim, label
        if key is not None: assert want[0]["signer"] == hm.signer_address(key), label
    assert seen == set(range(17))

def test_4097_copies_of_one_header(e, long_chain):
    raws, parent, want = long_chain; three = hm.headers([raws[0]] * 3, c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent)
    assert three[0] == want[0] and three[1] == three[2] and three[1]["status"] == hm.ANCESTOR and three[1]["hash"] == want[0]["hash"]   # a copy depends on itself and its predecessor alone
    check(e, [raws[0]] * 4097, c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent, want=[three[0]] + [three[1]] * 4096)

def test_the_recorded_header_with_a_seal_appended_has_the_recorded_hash_as_its_seal_hash(e):
    from test_headers_cpu import recorded
    h, want, _ = recorded(); sealed = dict(h, Extra=h["Extra"] + random.Random(89).randbytes(65)); assert want.hex() == "0a5843ac1cb04865017cb35a57b50b07084e5fcee39b5acadade33149f4fff9e"
    rc, o = e.headers([hm.encode(sealed), hm.encode(h)], 0, 0, 2**63, None)
    assert rc == 0 and bytes(o["sealhash"][0]) == want and bytes(o["hash"][0]) == hm.header_hash(sealed) != want and not o["sealhash"][1].any() and bytes(o["hash"][1]) == hm.header_hash(h)
    check(e, [hm.encode(sealed), hm.encode(h)], 0, 0, 2**63, None)

# ---- the process around the call -----------------------------------------------------------------------------------------------------------------------------------
def test_two_threads_get_the_answers_of_one(e, long_chain, corpus):
    raws, parent, _ = long_chain; jobs = [(raws[:100], c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent), ([x[2] for x in corpus], c.PERIOD, c.EPOCH, c.NOW, None)]; got = [None, None]
    snap = lambda k: (lambda r: (r[0], [a.tobytes() for a in r[1].values()]))(e.headers(*jobs[k])); want = [snap(0), snap(1)]
    def loop(k):
        for _ in range(3): got[k] = snap(k)
    ts = [threading.Thread(target=loop, args=(k,)) for k in range(2)]
    for th in ts: th.start()
    for th in ts: th.join()
    assert got == want and want[0][0] == 100

def test_the_calls_of_zk_txs_zk_bodies_and_zk_tx_roots_give_the_same_bytes_before_and_after(e, long_chain):
    import bodies_corpus as bc
    import tx_corpus as tc
    pool = bc.Pool(); body = pool.body("zprz" * 20); by = {}
    for label, raw, signer, chain_id in tc.valid_cases(): by.setdefault((signer, chain_id), []).append(raw)
    def snap(): return ([(k, [a.tobytes() for a in e.tx_senders(v, *k)[1].values()], [a.tobytes() for a in e.tx_signing_inputs(v, *k)[1].values()]) for k, v in sorted(by.items())],
                        [a.tobytes() for a in e.tx_records(body, pool.signer, pool.chain_id)[1].values()], [a.tobytes() for a in e.tx_roots(body, [0, 30, 80])[1:]])
    raws, parent, want = long_chain; before = snap(); check(e, raws[:200], c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent, want=want[:200]); assert snap() == before
    check(e, raws[:3], c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent, want=want[:3])                       # a smaller call in the workspace the others have grown

def test_the_ways_to_get_minus_one(e, long_chain):
    L = e.lib(); raws, parent, want = long_chain; pool = raws[:3]; blob = np.frombuffer(b"".join(pool), dtype=np.uint8).copy()
    off = np.array([0] + list(np.cumsum([len(p) for p in pool])), dtype=np.uint64); dec = off.copy(); dec[1], dec[2] = off[2], off[1]
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None; u64 = ctypes.c_uint64; ph = np.frombuffer(parent[0], dtype=np.uint8).copy()
    widths = (32, 32, 20, 20, 32, 32, 8, 8, 1, 1, 4, 4, 4, 4, 1)
    def call(fn, hd, of, n, have=1, php=ph, skip=None):
        o = [np.full(3 * w, 0xA5, dtype=np.uint8) for w in widths]; fn.restype = ctypes.c_int
        return fn(ptr(hd), ptr(of), n, u64(c.PERIOD), u64(c.CHAIN_EPOCH), u64(c.NOW), have, ptr(php), u64(parent[1]), u64(parent[2]), *[None if k == skip else ptr(a) for k, a in enumerate(o)]), o
    zeroed = lambda o, skip=None: all(not a.any() for k, a in enumerate(o) if k != skip)
    for fn, bad in ((L.zkgpu_headers, ARG), (L.zkHeaders, -1)):
        rc, o = call(fn, blob, off, -1); assert rc == bad and all(set(a) == {0xA5} for a in o)          # n < 0: nothing to zero
        rc, o = call(fn, None, off, 3); assert rc == bad and zeroed(o)
        rc, o = call(fn, blob, None, 3); assert rc == bad and zeroed(o)
        rc, o = call(fn, blob, dec, 3); assert rc == bad and zeroed(o) and b"decrease" in L.zkgpu_last_error()
        rc, o = call(fn, blob, off, 3, php=None); assert rc == bad and zeroed(o)                       # a parent without its hash
        for k in range(15):
            rc, o = call(fn, blob, off, 3, skip=k); assert rc == bad and zeroed(o, skip=k), k
        rc, o = call(fn, blob, off, 0); assert rc == 0 and all(set(a) == {0xA5} for a in o)            # n = 0: nothing queued, nothing written
        rc, o = call(fn, blob, off, 3); assert rc == 3 and bytes(o[0]) == b"".join(w["hash"] for w in want[:3]) and bytes(o[2]) == b"".join(w["signer"] for w in want[:3])
        rc, o = call(fn, blob, off, 3, have=0, php=None); assert rc == 0 and o[14][0] == hm.ANCESTOR and list(o[14][1:]) == [hm.OK, hm.OK]   # no parent: NULL is fine
    off2 = off.copy(); off2[2] = off2[1]                                                               # an empty header is MALFORMED, not an error
    rc, o = call(L.zkHeaders, blob, off2, 3); assert rc == 1 and list(o[14]) == [hm.OK, hm.MALFORMED, hm.MALFORMED] and not o[0][32:].any()

# ---- child-process legs ---------------------------------------------------------------------------------------------------------------------------------------------
def leg_poison(tmp):
    """every device allocation of this process starts full of 0xA5 bytes (ZK_DEBUG_POISON_ALLOC=1): what the kernels leave unwritten would show in the outputs"""
    from blockmaze_amd import engine as e
    assert os.environ.get("ZK_DEBUG_POISON_ALLOC") == "1"; e.init(); cases = c.cases()
    check(e, [x[2] for x in cases], c.PERIOD, c.EPOCH, c.NOW, cases[0][3])
    raws, parent, _ = c.chain(c.CHAIN_SEED, 65); want = check(e, raws, c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent); assert hm.accepted(want) == 65
    check(e, raws[:2], c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent, want=want[:2])                        # a smaller call in the grown workspace

def leg_chain(tmp):
    """The segment of tests/test_gpu_bodies.py — three mint proofs, a public transaction and a code-4 transaction in two blocks, and a block of public transactions only —
    under three signed headers whose TxHash is the block's transaction trie root: zkHeaders, then its tx_root, unchanged, as want_roots of VerifyChainBodiesRoots.  With a
    header that names another root the header call accepts all three (it never sees a body) and the chain call stops at that block."""
    import workload as w
    import bodies_corpus as bc
    import tx_corpus as tc
    import tx_roots_model as rm
    from blockmaze_amd import engine as e
    from test_gpu_chain_accounts import DEPTH
    e.keygen("mint", os.path.join(tmp, "mintpk.txt"), os.path.join(tmp, "mintvk.txt"), seed=0x5EED); z = e.Zk(); rng = random.Random(23); SIGNER, CID = t.EIP155, 1337
    def mint_of(d): p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return d, p
    mints = [mint_of(w.mint_instance(30 + i)) for i in range(3)]; keys = [rng.randrange(1, 2**24) for _ in range(3)]; senders = [sm.address(sm.mul(k, sm.G)) for k in keys]
    def mint_tx(j): d, p = mints[j]; return t.encode(t.sign_tx(tc.rand_tx(rng, Code=1, ZKValue=d["value_s"], ZKSN=d["sn_old"], ZKCMT=d["cmtA"], ZKProof=p.encode()), SIGNER, CID, keys[j], rng.randrange(1, 2**24)))
    def other(code): return t.encode(bc.signed(rng, SIGNER, CID, Code=code))
    M = [mint_tx(j) for j in range(3)]; segment = [other(0), M[0], M[1], other(4), M[2], other(0), other(0)]; first = [0, 2, 5, 7]
    right, defined = rm.tx_roots(segment, first, keccak_many=lambda msgs: [t.keccak256(m) for m in msgs]); assert defined == [True] * 3 and len(set(right)) == 3
    def headers_over(roots):
        parent = (rng.randbytes(32), 40, c.T0); prev = parent; raws = []
        for b, root in enumerate(roots):
            h = hm.sign_header(c.rand_header(rng, Number=41 + b, ParentHash=prev[0], Time=prev[2] + c.PERIOD, TxHash=root), c.KEYS[b], rng.randrange(1, sm.N)); raws.append(hm.encode(h))
            prev = (hm.header_hash(h), 41 + b, h["Time"])
        return raws, parent
    tree = e.Tree(DEPTH); leaves = w.deposit_instance(1, 8)["leaves"]; assert z.TreeAppend(tree.h, leaves) == 8
    for roots, accepted in ((right, 3), ([right[0], right[2], right[2]], 1)):
        raws, parent = headers_over(roots); k, o = z.Headers(raws, c.PERIOD, 0, c.NOW, parent)
        assert k == 3 and o["signer"] == [hm.signer_address(key) for key in c.KEYS[:3]] and o["tx_root"] == roots and o["status"] == [hm.OK] * 3
        a = e.AccountTable(); assert z.AcctsSet(a, senders, [d["cmtA_old"] for d, p in mints]) == 0; s = e.SpentSet(bytes(20))
        rc, out = z.VerifyChainBodiesRoots(None, segment, first, o["tx_root"], SIGNER, CID, a, tree.h, [8], 8, s.h, fill=0xA5)
        assert rc == accepted and out["roots"] == right and out["root_ok"] == [r == g for r, g in zip(roots, right)], (rc, out["root_ok"])
        a.close(); s.close(); assert z.TreeRewind(tree.h, 8) == 8
    tree.close()

def run_leg(name, tmp_path, **env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path), **env))
    assert r.returncode == 0 and "LEG OK " + name in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
def test_poisoned_allocations_come_out_equal(tmp_path): run_leg("poison", tmp_path, ZK_DEBUG_POISON_ALLOC="1")
def test_tx_root_into_verify_chain_bodies_roots_on_real_proofs(tmp_path): run_leg("chain", tmp_path)

if __name__ == "__main__":
    {"poison": leg_poison, "chain": leg_chain}[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
