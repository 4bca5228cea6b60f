"""The proof cache (blockmaze_amd/csrc/gpu_proof_cache.hip; include/zk_proof_cache.h, include/zkgpu.h): the digest kernel against the host model and hashlib, and the
cached entries against the uncached ones on the same records — the reference verdict everywhere — and against the Python model of tests/test_proof_cache_cpu.py.
Keys come from engine.keygen with fixed seeds, proofs are a handful of real send, mint, redeem and deposit proofs used in rotation; they are made once, by the leg
"make", and every other leg loads them.  Every leg runs in a process of its own under a time limit: `python tests/test_gpu_proof_cache.py <leg> <scratch dir>`."""
import hashlib, os, random, subprocess, sys, threading
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
from test_proof_cache_cpu import CacheModel, SALT, TAGS, model_digests, record_key

pytestmark = pytest.mark.gpu
KINDS = ("mint", "send", "deposit", "redeem")                      # by ZK_KIND_*
SEEDS_A, SEEDS_B = 0xB10C4A2E, 0x0DDBA11

# ---- the shared material ----------------------------------------------------------------------------------------------------------------------------------------
def leg_make(tmp):
    """key directories A and B (other seeds) and six valid records: two sends, two mints, a redeem and a deposit with its sixteen leaves"""
    from blockmaze_amd import engine as e
    import workload as w
    for d, seed in (("A", SEEDS_A), ("B", SEEDS_B)):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)
        for i, kind in enumerate(("send", "mint", "redeem", "deposit")): e.keygen(kind, os.path.join(tmp, d, kind + "pk.txt"), os.path.join(tmp, d, kind + "vk.txt"), seed=seed + 7 * i)
    z = e.Zk(); items = []
    for i in (1, 2):
        d = w.send_instance(i); p = z.GenSendProof(*w.send_args(d)); a = [d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]; assert z.VerifySendProof(p, *a); items.append(("send", p, a, 0))
    for i in (1, 2):
        d = w.mint_instance(i); p = z.GenMintProof(*w.mint_args(d)); items.append(("mint", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"]))
    d = w.mint_instance(1, redeem=True); p = z.GenRedeemProof(*w.mint_args(d)); items.append(("redeem", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"]))
    d = w.deposit_instance(1, 16); p = z.GenDepositProof(*w.deposit_args(d), d["leaves"], d["rt"], d["sk"]); items.append(("deposit", p, [d["rt"], d["pk_recv"], d["cmtB_old"], d["sn_old"], d["cmtB"], d["sn_s"]], 0))
    recs = e.records_from_items(items); rc, ok = z.VerifyBlockRecords(recs); assert rc == 6 and all(ok)
    np.savez(os.path.join(tmp, "base.npz"), recs=recs, leaves=np.frombuffer(b"".join(d["leaves"]), dtype=np.uint8).reshape(16, 32))

def base(tmp):
    from blockmaze_amd import engine as e
    f = np.load(os.path.join(tmp, "base.npz")); return e.Zk(), f["recs"].astype(e.RECORD_DTYPE), f["leaves"]
def vk_paths(tmp, d="A"): return [os.path.join(tmp, d, k + "vk.txt") for k in KINDS]
def vk_tags(tmp, d="A"): return [hashlib.sha256(open(p, "rb").read()).digest() for p in vk_paths(tmp, d)]
def keys_of(salt, tags, recs): return [k if int(r["kind"]) <= 3 else None for k, r in zip(model_digests(salt, tags, recs), recs)]
def counters(e, tmp): return (e.verify_rlc_counters(),) + tuple(e.verify_path_counters(p) for p in vk_paths(tmp))
def moved(a, b): return [tuple(y - x for x, y in zip(p, q)) for p, q in zip(a, b)]
def distinct(recs): return len({r.tobytes() for r in recs})
STATEMENT = {0: [(0, 32), (1, 32), (2, 32)], 1: [(0, 32), (1, 32), (2, 32), (3, 32)], 2: [(0, 32), (1, 20), (2, 32), (3, 32), (4, 32), (5, 32)], 3: [(0, 32), (1, 32), (2, 32)]}
def with_reserved(rec, j, v): r = rec.copy(); r["reserved"][j] = v; return r

def twin_block(recs):
    """about 200 records: each valid record three times, twelve twins with one proof character changed, twelve with one statement bit flipped, value_s + 1, and
    four with a `reserved` byte changed (still valid, another key); then a proof byte that is no hex digit and two unknown kinds"""
    rng = random.Random(0x7A1); out = []
    for rec in recs:
        out += [rec.copy(), rec.copy(), rec.copy()]; fields = STATEMENT[int(rec["kind"])]
        for _ in range(12):
            r = rec.copy(); at = rng.randrange(512); ch = r["proof"][at]; r["proof"][at] = ord("0123456789abcdef"[(int(chr(ch), 16) + 1 + rng.randrange(15)) % 16]); out.append(r)
        for _ in range(12):
            r = rec.copy(); a, ln = rng.choice(fields); r["args"][a][rng.randrange(ln)] ^= 1 << rng.randrange(8); out.append(r)
        r = rec.copy(); r["value_s"] = int(r["value_s"]) + 1; out.append(r)
        for t, j in enumerate((0, 3, 6, 6)): out.append(with_reserved(rec, j, 0x11 * (t + 1)))
    bad = recs[0].copy(); bad["proof"][77] = ord("G"); unk = recs[1].copy(); unk["kind"] = 4; unk2 = recs[2].copy(); unk2["kind"] = 255
    block = np.array(out + [bad, unk, unk2], dtype=recs.dtype); return block[np.random.default_rng(5).permutation(len(block))]

# ---- the legs (each in a fresh process) ------------------------------------------------------------------------------------------------------------------------
def leg_digest(tmp):
    """k_record_digest = the host model = hashlib at the wave and workgroup edges, the four kinds and unknown kinds interleaved, four distinct tags"""
    from blockmaze_amd import engine as e
    import block_records as br
    pool = np.concatenate([br.random_records(k, 260, 0xD16 + k) for k in range(4)]); np.random.default_rng(9).shuffle(pool); odd = np.arange(5, len(pool), 7); pool["kind"][odd] = np.array([4, 255, 9, 128], dtype=np.uint8)[np.arange(len(odd)) % 4]
    assert len(set(TAGS)) == 4 and sorted(set(int(k) for k in pool["kind"][:64])) == [0, 1, 2, 3, 4, 9, 128, 255]
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000):
        recs = pool[:n]; k0 = e.proof_cache_launches(); dev = [bytes(x) for x in e.record_digests(SALT, TAGS, recs, device=True)]; k1 = e.proof_cache_launches()
        host = [bytes(x) for x in e.record_digests(SALT, TAGS, recs, device=False)]; assert (k1 - k0, e.proof_cache_launches() - k1) == (1, 0), n
        want = model_digests(SALT, TAGS, recs); assert dev == want and host == want, (n, [i for i in range(n) if dev[i] != want[i]][:8])
    assert [bytes(x) for x in e.record_digests(SALT, TAGS, pool[5:6], device=True)] == [bytes(20)] and len(e.record_digests(SALT, TAGS, pool[:0], device=True)) == 0
    tail = np.repeat(pool[:1], 70); tail["args"][:, 5, 16:] = np.random.default_rng(10).integers(0, 256, (70, 16), dtype=np.uint8)   # records whose last 16 bytes differ only: the last block alone
    assert len({r.tobytes()[:704] for r in tail}) == 1; dev = [bytes(x) for x in e.record_digests(SALT, TAGS, tail, device=True)]; assert dev == model_digests(SALT, TAGS, tail) and len(set(dev)) == 70

def leg_verdicts(tmp):
    """the same verdicts, fewer verifications"""
    from blockmaze_amd import engine as e
    z, recs, _ = base(tmp); block = twin_block(recs); n = len(block); assert 190 <= n <= 210
    rc0, ok0 = z.VerifyBlockRecords(block); keyed = sum(int(k) <= 3 for k in block["kind"]); acc = block[np.array(ok0)]; assert rc0 == sum(ok0) and keyed == n - 2
    for rec in recs:                                                                               # the `reserved` twins are valid records of their own
        tw = [i for i in range(n) if block[i].tobytes()[8:] == rec.tobytes()[8:] and block[i]["kind"] == rec["kind"]]; assert len(tw) == 7 and all(ok0[i] for i in tw) and distinct(block[tw]) == 5
    assert 6 * 7 <= rc0 < n - 100
    c = e.ProofCache(1 << 12); rc1, ok1 = z.VerifyRecordsCached(c, block); assert (rc1, ok1) == (rc0, ok0) and c.stats() == (0, keyed, distinct(acc), distinct(acc))
    before = counters(e, tmp); rc2, ok2 = z.VerifyRecordsCached(c, block); mid = counters(e, tmp); assert (rc2, ok2) == (rc0, ok0)
    assert c.stats() == (rc0, keyed + keyed - rc0, distinct(acc), distinct(acc))
    rej = block[~np.array(ok0)]; rcr, okr = z.VerifyBlockRecords(rej); after = counters(e, tmp); assert rcr == 0 and not any(okr)
    assert moved(before, mid) == moved(mid, after) and any(any(m) for m in moved(mid, after)), (moved(before, mid), moved(mid, after))
    d = e.ProofCache(1 << 12); assert z.VerifyRecordsCached(d, acc) == (len(acc), [True] * len(acc)); before = counters(e, tmp)
    assert z.VerifyRecordsCached(d, acc) == (len(acc), [True] * len(acc)) and counters(e, tmp) == before and d.stats() == (len(acc), len(acc), distinct(acc), distinct(acc))   # valid records only: no verifier runs
    assert z.VerifyRecordsCached(None, block) == (rc0, ok0) and z.VerifyRecordsCached(c, block[:0]) == (0, [])

def leg_neighbours(tmp):
    """a neighbour of a stored record is never a hit: 64 single-bit flips over every field of one stored record per kind"""
    from blockmaze_amd import engine as e
    z, recs, _ = base(tmp); c = e.ProofCache(1 << 12); rng = random.Random(0xF11B)
    one = recs[[0, 2, 4, 5]]; assert sorted(int(k) for k in one["kind"]) == [0, 1, 2, 3] and z.VerifyRecordsCached(c, one) == (4, [True] * 4) and c.stats() == (0, 4, 4, 4)
    bits = [b for b in range(8)] + rng.sample(range(8, 64), 8) + rng.sample(range(64, 128), 8) + rng.sample(range(128, 8 * 528), 20) + rng.sample(range(8 * 528, 8 * 720), 20); assert len(set(bits)) == 64
    for rec in one:
        nb = np.array([rec] * 64, dtype=recs.dtype); raw = nb.view(np.uint8).reshape(64, 720)
        for i, b in enumerate(bits): raw[i, b // 8] ^= 1 << (b % 8)
        h0 = c.stats()[0]; want = z.VerifyBlockRecords(nb); assert z.VerifyRecordsCached(c, nb) == want and c.stats()[0] == h0, int(rec["kind"])
    assert z.VerifyRecordsCached(c, one) == (4, [True] * 4) and c.stats()[0] == 4

def leg_keys(tmp):
    """the verifying key is part of the key: what was stored under directory A is unknown under B (other seeds), and known again under A"""
    from blockmaze_amd import engine as e
    z, recs, _ = base(tmp); block = np.concatenate([recs, recs[::-1], recs[:3]]); n = len(block); c = e.ProofCache(1 << 12)
    assert z.VerifyRecordsCached(c, block) == (n, [True] * n) and c.stats() == (0, n, 6, 6)
    os.environ["ZK_PRFKEY_DIR"] = os.path.join(tmp, "B"); assert vk_tags(tmp, "B") != vk_tags(tmp, "A")
    assert z.VerifyBlockRecords(block) == (0, [False] * n) and z.VerifyRecordsCached(c, block) == (0, [False] * n) and c.stats() == (0, 2 * n, 6, 6)
    os.environ["ZK_PRFKEY_DIR"] = os.path.join(tmp, "A")
    before = counters(e, tmp); assert z.VerifyRecordsCached(c, block) == (n, [True] * n) and c.stats() == (n, 2 * n, 6, 6) and counters(e, tmp) == before

def leg_generations(tmp):
    """a cache of 8 entries against the model: rotation, the capacity / 2 cut, and a rotated-out record verified and accepted again"""
    from blockmaze_amd import engine as e
    z, recs, _ = base(tmp); tags = vk_tags(tmp); pool = np.array([with_reserved(recs[0], i % 7, 1 + i) for i in range(20)], dtype=recs.dtype); assert distinct(pool) == 20
    assert z.VerifyBlockRecords(pool) == (20, [True] * 20); keys = keys_of(SALT, tags, pool); c = e.ProofCache(8, SALT); m = CacheModel(8); seen = []
    for call in ([0, 1, 2], [3, 4], [5, 6, 7, 8, 9, 10], [11, 12, 13, 14], [9, 10, 5, 0], [15, 16, 17, 18, 19], [0, 1, 15, 19, 12, 3], [0, 0, 7, 7]):
        ok, hit = m.call([keys[i] for i in call], [True] * len(call)); h0 = c.stats()[0]; got = z.VerifyRecordsCached(c, pool[call])
        assert got == (len(call), ok) and c.stats() == m.stats() and c.stats()[3] <= 8, (call, got, c.stats(), m.stats()); seen.append((sum(hit), c.stats()[3]))
    assert seen[2] == (0, 6) and seen[4][0] == 1 and any(h for h, _ in seen[5:]) and max(n for _, n in seen) == 8, seen   # six candidates store four; record 0 was rotated out and comes back as a miss
    c.clear(); assert c.stats()[3] == 0 and z.VerifyRecordsCached(c, pool[:2]) == (2, [True, True])

def leg_chain(tmp):
    """chain state is not cached: roots and serial numbers decide as in verifyBlockFull although every proof is a hit"""
    from blockmaze_amd import engine as e
    z, recs, leaves = base(tmp); S1, M1, R1, D1 = recs[0], recs[2], recs[4], recs[5]
    block = np.array([S1, with_reserved(S1, 2, 9), M1, D1, with_reserved(D1, 4, 7), R1], dtype=recs.dtype); list_of = [-1, -1, -1, 0, 1, -1]; lists = [(0, 16), (0, 15)]
    c = e.ProofCache(1 << 12); assert z.VerifyRecordsCached(c, block) == (6, [True] * 6) and c.stats() == (0, 6, 6, 6)
    sc, su = z.SnSetNew(bytes(32)), z.SnSetNew(bytes(32)); before = counters(e, tmp); want = [[True, False, True, True, False, True], [True, False, True, True, False, True], [False] * 6, [False] * 6]
    for step, commit in enumerate((False, True, True, False)):
        got = z.VerifyBlockFullCached(c, block, leaves, lists, list_of, sc, commit); assert counters(e, tmp) == before and c.stats() == (6 * (step + 1), 6, 6, 6)
        ref = z.VerifyBlockFull(block, leaves, lists, list_of, su, commit); before = counters(e, tmp)
        assert got == ref and got[1] == want[step] and got[2] == (0 if step == 0 else 4), (step, got, ref)
    sn, s2 = z.SnSetNew(bytes(32)), z.SnSetNew(bytes(32))
    for commit in (False, True, True): assert z.VerifyBlockFullCached(None, block, leaves, lists, list_of, sn, commit) == z.VerifyBlockFull(block, leaves, lists, list_of, s2, commit)
    assert z.VerifyBlockFullCached(c, block, leaves, lists, list_of, None, True) == z.VerifyBlockFull(block, leaves, lists, list_of, None, True) == (5, [True, True, True, True, False, True], None)
    for s in (sc, su, sn, s2): z.SnSetFree(s)

def leg_clear(tmp):
    from blockmaze_amd import engine as e
    z, recs, _ = base(tmp); block = twin_block(recs); n = len(block); want = z.VerifyBlockRecords(block); c = z.ProofCacheNew(1 << 12); assert c and z.ProofCacheNew(1) is None
    assert z.VerifyRecordsCached(c, block) == want; h, m, ins, held = z.ProofCacheStats(c); assert (h, m) == (0, n - 2) and ins == held > 0
    assert z.ProofCacheClear(c) == 0 and z.ProofCacheStats(c) == (h, m, ins, 0)
    assert z.VerifyRecordsCached(c, block) == want and z.ProofCacheStats(c) == (0, 2 * (n - 2), 2 * ins, held)                # all misses again, the same verdicts
    assert z.VerifyRecordsCached(c, block) == want and z.ProofCacheStats(c)[0] == want[0]; z.ProofCacheFree(c)

def leg_threads(tmp):
    """four threads on overlapping blocks of 100 records beside a prover: every verdict the uncached one, every accepted record stored once"""
    from blockmaze_amd import engine as e
    import workload as w
    z, recs, _ = base(tmp); pool = []
    for i in range(160):
        r = with_reserved(recs[i % 6], i % 7, 1 + i // 6)
        if i % 5 == 4: r["args"][0][i % 32] ^= 1                                                   # one in five has a wrong statement
        pool.append(r)
    pool = np.array(pool, dtype=recs.dtype); assert distinct(pool) == 160; rc0, ok0 = z.VerifyBlockRecords(pool); assert rc0 == 128
    c = e.ProofCache(1 << 12); errors = []; made = []
    def verifier(t):
        try:
            for k in range(4):
                lo = 20 * ((t + k) % 4); got = z.VerifyRecordsCached(c, pool[lo:lo + 100])
                if got != (sum(ok0[lo:lo + 100]), ok0[lo:lo + 100]): errors.append(("verdicts", t, k))
        except Exception as ex: errors.append(("verifier", t, repr(ex)))
    def prover():
        try:
            for i in (5, 6): d = w.mint_instance(i); made.append((z.GenMintProof(*w.mint_args(d)), d))
        except Exception as ex: errors.append(("prover", repr(ex)))
    ths = [threading.Thread(target=verifier, args=(t,)) for t in range(4)] + [threading.Thread(target=prover)]
    for t in ths: t.start()
    for t in ths: t.join()
    assert not errors, errors[:5]
    assert len(made) == 2 and all(z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]) for p, d in made)
    h, m, ins, held = c.stats(); assert ins == held == 128 and h + m == 1600, c.stats()
    assert z.VerifyRecordsCached(c, pool) == (rc0, ok0) and c.stats()[0] == h + 128

LEGS = {"make": leg_make, "digest": leg_digest, "verdicts": leg_verdicts, "neighbours": leg_neighbours, "keys": leg_keys, "generations": leg_generations, "chain": leg_chain, "clear": leg_clear,
        "threads": leg_threads}

def run_leg(name, tmp, timeout=300):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ZK_PRFKEY_DIR=os.path.join(str(tmp), "A")))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

@pytest.fixture(scope="module")
def made(tmp_path_factory):
    d = tmp_path_factory.mktemp("proof_cache"); run_leg("make", d, 600); return d

def test_digest_kernel_equals_host_model_and_hashlib(tmp_path): run_leg("digest", tmp_path)
def test_same_verdicts_fewer_verifications(made): run_leg("verdicts", made)
def test_neighbour_of_a_stored_record_is_never_a_hit(made): run_leg("neighbours", made)
def test_verifying_key_is_part_of_the_key(made): run_leg("keys", made)
def test_generations_follow_the_model(made): run_leg("generations", made)
def test_chain_state_is_not_cached(made): run_leg("chain", made)
def test_clear_forgets_every_record(made): run_leg("clear", made)
def test_threads_on_one_cache_beside_a_prover(made): run_leg("threads", made)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
