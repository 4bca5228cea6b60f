"""The seeded mutants of tests/mutants.py on the device: k_tx_walk, k_hdr_walk and the split's two walks (csrc/gpu_txs.hip) against their models
byte for byte on every output of every mutant, with no tolerance — 6,000 transactions, twelve chains of 257 headers in which every second header is a mutant, 6,000
bodies; every decoder once more with each mutant between two copies of its base, whose outputs must be what they are without it.  tests/test_mutants_cpu.py states what
these inputs reach.  The models' hashes come from the device's plain one-range sponge (engine.keccak256, which tests/test_gpu_txs.py holds against the Python sponge at
every length to 300 and at the block edges), many messages a call; a seeded sample of 64 transactions and 64 headers is hashed by the Python sponge as well."""
import os, random, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import tx_model as t
import header_model as hm
import header_corpus as hc
import body_model as bdm
import bodies_model as bm
import mutants as mu

pytestmark = pytest.mark.gpu
NO_HASH = lambda msg: bytes(32)                                  # a transaction's status and code do not depend on its hashes

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    engine.init(); return engine

# ---- the models' hash function ------------------------------------------------------------------------------------------------------------------------------------------
class Sponge:
    """keccak for the models: the device's sponge, remembered a message.  A model is run twice: first with `collect`, which hands back zeros and notes the messages (no
    verdict but a header's ANCESTOR, TIMESTAMP and SEAL depends on a hash, and those come behind every message), then, the noted messages hashed in one call, with the
    object itself."""
    def __init__(self, e): self.e = e; self.memo = {}; self.noted = []
    def collect(self, msg): self.noted.append(bytes(msg)); return bytes(32)
    def flush(self):
        miss = sorted(set(m for m in self.noted if m not in self.memo)); self.noted = []
        if miss: self.memo.update(zip(miss, self.e.keccak256(miss)))
    def __call__(self, msg):
        msg = bytes(msg)
        if msg not in self.memo: self.memo[msg] = self.e.keccak256([msg])[0]
        return self.memo[msg]
@pytest.fixture(scope="module")
def sponge(e): return Sponge(e)

# ---- transactions -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def txs(sponge):
    """[(label, mutant, signer, chain_id, base, the model's signing inputs)]"""
    muts = mu.tx_mutants(mu.TX_SEED, mu.TX_COUNT)
    for x in muts: t.signing_inputs(x[1], x[2], x[3], sponge.collect)
    sponge.flush(); return [x + (t.signing_inputs(x[1], x[2], x[3], sponge),) for x in muts]
def grouped(cases):
    g = {}
    for x in cases: g.setdefault((x[2], x[3]), []).append(x)
    return sorted(g.values(), key=len)
def inputs_rows(o, n): return [dict(status=int(o["status"][k]), code=int(o["code"][k]), txhash=bytes(o["txhash"][k]), sighash=bytes(o["sighash"][k]), sig=bytes(o["sigs"][k]), deposit_from=bytes(o["deposit_from"][k])) for k in range(n)]
def check_inputs(e, raws, signer, chain_id, want, labels, lead=b""):
    """zkgpu_tx_signing_inputs on raws (behind a filler transaction of the bytes `lead`, which moves every other one in the upload) against `want`, every output"""
    rc, o = e.tx_signing_inputs(([lead] if lead else []) + list(raws), signer, chain_id); skip = 1 if lead else 0; got = inputs_rows(o, len(raws) + skip)
    assert rc == sum(w["status"] == t.OK for w in want), (rc, e.lib().zkgpu_last_error())
    for k, (g, w) in enumerate(zip(got[skip:], want)): assert g == w, (labels[k], k, raws[k].hex()[:400], {f: (g[f], w[f]) for f in g if g[f] != w[f]})
    if lead: assert got[0]["status"] == t.MALFORMED and not any(got[0]["txhash"] + got[0]["sig"])

def test_transactions_every_output_of_every_mutant(e, txs):
    seen = {k: 0 for k in (t.OK, t.MALFORMED, t.CHAIN_ID, t.SIG)}; assert len(txs) == mu.TX_COUNT
    for group in grouped(txs):
        check_inputs(e, [x[1] for x in group], group[0][2], group[0][3], [x[5] for x in group], [x[0] for x in group])
        for x in group: seen[x[5]["status"]] += 1
    assert all(seen.values()) and 5 * seen[t.MALFORMED] >= len(txs) and 5 * (len(txs) - seen[t.MALFORMED]) >= len(txs), seen

@pytest.mark.parametrize("lead", range(1, 8))
def test_the_largest_group_behind_one_to_seven_filler_bytes(e, txs, lead):
    group = grouped(txs)[-1]; assert len(group) >= 500
    check_inputs(e, [x[1] for x in group], group[0][2], group[0][3], [x[5] for x in group], [x[0] for x in group], lead=bytes([0x80 + lead - 1]) + bytes(lead - 1))

def test_senders_and_records_of_a_subset_of_decodable_mutants(e, txs, sponge):
    """zkgpu_tx_senders against tx_model.sender and zkgpu_tx_records against bodies_model.records on at most 256 decodable mutants of the largest group (the model's
    recovery is Python's): the walk's second instantiation, with the positions of the ZK fields, on inputs nobody chose"""
    group = grouped(txs)[-1]; signer, chain_id = group[0][2:4]; pool = [x for x in group if x[5]["status"] != t.MALFORMED and len(x[1]) < 4000]
    sub = random.Random(11).sample(pool, min(256, len(pool))); raws = [x[1] for x in sub]; assert len(sub) >= 100 and len({len(r) for r in raws}) >= 20
    rc, o = e.tx_senders(raws, signer, chain_id); want = [t.sender(r, signer, chain_id, sponge) for r in raws]
    for k, w in enumerate(want): assert (int(o["status"][k]), int(o["code"][k]), bytes(o["txhash"][k]), bytes(o["froms"][k])) == w, (sub[k][0], k, int(o["status"][k]), w[0])
    assert rc == sum(w[0] == t.OK for w in want)
    rc, o = e.tx_records(raws, signer, chain_id); recs, rec_froms, rec_of, froms, code, status, txhash = bm.records(raws, signer, chain_id, sponge); n, m = len(raws), len(recs)
    assert rc == m and m >= 20, (rc, m, e.lib().zkgpu_last_error())
    assert list(o["status"]) == status and list(o["code"]) == code and list(o["rec_of"]) == rec_of, [(sub[i][0], int(o["status"][i]), status[i]) for i in range(n) if o["status"][i] != status[i]][:5]
    assert o["froms"].tobytes() == b"".join(froms) and o["txhash"].tobytes() == b"".join(txhash) and o["rec_froms"].tobytes() == b"".join(rec_froms) + bytes(20 * (n - m))
    got = o["recs"].tobytes()
    for j in range(m): assert got[720 * j:720 * j + 720] == recs[j], (sub[rec_of.index(j)][0], j, next(k for k in range(720) if got[720 * j + k] != recs[j][k]))
    assert got[720 * m:] == b"\xa5" * (720 * (n - m))                                                # recs[m .. n) is left as it was

def test_a_transaction_mutant_between_two_copies_of_its_base_leaves_them_alone(e, txs):
    group = random.Random(12).sample(grouped(txs)[-1], 600); signer, chain_id = group[0][2:4]; bases = [x[4] for x in group]
    rc0, o0 = e.tx_signing_inputs(bases, signer, chain_id); alone = inputs_rows(o0, len(bases)); assert all(a["status"] != t.MALFORMED for a in alone)   # every base decodes
    rc, o = e.tx_signing_inputs([r for x in group for r in (x[4], x[1], x[4])], signer, chain_id); got = inputs_rows(o, 3 * len(group))
    for k, x in enumerate(group): assert got[3 * k] == alone[k] and got[3 * k + 2] == alone[k] and got[3 * k + 1] == x[5], (x[0], k)
    assert rc == sum(g["status"] == t.OK for g in got) and rc0 == sum(a["status"] == t.OK for a in alone)

# ---- headers ------------------------------------------------------------------------------------------------------------------------------------------------------------
def header_rows(o, n): return [{k: (bytes(o[k][i]) if o[k].ndim == 2 else int(o[k][i])) for k in hm.ZERO} for i in range(n)]
def model_headers(sponge, raws, parent):
    hm.headers(raws, hc.PERIOD, hc.CHAIN_EPOCH, hc.NOW, parent, keccak=sponge.collect); sponge.flush(); return hm.headers(raws, hc.PERIOD, hc.CHAIN_EPOCH, hc.NOW, parent, keccak=sponge)
def check_headers(e, raws, parent, want, start):
    rc, o = e.headers(raws, hc.PERIOD, hc.CHAIN_EPOCH, hc.NOW, parent, start=start); got = header_rows(o, len(raws))
    for i, (g, w) in enumerate(zip(got, want)): assert g == w, (i, start, raws[i].hex(), {f: (g[f], w[f]) for f in g if g[f] != w[f]})
    assert rc == hm.accepted(want), (rc, e.lib().zkgpu_last_error()); return got

@pytest.fixture(scope="module")
def chains(sponge):
    """[(headers, parent, bases, the model's outputs)] a seed"""
    out = []
    for seed in mu.HEADER_SEEDS: raws, parent, bases = mu.header_chains(seed); out.append((raws, parent, bases, model_headers(sponge, raws, parent)))
    return out

def test_headers_every_output_of_every_header_of_twelve_chains(e, chains):
    seen = set(); n = 0
    for raws, parent, bases, want in chains:
        for start in (0, 5): check_headers(e, raws, parent, want, start)
        seen |= {w["status"] for w in want}; n += len(raws)
    assert n == 3084 and len(seen) >= 12 and {hm.OK, hm.MALFORMED, hm.ANCESTOR} <= seen, seen

def test_a_header_mutant_between_two_copies_of_its_base_leaves_them_alone(e, chains, sponge):
    """base, mutant, base for every header of a chain: the whole call against the model — the links are the model's: the first copy stands behind its predecessor's
    second copy, the second behind the mutant — and everything of a copy that is no link against the call on the bases alone"""
    raws, parent, bases, _ = chains[0]; pairs = [(b, r) for b, r in zip(bases, raws) if r != b]; assert len(pairs) >= 100
    rc0, o0 = e.headers(bases, hc.PERIOD, hc.CHAIN_EPOCH, hc.NOW, parent); alone = {b: row for b, row in zip(bases, header_rows(o0, len(bases)))}; assert rc0 == len(bases)
    three = [x for b, r in pairs for x in (b, r, b)]; got = check_headers(e, three, parent, model_headers(sponge, three, parent), 0)
    for k, (b, r) in enumerate(pairs):
        for g in (got[3 * k], got[3 * k + 2]): assert {f: v for f, v in g.items() if f not in ("status", "signer")} == {f: v for f, v in alone[b].items() if f not in ("status", "signer")}, k

# ---- bodies -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bodies(): return mu.body_mutants(mu.BODY_SEED, mu.BODY_COUNT)

def check_split(e, raws, start=0):
    """zkgpu_test_body_split against body_model.split_all: k, n, block_first, body_status, tx_beg, tx_size, the packed bytes and their offsets; the entries beyond n
    (cap = n + 3) keep the fill"""
    s = bdm.split_all(raws, start=start); n = s["n"]; rc, o = e.body_split(raws, cap=n + 3, start=start, packed=True)
    assert rc == s["k"], (rc, s["k"], e.lib().zkgpu_last_error())
    bad = [b for b in range(len(raws)) if int(o["body_status"][b]) != s["body_status"][b]]; assert not bad, [(b, raws[b].hex()[:200], int(o["body_status"][b]), s["body_status"][b]) for b in bad[:5]]
    assert o["n_txs"] == n and list(o["block_first"]) == s["block_first"]
    assert list(o["tx_beg"][:n]) == s["tx_beg"] and list(o["tx_size"][:n]) == s["tx_size"]
    assert o["packed"] == s["packed"] and list(o["packed_off"][:n + 1]) == s["off"]
    assert set(o["tx_beg"][n:].tobytes()) <= {0xA5} and set(o["tx_size"][n:].tobytes()) <= {0xA5} and set(o["packed_off"][n + 1:].tobytes()) <= {0xA5}
    return s

@pytest.mark.parametrize("part", range(4))
def test_bodies_every_output_and_the_packed_transactions_through_the_walk(e, bodies, part):
    per = mu.BODY_COUNT // 4; assert per == 1500
    raws = [x[0] for x in bodies[per * part: per * (part + 1)]]; s = check_split(e, raws, start=part); assert {bdm.OK, bdm.MALFORMED} <= set(s["body_status"]) and s["n"] >= 500
    rc, o = e.tx_signing_inputs(s["txs"], t.EIP155, 1); want = [t.signing_inputs(r, t.EIP155, 1, NO_HASH) for r in s["txs"]]   # the elements of the accepted bodies: transactions, lone bytes and what the mutators left
    assert [int(x) for x in o["status"]] == [w["status"] for w in want] and [int(x) for x in o["code"]] == [w["code"] for w in want] and rc == sum(w["status"] == t.OK for w in want)
    assert len({w["status"] for w in want}) >= 2

def test_a_body_mutant_between_two_copies_of_its_base_leaves_them_alone(e, bodies):
    sub = random.Random(13).sample(bodies, 500); bases = [b for _, b in sub]
    def per_body(o, nb):
        """the transactions of every body, cut out of the packed bytes"""
        f = [int(x) for x in o["block_first"]]; off = [int(x) for x in o["packed_off"][:o["n_txs"] + 1]]
        return [(int(o["body_status"][b]), [o["packed"][off[i]:off[i + 1]] for i in range(f[b], f[b + 1])]) for b in range(nb)]
    s0 = check_split(e, bases); assert s0["k"] == len(bases); rc0, o0 = e.body_split(bases, cap=s0["n"], packed=True); alone = per_body(o0, len(bases))
    three = [x for m, b in sub for x in (b, m, b)]; s = check_split(e, three, start=3); rc, o = e.body_split(three, cap=s["n"], start=3, packed=True); got = per_body(o, len(three))
    for k in range(len(sub)): assert got[3 * k] == alone[k] and got[3 * k + 2] == alone[k], k

# ---- the Python sponge on a sample ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_python_sponge_gives_the_hashes_of_64_transactions_and_64_headers(txs, chains):
    """the road of the hashes above is the device's one-range sponge; here the models hash with tx_model.keccak256 itself"""
    pool = [x for x in txs if x[5]["status"] != t.MALFORMED and len(x[1]) < 1500]; sample = random.Random(14).sample(pool, 64)
    for x in sample: assert t.signing_inputs(x[1], x[2], x[3]) == x[5], x[0]
    assert len({len(x[1]) % 136 for x in sample}) >= 30
    rng = random.Random(15); seen = 0
    for raws, parent, bases, want in chains:
        picks = [i for i in range(len(raws)) if raws[i] != bases[i] and want[i]["status"] != hm.MALFORMED and want[i]["extra_size"] >= hm.SEAL_BYTES]
        for i in rng.sample(picks, 6 if seen < 60 else 4):
            h, spans, contents = hm.decode(raws[i]); assert (hm.header_hash(h), hm.seal_hash(h)) == (want[i]["hash"], want[i]["sealhash"]), i; seen += 1
        if seen >= 64: break
    assert seen == 64
