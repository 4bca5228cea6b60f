"""Transactions for the tests of include/zk_bodies.h, beside tests/tx_corpus.py (which stays as it is): deposits signed as the reference's wallet signs them — the
six-field hash, V = 27 / 28, (X, Y) the signing key —, every way the deposit rule refuses one, ZKProof lengths around 512, (X, Y) lengths, start residues mod 8, and
mixes of public, ZK and refused transactions.  Each case names the status it claims; tests/test_bodies_cpu.py holds every one to that claim with the model
(tests/bodies_model.py), and tests/test_gpu_bodies.py holds the device to the model."""
import random
import secp_model as sm
import tx_model as t
import tx_corpus as c
import bodies_model as bm

N = sm.N
ZK_CODES = (1, 2, 3, 5)
PROOF_LENGTHS = (0, 1, 511, 512, 513, 600)

def hexproof(rng, n): return rng.randbytes((n + 1) // 2).hex().encode()[:n]
def sign_deposit(tx, key, nonce, xy_key=None):
    """a deposit as SendDepositTx builds it: (X, Y) the receiver's public key, the signature HomesteadSigner's over the six-field hash (V = 27 / 28), by that key"""
    tx = dict(tx, Code=3); pt = sm.mul(key if xy_key is None else xy_key, sm.G); tx["X"], tx["Y"] = pt
    sig = sm.sign(bm.six_field_hash(tx), key, nonce); tx["R"] = int.from_bytes(sig[:32], "big"); tx["S"] = int.from_bytes(sig[32:64], "big"); tx["V"] = 27 + sig[64]; return tx
def signed(rng, signer, chain_id, **kw):
    """a transaction of any code, signed so that it has a sender: a deposit by its own rule, the others by the call's signer"""
    tx = c.rand_tx(rng, **kw); key = rng.randrange(1, 2**20); nonce = rng.randrange(1, 2**20)
    return sign_deposit(tx, key, nonce) if tx["Code"] == 3 else t.sign_tx(tx, signer, chain_id, key, nonce)
def short_coordinate_key(which, start=1, limit=20000):
    """the first key from `start` on whose public X (which = 0) or Y (1) has a leading zero byte: a seeded search, one point addition a step (one key in 256 has one)"""
    pt = sm.mul(start, sm.G)
    for key in range(start, start + limit):
        if pt[which] < 2**248: return key
        pt = sm.add(pt, sm.G)
    raise AssertionError("no key with a short coordinate")

def deposit_cases(seed=31):
    """[(label, claimed status, raw, signer, chain_id)]: the deposit rule of zk_bodies.h, every refused case from a deposit that is accepted"""
    rng = random.Random(seed); out = []
    def put(label, claim, tx, signer, chain_id): out.append((label, claim, t.encode(tx), signer, chain_id))
    for signer, chain_id in ((t.FRONTIER, 0), (t.HOMESTEAD, 1), (t.EIP155, 1), (t.EIP155, 2**40)):
        key, nonce = rng.randrange(1, 2**20), rng.randrange(1, 2**20); good = sign_deposit(c.rand_tx(rng), key, nonce); tag = " / signer %d id %d" % (signer, chain_id)
        put("valid" + tag, t.OK, good, signer, chain_id)
        put("the wrong key" + tag, bm.DEPOSIT_KEY, sign_deposit(good, key, nonce, xy_key=key + 1), signer, chain_id)
        put("X of 33 bytes" + tag, bm.DEPOSIT_KEY, dict(good, X=good["X"] + 2**256), signer, chain_id)
        put("Y of 33 bytes" + tag, bm.DEPOSIT_KEY, dict(good, Y=good["Y"] + 2**256), signer, chain_id)
        put("a high s" + tag, bm.DEPOSIT_KEY, dict(good, S=N - good["S"], V=55 - good["V"]), signer, chain_id)     # the same key under Frontier's rule: refused all the same
        put("V = 37" + tag, bm.DEPOSIT_KEY, dict(good, V=37), signer, chain_id)                                     # a protected V: HomesteadSigner does no chain-id arithmetic
        put("V = 0x0100" + tag, bm.DEPOSIT_KEY, dict(good, V=0x0100), signer, chain_id)
        put("V = 0" + tag, bm.DEPOSIT_KEY, dict(good, V=0), signer, chain_id)
        put("the other parity" + tag, bm.DEPOSIT_KEY, dict(good, V=55 - good["V"]), signer, chain_id)
        put("R = 0" + tag, bm.DEPOSIT_KEY, dict(good, R=0), signer, chain_id)
        put("R of 33 bytes" + tag, bm.DEPOSIT_KEY, dict(good, R=good["R"] + 2**256), signer, chain_id)
        put("S of 33 bytes" + tag, bm.DEPOSIT_KEY, dict(good, S=good["S"] + 2**256), signer, chain_id)
        put("another payload" + tag, bm.DEPOSIT_KEY, dict(good, Payload=good["Payload"] + b"\x01"), signer, chain_id)   # the six-field hash moves, the key with it
    # a deposit signed over the nine-field hash, as an EIP155 wallet would sign any other transaction: the reference never forms that hash for a deposit
    key, nonce = rng.randrange(1, 2**20), rng.randrange(1, 2**20); tx = c.rand_tx(rng, Code=3); tx["X"], tx["Y"] = sm.mul(key, sm.G)
    put("signed over nine fields", bm.DEPOSIT_KEY, t.sign_tx(tx, t.EIP155, 5, key, nonce), t.EIP155, 5)
    return out
def xy_length_cases(seed=32):
    """[(label, claimed status, raw, signer, chain_id)]: X and Y of 0, 1, 31 and 32 bytes.  32: any key.  31: the accepted case needs a key whose coordinate has a
    leading zero byte, found by search; a 31-byte coordinate under any other key is refused.  0 and 1 byte: no key has such a coordinate that a search could find, so
    only the refused side is held (the padding still decides the address that is compared)."""
    rng = random.Random(seed); out = []
    def put(label, claim, tx): out.append((label, claim, t.encode(tx), t.HOMESTEAD, 1))
    for which, name in ((0, "X"), (1, "Y")):
        key = short_coordinate_key(which, 1 + 7000 * which); good = sign_deposit(c.rand_tx(rng), key, rng.randrange(1, 2**20)); assert good[name].bit_length() <= 248 and good["XY"[1 - which]].bit_length() > 248
        put("%s of 31 bytes, accepted" % name, t.OK, good)
        put("%s of 31 bytes, one bit off" % name, bm.DEPOSIT_KEY, dict(good, **{name: good[name] ^ 1}))
        base = sign_deposit(c.rand_tx(rng), rng.randrange(1, 2**20), rng.randrange(1, 2**20)); assert base[name].bit_length() > 248
        put("%s of 32 bytes" % name, t.OK, base)
        for nbytes in (0, 1, 31): put("%s of %d bytes, refused" % (name, nbytes), bm.DEPOSIT_KEY, dict(base, **{name: base[name] >> (8 * (32 - nbytes))}))
    return out
def proof_length_cases(seed=33):
    """[(label, OK, raw, signer, chain_id)]: ZKProof of 0, 1, 511, 512, 513 and 600 characters under every ZK code"""
    rng = random.Random(seed); out = []
    for L in PROOF_LENGTHS:
        for code in ZK_CODES: out.append(("proof %d, code %d" % (L, code), t.OK, t.encode(signed(rng, t.EIP155, 9, Code=code, ZKProof=hexproof(rng, L))), t.EIP155, 9))
    return out
def alignment_cases(seed=34, signer=t.HOMESTEAD, chain_id=0):
    """[raw]: 16 pairs (a public filler, a ZK transaction).  The filler's length makes the ZK transaction start at every residue mod 8 of the upload, and its Payload's
    length moves its ZKProof over every residue mod 8 inside it; the assertion below says that all eight are met for both."""
    rng = random.Random(seed); raws = []; starts, proofs = set(), set(); at = 0
    for k in range(16):
        zk = t.encode(signed(rng, signer, chain_id, Code=ZK_CODES[k % 4], Payload=rng.randbytes(20 + k // 2)))
        base = signed(rng, signer, chain_id, Code=0, ZKProof=b"", AUX=b"")                          # (AUX is in no signing hash: it may change under the signature)
        for extra in range(12):
            fill = t.encode(dict(base, AUX=bytes(extra)))
            if (at + len(fill)) % 8 == k % 8: break
        else: raise AssertionError("no filler")
        raws += [fill, zk]; at += len(fill); tx, spans = t.decode(zk); pbeg = spans[14][1] - len(tx["ZKProof"])
        starts.add(at % 8); proofs.add((at + pbeg) % 8); at += len(zk)
    assert starts == set(range(8)) and proofs == set(range(8)), (starts, proofs)
    return raws

class Pool:
    """a few signed transactions of each class, reused to build bodies of any size: the model decides each distinct transaction once"""
    def __init__(self, seed=35, signer=t.EIP155, chain_id=7, each=3):
        rng = random.Random(seed); self.signer, self.chain_id = signer, chain_id
        self.public = [t.encode(signed(rng, signer, chain_id, Code=(0, 4)[k % 2], ZKProof=b"")) for k in range(each)]
        self.zk = [t.encode(signed(rng, signer, chain_id, Code=ZK_CODES[k % 4])) for k in range(max(each, 4))]
        self.refused = [t.encode(signed(rng, signer, chain_id, Code=1))[:-1],                                                  # MALFORMED
                        t.encode(dict(signed(rng, signer, chain_id, Code=2), R=0)),                                           # SIG
                        t.encode(dict(signed(rng, signer, chain_id, Code=3), V=37)),                                          # DEPOSIT_KEY
                        t.encode(signed(rng, t.EIP155, chain_id + 1, Code=5))]                                                # CHAIN_ID under EIP155
    def body(self, pattern):
        """pattern: a string of p (public), z (ZK), r (refused), one character a transaction"""
        count = {"p": 0, "z": 0, "r": 0}; src = {"p": self.public, "z": self.zk, "r": self.refused}; out = []
        for ch in pattern: out.append(src[ch][count[ch] % len(src[ch])]); count[ch] += 1
        return out
