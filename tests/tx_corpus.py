"""Transactions for the tests of include/zk_txs.h: valid ones over every shape the walk and the two hashes distinguish, and a seeded corpus of refusals built by
mutators from valid ones.  Each mutator names the rule it breaks and the status the reference's Sender would end with; tests/test_txs_cpu.py holds every one of
them to that claim with the model (tests/tx_model.py), and tests/test_gpu_txs.py holds the device to the model."""
import random
import secp_model as sm
import tx_model as t

N = sm.N
SIGNERS = (t.FRONTIER, t.HOMESTEAD, t.EIP155)
CHAIN_IDS = (0, 1, 127, 128, 255, 256, 2**62 - 1)
PAYLOAD_LENGTHS = (0, 55, 56, 255, 256, 65535, 65536)

def rand_tx(rng, **kw):
    """a transaction with every field in use, of about the size of a send (a 512-character ZKProof)"""
    tx = t.default_tx(Code=rng.randrange(6), AccountNonce=rng.randrange(2**20), Price=rng.randrange(2**40), GasLimit=rng.randrange(1, 2**24), Recipient=rng.randbytes(20),
                      Amount=rng.randrange(2**70), Payload=rng.randbytes(rng.randrange(0, 80)), ZKValue=rng.randrange(2**64), ZKSN=rng.randbytes(32), ZKSNS=rng.randbytes(32),
                      ZKNounce=rng.randrange(2**32), ZKAdrress=rng.randbytes(20), ZKCMT=rng.randbytes(32), ZKCMTS=rng.randbytes(32), ZKProof=rng.randbytes(256).hex().encode(),
                      RTcmt=rng.randbytes(32), CMTBlock=[rng.randrange(2**64) for _ in range(rng.randrange(4))], AUX=rng.randbytes(rng.randrange(0, 40)), X=rng.getrandbits(256), Y=rng.getrandbits(256),
                      DepositTxV=rng.randrange(2), DepositTxR=rng.getrandbits(256), DepositTxS=rng.getrandbits(256), V=27 + rng.randrange(2), R=rng.randrange(1, N), S=rng.randrange(1, N // 2))
    tx.update(kw); return tx
def v_for(signer, chain_id, parity, protect=True):
    return 35 + 2 * chain_id + parity if (signer == t.EIP155 and protect) else 27 + parity

def with_length_mod(rng, which, residue, signer, chain_id):
    """a transaction whose signing message (which = 'sig') or own encoding (which = 'tx') has a length of `residue` mod 136"""
    tx = rand_tx(rng, V=v_for(signer, chain_id, 1))
    for extra in range(300):
        if which == "sig":
            tx["Payload"] = bytes(60 + extra); six = t.encode_items(tx)[1:7]
            if signer == t.EIP155: six += [t.enc_int(chain_id), b"\x80", b"\x80"]
            if len(t.enc_list(six)) % 136 == residue: return tx
        else:
            tx["AUX"] = bytes(60 + extra)
            if len(t.encode(tx)) % 136 == residue: return tx
    raise AssertionError("no such length")

def valid_cases(seed=22):
    """[(label, raw, signer, chain_id)]: every shape the issue lists; R and S are random numbers — the walk and the hashes do not care, and the recovery has tests of its own"""
    rng = random.Random(seed); out = []
    def put(label, tx, signer, chain_id, **kw): out.append((label, t.encode(tx, **kw), signer, chain_id))
    for L in PAYLOAD_LENGTHS:
        for signer in SIGNERS: put("payload %d" % L, rand_tx(rng, Payload=rng.randbytes(L), V=v_for(signer, 1, L & 1)), signer, 1)
    for byte in (0x00, 0x7F, 0x80, 0xFF): put("payload one byte", rand_tx(rng, Payload=bytes([byte]), V=v_for(t.EIP155, 5, 0)), t.EIP155, 5)
    for which in ("sig", "tx"):
        for residue in (135, 0, 1):
            for signer in (t.HOMESTEAD, t.EIP155): put("%s %d mod 136" % (which, residue), with_length_mod(rng, which, residue, signer, 300), signer, 300)
    for signer in SIGNERS:
        put("recipient 0x80", rand_tx(rng, Recipient=None, V=v_for(signer, 1, 0)), signer, 1)
        put("recipient 0xC0", rand_tx(rng, Recipient=None, V=v_for(signer, 1, 1)), signer, 1, nil_as_list=True)
        for k in (0, 1, 3): put("cmtblock %d" % k, rand_tx(rng, CMTBlock=[rng.randrange(1, 2**64) for _ in range(k)], V=v_for(signer, 1, 1)), signer, 1)
        for code in range(6): put("code %d" % code, rand_tx(rng, Code=code, V=v_for(signer, 1, code & 1)), signer, 1)
        put("all zero", t.default_tx(V=v_for(signer, 1, 0), R=1, S=1), signer, 1)
    for cid in CHAIN_IDS:
        for parity in (0, 1):
            put("chain id %d" % cid, rand_tx(rng, V=v_for(t.EIP155, cid, parity)), t.EIP155, cid)
            put("chain id %d, unprotected" % cid, rand_tx(rng, V=27 + parity), t.EIP155, cid)
        put("chain id %d, wrong" % cid, rand_tx(rng, Code=(0, 1, 2, 4, 5)[cid % 5], V=v_for(t.EIP155, cid + 1, 0)), t.EIP155, cid)   # (a deposit's V is never looked at)
    put("deposit with a wide V", rand_tx(rng, Code=3, V=2**70, R=2**256, S=0), t.EIP155, 1)
    put("deposit with a wrong id", rand_tx(rng, Code=3, V=41), t.HOMESTEAD, 1)
    return out

# ---- the refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
IDX = {name: k for k, (name, _) in enumerate(t.FIELDS)}
def relist(items): return t.enc_list(items)
def swap(items, name, enc): items = list(items); items[IDX[name]] = enc; return relist(items)
def long_head(base, size, width): return bytes([base + 55 + width]) + size.to_bytes(width, "big")

def malformed_mutators():
    """[(rule, fn(items, raw, rng) -> bytes)]: every rule of zk_txs.h's MALFORMED list"""
    M = []
    M.append(("truncated by one byte", lambda it, raw, r: raw[:-1]))
    M.append(("surplus of one byte", lambda it, raw, r: raw + b"\x00"))
    M.append(("24 items", lambda it, raw, r: relist(it[:24])))
    M.append(("25 items", lambda it, raw, r: relist(it[:25])))
    M.append(("27 items", lambda it, raw, r: relist(it + [b"\x80"])))
    M.append(("long-form string size below 56", lambda it, raw, r: swap(it, "Payload", long_head(0x80, 5, 1) + bytes(range(1, 6)))))
    M.append(("long-form list size below 56", lambda it, raw, r: swap(it, "CMTBlock", long_head(0xC0, 2, 1) + b"\x01\x02")))
    M.append(("leading zero in a string size", lambda it, raw, r: swap(it, "Payload", long_head(0x80, 100, 2) + bytes(100))))
    M.append(("leading zero in the outer size", lambda it, raw, r: long_head(0xC0, len(b"".join(it)), 3 if len(b"".join(it)) < 65536 else 4) + b"".join(it)))
    M.append(("leading zero in a uint8", lambda it, raw, r: swap(it, "Code", b"\x81\x00")))
    M.append(("leading zero in a uint64", lambda it, raw, r: swap(it, "AccountNonce", b"\x82\x00\x05")))
    M.append(("leading zero in a big.Int", lambda it, raw, r: swap(it, "Price", b"\x82\x00\x05")))
    M.append(("leading zero in V", lambda it, raw, r: swap(it, "V", b"\x82\x00\x1b")))
    M.append(("0x00 as a uint8", lambda it, raw, r: swap(it, "Code", b"\x00")))
    M.append(("0x00 as a uint64", lambda it, raw, r: swap(it, "GasLimit", b"\x00")))
    M.append(("0x00 as a big.Int", lambda it, raw, r: swap(it, "Amount", b"\x00")))
    M.append(("uint64 of 9 bytes", lambda it, raw, r: swap(it, "ZKValue", b"\x89\x01" + bytes(8))))
    M.append(("Code of 2 bytes", lambda it, raw, r: swap(it, "Code", b"\x82\x01\x00")))
    M.append(("0x81 0x05 as a uint", lambda it, raw, r: swap(it, "ZKNounce", b"\x81\x05")))
    M.append(("0x81 0x05 as a big.Int", lambda it, raw, r: swap(it, "X", b"\x81\x05")))
    M.append(("0x81 0x05 as a string", lambda it, raw, r: swap(it, "AUX", b"\x81\x05")))
    M.append(("hash of 31 bytes", lambda it, raw, r: swap(it, "ZKSN", t.enc_str(bytes(30) + b"\x01"))))
    M.append(("hash of 33 bytes", lambda it, raw, r: swap(it, "RTcmt", t.enc_str(bytes(33)))))
    M.append(("hash of no bytes", lambda it, raw, r: swap(it, "ZKCMT", b"\x80")))
    M.append(("address of 19 bytes", lambda it, raw, r: swap(it, "ZKAdrress", t.enc_str(b"\x01" * 19))))
    M.append(("address of 21 bytes", lambda it, raw, r: swap(it, "ZKAdrress", t.enc_str(b"\x01" * 21))))
    M.append(("recipient of 19 bytes", lambda it, raw, r: swap(it, "Recipient", t.enc_str(b"\x01" * 19))))
    M.append(("recipient of 21 bytes", lambda it, raw, r: swap(it, "Recipient", t.enc_str(b"\x01" * 21))))
    M.append(("recipient a single byte", lambda it, raw, r: swap(it, "Recipient", b"\x05")))
    M.append(("recipient a list of one", lambda it, raw, r: swap(it, "Recipient", b"\xc1\x80")))
    M.append(("list where a string belongs", lambda it, raw, r: swap(it, "Payload", b"\xc0")))
    M.append(("list where a hash belongs", lambda it, raw, r: swap(it, "ZKCMTS", b"\xe0" + bytes(32))))
    M.append(("list where a big.Int belongs", lambda it, raw, r: swap(it, "S", b"\xc0")))
    M.append(("list where a uint belongs", lambda it, raw, r: swap(it, "AccountNonce", b"\xc0")))
    M.append(("string where the list belongs", lambda it, raw, r: swap(it, "CMTBlock", b"\x80")))
    M.append(("the transaction a string", lambda it, raw, r: t.enc_str(b"".join(it))))
    M.append(("the transaction a single byte", lambda it, raw, r: b"\x05"))
    M.append(("CMTBlock holds a list", lambda it, raw, r: swap(it, "CMTBlock", b"\xc1\xc0")))
    M.append(("CMTBlock holds 9 bytes", lambda it, raw, r: swap(it, "CMTBlock", t.enc_list([b"\x89\x01" + bytes(8)]))))
    M.append(("CMTBlock holds 0x00", lambda it, raw, r: swap(it, "CMTBlock", b"\xc1\x00")))
    M.append(("CMTBlock element past its list", lambda it, raw, r: swap(it, "CMTBlock", b"\xc2\x82\x01")))
    M.append(("inner length past the outer list", lambda it, raw, r: relist(it[:25] + [b"\xa0" + b"\x01" * 31])))
    M.append(("inner size header past the outer list", lambda it, raw, r: relist(it[:25] + [b"\xb9\x01"])))
    M.append(("inner length of 2^32", lambda it, raw, r: swap(it, "Payload", long_head(0x80, 2**32, 5) + bytes(8))))
    M.append(("inner length of 2^63", lambda it, raw, r: swap(it, "ZKProof", long_head(0x80, 2**63, 8) + bytes(8))))
    M.append(("outer length of 2^63", lambda it, raw, r: long_head(0xC0, 2**63, 8) + b"".join(it)))
    M.append(("empty transaction", lambda it, raw, r: b""))
    return M

def big_of(nbytes, rng): return int.from_bytes(b"\x01" + rng.randbytes(nbytes - 1), "big")
def signature_cases(rng):
    """[(rule, tx, signer, chain_id)]: transactions that decode and that the signers refuse (or, for the V that is in range, accept)"""
    out = []
    for signer in SIGNERS:
        for v in (0, 26, 29, 34, 35, 36): out.append(("V = %d" % v, rand_tx(rng, Code=rng.choice((0, 1, 2, 4, 5)), V=v), signer, 0))
        for v in (35, 36, 37, 38): out.append(("V = %d, id 1" % v, rand_tx(rng, Code=0, V=v), signer, 1))
        for nb in (2, 8, 9, 33): out.append(("V of %d bytes" % nb, rand_tx(rng, Code=2, V=big_of(nb, rng)), signer, 1))
        out.append(("V of 8 bytes that wraps", rand_tx(rng, Code=2, V=2**64 - 1), signer, 2**62 - 1))
        out.append(("R of 33 bytes", rand_tx(rng, Code=1, R=big_of(33, rng), V=v_for(signer, 9, 0)), signer, 9))
        out.append(("S of 33 bytes", rand_tx(rng, Code=1, S=big_of(33, rng), V=v_for(signer, 9, 1)), signer, 9))
        out.append(("R = 0", rand_tx(rng, Code=4, R=0, V=v_for(signer, 9, 1)), signer, 9))
        out.append(("S above N / 2", rand_tx(rng, Code=5, S=N // 2 + 1 + rng.randrange(N // 4), V=v_for(signer, 9, 0)), signer, 9))
        out.append(("R of 33 bytes and a wrong id", rand_tx(rng, Code=0, R=big_of(33, rng), V=v_for(t.EIP155, 8, 0)), signer, 9))
    return out

def refusal_corpus(seed=23, bases=6):
    """[(rule, claimed status of zkTxSenders or None where the model alone decides, raw, signer, chain_id)]"""
    rng = random.Random(seed); out = []; muts = malformed_mutators()
    for k in range(bases):
        signer = SIGNERS[k % 3]; chain_id = (1, 77, 2**40)[k // 3 % 3]; tx = rand_tx(rng, V=v_for(signer, chain_id, k & 1), Code=k % 6)
        if k == 1: tx["Payload"] = rng.randbytes(70000)                                            # a four-byte outer size
        tx = t.sign_tx(tx, signer, chain_id, rng.randrange(1, 2**20), rng.randrange(1, 2**20))
        items = t.encode_items(tx); raw = t.encode(tx); out.append(("valid", t.OK, raw, signer, chain_id))
        for rule, fn in muts: out.append((rule, t.MALFORMED, fn(items, raw, rng), signer, chain_id))
    for rule, tx, signer, chain_id in signature_cases(rng): out.append((rule, None, t.encode(tx), signer, chain_id))
    return out

def signed_cases(seed=24, count=36):
    """[(raw, signer, chain_id, the sender the reference would return, status)]: transactions signed under known keys (small keys and nonces: the model's
    multiplications stay short), deposits with any V, R, S, and refused records between them"""
    rng = random.Random(seed); out = []
    for k in range(count):
        signer = SIGNERS[k % 3]; chain_id = (0, 1, 1337, 2**62 - 1)[k % 4]; key = rng.randrange(1, 2**20); nonce = rng.randrange(1, 2**20)
        tx = t.sign_tx(rand_tx(rng, Code=(0, 1, 2, 4, 5)[k % 5], Recipient=None if k % 7 == 0 else rng.randbytes(20)), signer, chain_id, key, nonce)
        out.append((t.encode(tx, nil_as_list=(k % 14 == 0)), signer, chain_id, sm.address(sm.mul(key, sm.G)), t.OK))
        if k % 6 == 1: dep = rand_tx(rng, Code=3, V=rng.choice((0, 27, 41, 2**80)), R=rng.choice((0, 5, 2**257)), S=rng.randrange(N)); out.append((t.encode(dep), signer, chain_id, dep["ZKAdrress"], t.OK))
        if k % 6 == 2: out.append((t.encode(tx)[:-1], signer, chain_id, bytes(20), t.MALFORMED))
        if k % 6 == 3: bad = dict(tx, S=N - tx["S"]); out.append((t.encode(bad), signer, chain_id, None, None))          # high S: refused from Homestead on, another key under Frontier
        if k % 6 == 4: bad = dict(tx, R=0); out.append((t.encode(bad), signer, chain_id, bytes(20), t.SIG))
    return out
