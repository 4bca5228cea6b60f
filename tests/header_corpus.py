"""Headers for the tests of include/zk_headers.h: chains of linked headers signed by the model, and one case for every status of the header file, each built from a header
the model accepts.  A case is (label, the status it claims or None, the header's bytes, the parent of header 0 or None, the signing key or None); the calls' period,
epoch and clock are PERIOD, EPOCH and NOW for all of them.  EPOCH is 0, so the engine's default of 30000 (clique.go:56) is what decides a checkpoint here."""
import random
import header_model as hm
import secp_model as sm
import tx_model as t

PERIOD, EPOCH, NOW = 15, 0, 1_700_000_000
T0 = 1_600_000_000
CHAIN_SEED, GENESIS_SEED, CHAIN_EPOCH = 7, 9, 8                 # the chains of the device tests: a checkpoint every eight headers
KEYS = [0x1C0DE + 977 * k for k in range(1, 5)]
N, P = sm.N, sm.P

def rand_header(rng, **kw):
    cmt = [rng.randbytes(32) for _ in range(rng.randrange(3))]
    h = hm.default_header(Coinbase=rng.randbytes(20), Root=rng.randbytes(32), TxHash=rng.randbytes(32), ReceiptHash=rng.randbytes(32), Bloom=rng.randbytes(256), GasLimit=rng.randrange(1, 2**40),
                          GasUsed=rng.randrange(2**24), Extra=rng.randbytes(hm.VANITY_BYTES) + bytes(hm.SEAL_BYTES), RTCMT=rng.randbytes(32), CMT=cmt, Difficulty=1 + rng.randrange(2),
                          Nonce=(bytes(8), b"\xff" * 8)[rng.randrange(2)])
    h.update(kw); return h
def checkpoint_fields(rng, signers): return dict(Coinbase=bytes(20), Nonce=bytes(8), Extra=rng.randbytes(hm.VANITY_BYTES) + rng.randbytes(20 * signers) + bytes(hm.SEAL_BYTES))

def chain(seed, n, epoch=8, first=1, t0=T0):
    """n linked headers numbered from `first`, every one accepted under (PERIOD, epoch, NOW) -> (the headers' bytes, the parent of header 0 or None for a genesis at
    index 0, the signers' addresses, zero for a genesis)"""
    rng = random.Random(seed); parent = (rng.randbytes(32), first - 1, t0) if first else None; prev = parent; raws = []; signers = []
    for k in range(n):
        number = first + k; key = KEYS[rng.randrange(len(KEYS))]; kw = checkpoint_fields(rng, rng.randrange(4)) if number % epoch == 0 else {}
        h = rand_header(rng, Number=number, ParentHash=prev[0] if prev else rng.randbytes(32), Time=(prev[2] if prev else t0) + PERIOD + rng.randrange(3), **kw)
        h = hm.sign_header(h, key, rng.randrange(1, N)); raws.append(hm.encode(h)); prev = (hm.header_hash(h), number, h["Time"]); signers.append(hm.signer_address(key) if number else bytes(20))
    return raws, parent, signers

def _no_curve_x():
    r = 1
    while pow(r ** 3 + 7, (P - 1) // 2, P) == 1: r += 1
    return r
def _sig(r, s, v): return r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([v])

def cases(seed=25):
    """every status of zk_headers.h, each case built from an accepted header"""
    rng = random.Random(seed); out = []
    def base(number=5, parent_time=T0, dt=PERIOD, **kw):
        parent = (rng.randbytes(32), (number - 1) & hm.M64, parent_time)
        fields = checkpoint_fields(rng, 2) if number % 30000 == 0 else {}
        fields.update(kw); return rand_header(rng, Number=number, ParentHash=parent[0], Time=(parent_time + dt) & hm.M64, **fields), parent
    def add(label, claim, h, parent, sign=True, items=None, seal=None, raw=None, signer_key=None):
        """sign: seal h with a key of KEYS; seal: these 65 bytes instead; items: a function of the encoded items that returns the header's bytes; raw: these bytes"""
        key = signer_key or (KEYS[len(out) % len(KEYS)] if sign and seal is None else None)
        if key is not None and seal is None and len(h["Extra"]) >= hm.SEAL_BYTES: h = hm.sign_header(h, key, rng.randrange(1, N))
        if seal is not None: h = dict(h, Extra=h["Extra"][:-hm.SEAL_BYTES] + seal)
        if raw is None: raw = items(hm.encode_items(h)) if items else hm.encode(h)
        out.append((label, claim, bytes(raw), parent, key if claim == hm.OK and h["Number"] else None)); return h
    # ---- accepted
    h, p = base(); add("plain", hm.OK, h, p)
    h, p = base(number=0); add("genesis, no parent", hm.OK, dict(h, Difficulty=17), None)
    for k in (0, 1, 12):
        h, p = base(number=30000, **checkpoint_fields(rng, k)); add("checkpoint, %d signers" % k, hm.OK, h, p)
    h, p = base(number=60001, Nonce=b"\xff" * 8); add("vote", hm.OK, h, p)
    h, p = base(parent_time=2**64 - 5); h["Time"] = NOW; add("parent.Time + period wraps", hm.OK, h, p)      # 2^64 - 5 + 15 wraps to 10 <= Time
    for k in (0, 1, 2, 7, 8, 1986):
        h, p = base(CMT=[rng.randbytes(32) for _ in range(k)]); add("CMT of %d" % k, hm.OK, h, p)
    h, p = base(); hs = hm.sign_header(h, KEYS[0], rng.randrange(1, N)); sig = hs["Extra"][-65:]
    add("high s", hm.OK, h, p, seal=_sig(int.from_bytes(sig[:32], "big"), N - int.from_bytes(sig[32:64], "big"), sig[64] ^ 1), signer_key=KEYS[0])
    # ---- malformed (rule 1), each a re-encoding of an accepted header with one thing wrong
    def mal(label, fn):
        h, p = base(CMT=[rng.randbytes(32), rng.randbytes(32)]); add("malformed: " + label, hm.MALFORMED, h, p, items=fn)
    enc = t.enc_list
    def put(k, b): return lambda it: enc(it[:k] + [b(it[k]) if callable(b) else b] + it[k + 1:])
    mal("outer item a string", lambda it: t.head(0x80, len(b"".join(it))) + b"".join(it))
    mal("a byte behind the list", lambda it: enc(it) + b"\x00")
    mal("the list runs past the input", lambda it: enc(it)[:-1])
    mal("16 items", lambda it: enc(it[:16]))
    mal("18 items", lambda it: enc(it + [b"\x80"]))
    mal("outer length with a leading zero", lambda it: b"\xfa\x00" + len(b"".join(it)).to_bytes(2, "big") + b"".join(it))
    mal("long form below 56", put(2, lambda x: b"\xb8\x14" + x[1:]))
    mal("one byte below 0x80 under a header", put(7, b"\x81\x02"))
    for k, name, w in ((0, "ParentHash", 32), (1, "UncleHash", 32), (3, "Root", 32), (4, "TxHash", 32), (5, "ReceiptHash", 32), (13, "MixDigest", 32), (15, "RTCMT", 32), (2, "Coinbase", 20),
                       (6, "Bloom", 256), (14, "Nonce", 8)):
        for d in (-1, 1): mal("%s of %d bytes" % (name, w + d), put(k, t.enc_str(bytes([0x91]) * (w + d))))
    mal("ParentHash a lone byte", put(0, b"\x05")); mal("ParentHash a list", put(0, lambda x: b"\xe0" + x[1:])); mal("Nonce a list", put(14, lambda x: b"\xc8" + x[1:]))
    mal("Coinbase empty", put(2, b"\x80")); mal("Bloom a list", put(6, lambda x: b"\xf9" + x[1:]))
    for k, name in ((7, "Difficulty"), (8, "Number"), (11, "Time")):
        mal(name + " with a leading zero", put(k, b"\x82\x00\x01")); mal(name + " the byte 0x00", put(k, b"\x00")); mal(name + " a list", put(k, b"\xc1\x01"))
    for k, name in ((9, "GasLimit"), (10, "GasUsed")):
        mal(name + " of 9 bytes", put(k, b"\x89" + b"\x01" * 9)); mal(name + " with a leading zero", put(k, b"\x82\x00\x01")); mal(name + " the byte 0x00", put(k, b"\x00"))
        mal(name + " a list", put(k, b"\xc0"))
    mal("Number of 9 bytes", put(8, b"\x89" + b"\x01" * 9))
    mal("Extra a list", put(12, lambda x: b"\xf8" + x[1:]))
    mal("CMT a string", put(16, lambda x: b"\xb8" + x[1:])); mal("CMT element of 31 bytes", put(16, enc([t.enc_str(bytes(31))]))); mal("CMT element of 33 bytes", put(16, enc([t.enc_str(bytes(33))])))
    mal("CMT element a list", put(16, enc([b"\xe0" + bytes(32)]))); mal("CMT element a lone byte", put(16, enc([t.enc_str(bytes(32)), b"\x07"]))); mal("CMT element empty", put(16, enc([b"\x80"])))
    mal("CMT element past its list", put(16, b"\xe0\xa0" + bytes(31)))
    add("malformed: empty", hm.MALFORMED, *base(), raw=b"")
    add("malformed: one byte", hm.MALFORMED, *base(), raw=b"\xc0")
    # ---- verifyHeader's rules
    h, p = base(); add("future by a second", hm.FUTURE, dict(h, Time=NOW + 1), p)
    h, p = base(); add("future: Time of 9 bytes", hm.FUTURE, dict(h, Time=2**64 + 5), p)
    h, p = base(); add("Time = now", hm.OK, dict(h, Time=NOW), p)
    h, p = base(number=30000); add("checkpoint beneficiary", hm.CHECKPOINT_BENEFICIARY, dict(h, Coinbase=bytes(19) + b"\x01"), p)
    h, p = base(number=0); add("genesis beneficiary", hm.CHECKPOINT_BENEFICIARY, dict(h, Coinbase=b"\x01" + bytes(19)), None)
    for nonce in (bytes(7) + b"\x01", b"\xff" * 7 + b"\xfe", b"\xff" * 4 + bytes(4)):
        h, p = base(); add("vote nonce " + nonce.hex(), hm.VOTE, dict(h, Nonce=nonce), p)
    h, p = base(number=30000); add("checkpoint vote", hm.CHECKPOINT_VOTE, dict(h, Nonce=b"\xff" * 8), p)
    h, p = base(); add("vanity: Extra of 31", hm.VANITY, dict(h, Extra=bytes(31)), p); h, p = base(); add("vanity: Extra empty", hm.VANITY, dict(h, Extra=b""), p)
    h, p = base(); add("signature: Extra of 32", hm.SIGNATURE, dict(h, Extra=bytes(32)), p); h, p = base(); add("signature: Extra of 96", hm.SIGNATURE, dict(h, Extra=rng.randbytes(96)), p)
    for rest in (b"", b"\x7f", b"\x80"):                                                            # the seal hash's Extra' of 0, 1 and 1 bytes
        h, p = base(); add("seal hash: Extra' = %s" % (rest.hex() or "empty"), hm.SIGNATURE, dict(h, Extra=rest + bytes(65)), p)
    for k in (55, 56, 255, 256):
        h, p = base(); add("extra signers: Extra' of %d" % k, hm.EXTRA_SIGNERS, dict(h, Extra=rng.randbytes(k) + bytes(65)), p)
        h, p = base(number=30000); add("checkpoint signers: Extra' of %d" % k, hm.CHECKPOINT_SIGNERS, dict(h, Extra=rng.randbytes(k) + bytes(65)), p)
    h, p = base(); add("extra signers: one list entry", hm.EXTRA_SIGNERS, dict(h, Extra=rng.randbytes(52) + bytes(65)), p)
    h, p = base(number=30000); add("checkpoint signers: 19 bytes", hm.CHECKPOINT_SIGNERS, dict(h, Extra=rng.randbytes(51) + bytes(65)), p)
    h, p = base(); add("mix digest", hm.MIX_DIGEST, dict(h, MixDigest=bytes(31) + b"\x01"), p)
    h, p = base(); add("uncle hash", hm.UNCLE_HASH, dict(h, UncleHash=hm.UNCLE_HASH_EMPTY[:31] + bytes([hm.UNCLE_HASH_EMPTY[31] ^ 1])), p)
    for d in (0, 3, 255, 256, 2**70):
        h, p = base(); add("difficulty %d" % d, hm.DIFFICULTY, dict(h, Difficulty=d), p)
    # ---- verifyCascadingFields' rules
    h, p = base(); add("no parent", hm.ANCESTOR, h, None)
    h, p = base(); add("parent of another number", hm.ANCESTOR, h, (p[0], p[1] - 1, p[2]))
    h, p = base(); add("parent of another hash", hm.ANCESTOR, h, (p[0][:31] + bytes([p[0][31] ^ 0x80]), p[1], p[2]))
    h, p = base(number=2**64 - 1); add("number 2^64 - 1", hm.OK, h, p)
    h, p = base(dt=PERIOD - 1); add("a second too early", hm.TIMESTAMP, h, p)
    h, p = base(dt=0); add("the parent's time", hm.TIMESTAMP, h, p)
    # ---- the seal
    for recid in (4, 255):
        h, p = base(); hs = hm.sign_header(h, KEYS[1], rng.randrange(1, N)); add("recovery byte %d" % recid, hm.SEAL, h, p, seal=hs["Extra"][-65:-1] + bytes([recid]))
    for add2 in (2, 3):
        h, p = base(); hs = hm.sign_header(h, KEYS[2], rng.randrange(1, N)); s65 = hs["Extra"][-65:]; assert int.from_bytes(s65[:32], "big") >= hm.P_MINUS_N
        add("recovery id %d, r >= p - N" % add2, hm.SEAL, h, p, seal=s65[:64] + bytes([add2]))
        for r in (1, hm.P_MINUS_N - 1):
            h, p = base(); add("recovery id %d, r = %s" % (add2, "1" if r == 1 else "p - N - 1"), hm.SEAL_UNDECIDED, h, p, seal=_sig(r, rng.randrange(1, N), add2))
        h, p = base(); add("recovery id %d, r = p - N" % add2, hm.SEAL, h, p, seal=_sig(hm.P_MINUS_N, rng.randrange(1, N), add2))
        h, p = base(); add("recovery id %d, r below the bound, s = 0" % add2, hm.SEAL, h, p, seal=_sig(5, 0, add2))
        h, p = base(); add("recovery id %d, r below the bound, s = N" % add2, hm.SEAL, h, p, seal=_sig(5, N, add2))
    for label, r, s in (("R = 0", 0, 7), ("S = 0", 7, 0), ("R = N", N, 7), ("S = N", 7, N), ("R = 2^256 - 1", 2**256 - 1, 7), ("r no x of the curve", _no_curve_x(), 7)):
        for v in (0, 1):
            h, p = base(); add("%s, recovery id %d" % (label, v), hm.SEAL, h, p, seal=_sig(r, s, v))
    h, p = base(); hs = hm.sign_header(h, KEYS[3], rng.randrange(1, N)); add("another parity: another signer", None, h, p, seal=hs["Extra"][-65:-1] + bytes([hs["Extra"][-1] ^ 1]))
    return out
