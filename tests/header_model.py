"""Headers from their bytes on Python integers: the model of include/zk_headers.h.  A restatement of what the reference does with a batch of headers
between a peer's bytes and the snapshot: rlp.DecodeBytes into types.Header (core/types/block.go:72-90; rlp/decode.go), Header.Hash() (:105-107), and for the Clique
engine verifyHeader (consensus/clique/clique.go:269-326), verifyCascadingFields (:332-350), sigHash (:147-169) and ecrecover (:172-194) down to libsecp256k1's recovery
(crypto/secp256k1/secp256.go:105-122, :171-179; libsecp256k1/src/modules/recovery/main_impl.h:38-58, :87-121).  The Go code cannot run where these tests run: every rule
carries its citation.  Built on tx_model (the strict RLP head reader, the encoder, Keccak-256) and secp_model (sign, recover)."""
import secp_model as sm
import tx_model as t

(OK, MALFORMED, FUTURE, CHECKPOINT_BENEFICIARY, VOTE, CHECKPOINT_VOTE, VANITY, SIGNATURE, EXTRA_SIGNERS, CHECKPOINT_SIGNERS, MIX_DIGEST, UNCLE_HASH, DIFFICULTY, ANCESTOR,
 TIMESTAMP, SEAL, SEAL_UNDECIDED) = range(17)
STATUS_NAMES = ["OK", "MALFORMED", "FUTURE", "CHECKPOINT_BENEFICIARY", "VOTE", "CHECKPOINT_VOTE", "VANITY", "SIGNATURE", "EXTRA_SIGNERS", "CHECKPOINT_SIGNERS", "MIX_DIGEST",
                "UNCLE_HASH", "DIFFICULTY", "ANCESTOR", "TIMESTAMP", "SEAL", "SEAL_UNDECIDED"]
M64 = 2**64 - 1
EPOCH = 30000                                                   # clique.go:56, set by clique.New (:217-219) where the configuration says 0
VANITY_BYTES, SEAL_BYTES = 32, 65                               # clique.go:59-60
UNCLE_HASH_EMPTY = t.keccak256(b"\xc0")                         # clique.go:65: types.CalcUncleHash(nil) = rlpHash([]*Header(nil)); pinned by tests/golden/header_vectors.txt
P_MINUS_N = sm.P - sm.N                                         # main_impl.h:105: secp256k1_ecdsa_const_p_minus_order
# types.Header in order (block.go:72-90).  kinds: hash, addr, bloom (256 bytes), nonce (8 bytes), big, u64, bytes, hashes ([]*common.Hash)
FIELDS = [("ParentHash", "hash"), ("UncleHash", "hash"), ("Coinbase", "addr"), ("Root", "hash"), ("TxHash", "hash"), ("ReceiptHash", "hash"), ("Bloom", "bloom"), ("Difficulty", "big"),
          ("Number", "big"), ("GasLimit", "u64"), ("GasUsed", "u64"), ("Time", "big"), ("Extra", "bytes"), ("MixDigest", "hash"), ("Nonce", "nonce"), ("RTCMT", "hash"), ("CMT", "hashes")]
NFIELDS = len(FIELDS)
I_EXTRA, I_CMT, SEAL_FIELDS = 12, 16, 15                        # sigHash lists the upstream 15 (clique.go:150-166): no RTCMT, no CMT
ARRAY_BYTES = {"hash": 32, "addr": 20, "bloom": 256, "nonce": 8}

def default_header(**kw):
    h = dict(ParentHash=bytes(32), UncleHash=UNCLE_HASH_EMPTY, Coinbase=bytes(20), Root=bytes(32), TxHash=bytes(32), ReceiptHash=bytes(32), Bloom=bytes(256), Difficulty=2, Number=1,
             GasLimit=0, GasUsed=0, Time=0, Extra=bytes(VANITY_BYTES + SEAL_BYTES), MixDigest=bytes(32), Nonce=bytes(8), RTCMT=bytes(32), CMT=[])
    assert set(kw) <= set(h), kw; h.update(kw); return h
def encode_items(h, fields=NFIELDS):
    out = []
    for name, kind in FIELDS[:fields]:
        v = h[name]
        if kind in ("big", "u64"): out.append(t.enc_int(v))
        elif kind == "hashes": out.append(t.enc_list([t.enc_str(x) for x in v]))
        else: out.append(t.enc_str(v))
    return out
def encode(h): return t.enc_list(encode_items(h))

def decode(raw):
    """rlp.DecodeBytes(raw, &types.Header{}) -> (the fields, spans, contents): spans[k] = (start, end) of item k's encoding, contents[k] = (start, size) of its content;
    raises tx_model.Malformed where the reference returns an error"""
    raw = bytes(raw)
    if len(raw) > 2**32 - 1: raise t.Malformed("longer than 2^32 - 1 bytes")                  # (zk_headers.h's own bound)
    kind, pos, size = t.read_head(raw, 0, len(raw))
    if kind != "list": raise t.Malformed("not a list")                                         # decode.go:438, :762
    if pos + size != len(raw): raise t.Malformed("bytes after the list")                       # decode.go:142-144
    lim = len(raw); h = {}; spans = []; contents = []
    for name, fk in FIELDS:
        if pos == lim: raise t.Malformed("too few elements")                                   # :443-444
        start = pos; kind, beg, size = t.read_head(raw, pos, lim); pos = beg + size; body = raw[beg: beg + size]
        if fk == "u64": h[name] = t.dec_uint(raw, kind, beg, size, 8)                          # :703-734
        elif fk == "big":                                                                      # :271-287
            if kind == "list": raise t.Malformed("list where an integer belongs")
            if size and body[0] == 0: raise t.Malformed("leading zero in an integer")          # :282
            if name == "Number" and size > 8: raise t.Malformed("Number wider than 8 bytes")   # (zk_headers.h's own bound: the reference reads Number.Uint64())
            h[name] = int.from_bytes(body, "big")
        elif fk == "bytes":                                                                    # :386-393
            if kind == "list": raise t.Malformed("list where a string belongs")
            h[name] = body
        elif fk in ARRAY_BYTES:                                                                # decodeByteArray :395-430
            if kind == "list": raise t.Malformed("list where a byte array belongs")            # :426
            if kind == "byte" or size != ARRAY_BYTES[fk]: raise t.Malformed("byte array of the wrong length")   # :406, :412-416
            h[name] = body
        else:                                                                                  # []*common.Hash: decodeListSlice :323-336, makePtrDecoder :456-478 (no "nil" tag)
            if kind != "list": raise t.Malformed("string where a list belongs")
            vals = []; p = beg
            while p < beg + size:
                k2, b2, s2 = t.read_head(raw, p, beg + size)
                if k2 != "str" or s2 != 32: raise t.Malformed("CMT element that is no 32-byte string")
                vals.append(raw[b2: b2 + s2]); p = b2 + s2
            h[name] = vals
        spans.append((start, pos)); contents.append((beg, size))
    if pos != lim: raise t.Malformed("too many elements")                                      # :449, :778
    return h, spans, contents

def header_hash(h, keccak=t.keccak256): return keccak(encode(h))                                              # block.go:105-107: all 17 fields
def seal_hash(h, cut=SEAL_BYTES, keccak=t.keccak256):
    """clique.go:147-169: the upstream 15 fields, Extra without its last `cut` bytes"""
    assert len(h["Extra"]) >= cut; items = encode_items(h, SEAL_FIELDS); items[I_EXTRA] = t.enc_str(h["Extra"][:len(h["Extra"]) - cut]); return keccak(t.enc_list(items))

def seal_recover(sighash, sig):
    """crypto.Ecrecover(sighash, sig) as ecrecover calls it (clique.go:185) -> (OK, signer) | (SEAL, None) | (SEAL_UNDECIDED, None).  No ValidateSignatureValues, no low-s
    rule: this is not recoverPlain."""
    r = int.from_bytes(sig[:32], "big"); s = int.from_bytes(sig[32:64], "big"); v = sig[64]
    if v >= 4: return SEAL, None                                                               # secp256.go:175-177
    if r >= sm.N or s >= sm.N: return SEAL, None                                               # main_impl.h:48-51: overflow
    if r == 0 or s == 0: return SEAL, None                                                     # main_impl.h:96-98
    if v & 2:
        if r >= P_MINUS_N: return SEAL, None                                                   # main_impl.h:104-107
        return SEAL_UNDECIDED, None                                                            # x = r + N: zk_senders.h's recovery does not take it; the caller decides
    key = (bytes(sighash), bytes(sig))                                                         # (the curve arithmetic once a distinct seal: the tests decide the same headers in many batches)
    if key not in _RECOVERED: _RECOVERED[key] = sm.recover(sighash, sig[:64] + bytes([v]), False)   # main_impl.h:110-120
    ok, _, _, addr = _RECOVERED[key]
    return (OK, addr) if ok else (SEAL, None)
_RECOVERED = {}

ZERO = dict(status=MALFORMED, hash=bytes(32), sealhash=bytes(32), signer=bytes(20), coinbase=bytes(20), tx_root=bytes(32), rtcmt=bytes(32), number=0, time=0, difficulty=0, vote=0,
            extra_beg=0, extra_size=0, cmt_beg=0, cmt_count=0)
def standalone(h, epoch, now):
    """verifyHeader's own rules (clique.go:269-319) -> the first that applies, OK where none does"""
    number = h["Number"] & M64; checkpoint = number % epoch == 0; extra = len(h["Extra"])       # :273, :280
    if h["Time"] > now: return FUTURE                                                          # :276
    if checkpoint and h["Coinbase"] != bytes(20): return CHECKPOINT_BENEFICIARY                # :281
    if h["Nonce"] not in (b"\xff" * 8, bytes(8)): return VOTE                                  # :285
    if checkpoint and h["Nonce"] != bytes(8): return CHECKPOINT_VOTE                           # :288
    if extra < VANITY_BYTES: return VANITY                                                     # :292
    if extra < VANITY_BYTES + SEAL_BYTES: return SIGNATURE                                     # :295
    signers = extra - VANITY_BYTES - SEAL_BYTES
    if not checkpoint and signers: return EXTRA_SIGNERS                                        # :300
    if checkpoint and signers % 20: return CHECKPOINT_SIGNERS                                  # :303
    if h["MixDigest"] != bytes(32): return MIX_DIGEST                                          # :307
    if h["UncleHash"] != UNCLE_HASH_EMPTY: return UNCLE_HASH                                   # :311
    if number > 0 and h["Difficulty"] not in (1, 2): return DIFFICULTY                         # :315-318
    return OK
def headers(raws, period, epoch, now, parent, keccak=t.keccak256):
    """zkHeaders -> a dict of the header's outputs per header.  parent: None (have_parent = 0) or (hash, number, time) of the parent of header 0 as the caller found it.
    Every header is decided against its predecessor in the batch whatever that predecessor's status (clique.go:253 passes headers[:i]).  keccak: the hash function, as
    trie_model.derive_sha takes one; what is remembered of a header is remembered for each function apart."""
    epoch = epoch or EPOCH; out = []; prev = parent; _DECODED = _DECODED_BY.setdefault(keccak, {})
    for raw in raws:
        raw = bytes(raw)
        if raw not in _DECODED:                                                                # (the decoder and the two hashes once a distinct header, as for the seals)
            try: h, spans, contents = decode(raw); _DECODED[raw] = (h, contents, header_hash(h, keccak), seal_hash(h, keccak=keccak) if len(h["Extra"]) >= SEAL_BYTES else bytes(32))
            except t.Malformed: _DECODED[raw] = None
            assert _DECODED[raw] is None or encode(h) == raw                                   # the strict decoder: the re-encoding is the input
        if _DECODED[raw] is None: out.append(dict(ZERO)); prev = None; continue               # (a header behind one that does not decode has no parent: ANCESTOR)
        h, contents, hh, sealhash = _DECODED[raw]; number = h["Number"]; extra = h["Extra"]
        o = dict(ZERO, hash=hh, coinbase=h["Coinbase"], tx_root=h["TxHash"], rtcmt=h["RTCMT"], number=number, time=h["Time"] & M64, difficulty=min(h["Difficulty"], 255),
                 vote=1 if h["Nonce"] == b"\xff" * 8 else 0, extra_beg=contents[I_EXTRA][0], extra_size=contents[I_EXTRA][1], cmt_beg=contents[I_CMT][0], cmt_count=len(h["CMT"]))
        o["sealhash"] = sealhash                                                               # Author() reaches sigHash on any header with 65 bytes of Extra (clique.go:235-237, :179)
        status = standalone(h, epoch, now)
        if status == OK and number > 0:                                                        # verifyCascadingFields :334-336: the genesis is the always valid dead end
            if prev is None or prev[1] != (number - 1) & M64 or prev[0] != h["ParentHash"]: status = ANCESTOR   # :345
            elif ((prev[2] + period) & M64) > (h["Time"] & M64): status = TIMESTAMP             # :348, in uint64 arithmetic
            else:
                status, signer = seal_recover(o["sealhash"], extra[-SEAL_BYTES:])               # verifySeal :480 -> ecrecover :172-194
                if status == OK: o["signer"] = signer
        o["status"] = status; out.append(o); prev = (hh, number, h["Time"] & M64)
    return out
_DECODED_BY = {}
def accepted(outs):
    k = 0
    while k < len(outs) and outs[k]["status"] == OK: k += 1
    return k

def sign_header(h, key, nonce, recid_add=0):
    """h with the last 65 bytes of Extra replaced by the seal of `key` over sigHash (clique.go:647-651)"""
    h = dict(h); sig = sm.sign(seal_hash(h), key, nonce); h["Extra"] = h["Extra"][:-SEAL_BYTES] + sig[:64] + bytes([sig[64] + recid_add]); return h
def signer_address(key):
    if key not in _ADDRESS: _ADDRESS[key] = sm.address(sm.mul(key, sm.G))
    return _ADDRESS[key]
_ADDRESS = {}
