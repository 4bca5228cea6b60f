"""Sender inputs from raw transactions on Python integers: the model of include/zk_txs.h.  A restatement of what the reference does between a transaction's bytes in
a block body and recoverPlain: rlp.DecodeBytes into txdata (rlp/decode.go; core/types/transaction.go:64-100), signer.Hash (core/types/transaction_signing.go:179-189,
:231-240), the chain-id arithmetic on V (:151-161, :165-172 of transaction.go, :274-284), tx.Hash(), and Sender's rule for a deposit (:72-76).  The Go code cannot run
where these tests run: every rule carries its citation so that a reader can hold it against decode.go.  Built on secp_model's _f1600, recover, sign and address."""
import secp_model as sm

FRONTIER, HOMESTEAD, EIP155 = 0, 1, 2
OK, MALFORMED, CHAIN_ID, SIG = 0, 1, 2, 3
DEPOSIT = 3                                                     # transaction.go:43
M64 = 2**64 - 1
# txdata, in order (transaction.go:64-96; Hash has rlp:"-").  kinds: u8, u64, big, addr_nil (rlp:"nil"), bytes, hash, addr, u64s
FIELDS = [("Code", "u8"), ("AccountNonce", "u64"), ("Price", "big"), ("GasLimit", "u64"), ("Recipient", "addr_nil"), ("Amount", "big"), ("Payload", "bytes"),
          ("ZKValue", "u64"), ("ZKSN", "hash"), ("ZKSNS", "hash"), ("ZKNounce", "u64"), ("ZKAdrress", "addr"), ("ZKCMT", "hash"), ("ZKCMTS", "hash"), ("ZKProof", "bytes"),
          ("RTcmt", "hash"), ("CMTBlock", "u64s"), ("AUX", "bytes"), ("X", "big"), ("Y", "big"), ("DepositTxV", "big"), ("DepositTxR", "big"), ("DepositTxS", "big"),
          ("V", "big"), ("R", "big"), ("S", "big")]
NFIELDS = len(FIELDS)
I_RECIPIENT, I_ZKADDR, I_V, I_R, I_S = 4, 11, 23, 24, 25

# ---- the sponge -----------------------------------------------------------------------------------------------------------------------------------------------------
def sponge256(data, pad=0x01):
    """rate 136, capacity 512, 32 bytes out, any number of blocks; pad = 0x01 is the reference's Keccak-256, pad = 0x06 is SHA3-256 (the pin against hashlib)"""
    data = bytes(data); s = [0] * 25; full = len(data) // 136
    for blk in range(full + 1):
        block = bytearray(data[136 * blk: 136 * blk + 136])
        if blk == full: block.append(pad); block.extend(bytes(136 - len(block))); block[135] |= 0x80
        for k in range(17): s[k] ^= int.from_bytes(block[8 * k: 8 * k + 8], "little")
        sm._f1600(s)
    return b"".join(v.to_bytes(8, "little") for v in s[:4])
def keccak256(data): return sponge256(data, 0x01)

# ---- the encoder ----------------------------------------------------------------------------------------------------------------------------------------------------
def be(v): return v.to_bytes((v.bit_length() + 7) // 8, "big")
def head(base, n):                                              # rlp/encode.go puthead: short form to 55, then the length of the length
    return bytes([base + n]) if n < 56 else bytes([base + 55 + len(be(n))]) + be(n)
def enc_str(b): b = bytes(b); return b if len(b) == 1 and b[0] < 0x80 else head(0x80, len(b)) + b
def enc_int(v): return enc_str(be(v))
def enc_list(items): p = b"".join(items); return head(0xC0, len(p)) + p

def default_tx(**kw):
    """newTransaction's txdata (transaction.go:122-153) with every pointer set; fields by name"""
    tx = dict(Code=0, AccountNonce=0, Price=0, GasLimit=0, Recipient=None, Amount=0, Payload=b"", ZKValue=0, ZKSN=bytes(32), ZKSNS=bytes(32), ZKNounce=0, ZKAdrress=bytes(20),
              ZKCMT=bytes(32), ZKCMTS=bytes(32), ZKProof=b"", RTcmt=bytes(32), CMTBlock=[], AUX=b"", X=0, Y=0, DepositTxV=0, DepositTxR=0, DepositTxS=0, V=0, R=0, S=0)
    assert set(kw) <= set(tx), kw; tx.update(kw); return tx
def encode_items(tx, nil_as_list=False):
    """the encodings of the fields, one bytes object each; a nil Recipient as 0x80 (what the reference writes) or as 0xC0 (what its decoder also takes)"""
    out = []
    for name, kind in FIELDS:
        v = tx[name]
        if kind in ("u8", "u64", "big"): out.append(enc_int(v))
        elif kind == "addr_nil": out.append((b"\xc0" if nil_as_list else b"\x80") if v is None else enc_str(v))
        elif kind == "u64s": out.append(enc_list([enc_int(x) for x in v]))
        else: out.append(enc_str(v))
    return out
def encode(tx, nil_as_list=False): return enc_list(encode_items(tx, nil_as_list))

# ---- the strict decoder ---------------------------------------------------------------------------------------------------------------------------------------------
class Malformed(Exception):
    pass
def read_head(t, pos, lim):
    """Stream.readKind (decode.go:902-960) with Kind's bound (:883-894) -> (kind 'byte' | 'str' | 'list', start of the content, its size).  Every byte of the header
    lies below lim (willRead, :1016-1034)."""
    if pos >= lim: raise Malformed("value expected")
    b = t[pos]
    if b < 0x80: return "byte", pos, 1                           # :919-923
    if b < 0xB8: kind, size, beg = "str", b - 0x80, pos + 1      # :924-929
    elif b < 0xC0 or b >= 0xF8:                                  # :930-941, :949-960
        ll = b - (0xB7 if b < 0xC0 else 0xF7); kind = "str" if b < 0xC0 else "list"; beg = pos + 1 + ll
        if beg > lim: raise Malformed("size runs past the list")
        if ll > 1 and t[pos + 1] == 0: raise Malformed("leading zero in a size")           # readUint :980-985
        size = int.from_bytes(t[pos + 1: beg], "big")
        if size < 56: raise Malformed("long form below 56")      # :938, :957
    else: kind, size, beg = "list", b - 0xC0, pos + 1            # :942-948
    if size > lim - beg: raise Malformed("element larger than its list")                   # :886, :891
    if kind == "str" and size == 1 and t[beg] < 0x80: raise Malformed("one byte below 0x80 under a header")   # :662, :423, :726
    return kind, beg, size
def dec_uint(t, kind, beg, size, maxbytes):
    """Stream.uint (decode.go:703-734)"""
    if kind == "list": raise Malformed("list where a uint belongs")                         # :732
    if kind == "byte":
        if t[beg] == 0: raise Malformed("0x00 as a uint")                                    # :710
        return t[beg]
    if size > maxbytes: raise Malformed("uint overflow")                                     # :716
    if size and t[beg] == 0: raise Malformed("leading zero in a uint")                       # readUint :980, :721-723 (one byte: :726, the byte is below 0x80)
    return int.from_bytes(t[beg: beg + size], "big")
def decode(t):
    """rlp.DecodeBytes(t, &txdata) -> (the fields, spans): spans[k] = (start, end) of item k's encoding in t; raises Malformed where the reference returns an error"""
    t = bytes(t)
    if len(t) > 2**32 - 1: raise Malformed("longer than 2^32 - 1 bytes")                    # (zk_txs.h's own bound)
    kind, pos, size = read_head(t, 0, len(t))
    if kind != "list": raise Malformed("not a list")                                         # decode.go:438, :762
    if pos + size != len(t): raise Malformed("bytes after the list")                         # decode.go:142-144 ErrMoreThanOneValue
    lim = len(t); tx = {}; spans = []
    for name, fk in FIELDS:
        if pos == lim: raise Malformed("too few elements")                                   # :443-444
        start = pos; kind, beg, size = read_head(t, pos, lim); pos = beg + size; body = t[beg: beg + size]
        if fk == "u8": tx[name] = dec_uint(t, kind, beg, size, 1)
        elif fk == "u64": tx[name] = dec_uint(t, kind, beg, size, 8)
        elif fk == "big":                                                                    # :271-287
            if kind == "list": raise Malformed("list where an integer belongs")
            if size and body[0] == 0: raise Malformed("leading zero in an integer")          # :282 (the byte 0x00 is a one-byte string here: refused too)
            tx[name] = int.from_bytes(body, "big")
        elif fk == "bytes":                                                                  # :386-393
            if kind == "list": raise Malformed("list where a string belongs")
            tx[name] = body
        elif fk in ("hash", "addr", "addr_nil"):                                             # :395-430
            want = 32 if fk == "hash" else 20
            if fk == "addr_nil" and kind != "byte" and size == 0: tx[name] = None            # :486-496: an empty string or an empty list
            else:
                if kind == "list": raise Malformed("list where a byte array belongs")       # :426
                if kind == "byte" or size != want: raise Malformed("byte array of the wrong length")   # :406, :412-416
                tx[name] = body
        else:                                                                                # []uint64: :323-336
            if kind != "list": raise Malformed("string where a list belongs")               # :324, :762
            vals = []; p = beg
            while p < beg + size:
                k2, b2, s2 = read_head(t, p, beg + size); vals.append(dec_uint(t, k2, b2, s2, 8)); p = b2 + s2
            tx[name] = vals
        spans.append((start, pos))
    if pos != lim: raise Malformed("too many elements")                                      # :449, :778
    return tx, spans

# ---- the signers ----------------------------------------------------------------------------------------------------------------------------------------------------
def is_protected(v): return v not in (27, 28) if v.bit_length() <= 8 else True              # transaction.go:165-172
def derive_chain_id(v):                                                                      # transaction_signing.go:274-284
    if v.bit_length() <= 64: return 0 if v in (27, 28) else ((v - 35) & M64) // 2            # uint64 arithmetic: below 35 it wraps
    return (v - 35) // 2
def sig_hash(tx, signer, chain_id, keccak=keccak256):
    six = [enc_int(tx["AccountNonce"]), enc_int(tx["Price"]), enc_int(tx["GasLimit"]), b"\x80" if tx["Recipient"] is None else enc_str(tx["Recipient"]), enc_int(tx["Amount"]),
           enc_str(tx["Payload"])]
    if signer == EIP155 and is_protected(tx["V"]): six += [enc_int(chain_id), b"\x80", b"\x80"]   # :179-189; an unprotected V takes Homestead's road, :152-154
    return keccak(enc_list(six))
def signing_inputs(raw, signer, chain_id, keccak=keccak256):
    """zkTxSigningInputs for one transaction -> dict(status, code, txhash, sighash, sig, deposit_from): the header's outputs; keccak: the hash function, as
    trie_model.derive_sha takes one"""
    zero = dict(status=MALFORMED, code=0, txhash=bytes(32), sighash=bytes(32), sig=bytes(65), deposit_from=bytes(20))
    try: tx, spans = decode(raw)
    except Malformed: return zero
    reenc = encode(tx); code = tx["Code"]; v, r, s = tx["V"], tx["R"], tx["S"]; status = OK; vs = v
    assert reenc == raw or (tx["Recipient"] is None and raw[spans[I_RECIPIENT][0]] == 0xC0 and reenc == raw[:spans[I_RECIPIENT][0]] + b"\x80" + raw[spans[I_RECIPIENT][1]:])
    if signer == EIP155 and is_protected(v):
        if derive_chain_id(v) != chain_id: status = CHAIN_ID                                 # :155-157
        else: vs = v - 2 * chain_id - 8                                                      # :158-159
    if status == OK and (vs.bit_length() > 8 or r.bit_length() > 256 or s.bit_length() > 256): status = SIG   # :247; :255-258 cannot hold more than 32 bytes
    vbyte = ((vs - 27) & M64) & 0xFF                                                          # :250
    if code == DEPOSIT:                                                                      # :72-76: V, R and S are never looked at
        sig = (r.to_bytes(32, "big") if r.bit_length() <= 256 else bytes(32)) + (s.to_bytes(32, "big") if s.bit_length() <= 256 else bytes(32)) + bytes([vbyte if (status == OK or (status == SIG and vs.bit_length() <= 8)) else 0])
        status = OK
    else: sig = r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([vbyte]) if status == OK else bytes(65)
    return dict(status=status, code=code, txhash=keccak(reenc), sighash=sig_hash(tx, signer, chain_id, keccak), sig=sig, deposit_from=tx["ZKAdrress"] if code == DEPOSIT else bytes(20))
def sender(raw, signer, chain_id, keccak=keccak256):
    """zkTxSenders for one transaction -> (status, code, txhash, from): types.Sender(signer, tx) after the decode"""
    d = signing_inputs(raw, signer, chain_id, keccak)
    if d["status"] != OK: return d["status"], d["code"], d["txhash"], bytes(20)
    if d["code"] == DEPOSIT: return OK, d["code"], d["txhash"], d["deposit_from"]
    ok, _, _, addr = sm.recover(d["sighash"], d["sig"], signer != FRONTIER)
    return (OK if ok else SIG), d["code"], d["txhash"], addr
def sign_tx(tx, signer, chain_id, key, nonce):
    """SignTx (transaction_signing.go:56-63): V, R, S of tx set as the signer's SignatureValues sets them (:165-175, :219-227)"""
    tx = dict(tx); protect = signer == EIP155 and chain_id != 0; tx["V"] = 35 if protect else 27   # (any V of the right class: the hash depends on the class alone)
    sig = sm.sign(sig_hash(tx, signer, chain_id), key, nonce)
    tx["R"] = int.from_bytes(sig[:32], "big"); tx["S"] = int.from_bytes(sig[32:64], "big"); tx["V"] = sig[64] + (35 + 2 * chain_id if protect else 27); return tx
