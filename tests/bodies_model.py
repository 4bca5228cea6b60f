"""Records from the block bodies' bytes, and the chain call on them, on Python integers: the model of include/zk_bodies.h.  Built on tx_model (the strict decoder, the
hashes, Sender) and secp_model (the recovery, the address).  A restatement of what the reference's ApplyTransaction does with a transaction before its proof is
verified (core/state_processor.go:106-163) and of how zktx.go:122-210 marshals a transaction's fields into the verify calls.  The Go code cannot run where these tests
run: every rule carries its citation."""
import struct
import secp_model as sm
import tx_model as t

DEPOSIT_KEY = 4                                                 # zk_bodies.h: ZK_TX_DEPOSIT_KEY
KIND_OF_CODE = {1: 0, 2: 1, 3: 2, 5: 3}                         # transaction.go:40-46 MintTx, SendTx, DepositTx, RedeemTx -> zk_batch.h ZK_KIND_*; state_processor.go:108-164 has no branch for 0, 4, > 5
ZERO32 = bytes(32)

def six_field_hash(tx, keccak=t.keccak256):
    """HomesteadSigner's hash = FrontierSigner's (transaction_signing.go:231-240): never the nine-field one"""
    return t.sig_hash(dict(tx, V=27), t.HOMESTEAD, 0, keccak)
def deposit_key(tx, keccak=t.keccak256):
    """state_processor.go:141-146 for a decoded deposit -> (accepted, addr1).  addr1 = ExtractPKBAddress(HomesteadSigner{}, tx) (transaction_signing.go:96-113 ->
    :206-208 -> recoverPlain :246-271 with homestead = true); addr2 = PubkeyToAddress({X, Y}) (crypto.go:212-215)"""
    v, r, s, x, y = tx["V"], tx["R"], tx["S"], tx["X"], tx["Y"]
    if v.bit_length() > 8: return False, bytes(20)                                          # :247
    vb = (v - 27) & 0xFF                                                                     # :250, no chain-id arithmetic: 37 gives 10
    if r.bit_length() > 256 or s.bit_length() > 256: return False, bytes(20)                # :255-258 cannot hold them (ValidateSignatureValues, crypto.go:209, refuses them first: r, s < N)
    ok, _, _, addr1 = sm.recover(six_field_hash(tx, keccak), r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([vb]), True)   # :251 homestead = true whatever the block's signer
    if not ok: return False, bytes(20)                                                       # state_processor.go:144 err != nil
    if x.bit_length() > 256 or y.bit_length() > 256: return False, bytes(20)                # crypto.go:136-141: elliptic.Marshal slices out of range, the node dies; zk_bodies.h refuses
    addr2 = keccak(x.to_bytes(32, "big") + y.to_bytes(32, "big"))[12:]                 # crypto.go:212-215; no curve check
    return addr1 == addr2, addr1                                                             # state_processor.go:144 addr1 != addr2

def record_bytes(tx, pk=None):
    """the 720 bytes of the record of a decoded transaction with code 1, 2, 3 or 5: the model's own reading of zk_bodies.h's table"""
    code = tx["Code"]; kind = KIND_OF_CODE[code]; h = lambda name: bytes(tx[name])
    if code in (1, 5): value, args = tx["ZKValue"], [ZERO32, h("ZKSN"), h("ZKCMT")]                                   # zktx.go:122-133, :198-210
    elif code == 2: value, args = 0, [ZERO32, h("ZKSN"), h("ZKCMTS"), h("ZKCMT")]                                     # zktx.go:148-160
    else: value, args = 0, [h("RTcmt"), bytes(pk) + bytes(12), ZERO32, h("ZKSN"), h("ZKCMT"), h("ZKSNS")]             # zktx.go:180-194
    proof = bytes(tx["ZKProof"])[:512].ljust(512, b"\0")                                     # verify* reads 512 characters; a zero byte is no hex digit
    return struct.pack("<B7xQ", kind, value) + proof + b"".join(args).ljust(192, b"\0")

_memo = {}
def one(raw, signer, chain_id, keccak=t.keccak256):
    """zkTxRecords for one transaction -> (status, code, txhash, from, the record's 720 bytes or None)"""
    key = (bytes(raw), signer, chain_id, keccak)
    if key in _memo: return _memo[key]
    status, code, txhash, frm = t.sender(raw, signer, chain_id, keccak); rec = None
    if status != t.MALFORMED and code == t.DEPOSIT:                                          # (Sender never fails for a decoded deposit: transaction_signing.go:72-76)
        tx, _ = t.decode(raw); good, pk = deposit_key(tx, keccak)
        if good: rec = record_bytes(tx, pk)
        else: status, frm = DEPOSIT_KEY, bytes(20)
    elif status == t.OK and code in KIND_OF_CODE: rec = record_bytes(t.decode(raw)[0])
    _memo[key] = (status, code, txhash, frm, rec); return _memo[key]

def records(raws, signer, chain_id, keccak=t.keccak256):
    """zkTxRecords -> (recs: [720 bytes] x m, rec_froms: [20 bytes] x m, rec_of: [int] x n, froms, code, status, txhash)"""
    recs, rec_froms, rec_of, froms, code, status, txhash = [], [], [], [], [], [], []
    for raw in raws:
        st, c, th, frm, rec = one(raw, signer, chain_id, keccak); froms.append(frm); code.append(c); status.append(st); txhash.append(th)
        if rec is None: rec_of.append(-1)
        else: rec_of.append(len(recs)); recs.append(rec); rec_froms.append(frm)
    return recs, rec_froms, rec_of, froms, code, status, txhash

class Refused(Exception):
    pass
def chain_bodies(raws, block_first, signer, chain_id, chain_accounts, sizes_now):
    """verifyChainBodies' five steps over a records-level oracle.
    chain_accounts(recs, rec_froms, rec_block_first) -> (k, ok [bool] x len(recs), anchor_of [int], filled recs, sizes [per block]) or raises Refused — verifyChainAccounts;
    sizes_now() -> the sizes of the states as they stand.  -> (k, dict) or raises Refused"""
    n = len(raws); nb = len(block_first) - 1
    if nb < 0 or block_first[0] != 0 or block_first[nb] != n or any(block_first[b] > block_first[b + 1] for b in range(nb)): raise Refused("block_first")   # step 5
    recs, rec_froms, rec_of, froms, code, status, txhash = records(raws, signer, chain_id)                                  # step 1
    bad = [i for i in range(n) if status[i] != t.OK]
    B0 = nb if not bad else next(b for b in range(nb) if block_first[b + 1] > bad[0])                                        # step 2
    before = [0] * (n + 1)
    for i in range(n): before[i + 1] = before[i] + (rec_of[i] >= 0)
    rec_first = [before[block_first[b]] for b in range(B0 + 1)]; n0 = rec_first[B0]
    k, ok, anchor_of, filled, sizes = chain_accounts(recs[:n0], rec_froms[:n0], rec_first)                                   # step 3 (raises Refused: step 5)
    assert 0 <= k <= B0 and len(ok) == n0
    left = sizes[B0 - 1] if B0 else sizes_now()                                                                              # step 4: from B0 on, the sizes the call leaves
    return k, dict(B0=B0, n_recs=len(recs), recs=list(filled) + recs[n0:], rec_froms=rec_froms, rec_of=rec_of, froms=froms, code=code, status=status, txhash=txhash,
                   ok=list(ok) + [False] * (len(recs) - n0), anchor_of=list(anchor_of) + [-1] * (len(recs) - n0), sizes=list(sizes[:B0]) + [left] * (nb - B0))
