"""The transaction roots of a segment's bodies and the chain call that takes the headers' roots: the model of include/zk_tx_roots.h, on
tests/trie_model.py (DeriveSha) and tests/bodies_model.py (the steps of verifyChainBodies)."""
import tx_model as t
import trie_model as tm
import bodies_model as bm

_memo = {}
def keccak(b):
    """tx_model.keccak256, memoised: the same leaves and branches come back in test after test"""
    b = bytes(b)
    if b not in _memo: _memo[b] = t.keccak256(b)
    return _memo[b]

def decodes(raw):
    try: t.decode(raw); return True
    except t.Malformed: return False

def tx_roots(raws, block_first, keccak=keccak, keccak_many=None):
    """zkTxRoots -> (roots: [32 bytes] x n_blocks, defined: [bool] x n_blocks).  A block with a transaction that rlp.DecodeBytes refuses has no root (the body does
    not decode: core/types/block.go DecodeRLP): 32 zero bytes, defined False.  Otherwise DeriveSha over rlp.EncodeToBytes(tx) of each, whatever the other statuses"""
    roots, defined = [], []
    for b in range(len(block_first) - 1):
        blk = raws[block_first[b]:block_first[b + 1]]; good = all(decodes(r) for r in blk); defined.append(good)
        roots.append(tm.derive_sha([tm.tx_value(r) for r in blk], keccak, keccak_many) if good else bytes(32))
    return roots, defined

def chain_bodies_roots(raws, block_first, want_roots, signer, chain_id, chain_accounts, sizes_now, roots_of=tx_roots):
    """verifyChainBodiesRoots: bodies_model.chain_bodies with step 2 changed — B0 is the first block that holds a transaction with status != OK or whose root is undefined
    or differs from want_roots[b].  -> (k, chain_bodies' dict with roots and root_ok for ALL blocks) or raises bodies_model.Refused"""
    n = len(raws); nb = len(block_first) - 1
    if nb < 0 or block_first[0] != 0 or block_first[nb] != n or any(block_first[b] > block_first[b + 1] for b in range(nb)): raise bm.Refused("block_first")
    if len(want_roots) != nb: raise bm.Refused("want_roots")
    recs, rec_froms, rec_of, froms, code, status, txhash = bm.records(raws, signer, chain_id)                                # step 1, and the roots beside it
    roots, defined = roots_of(raws, block_first); root_ok = [defined[b] and roots[b] == bytes(want_roots[b]) for b in range(nb)]
    bad_block = lambda b: not root_ok[b] or any(status[i] != t.OK for i in range(block_first[b], block_first[b + 1]))
    B0 = next((b for b in range(nb) if bad_block(b)), nb)                                                                    # step 2
    before = [0] * (n + 1)
    for i in range(n): before[i + 1] = before[i] + (rec_of[i] >= 0)
    rec_first = [before[block_first[b]] for b in range(B0 + 1)]; n0 = rec_first[B0]
    k, ok, anchor_of, filled, sizes = chain_accounts(recs[:n0], rec_froms[:n0], rec_first)                                   # step 3
    assert 0 <= k <= B0 and len(ok) == n0
    left = sizes[B0 - 1] if B0 else sizes_now()                                                                              # step 4
    return k, dict(B0=B0, n_recs=len(recs), recs=list(filled) + recs[n0:], rec_froms=rec_froms, rec_of=rec_of, froms=froms, code=code, status=status, txhash=txhash,
                   ok=list(ok) + [False] * (len(recs) - n0), anchor_of=list(anchor_of) + [-1] * (len(recs) - n0), sizes=list(sizes[:B0]) + [left] * (nb - B0), roots=roots, root_ok=root_ok)
