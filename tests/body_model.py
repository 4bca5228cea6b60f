"""Block bodies from their bytes on Python integers: the model of include/zk_raw_bodies.h.  A restatement of what rlp.DecodeBytes(body, &types.Body{})
(core/types/block.go:143-146: Transactions, Uncles) decides about a body's STRUCTURE, built on tx_model.read_head — the strict head reader the transaction walk's model
uses — and of the rule that a block of this chain has no uncle.  The Go code cannot run where these tests run: every rule carries its citation so that a reader can
hold it against rlp/decode.go."""
import os
import tx_model as t
import tx_roots_model as rm
import bodies_model as bm

OK, MALFORMED, UNCLES = 0, 1, 2                                  # zk_raw_bodies.h: ZK_BODY_*

def vectors():
    """tests/golden/body_vectors.txt -> dict(block_txs, block_uncles)"""
    out = {}
    for line in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "body_vectors.txt")):
        w = line.split()
        if w and not w[0].startswith("#"): out[w[0]] = bytes.fromhex(w[1])
    return out

def body(txs, uncles=()):
    """rlp([[tx ...], [uncle ...]]): every tx and every uncle an encoded item"""
    return t.enc_list([t.enc_list(list(txs)), t.enc_list(list(uncles))])

def split(raw):
    """-> (status, [(beg, size)]): the status of one body and, where it is OK, the extent of every element of item 0 relative to the body's first byte — its head and its
    payload, or the lone byte.  A body that is not OK has no extents."""
    raw = bytes(raw); n = len(raw)
    try:
        if n > 2**32 - 1: raise t.Malformed("longer than 2^32 - 1 bytes")                     # (the library's own bound, as for headers)
        kind, pos, size = t.read_head(raw, 0, n)                                              # an empty body: io.ErrUnexpectedEOF, decode.go:142 with :910
        if kind != "list": raise t.Malformed("the body is no list")                          # makeStructDecoder :438, List :762
        if pos + size != n: raise t.Malformed("bytes after the list")                        # DecodeBytes :142-144 ErrMoreThanOneValue (a payload beyond the input: :886, :891)
        lim = n
        if pos == lim: raise t.Malformed("too few elements")                                 # :443-444
        k0, b0, s0 = t.read_head(raw, pos, lim)
        if k0 != "list": raise t.Malformed("Transactions is no list")                        # decodeListSlice :323-326
        pos = b0 + s0
        if pos == lim: raise t.Malformed("too few elements")                                 # :443-444
        k1, b1, s1 = t.read_head(raw, pos, lim)
        if k1 != "list": raise t.Malformed("Uncles is no list")                              # :323-326
        if b1 + s1 != lim: raise t.Malformed("too many elements")                            # :449, ListEnd :778
        extents = []; p = b0; end = b0 + s0
        while p < end:                                                                       # Stream.Kind reads every element's head before the element is decoded (:902-960)
            _, beg, size = t.read_head(raw, p, end); extents.append((p, beg + size - p)); p = beg + size
    except t.Malformed:
        return MALFORMED, []
    if s1: return UNCLES, []                                                                 # clique.go:450-455; block_validator.go:67 with zk_headers.h's UncleHash rule
    return OK, extents

def split_all(bodies, start=0):
    """zkBodySplit over bodies laid end to end from byte `start` of a buffer -> dict(k, n, block_first, body_status, tx_beg, tx_size, txs: the transactions' bytes, packed,
    off: the packed bytes and the running sum of the sizes)"""
    status, first, beg, size, txs = [], [0], [], [], []; at = start
    for raw in bodies:
        st, ext = split(raw); status.append(st)
        for b, s in ext: beg.append(at + b); size.append(s); txs.append(bytes(raw[b:b + s]))
        first.append(len(beg)); at += len(raw)
    off = [0]
    for s in size: off.append(off[-1] + s)
    k = next((b for b in range(len(bodies)) if status[b] != OK), len(bodies))
    return dict(k=k, n=len(beg), block_first=first, body_status=status, tx_beg=beg, tx_size=size, txs=txs, packed=b"".join(txs), off=off)

def chain_raw_bodies(bodies, want_roots, signer, chain_id, chain_accounts, sizes_now):
    """verifyChainRawBodies: the split, then tx_roots_model.chain_bodies_roots on the transactions it found, where a body that is not OK has no root — so it is B0 at the
    latest.  -> (k, chain_bodies_roots' dict and the split's) or raises bodies_model.Refused"""
    s = split_all(bodies)
    def roots_of(raws, block_first):
        roots, defined = rm.tx_roots(raws, block_first)
        return [r if st == OK else bytes(32) for r, st in zip(roots, s["body_status"])], [d and st == OK for d, st in zip(defined, s["body_status"])]
    k, o = rm.chain_bodies_roots(s["txs"], s["block_first"], want_roots, signer, chain_id, chain_accounts, sizes_now, roots_of=roots_of)
    o.update(n_txs=s["n"], block_first=s["block_first"], body_status=s["body_status"], tx_beg=s["tx_beg"], tx_size=s["tx_size"]); return k, o
