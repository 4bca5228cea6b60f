"""Bodies for the tests of include/zk_raw_bodies.h: every way to be malformed that the header lists, each built from a body that is accepted; the uncle rule; elements
that are no transactions; each head form at each payload length.  Each case names the status and the number of transactions it claims; tests/test_raw_bodies_cpu.py
holds every one to that claim with the model (tests/body_model.py), and tests/test_gpu_raw_bodies.py holds the device to the model."""
import tx_model as t
import bodies_corpus as bc
import body_model as bdm

def head_long(base, n, width):
    """a list (base 0xC0) or string (0x80) head in the long form with `width` size bytes, canonical or not"""
    return bytes([base + 55 + width]) + n.to_bytes(width, "big")

def cases(seed=41):
    """[(label, claimed status, body, claimed number of transactions)]"""
    pool = bc.Pool(seed=seed); txs = [pool.zk[0], pool.public[0], pool.zk[1]]; good = bdm.body(txs); out = []
    item0 = t.enc_list(txs); p0 = b"".join(txs); payload = item0 + b"\xc0"
    def put(label, claim, raw, n=0): out.append((label, claim, bytes(raw), n))
    put("accepted", bdm.OK, good, 3)
    put("accepted, no transaction", bdm.OK, bdm.body([]), 0)
    put("accepted, one transaction", bdm.OK, bdm.body(txs[:1]), 1)
    # MALFORMED, each from the accepted body
    put("empty", bdm.MALFORMED, b"")
    put("outer a string", bdm.MALFORMED, t.head(0x80, len(payload)) + payload)
    put("outer a lone byte", bdm.MALFORMED, b"\x05")
    put("outer payload one byte short", bdm.MALFORMED, good + b"\x00")                              # the list ends one byte before the input does
    put("outer payload one byte long", bdm.MALFORMED, good[:-1])                                    # the list ends one byte behind the input
    put("outer head cut", bdm.MALFORMED, good[:1])
    put("no item", bdm.MALFORMED, b"\xc0")
    put("one item", bdm.MALFORMED, t.enc_list([item0]))
    put("three items", bdm.MALFORMED, t.enc_list([item0, b"\xc0", b"\xc0"]))
    put("three items, the last a byte", bdm.MALFORMED, t.enc_list([item0, b"\xc0", b"\x01"]))
    put("item 0 a string", bdm.MALFORMED, t.enc_list([t.head(0x80, len(p0)) + p0, b"\xc0"]))
    put("item 0 a lone byte", bdm.MALFORMED, t.enc_list([b"\x01", b"\xc0"]))
    put("item 1 a string", bdm.MALFORMED, t.enc_list([item0, b"\x80"]))
    put("item 1 a lone byte", bdm.MALFORMED, t.enc_list([item0, b"\x7f"]))
    put("item 1 overruns the body", bdm.MALFORMED, t.head(0xC0, len(item0) + 1) + item0 + b"\xc1")
    # an element head that overruns item 0: the last transaction's head claims one byte more than item 0 holds
    last = txs[-1]; kind, beg, size = t.read_head(last, 0, len(last)); longer = t.head(0xC0, size + 1) + last[beg:]; assert len(longer) == len(last)
    put("an element head overruns item 0", bdm.MALFORMED, t.enc_list([t.enc_list(txs[:-1] + [longer]), b"\xc0"]))
    put("an element head cut by item 0's end", bdm.MALFORMED, t.enc_list([t.enc_list(txs[:-1] + [b"\xf9\x01"]), b"\xc0"]))
    # each non-canonical head form, on an element of item 0, on item 0, on item 1 and on the outer list
    small = t.enc_list([b"\x01" * 3]); assert small[0] == 0xC3
    put("element: long form under 56", bdm.MALFORMED, t.enc_list([t.enc_list(txs + [head_long(0xC0, 3, 1) + small[1:]]), b"\xc0"]))
    put("element: a leading zero length byte", bdm.MALFORMED, t.enc_list([t.enc_list([head_long(0xC0, len(txs[0]) - 3, 3) + txs[0][3:]] + txs[1:]), b"\xc0"]))
    put("element: 81 05", bdm.MALFORMED, t.enc_list([t.enc_list(txs + [b"\x81\x05"]), b"\xc0"]))
    put("element: string in long form under 56", bdm.MALFORMED, t.enc_list([t.enc_list(txs + [head_long(0x80, 3, 1) + b"abc"]), b"\xc0"]))
    put("item 0: long form under 56", bdm.MALFORMED, t.enc_list([head_long(0xC0, 3, 1) + small[1:], b"\xc0"]))
    put("item 0: a leading zero length byte", bdm.MALFORMED, t.enc_list([head_long(0xC0, len(p0), 3) + p0, b"\xc0"]))
    put("f8 00 as the uncle list", bdm.MALFORMED, t.enc_list([item0, b"\xf8\x00"]))
    put("uncles: a leading zero length byte", bdm.MALFORMED, t.enc_list([item0, head_long(0xC0, 60, 2) + bytes(60)]))
    put("outer: long form under 56", bdm.MALFORMED, head_long(0xC0, 2, 1) + b"\xc0\xc0")
    put("outer: a leading zero length byte", bdm.MALFORMED, head_long(0xC0, len(payload), 3) + payload)
    assert len(txs[0]) > 255 and len(p0) > 255 and len(payload) > 255                               # (the three-byte forms above have a zero first)
    # UNCLES: the list is canonical and not empty, whatever it holds; MALFORMED goes first
    header_shaped = t.enc_list([t.enc_str(bytes(32)), t.enc_str(bytes(32)), t.enc_str(bytes(20))] + [t.enc_str(bytes(32))] * 3 + [t.enc_str(bytes(256)), b"\x02", b"\x05", b"\x80", b"\x80", b"\x07",
                               t.enc_str(bytes(97)), t.enc_str(bytes(32)), t.enc_str(bytes(8)), t.enc_str(bytes(32)), b"\xc0"])
    put("one header-shaped uncle", bdm.UNCLES, bdm.body(txs, [header_shaped]))
    put("a junk uncle", bdm.UNCLES, bdm.body(txs, [b"\x05"]))
    put("junk bytes in the uncle list", bdm.UNCLES, t.enc_list([item0, b"\xc3\xff\xff\xff"]))       # canonical as a list; what it holds is not looked at
    put("an uncle and no transaction", bdm.UNCLES, bdm.body([], [header_shaped]))
    put("a bad element head and an uncle", bdm.MALFORMED, t.enc_list([t.enc_list(txs + [b"\x81\x05"]), t.enc_list([header_shaped])]))
    # elements that are no transactions: the body is OK, the walk refuses the transaction
    put("an element that is a string", bdm.OK, bdm.body([txs[0], t.enc_str(b"not a transaction"), txs[1]]), 3)
    put("an element that is a lone byte", bdm.OK, bdm.body([b"\x05", txs[0]]), 2)
    put("an element that is an empty string", bdm.OK, bdm.body([b"\x80"]), 1)
    put("an element that is an empty list", bdm.OK, bdm.body([txs[2], b"\xc0"]), 2)
    put("a malformed transaction", bdm.OK, bdm.body([txs[0], t.enc_list(t.encode_items(t.decode(txs[1])[0])[:-1])]), 2)   # a field short
    put("a transaction cut short eats into item 1", bdm.MALFORMED, bdm.body([txs[0], pool.refused[0]]))               # its head claims a byte that item 0 does not hold
    return out

def sized_list(n):
    """the payload of a list of exactly n bytes made of canonical elements: strings of 200 bytes, then a string and lone bytes that fill the rest"""
    out = b""
    while n - len(out) > 260: out += t.enc_str(bytes([0xAB]) * 200)
    rest = n - len(out)
    if rest >= 58: size = min(rest - 2, 255); out += t.enc_str(bytes([0xAB]) * size); rest -= size + 2
    return out + b"\x05" * rest

def head_form_bodies():
    """[(label, body)]: the outer list and item 0 at each payload length class — under 56, 56 .. 255, 256 .. 65,535, 65,536 and more — and at the borders between them"""
    out = []
    for n in (0, 1, 52, 53, 54, 55, 56, 57, 252, 253, 254, 255, 256, 257, 300, 65531, 65532, 65533, 65535, 65536, 65537, 70000):
        p = sized_list(n); raw = t.enc_list([t.head(0xC0, n) + p, b"\xc0"]); out.append(("item 0 of %d bytes" % n, raw))
    return out
