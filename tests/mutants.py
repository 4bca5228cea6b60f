"""Seeded mutants of transactions, headers and bodies for the tests of include/zk_txs.h, zk_headers.h and zk_raw_bodies.h: inputs that nobody chose.  The corpora of
tests/tx_corpus.py, header_corpus.py and body_corpus.py hold one case for every rule their authors thought of; the mutators here damage a valid encoding blindly (a bit,
a byte, a cut) or with a view to the item heads (a head byte pushed across a form's border at any depth, an element that grew by a byte with every enclosing length
repaired, so that the damage reaches a deep rule and does not die at "the list ends where the input ends").  Everything is a function of a seed through random.Random;
tests/test_mutants_cpu.py shows with the models alone that the corpora are worth running, tests/test_gpu_mutants.py holds the device to the models on them."""
import random
import tx_model as t
import tx_corpus as tc
import header_corpus as hc
import body_model as bdm

EDGE = (0x00, 0x01, 0x37, 0x38, 0x7F, 0x80, 0x81, 0x94, 0xA0, 0xB7, 0xB8, 0xB9, 0xBF, 0xC0, 0xC1, 0xF7, 0xF8, 0xF9, 0xFF)

# ---- walkers over an encoding ---------------------------------------------------------------------------------------------------------------------------------------
def _tree(raw, max_depth=None):
    """[(position, kind, content start, size, depth, index of the enclosing list's entry or -1)], depth-first; ends quietly at the first malformed head"""
    raw = bytes(raw); out = []; stack = [(0, len(raw), 0, -1)]                # (pos, lim, depth, parent)
    try:
        while stack:
            pos, lim, depth, parent = stack.pop()
            if pos >= lim: continue
            kind, beg, size = t.read_head(raw, pos, lim); out.append((pos, kind, beg, size, depth, parent))
            stack.append((beg + size, lim, depth, parent))                    # the next item of the same list, behind this one's content
            if kind == "list" and (max_depth is None or depth < max_depth): stack.append((beg, beg + size, depth + 1, len(out) - 1))
    except t.Malformed: pass
    return out
def items(raw, max_depth=None):
    """every item header of raw, depth-first, as (position, kind, content start, size); the outer item has depth 0, and max_depth leaves out what lies deeper"""
    return [x[:4] for x in _tree(raw, max_depth)]
def fix_outer(raw):
    """raw with the outer list's header rewritten so that the list ends where the bytes end; bytes that do not begin with a list header are returned as they are"""
    raw = bytes(raw)
    if not raw or raw[0] < 0xC0: return raw
    hl = 1 if raw[0] < 0xF8 else 1 + raw[0] - 0xF7; payload = raw[hl:]; return t.head(0xC0, len(payload)) + payload

def _item_end(x): return x[2] + x[3]
def _encoded(kind, content): return t.head(0xC0 if kind == "list" else 0x80, len(content)) + content
def _replace(raw, tree, k, new, repair=True):
    """raw with the whole encoding of item k replaced by `new`; repair: the header of every enclosing list is encoded again, up to the outermost"""
    pos, end, parent = tree[k][0], _item_end(tree[k]), tree[k][5]
    while repair and parent >= 0:
        p = tree[parent]; new = _encoded("list", raw[p[2]:pos] + new + raw[end:_item_end(p)]); pos, end, parent = p[0], _item_end(p), p[5]
    return raw[:pos] + new + raw[end:]

# ---- the mutators: (rng, raw) -> bytes ------------------------------------------------------------------------------------------------------------------------------
def m1(rng, raw):
    """flip one bit"""
    if not raw: return raw
    k = rng.randrange(len(raw)); return raw[:k] + bytes([raw[k] ^ (1 << rng.randrange(8))]) + raw[k + 1:]
def m2(rng, raw):
    """a random byte set to an EDGE byte"""
    if not raw: return raw
    k = rng.randrange(len(raw)); return raw[:k] + bytes([rng.choice(EDGE)]) + raw[k + 1:]
def _head_byte(rng, raw, tree, how):
    if not tree: return m2(rng, raw)
    k = tree[rng.randrange(len(tree))][0]; b = rng.choice(EDGE) if how == "edge" else (raw[k] + rng.choice((1, -1))) & 0xFF; return raw[:k] + bytes([b]) + raw[k + 1:]
def m3(rng, raw):
    """the first byte of a random item header set to an EDGE byte"""
    return _head_byte(rng, raw, _tree(raw), "edge")
def m4(rng, raw):
    """+1 or -1 on the first byte of a random item header"""
    return _head_byte(rng, raw, _tree(raw), "step")
def m5(rng, raw):
    """one byte deleted, the outer header repaired"""
    if not raw: return raw
    k = rng.randrange(len(raw)); return fix_outer(raw[:k] + raw[k + 1:])
def m6(rng, raw):
    """an EDGE byte inserted, the outer header repaired"""
    k = rng.randrange(len(raw) + 1); return fix_outer(raw[:k] + bytes([rng.choice(EDGE)]) + raw[k:])
def m7(rng, raw):
    """cut at a random position, one time in eight within the first three bytes"""
    return raw[:rng.randrange(3) if rng.randrange(8) == 0 else rng.randrange(len(raw) + 1)]
def _resize(rng, raw, repair):
    tree = _tree(raw)
    if not tree: return m2(rng, raw)
    k = rng.randrange(len(tree)); pos, kind, beg, size = tree[k][:4]; content = raw[beg:beg + size]; at = rng.randrange(size + 1)
    if size and rng.randrange(2): at = min(at, size - 1); content = content[:at] + content[at + 1:]
    else: content = content[:at] + bytes([rng.randrange(256)]) + content[at:]
    return _replace(raw, tree, k, _encoded(kind, content), repair)
def m8(rng, raw):
    """a random item's content grown or shrunk by one byte and its header encoded again, and so the header of every enclosing list"""
    return _resize(rng, raw, True)
def m9(rng, raw):
    """M8 with the enclosing headers left as they are"""
    return _resize(rng, raw, False)
def m10(rng, raw):
    """a short-form header in the long form ("long form below 56": at the item's own size or, half the time, with a content of 55 bytes, the border), a long form with a
    zero byte in front of its length, or a zero byte in front of a uint's content, the lengths around it repaired: the directed road to the two leading-zero rules"""
    tree = _tree(raw); way = rng.randrange(3)
    short = [k for k, x in enumerate(tree) if x[1] != "byte" and x[2] == x[0] + 1]; long_ = [k for k, x in enumerate(tree) if 1 < x[2] - x[0] < 9]   # (a length of 8 bytes has no wider form)
    uints = [k for k, x in enumerate(tree) if x[1] == "byte" or (x[1] == "str" and 1 <= x[3] <= 8)]
    if way == 0 and short:
        k = rng.choice(short); pos, kind, beg, size = tree[k][:4]; content = raw[beg:beg + size]
        if rng.randrange(2): content = bytes(1 + rng.randrange(0x7F) for _ in range(55)) if kind == "list" else (content + rng.randbytes(55))[:55]   # at the border: the largest size that is refused
        new = bytes([(0xF8 if kind == "list" else 0xB8), len(content)]) + content
    elif way == 1 and long_:
        k = rng.choice(long_); pos, kind, beg, size = tree[k][:4]; new = bytes([(raw[pos] + 1) & 0xFF, 0]) + raw[pos + 1:beg + size]
    elif uints:
        k = rng.choice(uints); pos, kind, beg, size = tree[k][:4]; new = _encoded("str", b"\x00" + raw[beg:beg + size])
    else: return m2(rng, raw)
    return _replace(raw, tree, k, new)
def m11(rng, raw):
    """one to three bytes behind the outer list"""
    return raw + bytes(rng.choice(EDGE) if rng.randrange(2) else rng.randrange(256) for _ in range(1 + rng.randrange(3)))
def m12(rng, raw):
    """for bodies: M3 or M4 on a header of depth 2 or less — the outer list, Transactions, Uncles and each element's head: the only bytes the split reads"""
    return _head_byte(rng, raw, _tree(raw, 2), "edge" if rng.randrange(2) else "step")
def m13(rng, raw):
    """a random string grown by 2 .. 135 bytes or cut to a random length, every length around it repaired: a decodable mutant of any length mod 136 (where the field
    takes any length), so that the sponges meet every phase of their rate-block edges and seams"""
    tree = _tree(raw); strs = [k for k, x in enumerate(tree) if x[1] == "str"]
    if not strs: return m2(rng, raw)
    k = rng.choice(strs); beg, size = tree[k][2:4]; content = raw[beg:beg + size]
    content = content[:rng.randrange(size + 1)] if rng.randrange(3) == 0 else content + rng.randbytes(2 + rng.randrange(134))
    return _replace(raw, tree, k, t.enc_str(content))
def m14(rng, raw):
    """for headers: a field whose length is free, every length around it repaired.  Two times in three the thirteenth item of the outer list, Extra, at a random length
    of 0 .. 299 bytes: accepted headers have Extra of 97 + 20 k bytes only, these have the header's and the seal's message at every length mod 136.  Otherwise the
    eighth or the twelfth, Difficulty or Time, as an integer of 1 .. 40 bytes: what stands before Extra in the seal's message, and so its first seam, moves"""
    tree = _tree(raw, 1); inner = [k for k, x in enumerate(tree) if x[4] == 1]
    if len(inner) < 13 or tree[inner[12]][1] == "list": return m13(rng, raw)
    if rng.randrange(3): return _replace(raw, tree, inner[12], t.enc_str(rng.randbytes(rng.randrange(300))))
    return _replace(raw, tree, inner[rng.choice((7, 11))], t.enc_str(bytes([1 + rng.randrange(255)]) + rng.randbytes(rng.randrange(40))))

BLIND = (("M1", m1), ("M2", m2), ("M3", m3), ("M4", m4), ("M5", m5), ("M6", m6), ("M7", m7), ("M8", m8), ("M9", m9), ("M10", m10), ("M11", m11), ("M13", m13))
HEADER = BLIND + (("M14", m14),) * 4                             # one header mutant in four has an Extra of a free length
def mutate(rng, raw, mutators=BLIND):
    """-> (the mutator's name, the mutant); one time in four a second mutator works on what the first has left"""
    name, fn = mutators[rng.randrange(len(mutators))]; out = fn(rng, bytes(raw))
    if rng.randrange(4) == 0: name2, fn2 = mutators[rng.randrange(len(mutators))]; out = fn2(rng, out); name += "+" + name2
    return name, out

# ---- the corpora ----------------------------------------------------------------------------------------------------------------------------------------------------
# what both test files run: tests/test_mutants_cpu.py states its conditions on exactly the inputs that tests/test_gpu_mutants.py hands to the device
TX_SEED, TX_COUNT, BODY_SEED, BODY_COUNT, HEADER_SEEDS = 1, 6000, 2, 6000, tuple(range(100, 112))
_VALID = []
def valid_txs():
    if not _VALID: _VALID.extend(tc.valid_cases())
    return _VALID
def tx_mutants(seed, count):
    """[(label, mutant, signer, chain_id, base)]: mutants of tx_corpus.valid_cases(), each with its base's signer and chain id and the base's bytes"""
    rng = random.Random(seed); valid = valid_txs(); out = []
    for _ in range(count):
        label, raw, signer, chain_id = valid[rng.randrange(len(valid))]; name, mut = mutate(rng, raw); out.append(("%s of %s" % (name, label), mut, signer, chain_id, raw))
    return out
def header_chains(seed):
    """-> (headers, parent, bases): header_corpus.chain(CHAIN_SEED, 257) with every header replaced by a mutant of itself with probability 1/2, so that the links of the
    batch sometimes hold and sometimes break; bases: the chain as it was"""
    bases, parent, _ = _chain(); rng = random.Random(seed)
    return [mutate(rng, raw, HEADER)[1] if rng.randrange(2) else raw for raw in bases], parent, list(bases)
_CHAIN = []
def _chain():
    if not _CHAIN: _CHAIN.append(hc.chain(hc.CHAIN_SEED, 257))
    return _CHAIN[0]
def body_mutants(seed, count):
    """[(mutant, base)]: bodies of 0 .. 5 elements, each element a valid transaction or a lone byte, no uncle; mutated with M12 half the time, otherwise as mutate does"""
    rng = random.Random(seed); valid = valid_txs(); out = []
    for _ in range(count):
        base = bdm.body([valid[rng.randrange(len(valid))][1] if rng.randrange(2) else bytes([rng.randrange(0x80)]) for _ in range(rng.randrange(6))])
        out.append((m12(rng, base) if rng.randrange(2) else mutate(rng, base)[1], base))
    return out
