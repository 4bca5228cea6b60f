"""The Merkle-Patricia trie of the reference on Python objects: the model of include/zk_tx_roots.h.  Two pieces:
  Trie          a restatement of trie/trie.go's insert (:218-285) and of the hasher (trie/hasher.go:77-199, trie/encoding.go hexToCompact, trie/node.go EncodeRLP) for
                arbitrary keys and values: nodes under 32 bytes are embedded, a branch has a value slot.  It is general so that the reference's own vectors
                (tests/golden/trie_vectors.txt) can pin it.
  derive_sha    core/types/derive_sha.go:32-41 on it: rlp(i) -> values[i].
and, beside them, level_root: the rules the device follows (sorted positions, adjacent prefixes, runs), which need every value to have at least 32 bytes.
The hash function is a parameter; callers memoise it.  The Go code cannot run where these tests run: every rule carries its citation."""
import os
import tx_model as t

EMPTY_ROOT = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")   # trie/trie.go:32

def vectors():
    """tests/golden/trie_vectors.txt -> dict(empty_root, inserts [(root, [(key, value)])], block_tx, block_txhash)"""
    out = {"inserts": []}
    for line in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trie_vectors.txt")):
        w = line.split()
        if not w or w[0].startswith("#"): continue
        if w[0] == "insert": out["inserts"].append((bytes.fromhex(w[1]), [tuple(x.encode() for x in kv.split("=")) for kv in w[2:]]))
        else: out[w[0]] = bytes.fromhex(w[1])
    return out

# ---- encoding.go ------------------------------------------------------------------------------------------------------------------------------------------------------
def key_to_hex(key):                                             # keybytesToHex :65-75: two nibbles a byte, then the terminator 16
    out = []
    for b in bytes(key): out += [b >> 4, b & 15]
    return out + [16]
def hex_to_compact(hexkey):                                      # hexToCompact :37-51
    hexkey = list(hexkey); term = 0
    if hexkey and hexkey[-1] == 16: term = 1; hexkey = hexkey[:-1]
    first = term << 5
    if len(hexkey) & 1: first |= 1 << 4 | hexkey[0]; hexkey = hexkey[1:]
    return bytes([first]) + bytes(hexkey[k] << 4 | hexkey[k + 1] for k in range(0, len(hexkey), 2))

# ---- trie.go, hasher.go -------------------------------------------------------------------------------------------------------------------------------------------
# a node: None | ("value", bytes) | ("short", hex key, node) | ("full", [17 nodes])
def _prefix_len(a, b):
    k = 0
    while k < len(a) and k < len(b) and a[k] == b[k]: k += 1
    return k
def _insert(n, key, value):                                      # trie.go:218-285 (no database here: no hashNode)
    if not key: return value                                      # :219-224
    if n is None: return ("short", key, value)                    # :265-266
    if n[0] == "short":
        m = _prefix_len(key, n[1])
        if m == len(n[1]): return ("short", n[1], _insert(n[2], key[m:], value))                                              # :230-236
        branch = [None] * 17                                                                                                    # :238-247
        branch[n[1][m]] = _insert(None, n[1][m + 1:], n[2]); branch[key[m]] = _insert(None, key[m + 1:], value)
        return ("full", branch) if m == 0 else ("short", key[:m], ("full", branch))                                             # :249-253
    assert n[0] == "full"
    kids = list(n[1]); kids[key[0]] = _insert(kids[key[0]], key[1:], value); return ("full", kids)                              # :255-263

class Trie:
    def __init__(self, keccak=t.keccak256): self.root = None; self.keccak = keccak
    def update(self, key, value):
        assert len(value) > 0                                     # (TryUpdate :203-214: an empty value deletes; not modelled)
        self.root = _insert(self.root, key_to_hex(key), ("value", bytes(value)))
    def _encode(self, n):
        """the RLP of the collapsed node (hasher.go:124-161 hashChildren, node.go EncodeRLP): a value as a string, nil as the empty string, a child by _ref"""
        if n[0] == "short": return t.enc_list([t.enc_str(hex_to_compact(n[1])), self._ref(n[2])])
        return t.enc_list([self._ref(c) for c in n[1]])
    def _ref(self, n):
        if n is None: return b"\x80"
        if n[0] == "value": return t.enc_str(n[1])
        enc = self._encode(n)
        return enc if len(enc) < 32 else t.enc_str(self.keccak(enc))                                                            # hasher.go:176-178: under 32 bytes it stays inside its parent
    def hash(self):
        if self.root is None: return EMPTY_ROOT                   # trie.go:446-453 Hash -> hashRoot :469-476
        return self.keccak(self._encode(self.root))               # force = true: the root is hashed whatever its size

    def hash_many(self, keccak_many):
        """hash() with a hash function that takes a list of messages: the nodes of one height go through it together, the lowest first"""
        if self.root is None: return EMPTY_ROOT
        levels = []                                                # levels[h]: the short and full nodes of height h (a value or nil below them: height 0)
        def height(n):
            if n is None or n[0] == "value": return -1
            h = 1 + (height(n[2]) if n[0] == "short" else max(height(c) for c in n[1]))
            while len(levels) <= h: levels.append([])
            levels[h].append(n); return h
        height(self.root); memo = {}; ref = {}
        def encode(n):                                             # _encode with the references of the levels below taken from ref
            items = [n[2]] if n[0] == "short" else n[1]
            refs = [b"\x80" if c is None else t.enc_str(c[1]) if c[0] == "value" else ref[id(c)] for c in items]
            return t.enc_list([t.enc_str(hex_to_compact(n[1]))] + refs) if n[0] == "short" else t.enc_list(refs)
        for nodes in levels:
            encs = [encode(n) for n in nodes]; big = sorted(set(x for x in encs if len(x) >= 32 and x not in memo))
            memo.update(zip(big, keccak_many(big)))
            for n, enc in zip(nodes, encs): ref[id(n)] = enc if len(enc) < 32 else t.enc_str(memo[enc])
        root = encode(self.root); return memo[root] if root in memo else keccak_many([root])[0]   # force = true

def derive_sha(values, keccak=t.keccak256, keccak_many=None):
    """core/types/derive_sha.go:32-41: keybuf = rlp(uint(i)), trie.Update(keybuf, list.GetRlp(i)), trie.Hash().  keccak_many: a hash function over a list of messages
    (the device's sponge takes many at once); the trie is the same, its nodes are hashed a height at a time"""
    tr = Trie(keccak)
    for i, v in enumerate(values): tr.update(t.enc_int(i), v)
    return tr.hash_many(keccak_many) if keccak_many else tr.hash()

def tx_value(raw):
    """rlp.EncodeToBytes(tx) of a transaction that decodes (derive_sha.go:38 GetRlp): the re-encoding, which differs from the input in a 0xC0 recipient only"""
    return t.encode(t.decode(raw)[0])

# ---- the rules the device follows -------------------------------------------------------------------------------------------------------------------
def key_nibbles(i): return key_to_hex(t.enc_int(i))[:-1]
def sorted_indices(n):
    """the indices of a list of n values in the order of their keys as byte strings: 1 .. min(n - 1, 127), then 0, then 128 .. n - 1"""
    if n == 0: return []
    m = min(n - 1, 127); return list(range(1, m + 1)) + [0] + list(range(128, n))
def level_root(values, keccak=t.keccak256):
    """the root from leaves, runs and adjacent prefixes alone; every value has at least 32 bytes, so every node is referenced by its hash"""
    n = len(values)
    if n == 0: return EMPTY_ROOT
    assert all(len(v) >= 32 for v in values)
    order = sorted_indices(n); keys = [key_nibbles(i) for i in order]
    lam = [-1] + [_prefix_len(keys[s - 1], keys[s]) for s in range(1, n)] + [-1]                    # lam[s]: the common prefix of the keys at s - 1 and s; -1 at both ends
    node = [None] * n
    for s in range(n):                                                                                # a leaf holds its key from max(lam[s], lam[s + 1]) + 1 on
        node[s] = keccak(t.enc_list([t.enc_str(hex_to_compact(keys[s][max(lam[s], lam[s + 1]) + 1:] + [16])), t.enc_str(values[order[s]])]))
    for d in range(max(len(k) for k in keys) - 1, -1, -1):                                            # one pass a depth, deepest first
        for s in range(n):
            if len(keys[s]) <= d or (s > 0 and lam[s] >= d): continue                                 # not the head of a run of keys that share d nibbles
            e = s + 1
            while e < n and lam[e] >= d: e += 1
            if e - s < 2 or _prefix_len(keys[s], keys[e - 1]) != d: continue                          # a branch at depth d: two members or more, first and last share exactly d
            kids = [b"\x80"] * 17; p = s
            while p < e:                                                                              # its children: the heads of its (d + 1)-runs
                kids[keys[p][d]] = t.enc_str(node[p]); p += 1
                while p < e and lam[p] >= d + 1: p += 1
            h = keccak(t.enc_list(kids)); P = max(lam[s], lam[e])
            if d > P + 1: h = keccak(t.enc_list([t.enc_str(hex_to_compact(keys[s][P + 1:d])), t.enc_str(h)]))   # an extension over nibbles [P + 1, d)
            node[s] = h
    return node[0]
