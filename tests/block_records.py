"""Block records (include/zk_records.h) for the tests: seeded random records, the edge cases of the converter, and independent models of what the ingest must
make of a record — the packed statement by workload.pack_public, the proof's coordinates by integer arithmetic modulo q."""
import random
import numpy as np
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import workload as w

Q = o.Q_MOD
KINDS = {"mint": 0, "send": 1, "deposit": 2, "redeem": 3}
N_INPUTS = {0: 4, 1: 5, 2: 6, 3: 4}
N_BITS = {0: 832, 1: 1024, 2: 1440, 3: 832}
SLOT = [0, 1, 3, 2, 5, 4, 6, 7]   # hex order A.x A.y B.x.c1 B.x.c0 B.y.c1 B.y.c0 C.x C.y -> the proof record's A.x A.y B.x.c0 B.x.c1 B.y.c0 B.y.c1 C.x C.y
_HEX = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)

def statement_fields(kind):
    """the byte ranges of a record that make up the kind's statement, in order: (field, index or None, length)"""
    if kind in (0, 3): return [("args", 0, 32), ("args", 1, 32), ("args", 2, 32), ("value_s", None, 8)]
    if kind == 1: return [("args", k, 32) for k in range(4)]
    return [("args", 0, 32), ("args", 1, 20)] + [("args", k, 32) for k in range(2, 6)]

def random_records(kind, n, seed, canonical=False):
    """n records of a kind with random statements, random 256-bit coordinates (most of them q or more: aliases; canonical: all below q) and garbage wherever the
    layout says `ignored`"""
    rng = np.random.default_rng(seed); r = np.zeros(n, dtype=e.RECORD_DTYPE); r["kind"] = kind
    r["reserved"] = rng.integers(0, 256, (n, 7), dtype=np.uint8); r["value_s"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    r["args"] = rng.integers(0, 256, (n, 6, 32), dtype=np.uint8); r["proof"] = _HEX[rng.integers(0, 16, (n, 512))]
    if canonical: r["proof"][:, 0::64] = _HEX[rng.integers(0, 3, (n, 8))]                    # (q = 0x3064...: a leading digit of 0, 1 or 2 is below it)
    return r

def set_coord(rec, k, value):
    """coordinate k (hex order) of one record := value, 64 lower-case digits"""
    rec["proof"][64 * k:64 * k + 64] = np.frombuffer(("%064x" % value).encode(), dtype=np.uint8)

def coordinate_values():
    """0, 1, q - 1, q, q + 1, kq + c for every k that stays below 2^256 (c = 0, 1, a fixed value, q - 1), 2^256 - 1"""
    c0 = random.Random(77).randrange(2, Q - 1); vals = [0, 1, Q - 1, Q, Q + 1, (1 << 256) - 1]
    for k in range(0, 6):
        for c in (0, 1, c0, Q - 1):
            if k * Q + c < (1 << 256): vals.append(k * Q + c)
    assert 5 * Q < (1 << 256) < 6 * Q
    return sorted(set(vals))

def coordinate_records(kind, seed, canonical=False):
    """every value of coordinate_values() in every one of the eight coordinates"""
    vals = coordinate_values(); r = random_records(kind, 8 * len(vals), seed, canonical)
    for i in range(len(r)): set_coord(r[i], i % 8, vals[i // 8])
    return r

BAD_BYTES = [ord("A"), ord("F"), 0, ord("g"), ord(" "), ord("/"), ord(":"), ord("`"), ord("G"), 0x80 | ord("1"), 0xff]
def bad_byte_records(kind, seed):
    """one byte that is no lower-case hex digit at the first, a middle and the last position of each of the eight coordinates -> (records, all to be unparsed)"""
    pos = [64 * k + p for k in range(8) for p in (0, 31, 63)]; r = random_records(kind, len(pos) * len(BAD_BYTES), seed)
    for i in range(len(r)): r["proof"][i, pos[i % len(pos)]] = BAD_BYTES[i // len(pos)]
    return r

def statement_records(kind, seed):
    """all-zero, all-ones and every single-bit statement, and value_s in {0, 1, 2^64 - 1}"""
    fields = statement_fields(kind); nbytes = sum(f[2] for f in fields); r = random_records(kind, 2 + 8 * nbytes + 3, seed)
    def put(rec, stream):
        at = 0
        for f, k, ln in fields:
            if f == "value_s": rec["value_s"] = int.from_bytes(stream[at:at + 8], "little")
            else: rec["args"][k][:ln] = np.frombuffer(stream[at:at + ln], dtype=np.uint8)
            at += ln
    put(r[0], bytes(nbytes)); put(r[1], b"\xff" * nbytes)
    for b in range(8 * nbytes):
        s = bytearray(nbytes); s[b // 8] = 1 << (b % 8); put(r[2 + b], bytes(s))
    for i, v in enumerate((0, 1, (1 << 64) - 1)): r["value_s"][2 + 8 * nbytes + i] = v
    return r

def edge_records(kind, seed):
    return np.concatenate([statement_records(kind, seed), coordinate_records(kind, seed + 1), bad_byte_records(kind, seed + 2)])

# ---- the models -----------------------------------------------------------------------------------------------------------
def model_inputs(rec):
    """the packed statement of one record by workload.pack_public"""
    kind = int(rec["kind"]); a = [bytes(rec["args"][k]) for k in range(6)]
    if kind in (0, 3): return w.pack_public(a[:3], extra_u64=int(rec["value_s"]))
    if kind == 1: return w.pack_public(a[:4])
    return w.pack_public([a[0], a[1][:20], a[2], a[3], a[4], a[5]])

def model_item(rec, strict=False):
    """(parsed, the eight Montgomery coordinates in the proof record's order): c mod q, times 2^256 mod q; all zero where the 512 bytes are not a proof"""
    p = bytes(rec["proof"])
    if any(ch not in b"0123456789abcdef" for ch in p): return 0, [0] * 8
    c = [int(p[64 * k:64 * k + 64], 16) for k in range(8)]
    if strict and any(x >= Q for x in c): return 0, [0] * 8
    out = [0] * 8
    for k in range(8): out[SLOT[k]] = (c[k] % Q) * (1 << 256) % Q
    return 1, out

def ints(a): return [[sum(int(x) << (64 * k) for k, x in enumerate(el)) for el in row] for row in a]

def check_against_models(recs, items, inputs, parsed, strict=False):
    kind = int(recs["kind"][0]); assert inputs.shape[1:] == (N_INPUTS[kind], 4) and items.shape[1:] == (8, 4)
    it, inp = ints(items), ints(inputs)
    for i in range(len(recs)):
        ok, c = model_item(recs[i], strict); assert int(parsed[i]) == ok and it[i] == c, (i, bytes(recs["proof"][i]))
        assert inp[i] == model_inputs(recs[i]), i

def same_arrays(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
