"""The proof cache without a device (include/zk_proof_cache.h; DESIGN.md "Proof cache"): the record digest's host model against hashlib, the Python model of the
two generations that tests/test_gpu_proof_cache.py compares the device cache with, and the entries' behaviour where no device is visible."""
import ctypes, hashlib, os, subprocess, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)

SALT = bytes(range(100, 132))
TAGS = [hashlib.sha256(b"tag of kind %d" % k).digest() for k in range(4)]
FLIP_BYTES = (0, 1, 7, 8, 15, 16, 527, 528, 703, 704, 719)   # the ends of every field, both sides of the last block boundary, the last byte

def record_key(salt, tag, rec):
    """the key of one record (720 bytes) under a salt and the tag of its kind's verifying key"""
    rec = bytes(rec); assert len(salt) == 32 and len(tag) == 32 and len(rec) == 720
    return hashlib.sha256(salt + tag + rec).digest()[:20]

def model_digests(salt, tags, recs):
    """what zkgpu_test_record_digests writes: the key of every record of kind 0..3, 20 zero bytes for any other kind"""
    raw = np.ascontiguousarray(recs).tobytes(); out = []
    for i in range(len(recs)):
        r = raw[720 * i:720 * i + 720]; out.append(record_key(salt, tags[r[0]], r) if r[0] <= 3 else bytes(20))
    return out

class CacheModel:
    """The two generations of ProofCache.  A key is any hashable value, None for a record that has none (it is never looked up and never stored).
    lookup: a key in either generation is a hit; nothing moves.  insert: the candidates in record order; more than capacity / 2 of them are cut to the first
    capacity / 2; if young would grow past capacity / 2 the old generation is dropped and young becomes old; then each candidate young does not hold is added."""
    def __init__(self, capacity):
        assert capacity >= 2; self.half = capacity // 2; self.young = {}; self.old = {}; self.hits = self.misses = self.inserted = 0
    def entries(self): return len(self.young) + len(self.old)
    def stats(self): return (self.hits, self.misses, self.inserted, self.entries())
    def lookup(self, keys):
        hit = [k is not None and (k in self.young or k in self.old) for k in keys]; keyed = sum(k is not None for k in keys)
        self.hits += sum(hit); self.misses += keyed - sum(hit); return hit
    def insert(self, candidates):
        cand = list(candidates)[:self.half]
        if not cand: return
        if len(self.young) + len(cand) > self.half: self.old = self.young; self.young = {}
        for k in cand:
            if k not in self.young: self.young[k] = True; self.inserted += 1
    def clear(self): self.young = {}; self.old = {}
    def call(self, keys, verdict):
        """one cached proof step: verdict[i] = what verification says of record i -> (ok, hit)"""
        hit = self.lookup(keys); ok = [bool(h or v) for h, v in zip(hit, verdict)]
        self.insert([k for k, h, v in zip(keys, hit, verdict) if k is not None and not h and v]); return ok, hit

def host_digests(recs):
    from blockmaze_amd import engine as e
    return [bytes(x) for x in e.record_digests(SALT, TAGS, recs, device=False)]

@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_host_digest_of_edge_records_equals_hashlib(kind):
    import block_records as br
    recs = br.edge_records(kind, 0xCAC4E + kind); recs["kind"] = kind; assert len(recs) > 1000
    assert host_digests(recs) == model_digests(SALT, TAGS, recs)

def test_host_digest_of_random_records_small_counts_and_unknown_kinds():
    import block_records as br
    from blockmaze_amd import engine as e
    recs = np.concatenate([br.random_records(k, 300, 0x5EED + k) for k in range(4)]); np.random.default_rng(3).shuffle(recs)
    got = host_digests(recs); want = model_digests(SALT, TAGS, recs); assert got == want and len(set(got)) == len(recs)
    assert host_digests(recs[:0]) == [] and host_digests(recs[:1]) == want[:1]
    odd = recs[:8].copy(); odd["kind"] = [4, 255, 0, 4, 1, 255, 2, 3]; got = host_digests(odd)
    assert got == model_digests(SALT, TAGS, odd) and [g == bytes(20) for g in got] == [True, True, False, True, False, True, False, False]
    # the tag and the salt are part of the key
    other = [bytes(x) for x in e.record_digests(bytes(32), TAGS, recs[:4], device=False)]; assert all(a != b for a, b in zip(other, want[:4]))
    other = [bytes(x) for x in e.record_digests(SALT, TAGS[1:] + TAGS[:1], recs[:4], device=False)]; assert all(a != b for a, b in zip(other, want[:4]))

def test_one_flipped_bit_is_another_key():
    import block_records as br
    base = np.concatenate([br.random_records(k, 1, 0xB17 + k) for k in range(4)]); recs = []; at = []
    for r in range(4):
        for byte in FLIP_BYTES[1:]:
            for bit in (0, 7):
                raw = bytearray(base[r:r + 1].tobytes()); raw[byte] ^= 1 << bit; recs.append(bytes(raw)); at.append((r, byte, bit))
        raw = bytearray(base[r:r + 1].tobytes()); raw[0] ^= 1 if r != 0 else 2; recs.append(bytes(raw)); at.append((r, 0, 0))   # byte 0 is the kind: a flip that stays a known kind
    from blockmaze_amd import engine as e
    arr = np.frombuffer(b"".join(recs), dtype=e.RECORD_DTYPE); got = host_digests(arr); want = model_digests(SALT, TAGS, arr); orig = host_digests(base)
    assert got == want and {a[1] for a in at} == set(FLIP_BYTES)
    for g, (r, byte, bit) in zip(got, at): assert g != orig[r], (r, byte, bit)
    assert len(set(got)) == len(got)

def test_cache_model_generations():
    m = CacheModel(8); assert m.half == 4
    ok, hit = m.call(list("abc"), [1, 1, 0]); assert ok == [True, True, False] and hit == [False] * 3 and m.stats() == (0, 3, 2, 2)
    ok, hit = m.call(["a", "c", None, "d"], [0, 1, 1, 1]); assert ok == [True, True, True, True] and hit == [True, False, False, False] and m.stats() == (1, 5, 4, 4)   # None: verified, never stored
    m.call(["e"], [1]); assert list(m.young) == ["e"] and list(m.old) == ["a", "b", "c", "d"] and m.entries() == 5           # young was full: a rotation before the insert
    ok, hit = m.call(["a", "e"], [0, 0]); assert hit == [True, True] and list(m.old) == ["a", "b", "c", "d"]                  # a hit in old is not refreshed
    m.call(list("fghijk"), [1] * 6); assert list(m.young) == list("fghi") and list(m.old) == ["e"] and m.entries() == 5       # six candidates: the first four, after a rotation
    ok, hit = m.call(["a", "j"], [1, 1]); assert hit == [False, False] and ok == [True, True]                                 # rotated out: verified again, stored again
    assert list(m.young) == ["a", "j"] and list(m.old) == list("fghi") and m.entries() <= 8
    m.call(["a", "a", "z"], [1, 1, 1]); assert list(m.young) == ["a", "j", "z"]                                                # a repeat inside a call is stored once
    m.clear(); assert m.entries() == 0 and m.lookup(["a"]) == [False]
    tiny = CacheModel(2); tiny.call(["a", "b"], [1, 1]); assert list(tiny.young) == ["a"] and tiny.entries() == 1
    tiny.call(["b"], [1]); assert list(tiny.young) == ["b"] and list(tiny.old) == ["a"] and tiny.entries() == 2

def declared_symbols(header):
    import re
    src = open(os.path.join(ROOT, "include", header)).read(); src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", " ".join(l for l in src.splitlines() if not l.strip().startswith("#")))) - {"defined", "sizeof"})

NO_DEVICE = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from blockmaze_amd import engine as e
L = e.lib(); L.zkProofCacheNew.restype = ctypes.c_void_p; L.zkgpu_proof_cache_create.restype = ctypes.c_void_p; L.zkgpu_test_proof_cache_create.restype = ctypes.c_void_p
assert e.device_count() == 0
assert L.zkProofCacheNew(ctypes.c_longlong(1000)) is None and L.zkProofCacheNew(ctypes.c_longlong(1)) is None
assert L.zkgpu_proof_cache_create(ctypes.c_uint64(1000)) is None and b"no HIP device" in L.zkgpu_last_error()
assert L.zkgpu_test_proof_cache_create(ctypes.c_uint64(8), bytes(32)) is None
out = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
assert L.zkProofCacheStats(None, out) == -1 and L.zkProofCacheClear(None) == -1 and list(out) == [7, 7, 7, 7]
L.zkProofCacheFree(None)
recs = np.zeros(3, dtype=e.RECORD_DTYPE); recs["kind"] = 9; ok = (ctypes.c_ubyte * 3)(1, 1, 1)
assert L.verifyRecordsCached(None, recs.ctypes.data_as(ctypes.c_void_p), 3, ok) == 0 and list(ok) == [0, 0, 0]   # no cache: verifyBlockRecords, which rejects an unknown kind
k = ctypes.c_uint64(5); assert L.zkgpu_test_proof_cache_launches(ctypes.byref(k)) == 0 and k.value == 0
try: e.record_digests(bytes(32), [bytes(32)] * 4, recs, device=True); raise SystemExit("the kernel road answered without a device")
except e.ZkGpuError: pass
print("NO DEVICE OK")
"""

def test_entries_without_a_device(tmp_path):
    """a process that sees no device: the library loads, every symbol of zk_proof_cache.h is there, no cache can be made, and NULL in place of a cache is the uncached entry"""
    from blockmaze_amd import engine as e
    syms = declared_symbols("zk_proof_cache.h"); assert syms == sorted(["zkProofCacheNew", "zkProofCacheFree", "zkProofCacheClear", "zkProofCacheStats", "verifyRecordsCached", "verifyBlockFullCached"])
    for s in syms: assert hasattr(e.lib(), s), s
    script = tmp_path / "no_device.py"; script.write_text(NO_DEVICE)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0 and "NO DEVICE OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
