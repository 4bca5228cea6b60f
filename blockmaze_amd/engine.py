"""ctypes binding of libzkgpu.so's engine layer (include/zkgpu.h).

This is plumbing for tests and the benchmark: numpy arrays in, numpy arrays out, every call goes through the C-ABI into
the HIP kernels.  There is no Python or CPU implementation behind it — if the shared library is missing or no MI355X is
visible the calls raise.
"""
import ctypes, os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libzkgpu.so")
if os.environ.get("ZKGPU_LIB"): LIB_PATH = os.environ["ZKGPU_LIB"]   # (A/B of two builds on one box: tools/ab_device.py "ZKGPU_LIB=tools/other_build.bin")

class ZkGpuError(RuntimeError):
    pass

_lib = None
def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ZkGpuError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.zkgpu_last_error.restype = ctypes.c_char_p; L.zkgpu_version.restype = ctypes.c_char_p
        L.zkgpu_domain_size.restype = ctypes.c_size_t; L.zkgpu_domain_size.argtypes = [ctypes.c_size_t]
        L.zkgpu_msm_create.restype = ctypes.c_void_p; L.zkgpu_r1cs_create.restype = ctypes.c_void_p
        _lib = L
    return _lib

def _check(rc):
    if rc != 0:
        raise ZkGpuError("zkgpu error %d: %s" % (rc, lib().zkgpu_last_error().decode()))

def _bytes(a):
    a = np.ascontiguousarray(a); return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))

def device_count(): return int(lib().zkgpu_device_count())
def device_numa_node(device=0): return int(lib().zkgpu_device_numa_node(int(device)))   # -1 unknown
def init(): _check(lib().zkgpu_init())

# arrays are uint64 with 4 words per field element (canonical, little-endian), same convention as oracle/pyoracle.py
def field_op(field, op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.uint64); out = np.zeros_like(a); n = a.size // 4
    bb = np.ascontiguousarray(b, dtype=np.uint64) if b is not None else None
    _check(lib().zkgpu_test_field_op(field, {"mul": 0, "add": 1, "sub": 2, "inv": 3, "sqr": 4, "neg": 5, "mul_lazy": 6, "sqr_lazy": 7, "sub_lazy": 8, "neg_masked": 9}[op], _bytes(a), _bytes(bb) if bb is not None else None, _bytes(out), ctypes.c_size_t(n))); return out
def fq2_op(op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.uint64); out = np.zeros_like(a); n = a.size // 8
    bb = np.ascontiguousarray(b, dtype=np.uint64) if b is not None else None
    _check(lib().zkgpu_test_fq2_op({"mul": 0, "sqr": 1, "inv": 2}[op], _bytes(a), _bytes(bb) if bb is not None else None, _bytes(out), ctypes.c_size_t(n))); return out
def fq2_sqrt(a):
    """key load's fq2_sqrt (keyops.cuh) on (n, 8) words: (roots (n, 8), ok (n,) uint8); a root is zero where ok is 0"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 8); n = a.shape[0]; buf = np.zeros(65 * n, dtype=np.uint8)
    _check(lib().zkgpu_test_fq2_op(3, _bytes(a), None, _bytes(buf), ctypes.c_size_t(n))); return buf[:64 * n].copy().view(np.uint64).reshape(n, 8), buf[64 * n:].copy()
def group_op(group, op, a, b=None):
    """group 1: (n,8) words, group 2: (n,16) words.  op: add / dbl / madd / mul_small (b = uint32 multipliers)"""
    a = np.ascontiguousarray(a, dtype=np.uint64); out = np.zeros_like(a); n = a.shape[0]
    if op == "mul_small":
        bb = np.zeros_like(a); bb[:, 0] = np.asarray(b, dtype=np.uint64)
    else:
        bb = np.ascontiguousarray(b, dtype=np.uint64) if b is not None else None
    _check(lib().zkgpu_test_group_op(group, {"add": 0, "dbl": 1, "madd": 2, "mul_small": 3}[op], _bytes(a), _bytes(bb) if bb is not None else None, _bytes(out), ctypes.c_size_t(n))); return out

# raw-limb probes of the 29-bit-limb arithmetic (csrc/probe29.hip): uint32 arrays, nine limbs an element, nothing converted on the way
FIELD29_OPS = {"mul": 0, "mul2": 1, "sqr": 2, "norm": 3, "sub2": 4, "sub4": 5, "sub6": 6, "sub12": 7, "sub18": 8, "cond_neg": 9, "sub_product": 10, "neg_product": 11,
               "add_raw": 12, "barrett": 13, "one": 14, "unpack": 15, "pack_words": 16, "to_words": 17, "product_is_zero": 18, "ntt_lazy": 19}
POINT29_OPS = {"madd": (0, 36, 19, 36), "madd_pp": (1, 36, 19, 36), "dbl_affine": (2, 0, 19, 36), "add": (3, 36, 36, 36), "quad_add": (4, 36, 36, 36), "quad_add_opp": (5, 36, 36, 36),
               "oct_add": (6, 72, 72, 72), "fq2_mul": (7, 18, 18, 18), "fq2_sqr": (8, 18, 0, 18), "g2_madd": (9, 72, 37, 72), "madd_chain": (10, 36, 19 * 32, 36 * 32)}   # code, words a point: a, b, out
def _u32(a): return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if a is not None else None
def field29_op(field, op, a, b=None, c=None, d=None):
    """field 0 = Fr29, 1 = Fq29; operands (n, 9) uint32.  Returns (n, 9) uint32 ((n, 45) for ntt_lazy)."""
    ops = [np.ascontiguousarray(x, dtype=np.uint32) if x is not None else None for x in (a, b, c, d)]; n = ops[0].shape[0]
    assert all(x is None or x.shape == (n, 9) for x in ops); out = np.zeros((n, 45 if op == "ntt_lazy" else 9), dtype=np.uint32)
    _check(lib().zkgpu_test_field29_op(int(field), FIELD29_OPS[op], _u32(ops[0]), _u32(ops[1]), _u32(ops[2]), _u32(ops[3]), _u32(out), ctypes.c_size_t(n))); return out
def point29_op(op, a, b=None):
    """a, b: (n, words) uint32 as POINT29_OPS says (the one an operation does not take: None).  Returns (limbs (n, words out), flags (n,))"""
    code, wa, wb, wo = POINT29_OPS[op]; a = np.ascontiguousarray(a, dtype=np.uint32) if wa else None; b = np.ascontiguousarray(b, dtype=np.uint32) if wb else None
    n = (a if wa else b).shape[0]; assert (not wa or a.shape == (n, wa)) and (not wb or b.shape == (n, wb))
    out = np.zeros((n, wo), dtype=np.uint32); flags = np.zeros(n, dtype=np.uint32)
    _check(lib().zkgpu_test_point29_op(code, _u32(a), _u32(b), _u32(out), _u32(flags), ctypes.c_size_t(n))); return out, flags

# secp256k1 test entries (csrc/gpu_senders.hip): Python integers in and out, 32 big-endian bytes a value on the way
SECP_OPS = {"fq_mul": 0, "fq_sqr": 1, "fq_add": 2, "fq_sub": 3, "fq_neg": 4, "fq_inv": 5, "fq_sqrt": 6, "fq_reduce": 7, "n_mul": 8, "n_inv": 9, "n_reduce": 10}
def _be32(vals): return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in vals), dtype=np.uint8).copy() if len(vals) else np.zeros(0, dtype=np.uint8)
def _ints32(buf): b = bytes(buf); return [int.from_bytes(b[k:k + 32], "big") for k in range(0, len(b), 32)]
def secp_ops(op, a, b=None):
    """out[i] = op(a[i], b[i]) on the device, one lane a pair"""
    n = len(a); aa = _be32(a); bb = _be32(b) if b is not None else None; assert b is None or len(b) == n; out = np.zeros(32 * n, dtype=np.uint8)
    _check(lib().zkgpu_test_secp_ops(SECP_OPS[op], _bytes(aa), _bytes(bb) if bb is not None else None, ctypes.c_size_t(n), _bytes(out))); return _ints32(out)
def secp_lincomb(u1, u2, points):
    """u1[i] G + u2[i] points[i] through the recovery's own launches -> [(x, y) or None for the point at infinity]"""
    n = len(u1); assert len(u2) == n and len(points) == n; out = np.zeros(64 * n, dtype=np.uint8); inf = np.zeros(max(1, n), dtype=np.uint8)
    _check(lib().zkgpu_test_secp_lincomb(_bytes(_be32(u1)), _bytes(_be32(u2)), _bytes(_be32([p[0] for p in points])), _bytes(_be32([p[1] for p in points])), ctypes.c_size_t(n), _bytes(out), _bytes(inf)))
    v = _ints32(out); return [None if inf[i] else (v[2 * i], v[2 * i + 1]) for i in range(n)]
def secp_gtable():
    """the resident table of G: [(x, y) of k G for k = 1 .. 15]"""
    out = np.zeros(15 * 64, dtype=np.uint8); _check(lib().zkgpu_test_secp_gtable(_bytes(out))); v = _ints32(out); return [(v[2 * k], v[2 * k + 1]) for k in range(15)]
def senders_counters():
    """the last recovery or lincomb call: {equal, opposite, at_infinity, to_infinity}: lanes x times the walk's point addition took each exceptional branch"""
    out = (ctypes.c_uint64 * 4)(); _check(lib().zkgpu_test_senders_counters(out)); return dict(zip(("equal", "opposite", "at_infinity", "to_infinity"), (int(x) for x in out)))
def recover_senders(hashes, sigs, homestead=True, want_pubs=True):
    """zkgpu_recover_senders -> (count or a ZKGPU_ERR_* code, froms (n, 20) uint8, pubs (n, 64) uint8 or None, ok (n,) uint8)"""
    hb = np.frombuffer(b"".join(bytes(h) for h in hashes), dtype=np.uint8).reshape(-1, 32).copy(); sb = np.frombuffer(b"".join(bytes(x) for x in sigs), dtype=np.uint8).reshape(-1, 65).copy()
    n = int(hb.shape[0]); assert sb.shape[0] == n; froms = np.full((n, 20), 0xA5, dtype=np.uint8); pubs = np.full((n, 64), 0xA5, dtype=np.uint8) if want_pubs else None; ok = np.full(n, 0xA5, dtype=np.uint8)
    rc = int(lib().zkgpu_recover_senders(_bytes(hb) if n else None, _bytes(sb) if n else None, n, int(bool(homestead)), _bytes(froms) if n else None, _bytes(pubs) if (want_pubs and n) else None, _bytes(ok) if n else None))
    return rc, froms, pubs, ok

# sender inputs from raw transactions (csrc/gpu_txs.hip; include/zk_txs.h)
SIGNER_FRONTIER, SIGNER_HOMESTEAD, SIGNER_EIP155 = 0, 1, 2
TX_OK, TX_MALFORMED, TX_CHAIN_ID, TX_SIG = 0, 1, 2, 3
def _tx_blob(txs):
    """a list of byte strings -> (the bytes end to end (at least one byte, so that the pointer is never null), off (n + 1) uint64)"""
    raw = [bytes(t) for t in txs]; off = np.zeros(len(raw) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(t) for t in raw], dtype=np.uint64) if raw else []
    return np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8).copy(), off
def _u64p(a): return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
def keccak256(msgs):
    """Keccak-256 of every byte string of msgs through the device's multi-block sponge -> [32 bytes]"""
    n = len(msgs); blob, off = _tx_blob(msgs); out = np.zeros((max(1, n), 32), dtype=np.uint8)
    _check(lib().zkgpu_test_keccak256(_bytes(blob), _u64p(off), ctypes.c_size_t(n), _bytes(out))); return [bytes(out[i]) for i in range(n)]
def tx_signing_inputs(txs, signer, chain_id):
    """zkgpu_tx_signing_inputs -> (count or a ZKGPU_ERR_* code, dict of txhash (n, 32), sighash (n, 32), sigs (n, 65), deposit_from (n, 20), code (n,), status (n,), uint8)"""
    n = len(txs); blob, off = _tx_blob(txs); o = {k: np.full((n, w) if w else n, 0xA5, dtype=np.uint8) for k, w in (("txhash", 32), ("sighash", 32), ("sigs", 65), ("deposit_from", 20), ("code", 0), ("status", 0))}
    p = lambda k: _bytes(o[k]) if n else None
    rc = int(lib().zkgpu_tx_signing_inputs(_bytes(blob), _u64p(off), n, int(signer), ctypes.c_uint64(chain_id), p("txhash"), p("sighash"), p("sigs"), p("deposit_from"), p("code"), p("status")))
    return rc, o
def tx_senders(txs, signer, chain_id, want_txhash=True):
    """zkgpu_tx_senders -> (count or a ZKGPU_ERR_* code, dict of txhash (n, 32) or None, froms (n, 20), code (n,), status (n,), uint8)"""
    n = len(txs); blob, off = _tx_blob(txs); o = {k: np.full((n, w) if w else n, 0xA5, dtype=np.uint8) for k, w in (("txhash", 32), ("froms", 20), ("code", 0), ("status", 0))}
    if not want_txhash: o["txhash"] = None
    p = lambda k: _bytes(o[k]) if (n and o[k] is not None) else None
    rc = int(lib().zkgpu_tx_senders(_bytes(blob), _u64p(off), n, int(signer), ctypes.c_uint64(chain_id), p("txhash"), p("froms"), p("code"), p("status")))
    return rc, o

# records from the block bodies' bytes (csrc/gpu_txs.hip, csrc/capi_bodies.cpp; include/zk_bodies.h)
TX_DEPOSIT_KEY = 4
def tx_records(txs, signer, chain_id, want_txhash=True):
    """zkgpu_tx_records -> (m or a ZKGPU_ERR_* code, dict of recs (n,) RECORD_DTYPE, rec_froms (n, 20), rec_of (n,) int32, txhash (n, 32) or None, froms (n, 20), code (n,),
    status (n,)); every array is handed in full of 0xA5 bytes, so recs[m:] keeps them"""
    n = len(txs); blob, off = _tx_blob(txs); o = {k: np.full((n, w) if w else n, 0xA5, dtype=np.uint8) for k, w in (("rec_froms", 20), ("txhash", 32), ("froms", 20), ("code", 0), ("status", 0))}
    o["recs"] = np.frombuffer(bytes([0xA5]) * (720 * n), dtype=RECORD_DTYPE).copy(); o["rec_of"] = np.full(n, -1515870811, dtype=np.int32)
    if not want_txhash: o["txhash"] = None
    p = lambda k: o[k].ctypes.data_as(ctypes.c_void_p) if (n and o[k] is not None) else None
    rc = int(lib().zkgpu_tx_records(_bytes(blob), _u64p(off), n, int(signer), ctypes.c_uint64(chain_id), p("recs"), p("rec_froms"), p("rec_of"), p("txhash"), p("froms"), p("code"), p("status")))
    return rc, o
def bodies_gather_bytewise(on): _check(lib().zkgpu_test_bodies_gather(int(bool(on))))   # test entry: k_body_gather's source reads, for the measurement of DESIGN.md §23

# trie roots of many lists (csrc/gpu_txs.hip, csrc/capi_tx_roots.cpp; include/zk_tx_roots.h)
def _first(lists_first): return np.ascontiguousarray(lists_first, dtype=np.int32).reshape(-1)
def _i32p(a): return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
def list_trie_roots(vals, first, start=0):
    """zkgpu_list_trie_roots: DeriveSha of every list; vals: byte strings taken verbatim, first: n_lists + 1 indices into vals; start: the blob begins at this byte of
    its buffer (off[0] = start).  -> (ZKGPU_OK or a ZKGPU_ERR_* code, roots (n_lists, 32) uint8, handed in full of 0xA5)"""
    n = len(vals); blob, off = _tx_blob(vals); f = _first(first); nl = int(f.size) - 1
    if start: blob = np.concatenate([np.zeros(start, dtype=np.uint8), blob]); off = off + np.uint64(start)
    roots = np.full((max(0, nl), 32), 0xA5, dtype=np.uint8)
    rc = int(lib().zkgpu_list_trie_roots(_bytes(blob), _u64p(off), n, _i32p(f), nl, _bytes(roots) if nl > 0 else None))
    return rc, roots
def tx_roots(txs, block_first):
    """zkgpu_tx_roots -> (the number of defined roots or a ZKGPU_ERR_* code, roots (n_blocks, 32) uint8, defined (n_blocks,) uint8), both handed in full of 0xA5"""
    n = len(txs); blob, off = _tx_blob(txs); f = _first(block_first); nb = int(f.size) - 1
    roots = np.full((max(0, nb), 32), 0xA5, dtype=np.uint8); defined = np.full(max(0, nb), 0xA5, dtype=np.uint8)
    rc = int(lib().zkgpu_tx_roots(_bytes(blob), _u64p(off), n, _i32p(f), nb, _bytes(roots) if nb > 0 else None, _bytes(defined) if nb > 0 else None))
    return rc, roots, defined

# headers from their bytes (csrc/gpu_txs.hip, csrc/capi_headers.cpp; include/zk_headers.h)
(HDR_OK, HDR_MALFORMED, HDR_FUTURE, HDR_CHECKPOINT_BENEFICIARY, HDR_VOTE, HDR_CHECKPOINT_VOTE, HDR_VANITY, HDR_SIGNATURE, HDR_EXTRA_SIGNERS, HDR_CHECKPOINT_SIGNERS, HDR_MIX_DIGEST,
 HDR_UNCLE_HASH, HDR_DIFFICULTY, HDR_ANCESTOR, HDR_TIMESTAMP, HDR_SEAL, HDR_SEAL_UNDECIDED) = range(17)
HEADER_OUTPUTS = (("hash", 32, np.uint8), ("sealhash", 32, np.uint8), ("signer", 20, np.uint8), ("coinbase", 20, np.uint8), ("tx_root", 32, np.uint8), ("rtcmt", 32, np.uint8),
                  ("number", 0, np.uint64), ("time", 0, np.uint64), ("difficulty", 0, np.uint8), ("vote", 0, np.uint8), ("extra_beg", 0, np.uint32), ("extra_size", 0, np.uint32),
                  ("cmt_beg", 0, np.uint32), ("cmt_count", 0, np.uint32), ("status", 0, np.uint8))                  # in the order of zkHeaders' arguments
def _headers_call(fn, hdrs, period, epoch, now, parent, fill, start=0):
    """parent: None or (hash: 32 bytes, number, time).  -> (the call's return value, dict of HEADER_OUTPUTS' arrays, each handed in full of `fill` bytes)"""
    n = len(hdrs); blob, off = _tx_blob(hdrs)
    if start: blob = np.concatenate([np.zeros(start, dtype=np.uint8), blob]); off = off + np.uint64(start)
    o = {k: np.frombuffer(bytes([fill]) * (np.dtype(dt).itemsize * max(1, n) * (w or 1)), dtype=dt).copy().reshape((max(1, n), w) if w else max(1, n)) for k, w, dt in HEADER_OUTPUTS}
    ph = np.frombuffer(bytes(parent[0]), dtype=np.uint8).copy() if parent is not None else None; u64 = ctypes.c_uint64
    rc = int(fn(_bytes(blob), _u64p(off), n, u64(period), u64(epoch), u64(now), 1 if parent is not None else 0, _bytes(ph) if ph is not None else None, u64(parent[1] if parent is not None else 0),
                u64(parent[2] if parent is not None else 0), *[o[k].ctypes.data_as(ctypes.c_void_p) for k, _, _ in HEADER_OUTPUTS]))
    return rc, {k: v[:n] for k, v in o.items()}
def headers(hdrs, period, epoch, now, parent, fill=0xA5, start=0):
    """zkgpu_headers -> (the number of leading headers with status HDR_OK or a ZKGPU_ERR_* code, dict of HEADER_OUTPUTS' arrays); start: the blob begins at this byte of its
    buffer (off[0] = start)"""
    f = lib().zkgpu_headers; f.restype = ctypes.c_int; return _headers_call(f, hdrs, period, epoch, now, parent, fill, start)

# block bodies from their bytes (csrc/gpu_txs.hip, csrc/capi_raw_bodies.cpp; include/zk_raw_bodies.h)
BODY_OK, BODY_MALFORMED, BODY_UNCLES = 0, 1, 2
ERR_CAP = -5
def _body_blob(bodies, start=0):
    """_tx_blob with `start` bytes in front: the blob begins at that byte of its buffer (body_off[0] = start)"""
    blob, off = _tx_blob(bodies)
    if start: blob = np.concatenate([np.full(start, 0xEE, dtype=np.uint8), blob]); off = off + np.uint64(start)
    return blob, off
def body_split(bodies, cap=None, start=0, packed=False, fill=0xA5):
    """zkgpu_body_split (packed: zkgpu_test_body_split) -> (k, ERR_CAP or a ZKGPU_ERR_* code, dict of n_txs, tx_beg (cap,) uint64, tx_size (cap,) uint32, block_first
    (n_blocks + 1,) int32, body_status (n_blocks,) uint8 and, with packed, packed: the bytes where the kernels read txs, cut at off[n], packed_off (cap + 1,) uint64);
    every array is handed in full of `fill` bytes.  cap None: room for one transaction a byte"""
    nb = len(bodies); blob, off = _body_blob(bodies, start); total = int(off[nb] - off[0]); cap = total if cap is None else int(cap)
    mk = lambda count, dt: np.frombuffer(bytes([fill]) * (np.dtype(dt).itemsize * max(1, count)), dtype=dt).copy()
    o = dict(tx_beg=mk(cap, np.uint64), tx_size=mk(cap, np.uint32), block_first=mk(nb + 1, np.int32), body_status=mk(nb, np.uint8)); n = ctypes.c_int(-7); vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    args = [_bytes(blob), _u64p(off), nb, cap, vp(o["tx_beg"]), vp(o["tx_size"]), vp(o["block_first"]), vp(o["body_status"]), ctypes.byref(n)]
    if packed:
        pk, po = mk(total, np.uint8), mk(cap + 1, np.uint64); f = lib().zkgpu_test_body_split; f.restype = ctypes.c_int; rc = int(f(*args, vp(pk), vp(po)))
        o["packed_off"] = po[:cap + 1]; o["packed"] = bytes(pk[:int(po[n.value])]) if rc >= 0 else bytes(pk[:total])
    else: f = lib().zkgpu_body_split; f.restype = ctypes.c_int; rc = int(f(*args))
    o["n_txs"] = int(n.value); o["tx_beg"] = o["tx_beg"][:cap]; o["tx_size"] = o["tx_size"][:cap]; o["body_status"] = o["body_status"][:nb]
    return rc, o

def msm(group, points, scalars, window_bits=0, filter_ones=False):
    points = np.ascontiguousarray(points, dtype=np.uint64); scalars = np.ascontiguousarray(scalars, dtype=np.uint64); n = scalars.size // 4
    out = np.zeros(8 if group == 1 else 16, dtype=np.uint64)
    fn = lib().zkgpu_msm_g1 if group == 1 else lib().zkgpu_msm_g2
    _check(fn(_bytes(points), _bytes(scalars), ctypes.c_size_t(n), int(window_bits), int(filter_ones), _bytes(out))); return out

class ResidentMsm:
    """bases resident in HBM (one proving-key query); run() launches only the kernels + the host combine"""
    def __init__(self, group, points, window_bits=0, filter_ones=False):
        points = np.ascontiguousarray(points, dtype=np.uint64); self.group = group; self.n = points.shape[0]
        self.h = lib().zkgpu_msm_create(group, _bytes(points), ctypes.c_size_t(self.n), int(window_bits), int(filter_ones))
        if not self.h: raise ZkGpuError(lib().zkgpu_last_error().decode())
    def set_scalars(self, scalars):
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64); _check(lib().zkgpu_msm_set_scalars(ctypes.c_void_p(self.h), _bytes(scalars), ctypes.c_size_t(scalars.size // 4)))
    def run(self):
        out = np.zeros(8 if self.group == 1 else 16, dtype=np.uint64); _check(lib().zkgpu_msm_run(ctypes.c_void_p(self.h), _bytes(out))); return out
    # test entry points of the uniform-scalar (H query) path, G1 only (include/zkgpu.h: zkgpu_test_msm_*)
    PATH_FIELDS = ("one_pass", "c", "W", "NB", "groups", "low_bits", "idx_bits", "region", "h_run", "h_maxp", "htail29", "ll", "run_in_effect", "any_inf", "WB", "RS",
                   "top", "lo_bits", "hi_bits", "row_chunks", "marg_block", "marg_blocks", "marg_count", "flag")
    H_STATE = {"counts": 0, "offsets": 1, "group_n": 2, "entries": 3, "hb29": 4}
    def path(self):
        """what the object decided when it was created (and the lane exponent of its last combine), as a namespace of ints; one_pass is a bool"""
        import types
        out = np.zeros(len(self.PATH_FIELDS), dtype=np.uint32); _check(lib().zkgpu_test_msm_path(ctypes.c_void_p(self.h), _u32(out)))
        d = {k: int(v) for k, v in zip(self.PATH_FIELDS, out)}; d["one_pass"] = bool(d["one_pass"]); d["htail29"] = bool(d["htail29"]); return types.SimpleNamespace(**d)
    def set_crowded(self, on): _check(lib().zkgpu_test_msm_set_crowded(ctypes.c_void_p(self.h), int(bool(on))))
    def run_product(self, a, b, z):
        """sum_i (a_i b_i z_i) P_i, the product formed inside the sort kernel; z: one element (4 words) or a table of n"""
        a, b, z = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in (a, b, z)); assert a.shape[0] == self.n == b.shape[0] and z.shape[0] in (1, self.n)
        out = np.zeros(8, dtype=np.uint64)
        _check(lib().zkgpu_test_msm_run_product(ctypes.c_void_p(self.h), _bytes(a), _bytes(b), _bytes(z), int(z.shape[0] == self.n and self.n > 1), _bytes(out))); return out
    def h_state(self, what):
        """device state of the last one-pass run (only meaningful when it did not fall back): uint32 words, see H_STATE"""
        p = self.path(); cap = {"counts": p.NB, "offsets": p.NB, "group_n": p.groups, "entries": p.groups * p.region, "hb29": p.NB * 48}[what]
        out = np.zeros(max(cap, 1), dtype=np.uint32); words = ctypes.c_size_t(0)
        _check(lib().zkgpu_test_msm_h_state(ctypes.c_void_p(self.h), self.H_STATE[what], _u32(out), ctypes.c_size_t(out.size), ctypes.byref(words))); return out[:words.value]
    # test entry points of the witness MSMs' three-launch path, both groups (include/zkgpu.h: zkgpu_test_msm_wpath and what follows it)
    WPATH_FIELDS = ("fused", "c", "W", "NB", "cap", "any_inf", "RS", "leader", "shared", "flag", "n_ones", "lanes", "T", "bucket_lanes", "ones_lanes", "min_slice", "WB",
                    "stream", "top", "tail_slots")
    W_STATE = {"fill": 0, "lane_off": 1, "ones": 2, "entries": 3}
    def wpath(self):
        """what the object decided when it was created and what its last synchronised fused run reported, as a namespace of ints; fused, leader and shared are bools"""
        import types
        out = np.zeros(len(self.WPATH_FIELDS), dtype=np.uint32); _check(lib().zkgpu_test_msm_wpath(ctypes.c_void_p(self.h), _u32(out)))
        d = {k: int(v) for k, v in zip(self.WPATH_FIELDS, out)}
        for k in ("fused", "leader", "shared"): d[k] = bool(d[k])
        return types.SimpleNamespace(**d)
    def w_state(self, what):
        """device state of the last fused run (only meaningful when it did not fall back): uint32 words, see W_STATE; entries: every bucket's end to end"""
        p = self.wpath(); cap = {"fill": p.NB, "lane_off": p.NB + 1, "ones": self.n, "entries": p.NB * p.cap}[what]
        out = np.zeros(max(cap, 1), dtype=np.uint32); words = ctypes.c_size_t(0)
        _check(lib().zkgpu_test_msm_w_state(ctypes.c_void_p(self.h), self.W_STATE[what], _u32(out), ctypes.c_size_t(out.size), ctypes.byref(words))); return out[:words.value]
    def share_sort(self, leader):
        """this object takes the leader's sort of the scalars; False if share_sort_with refused"""
        rc = int(lib().zkgpu_test_msm_share_sort(ctypes.c_void_p(self.h), ctypes.c_void_p(leader.h)))
        if rc < 0: _check(rc)
        return bool(rc)
    def set_stream(self, aux): _check(lib().zkgpu_test_msm_set_stream(ctypes.c_void_p(self.h), int(aux)))
    def _out(self): return np.zeros(8 if self.group == 1 else 16, dtype=np.uint64)
    def run_indexed(self, z_all, index):
        """point i takes the scalar z_all[index[i]]"""
        z = np.ascontiguousarray(z_all, dtype=np.uint64).reshape(-1, 4); idx = np.ascontiguousarray(index, dtype=np.uint32); assert idx.shape == (self.n,); out = self._out()
        _check(lib().zkgpu_test_msm_run_indexed(ctypes.c_void_p(self.h), _bytes(z), ctypes.c_size_t(z.shape[0]), _u32(idx), _bytes(out))); return out
    def run_tagged(self, z_all, tags, other_vars, n_other_bound=None, var_pos=None, index=None, base=0):
        """the sort from the assignment's tags (k_wsort_tagged): z_all with variable 0 = ONE, a tag byte a variable, the list of the variables tagged 2"""
        z = np.ascontiguousarray(z_all, dtype=np.uint64).reshape(-1, 4); nv = z.shape[0]; tags = np.ascontiguousarray(tags, dtype=np.uint8); assert tags.shape == (nv,)
        ov = np.ascontiguousarray(other_vars, dtype=np.uint32).reshape(-1); bound = ov.size if n_other_bound is None else int(n_other_bound)
        vp = np.ascontiguousarray(var_pos, dtype=np.uint32) if var_pos is not None else None; idx = np.ascontiguousarray(index, dtype=np.uint32) if index is not None else None
        assert (vp is None or vp.shape == (nv,)) and (idx is None or idx.shape == (self.n,)); out = self._out()
        _check(lib().zkgpu_test_msm_run_tagged(ctypes.c_void_p(self.h), _bytes(z), ctypes.c_size_t(nv), _bytes(tags), _u32(ov) if ov.size else None, ctypes.c_size_t(ov.size),
                                               ctypes.c_size_t(bound), _u32(vp), _u32(idx), ctypes.c_uint32(base), _bytes(out))); return out
    def close(self):
        if self.h: lib().zkgpu_msm_destroy(ctypes.c_void_p(self.h)); self.h = None
    def __del__(self):
        try: self.close()
        except Exception: pass

def run_pair(leader, follower):
    """the leader's run and the follower's, over the leader's scalars, both in flight before either result is taken -> (leader's sum, follower's sum)"""
    a, b = leader._out(), follower._out(); _check(lib().zkgpu_test_msm_run_pair(ctypes.c_void_p(leader.h), ctypes.c_void_p(follower.h), _bytes(a), _bytes(b))); return a, b

def domain_size(min_size): return int(lib().zkgpu_domain_size(min_size))
def domain_transform(min_size, op, data):
    data = np.ascontiguousarray(data, dtype=np.uint64).copy()
    _check(lib().zkgpu_domain_transform(ctypes.c_size_t(min_size), {"fft": 0, "ifft": 1, "cosetfft": 2, "icosetfft": 3}[op], _bytes(data))); return data

class R1cs:
    def __init__(self, n_inputs, n_vars, n_cons, rowptr, col, coeff):
        self.n_inputs, self.n_vars, self.n_cons = n_inputs, n_vars, n_cons
        self._keep = [[np.ascontiguousarray(x, dtype=np.uint32) for x in rowptr], [np.ascontiguousarray(x, dtype=np.uint32) for x in col], [np.ascontiguousarray(x, dtype=np.uint64) for x in coeff]]
        P32 = ctypes.POINTER(ctypes.c_uint32); P8 = ctypes.POINTER(ctypes.c_uint8)
        rp = (P32 * 3)(*[x.ctypes.data_as(P32) for x in self._keep[0]]); cl = (P32 * 3)(*[x.ctypes.data_as(P32) for x in self._keep[1]]); co = (P8 * 3)(*[x.ctypes.data_as(P8) for x in self._keep[2]])
        self.h = lib().zkgpu_r1cs_create(ctypes.c_size_t(n_inputs), ctypes.c_size_t(n_vars), ctypes.c_size_t(n_cons), rp, cl, co)
        if not self.h: raise ZkGpuError(lib().zkgpu_last_error().decode())
        self.m = domain_size(n_cons + n_inputs + 1)
    def witness_map(self, z):
        z = np.ascontiguousarray(z, dtype=np.uint64); H = np.zeros((self.m + 1, 4), dtype=np.uint64)
        _check(lib().zkgpu_witness_map(ctypes.c_void_p(self.h), _bytes(z), _bytes(H))); return H
    def fold_c(self, h_lagrange, L):
        """test entry: h_lagrange (m, 8), L (n_vars - n_inputs, 8) words -> the folded L query, (n_vars + 1, 8)"""
        P = np.ascontiguousarray(h_lagrange, dtype=np.uint64); L = np.ascontiguousarray(L, dtype=np.uint64); assert P.size == 8 * self.m and L.size == 8 * (self.n_vars - self.n_inputs)
        out = np.zeros((self.n_vars + 1, 8), dtype=np.uint64); _check(lib().zkgpu_test_fold_c(ctypes.c_void_p(self.h), _bytes(P), _bytes(L), _bytes(out))); return out
    def close(self):
        if self.h: lib().zkgpu_r1cs_destroy(ctypes.c_void_p(self.h)); self.h = None
    def __del__(self):
        try: self.close()
        except Exception: pass

# ---- key-side operations on caller arrays (test entries): points (n, 8) / (n, 16) words, canonical ----
def decompress(group, xs_mont, flags):
    """xs_mont: (n, 4) words for G1, (n, 8) for G2, Montgomery form; flags: n bytes (bit 0 lsb of y / y.c0, bit 1 infinity).  Raises if an x is on no point."""
    w = 4 * group; xs = np.ascontiguousarray(xs_mont, dtype=np.uint64).reshape(-1, w); n = xs.shape[0]; f = np.ascontiguousarray(flags, dtype=np.uint8); assert f.shape == (n,)
    out = np.zeros((n, 8 * group), dtype=np.uint64); _check(lib().zkgpu_test_decompress(int(group), _bytes(xs), _bytes(f), ctypes.c_size_t(n), _bytes(out))); return out
def fixed_base_mul(group, base, scalars):
    """base: 8 / 16 words (affine), scalars: (n, 4) words canonical -> scalars[i] * base"""
    b = np.ascontiguousarray(base, dtype=np.uint64).reshape(8 * group); k = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4); n = k.shape[0]
    out = np.zeros((n, 8 * group), dtype=np.uint64); _check(lib().zkgpu_test_fixed_base_mul(int(group), _bytes(b), _bytes(k), ctypes.c_size_t(n), _bytes(out))); return out
def h_query_lagrange(min_size, h):
    """h: (n_in, 8) words, n_in <= m -> the m points of the H query in the coset's Lagrange basis"""
    h = np.ascontiguousarray(h, dtype=np.uint64).reshape(-1, 8); out = np.zeros((domain_size(min_size), 8), dtype=np.uint64)
    _check(lib().zkgpu_test_h_query_lagrange(ctypes.c_size_t(min_size), _bytes(h), ctypes.c_size_t(h.shape[0]), _bytes(out))); return out

# ---- circuits, keys, prover, verifier ---------------------------------------------------------------------------------
KIND = {"mint": 0, "send": 1, "deposit": 2, "redeem": 3, "sha256": 100, "merkle": 101, "lesscmp": 102, "cmta": 103, "cmts": 104, "prf": 105, "crh": 106, "unpacker": 107}
def circuit_export(kind, path, tree_depth=8): _check(lib().zkgpu_circuit_export(KIND[kind], tree_depth, path.encode()))
def keygen(kind, pk_path, vk_path, seed=0, tree_depth=8): _check(lib().zkgpu_keygen(KIND[kind], tree_depth, ctypes.c_uint64(seed), pk_path.encode(), vk_path.encode()))
def keygen_from_r1cs(r1cs_path, pk_path, vk_path, seed=0): _check(lib().zkgpu_keygen_from_r1cs(r1cs_path.encode(), ctypes.c_uint64(seed), pk_path.encode(), vk_path.encode()))
def witness_sha256(left32, right32, path): _check(lib().zkgpu_witness_sha256(bytes(left32), bytes(right32), path.encode()))
def witness_hashblock(kind, bits, path): _check(lib().zkgpu_witness_hashblock(KIND[kind] - 104, bytes(bits), path.encode()))
def witness_cmta(bits576, path): _check(lib().zkgpu_witness_cmta(bytes(bits576), path.encode()))
def witness_unpacker(bits, path): _check(lib().zkgpu_witness_unpacker(len(bits), bytes(bits), path.encode()))
def witness_lesscmp(value_old, value_s, path): _check(lib().zkgpu_witness_lesscmp(ctypes.c_uint64(value_old), ctypes.c_uint64(value_s), path.encode()))
def _s(x): return x if isinstance(x, bytes) else x.encode()
def witness_send(value_A, r_s, sn, r, cmt_s, cmtA, value_s, pk_recv, value_A_new, sn_A_new, r_A_new, cmt_A_new, sk, pk_sender, path):
    _check(lib().zkgpu_witness_send(ctypes.c_uint64(value_A), _s(r_s), _s(sn), _s(r), _s(cmt_s), _s(cmtA), ctypes.c_uint64(value_s), _s(pk_recv), ctypes.c_uint64(value_A_new), _s(sn_A_new), _s(r_A_new), _s(cmt_A_new), _s(sk), _s(pk_sender), path.encode()))
def witness_mint_redeem(redeem, value, value_old, sn_old, r_old, sn, r, cmtA_old, cmtA, value_s, sk, path):
    _check(lib().zkgpu_witness_mint_redeem(int(redeem), ctypes.c_uint64(value), ctypes.c_uint64(value_old), _s(sn_old), _s(r_old), _s(sn), _s(r), _s(cmtA_old), _s(cmtA), ctypes.c_uint64(value_s), _s(sk), path.encode()))

def witness_deposit(value, value_old, sn_old, r_old, sn, r, sns, rs, cmtB_old, cmtB, value_s, pk, sn_A_old, cmtS, cmtarray, n, sk, path, tree_depth=8):
    _check(lib().zkgpu_witness_deposit(ctypes.c_uint64(value), ctypes.c_uint64(value_old), _s(sn_old), _s(r_old), _s(sn), _s(r), _s(sns), _s(rs), _s(cmtB_old), _s(cmtB), ctypes.c_uint64(value_s), _s(pk), _s(sn_A_old), _s(cmtS), _s(cmtarray), int(n), _s(sk), int(tree_depth), path.encode()))
def witness_merkle(depth, leaf32, siblings, position, path): _check(lib().zkgpu_witness_merkle(int(depth), bytes(leaf32), b"".join(bytes(x) for x in siblings), ctypes.c_uint64(position), path.encode()))

class Prover:
    """a reference-format proving key resident in HBM"""
    def __init__(self, pk_path, shard_rank=0, shard_world=1):
        lib().zkgpu_prover_load_shard.restype = ctypes.c_void_p
        self.h = lib().zkgpu_prover_load_shard(pk_path.encode(), ctypes.c_size_t(shard_rank), ctypes.c_size_t(shard_world))
        if not self.h: raise ZkGpuError(lib().zkgpu_last_error().decode())
        info = (ctypes.c_size_t * 3)(); _check(lib().zkgpu_prover_info(ctypes.c_void_p(self.h), info)); self.n_vars, self.n_inputs, self.m = (int(x) for x in info)
    def prove(self, z, r=None, s=None):
        """z: (n_vars, 4) uint64 canonical.  r, s: ints or None.  Returns the 512-character proof hex."""
        z = np.ascontiguousarray(z, dtype=np.uint64); assert z.size == 4 * self.n_vars
        R = int(r).to_bytes(32, "little") if r is not None else None; S = int(s).to_bytes(32, "little") if s is not None else None
        out = ctypes.create_string_buffer(513); _check(lib().zkgpu_prover_prove(ctypes.c_void_p(self.h), _bytes(z), R, S, out)); return out.value.decode()
    def set_witness(self, z):
        z = np.ascontiguousarray(z, dtype=np.uint64); assert z.size == 4 * self.n_vars; _check(lib().zkgpu_prover_set_witness(ctypes.c_void_p(self.h), _bytes(z)))
    def prove_resident(self, r=None, s=None):
        R = int(r).to_bytes(32, "little") if r is not None else None; S = int(s).to_bytes(32, "little") if s is not None else None
        out = ctypes.create_string_buffer(513); _check(lib().zkgpu_prover_prove_resident(ctypes.c_void_p(self.h), R, S, out)); return out.value.decode()
    def stash_witness(self):
        """keep the assignment handed over last in HBM; returns its slot"""
        slot = ctypes.c_uint32(0); _check(lib().zkgpu_prover_stash_witness(ctypes.c_void_p(self.h), ctypes.byref(slot))); return int(slot.value)
    def drop_stash(self, slot=None):
        """free a kept assignment (None: all of them)"""
        _check(lib().zkgpu_prover_drop_stash(ctypes.c_void_p(self.h), ctypes.c_uint32(0xffffffff if slot is None else slot)))
    def equal_column_groups(self):
        k = ctypes.c_uint32(0); _check(lib().zkgpu_prover_equal_column_groups(ctypes.c_void_p(self.h), ctypes.byref(k))); return int(k.value)
    def read_stash(self, slot):
        """the kept assignment of a slot back on the host: (n_vars, 4) uint64 canonical"""
        z = np.zeros((self.n_vars, 4), dtype=np.uint64); _check(lib().zkgpu_prover_read_stash(ctypes.c_void_p(self.h), ctypes.c_uint32(slot), z.ctypes.data_as(ctypes.c_void_p))); return z
    def stash_count(self):
        k = ctypes.c_uint32(0); _check(lib().zkgpu_prover_stash_count(ctypes.c_void_p(self.h), ctypes.byref(k))); return int(k.value)
    def prove_stashed(self, slot, r=None, s=None):
        R = int(r).to_bytes(32, "little") if r is not None else None; S = int(s).to_bytes(32, "little") if s is not None else None
        out = ctypes.create_string_buffer(513); _check(lib().zkgpu_prover_prove_stashed(ctypes.c_void_p(self.h), ctypes.c_uint32(slot), R, S, out)); return out.value.decode()
    def prove_partial(self):
        """this shard's 384-byte record of partial sums (device pipeline on the resident witness)"""
        out = ctypes.create_string_buffer(384); _check(lib().zkgpu_prover_prove_partial(ctypes.c_void_p(self.h), out)); return out.raw
    def finish(self, records, r, s):
        """add the shard records (list of 384-byte strings, any order) and assemble the proof with the given randomness"""
        buf = b"".join(records); out = ctypes.create_string_buffer(513)
        _check(lib().zkgpu_prover_finish(ctypes.c_void_p(self.h), buf, ctypes.c_size_t(len(records)), int(r).to_bytes(32, "little"), int(s).to_bytes(32, "little"), out)); return out.value.decode()
    def clone(self):
        """another prover object on the same resident key (shares the device tables, owns its streams and workspaces)"""
        lib().zkgpu_prover_clone.restype = ctypes.c_void_p; h = lib().zkgpu_prover_clone(ctypes.c_void_p(self.h))
        if not h: raise ZkGpuError(lib().zkgpu_last_error().decode())
        c = object.__new__(Prover); c.h = h; c.n_vars, c.n_inputs, c.m = self.n_vars, self.n_inputs, self.m; return c
    def prove_batch(self, zs, rs=None):
        """zs: list of (n_vars, 4) uint64 assignments; rs: list of (r, s) int pairs or None.  One call, len(zs) proofs (512-character hex each)."""
        if isinstance(zs, np.ndarray) and zs.ndim == 3: Z = np.ascontiguousarray(zs, dtype=np.uint64); n = Z.shape[0]; assert Z.shape[1:] == (self.n_vars, 4)   # already back to back: no copy
        else: n = len(zs); Z = np.ascontiguousarray(np.stack([np.ascontiguousarray(z, dtype=np.uint64).reshape(self.n_vars, 4) for z in zs])) if n else np.zeros((0, self.n_vars, 4), dtype=np.uint64)
        R = b"".join(int(r).to_bytes(32, "little") + int(s).to_bytes(32, "little") for r, s in rs) if rs is not None else None
        out = ctypes.create_string_buffer(513 * max(1, n)); _check(lib().zkgpu_prover_prove_batch(ctypes.c_void_p(self.h), _bytes(Z), ctypes.c_size_t(n), R, out))
        return [out.raw[513 * i:513 * i + 512].decode() for i in range(n)]
    def timings(self):
        t = (ctypes.c_double * 5)(); _check(lib().zkgpu_prover_timings(ctypes.c_void_p(self.h), t)); return dict(zip(("upload_ms", "enqueue_ms", "device_ms", "finish_ms", "total_ms"), (float(x) for x in t)))
    def close(self):
        if self.h: lib().zkgpu_prover_destroy(ctypes.c_void_p(self.h)); self.h = None
    def __del__(self):
        try: self.close()
        except Exception: pass

def profile_enable(on=True): _check(lib().zkgpu_profile_enable(int(on)))
def profile_report():
    import json
    buf = ctypes.create_string_buffer(1 << 22); _check(lib().zkgpu_profile_report(buf, ctypes.c_size_t(len(buf)))); return json.loads(buf.value.decode())

def verify_batch(vk_path, proofs_hex, inputs):
    """proofs_hex: list of n 512-character strings; inputs: list of n lists of canonical ints -> list of n booleans (GPU, kernel K9)"""
    n = len(proofs_hex); ni = len(inputs[0]) if n else 0; blob = "".join(proofs_hex).encode(); assert len(blob) == 512 * n
    buf = (ctypes.c_uint8 * max(1, 32 * n * ni))(); 
    for i, row in enumerate(inputs):
        assert len(row) == ni
        for j, v in enumerate(row): buf[32 * (i * ni + j):32 * (i * ni + j + 1)] = list(int(v).to_bytes(32, "little"))
    ok = (ctypes.c_uint8 * max(1, n))(); _check(lib().zkgpu_verify_batch(vk_path.encode(), blob, buf, ctypes.c_size_t(ni), ctypes.c_size_t(n), ok)); return [bool(ok[i]) for i in range(n)]

def _batch_args(proofs_hex, inputs, weights):
    n = len(proofs_hex); ni = len(inputs[0]) if n else 0; blob = "".join(proofs_hex).encode(); assert len(blob) == 512 * n
    buf = b"".join(int(v).to_bytes(32, "little") for row in inputs for v in row); assert len(buf) == 32 * n * ni
    wb = None if weights is None else b"".join(int(r).to_bytes(16, "little") for r in weights)
    assert wb is None or len(wb) == 16 * n
    return n, ni, blob, buf or b"\0", wb
def verify_batch_rlc(vk_path, proofs_hex, inputs, weights=None):
    """zkgpu_verify_batch_rlc: the verdicts of verify_batch by one randomized pairing-product check (weights: n ints in [1, 2^128), or None for fresh ones)
    -> (list of n booleans, True if the equation decided the call)"""
    n, ni, blob, buf, wb = _batch_args(proofs_hex, inputs, weights); ok = (ctypes.c_uint8 * max(1, n))(); by = ctypes.c_uint32(0)
    _check(lib().zkgpu_verify_batch_rlc(vk_path.encode(), blob, buf, ctypes.c_size_t(ni), ctypes.c_size_t(n), wb, ok, ctypes.byref(by)))
    return [bool(ok[i]) for i in range(n)], bool(by.value)
def verify_rlc_equation(vk_path, proofs_hex, inputs, weights, device=False):
    """the block equation for explicit weights, on the host model (no device) or through the device path -> (holds, 384-byte GT value of the left-hand side)"""
    n, ni, blob, buf, wb = _batch_args(proofs_hex, inputs, weights); gt = (ctypes.c_uint8 * 384)()
    f = lib().zkgpu_test_verify_rlc_device if device else lib().zkgpu_test_verify_rlc_host
    rc = f(vk_path.encode(), blob, buf, ctypes.c_size_t(ni), ctypes.c_size_t(n), wb, gt)
    if rc < 0: _check(rc)
    return rc == 1, bytes(gt)
def verify_rlc_counters():
    """(block equations that held, equations that failed, calls decided proof by proof), process-wide"""
    out = (ctypes.c_uint64 * 3)(); _check(lib().zkgpu_verify_rlc_counters(out)); return tuple(int(x) for x in out)

# ---- blocks as records (include/zk_records.h) -----------------------------------------------------------------------------
# one record = 720 bytes, no padding: the layout of zk_block_record (tests/test_block_records_cpu.py compares it with a C compiler's)
RECORD_DTYPE = np.dtype([("kind", "u1"), ("reserved", "u1", (7,)), ("value_s", "<u8"), ("proof", "u1", (512,)), ("args", "u1", (6, 32))])
assert RECORD_DTYPE.itemsize == 720
def records_from_items(items):
    """items as Zk.VerifyBlock takes them — (kind, proof hex, [big-endian byte strings in the order of the kind's verify symbol], value_s) — as one array of
    zk_block_record.  An argument keeps the meaning Zk.hx + blob256_from_hex give it: its last 32 (pk: 20) bytes, zero-extended on the left; a proof shorter than
    512 characters is padded with NULs (it does not parse), a longer one is cut as strnlen(proof, 512) cuts it.  One bytes object per item, no loop per byte."""
    import struct
    def arg(a, w): a = bytes(a)[-w:]; return (a.rjust(w, b"\0")).ljust(32, b"\0")
    out = []
    for kind, proof, args, value_s in items:
        k = KIND[kind] if isinstance(kind, str) else int(kind); pb = (proof.encode() if isinstance(proof, str) else bytes(proof or b""))[:512].split(b"\0")[0].ljust(512, b"\0")
        ab = b"".join(arg(a, 20 if (k == 2 and j == 1) else 32) for j, a in enumerate(args[:6])).ljust(192, b"\0")
        out.append(struct.pack("<B7xQ", k if 0 <= k <= 255 else 255, int(value_s or 0) & 0xFFFFFFFFFFFFFFFF) + pb + ab)
    return np.frombuffer(b"".join(out), dtype=RECORD_DTYPE).copy() if out else np.zeros(0, dtype=RECORD_DTYPE)
def _recs(recs):
    recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE); return recs, recs.ctypes.data_as(ctypes.c_void_p), int(recs.shape[0])
def ingest_records(recs, device=True):
    """zkgpu_test_ingest_records: records of one kind -> (items (n, 8, 4) uint64 Montgomery words, inputs (n, n_inputs, 4) uint64 canonical, parsed (n,) uint8),
    from k_ingest_records (device=True) or from the host converter (device=False: needs no device)"""
    recs, ptr, n = _recs(recs); items = np.zeros((max(1, n), 8, 4), dtype=np.uint64); inputs = np.zeros((max(1, n), 6, 4), dtype=np.uint64); parsed = np.zeros(max(1, n), dtype=np.uint8)
    ni = ctypes.c_size_t(0); _check(lib().zkgpu_test_ingest_records(ptr, ctypes.c_size_t(n), int(bool(device)), _bytes(items), _bytes(inputs), ctypes.byref(ni), _bytes(parsed)))
    k = int(ni.value); return items[:n], inputs.reshape(-1)[:n * k * 4].reshape(n, k, 4).copy(), parsed[:n]
def _weights(weights, n):
    wb = None if weights is None else b"".join(int(r).to_bytes(16, "little") for r in weights); assert wb is None or len(wb) == 16 * n; return wb
def verify_records_rlc(vk_path, recs, weights=None):
    """zkgpu_verify_records_rlc: verify_batch_rlc for records of one kind -> (list of n booleans, True if the equation decided the call)"""
    recs, ptr, n = _recs(recs); ok = (ctypes.c_uint8 * max(1, n))(); by = ctypes.c_uint32(0)
    _check(lib().zkgpu_verify_records_rlc(vk_path.encode(), ptr, ctypes.c_size_t(n), _weights(weights, n), ok, ctypes.byref(by))); return [bool(ok[i]) for i in range(n)], bool(by.value)
def _ints448(a): return [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in np.asarray(a, dtype=np.uint64).reshape(-1, 7)]
def records_rlc_equation(vk_path, recs, weights):
    """zkgpu_test_records_rlc: the block equation from records through the device path -> (holds, 384-byte GT value, the device's integer sums [sum r_i, sum r_i x_i0, ...])"""
    recs, ptr, n = _recs(recs); gt = (ctypes.c_uint8 * 384)(); sums = np.zeros(7 * 7, dtype=np.uint64); ni = {0: 4, 1: 5, 2: 6, 3: 4}[int(recs["kind"][0])]
    rc = lib().zkgpu_test_records_rlc(vk_path.encode(), ptr, ctypes.c_size_t(n), _weights(weights, n), gt, sums.ctypes.data_as(ctypes.c_void_p))
    if rc < 0: _check(rc)
    return rc == 1, bytes(gt), _ints448(sums[:7 * (ni + 1)])
def rlc_sums_host(inputs, weights, flags):
    """zkgpu_test_rlc_sums_host: inputs (n, n_inputs, 4) uint64 canonical, weights n ints, flags n bytes -> the host loop's integers [sum r_i, sum r_i x_i0, ...] over flag 1"""
    inputs = np.ascontiguousarray(inputs, dtype=np.uint64); n = len(weights); ni = inputs.shape[1] if n else 0; fl = np.ascontiguousarray(flags, dtype=np.uint8); assert fl.shape == (n,)
    sums = np.zeros(7 * (ni + 1), dtype=np.uint64)
    _check(lib().zkgpu_test_rlc_sums_host(_bytes(inputs) if inputs.size else None, ctypes.c_size_t(ni), _weights(weights, n) or b"\0", _bytes(fl) if n else b"\0", ctypes.c_size_t(n), sums.ctypes.data_as(ctypes.c_void_p)))
    return _ints448(sums)

def verify_schedule_on_host(vk_path, proof_hex, inputs):
    """the GPU verifier's operation schedule (csrc/verify_sched.hpp) interpreted on the host: (accept, {rounds, slots, products, linear_ops, constants, mul_waves, lin8_waves, lin1_waves}); needs no device"""
    buf = b"".join(int(x).to_bytes(32, "little") for x in inputs); st = (ctypes.c_uint32 * 8)()
    rc = lib().zkgpu_test_verify_schedule(vk_path.encode(), proof_hex.encode(), buf, ctypes.c_size_t(len(inputs)), st)
    if rc < 0: _check(rc)
    return rc == 1, dict(zip(("rounds", "slots", "products", "linear_ops", "constants", "mul_waves", "lin8_waves", "lin1_waves"), (int(x) for x in st)))
def equal_columns(r1cs_path):
    """groups (lists of variable numbers, 0 = ONE) of auxiliary variables whose columns coincide in A, B and C (host only)"""
    n = lib().zkgpu_test_equal_columns(r1cs_path.encode(), None, ctypes.c_size_t(0))
    if n < 0: _check(n)
    buf = (ctypes.c_uint32 * max(1, n))(); lib().zkgpu_test_equal_columns(r1cs_path.encode(), buf, ctypes.c_size_t(n)); out = []; i = 0
    while i < n: k = buf[i]; out.append([int(v) for v in buf[i + 1:i + 1 + k]]); i += 1 + k
    return out
def general_path_repeats():
    lib().zkgpu_general_path_repeats.restype = ctypes.c_uint64; return int(lib().zkgpu_general_path_repeats())
def verify_counters(vk_path):
    """(small verification calls taken by the key's GPU verifier, launches made for them)"""
    out = (ctypes.c_uint64 * 2)(); _check(lib().zkgpu_verify_counters(vk_path.encode(), out)); return int(out[0]), int(out[1])
def verify_path_counters(vk_path):
    """(small calls, launches for them, launches of the workgroup-per-proof branch, launches of the lane-per-proof branch) of the key's GPU verifier"""
    out = (ctypes.c_uint64 * 4)(); _check(lib().zkgpu_verify_path_counters(vk_path.encode(), out)); return tuple(int(x) for x in out)
def verify_trace(vk_path, proof_hex, inputs, every=1):
    """kernel K9 on one proof with its values written out after every `every`-th round, compared with the host model of the same arithmetic:
    (first differing round or -1, slot, the kernel's verdict)"""
    buf = b"".join(int(x).to_bytes(32, "little") for x in inputs); out = (ctypes.c_long * 3)()
    _check(lib().zkgpu_test_verify_trace(vk_path.encode(), proof_hex.encode(), buf, ctypes.c_size_t(len(inputs)), ctypes.c_uint32(every), out)); return int(out[0]), int(out[1]), int(out[2])
def verify(vk_path, proof_hex, inputs):
    """inputs: list of ints (packed public input).  True / False."""
    buf = b"".join(int(x).to_bytes(32, "little") for x in inputs)
    rc = lib().zkgpu_verify(vk_path.encode(), proof_hex.encode(), buf, ctypes.c_size_t(len(inputs)))
    if rc < 0: _check(rc)
    return bool(rc)

# ---- the commitment tree resident in HBM (include/zkgpu.h "commitment tree") ---------------------------------------------
class Tree:
    """append-only SHA-256 Merkle tree of depth 1..32 on the device; leaves, siblings and roots are 32-byte strings in blob order (the reverse of the hex the cgo symbols print)"""
    def __init__(self, depth):
        lib().zkgpu_tree_create.restype = ctypes.c_void_p; self.depth = int(depth); self.h = lib().zkgpu_tree_create(self.depth)
        if not self.h: raise ZkGpuError(lib().zkgpu_last_error().decode())
    def append(self, leaves):
        """leaves: a list of 32-byte strings, or one bytes object of n x 32 bytes"""
        buf = leaves if isinstance(leaves, (bytes, bytearray)) else b"".join(bytes(x) for x in leaves); assert len(buf) % 32 == 0
        _check(lib().zkgpu_tree_append(ctypes.c_void_p(self.h), bytes(buf), ctypes.c_size_t(len(buf) // 32)))
    def size(self):
        n = ctypes.c_uint64(0); _check(lib().zkgpu_tree_size(ctypes.c_void_p(self.h), ctypes.byref(n))); return int(n.value)
    def root(self):
        out = ctypes.create_string_buffer(32); _check(lib().zkgpu_tree_root(ctypes.c_void_p(self.h), out)); return out.raw
    def path(self, index):
        """the siblings of leaf `index`, leaf level first"""
        out = ctypes.create_string_buffer(32 * self.depth); _check(lib().zkgpu_tree_path(ctypes.c_void_p(self.h), ctypes.c_uint64(index), out)); return [out.raw[32 * k:32 * k + 32] for k in range(self.depth)]
    def find(self, leaf):
        """index of the first leaf equal to the blob; raises ZkGpuError if there is none"""
        i = ctypes.c_uint64(0); _check(lib().zkgpu_tree_find(ctypes.c_void_p(self.h), bytes(leaf), ctypes.byref(i))); return int(i.value)
    def launches(self):
        k = ctypes.c_uint64(0); _check(lib().zkgpu_test_tree_launches(ctypes.c_void_p(self.h), ctypes.byref(k))); return int(k.value)
    # past states: state m = the tree of the first m leaves, 0 <= m <= size()
    def roots_at(self, sizes):
        """the roots of the states `sizes` (any order, repeats allowed), one launch -> [32-byte root]"""
        m = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1); q = int(m.size); out = ctypes.create_string_buffer(max(1, 32 * q))
        _check(lib().zkgpu_tree_roots_at(ctypes.c_void_p(self.h), m.ctypes.data_as(ctypes.c_void_p) if q else None, ctypes.c_size_t(q), out)); return [out.raw[32 * i:32 * i + 32] for i in range(q)]
    def paths_at(self, size, indices):
        """-> ([siblings of leaf i in state `size`, leaf level first, for i in indices], the root of that state)"""
        ix = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1); q = int(ix.size); d = self.depth; out = ctypes.create_string_buffer(max(1, 32 * q * d)); root = ctypes.create_string_buffer(32)
        _check(lib().zkgpu_tree_paths_at(ctypes.c_void_p(self.h), ctypes.c_uint64(size), ix.ctypes.data_as(ctypes.c_void_p) if q else None, ctypes.c_size_t(q), out, root))
        return [[out.raw[32 * (i * d + k):32 * (i * d + k) + 32] for k in range(d)] for i in range(q)], root.raw
    def find_at(self, size, leaf):
        """index of the first of the first `size` leaves equal to the blob; raises ZkGpuError if there is none"""
        i = ctypes.c_uint64(0); _check(lib().zkgpu_tree_find_at(ctypes.c_void_p(self.h), ctypes.c_uint64(size), bytes(leaf), ctypes.byref(i))); return int(i.value)
    def match_roots(self, sizes, rts, hash_order=False):
        """for each 32-byte RT the lowest index a with root(sizes[a]) == RT, or -1; two launches.  hash_order: the RTs as the bytes of the common.Hash"""
        m = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1); k = int(m.size); buf = rts if isinstance(rts, (bytes, bytearray)) else b"".join(bytes(x) for x in rts); assert len(buf) % 32 == 0
        q = len(buf) // 32; out = np.full(max(1, q), -7, dtype=np.int32)
        _check(lib().zkgpu_tree_match_roots(ctypes.c_void_p(self.h), m.ctypes.data_as(ctypes.c_void_p) if k else None, ctypes.c_size_t(k), bytes(buf) if q else None, ctypes.c_size_t(q), int(bool(hash_order)),
                                            out.ctypes.data_as(ctypes.c_void_p)))
        return [int(x) for x in out[:q]]
    def match_roots_window(self, sizes, rts, lo, hi, hash_order=False):
        """match_roots with a window a record: the lowest a with lo[i] <= a < hi[i] and root(sizes[a]) == RT i, or -1; two launches"""
        m = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(-1); k = int(m.size); buf = rts if isinstance(rts, (bytes, bytearray)) else b"".join(bytes(x) for x in rts); assert len(buf) % 32 == 0
        q = len(buf) // 32; out = np.full(max(1, q), -7, dtype=np.int32); l = np.ascontiguousarray(lo, dtype=np.uint32).reshape(-1); h = np.ascontiguousarray(hi, dtype=np.uint32).reshape(-1); assert l.size == h.size == q
        _check(lib().zkgpu_tree_match_roots_window(ctypes.c_void_p(self.h), m.ctypes.data_as(ctypes.c_void_p) if k else None, ctypes.c_size_t(k), bytes(buf) if q else None, ctypes.c_size_t(q),
                                                   l.ctypes.data_as(ctypes.c_void_p) if q else None, h.ctypes.data_as(ctypes.c_void_p) if q else None, int(bool(hash_order)), out.ctypes.data_as(ctypes.c_void_p)))
        return [int(x) for x in out[:q]]
    def rewind(self, size):
        """the tree goes back to its first `size` leaves"""
        _check(lib().zkgpu_tree_rewind(ctypes.c_void_p(self.h), ctypes.c_uint64(size)))
    def state_launches(self):
        k = ctypes.c_uint64(0); _check(lib().zkgpu_test_tree_state_launches(ctypes.c_void_p(self.h), ctypes.byref(k))); return int(k.value)
    def close(self):
        if self.h: lib().zkgpu_tree_destroy(ctypes.c_void_p(self.h)); self.h = None
    def __del__(self):
        try: self.close()
        except Exception: pass
def tree_host(depth, leaves, index=None, want_root=True):
    """the host model of the same tree (notes.cpp: tree_levels), no device needed -> (root or None, siblings of `index` leaf level first or None)"""
    buf = leaves if isinstance(leaves, (bytes, bytearray)) else b"".join(bytes(x) for x in leaves); n = len(buf) // 32
    root = ctypes.create_string_buffer(32) if want_root else None; path = ctypes.create_string_buffer(32 * depth) if index is not None else None
    _check(lib().zkgpu_test_tree_host(int(depth), bytes(buf) if n else None, ctypes.c_size_t(n), ctypes.c_uint64(index or 0), root, path))
    return (root.raw if want_root else None), ([path.raw[32 * k:32 * k + 32] for k in range(depth)] if path is not None else None)

# ---- the set of spent serial numbers resident in HBM (include/zkgpu.h "the set of spent serial numbers"; the drop-in level is include/zk_spent.h) ----
ABSENT = (1 << 64) - 1
def _keys20(keys):
    """a list of 20-byte strings, one bytes object of n x 20 bytes, or an (n, 20) uint8 array -> (bytes, n)"""
    buf = keys.tobytes() if isinstance(keys, np.ndarray) else bytes(keys) if isinstance(keys, (bytes, bytearray)) else b"".join(bytes(k) for k in keys)
    assert len(buf) % 20 == 0; return buf, len(buf) // 20
class SpentSet:
    """append-only set of 20-byte keys on the device: the log of distinct keys in insertion order and an index over it; state m = the first m keys"""
    def __init__(self, exempt=None, log2_slots=None, seed=0):
        """log2_slots: the test entry (a table of 2^log2_slots slots and the given seed); otherwise 2^10 slots and a seed from getrandom"""
        L = lib(); L.zkgpu_snset_create.restype = ctypes.c_void_p; L.zkgpu_test_snset_create.restype = ctypes.c_void_p; ex = bytes(exempt) if exempt is not None else None
        self.h = L.zkgpu_snset_create(ex) if log2_slots is None else L.zkgpu_test_snset_create(int(log2_slots), ctypes.c_uint64(seed), ex)
        if not self.h: raise ZkGpuError(lib().zkgpu_last_error().decode())
    def size(self):
        n = ctypes.c_uint64(0); _check(lib().zkgpu_snset_size(ctypes.c_void_p(self.h), ctypes.byref(n))); return int(n.value)
    def spend(self, keys, mask=None, commit=True):
        """-> ([conflict code per record: 0 fresh or skipped, 1 in the set before the call, 2 an earlier masked-in record of the call has it], the size after the call)"""
        buf, n = _keys20(keys); m = bytes(bytearray(int(bool(x)) for x in mask)) if mask is not None else None; assert m is None or len(m) == n
        out = ctypes.create_string_buffer(max(1, n)); size = ctypes.c_uint64(0)
        _check(lib().zkgpu_snset_spend(ctypes.c_void_p(self.h), buf, m, ctypes.c_size_t(n), int(bool(commit)), out, ctypes.byref(size))); return list(out.raw[:n]), int(size.value)
    def spend_pairs(self, pairs, commit=True):
        """pairs: one entry a record — None or () (masked out), (k1,) or (k1, k2), 20-byte keys -> ([code per record: 0 accepted or masked out, 1 a key was in the set before
        the call or k2 is the exempt key, 2 an earlier accepted record of the call has one of the keys or k1 == k2], the size after the call)"""
        buf, nk, n = _pairs40(pairs); out = ctypes.create_string_buffer(max(1, n)); size = ctypes.c_uint64(0)
        _check(lib().zkgpu_snset_spend_pairs(ctypes.c_void_p(self.h), buf, nk, ctypes.c_size_t(n), int(bool(commit)), out, ctypes.byref(size))); return list(out.raw[:n]), int(size.value)
    def round_cap(self, rounds): _check(lib().zkgpu_test_snset_round_cap(ctypes.c_void_p(self.h), ctypes.c_uint32(rounds)))   # test entry: 0 = the default
    def query(self, size, keys):
        """-> [position of the key in the log if it is below `size`, else None]"""
        buf, q = _keys20(keys); out = (ctypes.c_uint64 * max(1, q))()
        _check(lib().zkgpu_snset_query(ctypes.c_void_p(self.h), ctypes.c_uint64(size), buf, ctypes.c_size_t(q), out)); return [None if out[i] == ABSENT else int(out[i]) for i in range(q)]
    def rewind(self, size): _check(lib().zkgpu_snset_rewind(ctypes.c_void_p(self.h), ctypes.c_uint64(size)))
    def read_log(self, first=0, count=None):
        """-> [20-byte key] of log entries first .. first + count - 1 (count None: to the end)"""
        count = self.size() - first if count is None else count; out = ctypes.create_string_buffer(max(1, 20 * count))
        _check(lib().zkgpu_snset_read_log(ctypes.c_void_p(self.h), ctypes.c_uint64(first), ctypes.c_uint64(count), out)); return [out.raw[20 * i:20 * i + 20] for i in range(count)]
    def slots(self):
        """test entry -> (the table as a uint32 array, the seed, the host's tombstone count)"""
        n = ctypes.c_uint64(0); seed = ctypes.c_uint64(0); tombs = ctypes.c_uint64(0); h = ctypes.c_void_p(self.h)
        _check(lib().zkgpu_test_snset_slots(h, None, ctypes.byref(n), ctypes.byref(seed), ctypes.byref(tombs))); t = np.zeros(int(n.value), dtype=np.uint32)
        _check(lib().zkgpu_test_snset_slots(h, t.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), ctypes.byref(seed), ctypes.byref(tombs))); return t, int(seed.value), int(tombs.value)
    def close(self):
        if self.h: lib().zkgpu_snset_destroy(ctypes.c_void_p(self.h)); self.h = None
    def __del__(self):
        try: self.close()
        except Exception: pass
def _pairs40(pairs):
    """[None | (k1,) | (k1, k2)] -> (n x 40 bytes, n bytes of key counts, n)"""
    buf = bytearray(); nk = bytearray()
    for p in pairs:
        p = tuple(p or ()); assert len(p) <= 2 and all(len(k) == 20 for k in p); nk.append(len(p)); buf += b"".join(bytes(k) for k in p) + bytes(20 * (2 - len(p)))
    return bytes(buf), bytes(nk), len(nk)
def snset_launches():
    """kernels launched by all spent sets of this process so far"""
    k = ctypes.c_uint64(0); _check(lib().zkgpu_test_snset_launches(ctypes.byref(k))); return int(k.value)
def snset_host(resident, exempt, keys, mask=None, commit=True):
    """zkgpu_test_snset_host: the plain sequential loop, no device needed -> ([conflict code], [appended key])"""
    rb, nr = _keys20(resident); kb, n = _keys20(keys); m = bytes(bytearray(int(bool(x)) for x in mask)) if mask is not None else None
    out = ctypes.create_string_buffer(max(1, n)); app = ctypes.create_string_buffer(max(1, 20 * n)); na = ctypes.c_size_t(0)
    _check(lib().zkgpu_test_snset_host(rb if nr else None, ctypes.c_size_t(nr), bytes(exempt) if exempt is not None else None, kb if n else None, m, ctypes.c_size_t(n), int(bool(commit)), out, app, ctypes.byref(na)))
    return list(out.raw[:n]), [app.raw[20 * i:20 * i + 20] for i in range(int(na.value))]
def snset_host_pairs(resident, exempt, pairs, commit=True):
    """zkgpu_test_snset_host_pairs: the sequential loop with up to two keys a record (pairs as SpentSet.spend_pairs takes them) -> ([conflict code], [appended key])"""
    rb, nr = _keys20(resident); buf, nk, n = _pairs40(pairs); out = ctypes.create_string_buffer(max(1, n)); app = ctypes.create_string_buffer(max(1, 40 * n)); na = ctypes.c_size_t(0)
    _check(lib().zkgpu_test_snset_host_pairs(rb if nr else None, ctypes.c_size_t(nr), bytes(exempt) if exempt is not None else None, buf if n else None, nk if n else None, ctypes.c_size_t(n), int(bool(commit)), out, app,
                                             ctypes.byref(na)))
    return list(out.raw[:n]), [app.raw[20 * i:20 * i + 20] for i in range(int(na.value))]
def snset_rounds():
    """(rounds the spent sets of this process have run on the device, calls the host finished after the round cap)"""
    r = ctypes.c_uint64(0); h = ctypes.c_uint64(0); _check(lib().zkgpu_test_snset_rounds(ctypes.byref(r), ctypes.byref(h))); return int(r.value), int(h.value)
def snset_home(key, seed, n_slots):
    """the documented mix (include/zkgpu.h): the home slot of a 20-byte key in a table of n_slots slots"""
    M = (1 << 64) - 1; h = seed
    for k in range(5): h = ((h ^ int.from_bytes(key[4 * k:4 * k + 4], "little")) * 0x9E3779B97F4A7C15) & M; h ^= h >> 32
    h = (h * 0xD6E8FEB86659FD93) & M; h ^= h >> 32; return h & (n_slots - 1)
def record_sn(rec):
    """the serial number a record (RECORD_DTYPE) spends, the 32 bytes of its common.Hash: snold = args[3] for deposit, args[1] for mint, send and redeem; the set's key is [12:]"""
    return bytes(rec["args"][3 if int(rec["kind"]) == KIND["deposit"] else 1])

# ---- the account table resident in HBM (include/zkgpu.h "the account table"; the drop-in level is include/zk_accounts.h) ----
ACCT_OLD_ARG = {0: 0, 1: 0, 2: 2, 3: 0}   # kind -> the args entry that holds the sender's balance commitment before the record
ACCT_NEW_ARG = {0: 2, 1: 3, 2: 4, 3: 2}   # ... and after it
def _vals32(values):
    buf = values.tobytes() if isinstance(values, np.ndarray) else bytes(values) if isinstance(values, (bytes, bytearray)) else b"".join(bytes(v) for v in values)
    assert len(buf) % 32 == 0; return buf, len(buf) // 32
class AccountTable:
    """a map from 20-byte addresses to 32-byte values on the device: an append-only log of (address, value, prev) entries and an index over it; state m = the first
    m entries, the value of an address at state m = that of its latest entry below m, or 32 zero bytes"""
    def __init__(self, log2_slots=None, seed=0):
        """log2_slots: the test entry (a table of 2^log2_slots slots and the given seed); otherwise 2^10 slots and a seed from getrandom"""
        L = lib(); L.zkgpu_accts_create.restype = ctypes.c_void_p; L.zkgpu_test_accts_create.restype = ctypes.c_void_p
        self.h = L.zkgpu_accts_create() if log2_slots is None else L.zkgpu_test_accts_create(int(log2_slots), ctypes.c_uint64(seed))
        if not self.h: raise ZkGpuError(lib().zkgpu_last_error().decode())
    def size(self):
        n = ctypes.c_uint64(0); _check(lib().zkgpu_accts_size(ctypes.c_void_p(self.h), ctypes.byref(n))); return int(n.value)
    def set(self, addrs, values):
        ab, n = _keys20(addrs); vb, nv = _vals32(values); assert n == nv; _check(lib().zkgpu_accts_set(ctypes.c_void_p(self.h), ab, vb, ctypes.c_size_t(n)))
    def get(self, addrs, at_size=-1):
        """-> [32-byte value of each address at state at_size (-1: now)]"""
        ab, n = _keys20(addrs); out = ctypes.create_string_buffer(max(1, 32 * n))
        _check(lib().zkgpu_accts_get(ctypes.c_void_p(self.h), ab, ctypes.c_size_t(n), ctypes.c_int64(at_size), out)); return [out.raw[32 * i:32 * i + 32] for i in range(n)]
    def fill(self, addrs, recs, chained):
        """-> a copy of the records (RECORD_DTYPE) with their old slots filled"""
        ab, n = _keys20(addrs); recs = np.array(recs, dtype=RECORD_DTYPE, copy=True); assert recs.shape == (n,)
        _check(lib().zkgpu_accts_fill(ctypes.c_void_p(self.h), ab, recs.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n), int(bool(chained)))); return recs
    def commit_chain(self, addrs, recs):
        ab, n = _keys20(addrs); recs, ptr, nr = _recs(recs); assert n == nr; _check(lib().zkgpu_accts_commit_chain(ctypes.c_void_p(self.h), ab, ptr, ctypes.c_size_t(n)))
    def fill_segment(self, addrs, recs):
        """fill(chained=True) by the tiled predecessor search: for a stretch of the chain, where one sender may have any share of the records"""
        ab, n = _keys20(addrs); recs = np.array(recs, dtype=RECORD_DTYPE, copy=True); assert recs.shape == (n,)
        _check(lib().zkgpu_accts_fill_segment(ctypes.c_void_p(self.h), ab, recs.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n))); return recs
    def commit_segment(self, addrs, recs):
        """commit_chain by the tiled predecessor search"""
        ab, n = _keys20(addrs); recs, ptr, nr = _recs(recs); assert n == nr; _check(lib().zkgpu_accts_commit_segment(ctypes.c_void_p(self.h), ab, ptr, ctypes.c_size_t(n)))
    def rewind(self, size): _check(lib().zkgpu_accts_rewind(ctypes.c_void_p(self.h), ctypes.c_uint64(size)))
    def read_log(self, first=0, count=None):
        """-> [(20-byte address, 32-byte value, prev)] of log entries first .. first + count - 1 (count None: to the end)"""
        count = self.size() - first if count is None else count; out = ctypes.create_string_buffer(max(1, 56 * count))
        _check(lib().zkgpu_accts_read_log(ctypes.c_void_p(self.h), ctypes.c_uint64(first), ctypes.c_uint64(count), out))
        return [(out.raw[56 * i:56 * i + 20], out.raw[56 * i + 20:56 * i + 52], int.from_bytes(out.raw[56 * i + 52:56 * i + 56], "little")) for i in range(count)]
    def slots(self):
        """test entry -> (the index as a uint32 array, the seed, the host's tombstone count)"""
        n = ctypes.c_uint64(0); seed = ctypes.c_uint64(0); tombs = ctypes.c_uint64(0); h = ctypes.c_void_p(self.h)
        _check(lib().zkgpu_test_accts_slots(h, None, ctypes.byref(n), ctypes.byref(seed), ctypes.byref(tombs))); t = np.zeros(int(n.value), dtype=np.uint32)
        _check(lib().zkgpu_test_accts_slots(h, t.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), ctypes.byref(seed), ctypes.byref(tombs))); return t, int(seed.value), int(tombs.value)
    def chain_cap(self, cap): _check(lib().zkgpu_test_accts_chain_cap(ctypes.c_void_p(self.h), ctypes.c_uint32(cap)))   # test entry: 0 = the default
    def close(self):
        if self.h: lib().zkgpu_accts_destroy(ctypes.c_void_p(self.h)); self.h = None
    def __del__(self):
        try: self.close()
        except Exception: pass
def accts_launches():
    """(kernels launched by all account tables of this process so far, predecessor searches the host finished)"""
    k = ctypes.c_uint64(0); h = ctypes.c_uint64(0); _check(lib().zkgpu_test_accts_launches(ctypes.byref(k), ctypes.byref(h))); return int(k.value), int(h.value)
def _accts_handle(a): return None if a is None else ctypes.c_void_p(a.h if isinstance(a, AccountTable) else a)

# ---- the proof cache (include/zkgpu.h "the proof cache"; the drop-in level is include/zk_proof_cache.h) ----
class ProofCache:
    """the records whose proof this process has accepted, by keyed digest, in two generations on the device.  salt: the test entry (32 given bytes instead of getrandom)"""
    def __init__(self, capacity, salt=None):
        L = lib(); L.zkgpu_proof_cache_create.restype = ctypes.c_void_p; L.zkgpu_test_proof_cache_create.restype = ctypes.c_void_p
        self.h = L.zkgpu_proof_cache_create(ctypes.c_uint64(capacity)) if salt is None else L.zkgpu_test_proof_cache_create(ctypes.c_uint64(capacity), bytes(salt))
        if not self.h: raise ZkGpuError(lib().zkgpu_last_error().decode())
    def stats(self):
        """-> (hits, misses, keys stored, entries held now)"""
        out = (ctypes.c_uint64 * 4)(); _check(lib().zkgpu_proof_cache_stats(ctypes.c_void_p(self.h), out)); return tuple(int(x) for x in out)
    def clear(self): _check(lib().zkgpu_proof_cache_clear(ctypes.c_void_p(self.h)))
    def close(self):
        if self.h: lib().zkgpu_proof_cache_destroy(ctypes.c_void_p(self.h)); self.h = None
    def __del__(self):
        try: self.close()
        except Exception: pass
def record_digests(salt, tags, recs, device=True):
    """zkgpu_test_record_digests: the cache keys of records under a 32-byte salt and the four kinds' 32-byte tags -> (n, 20) uint8, zeros for a kind above 3;
    from k_record_digest (device=True) or from the host model (device=False: needs no device)"""
    recs, ptr, n = _recs(recs); tb = b"".join(bytes(t) for t in tags); assert len(tb) == 128 and len(bytes(salt)) == 32; out = np.zeros((max(1, n), 20), dtype=np.uint8)
    _check(lib().zkgpu_test_record_digests(bytes(salt), tb, ptr, ctypes.c_size_t(n), int(bool(device)), _bytes(out))); return out[:n]
def proof_cache_launches():
    """digest kernels launched by this process so far"""
    k = ctypes.c_uint64(0); _check(lib().zkgpu_test_proof_cache_launches(ctypes.byref(k))); return int(k.value)
def _cache_handle(cache): return None if cache is None else ctypes.c_void_p(cache.h if isinstance(cache, ProofCache) else cache)

# ---- the roots of many commitment lists (include/zkgpu.h "the roots of many commitment lists"; the drop-in level is include/zk_roots.h) ----
def _leaf_array(leaves):
    """leaves: an (n, 32) uint8 array, one bytes object of n x 32 bytes, or a list of 32-byte strings -> flat uint8 array"""
    if isinstance(leaves, np.ndarray): a = np.ascontiguousarray(leaves, dtype=np.uint8).reshape(-1)
    else: a = np.frombuffer(leaves if isinstance(leaves, (bytes, bytearray)) else b"".join(bytes(x) for x in leaves), dtype=np.uint8)
    assert a.size % 32 == 0; return a
def _leaf_ranges(lists):
    r = np.ascontiguousarray(np.asarray(lists, dtype=np.uint64).reshape(-1, 2)); return r, (r.ctypes.data_as(ctypes.c_void_p) if r.shape[0] else None), int(r.shape[0])
def _list_roots(fn, depth, leaves, lists, hash_order):
    buf = _leaf_array(leaves); r, ptr, n = _leaf_ranges(lists); out = np.zeros((max(1, n), 32), dtype=np.uint8)
    _check(fn(int(depth), _bytes(buf) if buf.size else None, ctypes.c_size_t(buf.size // 32), ptr, ctypes.c_size_t(n), int(bool(hash_order)), _bytes(out))); return out[:n]
def list_roots(depth, leaves, lists, hash_order=False):
    """zkgpu_list_roots: lists = [(first, count)] into the shared leaves -> (n_lists, 32) uint8, root i over leaves[first:first + count] alone, on the device.
    hash_order: leaves and roots as the bytes of the common.Hash instead of blob order"""
    return _list_roots(lib().zkgpu_list_roots, depth, leaves, lists, hash_order)
def list_roots_host(depth, leaves, lists, hash_order=False):
    """zkgpu_test_list_roots_host: the same roots by the host model (notes.cpp: merkle_root), no device needed"""
    return _list_roots(lib().zkgpu_test_list_roots_host, depth, leaves, lists, hash_order)
def list_roots_launches():
    """root kernels launched by this process so far"""
    k = ctypes.c_uint64(0); _check(lib().zkgpu_test_list_roots_launches(ctypes.byref(k))); return int(k.value)
class _CmtLists(ctypes.Structure):   # zk_cmt_lists
    _fields_ = [("cmts", ctypes.c_void_p), ("n_cmts", ctypes.c_uint64), ("lists", ctypes.c_void_p), ("n_lists", ctypes.c_int)]
def _cmt_lists(cmts, lists):
    buf = _leaf_array(cmts); r, ptr, n = _leaf_ranges(lists)
    return _CmtLists(buf.ctypes.data_as(ctypes.c_void_p) if buf.size else None, buf.size // 32, ptr, n), (buf, r)   # (the arrays must outlive the call)

class Zk:
    """the drop-in symbols (what go-ethereum/zktx calls through cgo), bound the way zktx.go marshals them: "0x…" hex strings and uint64"""
    def __init__(self):
        L = lib()
        for f in ("genCMT", "genCMTS", "computePRF", "computeCRH", "genRoot", "genMintproof", "genSendproof", "genRedeemproof", "genDepositproof"): getattr(L, f).restype = ctypes.c_char_p
        for f in ("verifyMintproof", "verifySendproof", "verifyRedeemproof", "verifyDepositproof"): getattr(L, f).restype = ctypes.c_bool
        for f in ("zkTreeRoot", "genDepositproofTree"): getattr(L, f).restype = ctypes.c_char_p
        L.zkTreeNew.restype = ctypes.c_void_p; L.zkTreeAppend.restype = ctypes.c_longlong; L.verifyDepositproofDepth.restype = ctypes.c_bool
        for f in ("zkTreeRootAt", "genDepositproofTreeAt"): getattr(L, f).restype = ctypes.c_char_p
        L.zkTreeRewind.restype = ctypes.c_longlong; L.zkTreeRootsAt.restype = ctypes.c_int
        self.L = L
    @staticmethod
    def hx(b): return ("0x" + bytes(b).hex()).encode()          # common.ToHex
    def GenCMT(self, value, sn, r): return bytes.fromhex(self.L.genCMT(ctypes.c_uint64(value), self.hx(sn), self.hx(r)).decode())
    def GenCMTS(self, value, pk, rs, sn_old): return bytes.fromhex(self.L.genCMTS(ctypes.c_uint64(value), self.hx(pk), self.hx(rs), self.hx(sn_old)).decode())
    def ComputePRF(self, sk, r): return bytes.fromhex(self.L.computePRF(self.hx(sk), self.hx(r)).decode())
    def ComputeCRH(self, pk, r): return bytes.fromhex(self.L.computeCRH(self.hx(pk), self.hx(r)).decode())
    def GenRT(self, cmts): return bytes.fromhex(self.L.genRoot(b"".join(self.hx(c) for c in cmts), len(cmts)).decode())
    def GenSendProof(self, valueA, rS, snA, rA, cmtS, cmtA, valueS, pk_recv, valueANew, snAnew, rAnew, cmtAnew, sk, pk_sender):   # zktx.go:406-430
        return self.L.genSendproof(ctypes.c_uint64(valueA), self.hx(rS), self.hx(snA), self.hx(rA), self.hx(cmtS), self.hx(cmtA), ctypes.c_uint64(valueS), self.hx(pk_recv), ctypes.c_uint64(valueANew), self.hx(snAnew), self.hx(rAnew), self.hx(cmtAnew), self.hx(sk), self.hx(pk_sender)).decode()
    def VerifySendProof(self, proof, cmtA_old, sn_old, cmtS, cmtA_new): return bool(self.L.verifySendproof(proof.encode(), self.hx(cmtA_old), self.hx(sn_old), self.hx(cmtS), self.hx(cmtA_new)))
    def GenDepositProof(self, value, value_old, sn_old, r_old, sn, r, sns, rs, cmtB_old, cmtB, value_s, pk, sn_A_old, cmtS, cmts, RT, sk):
        return self.L.genDepositproof(ctypes.c_uint64(value), ctypes.c_uint64(value_old), self.hx(sn_old), self.hx(r_old), self.hx(sn), self.hx(r), self.hx(sns), self.hx(rs), self.hx(cmtB_old), self.hx(cmtB), ctypes.c_uint64(value_s),
                                      self.hx(pk), self.hx(sn_A_old), self.hx(cmtS), b"".join(self.hx(c) for c in cmts), len(cmts), self.hx(RT), self.hx(sk)).decode()
    def VerifyDepositProof(self, proof, RT, pk, cmtb_old, sn_old, cmtb, sns): return bool(self.L.verifyDepositproof(proof.encode(), self.hx(RT), self.hx(pk), self.hx(cmtb_old), self.hx(sn_old), self.hx(cmtb), self.hx(sns)))
    def GenMintProof(self, value, value_old, sn_old, r_old, sn, r, cmtA_old, cmtA, value_s, sk):
        return self.L.genMintproof(ctypes.c_uint64(value), ctypes.c_uint64(value_old), self.hx(sn_old), self.hx(r_old), self.hx(sn), self.hx(r), self.hx(cmtA_old), self.hx(cmtA), ctypes.c_uint64(value_s), self.hx(sk)).decode()
    def VerifyMintProof(self, proof, cmtA_old, sn_old, cmtA, value_s): return bool(self.L.verifyMintproof(proof.encode(), self.hx(cmtA_old), self.hx(sn_old), self.hx(cmtA), ctypes.c_uint64(value_s)))
    def VerifyBatch(self, items):
        """include/zk_batch.h: items = list of (kind, proof_hex, [big-endian byte strings in the order of the kind's verify symbol], value_s) -> (accepted, [bool])"""
        class Item(ctypes.Structure): _fields_ = [("kind", ctypes.c_int), ("proof", ctypes.c_char_p), ("args", ctypes.c_char_p * 6), ("value_s", ctypes.c_uint64)]
        arr = (Item * max(1, len(items)))(); keep = []
        for i, (kind, proof, args, value_s) in enumerate(items):
            arr[i].kind = KIND[kind] if isinstance(kind, str) else int(kind); pb = proof.encode() if isinstance(proof, str) else proof; keep.append(pb); arr[i].proof = pb; arr[i].value_s = int(value_s or 0)
            for j, a in enumerate(args): hb = self.hx(a); keep.append(hb); arr[i].args[j] = hb
        ok = (ctypes.c_ubyte * max(1, len(items)))(); self.L.verifyBatch.restype = ctypes.c_int; rc = self.L.verifyBatch(arr, len(items), ok); return rc, [bool(ok[i]) for i in range(len(items))]
    def VerifyBlock(self, items):
        """include/zk_block.h: the same items and verdicts as VerifyBatch, by one randomized check over the block -> (accepted, [bool])"""
        class Item(ctypes.Structure): _fields_ = [("kind", ctypes.c_int), ("proof", ctypes.c_char_p), ("args", ctypes.c_char_p * 6), ("value_s", ctypes.c_uint64)]
        arr = (Item * max(1, len(items)))(); keep = []
        for i, (kind, proof, args, value_s) in enumerate(items):
            arr[i].kind = KIND[kind] if isinstance(kind, str) else int(kind); pb = proof.encode() if isinstance(proof, str) else proof; keep.append(pb); arr[i].proof = pb; arr[i].value_s = int(value_s or 0)
            for j, a in enumerate(args): hb = self.hx(a); keep.append(hb); arr[i].args[j] = hb
        ok = (ctypes.c_ubyte * max(1, len(items)))(); self.L.verifyBlock.restype = ctypes.c_int; rc = self.L.verifyBlock(arr, len(items), ok); return rc, [bool(ok[i]) for i in range(len(items))]
    def VerifyBlockRecords(self, items):
        """include/zk_records.h: the items of VerifyBlock (or an array records_from_items made of them) as one array of binary records -> (accepted, [bool])"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs, ptr, n = _recs(recs)
        ok = (ctypes.c_ubyte * max(1, n))(); self.L.verifyBlockRecords.restype = ctypes.c_int; rc = self.L.verifyBlockRecords(ptr, n, ok); return rc, [bool(ok[i]) for i in range(n)]
    def GenRoots(self, cmts, lists, depth=8):
        """include/zk_roots.h: cmts = the shared array of commitments (big-endian, as common.Hash), lists = [(first, count)] -> [root as big-endian bytes]; raises on -1"""
        l, keep = _cmt_lists(cmts, lists); out = np.zeros((max(1, l.n_lists), 32), dtype=np.uint8); self.L.genRoots.restype = ctypes.c_int
        if self.L.genRoots(ctypes.byref(l), int(depth), _bytes(out)) != 0: raise ZkGpuError("genRoots: " + lib().zkgpu_last_error().decode())
        return [out[i].tobytes() for i in range(l.n_lists)]
    def VerifyBlockRecordsRoots(self, items, cmts, lists, list_of):
        """include/zk_roots.h: VerifyBlockRecords, and RT of record i against the depth-8 root of list list_of[i] (-1: no root check) -> (accepted, [bool]).
        lists = None passes no zk_cmt_lists at all"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs, ptr, n = _recs(recs)
        l, keep = _cmt_lists(cmts, lists) if lists is not None else (None, None); lo = np.ascontiguousarray(list_of, dtype=np.int32); assert lo.shape == (n,)
        ok = (ctypes.c_ubyte * max(1, n))(); self.L.verifyBlockRecordsRoots.restype = ctypes.c_int
        rc = self.L.verifyBlockRecordsRoots(ptr, n, ctypes.byref(l) if l is not None else None, lo.ctypes.data_as(ctypes.c_void_p) if n else None, ok); return rc, [bool(ok[i]) for i in range(n)]
    # include/zk_spent.h: the resident set of spent serial numbers at the drop-in level (serial numbers as the 32 bytes of their common.Hash)
    def SnSetNew(self, exempt_sn=None):
        self.L.zkSnSetNew.restype = ctypes.c_void_p; return self.L.zkSnSetNew(bytes(exempt_sn) if exempt_sn is not None else None)   # None on failure
    def SnSetFree(self, s): self.L.zkSnSetFree(ctypes.c_void_p(s))
    def SnSetSize(self, s): self.L.zkSnSetSize.restype = ctypes.c_longlong; return int(self.L.zkSnSetSize(ctypes.c_void_p(s) if s else None))
    def SnSetContains(self, s, sns, size=-1):
        """-> [bool], None on failure"""
        buf = b"".join(bytes(x) for x in sns); n = len(sns); out = ctypes.create_string_buffer(max(1, n))
        rc = self.L.zkSnSetContains(ctypes.c_void_p(s) if s else None, ctypes.c_longlong(size), buf, n, out); return [bool(b) for b in out.raw[:n]] if rc == 0 else None
    def SnSetRewind(self, s, size): self.L.zkSnSetRewind.restype = ctypes.c_longlong; return int(self.L.zkSnSetRewind(ctypes.c_void_p(s) if s else None, ctypes.c_longlong(size)))
    def SnSetSpend(self, s, sns, commit=True):
        """-> (the size after the call or -1, [spent?])"""
        buf = b"".join(bytes(x) for x in sns); n = len(sns); out = ctypes.create_string_buffer(max(1, n)); self.L.zkSnSetSpend.restype = ctypes.c_longlong
        size = int(self.L.zkSnSetSpend(ctypes.c_void_p(s) if s else None, buf, n, int(bool(commit)), out)); return size, [bool(b) for b in out.raw[:n]]
    def VerifyBlockFull(self, items, cmts, lists, list_of, s, commit):
        """include/zk_spent.h: VerifyBlockRecordsRoots, then the serial numbers of the accepted records against the set `s` (None: no set) -> (accepted, [bool], size after or None)"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs, ptr, n = _recs(recs)
        l, keep = _cmt_lists(cmts, lists) if lists is not None else (None, None); lo = np.ascontiguousarray(list_of, dtype=np.int32) if list_of is not None else None; assert lo is None or lo.shape == (n,)
        ok = (ctypes.c_ubyte * max(1, n))(); size = ctypes.c_longlong(-7); self.L.verifyBlockFull.restype = ctypes.c_int
        rc = self.L.verifyBlockFull(ptr, n, ctypes.byref(l) if l is not None else None, lo.ctypes.data_as(ctypes.c_void_p) if lo is not None and n else None, ctypes.c_void_p(s) if s else None, int(bool(commit)), ok, ctypes.byref(size))
        return rc, [bool(ok[i]) for i in range(n)], (None if size.value == -7 else int(size.value))
    # include/zk_spent_pk.h: two keys a record, a deposit's one-time pk address included
    def SnSetSpendPairs(self, s, sns, pks=None, commit=True):
        """pks: None, or one entry a record: 32 bytes with the address at [12:], or None / 32 zero bytes = no second key -> (the size after the call or -1, [spent?])"""
        n = len(sns); buf = b"".join(bytes(x) for x in sns); pb = b"".join(bytes(x) if x is not None else bytes(32) for x in pks) if pks is not None else None; assert pb is None or len(pb) == 32 * n
        out = ctypes.create_string_buffer(max(1, n)); self.L.zkSnSetSpendPairs.restype = ctypes.c_longlong
        size = int(self.L.zkSnSetSpendPairs(ctypes.c_void_p(s) if s else None, buf, pb, n, int(bool(commit)), out)); return size, [bool(b) for b in out.raw[:n]]
    def VerifyBlockState(self, cache, items, cmts, lists, list_of, s, commit):
        """VerifyBlockFullCached (cache None: VerifyBlockFull) with a deposit's pk address as its second key -> (accepted, [bool], size after or None)"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs, ptr, n = _recs(recs)
        l, keep = _cmt_lists(cmts, lists) if lists is not None else (None, None); lo = np.ascontiguousarray(list_of, dtype=np.int32) if list_of is not None else None; assert lo is None or lo.shape == (n,)
        ok = (ctypes.c_ubyte * max(1, n))(); size = ctypes.c_longlong(-7); self.L.verifyBlockState.restype = ctypes.c_int
        rc = self.L.verifyBlockState(_cache_handle(cache), ptr, n, ctypes.byref(l) if l is not None else None, lo.ctypes.data_as(ctypes.c_void_p) if lo is not None and n else None, ctypes.c_void_p(s) if s else None,
                                     int(bool(commit)), ok, ctypes.byref(size))
        return rc, [bool(ok[i]) for i in range(n)], (None if size.value == -7 else int(size.value))
    # include/zk_proof_cache.h: the proofs the pool has verified are not verified again with their block.  cache: a ProofCache, a handle of ProofCacheNew, or None
    def ProofCacheNew(self, capacity):
        self.L.zkProofCacheNew.restype = ctypes.c_void_p; return self.L.zkProofCacheNew(ctypes.c_longlong(capacity))   # None on failure
    def ProofCacheFree(self, c): self.L.zkProofCacheFree(_cache_handle(c))
    def ProofCacheClear(self, c): return int(self.L.zkProofCacheClear(_cache_handle(c)))
    def ProofCacheStats(self, c):
        """-> (hits, misses, records stored, entries held now), None on failure"""
        out = (ctypes.c_uint64 * 4)(); return tuple(int(x) for x in out) if self.L.zkProofCacheStats(_cache_handle(c), out) == 0 else None
    def VerifyRecordsCached(self, cache, items):
        """VerifyBlockRecords with the proof step behind the cache -> (accepted, [bool])"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs, ptr, n = _recs(recs)
        ok = (ctypes.c_ubyte * max(1, n))(); self.L.verifyRecordsCached.restype = ctypes.c_int; rc = self.L.verifyRecordsCached(_cache_handle(cache), ptr, n, ok); return rc, [bool(ok[i]) for i in range(n)]
    def VerifyBlockFullCached(self, cache, items, cmts, lists, list_of, s, commit):
        """VerifyBlockFull with the proof step behind the cache -> (accepted, [bool], size after or None)"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs, ptr, n = _recs(recs)
        l, keep = _cmt_lists(cmts, lists) if lists is not None else (None, None); lo = np.ascontiguousarray(list_of, dtype=np.int32) if list_of is not None else None; assert lo is None or lo.shape == (n,)
        ok = (ctypes.c_ubyte * max(1, n))(); size = ctypes.c_longlong(-7); self.L.verifyBlockFullCached.restype = ctypes.c_int
        rc = self.L.verifyBlockFullCached(_cache_handle(cache), ptr, n, ctypes.byref(l) if l is not None else None, lo.ctypes.data_as(ctypes.c_void_p) if lo is not None and n else None, ctypes.c_void_p(s) if s else None,
                                          int(bool(commit)), ok, ctypes.byref(size))
        return rc, [bool(ok[i]) for i in range(n)], (None if size.value == -7 else int(size.value))
    def GenRedeemProof(self, value, value_old, sn_old, r_old, sn, r, cmtA_old, cmtA, value_s, sk):
        return self.L.genRedeemproof(ctypes.c_uint64(value), ctypes.c_uint64(value_old), self.hx(sn_old), self.hx(r_old), self.hx(sn), self.hx(r), self.hx(cmtA_old), self.hx(cmtA), ctypes.c_uint64(value_s), self.hx(sk)).decode()
    def VerifyRedeemProof(self, proof, cmtA_old, sn_old, cmtA, value_s): return bool(self.L.verifyRedeemproof(proof.encode(), self.hx(cmtA_old), self.hx(sn_old), self.hx(cmtA), ctypes.c_uint64(value_s)))
    # include/zk_tree.h: the resident commitment tree at the drop-in level (hex strings as zktx.go marshals them)
    def TreeNew(self, depth):
        t = self.L.zkTreeNew(int(depth))
        if not t: raise ZkGpuError(lib().zkgpu_last_error().decode())
        return t
    def TreeFree(self, t): self.L.zkTreeFree(ctypes.c_void_p(t))
    def TreeAppend(self, t, cmts):
        """-> the new number of leaves, -1 on failure"""
        return int(self.L.zkTreeAppend(ctypes.c_void_p(t), b"".join(self.hx(c) for c in cmts), len(cmts)))
    def TreeRoot(self, t): return bytes.fromhex(self.L.zkTreeRoot(ctypes.c_void_p(t)).decode())
    def GenDepositProofTree(self, value, value_old, sn_old, r_old, sn, r, sns, rs, cmtB_old, cmtB, value_s, pk, sn_A_old, cmtS, sk, t):
        """-> (proof hex, root the proof was made against as big-endian bytes, or None on failure)"""
        rt = ctypes.create_string_buffer(65)
        p = self.L.genDepositproofTree(ctypes.c_uint64(value), ctypes.c_uint64(value_old), self.hx(sn_old), self.hx(r_old), self.hx(sn), self.hx(r), self.hx(sns), self.hx(rs), self.hx(cmtB_old), self.hx(cmtB), ctypes.c_uint64(value_s),
                                       self.hx(pk), self.hx(sn_A_old), self.hx(cmtS), self.hx(sk), ctypes.c_void_p(t) if t else None, rt).decode()
        return p, (bytes.fromhex(rt.value.decode()) if rt.value else None)
    # include/zk_tree_states.h: the tree at past sizes, and its rewind
    def TreeRootAt(self, t, size):
        """-> the root of the first `size` leaves as big-endian bytes, None on failure"""
        r = self.L.zkTreeRootAt(ctypes.c_void_p(t) if t else None, ctypes.c_longlong(size)); return bytes.fromhex(r.decode()) if r else None
    def TreeRootsAt(self, t, sizes, out=None):
        """-> [root as big-endian bytes], None on failure; out: a (q, 32) uint8 array to write into instead (then the return value is 0 / -1)"""
        m = np.ascontiguousarray(sizes, dtype=np.int64).reshape(-1); q = int(m.size); buf = out if out is not None else np.zeros((max(1, q), 32), dtype=np.uint8)
        rc = int(self.L.zkTreeRootsAt(ctypes.c_void_p(t) if t else None, m.ctypes.data_as(ctypes.c_void_p) if q else None, q, _bytes(buf)))
        if out is not None: return rc
        return [buf[i].tobytes() for i in range(q)] if rc == 0 else None
    def TreeRewind(self, t, size):
        """-> the new number of leaves, -1 on failure"""
        return int(self.L.zkTreeRewind(ctypes.c_void_p(t) if t else None, ctypes.c_longlong(size)))
    def GenDepositProofTreeAt(self, value, value_old, sn_old, r_old, sn, r, sns, rs, cmtB_old, cmtB, value_s, pk, sn_A_old, cmtS, sk, t, size):
        """GenDepositProofTree against the first `size` leaves -> (proof hex, root the proof was made against as big-endian bytes, or None on failure)"""
        rt = ctypes.create_string_buffer(65)
        p = self.L.genDepositproofTreeAt(ctypes.c_uint64(value), ctypes.c_uint64(value_old), self.hx(sn_old), self.hx(r_old), self.hx(sn), self.hx(r), self.hx(sns), self.hx(rs), self.hx(cmtB_old), self.hx(cmtB), ctypes.c_uint64(value_s),
                                         self.hx(pk), self.hx(sn_A_old), self.hx(cmtS), self.hx(sk), ctypes.c_void_p(t) if t else None, ctypes.c_longlong(size), rt).decode()
        return p, (bytes.fromhex(rt.value.decode()) if rt.value else None)
    # include/zk_tree_block.h: a block decided against the resident tree
    def VerifyBlockTree(self, cache, items, tree, anchors, s, commit):
        """tree: a handle of TreeNew or None; anchors: tree sizes -> (accepted, [bool], [anchor_of], set size after or None, tree size after or None)"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs, ptr, n = _recs(recs)
        an = np.ascontiguousarray(anchors if anchors is not None else [], dtype=np.int64).reshape(-1); na = int(an.size)
        ok = (ctypes.c_ubyte * max(1, n))(); of = (ctypes.c_int32 * max(1, n))(*([-7] * max(1, n))); size = ctypes.c_longlong(-7); tsize = ctypes.c_longlong(-7); self.L.verifyBlockTree.restype = ctypes.c_int
        rc = self.L.verifyBlockTree(_cache_handle(cache), ptr, n, ctypes.c_void_p(tree) if tree else None, an.ctypes.data_as(ctypes.c_void_p) if na else None, na, ctypes.c_void_p(s) if s else None,
                                    int(bool(commit)), ok, of, ctypes.byref(size), ctypes.byref(tsize))
        return rc, [bool(ok[i]) for i in range(n)], [int(of[i]) for i in range(n)], (None if size.value == -7 else int(size.value)), (None if tsize.value < 0 else int(tsize.value))   # (no tree: the call writes -1)
    # include/zk_tree_chain.h: a stretch of the chain decided against the resident tree
    def VerifyChainTree(self, cache, items, block_first, tree, prior_anchors, window, s):
        """block_first: n_blocks + 1 record indices; tree: a handle of TreeNew; prior_anchors: tree sizes; s: a set's handle or None
        -> (blocks accepted or -1, [bool], [anchor_of], [set size after block b] or None, [tree size after block b] or None)"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs, ptr, n = _recs(recs)
        bf = np.ascontiguousarray(block_first, dtype=np.int32).reshape(-1); nb = int(bf.size) - 1; pa = np.ascontiguousarray(prior_anchors if prior_anchors is not None else [], dtype=np.int64).reshape(-1); npa = int(pa.size)
        ok = (ctypes.c_ubyte * max(1, n))(); of = (ctypes.c_int32 * max(1, n))(*([-7] * max(1, n))); ss = np.full(max(1, nb), -7, dtype=np.int64); ts = np.full(max(1, nb), -7, dtype=np.int64); self.L.verifyChainTree.restype = ctypes.c_int
        rc = self.L.verifyChainTree(_cache_handle(cache), ptr, n, bf.ctypes.data_as(ctypes.c_void_p) if nb >= 0 else None, nb, ctypes.c_void_p(tree) if tree else None, pa.ctypes.data_as(ctypes.c_void_p) if npa else None, npa,
                                    int(window), ctypes.c_void_p(s) if s else None, ok, of, ss.ctypes.data_as(ctypes.c_void_p), ts.ctypes.data_as(ctypes.c_void_p))
        return (rc, [bool(ok[i]) for i in range(n)], [int(of[i]) for i in range(n)], ([int(x) for x in ss[:nb]] if rc >= 0 and s else None), ([int(x) for x in ts[:nb]] if rc >= 0 else None))
    # include/zk_accounts.h: the resident account table at the drop-in level, and a block decided with it.  a: a handle of AcctsNew or an AccountTable
    def AcctsNew(self): self.L.zkAcctsNew.restype = ctypes.c_void_p; return self.L.zkAcctsNew()   # None on failure
    def AcctsFree(self, a): self.L.zkAcctsFree(_accts_handle(a))
    def AcctsSize(self, a): self.L.zkAcctsSize.restype = ctypes.c_longlong; return int(self.L.zkAcctsSize(_accts_handle(a)))
    def AcctsSet(self, a, addrs, values):
        ab, n = _keys20(addrs); vb, nv = _vals32(values); assert n == nv; return int(self.L.zkAcctsSet(_accts_handle(a), ab, vb, n))
    def AcctsGet(self, a, addrs, at_size=-1):
        """-> [32-byte value], None on failure"""
        ab, n = _keys20(addrs); out = ctypes.create_string_buffer(max(1, 32 * n)); rc = self.L.zkAcctsGet(_accts_handle(a), ab, n, ctypes.c_longlong(at_size), out)
        return [out.raw[32 * i:32 * i + 32] for i in range(n)] if rc == 0 else None
    def AcctsRewind(self, a, size): return int(self.L.zkAcctsRewind(_accts_handle(a), ctypes.c_longlong(size)))
    def AcctsFillRecords(self, a, froms, items, chained):
        """-> (0 / -1, a copy of the records with their old slots filled)"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs = np.array(recs, dtype=RECORD_DTYPE, copy=True); n = int(recs.shape[0]); fb, nf = _keys20(froms); assert nf == n
        rc = int(self.L.zkAcctsFillRecords(_accts_handle(a), fb if n else None, recs.ctypes.data_as(ctypes.c_void_p), n, int(bool(chained)))); return rc, recs
    def VerifyBlockAccounts(self, cache, items, froms, a, tree, anchors, s, commit):
        """-> (leading accepted records or -1, [bool], [anchor_of], the records as they were verified, table size after or None, set size after or None, tree size after or None)"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs = np.array(recs, dtype=RECORD_DTYPE, copy=True); n = int(recs.shape[0]); fb, nf = _keys20(froms); assert nf == n
        an = np.ascontiguousarray(anchors if anchors is not None else [], dtype=np.int64).reshape(-1); na = int(an.size)
        ok = (ctypes.c_ubyte * max(1, n))(); of = (ctypes.c_int32 * max(1, n))(*([-7] * max(1, n))); asize = ctypes.c_longlong(-7); size = ctypes.c_longlong(-7); tsize = ctypes.c_longlong(-7)
        self.L.verifyBlockAccounts.restype = ctypes.c_int
        rc = self.L.verifyBlockAccounts(_cache_handle(cache), recs.ctypes.data_as(ctypes.c_void_p), fb if n else None, n, _accts_handle(a), ctypes.c_void_p(tree) if tree else None,
                                        an.ctypes.data_as(ctypes.c_void_p) if na else None, na, ctypes.c_void_p(s) if s else None, int(bool(commit)), ok, of, ctypes.byref(asize), ctypes.byref(size), ctypes.byref(tsize))
        return (rc, [bool(ok[i]) for i in range(n)], [int(of[i]) for i in range(n)], recs, (None if asize.value == -7 else int(asize.value)), (None if size.value == -7 else int(size.value)),
                (None if tsize.value < 0 else int(tsize.value)))
    # include/zk_accounts_chain.h: a stretch of the chain decided against the resident account table, tree and set
    def VerifyChainAccounts(self, cache, items, froms, block_first, a, tree, prior_anchors, window, s):
        """-> (blocks accepted or -1, [bool], [anchor_of], the records with the segment-wide chained fill, [table size after block b] or None, [set size after block b]
        or None, [tree size after block b] or None)"""
        recs = items if isinstance(items, np.ndarray) else records_from_items(items); recs = np.array(recs, dtype=RECORD_DTYPE, copy=True); n = int(recs.shape[0]); fb, nf = _keys20(froms); assert nf == n
        bf = np.ascontiguousarray(block_first, dtype=np.int32).reshape(-1); nb = int(bf.size) - 1; pa = np.ascontiguousarray(prior_anchors if prior_anchors is not None else [], dtype=np.int64).reshape(-1); npa = int(pa.size)
        ok = (ctypes.c_ubyte * max(1, n))(); of = (ctypes.c_int32 * max(1, n))(*([-7] * max(1, n))); sizes = [np.full(max(1, nb), -7, dtype=np.int64) for _ in range(3)]; self.L.verifyChainAccounts.restype = ctypes.c_int
        rc = self.L.verifyChainAccounts(_cache_handle(cache), recs.ctypes.data_as(ctypes.c_void_p), fb if n else None, n, bf.ctypes.data_as(ctypes.c_void_p) if nb >= 0 else None, nb, _accts_handle(a),
                                        ctypes.c_void_p(tree) if tree else None, pa.ctypes.data_as(ctypes.c_void_p) if npa else None, npa, int(window), ctypes.c_void_p(s) if s else None, ok, of,
                                        *[x.ctypes.data_as(ctypes.c_void_p) for x in sizes])
        out = [[int(x) for x in v[:nb]] if rc >= 0 else None for v in sizes]
        return (rc, [bool(ok[i]) for i in range(n)], [int(of[i]) for i in range(n)], recs, out[0], (out[1] if s else None), out[2])
    # include/zk_senders.h: the senders of n transactions from their signatures, on the device
    def RecoverSenders(self, hashes, sigs, homestead=True, want_pubs=True):
        """hashes: n x 32 bytes; sigs: n x 65 bytes (R || S || V).  -> (froms: [20 bytes], pubs: [64 bytes] or None, ok: [bool]); raises ZkGpuError where the call
        returns -1"""
        hb = np.frombuffer(b"".join(bytes(h) for h in hashes), dtype=np.uint8).reshape(-1, 32).copy(); sb = np.frombuffer(b"".join(bytes(x) for x in sigs), dtype=np.uint8).reshape(-1, 65).copy()
        n = int(hb.shape[0]); assert sb.shape[0] == n; froms = np.zeros((max(1, n), 20), dtype=np.uint8); pubs = np.zeros((max(1, n), 64), dtype=np.uint8) if want_pubs else None; ok = np.zeros(max(1, n), dtype=np.uint8)
        self.L.zkRecoverSenders.restype = ctypes.c_int
        rc = int(self.L.zkRecoverSenders(_bytes(hb), _bytes(sb), n, int(bool(homestead)), _bytes(froms), _bytes(pubs) if want_pubs else None, _bytes(ok)))
        if rc < 0: raise ZkGpuError("zkRecoverSenders: %s" % self.L.zkgpu_last_error().decode())
        assert rc == int(ok[:n].sum())
        return [bytes(froms[i]) for i in range(n)], ([bytes(pubs[i]) for i in range(n)] if want_pubs else None), [bool(ok[i]) for i in range(n)]
    # include/zk_txs.h: the recovery's inputs, or the senders themselves, from the raw transactions of a block body
    def TxSigningInputs(self, txs, signer, chain_id):
        """txs: n byte strings, one RLP transaction each.  -> (txhash: [32 bytes], sighash: [32 bytes], sigs: [65 bytes], deposit_from: [20 bytes], code: [int], status: [int]);
        raises ZkGpuError where the call returns -1"""
        n = len(txs); blob, off = _tx_blob(txs); o = [np.zeros((max(1, n), w), dtype=np.uint8) for w in (32, 32, 65, 20, 1, 1)]
        self.L.zkTxSigningInputs.restype = ctypes.c_int
        rc = int(self.L.zkTxSigningInputs(_bytes(blob), _u64p(off), n, int(signer), ctypes.c_uint64(chain_id), *[_bytes(a) for a in o]))
        if rc < 0: raise ZkGpuError("zkTxSigningInputs: %s" % self.L.zkgpu_last_error().decode())
        assert rc == int((o[5][:n, 0] == TX_OK).sum())
        return tuple([bytes(a[i]) for i in range(n)] for a in o[:4]) + tuple([int(a[i, 0]) for i in range(n)] for a in o[4:])
    def TxSenders(self, txs, signer, chain_id, want_txhash=True):
        """-> (froms: [20 bytes], txhash: [32 bytes] or None, code: [int], status: [int]); froms goes into VerifyChainAccounts as it is.  Raises ZkGpuError where the call
        returns -1"""
        n = len(txs); blob, off = _tx_blob(txs); th, fr, code, st = [np.zeros((max(1, n), w), dtype=np.uint8) for w in (32, 20, 1, 1)]
        self.L.zkTxSenders.restype = ctypes.c_int
        rc = int(self.L.zkTxSenders(_bytes(blob), _u64p(off), n, int(signer), ctypes.c_uint64(chain_id), _bytes(th) if want_txhash else None, _bytes(fr), _bytes(code), _bytes(st)))
        if rc < 0: raise ZkGpuError("zkTxSenders: %s" % self.L.zkgpu_last_error().decode())
        assert rc == int((st[:n, 0] == TX_OK).sum())
        return [bytes(fr[i]) for i in range(n)], ([bytes(th[i]) for i in range(n)] if want_txhash else None), [int(code[i, 0]) for i in range(n)], [int(st[i, 0]) for i in range(n)]
    # include/zk_bodies.h: the records of a block body's transactions, and a stretch of the chain decided from the bodies' bytes
    def TxRecords(self, txs, signer, chain_id, want_txhash=True):
        """-> (recs: the m records as an array of RECORD_DTYPE, rec_froms: [20 bytes] x m, rec_of: [int] x n, froms: [20 bytes], txhash: [32 bytes] or None, code: [int],
        status: [int]); raises ZkGpuError where the call returns -1"""
        n = len(txs); blob, off = _tx_blob(txs); recs = np.zeros(max(1, n), dtype=RECORD_DTYPE); rf, th, fr, code, st = [np.zeros((max(1, n), w), dtype=np.uint8) for w in (20, 32, 20, 1, 1)]
        of = np.zeros(max(1, n), dtype=np.int32); self.L.zkTxRecords.restype = ctypes.c_int
        m = int(self.L.zkTxRecords(_bytes(blob), _u64p(off), n, int(signer), ctypes.c_uint64(chain_id), recs.ctypes.data_as(ctypes.c_void_p), _bytes(rf), of.ctypes.data_as(ctypes.c_void_p),
                                   _bytes(th) if want_txhash else None, _bytes(fr), _bytes(code), _bytes(st)))
        if m < 0: raise ZkGpuError("zkTxRecords: %s" % self.L.zkgpu_last_error().decode())
        return (recs[:m].copy(), [bytes(rf[j]) for j in range(m)], [int(of[i]) for i in range(n)], [bytes(fr[i]) for i in range(n)], ([bytes(th[i]) for i in range(n)] if want_txhash else None),
                [int(code[i, 0]) for i in range(n)], [int(st[i, 0]) for i in range(n)])
    def VerifyChainBodies(self, cache, txs, block_first, signer, chain_id, a, tree, prior_anchors, window, s, fill=0):
        """block_first: n_blocks + 1 TRANSACTION indices.  -> (blocks accepted or -1, dict of n_recs, recs (the m records, old slots filled), rec_froms, rec_of, froms, txhash,
        code, status, ok [bool] x m, anchor_of [int] x m, accts_sizes, set_sizes (None without a set), tree_sizes); every output array is handed in full of `fill` bytes"""
        n = len(txs); blob, off = _tx_blob(txs); bf = np.ascontiguousarray(block_first, dtype=np.int32).reshape(-1); nb = int(bf.size) - 1
        pa = np.ascontiguousarray(prior_anchors if prior_anchors is not None else [], dtype=np.int64).reshape(-1); npa = int(pa.size)
        recs = np.frombuffer(bytes([fill]) * (720 * max(1, n)), dtype=RECORD_DTYPE).copy(); rf, th, fr, code, st, ok = [np.full((max(1, n), w), fill, dtype=np.uint8) for w in (20, 32, 20, 1, 1, 1)]
        of = np.full(max(1, n), -7, dtype=np.int32); an = np.full(max(1, n), -7, dtype=np.int32); sizes = [np.full(max(1, nb), -7, dtype=np.int64) for _ in range(3)]; m = ctypes.c_int(-7)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p); self.L.verifyChainBodies.restype = ctypes.c_int
        rc = int(self.L.verifyChainBodies(_cache_handle(cache), _bytes(blob), _u64p(off), n, vp(bf) if nb >= 0 else None, nb, int(signer), ctypes.c_uint64(chain_id), _accts_handle(a),
                                          ctypes.c_void_p(tree) if tree else None, vp(pa) if npa else None, npa, int(window), ctypes.c_void_p(s) if s else None, vp(recs), vp(rf), vp(of), vp(th), vp(fr),
                                          vp(code), vp(st), vp(ok), vp(an), *[vp(x) for x in sizes], ctypes.byref(m)))
        k = max(0, int(m.value)); out = [[int(x) for x in v[:nb]] if rc >= 0 else None for v in sizes]
        return rc, dict(n_recs=int(m.value), recs=recs[:k].copy(), rec_froms=[bytes(rf[j]) for j in range(k)], rec_of=[int(of[i]) for i in range(n)], froms=[bytes(fr[i]) for i in range(n)],
                        txhash=[bytes(th[i]) for i in range(n)], code=[int(code[i, 0]) for i in range(n)], status=[int(st[i, 0]) for i in range(n)], ok=[bool(ok[j, 0]) for j in range(k)],
                        anchor_of=[int(an[j]) for j in range(k)], accts_sizes=out[0], set_sizes=(out[1] if s else None), tree_sizes=out[2],
                        raw=dict(recs=recs, rec_froms=rf, rec_of=of, txhash=th, froms=fr, code=code, status=st, ok=ok, anchor_of=an))
    # include/zk_tx_roots.h: the transaction trie roots of a segment's bodies, and the chain call that holds them against the headers' roots
    def TxRoots(self, txs, block_first):
        """-> (roots: [32 bytes] x n_blocks, defined: [bool] x n_blocks); raises ZkGpuError where the call returns -1"""
        n = len(txs); blob, off = _tx_blob(txs); bf = _first(block_first); nb = int(bf.size) - 1
        roots = np.zeros((max(1, nb), 32), dtype=np.uint8); defined = np.zeros(max(1, nb), dtype=np.uint8); self.L.zkTxRoots.restype = ctypes.c_int
        rc = int(self.L.zkTxRoots(_bytes(blob), _u64p(off), n, _i32p(bf), nb, _bytes(roots), _bytes(defined)))
        if rc < 0: raise ZkGpuError("zkTxRoots: %s" % self.L.zkgpu_last_error().decode())
        assert rc == int(defined[:nb].sum())
        return [bytes(roots[b]) for b in range(nb)], [bool(defined[b]) for b in range(nb)]
    def VerifyChainBodiesRoots(self, cache, txs, block_first, want_roots, signer, chain_id, a, tree, prior_anchors, window, s, fill=0):
        """VerifyChainBodies with want_roots: [32 bytes] x n_blocks (header.TxHash of each block).  -> (blocks accepted or -1, VerifyChainBodies' dict and roots: [32 bytes] x
        n_blocks, root_ok: [bool] x n_blocks)"""
        n = len(txs); blob, off = _tx_blob(txs); bf = _first(block_first); nb = int(bf.size) - 1
        pa = np.ascontiguousarray(prior_anchors if prior_anchors is not None else [], dtype=np.int64).reshape(-1); npa = int(pa.size)
        recs = np.frombuffer(bytes([fill]) * (720 * max(1, n)), dtype=RECORD_DTYPE).copy(); rf, th, fr, code, st, ok = [np.full((max(1, n), w), fill, dtype=np.uint8) for w in (20, 32, 20, 1, 1, 1)]
        of = np.full(max(1, n), -7, dtype=np.int32); an = np.full(max(1, n), -7, dtype=np.int32); sizes = [np.full(max(1, nb), -7, dtype=np.int64) for _ in range(3)]; m = ctypes.c_int(-7)
        want = np.frombuffer(b"".join(bytes(r) for r in want_roots) or bytes(32), dtype=np.uint8).copy(); roots = np.full((max(1, nb), 32), fill, dtype=np.uint8); rok = np.full(max(1, nb), fill, dtype=np.uint8)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p); self.L.verifyChainBodiesRoots.restype = ctypes.c_int
        rc = int(self.L.verifyChainBodiesRoots(_cache_handle(cache), _bytes(blob), _u64p(off), n, vp(bf) if nb >= 0 else None, nb, int(signer), ctypes.c_uint64(chain_id), _accts_handle(a),
                                               ctypes.c_void_p(tree) if tree else None, vp(pa) if npa else None, npa, int(window), ctypes.c_void_p(s) if s else None, vp(recs), vp(rf), vp(of), vp(th),
                                               vp(fr), vp(code), vp(st), vp(ok), vp(an), *[vp(x) for x in sizes], ctypes.byref(m), vp(want), vp(roots), vp(rok)))
        k = max(0, int(m.value)); out = [[int(x) for x in v[:nb]] if rc >= 0 else None for v in sizes]
        return rc, dict(n_recs=int(m.value), recs=recs[:k].copy(), rec_froms=[bytes(rf[j]) for j in range(k)], rec_of=[int(of[i]) for i in range(n)], froms=[bytes(fr[i]) for i in range(n)],
                        txhash=[bytes(th[i]) for i in range(n)], code=[int(code[i, 0]) for i in range(n)], status=[int(st[i, 0]) for i in range(n)], ok=[bool(ok[j, 0]) for j in range(k)],
                        anchor_of=[int(an[j]) for j in range(k)], accts_sizes=out[0], set_sizes=(out[1] if s else None), tree_sizes=out[2],
                        roots=[bytes(roots[b]) for b in range(max(0, nb))], root_ok=[bool(rok[b]) for b in range(max(0, nb))],
                        raw=dict(recs=recs, rec_froms=rf, rec_of=of, txhash=th, froms=fr, code=code, status=st, ok=ok, anchor_of=an, roots=roots, root_ok=rok))
    # include/zk_raw_bodies.h: the bodies as a peer or the database delivered them, one offset a block
    def BodySplit(self, bodies, cap=None, start=0):
        """bodies: n_blocks byte strings, rlp([[tx ...], [uncle ...]]) each.  -> (k: the leading bodies with status BODY_OK, or -2 where cap is too small, and a dict: n_txs,
        block_first: [int] x (n_blocks + 1), body_status: [int], tx_beg, tx_size: [int] x n_txs (empty with -2)); raises ZkGpuError where the call returns -1"""
        nb = len(bodies); blob, off = _body_blob(bodies, start); cap = int(off[nb] - off[0]) if cap is None else int(cap)
        tb = np.zeros(max(1, cap), dtype=np.uint64); ts = np.zeros(max(1, cap), dtype=np.uint32); bf = np.zeros(nb + 1, dtype=np.int32); st = np.zeros(max(1, nb), dtype=np.uint8); n = ctypes.c_int(0)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p); self.L.zkBodySplit.restype = ctypes.c_int
        k = int(self.L.zkBodySplit(_bytes(blob), _u64p(off), nb, cap, vp(tb), vp(ts), vp(bf), vp(st), ctypes.byref(n)))
        if k == -1: raise ZkGpuError("zkBodySplit: %s" % self.L.zkgpu_last_error().decode())
        m = int(n.value) if k >= 0 else 0
        return k, dict(n_txs=int(n.value), block_first=[int(x) for x in bf], body_status=[int(x) for x in st[:nb]], tx_beg=[int(x) for x in tb[:m]], tx_size=[int(x) for x in ts[:m]])
    def VerifyChainRawBodies(self, cache, bodies, want_roots, signer, chain_id, a, tree, prior_anchors, window, s, cap=None, fill=0, start=0):
        """VerifyChainBodiesRoots on the bodies' bytes: no txs, no block_first.  -> (blocks accepted, -1 or -2, VerifyChainBodiesRoots' dict over the n_txs transactions
        the split found, and n_txs, block_first, body_status, tx_beg, tx_size); cap None: room for one transaction a byte"""
        nb = len(bodies); blob, off = _body_blob(bodies, start); cap = int(off[nb] - off[0]) if cap is None else int(cap); c1 = max(1, cap)
        pa = np.ascontiguousarray(prior_anchors if prior_anchors is not None else [], dtype=np.int64).reshape(-1); npa = int(pa.size)
        recs = np.frombuffer(bytes([fill]) * (720 * c1), dtype=RECORD_DTYPE).copy(); rf, th, fr, code, st, ok = [np.full((c1, w), fill, dtype=np.uint8) for w in (20, 32, 20, 1, 1, 1)]
        of = np.full(c1, -7, dtype=np.int32); an = np.full(c1, -7, dtype=np.int32); sizes = [np.full(max(1, nb), -7, dtype=np.int64) for _ in range(3)]; m = ctypes.c_int(-7)
        want = np.frombuffer(b"".join(bytes(r) for r in want_roots) or bytes(32), dtype=np.uint8).copy(); roots = np.full((max(1, nb), 32), fill, dtype=np.uint8); rok = np.full(max(1, nb), fill, dtype=np.uint8)
        tb = np.frombuffer(bytes([fill]) * (8 * c1), dtype=np.uint64).copy(); ts = np.frombuffer(bytes([fill]) * (4 * c1), dtype=np.uint32).copy(); bf = np.frombuffer(bytes([fill]) * (4 * (nb + 1)), dtype=np.int32).copy()
        bs = np.full(max(1, nb), fill, dtype=np.uint8); nt = ctypes.c_int(-7)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p); self.L.verifyChainRawBodies.restype = ctypes.c_int
        rc = int(self.L.verifyChainRawBodies(_cache_handle(cache), _bytes(blob), _u64p(off), nb, cap, int(signer), ctypes.c_uint64(chain_id), _accts_handle(a), ctypes.c_void_p(tree) if tree else None,
                                             vp(pa) if npa else None, npa, int(window), ctypes.c_void_p(s) if s else None, vp(recs), vp(rf), vp(of), vp(th), vp(fr), vp(code), vp(st), vp(ok), vp(an),
                                             *[vp(x) for x in sizes], ctypes.byref(m), vp(want), vp(roots), vp(rok), vp(tb), vp(ts), vp(bf), vp(bs), ctypes.byref(nt)))
        n = max(0, int(nt.value)) if rc >= 0 else 0; k = max(0, int(m.value)); out = [[int(x) for x in v[:nb]] if rc >= 0 else None for v in sizes]
        return rc, dict(n_recs=int(m.value), recs=recs[:k].copy(), rec_froms=[bytes(rf[j]) for j in range(k)], rec_of=[int(of[i]) for i in range(n)], froms=[bytes(fr[i]) for i in range(n)],
                        txhash=[bytes(th[i]) for i in range(n)], code=[int(code[i, 0]) for i in range(n)], status=[int(st[i, 0]) for i in range(n)], ok=[bool(ok[j, 0]) for j in range(k)],
                        anchor_of=[int(an[j]) for j in range(k)], accts_sizes=out[0], set_sizes=(out[1] if s else None), tree_sizes=out[2],
                        roots=[bytes(roots[b]) for b in range(nb)], root_ok=[bool(rok[b]) for b in range(nb)], n_txs=int(nt.value), block_first=[int(x) for x in bf],
                        body_status=[int(x) for x in bs[:nb]], tx_beg=[int(x) for x in tb[:n]], tx_size=[int(x) for x in ts[:n]],
                        raw=dict(recs=recs, rec_froms=rf, rec_of=of, txhash=th, froms=fr, code=code, status=st, ok=ok, anchor_of=an, roots=roots, root_ok=rok, tx_beg=tb, tx_size=ts, block_first=bf,
                                 body_status=bs))
    # include/zk_headers.h: a batch of headers decided from their bytes; tx_root goes into VerifyChainBodiesRoots as want_roots
    def Headers(self, hdrs, period, epoch, now, parent):
        """hdrs: n byte strings, one RLP header each; parent: None or (hash, number, time) of the parent of header 0.  -> (k, the leading headers with status HDR_OK, and a
        dict: hash, sealhash, signer, coinbase, tx_root, rtcmt: [bytes]; number, time, difficulty, vote, extra_beg, extra_size, cmt_beg, cmt_count, status: [int]); raises
        ZkGpuError where the call returns -1"""
        self.L.zkHeaders.restype = ctypes.c_int; k, o = _headers_call(self.L.zkHeaders, hdrs, period, epoch, now, parent, 0)
        if k < 0: raise ZkGpuError("zkHeaders: %s" % self.L.zkgpu_last_error().decode())
        return k, {name: ([bytes(r) for r in o[name]] if w else [int(x) for x in o[name]]) for name, w, _ in HEADER_OUTPUTS}
    def VerifyDepositProofDepth(self, depth, proof, RT, pk, cmtb_old, sn_old, cmtb, sns):
        return bool(self.L.verifyDepositproofDepth(int(depth), proof.encode(), self.hx(RT), self.hx(pk), self.hx(cmtb_old), self.hx(sn_old), self.hx(cmtb), self.hx(sns)))
