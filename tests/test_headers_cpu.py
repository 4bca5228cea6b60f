"""Headers from their bytes without a device (include/zk_headers.h): the Python model (tests/header_model.py) against the pins that do not come from our
own reading of the reference (tests/golden/header_vectors.txt: the header inside blockEnc of core/types/block_test.go with the hash that test records, and the empty
uncle hash), every case of tests/header_corpus.py held to the status it claims, the header file, the exports, and the entry in a process that sees no device."""
import os, random, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import header_corpus as c
import header_model as hm
import tx_model as t

def recorded():
    """-> (the recorded header as a 17-field dict: RTCMT and a CMT list appended to the 15 recorded fields; the recorded hash; the recorded uncle hash)"""
    v = {}
    for l in open(os.path.join(ROOT, "tests", "golden", "header_vectors.txt")):
        if not l.startswith("#"): k, x = l.split(); v[k] = b"" if x == "-" else bytes.fromhex(x)
    h = {name: (int.from_bytes(v[name], "big") if kind in ("big", "u64") else v[name]) for name, kind in hm.FIELDS[:hm.SEAL_FIELDS]}
    rng = random.Random(88); h["RTCMT"] = rng.randbytes(32); h["CMT"] = [rng.randbytes(32) for _ in range(3)]
    return h, v["hash"], v["uncle_hash"]

def test_pin_seal_hash_relists_the_upstream_fifteen_fields():
    """pin 1: with nothing cut, sigHash of the 17-field header is the recorded hash of the 15-field one — the re-listing of fields 0 .. 14 leaves RTCMT and CMT out"""
    h, want, _ = recorded(); assert want.hex() == "0a5843ac1cb04865017cb35a57b50b07084e5fcee39b5acadade33149f4fff9e"
    raw15 = t.enc_list(hm.encode_items(h, 15)); assert len(raw15) == 508 and t.keccak256(raw15) == want      # the recorded bytes themselves
    assert hm.seal_hash(h, cut=0) == want
    got, spans, contents = hm.decode(hm.encode(h)); assert got == h and len(spans) == 17

def test_pin_seal_hash_cuts_the_seal_and_header_hash_covers_all_seventeen():
    """pin 2: 65 bytes appended to Extra and cut again give the recorded hash; Header.Hash() of the 17-field header is another value"""
    h, want, _ = recorded(); sealed = dict(h, Extra=h["Extra"] + random.Random(89).randbytes(65))
    assert hm.seal_hash(sealed) == want and hm.seal_hash(sealed, cut=65) == want
    assert hm.header_hash(h) != want and hm.header_hash(sealed) != want and hm.header_hash(h) == t.keccak256(hm.encode(h))
    o = hm.headers([hm.encode(sealed)], 0, 0, 2**63, None)[0]; assert o["sealhash"] == want and o["hash"] == hm.header_hash(sealed) and o["status"] == hm.VOTE   # (a PoW nonce)

def test_pin_uncle_hash():
    h, _, uncle = recorded()
    assert uncle.hex() == "1dcc4de8dec75d7aab85b567b6ccd41ad312451b948a7413f0a142fd40d49347" and hm.UNCLE_HASH_EMPTY == uncle == h["UncleHash"]

def test_p_minus_n_is_the_header_files_constant():
    assert hm.P_MINUS_N == 0x14551231950b75fc4402da1722fc9baee
    assert "0x14551231950b75fc4402da1722fc9baee" in open(os.path.join(ROOT, "include", "zk_headers.h")).read()

@pytest.fixture(scope="module")
def corpus(): return c.cases()

def test_every_case_has_the_status_it_claims_and_every_status_is_there(corpus):
    seen = {}; labels = [x[0] for x in corpus]; assert len(set(labels)) == len(labels) >= 130
    for label, claim, raw, parent, key in corpus:
        o = hm.headers([raw], c.PERIOD, c.EPOCH, c.NOW, parent)[0]; seen[o["status"]] = seen.get(o["status"], 0) + 1
        if claim is not None: assert o["status"] == claim, (label, hm.STATUS_NAMES[o["status"]])
        if claim == hm.MALFORMED:
            with pytest.raises(t.Malformed): hm.decode(raw)
            assert o == hm.ZERO
        else:
            h = hm.decode(raw)[0]; assert o["hash"] == t.keccak256(raw) and (o["sealhash"] != bytes(32)) == (len(h["Extra"]) >= 65)
        if key is not None: assert o["signer"] == hm.signer_address(key), label
        elif o["status"] != hm.OK: assert o["signer"] == bytes(20), label
    assert sorted(seen) == list(range(17)), seen                                                  # every status of zk_headers.h, at least once
    assert seen[hm.MALFORMED] >= 55 and seen[hm.SEAL] >= 20 and seen[hm.SEAL_UNDECIDED] == 4 and seen[hm.OK] >= 15

def test_corpus_covers_what_the_issue_lists(corpus):
    by = {x[0]: x for x in corpus}
    for k in (0, 1, 2, 7, 8, 1986): assert hm.headers([by["CMT of %d" % k][2]], c.PERIOD, c.EPOCH, c.NOW, by["CMT of %d" % k][3])[0]["cmt_count"] == k
    assert by["CMT of 1986"][2][0] == 0xFA                                                          # the outer list's length needs three bytes
    for k, size in ((0, 32), (1, 52), (12, 272)):
        h = hm.decode(by["checkpoint, %d signers" % k][2])[0]; assert len(h["Extra"]) - 65 == size and h["Number"] == 30000
    for k in (55, 56, 255, 256): assert len(hm.decode(by["extra signers: Extra' of %d" % k][2])[0]["Extra"]) == k + 65
    o = hm.headers([by["parent.Time + period wraps"][2]], c.PERIOD, c.EPOCH, c.NOW, by["parent.Time + period wraps"][3])[0]; assert o["status"] == hm.OK
    assert by["parent.Time + period wraps"][3][2] + c.PERIOD > o["time"]                            # refused without the wrap
    assert hm.headers([by["genesis, no parent"][2]], c.PERIOD, c.EPOCH, c.NOW, None)[0] == dict(hm.headers([by["genesis, no parent"][2]], c.PERIOD, c.EPOCH, c.NOW, (bytes(32), 7, 7))[0])

def test_chains_are_accepted_and_no_random_case_is_undecided():
    """the chains the device tests run: every header OK with the signer that sealed it; the model alone gives no SEAL_UNDECIDED on the chosen seeds"""
    for seed, n, first in ((c.CHAIN_SEED, 40, 1), (c.GENESIS_SEED, 12, 0)):
        raws, parent, signers = c.chain(seed, n, first=first); outs = hm.headers(raws, c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent)
        assert hm.accepted(outs) == n and [o["signer"] for o in outs] == signers and all(o["status"] != hm.SEAL_UNDECIDED for o in outs)
        assert any(o["number"] % c.CHAIN_EPOCH == 0 for o in outs) and {o["vote"] for o in outs} == {0, 1}
        cut = hm.headers(raws[:5] + raws[6:], c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent); assert hm.accepted(cut) == 5 and cut[5]["status"] == hm.ANCESTOR and cut[6]["status"] == hm.OK
        bad = hm.headers(raws[:3] + [b"\xc0"] + raws[3:], c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent); assert [o["status"] for o in bad[2:6]] == [hm.OK, hm.MALFORMED, hm.ANCESTOR, hm.OK]
    # the device tests' longest chain, without the curve arithmetic of 257 recoveries: only a recovery byte of 2 or 3 can be undecided (seal_recover), and a seal made by
    # sign has 0 or 1 there
    raws, parent, signers = c.chain(c.CHAIN_SEED, 257); assert all(hm.decode(r)[0]["Extra"][-1] in (0, 1) for r in raws)
    for x in (b"\x02", b"\x03"): assert hm.seal_recover(bytes(32), bytes(31) + b"\x01" + bytes(31) + b"\x01" + x)[0] == hm.SEAL_UNDECIDED

def test_only_the_crafted_cases_are_undecided(corpus):
    for label, claim, raw, parent, key in corpus:
        if hm.headers([raw], c.PERIOD, c.EPOCH, c.NOW, parent)[0]["status"] == hm.SEAL_UNDECIDED: assert claim == hm.SEAL_UNDECIDED and label.startswith("recovery id"), label

# ---- the header file and the exports ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

def test_headers_symbols_exported_by_libzkgpu_only(e):
    from test_abi_exports import SYMS, declared_symbols
    from test_tree_block_cpu import defined
    L = e.lib(); have = defined(e.LIB_PATH)
    for s in ("zkHeaders", "zkgpu_headers"): getattr(L, s); assert s in have, s
    assert sorted(set(declared_symbols("zk_headers.h")) - {"uint8_t"}) == ["zkHeaders"]            # ("uint8_t (*hash)[32]" reads as a call to the helper)
    assert "zkgpu_headers" in declared_symbols("zkgpu.h")
    for lib, syms in SYMS.items():                                                                 # the four thin libraries: unchanged
        assert defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)) == sorted(syms), lib
    src = open(os.path.join(ROOT, "include", "zk_headers.h")).read()
    for k, name in enumerate(hm.STATUS_NAMES): assert "ZK_HDR_%s = %d" % (name, k) in src and getattr(e, "HDR_" + name) == k == getattr(hm, name)

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")])
def test_headers_header_compiles_as_c_and_cxx_when_included_twice(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_headers.h"\n#include "zk_headers.h"\n#include "zk_tx_roots.h"\n'
                   'int main(void) { const uint8_t hd[1] = {0xc0}; const uint64_t off[2] = {0, 1}; uint8_t h[1][32], sh[1][32], sg[1][20], cb[1][20], tr[1][32], rt[1][32], d[1], v[1], st[1];\n'
                   '  uint64_t num[1], tm[1]; uint32_t xb[1], xs[1], kb[1], kc[1];\n'
                   '  return zkHeaders(hd, off, 1, 15, 0, 1, 0, 0, 0, 0, h, sh, sg, cb, tr, rt, num, tm, d, v, xb, xs, kb, kc, st) == -1 && ZK_HDR_OK == 0 && ZK_HDR_SEAL_UNDECIDED == 16 ? 0 : 1; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

NO_DEVICE = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from blockmaze_amd import engine as e
L = e.lib(); assert e.device_count() == 0
NO_DEVICE, ARG = -1, -2
hdrs = [b"\xc0", b"\xc1\x80"]; parent = (bytes(32), 4, 1000)
zeroed = lambda o: not any(a.any() for a in o.values())
rc, o = e.headers(hdrs, 15, 0, 2000, parent); assert rc == NO_DEVICE and b"no HIP device" in L.zkgpu_last_error() and zeroed(o) and len(o) == 15   # the wrapper hands 0xA5 in
rc, o = e.headers(hdrs, 15, 0, 2000, None); assert rc == NO_DEVICE and zeroed(o)                   # no parent: parent_hash may be NULL
assert e.headers([], 15, 0, 2000, None)[0] == 0                                                    # n = 0 returns 0 and asks for no device
# bad arguments win over the missing device
u64 = ctypes.c_uint64; ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p); off = np.array([0, 1, 3], dtype=np.uint64); dec = np.array([0, 2, 1], dtype=np.uint64); blob = np.full(3, 0xC0, dtype=np.uint8)
sizes = [64, 64, 40, 40, 64, 64, 16, 16, 2, 2, 8, 8, 8, 8, 2]
def call(fn, hd, of, n, have, ph, skip=None):
    outs = [np.full(k, 0xA5, dtype=np.uint8) for k in sizes]; fn.restype = ctypes.c_int
    rc = fn(hd, of, n, u64(15), u64(0), u64(2000), have, ph, u64(4), u64(1000), *[None if k == skip else ptr(a) for k, a in enumerate(outs)])
    return rc, [a for k, a in enumerate(outs) if k != skip]
ph = np.zeros(32, dtype=np.uint8)
for fn, arg, nodev in ((L.zkgpu_headers, ARG, NO_DEVICE), (L.zkHeaders, -1, -1)):
    rc, outs = call(fn, ptr(blob), ptr(off), 2, 1, ptr(ph)); assert rc == nodev and b"no HIP device" in L.zkgpu_last_error() and not any(a.any() for a in outs)
    rc, outs = call(fn, ptr(blob), ptr(dec), 2, 1, ptr(ph)); assert rc == arg and b"decrease" in L.zkgpu_last_error() and not any(a.any() for a in outs)
    rc, outs = call(fn, ptr(blob), ptr(off), -1, 1, ptr(ph)); assert rc == arg and b"negative" in L.zkgpu_last_error() and all(set(a) == {0xA5} for a in outs)   # n < 0: nothing to zero
    rc, outs = call(fn, None, ptr(off), 2, 1, ptr(ph)); assert rc == arg and b"null" in L.zkgpu_last_error() and not any(a.any() for a in outs)
    rc, outs = call(fn, ptr(blob), None, 2, 1, ptr(ph)); assert rc == arg and b"null" in L.zkgpu_last_error() and not any(a.any() for a in outs)
    rc, outs = call(fn, ptr(blob), ptr(off), 2, 1, None); assert rc == arg and b"null" in L.zkgpu_last_error() and not any(a.any() for a in outs)             # a parent without its hash
    rc, outs = call(fn, ptr(blob), ptr(off), 2, 0, None); assert rc == nodev and b"no HIP device" in L.zkgpu_last_error()
    for skip in range(15):
        rc, outs = call(fn, ptr(blob), ptr(off), 2, 1, ptr(ph), skip=skip); assert rc == arg and b"null" in L.zkgpu_last_error() and not any(a.any() for a in outs), skip
z = e.Zk()
try: z.Headers(hdrs, 15, 0, 2000, parent); raise SystemExit("no error")
except e.ZkGpuError as err: assert "no HIP device" in str(err)
k, o = z.Headers([], 15, 0, 2000, None); assert k == 0 and len(o) == 15 and all(v == [] for v in o.values())
print("NO DEVICE OK")
"""

def test_headers_entries_without_a_device(e, tmp_path):
    """a process that sees no device: both entries return -1 / ZKGPU_ERR_NO_DEVICE with every output zeroed, and every bad argument is reported before the device is asked for"""
    script = tmp_path / "no_device.py"; script.write_text(NO_DEVICE); keys = tmp_path / "keys"; keys.mkdir()
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ZK_PRFKEY_DIR=str(keys)))
    assert r.returncode == 0 and "NO DEVICE OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])

def test_headers_layout_regions_ascend_and_align(tmp_path):
    """HeadersLayout (txs_layout.hpp) as a program of its own under ASan + UBSan: over n and byte totals the regions ascend without overlap, number and time are 8-byte
    aligned on the device and in the download, and the pinned buffer holds the upload and the download"""
    src = tmp_path / "hl.cpp"; exe = str(tmp_path / "hl")
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "txs_layout.hpp"\nusing namespace zk;\n#define CHECK(x) do { if (!(x)) { printf("FAILED %s n=%zu t=%zu\\n", #x, n, tb); return 1; } } while (0)\n'
                   'int main() { const size_t ns[] = {1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 4097, 65536}, ts[] = {0, 1, 7, 8, 9, 611, 70001};\n'
                   '  for (size_t n : ns) for (size_t tb : ts) { const HeadersLayout L = headers_layout(n, tb);\n'
                   '    const size_t r[] = {L.off, L.H, L.rs, L.v, L.rec, L.ok, L.recovered, L.head, L.sp_head, L.number, L.time, L.hash, L.sealhash, L.signer, L.coinbase, L.tx_root, L.rtcmt, L.extra_beg, L.extra_size,\n'
                   '                        L.cmt_beg, L.cmt_count, L.difficulty, L.vote, L.status, L.end};\n'
                   '    const size_t w[] = {2 * (n + 1), TXL_H_WORDS * n, 16 * n, (n + 3) / 4, TXL_SP_HEAD, (n + 3) / 4, 5 * n, TXL_HEAD_WORDS, TXL_SP_HEAD, 2 * n, 2 * n, 8 * n, 8 * n, 5 * n, 5 * n, 8 * n, 8 * n, n, n, n, n,\n'
                   '                        (n + 3) / 4, (n + 3) / 4, (n + 3) / 4};\n'
                   '    CHECK(4 * L.off >= tb && L.total8 == 4 * L.off && L.up == 4 * L.H && L.up % 8 == 0);\n'
                   '    for (int k = 0; k < 24; k++) CHECK(r[k] + w[k] <= r[k + 1]);\n'
                   '    CHECK(L.sp_head == L.head + TXL_HEAD_WORDS && L.down == L.head && L.down_end == L.end && L.down % 2 == 0 && L.number % 2 == 0 && L.time % 2 == 0 && (L.number - L.down) % 2 == 0);\n'
                   '    CHECK(L.pin_bytes == L.up + 4 * (L.down_end - L.down)); }\n'
                   '  puts("HEADERS LAYOUT OK"); return 0; }\n')
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "blockmaze_amd", "csrc"), str(src), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HEADERS LAYOUT OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
