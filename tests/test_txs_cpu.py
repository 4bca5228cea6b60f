"""Sender inputs from raw transactions without a device (include/zk_txs.h): the Python model (tests/tx_model.py) against the two pins that do not come
from our own reading of the reference — the ten EIP-155 vectors (tests/golden/eip155_vectors.txt) and hashlib's SHA3-256 for the sponge — its round trips, every
mutator of tests/tx_corpus.py held to the verdict it claims, the header, the exports, and every new entry in a process that sees no device."""
import hashlib, os, random, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import secp_model as sm
import tx_model as t
import tx_corpus as c

DROPIN = ["zkTxSenders", "zkTxSigningInputs"]
ENGINE = ["zkgpu_tx_signing_inputs", "zkgpu_tx_senders", "zkgpu_test_keccak256"]

def vectors():
    out = []
    for l in open(os.path.join(ROOT, "tests", "golden", "eip155_vectors.txt")):
        if l.startswith("#"): continue
        f = l.split(); out.append(dict(AccountNonce=int(f[0]), Price=int(f[1]), GasLimit=int(f[2]), Recipient=bytes.fromhex(f[3]), Amount=int(f[4]), Payload=b"" if f[5] == "-" else bytes.fromhex(f[5]),
                                       V=int(f[6]), R=int(f[7], 16), S=int(f[8], 16), sender=bytes.fromhex(f[9])))
    return out

def test_model_recovers_the_sender_of_all_ten_eip155_vectors():
    """each vector wrapped into a 26-field transaction: the six signing fields and V, R, S are the vector's, so the nine-field hash under chain id 1 and the V
    arithmetic are the reference test's own; the other fields do not enter the hash"""
    vs = vectors(); assert len(vs) == 10 and vs[0]["sender"].hex() == "f0f6f18bca1b28cd68e4357452947e021241e9ce"
    rng = random.Random(1)
    for k, v in enumerate(vs):
        sender = v.pop("sender"); tx = c.rand_tx(rng, Code=k % 3, **v); raw = t.encode(tx)
        assert t.sender(raw, t.EIP155, 1) == (t.OK, k % 3, t.keccak256(raw), sender), k
        assert t.sender(raw, t.EIP155, 2)[0] == t.CHAIN_ID and t.sender(raw, t.HOMESTEAD, 1)[0] == t.SIG      # 37 and 38 are no V of the older signers
        d = t.signing_inputs(raw, t.EIP155, 1); assert d["sig"][64] == v["V"] - 37 and d["status"] == t.OK and d["deposit_from"] == bytes(20)

def test_sponge_against_sha3_256_and_the_empty_code_hash():
    """the multi-block sponge with the padding byte as a parameter: 0x06 makes it SHA3-256, which hashlib has; every length 0 .. 300 and the block edges"""
    rng = random.Random(2)
    for n in list(range(301)) + [135, 136, 137, 271, 272, 273, 407, 408, 409]:
        msg = rng.randbytes(n); assert t.sponge256(msg, 0x06) == hashlib.sha3_256(msg).digest(), n
        if n < 140 or n > 270: assert t.keccak256(msg) == sm.keccak256(msg)
    assert t.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"      # emptyCodeHash, core/state/state_object.go

def test_encode_decode_round_trips():
    rng = random.Random(3)
    for k in range(40):
        tx = c.rand_tx(rng, Recipient=None if k % 4 == 0 else rng.randbytes(20), Payload=rng.randbytes((0, 1, 55, 56, 300)[k % 5])); raw = t.encode(tx)
        got, spans = t.decode(raw); assert got == tx and len(spans) == t.NFIELDS == 26 and spans[0][0] in (1, 2, 3, 4) and spans[-1][1] == len(raw) and t.encode(got) == raw
        assert all(spans[i][1] == spans[i + 1][0] for i in range(25))
        if tx["Recipient"] is None:
            alt = t.encode(tx, nil_as_list=True); assert alt != raw and t.decode(alt)[0] == tx                # 0xC0 is nil too, and re-encodes as 0x80
            assert t.signing_inputs(alt, t.HOMESTEAD, 0) == t.signing_inputs(raw, t.HOMESTEAD, 0)
    for label, raw, signer, chain_id in c.valid_cases():
        assert t.signing_inputs(raw, signer, chain_id)["status"] in ((t.OK, t.CHAIN_ID) if "wrong" in label else (t.OK,)), label

def test_v_arithmetic_of_the_three_signers():
    rng = random.Random(4); st = lambda tx, s, cid: t.signing_inputs(t.encode(tx), s, cid)
    for cid in c.CHAIN_IDS:
        for parity in (0, 1):
            d = st(c.rand_tx(rng, Code=0, V=35 + 2 * cid + parity), t.EIP155, cid); assert d["status"] == t.OK and d["sig"][64] == parity
            d = st(c.rand_tx(rng, Code=0, V=27 + parity), t.EIP155, cid); assert d["status"] == t.OK and d["sig"][64] == parity
    assert st(c.rand_tx(rng, Code=0, V=34), t.EIP155, 2**62 - 1)["status"] == t.CHAIN_ID and t.derive_chain_id(34) == (2**64 - 1) // 2   # the wrap below 35
    assert st(c.rand_tx(rng, Code=0, V=2**64 + 35), t.EIP155, 0)["status"] == t.CHAIN_ID and st(c.rand_tx(rng, Code=0, V=256), t.HOMESTEAD, 0)["status"] == t.SIG
    d = st(c.rand_tx(rng, Code=0, V=0), t.FRONTIER, 0); assert d["status"] == t.OK and d["sig"][64] == (0 - 27) & 0xFF                  # byte(0 - 27): left to the recovery
    assert t.sender(t.encode(c.rand_tx(rng, Code=0, V=0)), t.FRONTIER, 0)[0] == t.SIG
    dep = c.rand_tx(rng, Code=3, V=2**70, R=2**256, S=7); d = st(dep, t.EIP155, 1)
    assert d["status"] == t.OK and d["deposit_from"] == dep["ZKAdrress"] and d["sig"] == bytes(32) + (7).to_bytes(32, "big") + b"\0"
    assert t.sender(t.encode(dep), t.EIP155, 1) == (t.OK, 3, t.keccak256(t.encode(dep)), dep["ZKAdrress"])

def test_every_mutator_changes_the_verdict_it_claims():
    """each refusal is built from a transaction the model accepts; a mutator that claims MALFORMED must make the decoder raise, and every rule is present for every base"""
    corpus = c.refusal_corpus(); rules = {}; classes = {t.OK: 0, t.MALFORMED: 0, t.CHAIN_ID: 0, t.SIG: 0}; assert len(corpus) >= 300
    for rule, claim, raw, signer, chain_id in corpus:
        got = t.sender(raw, signer, chain_id)[0]; rules[rule] = rules.get(rule, 0) + 1; classes[got] += 1
        if claim is not None: assert got == claim, (rule, got)
        if claim == t.MALFORMED:
            with pytest.raises(t.Malformed): t.decode(raw)
    names = [r for r, _ in c.malformed_mutators()]; assert len(set(names)) == len(names) >= 45 and all(rules[r] == 6 for r in names) and rules["valid"] == 6
    assert classes[t.OK] >= 6 and classes[t.MALFORMED] >= 270 and classes[t.CHAIN_ID] >= 12 and classes[t.SIG] >= 30, classes

def test_signed_cases_recover_their_keys():
    for raw, signer, chain_id, sender, status in c.signed_cases(count=12):
        got = t.sender(raw, signer, chain_id)
        if status is not None: assert (got[0], got[3]) == (status, sender)

# ---- the header and the exports ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

def test_txs_symbols_exported_by_libzkgpu_only(e):
    from test_abi_exports import SYMS, declared_symbols
    from test_tree_block_cpu import defined
    L = e.lib(); have = defined(e.LIB_PATH)
    for s in DROPIN + ENGINE: getattr(L, s); assert s in have, s
    assert sorted(set(declared_symbols("zk_txs.h")) - {"uint8_t"}) == DROPIN                       # ("uint8_t (*txhash)[32]" reads as a call to the helper)
    for s in ENGINE: assert s in declared_symbols("zkgpu.h"), s
    for lib, syms in SYMS.items():                                                                 # the four thin libraries: unchanged
        assert defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)) == sorted(syms), lib

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")])
def test_txs_header_compiles_as_c_and_cxx_when_included_twice(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_txs.h"\n#include "zk_txs.h"\n#include "zk_senders.h"\n'
                   'int main(void) { const uint8_t tx[1] = {0xc0}; const uint64_t off[2] = {0, 1}; uint8_t th[1][32], sh[1][32], sg[1][65], fr[1][20], code[1], st[1];\n'
                   '  if (zkTxSigningInputs(tx, off, 1, ZK_SIGNER_EIP155, 1, th, sh, sg, fr, code, st) != -1) return 1;\n'
                   '  return zkTxSenders(tx, off, 1, ZK_SIGNER_FRONTIER, 0, 0, fr, code, st) == -1 && ZK_TX_OK == 0 && ZK_TX_SIG == 3 ? 0 : 1; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

NO_DEVICE = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from blockmaze_amd import engine as e
L = e.lib(); assert e.device_count() == 0
NO_DEVICE, ARG = -1, -2
txs = [b"\xc0", b"\xc1\x80"]
rc, o = e.tx_signing_inputs(txs, e.SIGNER_EIP155, 1); assert rc == NO_DEVICE and b"no HIP device" in L.zkgpu_last_error() and not any(a.any() for a in o.values())
rc, o = e.tx_senders(txs, e.SIGNER_HOMESTEAD, 0); assert rc == NO_DEVICE and not any(a.any() for a in o.values())   # the wrapper hands 0xA5 in: every output is zeroed
rc, o = e.tx_senders(txs, e.SIGNER_HOMESTEAD, 0, want_txhash=False); assert rc == NO_DEVICE and o["txhash"] is None and not o["froms"].any()
# bad arguments win over the missing device
rc, o = e.tx_signing_inputs(txs, 3, 1); assert rc == ARG and b"signer" in L.zkgpu_last_error() and not any(a.any() for a in o.values())
rc, o = e.tx_senders(txs, e.SIGNER_EIP155, 2**62); assert rc == ARG and b"chain id" in L.zkgpu_last_error() and not any(a.any() for a in o.values())
rc, o = e.tx_senders(txs, e.SIGNER_EIP155, 2**62 - 1); assert rc == NO_DEVICE
assert e.tx_senders([], e.SIGNER_EIP155, 1)[0] == 0 and e.tx_signing_inputs([], e.SIGNER_FRONTIER, 0)[0] == 0     # n = 0 returns 0 and asks for no device
buf = lambda n: np.full(n, 0xA5, dtype=np.uint8); ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p); off = np.array([0, 1, 3], dtype=np.uint64); dec = np.array([0, 2, 1], dtype=np.uint64)
blob = buf(3); L.zkTxSenders.restype = ctypes.c_int; L.zkTxSigningInputs.restype = ctypes.c_int; cid = ctypes.c_uint64(1)
th, sh, sg, fr, code, st = buf(64), buf(64), buf(130), buf(40), buf(2), buf(2); outs = (th, sh, sg, fr, code, st)
assert L.zkTxSigningInputs(ptr(blob), ptr(off), 2, 2, cid, *[ptr(a) for a in outs]) == -1 and not any(a.any() for a in outs)          # no device
th, sh, sg, fr, code, st = outs = [buf(k) for k in (64, 64, 130, 40, 2, 2)]
assert L.zkTxSigningInputs(ptr(blob), ptr(dec), 2, 2, cid, *[ptr(a) for a in outs]) == -1 and b"decrease" in L.zkgpu_last_error() and not any(a.any() for a in outs)
th, sh, sg, fr, code, st = outs = [buf(k) for k in (64, 64, 130, 40, 2, 2)]
assert L.zkTxSigningInputs(ptr(blob), ptr(off), -1, 2, cid, *[ptr(a) for a in outs]) == -1 and all(set(a) == {0xA5} for a in outs)     # n < 0: nothing to zero
th, sh, sg, fr, code, st = outs = [buf(k) for k in (64, 64, 130, 40, 2, 2)]
assert L.zkTxSigningInputs(None, ptr(off), 2, 2, cid, *[ptr(a) for a in outs]) == -1 and b"null" in L.zkgpu_last_error() and not any(a.any() for a in outs)
th, fr, code, st = outs = [buf(k) for k in (64, 40, 2, 2)]
assert L.zkTxSenders(ptr(blob), ptr(off), 2, 1, cid, ptr(th), None, ptr(code), ptr(st)) == -1 and b"null" in L.zkgpu_last_error() and not (th.any() or code.any() or st.any())
th, fr, code, st = outs = [buf(k) for k in (64, 40, 2, 2)]
assert L.zkTxSenders(ptr(blob), ptr(off), 2, 1, cid, None, ptr(fr), ptr(code), ptr(st)) == -1 and b"no HIP device" in L.zkgpu_last_error() and not (fr.any() or code.any() or st.any())
z = e.Zk()
for call in (lambda: z.TxSenders(txs, e.SIGNER_EIP155, 1), lambda: z.TxSigningInputs(txs, e.SIGNER_EIP155, 1)):
    try: call(); raise SystemExit("no error")
    except e.ZkGpuError as err: assert "no HIP device" in str(err)
assert z.TxSenders([], e.SIGNER_EIP155, 1) == ([], [], [], []) and z.TxSigningInputs([], 0, 0) == ([], [], [], [], [], [])
try: e.keccak256([b"abc"]); raise SystemExit("keccak: no error")
except e.ZkGpuError as err: assert "zkgpu error -1" in str(err) and "no HIP device" in str(err)
print("NO DEVICE OK")
"""

def test_txs_entries_without_a_device(e, tmp_path):
    """a process that sees no device: both calls return -1 / ZKGPU_ERR_NO_DEVICE with every output zeroed, and every bad argument is reported before the device is asked for"""
    script = tmp_path / "no_device.py"; script.write_text(NO_DEVICE); keys = tmp_path / "keys"; keys.mkdir()
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ZK_PRFKEY_DIR=str(keys)))
    assert r.returncode == 0 and "NO DEVICE OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])

def test_workspace_layouts_under_sanitizers(tmp_path):
    """txs_layout.hpp (the workspace of every call of gpu_txs.hip, carved once) as a program of its own under ASan + UBSan: over n, byte totals, list counts and flags
    the regions ascend without overlap inside the workspace, the 64-bit regions are aligned, and every size and offset is the one the host functions were written with"""
    exe = str(tmp_path / "txs_layout_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "blockmaze_amd", "csrc"), os.path.join(ROOT, "tests", "txs_layout_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "TXS LAYOUT OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
