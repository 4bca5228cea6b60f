"""Senders from signatures without a device (include/zk_senders.h; DESIGN.md "Senders from signatures"): the Python model against every line of the fixture the
reference's own libsecp256k1 decided (tests/golden/ecrecover_cases.txt, tools/make_senders_golden.py) and against the three vectors the reference owns; forge()
against the model's recover(); the header, the exports, and every new entry in a process that sees no device."""
import os, random, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import secp_model as m

DROPIN = ["zkRecoverSenders"]
ENGINE = ["zkgpu_recover_senders", "zkgpu_test_secp_ops", "zkgpu_test_secp_lincomb", "zkgpu_test_secp_gtable", "zkgpu_test_senders_counters"]

def lines():
    return [l.split() for l in open(os.path.join(ROOT, "tests", "golden", "ecrecover_cases.txt"))]

def test_model_agrees_with_every_fixture_line():
    """verdict, key and address of all lines — none is left out — and the fixture holds what the issue lists: at most 600 lines, the reference's test signature, both
    parities, both homestead flags, refusals before the library and by it, and forged cases that end at infinity"""
    ls = lines(); assert 400 <= len(ls) <= 600; kinds = dict(accepted=0, refused=0, v0=0, v1=0, hs0=0, hs1=0)
    for f in ls:
        h = bytes.fromhex(f[0]); sig = bytes.fromhex(f[1]); hs = int(f[2]); ok, X, Y, addr = m.recover(h, sig, bool(hs)); assert len(h) == 32 and len(sig) == 65 and hs in (0, 1)
        assert ok == (f[3] == "1"), f[:4]
        if ok: assert (X.to_bytes(32, "big") + Y.to_bytes(32, "big")).hex() == f[4] and addr.hex() == f[5] and len(f) == 6 and m.on_curve((X, Y))
        else: assert len(f) == 4
        kinds["accepted" if ok else "refused"] += 1; kinds["hs%d" % hs] += 1
        if ok: kinds["v%d" % sig[64]] += 1
    assert kinds["accepted"] >= 300 and kinds["refused"] >= 90 and min(kinds["v0"], kinds["v1"]) >= 60 and min(kinds["hs0"], kinds["hs1"]) >= 100, kinds

def test_model_against_the_three_vectors_the_reference_owns():
    assert m.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"                                   # the hash of no code, core/state/state_test.go:62
    msg = bytes.fromhex("ce0677bb30baa8cf067c88db9811f4333d131bf8bcf12fe7065d211dce971008")                                                # crypto/signature_test.go:31-33
    sig = bytes.fromhex("90f27b8b488db00b00606796d2987f6a5f59ae62ea05effe84fef5b8b0e549984a691139ad57a3f0b906637673aa2f63d1f55cb1a69199d4009eea23ceaddc9301")
    pub = bytes.fromhex("e32df42865e97135acfb65f3bae71bdc86f4d49150ad6a440b6f15878109880a0a2b2667f7e725ceea70c673093bf67663e0312623c8e091b13cf2c0f11ef652")
    ok, X, Y, _ = m.recover(msg, sig, False); assert ok and X.to_bytes(32, "big") + Y.to_bytes(32, "big") == pub
    key = int("289c2857d4598e37fb9647507e47a309d6133539bf21a8b9cb6df88fd5232032", 16)                                                      # crypto/crypto_test.go:33-34
    assert m.address(m.mul(key, m.G)).hex() == "970e8128ab834e8eac17ab8e3812f010678cf791"

def test_forge_computes_the_chosen_combination_and_sign_recovers_its_key():
    rng = random.Random(3); N = m.N
    for k in (1, 2, 16, N - 1, rng.randrange(1, N)):
        base = m.mul(k, m.G)
        for u1, u2 in ((0, 1), (1, 1), (N - 1, 1), (5, N - 5), (rng.randrange(N), rng.randrange(1, N)), ((-k * 77) % N, 77)):
            h, sig = m.forge(k, u1, u2); want = m.lincomb(u1, u2, base); ok, X, Y, addr = m.recover(h, sig, False)
            assert ok == (want is not None) and (not ok or ((X, Y) == want and addr == m.address(want)))
    assert m.recover(*m.forge(3, (-3 * 9) % N, 9), False)[0] is False                                                                        # u1 + k u2 = 0: Q at infinity
    for _ in range(8):
        key = rng.randrange(1, N); h = rng.getrandbits(256).to_bytes(32, "big"); sig = m.sign(h, key, rng.randrange(1, N)); ok, X, Y, addr = m.recover(h, sig, True)
        assert ok and (X, Y) == m.mul(key, m.G) and int.from_bytes(sig[32:64], "big") <= N // 2

# ---- the header and the exports ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

def test_senders_symbols_exported_by_libzkgpu_only(e):
    from test_abi_exports import SYMS, declared_symbols
    from test_tree_block_cpu import defined
    L = e.lib(); have = defined(e.LIB_PATH)
    for s in DROPIN + ENGINE: getattr(L, s); assert s in have, s
    assert sorted(set(declared_symbols("zk_senders.h")) - {"uint8_t"}) == DROPIN                    # ("uint8_t (*sighash)[32]" reads as a call to the helper)
    for s in ENGINE: assert s in declared_symbols("zkgpu.h"), s
    for lib, syms in SYMS.items():                                                                 # the four thin libraries: unchanged
        assert defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)) == sorted(syms), lib

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")])
def test_senders_header_compiles_as_c_and_cxx_when_included_twice(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_senders.h"\n#include "zk_senders.h"\n#include "zk_accounts_chain.h"\n'
                   'int main(void) { const uint8_t h[1][32] = {{0}}; const uint8_t s[1][65] = {{0}}; uint8_t froms[1][20]; uint8_t pubs[1][64]; unsigned char ok[1];\n'
                   '  return zkRecoverSenders(h, s, 1, 1, froms, pubs, ok) == -1 ? 0 : 1; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

NO_DEVICE = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from blockmaze_amd import engine as e
L = e.lib(); assert e.device_count() == 0
NO_DEVICE = -1
rc, froms, pubs, ok = e.recover_senders([bytes(32)] * 2, [bytes(65)] * 2); assert rc == NO_DEVICE and b"no HIP device" in L.zkgpu_last_error()
assert not froms.any() and not pubs.any() and not ok.any()                                     # the wrapper hands 0xA5 in: every output is zeroed
z = e.Zk()
try: z.RecoverSenders([bytes(32)] * 2, [bytes(65)] * 2); raise SystemExit("no error")
except e.ZkGpuError as err: assert "no HIP device" in str(err)
assert z.RecoverSenders([], []) == ([], [], [])                                                # n = 0 returns 0 and asks for no device
L.zkRecoverSenders.restype = ctypes.c_int
buf = lambda n: np.full(n, 0xA5, dtype=np.uint8); ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p); h, s, fr, pb, ok = buf(64), buf(130), buf(40), buf(128), buf(2)
assert L.zkRecoverSenders(ptr(h), ptr(s), 2, 1, ptr(fr), ptr(pb), ptr(ok)) == -1 and not fr.any() and not pb.any() and not ok.any()
for name, call in (("ops", lambda: e.secp_ops("fq_mul", [1], [2])), ("lincomb", lambda: e.secp_lincomb([1], [1], [(1, 2)])), ("gtable", e.secp_gtable), ("counters", e.senders_counters)):
    try: call(); raise SystemExit(name + ": no error")
    except e.ZkGpuError as err: assert "zkgpu error -1" in str(err) and "no HIP device" in str(err), (name, str(err))
print("NO DEVICE OK")
"""

def test_senders_entries_without_a_device(e, tmp_path):
    """a process that sees no device: zkRecoverSenders returns -1 with every output zeroed, the engine entry and the four test entries answer ZKGPU_ERR_NO_DEVICE"""
    script = tmp_path / "no_device.py"; script.write_text(NO_DEVICE); keys = tmp_path / "keys"; keys.mkdir()
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ZK_PRFKEY_DIR=str(keys)))
    assert r.returncode == 0 and "NO DEVICE OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
