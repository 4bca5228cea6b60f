"""GPU parity of the whole proving path through the C-ABI:
  * proof BYTES equal to the real reference prover's on the reference-made key files committed under tests/golden
  * keys made by the GPU key generator are accepted by the oracle's reader, and oracle / engine / (when the compiled
    reference harness travelled with the repo) the real libsnark prover and verifier all agree on them
  * the full-size send circuit: key generation, proof with fixed (r, s), verification, and the drop-in cgo symbols."""
import json, os, subprocess, sys
import numpy as np
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import workload as w
import verify_mutations as vm
import verify_crafted
from conftest import record_leg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
have_ref = os.path.exists(HARNESS)

def ref(*args):
    r = subprocess.run([HARNESS, *args], capture_output=True, text=True); return r.returncode, r.stdout

@pytest.mark.parametrize("name", ["groth16_small", "groth16_step"])
def test_proof_bytes_match_reference_prover(golden_dir, name):
    d = os.path.join(golden_dir, name); meta = json.load(open(os.path.join(d, "meta.json"))); z = o.load_witness(os.path.join(d, "wit.bin"))
    p = e.Prover(os.path.join(d, "pk.txt")); assert (p.n_vars, p.n_inputs, p.m) == (meta["n_vars"], meta["n_inputs"], meta["domain_m"])
    proof = p.prove(z, int(meta["r"], 16), int(meta["s"], 16))
    assert proof == meta["proof"]                                                     # the reference prover's serialized bytes
    inputs = o.from_arr(z[:meta["n_inputs"]]); vk = os.path.join(d, "vk.txt")
    assert e.verify(vk, proof, inputs)
    assert not e.verify(vk, proof, [inputs[0] ^ 1] + inputs[1:]) and not e.verify(vk, proof, inputs[:-1])
    tampered = proof[:130] + ("0" if proof[130] != "0" else "1") + proof[131:]; assert not e.verify(vk, tampered, inputs)
    assert not e.verify(vk, "zz" + proof[2:], inputs)                                 # non-hex input is rejected, not UB (sendcgo.cpp:25-35)
    z2 = z.copy(); z2[meta["n_vars"] - 1, 0] ^= 1
    if not o.r1cs_is_satisfied(o.parse_pk(os.path.join(d, "pk.txt"))[1], z2):
        with pytest.raises(e.ZkGpuError): p.prove(z2, 1, 1)
    p2 = p.prove(z); assert p2 != proof and e.verify(vk, p2, inputs)                   # fresh randomness: different bytes, still valid
    p.close()

@pytest.mark.parametrize("name,seed", [("groth16_small", 11), ("groth16_step", 12)])
def test_keygen_agrees_with_oracle_and_reference(golden_dir, tmp_path, name, seed):
    d = os.path.join(golden_dir, name); pk_path, vk_path = str(tmp_path / "pk.txt"), str(tmp_path / "vk.txt")
    e.keygen_from_r1cs(os.path.join(d, "r1cs.bin"), pk_path, vk_path, seed=seed)
    z = o.load_witness(os.path.join(d, "wit.bin")); pk, cs = o.parse_pk(pk_path); vk = o.parse_vk(vk_path)     # oracle reads the engine's key files
    g = o.SplitMix64(seed); r, s = g.field(), g.field()
    exp = o.proof_hex(o.prove(cs, z, pk, r, s)); assert o.verify(vk, z[:cs.n_inputs], o.prove(cs, z, pk, r, s))
    p = e.Prover(pk_path); got = p.prove(z, r, s); p.close(); assert got == exp
    assert e.verify(vk_path, got, o.from_arr(z[:cs.n_inputs]))
    if have_ref:                                                                       # the real libsnark on the engine's key files
        rc, out = ref("prove", pk_path, os.path.join(d, "wit.bin"), str(cs.n_inputs), "%x" % r, "%x" % s); assert rc == 0 and ("proof " + got) in out
        rc, out = ref("verify", vk_path, got, str(cs.n_inputs), *[str(x) for x in o.from_arr(z[:cs.n_inputs])]); assert rc == 0 and "verify 1" in out

@pytest.fixture(scope="module")
def send_keys(tmp_path_factory):
    d = tmp_path_factory.mktemp("prfKey"); e.keygen("send", str(d / "sendpk.txt"), str(d / "sendvk.txt"), seed=0xB10C4A2E); return d

def hexargs(args): return [("0x" + a.hex()) if isinstance(a, bytes) else a for a in args]

def test_send_proof_full_size(send_keys, tmp_path):
    pk_path, vk_path = str(send_keys / "sendpk.txt"), str(send_keys / "sendvk.txt"); p = e.Prover(pk_path); assert (p.n_vars, p.n_inputs, p.m) == (227046, 5, 262144)
    d = w.reference_send_fixture(); wp = str(tmp_path / "w.bin"); e.witness_send(*hexargs(w.send_args(d)), wp); z = o.load_witness(wp)
    g = o.SplitMix64(2024); r, s = g.field(), g.field(); proof = p.prove(z, r, s); inputs = w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]])
    assert e.verify(vk_path, proof, inputs) and not e.verify(vk_path, proof, inputs[::-1])
    assert p.prove(z, r, s) == proof                                                    # deterministic given (r, s)
    d2 = w.send_instance(1); e.witness_send(*hexargs(w.send_args(d2)), wp); z2 = o.load_witness(wp); proof2 = p.prove(z2)
    assert e.verify(vk_path, proof2, w.pack_public([d2["cmtA_old"], d2["sn_old"], d2["cmtS"], d2["cmtA"]])) and not e.verify(vk_path, proof2, inputs)
    print("timings", p.timings()); p.close()

def test_send_proof_full_size_equals_libsnark_prover_bytes(send_keys, tmp_path):
    """the REAL libsnark prover (oracle/_ref/ref_harness, compiled from /root/reference by oracle/Makefile) loads the engine-made 77 MB send key with the reference's
    own operator>>, proves the reference's send fixture with the same (r, s): identical proof bytes, and the reference verifier accepts.  The harness travels with
    the repo to the GPU box; its absence is a FAILURE here, not a skip, so a green run means this leg ran (also listed in the run's last line)."""
    import time
    assert have_ref, "oracle/_ref/ref_harness is missing: run __graft_entry__.build() where /root/reference exists"
    pk_path, vk_path = str(send_keys / "sendpk.txt"), str(send_keys / "sendvk.txt"); p = e.Prover(pk_path)
    d = w.reference_send_fixture(); wp = str(tmp_path / "w.bin"); e.witness_send(*hexargs(w.send_args(d)), wp); z = o.load_witness(wp)
    g = o.SplitMix64(2024); r, s = g.field(), g.field(); proof = p.prove(z, r, s); p.close(); inputs = w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]])
    t0 = time.time(); rc, out = ref("prove", pk_path, wp, "5", "%x" % r, "%x" % s); assert rc == 0 and ("proof " + proof) in out, out[-600:]
    rc, out = ref("verify", vk_path, proof, "5", *[str(x) for x in inputs]); assert rc == 0 and "verify 1" in out
    record_leg("libsnark prover+verifier on the full-size send key: same bytes", time.time() - t0)

def test_send_key_made_by_the_libsnark_generator(tmp_path):
    """the direction a deployment needs: a full-size send key written by the REFERENCE generator (r1cs_gg_ppzksnark.tcc:212-388 via `ref_harness e2e` on the exported
    send R1CS, serialised with libsnark's operator<<: 943 k compressed points with the real pattern of points at infinity, send/getpvk.cpp:41-51) is loaded by this
    engine — text parser, k_g1_decompress / k_g2_decompress, the key-load transforms (H into the coset's Lagrange basis, C folded into L) — and the reference's send
    fixture proved with the harness's (r, s) must give the very proof line the reference prover printed; once through the text loader, once through the container."""
    import time
    assert have_ref, "oracle/_ref/ref_harness is missing: run __graft_entry__.build() where /root/reference exists"
    r1cs, wp, out_dir = str(tmp_path / "send.r1cs"), str(tmp_path / "w.bin"), tmp_path / "refkey"; out_dir.mkdir(); e.circuit_export("send", r1cs)
    d = w.reference_send_fixture(); e.witness_send(*hexargs(w.send_args(d)), wp); z = o.load_witness(wp); g = o.SplitMix64(4002); r, s = g.field(), g.field()
    t0 = time.time(); rc, out = ref("e2e", r1cs, wp, "%x" % r, "%x" % s, str(out_dir)); t_ref = time.time() - t0
    assert rc == 0 and "satisfied 1" in out and "verify 1" in out, out[-800:]
    ref_proof = [l.split()[1] for l in out.splitlines() if l.startswith("proof ")][0]; pk_path, vk_path = str(out_dir / "pk.txt"), str(out_dir / "vk.txt")
    assert os.path.getsize(pk_path) > 60e6 and e.lib().zkgpu_key_container_valid(pk_path.encode()) == 0
    inputs = w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]])
    p = e.Prover(pk_path); assert (p.n_vars, p.n_inputs, p.m) == (227046, 5, 262144); got = p.prove(z, r, s); fresh = p.prove(z); p.close()
    assert got == ref_proof                                                              # text loader: the reference prover's bytes under the reference's key
    assert e.lib().zkgpu_key_container_valid(pk_path.encode()) == 1
    p = e.Prover(pk_path); again = p.prove(z, r, s); p.close(); assert again == ref_proof     # ... and from the container the first load left behind
    assert e.verify(vk_path, got, inputs) and e.verify(vk_path, fresh, inputs) and not e.verify(vk_path, got, inputs[::-1])
    rc, out = ref("verify", vk_path, fresh, "5", *[str(x) for x in inputs]); assert rc == 0 and "verify 1" in out      # the reference verifier on a fresh-randomness proof
    record_leg("libsnark GENERATOR's full-size send key loaded (text + container): the reference prover's bytes", t_ref)

def test_dropin_symbols_send(send_keys, monkeypatch):
    monkeypatch.setenv("ZK_PRFKEY_DIR", str(send_keys)); zk = e.Zk(); d = w.send_instance(5)
    proof = zk.GenSendProof(*w.send_args(d)); assert len(proof) == 512 and not proof.startswith("0000000000")
    assert zk.VerifySendProof(proof, d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"])
    assert not zk.VerifySendProof(proof, d["cmtA"], d["sn_old"], d["cmtS"], d["cmtA_old"])
    assert zk.GenSendProof(*w.send_args(d)) != proof                                    # second call reuses the resident key; r, s are fresh
    bad = dict(d); bad["value_s"] = d["value_s"] + 1                                    # cmtS no longer matches: unsatisfied -> default proof, the failure sentinel of api.go:1690
    sentinel = zk.GenSendProof(*w.send_args(bad)); assert sentinel.startswith("0000000000") and sentinel[:128] == "%064x%064x" % (1, 2)
    assert not zk.VerifySendProof(sentinel, d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"])
    # the release library has no test hook that fixes (r, s): the variable must be ignored (zero-knowledge cannot be switched off from the environment)
    monkeypatch.setenv("ZK_FIXED_RS", "1234:5678"); a = zk.GenSendProof(*w.send_args(d)); b = zk.GenSendProof(*w.send_args(d)); assert a != b and zk.VerifySendProof(a, d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]) and zk.VerifySendProof(b, d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"])

@pytest.fixture(scope="module")
def all_keys(tmp_path_factory, send_keys):
    """config 4 of BASELINE.json: all four pk/vk pairs in one key directory"""
    d = send_keys
    for kind in ("mint", "redeem", "deposit"): e.keygen(kind, str(d / (kind + "pk.txt")), str(d / (kind + "vk.txt")), seed=0xB10C4A2E + len(kind))
    return d

def test_dropin_symbols_all_four_circuits_mixed(all_keys, monkeypatch):
    """mint + redeem (step domain 196,608), deposit (2^19, depth-8 Merkle), send (2^18), interleaved on one GPU through the cgo symbols"""
    monkeypatch.setenv("ZK_PRFKEY_DIR", str(all_keys)); zk = e.Zk()
    for rnd in range(2):
        m = w.mint_instance(rnd); p = zk.GenMintProof(*w.mint_args(m)); assert len(p) == 512 and zk.VerifyMintProof(p, m["cmtA_old"], m["sn_old"], m["cmtA"], m["value_s"]) and not zk.VerifyMintProof(p, m["cmtA_old"], m["sn_old"], m["cmtA"], m["value_s"] + 1)
        dd = w.deposit_instance(rnd); p = zk.GenDepositProof(*w.deposit_args(dd), dd["leaves"], dd["rt"], dd["sk"])
        assert zk.VerifyDepositProof(p, dd["rt"], dd["pk_recv"], dd["cmtB_old"], dd["sn_old"], dd["cmtB"], dd["sn_s"]) and not zk.VerifyDepositProof(p, dd["cmtB"], dd["pk_recv"], dd["cmtB_old"], dd["sn_old"], dd["cmtB"], dd["sn_s"])
        r = w.mint_instance(rnd, redeem=True); p = zk.GenRedeemProof(*w.mint_args(r)); assert zk.VerifyRedeemProof(p, r["cmtA_old"], r["sn_old"], r["cmtA"], r["value_s"])
        s = w.send_instance(10 + rnd); p = zk.GenSendProof(*w.send_args(s)); assert zk.VerifySendProof(p, s["cmtA_old"], s["sn_old"], s["cmtS"], s["cmtA"])
    bad = dict(r); bad["value_s"] = r["value_old"] + 1; bad["value"] = 0; assert zk.GenRedeemProof(*w.mint_args(bad)).startswith("0000000000")       # value_s > value_old
    dd = w.reference_deposit_fixture(); p = zk.GenDepositProof(*w.deposit_args(dd), dd["leaves"], dd["rt"], dd["sk"]); assert zk.VerifyDepositProof(p, dd["rt"], dd["pk_recv"], dd["cmtB_old"], dd["sn_old"], dd["cmtB"], dd["sn_s"])
    wrong_rt = bytes.fromhex("39524a6ae253fca75a89240d93c0c6d893bcb66e783606dbb1fc7dff92dc543c"); assert not zk.VerifyDepositProof(p, wrong_rt, dd["pk_recv"], dd["cmtB_old"], dd["sn_old"], dd["cmtB"], dd["sn_s"])   # deposit/main.cpp wrong_rt
    missing = dict(dd); missing["leaves"] = dd["leaves"][:9]; assert zk.GenDepositProof(*w.deposit_args(missing), missing["leaves"], dd["rt"], dd["sk"]).startswith("0000000000")   # cmtS not in cmtarray: sentinel, not a crash

def test_reference_fixtures_with_their_golden_values_through_the_cgo_symbols(all_keys, monkeypatch):
    """SURVEY.md §8(c)'s golden values — captured from the reference's own executables and libzk_*.so — as LITERAL strings through the drop-in symbols on the GPU path:
    the send fixture of send/main.cpp:123-142 (sn_old, cmtA_old, sn, cmtA, r_s, cmtS), the deposit fixture of deposit/main.cpp:131-167 (cmtS at leaf 9, wit.root = the
    root of the 16 leaves, tree.root = the 10-leaf prefix tree, wrong_root), the mint / redeem fixtures of mint/main.cpp:121-129, redeem/main.cpp:121-129"""
    monkeypatch.setenv("ZK_PRFKEY_DIR", str(all_keys)); zk = e.Zk(); L = zk.L; H = lambda b: b"0x" + b.hex().encode(); U = lambda h, n=32: int(h, 16).to_bytes(n, "big"); c64 = __import__("ctypes").c_uint64
    sn_old, cmtA_old = "4a31770fe5354a1a9632ebe1481e108cd82ce514ac094c57b5ffdfaea8ac138a", "036bdbabf553bd57e41289b8c13b80a9aef29c464a2cfca0c9e99c69fb9be4ff"
    sn, cmtA = "9b2d319b594f146c785aac11592a3e59f32cd6e6176a4d7a52d15a0b8eb6db06", "589effbb69ee8401c4108ad1e9a3de34e0fc81e283c6da9e95e6b9555dcb2835"
    r_s, cmtS = "8fe3dac1d2c00b427c4406d3fdfe43df999e7c8cc70dd9bf57953c2a9622e1b9", "e4b1743ea76c314992849f07fd9d8352d63e669773862df96305a4fd924cdbb4"
    sk, r_old, r, pk_sender, pk_recv = b"0x1", b"0x123456", b"0x12", b"0x456", b"0x123"                                                # short strings, as main.cpp writes them (uint256S zero-extends)
    assert L.computePRF(sk, r_old).decode() == sn_old and L.genCMT(c64(22), b"0x" + sn_old.encode(), r_old).decode() == cmtA_old and L.computeCRH(pk_sender, r).decode() == r_s
    assert L.computePRF(sk, r).decode() == sn and L.genCMT(c64(14), b"0x" + sn.encode(), r).decode() == cmtA and L.genCMTS(c64(8), pk_recv, b"0x" + r_s.encode(), b"0x" + sn_old.encode()).decode() == cmtS
    X = lambda h: b"0x" + h.encode()
    proof = L.genSendproof(c64(22), X(r_s), X(sn_old), r_old, X(cmtS), X(cmtA_old), c64(8), pk_recv, c64(14), X(sn), r, X(cmtA), sk, pk_sender).decode(); assert len(proof) == 512 and not proof.startswith("0000000000")
    assert L.verifySendproof(proof.encode(), X(cmtA_old), X(sn_old), X(cmtS), X(cmtA)) and not L.verifySendproof(proof.encode(), X(cmtA), X(sn_old), X(cmtS), X(cmtA_old))
    # deposit: value 264 = 255 + 9, leaves "1".."16" with cmtS at index 9
    d_cmtS, wit_root, tree_root, wrong_root = "e4593e968e75e96fd5c51212cadd046547226e98c1715de9a10e6dfa3e9fdca5", "2630f036430a646118dbb95ba55e9e3803e35a680398d01f9942513ebbb7911e", "6b3ab57816ea4d7bb6410b4a81484d1b64d08e33cc29160a789eb7a94c75f267", "39524a6ae253fca75a89240d93c0c6d893bcb66e783606dbb1fc7dff92dc543c"
    dd = w.reference_deposit_fixture(); assert dd["cmtS"].hex() == d_cmtS; leaves = b"".join(H(x) for x in dd["leaves"])
    assert L.genRoot(leaves, 16).decode() == wit_root and L.genRoot(leaves[:66 * 10], 10).decode() == tree_root and L.genCMTS(c64(9), b"0x123", b"0x123", b"0x123").decode() == d_cmtS
    dp = zk.GenDepositProof(*w.deposit_args(dd), dd["leaves"], U(wrong_root), dd["sk"]); assert not dp.startswith("0000000000")               # the RT argument is ignored, the root is recomputed (depositcgo.cpp:402-403)
    va = [H(dd[k]) for k in ("pk_recv", "cmtB_old", "sn_old", "cmtB", "sn_s")]
    assert L.verifyDepositproof(dp.encode(), X(wit_root), *va) and not L.verifyDepositproof(dp.encode(), X(wrong_root), *va) and not L.verifyDepositproof(dp.encode(), X(tree_root), *va)
    # mint 13 = 6 + 7 and redeem 13 = 20 - 7 with sk "1", r_old "123456", r "123"
    for redeem, v, vo, vs in ((False, 13, 6, 7), (True, 13, 20, 7)):
        r3 = b"0x123"; so = L.computePRF(sk, r_old); sn_ = L.computePRF(sk, r3); co = L.genCMT(c64(vo), b"0x" + so, r_old); cn = L.genCMT(c64(v), b"0x" + sn_, r3); assert so.decode() == sn_old
        gen, ver = (L.genRedeemproof, L.verifyRedeemproof) if redeem else (L.genMintproof, L.verifyMintproof)
        pr = gen(c64(v), c64(vo), b"0x" + so, r_old, b"0x" + sn_, r3, b"0x" + co, b"0x" + cn, c64(vs), sk); assert not pr.startswith(b"0000000000")
        assert ver(pr, b"0x" + co, b"0x" + so, b"0x" + cn, c64(vs)) and not ver(pr, b"0x" + co, b"0x" + so, b"0x" + cn, c64(vs + 1))

def test_mint_redeem_deposit_full_size_against_libsnark(all_keys, tmp_path):
    """the other three circuits at full size against the REAL libsnark (oracle/_ref/ref_harness): the reference's mint fixture (mint/main.cpp:121-129) and its redeem and
    deposit fixtures (redeem/main.cpp:121-129, deposit/main.cpp:131-167) are proved on the GPU with fixed (r, s); the reference VERIFIER accepts all three proofs under the
    engine-made keys and rejects them against wrong public inputs; the reference PROVER, loading the same key files with its own operator>>, returns the same proof bytes for
    mint and redeem (step-radix-2 domain of 196,608 inside libfqfft, step_radix2_domain.tcc:39-140; redeem adds the less_comparison gadget, redeem/circuit/gadget.tcc:70-135)
    and deposit (basic radix-2 domain 2^19)."""
    import time
    assert have_ref, "oracle/_ref/ref_harness is missing: run __graft_entry__.build() where /root/reference exists"
    def u(h, n=32): return int(h, 16).to_bytes(n, "big")
    g = o.SplitMix64(2025); legs = []
    def mint_like(redeem, value, value_old, value_s):
        sk, r_old, r = u("1"), u("123456"), u("123"); sn_old = w.prf(sk, r_old); sn = w.prf(sk, r)
        return dict(sk=sk, r_old=r_old, r=r, value=value, value_old=value_old, value_s=value_s, sn_old=sn_old, sn=sn, cmtA_old=w.cmt(value_old, sn_old, r_old), cmtA=w.cmt(value, sn, r))
    cases = [("mint", mint_like(False, 13, 6, 7), True), ("redeem", mint_like(True, 13, 20, 7), True), ("deposit", w.reference_deposit_fixture(), True)]
    for kind, d, with_prover in cases:
        pk_path, vk_path, wp = str(all_keys / (kind + "pk.txt")), str(all_keys / (kind + "vk.txt")), str(tmp_path / (kind + ".bin"))
        if kind == "deposit":
            e.witness_deposit(*hexargs(w.deposit_args(d)), "".join("0x" + l.hex() for l in d["leaves"]), len(d["leaves"]), "0x" + d["sk"].hex(), wp); n_in = 6
            inputs = w.pack_public([d["rt"], d["pk_recv"], d["cmtB_old"], d["sn_old"], d["cmtB"], d["sn_s"]])
        else:
            e.witness_mint_redeem(kind == "redeem", *hexargs(w.mint_args(d)), wp); n_in = 4; inputs = w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
        z = o.load_witness(wp); assert o.from_arr(z[:n_in]) == inputs
        r, s = g.field(), g.field(); p = e.Prover(pk_path); proof = p.prove(z, r, s); p.close()
        t0 = time.time(); rc, out = ref("verify", vk_path, proof, str(n_in), *[str(x) for x in inputs]); assert rc == 0 and "verify 1" in out, (kind, out[-300:])
        rc, out = ref("verify", vk_path, proof, str(n_in), *[str(x) for x in inputs[::-1]]); assert "verify 0" in out, kind
        if with_prover: rc, out = ref("prove", pk_path, wp, str(n_in), "%x" % r, "%x" % s); assert rc == 0 and ("proof " + proof) in out, (kind, out[-600:])
        legs.append("%s %s%.1f s" % (kind, "prover+verifier " if with_prover else "verifier ", time.time() - t0))
    record_leg("libsnark on the full-size mint / redeem / deposit keys, reference fixtures (" + ", ".join(legs) + ")")

def _build_driver(tmp_path):
    lib = os.path.join(ROOT, "blockmaze_amd", "lib"); exe = str(tmp_path / "drv")
    subprocess.check_call(["gcc", "-O1", "-o", exe, os.path.join(ROOT, "tests", "dropin_driver.c"), "-L" + lib, "-lzk_mint", "-lzk_send", "-lzk_deposit", "-lzk_redeem", "-lff", "-lsnark", "-lpthread", "-Wl,-rpath," + lib, "-Wl,-rpath-link," + os.path.join(ROOT, "blockmaze_amd")])
    return exe

def test_c_driver_send_through_thin_libraries(send_keys, tmp_path):
    """tests/dropin_driver.c linked with the reference's cgo link line: genSendproof + verifySendproof on the reference's send fixture"""
    out = subprocess.run([_build_driver(tmp_path), "send"], capture_output=True, text=True, env=dict(os.environ, ZK_PRFKEY_DIR=str(send_keys))).stdout
    assert "proof_len 512" in out and "verify 1" in out and "verify_wrong 0" in out and "head 0000000000" not in out

def test_c_driver_all_circuits_and_threads(all_keys, tmp_path):
    """the same C caller for mint, redeem and deposit (the fixtures of the reference's main.cpp files; deposit computes its root with genRoot(n = 16): the golden value of
    SURVEY.md §8c) and from 8 pthreads at once, every thread proving and verifying all four circuits twice through the thin libzk_*.so — cgo calls arrive on arbitrary
    OS threads (zktx.go:406-430)"""
    exe = _build_driver(tmp_path); env = dict(os.environ, ZK_PRFKEY_DIR=str(all_keys))
    for kind in ("mint", "redeem", "deposit"):
        r = subprocess.run([exe, kind], capture_output=True, text=True, env=env); assert r.returncode == 0 and (kind + " ") in r.stdout and "proof_len 512" in r.stdout and "verify 1 verify_wrong 0" in r.stdout and "head 0000000000" not in r.stdout, (kind, r.stdout[-400:], r.stderr[-400:])
        if kind == "deposit": assert "root 2630f036430a646118dbb95ba55e9e3803e35a680398d01f9942513ebbb7911e" in r.stdout
    r = subprocess.run([exe, "threads"], capture_output=True, text=True, env=env, timeout=600); assert r.returncode == 0 and "threads_good 64 of 64" in r.stdout, (r.stdout[-600:], r.stderr[-600:])

def test_msm_sharding_matches_unsharded(send_keys, golden_dir, tmp_path):
    """K7: the queries cut into 1, 2, 3 and 8 contiguous shards (here all on one GPU), partial records added on the host: same proof bytes"""
    g = o.SplitMix64(77); r, s = g.field(), g.field()
    for pk_path, z in ((os.path.join(golden_dir, "groth16_step", "pk.txt"), o.load_witness(os.path.join(golden_dir, "groth16_step", "wit.bin"))),):
        full = e.Prover(pk_path); exp = full.prove(z, r, s); full.close()
        for world in (1, 2, 3, 8):
            recs = []
            for rank in range(world):
                p = e.Prover(pk_path, rank, world); p.set_witness(z); recs.append(p.prove_partial())
                if rank + 1 < world: p.close()
            assert p.finish(recs[::-1], r, s) == exp, world; p.close()              # record order does not matter
    pk_path = str(send_keys / "sendpk.txt"); d = w.send_instance(3); wp = str(tmp_path / "w.bin"); e.witness_send(*hexargs(w.send_args(d)), wp); z = o.load_witness(wp)
    full = e.Prover(pk_path); exp = full.prove(z, r, s); full.close(); recs = []
    for rank in range(2): p = e.Prover(pk_path, rank, 2); p.set_witness(z); recs.append(p.prove_partial()); p.close() if rank == 0 else None
    assert p.finish(recs, r, s) == exp and e.verify(str(send_keys / "sendvk.txt"), exp, w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]])); p.close()

@pytest.mark.parametrize("name", ["groth16_small", "groth16_step"])
def test_gpu_verifier_values_equal_the_host_model_round_by_round(golden_dir, name):
    """kernel K9 against the host model of its own arithmetic (vsched::simulate29, the interpreter the CPU tests pin against libsnark's verdicts): after EVERY round of the
    schedule the LDS slots the schedule has written hold the same nine limbs — on a valid proof (accepted) and on a tampered one (rejected).  A disagreement names its round."""
    d = os.path.join(golden_dir, name); meta = json.load(open(os.path.join(d, "meta.json"))); z = o.load_witness(os.path.join(d, "wit.bin")); vk = os.path.join(d, "vk.txt")
    inputs = o.from_arr(z[:meta["n_inputs"]]); good = meta["proof"]; bad = good[:100] + ("0" if good[100] != "0" else "1") + good[101:]
    assert e.verify_trace(vk, good, inputs, 1) == (-1, 0, 1)
    r, slot, verdict = e.verify_trace(vk, bad, inputs, 1); assert (r, verdict) == (-1, 0), (r, slot, verdict)

@pytest.mark.parametrize("name", ["groth16_small", "groth16_step"])
def test_batched_gpu_verifier_matches_host_verifier(golden_dir, name):
    """K9's large-batch branch: one workgroup per proof.  A batch mixing the reference prover's proof, fresh proofs, tampered proofs (each coordinate), wrong public inputs, the
    default proof and garbage must be decided exactly like the host verifier (which is pinned against libsnark's verifier and GT values)."""
    d = os.path.join(golden_dir, name); meta = json.load(open(os.path.join(d, "meta.json"))); z = o.load_witness(os.path.join(d, "wit.bin")); vk = os.path.join(d, "vk.txt")
    inputs = o.from_arr(z[:meta["n_inputs"]]); p = e.Prover(os.path.join(d, "pk.txt")); good = [meta["proof"]] + [p.prove(z) for _ in range(3)]; p.close()
    proofs, ins = verify_crafted.mixed_batch(good, inputs)
    got = e.verify_batch(vk, proofs, ins); exp = [e.verify(vk, pr, x) for pr, x in zip(proofs, ins)]
    assert got == exp and got[:len(good)] == [True] * len(good) and not any(got[len(good):])
    # ... and like the ORACLE's verifier (checker code pinned against libsnark's verifier and GT values in test_oracle_golden.py), wherever the record is 512 hex digits of a
    # non-zero proof (the oracle reads (0, 0) as the group's zero, a hex proof has Z = 1: see proof_from_hex)
    ovk = o.parse_vk(vk)
    for pr, x, g_ in zip(proofs, ins, got):
        if all(c in "0123456789abcdef" for c in pr) and pr != "0" * 512: assert o.verify(ovk, x, o.proof_words_from_hex(pr)) == g_
    assert e.verify_batch(vk, [], []) == []
    assert e.verify_batch(vk, [good[0]], [inputs[:-1]]) == [False]                        # wrong number of public inputs (strong IC)

@pytest.mark.parametrize("name", ["groth16_small", "groth16_step"])
def test_gpu_verifier_verdicts_are_the_reference_s_on_mutated_proofs(golden_dir, name):
    """kernel K9 on the ~290 committed mutations of the reference prover's proof (tests/golden/verify_mutations_*.txt: aliases c + kq, special values, off-curve,
    off-subgroup, malleations, re-randomisations, other statements) — one launch per input count, and one proof per launch for every fifth case: the verdict of the
    reference's verifier behind sendcgo.cpp:388-448 every time (an encoding on which the assert-enabled reference aborts is rejected)"""
    vk = os.path.join(golden_dir, name, "vk.txt"); cases = vm.read_golden(os.path.join(golden_dir, "verify_mutations_%s.txt" % name)); assert len(cases) >= 200; n_acc = 0
    for ni in sorted(set(len(c[2]) for c in cases)):
        grp = [c for c in cases if len(c[2]) == ni]; got = e.verify_batch(vk, [c[1] for c in grp], [c[2] for c in grp])
        for c, g_ in zip(grp, got): assert vm.agrees(g_, c[3]), (c[0], c[3]); n_acc += int(g_)
    assert n_acc >= 100
    for c in cases[::5]: assert vm.agrees(e.verify_batch(vk, [c[1]], [c[2]])[0], c[3]), (c[0], c[3])

def test_verify_symbols_decide_like_libsnark_on_mutated_proofs(all_keys, monkeypatch, tmp_path):
    """the accept set at the BOUNDARY, all four kinds at full size: a proof from gen*proof, ~280 seeded mutations of its 512 characters each (tests/verify_mutations.py),
    the verdict of the reference's verifier (oracle/_ref/ref_harness verifymany: r1cs_gg_ppzksnark_verifier_strong_IC on the engine-made vk.txt read by libsnark's
    operator>>, hex parsed as in sendcgo.cpp:388-448 / mintcgo.cpp / depositcgo.cpp:446-551 / redeemcgo.cpp) — and verify*proof (kernel K9, one proof per launch) as well
    as verifyBatch (one launch per kind) return exactly that for every case; then the same proofs against other statements"""
    import time
    assert have_ref, "oracle/_ref/ref_harness is missing: run __graft_entry__.build() where /root/reference exists"
    monkeypatch.setenv("ZK_PRFKEY_DIR", str(all_keys)); zk = e.Zk(); legs = []; items = []; expect = []
    m = w.mint_instance(41); r = w.mint_instance(42, redeem=True); sd = w.send_instance(43); dd = w.deposit_instance(44)
    kinds = [("mint", zk.GenMintProof(*w.mint_args(m)), [m["cmtA_old"], m["sn_old"], m["cmtA"]], m["value_s"], zk.VerifyMintProof),
             ("redeem", zk.GenRedeemProof(*w.mint_args(r)), [r["cmtA_old"], r["sn_old"], r["cmtA"]], r["value_s"], zk.VerifyRedeemProof),
             ("send", zk.GenSendProof(*w.send_args(sd)), [sd["cmtA_old"], sd["sn_old"], sd["cmtS"], sd["cmtA"]], None, zk.VerifySendProof),
             ("deposit", zk.GenDepositProof(*w.deposit_args(dd), dd["leaves"], dd["rt"], dd["sk"]), [dd["rt"], dd["pk_recv"], dd["cmtB_old"], dd["sn_old"], dd["cmtB"], dd["sn_s"]], None, zk.VerifyDepositProof)]
    for kind, proof, args, value_s, fn in kinds:
        vk = str(all_keys / (kind + "vk.txt")); inputs = w.pack_public(args, value_s); tail = [] if value_s is None else [value_s]; assert fn(proof, *args, *tail), kind
        cases = [c for c in vm.cases(vk, proof, inputs, 0xC0DE + len(kind)) if c[2] == inputs]; t0 = time.time(); ref_v = vm.reference_verdicts(HARNESS, vk, cases, tmp_path); legs.append("%s %d cases %.1f s" % (kind, len(cases), time.time() - t0))
        assert len(cases) >= 200 and ref_v.count(1) >= 100 and ref_v.count(0) >= 90, (kind, len(cases), ref_v.count(1))
        for (label, h, _), v in zip(cases, ref_v):
            assert vm.agrees(fn(h, *args, *tail), v), (kind, label, v)
            items.append((kind, h, args, value_s or 0)); expect.append(v == 1)
        # other statements: the reference packs whatever it is given (gadget.tcc witness_map) — a proof is bound to its own public input
        for j in range(len(args)):
            other = list(args); other[j] = bytes(x ^ (1 if i == len(args[j]) - 1 else 0) for i, x in enumerate(args[j])); oin = w.pack_public(other, value_s)
            v = vm.reference_verdicts(HARNESS, vk, [("other statement", proof, oin)], tmp_path)[0]; assert v == 0 and fn(proof, *other, *tail) is False, (kind, j)
    rc, ok = zk.VerifyBatch(items); assert ok == expect and rc == sum(expect)
    record_leg("libsnark verifier on mutated proofs of all four kinds (" + ", ".join(legs) + ")")

def test_concurrent_single_proof_verifications_share_launches(golden_dir):
    """go-ethereum verifies one proof a call from many goroutines: calls that meet inside the GPU verifier are ONE launch (gpu_verify.hip: Impl::Pending) — eight threads,
    valid and tampered proofs and wrong inputs interleaved, every caller gets its own verdict; fewer launches than calls"""
    import threading
    d = os.path.join(golden_dir, "groth16_small"); meta = json.load(open(os.path.join(d, "meta.json"))); z = o.load_witness(os.path.join(d, "wit.bin")); vk = os.path.join(d, "vk.txt")
    inputs = o.from_arr(z[:meta["n_inputs"]]); good = meta["proof"]; bad = good[:300] + ("0" if good[300] != "0" else "1") + good[301:]; wrong = list(inputs); wrong[0] = (wrong[0] + 1) % o.R_MOD
    cases = [(good, inputs, True), (bad, inputs, False), (good, wrong, False), (good, inputs, True)]
    assert [e.verify_batch(vk, [p], [x])[0] for p, x, _ in cases] == [w for _, _, w in cases]
    c0, l0 = e.verify_counters(vk); errs = []
    def caller(k):
        for i in range(60):
            p, x, want = cases[(i + k) % len(cases)]; got = e.verify_batch(vk, [p], [x])[0]
            if got != want: errs.append((k, i, got, want))
    ths = [threading.Thread(target=caller, args=(k,)) for k in range(8)]
    for t in ths: t.start()
    for t in ths: t.join()
    c1, l1 = e.verify_counters(vk); assert not errs, errs[:5]; assert c1 - c0 == 480 and 0 < l1 - l0 <= c1 - c0
    # (a batch of several proofs in one call still is one call)
    assert e.verify_batch(vk, [good, bad, good], [inputs, inputs, wrong]) == [True, False, False]

def test_gpu_verifier_random_curve_points_match_host(golden_dir):
    """K9 on 29-bit limbs keeps lazily reduced values whose bounds the schedule builder proves; here it is fed what a prover never produces — 160 "proofs" made of
    random multiples of the generators (on the curve, so that the whole pairing runs on arbitrary field values) under random or genuine public inputs, and valid proofs under
    random public inputs — shuffled among 24 valid proofs with fresh (r, s): every verdict must be the host verifier's, in one launch and record by record"""
    d = os.path.join(golden_dir, "groth16_small"); meta = json.load(open(os.path.join(d, "meta.json"))); z = o.load_witness(os.path.join(d, "wit.bin")); vk = os.path.join(d, "vk.txt")
    inputs = o.from_arr(z[:meta["n_inputs"]]); p = e.Prover(os.path.join(d, "pk.txt")); good = [p.prove(z) for _ in range(24)]; p.close()
    proofs, ins = verify_crafted.random_curve_batch(good, inputs)
    got = e.verify_batch(vk, proofs, ins); exp = [e.verify(vk, pr, x) for pr, x in zip(proofs, ins)]
    assert got == exp and sum(got) == 24
    for pr, x, v in list(zip(proofs, ins, got))[:40]: assert e.verify_batch(vk, [pr], [x]) == [v]       # ... and one record per launch

def test_batched_gpu_verifier_send_at_scale(send_keys, tmp_path):
    """512 send proofs in one launch (4 distinct valid proofs and their corrupted twins, interleaved)"""
    pk_path, vk_path = str(send_keys / "sendpk.txt"), str(send_keys / "sendvk.txt"); p = e.Prover(pk_path); proofs, ins, exp = [], [], []
    base = []; wp = str(tmp_path / "w.bin")
    for i in range(4):
        d = w.send_instance(40 + i); e.witness_send(*hexargs(w.send_args(d)), wp); z = o.load_witness(wp); base.append((p.prove(z), w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]])))
    p.close()
    for k in range(512):
        pr, x = base[k % 4]
        if k % 3 == 1: pr = pr[:300] + ("5" if pr[300] != "5" else "6") + pr[301:]
        if k % 3 == 2: x = list(x); x[k % len(x)] = (x[k % len(x)] + k) % o.R_MOD
        proofs.append(pr); ins.append(x); exp.append(k % 3 == 0)
    assert e.verify_batch(vk_path, proofs, ins) == exp
    assert all(e.verify(vk_path, *base[i]) for i in range(4))

def test_deposit_depth32_single_gpu(tmp_path):
    """BASELINE.json configs[4] on one GPU: the deposit circuit with the Merkle tree depth raised to 32: 1,070,591 variables, step domain
    2^20 + 2^17 = 1,179,648, H-query MSM of 1,179,647 points.  Key generation, witness, proof with fixed (r, s) (deterministic), host verifier, batched GPU verifier."""
    pk_path, vk_path, wp = str(tmp_path / "pk.txt"), str(tmp_path / "vk.txt"), str(tmp_path / "w.bin"); e.keygen("deposit", pk_path, vk_path, seed=32, tree_depth=32)
    p = e.Prover(pk_path); assert (p.n_vars, p.n_inputs, p.m) == (1070591, 6, 1179648)
    dd = w.deposit_instance(3); rt, _ = w.merkle_root_and_path(dd["leaves"], dd["index"], depth=32)
    cmtarray = "".join("0x" + l.hex() for l in dd["leaves"])
    e.witness_deposit(*hexargs(w.deposit_args(dd)), cmtarray, len(dd["leaves"]), "0x" + dd["sk"].hex(), wp, tree_depth=32); z = o.load_witness(wp)
    inputs = w.pack_public([rt, dd["pk_recv"], dd["cmtB_old"], dd["sn_old"], dd["cmtB"], dd["sn_s"]]); assert o.from_arr(z[:6]) == inputs
    proof = p.prove(z, 5, 7); assert p.prove(z, 5, 7) == proof; print("timings", p.timings()); p.close()
    assert e.verify(vk_path, proof, inputs) and not e.verify(vk_path, proof, inputs[::-1])
    assert e.verify_batch(vk_path, [proof, proof], [inputs, inputs[::-1]]) == [True, False]
    assert have_ref, "oracle/_ref/ref_harness is missing"                                # the reference verifier on the depth-32 key (step-radix-2 domain of 1,179,648 in the prover)
    import time; t0 = time.time(); rc, out = ref("verify", vk_path, proof, "6", *[str(x) for x in inputs]); assert rc == 0 and "verify 1" in out, out[-300:]
    rc, out = ref("verify", vk_path, proof, "6", *[str(x) for x in inputs[::-1]]); assert "verify 0" in out
    record_leg("libsnark verifier on the depth-32 deposit proof", time.time() - t0)
    # ... and the reference PROVER on the same 364 MB key with the same (r, s): the only circuit on the window-by-window MSM path (its tables pass the fixed-base cap) and on
    # the 2^20 + 2^17 step domain must give the same bytes (libfqfft step_radix2_domain.tcc:39-140, multiexp.tcc:165-282 at n = 1,179,647)
    t0 = time.time(); rc, out = ref("prove", pk_path, wp, "6", "5", "7"); assert rc == 0 and ("proof " + proof) in out, out[-600:]
    record_leg("libsnark prover on the depth-32 deposit key: same bytes", time.time() - t0)

@pytest.mark.parametrize("env", [{"ZK_WITNESS_DENSE": "1"}, {"ZK_HANDOVER_MAPPED": "0"}, {"ZK_VERIFY_WHILE_PROVING": "0", "ZK_VERIFY_STREAMS": "2"}, {"ZK_DEVICES": "all", "ZK_PROVERS_PER_KEY": "2"}, {"ZK_PROVERS_PER_KEY": "1", "ZK_WITNESS_THREADS": "0", "ZK_SUBMIT_THREADS": "0"}], ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_cgo_symbols_under_process_wide_switches(all_keys, env):
    """switches that only the cgo layer reads (a fresh process each: they are read once).  ZK_DEVICES=all: the prover pool spread over every visible GPU (one here);
    one prover per key with no helper threads at all; and the dense hand-over: the cgo path hands the circuit board's tagged assignment to the prover in compact form; an assignment with too many values other than 0 / 1 would go as a plain
    vector instead — a branch no BlockMaze circuit reaches, forced here by ZK_WITNESS_DENSE=1 (a fresh process: the switch is read once): proofs must still verify"""
    code = ("import os, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nfrom blockmaze_amd import engine as e\nimport workload as w\nzk = e.Zk()\n"
            "s = w.send_instance(41); p = zk.GenSendProof(*w.send_args(s)); m = w.mint_instance(42); q = zk.GenMintProof(*w.mint_args(m))\n"
            "print('DENSE', zk.VerifySendProof(p, s['cmtA_old'], s['sn_old'], s['cmtS'], s['cmtA']), zk.VerifyMintProof(q, m['cmtA_old'], m['sn_old'], m['cmtA'], m['value_s']))\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, ZK_PRFKEY_DIR=str(all_keys), **env), timeout=600)
    assert "DENSE True True" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])

def test_cgo_symbols_with_sharded_msms(all_keys):
    """ZK_SHARD_DEVICES=3 (capi_zk.cpp: prove_sharded): every gen*proof call runs on three shard provers — contiguous thirds of every query, here all on the box's one GPU —,
    each on its own thread (replicated rows / transforms, its slice of the five MSMs, a 384-byte record of partial sums), the calling thread adds the records and assembles
    the proof: no torch, no collective, what a go-ethereum process can use.  Proofs of send, mint and deposit are accepted by the per-proof verifier symbols of an
    unsharded process, a statement that does not hold yields the failure sentinel, and two callers at once are served one after the other"""
    code = """
import os, sys, json, threading
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))
from blockmaze_amd import engine as e
import workload as w
zk = e.Zk(); out = {}
d = w.send_instance(31); out['send'] = [zk.GenSendProof(*w.send_args(d)), d['cmtA_old'].hex(), d['sn_old'].hex(), d['cmtS'].hex(), d['cmtA'].hex()]
bad = dict(d); bad['value_s'] = d['value_s'] + 1; out['sentinel'] = zk.GenSendProof(*w.send_args(bad))
m = w.mint_instance(32); out['mint'] = [zk.GenMintProof(*w.mint_args(m)), m['cmtA_old'].hex(), m['sn_old'].hex(), m['cmtA'].hex(), m['value_s']]
dd = w.deposit_instance(33); out['deposit'] = [zk.GenDepositProof(*w.deposit_args(dd), dd['leaves'], dd['rt'], dd['sk'])] + [dd[k].hex() for k in ('rt', 'pk_recv', 'cmtB_old', 'sn_old', 'cmtB', 'sn_s')]
two = [None, None]
def call(i): two[i] = zk.GenSendProof(*w.send_args(d))
ts = [threading.Thread(target=call, args=(i,)) for i in range(2)]; [t.start() for t in ts]; [t.join() for t in ts]; out['two'] = two
print('RESULT ' + json.dumps(out))
""" % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZK_PRFKEY_DIR=str(all_keys), ZK_SHARD_DEVICES="3"), capture_output=True, text=True, timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]; assert line, (r.stdout[-2000:], r.stderr[-2000:]); out = json.loads(line[0][7:])
    os.environ["ZK_PRFKEY_DIR"] = str(all_keys); zk = e.Zk(); B = bytes.fromhex
    p, *a = out["send"]; assert len(p) == 512 and zk.VerifySendProof(p, *[B(x) for x in a]) and not zk.VerifySendProof(p, B(a[3]), B(a[1]), B(a[2]), B(a[0]))
    assert out["sentinel"].startswith("0000000000") and out["sentinel"][:128] == "%064x%064x" % (1, 2)
    p, *a = out["mint"]; assert zk.VerifyMintProof(p, B(a[0]), B(a[1]), B(a[2]), a[3])
    p, *a = out["deposit"]; assert zk.VerifyDepositProof(p, *[B(x) for x in a])
    d = out["send"][1:]; assert all(zk.VerifySendProof(q, *[B(x) for x in d]) for q in out["two"]) and out["two"][0] != out["two"][1]

def test_gpu_verifier_failure_falls_back_to_the_host_verdict(all_keys):
    """a fault on the GPU branch of verify_group (here forced by ZK_TEST_FAIL_GPU_VERIFY in a fresh process) must not turn an accept into a reject: single-proof symbols
    and verifyBatch are then decided by the prepared host verifier, valid proofs stay valid, invalid ones stay invalid, and the failure is logged"""
    code = ("import os, sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nfrom blockmaze_amd import engine as e\nimport workload as w\nzk = e.Zk()\n"
            "s = w.send_instance(61); p = zk.GenSendProof(*w.send_args(s)); a = [s['cmtA_old'], s['sn_old'], s['cmtS'], s['cmtA']]\n"
            "one = (zk.VerifySendProof(p, *a), zk.VerifySendProof(p, *a[::-1]))\n"
            "rc, ok = zk.VerifyBatch([('send', p, a, 0), ('send', p, a[::-1], 0), ('send', p, a, 0)])\n"
            "print('FALLBACK', one, rc, ok)\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, ZK_PRFKEY_DIR=str(all_keys), ZK_TEST_FAIL_GPU_VERIFY="1"), timeout=600)
    assert "FALLBACK (True, False) 2 [True, False, True]" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
    assert "GPU verifier failed" in r.stderr and "on the host" in r.stderr

def test_concurrent_cgo_calls_overlap_and_stay_correct(all_keys, monkeypatch):
    """cgo calls arrive on arbitrary OS threads (threading): 8 threads call genSendproof / genMintproof / genRedeemproof at the same time (pool of
    provers per key, each on its own stream set); every proof must verify against its own public inputs and none against its neighbour's"""
    import threading
    monkeypatch.setenv("ZK_PRFKEY_DIR", str(all_keys)); zk = e.Zk(); out = {}; errs = []
    def send_job(i):
        try:
            for j in range(3): s = w.send_instance(100 + 10 * i + j); out[("send", i, j)] = (s, zk.GenSendProof(*w.send_args(s)))
        except Exception as ex: errs.append(ex)
    def mint_job(i, redeem):
        try:
            for j in range(3): m = w.mint_instance(200 + 10 * i + j, redeem=redeem); out[("redeem" if redeem else "mint", i, j)] = (m, (zk.GenRedeemProof if redeem else zk.GenMintProof)(*w.mint_args(m)))
        except Exception as ex: errs.append(ex)
    ths = [threading.Thread(target=send_job, args=(i,)) for i in range(4)] + [threading.Thread(target=mint_job, args=(i, i % 2 == 1)) for i in range(4)]
    for t in ths: t.start()
    for t in ths: t.join()
    assert not errs and len(out) == 24
    for (kind, i, j), (d, p) in out.items():
        assert len(p) == 512 and not p.startswith("0000000000"), (kind, i, j)
        if kind == "send": assert zk.VerifySendProof(p, d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"])
        elif kind == "mint": assert zk.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"])
        else: assert zk.VerifyRedeemProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"])
    (d0, p0), (d1, p1) = out[("send", 0, 0)], out[("send", 1, 0)]; assert not zk.VerifySendProof(p0, d1["cmtA_old"], d1["sn_old"], d1["cmtS"], d1["cmtA"])


def test_one_pass_sort_overflow_inside_the_prover(golden_dir):
    """ZK_MSM_DIRECT_CAP=1 makes every bucket of the H query's one-pass sort overflow: the prover must notice, redo that MSM on the two-pass path (materialising the
    fused zinv*a*b product first) and still emit the reference prover's bytes"""
    code = ("import json, os, sys; sys.path.insert(0, %r); from blockmaze_amd import engine as e; from oracle import pyoracle as o; d = %r; "
            "meta = json.load(open(os.path.join(d, 'meta.json'))); z = o.load_witness(os.path.join(d, 'wit.bin')); p = e.Prover(os.path.join(d, 'pk.txt')); "
            "assert p.prove(z, int(meta['r'], 16), int(meta['s'], 16)) == meta['proof']; assert p.prove(z, int(meta['r'], 16), int(meta['s'], 16)) == meta['proof']; print('same bytes')")
    for name in ("groth16_small", "groth16_step"):
        r = subprocess.run([sys.executable, "-c", code % (ROOT, os.path.join(golden_dir, name))], capture_output=True, text=True, env=dict(os.environ, ZK_MSM_DIRECT_CAP="1"), timeout=300)
        assert "same bytes" in r.stdout, r.stderr[-2000:]

def test_gpu_verifier_reproduces_reference_pairing_values(ref_vectors, tmp_path):
    """K9 against libff's reduced_pairing VALUES (tests/golden/ref_vectors.txt), not against another verifier: keys crafted as in tests/test_verifier_cpu.py, whose
    alpha_g1_beta_g2 is the reference's GT value of e(aG1, bG2) and whose other two pairings cancel"""
    from test_verifier_cpu import write_vk, proof_hex, H
    G1, G2 = o.g1_gen(), o.g2_gen(); neg_g2 = (G2[0], ((o.Q_MOD - G2[1][0]) % o.Q_MOD, (o.Q_MOD - G2[1][1]) % o.Q_MOD)); C = o.g1_op("mul", G1, k=77); n = 0
    for l in ref_vectors:
        if l[0] != "pairing": continue
        a, b = H(l[1].split("=")[1]), H(l[2].split("=")[1]); gt = [int(l[3].split("=")[1])] + [int(x) for x in l[4:]]; A, B = o.g1_op("mul", G1, k=a), o.g2_op("mul", G2, k=b)
        vk = str(tmp_path / ("vk%d.txt" % n)); write_vk(vk, gt, G2, neg_g2, [C]); n += 1
        assert e.verify_batch(vk, [proof_hex(A, B, C), proof_hex(o.g1_op("dbl", A), B, C), proof_hex(A, B, o.g1_op("dbl", C))], [[], [], []]) == [True, False, False]
    assert n == 3

def test_verify_batch_symbol_mixed_block(all_keys, monkeypatch, tmp_path):
    """include/zk_batch.h: one call with a block's worth of proofs — 40 send records (above the GPU threshold: one K9 launch), 3 mint and 2 redeem (host) and junk —
    decided exactly like the per-proof verify symbols"""
    monkeypatch.setenv("ZK_PRFKEY_DIR", str(all_keys)); zk = e.Zk(); items, exp = [], []
    sends = [w.send_instance(500 + i) for i in range(4)]; sp = [zk.GenSendProof(*w.send_args(d)) for d in sends]
    for i in range(40):
        d = sends[i % 4]; pr = sp[i % 4]; args = [d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]
        if i % 5 == 1: pr = pr[:200] + ("7" if pr[200] != "7" else "8") + pr[201:]
        if i % 5 == 2: args = [d["cmtA"], d["sn_old"], d["cmtS"], d["cmtA_old"]]
        items.append(("send", pr, args, 0)); exp.append(i % 5 not in (1, 2))
    for i in range(3):
        m = w.mint_instance(600 + i); pr = zk.GenMintProof(*w.mint_args(m)); items.append(("mint", pr, [m["cmtA_old"], m["sn_old"], m["cmtA"]], m["value_s"] + (1 if i == 1 else 0))); exp.append(i != 1)
    for i in range(2):
        r = w.mint_instance(700 + i, redeem=True); pr = zk.GenRedeemProof(*w.mint_args(r)); items.append(("redeem", pr, [r["cmtA_old"], r["sn_old"], r["cmtA"]], r["value_s"])); exp.append(True)
    items.append(("send", "xyz", [bytes(32)] * 4, 0)); exp.append(False); items.append((9, sp[0], [bytes(32)] * 4, 0)); exp.append(False)
    rc, ok = zk.VerifyBatch(items); assert ok == exp and rc == sum(exp)
    singles = [zk.VerifySendProof(p, *a) for k, p, a, v in items[:40]]; assert singles == exp[:40]

def test_inputs_resident_in_hbm_give_the_same_proofs(golden_dir):
    """zkgpu_prover_stash_witness / zkgpu_prover_prove_stashed (what bench.py's timed region calls: the statements of a run handed over before the clock starts and kept in
    device memory): several assignments stashed, proved in another order and more than once — the bytes of zkgpu_prover_prove on the same (z, r, s), i.e. the reference
    prover's; an unknown slot is an error, an unsatisfying stashed assignment is reported like an unsatisfying host buffer"""
    d = os.path.join(golden_dir, "groth16_small"); meta = json.load(open(os.path.join(d, "meta.json"))); z = o.load_witness(os.path.join(d, "wit.bin")); r, s = int(meta["r"], 16), int(meta["s"], 16)
    cs = o.R1CS.load(os.path.join(d, "r1cs.bin")); p = e.Prover(os.path.join(d, "pk.txt")); bad = z.copy(); bad[5] = o.to_arr([12345])[0]; assert not o.r1cs_is_satisfied(cs, bad)
    p.set_witness(z); s0 = p.stash_witness(); p.set_witness(bad); s1 = p.stash_witness(); p.set_witness(z); s2 = p.stash_witness(); assert (s0, s1, s2) == (0, 1, 2)
    for slot in (s2, s0, s0, s2): assert p.prove_stashed(slot, r, s) == meta["proof"]
    with pytest.raises(e.ZkGpuError): p.prove_stashed(s1, r, s)
    assert p.prove_stashed(s0, r, s) == meta["proof"] and p.prove(z, r, s) == meta["proof"]                   # the object keeps working
    with pytest.raises(e.ZkGpuError): p.prove_stashed(7, r, s)
    fresh = p.prove_stashed(s0); assert fresh != meta["proof"] and e.verify(os.path.join(d, "vk.txt"), fresh, o.from_arr(z[:meta["n_inputs"]]))
    # a stash is the raw vector only: slots can be dropped and are used again, the count follows, a dropped slot is an error, and the prover's own hand-over still works between
    assert p.stash_count() == 3; p.drop_stash(s1); assert p.stash_count() == 2
    with pytest.raises(e.ZkGpuError): p.prove_stashed(s1, r, s)
    with pytest.raises(e.ZkGpuError): p.drop_stash(s1)
    p.set_witness(z); assert p.stash_witness() == s1 and p.prove_stashed(s1, r, s) == meta["proof"]
    assert p.prove_resident(r, s) == meta["proof"]                                                             # (the assignment proved last: the stash, read in place)
    p.drop_stash(); assert p.stash_count() == 0; p.set_witness(z); assert p.prove_resident(r, s) == meta["proof"] and p.stash_witness() == 0; p.close()
    q = e.Prover(os.path.join(d, "pk.txt"))
    with pytest.raises(e.ZkGpuError): q.stash_witness()                                                       # nothing was handed over yet
    q.close()

def test_stashed_assignments_of_the_send_circuit_classified_on_the_device(tmp_path):
    """the tags and the list of other values of a statement resident in HBM are derived inside prove_stashed (k_classify_witness; multiexp.tcc:443-496 is part of the
    prover): full-size send statements — stashed from the compact hand-over AND from the dense one (ZK-independent: a dense upload leaves no tags behind, the stash path
    must not need any) — give the bytes of zkgpu_prover_prove for the same (r, s)"""
    import workload as w
    pk, vk = str(tmp_path / "pk.txt"), str(tmp_path / "vk.txt"); e.keygen("send", pk, vk, seed=77); p = e.Prover(pk); hx = lambda a: [("0x" + x.hex()) if isinstance(x, bytes) else x for x in a]
    zs = []
    for i in range(3):
        d = w.send_instance(40 + i); wp = str(tmp_path / ("w%d.bin" % i)); e.witness_send(*hx(w.send_args(d)), wp); zs.append(o.load_witness(wp))
    want = [p.prove(z, 1000 + i, 2000 + i) for i, z in enumerate(zs)]; slots = []
    for z in zs: p.set_witness(z); slots.append(p.stash_witness())
    for i, z in enumerate(zs): assert np.array_equal(p.read_stash(slots[i]), np.asarray(z, dtype=np.uint64).reshape(-1, 4))      # what is resident is the raw vector
    for rep in range(2):
        for i in (2, 0, 1): assert p.prove_stashed(slots[i], 1000 + i, 2000 + i) == want[i]
    assert p.prove(zs[1], 1001, 2001) == want[1] and p.prove_stashed(slots[0], 1000, 2000) == want[0]         # host buffers and stashes interleaved
    for i, z in enumerate(zs): assert np.array_equal(p.read_stash(slots[i]), np.asarray(z, dtype=np.uint64).reshape(-1, 4))      # ... and proofs leave it as it was (send folds nothing)
    bad = zs[0].copy(); bad[300000 % len(bad)] = o.to_arr([3])[0]; p.set_witness(bad); sb = p.stash_witness()
    with pytest.raises(e.ZkGpuError, match="constraint [0-9]+ among"): p.prove_stashed(sb, 1, 2)                # the error names a violated constraint
    assert p.prove_stashed(slots[2], 1002, 2002) == want[2]; p.close()

def test_key_container_gives_the_same_prover(tmp_path):
    """the first load of a text key leaves <key>.gpucache behind (post-transform tables as raw aligned arrays); the next load maps it instead of parsing 77 MB
    of text — same proof bytes, a fraction of the time; a container whose key file changed is ignored and rebuilt"""
    import time, ctypes
    pk_path, vk_path, wp = str(tmp_path / "sendpk.txt"), str(tmp_path / "sendvk.txt"), str(tmp_path / "w.bin"); e.keygen("send", pk_path, vk_path, seed=0xC0FFEE)
    d = w.send_instance(77); e.witness_send(*hexargs(w.send_args(d)), wp); z = o.load_witness(wp); L = e.lib()
    assert L.zkgpu_key_container_valid(pk_path.encode()) == 0
    t0 = time.time(); p = e.Prover(pk_path); t_text = time.time() - t0; a = p.prove(z, 11, 22); p.close(); assert L.zkgpu_key_container_valid(pk_path.encode()) == 1
    t0 = time.time(); p = e.Prover(pk_path); t_cont = time.time() - t0; b = p.prove(z, 11, 22); p.close()
    print("key load: %.3f s from text, %.3f s from the container (%d MB)" % (t_text, t_cont, os.path.getsize(pk_path + ".gpucache") >> 20)); record_leg("send key load from text / container", None); record_leg("  text %.2f s, container %.2f s" % (t_text, t_cont), None)
    assert a == b and e.verify(vk_path, a, w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]])) and t_cont < 0.6 * t_text
    e.keygen("send", pk_path, vk_path, seed=0xC0FFEF)                                   # a different key at the same path: the old container must not be used
    assert L.zkgpu_key_container_valid(pk_path.encode()) == 0
    p = e.Prover(pk_path); c = p.prove(z, 11, 22); p.close(); assert c != a and e.verify(vk_path, c, w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]))

def test_key_generation_executables(tmp_path):
    """the reference's send_key / mint_key (src/X/getpvk.cpp:41-51): write Xpk.txt / Xvk.txt into the directory; the files load and prove"""
    exe = os.path.join(ROOT, "blockmaze_amd", "bin", "mint_key"); r = subprocess.run([exe], cwd=str(tmp_path), capture_output=True, text=True, env=dict(os.environ, ZK_KEY_SEED="77")); assert r.returncode == 0, r.stderr
    pk, vk = str(tmp_path / "mintpk.txt"), str(tmp_path / "mintvk.txt"); assert os.path.getsize(pk) > 40e6 and os.path.getsize(vk) > 1000
    m = w.mint_instance(9); wp = str(tmp_path / "w.bin"); e.witness_mint_redeem(False, *hexargs(w.mint_args(m)), wp); p = e.Prover(pk); proof = p.prove(o.load_witness(wp)); p.close()
    assert e.verify(vk, proof, w.pack_public([m["cmtA_old"], m["sn_old"], m["cmtA"]], m["value_s"]))

def test_equal_columns_are_folded_and_never_send_an_msm_to_the_general_path(tmp_path):
    """Variables whose columns coincide in A, B and C have equal points in every query; when both hold the same value other than 0 / 1 the two equal points used to meet in an
    incomplete addition now and then (ZZ = 0: the MSM repeated on the general path — 3 of 57,600 mixed proofs in round 5).  The prover folds such groups into one place at the
    head of every proof (k_merge_equal_columns): an equivalent assignment.  Mint (the circuit has such a pair): the pair's sum split into two EQUAL halves — every digit of the two
    scalars the same, the worst case — gives, for the same (r, s), the bytes of the untouched witness's proof, through the host buffer, the board's tags (cgo path: a real
    statement) and a stash, and no MSM is repeated; ZK_MERGE_EQUAL_COLUMNS=0 is the old behaviour (same bytes, by way of the general path or not)"""
    import workload as w
    pk, vk = str(tmp_path / "mintpk.txt"), str(tmp_path / "mintvk.txt"); e.keygen("mint", pk, vk, seed=4242); rpath = str(tmp_path / "mint.bin"); e.circuit_export("mint", rpath)
    groups = e.equal_columns(rpath); assert groups; a, b = groups[0][:2]
    m = w.mint_instance(3); hx = lambda x: [("0x" + v.hex()) if isinstance(v, bytes) else v for v in x]; wp = str(tmp_path / "w.bin"); e.witness_mint_redeem(False, *hx(w.mint_args(m)), wp); z = o.load_witness(wp)
    p = e.Prover(pk); assert p.equal_column_groups() == len(groups)
    r, s = 0x1234567, 0x7654321; want = p.prove(z, r, s); assert e.verify(vk, want, w.pack_public([m["cmtA_old"], m["sn_old"], m["cmtA"]], m["value_s"]))
    za, zb = o.from_arr(z[a - 1:a])[0], o.from_arr(z[b - 1:b])[0]; tot = (za + zb) % o.R_MOD; half = tot * pow(2, o.R_MOD - 2, o.R_MOD) % o.R_MOD; assert half > 1
    z2 = z.copy(); z2[a - 1] = o.to_arr([half])[0]; z2[b - 1] = o.to_arr([half])[0]
    before = e.general_path_repeats()
    for rep in range(6): assert p.prove(z2, r, s) == want
    p.set_witness(z2); slot = p.stash_witness()
    for rep in range(6): assert p.prove_stashed(slot, r, s) == want
    z3 = z.copy(); z3[a - 1] = o.to_arr([tot])[0]; z3[b - 1] = o.to_arr([0])[0]; assert p.prove(z3, r, s) == want          # (what the fold leaves, handed over as such)
    assert e.general_path_repeats() == before; p.close()

def test_no_proof_is_lost_when_witnesses_are_generated_on_several_threads(all_keys):
    """Witness generation fills a statement's SHA-256 compressions in side by side on a helper pool (one wave since round 6).  Its first version wrote a compression's output
    bits a second time while later compressions were reading them, and one proof in a thousand came back as the failure sentinel.  A soak through the cgo symbols, one caller and
    two at once, all four circuits interleaved: every proof is generated (a fresh process: the pool's size is read once) and a sample of each kind verifies."""
    code = """
import os, sys, threading
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))
from blockmaze_amd import engine as e
import workload as w
zk = e.Zk(); ss = [w.send_instance(500 + i) for i in range(8)]; ms = [w.mint_instance(500 + i) for i in range(4)]; rs = [w.mint_instance(500 + i, redeem=True) for i in range(4)]; ds = [w.deposit_instance(i) for i in range(2)]
lost = []; keep = {}
def run(k, n):
    for i in range(n):
        j = i + 3 * k; s = ss[j %% 8]; p = zk.GenSendProof(*w.send_args(s)); keep[('send', k)] = (p, s)
        if len(p) != 512 or p.startswith('0000000000'): lost.append(('send', k, i))
        if i %% 4 == 0:
            m = ms[j %% 4]; p = zk.GenMintProof(*w.mint_args(m)); keep[('mint', k)] = (p, m)
            if p.startswith('0000000000'): lost.append(('mint', k, i))
            r = rs[j %% 4]; p = zk.GenRedeemProof(*w.mint_args(r)); keep[('redeem', k)] = (p, r)
            if p.startswith('0000000000'): lost.append(('redeem', k, i))
        if i %% 8 == 0:
            d = ds[j %% 2]; p = zk.GenDepositProof(*w.deposit_args(d), d['leaves'], d['rt'], d['sk']); keep[('deposit', k)] = (p, d)
            if p.startswith('0000000000'): lost.append(('deposit', k, i))
run(0, 1200)
ths = [threading.Thread(target=run, args=(k, 900)) for k in (1, 2)]
for t in ths: t.start()
for t in ths: t.join()
ok = True
for (kind, k), (p, d) in keep.items():
    if kind == 'send': ok &= zk.VerifySendProof(p, d['cmtA_old'], d['sn_old'], d['cmtS'], d['cmtA'])
    elif kind == 'deposit': ok &= zk.VerifyDepositProof(p, d['rt'], d['pk_recv'], d['cmtB_old'], d['sn_old'], d['cmtB'], d['sn_s'])
    elif kind == 'mint': ok &= zk.VerifyMintProof(p, d['cmtA_old'], d['sn_old'], d['cmtA'], d['value_s'])
    else: ok &= zk.VerifyRedeemProof(p, d['cmtA_old'], d['sn_old'], d['cmtA'], d['value_s'])
print('SOAK lost', len(lost), lost[:5], 'verified', ok, 'general-path repeats', e.general_path_repeats())
""" % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, ZK_PRFKEY_DIR=str(all_keys)), timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("SOAK ")]; assert line, (r.stdout[-500:], r.stderr[-1500:])
    assert line[0].startswith("SOAK lost 0 [] verified True general-path repeats 0"), line[0]

def test_hand_over_takes_the_dense_path_on_its_own_for_a_random_assignment(tmp_path):
    """Prover::set_witness: an assignment with more than a quarter of its entries neither 0 nor 1 overruns the compact form's value area — noticed by the chunk whose
    reservation ends past it (groth16_prover.cpp: the scan's shared cursor) — and goes up as a plain copy instead.  No BlockMaze circuit does that (ZK_WITNESS_DENSE forces the
    same branch for them); a random R1CS of 40,000 variables does, on the threaded scan (625 words).  Proof bytes = the oracle's; a second system takes the
    plain-copy path again with a ragged last word (33,001 entries), each proved twice by one prover object: the same."""
    from r1cs_util import random_r1cs
    for seed, nv, nc in ((77, 40000, 30000), (78, 33000, 24000)):         # (fewer constraints than variables, no full-width coefficients: the device keeps at most 2,048 distinct ones)
        cs, z = random_r1cs(seed, 6, nv, nc, small_frac=0.8); others = int(np.count_nonzero((z[:, 1:] != 0).any(axis=1) | (z[:, 0] > 1)))
        assert others > (nv + 1) // 4                                                 # dense enough to overrun the value area
        d = tmp_path / ("s%d" % seed); d.mkdir(); cs.save(str(d / "r1cs.bin")); pk_path, vk_path = str(d / "pk.txt"), str(d / "vk.txt")
        e.keygen_from_r1cs(str(d / "r1cs.bin"), pk_path, vk_path, seed=seed)
        pk, cs_key = o.parse_pk(pk_path); g = o.SplitMix64(seed); r, s = g.field(), g.field(); exp = o.proof_hex(o.prove(cs_key, z, pk, r, s))
        p = e.Prover(pk_path); got = p.prove(z, r, s); again = p.prove(z, r, s); p.close(); assert got == exp and again == exp
        assert e.verify(vk_path, got, o.from_arr(z[:cs.n_inputs]))
