"""The resident commitment tree without a device: the host model of the tree (zkgpu_test_tree_host = notes.cpp's tree_levels, what the large GPU legs of
tests/test_gpu_commitment_tree.py compare against) equals the Python model of tests/workload.py in root and path; the new symbols are exported by libzkgpu.so and
by nothing else; include/zk_tree.h compiles as C and as C++; and without a HIP device every tree entry fails loudly — there is no host fallback tree."""
import ctypes, os, random, subprocess
import pytest
import workload as w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_ENGINE = ["zkgpu_tree_create", "zkgpu_tree_destroy", "zkgpu_tree_append", "zkgpu_tree_size", "zkgpu_tree_root", "zkgpu_tree_path", "zkgpu_tree_find", "zkgpu_test_tree_host"]
TREE_DROPIN = ["zkTreeNew", "zkTreeFree", "zkTreeAppend", "zkTreeRoot", "genDepositproofTree", "verifyDepositproofDepth"]
GOLDEN_ROOTS = {0: "8eb3c27b218349e6b9b6037b8042f3751ee820e8a0319a1bda439b247456088c", 1: "a19a0d1fac447f65d273d5831827ccfa96c193a1b39618a23d11628d48e27a9e",
                16: "2630f036430a646118dbb95ba55e9e3803e35a680398d01f9942513ebbb7911e"}   # genRoot over 0, 1 and 16 leaves (tests/test_abi_exports.py)

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

def model_levels(leaves_blob, depth):
    """every level of the Python model's tree (workload.merkle_root_and_path rebuilds it per call): levels[k] = nodes of level k in blob order, empty[k] = empty root"""
    levels = [list(leaves_blob)]; empty = [bytes(32)]
    for d in range(depth):
        cur = levels[-1]; nxt = [w._sha256_compress(cur[i] + (cur[i + 1] if i + 1 < len(cur) else empty[d])) for i in range(0, len(cur), 2)]
        empty.append(w._sha256_compress(empty[d] + empty[d])); levels.append(nxt)
    return levels, empty
def model_root(levels, empty, depth): return levels[depth][0] if levels[depth] else empty[depth]
def model_path(levels, empty, depth, index): return [levels[k][(index >> k) ^ 1] if ((index >> k) ^ 1) < len(levels[k]) else empty[k] for k in range(depth)]
def seeded_leaves(n, seed):
    rng = random.Random(seed); return [rng.getrandbits(256).to_bytes(32, "little") for _ in range(n)]

def test_model_levels_agree_with_workload():
    """the cached-levels helper of this file against workload.merkle_root_and_path itself (big-endian in, big-endian out)"""
    for depth, n in [(1, 2), (2, 3), (8, 17), (32, 5)]:
        leaves = seeded_leaves(n, 7 * depth + n); lv, em = model_levels(leaves, depth)
        for idx in range(n):
            rt, sibs = w.merkle_root_and_path([w.rev(x) for x in leaves], idx, depth)
            assert w.rev(rt) == model_root(lv, em, depth) and [w.rev(s) for s in sibs] == model_path(lv, em, depth, idx), (depth, n, idx)

@pytest.mark.parametrize("depth", [1, 2, 8, 32])
def test_host_tree_equals_python_model(e, depth):
    for n in [0, 1, 2, 3, 5, 16, 17, 255, 256]:
        if n > (1 << depth): continue
        leaves = seeded_leaves(n, 1000 * depth + n); lv, em = model_levels(leaves, depth)
        root, _ = e.tree_host(depth, leaves)
        assert root == model_root(lv, em, depth), (depth, n)
        for idx in sorted(set([0, 1, n // 2, n - 2, n - 1]) & set(range(n))):
            r2, path = e.tree_host(depth, leaves, idx)
            assert r2 == root and path == model_path(lv, em, depth, idx), (depth, n, idx)
            rt, sibs = w.merkle_root_and_path([w.rev(x) for x in leaves], idx, depth)                     # and the helper the issue names, as it stands
            assert w.rev(rt) == root and [w.rev(s) for s in sibs] == path, (depth, n, idx)

def test_host_tree_rejects_bad_arguments(e):
    leaves = seeded_leaves(3, 5)
    for depth, lv, idx in [(0, leaves, None), (33, leaves, None), (1, leaves, None), (8, leaves, 3)]:
        with pytest.raises(e.ZkGpuError): e.tree_host(depth, lv, idx)

def test_host_roots_at_depth_8_are_the_genroot_goldens(e):
    """the leaves of the SURVEY §8c goldens as tests/dropin_driver.c builds them: none, the number 1, the sixteen leaves of the reference's deposit fixture"""
    z = e.Zk(); sixteen = w.reference_deposit_fixture()["leaves"]
    for n, want in GOLDEN_ROOTS.items():
        cm = sixteen[:n] if n != 1 else [(1).to_bytes(32, "big")]
        assert z.GenRT(cm).hex() == want, n                                                                # (the driver's leaves: pins this test's reading of them)
        root, _ = e.tree_host(8, [w.rev(c) for c in cm]); assert w.rev(root).hex() == want, n

def defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l)

def test_tree_symbols_exported_by_libzkgpu_only(e):
    have = defined(e.LIB_PATH)
    for s in TREE_ENGINE + TREE_DROPIN: assert s in have, s
    from test_abi_exports import SYMS, declared_symbols
    assert sorted(declared_symbols("zk_tree.h")) == sorted(TREE_DROPIN)
    for s in TREE_ENGINE: assert s in declared_symbols("zkgpu.h"), s
    for lib, syms in SYMS.items():                                                                         # the four thin libraries: unchanged
        assert defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)) == sorted(syms), lib
        assert not set(declared_symbols(lib + ".h") + declared_symbols("zk_common.h")) & set(TREE_DROPIN), lib

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")])
def test_tree_header_compiles_as_c_and_cxx(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_tree.h"\n#include "zk_tree.h"\nint main(void) { zk_tree *t = zkTreeNew(8); char rt[65]; (void)rt; if (t) zkTreeFree(t); return 0; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

def test_no_device_no_tree(e, tmp_path, monkeypatch):
    import torch
    if torch.cuda.is_available(): pytest.skip("GPU present")
    L = e.lib(); L.zkgpu_tree_create.restype = ctypes.c_void_p
    assert L.zkgpu_tree_create(8) is None and b"no HIP device" in L.zkgpu_last_error()
    with pytest.raises(e.ZkGpuError, match="no HIP device"): e.Tree(32)
    n = ctypes.c_uint64(7); buf = ctypes.create_string_buffer(32 * 32)
    for rc in (L.zkgpu_tree_append(None, buf, ctypes.c_size_t(1)), L.zkgpu_tree_size(None, ctypes.byref(n)), L.zkgpu_tree_root(None, buf), L.zkgpu_tree_path(None, ctypes.c_uint64(0), buf),
               L.zkgpu_tree_find(None, buf, ctypes.byref(n))):
        assert rc == -1 and b"no HIP device" in L.zkgpu_last_error()                                      # ZKGPU_ERR_NO_DEVICE
    monkeypatch.setenv("ZK_PRFKEY_DIR", str(tmp_path)); z = e.Zk(); d = w.deposit_instance(0)
    assert z.L.zkTreeNew(8) is None and z.TreeAppend(None, [d["cmtS"]]) == -1 and z.L.zkTreeRoot(None) is None
    proof, rt = z.GenDepositProofTree(*w.deposit_args(d), d["sk"], None)
    assert len(proof) == 512 and proof.startswith("0" * 10) and rt is None                                 # the reference's sentinel, rt_out empty
    assert proof == z.GenDepositProof(*w.deposit_args(d), d["leaves"], d["rt"], d["sk"])                   # the very sentinel genDepositproof gives
    for depth in (8, 32, 0, 33): assert z.VerifyDepositProofDepth(depth, proof, d["rt"], d["pk_recv"], d["cmtB_old"], d["sn_old"], d["cmtB"], d["sn_s"]) is False   # no key file there

def test_sanitize_target_still_builds():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "blockmaze_amd", "csrc"), "-j8", "sanitize"], stdout=subprocess.DEVNULL)

def test_key_cli_depth_argument(e, tmp_path):
    """deposit_key <depth> [dir]: the depth is for the deposit circuit and lies in 1..32; the files are named after it (deposit32pk.txt) — without a device the generator
    itself fails, and says for which file"""
    exe = lambda k: os.path.join(ROOT, "blockmaze_amd", "bin", k + "_key")
    run = lambda *a: subprocess.run(list(a), capture_output=True, text=True, env=dict(os.environ, ZK_KEY_SEED="5"))
    assert run(exe("deposit"), "33", str(tmp_path)).returncode == 2 and run(exe("deposit"), "0").returncode == 2 and run(exe("mint"), "8", str(tmp_path)).returncode == 2
    import torch
    if not torch.cuda.is_available():
        r = run(exe("deposit"), "32", str(tmp_path)); assert r.returncode == 1 and "no HIP device" in r.stderr and not os.path.exists(tmp_path / "deposit32pk.txt")
