"""Past states of the resident commitment tree without a device (include/zk_tree_states.h, DESIGN.md "Past states of the commitment tree"): the new symbols are
exported by libzkgpu.so and by nothing else, the header compiles as C and as C++, every new entry fails loudly without a HIP device — there is no host tree — and
the rule the kernels of gpu_tree.hip implement (edge walk, sibling choice, rewind) is restated here in Python and checked against this file's model_levels for
every size and every index, which pins what tests/test_gpu_tree_states.py expects to tests/workload.py."""
import ctypes, functools, os, random, subprocess
import pytest
import workload as w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES_ENGINE = ["zkgpu_tree_roots_at", "zkgpu_tree_paths_at", "zkgpu_tree_find_at", "zkgpu_tree_rewind", "zkgpu_test_tree_state_launches"]
STATES_DROPIN = ["zkTreeRootAt", "zkTreeRootsAt", "zkTreeRewind", "genDepositproofTreeAt"]

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

comp = functools.lru_cache(maxsize=None)(w._sha256_compress)   # (the prefixes of one leaf list share almost all of their nodes)
def model_levels(leaves_blob, depth):
    """every level of the Python model's tree (workload.merkle_root_and_path rebuilds it per call): levels[k] = nodes of level k in blob order, empty[k] = empty root"""
    levels = [list(leaves_blob)]; empty = [bytes(32)]
    for d in range(depth):
        cur = levels[-1]; nxt = [comp(cur[i] + (cur[i + 1] if i + 1 < len(cur) else empty[d])) for i in range(0, len(cur), 2)]
        empty.append(comp(empty[d] + empty[d])); levels.append(nxt)
    return levels, empty
def model_root(levels, empty, depth): return levels[depth][0] if levels[depth] else empty[depth]
def model_path(levels, empty, depth, index): return [levels[k][(index >> k) ^ 1] if ((index >> k) ^ 1) < len(levels[k]) else empty[k] for k in range(depth)]
def seeded_leaves(n, seed):
    rng = random.Random(seed); return [rng.getrandbits(256).to_bytes(32, "little") for _ in range(n)]

# ---- the rule, as gpu_tree.hip states it: tree_edge_walk, k_tree_paths_at's choice of sibling, k_tree_rewind -------------------------------------------------
def edge_walk(stored, empty, depth, m):
    """B[k] = node (m - 1) >> k of level k in state m, from the stored nodes of a tree that holds at least m leaves"""
    B = [stored[0][m - 1]]
    for k in range(1, depth + 1):
        j = (m - 1) >> (k - 1); B.append(comp(stored[k - 1][j - 1] + B[-1]) if j & 1 else comp(B[-1] + empty[k - 1]))
    return B
def sibling_at(stored, empty, B, m, i, k):
    s = (i >> k) ^ 1
    if (s + 1) << k <= m: return stored[k][s]
    if s << k >= m: return empty[k]
    assert s == (m - 1) >> k; return B[k]

def test_model_levels_agree_with_workload():
    for depth, n in [(1, 2), (3, 5), (8, 17)]:
        leaves = seeded_leaves(n, 3 * depth + n); lv, em = model_levels(leaves, depth)
        for idx in range(n):
            rt, sibs = w.merkle_root_and_path([w.rev(x) for x in leaves], idx, depth)
            assert w.rev(rt) == model_root(lv, em, depth) and [w.rev(s) for s in sibs] == model_path(lv, em, depth, idx), (depth, n, idx)

@pytest.mark.parametrize("depth", [1, 2, 3, 8])
def test_rule_against_the_model_of_every_prefix(depth):
    n = 1 << depth; leaves = seeded_leaves(n, 900 + depth); stored, empty = model_levels(leaves, depth)
    for m in range(1, n + 1):
        lv, em = model_levels(leaves[:m], depth); B = edge_walk(stored, empty, depth, m)
        assert B[depth] == model_root(lv, em, depth), (depth, m)
        for k in range(depth + 1):
            assert B[k] == lv[k][(m - 1) >> k], (depth, m, k)                                            # B_k is the last node of level k in state m
            if m % (1 << k) == 0: assert stored[k][(m - 1) >> k] == B[k], (depth, m, k)                  # where 2^k divides m the stored node is B_k already
        for i in range(m):
            assert [sibling_at(stored, empty, B, m, i, k) for k in range(depth)] == model_path(lv, em, depth, i), (depth, m, i)
        # rewind to m: B_k written to stored[k][j_k] and nothing else; every node below the counts then holds its value in state m
        after = [list(x) for x in stored]
        for k in range(1, depth + 1): after[k][(m - 1) >> k] = B[k]
        for k in range(depth + 1): assert after[k][:len(lv[k])] == lv[k], (depth, m, k)

def defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l)

def test_state_symbols_exported_by_libzkgpu_only(e):
    have = defined(e.LIB_PATH)
    for s in STATES_ENGINE + STATES_DROPIN: assert s in have, s
    from test_abi_exports import SYMS, declared_symbols
    assert sorted(declared_symbols("zk_tree_states.h")) == sorted(STATES_DROPIN)
    for s in STATES_ENGINE: assert s in declared_symbols("zkgpu.h"), s
    for lib, syms in SYMS.items():                                                                         # the four thin libraries: unchanged
        assert defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)) == sorted(syms), lib
        assert not set(declared_symbols(lib + ".h") + declared_symbols("zk_common.h")) & set(STATES_DROPIN), lib

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")])
def test_states_header_compiles_as_c_and_cxx(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_tree_states.h"\n#include "zk_tree_states.h"\n'
                   'int main(void) { zk_tree *t = zkTreeNew(8); long long s[2] = {0, 0}; uint8_t r[64]; char rt[65]; (void)rt;\n'
                   '  if (t) { char *h = zkTreeRootAt(t, 0); (void)h; (void)zkTreeRootsAt(t, s, 2, r); (void)zkTreeRewind(t, 0); zkTreeFree(t); } return 0; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

def test_no_device_no_past_states(e, tmp_path, monkeypatch):
    import torch
    if torch.cuda.is_available(): pytest.skip("GPU present")
    L = e.lib(); n = ctypes.c_uint64(7); sizes = (ctypes.c_uint64 * 2)(0, 0); buf = ctypes.create_string_buffer(32 * 32); before = buf.raw
    for rc in (L.zkgpu_tree_roots_at(None, sizes, ctypes.c_size_t(2), buf), L.zkgpu_tree_paths_at(None, ctypes.c_uint64(0), sizes, ctypes.c_size_t(0), buf, buf),
               L.zkgpu_tree_find_at(None, ctypes.c_uint64(1), buf, ctypes.byref(n)), L.zkgpu_tree_rewind(None, ctypes.c_uint64(0)),
               L.zkgpu_test_tree_state_launches(None, ctypes.byref(n))):
        assert rc == -1 and b"no HIP device" in L.zkgpu_last_error()                                      # ZKGPU_ERR_NO_DEVICE
    assert buf.raw == before and n.value == 7
    monkeypatch.setenv("ZK_PRFKEY_DIR", str(tmp_path)); z = e.Zk(); d = w.deposit_instance(0)
    assert z.L.zkTreeRootAt(None, ctypes.c_longlong(0)) is None and z.TreeRootAt(None, 0) is None and z.TreeRewind(None, 0) == -1 and z.TreeRootsAt(None, [0, 0]) is None
    proof, rt = z.GenDepositProofTreeAt(*w.deposit_args(d), d["sk"], None, 1)
    assert len(proof) == 512 and proof.startswith("0" * 10) and rt is None                                 # the reference's sentinel, rt_out empty
    assert proof == z.GenDepositProof(*w.deposit_args(d), d["leaves"], d["rt"], d["sk"])                   # the very sentinel genDepositproof gives

def test_sanitize_target_still_builds():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "blockmaze_amd", "csrc"), "-j8", "sanitize"], stdout=subprocess.DEVNULL)
