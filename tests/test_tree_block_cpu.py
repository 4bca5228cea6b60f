"""A block against the resident tree without a device (include/zk_tree_block.h, DESIGN.md "A block against the resident tree"): the header compiles as C and as
C++, verifyBlockTree and zkgpu_tree_match_roots are exported by libzkgpu.so and by nothing else, a process that sees no device gets verifyBlockState's answer for
tree = NULL and a loud failure from the anchor entry — the tree has no host model —, and the Python model of the anchor step that tests/test_gpu_tree_match.py and
tests/test_gpu_tree_block.py compare the device with (the root of every PREFIX of the leaf list, by model_levels) is pinned to tests/workload.py."""
import functools, os, random, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import workload as w

BLOCK_ENGINE = ["zkgpu_tree_match_roots"]
BLOCK_DROPIN = ["verifyBlockTree"]

# ---- the model of the anchor step: model_levels / model_root of tests/test_gpu_commitment_tree.py, restated over prefixes ---------------------------------------
comp = functools.lru_cache(maxsize=None)(w._sha256_compress)   # (the prefixes of one leaf list share almost all of their nodes)
def model_levels(leaves_blob, depth):
    """every level of the Python model's tree: levels[k] = nodes of level k in blob order, empty[k] = empty root of level k"""
    levels = [list(leaves_blob)]; empty = [bytes(32)]
    for d in range(depth):
        cur = levels[-1]; levels.append([comp(cur[i] + (cur[i + 1] if i + 1 < len(cur) else empty[d])) for i in range(0, len(cur), 2)])
        empty.append(comp(empty[d] + empty[d]))
    return levels, empty
def model_root(levels, empty, depth): return levels[depth][0] if levels[depth] else empty[depth]
def seeded_leaves(n, seed):
    rng = random.Random(seed); return [rng.getrandbits(256).to_bytes(32, "little") for _ in range(n)]

class PrefixRoots:
    """root(m) = the root of the tree of depth `depth` over leaves[:m], in blob order; each size is computed once"""
    def __init__(self, leaves_blob, depth): self.leaves = list(leaves_blob); self.depth = depth; self.known = {}
    def root(self, m):
        assert 0 <= m <= len(self.leaves)
        if m not in self.known: self.known[m] = model_root(*model_levels(self.leaves[:m], self.depth), self.depth)
        return self.known[m]
def model_match(prefix_roots, sizes, rts_blob):
    """the anchor step: for every RT (32 bytes, blob order) the lowest a with root(sizes[a]) == RT, or -1"""
    first = {}
    for a, m in enumerate(sizes): first.setdefault(prefix_roots.root(m), a)
    return [first.get(bytes(rt), -1) for rt in rts_blob]

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

@pytest.mark.parametrize("depth", [1, 3, 8])
def test_anchor_model_agrees_with_workload_on_every_prefix(depth):
    """every prefix of a 20-leaf list (at depths 1 and 3 more leaves than a tree holds: both models then agree on the first 2^depth, which is all either looks at)"""
    leaves = seeded_leaves(20, 170 + depth); pr = PrefixRoots(leaves, depth); n = len(leaves); roots = []
    for m in range(n + 1):
        rt, _ = w.merkle_root_and_path([w.rev(x) for x in leaves[:m]], 0, depth); roots.append(w.rev(rt)); assert pr.root(m) == roots[m], (depth, m)
    assert len(set(roots[:(1 << depth) + 1])) == min(n, 1 << depth) + 1
    sizes = [n, 0, 3, n, 0, 1, 2]; rts = roots + [bytes(32), roots[1][:31] + bytes([roots[1][31] ^ 1]), bytes([roots[1][0] ^ 1]) + roots[1][1:], w.rev(roots[n])]
    want = [next((a for a, m in enumerate(sizes) if roots[m] == rt), -1) for rt in rts]; assert want[-4:] == [-1] * 4 and want[0] == 1 and want[1] == 5
    assert model_match(pr, sizes, rts) == want and model_match(pr, [], rts) == [-1] * len(rts) and model_match(pr, sizes, []) == []

def defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l)

def test_block_symbols_exported_by_libzkgpu_only(e):
    L = e.lib()
    for s in BLOCK_ENGINE + BLOCK_DROPIN: getattr(L, s)                                                   # (AttributeError: the symbol is not there)
    have = defined(e.LIB_PATH)
    for s in BLOCK_ENGINE + BLOCK_DROPIN: assert s in have, s
    from test_abi_exports import SYMS, declared_symbols
    assert sorted(declared_symbols("zk_tree_block.h")) == sorted(BLOCK_DROPIN)
    for s in BLOCK_ENGINE: assert s in declared_symbols("zkgpu.h"), s
    for h in ("zk_tree.h", "zk_tree_states.h", "zk_spent.h", "zk_spent_pk.h", "zk_proof_cache.h"): assert not set(declared_symbols(h)) & set(BLOCK_DROPIN), h
    for lib, syms in SYMS.items():                                                                         # the four thin libraries: unchanged
        assert defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)) == sorted(syms), lib
        assert not set(syms) & set(BLOCK_ENGINE + BLOCK_DROPIN), lib

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++11")])
def test_block_header_compiles_as_c_and_cxx_when_included_twice(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_tree_block.h"\n#include "zk_tree_block.h"\n'
                   'int main(void) { long long anchors[2] = {0, 0}, set_size = 0, tree_size = 0; unsigned char ok[1]; int32_t of[1]; zk_tree *t = zkTreeNew(8);\n'
                   '  if (t) { (void)verifyBlockTree(0, 0, 0, t, anchors, 2, 0, 0, ok, of, &set_size, &tree_size); zkTreeFree(t); } return 0; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

NO_DEVICE = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from blockmaze_amd import engine as e
import block_records as br
L = e.lib(); assert e.device_count() == 0
recs = np.concatenate([br.random_records(k, 3, 50 + k) for k in range(4)] + [br.random_records(9, 2, 60)]); n = len(recs); ptr = recs.ctypes.data_as(ctypes.c_void_p)
def state(recs_ptr, count):
    ok = (ctypes.c_ubyte * max(1, count))(*([1] * max(1, count))); size = ctypes.c_longlong(-7)
    return L.verifyBlockState(None, recs_ptr, count, None, None, None, 0, ok, ctypes.byref(size)), list(ok)[:count], size.value
def tree(recs_ptr, count, commit=0):
    ok = (ctypes.c_ubyte * max(1, count))(*([1] * max(1, count))); of = (ctypes.c_int32 * max(1, count))(*([5] * max(1, count))); size = ctypes.c_longlong(-7); tsize = ctypes.c_longlong(-7)
    rc = L.verifyBlockTree(None, recs_ptr, count, None, None, 0, None, commit, ok, of, ctypes.byref(size), ctypes.byref(tsize))
    return (rc, list(ok)[:count], size.value), list(of)[:count], tsize.value
# every kind and an unknown one: no record survives the host road (random proofs; this process has no key either), and the two entries say the same
want = state(ptr, n); got, of, tsize = tree(ptr, n); assert got == want and want[1] == [0] * n and want[0] <= 0 and of == [-1] * n and tsize == -1, (want, got, of, tsize)
got, of, tsize = tree(ptr, n, 1); assert got == want and of == [-1] * n and tsize == -1
# unknown kinds alone need no key: decided, all rejected
unk = br.random_records(9, 4, 61); uptr = unk.ctypes.data_as(ctypes.c_void_p)
want = state(uptr, 4); got, of, tsize = tree(uptr, 4); assert want == (0, [0] * 4, -7) and got == want and of == [-1] * 4 and tsize == -1, (want, got)
assert tree(None, 0)[0] == state(None, 0) == (0, [], -7) and tree(None, -1)[0][0] == state(None, -1)[0] == -1
z = e.Zk(); assert z.VerifyBlockTree(None, unk, None, None, None, False) == (0, [False] * 4, [-1] * 4, None, None)
# the anchor entry: no device, no answer, nothing written
out = (ctypes.c_int32 * 2)(7, 7); sizes = (ctypes.c_uint64 * 2)(0, 0)
assert L.zkgpu_tree_match_roots(None, sizes, ctypes.c_size_t(2), bytes(64), ctypes.c_size_t(2), 0, out) == -1 and b"no HIP device" in L.zkgpu_last_error() and list(out) == [7, 7]   # ZKGPU_ERR_NO_DEVICE
assert L.zkgpu_tree_match_roots(None, None, ctypes.c_size_t(0), None, ctypes.c_size_t(0), 1, None) == -1
try: e.Tree(5); raise SystemExit("a tree without a device")
except e.ZkGpuError: pass
print("NO DEVICE OK")
"""

def test_entries_without_a_device(e, tmp_path):
    """a process that sees no device: tree = NULL is verifyBlockState, anchor_of all -1 and *tree_size_out = -1; zkgpu_tree_match_roots fails with ZKGPU_ERR_NO_DEVICE"""
    script = tmp_path / "no_device.py"; script.write_text(NO_DEVICE); keys = tmp_path / "keys"; keys.mkdir()
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ZK_PRFKEY_DIR=str(keys)))
    assert r.returncode == 0 and "NO DEVICE OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
