"""The commitment tree resident in HBM (blockmaze_amd/csrc/gpu_tree.hip) and the deposit entry points that prove and verify against it (include/zk_tree.h).

Small trees are checked node for node against the Python model of tests/workload.py, the 2^20-leaf tree against the library's host model (zkgpu_test_tree_host =
notes.cpp's tree_levels, itself pinned to the Python model by tests/test_commitment_tree_cpu.py).  Every leg runs in a process of its own under a time limit:
`python tests/test_gpu_commitment_tree.py <leg> <scratch dir>` is what each test starts."""
import os, random, subprocess, sys, threading, time
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import workload as w

pytestmark = pytest.mark.gpu
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
TILE = 512                       # gpu_tree.hip: TREE_TILE, the nodes of a level one workgroup takes; it carries them 9 levels up, so the next tiling is of level 9
GOLDEN_ROOTS = {0: "8eb3c27b218349e6b9b6037b8042f3751ee820e8a0319a1bda439b247456088c", 1: "a19a0d1fac447f65d273d5831827ccfa96c193a1b39618a23d11628d48e27a9e",
                16: "2630f036430a646118dbb95ba55e9e3803e35a680398d01f9942513ebbb7911e"}   # genRoot over 0, 1 and 16 leaves (tests/test_abi_exports.py)

def model_levels(leaves_blob, depth):
    """every level of the Python model's tree (workload.merkle_root_and_path rebuilds it per call): levels[k] in blob order, empty[k] = empty root of level k"""
    levels = [list(leaves_blob)]; empty = [bytes(32)]
    for d in range(depth):
        cur = levels[-1]; levels.append([w._sha256_compress(cur[i] + (cur[i + 1] if i + 1 < len(cur) else empty[d])) for i in range(0, len(cur), 2)])
        empty.append(w._sha256_compress(empty[d] + empty[d]))
    return levels, empty
def model_root(levels, empty, depth): return levels[depth][0] if levels[depth] else empty[depth]
def model_path(levels, empty, depth, index): return [levels[k][(index >> k) ^ 1] if ((index >> k) ^ 1) < len(levels[k]) else empty[k] for k in range(depth)]
def seeded_leaves(n, seed):
    rng = random.Random(seed); return [rng.getrandbits(256).to_bytes(32, "little") for _ in range(n)]
def dep_public(d, rt): return [rt, d["pk_recv"], d["cmtB_old"], d["sn_old"], d["cmtB"], d["sn_s"]]

# ---- the legs (each in a fresh process) ------------------------------------------------------------------------------------------------------------------------
def leg_small(tmp):
    from blockmaze_amd import engine as e
    z = e.Zk()
    for depth in (1, 2, 8, 20, 32):
        cap = min(256, 1 << depth); leaves = seeded_leaves(cap, 40 + depth); t = e.Tree(depth); n = 0; assert t.size() == 0
        lv, em = model_levels([], depth); assert t.root() == model_root(lv, em, depth), depth                                  # the empty tree
        for want in (1, 2, 1, 12, 1, 239):
            k = min(want, cap - n)
            if not k: break
            before = t.launches(); t.append(leaves[n:n + k]); n += k; assert t.size() == n and t.launches() == before + 1, (depth, n)   # a small append: one launch in total
            lv, em = model_levels(leaves[:n], depth); assert t.root() == model_root(lv, em, depth), (depth, n)
            for i in range(n): assert t.path(i) == model_path(lv, em, depth, i), (depth, n, i)
            rt, sibs = w.merkle_root_and_path([w.rev(x) for x in leaves[:n]], n - 1, depth)                                       # the model's own function on the newest leaf
            assert w.rev(rt) == t.root() and [w.rev(s) for s in sibs] == t.path(n - 1), (depth, n)
            if depth == 8:                                                                                                         # genRoot over the same prefix
                zt = z.TreeNew(8); assert z.TreeAppend(zt, [w.rev(x) for x in leaves[:n]]) == n
                assert z.TreeRoot(zt) == z.GenRT([w.rev(x) for x in leaves[:n]]) == w.rev(t.root()); z.TreeFree(zt)
        assert n == cap
        if depth in (1, 8):                                                                                                        # the 3rd leaf at depth 1, the 257th at depth 8
            root = t.root()
            for extra in (1, 5):
                with pytest.raises(e.ZkGpuError): t.append(seeded_leaves(extra, 9))
                assert t.size() == cap and t.root() == root
            with pytest.raises(e.ZkGpuError): t.path(cap)
        t.close()
    t = e.Tree(8); t.append(seeded_leaves(250, 3)); root = t.root()                                                                 # a batch that only partly fits is refused whole
    with pytest.raises(e.ZkGpuError): t.append(seeded_leaves(7, 4))
    assert t.size() == 250 and t.root() == root; t.append(seeded_leaves(6, 4)); assert t.size() == 256; t.close()
    # the three golden strings through the drop-in entries
    sixteen = w.reference_deposit_fixture()["leaves"]; zt = z.TreeNew(8); assert z.TreeRoot(zt).hex() == GOLDEN_ROOTS[0]
    assert z.TreeAppend(zt, [(1).to_bytes(32, "big")]) == 1 and z.TreeRoot(zt).hex() == GOLDEN_ROOTS[1]; z.TreeFree(zt)
    zt = z.TreeNew(8); assert z.TreeAppend(zt, sixteen[:9]) == 9 and z.TreeAppend(zt, sixteen[9:]) == 16 and z.TreeRoot(zt).hex() == GOLDEN_ROOTS[16]
    assert z.TreeAppend(zt, sixteen * 16) == -1 and z.TreeRoot(zt).hex() == GOLDEN_ROOTS[16]; z.TreeFree(zt)                       # 16 + 256 leaves: refused, unchanged
    zt = z.TreeNew(1); assert z.TreeAppend(zt, sixteen[:2]) == 2 and z.TreeAppend(zt, sixteen[2:3]) == -1; z.TreeFree(zt)
    for bad in (0, 33, -1):
        with pytest.raises(e.ZkGpuError): e.Tree(bad)

def leg_large(tmp):
    from blockmaze_amd import engine as e
    depth, bulk = 32, 1 << 20; N = bulk + 3; blob = random.Random(2024).randbytes(32 * N); leaf = lambda i: blob[32 * i:32 * i + 32]
    t = e.Tree(depth); t0 = time.time(); t.append(blob[:32 * bulk]); dt = time.time() - t0; assert 3 <= t.launches() <= 4, t.launches()    # not one launch a level
    print("bulk append of 2^20 leaves: %.2f ms, %d launches" % (1e3 * dt, t.launches()))
    for i in range(bulk, N): before = t.launches(); t.append(leaf(i)); assert t.launches() == before + 1
    assert t.size() == N
    root, _ = e.tree_host(depth, blob); assert t.root() == root
    # the two ends, both sides of the tile boundaries of level 0 (multiples of 512 leaves) and of level 9 (multiples of 512 * 512 leaves), of the seam between the
    # bulk append and the single ones, then seeded indices up to 64
    rng = random.Random(7); idx = [0, N - 1, TILE - 1, TILE, TILE * TILE - 1, TILE * TILE, 3 * TILE * TILE - 1, 3 * TILE * TILE, bulk - 1, bulk, bulk + 1, bulk - TILE, bulk - TILE - 1]
    for _ in range(6): b = TILE * rng.randrange(1, bulk // TILE); idx += [b - 1, b]
    while len(idx) < 64: idx.append(rng.randrange(N))
    want = {}
    for i in idx:
        want[i] = e.tree_host(depth, blob, i, want_root=False)[1]; assert t.path(i) == want[i], i
        assert t.find(leaf(i)) == i
    # the same leaves in seeded batches of 1 .. 70,000: the same tree
    u = e.Tree(depth); n = 0; calls = 0
    while n < N: k = min(rng.randint(1, 70000), N - n); u.append(blob[32 * n:32 * (n + k)]); n += k; calls += 1
    print("%d random batches, %d launches" % (calls, u.launches()))
    assert u.size() == N and u.root() == root
    for i in idx: assert u.path(i) == want[i], i
    t.close(); u.close()

def leg_find(tmp):
    from blockmaze_amd import engine as e
    leaves = seeded_leaves(1000, 77); leaves[700] = leaves[123]; leaves[999] = leaves[123]; t = e.Tree(20)
    with pytest.raises(e.ZkGpuError): t.find(leaves[0])                                            # the empty tree holds nothing
    t.append(leaves[:5])
    with pytest.raises(e.ZkGpuError): t.find(bytes(32))                                            # the zero blob beyond `size` is no leaf
    with pytest.raises(e.ZkGpuError): t.find(leaves[5])                                            # not appended yet
    t.append(leaves[5:]); assert t.find(leaves[123]) == 123 and t.find(leaves[0]) == 0 and t.find(leaves[998]) == 998
    with pytest.raises(e.ZkGpuError): t.find(seeded_leaves(1, 78)[0])
    with pytest.raises(e.ZkGpuError): t.find(bytes(32))
    t.append([bytes(32), bytes(32)]); assert t.find(bytes(32)) == 1000                             # a zero leaf that WAS appended is a leaf
    t.close()

def leg_deposit8(tmp):
    from blockmaze_amd import engine as e
    e.keygen("deposit", os.path.join(tmp, "depositpk.txt"), os.path.join(tmp, "depositvk.txt"), seed=0xB10C4A2E + 7); z = e.Zk()
    d = w.deposit_instance(11, n_leaves=256); t = z.TreeNew(8); assert z.TreeAppend(t, d["leaves"][:100]) == 100 and z.TreeAppend(t, d["leaves"][100:]) == 256
    proof, rt = z.GenDepositProofTree(*w.deposit_args(d), d["sk"], t); assert not proof.startswith("0000000000") and rt is not None
    assert rt == z.GenRT(d["leaves"]) == d["rt"] == z.TreeRoot(t)
    assert z.VerifyDepositProof(proof, *dep_public(d, rt)) and z.VerifyDepositProofDepth(8, proof, *dep_public(d, rt))
    assert not z.VerifyDepositProof(proof, *dep_public(d, z.GenRT(d["leaves"][:255])))            # another root
    other = w.deposit_instance(12); p2, rt2 = z.GenDepositProofTree(*w.deposit_args(other), other["sk"], t)   # its cmtS is not in this tree
    assert p2.startswith("0000000000") and len(p2) == 512 and rt2 is None
    p3, rt3 = z.GenDepositProofTree(*w.deposit_args(d), d["sk"], None); assert p3 == p2 and rt3 is None       # no tree
    z.TreeFree(t)

def leg_deposit32(tmp):
    from blockmaze_amd import engine as e
    pk32, vk32 = os.path.join(tmp, "deposit32pk.txt"), os.path.join(tmp, "deposit32vk.txt"); e.keygen("deposit", pk32, vk32, seed=32, tree_depth=32)
    e.keygen("deposit", os.path.join(tmp, "depositpk.txt"), os.path.join(tmp, "depositvk.txt"), seed=0xB10C4A2E + 7); z = e.Zk()
    d = w.deposit_instance(21, n_leaves=1024); t = z.TreeNew(32); assert z.TreeAppend(t, d["leaves"]) == 1024
    t0 = time.time(); proof, rt = z.GenDepositProofTree(*w.deposit_args(d), d["sk"], t); first = time.time() - t0
    t0 = time.time(); proof2, rt2 = z.GenDepositProofTree(*w.deposit_args(d), d["sk"], t); print("genDepositproofTree at depth 32: first call %.1f s (key load), second %.2f ms" % (first, 1e3 * (time.time() - t0)))
    assert not proof.startswith("0000000000") and rt == rt2 == z.TreeRoot(t)
    rt_model, _ = w.merkle_root_and_path(d["leaves"], d["index"], depth=32); assert rt == rt_model
    for p in (proof, proof2):
        assert z.VerifyDepositProofDepth(32, p, *dep_public(d, rt))
        assert e.verify(vk32, p, w.pack_public(dep_public(d, rt_model)))
        assert not z.VerifyDepositProofDepth(8, p, *dep_public(d, rt))                              # the depth-8 key is another key
    assert not z.VerifyDepositProofDepth(32, proof, *dep_public(d, d["rt"]))                       # (another root: the instance's own rt is not the depth-32 root)
    if os.path.exists(HARNESS):
        inputs = w.pack_public(dep_public(d, rt_model)); r = subprocess.run([HARNESS, "verify", vk32, proof, "6", *[str(x) for x in inputs]], capture_output=True, text=True)
        assert r.returncode == 0 and "verify 1" in r.stdout, r.stdout[-300:]
        print("LEG libsnark verifier on the depth-32 tree proof")
    z.TreeFree(t)

def leg_concurrency(tmp):
    from blockmaze_amd import engine as e
    e.keygen("deposit", os.path.join(tmp, "depositpk.txt"), os.path.join(tmp, "depositvk.txt"), seed=0xB10C4A2E + 7); z = e.Zk()
    ds = [w.deposit_instance(31, n_leaves=20), w.deposit_instance(32, n_leaves=20)]; start = ds[0]["leaves"] + ds[1]["leaves"]; more = [w.rev(x) for x in seeded_leaves(200, 5)]
    t = z.TreeNew(8); assert z.TreeAppend(t, start) == 40
    z.GenDepositProofTree(*w.deposit_args(ds[0]), ds[0]["sk"], t)                                   # (the key is loaded before the threads start)
    got = [[], []]; errs = []
    def appender():
        try:
            for i, c in enumerate(more): assert z.TreeAppend(t, [c]) == 41 + i; time.sleep(0.0005)
        except BaseException as x: errs.append(x)
    def prover(j):
        try:
            for _ in range(10): got[j].append(z.GenDepositProofTree(*w.deposit_args(ds[j]), ds[j]["sk"], t))
        except BaseException as x: errs.append(x)
    th = [threading.Thread(target=appender), threading.Thread(target=prover, args=(0,)), threading.Thread(target=prover, args=(1,))]
    for x in th: x.start()
    for x in th: x.join()
    assert not errs, errs
    # the model's roots of the prefixes: 40 .. 240 leaves
    roots = set()
    for k in range(len(more) + 1): lv, em = model_levels([w.rev(x) for x in start + more[:k]], 8); roots.add(w.rev(model_root(lv, em, 8)))
    seen = set()
    for j in range(2):
        assert len(got[j]) == 10
        for proof, rt in got[j]:
            assert rt is not None and not proof.startswith("0000000000") and rt in roots, j
            assert z.VerifyDepositProof(proof, *dep_public(ds[j], rt)); seen.add(rt)
    print("distinct roots proved against: %d" % len(seen))
    assert z.TreeRoot(t) == z.GenRT(start + more); z.TreeFree(t)

LEGS = {"small": leg_small, "large": leg_large, "find": leg_find, "deposit8": leg_deposit8, "deposit32": leg_deposit32, "concurrency": leg_concurrency}

def run_leg(name, tmp_path, timeout, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path), **(env or {})))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

def test_small_trees_against_the_python_model(tmp_path): run_leg("small", tmp_path, 600)
def test_large_tree_against_the_host_model(tmp_path): print(run_leg("large", tmp_path, 900))
def test_find(tmp_path): run_leg("find", tmp_path, 300)
def test_deposit_through_the_tree_at_depth_8(tmp_path): run_leg("deposit8", tmp_path, 600)
def test_deposit_through_the_tree_at_depth_32(tmp_path):
    out = run_leg("deposit32", tmp_path, 900, {"ZK_PROVERS_PER_KEY": "2"}); print(out)
    if "LEG libsnark" in out:
        from conftest import record_leg; record_leg("libsnark verifier on the depth-32 proof made against the resident tree")
def test_appends_and_proofs_at_the_same_time(tmp_path): run_leg("concurrency", tmp_path, 600)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
