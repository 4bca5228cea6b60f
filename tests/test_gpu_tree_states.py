"""Past states of the resident commitment tree (blockmaze_amd/csrc/gpu_tree.hip: k_tree_roots_at, k_tree_paths_at, k_tree_rewind; include/zk_tree_states.h): roots,
paths and proofs at any earlier size, and the rewind after a reorganisation.

The model is always the existing one applied to the PREFIX: the Python model of tests/workload.py over leaves[:m] for small trees, the library's host model
(zkgpu_test_tree_host) over the first m leaves for large ones; tests/test_tree_states_cpu.py pins the rule to the same model.  Every leg runs in a process of its
own under a time limit: `python tests/test_gpu_tree_states.py <leg> <scratch dir>` is what each test starts."""
import ctypes, functools, os, random, subprocess, sys, threading
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import workload as w

pytestmark = pytest.mark.gpu
GOLDEN_ROOTS = {0: "8eb3c27b218349e6b9b6037b8042f3751ee820e8a0319a1bda439b247456088c", 1: "a19a0d1fac447f65d273d5831827ccfa96c193a1b39618a23d11628d48e27a9e",
                16: "2630f036430a646118dbb95ba55e9e3803e35a680398d01f9942513ebbb7911e"}   # genRoot over 0, 1 and 16 leaves (tests/test_abi_exports.py)

comp = functools.lru_cache(maxsize=None)(w._sha256_compress)   # (the prefixes of one leaf list share almost all of their nodes)
def model_levels(leaves_blob, depth):
    """every level of the Python model's tree (workload.merkle_root_and_path rebuilds it per call): levels[k] in blob order, empty[k] = empty root of level k"""
    levels = [list(leaves_blob)]; empty = [bytes(32)]
    for d in range(depth):
        cur = levels[-1]; levels.append([comp(cur[i] + (cur[i + 1] if i + 1 < len(cur) else empty[d])) for i in range(0, len(cur), 2)])
        empty.append(comp(empty[d] + empty[d]))
    return levels, empty
def model_root(levels, empty, depth): return levels[depth][0] if levels[depth] else empty[depth]
def model_path(levels, empty, depth, index): return [levels[k][(index >> k) ^ 1] if ((index >> k) ^ 1) < len(levels[k]) else empty[k] for k in range(depth)]
def seeded_leaves(n, seed):
    rng = random.Random(seed); return [rng.getrandbits(256).to_bytes(32, "little") for _ in range(n)]
def dep_public(d, rt): return [rt, d["pk_recv"], d["cmtB_old"], d["sn_old"], d["cmtB"], d["sn_s"]]
def is_sentinel(proof): return proof.startswith("0000000000") and len(proof) == 512
def u64s(v): return (ctypes.c_uint64 * max(1, len(v)))(*v)
FILL = bytes(range(7, 7 + 64)) * 40                             # what an output buffer holds before a call that must write nothing

def check_state(e, t, leaves, depth, every_path=True):
    """size, root, every path and find of the tree's current state against the model of the current leaf list"""
    n = len(leaves); lv, em = model_levels(leaves, depth); assert t.size() == n and t.root() == model_root(lv, em, depth), (depth, n)
    for i in (range(n) if every_path else sorted(set([0, n // 2, n - 1]) & set(range(n)))): assert t.path(i) == model_path(lv, em, depth, i), (depth, n, i)
    if n:
        sibs, root = t.paths_at(n, list(range(n))); assert root == model_root(lv, em, depth) and sibs == [model_path(lv, em, depth, i) for i in range(n)], (depth, n)
        for i in sorted(set([0, n // 3, n - 1])): assert t.find(leaves[i]) == leaves.index(leaves[i]), (depth, n, i)
    else:
        with pytest.raises(e.ZkGpuError): t.find(bytes(32))

# ---- the legs (each in a fresh process) ------------------------------------------------------------------------------------------------------------------------
def leg_small(tmp):
    from blockmaze_amd import engine as e
    z = e.Zk(); L = e.lib()
    for depth in (1, 2, 3, 8, 20, 32):
        n = min(256, 1 << depth); leaves = seeded_leaves(n, 140 + depth); rng = random.Random(depth)
        if n >= 8: leaves[n - 3] = leaves[2]                                                           # one blob twice: find gives the first
        t = e.Tree(depth); at = 0
        assert t.roots_at([]) == [] and t.roots_at([0, 0]) == [model_root(*model_levels([], depth), depth)] * 2 and t.state_launches() <= 1
        for want in (1, 2, 1, 12, 1, 239):
            k = min(want, n - at)
            if k: t.append(leaves[at:at + k]); at += k
        assert at == n == t.size()
        models = [model_levels(leaves[:m], depth) for m in range(n + 1)]; roots = [model_root(lv, em, depth) for lv, em in models]
        # one call with ALL sizes, shuffled and with duplicates
        sizes = list(range(n + 1)) + [rng.randrange(n + 1) for _ in range(40)] + [0, n, n]; rng.shuffle(sizes)
        before = t.state_launches(); got = t.roots_at(sizes); assert t.state_launches() - before <= 2, depth
        assert got == [roots[m] for m in sizes], (depth, [m for m, g in zip(sizes, got) if g != roots[m]][:8])
        # every path of a state, in one call
        pows = [1 << k for k in range(depth + 1)]; marks = [1, 2, 3, n - 1, n] + [p + s for p in pows for s in (-1, 0, 1)]
        for m in (range(n + 1) if depth <= 3 else sorted(set(x for x in marks if 1 <= x <= n))):
            lv, em = models[m]; before = t.state_launches(); sibs, root = t.paths_at(m, list(range(m))); assert t.state_launches() - before <= 2, (depth, m)
            assert root == roots[m], (depth, m)
            for i in range(m): assert sibs[i] == model_path(lv, em, depth, i), (depth, m, i)
        sibs, root = t.paths_at(n, [n - 1, 0, n - 1]); assert sibs[0] == sibs[2] == t.path(n - 1) and sibs[1] == t.path(0) and root == t.root()   # any order, repeats
        # find_at: a leaf at index >= m is absent, a duplicated leaf gives its first index
        for i in sorted(set([0, 1, n // 2, n - 1])):
            first = leaves.index(leaves[i]); assert t.find_at(first + 1, leaves[i]) == first == t.find_at(n, leaves[i]), (depth, i)
            with pytest.raises(e.ZkGpuError): t.find_at(first, leaves[i])
        if n >= 8:
            assert t.find_at(n, leaves[n - 3]) == 2 and t.find_at(3, leaves[n - 3]) == 2
            with pytest.raises(e.ZkGpuError): t.find_at(2, leaves[n - 3])
        with pytest.raises(e.ZkGpuError): t.find_at(n, bytes(32))
        with pytest.raises(e.ZkGpuError): t.find_at(0, leaves[0])
        # bad arguments fail and write nothing: a size above the tree's, an index that is not below its size, a null pointer
        h = ctypes.c_void_p(t.h); buf = ctypes.create_string_buffer(FILL, len(FILL)); rbuf = ctypes.create_string_buffer(FILL[:32], 32); idx = ctypes.c_uint64(77)
        before = t.state_launches(); root = t.root()
        bad = [L.zkgpu_tree_roots_at(h, u64s([0, n + 1, 1]), ctypes.c_size_t(3), buf), L.zkgpu_tree_roots_at(h, u64s([1 << 40]), ctypes.c_size_t(1), buf),
               L.zkgpu_tree_roots_at(h, None, ctypes.c_size_t(1), buf), L.zkgpu_tree_roots_at(h, u64s([1]), ctypes.c_size_t(1), None),
               L.zkgpu_tree_paths_at(h, ctypes.c_uint64(n + 1), u64s([0]), ctypes.c_size_t(1), buf, rbuf), L.zkgpu_tree_paths_at(h, ctypes.c_uint64(n + 1), None, ctypes.c_size_t(0), buf, rbuf),
               L.zkgpu_tree_paths_at(h, ctypes.c_uint64(n), u64s([0, n]), ctypes.c_size_t(2), buf, rbuf), L.zkgpu_tree_paths_at(h, ctypes.c_uint64(1), u64s([1]), ctypes.c_size_t(1), buf, rbuf),
               L.zkgpu_tree_paths_at(h, ctypes.c_uint64(0), u64s([0]), ctypes.c_size_t(1), buf, rbuf), L.zkgpu_tree_paths_at(h, ctypes.c_uint64(1), None, ctypes.c_size_t(1), buf, rbuf),
               L.zkgpu_tree_paths_at(h, ctypes.c_uint64(1), u64s([0]), ctypes.c_size_t(1), None, rbuf),
               L.zkgpu_tree_find_at(h, ctypes.c_uint64(n + 1), leaves[0], ctypes.byref(idx)), L.zkgpu_tree_find_at(h, ctypes.c_uint64(n), None, ctypes.byref(idx)),
               L.zkgpu_tree_rewind(h, ctypes.c_uint64(n + 1)), L.zkgpu_tree_rewind(h, ctypes.c_uint64(1 << 63))]
        assert bad == [-2] * len(bad), (depth, bad)                                                      # ZKGPU_ERR_ARG
        assert buf.raw == FILL and rbuf.raw == FILL[:32] and idx.value == 77 and t.size() == n and t.root() == root and t.state_launches() == before, depth
        sibs, root0 = t.paths_at(0, []); assert sibs == [] and root0 == roots[0]                          # q = 0 is a valid call
        sibs, root1 = t.paths_at(n, []); assert sibs == [] and root1 == roots[n]
        t.close()
    # depth 8 through the drop-in entries: zkTreeRootAt(m) is genRoot over the first m commitments
    cm = [w.rev(x) for x in seeded_leaves(256, 148)]; zt = z.TreeNew(8); assert z.TreeAppend(zt, cm[:77]) == 77 and z.TreeAppend(zt, cm[77:]) == 256
    want = [z.GenRT(cm[:m]) for m in range(257)]; assert [z.TreeRootAt(zt, m) for m in range(257)] == want and want[0].hex() == GOLDEN_ROOTS[0]
    sizes = list(range(257)) * 2; random.Random(5).shuffle(sizes); assert z.TreeRootsAt(zt, sizes) == [want[m] for m in sizes] and z.TreeRootsAt(zt, []) == []
    import numpy as np
    out = np.frombuffer(FILL[:96], dtype=np.uint8).reshape(3, 32).copy()
    for bad in ([0, 257, 1], [0, -1, 1], [-(1 << 62), 0, 0]): assert z.TreeRootsAt(zt, bad, out=out) == -1 and out.tobytes() == FILL[:96], bad
    assert z.TreeRootAt(zt, 257) is None and z.TreeRootAt(zt, -1) is None and z.TreeRewind(zt, 257) == -1 and z.TreeRewind(zt, -1) == -1 and z.TreeRoot(zt) == want[256]
    z.TreeFree(zt)
    sixteen = w.reference_deposit_fixture()["leaves"]; zt = z.TreeNew(8); assert z.TreeAppend(zt, sixteen + cm[:5]) == 21                 # the golden strings
    assert z.TreeRootAt(zt, 16).hex() == GOLDEN_ROOTS[16] and z.TreeRootAt(zt, 0).hex() == GOLDEN_ROOTS[0]; z.TreeFree(zt)
    zt = z.TreeNew(8); assert z.TreeAppend(zt, [(1).to_bytes(32, "big")] + cm[:3]) == 4 and z.TreeRootAt(zt, 1).hex() == GOLDEN_ROOTS[1]; z.TreeFree(zt)

def leg_rewind(tmp):
    from blockmaze_amd import engine as e
    for depth in (1, 2, 6, 9, 32):
        cap = 1 << depth; rng = random.Random(1000 + depth); t = e.Tree(depth); leaves = []; fresh = iter(seeded_leaves(6000, 2000 + depth)); steps = 0
        def append(k):
            k = min(k, cap - len(leaves))
            if not k: return
            new = [next(fresh) for _ in range(k)]; before = t.launches(); t.append(new); leaves.extend(new)
            if k <= 100: assert t.launches() == before + 1, (depth, len(leaves), k)                     # a small append, after a rewind too, is ONE launch
        def rewind(m):
            n = len(leaves)
            if m > n:
                root = t.root()
                with pytest.raises(e.ZkGpuError): t.rewind(m)
                assert t.size() == n and t.root() == root; return
            before = t.state_launches(); t.rewind(m); del leaves[m:]; assert t.state_launches() - before <= (0 if m in (0, n) else 1), (depth, n, m)
        pow2 = lambda: 1 << max(0, len(leaves).bit_length() - 1 - rng.randrange(2))
        script = [("a", 1), ("r", 0), ("a", 37), ("r", lambda: len(leaves) - 1), ("a", 3), ("r", lambda: len(leaves)), ("r", lambda: len(leaves) + 1), ("a", 300), ("r", pow2), ("a", 2),
                  ("r", lambda: len(leaves) - 1), ("r", 1), ("a", 90), ("r", pow2), ("r", lambda: min(len(leaves), pow2() + 1)), ("a", 1), ("r", 0), ("r", 0), ("r", 1), ("a", 64), ("r", lambda: len(leaves) + 5)]
        for _ in range(10): script.append(("a", rng.randrange(1, 80)) if rng.random() < 0.5 else ("r", lambda: rng.randrange(0, len(leaves) + 1)))
        for op, arg in script:
            arg = arg() if callable(arg) else arg
            if op == "a": append(arg)
            else: rewind(max(0, arg))
            check_state(e, t, leaves, depth); steps += 1
        t.close(); print("depth %d: %d steps, %d leaves at the end" % (depth, steps, len(leaves)))
    # capacity: the allocation grows (2,048 -> 4,096 leaves) after rewinds, and only the live nodes move
    depth = 20; a = seeded_leaves(1500, 31); b = seeded_leaves(1100, 32); t = e.Tree(depth); t.append(a)
    for m in (1025, 1024, 1000): t.rewind(m); assert t.size() == m and t.root() == e.tree_host(depth, a[:m])[0], m
    now = a[:1000] + b; t.append(b); assert t.size() == 2100
    u = e.Tree(depth); u.append(now); root, _ = e.tree_host(depth, now); assert t.root() == u.root() == root
    idx = [0, 999, 1000, 1023, 1024, 1025, 1499, 1500, 2047, 2048, 2099] + [random.Random(9).randrange(2100) for _ in range(53)]
    sibs, r2 = t.paths_at(2100, idx); assert r2 == root
    for i, s in zip(idx, sibs): assert s == t.path(i) == u.path(i) == e.tree_host(depth, now, i, want_root=False)[1], i
    assert t.roots_at([1000, 1024, 1025, 1500]) == u.roots_at([1000, 1024, 1025, 1500]) == [e.tree_host(depth, now[:m])[0] for m in (1000, 1024, 1025, 1500)]
    t.close(); u.close()

def leg_tiles(tmp):
    from blockmaze_amd import engine as e
    depth, big = 32, 1 << 18; N = big + 515; blob = random.Random(2025).randbytes(32 * N); t = e.Tree(depth); t.append(blob); assert t.size() == N
    def check(tree, data, sizes):
        before = tree.state_launches(); got = tree.roots_at(sizes); assert tree.state_launches() - before <= 2
        for m, r in zip(sizes, got):
            rng = random.Random(m); idx = sorted(set([0, m - 1, (m - 1) ^ 1 if (m - 1) ^ 1 < m else 0, m // 2, 511 % m, 512 % m, (big - 1) % m, rng.randrange(m)]))
            sibs, root = tree.paths_at(m, idx); assert root == r, m
            prefix = data[:32 * m]; assert r == e.tree_host(depth, prefix)[0], m
            for i, s in zip(idx, sibs): assert s == e.tree_host(depth, prefix, i, want_root=False)[1], (m, i)
    check(t, blob, [511, 512, 513, big - 1, big, big + 1, N - 1, N])
    other = random.Random(2026).randbytes(32 * 600); t.rewind(big + 1); t.append(other); now = blob[:32 * (big + 1)] + other; M = big + 601; assert t.size() == M
    root, _ = e.tree_host(depth, now); assert t.root() == root
    for i in (0, big - 1, big, big + 1, big + 2, big + 514, big + 515, M - 1): assert t.path(i) == e.tree_host(depth, now, i, want_root=False)[1], i
    check(t, now, [big + 1, big + 2, M])
    t.close()

def deposit_at_40(seed):
    d = w.deposit_instance(seed, n_leaves=256); lv = d["leaves"]; lv[d["index"]], lv[40] = lv[40], lv[d["index"]]; d["index"] = 40; assert lv[40] == d["cmtS"] and lv.count(d["cmtS"]) == 1
    return d

def leg_deposit8(tmp):
    from blockmaze_amd import engine as e
    e.keygen("deposit", os.path.join(tmp, "depositpk.txt"), os.path.join(tmp, "depositvk.txt"), seed=0xB10C4A2E + 7); z = e.Zk()
    d = deposit_at_40(11); lv = d["leaves"]; t = z.TreeNew(8); assert z.TreeAppend(t, lv[:100]) == 100 and z.TreeAppend(t, lv[100:]) == 256
    args = w.deposit_args(d); now = z.GenRT(lv); rt100 = z.GenRT(lv[:100]); assert now != rt100
    proof, rt = z.GenDepositProofTreeAt(*args, d["sk"], t, 100); assert not is_sentinel(proof) and rt == rt100 == z.TreeRootAt(t, 100)
    assert z.VerifyDepositProof(proof, *dep_public(d, rt100)) and not z.VerifyDepositProof(proof, *dep_public(d, now))
    for size in (40, 257, -1, 0):                                                                   # cmtS not yet in; more than the tree holds; no size at all
        p, r = z.GenDepositProofTreeAt(*args, d["sk"], t, size); assert is_sentinel(p) and r is None, size
    p, r = z.GenDepositProofTreeAt(*args, d["sk"], t, 41); assert not is_sentinel(p) and r == z.GenRT(lv[:41]) and z.VerifyDepositProof(p, *dep_public(d, r))
    p256, r256 = z.GenDepositProofTreeAt(*args, d["sk"], t, 256); pt, rtt = z.GenDepositProofTree(*args, d["sk"], t)
    assert r256 == rtt == now and not is_sentinel(p256) and z.VerifyDepositProof(p256, *dep_public(d, now)) and z.VerifyDepositProof(pt, *dep_public(d, now))
    assert z.TreeRewind(t, 60) == 60
    p, r = z.GenDepositProofTreeAt(*args, d["sk"], t, 100); assert is_sentinel(p) and r is None       # the tree was rewound below 100
    p, r = z.GenDepositProofTreeAt(*args, d["sk"], t, 60); rt60 = z.GenRT(lv[:60]); assert not is_sentinel(p) and r == rt60 == z.TreeRoot(t)
    assert z.VerifyDepositProof(p, *dep_public(d, rt60)) and not z.VerifyDepositProof(p, *dep_public(d, rt100))
    p, r = z.GenDepositProofTreeAt(*args, d["sk"], None, 60); assert is_sentinel(p) and r is None     # no tree
    z.TreeFree(t)

def leg_concurrency(tmp):
    from blockmaze_amd import engine as e
    e.keygen("deposit", os.path.join(tmp, "depositpk.txt"), os.path.join(tmp, "depositvk.txt"), seed=0xB10C4A2E + 7); z = e.Zk()
    ds = [w.deposit_instance(41, n_leaves=50), w.deposit_instance(42, n_leaves=50)]; tail = [w.rev(x) for x in seeded_leaves(20, 6)]; more = [w.rev(x) for x in seeded_leaves(100, 7)]
    base = ds[0]["leaves"] + ds[1]["leaves"] + tail; t = z.TreeNew(8); assert z.TreeAppend(t, base) == 120; rt100 = z.GenRT(base[:100])
    z.GenDepositProofTreeAt(*w.deposit_args(ds[0]), ds[0]["sk"], t, 100)                            # (the key is loaded before the threads start)
    got = [[], []]; errs = []
    def rewinder():                                                                                  # never below 115 leaves: state 100 stays what it is
        try:
            rng = random.Random(3)
            for _ in range(200):
                r = rng.randrange(1, 6); assert z.TreeRewind(t, 120 - r) == 120 - r; assert z.TreeAppend(t, base[120 - r:]) >= 120
        except BaseException as x: errs.append(x)
    def appender():                                                                                  # (its leaves go again with the next rewind: the tree stays small)
        try:
            for c in more: assert z.TreeAppend(t, [c]) >= 116
        except BaseException as x: errs.append(x)
    def prover(j):
        try:
            for _ in range(10): got[j].append(z.GenDepositProofTreeAt(*w.deposit_args(ds[j]), ds[j]["sk"], t, 100))
        except BaseException as x: errs.append(x)
    th = [threading.Thread(target=rewinder), threading.Thread(target=appender), threading.Thread(target=prover, args=(0,)), threading.Thread(target=prover, args=(1,))]
    for x in th: x.start()
    for x in th: x.join()
    assert not errs, errs
    for j in range(2):
        assert len(got[j]) == 10
        for proof, rt in got[j]: assert rt == rt100 and not is_sentinel(proof) and z.VerifyDepositProof(proof, *dep_public(ds[j], rt100)), j
    assert z.TreeRootAt(t, 100) == rt100 and z.TreeRootAt(t, 115) == z.GenRT(base[:115]); z.TreeFree(t)

LEGS = {"small": leg_small, "rewind": leg_rewind, "tiles": leg_tiles, "deposit8": leg_deposit8, "concurrency": leg_concurrency}

def run_leg(name, tmp_path, timeout, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=timeout,
                       env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path), **(env or {})))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

def test_roots_paths_and_find_at_every_size_of_small_trees(tmp_path): run_leg("small", tmp_path, 600)
def test_rewind_then_append_sequences(tmp_path): print(run_leg("rewind", tmp_path, 600))
def test_past_states_across_both_tilings(tmp_path): run_leg("tiles", tmp_path, 600)
def test_deposit_at_a_past_size_at_depth_8(tmp_path): run_leg("deposit8", tmp_path, 600)
def test_rewinds_appends_and_proofs_at_the_same_time(tmp_path): run_leg("concurrency", tmp_path, 600)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
