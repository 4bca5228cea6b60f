"""The anchor step with a window a record on the device (blockmaze_amd/csrc/gpu_tree.hip: CommitmentTree::match_roots_window, k_tree_match_roots_window;
include/zkgpu.h: zkgpu_tree_match_roots_window) against the prefix model of tests/test_tree_block_cpu.py restricted to the window: for each RT the lowest anchor
a with lo <= a < hi whose prefix root it equals.  Anchor lists cross the LDS tile of 256 roots, record counts cross the wave and the workgroup, and the windows are
empty, one wide, the whole list, astride a tile edge, and far apart inside one workgroup.  Every leg runs in a process of its own under a time limit:
`python tests/test_gpu_tree_match_window.py <leg> <scratch dir>` is what each test starts."""
import ctypes, os, random, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import workload as w
from test_tree_block_cpu import PrefixRoots, seeded_leaves

pytestmark = pytest.mark.gpu
TREES = [(1, 2), (2, 4), (8, 200), (32, 1000)]                  # (depth, leaves)
ANCHORS = [0, 1, 255, 256, 257, 600]                            # the kernel takes the roots in tiles of 256
RECORDS = [0, 1, 255, 256, 257, 1000]                           # ... and the records in workgroups of 256
POOL = 40                                                       # distinct sizes a large tree's anchors are drawn from (each costs the model one walk in Python)

def model_match_window(pr, sizes, rts, lo, hi):
    """for every RT (blob order) the lowest a in [lo, hi) with root(sizes[a]) == RT, or -1"""
    roots = [pr.root(m) for m in sizes]; return [next((a for a in range(l, h) if roots[a] == bytes(rt)), -1) for rt, l, h in zip(rts, lo, hi)]

def anchor_list(rng, n, length):
    """`length` sizes with many repeats (a repeated root must be found at its lowest index INSIDE the window); two sizes stay outside every list"""
    pool = sorted(set([0, n] + [rng.randrange(n + 1) for _ in range(POOL)]) - {1, n - 1}) if n > 4 else [0, n]
    return [rng.choice(pool) for _ in range(length)]

def windows(rng, m, q):
    """one window a record, by turns: empty, one wide, the whole list, astride the tile edge, a random one; in block order or not, the kernel must not care"""
    lo, hi = [], []
    for i in range(q):
        kind = i % 5
        if kind == 0 or m == 0: l = rng.randrange(m + 1); h = l
        elif kind == 1: l = rng.randrange(m); h = l + 1
        elif kind == 2: l, h = 0, m
        elif kind == 3: l, h = min(250, m), min(262, m)
        else: l = rng.randrange(m + 1); h = rng.randrange(l, m + 1)
        lo.append(l); hi.append(h)
    return lo, hi

def leg_differential(tmp):
    from blockmaze_amd import engine as e
    calls = 0; matched = 0; shadowed = 0; higher = 0
    for depth, n in TREES:
        leaves = seeded_leaves(n, 500 + depth); t = e.Tree(depth); t.append(leaves); assert t.size() == n; pr = PrefixRoots(leaves, depth); rng = random.Random(depth)
        outside = [pr.root(1), pr.root(n - 1)] if n > 4 else []
        for length in ANCHORS:
            sizes = anchor_list(rng, n, length); roots = [pr.root(m) for m in sizes]
            for q in RECORDS:
                lo, hi = windows(rng, length, q)
                # by turns: a root of the window, a root of the list (often only OUTSIDE the window), a root of the tree that is no anchor's, an almost-root, 32 zero bytes
                rts = []
                for i in range(q):
                    pick = (i // 5) % 5
                    if pick == 0 and lo[i] < hi[i]: rts.append(roots[rng.randrange(lo[i], hi[i])])
                    elif pick <= 1 and length: rts.append(rng.choice(roots))
                    elif pick == 2 and outside: rts.append(rng.choice(outside))
                    elif pick == 3 and length: r = bytearray(rng.choice(roots)); r[rng.choice([0, 4, 31])] ^= 0x80; rts.append(bytes(r))
                    else: rts.append(bytes(32))
                want = model_match_window(pr, sizes, rts, lo, hi); before = t.state_launches()
                got = t.match_roots_window(sizes, rts, lo, hi); assert got == want, (depth, length, q, [(i, lo[i], hi[i], got[i], want[i]) for i in range(q) if got[i] != want[i]][:8])
                assert t.state_launches() - before == (2 if q and length else 0), (depth, length, q)     # the roots, then the compare: two launches whatever q and m are
                assert t.match_roots_window(sizes, [w.rev(r) for r in rts], lo, hi, hash_order=True) == want, (depth, length, q, "hash order")
                assert t.state_launches() - before == (4 if q and length else 0)
                # every window the whole list: match_roots on the same input
                assert t.match_roots_window(sizes, rts, [0] * q, [length] * q) == t.match_roots(sizes, rts), (depth, length, q, "whole list")
                calls += 3; matched += sum(x >= 0 for x in want)
                for i in range(q):
                    first = roots.index(rts[i]) if rts[i] in roots else -1
                    shadowed += first >= 0 and want[i] < 0                                                # a root that exists only outside the window
                    higher += first >= 0 and want[i] > first                                              # the lowest index inside the window is not the lowest overall
        t.close()
    print("calls", calls, "matched", matched, "only outside the window", shadowed, "lowest inside above lowest overall", higher); assert matched > 1000 and shadowed > 200 and higher > 200

def leg_far_apart_and_edges(tmp):
    """one workgroup whose windows lie far apart: the union runs over three tiles and each lane must still look at its own window alone"""
    from blockmaze_amd import engine as e
    depth, n = 12, 700; leaves = seeded_leaves(n, 91); t = e.Tree(depth); t.append(leaves); pr = PrefixRoots(leaves, depth)
    sizes = list(range(100, 700)); m = len(sizes); roots = [pr.root(x) for x in sizes]; assert m == 600 and len(set(roots)) == m
    lo = [0, 590] * 100; hi = [8, 600] * 100; rts = [roots[(3 * i) % 8] if i % 2 == 0 else roots[590 + (7 * i) % 10] for i in range(200)]
    rts[10] = roots[595]; rts[11] = roots[3]; rts[12] = roots[8]; rts[13] = roots[589]                    # the other lane's window, and one past each end of its own
    want = model_match_window(pr, sizes, rts, lo, hi); assert want[10:14] == [-1] * 4 and min(want[:10]) >= 0
    assert t.match_roots_window(sizes, rts, lo, hi) == want
    # astride the tile edge, with the same root on both sides of it and on both sides of the window
    sizes2 = list(sizes); sizes2[249] = sizes2[255] = sizes2[256] = sizes2[262] = 650; r650 = pr.root(650); los = [250, 256, 250, 257, 263, 0, 250]; his = [262, 262, 255, 262, 600, 249, 250]
    assert t.match_roots_window(sizes2, [r650] * 7, los, his) == [255, 256, -1, -1, 550, -1, -1] and t.match_roots(sizes2, [r650]) == [249]
    # a workgroup of live lanes that all have empty windows beside one that has not, and records beyond the last workgroup's q
    q = 300; los = [5] * q; his = [5] * q; his[299] = 6; rts = [roots[5]] * q
    assert t.match_roots_window(sizes, rts, los, his) == [-1] * 299 + [5]
    t.close()

FILL = 0x5A5A5A5A
def leg_errors(tmp):
    from blockmaze_amd import engine as e
    L = e.lib(); depth, n = 20, 300; leaves = seeded_leaves(n, 77); t = e.Tree(depth); t.append(leaves); pr = PrefixRoots(leaves, depth)
    h = ctypes.c_void_p(t.h); out = (ctypes.c_int32 * 4)(*([FILL] * 4)); rts = pr.root(300) + pr.root(250) + pr.root(0) + bytes(32); z = ctypes.c_size_t
    def u64s(v): return (ctypes.c_uint64 * max(1, len(v)))(*v)
    def u32s(v): return (ctypes.c_uint32 * max(1, len(v)))(*v)
    good = u64s([300, 250, 0]); lo = u32s([0, 0, 0, 0]); hi = u32s([3, 3, 3, 3]); before = t.state_launches(); root = t.root(); f = L.zkgpu_tree_match_roots_window
    bad = [f(h, u64s([0, 301, 1]), z(3), rts, z(4), lo, hi, 0, out), f(h, u64s([1 << 40, 0, 0]), z(3), rts, z(4), lo, hi, 0, out),                    # a size above the tree's
           f(h, good, z(3), rts, z(4), u32s([0, 2, 0, 0]), u32s([3, 1, 3, 3]), 0, out), f(h, good, z(3), rts, z(4), lo, u32s([3, 3, 4, 3]), 0, out),  # lo > hi; hi > m
           f(h, good, z(3), rts, z(4), u32s([0, 0, 0, 0xffffffff]), u32s([3, 3, 3, 0xffffffff]), 0, out),                                             # ... even for an empty window
           f(h, None, z(3), rts, z(4), lo, hi, 0, out), f(h, good, z(3), None, z(4), lo, hi, 0, out), f(h, good, z(3), rts, z(4), None, hi, 0, out),  # a null pointer with a count
           f(h, good, z(3), rts, z(4), lo, None, 0, out), f(h, good, z(3), rts, z(4), lo, hi, 0, None), f(h, good, z(1 << 31), rts, z(4), lo, hi, 0, out),   # 2^31 anchors
           f(None, good, z(3), rts, z(4), lo, hi, 0, out)]
    assert bad == [-2] * len(bad) and list(out) == [FILL] * 4 and t.state_launches() == before and t.size() == n and t.root() == root, bad   # ZKGPU_ERR_ARG, nothing written
    assert f(h, None, z(0), None, z(0), None, None, 1, None) == 0 and t.state_launches() == before                                             # nothing to do is a valid call
    assert f(h, good, z(3), rts, z(4), lo, hi, 0, out) == 0 and list(out) == [0, 1, 2, -1] and t.state_launches() == before + 2
    with pytest.raises(e.ZkGpuError): t.match_roots_window([300], [pr.root(300)], [0], [2])
    assert t.match_roots_window([], [pr.root(0)], [0], [0]) == [-1] and t.state_launches() == before + 2                                         # no anchors: -1, no launch
    t.close()

LEGS = {"differential": leg_differential, "far_apart_and_edges": leg_far_apart_and_edges, "errors": leg_errors}

def run_leg(name, tmp_path, timeout=300):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path)))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

def test_windowed_match_against_the_prefix_model_in_both_byte_orders(tmp_path): print(run_leg("differential", tmp_path))
def test_windows_far_apart_in_one_workgroup_and_astride_a_tile_edge(tmp_path): run_leg("far_apart_and_edges", tmp_path)
def test_bad_windows_and_sizes_write_nothing(tmp_path): run_leg("errors", tmp_path)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
