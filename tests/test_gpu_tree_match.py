"""The anchor step on the device (blockmaze_amd/csrc/gpu_tree.hip: CommitmentTree::match_roots, k_tree_match_roots; include/zkgpu.h: zkgpu_tree_match_roots)
against the Python model of tests/test_tree_block_cpu.py: model_levels / model_root over the PREFIXES of the leaf list, and for each RT the lowest anchor whose
prefix root it equals.  Anchor lists cross the LDS tile of 256 roots and end in a partly filled one, record counts cross the wave and the workgroup, and the RTs
hold every way of being almost a root.  Every leg runs in a process of its own under a time limit: `python tests/test_gpu_tree_match.py <leg> <scratch dir>` is
what each test starts."""
import ctypes, os, random, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import workload as w
from test_tree_block_cpu import PrefixRoots, model_match, seeded_leaves

pytestmark = pytest.mark.gpu
TREES = [(1, 2), (2, 4), (8, 200), (32, 1000)]                  # (depth, leaves)
ANCHORS = [0, 1, 255, 256, 257, 600]                            # k_tree_match_roots takes the roots in tiles of 256
RECORDS = [0, 1, 63, 64, 65, 257, 1000]
POOL = 150                                                      # distinct sizes a large tree's anchors are drawn from (each costs the model one walk in Python)

def flip(b, byte, bit): b = bytearray(b); b[byte] ^= bit; return bytes(b)

def size_pools(rng, n):
    """(the sizes anchor lists are drawn from, a few sizes that stay outside every list: their roots are roots of the tree and no anchor's)"""
    outside = [1] if n == 2 else [3] if n == 4 else [7, n // 2, n - 1]
    marks = [0, 1, 2, n - 2, n] + [(1 << k) + s for k in range(1, 10) for s in (-1, 0, 1)] + [rng.randrange(n + 1) for _ in range(POOL)]
    inside = [m for m in range(n + 1) if m not in outside] if n + 1 <= POOL + 60 else sorted(set(m for m in marks if 0 <= m <= n and m not in outside))[:POOL]
    return inside, outside

def anchor_list(rng, n, length, inside):
    """`length` sizes, unsorted and with repeats; from three entries on, size 0 is among them and the current size n twice"""
    if length == 0: return []
    if length == 1: return [n]
    a = [rng.choice(inside) for _ in range(length)]
    if length >= 3: p0, p1, p2 = rng.sample(range(length), 3); a[p0] = 0; a[p1] = n; a[p2] = n
    return a

def rt_cases(pr, n, sizes, outside):
    """RTs in blob order: each anchor's root; a root with bit 0 of its first byte flipped; with the last bit of its last byte
    flipped (a compare that stops after the first word takes it for the root); the root of a size that is no anchor; a root in the other byte order; 32 zero bytes"""
    roots = [pr.root(m) for m in dict.fromkeys(sizes)] or [pr.root(n)]; assert outside and not set(outside) & set(sizes)
    out = roots + [flip(r, 0, 1) for r in roots[:8]] + [flip(r, 31, 0x80) for r in roots[:8]] + [flip(r, 31, 1) for r in roots[-4:]] + [pr.root(m) for m in outside] + [w.rev(r) for r in roots[:8]]
    assert all(r != w.rev(r) for r in out)                                                            # no palindrome: a root in the other order must not match
    return out + [bytes(32)]

def leg_differential(tmp):
    from blockmaze_amd import engine as e
    calls = 0; matched = 0
    for depth, n in TREES:
        leaves = seeded_leaves(n, 300 + depth); t = e.Tree(depth); t.append(leaves[:n // 2]); t.append(leaves[n // 2:]); assert t.size() == n
        pr = PrefixRoots(leaves, depth); rng = random.Random(depth); inside, outside = size_pools(rng, n)
        for length in ANCHORS:
            sizes = anchor_list(rng, n, length, inside); cases = rt_cases(pr, n, sizes, outside)
            for q in RECORDS:
                rts = [cases[i % len(cases)] for i in range(q)]; rng.shuffle(rts); want = model_match(pr, sizes, rts); before = t.state_launches()
                got = t.match_roots(sizes, rts); assert got == want, (depth, length, q, [i for i in range(q) if got[i] != want[i]][:8])
                assert t.state_launches() - before == (2 if q and length else 0), (depth, length, q)   # the roots, then the compare: two launches whatever q and m are
                got = t.match_roots(sizes, [w.rev(r) for r in rts], hash_order=True); assert got == want, (depth, length, q, "hash order")
                assert t.state_launches() - before == (4 if q and length else 0)
                if not length: assert got == [-1] * q
                calls += 2; matched += sum(x >= 0 for x in want)
                if q >= len(cases) and length >= 3:                                                       # every kind of case is in: roots found at their LOWEST index, the rest not found
                    assert set(want) >= {-1, sizes.index(0), sizes.index(n)} and sizes.index(n) < len(sizes) - 1
        t.close()
    print("calls", calls, "records matched", matched); assert matched > 1000

FILL = 0x5A5A5A5A
def leg_errors_and_rewind(tmp):
    from blockmaze_amd import engine as e
    L = e.lib(); depth, n = 20, 300; leaves = seeded_leaves(n, 77); other = seeded_leaves(200, 78); t = e.Tree(depth); t.append(leaves); pr = PrefixRoots(leaves, depth)
    h = ctypes.c_void_p(t.h); out = (ctypes.c_int32 * 4)(*([FILL] * 4)); rts = pr.root(300) + pr.root(250) + pr.root(0) + bytes(32); z = ctypes.c_size_t
    def u64s(v): return (ctypes.c_uint64 * max(1, len(v)))(*v)
    before = t.state_launches(); root = t.root()
    bad = [L.zkgpu_tree_match_roots(h, u64s([0, 301, 1]), z(3), rts, z(4), 0, out), L.zkgpu_tree_match_roots(h, u64s([1 << 40]), z(1), rts, z(4), 0, out),      # a size above the tree's
           L.zkgpu_tree_match_roots(h, None, z(1), rts, z(4), 0, out), L.zkgpu_tree_match_roots(h, u64s([1]), z(1), None, z(4), 0, out),                          # a null pointer with a count
           L.zkgpu_tree_match_roots(h, u64s([1]), z(1), rts, z(4), 0, None), L.zkgpu_tree_match_roots(h, u64s([1]), z(1 << 31), rts, z(4), 0, out),              # 2^31 anchors
           L.zkgpu_tree_match_roots(None, u64s([1]), z(1), rts, z(4), 0, out)]
    assert bad == [-2] * len(bad) and list(out) == [FILL] * 4 and t.state_launches() == before and t.size() == n and t.root() == root, bad   # ZKGPU_ERR_ARG, nothing written
    assert L.zkgpu_tree_match_roots(h, None, z(0), None, z(0), 1, None) == 0 and t.state_launches() == before                                  # nothing to do is a valid call
    sizes = [300, 250, 0, 250]; assert t.match_roots(sizes, [rts[32 * i:32 * i + 32] for i in range(4)]) == [0, 1, 2, -1]
    # a reorganisation: below the anchor the same call fails; grown back with other leaves, the anchor names ANOTHER state and matches that state's root only
    t.rewind(260); before = t.state_launches()
    assert L.zkgpu_tree_match_roots(h, u64s(sizes), z(4), rts, z(4), 0, out) == -2 and list(out) == [FILL] * 4 and t.state_launches() == before
    with pytest.raises(e.ZkGpuError): t.match_roots(sizes, [pr.root(250)])
    assert t.match_roots([260, 250, 0], [pr.root(260), pr.root(250), pr.root(300)]) == [0, 1, -1]
    t.append(other[:140]); now = PrefixRoots(leaves[:260] + other[:140], depth); assert t.size() == 400 and now.root(300) != pr.root(300) and now.root(250) == pr.root(250)
    assert t.match_roots(sizes, [pr.root(300), now.root(300), pr.root(250), now.root(400)]) == [-1, 0, 1, -1]
    assert t.match_roots(sizes + [400], [now.root(400), w.rev(now.root(400))]) == [4, -1] and t.match_roots(sizes + [400], [w.rev(now.root(400))], hash_order=True) == [4]
    t.close()

LEGS = {"differential": leg_differential, "errors_and_rewind": leg_errors_and_rewind}

def run_leg(name, tmp_path, timeout=300):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path)))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

def test_match_against_the_prefix_model_in_both_byte_orders(tmp_path): print(run_leg("differential", tmp_path))
def test_bad_sizes_write_nothing_and_a_rewound_anchor_names_the_new_state(tmp_path): run_leg("errors_and_rewind", tmp_path)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
