"""verifyChainTree (include/zk_tree_chain.h; DESIGN.md "A stretch of the chain") on the device: segments of real proofs decided against a resident tree of depth 5
in one call, and compared exactly — verdicts, anchors, the set's log, the tree's root and size, the sizes after every block, the return value — with the loop the
header names as its specification, run on a twin tree and a twin set through the calls that existed before it: verifyBlockTree(commit = 1) block after block, and
zkSnSetRewind / zkTreeRewind for the first block with a rejected record.  One deposit is proved against the tree AFTER block 0's send, which no single older call
can decide without a commit in between.  The leg runs in a process of its own under a time limit: `python tests/test_gpu_tree_chain.py chain <scratch dir>` is
what the test starts."""
import os, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import workload as w
from test_gpu_tree_block import Stderr, flip, key, sn
from test_tree_block_cpu import PrefixRoots

pytestmark = pytest.mark.gpu
DEPTH, DEEP = 5, 10

def loop(z, cache, items, first, t, prior, window, s):
    """the specification, by the older calls -> what Zk.VerifyChainTree returns"""
    n = len(items); nb = len(first) - 1; A = list(prior); ok = [False] * n; of = [-1] * n; ss = []; ts = []; accepted = nb
    for b in range(nb):
        hi = len(prior) + b; lo = max(0, hi - window); block = items[first[b]:first[b + 1]]; set0 = z.SnSetSize(s) if s else None; tree0 = tree_size(z, t)
        if not len(block): A.append(tree0); ss.append(set0); ts.append(tree0); continue                    # nothing to decide: the sizes of the block before it
        rc, okb, ofb, ssz, tsz = z.VerifyBlockTree(cache, block, t, A[lo:hi], s, True); assert rc >= 0, (b, rc)
        if rc != len(block):
            assert z.TreeRewind(t, tree0) == tree0 and (not s or z.SnSetRewind(s, set0) == set0)
            rc, okb, ofb, _, _ = z.VerifyBlockTree(cache, block, t, A[lo:hi], s, False); assert 0 <= rc < len(block); accepted = b
        ok[first[b]:first[b + 1]] = okb; of[first[b]:first[b + 1]] = [a + lo if a >= 0 else -1 for a in ofb]
        if accepted == b: break
        A.append(tsz); ss.append(ssz); ts.append(tsz)
    ss += [z.SnSetSize(s) if s else None] * (nb - accepted); ts += [tree_size(z, t)] * (nb - accepted)
    return accepted, ok, of, (ss if s else None), ts
def tree_size(z, t):
    import ctypes
    from blockmaze_amd import engine as e
    n = ctypes.c_uint64(0); assert e.lib().zkgpu_tree_size(ctypes.c_void_p(t), ctypes.byref(n)) == 0; return int(n.value)

def leg_chain(tmp):
    from blockmaze_amd import engine as e
    for i, kind in enumerate(("send", "mint")): e.keygen(kind, os.path.join(tmp, kind + "pk.txt"), os.path.join(tmp, kind + "vk.txt"), seed=0xC4A10000 + 7 * i)
    for d in (DEPTH, DEEP): e.keygen("deposit", os.path.join(tmp, "deposit%dpk.txt" % d), os.path.join(tmp, "deposit%dvk.txt" % d), seed=50 + d, tree_depth=d)
    z = e.Zk(); exempt = bytes(20)
    def mint(i): d = w.mint_instance(i); p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("mint", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    def send(i): d = w.send_instance(i); p = z.GenSendProof(*w.send_args(d)); a = [d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]; assert z.VerifySendProof(p, *a); return ("send", p, a, 0)
    def dep_args(d, rt): return [rt, d["pk_recv"], d["cmtB_old"], d["sn_old"], d["cmtB"], d["sn_s"]]
    # the tree before the segment: three blocks of eight commitments, each with one deposit's note among them; `twin` is driven by the loop
    ds = [w.deposit_instance(i, 8) for i in (1, 2, 3)]; tree = e.Tree(DEPTH); twin = e.Tree(DEPTH); t = tree.h; leaves = []
    for d in ds: assert z.TreeAppend(t, d["leaves"]) == z.TreeAppend(twin.h, d["leaves"]); leaves += [w.rev(x) for x in d["leaves"]]
    S1, S2, S3, M1, M2 = send(1), send(2), send(3), mint(1), mint(2); S2bad = ("send", S2[1], [S2[2][0], S2[2][1], flip(S2[2][2]), S2[2][3]], 0); assert not z.VerifySendProof(S2bad[1], *S2bad[2])
    def cm(S): return w.rev(S[2][2])
    def deposit(d, size, by_hand=()):
        """a deposit proved against the first `size` leaves of the tree with the commitments of `by_hand` appended for the while"""
        if by_hand: assert z.TreeAppend(t, [S[2][2] for S in by_hand]) == 24 + len(by_hand)
        p, rt = z.GenDepositProofTreeAt(*w.deposit_args(d), d["sk"], t, size); assert z.TreeRewind(t, 24) == 24
        assert rt == w.rev(PrefixRoots(leaves + [cm(S) for S in by_hand], DEPTH).root(size)) and z.VerifyDepositProofDepth(DEPTH, p, *dep_args(d, rt)); return ("deposit", p, dep_args(d, rt), 0)
    D1, D3 = deposit(ds[0], 8), deposit(ds[2], 24)
    Dafter = deposit(ds[1], 25, (S1,))                                                                     # against the root AFTER a block that holds S1 alone among its sends
    Dend = deposit(ds[2], 26, (S1, S2))                                                                    # ... after S1 and S2
    root0 = tree.root(); assert tree.size() == 24 and twin.root() == root0; prior = [8, 16, 24]          # the start of the segment is the last prior anchor
    sets = []
    def fresh():
        s = e.SpentSet(exempt); assert s.spend([key(bytes(range(32)))]) == ([0], 1); sets.append(s); return s
    def both(items, first, window, prior=prior, with_set=True, cache=None, keep=False):
        """the call on (tree, a), the loop on (twin, b), both from the state before the segment -> the call's answer; everything compared"""
        a, b = (fresh(), fresh()) if with_set else (None, None)
        got = z.VerifyChainTree(cache, items, first, t, prior, window, a.h if a else None); want = loop(z, None, items, first, twin.h, prior, window, b.h if b else None)
        assert got == want, (got, want)
        assert tree.size() == twin.size() == got[4][-1 if got[0] == len(first) - 1 else got[0]] if len(first) > 1 else tree.size() == twin.size() == 24
        assert tree.root() == twin.root() and (not with_set or a.read_log() == b.read_log())
        state = (tree.size(), tree.root(), a.read_log() if a else None)
        if not keep: assert z.TreeRewind(t, 24) == 24 and z.TreeRewind(twin.h, 24) == 24 and tree.root() == root0
        return got, state, (a, b)
    def seg(*blocks):
        first = [0]
        for blk in blocks: first.append(first[-1] + len(blk))
        return [it for blk in blocks for it in blk], first

    # a valid segment of four blocks; Dafter in block 1 matches s_0 = A[3], the size after block 0, which exists in no tree before the call
    items, first = seg([S1, M1], [Dafter, D1], [S2], [D3, M2]); n = len(items)
    got, state, _ = both(items, first, 8); assert got == (4, [True] * n, [-1, -1, 3, 0, -1, 2, -1], [1 + 2, 1 + 6, 1 + 7, 1 + 10], [25, 25, 26, 26]), got
    assert state[0] == 26 and state[1] == PrefixRoots(leaves + [cm(S1), cm(S2)], DEPTH).root(26)
    assert state[2][1:] == [key(sn(S1)), key(sn(M1)), key(sn(Dafter)), Dafter[2][1], key(sn(D1)), D1[2][1], key(sn(S2)), key(sn(D3)), D3[2][1], key(sn(M2))]
    # a bad proof in block 2: two blocks accepted, the state as after block 1, block 3 not decided
    items, first = seg([S1, M1], [Dafter, D1], [M2, S2bad, S3], [D3])
    got, state, _ = both(items, first, 8); assert got == (2, [True] * 4 + [True, False, True] + [False], [-1, -1, 3, 0, -1, -1, -1, -1], [3, 7, 7, 7], [25, 25, 25, 25]), got
    assert state[0] == 25 and len(state[2]) == 7
    # block 2 spends a serial number of block 0 again; the deposit after it in the block keeps its verdict and its anchor
    items, first = seg([S1, M1], [D1], [S2, M1, Dafter], [D3])
    got, state, _ = both(items, first, 8); assert got == (2, [True] * 3 + [True, False, True] + [False], [-1, -1, 0, -1, -1, 3, -1], [3, 5, 5, 5], [25, 25, 25, 25]), got
    # a window: Dafter's anchor s_0 = A[3] lies one block outside a window of 2 in block 3, and is the oldest anchor of a window of 3
    items, first = seg([S1], [S2], [S3], [Dafter])
    got, _, _ = both(items, first, 2); assert got == (3, [True, True, True, False], [-1] * 4, [2, 3, 4, 4], [25, 26, 27, 27]), got
    got, _, _ = both(items, first, 3); assert got == (4, [True] * 4, [-1, -1, -1, 3], [2, 3, 4, 6], [25, 26, 27, 27]), got
    # a deposit anchored at its own block's end is no deposit of that block; one block later it is
    got, _, _ = both(*seg([S1], [S2, Dend]), 8); assert got[:3] == (1, [True, True, False], [-1] * 3), got
    got, _, _ = both(*seg([S1], [S2], [Dend]), 8); assert got[:3] == (3, [True] * 3, [-1, -1, 4]), got
    # empty blocks: their sizes are those of the block before them, and they count as anchors
    got, _, _ = both(*seg([], [S1], [], [Dafter], []), 2); assert got == (5, [True, True], [-1, 4], [1, 2, 2, 4, 4], [24, 25, 25, 25, 25]), got   # (A[4] = s_1 and A[5] = s_2 are the same size: the lower one)
    # no block at all, and no window at all
    got, state, _ = both([], [0], 8); assert got == (0, [], [], [], []) and state[0] == 24 and len(state[2]) == 1, got
    got, _, _ = both(*seg([S1], [D1], [M1]), 0); assert got[:3] == (1, [True, False, False], [-1] * 3), got
    got, _, _ = both(*seg([S1], [M1]), 0); assert got[0] == 2
    # a segment that does not fit its tree, a bad prior anchor, a malformed block_first: -1 and nothing changed, before any key is looked at
    a = fresh(); log0 = a.read_log(); full = e.Tree(1); full.append([bytes([1]) * 32, bytes([2]) * 32]); froot = full.root(); items, first = seg([M1], [S1])
    with Stderr(os.path.join(tmp, "full.err")) as err: got = z.VerifyChainTree(None, items, first, full.h, [2], 4, a.h)
    assert got == (-1, [False] * 2, [-1] * 2, None, None) and full.size() == 2 and full.root() == froot and a.read_log() == log0 and b"do not fit" in err.text and b"mint" not in err.text; full.close()
    for bad in ([16, 25, 8], [16, -1], [1 << 40]): assert z.VerifyChainTree(None, items, first, t, bad, 4, a.h) == (-1, [False] * 2, [-1] * 2, None, None), bad
    for bad in ([0, 2, 1], [0, 1, 1], [1, 1, 2], [0, 3, 2]): assert z.VerifyChainTree(None, items, bad, t, prior, 4, a.h)[0] == -1, bad
    assert z.VerifyChainTree(None, items, first, t, prior, -1, a.h)[0] == -1 and tree.size() == 24 and tree.root() == root0 and a.read_log() == log0
    # the same segment twice: the second time block 0 is rejected and nothing changes
    items, first = seg([S1, M1], [Dafter, D1], [S2], [D3, M2]); n = len(items)
    got, state, (a, b) = both(items, first, 8, keep=True); assert got[0] == 4
    again = z.VerifyChainTree(None, items, first, t, prior + got[4], 8, a.h); want = loop(z, None, items, first, twin.h, prior + got[4], 8, b.h)
    assert again == want == (0, [False, False] + [False] * 5, [-1] * n, [11] * 4, [26] * 4), (again, want)
    assert (tree.size(), tree.root(), a.read_log()) == state and twin.root() == state[1] and b.read_log() == state[2]
    assert z.TreeRewind(t, 24) == 24 and z.TreeRewind(twin.h, 24) == 24
    # a shared proof cache: the first pass stores every record, the second pass after a rewind is all hits
    c = e.ProofCache(64); a = fresh(); first_pass = z.VerifyChainTree(c, items, first, t, prior, 8, a.h); h1 = c.stats(); assert first_pass == got and h1[0] == 0 and h1[1] == n, h1
    assert z.TreeRewind(t, 24) == 24 and z.SnSetRewind(a.h, 1) == 1
    assert z.VerifyChainTree(c, items, first, t, prior, 8, a.h) == got; h2 = c.stats(); assert h2[0] - h1[0] == n and h2[1] == h1[1], (h1, h2); assert z.TreeRewind(t, 24) == 24
    for s in sets: s.close()
    tree.close(); twin.close()

    # without a set, 600 blocks of the same send and the same deposit at depth 10: the anchors of the segment cross two tile edges of the compare
    deep = e.Tree(DEEP); dtwin = e.Tree(DEEP); d = ds[0]; assert z.TreeAppend(deep.h, d["leaves"]) == 8 == z.TreeAppend(dtwin.h, d["leaves"])
    p, rt = z.GenDepositProofTreeAt(*w.deposit_args(d), d["sk"], deep.h, 8); D10 = ("deposit", p, dep_args(d, rt), 0); assert z.VerifyDepositProofDepth(DEEP, p, *D10[2])
    recs = e.records_from_items([S1, D10] * 600); first = list(range(0, 1201, 2)); sizes = [9 + b for b in range(600)]
    for window, accepted in ((4, 4), (700, 600)):
        got = z.VerifyChainTree(None, recs, first, deep.h, [8], window, None); want = loop(z, None, recs, first, dtwin.h, [8], window, None)
        assert got[0] == want[0] == accepted and got[3] is None and got[4] == want[4] == sizes[:accepted] + [8 + accepted] * (600 - accepted), (window, got[0], want[0])
        assert got[1] == want[1] == [True] * (2 * accepted) + ([True, False] if accepted < 600 else []) + [False] * (2 * (600 - accepted) - (2 if accepted < 600 else 0))
        assert got[2] == want[2] == [-1, 0] * accepted + [-1] * (2 * (600 - accepted))
        assert deep.size() == dtwin.size() == 8 + accepted and deep.root() == dtwin.root()
        deep.rewind(8); dtwin.rewind(8)
    deep.close(); dtwin.close()

LEGS = {"chain": leg_chain}

def run_leg(name, tmp_path, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path)))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

def test_verify_chain_tree(tmp_path): run_leg("chain", tmp_path)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
