"""verifyBlockTree (include/zk_tree_block.h; DESIGN.md "A block against the resident tree") on the device: a block of real proofs decided against a resident tree of
depth 5 — deposits under the depth-5 key, their roots against the tree's states at the anchors, both keys of every record against the spent set, the accepted
sends' commitments appended — and compared with a Python restatement of the six steps over the models the suite already has: the single-proof verify symbols for
the proof step, the prefix roots of tests/test_tree_block_cpu.py for the anchor step and the tree after the append, model_pairs of tests/test_snset_pairs_cpu.py for
the spend step.  The leg runs in a process of its own under a time limit: `python tests/test_gpu_tree_block.py block <scratch dir>` is what the test starts."""
import os, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import workload as w
from test_snset_pairs_cpu import model_pairs
from test_tree_block_cpu import PrefixRoots, model_match

pytestmark = pytest.mark.gpu
DEPTH = 5

def sn(it): return it[2][3 if it[0] == "deposit" else 1]
def key(x): return bytes(x)[-20:]                                   # what common.BytesToAddress keeps of a hash; a pk address as it is
def flip(b): return bytes([b[0] ^ 1]) + b[1:]

def restate(items, proof_ok, leaves_blob, anchors, log, exempt, commit, with_set=True):
    """the six steps of include/zk_tree_block.h on Python lists -> (accepted, ok, anchor_of, the set's log after, the tree's leaves after)"""
    n = len(items); ok = list(proof_ok); anchor_of = [-1] * n; pr = PrefixRoots(leaves_blob, DEPTH)                                # 2. the proof step: given
    for i, it in enumerate(items):                                                                                                   # 3. the anchor step
        if ok[i] and it[0] == "deposit": anchor_of[i] = model_match(pr, anchors, [w.rev(it[2][0])])[0]; ok[i] = anchor_of[i] >= 0
    if with_set:                                                                                                                     # 4. the spend step
        pairs = [None if not ok[i] else (key(sn(it)), key(it[2][1])) if it[0] == "deposit" else (key(sn(it)),) for i, it in enumerate(items)]
        codes, log = model_pairs(log, exempt, pairs, commit); ok = [bool(o and not c) for o, c in zip(ok, codes)]
    after = list(leaves_blob) + ([w.rev(it[2][2]) for i, it in enumerate(items) if ok[i] and it[0] == "send"] if commit else [])     # 5. the append step
    return sum(ok), ok, anchor_of, log, after

class Stderr:
    """what the process writes to file descriptor 2 inside the block (the library prints there)"""
    def __init__(self, path): self.path = path
    def __enter__(self): sys.stderr.flush(); self.keep = os.dup(2); self.f = open(self.path, "wb"); os.dup2(self.f.fileno(), 2); return self
    def __exit__(self, *a): os.dup2(self.keep, 2); os.close(self.keep); self.f.close(); self.text = open(self.path, "rb").read()

def leg_block(tmp):
    from blockmaze_amd import engine as e
    for i, kind in enumerate(("send", "mint", "redeem", "deposit")): e.keygen(kind, os.path.join(tmp, kind + "pk.txt"), os.path.join(tmp, kind + "vk.txt"), seed=0xB10C4A2E + 7 * i)
    e.keygen("deposit", os.path.join(tmp, "deposit5pk.txt"), os.path.join(tmp, "deposit5vk.txt"), seed=55, tree_depth=DEPTH)
    z = e.Zk(); exempt = bytes(20)
    def mint(i): d = w.mint_instance(i); p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("mint", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    def redeem(i): d = w.mint_instance(i, redeem=True); p = z.GenRedeemProof(*w.mint_args(d)); assert z.VerifyRedeemProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("redeem", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    def send(i): d = w.send_instance(i); p = z.GenSendProof(*w.send_args(d)); a = [d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]; assert z.VerifySendProof(p, *a); return ("send", p, a, 0)
    def dep_args(d, rt): return [rt, d["pk_recv"], d["cmtB_old"], d["sn_old"], d["cmtB"], d["sn_s"]]
    # the tree: three "blocks" of eight commitments, each with one deposit's note among them
    ds = [w.deposit_instance(i, 8) for i in (1, 2, 3)]; tree = e.Tree(DEPTH); t = tree.h; leaves = []
    for j, d in enumerate(ds): assert z.TreeAppend(t, d["leaves"]) == 8 * (j + 1); leaves += [w.rev(x) for x in d["leaves"]]
    pr = PrefixRoots(leaves, DEPTH); anchors = [16, 8, 8]
    def deposit(d, size):
        p, rt = z.GenDepositProofTreeAt(*w.deposit_args(d), d["sk"], t, size); assert rt == w.rev(pr.root(size)) and z.VerifyDepositProofDepth(DEPTH, p, *dep_args(d, rt))
        assert not z.VerifyDepositProof(p, *dep_args(d, rt)); return ("deposit", p, dep_args(d, rt), 0)                          # (the depth-8 key is another key)
    D1, D2, D3 = deposit(ds[0], 8), deposit(ds[1], 16), deposit(ds[2], 24)                                                      # D3: a root of the tree, and no anchor's
    D1x = ("deposit", D1[1], [D2[2][0]] + D1[2][1:], 0); assert not z.VerifyDepositProofDepth(DEPTH, D1x[1], *D1x[2])           # D1's proof under the root of size 16: not its statement
    d8 = w.deposit_instance(4, 16); p8 = z.GenDepositProof(*w.deposit_args(d8), d8["leaves"], d8["rt"], d8["sk"]); D8 = ("deposit", p8, dep_args(d8, d8["rt"]), 0)
    assert z.VerifyDepositProof(p8, *D8[2]) and not z.VerifyDepositProofDepth(DEPTH, p8, *D8[2])                                 # a proof under the depth-8 key
    S1, S2, M1, R1 = send(1), send(2), mint(1), redeem(1); S1bad = ("send", S1[1], [S1[2][0], S1[2][1], flip(S1[2][2]), S1[2][3]], 0); assert not z.VerifySendProof(S1bad[1], *S1bad[2])
    items = [M1, D1, S1, D2, D3, D1x, D8, S1bad, R1, S2, M1]; n = len(items); recs = e.records_from_items(items)
    proof_ok = [True, True, True, True, True, False, False, False, True, True, True]
    def fresh():
        s = e.SpentSet(exempt); assert s.spend([key(sn(R1)), key(bytes(range(32)))]) == ([0, 0], 2); return s                  # R1's serial number is spent already
    s = fresh(); log0 = s.read_log(); root0 = tree.root(); assert tree.size() == 24 and root0 == pr.root(24)
    want0 = restate(items, proof_ok, leaves, anchors, log0, exempt, False); want1 = restate(items, proof_ok, leaves, anchors, log0, exempt, True)
    assert want0[1] == want1[1] == [True, True, True, True, False, False, False, False, False, True, False]                      # D3: no anchor; R1: spent before; the second M1: spent by the first
    assert want1[2] == [-1, 1, -1, 0, -1, -1, -1, -1, -1, -1, -1] and len(want1[3]) == 2 + 3 + 2 * 2 and len(want1[4]) == 26    # D1 at the LOWER of the two 8s, D2 at 16
    # commit = 0: the pool's call changes nothing
    got = z.VerifyBlockTree(None, recs, t, anchors, s.h, False); assert got == (want0[0], want0[1], want0[2], 2, 24), got
    assert tree.size() == 24 and tree.root() == root0 and s.size() == 2 and s.read_log() == log0
    assert z.VerifyBlockTree(None, recs, t, anchors, None, False) == restate(items, proof_ok, leaves, anchors, [], None, False, with_set=False)[:3] + (None, 24)   # no set: no spend step
    assert z.VerifyBlockTree(None, recs, t, [], s.h, False)[1:3] == ([True, False, True, False, False, False, False, False, False, True, False], [-1] * n)    # no anchor: no deposit
    assert z.VerifyBlockTree(None, recs, t, [24, 0], s.h, False)[1:3] == ([True, False, True, False, True, False, False, False, False, True, False], [-1, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1])
    # bad anchors and a block that cannot fit: -1 and nothing changed
    for bad in ([16, 25, 8], [16, -1], [1 << 40]):
        assert z.VerifyBlockTree(None, recs, t, bad, s.h, True) == (-1, [False] * n, [-1] * n, None, None), bad
    assert tree.size() == 24 and tree.root() == root0 and s.read_log() == log0
    full = e.Tree(1); full.append([bytes([1]) * 32, bytes([2]) * 32]); froot = full.root(); one = e.records_from_items([S1])
    with Stderr(os.path.join(tmp, "full.err")) as err: got = z.VerifyBlockTree(None, one, full.h, [2], s.h, True)
    assert got == (-1, [False], [-1], None, None) and full.size() == 2 and full.root() == froot and s.read_log() == log0
    assert b"do not fit" in err.text and b"deposit" not in err.text                                                                  # refused before any key is looked at
    assert z.VerifyBlockTree(None, one, full.h, [2], s.h, False) == (1, [True], [-1], 2, 2); full.close()                            # the pool's call appends nothing: it fits
    # commit = 1: the set advances as verifyBlockState would advance it, the tree grows by S1 then S2
    got = z.VerifyBlockTree(None, recs, t, anchors, s.h, True); assert got == (want1[0], want1[1], want1[2], len(want1[3]), 26), got
    assert s.read_log() == want1[3] and tree.size() == 26 and tree.root() == PrefixRoots(want1[4], DEPTH).root(26) and want1[4][24:] == [w.rev(S1[2][2]), w.rev(S2[2][2])]
    assert tree.roots_at([24, 8]) == [root0, pr.root(8)]
    # (verifyBlockState itself knows the depth-8 key only and rejects D1 and D2; what it does to the set is spend_pairs on the accepted records' keys, in record order)
    state = fresh(); pairs_sn = [sn(it) for i, it in enumerate(items) if want1[1][i]]; pairs_pk = [bytes(12) + it[2][1] if it[0] == "deposit" else None for i, it in enumerate(items) if want1[1][i]]
    assert z.SnSetSpendPairs(state.h, pairs_sn, pairs_pk) == (len(want1[3]), [False] * len(pairs_sn)) and state.read_log() == s.read_log(); state.close()
    # the same block again: every record is spent, nothing is appended
    assert z.VerifyBlockTree(None, recs, t, anchors, s.h, True) == (0, [False] * n, want1[2], len(want1[3]), 26) and tree.root() == PrefixRoots(want1[4], DEPTH).root(26) and s.read_log() == want1[3]
    # a reorganisation: tree and set back to the sizes stored before the block; the same call gives the first run's verdicts and the same root
    root1 = tree.root(); assert z.TreeRewind(t, 24) == 24 and z.SnSetRewind(s.h, 2) == 2 and tree.root() == root0 and s.read_log() == log0
    assert z.VerifyBlockTree(None, recs, t, anchors, s.h, True) == got and tree.root() == root1 and s.read_log() == want1[3]
    # tree = None: verifyBlockState without lists, under the depth-8 key
    a, b = fresh(), fresh()
    for commit in (False, True):
        rc, ok8, size8 = z.VerifyBlockState(None, recs, None, None, None, a.h, commit); assert z.VerifyBlockTree(None, recs, None, None, b.h, commit) == (rc, ok8, [-1] * n, size8, None)
        assert ok8 == [True, False, True, False, False, False, True, False, False, True, False] and a.read_log() == b.read_log()   # D8 is the only deposit that key accepts
    assert z.VerifyBlockTree(None, recs, None, [5], None, True) == z.VerifyBlockState(None, recs, None, None, None, None, True)[:2] + ([-1] * n, None, None); a.close(); b.close()
    # a block without deposits: verifyBlockFull's verdicts and set size
    nd = [M1, S1, R1, M1, S2, S1bad, S1]; a, b = fresh(), fresh(); scratch = e.Tree(DEPTH)
    rc, okf, sizef = z.VerifyBlockFull(nd, None, None, None, b.h, True); assert (rc, okf, sizef) == (3, [True, True, False, False, True, False, False], 5)
    assert z.VerifyBlockTree(None, nd, scratch.h, [0], a.h, True) == (rc, okf, [-1] * 7, sizef, 2) and a.read_log() == b.read_log() and scratch.root() == PrefixRoots(want1[4][24:], DEPTH).root(2)
    a.close(); b.close(); scratch.close()
    # behind one proof cache shared with verifyRecordsCached: the tag of a deposit record follows the key of the depth
    c = e.ProofCache(64); u = fresh(); assert z.TreeRewind(t, 24) == 24
    first = z.VerifyBlockTree(c, recs, t, anchors, u.h, False); h1 = c.stats(); second = z.VerifyBlockTree(c, recs, t, anchors, u.h, True); h2 = c.stats()
    assert first == (want0[0], want0[1], want0[2], 2, 24) and second == got and h1[0] == 0 and h2[0] - h1[0] == sum(proof_ok) and h2[1] == h1[1] + n - sum(proof_ok), (h1, h2)   # every valid record is a hit
    assert z.VerifyRecordsCached(c, [D8, S1]) == (2, [True, True]); h3 = c.stats(); assert (h3[0] - h2[0], h3[1] - h2[1]) == (1, 1)                        # S1 is known, D8 is verified and stored: depth-8 tag
    assert z.VerifyBlockTree(c, [D8, S1], t, [26], None, False)[:3] == (1, [False, True], [-1, -1]); h4 = c.stats(); assert (h4[0] - h3[0], h4[1] - h3[1]) == (1, 1)   # ... which is no hit at depth 5
    assert z.VerifyRecordsCached(c, [D1, D8]) == (1, [False, True]); h5 = c.stats(); assert (h5[0] - h4[0], h5[1] - h4[1]) == (1, 1)                        # and D1, stored under the depth-5 tag, is none at depth 8
    u.close(); s.close(); tree.close()

LEGS = {"block": leg_block}

def run_leg(name, tmp_path, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path)))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

def test_verify_block_tree(tmp_path): run_leg("block", tmp_path)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
