"""verifyChainAccounts (include/zk_accounts_chain.h; DESIGN.md "A stretch of the chain with accounts") on the device: segments of real proofs at depth 5 whose records
arrive with their old balance commitments ZEROED, decided in one call against the resident account table, tree and spent set, and compared exactly — return value,
verdicts, anchors mapped into A, the returned records, the three logs, the tree's root and all three sizes arrays — with the loop the header names as its
specification, run on a twin table, set and tree through the call that existed before it: verifyBlockAccounts(commit = 1) block after block, with the windows cut
from A.  The leg runs in a process of its own under a time limit: `python tests/test_gpu_chain_accounts.py chain <scratch dir>`."""
import os, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import workload as w
from test_gpu_block_accounts import ZERO, key, with_old

pytestmark = pytest.mark.gpu
DEPTH = 5

def loop(z, e, blocks, froms, a, tree, prior, window, s):
    """the specification, by the older call -> what Zk.VerifyChainAccounts returns, the records of the blocks that were looked at only"""
    A = list(prior); ok = []; of = []; recs = []; sizes = ([], [], []); nb = len(blocks); accepted = nb; n = sum(len(b) for b in blocks)
    def now(): return (a.size(), len(s.read_log()), tree.size())
    for b, (blk, frm) in enumerate(zip(blocks, froms)):
        hi = len(prior) + b; lo = max(0, hi - window)
        if blk:
            rc, okb, ofb, rb, asz, ssz, tsz = z.VerifyBlockAccounts(None, e.records_from_items([with_old(it, ZERO) for it in blk]), frm, a, tree.h, A[lo:hi], s.h, True); assert rc >= 0, (b, rc)
            ok += okb; of += [x + lo if x >= 0 else -1 for x in ofb]; recs += [r.tobytes() for r in rb]; assert (asz, ssz, tsz) == now()
            if rc != len(blk): accepted = b; break
        A.append(tree.size())
        for k, v in enumerate(now()): sizes[k].append(v)
    for k, v in enumerate(now()): sizes[k].extend([v] * (nb - accepted))
    return (accepted, ok + [False] * (n - len(ok)), of + [-1] * (n - len(of)), recs) + sizes

def leg_chain(tmp):
    import ctypes
    from blockmaze_amd import engine as e
    for i, kind in enumerate(("send", "mint")): e.keygen(kind, os.path.join(tmp, kind + "pk.txt"), os.path.join(tmp, kind + "vk.txt"), seed=0xACC8 + 7 * i)
    e.keygen("deposit", os.path.join(tmp, "deposit5pk.txt"), os.path.join(tmp, "deposit5vk.txt"), seed=57, tree_depth=DEPTH)
    z = e.Zk(); exempt = bytes(20); X, Y, Z, W = (bytes([0xB0 + k]) * 20 for k in range(4))
    def mint_of(d): p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("mint", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    def send_on(sk, value_old, r_old, i):
        """a send that spends the note (value_old, r_old) of key sk: the rest as workload.send_instance(i) draws it"""
        s = w.send_instance(i); d = dict(s, sk=sk, r_old=r_old, value_old=value_old); d["value_s"] = s["value_s"] % (value_old + 1); d["value"] = value_old - d["value_s"]
        d["sn_old"] = w.prf(sk, r_old); d["cmtA_old"] = w.cmt(value_old, d["sn_old"], r_old); d["sn"] = w.prf(sk, d["r"]); d["cmtS"] = w.cmts(d["value_s"], d["pk_recv"], d["r_s"], d["sn_old"]); d["cmtA"] = w.cmt(d["value"], d["sn"], d["r"])
        p = z.GenSendProof(*w.send_args(d)); a = [d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]; assert z.VerifySendProof(p, *a); return ("send", p, a, 0)
    dm = w.mint_instance(1); M = mint_of(dm); S = send_on(dm["sk"], dm["value"], dm["r"], 1); assert S[2][0] == M[2][2]                      # X: a mint, then a send made on the mint's cmtA
    Sstale = send_on(dm["sk"], dm["value_old"], dm["r_old"], 2); assert Sstale[2][0] == M[2][0]                                                  # ... and one made on X's value BEFORE the segment
    MY = mint_of(w.mint_instance(2)); MW = mint_of(w.mint_instance(3))
    dd = w.deposit_instance(1, 8); tree = e.Tree(DEPTH); twin = e.Tree(DEPTH); t = tree.h; assert z.TreeAppend(t, dd["leaves"]) == 8 == z.TreeAppend(twin.h, dd["leaves"]); root0 = tree.root()
    p, rt = z.GenDepositProofTreeAt(*w.deposit_args(dd), dd["sk"], t, 8); D = ("deposit", p, [rt, dd["pk_recv"], dd["cmtB_old"], dd["sn_old"], dd["cmtB"], dd["sn_s"]], 0); assert z.VerifyDepositProofDepth(DEPTH, p, *D[2])
    Mbad = ("mint", M[1][:100] + ("0" if M[1][100] != "0" else "1") + M[1][101:], M[2], M[3]); assert not z.VerifyMintProof(Mbad[1], *Mbad[2], Mbad[3])
    start = {X: M[2][0], Y: MY[2][0], Z: D[2][2], W: MW[2][0]}; kept = []
    def zeroed(items): return e.records_from_items([with_old(it, ZERO) for it in items])                                                          # the records as they arrive: no old
    def fresh():
        a = e.AccountTable(); assert z.AcctsSet(a, list(start), list(start.values())) == 0; s = e.SpentSet(exempt); assert s.spend([key(bytes(range(32)))]) == ([0], 1); kept.extend([a, s]); return a, s
    def states(a, s, tr): return (a.read_log(), z.AcctsGet(a, [X, Y, Z, W]), s.read_log(), tr.size(), tr.root())
    def seg(blocks, senders):
        first = [0]
        for blk in blocks: first.append(first[-1] + len(blk))
        return [it for blk in blocks for it in blk], [f for frm in senders for f in frm], first
    def both(blocks, senders, window, prior=(8,), state=None, keep=False):
        """the call on (a, s, tree), the loop on (b, r, twin), both from the same state -> (the call's answer, the call's states); everything compared"""
        (a, s), (b, r) = state if state else (fresh(), fresh()); items, frm, first = seg(blocks, senders); n = len(items)
        filled = z.AcctsFillRecords(b, frm, zeroed(items), True) if n else None                                      # the chained fill over the whole segment, by the older entry
        got = z.VerifyChainAccounts(None, zeroed(items) if n else e.records_from_items([M])[:0], frm, first, a, t, list(prior), window, s.h)
        want = loop(z, e, blocks, senders, b, twin, list(prior), window, r)
        assert got[:3] == want[:3] and got[4:] == want[4:], (got[:3], got[4:], want[:3], want[4:])
        assert [x.tobytes() for x in got[3][:len(want[3])]] == want[3]                                             # the blocks the loop looked at: the statements it verified
        if n: assert filled[0] == 0 and got[3].tobytes() == filled[1].tobytes()                                    # ... and the whole segment: zkAcctsFillRecords(chained = 1)
        st = states(a, s, tree); assert st == states(b, r, twin)
        if not keep: assert z.TreeRewind(t, 8) == 8 and z.TreeRewind(twin.h, 8) == 8 and tree.root() == root0
        return got, st, ((a, s), (b, r))

    # 1. accepted whole: X's chain crosses a block border, an empty block, and a deposit anchored on a prior size (A[0] = 8)
    got, st, pairs = both([[M], [S, MY], [], [D]], [[X], [X, Y], [], [Z]], 8, keep=True)
    assert got[:3] == (4, [True] * 4, [-1, -1, -1, 0]) and got[4:] == ([5, 7, 7, 8], [2, 4, 4, 6], [8, 9, 9, 9]), (got[:3], got[4:])
    assert bytes(got[3]["args"][1][0]) == M[2][2] and st[1] == [S[2][3], MY[2][2], D[2][4], start[W]] and st[3] == 9
    # 6. a reorganisation: all three back to the sizes after block 0, and the tail imported again ends in the same states
    (a, s), (b, r) = pairs
    for acc, sn_set, tr in ((a, s, tree), (b, r, twin)): assert z.AcctsRewind(acc, got[4][0]) == 0 and z.SnSetRewind(sn_set.h, got[5][0]) == got[5][0] and z.TreeRewind(tr.h, got[6][0]) == got[6][0]
    again, st2, _ = both([[S, MY], [], [D]], [[X, Y], [], [Z]], 8, prior=(8, got[6][0]), state=pairs)
    assert again[:3] == (3, [True] * 3, [-1, -1, 0]) and again[4:] == (got[4][1:], got[5][1:], got[6][1:]) and st2 == st
    # 2. X's send in block 1 made against the value before the segment: one block accepted; D after it in the block is not decided; the states are those after block 0
    got, st, _ = both([[M, MY], [Sstale, D], [MW]], [[X, Y], [X, Z], [W]], 8)
    assert got[:3] == (1, [True, True, False, False, False], [-1] * 5) and got[4:] == ([6] * 3, [3] * 3, [8] * 3), (got[:3], got[4:])
    assert bytes(got[3]["args"][2][0]) == M[2][2] != Sstale[2][0] and st[1] == [M[2][2], MY[2][2], start[Z], start[W]]
    # 3. the mutated mint first: nothing is accepted and nothing moves, bit for bit
    a, s = fresh(); b, r = fresh(); before = states(a, s, tree)
    got, st, _ = both([[Mbad, MY], [S]], [[X, Y], [X]], 8, state=((a, s), (b, r))); assert got[:3] == (0, [False] * 3, [-1] * 3) and got[4:] == ([4] * 2, [1] * 2, [8] * 2) and st == before
    # 4. the window: D's only anchor, A[0] = 8, lies outside a window of one in block 2 (A = 8, 8, 9), and inside a window of three
    got, _, _ = both([[M], [S], [D]], [[X], [X], [Z]], 1); assert got[:3] == (2, [True, True, False], [-1] * 3) and got[6] == [8, 9, 9], got[:3]
    got, _, _ = both([[M], [S], [D]], [[X], [X], [Z]], 3); assert got[:3] == (3, [True] * 3, [-1, -1, 0]), got[:3]
    # 5. empty calls
    got, st, _ = both([[], []], [[], []], 8); assert got[:3] == (2, [], []) and got[4:] == ([4, 4], [1, 1], [8, 8])
    got, st, _ = both([], [], 8); assert got[:3] == (0, [], []) and got[4:] == ([], [], [])
    # 7. bad arguments: -1, recs is not written, the states are unchanged
    a, s = fresh(); before = states(a, s, tree); items, frm, first = seg([[M], [S, MY]], [[X], [X, Y]]); n = 3; clean = zeroed(items).tobytes()
    def refused(got): return got[:3] == (-1, [False] * n, [-1] * n) and got[3].tobytes() == clean and got[4:] == (None, None, None) and states(a, s, tree) == before
    assert refused(z.VerifyChainAccounts(None, zeroed(items), frm, first, None, t, [8], 8, s.h))                    # no table
    assert refused(z.VerifyChainAccounts(None, zeroed(items), frm, [0, 1, 2], a, t, [8], 8, s.h))                   # block_first does not end at n
    assert refused(z.VerifyChainAccounts(None, zeroed(items), frm, first, a, t, [8, 9], 8, s.h))                    # a prior anchor above the tree
    assert refused(z.VerifyChainAccounts(None, zeroed(items), frm, first, a, None, [8], 8, s.h))                    # no tree
    L = e.lib(); L.verifyChainAccounts.restype = ctypes.c_int; recs = zeroed(items); ok = (ctypes.c_ubyte * n)(7, 7, 7); of = (ctypes.c_int32 * n)(7, 7, 7); bf = (ctypes.c_int * 3)(*first); pa = (ctypes.c_longlong * 1)(8)
    assert L.verifyChainAccounts(None, recs.ctypes.data_as(ctypes.c_void_p), None, n, bf, 2, ctypes.c_void_p(a.h), ctypes.c_void_p(t), pa, 1, 8, ctypes.c_void_p(s.h), ok, of, None, None, None) == -1   # no froms
    assert list(ok) == [0] * n and list(of) == [-1] * n and recs.tobytes() == clean and states(a, s, tree) == before
    assert z.VerifyChainAccounts(None, zeroed(items), frm, first, a, t, [8], 8, s.h)[0] == 2                         # and the same call with its arguments in order
    for x in kept: x.close()
    tree.close(); twin.close()

LEGS = {"chain": leg_chain}

def run_leg(name, tmp_path, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path)))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

def test_verify_chain_accounts(tmp_path): run_leg("chain", tmp_path)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
