"""verifyBlockAccounts (include/zk_accounts.h; DESIGN.md "Account table") on the device: a block of real proofs at depth 5 whose records arrive with their old
balance commitments ZEROED, decided from the resident account table, tree and spent set, against a Python loop that restates core/state_processor.go over code
that was here before: `old` from a dict, the single-proof verify symbols, the prefix roots of tests/test_tree_block_cpu.py, model_pairs of
tests/test_snset_pairs_cpu.py.  The leg runs in a process of its own under a time limit: `python tests/test_gpu_block_accounts.py block <scratch dir>`."""
import os, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import workload as w
from test_snset_pairs_cpu import model_pairs
from test_tree_block_cpu import PrefixRoots, model_match

pytestmark = pytest.mark.gpu
DEPTH = 5; ZERO = bytes(32)
OLD = {"mint": 0, "redeem": 0, "send": 0, "deposit": 2}; NEW = {"mint": 2, "redeem": 2, "send": 3, "deposit": 4}

def sn(it): return it[2][3 if it[0] == "deposit" else 1]
def key(x): return bytes(x)[-20:]
def with_old(it, old): a = list(it[2]); a[OLD[it[0]]] = old; return (it[0], it[1], a, it[3])

def oracle(z, items, froms, state, leaves_blob, anchors, log, exempt):
    """the reference's loop: old := state[from]; the proof under that statement; the deposit's root among the anchors; the keys against the set; then state[from] :=
    new and the keys are burnt.  The first failure ends the block.  -> (leading accepted, the statements as verified up to there, anchor_of, state, log, leaves)"""
    cur = dict(state); pr = PrefixRoots(leaves_blob, DEPTH); seen = []; anchor_of = []; log = list(log); sends = []
    for it, frm in zip(items, froms):
        it = with_old(it, cur.get(frm, ZERO)); seen.append(it); a = it[2]; anchor_of.append(-1)
        ok = (z.VerifyMintProof(it[1], a[0], a[1], a[2], it[3]) if it[0] == "mint" else z.VerifySendProof(it[1], *a) if it[0] == "send" else z.VerifyDepositProofDepth(DEPTH, it[1], *a))
        if ok and it[0] == "deposit": anchor_of[-1] = model_match(pr, anchors, [w.rev(a[0])])[0]; ok = anchor_of[-1] >= 0
        if ok:
            codes, after = model_pairs(log, exempt, [(key(sn(it)), key(a[1])) if it[0] == "deposit" else (key(sn(it)),)], True); ok = not codes[0]
            if ok: log = after
        if not ok: return len(seen) - 1, seen, anchor_of, None, None, None
        cur[frm] = a[NEW[it[0]]]
        if it[0] == "send": sends.append(w.rev(a[2]))
    return len(items), seen, anchor_of, cur, log, list(leaves_blob) + sends

def leg_block(tmp):
    from blockmaze_amd import engine as e
    for i, kind in enumerate(("send", "mint")): e.keygen(kind, os.path.join(tmp, kind + "pk.txt"), os.path.join(tmp, kind + "vk.txt"), seed=0xACC7 + 7 * i)
    e.keygen("deposit", os.path.join(tmp, "deposit5pk.txt"), os.path.join(tmp, "deposit5vk.txt"), seed=56, tree_depth=DEPTH)
    z = e.Zk(); exempt = bytes(20); X, Y, Z, W = (bytes([0xA0 + k]) * 20 for k in range(4))
    def mint_of(d): p = z.GenMintProof(*w.mint_args(d)); assert z.VerifyMintProof(p, d["cmtA_old"], d["sn_old"], d["cmtA"], d["value_s"]); return ("mint", p, [d["cmtA_old"], d["sn_old"], d["cmtA"]], d["value_s"])
    def send_on(sk, value_old, r_old, i):
        """a send that spends the note (value_old, r_old) of key sk: the rest as workload.send_instance(i) draws it"""
        s = w.send_instance(i); d = dict(s, sk=sk, r_old=r_old, value_old=value_old); d["value_s"] = s["value_s"] % (value_old + 1); d["value"] = value_old - d["value_s"]
        d["sn_old"] = w.prf(sk, r_old); d["cmtA_old"] = w.cmt(value_old, d["sn_old"], r_old); d["sn"] = w.prf(sk, d["r"]); d["cmtS"] = w.cmts(d["value_s"], d["pk_recv"], d["r_s"], d["sn_old"]); d["cmtA"] = w.cmt(d["value"], d["sn"], d["r"])
        p = z.GenSendProof(*w.send_args(d)); a = [d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]; assert z.VerifySendProof(p, *a); return ("send", p, a, 0)
    dm = w.mint_instance(1); M = mint_of(dm); S = send_on(dm["sk"], dm["value"], dm["r"], 1); assert S[2][0] == M[2][2]                      # X: a mint, then a send made on the mint's cmtA
    Sstale = send_on(dm["sk"], dm["value_old"], dm["r_old"], 2); assert Sstale[2][0] == M[2][0]                                                  # ... and one made on X's value BEFORE the block
    MY = mint_of(w.mint_instance(2)); MW = mint_of(w.mint_instance(3))
    dd = w.deposit_instance(1, 8); tree = e.Tree(DEPTH); t = tree.h; assert z.TreeAppend(t, dd["leaves"]) == 8; leaves = [w.rev(x) for x in dd["leaves"]]; anchors = [8]
    p, rt = z.GenDepositProofTreeAt(*w.deposit_args(dd), dd["sk"], t, 8); D = ("deposit", p, [rt, dd["pk_recv"], dd["cmtB_old"], dd["sn_old"], dd["cmtB"], dd["sn_s"]], 0); assert z.VerifyDepositProofDepth(DEPTH, p, *D[2])
    Mbad = ("mint", M[1][:100] + ("0" if M[1][100] != "0" else "1") + M[1][101:], M[2], M[3]); assert not z.VerifyMintProof(Mbad[1], *Mbad[2], Mbad[3])
    start = {X: M[2][0], Y: MY[2][0], Z: D[2][2]}
    def zeroed(items): return e.records_from_items([with_old(it, ZERO) for it in items])                                                          # the records as they arrive: no old
    def fresh():
        a = e.AccountTable(); assert z.AcctsSet(a, list(start), list(start.values())) == 0; s = e.SpentSet(exempt); assert s.spend([key(bytes(range(32)))]) == ([0], 1); return a, s
    def states(a, s): return (a.read_log(), z.AcctsGet(a, [X, Y, Z, W]), s.read_log(), tree.size(), tree.root())
    def run(items, froms, a, s, commit):
        want = oracle(z, items, froms, start, leaves, anchors, s.read_log(), exempt); got = z.VerifyBlockAccounts(None, zeroed(items), froms, a, t, anchors, s.h, commit); f = want[0]; n = len(items)
        assert got[0] == f and got[1] == [i < f for i in range(n)] and got[2] == [want[2][i] if i < f else -1 for i in range(n)], (got[:3], want[0], want[2])
        for i in range(min(f + 1, n)): assert got[3][i].tobytes() == e.records_from_items([want[1][i]])[0].tobytes(), i                           # the statements that were verified come back
        return want, got
    items = [M, S, MY, D]; froms = [X, X, Y, Z]; n = 4
    # 2. commit = 0: decided, and all three states unchanged bit for bit
    a, s = fresh(); before = states(a, s); want, got = run(items, froms, a, s, False); assert want[0] == n and got[4:] == (3, 1, 8) and states(a, s) == before
    # the pool's road: an unchained fill, then verifyBlockTree(commit = 0) — X's send is not valid against the current state, everything else is
    rc, flat = z.AcctsFillRecords(a, froms, zeroed(items), False); assert rc == 0 and bytes(flat["args"][1][0]) == start[X] and z.VerifyBlockTree(None, flat, t, anchors, s.h, False)[:2] == (3, [True, False, True, True])
    rc, chained = z.AcctsFillRecords(a, froms, zeroed(items), True); assert rc == 0 and chained.tobytes() == got[3].tobytes() and states(a, s) == before
    # 3. the mint's proof mutated: f = 0, X's send after it is not decided, nothing is committed
    want, got = run([Mbad, S, MY, D], froms, a, s, True); assert want[0] == 0 and got[4:] == (3, 1, 8) and states(a, s) == before
    # 4. X's second transaction made against the pre-state value: rejected at its index, the verdicts before it are 1; set and tree are taken back
    want, got = run([M, MY, Sstale, D], [X, Y, X, Z], a, s, True); assert want[0] == 2 and got[1] == [True, True, False, False] and got[4:] == (3, 1, 8) and states(a, s) == before
    assert bytes(got[3]["args"][2][0]) == M[2][2] != Sstale[2][0]
    # 5. an absent sender: its fill is the zero hash, no proof verifies under it
    want, got = run([MY, MW, D], [Y, W, Z], a, s, True); assert want[0] == 1 and bytes(got[3]["args"][1][0]) == ZERO and states(a, s) == before
    # 1. all valid, commit = 1: every sender at its last new, set and tree as verifyBlockTree leaves them
    ref_s = e.SpentSet(exempt); assert ref_s.spend([key(bytes(range(32)))]) == ([0], 1); ref_t = e.Tree(DEPTH); assert z.TreeAppend(ref_t.h, dd["leaves"]) == 8
    ref = z.VerifyBlockTree(None, e.records_from_items(items), ref_t.h, anchors, ref_s.h, True); assert ref[:2] == (n, [True] * n)
    want, got = run(items, froms, a, s, True); assert want[0] == n and got[4:] == (3 + n, ref[3], ref[4]) and got[2] == ref[2]
    assert z.AcctsGet(a, [X, Y, Z, W]) == [S[2][3], MY[2][2], D[2][4], ZERO] == [want[3].get(k, ZERO) for k in (X, Y, Z, W)] and z.AcctsGet(a, [X, Y, Z], 3) == list(start.values())
    assert [(x, v) for x, v, _ in a.read_log()] == list(start.items()) + [(X, M[2][2]), (X, S[2][3]), (Y, MY[2][2]), (Z, D[2][4])] and [p for _, _, p in a.read_log()] == [0, 0, 0, 1, 4, 2, 3]
    assert s.read_log() == ref_s.read_log() == want[4] and tree.size() == ref_t.size() == 9 and tree.root() == ref_t.root() == PrefixRoots(want[5], DEPTH).root(9)
    # the same block again: X's mint no longer proves X's value, and nothing moves
    after = states(a, s); got = z.VerifyBlockAccounts(None, zeroed(items), froms, a, t, anchors, s.h, True); assert got[:3] == (0, [False] * n, [-1] * n) and got[4:] == (7, len(want[4]), 9) and states(a, s) == after
    # a reorganisation: all three back to the sizes before the block, and the block is valid again
    assert z.AcctsRewind(a, 3) == 0 and z.SnSetRewind(s.h, 1) == 1 and z.TreeRewind(t, 8) == 8 and states(a, s) == before
    assert z.VerifyBlockAccounts(None, zeroed(items), froms, a, t, anchors, s.h, True)[0] == n and states(a, s) == after
    # bad arguments: -1, nothing written to the states
    assert z.VerifyBlockAccounts(None, zeroed(items), froms, None, t, anchors, s.h, True)[:3] == (-1, [False] * n, [-1] * n)
    got = z.VerifyBlockAccounts(None, zeroed(items), froms, a, t, [99], s.h, True); assert got[:3] == (-1, [False] * n, [-1] * n) and states(a, s) == after
    assert got[3].tobytes() == zeroed(items).tobytes() and got[4:] == (None, None, None)                                                          # a bad anchor is found before the fill: recs is not written
    L = e.lib(); ok = (__import__("ctypes").c_ubyte * n)(); recs = zeroed(items)
    assert L.verifyBlockAccounts(None, recs.ctypes.data_as(__import__("ctypes").c_void_p), None, n, __import__("ctypes").c_void_p(a.h), None, None, 0, None, 1, ok, None, None, None, None) == -1 and states(a, s) == after
    a.close(); s.close(); ref_s.close(); ref_t.close(); tree.close()

LEGS = {"block": leg_block}

def run_leg(name, tmp_path, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path)], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, ZK_PRFKEY_DIR=str(tmp_path)))
    assert r.returncode == 0 and ("LEG OK " + name) in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout

def test_verify_block_accounts(tmp_path): run_leg("block", tmp_path)

if __name__ == "__main__":
    LEGS[sys.argv[1]](sys.argv[2]); print("LEG OK " + sys.argv[1])
