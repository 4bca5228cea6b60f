"""Child process of tests/test_gpu_list_roots.py: one job a process, so that a device fault ends the job and not the test session.
usage: python list_roots_child.py OP JOB.npz   ->   a line "RESULT <json>" """
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from blockmaze_amd import engine as e
import workload as w

def op_roots(job):
    """kernel = host model, byte for byte and position by position, for every case of the job; and the kernel launches each call took"""
    out = []
    for k in range(int(job["n_cases"])):
        leaves = job["leaves_%d" % k]; lists = job["lists_%d" % k]; depth = int(job["depth_%d" % k]); hash_order = bool(job["hash_%d" % k])
        host = e.list_roots_host(depth, leaves, lists, hash_order); l0 = e.list_roots_launches(); dev = e.list_roots(depth, leaves, lists, hash_order); l1 = e.list_roots_launches()
        bad = np.nonzero((dev != host).any(axis=1))[0]
        out.append({"case": k, "n": int(len(lists)), "differ": int(len(bad)), "first": [int(i) for i in bad[:5]], "launches": l1 - l0, "distinct": int(len(set(bytes(r) for r in host)))})
    return out

def op_genroots(job):
    """Zk.GenRoots at depth 8 against Zk.GenRT, list by list"""
    z = e.Zk(); cmts = job["cmts"]; lists = [(int(f), int(c)) for f, c in job["lists"]]
    return {"roots": [r.hex() for r in z.GenRoots(cmts, lists)], "rt": [z.GenRT([bytes(x) for x in cmts[f:f + c]]).hex() for f, c in lists]}

def op_setup(job):
    """deposit, send and mint keys made with seeds under ZK_PRFKEY_DIR; three valid deposit proofs over 16, 1 and 256 leaves and one valid send proof"""
    d = os.environ["ZK_PRFKEY_DIR"]
    for i, kind in enumerate(("send", "mint", "redeem", "deposit")):
        if kind != "redeem": e.keygen(kind, os.path.join(d, kind + "pk.txt"), os.path.join(d, kind + "vk.txt"), seed=0xB10C4A2E + 7 * i)
    z = e.Zk(); deposits = []
    for i, n in enumerate((16, 1, 256)):
        x = w.deposit_instance(40 + i, n); pr = z.GenDepositProof(*w.deposit_args(x), x["leaves"], x["rt"], x["sk"]); args = [x["rt"], x["pk_recv"], x["cmtB_old"], x["sn_old"], x["cmtB"], x["sn_s"]]
        assert z.VerifyDepositProof(pr, *args), n
        deposits.append({"proof": pr, "args": [a.hex() for a in args], "leaves": [l.hex() for l in x["leaves"]]})
    sd = w.send_instance(91); pr = z.GenSendProof(*w.send_args(sd)); args = [sd["cmtA_old"], sd["sn_old"], sd["cmtS"], sd["cmtA"]]; assert z.VerifySendProof(pr, *args)
    return {"deposits": deposits, "send": {"proof": pr, "args": [a.hex() for a in args]}}

def op_block(job):
    """verifyBlockRecords, verifyBlockRecordsRoots and verifyBlockRecords again on the same records, each with the movement of the block-equation counters"""
    z = e.Zk(); recs = job["recs"]; cmts = job["cmts"]; lists = job["lists"]; list_of = job["list_of"]; out = {}
    def counted(fn):
        c0 = e.verify_rlc_counters(); rc, ok = fn(); c1 = e.verify_rlc_counters(); return {"rc": rc, "ok": [int(x) for x in ok], "moved": [c1[k] - c0[k] for k in range(3)]}
    out["before"] = counted(lambda: z.VerifyBlockRecords(recs))
    out["roots"] = counted(lambda: z.VerifyBlockRecordsRoots(recs, cmts, lists, list_of))
    out["after"] = counted(lambda: z.VerifyBlockRecords(recs))
    return out

if __name__ == "__main__":
    job = np.load(sys.argv[2], allow_pickle=False)
    print("RESULT " + json.dumps({"roots": op_roots, "genroots": op_genroots, "setup": op_setup, "block": op_block}[sys.argv[1]](job)))
