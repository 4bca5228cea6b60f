"""Child process of tests/test_gpu_block_records.py: one job a process, so that a device fault ends the job and not the test session.
usage: python block_records_child.py OP JOB.npz   ->   a line "RESULT <json>" """
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from blockmaze_amd import engine as e
import block_records as br

def op_ingest(job):
    """kernel = model, byte for byte: every array of the job through k_ingest_records and through records_to_host"""
    out = []
    for name in sorted(job.files):
        recs = job[name]; dev = e.ingest_records(recs, device=True); host = e.ingest_records(recs, device=False)
        diff = [int((d.reshape(len(recs), -1) != h.reshape(len(recs), -1)).any(axis=1).sum()) for d, h in zip(dev, host)]
        out.append({"name": name, "n": int(len(recs)), "differ": diff, "parsed": int(host[2].sum()), "first": [int(i) for i in np.nonzero((dev[0].reshape(len(recs), -1) != host[0].reshape(len(recs), -1)).any(axis=1))[0][:5]]})
    return out

def op_equation(job):
    """the device's sums and equation from records against the host loop's sums and the host model of the equation"""
    vk = str(job["vk"]); out = []
    for k in range(int(job["n_sets"])):
        recs = job["recs_%d" % k]; flags = job["flags_%d" % k]; items, inputs, parsed = e.ingest_records(recs, device=False)
        proofs = [bytes(p).decode("latin-1") for p in recs["proof"]]; ins = br.ints(inputs); model = bool(job["model_%d" % k])
        for label, ws in (("random", [int.from_bytes(bytes(x), "little") for x in job["w_%d" % k]]), ("ones", [1] * len(recs)), ("max", [(1 << 128) - 1] * len(recs))):
            dev_holds, dev_gt, dev_sums = e.records_rlc_equation(vk, recs, ws); host_sums = e.rlc_sums_host(inputs, ws, flags)
            host_holds, host_gt = e.verify_rlc_equation(vk, proofs, ins, ws) if model else (bool(job["holds_%d" % k]), dev_gt)   # (a large set: the sums and the known outcome)
            out.append({"set": k, "weights": label, "dev": dev_holds, "host": host_holds, "same_gt": dev_gt == host_gt, "same_sums": dev_sums == host_sums, "nonzero": all(s > 0 for s in host_sums)})
    return out

def op_no_device(job):
    """verifyBlockRecords in a process that sees no device: the host decides"""
    assert e.device_count() == 0
    rc, ok = e.Zk().VerifyBlockRecords(job["recs"]); return {"rc": rc, "ok": ok, "counters": e.verify_rlc_counters()}

if __name__ == "__main__":
    job = np.load(sys.argv[2], allow_pickle=False)
    print("RESULT " + json.dumps({"ingest": op_ingest, "equation": op_equation, "no_device": op_no_device}[sys.argv[1]](job)))
