"""The randomized block check on the device (gpu_verify_block.hip) against verifyBatch's verdicts and the host model: zkgpu_verify_batch_rlc in fresh child
processes, and the drop-in verifyBlock (include/zk_block.h) on send, mint and redeem keys made with seeds."""
import json, os, random, subprocess, sys, time
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import workload as w
import verify_mutations as vm
from conftest import record_leg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
N0 = 8192   # RLC_MIN_RECORDS (capi_zk.cpp)

CHILD = """
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from blockmaze_amd import engine as e
out = []
for c in json.load(open(sys.argv[1])):
    if c["op"] == "rlc":
        before = e.verify_rlc_counters(); pp = e.verify_path_counters(c["vk"]); got, by = e.verify_batch_rlc(c["vk"], c["proofs"], c["inputs"])
        after = e.verify_rlc_counters(); pp_after = e.verify_path_counters(c["vk"])
        out.append({"got": got, "by": by, "ref": e.verify_batch(c["vk"], c["proofs"], c["inputs"]), "before": before, "after": after, "pp": pp, "pp_after": pp_after})
    else:
        dh, gh = e.verify_rlc_equation(c["vk"], c["proofs"], c["inputs"], c["w"]); dd, gd = e.verify_rlc_equation(c["vk"], c["proofs"], c["inputs"], c["w"], device=True)
        out.append({"host": dh, "dev": dd, "same_gt": gh == gd})
print("RESULT " + json.dumps(out))
""" % (ROOT, os.path.join(ROOT, "tests"))

def in_child(tmp_path, calls, timeout=900):
    job = str(tmp_path / ("job_%d.json" % len(os.listdir(str(tmp_path))))); json.dump(calls, open(job, "w"))
    r = subprocess.run([sys.executable, "-c", CHILD, job], capture_output=True, text=True, timeout=timeout)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]; assert r.returncode == 0 and line, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(line[0][7:])

def corpus(golden_dir, name):
    """(vk, the key's input count, every committed mutation of the corpus)"""
    ni = json.load(open(os.path.join(golden_dir, name, "meta.json")))["n_inputs"]
    return os.path.join(golden_dir, name, "vk.txt"), ni, vm.read_golden(os.path.join(golden_dir, "verify_mutations_%s.txt" % name))

def moved(r): return [r["after"][k] - r["before"][k] for k in range(3)]   # (equations that held, that failed, calls decided proof by proof)

@pytest.mark.parametrize("name", ["groth16_small", "groth16_step"])
def test_block_verdicts_equal_verify_batch_on_the_mutation_corpora(golden_dir, name, tmp_path):
    """every committed mutation, grouped by input count as test_gpu_verify_paths.py groups them and cycled into calls of 1, 65, 300 and 8,193 records: every verdict
    is the reference's and zkgpu_verify_batch's (a group with the wrong input count is rejected before any device work).  The accepted records alone in 8,193: one
    equation decides, the per-proof kernels do not run.  The same with one valid proof under a wrong statement among them: the equation fails, the call falls back
    to the per-proof path and that record is the only one rejected"""
    vk, ni, cases = corpus(golden_dir, name); groups = [[c for c in cases if len(c[2]) == k] for k in sorted(set(len(c[2]) for c in cases))]; assert len(groups) >= 2
    calls, kinds = [], []
    for g in groups:
        for n in (1, 65, 300, 8193): calls.append([g[i % len(g)] for i in range(n)]); kinds.append(("cycled", len(g[0][2]), n))
    good = [c for c in cases if c[3] == 1 and len(c[2]) == ni]; assert len(good) >= 20
    calls.append([good[i % len(good)] for i in range(8193)]); kinds.append(("valid", ni, 8193))
    wrong = list(good[0][2]); wrong[0] = (wrong[0] + 1) % o.R_MOD; one_bad = [good[i % len(good)] for i in range(8193)]; one_bad[4321] = ("wrong statement", good[0][1], wrong, 0)
    calls.append(one_bad); kinds.append(("one bad", ni, 8193))
    res = in_child(tmp_path, [{"op": "rlc", "vk": vk, "proofs": [c[1] for c in cl], "inputs": [c[2] for c in cl]} for cl in calls])
    for cl, kd, r in zip(calls, kinds, res):
        assert r["got"] == r["ref"], kd
        assert all(vm.agrees(g_, c[3]) for g_, c in zip(r["got"], cl)), kd
        if kd[1] != ni: assert not any(r["got"]) and not r["by"] and moved(r) == [0, 0, 1] and r["pp_after"] == r["pp"], kd
        elif kd[0] == "cycled": assert r["by"] is False and moved(r) == ([0, 1, 1] if kd[2] >= N0 else [0, 0, 1]), (kd, moved(r))   # (the corpus holds bad records)
    r = res[-2]; assert r["by"] and all(r["got"]) and moved(r) == [1, 0, 0] and r["pp_after"] == r["pp"], (moved(r), r["pp"], r["pp_after"])
    r = res[-1]; assert not r["by"] and moved(r) == [0, 1, 1] and r["got"].count(False) == 1 and not r["got"][4321]

@pytest.fixture(scope="module")
def keys(tmp_path_factory):
    d = tmp_path_factory.mktemp("prfKey")
    for i, kind in enumerate(("send", "mint", "redeem")): e.keygen(kind, str(d / (kind + "pk.txt")), str(d / (kind + "vk.txt")), seed=0xB10C4A2E + 7 * i)
    return d

def shifted(h, P):
    A, B, C = vm.points(vm.coords(h)); return vm.to_hex(vm.from_points(A, B, o.g1_op("add", C, P)))

@pytest.mark.parametrize("name", ["groth16_small", "groth16_step", "send"])
def test_device_equation_equals_host_model(golden_dir, name, keys, tmp_path):
    """the same explicit weights on the device path and on the host model: the same outcome and the same GT value, for passing and failing calls, on both golden
    keys and on a send key (valid proofs, wrong statements, the +-D pair)"""
    rng = random.Random(3)
    if name == "send":
        vk = str(keys / "sendvk.txt"); p = e.Prover(str(keys / "sendpk.txt")); wp = str(tmp_path / "w.bin"); good = []
        for i in range(3):
            d = w.send_instance(60 + i); e.witness_send(*[("0x" + a.hex()) if isinstance(a, bytes) else a for a in w.send_args(d)], wp)
            good.append(("valid", p.prove(o.load_witness(wp)), w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]), 1))
        p.close(); D = o.g1_op("mul", o.g1_gen(), k=rng.randrange(1, o.R_MOD))
        bad = [("+D", shifted(good[0][1], D), good[0][2], 0), ("-D", shifted(good[1][1], vm.g1_neg(D)), good[1][2], 0), ("statement", good[2][1], good[0][2], 0)]
        sets = [[good[i % 3] for i in range(20)], [good[i % 3] for i in range(10)] + bad, [good[0], good[1]] + bad[:2]]
    else:
        vk, ni, cases = corpus(golden_dir, name); cases = [c for c in cases if len(c[2]) == ni]; good = [c for c in cases if c[3] == 1]; bad = [c for c in cases if c[3] != 1]
        sets = [rng.sample(good, 40), rng.sample(good, 30) + rng.sample(bad, 5), rng.sample(cases, 70)]
    res = in_child(tmp_path, [{"op": "eq", "vk": vk, "proofs": [c[1] for c in s], "inputs": [c[2] for c in s], "w": [rng.randrange(1, 1 << 128) for _ in s]} for s in sets])
    assert res[0]["host"] and not res[1]["host"]
    for r in res: assert r["host"] == r["dev"] and r["same_gt"], r

def test_verify_block_symbol_decides_like_verify_batch(keys, monkeypatch, tmp_path):
    """verifyBlock (include/zk_block.h) on blocks of send, mint and redeem records, against verifyBatch on the same items (and libsnark's verdicts where the reference
    harness is there):
      * a mixed block of more than 8,192 records — the ~280 seeded mutations of a send proof (tests/verify_mutations.py) cycled, other statements, the +-D pair and
        mint / redeem records interleaved: the send group's equation fails, every group is decided proof by proof;
      * the same kinds in a block below the threshold (700 records): the per-proof path at once;
      * only valid records, at least 8,192 of each kind: ONE equation decides the whole block, the per-proof kernels do not run;
      * 8,192 valid send records and the +-D pair: the pair alone is rejected."""
    t0 = time.time(); monkeypatch.setenv("ZK_PRFKEY_DIR", str(keys)); zk = e.Zk(); vk = str(keys / "sendvk.txt")
    sends = []
    for i in range(2):
        sd = w.send_instance(91 + i); pr = zk.GenSendProof(*w.send_args(sd)); args = [sd["cmtA_old"], sd["sn_old"], sd["cmtS"], sd["cmtA"]]; assert zk.VerifySendProof(pr, *args)
        sends.append((pr, args))
    (proof, args), (proof2, args2) = sends; inputs = w.pack_public(args)
    cases = [c for c in vm.cases(vk, proof, inputs, 0xF00D) if c[2] == inputs]; assert len(cases) >= 200
    D = o.g1_op("mul", o.g1_gen(), k=random.Random(5).randrange(1, o.R_MOD))
    pair = [("send", shifted(proof, D), args, 0), ("send", shifted(proof2, vm.g1_neg(D)), args2, 0)]
    small, valid_small = [], []
    for i in range(3):
        m = w.mint_instance(92 + i); pr = zk.GenMintProof(*w.mint_args(m)); a = [m["cmtA_old"], m["sn_old"], m["cmtA"]]
        small.append(("mint", pr, a, m["value_s"] + (1 if i == 1 else 0))); valid_small.append(("mint", pr, a, m["value_s"]))
        r = w.mint_instance(95 + i, redeem=True); pr = zk.GenRedeemProof(*w.mint_args(r)); a = [r["cmtA_old"], r["sn_old"], r["cmtA"]]
        small.append(("redeem", pr, a, r["value_s"])); valid_small.append(("redeem", pr, a, r["value_s"]))
    def mixed(n_send):
        items = []
        for k in range(n_send):
            if k % 100 == 50: o_args = list(args); o_args[k % 4] = bytes(x ^ (1 if j == len(args[k % 4]) - 1 else 0) for j, x in enumerate(args[k % 4])); items.append(("send", proof, o_args, 0))
            else: items.append(("send", cases[k % len(cases)][1], args, 0))
            if k % 23 == 7: items.append(small[(k // 23) % len(small)])
            if k == n_send // 2: items.extend(pair)
        return items
    def check(items, label):
        c0 = e.verify_rlc_counters(); p0 = e.verify_path_counters(vk); rc, ok = zk.VerifyBlock(items); c1 = e.verify_rlc_counters(); p1 = e.verify_path_counters(vk)
        rb, okb = zk.VerifyBatch(items); bad = [(i, items[i][0], ok[i], okb[i]) for i in range(len(items)) if ok[i] != okb[i]]
        assert not bad and rc == rb == sum(okb), (label, len(bad), bad[:5], rc, rb)
        return ok, [c1[k] - c0[k] for k in range(3)], p1 != p0
    big = mixed(8200); assert sum(1 for it in big if it[0] == "send") >= N0 and len(big) >= 8500
    ok, moved_, ran = check(big, "mixed block"); assert moved_ == [0, 1, 1] and ran
    ipair = [i for i, it in enumerate(big) if it in pair]; assert len(ipair) == 2 and not any(ok[i] for i in ipair)
    if os.path.exists(HARNESS):   # the send records' verdicts are libsnark's
        sc = [(str(i), it[1], w.pack_public(it[2])) for i, it in enumerate(big) if it[0] == "send"]; uniq = {}
        for c in sc: uniq.setdefault((c[1], tuple(c[2])), c)
        ref = dict(zip(uniq.keys(), vm.reference_verdicts(HARNESS, vk, list(uniq.values()), tmp_path)))
        assert all(vm.agrees(ok[int(c[0])], ref[(c[1], tuple(c[2]))]) for c in sc)
    ok, moved_, ran = check(mixed(640), "below the threshold"); assert moved_ == [0, 0, 1]
    valid = [("send",) + sends[k % 2] + (0,) for k in range(N0)] + [valid_small[k % len(valid_small)] for k in range(2 * N0)]
    random.Random(9).shuffle(valid)
    ok, moved_, ran = check(valid, "valid records of three kinds"); assert all(ok) and moved_ == [1, 0, 0] and not ran
    with_pair = [("send",) + sends[k % 2] + (0,) for k in range(N0)]; with_pair[100:100] = pair
    ok, moved_, ran = check(with_pair, "the +-D pair"); assert moved_ == [0, 1, 1] and ok == [not (100 <= i < 102) for i in range(len(with_pair))]
    record_leg("verifyBlock: %d-record mixed block, %d valid records of three kinds" % (len(big), len(valid)), time.time() - t0)
