"""The three GPU paths of BatchVerifier::verify (gpu_verify.hip) against the same verdicts:
  * up to 64 proofs: the small contexts (k_verify_acc_quads + k_verify_sched29, kernel K9);
  * 65 to ZK_VERIFY_WAVE_MAX (default 8,192): the same kernels, the large-batch workgroup branch;
  * more: the LANE branch (pairing.cuh: k_verify_acc + k_verify_batch, one lane per proof, its own bytecode and its own handling of an accumulator at infinity).
ZK_VERIFY_WAVE_MAX is read once per process: the lane legs run in a fresh child process with ZK_VERIFY_WAVE_MAX=0, every call of at least 65 records (fewer go to the
small contexts whatever the switch says), and the path counters (zkgpu_verify_path_counters) show that the branch meant really ran."""
import json, os, subprocess, sys, time
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import workload as w
import verify_mutations as vm
import verify_crafted as vc
from conftest import record_leg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
have_ref = os.path.exists(HARNESS)

def padded(items, n_min=65):
    """items cycled to at least n_min, never a multiple of 64 (the last workgroup of the lane kernel stays partial)"""
    n = max(n_min, len(items)); n += n % 64 == 0; return [items[i % len(items)] for i in range(n)]

CHILD = """
import json, sys
sys.path.insert(0, %r)
from blockmaze_amd import engine as e
out = []
for call in json.load(open(sys.argv[1])):
    before = e.verify_path_counters(call["vk"]); got = e.verify_batch(call["vk"], call["proofs"], call["inputs"]); after = e.verify_path_counters(call["vk"])
    out.append({"got": [int(v) for v in got], "before": before, "after": after})
print("RESULT " + json.dumps(out))
""" % ROOT

def in_child(tmp_path, calls, wave_max=0, timeout=300):
    """calls: [(vk path, proofs, inputs)], each one zkgpu_verify_batch call in ONE fresh process with ZK_VERIFY_WAVE_MAX=wave_max -> [(verdicts, counters before,
    counters after)]"""
    job = str(tmp_path / ("job_%d.json" % len(os.listdir(str(tmp_path)))))
    json.dump([{"vk": vk, "proofs": list(p), "inputs": [list(x) for x in ins]} for vk, p, ins in calls], open(job, "w"))
    r = subprocess.run([sys.executable, "-c", CHILD, job], env=dict(os.environ, ZK_VERIFY_WAVE_MAX=str(wave_max)), capture_output=True, text=True, timeout=timeout)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]; assert r.returncode == 0 and line, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    res = json.loads(line[0][7:]); assert len(res) == len(calls); return [([bool(v) for v in c["got"]], c["before"], c["after"]) for c in res]

def took_lane(before, after, n=1):
    """the call ran the lane kernel n times and the workgroup branch not at all (counters: small calls, small launches, workgroup launches, lane launches)"""
    return after[3] - before[3] == n and after[2] == before[2] and after[:2] == before[:2]
def took_wave(before, after):
    return after[2] - before[2] == 1 and after[3] == before[3] and after[:2] == before[:2]

# ---- (a) the mutation corpora ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["groth16_small", "groth16_step"])
def test_lane_verifier_verdicts_are_the_reference_s_on_mutated_proofs(golden_dir, name, tmp_path):
    """the ~290 committed mutations of the reference prover's proof (tests/golden/verify_mutations_*.txt, with the verdicts of the reference's verifier), one lane
    launch per input-count group: every verdict is the reference's (an encoding on which the assert-enabled reference aborts is rejected)"""
    t0 = time.time(); vk = os.path.join(golden_dir, name, "vk.txt"); cases = vm.read_golden(os.path.join(golden_dir, "verify_mutations_%s.txt" % name)); assert len(cases) >= 200
    ni = json.load(open(os.path.join(golden_dir, name, "meta.json")))["n_inputs"]; groups = [[c for c in cases if len(c[2]) == k] for k in sorted(set(len(c[2]) for c in cases))]
    res = in_child(tmp_path, [(vk, [c[1] for c in padded(g)], [c[2] for c in padded(g)]) for g in groups]); n_acc = 0; lanes = 0
    for g, (got, before, after) in zip(groups, res):
        assert len(got) == len(padded(g)) >= 65
        for c, v in zip(padded(g), got): assert vm.agrees(v, c[3]), (c[0], c[3])
        n_acc += sum(got[:len(g)])
        if len(g[0][2]) == ni: assert took_lane(before, after), (before, after); lanes += 1
        else: assert after == before and not any(got)                                # (a wrong input count is rejected before the device)
    assert lanes == 1 and n_acc >= 100
    record_leg("lane verifier: mutations of " + name, time.time() - t0)

# ---- (b) random curve points, (c) the mixed batch -----------------------------------------------------------------------------------------------------------------
def test_lane_verifier_random_curve_points_match_host(golden_dir, tmp_path):
    """the 160 + 24 records of test_gpu_verifier_random_curve_points_match_host (random multiples of the generators under random or genuine inputs, valid proofs under
    random inputs, 24 valid proofs) in one lane launch: the host verifier's verdicts, exactly 24 accepted"""
    t0 = time.time(); d = os.path.join(golden_dir, "groth16_small"); meta = json.load(open(os.path.join(d, "meta.json"))); z = o.load_witness(os.path.join(d, "wit.bin")); vk = os.path.join(d, "vk.txt")
    inputs = o.from_arr(z[:meta["n_inputs"]]); p = e.Prover(os.path.join(d, "pk.txt")); good = [p.prove(z) for _ in range(24)]; p.close()
    proofs, ins = vc.random_curve_batch(good, inputs); assert len(proofs) == 184 and len(proofs) % 64
    exp = [e.verify(vk, pr, x) for pr, x in zip(proofs, ins)]; assert sum(exp) == 24
    [(got, before, after)] = in_child(tmp_path, [(vk, proofs, ins)]); assert took_lane(before, after), (before, after)
    assert got == exp and sum(got) == 24
    record_leg("lane verifier: random curve points", time.time() - t0)

@pytest.mark.parametrize("name", ["groth16_small", "groth16_step"])
def test_lane_verifier_mixed_batch_matches_host_and_oracle(golden_dir, name, tmp_path):
    """the batch of test_batched_gpu_verifier_matches_host_verifier (valid proofs, a flipped digit in every coordinate, wrong inputs, all-zero inputs, the all-zero
    record, text that is not hex, a spliced proof) cycled past 64 records, in one lane launch: the host verifier's verdicts and the oracle's"""
    t0 = time.time(); d = os.path.join(golden_dir, name); meta = json.load(open(os.path.join(d, "meta.json"))); z = o.load_witness(os.path.join(d, "wit.bin")); vk = os.path.join(d, "vk.txt")
    inputs = o.from_arr(z[:meta["n_inputs"]]); p = e.Prover(os.path.join(d, "pk.txt")); good = [meta["proof"]] + [p.prove(z) for _ in range(3)]; p.close()
    proofs, ins = vc.mixed_batch(good, inputs); recs = padded(list(zip(proofs, ins))); exp = [e.verify(vk, pr, x) for pr, x in recs]
    assert exp[:len(good)] == [True] * len(good) and not any(exp[len(good):len(proofs)]) and len(recs) >= 65
    [(got, before, after)] = in_child(tmp_path, [(vk, [r[0] for r in recs], [r[1] for r in recs])]); assert took_lane(before, after), (before, after)
    assert got == exp
    ovk = o.parse_vk(vk)
    for (pr, x), g_ in zip(recs[:len(proofs)], got):
        if all(c in "0123456789abcdef" for c in pr) and pr != "0" * 512: assert o.verify(ovk, x, o.proof_words_from_hex(pr)) == g_
    record_leg("lane verifier: mixed batch " + name, time.time() - t0)

# ---- (d) crafted keys: the accumulator's edge cases on both kernels ----------------------------------------------------------------------------------------------
# the crafted cases whose accumulation meets a degenerate sum in k_verify_acc_quads (an incomplete addition: ZZ = 0): K9 hands them back (verdict 2), the host decides
HANDED_BACK = ["ic=[O] / valid", "ic=[P,-P] / valid x=1", "ic=[P,P] / valid x=1", "ic=[P,P], x=r-1 / valid x=r-1", "ic=[O,P,P] / valid x=(1,1)", "ic=[O,P,-P] / valid x=(1,1)",
               "ic=[Q,P,256P], doubling of windows / valid x=(256,1)", "5 inputs, acc = O / valid solved", "16 inputs, acc = O / valid solved"]

def test_crafted_keys_on_the_small_contexts_and_the_lane_kernel(golden_dir, tmp_path):
    """tests/verify_crafted.py (acc at infinity from IC[0], from P + (-P), from full-width inputs; doublings at IC[0] and inside the sum; IC points at infinity; zero
    inputs; 1, 5 and 16 inputs) on K9 — one batch per key and one call per record — and on the lane kernel (a fresh process, one padded launch per key): the host
    verifier's verdict every time, which tests/test_verifier_crafted_keys_cpu.py pins to libsnark (its stored answers are checked here too).  Where K9's incomplete
    additions meet a degenerate sum the record must come back to the host (verdict 2) instead of reaching a verdict from a wrong accumulator"""
    t0 = time.time(); stored = json.load(open(os.path.join(golden_dir, "verify_crafted_keys.json"))); keys = vc.write_keys(tmp_path); assert vc.cases_sha256(keys) == stored["cases_sha256"]
    exp = {}
    for label, path, h, x in vc.labelled(keys): exp[label] = int(e.verify(path, h, x)); assert exp[label] == stored["verdicts"][label], label
    for path, label, cs in keys:
        before = e.verify_path_counters(path)
        got = e.verify_batch(path, [c[1] for c in cs], [c[2] for c in cs]); assert [int(v) for v in got] == [exp[label + " / " + c[0]] for c in cs], (label, got)
        for cl, h, x in cs: assert int(e.verify_batch(path, [h], [x])[0]) == exp[label + " / " + cl], (label, cl)
        after = e.verify_path_counters(path); assert after[0] - before[0] == 1 + len(cs) and after[2:] == before[2:], (label, before, after)
    where = {label + " / " + cl: (path, h, x) for path, label, cs in keys for cl, h, x in cs}
    for k in HANDED_BACK:
        path, h, x = where[k]; assert e.verify_trace(path, h, x, 64)[2] == 2 and exp[k] == 1, k
    path, h, x = where["ic=[P] / valid"]; assert e.verify_trace(path, h, x, 64)[2] == 1
    t1 = time.time(); calls = [(path, [c[1] for c in padded(cs)], [c[2] for c in padded(cs)]) for path, label, cs in keys]; res = in_child(tmp_path, calls)
    for (path, label, cs), (got, before, after) in zip(keys, res):
        assert took_lane(before, after), (label, before, after)
        assert [int(v) for v in got] == [exp[label + " / " + c[0]] for c in padded(cs)], (label, [c[0] for c, v in zip(padded(cs), got) if int(v) != exp[label + " / " + c[0]]])
    record_leg("crafted keys: K9 %.1f s, lane kernel" % (t1 - t0), time.time() - t1)

# ---- (e) the boundary at the shipped default, (f) through the cgo symbol -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys(tmp_path_factory):
    d = tmp_path_factory.mktemp("prfKey")
    for i, kind in enumerate(("send", "mint", "redeem")): e.keygen(kind, str(d / (kind + "pk.txt")), str(d / (kind + "vk.txt")), seed=0xB10C4A2E + 7 * i)
    return d

def send_records(keys, tmp_path):
    """4 valid send proofs and, for each, its 8 corrupted twins, its statement with each input + 1, the other proofs' statements, an alias and the (-A, -B) malleation;
    the all-zero record and a spliced proof -> [(label, proof hex, inputs)]"""
    p = e.Prover(str(keys / "sendpk.txt")); base = []; wp = str(tmp_path / "w.bin")
    for i in range(4):
        d = w.send_instance(70 + i); e.witness_send(*[("0x" + a.hex()) if isinstance(a, bytes) else a for a in w.send_args(d)], wp); z = o.load_witness(wp)
        base.append((p.prove(z), w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]])))
    p.close(); out = []
    for i, (pr, x) in enumerate(base):
        out.append(("valid #%d" % i, pr, x))
        for k in range(8): pos = 64 * k + 29; out.append(("#%d %s flipped" % (i, vm.ORDER[k]), pr[:pos] + ("3" if pr[pos] != "3" else "4") + pr[pos + 1:], x))
        for j in range(len(x)): bad = list(x); bad[j] = (bad[j] + 1) % o.R_MOD; out.append(("#%d input %d + 1" % (i, j), pr, bad))
        for j in range(4):
            if j != i: out.append(("#%d under the statement of #%d" % (i, j), pr, base[j][1]))
        c = vm.coords(pr); c[0] += o.Q_MOD; out.append(("#%d A.x + q" % i, vm.to_hex(c), x))
        A, B, C = vm.points(vm.coords(pr)); out.append(("#%d (-A, -B)" % i, vm.to_hex(vm.from_points(vm.g1_neg(A), vm.g2_neg(B), C)), x))
    out.append(("all zero", "0" * 512, base[0][1])); out.append(("spliced", base[0][0][:128] + base[1][0][128:], base[0][1]))
    return out

def test_wave_max_boundary_on_a_full_size_send_key(keys, tmp_path):
    """about 80 distinct send records cycled into ONE call of 8,192 (the workgroup branch, the shipped ZK_VERIFY_WAVE_MAX) and one of 8,193 (the lane kernel): the same,
    right verdict for every record — libsnark's (oracle/_ref/ref_harness verifymany) where it is there, the host verifier's otherwise; then the same boundary in a
    process with ZK_VERIFY_WAVE_MAX=100, at 100 and 101 records"""
    t0 = time.time(); vk = str(keys / "sendvk.txt"); recs = send_records(keys, tmp_path); host = [int(e.verify(vk, h, x)) for _, h, x in recs]
    exp = vm.reference_verdicts(HARNESS, vk, recs, tmp_path) if have_ref else host
    assert [vm.agrees(h_, v) for h_, v in zip(host, exp)] == [True] * len(recs) and 60 <= len(recs) <= 120 and 12 <= exp.count(1) and exp.count(0) >= 50
    for n, took in ((8192, took_wave), (8193, took_lane)):
        cyc = [recs[i % len(recs)] for i in range(n)]; before = e.verify_path_counters(vk)
        got = e.verify_batch(vk, [c[1] for c in cyc], [c[2] for c in cyc]); after = e.verify_path_counters(vk); assert took(before, after), (n, before, after)
        bad = [(i, cyc[i][0]) for i in range(n) if not vm.agrees(got[i], exp[i % len(recs)])]; assert not bad, (n, len(bad), bad[:5])
    t1 = time.time(); calls = [(vk, [recs[i % len(recs)][1] for i in range(n)], [recs[i % len(recs)][2] for i in range(n)]) for n in (100, 101)]
    (g100, b100, a100), (g101, b101, a101) = in_child(tmp_path, calls, wave_max=100)
    assert took_wave(b100, a100) and took_lane(b101, a101), (b100, a100, b101, a101)
    for n, got in ((100, g100), (101, g101)): assert all(vm.agrees(got[i], exp[i % len(recs)]) for i in range(n)), n
    record_leg("send key at 8,192 / 8,193 records%s (%.1f s), ZK_VERIFY_WAVE_MAX=100" % (" against libsnark" if have_ref else "", t1 - t0), time.time() - t1)

def test_verify_batch_symbol_takes_the_lane_kernel_and_decides_like_libsnark(keys, monkeypatch, tmp_path):
    """verifyBatch (include/zk_batch.h) with more than 8,192 send records: the ~280 seeded mutations of a gen*proof proof (tests/verify_mutations.py) cycled, other
    statements and a few mint / redeem records interleaved.  The send group takes the lane kernel (counters of the send key), and every verdict is libsnark's"""
    assert have_ref, "oracle/_ref/ref_harness is missing: run __graft_entry__.build() where /root/reference exists"
    t0 = time.time(); monkeypatch.setenv("ZK_PRFKEY_DIR", str(keys)); zk = e.Zk(); vk = str(keys / "sendvk.txt")
    sd = w.send_instance(91); proof = zk.GenSendProof(*w.send_args(sd)); args = [sd["cmtA_old"], sd["sn_old"], sd["cmtS"], sd["cmtA"]]; inputs = w.pack_public(args)
    assert zk.VerifySendProof(proof, *args)
    cases = [c for c in vm.cases(vk, proof, inputs, 0xF00D) if c[2] == inputs]; ref_v = vm.reference_verdicts(HARNESS, vk, cases, tmp_path)
    assert len(cases) >= 200 and ref_v.count(1) >= 100 and ref_v.count(0) >= 90
    others = []
    for j in range(len(args)):
        other = list(args); other[j] = bytes(x ^ (1 if i == len(args[j]) - 1 else 0) for i, x in enumerate(args[j])); others.append((other, vm.reference_verdicts(HARNESS, vk, [("other", proof, w.pack_public(other))], tmp_path)[0]))
    assert [v for _, v in others] == [0] * len(args)
    small = []
    for i in range(3):
        m = w.mint_instance(92 + i); small.append(("mint", zk.GenMintProof(*w.mint_args(m)), [m["cmtA_old"], m["sn_old"], m["cmtA"]], m["value_s"] + (1 if i == 1 else 0), i != 1))
        r = w.mint_instance(95 + i, redeem=True); small.append(("redeem", zk.GenRedeemProof(*w.mint_args(r)), [r["cmtA_old"], r["sn_old"], r["cmtA"]], r["value_s"], True))
    items, expect = [], []
    for k in range(8200):
        if k % 100 == 50: o_args, v = others[(k // 100) % len(others)]; items.append(("send", proof, o_args, 0)); expect.append(v == 1)
        else: (_, h, _), v = cases[k % len(cases)], ref_v[k % len(cases)]; items.append(("send", h, args, 0)); expect.append(v == 1)
        if k % 1500 == 7: kind, pr, a, vs, ok = small[(k // 1500) % len(small)]; items.append((kind, pr, a, vs)); expect.append(ok)
    assert sum(1 for it in items if it[0] == "send") >= 8193
    before = e.verify_path_counters(vk); rc, ok = zk.VerifyBatch(items); after = e.verify_path_counters(vk)
    assert took_lane(before, after), (before, after)
    bad = [(i, items[i][0], ok[i], expect[i]) for i in range(len(items)) if ok[i] != expect[i]]; assert not bad, (len(bad), bad[:5])
    assert rc == sum(expect)
    record_leg("verifyBatch: %d send records on the lane kernel against libsnark" % sum(1 for it in items if it[0] == "send"), time.time() - t0)
