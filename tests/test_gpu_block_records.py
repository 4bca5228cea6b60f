"""Blocks as records (include/zk_records.h) on the device: k_ingest_records against the host converter byte for byte, the device's integer sums and equation
against the host's, and verifyBlockRecords against verifyBlock and verifyBatch on send, mint, redeem and deposit keys made with seeds.  Device work that the
drop-in symbols do not need runs in fresh child processes (tests/block_records_child.py), one job each, under a timeout; nothing is retried."""
import json, os, random, subprocess, sys, threading, time
import numpy as np
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import workload as w
import verify_mutations as vm
import block_records as br
from conftest import record_leg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
CHILD = os.path.join(ROOT, "tests", "block_records_child.py")
N0 = 8192   # RLC_MIN_RECORDS (capi_zk.cpp)

def in_child(tmp_path, op, arrays, timeout=900, env=None):
    job = str(tmp_path / ("job_%d.npz" % len(os.listdir(str(tmp_path))))); np.savez(job, **arrays)
    r = subprocess.run([sys.executable, CHILD, op, job], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]; assert r.returncode == 0 and line, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(line[0][7:])

@pytest.fixture(scope="module")
def keys(tmp_path_factory):
    d = tmp_path_factory.mktemp("prfKey")
    for i, kind in enumerate(("send", "mint", "redeem", "deposit")): e.keygen(kind, str(d / (kind + "pk.txt")), str(d / (kind + "vk.txt")), seed=0xB10C4A2E + 7 * i)
    return d

@pytest.fixture(scope="module")
def send_proofs(keys):
    """(Zk, [(proof, args)] of three valid send proofs)"""
    old = os.environ.get("ZK_PRFKEY_DIR"); os.environ["ZK_PRFKEY_DIR"] = str(keys); zk = e.Zk(); out = []
    for i in range(3):
        sd = w.send_instance(91 + i); pr = zk.GenSendProof(*w.send_args(sd)); args = [sd["cmtA_old"], sd["sn_old"], sd["cmtS"], sd["cmtA"]]; assert zk.VerifySendProof(pr, *args); out.append((pr, args))
    yield zk, out
    if old is None: os.environ.pop("ZK_PRFKEY_DIR", None)
    else: os.environ["ZK_PRFKEY_DIR"] = old

def shifted(h, P):
    A, B, C = vm.points(vm.coords(h)); return vm.to_hex(vm.from_points(A, B, o.g1_op("add", C, P)))

def ingest_corpus(kind, mutations):
    """at least 20,000 records of a kind: seeded random, every edge case, every mutation of a send proof; and calls of 1, 63, 64, 65 and 8,193 records"""
    big = np.concatenate([br.random_records(kind, 20000, 0xD00D + kind), br.edge_records(kind, 0xE66 + kind), mutations]); big["kind"] = kind
    out = {"all": big}
    for n in (1, 63, 64, 65, 8193): out["n%05d" % n] = big[len(big) - n:].copy() if n < 100 else big[:n].copy()
    return out

@pytest.mark.parametrize("strict", [False, True])
def test_ingest_kernel_equals_the_host_converter(keys, send_proofs, tmp_path, strict):
    """zkgpu_test_ingest_records(device = 1) = (device = 0), byte for byte, for the four kinds; once more under ZK_STRICT_PROOF_ENCODING=1, in a child of its own"""
    zk, sends = send_proofs; proof, args = sends[0]; cases = vm.cases(str(keys / "sendvk.txt"), proof, w.pack_public(args), 0xF00D); assert len(cases) >= 250
    mutations = e.records_from_items([("send", c[1], args, 0) for c in cases])
    for kind in range(4):
        corpus = ingest_corpus(kind, mutations); assert len(corpus["all"]) >= 20000
        if strict: corpus = {"all": np.concatenate([corpus["all"], br.random_records(kind, 2000, 77, canonical=True), br.coordinate_records(kind, 78, canonical=True)])}
        res = in_child(tmp_path, "ingest", corpus, env={"ZK_STRICT_PROOF_ENCODING": "1"} if strict else None)
        for r in res: assert r["differ"] == [0, 0, 0], (kind, strict, r)
        total = [r for r in res if r["name"] == "all"][0]; assert 0 < total["parsed"] < total["n"], total    # (both outcomes of the parse are in the corpus)

def screen_flags(recs):
    """the screen by an independent road: 1 where the 512 bytes parse and A, B, C are points of their curves other than (0, 0)"""
    fl = []
    for rec in recs:
        ok, _ = br.model_item(rec)
        if not ok: fl.append(0); continue
        A, B, C = vm.points([c % br.Q for c in vm.coords(bytes(rec["proof"]).decode())]); zero = lambda P: all(x == 0 for x in (P if isinstance(P[0], int) else P[0] + P[1]))
        fl.append(1 if not zero(A) and not zero(C) and not (B[0][0] == B[0][1] == B[1][0] == B[1][1] == 0) and o.g1_on_curve(A) and o.g2_on_curve(B) and o.g1_on_curve(C) else 0)
    return np.array(fl, dtype=np.uint8)

def test_device_sums_and_equation_equal_the_host(keys, send_proofs, tmp_path):
    """explicit weights — random, all 1, all 2^128 - 1 — on valid sets, sets with bad records and the +-D pair (send key): the device's 448-bit sums are the host
    loop's bit for bit, and the equation's outcome and GT value are the host model's; on 20,000 records (several workgroups a row, a second grid-stride trip, a
    full fold) the sums again, and the equation holds"""
    zk, sends = send_proofs; rng = random.Random(3); vk = str(keys / "sendvk.txt")
    good = [("send", p, a, 0) for p, a in sends]; D = o.g1_op("mul", o.g1_gen(), k=rng.randrange(1, o.R_MOD)); c = vm.coords(sends[0][0]); off = list(c); off[7] = (off[7] + 1) % br.Q
    bad = [("send", shifted(sends[0][0], D), sends[0][1], 0), ("send", shifted(sends[1][0], vm.g1_neg(D)), sends[1][1], 0), ("send", sends[2][0], sends[0][1], 0)]
    screened = [("send", vm.to_hex(off), sends[0][1], 0), ("send", sends[1][0].upper(), sends[1][1], 0), ("send", sends[2][0][:100] + "\0" + sends[2][0][101:], sends[2][1], 0)]
    sets = [[good[i % 3] for i in range(20)], [good[i % 3] for i in range(10)] + bad, [good[0], good[1]] + bad[:2], [good[i % 3] for i in range(70)] + screened + bad[2:], [good[1]]]
    # 20,000 records: 79 workgroups of k_block_scalar_sums a row — more than the 64 the grid holds, so lanes take a second trip and the fold sees 64 partials
    large = [good[i % 3] for i in range(20000)]
    for i in (0, 255, 256, 16383, 16384, 19999): large[i] = screened[i % 3]
    sets.append(large); unit = {id(it): int(screen_flags(e.records_from_items([it]))[0]) for it in good + bad + screened}
    job = {"vk": np.array(vk), "n_sets": np.array(len(sets))}
    for k, s in enumerate(sets):
        recs = e.records_from_items(s); fl = np.array([unit[id(it)] for it in s], dtype=np.uint8); job["recs_%d" % k] = recs; job["flags_%d" % k] = fl
        job["model_%d" % k] = np.array(len(s) < 1000); job["holds_%d" % k] = np.array(True)       # (the large set: valid records and screened ones, so every equation holds)
        job["w_%d" % k] = np.frombuffer(b"".join(rng.randrange(1, 1 << 128).to_bytes(16, "little") for _ in s), dtype=np.uint8).reshape(len(s), 16)
    assert job["flags_3"].tolist().count(0) == 3 and all(job["flags_%d" % k].all() for k in (0, 1, 2, 4)) and job["flags_5"].tolist().count(0) == 6
    res = in_child(tmp_path, "equation", job); assert len(res) == 3 * len(sets)
    for r in res: assert r["dev"] == r["host"] and r["same_gt"] and r["same_sums"] and r["nonzero"], r
    by = {(r["set"], r["weights"]): r["host"] for r in res}
    assert by[(0, "random")] and by[(4, "max")] and not by[(1, "random")] and not by[(2, "random")] and by[(2, "ones")] and not by[(3, "random")]   # (+D and -D cancel under equal weights)

def test_verify_block_records_symbol_decides_like_verify_block(keys, send_proofs, tmp_path):
    """verifyBlockRecords on the four blocks of test_verify_block_symbol_decides_like_verify_batch — a mixed block above the threshold, the same kinds below it, at
    least 8,192 valid records of each of three kinds, 8,192 valid records and the +-D pair: ok[] is verifyBlock's and verifyBatch's on the equivalent items and the
    counters move as they do there.  Records whose proof bytes are corrupted (upper case, NUL) inside a valid block are the only ones rejected and the equation still
    decides the rest; a deposit record with garbage behind its 20 pk bytes decides like the clean one."""
    t0 = time.time(); zk, sends = send_proofs; vk = str(keys / "sendvk.txt"); (proof, args), (proof2, args2) = sends[:2]; inputs = w.pack_public(args)
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
    def counted(fn, arg):
        c0 = e.verify_rlc_counters(); p0 = e.verify_path_counters(vk); rc, ok = fn(arg); c1 = e.verify_rlc_counters(); p1 = e.verify_path_counters(vk)
        return rc, ok, [c1[k] - c0[k] for k in range(3)], p1 != p0
    def check(items, label, recs=None):
        rc, ok, moved, ran = counted(zk.VerifyBlockRecords, e.records_from_items(items) if recs is None else recs)
        rk, okk, moved_k, ran_k = counted(zk.VerifyBlock, items); rb, okb = zk.VerifyBatch(items)
        bad = [(i, items[i][0], ok[i], okk[i], okb[i]) for i in range(len(items)) if not (ok[i] == okk[i] == okb[i])]
        assert not bad and rc == rk == rb == sum(okb), (label, len(bad), bad[:5], rc, rk, rb)
        assert moved == moved_k and ran == ran_k, (label, moved, moved_k, ran, ran_k)
        return ok, moved, ran
    big = mixed(8200); assert sum(1 for it in big if it[0] == "send") >= N0 and len(big) >= 8500
    ok, moved, ran = check(big, "mixed block"); assert moved == [0, 1, 1] and ran
    ipair = [i for i, it in enumerate(big) if it in pair]; assert len(ipair) == 2 and not any(ok[i] for i in ipair)
    if os.path.exists(HARNESS):   # the send records' verdicts are libsnark's
        sc = [(str(i), it[1], w.pack_public(it[2])) for i, it in enumerate(big) if it[0] == "send"]; uniq = {}
        for c in sc: uniq.setdefault((c[1], tuple(c[2])), c)
        ref = dict(zip(uniq.keys(), vm.reference_verdicts(HARNESS, vk, list(uniq.values()), tmp_path)))
        assert all(vm.agrees(ok[int(c[0])], ref[(c[1], tuple(c[2]))]) for c in sc)
    ok, moved, ran = check(mixed(640), "below the threshold"); assert moved == [0, 0, 1]
    valid = [("send",) + sends[k % 2] + (0,) for k in range(N0)] + [valid_small[k % len(valid_small)] for k in range(2 * N0)]
    random.Random(9).shuffle(valid)
    ok, moved, ran = check(valid, "valid records of three kinds"); assert all(ok) and moved == [1, 0, 0] and not ran
    with_pair = [("send",) + sends[k % 2] + (0,) for k in range(N0)]; with_pair[100:100] = pair
    ok, moved, ran = check(with_pair, "the +-D pair"); assert moved == [0, 1, 1] and ok == [not (100 <= i < 102) for i in range(len(with_pair))]
    # corrupted proof bytes fail the screen, not the equation
    items = [("send",) + sends[k % 3] + (0,) for k in range(N0 + 50)]; corrupt = {17: lambda p: p.upper(), 4000: lambda p: p[:300] + "\0" + p[301:], N0 + 49: lambda p: p[:511] + "G", 5: lambda p: p[:64]}
    for i, f in corrupt.items(): items[i] = ("send", f(items[i][1]), items[i][2], 0)
    ok, moved, ran = check(items, "corrupted proof bytes"); assert moved == [1, 0, 0] and not ran and ok == [i not in corrupt for i in range(len(items))]
    recs = e.records_from_items([("send",) + sends[k % 3] + (0,) for k in range(N0)]); recs["proof"][123, 200] = ord("A"); recs["proof"][N0 - 1, 0] = 0; recs["reserved"] = 0xa5; recs["args"][:, 4:, :] = 0x5a
    rc, ok, moved, ran = counted(zk.VerifyBlockRecords, recs); assert moved == [1, 0, 0] and not ran and rc == N0 - 2 and ok == [i not in (123, N0 - 1) for i in range(N0)]
    # an unknown kind is rejected and does not disturb the rest
    recs = e.records_from_items([("send",) + sends[k % 3] + (0,) for k in range(40)]); recs["kind"][7] = 4; recs["kind"][9] = 255
    rc, ok = zk.VerifyBlockRecords(recs); assert rc == 38 and ok == [i not in (7, 9) for i in range(40)]
    # deposit at depth 8: garbage behind the 20 pk bytes changes nothing
    d = w.deposit_instance(11); dp = zk.GenDepositProof(*w.deposit_args(d), d["leaves"], d["rt"], d["sk"]); dargs = [d["rt"], d["pk_recv"], d["cmtB_old"], d["sn_old"], d["cmtB"], d["sn_s"]]
    assert zk.VerifyDepositProof(dp, *dargs)
    ditems = [("deposit", dp, dargs, 0), ("deposit", dp, [dargs[0], bytes(20)] + dargs[2:], 0)] + [("send",) + sends[0] + (0,)]
    clean = e.records_from_items(ditems); dirty = clean.copy(); dirty["args"][:2, 1, 20:] = np.random.default_rng(4).integers(0, 256, (2, 12), dtype=np.uint8); dirty["value_s"] = 99
    rb, okb = zk.VerifyBatch(ditems); assert okb == [True, False, True]
    for recs in (clean, dirty): rc, ok = zk.VerifyBlockRecords(recs); assert (rc, ok) == (rb, okb)
    record_leg("verifyBlockRecords: %d-record mixed block, %d valid records of three kinds" % (len(big), len(valid)), time.time() - t0)

def test_records_calls_from_threads_beside_provers(keys, send_proofs):
    """60 calls of 9,000 valid records (one wrong statement in every third call) from three threads beside two genSendproof callers: every verdict right, every
    proof made verifies — the ingest's staging area and the verifier's workspace are reused under the device mutex"""
    zk, sends = send_proofs; base = e.records_from_items([("send",) + sends[k % 3] + (0,) for k in range(9000)]); errors = []; made = []
    def verifier(t):
        try:
            for c in range(20):
                recs = base.copy(); bad = (c + t) % 3 == 0; at = (997 * c + 31 * t) % 9000
                if bad: recs["args"][at, 2, 31] ^= 1
                rc, ok = zk.VerifyBlockRecords(recs); want = [not (bad and i == at) for i in range(9000)]
                if ok != want or rc != sum(want): errors.append(("verdicts", t, c, rc, ok.count(False)))
        except Exception as ex: errors.append(("verifier", t, repr(ex)))
    def prover(t):
        try:
            for c in range(6):
                sd = w.send_instance(200 + 10 * t + c); made.append((zk.GenSendProof(*w.send_args(sd)), [sd["cmtA_old"], sd["sn_old"], sd["cmtS"], sd["cmtA"]]))
        except Exception as ex: errors.append(("prover", t, repr(ex)))
    before = e.verify_rlc_counters(); ths = [threading.Thread(target=verifier, args=(t,)) for t in range(3)] + [threading.Thread(target=prover, args=(t,)) for t in range(2)]
    for t in ths: t.start()
    for t in ths: t.join()
    after = e.verify_rlc_counters(); assert not errors, errors[:5]
    assert len(made) == 12 and all(zk.VerifySendProof(p, *a) for p, a in made)
    assert [after[k] - before[k] for k in range(3)] == [40, 20, 20]

def test_verify_block_records_without_a_device(keys, send_proofs, tmp_path):
    """a process that sees no device decides a 700-record mixed block on the host, as verifyBlock does: ok[] is the parent's verifyBatch verdicts"""
    zk, sends = send_proofs; m = w.mint_instance(92); mp = zk.GenMintProof(*w.mint_args(m)); ma = [m["cmtA_old"], m["sn_old"], m["cmtA"]]
    items = []
    for k in range(700):
        p, a = sends[k % 3]
        if k % 7 == 3: items.append(("mint", mp, ma, m["value_s"] + (k % 2)))
        elif k % 11 == 5: items.append(("send", p, sends[(k + 1) % 3][1], 0))
        elif k % 13 == 6: items.append(("send", p[:200] + "Z" + p[201:], a, 0))
        else: items.append(("send", p, a, 0))
    rb, okb = zk.VerifyBatch(items); assert 0 < rb < 700
    res = in_child(tmp_path, "no_device", {"recs": e.records_from_items(items)}, env={"HIP_VISIBLE_DEVICES": "", "ZK_PRFKEY_DIR": str(keys)})
    assert res["ok"] == okb and res["rc"] == rb and res["counters"] == [0, 0, 1]
