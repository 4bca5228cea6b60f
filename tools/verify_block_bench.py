#!/usr/bin/env python3
"""The randomized block check against the per-proof batch verifier, same process, same all-valid proofs.
  * engine level: zkgpu_verify_batch_rlc against zkgpu_verify_batch on send proofs.  Device time per call from the HIP-event stages ("verify.batch": kernel K9's
    launches, "verify.block": the block kernels, chosen by the path the call reports), wall time of the C call itself (both calls get the same packed buffers).
    Below the crossover (RLC_MIN_RECORDS, capi_zk.cpp) the entry takes the per-proof path; the block kernels' own time there is measured through the test entry.
  * drop-in level: verifyBlock against verifyBatch (wall time of the call, statement packing included for both) on blocks of send records and on blocks with
    the same number of send, mint and redeem records.
  * from records (--records): the C calls alone — the item array and the record array are built before the clock starts — verifyBlock against verifyBlockRecords
    (include/zk_records.h) where the library has it, every block warmed up, medians of --reps calls; for the new entry the device stages of one more call
    (upload, k_ingest_records, block kernels, k_block_scalar_sums) beside the host's spans (staging copy, weights, S_acc, the closing Miller loops and final
    exponentiation; host.other is what is left of the wall time) and the equation forced at 4,096 and 6,144 records through the test entry.
  * --alternate OTHER_LIB N: the --records run in fresh processes, this build and OTHER_LIB (through ZKGPU_LIB) in turn, N times; medians and p10-p90 over
    the processes' medians, one table.
python tools/verify_block_bench.py [sizes...] | --records [--reps R] | --alternate OTHER_LIB N"""
import ctypes, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
BLOCKS = (("send 8192", {"send": 8192}), ("send 16384", {"send": 16384}), ("send 65536", {"send": 65536}), ("send+mint+redeem 8192 each", {"send": 8192, "mint": 8192, "redeem": 8192}),
          ("send+mint+redeem 4096/2048/2048", {"send": 4096, "mint": 2048, "redeem": 2048}))
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
if "--alternate" in sys.argv:
    other, rounds = sys.argv[sys.argv.index("--alternate") + 1], int(sys.argv[sys.argv.index("--alternate") + 2]); runs = {"this": [], "other": []}
    for k in range(rounds):
        for who in (("this", "other") if k % 2 == 0 else ("other", "this")):
            env = dict(os.environ); env.pop("ZKGPU_LIB", None)
            if who == "other": env["ZKGPU_LIB"] = other
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--records", "--reps", "5"], capture_output=True, text=True, env=env, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
            if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
            runs[who].append(json.loads(line[0][5:])); print("round %d %s done" % (k, who), flush=True)
    def col(who, label, key): v = [r[label][key] for r in runs[who] if key in r[label]]; return "%8.2f (%7.2f-%7.2f)" % (pct(v, 0.5), pct(v, 0.1), pct(v, 0.9)) if v else "       -"
    print("wall time of the C call, ms: median (p10-p90) over %d processes a build, each the median of 5 calls" % rounds)
    print("%-34s | %-28s | %-28s | %-28s" % ("block", "other verifyBlock", "this verifyBlock", "this verifyBlockRecords"))
    for label, _ in BLOCKS: print("%-34s | %s | %s | %s" % (label, col("other", label, "block"), col("this", label, "block"), col("this", label, "records")))
    print("this build, verifyBlockRecords, device stages of one call (ms) and the host's share of the wall time")
    for label, _ in BLOCKS:
        st = [r[label]["stages"] for r in runs["this"] if "stages" in r[label]]
        if st: print("%-34s | " % label + " | ".join("%s %7.3f" % (k, pct([x.get(k, 0.0) for x in st], 0.5)) for k in ("wall", "host.staging", "host.weights", "verify.upload", "verify.ingest", "verify.block", "verify.sums", "host.s_acc", "host.closing", "verify.batch", "host.other")))
    for n in (4096, 6144):
        v = [r["forced"][str(n)] for r in runs["this"] if "forced" in r]
        if v: print("equation forced at %d send records (test entry, records): %8.2f ms (%7.2f-%7.2f)" % (n, pct(v, 0.5), pct(v, 0.1), pct(v, 0.9)))
    sys.exit(0)
from blockmaze_amd import engine as e
from oracle import pyoracle as o
import workload as w
RECORDS = "--records" in sys.argv; REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
sizes = [] if RECORDS else [int(a) for a in sys.argv[1:]] or [64, 256, 1024, 4096, 6144, 8192, 12288, 16384, 65536]
tmp = tempfile.mkdtemp()
for i, kind in enumerate(("send", "mint", "redeem")): e.keygen(kind, os.path.join(tmp, kind + "pk.txt"), os.path.join(tmp, kind + "vk.txt"), seed=1 + i)
vk = os.path.join(tmp, "sendvk.txt"); p = e.Prover(os.path.join(tmp, "sendpk.txt")); base = []
for i in range(4):
    d = w.send_instance(i); wp = os.path.join(tmp, "w.bin"); e.witness_send(*[("0x" + a.hex()) if isinstance(a, bytes) else a for a in w.send_args(d)], wp)
    base.append((p.prove(o.load_witness(wp)), w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]])))
p.close()
L = e.lib(); e.verify_batch(vk, [base[0][0]], [base[0][1]]); e.verify_batch_rlc(vk, [base[0][0]], [base[0][1]])
def staged(fn):
    e.profile_enable(True); t0 = time.perf_counter(); r = fn(); t = time.perf_counter() - t0; st = e.profile_report(); e.profile_enable(False)
    return r, 1e3 * t, {k: v["ms_total"] for k, v in st.items()}
print("engine level, send key (seed 1), 4 valid proofs cycled", flush=True)
for n in sizes:
    proofs = [base[i % 4][0] for i in range(n)]; ins = [base[i % 4][1] for i in range(n)]
    _, ni, blob, buf, _ = e._batch_args(proofs, ins, None); ok = (ctypes.c_uint8 * n)(); by = ctypes.c_uint32(0)
    rc, tb, sb = staged(lambda: L.zkgpu_verify_batch(vk.encode(), blob, buf, ctypes.c_size_t(ni), ctypes.c_size_t(n), ok)); assert rc == 0 and all(ok[:n])
    rc, tr, sr = staged(lambda: L.zkgpu_verify_batch_rlc(vk.encode(), blob, buf, ctypes.c_size_t(ni), ctypes.c_size_t(n), None, ok, ctypes.byref(by))); assert rc == 0 and all(ok[:n])
    db = sb.get("verify.batch", 0.0); dr = sr.get("verify.block" if by.value else "verify.batch", 0.0)
    line = "n = %6d: verify_batch device %8.2f ms (call %8.2f) | verify_batch_rlc %s device %8.2f ms (call %8.2f) ratio %.2f" % (n, db, tb, "equation " if by.value else "per-proof", dr, tr, dr / db)
    if not by.value:
        wts = [1 + i for i in range(n)]; (okk, _), _, sk = staged(lambda: e.verify_rlc_equation(vk, proofs, ins, wts, device=True)); assert okk
        line += " | block kernels alone %8.2f ms" % sk.get("verify.block", 0.0)
    print(line, flush=True)
os.environ["ZK_PRFKEY_DIR"] = tmp; zk = e.Zk(); items = {"send": [], "mint": [], "redeem": []}
for i in range(2):
    d = w.send_instance(10 + i); items["send"].append(("send", zk.GenSendProof(*w.send_args(d)), [d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]], 0))
    m = w.mint_instance(20 + i); items["mint"].append(("mint", zk.GenMintProof(*w.mint_args(m)), [m["cmtA_old"], m["sn_old"], m["cmtA"]], m["value_s"]))
    r = w.mint_instance(30 + i, redeem=True); items["redeem"].append(("redeem", zk.GenRedeemProof(*w.mint_args(r)), [r["cmtA_old"], r["sn_old"], r["cmtA"]], r["value_s"]))
zk.VerifyBatch(items["send"] + items["mint"] + items["redeem"]); zk.VerifyBlock(items["send"] + items["mint"] + items["redeem"])
if RECORDS:
    class Item(ctypes.Structure): _fields_ = [("kind", ctypes.c_int), ("proof", ctypes.c_char_p), ("args", ctypes.c_char_p * 6), ("value_s", ctypes.c_uint64)]
    has_records = hasattr(L, "verifyBlockRecords") and hasattr(e, "records_from_items"); out = {}
    def timed(fn, reps, want):
        ts = []
        for _ in range(reps): t0 = time.perf_counter(); rc = fn(); ts.append(1e3 * (time.perf_counter() - t0)); assert rc == want, rc
        return pct(ts, 0.5)
    for label, per_kind in BLOCKS:
        blk = [items[k][i % 2] for k, m in per_kind.items() for i in range(m)]; n = len(blk); arr = (Item * n)(); keep = []; ok = (ctypes.c_ubyte * n)()
        for i, (kind, proof, args, value_s) in enumerate(blk):
            arr[i].kind = e.KIND[kind]; pb = proof.encode(); keep.append(pb); arr[i].proof = pb; arr[i].value_s = int(value_s)
            for j, a in enumerate(args): hb = zk.hx(a); keep.append(hb); arr[i].args[j] = hb
        L.verifyBlock.restype = ctypes.c_int; f_block = lambda: L.verifyBlock(arr, n, ok); f_block(); row = {"block": timed(f_block, REPS, n)}
        if has_records:
            recs = e.records_from_items(blk); ptr = recs.ctypes.data_as(ctypes.c_void_p); L.verifyBlockRecords.restype = ctypes.c_int
            f_rec = lambda: L.verifyBlockRecords(ptr, n, ok); f_rec(); row["records"] = timed(f_rec, REPS, n)
            _, wall, st = staged(f_rec); st["host.other"] = wall - sum(st.values()); st["wall"] = wall; row["stages"] = st
        out[label] = row; print(label, row, flush=True)
    if has_records:
        out["forced"] = {}
        for n in (4096, 6144):
            recs = e.records_from_items([items["send"][i % 2] for i in range(n)]); ptr = recs.ctypes.data_as(ctypes.c_void_p); gt = (ctypes.c_uint8 * 384)(); sums = (ctypes.c_uint64 * 49)()
            wb = b"".join((1 + i).to_bytes(16, "little") for i in range(n)); kvk = os.path.join(tmp, "sendvk.txt").encode()
            f_eq = lambda: L.zkgpu_test_records_rlc(kvk, ptr, ctypes.c_size_t(n), wb, gt, sums); assert f_eq() == 1; out["forced"][str(n)] = timed(f_eq, REPS, 1)
    print("JSON " + json.dumps(out), flush=True); sys.exit(0)
print("drop-in level (wall time of the call, statement packing included)", flush=True)
for label, per_kind in (("send", {"send": 16384}), ("send", {"send": 65536}), ("send+mint+redeem", {"send": 8192, "mint": 8192, "redeem": 8192}),
                        ("send+mint+redeem", {"send": 4096, "mint": 2048, "redeem": 2048})):
    blk = [items[k][i % 2] for k, m in per_kind.items() for i in range(m)]
    c0 = e.verify_rlc_counters(); t0 = time.perf_counter(); rc, ok = zk.VerifyBlock(blk); tbk = time.perf_counter() - t0; c1 = e.verify_rlc_counters()
    t0 = time.perf_counter(); rb, okb = zk.VerifyBatch(blk); tbt = time.perf_counter() - t0; assert rc == rb == len(blk) and ok == okb
    print("%-16s %s: verifyBatch %8.2f ms | verifyBlock %8.2f ms (%s) ratio %.2f" % (label, "/".join(str(m) for m in per_kind.values()), 1e3 * tbt, 1e3 * tbk,
          "one equation" if c1[0] - c0[0] == 1 else "per-proof", tbk / tbt), flush=True)
