#!/usr/bin/env python3
"""The randomized block check against the per-proof batch verifier, same process, same all-valid proofs.
  * engine level: zkgpu_verify_batch_rlc against zkgpu_verify_batch on send proofs.  Device time per call from the HIP-event stages ("verify.batch": kernel K9's
    launches, "verify.block": the block kernels, chosen by the path the call reports), wall time of the C call itself (both calls get the same packed buffers).
    Below the crossover (RLC_MIN_RECORDS, capi_zk.cpp) the entry takes the per-proof path; the block kernels' own time there is measured through the test entry.
  * drop-in level: verifyBlock against verifyBatch (wall time of the call, statement packing included for both) on blocks of send records and on blocks with
    the same number of send, mint and redeem records.
python tools/verify_block_bench.py [sizes...]"""
import ctypes, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from blockmaze_amd import engine as e
from oracle import pyoracle as o
import workload as w
sizes = [int(a) for a in sys.argv[1:]] or [64, 256, 1024, 4096, 6144, 8192, 12288, 16384, 65536]
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
print("drop-in level (wall time of the call, statement packing included)", flush=True)
for label, per_kind in (("send", {"send": 16384}), ("send", {"send": 65536}), ("send+mint+redeem", {"send": 8192, "mint": 8192, "redeem": 8192}),
                        ("send+mint+redeem", {"send": 4096, "mint": 2048, "redeem": 2048})):
    blk = [items[k][i % 2] for k, m in per_kind.items() for i in range(m)]
    c0 = e.verify_rlc_counters(); t0 = time.perf_counter(); rc, ok = zk.VerifyBlock(blk); tbk = time.perf_counter() - t0; c1 = e.verify_rlc_counters()
    t0 = time.perf_counter(); rb, okb = zk.VerifyBatch(blk); tbt = time.perf_counter() - t0; assert rc == rb == len(blk) and ok == okb
    print("%-16s %s: verifyBatch %8.2f ms | verifyBlock %8.2f ms (%s) ratio %.2f" % (label, "/".join(str(m) for m in per_kind.values()), 1e3 * tbt, 1e3 * tbk,
          "one equation" if c1[0] - c0[0] == 1 else "per-proof", tbk / tbt), flush=True)
