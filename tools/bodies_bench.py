#!/usr/bin/env python3
"""zkTxRecords beside zkTxSenders, and verifyChainBodies beside zkTxSenders + verifyChainAccounts; its output is the tables of profiles/bodies.txt.

    python tools/bodies_bench.py [--processes 5] [--calls 5] [--parent-lib OTHER/libzkgpu.so]
    python tools/bodies_bench.py --chain [--blocks 64] [--block 128] [--processes 5] [--calls 5] [--parent-lib OTHER/libzkgpu.so] [--keep DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bodies_bench.py --one 8192    # the kernels' share: a warm-up call and one call of zkTxRecords
    python tools/bodies_bench.py --summarize KERNEL_STATS.csv

DESIGN.md §12's protocol: fresh processes, every size warmed up by one call, a device synchronise (hipDeviceSynchronize) before every clock read; a process reports
the median of `calls` calls, the table the median and p10-p90 of those over the processes.  Only the C call is timed: the arrays are built before the clock starts.
Records: n = 128, 8,192 and 65,536 send-sized transactions (a 512-character ZKProof; 64 distinct ones, signed by the model under EIP155, repeated: lanes share
nothing), every one a ZK transaction ("zk") or every second one public ("mix").  The processes alternate between three kinds: "snd" times zkTxSenders, "rec"
zkTxRecords with the gather reading aligned words, "byt" zkTxRecords with the gather reading bytes; what records cost is read as a difference on one box in one session.
Chain: blocks x block distinct valid mint proofs, every transaction signed by a sender of its own, against a table of 2^16 other addresses, a set of 2^12 other
keys, a tree of depth 8, window 8 (§20's states).  "bodies" times verifyChainBodies; "parts" times zkTxSenders, then verifyChainAccounts on records built by the
caller OUTSIDE the timed region — on --parent-lib where given (ZKGPU_LIB).  That untimed build is the per-transaction host loop this header removes; it is Go in the
node, which no machine here runs: no ratio is claimed for it.  "trip" times a download and an upload of the m records through pinned memory, the part of verifyChainBodies
that handing the records on without the trip through recs would save.  One side is called faster only where the medians differ by more than the two spreads together."""
import ctypes, json, os, random, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [128, 8192, 65536]
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
def arg(name, default): return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
def sarg(name, default=None): return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
def spread(v): return "%9.3f (%9.3f-%9.3f)" % (pct(v, 0.5), pct(v, 0.1), pct(v, 0.9))
def verdict(a, b):
    d = pct(a, 0.5) - pct(b, 0.5); both = (pct(a, 0.9) - pct(a, 0.1)) + (pct(b, 0.9) - pct(b, 0.1))
    return "%+9.3f   spreads %.3f   %s" % (d, both, "beyond the spreads" if abs(d) > both else "inside the spreads: no difference claimed")
def children(kinds, procs, extra, env_of=lambda kind: None):
    runs = {k: [] for k in kinds}
    for p in range(procs):
        for kind in kinds:                                                                           # alternating: one session, one box
            env = dict(os.environ); env.update(env_of(kind) or {})
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind] + extra, capture_output=True, text=True, timeout=1500, env=env)
            line = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
            if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
            runs[kind].append(json.loads(line[0][5:])); print("process %d %s done" % (p, kind), flush=True)
    return runs

if "--summarize" in sys.argv:
    import csv
    print("average ns a launch, share of the run:")
    for r in csv.DictReader(open(sarg("--summarize"))): print("   %-18s %12.0f %6.1f %%  (%s calls)" % (r["Name"].split("(")[0].replace("zk::", ""), float(r["AverageNs"]), float(r["Percentage"]), r["Calls"]))
    sys.exit(0)

if "--child" not in sys.argv and "--one" not in sys.argv and "--chain" not in sys.argv:
    procs, calls = arg("--processes", 5), arg("--calls", 5); runs = children(("snd", "rec", "byt"), procs, ["--calls", str(calls)])
    print("wall time of the C call, ms: median (p10-p90) over %d processes a kind, alternating, each the median of %d calls after a warm-up call; %d bytes a transaction" % (procs, calls, runs["snd"][0]["bytes"]))
    for mix in ("zk", "mix"):
        for n in SIZES:
            v = {k: [r["%s_%d" % (mix, n)] for r in runs[k]] for k in runs}
            print("   %-3s n = %6d   zkTxSenders %s   zkTxRecords %s   (gather bytewise %s)" % (mix, n, spread(v["snd"]), spread(v["rec"]), spread(v["byt"])))
            print("       records cost (zkTxRecords less zkTxSenders)   %s" % verdict(v["rec"], v["snd"]))
            print("       bytewise less aligned                          %s" % verdict(v["byt"], v["rec"]))
    if "--parent-lib" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tools")); from proof_cache_bench import bench_ab
        bench_ab(sarg("--parent-lib"))
    sys.exit(0)

if "--chain" in sys.argv and "--child" not in sys.argv:
    procs, calls, blocks, block = arg("--processes", 5), arg("--calls", 5), arg("--blocks", 64), arg("--block", 128); d = sarg("--keep") or tempfile.mkdtemp(prefix="bodies_bench_")
    if not os.path.exists(os.path.join(d, "segment.json")):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "setup", "--dir", d, "--blocks", str(blocks), "--block", str(block)], timeout=3000)
        if r.returncode != 0: sys.exit(1)
    parent = sarg("--parent-lib"); extra = ["--dir", d, "--calls", str(calls), "--blocks", str(blocks), "--block", str(block)]
    runs = children(("bodies", "parts"), procs, extra, lambda kind: {"ZKGPU_LIB": parent} if (kind == "parts" and parent) else None)
    print("wall time, ms: median (p10-p90) over %d processes a road, alternating, each the median of %d calls after a warm-up call; %d blocks x %d mint records" % (procs, calls, blocks, block))
    b, p, trip = [r["ms"] for r in runs["bodies"]], [r["ms"] for r in runs["parts"]], [r["trip_ms"] for r in runs["bodies"]]
    print("   verifyChainBodies                                   %s" % spread(b))
    print("   zkTxSenders + verifyChainAccounts%s   %s   (the records built by the caller outside the timed region)" % (" on the parent's library" if parent else " on this build", spread(p)))
    print("   verifyChainBodies less the comparand                %s" % verdict(b, p))
    print("   the trip: 720 m bytes down and up again             %s   %.2f %% of verifyChainBodies" % (spread(trip), 100 * pct(trip, 0.5) / pct(b, 0.5)))
    sys.exit(0)

import numpy as np
import secp_model as sm
import tx_model as t
import tx_corpus as c
kind = sarg("--child", "rec"); CALLS = arg("--calls", 5); CHAIN = 1337
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

if kind == "setup":
    from blockmaze_amd import engine as e
    import workload as w
    d = sarg("--dir"); n = arg("--blocks", 64) * arg("--block", 128); os.environ["ZK_PRFKEY_DIR"] = d; t0 = time.time(); rng = random.Random(10)
    e.keygen("mint", os.path.join(d, "mintpk.txt"), os.path.join(d, "mintvk.txt"), seed=8); zk = e.Zk(); raws, olds, froms = [], [], []
    for i in range(n):
        x = w.mint_instance(5000 + i); proof = zk.GenMintProof(*w.mint_args(x)); key = 1 + i
        tx = c.rand_tx(rng, Code=1, Payload=b"", AUX=b"", ZKValue=x["value_s"], ZKSN=x["sn_old"], ZKCMT=x["cmtA"], ZKProof=proof.encode())
        raws.append(t.encode(t.sign_tx(tx, t.EIP155, CHAIN, key, rng.randrange(1, 2**20))).hex()); olds.append(x["cmtA_old"].hex())
    json.dump(dict(raws=raws, olds=olds), open(os.path.join(d, "segment.json"), "w")); print("setup: %d distinct mint proofs in signed transactions after %.0f s" % (n, time.time() - t0), flush=True)
    sys.exit(0)

from blockmaze_amd import engine as e
hip = ctypes.CDLL("libamdhip64.so")
def now(): hip.hipDeviceSynchronize(); return time.perf_counter()

if kind in ("bodies", "parts"):
    d = sarg("--dir"); os.environ["ZK_PRFKEY_DIR"] = d; BLOCK = arg("--block", 128); seg = json.load(open(os.path.join(d, "segment.json"))); raws = [bytes.fromhex(x) for x in seg["raws"]]; n = len(raws); nb = n // BLOCK
    e.init(); L = e.lib(); zk = e.Zk(); rng = np.random.default_rng(78); blob, off = e._tx_blob(raws); cid = ctypes.c_uint64(CHAIN); P = e._bytes
    fr, txhash, code, status = zk.TxSenders(raws, t.EIP155, CHAIN); assert status == [0] * n; froms = np.frombuffer(b"".join(fr), dtype=np.uint8).reshape(n, 20).copy()
    olds = np.frombuffer(b"".join(bytes.fromhex(x) for x in seg["olds"]), dtype=np.uint8).reshape(n, 32); other = rng.integers(0, 256, (1 << 16, 20), dtype=np.uint8)
    s = e.SpentSet(bytes(20)); s.spend(rng.integers(0, 256, (1 << 12, 20), dtype=np.uint8)); s0 = s.size(); tree = e.Tree(8); th = ctypes.c_void_p(tree.h); sh = ctypes.c_void_p(s.h)
    a = e.AccountTable(); a.set(other, rng.integers(0, 256, (1 << 16, 32), dtype=np.uint8)); a.set(froms, olds); n0 = a.size(); ah = ctypes.c_void_p(a.h)
    prior = np.zeros(1, dtype=np.int64); first = np.arange(0, n + 1, BLOCK, dtype=np.int32); ok = np.zeros(n, dtype=np.uint8); of = np.zeros(n, dtype=np.int32); sizes = [np.zeros(nb, dtype=np.int64) for _ in range(3)]
    th32, f20, cd, st = [np.zeros((n, w), dtype=np.uint8) for w in (32, 20, 1, 1)]; times, trips = [], []
    for f in (L.zkTxSenders, L.verifyChainAccounts): f.restype = ctypes.c_int
    if kind == "bodies":
        L.verifyChainBodies.restype = ctypes.c_int; recs = np.zeros(n, dtype=e.RECORD_DTYPE); rf = np.zeros((n, 20), dtype=np.uint8); rec_of = np.zeros(n, dtype=np.int32); m = ctypes.c_int(0)
    else:                                                                                            # the caller's own loop over the transactions, outside the timed region
        built = e.records_from_items([("mint", tx["ZKProof"], [bytes(32), tx["ZKSN"], tx["ZKCMT"]], tx["ZKValue"]) for tx in (t.decode(r)[0] for r in raws)])
    for call in range(CALLS + 1):
        if kind == "bodies":
            t0 = now()
            rc = L.verifyChainBodies(None, P(blob), e._u64p(off), n, vp(first), nb, 2, cid, ah, th, vp(prior), 1, 8, sh, vp(recs), vp(rf), vp(rec_of), vp(th32), vp(f20), vp(cd), vp(st), vp(ok), vp(of), *[vp(x) for x in sizes], ctypes.byref(m))
            t1 = now(); assert rc == nb and m.value == n, (rc, m.value)
        else:
            recs = built.copy(); t0 = now()
            assert L.zkTxSenders(P(blob), e._u64p(off), n, 2, cid, vp(th32), vp(f20), vp(cd), vp(st)) == n
            rc = L.verifyChainAccounts(None, vp(recs), vp(f20), n, vp(first), nb, ah, th, vp(prior), 1, 8, sh, vp(ok), vp(of), *[vp(x) for x in sizes]); t1 = now(); assert rc == nb, rc
        assert sizes[0][-1] == n0 + n and sizes[1][-1] == s0 + n; a.rewind(n0); s.rewind(s0)
        if call: times.append(1e3 * (t1 - t0))
    out = {"ms": statistics.median(times)}
    if kind == "bodies":                                                                             # the trip alone: 720 m bytes from the device into pinned memory and back
        nbytes = 720 * n; dev = ctypes.c_void_p(); pin = ctypes.c_void_p(); assert hip.hipMalloc(ctypes.byref(dev), ctypes.c_size_t(nbytes)) == 0 and hip.hipHostMalloc(ctypes.byref(pin), ctypes.c_size_t(nbytes), 0) == 0
        for call in range(CALLS + 1):
            t0 = now(); assert hip.hipMemcpy(pin, dev, ctypes.c_size_t(nbytes), 2) == 0 and hip.hipMemcpy(dev, pin, ctypes.c_size_t(nbytes), 1) == 0; t1 = now()
            if call: trips.append(1e3 * (t1 - t0))
        out["trip_ms"] = statistics.median(trips); hip.hipFree(dev); hip.hipHostFree(pin)
    print("JSON " + json.dumps(out)); sys.exit(0)

rng = random.Random(9); zk_pool, pub_pool = [], []
for k in range(64):
    tx = c.rand_tx(rng, Code=2, Payload=b"", AUX=b"", CMTBlock=[rng.randrange(2**32)]); zk_pool.append(t.encode(t.sign_tx(tx, t.EIP155, CHAIN, rng.randrange(1, 2**24), rng.randrange(1, 2**24))))
    pub_pool.append(t.encode(t.sign_tx(dict(tx, Code=0), t.EIP155, CHAIN, rng.randrange(1, 2**24), rng.randrange(1, 2**24))))
import bodies_model as bm
want = bm.records([zk_pool[0], pub_pool[1]], t.EIP155, CHAIN); assert want[5] == [t.OK, t.OK] and len(want[0]) == 1
e.init(); L = e.lib(); out = {"bytes": int(statistics.mean(len(p) for p in zk_pool))}; L.zkTxSenders.restype = ctypes.c_int; L.zkTxRecords.restype = ctypes.c_int
if kind == "byt": e.bodies_gather_bytewise(True)
if "--one" in sys.argv: SIZES = [arg("--one", 8192)]; CALLS = 1                                      # one warm-up call and one call: what a profiler run looks at
for mix in ("zk", "mix"):
    if "--one" in sys.argv and mix == "mix": continue
    for n in SIZES:
        raws = [(pub_pool if (mix == "mix" and i % 2) else zk_pool)[i % 64] for i in range(n)]; blob, off = e._tx_blob(raws); P = e._bytes; cid = ctypes.c_uint64(CHAIN); m = n if mix == "zk" else (n + 1) // 2
        th, fr, code, st, rf = [np.zeros(n * w, dtype=np.uint8) for w in (32, 20, 1, 1, 20)]; recs = np.zeros(n, dtype=e.RECORD_DTYPE); rec_of = np.zeros(n, dtype=np.int32)
        def senders(): assert L.zkTxSenders(P(blob), e._u64p(off), n, 2, cid, P(th), P(fr), P(code), P(st)) == n
        def records(): assert L.zkTxRecords(P(blob), e._u64p(off), n, 2, cid, vp(recs), P(rf), vp(rec_of), P(th), P(fr), P(code), P(st)) == m
        call = senders if kind == "snd" else records; call(); ts = []
        for _ in range(CALLS): t0 = now(); call(); ts.append(1e3 * (now() - t0))
        out["%s_%d" % (mix, n)] = statistics.median(ts)
        if kind != "snd": assert recs[0].tobytes() == want[0][0] and bytes(rf[:20]) == want[1][0]
print("JSON " + json.dumps(out))
