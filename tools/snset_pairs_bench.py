#!/usr/bin/env python3
"""Two keys a record on one GPU (DESIGN.md "Two keys a record"); its output is profiles/snset_pairs.txt.

    python tools/snset_pairs_bench.py [--processes 5] [--calls 5] [--size 20] [--chain 4096] [--no-block] [--parent-lib OTHER/libzkgpu.so [--bench-reps 2]]

The protocol of tools/snset_bench.py: fresh processes, every configuration warmed up, a device synchronise (hipDeviceSynchronize) before every clock read; a process
reports the median of `calls` calls, the tables the median and p10-p90 of those over the processes.  Only the C calls are timed: keys are drawn before the clock starts.
  1. zkgpu_snset_spend_pairs with commit = 1 at n = 1, 8,192 and 65,536 records of fresh keys, every other record with two keys, no conflict inside the batch, on a
     set of 2^20 entries, against the same loop on a std::unordered_set (tools/snset_pairs_host.cpp) on one core of the same box, alternating.  After each call both
     sets go back to their size outside the clock (rewind; erase).  Rewinds leave tombstones, so some calls carry a rebuild: the column `rebuilds` counts them.
  2. The same batch of single keys through zkgpu_snset_spend_pairs and through zkgpu_snset_spend, alternating: what the fourth launch and the wider arrays cost.
  3. The alternating chain of L = 4,096 records (s1,p1), (s1,p2), (s3,p2), (s3,p4), ..., check-only: on the device alone (no cap: L / 2 rounds), and with the default
     cap of 8 rounds and the host finish; and the host loop of 1 on the same chain.
  4. verifyBlockState against verifyBlockFull (a set of 2^16 other keys, commit = 0) on 8,192 and 65,536 valid send records, 64 distinct proofs in rotation,
     alternating, one process.
  5. With --parent-lib: bench.py --gpus 1 --steps 50 --warmup 5 on this build and on the other library (ZKGPU_LIB), alternating; proofs/s, median step, and the bytes of
     the last proof of each run compared."""
import ctypes, json, os, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
NS = (1, 8192, 65536)
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
def arg(name, default, conv=int): return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

def host_lib():
    """tools/snset_pairs_host.cpp as a shared object in a temporary directory (SNSET_PAIRS_HOST_SO: the parent builds it once and its children load that one)"""
    so = os.environ.get("SNSET_PAIRS_HOST_SO")
    if not so:
        so = os.path.join(tempfile.mkdtemp(prefix="snset_pairs_host"), "libsnset_pairs_host.so"); subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tools", "snset_pairs_host.cpp"), "-o", so])
        os.environ["SNSET_PAIRS_HOST_SO"] = so
    H = ctypes.CDLL(so); H.hostpairs_new.restype = ctypes.c_void_p; H.hostpairs_size.restype = ctypes.c_uint64; return H

def run_child(args, timeout=900):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    line = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
    if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
    return json.loads(line[0][5:])

def parent():
    procs, calls, lg, L = arg("--processes", 5), arg("--calls", 5), arg("--size", 20), arg("--chain", 4096); host_lib()
    print("wall time of the C calls, ms: median (p10-p90) over %d processes, each the median of %d calls" % (procs, calls))
    runs = [run_child(["--child", str(lg), "--calls", str(calls), "--chain", str(L)]) for _ in range(procs)]; print("set of 2^%d entries (%d slots after filling)" % (lg, runs[0]["slots"]), flush=True)
    def col(key): v = [r[key] for r in runs]; return pct(v, 0.5), pct(v, 0.1), pct(v, 0.9)
    def versus(label, a, b, names, extra=""):
        (ma, la, ha), (mb, lb, hb) = col(a), col(b); gate = mb - ma > (ha - la) + (hb - lb)
        print("   %-34s | %9.4f (%9.4f-%9.4f) | %9.4f (%9.4f-%9.4f) | %7.2fx | %s%s" % (label, ma, la, ha, mb, lb, hb, mb / ma, "%s faster by more than both spreads" % names[0] if gate else
              "%s faster by more than both spreads" % names[1] if ma - mb > (ha - la) + (hb - lb) else "within the spreads", extra))
    print("   %-34s | %-31s | %-31s | %8s |" % ("1.", "spend_pairs", "std::unordered_set, one core", "ratio"))
    for n in NS: versus("pairs, commit, n = %d" % n, "pairs_dev_%d" % n, "pairs_host_%d" % n, ("device", "host"), "; rebuilds in %d of %d timed calls" % (sum(r["pairs_rebuilds_%d" % n] for r in runs), procs * calls))
    print("   %-34s | %-31s | %-31s | %8s |" % ("2.", "spend_pairs", "spend", "ratio"))
    for n in NS: versus("single keys, commit, n = %d" % n, "single_pairs_%d" % n, "single_spend_%d" % n, ("spend_pairs", "spend"))
    print("   3. the alternating chain of %d records, check-only" % L)
    for key, label in (("chain_device", "on the device alone (%d rounds)" % runs[0]["chain_device_rounds"]), ("chain_capped", "default cap: %d rounds and the host finish" % runs[0]["chain_capped_rounds"]),
                       ("chain_host", "std::unordered_set, one core")):
        m, l, h = col(key); print("      %-44s | %9.4f (%9.4f-%9.4f)" % (label, m, l, h))
    if "--no-block" not in sys.argv:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-block", "--calls", str(calls)], capture_output=True, text=True, timeout=1500)
        if r.returncode != 0: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
        print("\n".join(l[4:] for l in r.stdout.splitlines() if l.startswith("OUT ")), flush=True)   # (the library's own progress lines stay out of the table)
    bench_ab()

def bench_ab():
    other = arg("--parent-lib", None, str)
    if not other: return
    print("5. bench.py --gpus 1 --steps 50 --warmup 5, this build and the parent commit's library (ZKGPU_LIB), alternating in one session:"); proofs = {}
    for rep in range(arg("--bench-reps", 2)):
        for who in ("this", "parent"):
            env = dict(os.environ); env.pop("ZKGPU_LIB", None); out = tempfile.mkdtemp()
            if who == "parent": env["ZKGPU_LIB"] = os.path.abspath(other)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "5", "--dump-outputs", out], capture_output=True, text=True, timeout=900, env=env)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
            j = json.loads(line[-1]); s = j["step_ms"]; proofs.setdefault(who, set()).add(open(os.path.join(out, "proof.npy"), "rb").read())
            print("   %-7s value %8.1f proofs/s  p50 step %.4f ms (p10 %.4f, p90 %.4f)" % (who, j["value"], s["p50"], s.get("p10", 0.0), s.get("p90", 0.0)), flush=True)
    same = len(proofs["this"]) == 1 and proofs["this"] == proofs["parent"]
    print("   the last proof of every run: %s" % ("the same bytes from both libraries" if same else "DIFFERENT BYTES"))

def child(lg):
    from blockmaze_amd import engine as e
    CALLS = arg("--calls", 5); L_CHAIN = arg("--chain", 4096); hip = ctypes.CDLL("libamdhip64.so"); e.init(); L = e.lib(); H = host_lib(); S = 1 << lg; out = {}
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    rng = np.random.default_rng(os.getpid()); fresh = lambda n: rng.integers(0, 256, (n, 20), dtype=np.uint8)   # (160 random bits: repeats do not happen)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p); z = ctypes.c_size_t; u = ctypes.c_uint64
    s = e.SpentSet(); h = ctypes.c_void_p(s.h); hs = ctypes.c_void_p(H.hostpairs_new()); base = fresh(S); conf = np.zeros(max(max(NS), L_CHAIN) + 1, dtype=np.uint8); conf2 = conf.copy(); size = u(0)
    ones = np.ones(1 << 16, dtype=np.uint8); wide = np.zeros((1 << 16, 2, 20), dtype=np.uint8)
    for at in range(0, S, 1 << 16):                                                                     # filled in blocks of 2^16 keys, both sets
        blk = base[at:at + (1 << 16)]; assert L.zkgpu_snset_spend(h, ptr(blk), None, z(len(blk)), 1, ptr(conf), ctypes.byref(size)) == 0
        wide[:len(blk), 0] = blk; H.hostpairs_spend(hs, ptr(wide), ptr(ones), u(len(blk)), ptr(conf))
    assert size.value == S == H.hostpairs_size(hs); out["slots"] = len(s.slots()[0])
    for n in NS:                                                                                         # 1: every other record with two keys, device and host alternating
        ta, tb, reb = [], [], 0; nk = np.ones(n, dtype=np.uint8); nk[1::2] = 2; added = int(nk.sum())
        for i in range(CALLS + 1):
            k = fresh(2 * n).reshape(n, 2, 20); k0 = e.snset_launches(); r0 = e.snset_rounds()
            t0 = now(); rc = L.zkgpu_snset_spend_pairs(h, ptr(k), ptr(nk), z(n), 1, ptr(conf), ctypes.byref(size)); t1 = now(); H.hostpairs_spend(hs, ptr(k), ptr(nk), u(n), ptr(conf2)); t2 = now()
            assert rc == 0 and size.value == S + added and H.hostpairs_size(hs) == S + added and not conf[:n].any() and not conf2[:n].any(); d = e.snset_launches() - k0
            assert e.snset_rounds() == (r0[0] + 1, r0[1]) and d in (4, 5), d
            assert L.zkgpu_snset_rewind(h, u(S)) == 0; H.hostpairs_undo(hs)
            if i: ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1)); reb += d == 5
        out["pairs_dev_%d" % n] = statistics.median(ta); out["pairs_host_%d" % n] = statistics.median(tb); out["pairs_rebuilds_%d" % n] = reb
    for n in NS:                                                                                         # 2: one key a record, through both entries
        ta, tb = [], []; nk = np.ones(n, dtype=np.uint8)
        for i in range(CALLS + 1):
            k = fresh(n); k2 = np.zeros((n, 2, 20), dtype=np.uint8); k2[:, 0] = k
            t0 = now(); rc = L.zkgpu_snset_spend_pairs(h, ptr(k2), ptr(nk), z(n), 1, ptr(conf), ctypes.byref(size)); t1 = now(); assert rc == 0 and size.value == S + n and not conf[:n].any()
            assert L.zkgpu_snset_rewind(h, u(S)) == 0
            t2 = now(); rc = L.zkgpu_snset_spend(h, ptr(k), None, z(n), 1, ptr(conf), ctypes.byref(size)); t3 = now(); assert rc == 0 and size.value == S + n and not conf[:n].any()
            assert L.zkgpu_snset_rewind(h, u(S)) == 0
            if i: ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t3 - t2))
        out["single_pairs_%d" % n] = statistics.median(ta); out["single_spend_%d" % n] = statistics.median(tb)
    # 3: the alternating chain, check-only: the rounds alone, the default cap with the host finish, the host loop
    ks = fresh(2 * L_CHAIN + 2); ch = np.zeros((L_CHAIN, 2, 20), dtype=np.uint8); nk = np.full(L_CHAIN, 2, dtype=np.uint8)
    for i in range(L_CHAIN): ch[i, 0] = ks[2 * (i // 2)]; ch[i, 1] = ks[2 * ((i + 1) // 2) + 1]
    want = np.array([i % 2 * 2 for i in range(L_CHAIN)], dtype=np.uint8)
    for key, cap in (("chain_device", 1 << 30), ("chain_capped", 0)):
        s.round_cap(cap); ts = []
        for i in range(CALLS + 1):
            r0 = e.snset_rounds(); t0 = now(); rc = L.zkgpu_snset_spend_pairs(h, ptr(ch), ptr(nk), z(L_CHAIN), 0, ptr(conf), ctypes.byref(size)); t1 = now(); r1 = e.snset_rounds()
            assert rc == 0 and size.value == S and (conf[:L_CHAIN] == want).all(); out[key + "_rounds"] = r1[0] - r0[0]; assert r1[1] - r0[1] == (cap == 0)
            if i: ts.append(1e3 * (t1 - t0))
        out[key] = statistics.median(ts)
    ts = []
    for i in range(CALLS + 1):
        t0 = now(); H.hostpairs_spend(hs, ptr(ch), ptr(nk), u(L_CHAIN), ptr(conf2)); t1 = now(); assert ((conf2[:L_CHAIN] != 0) == (want != 0)).all(); H.hostpairs_undo(hs)
        if i: ts.append(1e3 * (t1 - t0))
    out["chain_host"] = statistics.median(ts)
    assert s.read_log(S - 2, 2) == [base[S - 2].tobytes(), base[S - 1].tobytes()]; s.close(); H.hostpairs_free(hs); print("JSON " + json.dumps(out), flush=True)

def child_block():
    from blockmaze_amd import engine as e
    import workload as w
    CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so"); e.init()
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    d = tempfile.mkdtemp(prefix="snset_keys"); os.environ["ZK_PRFKEY_DIR"] = d; e.keygen("send", os.path.join(d, "sendpk.txt"), os.path.join(d, "sendvk.txt"), seed=8); zk = e.Zk(); items = []
    for i in range(64): x = w.send_instance(300 + i); items.append(("send", zk.GenSendProof(*w.send_args(x)), [x["cmtA_old"], x["sn_old"], x["cmtS"], x["cmtA"]], 0))
    unit = e.records_from_items(items); s = zk.SnSetNew(); assert s
    print("OUT 4. verifyBlockState against verifyBlockFull (a set of 2^16 other keys, commit = 0), valid send records, 64 distinct proofs in rotation, alternating, one process, median of %d calls (p10-p90), ms" % CALLS)
    assert zk.SnSetSpend(s, [os.urandom(32) for _ in range(1 << 16)])[0] == 1 << 16
    for n in (8192, 65536):
        recs = np.ascontiguousarray(np.tile(unit, n // 64)); lo = [-1] * n; ta, tb = [], []
        for i in range(CALLS + 1):
            t0 = now(); rc0, ok0, size0 = zk.VerifyBlockFull(recs, None, None, lo, s, False); t1 = now(); rc1, ok1, size = zk.VerifyBlockState(None, recs, None, None, lo, s, False); t2 = now()
            assert rc0 == rc1 == 64 and ok1 == ok0 and ok1[:64] == [True] * 64 and not any(ok1[64:]) and size == size0 == 1 << 16
            if i: ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1))
        print("OUT    n = %-6d verifyBlockFull %8.3f (%8.3f-%8.3f)   verifyBlockState %8.3f (%8.3f-%8.3f)   the difference %+.3f ms (both through the Python binding)"
              % (n, statistics.median(ta), pct(ta, 0.1), pct(ta, 0.9), statistics.median(tb), pct(tb, 0.1), pct(tb, 0.9), statistics.median(tb) - statistics.median(ta)), flush=True)
    zk.SnSetFree(s)

if __name__ == "__main__":
    if "--child" in sys.argv: child(int(sys.argv[sys.argv.index("--child") + 1]))
    elif "--child-block" in sys.argv: child_block()
    else: parent()
