#!/usr/bin/env python3
"""The resident set of spent serial numbers on one GPU (DESIGN.md "Spent serial numbers"); its output is profiles/snset.txt.

    python tools/snset_bench.py [--processes 5] [--calls 5] [--sizes 16,20,24] [--no-block] [--parent-lib OTHER/libzkgpu.so [--bench-reps 2]]

The protocol of tools/list_roots_bench.py: fresh processes, every configuration warmed up, a device synchronise (hipDeviceSynchronize) before every clock read; a
process reports the median of `calls` calls, the tables the median and p10-p90 of those over the processes.  Only the C calls are timed: keys are drawn before the clock starts.
  1. zkgpu_snset_spend with commit = 1 at n = 1, 8,192 and 65,536 fresh keys on sets of 2^16, 2^20 and 2^24 entries, against the same loop on a std::unordered_set
     (tools/snset_host.cpp) on one core of the same box, alternating.  After each call both sets go back to their size outside the clock (rewind; erase).  Rewinds leave
     tombstones, so some calls carry a rebuild: the column `rebuilds` says how many of the timed calls did (the launch counter moved by four, not three).
  2. zkgpu_snset_query of 1 and of 8,192 keys (half of them present) against the same look-ups on the host set.
  3. zkgpu_snset_rewind by 1, by 1,000 and by 2^19 entries (the last on sets that hold more), the entries put back outside the clock.
  4. A rebuild at 2^20 entries: a set filled to exactly 2^20 entries has 2^21 slots and no room for one more key, so a check-only spend of one key runs on a rebuilt
     copy, every time; the same call on a set with room is the other column.
  5. verifyBlockFull with a set (commit = 0) against verifyBlockRecordsRoots on 8,192 and 65,536 valid send records (64 distinct proofs in rotation, so every serial
     number repeats: the slot of a key is hit by 128 or 1,024 lanes), alternating, one process.
  6. With --parent-lib: bench.py --gpus 1 --steps 50 --warmup 5 on this build and on the other library (ZKGPU_LIB), alternating; proofs/s, median step, and the bytes of
     the last proof of each run compared."""
import ctypes, json, os, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
NS = (1, 8192, 65536); QS = (1, 8192); BACK = (1, 1000, 1 << 19)
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
def arg(name, default, conv=int): return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

def host_lib():
    """tools/snset_host.cpp as a shared object in a temporary directory (SNSET_HOST_SO: the parent builds it once and its children load that one)"""
    so = os.environ.get("SNSET_HOST_SO")
    if not so:
        so = os.path.join(tempfile.mkdtemp(prefix="snset_host"), "libsnset_host.so"); subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tools", "snset_host.cpp"), "-o", so])
        os.environ["SNSET_HOST_SO"] = so
    H = ctypes.CDLL(so); H.hostset_new.restype = ctypes.c_void_p; H.hostset_size.restype = ctypes.c_uint64; return H

def run_child(args, timeout=1500):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    line = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
    if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
    return json.loads(line[0][5:])

def parent():
    procs, calls = arg("--processes", 5), arg("--calls", 5); sizes = [int(x) for x in arg("--sizes", "16,20,24", str).split(",")]; host_lib()
    print("wall time of the C calls, ms: median (p10-p90) over %d processes, each the median of %d calls" % (procs, calls))
    for lg in sizes:
        runs = [run_child(["--child", str(lg), "--calls", str(calls)]) for _ in range(procs)]; print("set of 2^%d entries (%d slots after filling)" % (lg, runs[0]["slots"]), flush=True)
        def col(key): v = [r[key] for r in runs]; return pct(v, 0.5), pct(v, 0.1), pct(v, 0.9)
        def versus(label, a, b, extra=""):
            (ma, la, ha), (mb, lb, hb) = col(a), col(b); gate = mb - ma > (ha - la) + (hb - lb)
            print("   %-26s | %9.4f (%9.4f-%9.4f) | %9.4f (%9.4f-%9.4f) | %7.2fx | %s%s" % (label, ma, la, ha, mb, lb, hb, mb / ma, "device faster by more than both spreads" if gate else
                  "host faster by more than both spreads" if ma - mb > (ha - la) + (hb - lb) else "within the spreads", extra))
        print("   %-26s | %-31s | %-31s | %8s |" % ("", "device", "std::unordered_set, one core", "ratio"))
        for n in NS: versus("1. spend, commit, n = %d" % n, "spend_dev_%d" % n, "spend_host_%d" % n, "; rebuilds in %d of %d timed calls" % (sum(r["spend_rebuilds_%d" % n] for r in runs), procs * calls))
        for q in QS: versus("2. query of %d" % q, "query_dev_%d" % q, "query_host_%d" % q)
        for b in BACK:
            if ("rewind_%d" % b) in runs[0]: m, l, h = col("rewind_%d" % b); print("   3. rewind by %-13d | %9.4f (%9.4f-%9.4f)" % (b, m, l, h))
        if "tight_1" in runs[0]:
            (ma, la, ha), (mb, lb, hb) = col("tight_1"), col("roomy_1")
            print("   4. check-only spend of one key: with a rebuild of 2^%d entries %9.4f (%9.4f-%9.4f), with room %9.4f (%9.4f-%9.4f): the rebuild costs %.4f ms" % (lg, ma, la, ha, mb, lb, hb, ma - mb))
    if "--no-block" not in sys.argv:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-block", "--calls", str(calls)], capture_output=True, text=True, timeout=1500)
        if r.returncode != 0: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
        print("\n".join(l[4:] for l in r.stdout.splitlines() if l.startswith("OUT ")), flush=True)   # (the library's own progress lines stay out of the table)
    bench_ab()

def bench_ab():
    other = arg("--parent-lib", None, str)
    if not other: return
    print("6. bench.py --gpus 1 --steps 50 --warmup 5, this build and the parent commit's library (ZKGPU_LIB), alternating in one session:"); proofs = {}
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
    CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so"); e.init(); L = e.lib(); H = host_lib(); S = 1 << lg; out = {}
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    rng = np.random.default_rng(os.getpid()); fresh = lambda n: rng.integers(0, 256, (n, 20), dtype=np.uint8)   # (160 random bits: repeats do not happen)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p); z = ctypes.c_size_t; u = ctypes.c_uint64
    s = e.SpentSet(); h = ctypes.c_void_p(s.h); hs = ctypes.c_void_p(H.hostset_new()); base = fresh(S); conf = np.zeros(max(NS) + 1, dtype=np.uint8); size = u(0)
    for at in range(0, S, 1 << 16):                                                                     # filled in blocks of 2^16 keys, both sets
        blk = base[at:at + (1 << 16)]; assert L.zkgpu_snset_spend(h, ptr(blk), None, z(len(blk)), 1, ptr(conf), ctypes.byref(size)) == 0; H.hostset_spend(hs, ptr(blk), u(len(blk)), 1, ptr(conf))
    assert size.value == S == H.hostset_size(hs); out["slots"] = len(s.slots()[0])
    def check_only_one():
        ts = []
        for i in range(CALLS + 1):
            k = fresh(1); k0 = e.snset_launches(); t0 = now(); rc = L.zkgpu_snset_spend(h, ptr(k), None, z(1), 0, ptr(conf), None); t1 = now(); assert rc == 0; ts.append((1e3 * (t1 - t0), e.snset_launches() - k0))
        return statistics.median(t for t, _ in ts[1:]), [d for _, d in ts[1:]]
    if lg == 20:                                                                                         # 4: no room for one more key in 2^21 slots
        assert out["slots"] == 1 << 21; out["tight_1"], d = check_only_one(); assert d == [4] * CALLS, d
    for n in NS:                                                                                         # 1: spend with commit, device and host alternating
        ta, tb, reb = [], [], 0
        for i in range(CALLS + 1):
            k = fresh(n); k0 = e.snset_launches()
            t0 = now(); rc = L.zkgpu_snset_spend(h, ptr(k), None, z(n), 1, ptr(conf), ctypes.byref(size)); t1 = now(); H.hostset_spend(hs, ptr(k), u(n), 1, ptr(conf)); t2 = now()
            assert rc == 0 and size.value == S + n and H.hostset_size(hs) == S + n and not conf[:n].any(); d = e.snset_launches() - k0
            assert L.zkgpu_snset_rewind(h, u(S)) == 0; H.hostset_undo(hs)
            if i: ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1)); reb += d == 4
        out["spend_dev_%d" % n] = statistics.median(ta); out["spend_host_%d" % n] = statistics.median(tb); out["spend_rebuilds_%d" % n] = reb
    if lg == 20: out["roomy_1"], d = check_only_one(); assert d == [3] * CALLS, d
    for q in QS:                                                                                         # 2: queries, half of the keys present
        ta, tb = [], []; idx = np.zeros(q, dtype=np.uint64); inn = np.zeros(q, dtype=np.uint8)
        for i in range(CALLS + 1):
            k = fresh(q); k[::2] = base[rng.integers(0, S, len(k[::2]))]
            t0 = now(); rc = L.zkgpu_snset_query(h, u(S), ptr(k), z(q), ptr(idx)); t1 = now(); H.hostset_query(hs, ptr(k), u(q), ptr(inn)); t2 = now()
            assert rc == 0 and ((idx != np.uint64(e.ABSENT)) == (inn != 0)).all() and inn[::2].all() and not inn[1::2].any()
            if i: ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1))
        out["query_dev_%d" % q] = statistics.median(ta); out["query_host_%d" % q] = statistics.median(tb)
    for b in BACK:                                                                                       # 3: rewind, the entries put back outside the clock
        if b >= S: continue
        ts = []; big = np.zeros(b, dtype=np.uint8)
        for i in range(CALLS + 1):
            t0 = now(); rc = L.zkgpu_snset_rewind(h, u(S - b)); t1 = now(); assert rc == 0
            assert L.zkgpu_snset_spend(h, ptr(base[S - b:]), None, z(b), 1, ptr(big), ctypes.byref(size)) == 0 and size.value == S and not big.any()
            if i: ts.append(1e3 * (t1 - t0))
        out["rewind_%d" % b] = statistics.median(ts)
    assert s.read_log(S - 2, 2) == [base[S - 2].tobytes(), base[S - 1].tobytes()]; s.close(); H.hostset_free(hs); print("JSON " + json.dumps(out), flush=True)

def child_block():
    from blockmaze_amd import engine as e
    import workload as w
    CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so"); e.init()
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    d = tempfile.mkdtemp(prefix="snset_keys"); os.environ["ZK_PRFKEY_DIR"] = d; e.keygen("send", os.path.join(d, "sendpk.txt"), os.path.join(d, "sendvk.txt"), seed=8); zk = e.Zk(); items = []
    for i in range(64): x = w.send_instance(300 + i); items.append(("send", zk.GenSendProof(*w.send_args(x)), [x["cmtA_old"], x["sn_old"], x["cmtS"], x["cmtA"]], 0))
    unit = e.records_from_items(items); s = zk.SnSetNew(); assert s
    print("OUT 5. verifyBlockFull (a set of 2^16 other keys, commit = 0) against verifyBlockRecordsRoots, valid send records, 64 distinct proofs in rotation, alternating, one process, median of %d calls (p10-p90), ms" % CALLS)
    assert zk.SnSetSpend(s, [os.urandom(32) for _ in range(1 << 16)])[0] == 1 << 16
    for n in (8192, 65536):
        recs = np.ascontiguousarray(np.tile(unit, n // 64)); lo = [-1] * n; ta, tb = [], []
        for i in range(CALLS + 1):
            t0 = now(); rc0, ok0 = zk.VerifyBlockRecordsRoots(recs, None, None, lo); t1 = now(); rc1, ok1, size = zk.VerifyBlockFull(recs, None, None, lo, s, False); t2 = now()
            assert rc0 == n and rc1 == 64 and ok1[:64] == [True] * 64 and not any(ok1[64:]) and size == 1 << 16
            if i: ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1))
        print("OUT    n = %-6d verifyBlockRecordsRoots %8.3f (%8.3f-%8.3f)   verifyBlockFull %8.3f (%8.3f-%8.3f)   the serial-number check adds %+.3f ms (both through the Python binding)"
              % (n, statistics.median(ta), pct(ta, 0.1), pct(ta, 0.9), statistics.median(tb), pct(tb, 0.1), pct(tb, 0.9), statistics.median(tb) - statistics.median(ta)), flush=True)
    zk.SnSetFree(s)

if __name__ == "__main__":
    if "--child" in sys.argv: child(int(sys.argv[sys.argv.index("--child") + 1]))
    elif "--child-block" in sys.argv: child_block()
    else: parent()
