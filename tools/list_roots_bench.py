#!/usr/bin/env python3
"""The roots of many commitment lists on the device against the host road (DESIGN.md "Roots of many lists"); its output is profiles/list_roots.txt.

    python tools/list_roots_bench.py [--processes 5] [--calls 5]

Fresh processes, every size warmed up, a device synchronise (hipDeviceSynchronize) before every clock read; a process reports the median of `calls` calls, the
table the median and p10-p90 of those over the processes.  Only the C calls are timed: the arrays, the hex strings and the records are built before the clock starts.
  a. genRoots over n lists of m commitments (one call, hash order, depth 8) against n genRoot calls on one thread on the same commitments, alternating;
     n = 64, 1,024 and 8,192, m = 256 and 16; and small n at m = 256 for the smallest n at which the one call is faster.
     Gate: at 8,192 x 256 genRoots is faster by more than the two p10-p90 spreads together.
  b. verifyBlockRecordsRoots on 8,192 deposit records with one list of 256 commitments each against verifyBlockRecords on the same records plus the 8,192
     genRoot calls; the same gate; and the added time split by the library's stages (range checks, plan = sorting into classes, upload, kernels, download, compare)."""
import ctypes, json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [(64, 256), (1024, 256), (8192, 256), (64, 16), (1024, 16), (8192, 16)]; SMALL = [1, 2, 4, 8, 16, 32]
STAGES = ("host.roots_ranges", "host.roots_plan", "roots.upload", "roots.kernels", "roots.download", "host.roots_compare")
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
def arg(name, default): return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

if "--child" not in sys.argv:
    procs, calls = arg("--processes", 5), arg("--calls", 5); runs = []
    for k in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(calls)], capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
        if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
        runs.append(json.loads(line[0][5:])); print("process %d done" % k, flush=True)
    def col(key): v = [r[key] for r in runs]; return pct(v, 0.5), pct(v, 0.1), pct(v, 0.9)
    def row(label, a, b):
        (ma, la, ha), (mb, lb, hb) = col(a), col(b); gate = mb - ma > (ha - la) + (hb - lb)
        print("%-28s | %9.3f (%9.3f-%9.3f) | %9.3f (%9.3f-%9.3f) | %7.1fx | %s" % (label, ma, la, ha, mb, lb, hb, mb / ma, "faster by more than both spreads" if gate else "NOT faster by more than both spreads")); return gate
    print("wall time of the C calls, ms: median (p10-p90) over %d processes, each the median of %d calls" % (procs, calls))
    print("a. %-25s | %-33s | %-33s | %8s |" % ("lists x commitments", "genRoots, one call", "genRoot, n calls on one thread", "ratio"))
    gates = {}
    for n, m in SIZES: gates[(n, m)] = row("%5d x %3d" % (n, m), "dev_%d_%d" % (n, m), "host_%d_%d" % (n, m))
    for n in SMALL: gates[(n, 256)] = row("%5d x 256" % n, "dev_%d_256" % n, "host_%d_256" % n)
    faster = [n for n in SMALL + [64, 1024, 8192] if col("dev_%d_256" % n)[0] < col("host_%d_256" % n)[0]]
    print("smallest n (of %s) at which one genRoots call over lists of 256 is faster than n genRoot calls: %s" % (SMALL + [64, 1024, 8192], faster[0] if faster else "none"))
    print("gate a (8,192 x 256): %s" % ("met" if gates[(8192, 256)] else "MISSED"))
    print("b. 8,192 deposit records, one list of 256 commitments each")
    gb = row("verifyBlockRecordsRoots", "block_roots", "block_plus_genroot"); print("   (right column: verifyBlockRecords + 8,192 genRoot calls; verifyBlockRecords alone: %.3f ms)" % col("block_plain")[0])
    print("gate b: %s" % ("met" if gb else "MISSED"))
    print("   added time of the root check by stage, ms (median over the processes; device stages by HIP events, host spans by the clock, one profiled call each):")
    print("   " + " | ".join("%s %.3f" % (s, pct([r["stages"].get(s, 0.0) for r in runs], 0.5)) for s in STAGES))
    sys.exit(0)

from blockmaze_amd import engine as e
import numpy as np
import workload as w
CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so"); libc = ctypes.CDLL(None); libc.free.argtypes = [ctypes.c_void_p]
def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
def alternate(fa, fb):
    fa(); fb(); ta, tb = [], []                                                                      # warm-up of this size
    for _ in range(CALLS):
        t0 = now(); fa(); t1 = now(); fb(); t2 = now(); ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1))
    return statistics.median(ta), statistics.median(tb)
e.init(); zk = e.Zk(); L = e.lib(); L.genRoot.restype = ctypes.c_void_p; L.genRoots.restype = ctypes.c_int; out = {}
rng = np.random.default_rng(1)
def roots_case(n, m):
    k = min(n, 64); block = rng.integers(0, 256, (k * m, 32), dtype=np.uint8); cmts = np.ascontiguousarray(np.tile(block, (n // k, 1)))   # (64 distinct lists, repeated: the strings are made once)
    lists = [(i * m, m) for i in range(n)]; l, keep = e._cmt_lists(cmts, lists); roots = np.zeros((n, 32), dtype=np.uint8); rp = e._bytes(roots)
    hexes = [b"".join(b"0x" + cmts[i].tobytes().hex().encode() for i in range(f, f + c)) for f, c in lists[:k]] * (n // k); last = []
    def dev(): assert L.genRoots(ctypes.byref(l), 8, rp) == 0
    def host():
        for h in hexes: p = L.genRoot(h, m); last[:] = [ctypes.string_at(p)]; libc.free(p)
    d, h = alternate(dev, host); assert roots[n - 1].tobytes().hex() == last[0].decode()
    out["dev_%d_%d" % (n, m)] = d; out["host_%d_%d" % (n, m)] = h
for n, m in SIZES: roots_case(n, m)
for n in SMALL: roots_case(n, 256)
# b. a block of deposit records
tmp = tempfile.mkdtemp(); os.environ["ZK_PRFKEY_DIR"] = tmp; e.keygen("deposit", os.path.join(tmp, "depositpk.txt"), os.path.join(tmp, "depositvk.txt"), seed=3)
x = w.deposit_instance(7, 256); pr = zk.GenDepositProof(*w.deposit_args(x), x["leaves"], x["rt"], x["sk"]); args = [x["rt"], x["pk_recv"], x["cmtB_old"], x["sn_old"], x["cmtB"], x["sn_s"]]
N = 8192; recs, ptr, _ = e._recs(e.records_from_items([("deposit", pr, args, 0)] * N)); one = np.frombuffer(b"".join(x["leaves"]), dtype=np.uint8).reshape(256, 32)
cmts = np.ascontiguousarray(np.tile(one, (N, 1))); lists = [(256 * i, 256) for i in range(N)]; l, keep = e._cmt_lists(cmts, lists); list_of = np.arange(N, dtype=np.int32); lp = list_of.ctypes.data_as(ctypes.c_void_p)
ok = (ctypes.c_ubyte * N)(); L.verifyBlockRecords.restype = ctypes.c_int; L.verifyBlockRecordsRoots.restype = ctypes.c_int; hexes = [b"".join(zk.hx(c) for c in x["leaves"])] * N
def with_roots(): assert L.verifyBlockRecordsRoots(ptr, N, ctypes.byref(l), lp, ok) == N
def plain(): assert L.verifyBlockRecords(ptr, N, ok) == N
def plain_and_genroot():
    plain()
    for h in hexes: libc.free(L.genRoot(h, 256))
out["block_roots"], out["block_plus_genroot"] = alternate(with_roots, plain_and_genroot); out["block_plain"], _ = alternate(plain, lambda: None)
e.profile_enable(True); with_roots(); rep = e.profile_report(); e.profile_enable(False); out["stages"] = {k: v["ms_total"] for k, v in rep.items() if k in STAGES}
print("JSON " + json.dumps(out), flush=True)
