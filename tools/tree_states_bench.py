#!/usr/bin/env python3
"""Past states of the resident commitment tree on one GPU (DESIGN.md "Past states of the commitment tree"); its output is profiles/tree_states.txt.

    python tools/tree_states_bench.py [--processes 5] [--calls 5] [--proof-calls 200] [--parent-lib OTHER/libzkgpu.so [--bench-reps 2] [--bench-only]]

The protocol of tools/list_roots_bench.py: fresh processes, every size warmed up, a device synchronise (hipDeviceSynchronize) before every clock read; a process
reports the median of `calls` calls, the tables the median and p10-p90 of those over the processes.  Only the C calls are timed: arrays are built before the clock starts.
  1. Rewind against what a caller does without it, on a depth-32 tree of 2^20 leaves: zkgpu_tree_rewind by 1 leaf, by 1,000 leaves and to 2^19 leaves, each
     against zkgpu_tree_create + ONE zkgpu_tree_append of the surviving leaves from host memory as bytes (the drop-in road, hex strings, costs more), alternating;
     between calls the rewound tree gets its leaves back and the rebuilt tree is destroyed, outside the clock.  Gate: the rewind is faster by more than the two
     p10-p90 spreads together at each of the three.
  2. Latencies on that tree: roots_at with 1, 64 and 8,192 random sizes, paths_at with 1 and 64 random leaves of a random size, find_at + paths_at of one leaf (the
     two kernels of snapshot_at, which has no entry of its own, with one download more), beside root, path and the append of one leaf.
  3. genDepositproofTreeAt against genDepositproofTree at depth 8, 256 leaves, `proof-calls` calls each, interleaved, one process; the past size is 201, whose
     edge walk is the longest a depth-8 tree has (eight compressions).
  4. With --parent-lib: bench.py --gpus 1 --steps 50 --warmup 5 on this build and on the other library (ZKGPU_LIB), alternating; proofs/s, median step, and the
     bytes of the last proof of each run compared."""
import ctypes, json, os, random, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
DEPTH, N = 32, 1 << 20; TARGETS = [("by 1 leaf", N - 1), ("by 1,000 leaves", N - 1000), ("to 2^19 leaves", N >> 1)]
LAT = ["roots_at_1", "roots_at_64", "roots_at_8192", "paths_at_1", "paths_at_64", "find_at+paths_at_1", "root", "path", "append_1"]
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
def arg(name, default, conv=int): return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

def parent():
    procs, calls = arg("--processes", 5), arg("--calls", 5); runs = []
    if "--bench-only" in sys.argv: return bench_ab()                                                  # (part 4 alone, for a session of its own)
    for k in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(calls)], capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
        if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
        runs.append(json.loads(line[0][5:])); print("process %d done" % k, flush=True)
    def col(key): v = [r[key] for r in runs]; return pct(v, 0.5), pct(v, 0.1), pct(v, 0.9)
    print("wall time of the C calls, ms: median (p10-p90) over %d processes, each the median of %d calls; depth %d, %d leaves" % (procs, calls, DEPTH, N))
    print("1. %-18s | %-30s | %-36s | %9s |" % ("rewind", "zkgpu_tree_rewind", "zkgpu_tree_create + one bulk append", "ratio")); ok = True
    for label, m in TARGETS:
        (ma, la, ha), (mb, lb, hb) = col("rewind_%d" % m), col("rebuild_%d" % m); gate = mb - ma > (ha - la) + (hb - lb); ok = ok and gate
        print("   %-18s | %8.4f (%8.4f-%8.4f) | %10.3f (%10.3f-%10.3f) | %8.1fx | %s" % (label, ma, la, ha, mb, lb, hb, mb / ma, "faster by more than both spreads" if gate else "NOT faster by more than both spreads"))
    print("gate 1: %s" % ("met at all three" if ok else "MISSED"))
    print("2. latencies on the same tree (sizes and indices drawn at random for every call)")
    for key in LAT: m, l, h = col("lat_" + key); print("   %-22s %8.4f (%8.4f-%8.4f)" % (key.replace("_", " "), m, l, h))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-proofs", "--proof-calls", str(arg("--proof-calls", 200))], capture_output=True, text=True, timeout=900)
    if r.returncode != 0: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
    print(r.stdout.rstrip(), flush=True)
    bench_ab()

def bench_ab():
    other = arg("--parent-lib", None, str)
    if other:
        print("4. bench.py --gpus 1 --steps 50 --warmup 5, this build and the parent commit's library (ZKGPU_LIB), alternating in one session:"); proofs = {}
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

def child():
    from blockmaze_amd import engine as e
    CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so"); e.init(); L = e.lib(); L.zkgpu_tree_create.restype = ctypes.c_void_p; out = {}
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    def med(fn, prep=lambda: None, after=lambda: None):
        ts = []
        for i in range(CALLS + 1):                                                                      # (the first call warms this size up)
            prep(); t0 = now(); fn(); t1 = now(); after(); ts.append(1e3 * (t1 - t0))
        return statistics.median(ts[1:])
    rng = random.Random(os.getpid()); blob = random.Random(1).randbytes(32 * N); t = e.Tree(DEPTH); t.append(blob); h = ctypes.c_void_p(t.h); full = t.root()
    # 1. rewind against create + bulk append
    for _, m in TARGETS:
        made = []; ta, tb = [], []
        def rewind(): assert L.zkgpu_tree_rewind(h, ctypes.c_uint64(m)) == 0
        def rebuild():
            u = L.zkgpu_tree_create(DEPTH); made.append(u); assert u and L.zkgpu_tree_append(ctypes.c_void_p(u), blob, ctypes.c_size_t(m)) == 0
        for i in range(CALLS + 1):
            t0 = now(); rewind(); t1 = now(); rebuild(); t2 = now()
            if i: ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1))
            else:
                r = ctypes.create_string_buffer(32); assert L.zkgpu_tree_root(ctypes.c_void_p(made[0]), r) == 0 and r.raw == t.root() == e.tree_host(DEPTH, blob[:32 * m])[0]
            L.zkgpu_tree_destroy(ctypes.c_void_p(made.pop())); t.append(blob[32 * m:]); assert t.size() == N
        assert t.root() == full; out["rewind_%d" % m] = statistics.median(ta); out["rebuild_%d" % m] = statistics.median(tb)
    # 2. latencies
    for q in (1, 64, 8192):
        box = {}
        def prep(): box["s"] = (ctypes.c_uint64 * q)(*[rng.randrange(N + 1) for _ in range(q)])
        buf = ctypes.create_string_buffer(32 * q); out["lat_roots_at_%d" % q] = med(lambda: L.zkgpu_tree_roots_at(h, box["s"], ctypes.c_size_t(q), buf), prep)
    for q in (1, 64):
        box = {}
        def prep(): m = rng.randrange(q, N + 1); box["m"] = ctypes.c_uint64(m); box["i"] = (ctypes.c_uint64 * q)(*[rng.randrange(m) for _ in range(q)])
        buf = ctypes.create_string_buffer(32 * q * DEPTH); root = ctypes.create_string_buffer(32)
        out["lat_paths_at_%d" % q] = med(lambda: L.zkgpu_tree_paths_at(h, box["m"], box["i"], ctypes.c_size_t(q), buf, root), prep)
    box = {}; idx = ctypes.c_uint64(0); buf = ctypes.create_string_buffer(32 * DEPTH); root = ctypes.create_string_buffer(32)
    def prep(): i = rng.randrange(N >> 2); box["leaf"] = blob[32 * i:32 * i + 32]; box["m"] = ctypes.c_uint64(rng.randrange(N >> 2, N + 1))   # (a leaf of the first quarter, as tools/tree_bench.py)
    def snap(): assert L.zkgpu_tree_find_at(h, box["m"], box["leaf"], ctypes.byref(idx)) == 0 and L.zkgpu_tree_paths_at(h, box["m"], ctypes.byref(idx), ctypes.c_size_t(1), buf, root) == 0
    out["lat_find_at+paths_at_1"] = med(snap, prep)
    out["lat_root"] = med(lambda: L.zkgpu_tree_root(h, root)); out["lat_path"] = med(lambda: L.zkgpu_tree_path(h, ctypes.c_uint64(rng.randrange(N)), buf))
    one = rng.randbytes(32); out["lat_append_1"] = med(lambda: L.zkgpu_tree_append(h, one, ctypes.c_size_t(1)), after=lambda: t.rewind(N))
    assert t.root() == full; t.close(); print("JSON " + json.dumps(out), flush=True)

def child_proofs():
    from blockmaze_amd import engine as e
    import workload as w
    calls = arg("--proof-calls", 200); hip = ctypes.CDLL("libamdhip64.so"); e.init()
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    d = tempfile.mkdtemp(prefix="tree_states_keys"); os.environ["ZK_PRFKEY_DIR"] = d; z = e.Zk(); e.keygen("deposit", os.path.join(d, "depositpk.txt"), os.path.join(d, "depositvk.txt"), seed=8)
    di = w.deposit_instance(50, n_leaves=256); lv = di["leaves"]; lv[di["index"]], lv[40] = lv[40], lv[di["index"]]; t = z.TreeNew(8); assert z.TreeAppend(t, lv) == 256
    cur = lambda: z.GenDepositProofTree(*w.deposit_args(di), di["sk"], t); past = lambda: z.GenDepositProofTreeAt(*w.deposit_args(di), di["sk"], t, 201)
    for _ in range(10): assert cur()[1] == z.GenRT(lv) and past()[1] == z.GenRT(lv[:201])
    a, b = [], []
    for _ in range(calls):
        t0 = now(); cur(); t1 = now(); past(); t2 = now(); a.append(1e3 * (t1 - t0)); b.append(1e3 * (t2 - t1))
    print("3. depth 8, 256 leaves, the same instance, %d calls each, interleaved, one process (ms per call, the Python binding included on both sides)" % calls)
    for name, v in (("genDepositproofTree", a), ("genDepositproofTreeAt(201)", b)): print("   %-27s median %.4f (p10 %.4f - p90 %.4f)" % (name, statistics.median(v), pct(v, 0.1), pct(v, 0.9)))
    print("   difference of the medians: %+.4f ms" % (statistics.median(b) - statistics.median(a))); z.TreeFree(t)

if __name__ == "__main__":
    if "--child" in sys.argv: child()
    elif "--child-proofs" in sys.argv: child_proofs()
    else: parent()
