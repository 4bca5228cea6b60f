#!/usr/bin/env python3
"""A block against the resident tree on one GPU (DESIGN.md "A block against the resident tree"); its output is profiles/tree_block.txt.

    python tools/tree_block_bench.py [--processes 5] [--calls 5] [--parent-lib OTHER/libzkgpu.so [--bench-reps 2]] [--no-gate] [--no-loop] [--keep DIR]

The protocol of tools/list_roots_bench.py: fresh processes, every size warmed up, a device synchronise (hipDeviceSynchronize) before every clock read; a process
reports the median of `calls` calls, the tables the median and p10-p90 of those over the processes.  Only the C calls are timed.  A setup process makes the keys
(deposit at depth 32, send) and 64 proofs of each kind once; every timed process builds the same tree of 2^20 seeded leaves from them.
  1. The gate: 8,192 deposit records at depth 32 (64 distinct proofs in rotation, each made against the tree's state at one of 64 anchors), a set of 2^16 other keys,
     commit = 0.  verifyBlockTree on this build against what the parent commit's library (--parent-lib, through ZKGPU_LIB; without it this build runs both roads) can
     do for the same block: a loop of verifyDepositproofDepth(32, ...), one zkTreeRootsAt, the compare on the host, zkSnSetSpendPairs.  Processes alternate.
  2. The anchor step alone: zkgpu_tree_match_roots for 8,192 RTs against 64 and against 4,096 anchors, beside zkgpu_tree_roots_at of the same sizes.
  3. verifyBlockTree at depth 8 (an empty tree, one anchor) against verifyBlockState on the same send-only block of 8,192 records, alternating.
     --no-loop leaves the proof-by-proof processes out: tables 2 and 3 and this build's side of table 1 alone.
  4. With --parent-lib: bench.py --gpus 1 --steps 50 --warmup 5 on this build and on the other library, alternating; proofs/s, median step, the last proof's bytes."""
import ctypes, json, os, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
N, DISTINCT, LEAVES, DEPTH = 8192, 64, 1 << 20, 32
ANCHORS = [LEAVES - 4096 * j for j in range(DISTINCT)]                       # the tree's sizes after its last 64 "blocks"; proof j is made against anchor j
MANY = [LEAVES - 17 * j for j in range(4096)]
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
def arg(name, default, conv=int): return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

def tree_leaves(cmts):
    """2^20 seeded leaves in blob order, the 64 notes' commitments in front"""
    blob = bytearray(np.random.default_rng(2030).integers(0, 256, 32 * LEAVES, dtype=np.uint8).tobytes())
    for j, c in enumerate(cmts): blob[32 * j:32 * j + 32] = bytes(c)[::-1]
    return bytes(blob)

def setup(d):
    from blockmaze_amd import engine as e
    import workload as w
    os.environ["ZK_PRFKEY_DIR"] = d; t0 = time.time()
    e.keygen("deposit", os.path.join(d, "deposit32pk.txt"), os.path.join(d, "deposit32vk.txt"), seed=32, tree_depth=DEPTH); e.keygen("send", os.path.join(d, "sendpk.txt"), os.path.join(d, "sendvk.txt"), seed=8)
    print("OUT setup: keys after %.0f s" % (time.time() - t0), flush=True); zk = e.Zk(); ds = [w.deposit_instance(500 + j) for j in range(DISTINCT)]; t = zk.TreeNew(DEPTH)
    leaves = tree_leaves([x["cmtS"] for x in ds]); assert e.lib().zkgpu_tree_append(ctypes.c_void_p(t), leaves, ctypes.c_size_t(LEAVES)) == 0; dep = []; strings = []
    for j, x in enumerate(ds):
        p, rt = zk.GenDepositProofTreeAt(*w.deposit_args(x), x["sk"], t, ANCHORS[j]); a = [rt, x["pk_recv"], x["cmtB_old"], x["sn_old"], x["cmtB"], x["sn_s"]]
        assert rt is not None and zk.VerifyDepositProofDepth(DEPTH, p, *a); dep.append(("deposit", p, a, 0)); strings.append([p] + [zk.hx(v).decode() for v in a])
    snd = []
    for i in range(DISTINCT): x = w.send_instance(300 + i); snd.append(("send", zk.GenSendProof(*w.send_args(x)), [x["cmtA_old"], x["sn_old"], x["cmtS"], x["cmtA"]], 0))
    np.save(os.path.join(d, "deposit.npy"), e.records_from_items(dep)); np.save(os.path.join(d, "send.npy"), e.records_from_items(snd))
    json.dump({"strings": strings, "cmts": [x["cmtS"].hex() for x in ds]}, open(os.path.join(d, "deposit.json"), "w")); zk.TreeFree(t)
    print("OUT setup: %d deposit proofs at depth %d and %d send proofs after %.0f s" % (DISTINCT, DEPTH, DISTINCT, time.time() - t0), flush=True)

def child(d, road, result):
    """road "tree": verifyBlockTree, the anchor step alone and the depth-8 comparison; road "loop": what a library without verifyBlockTree does for the gate's block"""
    from blockmaze_amd import engine as e
    os.environ["ZK_PRFKEY_DIR"] = d; CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so"); e.init(); L = e.lib(); zk = e.Zk(); out = {}
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    meta = json.load(open(os.path.join(d, "deposit.json"))); unit = np.load(os.path.join(d, "deposit.npy")); recs = np.ascontiguousarray(np.tile(unit, N // DISTINCT)); ptr = recs.ctypes.data_as(ctypes.c_void_p)
    tree = e.Tree(DEPTH); tree.append(tree_leaves([bytes.fromhex(c) for c in meta["cmts"]])); th = ctypes.c_void_p(tree.h); s = zk.SnSetNew(); assert s and zk.SnSetSpend(s, [os.urandom(32) for _ in range(1 << 16)])[0] == 1 << 16
    sh = ctypes.c_void_p(s); an = np.array(ANCHORS, dtype=np.int64); ok = (ctypes.c_ubyte * N)(); of = (ctypes.c_int32 * N)(); size = ctypes.c_longlong(0); tsize = ctypes.c_longlong(0)
    L.zkSnSetSpendPairs.restype = ctypes.c_longlong
    if road == "tree":
        ts = []
        for i in range(CALLS + 1):
            t0 = now(); rc = L.verifyBlockTree(None, ptr, N, th, an.ctypes.data_as(ctypes.c_void_p), DISTINCT, sh, 0, ok, of, ctypes.byref(size), ctypes.byref(tsize)); t1 = now()
            assert rc == DISTINCT and list(of)[:DISTINCT] == list(range(DISTINCT)) and list(ok)[:DISTINCT] == [1] * DISTINCT and not any(list(ok)[DISTINCT:]) and (size.value, tsize.value) == (1 << 16, LEAVES)
            if i: ts.append(1e3 * (t1 - t0))
        out["gate"] = statistics.median(ts)
        # 2. the anchor step alone
        rts = np.ascontiguousarray(recs["args"][:, 0, :]); match = np.zeros(N, dtype=np.int32); roots = np.zeros((4096, 32), dtype=np.uint8); z = ctypes.c_size_t; vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for name, sizes in (("64", ANCHORS), ("4096", MANY)):
            m = np.array(sizes, dtype=np.uint64); ta, tb = [], []
            for i in range(CALLS + 1):
                t0 = now(); r1 = L.zkgpu_tree_match_roots(th, vp(m), z(len(m)), vp(rts), z(N), 1, vp(match)); t1 = now(); r2 = L.zkgpu_tree_roots_at(th, vp(m), z(len(m)), vp(roots)); t2 = now()
                assert r1 == 0 and r2 == 0 and match[0] == 0 and (match[1:DISTINCT] == (np.arange(1, DISTINCT) if name == "64" else -1)).all()   # (the 4,096 sizes share the current size with the 64 and nothing else)
                if i: ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1))
            out["match_" + name] = statistics.median(ta); out["roots_" + name] = statistics.median(tb)
        # 3. depth 8 against verifyBlockState, a send-only block
        srecs = np.ascontiguousarray(np.tile(np.load(os.path.join(d, "send.npy")), N // DISTINCT)); sp = srecs.ctypes.data_as(ctypes.c_void_p); t8 = e.Tree(8); zero = np.zeros(1, dtype=np.int64); ta, tb = [], []
        for i in range(CALLS + 1):
            t0 = now(); r1 = L.verifyBlockTree(None, sp, N, ctypes.c_void_p(t8.h), zero.ctypes.data_as(ctypes.c_void_p), 1, sh, 0, ok, of, ctypes.byref(size), ctypes.byref(tsize)); t1 = now()
            r2 = L.verifyBlockState(None, sp, N, None, None, sh, 0, ok, ctypes.byref(size)); t2 = now(); assert r1 == r2 == DISTINCT and tsize.value == 0
            if i: ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1))
        out["tree8"] = statistics.median(ta); out["state8"] = statistics.median(tb)
    else:
        # one proof a call, as a node without a block entry for the tree verifies; the library prints a line a proof, which goes to /dev/null
        L.verifyDepositproofDepth.restype = ctypes.c_bool; calls = [[x.encode() for x in row] for row in meta["strings"]]; roots = np.zeros((DISTINCT, 32), dtype=np.uint8); spent = (ctypes.c_ubyte * N)()
        sns = np.ascontiguousarray(recs["args"][:, 3, :]); pks = np.zeros((N, 32), dtype=np.uint8); pks[:, 12:] = recs["args"][:, 1, :20]; rts = recs["args"][:, 0, :]
        sys.stdout.flush(); keep = os.dup(1); null = os.open(os.devnull, os.O_WRONLY); os.dup2(null, 1); ts = []
        for i in range(CALLS + 1):
            t0 = now(); good = np.zeros(N, dtype=bool)
            for k in range(N): good[k] = L.verifyDepositproofDepth(DEPTH, *calls[k % DISTINCT])
            assert L.zkTreeRootsAt(th, an.ctypes.data_as(ctypes.c_void_p), DISTINCT, roots.ctypes.data_as(ctypes.c_void_p)) == 0
            known = set(r.tobytes() for r in roots); good &= np.array([r.tobytes() in known for r in rts])
            assert good.all()                                                                                                        # (a caller would leave a rejected record out of the pairs call)
            after = L.zkSnSetSpendPairs(sh, sns.ctypes.data_as(ctypes.c_void_p), pks.ctypes.data_as(ctypes.c_void_p), N, 0, spent); t1 = now()
            assert after == 1 << 16 and list(spent)[:DISTINCT] == [0] * DISTINCT and all(list(spent)[DISTINCT:])
            if i: ts.append(1e3 * (t1 - t0))
        os.dup2(keep, 1); os.close(keep); os.close(null); out["loop"] = statistics.median(ts)
    zk.SnSetFree(s); tree.close(); json.dump(out, open(result, "w"))

def run(args, env=None):
    """a child process; its lines that begin with OUT are printed as they come (the library's own progress lines stay out of the table)"""
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, env=env)
    for line in p.stdout:
        if line.startswith("OUT "): print(line[4:], end="", flush=True)
    if p.wait() != 0: print("a child process failed:", args); sys.exit(1)

def parent():
    procs, calls, other = arg("--processes", 5), arg("--calls", 5), arg("--parent-lib", None, str); d = arg("--keep", None, str) or tempfile.mkdtemp(prefix="tree_block")
    runs = {"tree": [], "loop": []}
    if "--no-gate" not in sys.argv:
        if not os.path.exists(os.path.join(d, "deposit.json")): run(["--setup", d])
        for p in range(procs):
            for road in (("tree",) if "--no-loop" in sys.argv else ("tree", "loop")):
                env = dict(os.environ); env.pop("ZKGPU_LIB", None); res = os.path.join(d, "result.json")
                if road == "loop" and other: env["ZKGPU_LIB"] = os.path.abspath(other)
                run(["--child", d, road, res, "--calls", str(calls)], env=env); runs[road].append(json.load(open(res))); print("   (process %d, %s: %s)" % (p, road, json.dumps(runs[road][-1])), flush=True)
        def col(road, key): v = [r[key] for r in runs[road]]; return pct(v, 0.5), pct(v, 0.1), pct(v, 0.9)
        print("wall time of the C calls, ms: median (p10-p90) over %d processes, each the median of %d calls" % (procs, calls))
        (ma, la, ha) = col("tree", "gate"); (mb, lb, hb) = col("loop", "loop") if runs["loop"] else (float("nan"),) * 3; gate = mb - ma > (ha - la) + (hb - lb)
        print("1. the gate: %d deposit records at depth %d, %d distinct proofs, %d anchors, a tree of 2^20 leaves, a set of 2^16 keys, commit = 0" % (N, DEPTH, DISTINCT, DISTINCT))
        print("   verifyBlockTree %9.3f (%9.3f-%9.3f) | verifyDepositproofDepth x %d + zkTreeRootsAt + compare + zkSnSetSpendPairs on %s %10.2f (%10.2f-%10.2f) | %7.1fx | %s"
              % (ma, la, ha, N, "the parent's library" if other else "this build", mb, lb, hb, mb / ma, "the gate is met: faster by more than both spreads" if gate else "the loop was not run" if not runs["loop"] else "THE GATE IS NOT MET"))
        print("2. the anchor step alone, %d RTs: zkgpu_tree_match_roots beside zkgpu_tree_roots_at of the same sizes" % N)
        for name in ("64", "4096"):
            (ma, la, ha), (mb, lb, hb) = col("tree", "match_" + name), col("tree", "roots_" + name)
            print("   %5s anchors: match_roots %8.4f (%8.4f-%8.4f) | roots_at %8.4f (%8.4f-%8.4f) | the difference %+.4f ms" % (name, ma, la, ha, mb, lb, hb, ma - mb))
        (ma, la, ha), (mb, lb, hb) = col("tree", "tree8"), col("tree", "state8")
        print("3. a send-only block of %d records: verifyBlockTree at depth 8 %8.3f (%8.3f-%8.3f) | verifyBlockState %8.3f (%8.3f-%8.3f) | the difference %+.3f ms" % (N, ma, la, ha, mb, lb, hb, ma - mb), flush=True)
    if "--no-loop" not in sys.argv: bench_ab(other)

def bench_ab(other):
    if not other: return
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

if __name__ == "__main__":
    if "--setup" in sys.argv: setup(sys.argv[sys.argv.index("--setup") + 1])
    elif "--child" in sys.argv: i = sys.argv.index("--child"); child(sys.argv[i + 1], sys.argv[i + 2], sys.argv[i + 3])
    else: parent()
