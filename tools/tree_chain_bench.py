#!/usr/bin/env python3
"""A stretch of the chain in one call on one GPU (DESIGN.md "A stretch of the chain"); its output is profiles/tree_chain.txt.

    python tools/tree_chain_bench.py [--processes 5] [--calls 3] [--parent-lib OTHER/libzkgpu.so [--bench-reps 2]] [--set-proofs 8192] [--no-bench] [--keep DIR]

The protocol of tools/tree_block_bench.py, whose helpers it uses: fresh processes, everything warmed up by one untimed call, a device synchronise before every clock
read; a process reports the median of `calls` calls, the tables the median and p10-p90 of those over the processes.  Only the C calls are timed; the rewind that
puts the tree and the set back between two calls is not.  A setup process makes the keys (deposit at depth 20, send, mint) and the proofs once.
  1. The gate: segments of 64 and of 512 blocks of 128 records without a set.  The records are a rotation of 64 distinct proofs — 24 sends, 24 mints, 16 deposits,
     each deposit made against one of 16 states of the tree before the segment, which are the prior anchors; window 1,024 keeps them in reach of every block.
     verifyChainTree on this build against the loop of verifyBlockTree(commit = 1), one call a block with the anchors of its window, on the parent commit's library
     (--parent-lib, through ZKGPU_LIB; without it this build runs both roads).  Processes alternate.
  2. With a set: --set-proofs distinct mint proofs as blocks of 128, the same two roads.
  3. The compare alone: zkgpu_tree_match_roots_window with window 64 beside zkgpu_tree_match_roots on the same 8,192 RTs, against 64 and against 4,096 anchors;
     record i sits in "block" i * anchors / 8,192 and names an anchor of its own window, so both entries give the same answer.
  4. With --parent-lib: bench.py --gpus 1 --steps 50 --warmup 5 on this build and on the other library, alternating (the prover is not touched)."""
import ctypes, json, os, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from tree_block_bench import arg, bench_ab, pct
DEPTH, LEAVES, BLOCK, WINDOW, N = 20, 4096, 128, 1024, 8192
SEGMENTS = (64, 512)
PRIOR = [LEAVES - 16 * j for j in range(15, -1, -1)]                           # oldest first; the last one is the start of the segment
KINDS = ["send", "mint", "deposit", "send", "mint", "send", "mint", "deposit"] * 8   # the rotation: 24 sends, 24 mints, 16 deposits

def tree_leaves(cmts):
    blob = bytearray(np.random.default_rng(2031).integers(0, 256, 32 * LEAVES, dtype=np.uint8).tobytes())
    for j, c in enumerate(cmts): blob[32 * j:32 * j + 32] = bytes(c)[::-1]
    return bytes(blob)

def setup(d):
    from blockmaze_amd import engine as e
    import workload as w
    os.environ["ZK_PRFKEY_DIR"] = d; t0 = time.time(); nset = arg("--set-proofs", N)
    e.keygen("deposit", os.path.join(d, "deposit%dpk.txt" % DEPTH), os.path.join(d, "deposit%dvk.txt" % DEPTH), seed=20, tree_depth=DEPTH)
    for kind in ("send", "mint"): e.keygen(kind, os.path.join(d, kind + "pk.txt"), os.path.join(d, kind + "vk.txt"), seed=8)
    print("OUT setup: keys after %.0f s" % (time.time() - t0), flush=True); zk = e.Zk(); ds = [w.deposit_instance(700 + j) for j in range(16)]; t = zk.TreeNew(DEPTH)
    assert e.lib().zkgpu_tree_append(ctypes.c_void_p(t), tree_leaves([x["cmtS"] for x in ds]), ctypes.c_size_t(LEAVES)) == 0; items = []; count = {"send": 0, "mint": 0, "deposit": 0}
    def mint(i): x = w.mint_instance(i); return ("mint", zk.GenMintProof(*w.mint_args(x)), [x["cmtA_old"], x["sn_old"], x["cmtA"]], x["value_s"])
    for kind in KINDS:
        j = count[kind]; count[kind] += 1
        if kind == "send": x = w.send_instance(400 + j); items.append(("send", zk.GenSendProof(*w.send_args(x)), [x["cmtA_old"], x["sn_old"], x["cmtS"], x["cmtA"]], 0))
        elif kind == "mint": items.append(mint(400 + j))
        else:
            x = ds[j]; p, rt = zk.GenDepositProofTreeAt(*w.deposit_args(x), x["sk"], t, PRIOR[j]); a = [rt, x["pk_recv"], x["cmtB_old"], x["sn_old"], x["cmtB"], x["sn_s"]]
            assert rt is not None and zk.VerifyDepositProofDepth(DEPTH, p, *a); items.append(("deposit", p, a, 0))
    np.save(os.path.join(d, "unit.npy"), e.records_from_items(items)); json.dump({"cmts": [x["cmtS"].hex() for x in ds]}, open(os.path.join(d, "chain.json"), "w")); zk.TreeFree(t)
    print("OUT setup: the rotation of %d proofs after %.0f s" % (len(items), time.time() - t0), flush=True)
    np.save(os.path.join(d, "mints.npy"), e.records_from_items([mint(1000 + i) for i in range(nset)]))
    print("OUT setup: %d distinct mint proofs after %.0f s" % (nset, time.time() - t0), flush=True)

def child(d, road, result):
    """road "chain": verifyChainTree and the compare alone; road "loop": verifyBlockTree(commit = 1) block after block, as a library without the segment call is used"""
    from blockmaze_amd import engine as e
    os.environ["ZK_PRFKEY_DIR"] = d; CALLS = arg("--calls", 3); hip = ctypes.CDLL("libamdhip64.so"); e.init(); L = e.lib(); zk = e.Zk(); out = {}
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p); z = ctypes.c_size_t
    meta = json.load(open(os.path.join(d, "chain.json"))); unit = np.load(os.path.join(d, "unit.npy")); mints = np.load(os.path.join(d, "mints.npy")); stride = unit.dtype.itemsize
    tree = e.Tree(DEPTH); tree.append(tree_leaves([bytes.fromhex(c) for c in meta["cmts"]])); th = ctypes.c_void_p(tree.h); prior = np.array(PRIOR, dtype=np.int64); npri = len(PRIOR)
    sends = int((unit["kind"] == e.KIND["send"]).sum()) * (BLOCK // len(unit)); deposits = [i for i, k in enumerate(KINDS) if k == "deposit"]
    def segment(recs, nb, sh, grows):
        """-> ms of one decision of the segment; the tree and the set are put back afterwards, untimed"""
        n = len(recs); ptr = vp(recs); ok = (ctypes.c_ubyte * n)(); of = (ctypes.c_int32 * n)(); tsize = ctypes.c_longlong(0); set0 = zk.SnSetSize(sh.value) if sh else 0
        if road == "chain":
            first = np.arange(0, n + 1, BLOCK, dtype=np.int32); ts = np.zeros(nb, dtype=np.int64); t0 = now()
            rc = L.verifyChainTree(None, ptr, n, vp(first), nb, th, vp(prior), npri, WINDOW, sh, ok, of, None, vp(ts)); t1 = now()
            assert rc == nb and all(ok) and ts[-1] == LEAVES + grows * nb, (rc, ts[-1])
            if grows: assert [of[i] for i in deposits] == list(range(16)) and [of[n - len(KINDS) + i] for i in deposits] == list(range(16))
        else:
            A = np.zeros(npri + nb, dtype=np.int64); A[:npri] = prior; base = recs.ctypes.data; t0 = now()
            for b in range(nb):
                hi = npri + b; lo = max(0, hi - WINDOW)
                rc = L.verifyBlockTree(None, ctypes.c_void_p(base + b * BLOCK * stride), BLOCK, th, ctypes.c_void_p(A.ctypes.data + 8 * lo), hi - lo, sh, 1, ok, of, None, ctypes.byref(tsize)); A[hi] = tsize.value
                if rc != BLOCK: raise SystemExit("block %d: %d of %d records accepted" % (b, rc, BLOCK))
            t1 = now(); assert A[-1] == LEAVES + grows * nb
        assert zk.TreeRewind(tree.h, LEAVES) == LEAVES and (not sh or zk.SnSetRewind(sh.value, set0) == set0)
        return 1e3 * (t1 - t0)
    for nb in SEGMENTS:
        recs = np.ascontiguousarray(np.tile(unit, nb * BLOCK // len(unit))); out["seg_%d" % nb] = statistics.median([segment(recs, nb, None, sends) for i in range(CALLS + 1)][1:])
    s = zk.SnSetNew(); assert s and zk.SnSetSpend(s, [os.urandom(32) for _ in range(1 << 12)])[0] == 1 << 12; nb = len(mints) // BLOCK; recs = np.ascontiguousarray(mints[:nb * BLOCK])
    out["set"] = statistics.median([segment(recs, nb, ctypes.c_void_p(s), 0) for i in range(CALLS + 1)][1:]); out["set_blocks"] = nb; zk.SnSetFree(s)
    if road == "chain":                                                                              # 3. the compare alone
        for m in (64, 4096):
            sizes = np.array([LEAVES - j for j in range(m)], dtype=np.uint64); roots = np.zeros((m, 32), dtype=np.uint8); assert L.zkgpu_tree_roots_at(th, vp(sizes), z(m), vp(roots)) == 0
            i = np.arange(N); hi = np.minimum(m, 1 + i * m // N).astype(np.uint32); lo = np.maximum(0, hi.astype(np.int64) - 64).astype(np.uint32); at = np.maximum(lo.astype(np.int64), hi.astype(np.int64) - 1 - i % 64)
            rts = np.ascontiguousarray(roots[at]); a = np.zeros(N, dtype=np.int32); b = np.zeros(N, dtype=np.int32); ta, tb = [], []
            for k in range(5 * CALLS + 1):
                t0 = now(); r1 = L.zkgpu_tree_match_roots_window(th, vp(sizes), z(m), vp(rts), z(N), vp(lo), vp(hi), 0, vp(a)); t1 = now(); r2 = L.zkgpu_tree_match_roots(th, vp(sizes), z(m), vp(rts), z(N), 0, vp(b)); t2 = now()
                assert r1 == 0 and r2 == 0 and (a == at).all() and (b == at).all()
                if k: ta.append(1e3 * (t1 - t0)); tb.append(1e3 * (t2 - t1))
            out["window_%d" % m] = statistics.median(ta); out["full_%d" % m] = statistics.median(tb)
    tree.close(); json.dump(out, open(result, "w"))

def run(args, env=None):
    """a child process of this tool; its lines that begin with OUT are printed as they come"""
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, env=env)
    for line in p.stdout:
        if line.startswith("OUT "): print(line[4:], end="", flush=True)
    if p.wait() != 0: print("a child process failed:", args); sys.exit(1)

def parent():
    procs, calls, other = arg("--processes", 5), arg("--calls", 3), arg("--parent-lib", None, str); d = arg("--keep", None, str) or tempfile.mkdtemp(prefix="tree_chain")
    if not os.path.exists(os.path.join(d, "mints.npy")): run(["--setup", d, "--set-proofs", str(arg("--set-proofs", N))])
    runs = {"chain": [], "loop": []}
    for p in range(procs):
        for road in ("chain", "loop"):
            env = dict(os.environ); env.pop("ZKGPU_LIB", None); res = os.path.join(d, "result.json")
            if road == "loop" and other: env["ZKGPU_LIB"] = os.path.abspath(other)
            run(["--child", d, road, res, "--calls", str(calls)], env=env); runs[road].append(json.load(open(res))); print("   (process %d, %s: %s)" % (p, road, json.dumps(runs[road][-1])), flush=True)
    def col(road, key): v = [r[key] for r in runs[road]]; return pct(v, 0.5), pct(v, 0.1), pct(v, 0.9)
    who = "the parent's library" if other else "this build"; met = True
    print("wall time of the C calls, ms: median (p10-p90) over %d processes, each the median of %d calls" % (procs, calls))
    print("1. the gate: blocks of %d records, a rotation of 64 distinct proofs (24 sends, 24 mints, 16 deposits at depth %d), 16 prior anchors, window %d, no set" % (BLOCK, DEPTH, WINDOW))
    def row(name, key):
        (ma, la, ha), (mb, lb, hb) = col("chain", key), col("loop", key); gate = mb - ma > (ha - la) + (hb - lb)
        print("   %-28s verifyChainTree %9.3f (%9.3f-%9.3f) | verifyBlockTree(commit = 1) a block on %s %10.2f (%10.2f-%10.2f) | %6.1fx | %s"
              % (name, ma, la, ha, who, mb, lb, hb, mb / ma, "the gate is met: faster by more than both spreads" if gate else "THE GATE IS NOT MET"), flush=True); return gate
    for nb in SEGMENTS: met &= row("%d blocks, %d records:" % (nb, nb * BLOCK), "seg_%d" % nb)
    nb = runs["chain"][0]["set_blocks"]; print("2. with a set of 2^12 other keys: %d distinct mint proofs as %d blocks of %d" % (nb * BLOCK, nb, BLOCK)); row("%d blocks, %d records:" % (nb, nb * BLOCK), "set")
    print("3. the compare alone, %d RTs in block order, window 64: zkgpu_tree_match_roots_window beside zkgpu_tree_match_roots (both with zkgpu_tree_roots_at's launch)" % N)
    for m in (64, 4096):
        (ma, la, ha), (mb, lb, hb) = col("chain", "window_%d" % m), col("chain", "full_%d" % m)
        print("   %5d anchors: window %8.4f (%8.4f-%8.4f) | match_roots %8.4f (%8.4f-%8.4f) | the difference %+.4f ms" % (m, ma, la, ha, mb, lb, hb, ma - mb), flush=True)
    if "--no-bench" not in sys.argv: bench_ab(other)
    if not met: sys.exit(2)

if __name__ == "__main__":
    if "--setup" in sys.argv: setup(sys.argv[sys.argv.index("--setup") + 1])
    elif "--child" in sys.argv: i = sys.argv.index("--child"); child(sys.argv[i + 1], sys.argv[i + 2], sys.argv[i + 3])
    else: parent()
