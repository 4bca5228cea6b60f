"""Measurements of the resident commitment tree (DESIGN.md "Commitment tree") on one GPU; its output is profiles/commitment_tree.txt.

    python tools/tree_bench.py [--max-log 22] [--calls 200] [--no-proofs]

Every clock read comes after a device synchronise (hipDeviceSynchronize), every size is warmed up first.
  1. bulk build at depth 32, 2^10 .. 2^max-log leaves: a fresh tree and one append of all leaves, against the host model on the same leaves on the same box
     (zkgpu_test_tree_host = notes.cpp's tree_levels, the tree genRoot builds), the two alternating; and, from the library's HIP-event stages, the device time of the
     upload and of the append kernels inside that call;
  2. latency of a single-leaf append, of root and of path on a tree of 2^20 leaves;
  3. genDepositproofTree against genDepositproof at depth 8: the same instance, 256 leaves, `calls` calls each, interleaved;
  4. genDepositproofTree at depth 32 on a tree of 2^20 leaves, and the time of a find + path on that tree (the two kernels of the call's snapshot, with one download more)."""
import argparse, ctypes, os, random, statistics, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path: sys.path.insert(0, p)
from blockmaze_amd import engine as e
import workload as w

hip = ctypes.CDLL("libamdhip64.so")
def now():
    hip.hipDeviceSynchronize(); return time.perf_counter()
def stats(xs):
    xs = sorted(xs); q = lambda f: xs[min(len(xs) - 1, int(f * len(xs)))]
    return "median %9.3f  p10 %9.3f  p90 %9.3f  min %9.3f  max %9.3f" % (statistics.median(xs), q(0.1), q(0.9), xs[0], xs[-1])
def timed(fn):
    t0 = now(); r = fn(); return 1e3 * (now() - t0), r
def stages():
    rep = e.profile_report(); return {k: v["ms_total"] / max(1, v["count"]) for k, v in rep.items() if k.startswith("tree.")}

def bulk(max_log, reps):
    print("== bulk build, depth 32: a fresh tree and one append of n leaves (ms, medians), against the host model on the same leaves, alternating")
    print("(create / append: the two calls, timed one by one; upload, kernels: device time of the two stages inside append, by HIP events in a run of their own;")
    print(" other = append - upload - kernels: the allocation of the grown levels, launches, the closing synchronisation, the binding.  ratio = host model /")
    print(" (create + append).  bound by = the largest of upload, kernels, other + create.  first call = the first device call after the host model has run, a 32-byte")
    print(" root download from another tree, median and maximum: after a stretch of host work the next device call can take tens of ms, whatever that call is (seen")
    print(" after host-model runs of 25-400 ms, in rows that vary from run to run) - here this call takes it, outside the build's time.  The trees of a size are closed")
    print(" after its timed loop; close = one of those calls)")
    print("%8s %9s %9s | %9s %9s %9s %9s | %10s %8s | %9s %8s %8s   bound by" % ("leaves", "create", "append", "upload", "kernels", "other", "launches", "host model", "ratio", "close", "first", "(max)"))
    ping = e.Tree(8); ping.append(bytes(32))
    blob = random.Random(1).randbytes(32 << max_log)
    for lg in range(10, max_log + 1):
        n = 1 << lg; leaves = blob[:32 * n]; keep = []
        def dev():
            c, t = timed(lambda: e.Tree(32)); a, _ = timed(lambda: t.append(leaves)); keep.append(t); return c, a, t.launches(), t.root()
        def host(): return e.tree_host(32, leaves)[0]
        dev(); host()                                                                                  # warm-up of this size
        e.profile_enable(True); dev(); st = stages(); e.profile_enable(False)                          # a run of its own for the device-side stage times
        cs, as_, hs, ws = [], [], [], []
        for _ in range(reps if lg <= 18 else max(5, reps // 2)):
            h, r2 = timed(host); ws.append(timed(ping.root)[0]); c, a, k, r1 = dev(); assert r1 == r2; cs.append(c); as_.append(a); hs.append(h)
        x, _ = timed(keep.pop().close)
        for t in keep: t.close()
        c, a, h = (statistics.median(v) for v in (cs, as_, hs)); up, ke = st.get("tree.upload", 0.0), st.get("tree.append", 0.0); other = max(0.0, a - up - ke)
        bound = max((other + c, "allocation, launches, synchronisation"), (up, "upload"), (ke, "kernels"))[1]
        print("%8d %9.3f %9.3f | %9.3f %9.3f %9.3f %9d | %10.3f %7.1fx | %9.3f %8.3f %8.3f   %s" % (n, c, a, up, ke, other, k, h, h / (c + a), x, statistics.median(ws), max(ws), bound))
    print("(kernels, up to 2^17 leaves: 0.12-0.15 ms whatever the size - the time of the dependent chain of compressions from the last tile to the root, one lane, about")
    print(" 4 us a level; it is latency, not VALU throughput.  Upload: from pageable host memory.  Nothing here is bound by the launch count: two or three launches)")
    ping.close()

def latencies(calls):
    print("== latencies on a tree of 2^20 leaves, depth 32 (ms per call, %d calls each)" % calls)
    blob = random.Random(2).randbytes(32 << 20); t = e.Tree(32); t.append(blob); rng = random.Random(3)
    one = [rng.randbytes(32) for _ in range(calls + 20)]
    for x in one[:20]: t.append(x); t.root(); t.path(rng.randrange(1 << 20))                            # warm-up
    print("append of one leaf   " + stats([timed(lambda: t.append(x))[0] for x in one[20:]]))
    print("root                 " + stats([timed(t.root)[0] for _ in range(calls)]))
    print("path                 " + stats([timed(lambda: t.path(rng.randrange(1 << 20)))[0] for _ in range(calls)]))
    print("find (first quarter) " + stats([timed(lambda: t.find(blob[32 * i:32 * i + 32]))[0] for i in (rng.randrange(1 << 18) for _ in range(calls))]))
    return t, blob

def proofs(calls, big, blob):
    d = tempfile.mkdtemp(prefix="tree_bench_keys"); os.environ["ZK_PRFKEY_DIR"] = d; z = e.Zk()
    e.keygen("deposit", os.path.join(d, "depositpk.txt"), os.path.join(d, "depositvk.txt"), seed=8)
    di = w.deposit_instance(50, n_leaves=256); t = z.TreeNew(8); assert z.TreeAppend(t, di["leaves"]) == 256
    old = lambda: z.GenDepositProof(*w.deposit_args(di), di["leaves"], di["rt"], di["sk"]); new = lambda: z.GenDepositProofTree(*w.deposit_args(di), di["sk"], t)
    for _ in range(10): assert not old().startswith("0000000000"); assert new()[1] == di["rt"]
    a, b = [], []
    for _ in range(calls): a.append(timed(old)[0]); b.append(timed(new)[0])
    print("== depth 8, 256 leaves, the same instance, %d calls each, interleaved (ms per call, Python binding included on both sides)" % calls)
    print("genDepositproof      " + stats(a)); print("genDepositproofTree  " + stats(b))
    print("difference of medians %+.3f ms; run-to-run spread (p90 - p10): genDepositproof %.3f, genDepositproofTree %.3f" % (
        statistics.median(b) - statistics.median(a), sorted(a)[int(.9 * calls)] - sorted(a)[int(.1 * calls)], sorted(b)[int(.9 * calls)] - sorted(b)[int(.1 * calls)]))
    z.TreeFree(t)
    e.keygen("deposit", os.path.join(d, "deposit32pk.txt"), os.path.join(d, "deposit32vk.txt"), seed=32, tree_depth=32)
    di = w.deposit_instance(51, n_leaves=16); leaf = w.rev(di["cmtS"])
    big.append(leaf); t32 = ctypes.c_void_p(big.h)                                                     # the engine's tree handle is the drop-in's zk_tree
    new = lambda: z.GenDepositProofTree(*w.deposit_args(di), di["sk"], t32.value)
    p, rt = new(); assert rt is not None and z.VerifyDepositProofDepth(32, p, rt, di["pk_recv"], di["cmtB_old"], di["sn_old"], di["cmtB"], di["sn_s"])
    for _ in range(10): new()
    n = max(20, calls // 4); c = [timed(new)[0] for _ in range(n)]; idx = big.size() - 1
    s = [timed(lambda: (big.find(leaf), big.path(idx)))[0] for _ in range(n)]
    print("== depth 32, a tree of 2^20 + %d leaves, the leaf at the end (the longest scan), %d calls (ms per call)" % (big.size() - (1 << 20), n))
    print("genDepositproofTree  " + stats(c)); print("find + path          " + stats(s))
    print("share of the call taken by the tree: at most %.1f %% (find + path: the snapshot's two kernels, with one download more than the snapshot makes)" % (100 * statistics.median(s) / statistics.median(c)))
    print("(README quotes 2.9-3.5 ms a proof for the depth-32 engine path zkgpu_prover_prove, which starts from a finished assignment; this call also builds the assignment)")

if __name__ == "__main__":
    ap = argparse.ArgumentParser(); ap.add_argument("--max-log", type=int, default=22); ap.add_argument("--calls", type=int, default=200); ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--no-proofs", action="store_true"); a = ap.parse_args()
    e.init(); print("# tools/tree_bench.py on %s, %d visible device(s); times in ms, a device synchronise before every clock read" % (e.lib().zkgpu_version().decode(), e.device_count()))
    bulk(a.max_log, a.reps); big, blob = latencies(a.calls)
    if not a.no_proofs: proofs(a.calls, big, blob)
    big.close()
