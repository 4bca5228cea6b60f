#!/usr/bin/env python3
"""A stretch of the chain with accounts on one GPU (DESIGN.md "A stretch of the chain with accounts"); its output is profiles/accounts_chain.txt.

    python tools/accounts_chain_bench.py [--processes 5] [--calls 5] [--parent-lib OTHER/libzkgpu.so [--bench-reps 2]] [--no-chain] [--no-table] [--no-bench] [--keep DIR]

The protocol of tools/tree_block_bench.py, whose helpers it uses: fresh processes, everything warmed up by one untimed call, a device synchronise before every clock
read; a process reports the median of `calls` calls, the tables the median and p10-p90 of those over the processes.  Only the C calls are timed; the rewinds that put
the table, the set and the tree back between two calls are not.
  a. verifyChainAccounts on this build on a segment of 64 blocks x 128 distinct valid mint proofs, every record from a sender of its own, the records arriving with
     zeroed old slots, against the loop of verifyBlockAccounts(commit = 1), one call a block, on the parent commit's library (--parent-lib, through ZKGPU_LIB; without
     it this build runs both roads).  A table of 2^16 other addresses, a set of 2^12 other keys, a tree of depth 8, window 8.  Processes alternate.
  b. fill_segment + commit_segment against fill(chained = 1) + commit_chain on one table of 2^16 addresses, alternating in the order segment, older, older, segment, at 8,192 and 65,536 records with
     distinct senders, 64 records a sender and 4,096 records a sender; every sender is resident.  The last mix takes the host finish on the older road.
  c. With --parent-lib: bench.py --gpus 1 --steps 50 --warmup 5 on this build and on the other library, alternating (the prover is not touched).
One side is called faster only where the medians differ by more than the two p10-p90 spreads together."""
import ctypes, json, os, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from tree_block_bench import arg, bench_ab, pct
BLOCKS, BLOCK, WINDOW, TABLE_LOG = 64, 128, 8, 16
SIZES = (8192, 65536); MIXES = (("distinct", 1), ("64 a sender", 64), ("4,096 a sender", 4096))
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p); z = ctypes.c_size_t

def setup(d):
    from blockmaze_amd import engine as e
    import workload as w
    os.environ["ZK_PRFKEY_DIR"] = d; t0 = time.time(); e.keygen("mint", os.path.join(d, "mintpk.txt"), os.path.join(d, "mintvk.txt"), seed=8); zk = e.Zk(); items = []
    for i in range(BLOCKS * BLOCK): x = w.mint_instance(5000 + i); items.append(("mint", zk.GenMintProof(*w.mint_args(x)), [x["cmtA_old"], x["sn_old"], x["cmtA"]], x["value_s"]))
    np.save(os.path.join(d, "segment.npy"), e.records_from_items(items)); print("OUT setup: %d distinct mint proofs after %.0f s" % (len(items), time.time() - t0), flush=True)

def child_chain(d, road, result):
    """road "chain": verifyChainAccounts; road "loop": verifyBlockAccounts(commit = 1) block after block, as a library without the segment call is used"""
    from blockmaze_amd import engine as e
    os.environ["ZK_PRFKEY_DIR"] = d; CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so"); e.init(); L = e.lib(); zk = e.Zk()
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    full = np.load(os.path.join(d, "segment.npy")); n = len(full); nb = n // BLOCK; stride = full.dtype.itemsize; rng = np.random.default_rng(78)
    froms = rng.integers(0, 256, (n, 20), dtype=np.uint8); other = rng.integers(0, 256, (1 << TABLE_LOG, 20), dtype=np.uint8); olds = np.ascontiguousarray(full["args"][:, 0, :]); zeroed = full.copy(); zeroed["args"][:, 0, :] = 0
    s = e.SpentSet(bytes(20)); s.spend(rng.integers(0, 256, (1 << 12, 20), dtype=np.uint8)); s0 = s.size(); tree = e.Tree(8); th = ctypes.c_void_p(tree.h); sh = ctypes.c_void_p(s.h)
    t = e.AccountTable(); t.set(other, rng.integers(0, 256, (1 << TABLE_LOG, 32), dtype=np.uint8)); t.set(froms, olds); n0 = t.size(); ah = ctypes.c_void_p(t.h)
    ok = (ctypes.c_ubyte * n)(); of = (ctypes.c_int32 * n)(); prior = np.zeros(1, dtype=np.int64); first = np.arange(0, n + 1, BLOCK, dtype=np.int32); times = []
    for call in range(CALLS + 1):
        recs = zeroed.copy(); base = recs.ctypes.data
        if road == "chain":
            sizes = [np.zeros(nb, dtype=np.int64) for _ in range(3)]; t0 = now()
            rc = L.verifyChainAccounts(None, vp(recs), vp(froms), n, vp(first), nb, ah, th, vp(prior), 1, WINDOW, sh, ok, of, vp(sizes[0]), vp(sizes[1]), vp(sizes[2])); t1 = now()
            assert rc == nb and sizes[0][-1] == n0 + n and sizes[1][-1] == s0 + n, (rc, sizes[0][-1], sizes[1][-1])
        else:
            A = np.zeros(1 + nb, dtype=np.int64); asz = ctypes.c_longlong(0); ssz = ctypes.c_longlong(0); tsz = ctypes.c_longlong(0); t0 = now()
            for b in range(nb):
                hi = 1 + b; lo = max(0, hi - WINDOW)
                rc = L.verifyBlockAccounts(None, ctypes.c_void_p(base + b * BLOCK * stride), ctypes.c_void_p(froms.ctypes.data + 20 * b * BLOCK), BLOCK, ah, th, ctypes.c_void_p(A.ctypes.data + 8 * lo), hi - lo, sh, 1, ok, of,
                                           ctypes.byref(asz), ctypes.byref(ssz), ctypes.byref(tsz)); A[hi] = tsz.value
                if rc != BLOCK: raise SystemExit("block %d: %d of %d records accepted" % (b, rc, BLOCK))
            t1 = now(); assert asz.value == n0 + n and ssz.value == s0 + n
        assert recs.tobytes() == full.tobytes(); t.rewind(n0); s.rewind(s0)
        if call: times.append(1e3 * (t1 - t0))
    json.dump({"ms": statistics.median(times)}, open(result, "w"))

def child_table(result):
    from blockmaze_amd import engine as e
    CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so"); e.init(); L = e.lib(); out = {}
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    rng = np.random.default_rng(1950); N = 1 << TABLE_LOG; addrs = rng.integers(0, 256, (N, 20), dtype=np.uint8); vals = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    t = e.AccountTable(); h = ctypes.c_void_p(t.h); t.set(addrs, vals); assert t.size() == N
    for n in SIZES:
        for mix, per in MIXES:
            who = np.repeat(rng.permutation(N)[:n // per], per)[rng.permutation(n)]; froms = np.ascontiguousarray(addrs[who])
            base = np.zeros(n, dtype=e.RECORD_DTYPE); base["kind"] = rng.integers(0, 4, n); base["args"] = rng.integers(0, 256, (n, 6, 32), dtype=np.uint8); seg, old = [], []; h0 = e.accts_launches()[1]
            def seg_road(r): rc = L.zkgpu_accts_fill_segment(h, vp(froms), vp(r), z(n)) or L.zkgpu_accts_commit_segment(h, vp(froms), vp(r), z(n)); return rc
            def old_road(r): rc = L.zkgpu_accts_fill(h, vp(froms), vp(r), z(n), 1) or L.zkgpu_accts_commit_chain(h, vp(froms), vp(r), z(n)); return rc
            for call in range(CALLS + 1):                                                           # a round: segment, older, older, segment — neither road is always the first after the copies
                got = []
                for road, into in ((seg_road, seg), (old_road, old), (old_road, old), (seg_road, seg)):
                    r = base.copy(); t0 = now(); rc = road(r); t1 = now(); assert rc == 0 and t.size() == N + n; got.append((r.tobytes(), t.read_log(N, 64))); t.rewind(N)
                    if call: into.append(1e3 * (t1 - t0))
                assert all(g == got[0] for g in got)
            out["%d|%s" % (n, mix)] = (statistics.median(seg), statistics.median(old), (e.accts_launches()[1] - h0) // (2 * (CALLS + 1)))
    json.dump(out, open(result, "w"))

def run(args, env=None):
    """a child process of this tool; its lines that begin with OUT are printed as they come"""
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + args + ["--calls", str(arg("--calls", 5))], stdout=subprocess.PIPE, text=True, env=env)
    for line in p.stdout:
        if line.startswith("OUT "): print(line[4:], end="", flush=True)
    if p.wait() != 0: print("a child process failed:", args); sys.exit(1)

def spread(v): return "%9.3f (%9.3f-%9.3f)" % (pct(v, 0.5), pct(v, 0.1), pct(v, 0.9))
def verdict(a, b, name_a, name_b):
    gap = abs(pct(a, 0.5) - pct(b, 0.5)); both = (pct(a, 0.9) - pct(a, 0.1)) + (pct(b, 0.9) - pct(b, 0.1))
    return "no difference beyond the spreads" if gap <= both else "%s faster, %.2fx" % ((name_a, pct(b, 0.5) / pct(a, 0.5)) if pct(a, 0.5) < pct(b, 0.5) else (name_b, pct(a, 0.5) / pct(b, 0.5)))

def main():
    P = arg("--processes", 5); other = arg("--parent-lib", None, str); d = arg("--keep", None, str) or tempfile.mkdtemp(prefix="accounts_chain"); res = os.path.join(d, "result.json")
    print("wall time of the C calls, ms: median (p10-p90) over %d processes, each the median of %d calls" % (P, arg("--calls", 5)))
    if "--no-chain" not in sys.argv:
        if not os.path.exists(os.path.join(d, "segment.npy")): run(["--setup", d])
        print("a. %d blocks x %d distinct mint proofs, each from a sender of its own, zeroed old slots; a table of 2^%d other addresses, a set of 2^12 other keys, a tree of depth 8" % (BLOCKS, BLOCK, TABLE_LOG))
        chain, loop = [], []
        for p in range(P):
            for road, into in (("chain", chain), ("loop", loop)):
                env = dict(os.environ); env.pop("ZKGPU_LIB", None)
                if road == "loop" and other: env["ZKGPU_LIB"] = os.path.abspath(other)
                run(["--child-chain", d, road, res], env); into.append(json.load(open(res))["ms"])
        print("   verifyChainAccounts %s | verifyBlockAccounts(commit = 1) a block on %s %s | %s" % (spread(chain), "the parent's library" if other else "this build", spread(loop), verdict(chain, loop, "the segment call", "the loop")), flush=True)
    if "--no-table" not in sys.argv:
        print("b. fill_segment + commit_segment (the tiled search) against fill(chained = 1) + commit_chain on one table of 2^%d addresses, every sender resident; a round is segment, older, older, segment, so a process reports the median of %d calls a road" % (TABLE_LOG, 2 * arg("--calls", 5))); runs = []
        for p in range(P): run(["--child-table", res]); runs.append(json.load(open(res)))
        for k in runs[0]:
            n, mix = k.split("|"); seg = [r[k][0] for r in runs]; old = [r[k][1] for r in runs]
            print("   n = %6s  %-15s  segment road %s | older road %s, %d host finishes a pair of calls | %s" % (n, mix, spread(seg), spread(old), runs[0][k][2], verdict(seg, old, "the segment road", "the older road")), flush=True)
    if "--no-bench" not in sys.argv and other: print("c. the prover beside it:"); bench_ab(other)

if __name__ == "__main__":
    if "--setup" in sys.argv: setup(sys.argv[sys.argv.index("--setup") + 1])
    elif "--child-chain" in sys.argv: i = sys.argv.index("--child-chain"); child_chain(sys.argv[i + 1], sys.argv[i + 2], sys.argv[i + 3])
    elif "--child-table" in sys.argv: child_table(sys.argv[sys.argv.index("--child-table") + 1])
    else: main()
