#!/usr/bin/env python3
"""The account table on one GPU against the host loop it replaces (DESIGN.md "Account table"); its output is profiles/accounts.txt.

    python tools/accounts_bench.py [--processes 5] [--calls 5] [--parent-lib OTHER/libzkgpu.so [--bench-reps 2]] [--no-block] [--no-bench]

The protocol of tools/tree_block_bench.py: fresh processes, everything warmed up by one untimed call, a device synchronise before every clock read; a process reports
the median of `calls` calls, the tables the median and p10-p90 of those over the processes.  Only the C calls are timed; the rewinds between two calls are not.
  1. fill(chained = 1) + commit_chain against tools/accounts_host.cpp — the std::unordered_map loop of a node, one core of the same box —, the two alternating call
     by call, at n = 1, 8,192 and 65,536 on tables of 2^16 and 2^20 addresses; senders distinct, and 64 records a sender.  Every sender is resident.
  2. verifyBlockAccounts(commit = 1) on this build against the host loop + verifyBlockTree(commit = 1) on the parent commit's library (--parent-lib, through
     ZKGPU_LIB; without it this build runs both roads): one block of 128 distinct mint proofs of 128 senders, records arriving with zeroed old slots, a table of 2^16
     other addresses, a set of 2^12 other keys, a tree of depth 8.  Processes alternate.
  3. With --parent-lib: bench.py --gpus 1 --steps 50 --warmup 5 on this build and on the other library, alternating (the prover is not touched)."""
import ctypes, json, os, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from tree_block_bench import arg, bench_ab, pct
SIZES = (1, 8192, 65536); TABLES = (16, 20); BLOCK = 128
HOST_SO = os.path.join(ROOT, "tools", "accounts_host.so")

def host_lib():
    if not os.path.exists(HOST_SO): subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tools", "accounts_host.cpp"), "-o", HOST_SO])
    H = ctypes.CDLL(HOST_SO); H.accounts_host_new.restype = ctypes.c_void_p; H.accounts_host_size.restype = ctypes.c_uint64; return H
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p); z = ctypes.c_size_t

def child_table(lg, result):
    from blockmaze_amd import engine as e
    CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so"); e.init(); L = e.lib(); H = host_lib(); out = {}
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    rng = np.random.default_rng(1900 + lg); N = 1 << lg; addrs = rng.integers(0, 256, (N, 20), dtype=np.uint8); vals = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    t = e.AccountTable(); h = ctypes.c_void_p(t.h); hh = ctypes.c_void_p(H.accounts_host_new())
    for i in range(0, N, 65536): t.set(addrs[i:i + 65536], vals[i:i + 65536])
    H.accounts_host_set(hh, vp(addrs), vp(vals), z(N)); assert t.size() == N == H.accounts_host_size(hh)
    for n in SIZES:
        for mix in ("distinct", "64 a sender"):
            if mix != "distinct" and n < 64: continue
            who = rng.permutation(N)[:n] if mix == "distinct" else np.repeat(rng.permutation(N)[:n // 64], 64)[rng.permutation(n)]
            froms = np.ascontiguousarray(addrs[who]); base = np.zeros(n, dtype=e.RECORD_DTYPE); base["kind"] = rng.integers(0, 4, n); base["args"] = rng.integers(0, 256, (n, 6, 32), dtype=np.uint8)
            dev, host = [], []
            for call in range(CALLS + 1):
                a = base.copy(); b = base.copy()
                t0 = now(); rc = L.zkgpu_accts_fill(h, vp(froms), vp(a), z(n), 1) or L.zkgpu_accts_commit_chain(h, vp(froms), vp(a), z(n)); t1 = now(); assert rc == 0
                H.accounts_host_block(hh, vp(froms), vp(b), z(n)); t2 = time.perf_counter()
                assert a.tobytes() == b.tobytes() and t.size() == N + n == H.accounts_host_size(hh); t.rewind(N); H.accounts_host_rewind(hh, ctypes.c_uint64(N))
                if call: dev.append((t1 - t0) * 1e3); host.append((t2 - t1) * 1e3)
            out["%d|%s" % (n, mix)] = (statistics.median(dev), statistics.median(host))
    json.dump(out, open(result, "w"))

def setup_block(d):
    from blockmaze_amd import engine as e
    import workload as w
    os.environ["ZK_PRFKEY_DIR"] = d; e.keygen("mint", os.path.join(d, "mintpk.txt"), os.path.join(d, "mintvk.txt"), seed=8); zk = e.Zk(); items = []
    for i in range(BLOCK): x = w.mint_instance(3000 + i); items.append(("mint", zk.GenMintProof(*w.mint_args(x)), [x["cmtA_old"], x["sn_old"], x["cmtA"]], x["value_s"]))
    np.save(os.path.join(d, "block.npy"), e.records_from_items(items))

def child_block(d, road, result):
    """road "accounts": verifyBlockAccounts on records with zeroed old slots; road "loop": the host loop fills them, then verifyBlockTree — what a library without the table is used like"""
    from blockmaze_amd import engine as e
    os.environ["ZK_PRFKEY_DIR"] = d; CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so"); e.init(); L = e.lib(); zk = e.Zk(); H = host_lib()
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    full = np.load(os.path.join(d, "block.npy")); n = len(full); rng = np.random.default_rng(77); froms = rng.integers(0, 256, (n, 20), dtype=np.uint8); other = rng.integers(0, 256, (1 << 16, 20), dtype=np.uint8)
    olds = np.ascontiguousarray(full["args"][:, 0, :]); zeroed = full.copy(); zeroed["args"][:, 0, :] = 0
    s = e.SpentSet(bytes(20)); s.spend(rng.integers(0, 256, (1 << 12, 20), dtype=np.uint8)); s0 = s.size(); tree = e.Tree(8); th = ctypes.c_void_p(tree.h); anchors = np.zeros(1, dtype=np.int64)
    ok = (ctypes.c_ubyte * n)(); of = (ctypes.c_int32 * n)(); ss = ctypes.c_longlong(0); ts = ctypes.c_longlong(0); times = []
    if road == "accounts":
        t = e.AccountTable(); t.set(other, rng.integers(0, 256, (1 << 16, 32), dtype=np.uint8)); t.set(froms, olds); n0 = t.size(); asz = ctypes.c_longlong(0)
    else:
        hh = ctypes.c_void_p(H.accounts_host_new()); H.accounts_host_set(hh, vp(other), vp(rng.integers(0, 256, (1 << 16, 32), dtype=np.uint8)), z(1 << 16)); H.accounts_host_set(hh, vp(froms), vp(olds), z(n)); n0 = H.accounts_host_size(hh)
    for call in range(CALLS + 1):
        recs = zeroed.copy(); t0 = now()
        if road == "accounts": rc = L.verifyBlockAccounts(None, vp(recs), vp(froms), n, ctypes.c_void_p(t.h), th, vp(anchors), 1, ctypes.c_void_p(s.h), 1, ok, of, ctypes.byref(asz), ctypes.byref(ss), ctypes.byref(ts))
        else: H.accounts_host_block(hh, vp(froms), vp(recs), z(n)); rc = L.verifyBlockTree(None, vp(recs), n, th, vp(anchors), 1, ctypes.c_void_p(s.h), 1, ok, of, ctypes.byref(ss), ctypes.byref(ts))
        t1 = now(); assert rc == n and recs.tobytes() == full.tobytes(), rc
        s.rewind(s0)
        if road == "accounts": t.rewind(n0)
        else: H.accounts_host_rewind(hh, ctypes.c_uint64(n0))
        if call: times.append((t1 - t0) * 1e3)
    json.dump({"ms": statistics.median(times)}, open(result, "w"))

def run_child(args, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args + ["--calls", str(arg("--calls", 5))], capture_output=True, text=True, timeout=900, env=env or dict(os.environ))
    if r.returncode != 0: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)

def spread(v): return "%8.3f (%.3f-%.3f)" % (statistics.median(v), pct(v, 0.1), pct(v, 0.9))

def main():
    P = arg("--processes", 5); other = arg("--parent-lib", None, str); host_lib(); tmp = tempfile.mkdtemp()
    print("1. fill(chained = 1) + commit_chain on the device against the unordered_map loop on one host core, alternating; ms, median over %d processes (p10-p90), each the median of %d calls" % (P, arg("--calls", 5)))
    for lg in TABLES:
        runs = []
        for p in range(P): res = os.path.join(tmp, "t%d_%d.json" % (lg, p)); run_child(["--child-table", str(lg), res]); runs.append(json.load(open(res)))
        for k in runs[0]:
            n, mix = k.split("|"); dev = [r[k][0] for r in runs]; host = [r[k][1] for r in runs]; gap = abs(statistics.median(dev) - statistics.median(host)); both = (pct(dev, 0.9) - pct(dev, 0.1)) + (pct(host, 0.9) - pct(host, 0.1))
            print("   2^%d addresses  n = %6s  %-11s  device %s   host %s   %s" % (lg, n, mix, spread(dev), spread(host), ("device faster" if statistics.median(dev) < statistics.median(host) else "host faster") if gap > both else "no difference beyond the spreads"), flush=True)
    if "--no-block" not in sys.argv:
        print("2. one block of %d mint proofs, commit = 1: verifyBlockAccounts on this build against the host loop + verifyBlockTree on %s; ms" % (BLOCK, "the parent commit's library" if other else "this build"))
        d = tempfile.mkdtemp(); run_child(["--setup-block", d]); acc, loop = [], []
        for p in range(P):
            for road, into in (("accounts", acc), ("loop", loop)):
                env = dict(os.environ); env.pop("ZKGPU_LIB", None)
                if road == "loop" and other: env["ZKGPU_LIB"] = os.path.abspath(other)
                res = os.path.join(tmp, "b%s_%d.json" % (road, p)); run_child(["--child-block", d, road, res], env); into.append(json.load(open(res))["ms"])
        print("   verifyBlockAccounts %s   host loop + verifyBlockTree %s   added %+.3f ms (the two spreads together %.3f)" % (spread(acc), spread(loop), statistics.median(acc) - statistics.median(loop),
              (pct(acc, 0.9) - pct(acc, 0.1)) + (pct(loop, 0.9) - pct(loop, 0.1))), flush=True)
    if "--no-bench" not in sys.argv: bench_ab(other)

if __name__ == "__main__":
    if "--child-table" in sys.argv: i = sys.argv.index("--child-table"); child_table(int(sys.argv[i + 1]), sys.argv[i + 2])
    elif "--setup-block" in sys.argv: setup_block(sys.argv[sys.argv.index("--setup-block") + 1])
    elif "--child-block" in sys.argv: i = sys.argv.index("--child-block"); child_block(sys.argv[i + 1], sys.argv[i + 2], sys.argv[i + 3])
    else: main()
