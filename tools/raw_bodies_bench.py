#!/usr/bin/env python3
"""zkBodySplit alone, and verifyChainRawBodies beside verifyChainBodiesRoots; its output is the tables of profiles/raw_bodies.txt.

    python tools/raw_bodies_bench.py [--processes 5] [--calls 5]
    python tools/raw_bodies_bench.py --chain [--blocks 64] [--block 128] [--processes 5] [--calls 5] [--parent-lib OTHER/libzkgpu.so] [--keep DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/raw_bodies_bench.py --child raw --calls 1 --dir DIR    # the kernels' shares: a warm-up call and one call
    python tools/raw_bodies_bench.py --summarize KERNEL_STATS.csv

DESIGN.md §12's protocol, as tools/tx_roots_bench.py applies it: fresh processes, every shape warmed up by one call, a device synchronise before every clock read; a
process reports the median of `calls` calls, the table the median and p10-p90 of those over the processes.  Only the C call is timed.
Split: send-sized transactions (§23's pool of 64 distinct ones, repeated) wrapped into bodies of four shapes, blocks x transactions a block: 64 x 128, 8,192 x 1,
1 x 8,192 and 1 x 65,536.  The last two are one lane walking one list, a chain of dependent reads: their time an element is printed beside them.
Chain: §23's segment (tools/bodies_bench.py builds it: blocks x block distinct valid mint proofs) and states.  "raw" times verifyChainRawBodies on the segment wrapped
into bodies; "roots" times verifyChainBodiesRoots on the segment with off and block_first made outside the clock — on --parent-lib where given (ZKGPU_LIB).  One side
is called slower only where the medians differ by more than the two spreads together.  The Go loop that the new call replaces runs on no machine here: no ratio to
it is claimed."""
import ctypes, json, os, random, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = [(64, 128), (8192, 1), (1, 8192), (1, 65536)]
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

if "--child" not in sys.argv and "--chain" not in sys.argv:
    procs, calls = arg("--processes", 5), arg("--calls", 5); runs = children(("split",), procs, ["--calls", str(calls)])["split"]
    print("wall time of zkBodySplit, ms: median (p10-p90) over %d processes, each the median of %d calls after a warm-up call; %d bytes a transaction" % (procs, calls, runs[0]["bytes"]))
    for nb, per in SHAPES:
        v = [r["%dx%d" % (nb, per)] for r in runs]; tail = "   %7.1f ns an element: one lane, a chain of dependent reads" % (1e6 * pct(v, 0.5) / per) if nb == 1 else ""
        print("   %5d bodies x %6d transactions   %s%s" % (nb, per, spread(v), tail))
    sys.exit(0)

if "--chain" in sys.argv and "--child" not in sys.argv:
    procs, calls, blocks, block = arg("--processes", 5), arg("--calls", 5), arg("--blocks", 64), arg("--block", 128); d = sarg("--keep") or tempfile.mkdtemp(prefix="raw_bodies_bench_")
    if not os.path.exists(os.path.join(d, "segment.json")):                                          # §23's segment, built by §23's tool
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bodies_bench.py"), "--child", "setup", "--dir", d, "--blocks", str(blocks), "--block", str(block)], timeout=3000)
        if r.returncode != 0: sys.exit(1)
    parent = sarg("--parent-lib"); extra = ["--dir", d, "--calls", str(calls), "--blocks", str(blocks), "--block", str(block)]
    runs = children(("raw", "roots"), procs, extra, lambda kind: {"ZKGPU_LIB": parent} if (kind == "roots" and parent) else None)
    print("wall time, ms: median (p10-p90) over %d processes a call, alternating, each the median of %d calls after a warm-up call; %d blocks x %d mint records" % (procs, calls, blocks, block))
    a, b = [r["ms"] for r in runs["raw"]], [r["ms"] for r in runs["roots"]]
    print("   verifyChainRawBodies                                %s" % spread(a))
    print("   verifyChainBodiesRoots%s         %s   (off and block_first made outside the timed region)" % (" on the parent's library" if parent else " on this build        ", spread(b)))
    print("   verifyChainRawBodies less verifyChainBodiesRoots    %s" % verdict(a, b))
    sys.exit(0)

import numpy as np
import tx_model as t
import tx_corpus as c
import body_model as bdm
kind = sarg("--child", "split"); CALLS = arg("--calls", 5); CHAIN = 1337
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
from blockmaze_amd import engine as e
hip = ctypes.CDLL("libamdhip64.so")
def now(): hip.hipDeviceSynchronize(); return time.perf_counter()

if kind in ("raw", "roots"):
    d = sarg("--dir"); os.environ["ZK_PRFKEY_DIR"] = d; BLOCK = arg("--block", 128); seg = json.load(open(os.path.join(d, "segment.json"))); raws = [bytes.fromhex(x) for x in seg["raws"]]; n = len(raws); nb = n // BLOCK
    e.init(); L = e.lib(); zk = e.Zk(); rng = np.random.default_rng(78); cid = ctypes.c_uint64(CHAIN); P = e._bytes
    fr, txhash, code, status = zk.TxSenders(raws, t.EIP155, CHAIN); assert status == [0] * n; froms = np.frombuffer(b"".join(fr), dtype=np.uint8).reshape(n, 20).copy()
    olds = np.frombuffer(b"".join(bytes.fromhex(x) for x in seg["olds"]), dtype=np.uint8).reshape(n, 32); other = rng.integers(0, 256, (1 << 16, 20), dtype=np.uint8)
    s = e.SpentSet(bytes(20)); s.spend(rng.integers(0, 256, (1 << 12, 20), dtype=np.uint8)); s0 = s.size(); tree = e.Tree(8); th = ctypes.c_void_p(tree.h); sh = ctypes.c_void_p(s.h)
    a = e.AccountTable(); a.set(other, rng.integers(0, 256, (1 << 16, 32), dtype=np.uint8)); a.set(froms, olds); n0 = a.size(); ah = ctypes.c_void_p(a.h)
    prior = np.zeros(1, dtype=np.int64); first = np.arange(0, n + 1, BLOCK, dtype=np.int32); ok = np.zeros(n, dtype=np.uint8); of = np.zeros(n, dtype=np.int32); sizes = [np.zeros(nb, dtype=np.int64) for _ in range(3)]
    th32, f20, cd, st = [np.zeros((n, w), dtype=np.uint8) for w in (32, 20, 1, 1)]; times = []; recs = np.zeros(n, dtype=e.RECORD_DTYPE); rf = np.zeros((n, 20), dtype=np.uint8); rec_of = np.zeros(n, dtype=np.int32); m = ctypes.c_int(0)
    got, defined = zk.TxRoots(raws, first); assert all(defined); want = np.frombuffer(b"".join(got), dtype=np.uint8).copy(); roots = np.zeros((nb, 32), dtype=np.uint8); rok = np.zeros(nb, dtype=np.uint8)
    outs = [vp(recs), vp(rf), vp(rec_of), vp(th32), vp(f20), vp(cd), vp(st), vp(ok), vp(of), *[vp(x) for x in sizes], ctypes.byref(m), vp(want), vp(roots), vp(rok)]
    if kind == "roots":                                                                              # off and block_first: the caller's, made before the clock starts
        blob, off = e._tx_blob(raws); L.verifyChainBodiesRoots.restype = ctypes.c_int
        def call(): return L.verifyChainBodiesRoots(None, P(blob), e._u64p(off), n, vp(first), nb, 2, cid, ah, th, vp(prior), 1, 8, sh, *outs)
    else:
        bodies = [bdm.body(raws[b * BLOCK:(b + 1) * BLOCK]) for b in range(nb)]; blob, boff = e._tx_blob(bodies); tb = np.zeros(n, dtype=np.uint64); ts = np.zeros(n, dtype=np.uint32); bf = np.zeros(nb + 1, dtype=np.int32)
        bs = np.zeros(nb, dtype=np.uint8); nt = ctypes.c_int(0); L.verifyChainRawBodies.restype = ctypes.c_int
        def call(): return L.verifyChainRawBodies(None, P(blob), e._u64p(boff), nb, n, 2, cid, ah, th, vp(prior), 1, 8, sh, *outs, vp(tb), vp(ts), vp(bf), vp(bs), ctypes.byref(nt))
    for k in range(CALLS + 1):
        t0 = now(); rc = call(); t1 = now(); assert rc == nb and m.value == n, (rc, m.value, L.zkgpu_last_error())
        assert sizes[0][-1] == n0 + n and sizes[1][-1] == s0 + n and rok.all() and roots.tobytes() == want.tobytes(); a.rewind(n0); s.rewind(s0)
        if kind == "raw": assert nt.value == n and list(bf) == list(first) and not bs.any() and all(blob[int(tb[i]):int(tb[i]) + int(ts[i])].tobytes() == raws[i] for i in (0, 1, n // 2, n - 1))
        if k: times.append(1e3 * (t1 - t0))
    print("JSON " + json.dumps({"ms": statistics.median(times)})); sys.exit(0)

rng = random.Random(9); pool = []
for k in range(64):
    tx = c.rand_tx(rng, Code=2, Payload=b"", AUX=b"", CMTBlock=[rng.randrange(2**32)]); pool.append(t.encode(t.sign_tx(tx, t.EIP155, CHAIN, rng.randrange(1, 2**24), rng.randrange(1, 2**24))))
e.init(); L = e.lib(); out = {"bytes": int(statistics.mean(len(p) for p in pool))}; L.zkBodySplit.restype = ctypes.c_int
for nb, per in SHAPES:
    n = nb * per; bodies = [bdm.body([pool[(b * per + j) % 64] for j in range(per)]) for b in range(nb)]; blob, off = e._tx_blob(bodies)
    tb = np.zeros(n, dtype=np.uint64); ts = np.zeros(n, dtype=np.uint32); bf = np.zeros(nb + 1, dtype=np.int32); bs = np.zeros(nb, dtype=np.uint8); nt = ctypes.c_int(0)
    def split(): assert L.zkBodySplit(e._bytes(blob), e._u64p(off), nb, n, vp(tb), vp(ts), vp(bf), vp(bs), ctypes.byref(nt)) == nb and nt.value == n
    split(); assert list(bf) == list(range(0, n + 1, per)) and blob[int(tb[n - 1]):int(tb[n - 1]) + int(ts[n - 1])].tobytes() == pool[(n - 1) % 64]; times = []
    for _ in range(CALLS): t0 = now(); split(); times.append(1e3 * (now() - t0))
    out["%dx%d" % (nb, per)] = statistics.median(times)
print("JSON " + json.dumps(out))
