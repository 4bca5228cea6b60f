#!/usr/bin/env python3
"""zkTxRoots beside zkTxSenders, and verifyChainBodiesRoots beside verifyChainBodies; its output is the tables of profiles/tx_roots.txt.

    python tools/tx_roots_bench.py [--processes 5] [--calls 5]
    python tools/tx_roots_bench.py --chain [--blocks 64] [--block 128] [--processes 5] [--calls 5] [--parent-lib OTHER/libzkgpu.so] [--keep DIR]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/tx_roots_bench.py --one 8192    # the kernels' share: a warm-up call and one call of zkTxRoots
    python tools/tx_roots_bench.py --summarize KERNEL_STATS.csv

DESIGN.md §12's protocol, as tools/bodies_bench.py applies it: fresh processes, every size warmed up by one call, a device synchronise before every clock read; a
process reports the median of `calls` calls, the table the median and p10-p90 of those over the processes.  Only the C call is timed.
Roots: n = 128, 8,192 and 65,536 send-sized transactions (§23's pool of 64 distinct ones, repeated), in blocks of 128 ("b128") and as one block ("one").  The
processes alternate between "snd", which times zkTxSenders on the same bytes, and "rts", which times zkTxRoots.  The two calls do different work — a recovery, a
trie — and the reference's DeriveSha is Go, which no machine here runs: the times stand side by side and no ratio is claimed.
Chain: §23's segment (tools/bodies_bench.py builds it: blocks x block distinct valid mint proofs) and states.  "roots" times verifyChainBodiesRoots with the roots
zkTxRoots gives for the segment; "bodies" times verifyChainBodies — on --parent-lib where given (ZKGPU_LIB).  One side is called slower only where the medians differ
by more than the two spreads together."""
import ctypes, json, os, random, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [128, 8192, 65536]
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

if "--child" not in sys.argv and "--one" not in sys.argv and "--chain" not in sys.argv:
    procs, calls = arg("--processes", 5), arg("--calls", 5); runs = children(("snd", "rts"), procs, ["--calls", str(calls)])
    print("wall time of the C call, ms: median (p10-p90) over %d processes a kind, alternating, each the median of %d calls after a warm-up call; %d bytes a transaction" % (procs, calls, runs["snd"][0]["bytes"]))
    for n in SIZES:
        print("   n = %6d   zkTxSenders %s" % (n, spread([r["snd_%d" % n] for r in runs["snd"]])))
        for shape in ("b128", "one"): print("                zkTxRoots, %-16s %s" % ("blocks of 128" if shape == "b128" else "one block", spread([r["%s_%d" % (shape, n)] for r in runs["rts"]])))
    sys.exit(0)

if "--chain" in sys.argv and "--child" not in sys.argv:
    procs, calls, blocks, block = arg("--processes", 5), arg("--calls", 5), arg("--blocks", 64), arg("--block", 128); d = sarg("--keep") or tempfile.mkdtemp(prefix="tx_roots_bench_")
    if not os.path.exists(os.path.join(d, "segment.json")):                                          # §23's segment, built by §23's tool
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bodies_bench.py"), "--child", "setup", "--dir", d, "--blocks", str(blocks), "--block", str(block)], timeout=3000)
        if r.returncode != 0: sys.exit(1)
    parent = sarg("--parent-lib"); extra = ["--dir", d, "--calls", str(calls), "--blocks", str(blocks), "--block", str(block)]
    runs = children(("roots", "bodies"), procs, extra, lambda kind: {"ZKGPU_LIB": parent} if (kind == "bodies" and parent) else None)
    print("wall time, ms: median (p10-p90) over %d processes a call, alternating, each the median of %d calls after a warm-up call; %d blocks x %d mint records" % (procs, calls, blocks, block))
    a, b = [r["ms"] for r in runs["roots"]], [r["ms"] for r in runs["bodies"]]
    print("   verifyChainBodiesRoots                              %s" % spread(a))
    print("   verifyChainBodies%s              %s" % (" on the parent's library" if parent else " on this build        ", spread(b)))
    print("   verifyChainBodiesRoots less verifyChainBodies       %s" % verdict(a, b))
    sys.exit(0)

import numpy as np
import tx_model as t
import tx_corpus as c
kind = sarg("--child", "rts"); CALLS = arg("--calls", 5); CHAIN = 1337
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
from blockmaze_amd import engine as e
hip = ctypes.CDLL("libamdhip64.so")
def now(): hip.hipDeviceSynchronize(); return time.perf_counter()

if kind in ("roots", "bodies"):
    d = sarg("--dir"); os.environ["ZK_PRFKEY_DIR"] = d; BLOCK = arg("--block", 128); seg = json.load(open(os.path.join(d, "segment.json"))); raws = [bytes.fromhex(x) for x in seg["raws"]]; n = len(raws); nb = n // BLOCK
    e.init(); L = e.lib(); zk = e.Zk(); rng = np.random.default_rng(78); blob, off = e._tx_blob(raws); cid = ctypes.c_uint64(CHAIN); P = e._bytes
    fr, txhash, code, status = zk.TxSenders(raws, t.EIP155, CHAIN); assert status == [0] * n; froms = np.frombuffer(b"".join(fr), dtype=np.uint8).reshape(n, 20).copy()
    olds = np.frombuffer(b"".join(bytes.fromhex(x) for x in seg["olds"]), dtype=np.uint8).reshape(n, 32); other = rng.integers(0, 256, (1 << 16, 20), dtype=np.uint8)
    s = e.SpentSet(bytes(20)); s.spend(rng.integers(0, 256, (1 << 12, 20), dtype=np.uint8)); s0 = s.size(); tree = e.Tree(8); th = ctypes.c_void_p(tree.h); sh = ctypes.c_void_p(s.h)
    a = e.AccountTable(); a.set(other, rng.integers(0, 256, (1 << 16, 32), dtype=np.uint8)); a.set(froms, olds); n0 = a.size(); ah = ctypes.c_void_p(a.h)
    prior = np.zeros(1, dtype=np.int64); first = np.arange(0, n + 1, BLOCK, dtype=np.int32); ok = np.zeros(n, dtype=np.uint8); of = np.zeros(n, dtype=np.int32); sizes = [np.zeros(nb, dtype=np.int64) for _ in range(3)]
    th32, f20, cd, st = [np.zeros((n, w), dtype=np.uint8) for w in (32, 20, 1, 1)]; times = []; recs = np.zeros(n, dtype=e.RECORD_DTYPE); rf = np.zeros((n, 20), dtype=np.uint8); rec_of = np.zeros(n, dtype=np.int32); m = ctypes.c_int(0)
    fn = L.verifyChainBodiesRoots if kind == "roots" else L.verifyChainBodies; fn.restype = ctypes.c_int; tail = []
    if kind == "roots":                                                                              # the headers' roots: what zkTxRoots gives for these bodies
        got, defined = zk.TxRoots(raws, first); assert all(defined); want = np.frombuffer(b"".join(got), dtype=np.uint8).copy(); roots = np.zeros((nb, 32), dtype=np.uint8); rok = np.zeros(nb, dtype=np.uint8)
        tail = [vp(want), vp(roots), vp(rok)]
    for call in range(CALLS + 1):
        t0 = now()
        rc = fn(None, P(blob), e._u64p(off), n, vp(first), nb, 2, cid, ah, th, vp(prior), 1, 8, sh, vp(recs), vp(rf), vp(rec_of), vp(th32), vp(f20), vp(cd), vp(st), vp(ok), vp(of), *[vp(x) for x in sizes], ctypes.byref(m), *tail)
        t1 = now(); assert rc == nb and m.value == n, (rc, m.value)
        assert sizes[0][-1] == n0 + n and sizes[1][-1] == s0 + n and (kind == "bodies" or (rok.all() and roots.tobytes() == want.tobytes())); a.rewind(n0); s.rewind(s0)
        if call: times.append(1e3 * (t1 - t0))
    print("JSON " + json.dumps({"ms": statistics.median(times)})); sys.exit(0)

rng = random.Random(9); pool = []
for k in range(64):
    tx = c.rand_tx(rng, Code=2, Payload=b"", AUX=b"", CMTBlock=[rng.randrange(2**32)]); pool.append(t.encode(t.sign_tx(tx, t.EIP155, CHAIN, rng.randrange(1, 2**24), rng.randrange(1, 2**24))))
e.init(); L = e.lib(); out = {"bytes": int(statistics.mean(len(p) for p in pool))}; L.zkTxSenders.restype = ctypes.c_int; L.zkTxRoots.restype = ctypes.c_int
import trie_model as tm
small = [bytes(r) for r in e.tx_roots(pool[:3], [0, 3])[1]]; assert small == [tm.derive_sha(pool[:3], keccak_many=e.keccak256)]   # the call that is timed computes DeriveSha
if "--one" in sys.argv: SIZES = [arg("--one", 8192)]; CALLS = 1                                      # one warm-up call and one call: what a profiler run looks at
for n in SIZES:
    raws = [pool[i % 64] for i in range(n)]; blob, off = e._tx_blob(raws); P = e._bytes; cid = ctypes.c_uint64(CHAIN)
    th, fr, code, st = [np.zeros(n * w, dtype=np.uint8) for w in (32, 20, 1, 1)]
    def senders(): assert L.zkTxSenders(P(blob), e._u64p(off), n, 2, cid, P(th), P(fr), P(code), P(st)) == n
    shapes = [("snd", None)] if kind == "snd" else [("b128", np.arange(0, n + 1, 128, dtype=np.int32)), ("one", np.array([0, n], dtype=np.int32))]
    if "--one" in sys.argv: shapes = shapes[:1]
    for name, first in shapes:
        if first is not None: nb = int(first.size) - 1; roots = np.zeros(32 * nb, dtype=np.uint8); defined = np.zeros(nb, dtype=np.uint8)
        def tx_roots(): assert L.zkTxRoots(P(blob), e._u64p(off), n, vp(first), nb, P(roots), P(defined)) == nb
        call = senders if first is None else tx_roots; call(); ts = []
        for _ in range(CALLS): t0 = now(); call(); ts.append(1e3 * (now() - t0))
        out["%s_%d" % (name, n)] = statistics.median(ts)
print("JSON " + json.dumps(out))
