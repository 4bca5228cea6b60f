#!/usr/bin/env python3
"""zkTxSigningInputs and zkTxSenders on the device, with zkRecoverSenders alone beside them; its output is the table of profiles/txs.txt.

    python tools/txs_bench.py [--processes 5] [--calls 5] [--parent-lib OTHER/libzkgpu.so [--bench-reps 2]]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/txs_bench.py --one 8192     # the kernels' share: a warm-up call and one call of zkTxSenders
    python tools/txs_bench.py --summarize KERNEL_STATS.csv

DESIGN.md §12's protocol: fresh processes, every size warmed up by one call, a device synchronise (hipDeviceSynchronize) before every clock read; a process reports
the median of `calls` calls, the table the median and p10-p90 of those over the processes.  Only the C call is timed: the arrays are built before the clock starts.
n = 128, 8,192 and 65,536 send-sized transactions (a 512-character ZKProof, about 0.9 KB; 64 distinct ones, signed by the model under EIP155, repeated: lanes
share nothing, so a repeated transaction costs what a new one costs).  The processes alternate between the two kinds — "txs" times the two new calls, "rec"
times zkRecoverSenders alone on the signing inputs of the same transactions — so that the cost of the walk and the hashes is read as a difference on one box in
one session.  With --parent-lib: bench.py --gpus 1 --steps 50 --warmup 5 on this build and on the other library (ZKGPU_LIB), alternating, by
tools/proof_cache_bench.py's helper.  The reference's decode and hash are Go, which no machine here runs: no ratio against it is claimed."""
import ctypes, json, os, random, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [128, 8192, 65536]
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
def arg(name, default): return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

if "--summarize" in sys.argv:
    import csv
    print("average ns a launch, share of the run:")
    for r in csv.DictReader(open(sys.argv[sys.argv.index("--summarize") + 1])): print("   %-18s %12.0f %6.1f %%  (%s calls)" % (r["Name"].split("(")[0].replace("zk::", ""), float(r["AverageNs"]), float(r["Percentage"]), r["Calls"]))
    sys.exit(0)

if "--child" not in sys.argv and "--one" not in sys.argv:
    procs, calls = arg("--processes", 5), arg("--calls", 5); runs = {"txs": [], "rec": []}
    for k in range(procs):
        for kind in ("txs", "rec"):                                                                  # alternating: one session, one box
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--calls", str(calls)], capture_output=True, text=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
            if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
            runs[kind].append(json.loads(line[0][5:])); print("process %d %s done" % (k, kind), flush=True)
    print("wall time of the C call, ms: median (p10-p90) over %d processes a kind, alternating, each the median of %d calls after a warm-up call; %d bytes a transaction" % (procs, calls, runs["txs"][0]["bytes"]))
    med = {}
    for name, kind, key in (("zkTxSigningInputs", "txs", "inputs"), ("zkTxSenders", "txs", "senders"), ("zkRecoverSenders", "rec", "recover")):
        for n in SIZES:
            v = [r["%s_%d" % (key, n)] for r in runs[kind]]; med[(key, n)] = (pct(v, 0.5), pct(v, 0.1), pct(v, 0.9))
            print("   %-18s n = %6d   %9.3f (%9.3f-%9.3f) ms   %8.3f us a transaction" % (name, n, med[(key, n)][0], med[(key, n)][1], med[(key, n)][2], 1e3 * med[(key, n)][0] / n))
    print("zkTxSenders less zkRecoverSenders (the walk, the hashes, the larger upload), ms; the two spreads together beside it:")
    for n in SIZES:
        s, r = med[("senders", n)], med[("recover", n)]; both = (s[2] - s[1]) + (r[2] - r[1])
        print("   n = %6d   %+9.3f   spreads %.3f   %s" % (n, s[0] - r[0], both, "beyond the spreads" if abs(s[0] - r[0]) > both else "inside the spreads: no difference claimed"))
    if "--parent-lib" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tools")); from proof_cache_bench import bench_ab
        bench_ab(sys.argv[sys.argv.index("--parent-lib") + 1])
    sys.exit(0)

import numpy as np
import secp_model as sm
import tx_model as t
import tx_corpus as c
from blockmaze_amd import engine as e
CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so")
def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
kind = sys.argv[sys.argv.index("--child") + 1] if "--child" in sys.argv else "txs"
rng = random.Random(9); CHAIN = 1337; pool = []
for k in range(64):
    tx = c.rand_tx(rng, Code=2, Payload=b"", AUX=b"", CMTBlock=[rng.randrange(2**32)]); pool.append(t.encode(t.sign_tx(tx, t.EIP155, CHAIN, rng.randrange(1, 2**24), rng.randrange(1, 2**24))))
want = [t.sender(r, t.EIP155, CHAIN) for r in pool[:2]]; assert all(w[0] == t.OK for w in want)
e.init(); L = e.lib(); out = {"bytes": int(statistics.mean(len(p) for p in pool))}
for f in (L.zkRecoverSenders, L.zkTxSenders, L.zkTxSigningInputs): f.restype = ctypes.c_int
if "--one" in sys.argv: SIZES = [arg("--one", 8192)]; CALLS = 1                                      # one warm-up call and one call: what a profiler run looks at
for n in SIZES:
    raws = [pool[i % 64] for i in range(n)]; blob, off = e._tx_blob(raws); P = e._bytes; cid = ctypes.c_uint64(CHAIN)
    th, sh, sg, fr, code, st = [np.zeros(n * w, dtype=np.uint8) for w in (32, 32, 65, 20, 1, 1)]; pubs = np.zeros(64 * n, dtype=np.uint8); ok = np.zeros(n, dtype=np.uint8)
    def inputs(): assert L.zkTxSigningInputs(P(blob), e._u64p(off), n, 2, cid, P(th), P(sh), P(sg), P(fr), P(code), P(st)) == n
    def senders(): assert L.zkTxSenders(P(blob), e._u64p(off), n, 2, cid, P(th), P(fr), P(code), P(st)) == n
    def recover(): assert L.zkRecoverSenders(P(sh), P(sg), n, 1, P(fr), None, P(ok)) == n
    inputs()                                                                                         # (the recovery's inputs come from here in both kinds)
    for name, call in ((("inputs", inputs), ("senders", senders)) if kind == "txs" else (("recover", recover),)):
        if "--one" in sys.argv and name != "senders": continue
        call(); ts = []
        for _ in range(CALLS): t0 = now(); call(); ts.append(1e3 * (now() - t0))
        out["%s_%d" % (name, n)] = statistics.median(ts)
        if name != "inputs": assert bytes(fr[:20]) == want[0][3] and bytes(fr[20:40]) == want[1][3]
print("JSON " + json.dumps(out))
