#!/usr/bin/env python3
"""zkRecoverSenders on the device (DESIGN.md "Senders from signatures"); its output is the table of profiles/senders.txt.

    python tools/senders_bench.py [--processes 5] [--calls 5] [--parent-lib OTHER/libzkgpu.so [--bench-reps 2]]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/senders_bench.py --one 8192     # the kernels' share: two calls of n
    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES --output-format csv -d OUT -- python tools/senders_bench.py --one 8192   # instructions, in a run of its own
    python tools/senders_bench.py --summarize KERNEL_STATS.csv COUNTER_COLLECTION.csv                            # the two tables of profiles/senders.txt from those files
    (the instructions of one product: tools/secp_mul_count.hip)

DESIGN.md §12's protocol: fresh processes, every size warmed up by one call, a device synchronise (hipDeviceSynchronize) before every clock read; a process reports
the median of `calls` calls, the table the median and p10-p90 of those over the processes.  Only the C call is timed: the arrays are built before the clock starts.
n = 1, 128, 8,192 and 65,536 valid signatures (256 distinct ones, signed by the model, repeated: lanes share nothing, so a repeated signature costs what a new one
costs), with pubs, homestead on.  With --parent-lib: bench.py --gpus 1 --steps 50 --warmup 5 on this build and on the other library (ZKGPU_LIB), alternating,
by tools/proof_cache_bench.py's helper: the prover is not touched, so every run must lie inside the others' spread and the last proof must be the same bytes.  The comparand, the reference's own libsecp256k1, is timed on another machine by tools/make_senders_golden.py --time."""
import ctypes, json, os, random, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [1, 128, 8192, 65536]
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
def arg(name, default): return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

PRODUCTS = {"k_secp_lift": 269, "k_secp_scalars": 338, "k_secp_rtable": 515, "k_secp_walk": 3084, "k_secp_affine": 274, "k_secp_address": 0}   # a signature, counted from the source
if "--count-isa" in sys.argv:
    import re
    cur = None; cnt = {}
    for l in open(sys.argv[sys.argv.index("--count-isa") + 1]):
        mm = re.match(r"^(_Z\w+):", l)
        if mm: cur = mm.group(1); cnt[cur] = {}
        elif cur and re.match(r"^\s+v_\w+", l): op = l.split()[0]; cnt[cur][op] = cnt[cur].get(op, 0) + 1
        if "s_endpgm" in l: cur = None
    for k, v in cnt.items(): print("%-28s %4d VALU lines: %s" % (k, sum(v.values()), ", ".join("%s %d" % x for x in sorted(v.items(), key=lambda x: -x[1])[:6])))
    sys.exit(0)
if "--summarize" in sys.argv:
    import csv, collections
    i = sys.argv.index("--summarize"); name = lambda k: k.split("(")[0].replace("zk::", "")
    print("average ns a launch, share of the run:")
    for r in csv.DictReader(open(sys.argv[i + 1])): print("   %-18s %12.0f %6.1f %%  (%s calls)" % (name(r["Name"]), float(r["AverageNs"]), float(r["Percentage"]), r["Calls"]))
    acc = collections.defaultdict(lambda: collections.defaultdict(float))
    for r in csv.DictReader(open(sys.argv[i + 2])): acc[name(r["Kernel_Name"])][r["Counter_Name"]] += float(r["Counter_Value"])
    print("SQ_INSTS_VALU a wave (= a signature: a wave instruction serves its 64 lanes), products a signature, instructions a product:"); ti = tp = 0
    for k, pr in PRODUCTS.items():
        if k not in acc: continue
        per = acc[k]["SQ_INSTS_VALU"] / acc[k]["SQ_WAVES"]; ti += per; tp += pr
        print("   %-18s %12.0f %6d %s   (%d waves)" % (k, per, pr, "%6.0f" % (per / pr) if pr else "", acc[k]["SQ_WAVES"]))
    print("   %-18s %12.0f %6d %6.0f   at 4.3 cycles an instruction and 2.4 GHz: %.3f ms a wave alone on its SIMD" % ("all", ti, tp, ti / tp, ti * 4.3 / 2.4e6))
    sys.exit(0)

if "--child" not in sys.argv and "--one" not in sys.argv:
    procs, calls = arg("--processes", 5), arg("--calls", 5); runs = []
    for k in range(procs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(calls)], capture_output=True, text=True, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
        if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
        runs.append(json.loads(line[0][5:])); print("process %d done" % k, flush=True)
    print("zkRecoverSenders, wall time of the C call, ms: median (p10-p90) over %d processes, each the median of %d calls after a warm-up call" % (procs, calls))
    for n in SIZES if runs else []:
        v = [r["ms_%d" % n] for r in runs]; med = pct(v, 0.5)
        print("   n = %6d   %9.3f (%9.3f-%9.3f) ms   %9.3f us a signature   %10.0f signatures/s" % (n, med, pct(v, 0.1), pct(v, 0.9), 1e3 * med / n, n / med * 1e3))
    if "--parent-lib" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tools")); from proof_cache_bench import bench_ab
        bench_ab(sys.argv[sys.argv.index("--parent-lib") + 1])
    sys.exit(0)

import numpy as np
import secp_model as m
from blockmaze_amd import engine as e
CALLS = arg("--calls", 5); hip = ctypes.CDLL("libamdhip64.so")
def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
rng = random.Random(9); hs = []; sg = []
for _ in range(256): h = rng.getrandbits(256).to_bytes(32, "big"); hs.append(h); sg.append(m.sign(h, rng.randrange(1, m.N), rng.randrange(1, m.N)))
e.init(); L = e.lib(); L.zkRecoverSenders.restype = ctypes.c_int; out = {}
if "--one" in sys.argv: SIZES = [arg("--one", 8192)]; CALLS = 1                                      # one warm-up call and one call: what a profiler run looks at
for n in SIZES:
    hb = np.frombuffer(b"".join(hs[i % 256] for i in range(n)), dtype=np.uint8).copy(); sb = np.frombuffer(b"".join(sg[i % 256] for i in range(n)), dtype=np.uint8).copy()
    froms = np.zeros(20 * n, dtype=np.uint8); pubs = np.zeros(64 * n, dtype=np.uint8); ok = np.zeros(n, dtype=np.uint8); a = [e._bytes(x) for x in (hb, sb)]; b = [e._bytes(x) for x in (froms, pubs, ok)]
    def call(): assert L.zkRecoverSenders(a[0], a[1], n, 1, b[0], b[1], b[2]) == n
    call(); t = []
    for _ in range(CALLS): t0 = now(); call(); t.append(1e3 * (now() - t0))
    assert bytes(froms[-20:]) == m.recover(hs[(n - 1) % 256], sg[(n - 1) % 256], True)[3]
    out["ms_%d" % n] = statistics.median(t)
print("JSON " + json.dumps(out))
