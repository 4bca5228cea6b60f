#!/usr/bin/env python3
"""zkHeaders beside zkRecoverSenders; its output is the table of profiles/headers.txt.

    python tools/headers_bench.py [--processes 5] [--calls 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/headers_bench.py --one 8192    # the kernels' share: a warm-up call and one call of zkHeaders
    python tools/headers_bench.py --summarize KERNEL_STATS.csv

DESIGN.md §12's protocol, as tools/tx_roots_bench.py applies it: fresh processes, every size warmed up by one call, a device synchronise before every clock read; a
process reports the median of `calls` calls, the table the median and p10-p90 of those over the processes.  Only the C call is timed.
n = 128, 8,192 and 65,536 headers: a chain of 64 linked headers signed by the model (tests/header_corpus.py: a checkpoint every eight, CMT lists of 0 to 2 elements,
about 610 bytes a header), repeated.  Every 64th header after the first is therefore ZK_HDR_ANCESTOR and the call returns 64; the device does the same work for it as
for an accepted one — the walk, both hashes and the recovery's six launches run for every lane, whatever the lane's status.  The processes alternate between "hdr",
which times zkHeaders, and "rec", which times zkRecoverSenders (homestead = 0) on the seal hashes and seals of the same headers: the recovery is inside zkHeaders, so
the second number says how much of the first it is.  The reference's VerifyHeaders is Go, which no machine here runs: no ratio is claimed."""
import ctypes, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = [128, 8192, 65536]
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
def arg(name, default): return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
def sarg(name, default=None): return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
def spread(v): return "%9.3f (%9.3f-%9.3f)" % (pct(v, 0.5), pct(v, 0.1), pct(v, 0.9))

if "--summarize" in sys.argv:
    import csv
    print("average ns a launch, share of the run:")
    for r in csv.DictReader(open(sarg("--summarize"))): print("   %-22s %12.0f %6.1f %%  (%s calls)" % (r["Name"].split("(")[0].replace("zk::", ""), float(r["AverageNs"]), float(r["Percentage"]), r["Calls"]))
    sys.exit(0)

if "--child" not in sys.argv and "--one" not in sys.argv:
    procs, calls = arg("--processes", 5), arg("--calls", 5); runs = {"hdr": [], "rec": []}
    for p in range(procs):
        for kind in ("hdr", "rec"):                                                                  # alternating: one session, one box
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--calls", str(calls)], capture_output=True, text=True, timeout=1500)
            line = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
            if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
            runs[kind].append(json.loads(line[0][5:])); print("process %d %s done" % (p, kind), flush=True)
    print("wall time of the C call, ms: median (p10-p90) over %d processes a kind, alternating, each the median of %d calls after a warm-up call; %d bytes a header" % (procs, calls, runs["hdr"][0]["bytes"]))
    for n in SIZES: print("   n = %6d   zkHeaders %s   zkRecoverSenders %s" % (n, spread([r["hdr_%d" % n] for r in runs["hdr"]]), spread([r["rec_%d" % n] for r in runs["rec"]])))
    sys.exit(0)

import numpy as np
import header_corpus as c
import header_model as hm
kind = sarg("--child", "hdr"); CALLS = arg("--calls", 5)
from blockmaze_amd import engine as e
hip = ctypes.CDLL("libamdhip64.so")
def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
pool, parent, signers = c.chain(c.CHAIN_SEED, 64); e.init(); L = e.lib(); out = {"bytes": int(statistics.mean(len(p) for p in pool))}
k, o = e.Zk().Headers(pool, c.PERIOD, c.CHAIN_EPOCH, c.NOW, parent); assert k == 64 and o["signer"] == signers     # the call that is timed decides the chain
seals = [hm.decode(p)[0]["Extra"][-65:] for p in pool]; P = e._bytes; vp = lambda a: a.ctypes.data_as(ctypes.c_void_p); u64 = ctypes.c_uint64
L.zkHeaders.restype = ctypes.c_int; L.zkRecoverSenders.restype = ctypes.c_int
if "--one" in sys.argv: SIZES = [arg("--one", 8192)]; CALLS = 1                                      # one warm-up call and one call: what a profiler run looks at
for n in SIZES:
    raws = [pool[i % 64] for i in range(n)]; blob, off = e._tx_blob(raws); ph = np.frombuffer(parent[0], dtype=np.uint8).copy()
    outs = [np.zeros(n * w, dtype=np.uint8) for w in (32, 32, 20, 20, 32, 32, 8, 8, 1, 1, 4, 4, 4, 4, 1)]
    def headers(): assert L.zkHeaders(P(blob), e._u64p(off), n, u64(c.PERIOD), u64(c.CHAIN_EPOCH), u64(c.NOW), 1, P(ph), u64(parent[1]), u64(parent[2]), *[vp(a) for a in outs]) == 64
    hashes = np.frombuffer(b"".join(o["sealhash"][i % 64] for i in range(n)), dtype=np.uint8).copy(); sigs = np.frombuffer(b"".join(seals[i % 64] for i in range(n)), dtype=np.uint8).copy()
    froms = np.zeros(20 * n, dtype=np.uint8); ok = np.zeros(n, dtype=np.uint8)
    def recover(): assert L.zkRecoverSenders(P(hashes), P(sigs), n, 0, P(froms), None, P(ok)) == n
    call = headers if kind == "hdr" else recover; call(); ts = []
    for _ in range(CALLS): t0 = now(); call(); ts.append(1e3 * (now() - t0))
    out["%s_%d" % (kind, n)] = statistics.median(ts)
    if kind == "rec": assert froms[:20 * 64].tobytes() == b"".join(signers)
print("JSON " + json.dumps(out))
