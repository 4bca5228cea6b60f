#!/usr/bin/env python3
"""The proof cache on one GPU (DESIGN.md "Proof cache"); its output is profiles/proof_cache.txt.

    python tools/proof_cache_bench.py [--processes 5] [--calls 5] [--parent-lib OTHER/libzkgpu.so [--bench-reps 2]]

The protocol of tools/snset_bench.py: fresh processes, every size warmed up, a device synchronise (hipDeviceSynchronize) before every clock read; a process reports
the median of `calls` calls, the tables the median and p10-p90 of those over the processes.  Only the C calls are timed.  Keys and eight send proofs are made once, by a
process of their own; a block is those proofs in rotation with the `reserved` bytes counting up, so every record is valid and has a key of its own, and the serial
numbers repeat as they do in tools/snset_bench.py.  The set holds 2^16 other keys and every call is check-only (commit = 0).
  1. verifyBlockFullCached at 8,192 and 65,536 records — every record stored by an earlier call (the gate), no record stored (the cache cleared outside the clock, so
     the call also stores them all), every second record stored — beside verifyBlockFull of this build in the same process and, with --parent-lib, verifyBlockFull of
     the other library (ZKGPU_LIB) in processes that alternate with this build's.
  2. One record through verifyRecordsCached, stored and not stored, beside verifySendproof.
  3. The digest of n records alone (zkgpu_test_record_digests): the kernel and the host model on one core; DIGEST_DEVICE_MIN comes from this table.
  4. With --parent-lib: bench.py --gpus 1 --steps 50 --warmup 5 on this build and on the other library, alternating."""
import ctypes, json, os, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
NS = (8192, 65536); DIGEST_NS = (1, 4, 8, 16, 32, 64, 128, 256, 8192, 65536)
def pct(v, q): v = sorted(v); return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]
def arg(name, default, conv=int): return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default

def run_child(args, env=None, timeout=1500):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("JSON ")]
    if r.returncode != 0 or not line: print(r.stdout[-2000:], r.stderr[-3000:]); sys.exit(1)
    return json.loads(line[0][5:])

def parent():
    procs, calls = arg("--processes", 5), arg("--calls", 5); other = arg("--parent-lib", None, str); d = tempfile.mkdtemp(prefix="proof_cache_bench")
    env = dict(os.environ, ZK_PRFKEY_DIR=d); env.pop("ZKGPU_LIB", None); run_child(["--make", d], env); this, prev = [], []
    for _ in range(procs):
        this.append(run_child(["--child", d, "--calls", str(calls)], env))
        if other: prev.append(run_child(["--child", d, "--calls", str(calls), "--uncached-only"], dict(env, ZKGPU_LIB=os.path.abspath(other))))
    def col(runs, key): v = [r[key] for r in runs]; return pct(v, 0.5), pct(v, 0.1), pct(v, 0.9)
    fmt = lambda c: "%9.4f (%9.4f-%9.4f)" % c
    print("wall time of the C calls, ms: median (p10-p90) over %d processes, each the median of %d calls" % (procs, calls))
    print("1. a block of valid send records, a set of 2^16 other keys, commit = 0")
    for n in NS:
        print("   n = %d" % n); base = col(prev, "full_%d" % n) if prev else None
        if base: print("      %-44s | %s" % ("verifyBlockFull, the parent commit's library", fmt(base)))
        print("      %-44s | %s" % ("verifyBlockFull, this build", fmt(col(this, "full_%d" % n))))
        for key, label in (("hit_%d" % n, "verifyBlockFullCached, every record stored"), ("half_%d" % n, "verifyBlockFullCached, every second stored"), ("miss_%d" % n, "verifyBlockFullCached, no record stored")):
            c = col(this, key); line = "      %-44s | %s" % (label, fmt(c))
            if base:
                line += " | %+9.4f ms against the parent" % (c[0] - base[0])
                spread = (c[2] - c[1]) + (base[2] - base[1])
                if key.startswith("hit"): line += "; GATE %s: the margin is %.4f ms, the two spreads together %.4f" % ("met" if base[0] - c[0] > spread else "NOT MET", base[0] - c[0], spread)
            print(line)
        print("      where an all-miss call's time goes, ms (median over the processes): the keys %.4f, the lookup %.4f, storing %.4f" % tuple(col(this, "%s_%d" % (k, n))[0] for k in ("t_digest", "t_lookup", "t_insert")))
    print("2. one send record")
    for key, label in (("one_hit", "verifyRecordsCached, stored"), ("one_miss", "verifyRecordsCached, not stored"), ("one_plain", "verifySendproof")): print("      %-44s | %s" % (label, fmt(col(this, key))))
    print("3. the keys of n records alone: the kernel k_record_digest (upload, launch, download) and the host model on one core")
    for n in DIGEST_NS: a, b = col(this, "digest_dev_%d" % n), col(this, "digest_host_%d" % n); print("      n = %-6d | device %s | host %s | %s" % (n, fmt(a), fmt(b), "device" if a[0] < b[0] else "host"))
    bench_ab(other)

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

def make(d):
    from blockmaze_amd import engine as e
    import workload as w
    e.keygen("send", os.path.join(d, "sendpk.txt"), os.path.join(d, "sendvk.txt"), seed=8); zk = e.Zk(); items = []
    for i in range(8): x = w.send_instance(300 + i); items.append(("send", zk.GenSendProof(*w.send_args(x)), [x["cmtA_old"], x["sn_old"], x["cmtS"], x["cmtA"]], 0))
    np.save(os.path.join(d, "unit.npy"), e.records_from_items(items)); print("JSON {}")

def block(unit, n):
    recs = np.ascontiguousarray(np.tile(unit, n // len(unit))); recs["reserved"][:, :4] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4); return recs

def child(d):
    from blockmaze_amd import engine as e
    import workload as w
    CALLS = arg("--calls", 5); plain = "--uncached-only" in sys.argv; hip = ctypes.CDLL("libamdhip64.so"); e.init(); zk = e.Zk(); L = e.lib(); out = {}
    def now(): hip.hipDeviceSynchronize(); return time.perf_counter()
    def timed(fn, before=None, after=None):
        ts = []
        for i in range(CALLS + 1):
            if before: before()
            t0 = now(); r = fn(); t1 = now()
            if i: ts.append(1e3 * (t1 - t0))
        return statistics.median(ts), (after(r) if after else r)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p); z = ctypes.c_size_t; u = ctypes.c_uint64
    unit = np.load(os.path.join(d, "unit.npy")); s = zk.SnSetNew(); assert s and zk.SnSetSpend(s, [os.urandom(32) for _ in range(1 << 16)])[0] == 1 << 16; sp = ctypes.c_void_p(s)
    for n in NS:
        recs = block(unit, n); rp = p(recs); ok = np.zeros(n, dtype=np.uint8); size = ctypes.c_longlong(0)
        def verdict(rc): return rc, ok.tobytes(), size.value
        out["full_%d" % n], want = timed(lambda: L.verifyBlockFull(rp, n, None, None, sp, 0, p(ok), ctypes.byref(size)), None, verdict); assert want[0] == 8 and want[2] == 1 << 16
        if plain: continue
        c = e.ProofCache(4 * n); ch = ctypes.c_void_p(c.h); cached = lambda: L.verifyBlockFullCached(ch, rp, n, None, None, sp, 0, p(ok), ctypes.byref(size)); fill = lambda r: zk.VerifyRecordsCached(c, r)
        assert fill(recs) == (n, [True] * n) and c.stats()[3] == n
        out["hit_%d" % n], got = timed(cached, None, verdict); assert got == want and c.stats()[:2] == ((CALLS + 1) * n, n)
        out["miss_%d" % n], got = timed(cached, c.clear, verdict); assert got == want and c.stats()[3] == n
        out["half_%d" % n], got = timed(cached, lambda: (c.clear(), fill(recs[::2])), verdict); assert got == want and c.stats()[3] == n
        # the parts of an all-miss call on their own: the keys, a lookup of n absent keys, storing n keys
        tags = bytes(128); keys = np.zeros((n, 20), dtype=np.uint8); out["t_digest_%d" % n], _ = timed(lambda: L.zkgpu_test_record_digests(bytes(32), tags, rp, z(n), 1, p(keys)))
        t = e.SpentSet(); t.spend(os.urandom(20 * n)); idx = np.zeros(n, dtype=np.uint64); conf = np.zeros(n, dtype=np.uint8); h = ctypes.c_void_p(t.h)
        out["t_lookup_%d" % n], _ = timed(lambda: L.zkgpu_snset_query(h, u(n), p(keys), z(n), p(idx)))
        out["t_insert_%d" % n], _ = timed(lambda: L.zkgpu_snset_spend(h, p(keys), None, z(n), 1, p(conf), None), lambda: t.rewind(n)); t.close(); c.close()
    if not plain:
        one = block(unit, 8)[:1].copy(); op = p(one); ok1 = np.zeros(1, dtype=np.uint8); c = e.ProofCache(1024); ch = ctypes.c_void_p(c.h); call = lambda: (L.verifyRecordsCached(ch, op, 1, p(ok1)), int(ok1[0]))
        assert call() == (1, 1)
        out["one_hit"], got = timed(call); assert got == (1, 1) and c.stats()[0] == CALLS + 1
        out["one_miss"], got = timed(call, c.clear); assert got == (1, 1)
        x = w.send_instance(300); a = [zk.hx(x[k]) for k in ("cmtA_old", "sn_old", "cmtS", "cmtA")]; proof = bytes(unit[0]["proof"])
        out["one_plain"], got = timed(lambda: L.verifySendproof(proof, *a)); assert got
        big = block(unit, max(DIGEST_NS)); bp = p(big); tags = b"".join(bytes([k]) * 32 for k in range(4)); ka = np.zeros((max(DIGEST_NS), 20), dtype=np.uint8); kb = np.zeros_like(ka)
        for n in DIGEST_NS:
            out["digest_dev_%d" % n], rc = timed(lambda: L.zkgpu_test_record_digests(bytes(32), tags, bp, z(n), 1, p(ka))); assert rc == 0
            out["digest_host_%d" % n], rc = timed(lambda: L.zkgpu_test_record_digests(bytes(32), tags, bp, z(n), 0, p(kb))); assert rc == 0 and ka[:n].tobytes() == kb[:n].tobytes() and ka[:n].any()
    zk.SnSetFree(s); print("JSON " + json.dumps(out), flush=True)

if __name__ == "__main__":
    if "--make" in sys.argv: make(sys.argv[sys.argv.index("--make") + 1])
    elif "--child" in sys.argv: child(sys.argv[sys.argv.index("--child") + 1])
    else: parent()
