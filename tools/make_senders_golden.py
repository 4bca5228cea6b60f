#!/usr/bin/env python3
"""Writes tests/golden/ecrecover_cases.txt: (hash, signature, homestead) cases with the verdict and the public key the REFERENCE's own libsecp256k1 gives, and times
that library.  Run once, by hand, on a machine that has the reference tree; no test runs it.

    python tools/make_senders_golden.py --reference /path/to/reference            # writes the fixture
    python tools/make_senders_golden.py --reference /path/to/reference --time 5000 # microseconds per recovery, one core

The library is compiled in place, with the #defines of crypto/secp256k1/secp256.go:23-28, into oracle/_ref/ (git-ignored); the few lines of C below only call it:
secp256k1_ecdsa_recoverable_signature_parse_compact + secp256k1_ecdsa_recover + secp256k1_ec_pubkey_serialize, as ext.h's secp256k1_ext_ecdsa_recover does.
Go is not needed: the twelve lines of crypto.ValidateSignatureValues (crypto/crypto.go:199-210), which recoverPlain runs in front of the library, are restated in
validate() below.  The address column is the model's Keccak-256 (tests/secp_model.py), which tests/test_senders_cpu.py pins to the reference's own vectors."""
import argparse, os, random, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp_model as m

DRIVER = r"""
#define USE_NUM_NONE
#define USE_FIELD_10X26
#define USE_FIELD_INV_BUILTIN
#define USE_SCALAR_8X32
#define USE_SCALAR_INV_BUILTIN
#define NDEBUG
#include "src/secp256k1.c"
#include "src/modules/recovery/main_impl.h"
#include <stdio.h>
#include <string.h>
#include <time.h>
static int recover(const secp256k1_context *ctx, unsigned char *pub65, const unsigned char *sig65, const unsigned char *msg32) {
  secp256k1_ecdsa_recoverable_signature sig; secp256k1_pubkey pubkey; size_t len = 65;
  if (!secp256k1_ecdsa_recoverable_signature_parse_compact(ctx, &sig, sig65, (int)sig65[64])) return 0;
  if (!secp256k1_ecdsa_recover(ctx, &pubkey, &sig, msg32)) return 0;
  return secp256k1_ec_pubkey_serialize(ctx, pub65, &len, &pubkey, SECP256K1_EC_UNCOMPRESSED);
}
static int unhex(const char *s, unsigned char *out, int n) { for (int i = 0; i < n; i++) { unsigned v; if (sscanf(s + 2 * i, "%2x", &v) != 1) return 0; out[i] = (unsigned char)v; } return 1; }
int main(int argc, char **argv) {
  secp256k1_context *ctx = secp256k1_context_create(SECP256K1_CONTEXT_SIGN | SECP256K1_CONTEXT_VERIFY);
  char h[80], s[140]; unsigned char msg[32], sig[65], pub[65];
  if (argc == 4) {                                                  /* time: count, hash, signature */
    int n = atoi(argv[1]), good = 0; struct timespec a, b;
    if (!unhex(argv[2], msg, 32) || !unhex(argv[3], sig, 65)) return 2;
    clock_gettime(CLOCK_MONOTONIC, &a); for (int i = 0; i < n; i++) good += recover(ctx, pub, sig, msg); clock_gettime(CLOCK_MONOTONIC, &b);
    printf("%d %d %.3f\n", n, good, ((b.tv_sec - a.tv_sec) * 1e9 + (b.tv_nsec - a.tv_nsec)) / 1e3 / n); return 0;
  }
  while (scanf("%79s %139s", h, s) == 2) {
    if (strlen(h) != 64 || strlen(s) != 130 || !unhex(h, msg, 32) || !unhex(s, sig, 65)) return 2;
    if (!recover(ctx, pub, sig, msg)) { printf("0\n"); continue; }
    printf("1 "); for (int i = 1; i < 65; i++) printf("%02x", pub[i]); printf("\n");
  }
  return 0;
}
"""

def build(reference):
    src_dir = os.path.join(reference, "go-ethereum", "crypto", "secp256k1", "libsecp256k1"); out = os.path.join(ROOT, "oracle", "_ref"); os.makedirs(out, exist_ok=True)
    drv = os.path.join(out, "ecrecover_driver.c"); exe = os.path.join(out, "ecrecover_driver")
    with open(drv, "w") as f: f.write(DRIVER)
    subprocess.check_call(["gcc", "-O2", "-w", "-I", src_dir, "-I", os.path.join(src_dir, "src"), drv, "-o", exe]); return exe

def validate(v, r, s, homestead):
    """crypto.go:199-210"""
    if r < 1 or s < 1: return False
    if homestead and s > m.N // 2: return False
    return r < m.N and s < m.N and v in (0, 1)

TESTMSG = "ce0677bb30baa8cf067c88db9811f4333d131bf8bcf12fe7065d211dce971008"             # crypto/signature_test.go:31-33
TESTSIG = "90f27b8b488db00b00606796d2987f6a5f59ae62ea05effe84fef5b8b0e549984a691139ad57a3f0b906637673aa2f63d1f55cb1a69199d4009eea23ceaddc9301"

def cases():
    rng = random.Random(20260101); out = []; N, P = m.N, m.P
    def b32(v): return v.to_bytes(32, "big")
    def put(h, r, s, v, hs): out.append((h if isinstance(h, bytes) else b32(h), b32(r) + b32(s) + bytes([v]), hs))
    def valid():
        h = rng.getrandbits(256); sig = m.sign(b32(h), rng.randrange(1, N), rng.randrange(1, N)); return h, int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:64], "big"), sig[64]
    out.append((bytes.fromhex(TESTMSG), bytes.fromhex(TESTSIG), 0)); out.append((bytes.fromhex(TESTMSG), bytes.fromhex(TESTSIG), 1))
    parities = [0, 0]
    while len(out) < 202:                                                                # 200 seeded random signatures, both parities
        h, r, s, v = valid(); parities[v] += 1; put(h, r, s, v, len(out) & 1)
    assert min(parities) >= 60
    for hs in (0, 1):
        h, r, s, v = valid()
        for bad_v in (2, 3, 4, 27, 28, 255): put(h, r, s, bad_v, hs)
        for bad_r in (0, N - 1, N, 2**256 - 1): put(h, bad_r, s, v, hs)
        for odd_s in (0, 1, N // 2, N // 2 + 1, N - 1, N): put(h, r, odd_s, v, hs)
        on = off = 0
        while on + off < 40:                                                             # random r, about half of them no x of the curve
            x = rng.randrange(1, N); is_x = pow(x ** 3 + 7, (P - 1) // 2, P) == 1
            if (is_x and on >= 20) or (not is_x and off >= 20): continue
            on += is_x; off += not is_x; put(h, x, s, (on + off) & 1, hs)
        for hh in (0, N - 1, N, N + 1, 2**256 - 1): put(hh, r, s, v, hs)
        for x in (1, 2, 3, 4, P - N - 1, P - N - 2): put(h, x, s, v, hs)                  # r below p - N: the values for which a recid of 2 or 3 would name another point
    ks = [1, 2, 16, N - 1, 3, N - 2] + [rng.randrange(1, N) for _ in range(6)]
    while len(out) < 10**9:
        i = sum(1 for c in out if c[2] == 2); k = ks[i % len(ks)]
        if i >= 100: break
        if i < 30: u2 = rng.randrange(1, N); u1 = (-k * u2) % N                           # u1 + k u2 = 0: Q at infinity
        elif i < 60: u1 = rng.choice([0, 1, 2, 15, 16, N - 1, N - 15]); u2 = rng.choice([1, 2, 15, 16, N - 1, N - 16])
        else: u1 = rng.randrange(N); u2 = rng.randrange(1, N)
        h, sig = m.forge(k, u1, u2); out.append((h, sig, 2))                              # (2: a forged case, homestead off — s is anything)
    return [(h, sig, 0 if hs == 2 else hs) for h, sig, hs in out]

def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--reference", required=True); ap.add_argument("--time", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ecrecover_cases.txt")); a = ap.parse_args()
    exe = build(a.reference)
    if a.time:
        n, good, us = subprocess.run([exe, str(a.time), TESTMSG, TESTSIG], capture_output=True, text=True, check=True).stdout.split()
        assert n == good; print("reference libsecp256k1 recovery: %s us each, %s recoveries of the reference's test signature, one core" % (us, n)); return
    cs = cases(); asked = [(i, c) for i, c in enumerate(cs) if validate(c[1][64], int.from_bytes(c[1][:32], "big"), int.from_bytes(c[1][32:64], "big"), c[2])]
    res = subprocess.run([exe], input="".join("%s %s\n" % (c[0].hex(), c[1].hex()) for _, c in asked), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(res) == len(asked); verdict = {i: r.split() for (i, _), r in zip(asked, res)}; lines = []
    for i, (h, sig, hs) in enumerate(cs):
        v = verdict.get(i, ["0"])
        if v[0] == "1": xy = bytes.fromhex(v[1]); lines.append("%s %s %d 1 %s %s" % (h.hex(), sig.hex(), hs, xy.hex(), m.keccak256(xy)[12:].hex()))
        else: lines.append("%s %s %d 0" % (h.hex(), sig.hex(), hs))
    assert len(lines) <= 600
    with open(a.out, "w") as f: f.write("\n".join(lines) + "\n")
    print("%d cases, %d accepted, %d refused before the library, %d refused by it -> %s" % (len(lines), sum(l.split()[3] == "1" for l in lines), len(cs) - len(asked),
                                                                                         sum(v[0] == "0" for v in verdict.values()), a.out))
if __name__ == "__main__": main()
