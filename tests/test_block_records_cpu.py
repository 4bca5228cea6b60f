"""Blocks as records (include/zk_records.h) without a device: the header and its layout, the host converter records_to_host against independent models, and the
integer sums the refactored rlc_acc_sum starts from."""
import ctypes, os, random, re, subprocess, sys
import numpy as np
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import block_records as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def declared_symbols(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S); src = re.sub(r"//[^\n]*", "", src)
    return sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", " ".join(l for l in src.splitlines() if not l.strip().startswith("#"))))
                  - {"defined", "sizeof", "static_assert", "_Static_assert"})

def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(l.split()[-1] for l in out.splitlines() if " T " in l)

def test_records_header_symbol_and_layout(tmp_path):
    """zk_records.h declares exactly verifyBlockRecords; libzkgpu.so exports it and none of the four drop-in libraries does; a C compiler lays zk_block_record out
    as engine.RECORD_DTYPE does: 720 bytes, every field where numpy puts it"""
    assert declared_symbols("zk_records.h") == ["verifyBlockRecords"]
    assert "verifyBlockRecords" in exported(os.path.join(ROOT, "blockmaze_amd", "libzkgpu.so"))
    for lib in ("zk_mint", "zk_send", "zk_deposit", "zk_redeem"): assert "verifyBlockRecords" not in exported(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib)), lib
    for s in ("zkgpu_verify_records_rlc", "zkgpu_test_ingest_records", "zkgpu_test_records_rlc", "zkgpu_test_rlc_sums_host"): assert hasattr(e.lib(), s), s
    src = tmp_path / "layout.c"; exe = str(tmp_path / "layout")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zk_records.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(zk_block_record), '
                   'offsetof(zk_block_record, kind), offsetof(zk_block_record, reserved), offsetof(zk_block_record, value_s), offsetof(zk_block_record, proof), '
                   'offsetof(zk_block_record, args), sizeof(((zk_block_record *)0)->proof), sizeof(((zk_block_record *)0)->args)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    f = e.RECORD_DTYPE.fields
    assert got == [720, 0, 1, 8, 16, 528, 512, 192]
    assert got == [e.RECORD_DTYPE.itemsize] + [f[k][1] for k in ("kind", "reserved", "value_s", "proof", "args")] + [f["proof"][0].itemsize, f["args"][0].itemsize]
    r = e.records_from_items([("deposit", "ab" * 256, [bytes([k + 1]) * (20 if k == 1 else 32) for k in range(6)], 7), ("send", "12", [b"\x05"], 0)])
    assert r["kind"].tolist() == [2, 1] and r["value_s"].tolist() == [7, 0] and bytes(r["proof"][0]) == b"ab" * 256 and bytes(r["proof"][1]) == b"12" + bytes(510)
    assert bytes(r["args"][0][1]) == b"\x02" * 20 + bytes(12) and bytes(r["args"][0][5]) == b"\x06" * 32 and bytes(r["args"][1][0]) == bytes(31) + b"\x05"

@pytest.mark.parametrize("kind", ["mint", "send", "deposit", "redeem"])
def test_host_converter_against_the_models(kind):
    """records_to_host (zkgpu_test_ingest_records, device = 0) on seeded random records and every edge case: the inputs are workload.pack_public's (4 / 5 / 6 / 4 of them
    for 832 / 1,024 / 1,440 / 832 bits), the proof's coordinates are (c mod q) 2^256 mod q for every 256-bit c, `parsed` is 0 exactly where a byte is no lower-case hex
    digit; what the layout calls ignored changes nothing"""
    k = br.KINDS[kind]; fields = br.statement_fields(k); assert 8 * sum(f[2] for f in fields) == br.N_BITS[k] and -(-br.N_BITS[k] // 253) == br.N_INPUTS[k]
    recs = np.concatenate([br.random_records(k, 300, 0xA11CE + k), br.edge_records(k, 0xB0B + k)])
    items, inputs, parsed = e.ingest_records(recs, device=False); br.check_against_models(recs, items, inputs, parsed)
    bad = br.bad_byte_records(k, 5); assert not e.ingest_records(bad, device=False)[2].any() and not e.ingest_records(bad, device=False)[0].any()
    assert e.ingest_records(br.coordinate_records(k, 6), device=False)[2].all()              # every 256-bit value is a coordinate
    # garbage where the layout says `ignored`
    clean = br.random_records(k, 64, 9); dirty = clean.copy(); rng = np.random.default_rng(10)
    dirty["reserved"] = rng.integers(0, 256, dirty["reserved"].shape, dtype=np.uint8)
    used = {0: 3, 1: 4, 2: 6, 3: 3}[k]
    if used < 6: dirty["args"][:, used:, :] = rng.integers(0, 256, (64, 6 - used, 32), dtype=np.uint8)
    if k == 2: dirty["args"][:, 1, 20:] = rng.integers(0, 256, (64, 12), dtype=np.uint8)
    if k in (1, 2): dirty["value_s"] = rng.integers(0, 1 << 64, 64, dtype=np.uint64)
    assert dirty.tobytes() != clean.tobytes() and br.same_arrays(e.ingest_records(clean, device=False), e.ingest_records(dirty, device=False))
    if k in (0, 3):                                                                          # ... and value_s is part of a mint / redeem statement
        other = clean.copy(); other["value_s"] ^= np.uint64(1); assert not br.same_arrays(e.ingest_records(clean, device=False)[1:2], e.ingest_records(other, device=False)[1:2])

def test_host_converter_strict_encoding(tmp_path):
    """ZK_STRICT_PROOF_ENCODING=1 (read once a process: a child): a coordinate of q or more is not a proof"""
    recs = np.concatenate([br.coordinate_records(1, 21, canonical=True), br.random_records(1, 50, 22), br.random_records(1, 50, 23, canonical=True)]); np.save(str(tmp_path / "recs.npy"), recs)
    child = ("import sys, numpy as np\nsys.path.insert(0, %r); sys.path.insert(0, %r)\nfrom blockmaze_amd import engine as e\nimport block_records as br\n"
             "recs = np.load(sys.argv[1]); items, inputs, parsed = e.ingest_records(recs, device=False); br.check_against_models(recs, items, inputs, parsed, strict=True)\n"
             "assert 0 < int(parsed.sum()) < len(recs); print('STRICT OK')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", child, str(tmp_path / "recs.npy")], capture_output=True, text=True, timeout=600, env=dict(os.environ, ZK_STRICT_PROOF_ENCODING="1"))
    assert r.returncode == 0 and "STRICT OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])

@pytest.mark.parametrize("n", [1, 2, 5000])
@pytest.mark.parametrize("weights", ["random", "ones", "max"])
def test_rlc_integer_sums_on_the_host(n, weights):
    """zkgpu_test_rlc_sums_host against Python integers: the exact sums of r_i and r_i x_ij over the records flagged 1, inputs up to r - 1, flags 0 / 1 / 2 mixed"""
    rng = random.Random(1000 * n + len(weights)); ni = 5
    ws = [rng.randrange(1, 1 << 128) if weights == "random" else 1 if weights == "ones" else (1 << 128) - 1 for _ in range(n)]
    xs = [[rng.choice([o.R_MOD - 1, 0, 1, rng.randrange(o.R_MOD), (1 << 253) - 1]) for _ in range(ni)] for _ in range(n)]
    fl = [1 if n <= 2 else rng.choice([0, 1, 1, 1, 2]) for _ in range(n)]
    if n == 2: fl[1] = 2
    arr = np.array([[[(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for x in row] for row in xs], dtype=np.uint64)
    got = e.rlc_sums_host(arr, ws, fl)
    want = [sum(r for r, f in zip(ws, fl) if f == 1)] + [sum(r * row[j] for r, row, f in zip(ws, xs, fl) if f == 1) for j in range(ni)]
    assert got == want and max(want) < (1 << 448)
    assert e.rlc_sums_host(arr, ws, [0] * n) == [0] * (ni + 1)
