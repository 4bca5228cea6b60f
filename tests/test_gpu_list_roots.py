"""The roots of many commitment lists on the device (gpu_list_roots.hip; include/zk_roots.h): k_list_roots against the host model byte for byte at every
class boundary, in the long shape and on a block's worth of overlapping lists, with the launch counts pinned; genRoots against genRoot; and
verifyBlockRecordsRoots against verifyBlockRecords, the Python model of the root (tests/test_commitment_tree_cpu.py) and the header's rejection rules, on a small
block (the per-proof path) and on 8,192 records (the equation).  Device work runs in fresh child processes (tests/list_roots_child.py), one job each, under
a timeout; nothing is retried."""
import json, os, random, subprocess, sys
import numpy as np
import pytest
from blockmaze_amd import engine as e
import workload as w
from test_commitment_tree_cpu import model_levels, model_root, GOLDEN_ROOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "list_roots_child.py")
LONG = 262145   # 513 tiles of 512 leaves: the first pass leaves 513 nodes, one more than a window, so this is the smallest list that needs a second tiled pass

def in_child(tmp_path, op, arrays, timeout=300, env=None):
    job = str(tmp_path / ("job_%d.npz" % len(os.listdir(str(tmp_path))))); np.savez(job, **arrays)
    r = subprocess.run([sys.executable, CHILD, op, job], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]; assert r.returncode == 0 and line, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(line[0][7:])

def leaf_pool(n, seed): return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
def cases_job(cases):
    """cases: [(depth, hash_order, leaves (n, 32), [(first, count)])]"""
    job = {"n_cases": np.array(len(cases))}
    for k, (depth, hash_order, leaves, lists) in enumerate(cases):
        job["leaves_%d" % k] = leaves; job["lists_%d" % k] = np.array(lists, dtype=np.uint64).reshape(-1, 2); job["depth_%d" % k] = np.array(depth); job["hash_%d" % k] = np.array(bool(hash_order))
    return job
def ranges_for(counts, n_pool, rng):
    """a range of the pool for every count, at a random offset: the ranges overlap"""
    return [(rng.randrange(0, n_pool - c + 1), c) for c in counts]

def test_packed_shape_at_every_class_boundary(tmp_path):
    """depth 8: lists of 0 .. 256 leaves on both sides of every power of two, each length three times in shuffled order, in blob order and in hash order; depth 1
    (0, 1, 2 leaves), depth 2 (0 .. 4) and depth 32 (1, 3, 200: a lone-lane chain of 24 to 32 levels, where a wrong empty[k] index shows): the roots are the
    host model's, each at its caller's position, and no call takes more than 8 launches"""
    rng = random.Random(0xC1A55); pool = leaf_pool(700, 1)
    lengths = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256] * 3; rng.shuffle(lengths)
    cases = [(8, False, pool, ranges_for(lengths, 700, rng)), (8, True, pool, ranges_for(lengths, 700, rng))]
    for hash_order in (False, True):
        cases += [(1, hash_order, pool, ranges_for([0, 1, 2, 2, 1, 0], 700, rng)), (2, hash_order, pool, ranges_for([0, 1, 2, 3, 4, 4, 3], 700, rng)), (32, hash_order, pool, ranges_for([1, 3, 200], 700, rng))]
    res = in_child(tmp_path, "roots", cases_job(cases)); assert len(res) == len(cases)
    for r, c in zip(res, cases):
        assert r["differ"] == 0 and r["n"] == len(c[3]) and 1 <= r["launches"] <= 8, (c[0], c[1], r)
        assert r["distinct"] >= len(set(n for _, n in c[3])) - 1, r                                      # (the model's roots are not all one value)
    assert res[0]["launches"] == 8 and res[2]["launches"] == 1 and res[4]["launches"] == 3             # classes of 2, 4, ... 256 leaves; {0, 1, 2}; {1}, {3}, {200}

def test_long_shape(tmp_path):
    """depth 9 with 511 and 512 leaves (the widest packed list); depth 10 with 513, 1,023 and 1,024 (a ragged and a full second tile); depth 20 with one list of
    262,145 leaves — at most 3 launches — and that list beside lists of 0, 1 and 300 leaves; the last once more in hash order"""
    pool = leaf_pool(LONG + 7, 2)
    cases = [(9, False, pool[:600], [(5, 511), (60, 512)]), (10, False, pool[:1100], [(0, 513), (40, 1023), (70, 1024)]), (20, False, pool, [(3, LONG)]),
             (20, False, pool, [(9, 0), (3, LONG), (100, 1), (2000, 300)]), (20, True, pool, [(2000, 300), (0, LONG), (9, 0), (100, 1)])]
    res = in_child(tmp_path, "roots", cases_job(cases)); assert len(res) == len(cases)
    for r, c in zip(res, cases): assert r["differ"] == 0 and r["n"] == len(c[3]) and r["distinct"] == len(c[3]), (c[0], c[1], r)
    assert [r["launches"] for r in res] == [1, 2, 3, 5, 5], res    # 512: one class; 513 .. 1,024: a pass and the class of two nodes above it; 262,145: two passes and a class; beside {0, 1} and {300}

def test_a_blocks_worth_of_lists(tmp_path):
    """3,000 lists of 0 .. 256 leaves over a shared array of 40,000 leaves (the ranges overlap), depth 8, hash order: the model's roots, in at most 8 launches
    whatever the number of lists; and the 262,145-leaf list in at most 3"""
    rng = random.Random(0xB10C); pool = leaf_pool(40000, 3); lists = ranges_for([rng.randrange(0, 257) for _ in range(3000)], 40000, rng)
    res = in_child(tmp_path, "roots", cases_job([(8, True, pool, lists), (20, True, leaf_pool(LONG, 4), [(0, LONG)])]))
    assert res[0]["differ"] == 0 and res[0]["n"] == 3000 and res[0]["distinct"] > 2900 and res[0]["launches"] <= 8, res[0]
    assert res[1]["differ"] == 0 and res[1]["launches"] <= 3, res[1]

def test_genroots_equals_genroot(tmp_path):
    """50 seeded lists and the three golden cases: Zk.GenRoots at depth 8 = Zk.GenRT list by list"""
    rng = random.Random(0x6E4); sixteen = w.reference_deposit_fixture()["leaves"]; golden = [(1).to_bytes(32, "big")] + sixteen
    cmts = np.concatenate([np.frombuffer(b"".join(golden), dtype=np.uint8).reshape(-1, 32), leaf_pool(2000, 5)])
    lists = [(0, 0), (0, 1), (1, 16)] + [(17 + f, c) for f, c in ranges_for([rng.choice([0, 1, 2, 16, 255, 256, rng.randrange(0, 257)]) for _ in range(50)], 2000, rng)]
    res = in_child(tmp_path, "genroots", {"cmts": cmts, "lists": np.array(lists, dtype=np.uint64)})
    assert res["roots"] == res["rt"] and len(res["rt"]) == 53 and res["roots"][:3] == [GOLDEN_ROOTS[n] for n in (0, 1, 16)]

@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """keys made with seeds, and the proofs of the two block tests, from one child"""
    d = tmp_path_factory.mktemp("prfKey"); res = in_child(tmp_path_factory.mktemp("setup"), "setup", {"x": np.zeros(1)}, env={"ZK_PRFKEY_DIR": str(d)})
    deposits = [("deposit", x["proof"], [bytes.fromhex(a) for a in x["args"]], [bytes.fromhex(l) for l in x["leaves"]]) for x in res["deposits"]]
    return str(d), deposits, ("send", res["send"]["proof"], [bytes.fromhex(a) for a in res["send"]["args"]], 0)

class Lists:
    """the shared array of commitments (big-endian) and the ranges, as the test builds them; root(j) is the Python model's"""
    def __init__(self): self.cmts = []; self.ranges = []; self.cache = {}
    def add(self, leaves): self.ranges.append((len(self.cmts), len(leaves))); self.cmts += list(leaves); return len(self.ranges) - 1
    def again(self, j): self.ranges.append(self.ranges[j]); return len(self.ranges) - 1              # a coinciding range
    def root(self, j):
        f, c = self.ranges[j]; key = b"".join(self.cmts[f:f + c])
        if key not in self.cache: lv, em = model_levels([w.rev(x) for x in self.cmts[f:f + c]], 8); self.cache[key] = w.rev(model_root(lv, em, 8))
        return self.cache[key]
    def arrays(self): return np.frombuffer(b"".join(self.cmts), dtype=np.uint8).reshape(-1, 32), np.array(self.ranges, dtype=np.uint64).reshape(-1, 2)

def expected(items, list_of, L, plain):
    """record by record: verifyBlockRecords's verdict AND the header's rejection rules AND the Python model's root = the record's RT"""
    out = []
    for it, j, ok in zip(items, list_of, plain):
        if j != -1: ok = bool(ok) and 0 <= j < len(L.ranges) and it[0] == "deposit" and L.ranges[j][1] <= 256 and L.root(j) == it[2][0]
        out.append(int(bool(ok)))
    return out

def run_block(tmp_path, keys, items, list_of, L):
    cmts, ranges = L.arrays()
    res = in_child(tmp_path, "block", {"recs": e.records_from_items(items), "cmts": cmts, "lists": ranges, "list_of": np.array(list_of, dtype=np.int32)}, env={"ZK_PRFKEY_DIR": keys})
    want = expected(items, list_of, L, res["before"]["ok"])
    assert res["roots"]["ok"] == want and res["roots"]["rc"] == sum(want), [(i, items[i][0], list_of[i], res["before"]["ok"][i], res["roots"]["ok"][i], want[i]) for i in range(len(items)) if res["roots"]["ok"][i] != want[i]][:8]
    assert res["after"]["ok"] == res["before"]["ok"] and res["after"]["rc"] == res["before"]["rc"] == sum(res["before"]["ok"])   # the new entry leaves no state behind
    assert res["roots"]["moved"] == res["before"]["moved"] == res["after"]["moved"], res                 # decided by the equation, or per proof, exactly as verifyBlockRecords
    return res, want

def test_verify_block_records_roots_small_block(tmp_path, setup):
    """three valid deposit proofs over 16, 1 and 256 leaves: each with its own list, with a list that differs in one byte of one leaf, with two leaves swapped (the
    one-leaf list has no two leaves: its variant is the list itself and the model says so), with the last leaf dropped, and with no root check; list_of = n_lists
    and -2; a valid proof whose RT was changed to the root of another list, naming its own list and naming that other list (the proof rejects it); a wrong proof with
    a matching list; a list of 257 commitments; a valid send record without a check and naming list 0"""
    keys, deposits, send = setup; L = Lists(); items = []; list_of = []
    def rec(d, rt=None, proof=None): return ("deposit", proof or d[1], [rt or d[2][0]] + d[2][1:], 0)
    own = []
    for d in deposits:
        leaves = d[3]; n = len(leaves); one = list(leaves); one[n // 2] = bytes([leaves[n // 2][0] ^ 1]) + leaves[n // 2][1:]; sw = list(leaves); sw[0], sw[n - 1] = sw[n - 1], sw[0]
        own.append(L.add(leaves))
        for j in (own[-1], L.add(one), L.add(sw), L.add(leaves[:-1]), -1): items.append(rec(d)); list_of.append(j)
    long_list = L.add(deposits[2][3] + [bytes(32)]); n_lists = len(L.ranges)
    items += [rec(deposits[0]), rec(deposits[0])]; list_of += [n_lists, -2]
    other = L.root(own[1]); assert other == deposits[1][2][0] and other != deposits[0][2][0]             # (the model's root of a proof's own list is the RT it was made with)
    items += [rec(deposits[0], rt=other), rec(deposits[0], rt=other)]; list_of += [own[0], own[1]]
    items += [rec(deposits[0], proof=deposits[1][1]), rec(deposits[2]), send, send]; list_of += [own[0], long_list, -1, 0]
    res, want = run_block(tmp_path, keys, items, list_of, L)
    plain = res["before"]["ok"]; assert plain == [1] * 17 + [0, 0, 0, 1, 1, 1] and res["before"]["moved"] == [0, 0, 1]
    assert want == [1, 0, 0, 0, 1] + [1, 0, 1, 0, 1] + [1, 0, 0, 0, 1] + [0, 0] + [0, 0] + [0, 0, 1, 0]

def test_verify_block_records_roots_through_the_equation(tmp_path, setup):
    """8,192 deposit records, the three valid proofs in rotation, naming 100 lists (coinciding ranges and copies); six records name a list of other commitments:
    the equation decides, as it does for verifyBlockRecords; then two records get another proof's bytes as well: the equation fails and every record is decided one
    by one, as for verifyBlockRecords"""
    keys, deposits, send = setup; L = Lists(); n = 8192
    for p in range(3): L.add(deposits[p][3])
    for j in range(3, 97): L.again(j % 3)
    for j in range(97, 100): L.add(deposits[j % 3][3])
    assert len(L.ranges) == 100
    items = [("deposit", deposits[i % 3][1], deposits[i % 3][2], 0) for i in range(n)]; list_of = [(i % 3) + 3 * ((i // 3) % 33) for i in range(n)]; list_of[3 * 700] = 99
    wrong = (0, 255, 256, 4095, 8190, 8191)
    for i in wrong: list_of[i] = list_of[i] + 1 if list_of[i] < 99 else 1
    res, want = run_block(tmp_path, keys, items, list_of, L)
    assert res["before"]["moved"] == [1, 0, 0] and sum(res["before"]["ok"]) == n and want == [int(i not in wrong) for i in range(n)]
    bad_proof = (1000, 5000)
    for i in bad_proof: items[i] = ("deposit", deposits[(i + 1) % 3][1], deposits[i % 3][2], 0)
    res, want = run_block(tmp_path, keys, items, list_of, L)
    assert res["before"]["moved"] == [0, 1, 1] and want == [int(i not in wrong + bad_proof) for i in range(n)]
