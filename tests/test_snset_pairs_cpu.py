"""Two keys a record without a device (include/zk_spent_pk.h, DESIGN.md "Two keys a record"): the sequential semantics as a Python dict model against the library's
host model (zkgpu_test_snset_host_pairs), and a Python restatement of the device's round rule (probe-minimum, wins, decide) against the same model — equal codes and
equal logs on every small batch and on seeded random ones, with the round counts the design states: one round without a conflict inside the batch, ceil(L / 2) for
the alternating chain of L records.  The new header compiles as C, declares exactly its two symbols, and libzkgpu.so — and nothing else — exports them."""
import ctypes, itertools, os, random, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
from test_snset_cpu import model_spend, universe

PAIRS_ENGINE = ["zkgpu_snset_spend_pairs", "zkgpu_test_snset_host_pairs", "zkgpu_test_snset_round_cap", "zkgpu_test_snset_rounds"]
PAIRS_DROPIN = ["zkSnSetSpendPairs", "verifyBlockState"]

@pytest.fixture(scope="module")
def e():
    from blockmaze_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        import __graft_entry__ as g; g.build()
    engine.lib(); return engine

def checked_keys(exempt, p):
    """the keys of a record that are checked and inserted, or None if its second key is the exempt key"""
    p = tuple(p or ())
    if len(p) == 2 and exempt is not None and p[1] == exempt: return None
    return [k for j, k in enumerate(p) if not (j == 0 and exempt is not None and k == exempt)]

def model_pairs(log, exempt, pairs, commit):
    """the sequential semantics of include/zkgpu.h on a Python list (the log) -> (codes, the log after the call)"""
    state = set(log); seen = set(); out = []; log = list(log)
    for p in pairs:
        ks = checked_keys(exempt, p)
        if ks is None or any(k in state for k in ks): out.append(1)
        elif any(k in seen for k in ks) or (len(ks) == 2 and ks[0] == ks[1]): out.append(2)
        else:
            out.append(0); seen.update(ks)
            if commit: log.extend(ks)
    return out, log

LIVE, ACCEPTED, REJECTED = 0, 1, 2
def rounds_pairs(log, exempt, pairs, commit, cap=None):
    """the device's rounds restated: entry 2i + j is key j of record i.  Probe: a key's slot ends at the lowest entry among the claimants that are not rejected, or at
    the resident entry.  Wins: a live record with a resident key is rejected with code 1, one whose entries all hold their slots is accepted.  Decide: a live record
    that lost a slot to an accepted record or to its own other entry is rejected with code 2; one that lost only to records that did not win stays live.  After
    `cap` rounds the live records are walked in order against the keys of the accepted ones -> (codes, the log after the call, rounds)"""
    state = set(log); n = len(pairs); status = [LIVE] * n; code = [0] * n; entries = {}
    for i, p in enumerate(pairs):
        ks = checked_keys(exempt, p)
        if ks is None: status[i] = REJECTED; code[i] = 1; continue
        p = tuple(p or ()); entries[i] = [(2 * i + j, k) for j, k in enumerate(p) if not (j == 0 and exempt is not None and k == exempt)]
    rounds = 0
    while True:
        rounds += 1; slot = {}
        for i in range(n):
            if status[i] != REJECTED:
                for en, k in entries[i]:
                    if k not in state: slot[k] = min(slot.get(k, en), en)
        win = [False] * n
        for i in range(n):
            if status[i] == LIVE:
                if any(k in state for en, k in entries[i]): status[i] = REJECTED; code[i] = 1
                elif all(slot[k] == en for en, k in entries[i]): status[i] = ACCEPTED
            win[i] = status[i] == ACCEPTED
        live = 0
        for i in range(n):
            if status[i] == LIVE:
                holders = [slot[k] >> 1 for en, k in entries[i] if slot[k] != en]
                if any(h == i or win[h] for h in holders): status[i] = REJECTED; code[i] = 2
                else: live += 1
        if not live: break
        if cap is not None and rounds >= cap:
            taken = set(k for i in range(n) if status[i] == ACCEPTED for en, k in entries[i])
            for i in range(n):
                if status[i] == LIVE:
                    ks = [k for en, k in entries[i]]
                    if any(k in taken for k in ks) or (len(ks) == 2 and ks[0] == ks[1]): status[i] = REJECTED; code[i] = 2
                    else: status[i] = ACCEPTED; taken.update(ks)
            break
    out = list(log)
    if commit:
        for i in range(n):
            if status[i] == ACCEPTED: out.extend(k for en, k in entries[i])
    return code, out, rounds

def chain(L, U):
    """(s1, p1), (s1, p2), (s3, p2), (s3, p4), ...: every record is a valid deposit that shares one key with its neighbour -> the pairs"""
    return [(U[2 * (i // 2 * 2)], U[2 * ((i + 1) // 2 * 2) + 1]) for i in range(L)]

def small_batches():
    K = [bytes([c]) * 20 for c in b"ABC"]; rec = [None] + [(a,) for a in K] + [(a, b) for a in K for b in K]; assert len(rec) == 13
    for r in range(4):
        for batch in itertools.product(rec, repeat=r):
            for resident in ([], K[:1], K[:2]):
                for exempt in (None, K[2]): yield resident, exempt, list(batch)

def random_batches(count, seed):
    rng = random.Random(seed)
    for t in range(count):
        U = universe(rng.choice([3, 6, 12, 40]), 1000 + t); exempt = U[0] if rng.random() < 0.5 else None; pool = [k for k in U if k != exempt]
        resident = rng.sample(pool, rng.randrange(0, max(1, len(pool) // 2))); n = rng.randrange(0, 65)
        yield resident, exempt, [None if r < 0.1 else (rng.choice(U),) if r < 0.45 else (rng.choice(U), rng.choice(U)) for r in (rng.random() for _ in range(n))]

def test_host_model_equals_the_dict_model_on_every_small_batch(e):
    cases = 0; codes = set()
    for resident, exempt, batch in small_batches():
        commit = cases % 2 == 0; want, log = model_pairs(resident, exempt, batch, commit); got, app = e.snset_host_pairs(resident, exempt, batch, commit)
        assert got == want and app == log[len(resident):], (resident, exempt, batch); cases += 1; codes |= set(want)
    assert cases == 6 * (1 + 13 + 13 ** 2 + 13 ** 3) and codes == {0, 1, 2}
    A, B, C = (bytes([c]) * 20 for c in b"ABC")
    assert e.snset_host_pairs([], C, [(C, A), (C,), (B, C), (A, A), (B, B), (B,)]) == ([0, 0, 1, 2, 2, 0], [A, B])   # exempt first: skipped, k2 counts; exempt second: rejected; k1 == k2
    assert e.snset_host_pairs([A], None, [(B, A), (B, C), (C, B), (C,)]) == ([1, 0, 2, 2], [B, C])                    # a rejected record inserts nothing; an accepted one both keys

def test_host_model_equals_the_dict_model_on_random_batches(e):
    for t, (resident, exempt, batch) in enumerate(random_batches(3000, 5)):
        commit = t % 3 != 0; want, log = model_pairs(resident, exempt, batch, commit); got, app = e.snset_host_pairs(resident, exempt, batch, commit)
        assert got == want and app == log[len(resident):], t

def test_round_rule_equals_the_sequential_model():
    most = 0
    for resident, exempt, batch in itertools.chain(small_batches(), random_batches(3000, 6)):
        want, log = model_pairs(resident, exempt, batch, True); got, out, rounds = rounds_pairs(resident, exempt, batch, True); most = max(most, rounds)
        assert (got, out) == (want, log), (resident, exempt, batch)
        assert rounds_pairs(resident, exempt, batch, True, cap=1)[:2] == (want, log)                      # the host finish after one round gives the same
    assert most >= 3, most                                                                              # (batches that need several rounds are among them)

def test_round_counts_chain_no_conflict_and_single_key(e):
    U = universe(200, 9)
    for L in (2, 3, 4, 12, 13):
        c = chain(L, U); assert all(len(set(c[i]) & set(c[i + 1])) == 1 for i in range(L - 1)) and len(set(c)) == L
        want, log = model_pairs([], None, c, True); assert want == [i % 2 * 2 for i in range(L)]              # every other deposit goes
        assert rounds_pairs([], None, c, True) == (want, log, (L + 1) // 2), L
        assert rounds_pairs([], None, c, True, cap=2)[:2] == (want, log) and e.snset_host_pairs([], None, c) == (want, log)
    free = [(U[2 * i], U[2 * i + 1]) if i % 2 else (U[2 * i],) for i in range(50)]; assert rounds_pairs(U[150:199], U[199], free, True) == ([0] * 50, U[150:199] + [k for p in free for k in p], 1)
    assert rounds_pairs(U[:3], None, [(U[0], U[10]), (U[10], U[11]), (U[11],)], True) == ([1, 0, 2], U[:3] + [U[10], U[11]], 2)   # rejected for a resident key: its other key is free again
    rng = random.Random(10)
    for t in range(300):
        keys = [rng.choice(U[:12]) for _ in range(rng.randrange(1, 40))]; mask = [rng.random() < 0.8 for _ in keys]; resident = U[:rng.randrange(0, 5)]; exempt = U[5] if t % 2 else None
        pairs = [(k,) if m else None for k, m in zip(keys, mask)]; want = model_spend(resident, exempt, keys, mask, True)
        assert model_pairs(resident, exempt, pairs, True) == want and rounds_pairs(resident, exempt, pairs, True)[:2] == want
        got, app = e.snset_host_pairs(resident, exempt, pairs); assert (got, resident + app) == want and (got, app) == e.snset_host(resident, exempt, keys, mask)

def defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l)

def test_pairs_symbols_exported_by_libzkgpu_only(e):
    L = e.lib()
    for s in PAIRS_ENGINE + PAIRS_DROPIN: getattr(L, s)                                                   # (AttributeError: the symbol is not there)
    have = defined(e.LIB_PATH)
    for s in PAIRS_ENGINE + PAIRS_DROPIN: assert s in have, s
    from test_abi_exports import SYMS
    from test_block_records_cpu import declared_symbols
    assert sorted(declared_symbols("zk_spent_pk.h")) == sorted(PAIRS_DROPIN)
    for s in PAIRS_ENGINE: assert s in declared_symbols("zkgpu.h"), s
    assert not set(declared_symbols("zk_spent.h")) & set(PAIRS_DROPIN) and "zk_spent_pk.h" in open(os.path.join(ROOT, "include", "zk_spent.h")).read()
    for lib in SYMS: assert not set(defined(os.path.join(ROOT, "blockmaze_amd", "lib", "lib%s.so" % lib))) & set(PAIRS_ENGINE + PAIRS_DROPIN), lib

@pytest.mark.parametrize("compiler,lang,std", [("gcc", "c", "-std=c11"), ("g++", "c++", "-std=c++11")])
def test_pairs_header_compiles_as_c_and_cxx_when_included_twice(tmp_path, compiler, lang, std):
    src = tmp_path / ("t." + ("c" if lang == "c" else "cpp"))
    src.write_text('#include "zk_spent_pk.h"\n#include "zk_spent_pk.h"\n'
                   'int main(void) { uint8_t sn[64] = {0}, pk[64] = {0}; unsigned char out[2]; long long size = 0; zk_snset *s = zkSnSetNew(sn);\n'
                   '  if (s) { (void)zkSnSetSpendPairs(s, sn, pk, 2, 1, out); (void)verifyBlockState(0, 0, 0, 0, 0, s, 0, out, &size); zkSnSetFree(s); } return 0; }\n')
    subprocess.check_call([compiler, "-x", lang, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])

def test_host_model_argument_errors_write_nothing(e):
    L = e.lib(); U = universe(4, 3); keys = b"".join(U); fill = bytes(range(9, 9 + 80)); out = ctypes.create_string_buffer(fill[:2], 2); app = ctypes.create_string_buffer(fill, 80); na = ctypes.c_size_t(77)
    z = ctypes.c_size_t; nk = bytes([2, 2])
    bad = [L.zkgpu_test_snset_host_pairs(None, z(2), None, keys, nk, z(2), 1, out, app, ctypes.byref(na)), L.zkgpu_test_snset_host_pairs(None, z(0), None, None, nk, z(2), 1, out, app, ctypes.byref(na)),
           L.zkgpu_test_snset_host_pairs(None, z(0), None, keys, None, z(2), 1, out, app, ctypes.byref(na)), L.zkgpu_test_snset_host_pairs(None, z(0), None, keys, nk, z(2), 1, None, app, ctypes.byref(na)),
           L.zkgpu_test_snset_host_pairs(None, z(0), None, keys, nk, z(2), 1, out, None, ctypes.byref(na)), L.zkgpu_test_snset_host_pairs(None, z(0), None, keys, nk, z(2), 1, out, app, None),
           L.zkgpu_test_snset_host_pairs(None, z(0), None, keys, bytes([2, 3]), z(2), 1, out, app, ctypes.byref(na)), L.zkgpu_test_snset_rounds(None, None)]
    assert bad == [-2] * len(bad) and out.raw == fill[:2] and app.raw == fill and na.value == 77
    assert L.zkgpu_test_snset_host_pairs(None, z(0), None, keys, nk, z(2), 0, out, None, ctypes.byref(na)) == 0 and na.value == 0 and out.raw == bytes(2)   # check-only needs no room for keys
    r, h = e.snset_rounds(); assert r >= h >= 0
