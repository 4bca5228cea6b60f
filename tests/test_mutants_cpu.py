"""The seeded mutants of tests/mutants.py without a device: conditions on the inputs that tests/test_gpu_mutants.py hands to the device, checked against the models
(tests/tx_model.py, header_model.py, body_model.py) alone.  They show that the corpora are worth running: that they are a function of their seed, that neither verdict
crowds out the other, that every rule of the transaction decoder is reached, that the decodable mutants differ from their bases in length and in element count, and that
the lengths of the headers sweep the phases of the sponge's rate blocks and of the seal message's three seams.  Where a condition fails a mutator is missing or
misdirected: the conditions stay."""
import collections, os, re, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path: sys.path.insert(0, _p)
import tx_model as t
import header_model as hm
import header_corpus as hc
import body_model as bdm
import mutants as mu

NO_HASH = lambda msg: bytes(32)                                  # a transaction's status does not depend on its hashes

def message(raw):
    try: t.decode(raw); return None
    except t.Malformed as err: return str(err)

@pytest.fixture(scope="module")
def txs(): return mu.tx_mutants(mu.TX_SEED, mu.TX_COUNT)
@pytest.fixture(scope="module")
def bodies(): return mu.body_mutants(mu.BODY_SEED, mu.BODY_COUNT)
@pytest.fixture(scope="module")
def chains():
    """[(headers, the model's outputs)] a seed of HEADER_SEEDS"""
    out = []
    for seed in mu.HEADER_SEEDS: raws, parent, bases = mu.header_chains(seed); out.append((raws, hm.headers(raws, hc.PERIOD, hc.CHAIN_EPOCH, hc.NOW, parent)))
    return out

# ---- the walkers and the seeds ----------------------------------------------------------------------------------------------------------------------------------------
def test_items_and_fix_outer_on_a_valid_transaction_and_on_damage():
    label, raw, signer, chain_id = mu.valid_txs()[0]; tx, spans = t.decode(raw); its = mu.items(raw)
    assert its[0] == (0,) + t.read_head(raw, 0, len(raw)) and [x[0] for x in its[1:] if x[0] in {s for s, _ in spans}] == [s for s, _ in spans]   # depth-first: the outer list, then its 26 items in order
    assert len(its) == 1 + t.NFIELDS + len(tx["CMTBlock"]) and mu.items(raw, 0) == its[:1] and len(mu.items(raw, 1)) == 1 + t.NFIELDS
    assert mu.items(b"") == [] and mu.items(b"\xf8\x05" + bytes(5)) == [] and mu.items(raw[:-1]) == []                  # the first head is malformed: nothing, quietly
    assert mu.items(raw + b"\x05\x81")[:len(its)] == its and mu.items(raw + b"\x05\x81")[-1] == (len(raw), "byte", len(raw), 1)   # what stands behind the list is walked until a head is malformed
    for cut in (raw[:-1], raw + b"\x00", raw[:1] + raw[5:]): fixed = mu.fix_outer(cut); k, beg, size = t.read_head(fixed, 0, len(fixed)); assert k == "list" and beg + size == len(fixed) and fixed[beg:] == cut[3:]
    assert mu.fix_outer(b"") == b"" and mu.fix_outer(b"\x85abc") == b"\x85abc" and mu.fix_outer(b"\xf9\x01") == b"\xc0" and mu.fix_outer(b"\xc5\x01") == b"\xc1\x01"
    assert len(mu.EDGE) == 19 and set(mu.EDGE) >= {0x7F, 0x80, 0xB7, 0xB8, 0xBF, 0xC0, 0xF7, 0xF8}

def test_the_same_seed_gives_the_same_bytes_and_another_seed_other_bytes():
    for make in (lambda s: mu.tx_mutants(s, 200), lambda s: mu.body_mutants(s, 200), lambda s: mu.header_chains(s)[0]):
        assert make(5) == make(5) and make(5) != make(6)

def test_every_mutator_changes_its_input_and_m8_keeps_the_outer_list_whole():
    import random
    rng = random.Random(3); label, raw, signer, chain_id = mu.valid_txs()[3]; header = mu.header_chains(0)[2][8]
    for name, fn in mu.BLIND + (("M12", mu.m12), ("M14", mu.m14)):
        outs = [fn(rng, base) for base in (raw, header) for _ in range(20)]; assert sum(o not in (raw, header) for o in outs) >= 30, name
    for base in (raw, header):
        for _ in range(50):
            for fn in (mu.m8, mu.m10, mu.m13, mu.m14):
                out = fn(rng, base)
                try: k, beg, size = t.read_head(out, 0, len(out)); assert beg + size == len(out), fn.__name__      # repaired up to the outermost: the damage lies deeper
                except t.Malformed as err: assert fn is mu.m10 and "size" in str(err) or "56" in str(err), (fn.__name__, str(err))   # (M10 on the outer header itself)

# ---- transactions -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_transactions_reach_every_message_of_the_model_and_every_status(txs):
    source = open(os.path.join(ROOT, "tests", "tx_model.py")).read(); rules = set(re.findall(r'Malformed\("([^"]+)"\)', source)); assert len(rules) >= 21, rules
    wanted = {r for r in rules if "2^32" not in r}; assert len(wanted) == len(rules) - 1                          # (a transaction of 4 GiB is not made here)
    seen = collections.Counter(message(x[1]) for x in txs); n = len(txs); assert n == mu.TX_COUNT
    assert set(seen) - {None} <= wanted and all(seen[r] >= 3 for r in wanted), sorted((seen[r], r) for r in wanted)
    malformed = n - seen[None]; assert 5 * malformed >= n and 5 * seen[None] >= n, seen[None]
    status = collections.Counter(); longer = 0
    for label, raw, signer, chain_id, base in txs:
        if message(raw) is None: status[t.signing_inputs(raw, signer, chain_id, NO_HASH)["status"]] += 1; longer += len(raw) != len(base)
    assert set(status) == {t.OK, t.CHAIN_ID, t.SIG} and longer >= 50, (status, longer)
    print("transactions: %d mutants, %d decode, %d messages, the rarest %d times; statuses %s; %d decodable of another length; %d residues mod 136" %
          (n, seen[None], len(wanted), min(seen[r] for r in wanted), dict(status), longer, len({len(x[1]) % 136 for x in txs if message(x[1]) is None})))

# ---- headers ----------------------------------------------------------------------------------------------------------------------------------------------------------
def seams(raw):
    """the positions, in the seal hash's message, at which its pieces meet: the fields before Extra | Extra's fresh header | Extra less the seal | MixDigest and Nonce;
    from the model's spans (header_model.seal_hash, clique.go:147-169)"""
    h, spans, contents = hm.decode(raw); rest = h["Extra"][:-hm.SEAL_BYTES]; a_len = spans[hm.I_EXTRA - 1][1] - spans[0][0]; mid = len(t.enc_str(rest)) - len(rest)
    c_len = spans[hm.SEAL_FIELDS - 1][1] - spans[hm.I_EXTRA + 1][0]; pre = len(t.head(0xC0, a_len + mid + len(rest) + c_len)); items = hm.encode_items(h, hm.SEAL_FIELDS)
    assert a_len == len(b"".join(items[:hm.I_EXTRA])) and c_len == len(b"".join(items[hm.I_EXTRA + 1:]))
    return pre + a_len, pre + a_len + mid, pre + a_len + mid + len(rest)

def test_headers_reach_twelve_statuses_and_every_phase_of_the_blocks_and_seams(chains):
    status = collections.Counter(); residues = set(); phase = [collections.Counter() for _ in range(3)]; n = 0
    seen_raws = set()                                                                             # (a header that several chains hold counts once)
    for raws, outs in chains:
        for raw, o in zip(raws, outs):
            status[o["status"]] += 1; n += 1
            if o["status"] == hm.MALFORMED: continue
            residues.add(len(raw) % 136)
            if o["extra_size"] >= hm.SEAL_BYTES:
                for k, at in enumerate(seams(raw)): phase[k][at % 8] += raw not in seen_raws
                seen_raws.add(raw)
    assert n == 257 * len(mu.HEADER_SEEDS) == 3084
    assert 5 * status[hm.MALFORMED] >= n and 5 * (n - status[hm.MALFORMED]) >= n, status
    assert len(status) >= 12, status
    assert len(residues) >= 100, len(residues)
    assert all(set(p) == set(range(8)) and min(p.values()) >= 1 for p in phase), phase
    print("headers: %d, %s; %d residues mod 136; the rarest phase of each seam %s times" % (n, {hm.STATUS_NAMES[k]: v for k, v in sorted(status.items())}, len(residues), [min(p.values()) for p in phase]))

# ---- bodies -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_bodies_reach_the_three_statuses_and_other_element_counts(bodies):
    status = collections.Counter(); other = 0
    for raw, base in bodies:
        st, ext = bdm.split(raw); status[st] += 1; b_st, b_ext = bdm.split(base); assert b_st == bdm.OK
        if st == bdm.OK: other += len(ext) != len(b_ext)
    n = len(bodies); assert n == mu.BODY_COUNT and set(status) == {bdm.OK, bdm.MALFORMED, bdm.UNCLES}, status
    assert 5 * status[bdm.MALFORMED] >= n and 5 * (n - status[bdm.MALFORMED]) >= n and other >= 50, (status, other)
    print("bodies: %d, %s; %d accepted with another element count" % (n, dict(status), other))
