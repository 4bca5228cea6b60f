"""Whole keys, element by element.  The other key tests see a proving key through sums weighted by a witness, where the point of a variable whose value is 0 (about half
of a BlockMaze witness, the structural zeros in every fixture) drops out.  Here every point the engine's generator writes is compared with the oracle's independent
generator on the same seven toxic values, on small circuits with real structure (+-1 and power-of-two coefficients, variables absent from A or B, equal columns, step
domains with a small part far smaller than the big one), and the loaded key proves their golden witnesses to the oracle's bytes under every key-load switch."""
import hashlib, json, os, subprocess, sys
import numpy as np
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
from r1cs_util import random_r1cs
import key_model as km

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R_MOD
UNPACKER_BITS = (832, 1024, 1440)                                                     # domains 1,024, 1,040 (step) and 1,536 (step)
GADGETS = ["lesscmp"] + ["unpacker%d" % b for b in UNPACKER_BITS]

def sparse_random_system(seed=90):
    """about 300 variables; some occur in no row of A, some in no row of B, some in no constraint at all (their term goes to another variable of the row)"""
    cs, _ = random_r1cs(seed, 4, 300, 340); no_a = set(range(10, 300, 13)); no_b = set(range(11, 300, 17)); nowhere = set(range(12, 300, 29)) | {300}
    banned = [no_a | nowhere, no_b | nowhere, nowhere]; rows_of = []
    for mtx in range(3):
        rp, cl, co = cs.rowptr[mtx], cs.col[mtx], o.from_arr(cs.coeff[mtx]); rows = {}
        for k in range(cs.n_cons):
            terms = {}
            for t in range(int(rp[k]), int(rp[k + 1])):
                c = int(cl[t]); c = 1 + (c * 7 + k) % 9 if c in banned[mtx] else c; terms[c] = (terms.get(c, 0) + co[t]) % R     # variables 1 .. 9 are in no banned set
            rows[k] = [(c, v) for c, v in terms.items() if v]
        rows_of.append(rows)
    out = o.R1CS(4, 300, 340, *km.csr(rows_of, 340)); used = [set(out.col[mtx].tolist()) for mtx in range(3)]
    assert not (used[0] & (no_a | nowhere)) and not (used[1] & (no_b | nowhere)) and not (used[2] & nowhere) and (no_a - nowhere) & used[1] and (no_b - nowhere) & used[0]
    return out

@pytest.fixture(scope="module")
def systems(tmp_path_factory, golden_dir):
    """name -> (path of the R1CS file, the system)"""
    t = tmp_path_factory.mktemp("systems"); out = {}
    for name in ("groth16_small", "groth16_step"): p = os.path.join(golden_dir, name, "r1cs.bin"); out[name] = (p, o.R1CS.load(p))
    p = str(t / "lesscmp.bin"); e.circuit_export("lesscmp", p); out["lesscmp"] = (p, o.R1CS.load(p))
    for b in UNPACKER_BITS: p = str(t / ("unpacker%d.bin" % b)); e.circuit_export("unpacker", p, b); out["unpacker%d" % b] = (p, o.R1CS.load(p))
    sp = sparse_random_system(); a, b = (sp.swapped(), sp) if sp.swap_ab_beneficial() else (sp, sp.swapped())       # a: A touches at least as many variables as B
    assert not a.swap_ab_beneficial() and b.swap_ab_beneficial()
    for name, cs in (("sparse300", a), ("sparse300 B wider", b)): p = str(t / (name.replace(" ", "_") + ".bin")); cs.save(p); out[name] = (p, cs)
    return out

KEYS = {}
def generated_key(systems, tmp_path_factory, name):
    """the engine's key files for a system, made once a module: (pk path, vk path, seed)"""
    if name not in KEYS:
        t = tmp_path_factory.mktemp("key"); seed = 1000 + len(KEYS); pk, vk = str(t / "pk.txt"), str(t / "vk.txt"); e.keygen_from_r1cs(systems[name][0], pk, vk, seed=seed); KEYS[name] = (pk, vk, seed)
    return KEYS[name]

def rows_of(cs):
    """every row of every matrix as a sorted list of (variable, coefficient)"""
    out = []
    for mtx in range(3):
        rp, cl, co = cs.rowptr[mtx], cs.col[mtx].tolist(), o.from_arr(cs.coeff[mtx]) if len(cs.col[mtx]) else []
        out.append([sorted(zip(cl[int(rp[k]):int(rp[k + 1])], co[int(rp[k]):int(rp[k + 1])])) for k in range(cs.n_cons)])
    return out

def assert_same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp); assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if got.ndim == 1: got, exp = got.reshape(-1, 1), exp.reshape(-1, 1)
    d = np.nonzero(np.any(got != exp, axis=1))[0]; assert not len(d), "%s: %d of %d elements differ, the first at %d" % (what, len(d), len(got), int(d[0]))

@pytest.mark.parametrize("name", ["groth16_small", "groth16_step", "lesscmp", "unpacker832", "unpacker1024", "unpacker1440", "sparse300", "sparse300 B wider"])
def test_generated_key_equals_the_oracles_element_by_element(systems, tmp_path_factory, name):
    cs = systems[name][1]; pk_path, vk_path, seed = generated_key(systems, tmp_path_factory, name); got_pk, got_cs = o.parse_pk(pk_path); got_vk = o.parse_vk(vk_path)
    g = o.SplitMix64(seed); pk, vk, used = o.setup(cs, [g.field() for _ in range(7)])                                # ToxicWaste::from_seed draws the same seven, in this order
    assert (used is not cs) == cs.swap_ab_beneficial()
    if name.startswith("sparse300"): assert cs.swap_ab_beneficial() == (name == "sparse300 B wider")
    if name.startswith("unpacker"): assert cs.domain_m == {832: 1024, 1024: 1040, 1440: 1536}[int(name[8:])]
    for what in ("head", "A", "B_idx", "B_g2", "B_g1", "H", "L"): assert_same(getattr(got_pk, what), getattr(pk, what), name + " pk." + what)
    for what in ("gt", "gamma_g2", "delta_g2", "IC"): assert_same(getattr(got_vk, what), getattr(vk, what), name + " vk." + what)
    assert len(pk.A) == cs.n_vars + 1 and len(pk.H) == cs.domain_m - 1 and len(pk.L) == cs.n_vars - cs.n_inputs and len(vk.IC) == cs.n_inputs + 1
    assert (got_cs.n_inputs, got_cs.n_vars, got_cs.n_cons) == (used.n_inputs, used.n_vars, used.n_cons) and rows_of(got_cs) == rows_of(used)      # the stored system, swap included

# ---- the loaded key ------------------------------------------------------------------------------------------------------------------------------------------------
def golden_witnesses(name, t):
    """the witness files of a gadget's golden cases, each checked against the hash of libsnark's assignment"""
    out = []
    if name == "lesscmp":
        for i, pr in enumerate(json.load(open(os.path.join(ROOT, "tests", "golden", "lesscmp_gadget.json")))["pairs"]):
            if not pr["satisfied"]: continue
            wp = str(t / ("lesscmp_%d.bin" % i)); e.witness_lesscmp(pr["value_old"], pr["value_s"], wp); assert hashlib.sha256(open(wp, "rb").read()).hexdigest() == pr["witness_sha256"]; out.append(wp)
    else:
        nbits = int(name[8:]); gold = json.load(open(os.path.join(ROOT, "tests", "golden", "unpacker_gadget.json")))["bits%d" % nbits]
        for seed in (5, 6):
            g = o.SplitMix64(seed); bits = [g.next() & 1 for _ in range(nbits)]; wp = str(t / ("%s_%d.bin" % (name, seed))); e.witness_unpacker(bits, wp)
            assert hashlib.sha256(open(wp, "rb").read()).hexdigest() == gold["seed%d" % seed]["witness_sha256"]; out.append(wp)
    return out

@pytest.fixture(scope="module")
def jobs(systems, tmp_path_factory):
    """[pk path, witness path, r, s] for every golden witness of the four gadgets, and the bytes the oracle's prover gives on the engine's key"""
    t = tmp_path_factory.mktemp("witnesses"); out, exp, by = [], [], {}; g = o.SplitMix64(4242)
    for name in GADGETS:
        pk_path, vk_path, _ = generated_key(systems, tmp_path_factory, name); pk, cs = o.parse_pk(pk_path); vk = o.parse_vk(vk_path)
        for wp in golden_witnesses(name, t):
            z = o.load_witness(wp); r, s = g.field() % R, g.field() % R; assert o.r1cs_is_satisfied(cs, z); words = o.prove(cs, z, pk, r, s); assert o.verify(vk, z[:cs.n_inputs], words)
            out.append([pk_path, wp, "%x" % r, "%x" % s]); exp.append(o.proof_hex(words)); by.setdefault(name, []).append(len(out) - 1)
    return out, exp, by

@pytest.mark.parametrize("name", GADGETS)
def test_loaded_key_proves_the_golden_witnesses_to_the_oracles_bytes(systems, tmp_path_factory, jobs, name):
    out, exp, by = jobs; pk_path, vk_path, _ = generated_key(systems, tmp_path_factory, name); p = e.Prover(pk_path); assert len(by[name]) == (6 if name == "lesscmp" else 2)
    for i in by[name]:
        _, wp, r, s = out[i]; z = o.load_witness(wp); got = p.prove(z, int(r, 16), int(s, 16)); assert got == exp[i], (name, wp)
        assert e.verify(vk_path, got, o.from_arr(z[:p.n_inputs]))
    p.close()

PROVE_CODE = """
import json, sys
sys.path.insert(0, %r)
from blockmaze_amd import engine as e
import numpy as np
def rd(p):
    b = open(p, 'rb').read(); n = int(np.frombuffer(b, dtype=np.uint64, count=1)[0]); return np.frombuffer(b, dtype=np.uint64, count=4 * n, offset=8).reshape(n, 4).copy()
out = []; provers = {}
for pk, wit, r, s in json.loads(sys.argv[1]):
    if pk not in provers: provers[pk] = e.Prover(pk)
    out.append(provers[pk].prove(rd(wit), int(r, 16), int(s, 16)))
for p in provers.values(): p.close()
print('PROOFS ' + json.dumps(out))
"""

@pytest.mark.parametrize("switch", ["ZK_H_LAGRANGE", "ZK_FOLD_C", "ZK_MERGE_EQUAL_COLUMNS"])
def test_key_load_switches_give_the_same_bytes(jobs, switch):
    """a fresh process a switch (each is read once): the H query as it is in the file, C transformed proof by proof, equal columns left apart"""
    out, exp, _ = jobs
    r = subprocess.run([sys.executable, "-c", PROVE_CODE % ROOT, json.dumps(out)], capture_output=True, text=True, env=dict(os.environ, **{switch: "0"}), timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("PROOFS ")]; assert line, r.stderr[-2000:]
    got = json.loads(line[0][7:]); assert len(got) == len(exp) == 12
    for i, (a, b) in enumerate(zip(got, exp)): assert a == b, (switch, out[i][:2])
