"""CPU companion of tests/test_gpu_field29.py: the input builders and the integer model of the 29-bit-limb arithmetic (tests/field29_model.py), without a device.
Every generated input keeps to the contract of the operation it is meant for (a device mismatch can never be blamed on an illegal input), every edge class occurs in
every operand position of every operation, the all-ceiling vectors and the tops of the value intervals are there, and the checkers reject wrong answers: a value off
by p, 2^29 moved between neighbouring limbs (same value, broken limb bound), a point off by a sign."""
import importlib.util, os, re, shutil, sys
import pytest
import field29_model as m

CASES = [(m.FQ, op) for op in m.OPS_FQ] + [(m.FR, op) for op in m.OPS_FR]
IDS = ["%s-%s" % ("Fq29" if f else "Fr29", op) for f, op in CASES]
N = 400

def rows(field, op):
    ins = m.inputs(field, op, N); return [[x[i] for x in ins] for i in range(len(ins[0]))] if ins else [[]] * 4

def test_constants_are_those_of_the_generated_file():
    """the moduli are the oracle's, and K_c / KL_2 — derived here from what their comments promise — are the limbs the committed file holds"""
    from oracle import pyoracle as o
    assert m.Q_MOD == o.Q_MOD and m.R_MOD == o.R_MOD
    src = open(os.path.join(m.CSRC, "field29_gfx950.inc")).read(); arr = lambda t: [int(x, 16) for x in re.findall(r"0x[0-9a-f]+", t)]
    for c in (2, 4, 6, 12, 18): assert arr(re.search(r" K%d\[9\] = \{([^}]*)\}" % c, src).group(1)) == m.K(c), c
    kl = re.findall(r" KL2\[9\] = \{([^}]*)\}", src); assert len(kl) == 2 and arr(kl[0]) == m.KL2(m.FQ) and arr(kl[1]) == m.KL2(m.FR)
    p29 = re.findall(r" P29\[9\] = \{([^}]*)\}", src); assert arr(p29[0]) == m.limbs29(m.Q_MOD) and arr(p29[1]) == m.limbs29(m.R_MOD)
    assert m.params()[2] == [m.limbs29(k * m.Q_MOD) for k in range(5)]

@pytest.mark.parametrize("field,op", CASES, ids=IDS)
def test_inputs_keep_to_the_contract_and_cover_the_edges(field, op):
    spec = m.contract(field, op); R = rows(field, op)
    for r in R: m.legal(field, op, r)
    for k, (ceil, edges, vmax, cap) in enumerate(spec):
        assert max(edges) == ceil                                                   # the ceiling is one of the classes
        for e in edges: assert any(e in r[k][:8] for r in R), (op, k, "edge class missing", e)
        if op != "unpack":   # a representative at the top of its value interval, and one with no top limb at all
            assert any(r[k][8] == m.top_limb(None, r[k][:8], vmax, cap, 1) for r in R) and any(r[k][8] == 0 for r in R), (op, k)
    if spec: assert any(all(r[k][:8] == [s[0]] * 8 for k, s in enumerate(spec)) for r in R), (op, "the all-ceiling vector")
    if op == "cond_neg": assert {r[1][0] for r in R} == {0, 1}
    if op == "product_is_zero": assert sum(m.model(field, op, *r)[0] for r in R) >= 2 and sum(1 - m.model(field, op, *r)[0] for r in R) >= 12
    if op == "barrett": assert sum(m.val(r[0]) % m.Q_MOD == 0 for r in R) >= 20

@pytest.mark.parametrize("field,op", CASES, ids=IDS)
def test_checker_takes_the_model_and_rejects_wrong_answers(field, op):
    p = m.MOD[field]; R = rows(field, op); rejected = {"off_by_p": 0, "limb_moved": 0, "one_bit": 0}
    for r in R[:60] + R[-40:]:
        right = m.model(field, op, *r); m.check(field, op, right, *r)
        wrong = []
        for k in range(0, len(right), 9):                                          # (ntt_lazy returns five elements)
            e = right[k:k + 9]
            if op not in ("unpack", "pack_words", "to_words", "product_is_zero"):
                wrong.append(("off_by_p", right[:k] + m.limbs29(m.val(e) + p) + right[k + 9:]))
                i = next((i for i in range(8) if e[i + 1] >= 1 and e[i] + (1 << m.B) < 1 << 32), None)
                if i is not None: w = list(e); w[i] += 1 << m.B; w[i + 1] -= 1; assert m.val(w) == m.val(e); wrong.append(("limb_moved", right[:k] + w + right[k + 9:]))
            w = list(e); w[0] ^= 1; wrong.append(("one_bit", right[:k] + w + right[k + 9:]))
        for name, w in wrong:
            with pytest.raises(AssertionError): m.check(field, op, w, *r)
            rejected[name] += 1
    assert rejected["one_bit"] and (rejected["off_by_p"] and rejected["limb_moved"] or op in ("unpack", "pack_words", "to_words", "product_is_zero"))

def test_value_checks_bite_without_the_limb_comparison():
    """the value identity and the limb bound are checks of their own: without the exact-limb comparison a result off by p still fails by its value, and one with
    2^29 moved to the neighbouring limb by its limb bound"""
    for field, op in ((m.FQ, "mul"), (m.FQ, "mul_kara"), (m.FQ, "mul2"), (m.FQ, "sqr"), (m.FQ, "sub2"), (m.FQ, "sub4"), (m.FQ, "sub18"), (m.FQ, "norm"), (m.FQ, "barrett"), (m.FR, "mul"), (m.FR, "sqr")):
        n_moved = 0
        for r in rows(field, op)[:60]:
            right = m.model(field, op, *r); m.check(field, op, right, *r, exact=False)
            with pytest.raises(AssertionError, match="value"): m.check(field, op, m.limbs29(m.val(right) + m.MOD[field]), *r, exact=False)
            i = next((i for i in range(8) if right[i] >= 8 and right[i + 1]), None)          # (a limb below 8 may take 2^29 and stay normalized)
            if i is not None:
                n_moved += 1; w = list(right); w[i] += 1 << m.B; w[i + 1] -= 1
                with pytest.raises(AssertionError, match="limb bound"): m.check(field, op, w, *r, exact=False)
        assert n_moved

def test_a_subtrahend_just_under_c_p_is_outside_the_contract():
    """why a subtrahend's contract is stated on its top limb, not as "value below c p": K_c lends 3 or 4 units of every limb to the one below (KL_2: 1 or 2), so its top
    limb is short of c p's, and for b = c p - 1 the top limb of a + K_c - b wraps below zero although the difference is 1.  The generator asserts the top-limb condition
    for every caller; the builders keep to it, and legal() turns such an operand down"""
    zero = [0] * 9
    for field in (m.FQ, m.FR):
        t = m.limbs29(2 * m.MOD[field] - 1); assert t[8] == m.KL2(field)[8] + 1 and m.model(field, "sub_product", zero, t)[8] == -1
        with pytest.raises(AssertionError, match="top limb"): m.legal(field, "sub_product", [zero, t])
        ok = m.limbs29((m.KL2(field)[8] + 1 << m.TOP) - 1); m.legal(field, "sub_product", [zero, ok]); m.check(field, "sub_product", m.model(field, "sub_product", zero, ok), zero, ok)
        assert m.val(ok) * 100 > 199 * m.MOD[field]                                 # (any value below 1.99 p keeps to it)
    for c in (2, 4, 6, 12, 18):
        b = m.limbs29(c * m.Q_MOD - 1); assert b[8] > m.K(c)[8] and m.val(m.sub_c(c, zero, b)) == (1 << 264) + 1
        with pytest.raises(AssertionError, match="top limb"): m.legal(m.FQ, "sub%d" % c, [zero, b])
        ok = m.limbs29((m.K(c)[8] + 1 << m.TOP) - 1); m.legal(m.FQ, "sub%d" % c, [zero, ok]); m.check(m.FQ, "sub%d" % c, m.sub_c(c, zero, ok), zero, ok)
        assert m.val(ok) * 100 > (100 * c - 1) * m.Q_MOD                            # (any value below (c - 0.01) p keeps to it)

def test_model_agrees_with_the_generator(tmp_path):
    """the products and the Barrett step of the model against the generator's own integer model of its column schedule, at the ceilings (the generator writes files
    next to itself: it runs from a copy)"""
    shutil.copy(os.path.join(m.CSRC, "gen_field29.py"), tmp_path / "gen_field29.py")
    spec = importlib.util.spec_from_file_location("gen_field29_copy", str(tmp_path / "gen_field29.py")); g = importlib.util.module_from_spec(spec)
    out = sys.stdout; sys.stdout = open(os.devnull, "w")
    try: spec.loader.exec_module(g)
    finally: sys.stdout.close(); sys.stdout = out
    assert g.Q == m.R_MOD                                                           # the module ends on the constants of Fr
    mulcols = [[("a%d" % i, "b%d" % (k - i)) for i in range(max(0, k - 8), min(k, 8) + 1)] for k in range(17)]
    for r in rows(m.FR, "mul")[:200]:
        env = {"a%d" % i: r[0][i] for i in range(9)}; env.update({"b%d" % i: r[1][i] for i in range(9)}); assert g.model_product(mulcols, env) == m.model(m.FR, "mul", *r)
    for r in rows(m.FQ, "barrett"): assert g.barrett(r[0])[0] == m.model(m.FQ, "barrett", *r)
    assert g.adjusted_light(2) == m.KL2(m.FR) and g.KS_SAVE == {c: m.K(c) for c in (2, 4, 6, 12, 18)}

# ---- points ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_g1_inputs_are_on_the_curve_within_the_invariant_and_cover_the_edges():
    A, Bq, exp = m.g1_madd_cases(96); seen = {"X": set(), "Y": set()}
    for i, (w, b) in enumerate(zip(A, Bq)):
        pt = m.g1_affine(w); assert m.g1_on_curve(pt); m.check_g1(w, pt)                                   # limbs normalized, X < 5.5 p, Y < 3.6 p, ZZ, ZZZ < 1.1 p
        assert (m.val(w[18:27]) * m.RINV) ** 3 % m.Q_MOD == (m.val(w[27:36]) * m.RINV) ** 2 % m.Q_MOD       # ZZ^3 = ZZZ^2
        seen["X"].update(w[0:8]); seen["Y"].update(w[9:17])
        x, y = m.val(b[0:9]), m.val(b[9:18]); assert x < m.Q_MOD and y < m.Q_MOD and max(b[:17]) <= m.M and b[18] in (0, 1)
        q = (x * m.RINV % m.Q_MOD, y * m.RINV % m.Q_MOD); assert m.g1_on_curve(q) and exp[i] is not None
    for c in "XY":
        assert set(m.EDGE_NORM) <= seen[c], (c, set(m.EDGE_NORM) - seen[c])
        assert any(w[9 * "XY".index(c):][:8] == [m.NORM] * 8 for w in A), "the all-ceiling coordinate"
    assert {b[18] for b in Bq} == {0, 1}
    assert set(m.EDGE_EXACT) <= set(sum((b[0:8] for b in Bq), [])) and set(m.EDGE_EXACT) <= set(sum((b[9:17] for b in Bq), []))
    # representatives up to the invariant's limit: X + 4 q, Y + 2 q
    assert max(m.val(w[0:9]) // m.Q_MOD for w in A) >= 4 and max(m.val(w[9:18]) // m.Q_MOD for w in A) >= 2

def test_pair_cases_put_every_kind_into_every_wave():
    kinds = {"plain", "a_inf", "b_inf", "both_inf", "opposite", "equal", "generator", "plain_top"}
    R = m.g1_pair_cases(64)
    for w in range(0, 64, 16): assert {r[0] for r in R[w:w + 16]} == kinds                                   # 16 quads a wave
    for kind, a, b, exp in R:
        for w in (a, b):
            if any(w): m.check_g1(w, m.g1_affine(w)); assert m.g1_on_curve(m.g1_affine(w))
        if kind == "opposite": assert m.g1_affine(b) == m.g1_neg(m.g1_affine(a)) and exp is None
        if kind in ("equal", "generator"): assert m.g1_affine(b) == m.g1_affine(a) and a != b and m.g1_on_curve(exp)
    R = m.g2_pair_cases(32)
    for w in range(0, 32, 8): assert {r[0] for r in R[w:w + 8]} == kinds - {"generator"}                    # 8 octets a wave
    for kind, a, b, exp in R:
        for c in (a, b):
            if any(any(l) for l in c): m.check_g2(c, m.g2_affine(c), m.G2_OCT_INV); assert m.g2_on_curve(m.g2_affine(c))
        if kind == "opposite": assert m.g2_affine(b) == m.g2_neg(m.g2_affine(a))
        if kind == "equal": assert m.g2_affine(b) == m.g2_affine(a)

def test_g2_and_fq2_inputs_keep_to_their_contracts():
    A, Bq, exp = m.g2_madd_cases(24)
    for c, b, e in zip(A, Bq, exp):
        m.check_g2(c, m.g2_affine(c), m.G2_LANE_INV); assert m.g2_on_curve(m.g2_affine(c)) and e is not None and len(b) == 37 and max(b[:8] + b[9:17] + b[18:26] + b[27:35]) <= m.M
        assert all(m.val(b[9 * k:9 * k + 9]) < m.Q_MOD for k in range(4))
    a, b = m.fq2_cases(200); cap = m.K(12)[8]
    for x in a + b:
        for comp in x: assert max(comp[:8]) <= m.NORM and m.val(comp) < m.FQ2_UNITS * m.Q_MOD and comp[8] <= cap
    for e in m.EDGE_NORM:
        for pos in range(2): assert any(e in x[pos][:8] for x in a) and any(e in x[pos][:8] for x in b)
    assert any(all(comp[:8] == [m.NORM] * 8 for comp in x + y) for x, y in zip(a, b))
    # the raw sums the Karatsuba product takes stay below 2^30 + 16, the two differences' subtrahends below their constants
    assert 2 * m.NORM <= m.KARA and 2 * (m.FQ2_UNITS ** 2 * m.Q_MOD // m.RP + 1) < 4

def test_point_checkers_reject_wrong_points():
    import random
    rnd = random.Random(3); A, Bq, exp = m.g1_madd_cases(16)
    for e in exp:
        good = m.g1_raw(rnd, e, 4, 2); m.check_g1(good, e)
        bad_sign = m.g1_raw(rnd, m.g1_neg(e), 0, 0); over = m.g1_raw(rnd, e, 6, 0); over_y = m.g1_raw(rnd, e, 0, 4)
        moved = list(good); i = next(i for i in range(8) if good[i] >= 8 and good[i + 1]); moved[i] += 1 << m.B; moved[i + 1] -= 1
        zz0 = good[:18] + m.limbs29(m.Q_MOD) + good[27:]
        for w in (bad_sign, over, over_y, moved, zz0):
            with pytest.raises(AssertionError): m.check_g1(w, e)
        with pytest.raises(AssertionError): m.check_g1(good, None)                                             # a point where ZZ = 0 (mod q) was due
        m.check_g1(zz0, None); m.check_g1(zz0, e, allow_zz0=True)
    A, Bq, exp = m.g2_madd_cases(8)
    for e in exp:
        good = m.g2_raw(rnd, e, 3, 3); m.check_g2(good, e, m.G2_LANE_INV)
        moved = [list(l) for l in good]; i = next(i for i in range(8) if good[3][i] >= 8 and good[3][i + 1]); moved[3][i] += 1 << m.B; moved[3][i + 1] -= 1
        for w in (m.g2_raw(rnd, m.g2_neg(e), 0, 0), m.g2_raw(rnd, e, 5, 0), moved):
            with pytest.raises(AssertionError): m.check_g2(w, e, m.G2_LANE_INV)
    a, b = m.fq2_cases(40)
    for x, y in zip(a, b):
        for yy in (y, None):
            good = m.fq2_mul_model(x, y) if yy is not None else m.fq2_sqr_model(x); m.check_fq2(good, x, yy)
            for h in range(2):
                off = [list(l) for l in good]; off[h] = m.norm([u + v for u, v in zip(good[h], m.limbs29(m.Q_MOD))])
                with pytest.raises(AssertionError): m.check_fq2(off, x, yy)                                     # the same residue, other limbs
                sign = [list(l) for l in good]; sign[h] = m.limbs29((-m.val(good[h])) % m.Q_MOD)
                if sign[h] != good[h]:
                    with pytest.raises(AssertionError): m.check_fq2(sign, x, yy)
