"""The emitted HIP of the arithmetic on nine 29-bit limbs (field29_gfx950.inc: Fq29, Fr29) and the point formulas built on it (msm.cuh, htail29.cuh, oct29.cuh) against
big-integer arithmetic, limb for limb, at the bounds of every operand's contract.  The probes (csrc/probe29.hip) move raw limbs: nothing is normalized on the way, so
the device gets operands with limbs at 0, 2^29 - 1, 2^29 + 7 and at each wide operand's ceiling, values at the top of their intervals, and the all-ceiling vectors the
generator calls "the column bound at its worst".  Every comparison is exact; tests/test_field29_model_cpu.py shows that every input is legal and that the checkers
bite.  This is the gate for a change to gen_field29.py or to a caller's operand sizes."""
import numpy as np
import pytest
from blockmaze_amd import engine as e
import field29_model as m

pytestmark = pytest.mark.gpu
N = 3000

def arr(rows): return np.array(rows, dtype=np.uint64).astype(np.uint32)

@pytest.mark.parametrize("field,op", [(m.FQ, op) for op in m.OPS_FQ] + [(m.FR, op) for op in m.OPS_FR],
                         ids=["%s-%s" % (f, op) for f, ops in (("Fq29", m.OPS_FQ), ("Fr29", m.OPS_FR)) for op in ops])
def test_field_ops_match_the_integer_model(field, op):
    ins = m.inputs(field, op, N); dev = [arr(x) for x in ins] if ins else [np.zeros((4, 9), dtype=np.uint32)]
    got = e.field29_op(field, m.device_op(op), *dev); assert len(got) == (len(ins[0]) if ins else 4)
    for i, g in enumerate(got.tolist()): m.check(field, op, g, *[x[i] for x in ins])

def zz_is_zero(w): return m.val(w[18:27]) % m.Q_MOD == 0

@pytest.mark.parametrize("op", ["madd", "madd_pp"])
def test_g1_mixed_addition(op):
    """madd_head + madd_tail / madd_tail_pp on accumulators with edge limbs at the top of the invariant; the affine y canonical and as the wide K_2 - y"""
    A, Bq, exp = m.g1_madd_cases(256); out, flags = e.point29_op(op, arr(A), arr(Bq))
    for w, x, f in zip(out.tolist(), exp, flags.tolist()): m.check_g1(w, x); assert f == 0
    if op == "madd_pp":
        # the operand equal to +-the accumulator: P^2 = 0 (and R^2 = 0 for the equal one) is what k_wacc_lanes29 looks at before the tail; the tail leaves ZZ = 0 (mod q)
        import random
        rnd = random.Random(9); acc = m.g1_accs(32, 21); ops = []; want = []
        for i, (w, pt) in enumerate(acc):
            s = rnd.randrange(2); y = pt[1] if i & 1 else m.Q_MOD - pt[1]                     # the point added: pt for odd i, -pt for even i
            ops.append(m.rep(pt[0] * m.RP, 0) + m.rep((m.Q_MOD - y if s else y) * m.RP, 0) + [s]); want.append(3 if i & 1 else 1)
        out, flags = e.point29_op(op, arr([a[0] for a in acc]), arr(ops)); assert flags.tolist() == want and all(zz_is_zero(w) for w in out.tolist())

def test_g1_doubling_of_an_affine_point():
    Bq, exp = m.g1_dbl_cases(256); out, _ = e.point29_op("dbl_affine", None, arr(Bq))
    for w, x in zip(out.tolist(), exp): m.check_g1(w, x)

def test_g1_general_addition():
    R = m.g1_pair_cases(256, infinity=False); out, flags = e.point29_op("add", arr([r[1] for r in R]), arr([r[2] for r in R]))
    for (kind, a, b, x), w, f in zip(R, out.tolist(), flags.tolist()):
        if kind in ("opposite", "equal", "generator"): assert zz_is_zero(w) and f == 2, kind          # what k_hacc_combine29 looks for
        else: m.check_g1(w, x); assert f == 0

@pytest.mark.parametrize("op", ["quad_add", "quad_add_opp"])
def test_g1_quad_cooperative_addition(op):
    """full waves in which every quad holds a different case: plain sums, either or both operands at infinity, B = -A, B = A, A = B = +-G"""
    R = m.g1_pair_cases(256, seed=31 if op == "quad_add" else 37); out, flags = e.point29_op(op, arr([r[1] for r in R]), arr([r[2] for r in R]))
    for (kind, a, b, x), w, f in zip(R, out.tolist(), flags.tolist()):
        if kind == "both_inf": assert f == 1
        elif kind == "a_inf": assert f == 0 and w == b
        elif kind == "b_inf": assert f == 0 and w == a
        elif kind in ("plain", "plain_top"): assert f == 0; m.check_g1(w, x)
        elif op == "quad_add": assert f == 0 and zz_is_zero(w), kind                                  # the incomplete form: ZZ = 0 (mod q) is what k_hbits29 looks for
        elif kind == "opposite": assert f == 1
        elif kind == "equal": assert f == 0; m.check_g1(w, x)                                         # by way of the generator: 2 A
        else: assert f == 0; m.check_g1(w, x, allow_zz0=True)                                         # A = B = +-G: the right point or ZZ = 0 (mod q), never a wrong one

def test_g1_run_of_mixed_additions_keeps_the_invariant():
    """one accumulator through 32 mixed additions, as a run of k_hacc_runs29: the right sum and the invariant after every step"""
    A, Bq, exp = m.g1_chain_cases(48); out, _ = e.point29_op("madd_chain", arr(A), arr(Bq)); out = out.reshape(-1, 36).tolist(); assert len(out) == len(exp)
    for w, x in zip(out, exp): m.check_g1(w, x)

def test_fq2_products():
    a, b = m.fq2_cases(1000); A = arr([x[0] + x[1] for x in a]); Bv = arr([x[0] + x[1] for x in b])
    mul, _ = e.point29_op("fq2_mul", A, Bv); sqr, _ = e.point29_op("fq2_sqr", A)
    for x, y, g, s in zip(a, b, mul.tolist(), sqr.tolist()): m.check_fq2([g[:9], g[9:]], x, y); m.check_fq2([s[:9], s[9:]], x)

def test_g2_mixed_addition():
    A, Bq, exp = m.g2_madd_cases(200); out, _ = e.point29_op("g2_madd", arr([m.lane_words(c) for c in A]), arr(Bq))
    for w, x in zip(out.tolist(), exp): m.check_g2(m.lane_lists(w), x, m.G2_LANE_INV)

def test_g2_oct_cooperative_addition():
    """full waves in which every group of eight lanes holds a different case"""
    R = m.g2_pair_cases(192); out, flags = e.point29_op("oct_add", arr([m.oct_words(r[1]) for r in R]), arr([m.oct_words(r[2]) for r in R]))
    for (kind, a, b, x), w, f in zip(R, out.tolist(), flags.tolist()):
        c = m.oct_lists(w)
        if kind == "both_inf": assert f == 1
        elif kind == "a_inf": assert f == 0 and c == b
        elif kind == "b_inf": assert f == 0 and c == a
        elif kind in ("plain", "plain_top"): assert f == 0; m.check_g2(c, x, m.G2_OCT_INV)
        else: assert f == 0 and m.val(c[4]) % m.Q_MOD == 0 and m.val(c[5]) % m.Q_MOD == 0, kind        # ZZ = 0 (mod q): what k_wtail_g2_29 looks for
