"""Integer model, input builders and checkers for the arithmetic on nine 29-bit limbs (blockmaze_amd/csrc/field29_gfx950.inc: Fq29, Fr29) and the point formulas
built on it.  Shared by tests/test_field29_model_cpu.py (the builders keep to every operation's contract, cover the edge classes, and the checkers reject wrong
answers) and tests/test_gpu_field29.py (the device's limbs against this model).

Expected values come from big integers, never from the generator's column schedule:
  val(l) = sum l[i] 2^(29 i);  p = q for Fq29, r for Fr29;  R' = 2^261
  product of A = val(a) val(b) (+ val(c) val(d)): limbs 0..7 are the 29-bit digits, limb 8 the rest, of (A + m p) / R' with m = -A p^-1 mod R'
  differences: val(out) = val(a) + c p - val(b) exactly, limbs 0..7 below 2^29 + 8 after a carry step
The contracts are the generator's (gen_field29.py): which operand may be how wide, which value bound each operand keeps.  A subtrahend's contract is stated on its
TOP LIMB (at most the constant's, which any value below (c - 0.01) p satisfies): the constant K_c = c p lends 3 or 4 units of every limb to the one below, so its top
limb is a few units short of c p's."""
import functools, os, random, re
from fractions import Fraction

B = 29; M = (1 << B) - 1; NL = 9; RP = 1 << (B * NL); TOP = B * (NL - 1)
Q_MOD = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FR, FQ = 0, 1
MOD = {FR: R_MOD, FQ: Q_MOD}
WIDE = int(2 ** 31.4)                       # the one wide operand of a product
NORM = (1 << B) + 7                         # a normalized limb's ceiling (below 2^29 + 8)
KARA = (1 << 30) + 15                       # both operands of fq2_29_mul's Karatsuba product (below 2^30 + 16)
DUAL = (1 << 30) + 8                        # a and c of mul2
SUBT = 3 * ((1 << B) + 8) - 1               # a subtrahend of sub<C>
LAZY1 = NORM + (1 << 30) + 64               # a normalized limb after one butterfly stage without a carry step
EDGE_EXACT = [0, 1, 7, 8, 1 << 28, M]
EDGE_NORM = EDGE_EXACT + [1 << B, NORM]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blockmaze_amd", "csrc")

def val(l): return sum(int(v) << (B * i) for i, v in enumerate(l))
def limbs29(x):
    assert x >= 0; return [(x >> (B * i)) & M for i in range(NL - 1)] + [x >> TOP]
def units(x, p): return Fraction(x) * p                                          # x p for a decimal x such as "5.5"
def bound(x, p): return int(Fraction(x) * p)
def spread(p, c, lo, hi):
    """c p with limbs 0..7 in [lo, hi), hi - lo <= 2^29: the one way to write it so (what K_c and KL_2 are, by their comments)"""
    rest = c * p; l = []
    for i in range(NL - 1):
        v = rest & M
        while v < lo: v += 1 << B
        assert v < hi; l.append(v); rest = (rest - v) >> B
    assert rest > 0; l.append(rest); assert val(l) == c * p; return l
@functools.lru_cache(None)
def _K(c): return tuple(spread(Q_MOD, c, 3 * (1 << B) + 64, 4 << B))
def K(c): return list(_K(c))
@functools.lru_cache(None)
def _KL2(field): return tuple(spread(MOD[field], 2, (1 << B) + 64, (2 << B) + 64))
def KL2(field): return list(_KL2(field))
@functools.lru_cache(None)
def params():
    """MU, MU_SHIFT and KP of the Barrett step, from the generated header (data, as the device code reads them)"""
    src = open(os.path.join(CSRC, "field29_params.h")).read()
    mu = int(re.search(r"\bMU = (0x[0-9a-f]+)u", src).group(1), 16); sh = int(re.search(r"\bMU_SHIFT = (\d+)", src).group(1))
    kp = re.search(r"KP\[5\]\[9\] = \{(.*)\};", src).group(1); kp = [[int(x, 16) for x in re.findall(r"0x[0-9a-f]+", row)] for row in re.findall(r"\{([^{}]*)\}", kp)]
    assert len(kp) == 5 and all(len(r) == 9 for r in kp); return mu, sh, kp

# ---- the model: one element at a time, lists of nine integers --------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _pinv(p): return pow(p, -1, RP)
def product(p, A):
    m = (-A * _pinv(p)) % RP; t = A + m * p; assert t % RP == 0; return limbs29(t >> (B * NL))
def norm(l): return [l[0] & M] + [(l[i] & M) + (l[i - 1] >> B) for i in range(1, 8)] + [(l[8] + (l[7] >> B)) & 0xffffffff]
def sub_c(c, a, b): return norm([(x + k - y) & 0xffffffff for x, k, y in zip(a, K(c), b)])
def unpack(w):
    v = sum(int(x) << (32 * j) for j, x in enumerate(w[:8])); return limbs29(v)
def words(v): return [(v >> (32 * j)) & 0xffffffff for j in range(8)] + [0]
def barrett(l):
    mu, sh, _ = params(); q = (l[8] * mu) >> sh; q = q - 1 if q else 0; npl = limbs29((1 << 264) - Q_MOD)
    acc = [l[i] + q * npl[i] for i in range(9)]
    t = [acc[0] & M] + [(acc[i] & M) + (acc[i - 1] >> B) for i in range(1, 8)] + [(acc[8] + (acc[7] >> B)) & 0xffffffff]
    return norm(t), q

OPS_FQ = ["mul", "mul_kara", "mul2", "sqr", "norm", "sub2", "sub4", "sub6", "sub12", "sub18", "cond_neg", "sub_product", "neg_product", "add_raw", "barrett", "one", "unpack",
          "pack_words", "to_words", "product_is_zero"]
OPS_FR = ["mul", "sqr", "norm", "sub_product", "neg_product", "add_raw", "unpack", "pack_words", "to_words", "ntt_lazy"]
def device_op(op): return "mul" if op == "mul_kara" else op                     # (the Karatsuba product is Fq29::mul with both operands wide)

def model(field, op, a=None, b=None, c=None, d=None):
    """the limbs the device must return (a list of 9, or 45 for ntt_lazy)"""
    p = MOD[field]
    if op in ("mul", "mul_kara"): return product(p, val(a) * val(b))
    if op == "mul2": return product(p, val(a) * val(b) + val(c) * val(d))
    if op == "sqr": return product(p, val(a) ** 2)
    if op == "norm": return norm(a)
    if op.startswith("sub") and op[3:].isdigit(): return sub_c(int(op[3:]), a, b)
    if op == "cond_neg": return [k - x for k, x in zip(K(2), a)] if b[0] & 1 else list(a)
    if op == "sub_product": return [x + k - y for x, k, y in zip(a, KL2(field), b)]
    if op == "neg_product": return [k - y for k, y in zip(KL2(field), a)]
    if op == "add_raw": return [x + y for x, y in zip(a, b)]
    if op == "barrett": return barrett(a)[0]
    if op == "one": return limbs29(RP % p)
    if op == "unpack": return unpack(a)
    if op == "pack_words": return words(val(a))
    if op == "to_words": return words(val(product(p, val(a) * ((1 << 256) % p))))
    if op == "product_is_zero": return [1 if val(a) % p == 0 else 0] + [0] * 8
    if op == "ntt_lazy":
        kl = KL2(field); dd = [x + 2 * k - y - z for x, k, y, z in zip(a, kl, b, c)]; ss = [x + y + z for x, y, z in zip(a, b, c)]
        pd = product(p, val(dd) * val(d)); ps = product(p, val(ss) * val(d)); return dd + ss + pd + ps + norm([x + k - y for x, k, y in zip(a, kl, pd)])
    raise KeyError(op)

def check(field, op, got, a=None, b=None, c=None, d=None, exact=True):
    """raises AssertionError unless `got` is what the operation must return: the value identity and the limb bounds, stated on their own, and (exact) the very limbs of the model"""
    p = MOD[field]; got = [int(x) for x in got]; exp = model(field, op, a, b, c, d)
    def normalized(l, ceil=(1 << B) + 8): assert all(0 <= x < ceil for x in l[:8]), ("limb bound", op, l)
    if op in ("mul", "mul_kara", "mul2", "sqr"):
        A = val(a) * val(b) + val(c) * val(d) if op == "mul2" else val(a) ** 2 if op == "sqr" else val(a) * val(b)
        normalized(got, 1 << B); assert val(got) * RP == A + ((-A * _pinv(p)) % RP) * p, ("product's value", op)
    elif op == "norm": normalized(got); assert val(got) == val(a), ("value", op)
    elif op.startswith("sub") and op[3:].isdigit(): normalized(got); assert val(got) == val(a) + int(op[3:]) * p - val(b), ("value", op)
    elif op == "cond_neg": assert val(got) == (2 * p - val(a) if b[0] & 1 else val(a)) and all(0 <= x < 1 << 31 for x in got), ("value", op)
    elif op == "sub_product": assert val(got) == val(a) + 2 * p - val(b) and all(0 <= x < 1 << 32 for x in got), ("value", op)
    elif op == "neg_product": assert val(got) == 2 * p - val(a) and all(0 <= x < (1 << 30) + 64 for x in got[:8]), ("value", op)
    elif op == "add_raw": assert val(got) == val(a) + val(b), ("value", op)
    elif op == "barrett":
        _, q = barrett(a); V = val(a); normalized(got, (1 << B) + 2); assert val(got) == V - q * p and val(got) < bound("4.1", p), ("value", op)
        f = list(got)
        for i in range(8): f[i + 1] += f[i] >> B; f[i] &= M
        assert (V % p == 0) == any(f == kp for kp in params()[2]), ("multiple of p", op)
    elif op == "to_words": v = sum(x << (32 * j) for j, x in enumerate(got[:8])); assert v < 2 * p and (v * RP - val(a) * (1 << 256)) % p == 0, ("value", op)
    elif op in ("unpack", "pack_words"): assert (val(got) if op == "unpack" else sum(x << (32 * j) for j, x in enumerate(got[:8]))) == \
            (sum(int(x) << (32 * j) for j, x in enumerate(a[:8])) if op == "unpack" else val(a)), ("value", op)
    elif op == "ntt_lazy":
        kl = KL2(field); dd, ss, pd, ps, fin = (got[9 * k:9 * k + 9] for k in range(5))
        assert val(dd) == val(a) + 4 * p - val(b) - val(c) and val(ss) == val(a) + val(b) + val(c) and all(x < WIDE for x in dd + ss), ("value", op)
        for r, w in ((pd, dd), (ps, ss)): normalized(r, 1 << B); assert val(r) * RP == val(w) * val(d) + ((-val(w) * val(d) * _pinv(p)) % RP) * p, ("product's value", op)
        normalized(fin); assert val(fin) == val(a) + 2 * p - val(pd), ("value", op)
    assert not exact or got == exp, ("limbs", op, got, exp)

# ---- contracts: for every operation, what each operand may be ----------------------------------------------------------------------------------------------------
# operand = (ceiling of limbs 0..7, edge classes that must occur, value bound (exclusive), cap of the top limb or None)
def contract(field, op):
    p = MOD[field]; big = 1 << 258                                               # every value of the formulas stays below 11 p < 2^258 (gen_field29.py)
    n = (NORM, EDGE_NORM, big, None); ex = lambda vmax, cap=None: (M, EDGE_EXACT, vmax, cap)
    if op == "mul": return [(WIDE, EDGE_NORM + [WIDE], big, None), n]
    if op == "mul_kara": return [(KARA, EDGE_NORM + [KARA], big, None)] * 2
    if op == "mul2": w = (DUAL, EDGE_NORM + [DUAL], big, None); return [w, n, w, n]
    if op in ("sqr", "to_words"): return [n]
    if op == "norm": return [((1 << 32) - 1, EDGE_NORM + [(1 << 32) - 1], 1 << 264, (1 << 32) - 8)]
    if op.startswith("sub") and op[3:].isdigit(): c = int(op[3:]); return [n, (SUBT, EDGE_NORM + [SUBT], c * p, K(c)[8])]
    if op == "cond_neg": return [ex(p)]                                          # (and the sense, 0 or 1, in a second operand's first word)
    if op == "sub_product": return [(LAZY1, EDGE_NORM + [LAZY1], big, None), ex(2 * p, KL2(field)[8])]
    if op == "neg_product": return [ex(2 * p, KL2(field)[8])]
    if op == "add_raw": return [((1 << 31) - 1, EDGE_NORM + [(1 << 31) - 1], 1 << 263, None)] * 2
    if op == "barrett": return [((1 << 31) - 1, EDGE_NORM + [(1 << 31) - 1], 1200 * p, None)]
    if op == "one": return []
    if op == "unpack": return [((1 << 32) - 1, [0, (1 << 32) - 1], 1 << 264, None)]                  # eight 32-bit words (the ninth is ignored)
    if op == "pack_words": return [ex(1 << 256)]
    if op == "product_is_zero": return [ex(2 * p)]
    if op == "ntt_lazy": return [(NORM, EDGE_NORM, 1 << 257, None), ex(2 * p, KL2(field)[8]), ex(2 * p, KL2(field)[8]), (NORM, EDGE_NORM, 1 << 256, None)]
    raise KeyError(op)

def legal(field, op, operands):
    """raises AssertionError unless the operands (lists of nine integers) keep to the contract of the operation"""
    spec = contract(field, op)
    if op == "cond_neg": assert len(operands) == 2 and operands[1][0] in (0, 1) and not any(operands[1][1:]); operands = operands[:1]
    assert len(operands) == len(spec)
    for k, (l, (ceil, _, vmax, cap)) in enumerate(zip(operands, spec)):
        assert len(l) == 9 and all(0 <= x <= ceil for x in l[:8]) and 0 <= l[8] < 1 << 32, (op, k, "limbs", l)
        if op == "unpack": continue
        assert val(l) < vmax, (op, k, "value"); assert cap is None or l[8] <= cap, (op, k, "top limb")
    if op == "mul": assert 9 * WIDE * ((1 << B) + 8) + 9 * (1 << 58) + (1 << 35) < 1 << 64                   # the generator's column bounds, for the ceilings used here
    if op == "mul_kara": assert 9 * ((1 << 30) + 16) ** 2 + 9 * (1 << 58) + (1 << 35) < 1 << 64
    if op == "mul2": assert 18 * ((1 << 30) + 8) * ((1 << B) + 8) + 9 * (1 << 58) + (1 << 35) < 1 << 64
    if op == "ntt_lazy": assert NORM + 2 * ((1 << 30) + 64) < WIDE

def top_limb(rnd, low, vmax, cap, mode):
    """a top limb that keeps the value below vmax (and the limb at most cap): mode 0 none, 1 the largest, else any"""
    tmax = (vmax - 1 - val(low + [0])) >> TOP; tmax = min(tmax, (1 << 32) - 1 if cap is None else cap); assert tmax >= 0
    return 0 if mode == 0 else tmax if mode == 1 else rnd.randrange(0, tmax + 1)
def draw(rnd, ceil, edges, vmax, cap):
    low = [rnd.choice(edges) if rnd.random() < 0.6 else rnd.randrange(0, ceil + 1) for _ in range(8)]
    return low + [top_limb(rnd, low, vmax, cap, rnd.randrange(3))]

def inputs(field, op, n=2000, seed=29):
    """n elements for the operation: a list of operand lists [[a limbs] ...] per operand position.  The first elements are the striped ones — every low limb of every
    operand at the same edge class, the all-ceiling vector first, with the top limb at the top of its interval and at zero —, then edge-heavy random draws, then the
    named special cases of the operation."""
    rnd = random.Random(seed * 1000 + field * 100 + (OPS_FQ + OPS_FR).index(op)); spec = contract(field, op); p = MOD[field]; rows = []
    width = max([len(s[1]) for s in spec] + [1])
    for j in range(width):
        for mode in (1, 0):
            row = []
            for ceil, edges, vmax, cap in spec:
                e = edges[max(len(edges) - 1 - j, 0)]; row.append([e] * 8 + [top_limb(rnd, [e] * 8, vmax, cap, mode)])
            rows.append(row)
    special = []
    if op == "cond_neg": special = [[limbs29(v)] for v in (0, 0, 1, 1, p - 1, p - 1)]
    if op == "product_is_zero":
        special = [[limbs29(v)] for v in (0, p, 1, p - 1, p + 1)]
        for i in range(9):
            for dlt in (1, -1):
                l = limbs29(p); l[i] += dlt
                if 0 <= l[i] <= M or i == 8: special.append([l])
    if op == "barrett":
        k6 = K(6)
        for j in list(range(0, 13)) + [100, 600, 1199]: special.append([limbs29(j * p)])                                     # exact multiples of p
        for k in range(0, 5):                                                                                                  # (v + k p) + (6 p - v) as the verifier forms it: (6 + k) p on wide limbs
            v = rnd.randrange(0, p); special.append([[u + w for u, w in zip(limbs29(v + k * p), norm([w - x for w, x in zip(k6, limbs29(v))]))]])
        special += [[limbs29(j * p + dlt)] for j in (0, 1, 5, 1199) for dlt in (1, p - 1)]
    if op == "unpack":
        special = [[[(1 << 32) - 1] * 8 + [0]], [[0] * 9]]
        for i in range(1, 9):
            for bit in (29 * i - 1, 29 * i, 29 * i + 1): special.append([words(1 << bit)]); special.append([words(((1 << 256) - 1) ^ (1 << bit))])
        special += [[words(1 << 255)], [words(1)]]
    if op == "pack_words": special = [[limbs29((1 << 256) - 1)], [limbs29(0)]] + [[limbs29(1 << bit)] for i in range(1, 8) for bit in (32 * i - 1, 32 * i)]
    while len(rows) + len(special) < n:
        row = [draw(rnd, *s) for s in spec]
        if op == "unpack": row[0][8] = 0
        rows.append(row)
    rows += special
    if op == "unpack":
        for r in rows: r[0][8] = 0
    if op == "cond_neg": rows = [r + [[i & 1] + [0] * 8] for i, r in enumerate(rows)]                                          # both senses, the striped rows and the special cases included
    return [[r[k] for r in rows] for k in range(len(rows[0]))] if spec else []

# ---- points -------------------------------------------------------------------------------------------------------------------------------------------------------
# invariants of the formulas in units of p, from gen_field29.py (check_bounds, check_bounds_add, check_bounds_dbl, check_bounds_g2, check_bounds_oct)
G1_INV = ("5.5", "3.6", "1.1", "1.1")                                                           # X, Y, ZZ, ZZZ
G2_LANE_INV = (("4.1", "4.1"), ("4.1", "4.1"), ("3.2", "5.7"), ("3.2", "5.7"))                  # XYZZ2_29::madd, per component
G2_OCT_INV = (("5.5", "5.5"), ("4.1", "4.1"), ("5.7", "5.7"), ("5.7", "5.7"))                    # oct29_add
RINV = pow(RP, -1, Q_MOD)
def inv(x): return pow(x % Q_MOD, -1, Q_MOD)
def fq_sqrt(a):
    a %= Q_MOD; y = pow(a, (Q_MOD + 1) // 4, Q_MOD); return y if y * y % Q_MOD == a else None      # q = 3 mod 4
def fq_cbrt(a):
    """a cube root in Fq (q = 1 mod 9, q - 1 = 9 t): None for a non-cube"""
    a %= Q_MOD; t = (Q_MOD - 1) // 9; assert t % 3 and (Q_MOD - 1) % 27
    if a == 0: return 0
    if pow(a, (Q_MOD - 1) // 3, Q_MOD) != 1: return None
    g = 2
    while pow(g, (Q_MOD - 1) // 3, Q_MOD) == 1: g += 1
    h = pow(g, t, Q_MOD); at = pow(a, t, Q_MOD); k = [pow(h, 3 * i, Q_MOD) for i in range(3)].index(at)
    m = pow(3, -1, t); j = (3 * m - 1) // t; r = pow(a, m, Q_MOD) * pow(h, -k * j, Q_MOD) % Q_MOD; assert pow(r, 3, Q_MOD) == a; return r
def f2(a): return (a[0] % Q_MOD, a[1] % Q_MOD)
def f2_mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % Q_MOD, (a[0] * b[1] + a[1] * b[0]) % Q_MOD)
def f2_add(a, b): return ((a[0] + b[0]) % Q_MOD, (a[1] + b[1]) % Q_MOD)
def f2_sub(a, b): return ((a[0] - b[0]) % Q_MOD, (a[1] - b[1]) % Q_MOD)
def f2_scale(a, k): return (a[0] * k % Q_MOD, a[1] * k % Q_MOD)
def f2_inv(a): n = inv(a[0] * a[0] + a[1] * a[1]); return (a[0] * n % Q_MOD, -a[1] * n % Q_MOD)
def f2_sqrt(a):
    a = f2(a)
    if a == (0, 0): return a
    s = fq_sqrt(a[0] * a[0] + a[1] * a[1])
    if s is None: return None
    for sg in (s, -s):
        x0 = fq_sqrt((a[0] + sg) * inv(2))
        if x0: r = (x0, a[1] * inv(2 * x0) % Q_MOD); return r if f2_mul(r, r) == a else None
    return None
B2 = f2_scale(f2_inv((9, 1)), 3)                                                                 # the twist's coefficient 3 / (9 + u)

def norm_limbs(rnd, vmax, edges=EDGE_NORM, ceil=NORM): return draw(rnd, ceil, edges, vmax, None)
def rep(v, j): return limbs29(v % Q_MOD + j * Q_MOD)                                              # the representative v + j q, exact limbs
def g1_affine(w):
    """36 raw words -> the affine point (canonical integers), None if ZZ = 0 (mod q)"""
    X, Y, ZZ, ZZZ = (val(w[9 * k:9 * k + 9]) for k in range(4))
    if ZZ % Q_MOD == 0 or ZZZ % Q_MOD == 0: return None
    return (X * inv(ZZ) % Q_MOD, Y * inv(ZZZ) % Q_MOD)
def g2_affine(c):
    """eight lists of nine limbs, X.c0 X.c1 Y.c0 Y.c1 ZZ.c0 ZZ.c1 ZZZ.c0 ZZZ.c1 -> ((x0, x1), (y0, y1)), None if ZZ = 0 (mod q)"""
    X, Y, ZZ, ZZZ = (f2((val(c[2 * k]), val(c[2 * k + 1]))) for k in range(4))
    if ZZ == (0, 0) or ZZZ == (0, 0): return None
    return (f2_mul(X, f2_inv(ZZ)), f2_mul(Y, f2_inv(ZZZ)))
def g1_on_curve(pt): return (pt[1] * pt[1] - pt[0] ** 3 - 3) % Q_MOD == 0
def g2_on_curve(pt): x, y = pt; return f2_sub(f2_mul(y, y), f2_add(f2_mul(x, f2_mul(x, x)), B2)) == (0, 0)

def g1_acc(rnd, first="X", jmax=(4, 2)):
    """an on-curve accumulator within G1_INV whose first coordinate has limbs from the edge set; returns (36 words, affine point)"""
    while True:
        lam = rnd.randrange(1, Q_MOD); l2 = lam * lam % Q_MOD; l3 = l2 * lam % Q_MOD
        if first == "X":
            X = norm_limbs(rnd, bound(G1_INV[0], Q_MOD)); x = val(X) * RINV * inv(l2) % Q_MOD; y = fq_sqrt(x ** 3 + 3)
            if y is None: continue
            if rnd.random() < 0.5: y = Q_MOD - y
            Y = rep(y * l3 * RP, rnd.randrange(jmax[1] + 1))
        else:
            Y = norm_limbs(rnd, bound(G1_INV[1], Q_MOD)); y = val(Y) * RINV * inv(l3) % Q_MOD; x = fq_cbrt(y * y - 3)
            if x is None: continue
            X = rep(x * l2 * RP, rnd.randrange(jmax[0] + 1))
        return X + Y + rep(l2 * RP, 0) + rep(l3 * RP, 0), (x, y)
def g1_raw(rnd, pt, jx=0, jy=0, lam=None):
    """some raw form of the affine point pt (exact limbs, representatives x + jx q, y + jy q)"""
    lam = rnd.randrange(1, Q_MOD) if lam is None else lam; l2 = lam * lam % Q_MOD; l3 = l2 * lam % Q_MOD
    return rep(pt[0] * l2 * RP, jx) + rep(pt[1] * l3 * RP, jy) + rep(l2 * RP, 0) + rep(l3 * RP, 0)
def g1_operand(rnd, first="x"):
    """an affine operand as the tables hold it: canonical x 2^261 and y 2^261 with edge limbs in the coordinate chosen first, and a sign; returns (19 words, the
    point that is added)"""
    while True:
        if first == "x":
            px = draw(rnd, M, EDGE_EXACT, Q_MOD, None); x = val(px) * RINV % Q_MOD; y = fq_sqrt(x ** 3 + 3)
            if y is None: continue
            if rnd.random() < 0.5: y = Q_MOD - y
            py = rep(y * RP, 0)
        else:
            py = draw(rnd, M, EDGE_EXACT, Q_MOD, None); y = val(py) * RINV % Q_MOD; x = fq_cbrt(y * y - 3)
            if x is None: continue
            px = rep(x * RP, 0)
        if y == 0: continue
        s = rnd.randrange(2); return px + py + [s], (x, (Q_MOD - y) % Q_MOD if s else y)
def g1_neg(pt): return None if pt is None else (pt[0], (Q_MOD - pt[1]) % Q_MOD)

def check_g1(w, expect, inv_bounds=G1_INV, allow_zz0=False):
    """raises AssertionError unless the 36 raw words are `expect` (an affine point; None: ZZ must be 0 mod q) within the invariant, limbs 0..7 below 2^29 + 8"""
    w = [int(x) for x in w]
    for k in range(4):
        l = w[9 * k:9 * k + 9]; assert all(x < (1 << B) + 8 for x in l[:8]), ("limb bound", k, l); assert val(l) < units(inv_bounds[k], Q_MOD), ("invariant", k)
    got = g1_affine(w)
    if got is None: assert expect is None or allow_zz0, "ZZ = 0 (mod q)"; return
    assert expect is not None, "a point where ZZ = 0 (mod q) was due"; assert got == expect, ("point", got, expect)
def check_g2(c, expect, inv_bounds):
    c = [[int(x) for x in l] for l in c]
    for k in range(4):
        for h in range(2):
            l = c[2 * k + h]; assert all(x < (1 << B) + 8 for x in l[:8]), ("limb bound", k, h, l); assert val(l) < units(inv_bounds[k][h], Q_MOD), ("invariant", k, h)
    got = g2_affine(c)
    if got is None: assert expect is None, "ZZ = 0 (mod q)"; return
    assert expect is not None, "a point where ZZ = 0 (mod q) was due"; assert got == expect, ("point", got, expect)

def g2_acc(rnd, inv_bounds, jz=(0, 0)):
    """an on-curve G2 accumulator whose X components have limbs from the edge set: eight limb lists X.c0 X.c1 Y.c0 .. ZZZ.c1 within inv_bounds, and the affine point.
    Y takes representatives up to its bound, ZZ / ZZZ up to jz per component."""
    jy = [int(Fraction(inv_bounds[1][h])) - 1 for h in range(2)]
    while True:
        lam = (rnd.randrange(1, Q_MOD), rnd.randrange(Q_MOD)); l2 = f2_mul(lam, lam); l3 = f2_mul(l2, lam)
        X = [norm_limbs(rnd, bound(inv_bounds[0][h], Q_MOD)) for h in range(2)]
        x = f2_mul(f2_scale((val(X[0]), val(X[1])), RINV), f2_inv(l2)); y = f2_sqrt(f2_add(f2_mul(x, f2_mul(x, x)), B2))
        if y is None or y == (0, 0): continue
        if rnd.random() < 0.5: y = f2_sub((0, 0), y)
        Yv = f2_scale(f2_mul(y, l3), RP); Z2 = f2_scale(l2, RP); Z3 = f2_scale(l3, RP)
        return X + [rep(Yv[h], rnd.randrange(jy[h] + 1)) for h in range(2)] + [rep(Z2[h], rnd.randrange(jz[h] + 1)) for h in range(2)] + \
            [rep(Z3[h], rnd.randrange(jz[h] + 1)) for h in range(2)], (x, y)
def g2_raw(rnd, pt, jx=0, jy=0):
    lam = (rnd.randrange(1, Q_MOD), rnd.randrange(Q_MOD)); l2 = f2_mul(lam, lam); l3 = f2_mul(l2, lam)
    X = f2_scale(f2_mul(pt[0], l2), RP); Y = f2_scale(f2_mul(pt[1], l3), RP); Z2 = f2_scale(l2, RP); Z3 = f2_scale(l3, RP)
    return [rep(X[0], jx), rep(X[1], jx), rep(Y[0], jy), rep(Y[1], jy), rep(Z2[0], 0), rep(Z2[1], 0), rep(Z3[0], 0), rep(Z3[1], 0)]
def g2_operand(rnd):
    """an affine G2 operand: canonical x 2^261 with edge limbs, y 2^261, a sign; returns (37 words, the point that is added)"""
    while True:
        px = [draw(rnd, M, EDGE_EXACT, Q_MOD, None) for _ in range(2)]; x = f2_scale((val(px[0]), val(px[1])), RINV); y = f2_sqrt(f2_add(f2_mul(x, f2_mul(x, x)), B2))
        if y is None or y == (0, 0): continue
        s = rnd.randrange(2); yr = f2_scale(y, RP); return px[0] + px[1] + rep(yr[0], 0) + rep(yr[1], 0) + [s], (x, f2_sub((0, 0), y) if s else y)
def g2_neg(pt): return None if pt is None else (pt[0], f2_sub((0, 0), pt[1]))
def oct_words(c): return sum((c[2 * k + h] for h in range(2) for k in range(4)), [])              # component-major: the slots of the eight lanes
def oct_lists(w): w = [int(x) for x in w]; return [w[9 * (4 * h + k):9 * (4 * h + k) + 9] for k in range(4) for h in range(2)]
def lane_words(c): return sum(c, [])
def lane_lists(w): w = [int(x) for x in w]; return [w[9 * i:9 * i + 9] for i in range(8)]

# fq2_29_mul / fq2_29_sqr (msm.cuh) on the model's operations: the exact limbs, next to the product in Fq2 they must represent
def fq2_mul_model(a, b):
    v0 = model(FQ, "mul", a[0], b[0]); v1 = model(FQ, "mul", a[1], b[1]); v2 = model(FQ, "mul_kara", model(FQ, "add_raw", a[0], a[1]), model(FQ, "add_raw", b[0], b[1]))
    return [sub_c(2, v0, v1), sub_c(4, v2, model(FQ, "add_raw", v0, v1))]
def fq2_sqr_model(a):
    m = model(FQ, "mul", a[0], a[1]); return [model(FQ, "mul", model(FQ, "add_raw", a[0], a[1]), sub_c(12, a[0], a[1])), norm([2 * x for x in m])]
def check_fq2(got, a, b=None):
    """fq2_29_mul(a, b), or fq2_29_sqr(a) for b = None: the exact limbs, normalized, and the Fq2 product they stand for"""
    got = [[int(x) for x in l] for l in got]; exp = fq2_mul_model(a, b) if b is not None else fq2_sqr_model(a); bb = a if b is None else b
    want = f2_scale(f2_mul((val(a[0]), val(a[1])), (val(bb[0]), val(bb[1]))), RINV)
    for h in range(2): assert all(x < (1 << B) + 8 for x in got[h][:8]), ("limb bound", h); assert val(got[h]) % Q_MOD == want[h], ("value", h)
    assert got == exp, ("limbs", got, exp)

# ---- the cases of the point probes: operands as uint32 rows, and what must come back --------------------------------------------------------------------------------
def _oracle():
    from oracle import pyoracle as o; return o
def g1_acc_low(rnd, first, low):
    """g1_acc with the eight low limbs of the first coordinate given (the all-ceiling vector): only the top limb and the scaling are drawn"""
    while True:
        w, pt = g1_acc(rnd, first)
        k = 0 if first == "X" else 9; top = w[k + 8]; cand = low + [top]
        if val(cand) >= bound(G1_INV[0 if first == "X" else 1], Q_MOD): continue
        # re-derive the point from the forced coordinate with the scaling of w (ZZ = lam^2 R', ZZZ = lam^3 R')
        l2 = val(w[18:27]) * RINV % Q_MOD; l3 = val(w[27:36]) * RINV % Q_MOD
        if first == "X":
            x = val(cand) * RINV * inv(l2) % Q_MOD; y = fq_sqrt(x ** 3 + 3)
            if y is None: continue
            return cand + rep(y * l3 * RP, 2) + w[18:], (x, y)
        y = val(cand) * RINV * inv(l3) % Q_MOD; x = fq_cbrt(y * y - 3)
        if x is None: continue
        return rep(x * l2 * RP, 4) + cand + w[18:], (x, y)
def g1_accs(n, seed):
    """n accumulators within the invariant: first coordinate X or Y in turn, the all-ceiling and all-zero low limbs first"""
    rnd = random.Random(seed); out = [g1_acc_low(rnd, f, [e] * 8) for f in ("X", "Y") for e in (NORM, 0, 1 << B, M)]
    while len(out) < n: out.append(g1_acc(rnd, "XY"[len(out) & 1]))
    return out[:n]
def g1_operands(n, seed):
    rnd = random.Random(seed); return [g1_operand(rnd, "xy"[(i >> 1) & 1]) for i in range(n)]
def g1_madd_cases(n, seed=1):
    o = _oracle(); A = g1_accs(n, seed); Bq = g1_operands(n, seed + 1); assert all(a[1][0] != b[1][0] for a, b in zip(A, Bq))
    return [a[0] for a in A], [b[0] for b in Bq], [o.g1_op("add", a[1], b[1]) for a, b in zip(A, Bq)]
def g1_dbl_cases(n, seed=3):
    o = _oracle(); Bq = g1_operands(n, seed); return [b[0] for b in Bq], [o.g1_op("dbl", b[1]) for b in Bq]
def g1_chain_cases(n, steps=32, seed=5):
    """n runs: an accumulator and `steps` operands; the sums after every step"""
    o = _oracle(); A = g1_accs(n, seed); Bq = g1_operands(n * steps, seed + 1); exp = []
    for i, a in enumerate(A):
        cur = a[1]
        for b in Bq[i * steps:(i + 1) * steps]: assert cur[0] != b[1][0]; cur = o.g1_op("add", cur, b[1]); exp.append(cur)
    return [a[0] for a in A], [sum((b[0] for b in Bq[i * steps:(i + 1) * steps]), []) for i in range(n)], exp
G1_GEN = (1, 2)
def g1_pair_cases(n, seed=7, infinity=True, degenerate=True):
    """pairs of accumulators for the general additions.  Returns rows of (kind, A words, B words, expected affine point or None).  Kinds in turn, so that every wave of a
    cooperative form holds all of them: plain | A at infinity | B at infinity | both | B = -A | B = A | A = B = +-G | plain at the largest representatives"""
    o = _oracle(); rnd = random.Random(seed); acc = g1_accs(2 * n, seed + 1); rows = []; zero = [0] * 36
    for i in range(n):
        (wa, pa), (wb, pb) = acc[2 * i], acc[2 * i + 1]; kind = ("plain", "a_inf", "b_inf", "both_inf", "opposite", "equal", "generator", "plain_top")[i % 8]
        if kind in ("a_inf", "b_inf", "both_inf") and not infinity: kind = "plain"
        if kind in ("opposite", "equal", "generator") and not degenerate: kind = "plain"
        if kind == "plain": rows.append((kind, wa, wb, o.g1_op("add", pa, pb)))
        elif kind == "plain_top": rows.append((kind, g1_raw(rnd, pa, 4, 2), g1_raw(rnd, pb, 4, 2), o.g1_op("add", pa, pb)))
        elif kind == "a_inf": rows.append((kind, zero, wb, pb))
        elif kind == "b_inf": rows.append((kind, wa, zero, pa))
        elif kind == "both_inf": rows.append((kind, zero, zero, None))
        elif kind == "opposite": rows.append((kind, wa, g1_raw(rnd, g1_neg(pa), rnd.randrange(5), rnd.randrange(3)), None))
        elif kind == "equal": rows.append((kind, wa, g1_raw(rnd, pa, rnd.randrange(5), rnd.randrange(3)), o.g1_op("dbl", pa)))
        else: g = G1_GEN if i & 8 else g1_neg(G1_GEN); rows.append((kind, g1_raw(rnd, g, 1, 1), g1_raw(rnd, g, 0, 2), o.g1_op("dbl", g)))
    return rows
def g2_pair_cases(n, seed=11):
    """the same for oct29_add: pairs of G2 accumulators within its invariant, as lists of eight limb lists"""
    o = _oracle(); rnd = random.Random(seed); rows = []; zero = [[0] * 9 for _ in range(8)]
    for i in range(n):
        (ca, pa), (cb, pb) = g2_acc(rnd, G2_OCT_INV, (4, 4)), g2_acc(rnd, G2_OCT_INV, (4, 4)); kind = ("plain", "a_inf", "b_inf", "both_inf", "opposite", "equal", "plain", "plain_top")[i % 8]
        if kind == "plain": rows.append((kind, ca, cb, o.g2_op("add", pa, pb)))
        elif kind == "plain_top": rows.append((kind, g2_raw(rnd, pa, 4, 3), g2_raw(rnd, pb, 4, 3), o.g2_op("add", pa, pb)))
        elif kind == "a_inf": rows.append((kind, zero, cb, pb))
        elif kind == "b_inf": rows.append((kind, ca, zero, pa))
        elif kind == "both_inf": rows.append((kind, zero, zero, None))
        elif kind == "opposite": rows.append((kind, ca, g2_raw(rnd, g2_neg(pa), rnd.randrange(5), rnd.randrange(4)), None))
        else: rows.append((kind, ca, g2_raw(rnd, pa, rnd.randrange(5), rnd.randrange(4)), None))
    return rows
def g2_madd_cases(n, seed=13):
    o = _oracle(); rnd = random.Random(seed); A = [g2_acc(rnd, G2_LANE_INV, (2, 4)) for _ in range(n)]; Bq = [g2_operand(rnd) for _ in range(n)]
    assert all(a[1][0] != b[1][0] for a, b in zip(A, Bq)); return [a[0] for a in A], [b[0] for b in Bq], [o.g2_op("add", a[1], b[1]) for a, b in zip(A, Bq)]
FQ2_UNITS = 12                                                                                    # components of fq2_29_mul's / fq2_29_sqr's operands: below 12 p (K_12 in the squaring)
def fq2_cases(n, seed=17):
    """operands of fq2_29_mul / fq2_29_sqr: components normalized, below 12 p, the second component's top limb at most K_12's; the all-ceiling pair first"""
    rnd = random.Random(seed); vmax = FQ2_UNITS * Q_MOD; cap = K(12)[8]; rows = []
    for e in reversed(EDGE_NORM):
        for mode in (1, 0): rows.append([[[e] * 8 + [top_limb(rnd, [e] * 8, vmax, cap, mode)] for _ in range(2)] for _ in range(2)])
    while len(rows) < n: rows.append([[draw(rnd, NORM, EDGE_NORM, vmax, cap) for _ in range(2)] for _ in range(2)])
    return [r[0] for r in rows], [r[1] for r in rows]
