"""Test helper: the big-integer model of the key-side operations (keyops.cuh, ecntt.cuh), built on the CPU oracle alone.  Points are k * G with KNOWN scalars k, so every
expected point is one scalar multiplication of the generator by the oracle; tests/test_key_model_cpu.py checks the model itself against the oracle's transforms."""
import numpy as np
from oracle import pyoracle as o

R, Q = o.R_MOD, o.Q_MOD
RADIX2_DOMAINS = [2, 4, 8, 64, 128, 256]            # below, at and above one 64-lane workgroup of butterflies
STEP_DOMAINS = [3, 5, 6, 12, 24, 48, 96, 1040]      # S = 1, 1, 2, 4; 16 + 8; 32 + 16; 64 + 32; 1,024 + 16 (the unpacker's)
COSET_GEN = 5                                       # libff's multiplicative generator of Fr: the coset is g * <w>

def rand_fr(seed, n):
    g = o.SplitMix64(seed); return [g.field() % R for _ in range(n)]

def scalars_to_g1(ks):
    """[k * G] as an (n, 8) array; k = 0 is the point at infinity"""
    G = o.g1_gen(); return o.g1_arr([o.g1_op("mul", G, k=k % R) if k % R else None for k in ks])

def split_of(m):
    """(B, S) of a step domain, (m, 0) of a radix-2 one"""
    B = 1 << (m.bit_length() - 1); return (m, 0) if B == m else (B, m - B)

# ---- the H query in the coset's Lagrange basis ----------------------------------------------------------------------------------------------------------
def icoset_columns(m, js):
    """column j of M, M[i][j] = icosetFFT(e_j)_i, for j in js: the definition in the header of ecntt.cuh, no symmetry assumed"""
    for j in js:
        if (m, j) not in _COLUMNS: e = np.zeros((m, 4), dtype=np.uint64); e[j, 0] = 1; _COLUMNS[(m, j)] = o.from_arr(o.domain_op("icosetfft", m, e))
    return {j: _COLUMNS[(m, j)] for j in js}
_COLUMNS = {}
def sample_columns(m, n=64):
    """all columns of a small domain; of a large one the first, the last, those around B (the seam of a step domain) and a stride through the rest, n in all"""
    if m <= 256: return list(range(m))
    B, S = split_of(m); js = {0, 1, m - 1, m - 2, B - 1, B % m, (B + 1) % m, S, max(S - 1, 0)}; k = 0
    while len(js) < n: js.add((37 * k + 5) % m); k += 1
    return sorted(js)

def lagrange_scalars(m, h, js=None):
    """p_j = sum_i M[i][j] h_i for j in js (default: all), h padded with zeros to m"""
    js = list(range(m)) if js is None else list(js); h = list(h) + [0] * (m - len(h)); cols = icoset_columns(m, js)
    return [sum(c * x for c, x in zip(cols[j], h) if x) % R for j in js]

def h_cases(m, seed):
    """name -> the scalars h_i of the H query (H_i = h_i * G; 0 = the point at infinity).  The kernels first multiply H_i by g^-i (ecntt.cuh: k_ecntt_prescale), so the
    cases 'scaled ...' choose h so that the operands of the FIRST additions (m/2 apart; B apart on a step domain) are equal / opposite points there"""
    B, S = split_of(m); half = B if S else m // 2; n_pair = S if S else half; g = o.SplitMix64(seed); base = g.field() % R
    rnd = [(base + i) % R for i in range(m)]                                            # consecutive multiples, as o.g1_consecutive makes them
    cases = {"ordinary": rnd[:m - 1], "full": rnd[:m]}
    if m > 2: cases["short"] = rnd[:max(1, m - 1 - max(1, m // 3))]                  # n_in < m - 1
    holes = list(rnd[:m - 1]); holes[0] = 0; holes[-1] = 0
    for i in range(1, m - 1, 3): holes[i] = 0
    cases["infinity inside"] = holes
    cases["all equal"] = [base] * (m - 1)
    opp = list(rnd[:m]); eq = list(rnd[:m]); sopp = list(rnd[:m]); gh = pow(COSET_GEN, half, R)
    for i in range(n_pair): opp[i + half] = (R - opp[i]) % R; eq[i + half] = eq[i] * gh % R; sopp[i + half] = (R - sopp[i]) * gh % R
    cases["opposite halves"] = opp[:m - 1] if not S else opp                             # H_(i + m/2) = -H_i
    cases["scaled equal"] = eq; cases["scaled opposite"] = sopp
    return cases

# ---- C folded into L ------------------------------------------------------------------------------------------------------------------------------------
def c_columns(cs):
    """column v of C as {row: coefficient}, v = 0 .. n_vars"""
    cols = [dict() for _ in range(cs.n_vars + 1)]; rp, cl, co = cs.rowptr[2], cs.col[2], o.from_arr(cs.coeff[2]) if len(cs.col[2]) else []
    for k in range(cs.n_cons):
        for e in range(int(rp[k]), int(rp[k + 1])): cols[int(cl[e])][k] = (cols[int(cl[e])].get(k, 0) + co[e]) % R
    return cols

def zinv_table(m):
    """1 / Z on the coset, element by element: the oracle's divide_by_Z_on_coset applied to the all-ones vector"""
    return o.from_arr(o.domain_op("divZ", m, o.to_arr([1] * m)))

def coset_values(m, vec):
    """T(vec) = cosetFFT(iFFT(vec))"""
    return o.from_arr(o.domain_op("cosetfft", m, o.domain_op("ifft", m, o.to_arr(vec))))

def fold_share(m, col, p, zinv):
    """sum_j zinv_j T(c_v)_j p_j for one column {row: coefficient}"""
    if not col: return 0
    vec = [0] * m
    for k, c in col.items(): vec[k] = c
    return sum(z * t * pj for z, t, pj in zip(zinv, coset_values(m, vec), p)) % R

def fold_scalars(cs, ell, p):
    """l*_v = [v > n_inputs] l_v - sum_j zinv_j T(c_v)_j p_j for v = 0 .. n_vars; ell: the n_vars - n_inputs scalars of L, p: the m scalars of the Lagrange points"""
    m = cs.domain_m; zinv = zinv_table(m); out = []
    for v, col in enumerate(c_columns(cs)):
        own = ell[v - cs.n_inputs - 1] if v > cs.n_inputs else 0; out.append((own - fold_share(m, col, p, zinv)) % R)
    return out

def csr(rows_of, n_cons):
    """three lists (one a matrix) of {row: [(col, coeff), ...]} -> the CSR arrays R1CS takes"""
    rp, col, co = [], [], []
    for rows in rows_of:
        ptr = [0]; cc = []; vv = []
        for k in range(n_cons):
            for c, v in sorted(rows.get(k, [])): cc.append(c); vv.append(v % R)
            ptr.append(len(cc))
        rp.append(np.array(ptr, dtype=np.uint32)); col.append(np.array(cc, dtype=np.uint32)); co.append(o.to_arr(vv) if vv else np.zeros((0, 4), dtype=np.uint64))
    return rp, col, co

CRAFTED_INPUTS, CRAFTED_VARS, CRAFTED_INF_VAR = 2, 10, 8
def crafted_c_system(m, seed):
    """a system on the domain of size m whose C has one column of each kind: 0 ONE, 1 an input column, 2 an input column without an entry, 3 no entry, 4 only +1,
    5 only r - 1, 6 general coefficients, 7 many rows (every row, coefficients of all three kinds), 8 the column whose fold the test makes equal to l_v, 9 a mix that
    reaches the last row, 10 a single entry"""
    ni, nv = CRAFTED_INPUTS, CRAFTED_VARS; nc = m - ni - 1; g = o.SplitMix64(seed); C = {}
    def put(v, k, c): C.setdefault(k, []).append((v, c))
    put(0, 0, 5); put(0, 3, 1); put(0, nc - 1, R - 1)
    put(1, 1, 7); put(1, 2, R - 1)
    for k in (0, 5, 9): put(4, k, 1)
    for k in (1, 6, nc - 2): put(5, k, R - 1)
    put(6, 2, g.field() % R); put(6, 7, (1 << 200) + 3); put(6, 11, R - 2)
    for k in range(nc): put(7, k, (1, R - 1, g.field() % R, 1 << (k % 64))[k % 4])
    put(8, 4, 3); put(8, 8, 1)
    put(9, nc - 1, 1); put(9, 10, R - 1); put(9, 12, g.field() % R)
    put(10, nc // 2, 2)
    AB = {k: [(1 + k % nv, 1)] for k in range(nc)}                                    # A and B do not matter to the fold; one entry a row keeps them well formed
    rp, col, co = csr([AB, AB, C], nc); cs = o.R1CS(ni, nv, nc, rp, col, co); assert cs.domain_m == m
    return cs

# ---- compression ------------------------------------------------------------------------------------------------------------------------------------------
def compress_g1(p):
    """(x, flags): flags bit 0 = lsb of y, bit 1 = infinity"""
    return (0, 2) if p is None else (p[0], p[1] & 1)
def compress_g2(p):
    return ((0, 0), 2) if p is None else (p[0], p[1][0] & 1)
TWIST_B = None
def twist_b():
    global TWIST_B
    if TWIST_B is None: TWIST_B = o.fq2_op("mul", (3, 0), o.fq2_op("inv", (9, 1)))       # 3 / (9 + u)
    return TWIST_B
def g1_rhs(x): return (x * x * x + 3) % Q
def g2_rhs(x):
    x3 = o.fq2_op("mul", o.fq2_op("sqr", x), x); b = twist_b(); return ((x3[0] + b[0]) % Q, (x3[1] + b[1]) % Q)
def fq2_is_square(a):
    """Euler's criterion through the norm: a in Fq2 is a square iff N(a) = a0^2 + a1^2 is a square in Fq (0 counts as one)"""
    n = (a[0] * a[0] + a[1] * a[1]) % Q; return n == 0 or pow(n, (Q - 1) // 2, Q) == 1
def decompress_g1_model(x, flags):
    if flags & 2: return None
    y = o.field_op(o.FQ, "sqrt", [g1_rhs(x)])[0]; assert y * y % Q == g1_rhs(x)
    return (x, y if (y & 1) == (flags & 1) else Q - y)
def decompress_g2_model(x, flags):
    if flags & 2: return None
    y = o.fq2_op("sqrt", g2_rhs(x)); assert y is not None
    return (x, y if (y[0] & 1) == (flags & 1) else ((Q - y[0]) % Q, (Q - y[1]) % Q))
