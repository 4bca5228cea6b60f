"""GPU parity of the key-side kernels, each on its own and point by point: fixed-base multiplication and decompression (keyops.cuh), the H query into the coset's Lagrange
basis and C folded into L (ecntt.cuh), through the zkgpu_test_* entries that call the host functions of key generation and key load unchanged.  Every expected point is
k * G for a scalar k worked out in Python integers (tests/key_model.py, itself checked by tests/test_key_model_cpu.py); every comparison is equality of words.  Nothing
here is weighted by a witness: a wrong point for a variable that is 0 in every fixture fails like any other."""
import os
import numpy as np
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import key_model as km

pytestmark = pytest.mark.gpu
R, Q = km.R, km.Q

def first_difference(got, exp):
    d = np.nonzero(np.any(np.asarray(got) != np.asarray(exp), axis=1))[0]; return None if not len(d) else int(d[0])

# ---- fixed-base multiplication ------------------------------------------------------------------------------------------------------------------------------
def window_scalars():
    g = o.SplitMix64(31); ks = [0, 1, 255, 256, R - 1, (1 << 248) - 1, int("2f" + "ff" * 31, 16)]                  # the last two: every byte 0xFF, below r
    for w in range(32): ks += [1 << (8 * w), (1 << (8 * w)) - 1]
    for w in range(32): ks += [d << (8 * w) for d in (1, 0x2F if w == 31 else 0x80, 0x30 if w == 31 else 0xFF) if d << (8 * w) < R]     # a single non-zero byte
    for k in range(1, 25): ks.append(((g.field() % R) >> (8 * k)) << (8 * k))                                        # the low k windows zero
    for k in range(1, 9): ks.append((g.field() % R) & ((1 << (8 * k)) - 1))                                          # the high windows zero
    ks += [g.field() % R for _ in range(300 - len(ks))]
    assert len(ks) == 300 and all(0 <= k < R for k in ks); return ks

@pytest.mark.parametrize("group", [1, 2])
def test_fixed_base_mul_every_scalar(group):
    ks = window_scalars(); kb = o.SplitMix64(32 + group).field() % R
    if group == 1: base = o.g1_op("mul", o.g1_gen(), k=kb); arr, mul = o.g1_arr, o.g1_op
    else: base = o.g2_op("mul", o.g2_gen(), k=kb); arr, mul = o.g2_arr, o.g2_op
    got = e.fixed_base_mul(group, arr([base])[0], o.to_arr(ks)); exp = arr([mul("mul", base, k=k) if k else None for k in ks])
    assert not got[0].any()                                                                                          # the scalar 0 gives the point at infinity
    i = first_difference(got, exp); assert i is None, "scalar %d = %x" % (i, ks[i])

# ---- decompression ---------------------------------------------------------------------------------------------------------------------------------------------
def off_curve_x(group):
    if group == 1:
        x = 1
        while pow(km.g1_rhs(x), (Q - 1) // 2, Q) == 1: x += 1
        assert o.field_op(o.FQ, "sqrt", [km.g1_rhs(x)]) == [0]; return x                                              # the oracle finds no root either
    x = (1, 1)
    while km.fq2_is_square(km.g2_rhs(x)): x = (x[0] + 1, 1)
    assert o.fq2_op("sqrt", km.g2_rhs(x)) is None; return x

def compressed(group, n, seed):
    """n points: consecutive multiples and their negatives (both parities for the same x), the point at infinity at the first and last index and in runs; an entry flagged
    infinity carries an x that is on no point, which the flag must keep from being looked at.  -> (x in Montgomery form, flags, the points)"""
    k0 = o.SplitMix64(seed).field() % R; h = (n + 1) // 2
    if group == 1: pts = o.g1_from(o.g1_consecutive(k0, h)); pts = (pts + [o.g1_op("neg", p) for p in pts])[:n]
    else: pts = o.g2_from(o.g2_consecutive(k0, h)); pts = (pts + [o.g2_op("neg", p) for p in pts])[:n]
    if n > 2:
        for i in [0, n - 1] + list(range(n // 3, min(n // 3 + 5, n))) + list(range(n // 2 + 1, n, 17)): pts[i] = None
    bad = off_curve_x(group); comp = [(km.compress_g1 if group == 1 else km.compress_g2)(p) for p in pts]; flags = np.array([f for _, f in comp], dtype=np.uint8)
    if group == 1: xs = o.to_arr(o.to_mont(o.FQ, [bad if f & 2 else x for x, f in comp]))
    else: xs = o.to_arr(o.to_mont(o.FQ, [c for x, f in comp for c in (bad if f & 2 else x)])).reshape(n, 8)
    return xs, flags, pts

@pytest.mark.parametrize("group,n", [(1, 1), (1, 127), (1, 128), (1, 129), (1, 1000), (2, 1), (2, 63), (2, 64), (2, 65), (2, 600)])
def test_decompression_gives_every_point_back(group, n):
    xs, flags, pts = compressed(group, n, 40 + n); got = e.decompress(group, xs, flags); exp = (o.g1_arr if group == 1 else o.g2_arr)(pts)
    if n > 2: assert set(flags.tolist()) == {0, 1, 2}
    i = first_difference(got, exp); assert i is None, "point %d, flags %d" % (i, flags[i])

@pytest.mark.parametrize("group,n,at", [(1, 1, 0), (1, 129, 128), (1, 129, 5), (2, 1, 0), (2, 65, 64), (2, 65, 7)])
def test_decompression_refuses_an_x_on_no_point(group, n, at):
    xs, flags, pts = compressed(group, n, 50 + n); bad = off_curve_x(group); flags[at] = 1
    xs[at] = o.to_arr(o.to_mont(o.FQ, [bad] if group == 1 else list(bad))).reshape(-1)
    with pytest.raises(e.ZkGpuError, match="not on the curve"): e.decompress(group, xs, flags)

def test_fq2_sqrt_every_branch():
    """0; elements of Fq, residues and non-residues (the latter, -1 among them, are squares in Fq2 and take the branch alpha == -1, which a random twist point meets with
    probability about 1/q); u * c; squares of random elements; non-squares"""
    g = o.SplitMix64(61); fq = [g.field() % Q for _ in range(24)] + [1, 2, 3, 4, Q - 1, Q - 2, Q - 4]
    res = [c for c in fq if pow(c, (Q - 1) // 2, Q) == 1]; non = [c for c in fq if pow(c, (Q - 1) // 2, Q) == Q - 1]; assert len(res) > 5 and len(non) > 5 and Q - 1 in non
    els = [(0, 0)] + [(c, 0) for c in res + non] + [(0, c) for c in fq[:12] + [1, Q - 1]]
    rnd = [(g.field() % Q, g.field() % Q) for _ in range(80)]; els += [o.fq2_op("sqr", a) for a in rnd[:40]] + rnd[40:]
    sq = [km.fq2_is_square(a) for a in els]; assert sq.count(False) >= 10 and all(sq[:1 + len(res) + len(non)])
    roots, ok = e.fq2_sqrt(o.to_arr([c for a in els for c in a]).reshape(-1, 8))
    for i, a in enumerate(els):
        assert bool(ok[i]) == sq[i] == (o.fq2_op("sqrt", a) is not None), (i, a)
        if sq[i]: y = tuple(o.from_arr(roots[i])); assert ((y[0] * y[0] - y[1] * y[1]) % Q, 2 * y[0] * y[1] % Q) == a, (i, a)

# ---- the H query in the coset's Lagrange basis -------------------------------------------------------------------------------------------------------------------
def points_of(hs, base, run):
    """h_i * G, taken from the run of consecutive multiples base * G, (base + 1) * G, ... (or its negatives) where h_i lies in it, by a multiplication otherwise"""
    out = np.zeros((len(hs), 8), dtype=np.uint64); G = o.g1_gen()
    for i, h in enumerate(hs):
        if h == 0: continue
        if (h - base) % R < len(run): out[i] = run[(h - base) % R]
        elif (-h - base) % R < len(run): out[i] = run[(-h - base) % R]; out[i, 4:] = o.limbs(Q - o.from_arr(out[i, 4:])[0])
        else: out[i] = o.g1_arr([o.g1_op("mul", G, k=h)])[0]
    return out

@pytest.mark.parametrize("m", km.RADIX2_DOMAINS + km.STEP_DOMAINS)
def test_h_query_in_the_lagrange_basis_point_by_point(m):
    """P_j == (sum_i M[i][j] h_i) * G with column j of M = icosetFFT(e_j) by the oracle: every point of every domain up to 256; at 1,040 sixty-four columns point by point
    and three dense random v with sum_j v_j P_j == sum_i icosetFFT(v)_i H_i"""
    assert e.domain_size(m) == o.domain_size(m) == m; seed = 7 * m; base = o.SplitMix64(seed).field() % R; run = o.g1_consecutive(base, m); js = km.sample_columns(m)
    for name, h in km.h_cases(m, seed).items():
        H = points_of(h, base, run); got = e.h_query_lagrange(m, H); exp = km.scalars_to_g1(km.lagrange_scalars(m, h, js))
        i = first_difference(got[js], exp); assert i is None, (m, name, "point %d" % js[i])
        if len(js) < m:
            for t in range(3):
                v = o.to_arr(km.rand_fr(100 * t + m, m)); assert o.msm_g1(got, v) == o.msm_g1(H, o.domain_op("icosetfft", m, v)[:len(H)]), (m, name, t)

# ---- C folded into L ----------------------------------------------------------------------------------------------------------------------------------------------
def fold_system(name, tmp_path, golden_dir):
    if name == "lesscmp": p = str(tmp_path / "lc.bin"); e.circuit_export("lesscmp", p); return o.R1CS.load(p)
    if name == "groth16_step": return o.R1CS.load(os.path.join(golden_dir, "groth16_step", "r1cs.bin"))
    return km.crafted_c_system(int(name[7:]), int(name[7:]))

@pytest.mark.parametrize("name,m", [("lesscmp", 256), ("groth16_step", 48), ("crafted64", 64), ("crafted96", 96)])
def test_c_folded_into_l_point_by_point(name, m, tmp_path, golden_dir):
    """L*_v == ([v > n_inputs] l_v - sum_j zinv_j T(c_v)_j p_j) * G for every variable, T = cosetFFT . iFFT and zinv by the oracle"""
    cs = fold_system(name, tmp_path, golden_dir); assert cs.domain_m == m; g = o.SplitMix64(70 + m); p0, l0 = g.field() % R, g.field() % R; nl = cs.n_vars - cs.n_inputs
    p = [(p0 + j) % R for j in range(m)]; ell = [(l0 + i) % R for i in range(nl)]; P = o.g1_consecutive(p0, m); L = o.g1_consecutive(l0, nl)
    if name.startswith("crafted"):                                                     # the column whose fold is l_v itself: the result is the point at infinity
        v = km.CRAFTED_INF_VAR; share = km.fold_share(m, km.c_columns(cs)[v], p, km.zinv_table(m)); assert share; ell[v - cs.n_inputs - 1] = share
        L[v - cs.n_inputs - 1] = km.scalars_to_g1([share])[0]
    exp_k = km.fold_scalars(cs, ell, p); exp = km.scalars_to_g1(exp_k)
    if name.startswith("crafted"): assert exp_k[km.CRAFTED_INF_VAR] == 0 and exp_k[2] == 0 and exp_k[3] == ell[3 - cs.n_inputs - 1]
    dev = e.R1cs(cs.n_inputs, cs.n_vars, cs.n_cons, cs.rowptr, cs.col, cs.coeff); got = dev.fold_c(P, L); dev.close()
    i = first_difference(got, exp); assert i is None, (name, "variable %d" % i)
