"""The big-integer model of the key-side operations (tests/key_model.py), which tests/test_gpu_key_ops.py holds the kernels to, against the CPU oracle alone: no device,
no engine arithmetic.  The model computes point by point; the identities here are the ones the prover relies on, computed another way."""
import json, os
import numpy as np
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import key_model as km

R, Q = km.R, km.Q

@pytest.mark.parametrize("m", km.RADIX2_DOMAINS + km.STEP_DOMAINS)
def test_transpose_identity(m):
    """sum_j v_j p_j == sum_i icosetFFT(v)_i h_i: the columns of the model's matrix against one transform of v by the oracle, for every kind of H query the GPU test uses"""
    assert o.domain_size(m) == m
    a = km.rand_fr(900 + m, m); assert o.from_arr(o.domain_op("icosetfft", m, o.domain_op("cosetfft", m, o.to_arr(a)))) == a     # the coset round trip is exact
    for name, h in km.h_cases(m, 7 * m).items():
        assert len(h) <= m; js = km.sample_columns(m); p = km.lagrange_scalars(m, h, js); hp = list(h) + [0] * (m - len(h))
        for t in range(2):                                                              # (at 1,040 v lives on the 64 sampled columns: the identity needs no other)
            v = [0] * m
            for j, x in zip(js, km.rand_fr(1000 * t + m, len(js))): v[j] = x
            hv = o.from_arr(o.domain_op("icosetfft", m, o.to_arr(v)))
            assert sum(v[j] * pj for j, pj in zip(js, p)) % R == sum(x * y for x, y in zip(hv, hp)) % R, (m, name)

def test_h_cases_meet_in_the_first_additions():
    """the 'scaled' cases make the operands of the first additions equal / opposite AFTER the kernels' factor g^-i, which is what sends add_inl into its doubling and
    cancelling branches"""
    for m in (8, 12, 96):
        B, S = km.split_of(m); half = B if S else m // 2; c = km.h_cases(m, 3); gi = pow(km.COSET_GEN, R - 2, R)
        for i in range(S if S else half):
            f = lambda h, k: h[k] * pow(gi, k, R) % R
            assert f(c["scaled equal"], i) == f(c["scaled equal"], i + half) and (f(c["scaled opposite"], i) + f(c["scaled opposite"], i + half)) % R == 0

def lesscmp_system(tmp_path):
    p = str(tmp_path / "lc.bin"); e.circuit_export("lesscmp", p); return o.R1CS.load(p)       # host only: no device behind circuit_export

def fold_systems(tmp_path, golden_dir):
    return {"lesscmp": lesscmp_system(tmp_path), "groth16_step": o.R1CS.load(os.path.join(golden_dir, "groth16_step", "r1cs.bin")),
            "crafted64": km.crafted_c_system(64, 64), "crafted96": km.crafted_c_system(96, 96)}

def test_fold_identity(tmp_path, golden_dir):
    """sum_v z_v l*_v == sum_{v > ni} z_v l_v - sum_j zinv_j C_j(z) p_j with C_j(z) the values of the C polynomial of the assignment z on the coset: the model folds column
    by column, the right-hand side transforms <C_k, z> once"""
    for name, cs in fold_systems(tmp_path, golden_dir).items():
        m = cs.domain_m; assert m == {"lesscmp": 256, "groth16_step": 48, "crafted64": 64, "crafted96": 96}[name]
        p = km.rand_fr(11, m); ell = km.rand_fr(12, cs.n_vars - cs.n_inputs); ls = km.fold_scalars(cs, ell, p); assert len(ls) == cs.n_vars + 1
        cols = km.c_columns(cs); zinv = km.zinv_table(m)
        for v, col in enumerate(cols):                                                  # a column without an entry folds to its own L point, or to nothing
            if not col: assert ls[v] == (ell[v - cs.n_inputs - 1] if v > cs.n_inputs else 0)
        for t in range(2):
            z = [1] + km.rand_fr(13 + t, cs.n_vars)
            if t: z = [x if i % 2 else 0 for i, x in enumerate(z)]                      # half of the entries 0, as in a real witness
            cz = [0] * m
            for v, col in enumerate(cols):
                for k, c in col.items(): cz[k] = (cz[k] + c * z[v]) % R
            rhs = (sum(z[v] * ell[v - cs.n_inputs - 1] for v in range(cs.n_inputs + 1, cs.n_vars + 1)) - sum(a * b * c for a, b, c in zip(zinv, km.coset_values(m, cz), p))) % R
            assert sum(a * b for a, b in zip(z, ls)) % R == rhs, (name, t)

def test_crafted_columns_are_of_every_kind():
    cs = km.crafted_c_system(64, 64); cols = km.c_columns(cs)
    assert cols[0] and cols[1] and not cols[2] and not cols[3] and set(cols[4].values()) == {1} and set(cols[5].values()) == {R - 1}
    assert not (set(cols[6].values()) & {1, R - 1}) and len(cols[7]) == cs.n_cons and {1, R - 1} < set(cols[7].values()) and len(cols[10]) == 1 and (cs.n_cons - 1) in cols[9]

def test_compress_then_sqrt_gives_the_point_back():
    g = o.SplitMix64(21); P1 = o.g1_from(o.g1_consecutive(g.field(), 40)); P2 = o.g2_from(o.g2_consecutive(g.field(), 24))
    P1 += [o.g1_op("neg", p) for p in P1] + [None]; P2 += [o.g2_op("neg", p) for p in P2] + [None]
    for p in P1: assert km.decompress_g1_model(*km.compress_g1(p)) == p
    for p in P2: assert km.decompress_g2_model(*km.compress_g2(p)) == p
    assert {km.compress_g1(p)[1] for p in P1} == {0, 1, 2} == {km.compress_g2(p)[1] for p in P2}        # both parities occur, for the same x

def test_square_test_in_fq2_agrees_with_the_oracle():
    g = o.SplitMix64(22); els = [(0, 0), (Q - 1, 0), (0, 1), (4, 0), (0, 5)] + [(g.field() % Q, g.field() % Q) for _ in range(40)]
    for a in els:
        y = o.fq2_op("sqrt", a); assert (y is not None) == km.fq2_is_square(a), a
        if y is not None: assert o.fq2_op("sqr", y) == a
