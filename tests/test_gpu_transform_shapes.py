"""The transforms at the tile shapes no other test reaches (csrc/gpu.hip ntt_two_pass_launch picks the shape from log n: two columns a tile at 2^12 .. 2^20, an
11-stage row tile without the second column at 2^21, 11-stage tiles in both passes at 2^22; the stage-per-launch path beyond): exact against the oracle at 2^17,
2^19, 2^20, 2^21, 2^22 and the step domain 2^21 + 2^19; the top of the field on the 11-stage tiles against closed forms on Python integers; the coset forms at 2^23.
Integer work: every comparison is bit-exact.  One oracle call above 2^20 a test; its share of the time goes to the summary line (conftest.record_leg)."""
import functools, itertools, random, time
import numpy as np
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
from conftest import record_leg

pytestmark = pytest.mark.gpu
R = o.R_MOD
OPS = ("fft", "ifft", "cosetfft", "icosetfft")
STEP = (1 << 21) + (1 << 19)

@functools.lru_cache(maxsize=1)
def full_width(m):
    """one seeded vector a size, read-only: canonical values over the whole width (a top limb below r's own top limb, the other three limbs anything)"""
    n = o.domain_size(m); assert n == e.domain_size(m) == m; rng = np.random.default_rng(m); a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, R >> 192, size=n, dtype=np.uint64); a.setflags(write=False); return a

def against_oracle(m, op):
    a = full_width(m); t0 = time.time(); exp = o.domain_op(op, m, a); t_o = time.time() - t0
    record_leg("oracle %s at m = %d" % (op, m), t_o)
    assert np.array_equal(e.domain_transform(m, op, a), exp), (m, op)

@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("m", [1 << 17, 1 << 19, 1 << 20])
def test_two_column_tiles_match_the_oracle(m, op): against_oracle(m, op)

@pytest.mark.parametrize("op", ["fft", "icosetfft"])
@pytest.mark.parametrize("m", [1 << 21, 1 << 22, STEP])
def test_eleven_stage_tiles_match_the_oracle(m, op): against_oracle(m, op)

@pytest.mark.parametrize("m", [1 << 21, 1 << 22, STEP])
def test_eleven_stage_tiles_round_trips(m):
    """with fft and icosetfft exact on this vector (the test above), ifft(fft(a)) == a pins ifft on fft(a), and cosetfft(icosetfft(a)) == a pins cosetfft on
    icosetfft(a)"""
    a = full_width(m)
    assert np.array_equal(e.domain_transform(m, "ifft", e.domain_transform(m, "fft", a)), a)
    assert np.array_equal(e.domain_transform(m, "cosetfft", e.domain_transform(m, "icosetfft", a)), a)

# ---- the top of the field on the 11-stage tiles, against closed forms -------------------------------------------------------------------------------------------
def root_of_unity(n): s = n.bit_length() - 1; assert n == 1 << s; return pow(pow(5, (R - 1) >> 28, R), 1 << (28 - s), R)   # alt_bn128_init.cpp:112-116, squared down to order n
@functools.lru_cache(maxsize=1)
def coset_generator():
    """Fr::multiplicative_generator as the oracle has it: cosetfft of (0, 1) on the domain of size 2 is (g, -g)"""
    out = o.from_arr(o.domain_op("cosetfft", 2, o.to_arr([0, 1]))); assert (out[0] + out[1]) % R == 0; return out[0]
def ints_of(a): b = a.tobytes(); return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
def row_of(v): return np.array(o.limbs(v % R), dtype=np.uint64)
def sparse(n, entries):
    a = np.zeros((n, 4), dtype=np.uint64)
    for k, v in entries.items(): a[k] = row_of(v)
    return a

@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n", [1 << 21, 1 << 22])
def test_top_of_the_field_on_the_eleven_stage_tiles(n, op):
    """The patterns of test_gpu_engine.py's top-of-field test with t = r - 1, where the oracle takes seconds: closed forms instead.  With w the root of unity of
    order n, g the coset generator, x_k = g w^k and G = g^n:
      every element t:          fft -> n t at 0;  ifft -> t at 0;  icosetfft -> t at 0;  cosetfft -> t (G - 1) / (x_k - 1) at every k
      t at the odd indices:     fft -> (n/2) t at 0 and -(n/2) t at n/2;  ifft -> t/2 and -t/2 there;  icosetfft -> t/2 at 0, -t/2 g^(-n/2) at n/2;
                                cosetfft -> t x_k (G - 1) / (x_k^2 - 1) at every k
      t at index j:             fft -> t w^(jk);  ifft -> t w^(-jk) / n;  cosetfft -> t g^j w^(jk);  icosetfft -> t w^(-jk) g^(-k) / n
    Every index for the two constant patterns (the dense cosetfft ones by multiplying out the denominator), 64 seeded indices and the corners for the impulses."""
    t = R - 1; w = root_of_unity(n); g = coset_generator(); ninv = pow(n, -1, R); h = n // 2; assert pow(w, h, R) == R - 1
    every = np.tile(row_of(t), (n, 1)); odd = np.zeros((n, 4), dtype=np.uint64); odd[1::2] = row_of(t)
    got_all = e.domain_transform(n, op, every); got_odd = e.domain_transform(n, op, odd)
    if op != "cosetfft":
        exp_all = {"fft": {0: n * t}, "ifft": {0: t}, "icosetfft": {0: t}}[op]
        half = t * pow(2, -1, R); exp_odd = {"fft": {0: h * t, h: -h * t}, "ifft": {0: half, h: -half}, "icosetfft": {0: half, h: -half * pow(g, -h, R)}}[op]
        assert np.array_equal(got_all, sparse(n, exp_all)), "every element"
        assert np.array_equal(got_odd, sparse(n, exp_odd)), "alternating"
    else:
        G1 = (pow(g, n, R) - 1) % R; c = t * G1 % R; xs = itertools.accumulate(itertools.repeat(w, n - 1), lambda x, ww: x * ww % R, initial=g)
        bad = [k for k, (x, ya, yo) in enumerate(zip(xs, ints_of(got_all), ints_of(got_odd))) if ya >= R or yo >= R or ya * (x - 1) % R != c or (yo * (x * x - 1) - c * x) % R]
        assert not bad, bad[:8]
    rng = random.Random(n); ks = [0, 1, h, n - 1] + [rng.randrange(n) for _ in range(64)]
    for j in (0, 1, n - 1):
        a = np.zeros((n, 4), dtype=np.uint64); a[j] = row_of(t); got = e.domain_transform(n, op, a)
        for k in ks:
            exp = {"fft": t * pow(w, j * k, R), "ifft": t * pow(w, -j * k, R) * ninv, "cosetfft": t * pow(g, j, R) * pow(w, j * k, R), "icosetfft": t * pow(w, -j * k, R) * pow(g, -k, R) * ninv}[op] % R
            assert o.from_arr(got[k:k + 1])[0] == exp, (j, k)

# ---- beyond the tiles -------------------------------------------------------------------------------------------------------------------------------------------
def test_coset_forms_beyond_two_pass_tiles():
    """2^23 points, the stage-per-launch path, which folds the coset factors and the 1 / n into its pre_scale table: cosetfft of unit impulses at 1 and 12,345 is
    g w^k + g^12345 w^(12345 k), and icosetfft undoes cosetfft on that vector and on a dense one"""
    m = 1 << 23; w = root_of_unity(m); g = coset_generator(); a = np.zeros((m, 4), dtype=np.uint64); a[1, 0] = 1; a[12345, 0] = 1; f = e.domain_transform(m, "cosetfft", a)
    for k in (0, 1, 2, 12345, m // 2, m - 1): assert o.from_arr(f[k:k + 1])[0] == (g * pow(w, k, R) + pow(g, 12345, R) * pow(w, 12345 * k, R)) % R, k
    assert np.array_equal(e.domain_transform(m, "icosetfft", f), a)
    d = np.random.default_rng(23).integers(0, 1 << 62, size=(m, 4), dtype=np.uint64); d[:, 3] >>= 2
    assert np.array_equal(e.domain_transform(m, "icosetfft", e.domain_transform(m, "cosetfft", d)), d)
