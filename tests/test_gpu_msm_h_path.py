"""The H query's one-pass MSM path on its own: k_hsort_bin / k_hsort_group / k_hacc_runs29 / k_hacc_combine29 (msm.cuh), k_hmarg29 / k_hbits29 (htail29.cuh) and the
flag-and-repeat logic of MsmImpl::finish_sync, against the plain-integer model of tests/msm_h_model.py and the CPU oracle.

Every object is ResidentMsm(1, P, c, filter_ones=2) — the uniform-scalar hint.  The one-pass sort needs at most 20 digits a scalar, i.e. a window of 13 bits or more;
path() says which path an object takes, and general_path_repeats() whether a run was repeated on the two-pass path.  The points are (B0 + i) G, so the expected sum is
one scalar multiplication, (sum k_i (B0 + i) mod r) G; up to 3,000 points the oracle's MSM is compared as well.  Integer work: every comparison is exact.

Whether an input overflows the path (a group's region, or more than h_maxp pieces in a bucket) follows from the model's entries alone (msm_h_model.overflow_expected):
the tests assert the repeat counter against that prediction, so an ordinary input that fell back — or a crowded one that did not — fails.  (The entries are those of
k_i + m_i r where the sort spreads the scalars over multiples of r: windows 13, 14, 18, 19, see msm_h_model.spread.)  path().flag is the flag
word the run raised: bit 0 from the sort and the accumulation / combine (overflow, or ZZ = 0 in a bucket sum), bit 1 with result-slot bits from the tail."""
import functools, json, os, subprocess, sys
import numpy as np
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import msm_h_model as hm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R_MOD
B0 = (1 << 45) + 0x5eed                                                                           # far above n^2: no partial sum of a bucket is +-its next operand by accident
WINDOWS = [13, 14, 15, 16, 17, 18, 19]

@functools.lru_cache(maxsize=None)
def consecutive(n):
    P = o.g1_consecutive(B0, n); P.setflags(write=False); return P
@functools.lru_cache(maxsize=None)
def gen(): return o.g1_gen()
def mul_g(s): s %= R; return None if s == 0 else o.g1_op("mul", gen(), k=s)
def linear_sum(ks, skip=()): return mul_g(sum(k * (B0 + i) for i, k in enumerate(ks) if i not in skip))
def rand_scalars(seed, n): g = o.SplitMix64(seed); return [g.field() for _ in range(n)]
_MODEL = {}                                                                                       # the model's entries per scalar vector: computed once
def _key(ks, n, c, inf): return (n, c, hash(tuple(ks)), hash(tuple(inf)) if inf is not None else 0)
def entries_of(ks, n, c, inf=None):
    key = _key(ks, n, c, inf)
    if key not in _MODEL:
        if len(_MODEL) > 8: _MODEL.clear()
        _MODEL[key] = hm.expected_entries(inf if inf is not None else [0] * n, ks, n, c)
    return _MODEL[key]
def tail_coincidence(ks, n, c, inf=None):
    """the test points are in arithmetic progression, so P_a + P_b = P_c + P_d whenever a + b = c + d in one window — and where few entries meet (sparse buckets) two
    partial sums of the tail are now and then the same point: a true doubling, which the path must and does flag (msm_h_model.tail_degenerate walks the tail's
    additions).  A key holds no such relations; scalars that run into one are not what these tests call ordinary.  (Not looked for where buckets hold more than
    two entries on average: equal sums then need equal numbers of entries per window as well)"""
    if n * hm.num_windows(c) > 2 << (c - 1): return []
    key = ("tail",) + _key(ks, n, c, inf)
    if key not in _MODEL: _MODEL[key] = hm.tail_degenerate({b: hm.bucket_scalar(es, n, c, B0) for b, es in entries_of(ks, n, c, inf).items()}, 1 << (c - 1))
    return _MODEL[key]
def full_scalars(seed, n, c, inf=None):
    """uniform scalars of full width (below 2^253), free of such coincidences: the next seed of a fixed sequence otherwise"""
    while True:
        ks = rand_scalars(seed, n)
        if not tail_coincidence(ks, n, c, inf): return ks
        seed += 1000003
def spread_scalars(seed, n, c, inf=None):
    """the tests' ordinary input: uniform scalars of full width, free of coincidences (full_scalars).  The sort spreads them over multiples of r where the top
    window is narrow (msm_h_model.spread), so they fill every window's buckets evenly at every window size"""
    return full_scalars(seed, n, c, inf)
def with_low_digits(i, c, pattern):
    """a scalar for index i whose sorted form k + m_i r has the digits of `pattern` in every window but the top one"""
    return (pattern - hm.multiple(i, c) * R) % (1 << (c * (hm.num_windows(c) - 1)))
def plain_indices(c, count, start=0):
    """the first `count` indices from `start` on whose scalars the sort leaves as they are (m_i = 0)"""
    out = []; i = start
    while len(out) < count:
        if hm.multiple(i, c) == 0: out.append(i)
        i += 1
    return out
def neg(pt):                                                                                      # (x, -y) on the stored words
    r = pt.copy(); r[4:] = o.limbs((o.Q_MOD - o.from_arr(pt)[1]) % o.Q_MOD); return r

def check_path(m, n, c, run=None):
    """path() against the model's restatement of the constructor; returns the model's shape"""
    p = m.path(); s = hm.hsort_shape(n, c, run); assert s is not None and p.one_pass, (c, n, vars(p))
    for k in ("c", "W", "NB", "groups", "low_bits", "idx_bits", "region", "h_run", "h_maxp", "htail29"): assert getattr(p, k) == s[k], (k, vars(p), s)
    t = hm.htail_shape(s["NB"])
    for k in t: assert getattr(p, k) == t[k], (k, vars(p), t)
    assert p.WB == 1 and p.RS == t["top"] + 1
    return s

def run_and_check(m, ks, expect, repeats=0):
    """one run on scalars ks: the sum, and by how much the repeat counter moved (repeats = None: once or not at all)"""
    before = e.general_path_repeats(); m.set_scalars(o.to_arr(ks)); got = o.g1_from(m.run())[0]
    assert got == expect; moved = e.general_path_repeats() - before; assert moved == repeats or (repeats is None and moved in (0, 1)), "repeats of the general path: %d, expected %d (flag word 0x%x)" % (moved, -1 if repeats is None else repeats, m.path().flag)

def model_overflow(ks, n, c, shape, inf=None, run=None):
    return int(hm.overflow_expected(entries_of(ks, n, c, inf), shape, run))
def model_repeats(ks, n, c, shape, inf=None, run=None):
    """how often the run is repeated on the general path, on the consecutive test points: once if the path overflows or the tail meets a coincidence (above)"""
    return int(bool(model_overflow(ks, n, c, shape, inf, run) or tail_coincidence(ks, n, c, inf)))

# ---- shapes -------------------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(c, n) for c in WINDOWS for n in (1, 2, 511, 512, 513, 3000)] + [(13, 40000), (16, 70000), (19, 70000)]

@pytest.mark.parametrize("c,n", SHAPES)
def test_every_window_and_size_takes_the_one_pass_path_and_sums_right(c, n):
    """windows 13..19 x sizes around one sort workgroup (512 scalars), and three larger ones (every bucket of window 13 filled; windows 16 and 19 sparse): the shape the
    object reports is the model's, random scalars stay on the fast path, the sum is exact, and the combine ran with the lanes the model expects"""
    P = consecutive(n); m = e.ResidentMsm(1, P, c, filter_ones=2); s = check_path(m, n, c)
    print("shape c=%d n=%d: %s" % (c, n, vars(m.path())))
    ks = spread_scalars(100 * c + n, n, c); exp = linear_sum(ks); assert model_repeats(ks, n, c, s) == 0
    if n <= 3000: assert exp == o.msm_g1(P, o.to_arr(ks))
    run_and_check(m, ks, exp); assert m.path().ll == hm.combine_lanes(n, c, s["h_run"]) == 1
    # once more on the same object, other scalars
    ks = full_scalars(100 * c + n + 1, n, c); exp = linear_sum(ks); assert model_overflow(ks, n, c, s) == 0
    if n <= 3000: assert exp == o.msm_g1(P, o.to_arr(ks))
    run_and_check(m, ks, exp); m.close()

@pytest.mark.parametrize("c,n", SHAPES)
def test_full_width_random_scalars_stay_on_the_one_pass_path(c, n):
    """An ordinary input — uniform scalars of full width — must not fall back, at any window.  The last window holds only 254 - c (W - 1) bits of a scalar — 7, 2,
    14, 14, 16, 2, 7 for c = 13..19 — so at c = 14 / 18 its n digits would land in buckets 0..2 and at c = 13 / 19 in buckets 0..96, far beyond a region and
    h_maxp sized for n W / NB entries a bucket: before the sort spread such scalars over multiples of r (msm.cuh: hsort_spread) this failed at c = 13 (n = 3,000;
    40,000), c = 14 and 18 (n = 511 to 3,000) and c = 19 (n = 3,000; 70,000) — 872 entries in a bucket sized for 364 at (13, 40,000), 72,990 in a region of 5,888
    at (19, 70,000) — and every H query of a realistic size was repeated on the general path at those windows"""
    P = consecutive(n); m = e.ResidentMsm(1, P, c, filter_ones=2); check_path(m, n, c); ks = full_scalars(100 * c + n, n, c); run_and_check(m, ks, linear_sum(ks)); m.close()

@pytest.mark.parametrize("c", [12, 20])
def test_windows_outside_13_to_19_take_the_two_pass_path(c):
    n = 300; P = consecutive(n); m = e.ResidentMsm(1, P, c, filter_ones=2); assert hm.hsort_shape(n, c) is None and not m.path().one_pass
    ks = rand_scalars(c, n); exp = linear_sum(ks); assert exp == o.msm_g1(P, o.to_arr(ks)); run_and_check(m, ks, exp); m.close()   # (complete formulas: nothing to repeat)

# ---- scalars at the digit boundaries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 513])
@pytest.mark.parametrize("c", WINDOWS)
def test_scalars_at_the_digit_boundaries(c, n):
    """all 2^(c-1) (the one digit that stays positive: bucket NB - 1), all 2^(c-1) + 1 (negative, with a carry), all 2^c - 1 (-1 and a carry), r - 1 - i (19 or 20
    full digits), a single scalar at either end, all zero; then random scalars on the same object.  Equal scalars pile n entries into one bucket: 40 of them fit its
    pieces, 513 do not and must come out right through the repeat — as the model predicts for each vector"""
    P = consecutive(n); m = e.ResidentMsm(1, P, c, filter_ones=2); s = check_path(m, n, c); half = 1 << (c - 1)
    first = [0] * n; first[0] = R - 2; last = [0] * n; last[n - 1] = half + 1
    vectors = {"half": [half] * n, "half+1": [half + 1] * n, "full-1": [(1 << c) - 1] * n, "r-1-i": [R - 1 - i for i in range(n)], "first": first, "last": last, "zero": [0] * n}
    for name, ks in vectors.items():
        rep = model_repeats(ks, n, c, s)
        if name in ("first", "last", "zero") or (n == 40 and hm.spread(c) == 1 and name in ("half", "half+1")): assert rep == 0, name   # (40 entries in a bucket: at most four pieces of 14)
        if n == 513 and hm.spread(c) == 1 and name in ("half", "half+1", "full-1", "r-1-i"): assert rep == 1, name   # (r - 1 - i: the digits above window 0 are the same for every i; where the sort spreads the scalars, equal ones no longer share their buckets)
        exp = linear_sum(ks); assert exp == o.msm_g1(P, o.to_arr(ks)) and (name != "zero" or exp is None), name
        # (equal or consecutive scalars on consecutive points: partial sums INSIDE a bucket can be the same point too — P_a - P_b = P_c - P_d whenever a - b = c - d —
        #  and the order inside a bucket is not fixed: where the model sees no reason for a repeat, these vectors may still meet one.  A lone scalar or none cannot)
        run_and_check(m, ks, exp, rep if rep == 1 or name in ("first", "last", "zero") else None)
    ks = spread_scalars(7 * c + n, n, c); run_and_check(m, ks, linear_sum(ks)); m.close()

# ---- run lengths and combine lanes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [4, 11, 14, 15, 64])
def test_run_lengths(run, monkeypatch):
    """ZK_MSM_H_RUN (read per object): the three regimes' lengths, the shortest and the longest the switch takes"""
    monkeypatch.setenv("ZK_MSM_H_RUN", str(run)); c, n = 13, 3000; P = consecutive(n); m = e.ResidentMsm(1, P, c, filter_ones=2); s = check_path(m, n, c, run)
    assert m.path().h_run == run == m.path().run_in_effect
    for seed in (1, 2):
        ks = spread_scalars(seed * 1000 + run, n, c); exp = linear_sum(ks); assert exp == o.msm_g1(P, o.to_arr(ks)) and model_repeats(ks, n, c, s) == 0; run_and_check(m, ks, exp)
    m.close()

@pytest.mark.parametrize("n,ll", [(16384, 2), (40000, 3)])
def test_combine_with_four_and_eight_lanes(n, ll, monkeypatch):
    """runs of 4 at window 13: 20 and 48 pieces a bucket, which the combine shares among 4 and 8 lanes (the 8-lane form is otherwise reached by the depth-32 deposit only)"""
    monkeypatch.setenv("ZK_MSM_H_RUN", "4"); c = 13; P = consecutive(n); m = e.ResidentMsm(1, P, c, filter_ones=2); s = check_path(m, n, c, 4)
    ks = spread_scalars(n, n, c); assert model_repeats(ks, n, c, s) == 0; run_and_check(m, ks, linear_sum(ks)); assert m.path().ll == ll == hm.combine_lanes(n, c, 4)
    m.close()

@pytest.mark.parametrize("c,n", [(13, 3000), (16, 3000), (16, 70000)])
def test_crowded_runs_on_an_object_sized_for_short_ones(c, n):
    """set_crowded: runs of 40 while the pieces are laid out by h_maxp, sized for runs of 14 — back and forth on one object: the piece index of the accumulation and the
    piece count of the combine must agree at either length"""
    P = consecutive(n); m = e.ResidentMsm(1, P, c, filter_ones=2); s = check_path(m, n, c)
    for i, on in enumerate((True, False, True)):
        m.set_crowded(on); run = 40 if on else s["h_run"]; assert m.path().run_in_effect == run and m.path().h_maxp == s["h_maxp"]
        ks = spread_scalars(40 + i + n, n, c); assert model_repeats(ks, n, c, s, run=run) == 0; run_and_check(m, ks, linear_sum(ks))
        assert m.path().ll == hm.combine_lanes(n, c, run)
    m.close()

# ---- key points at infinity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [13, 16])
def test_key_points_at_infinity(c):
    """zero rows in the key (k_hacc_runs29<1>, and the sort's skip): at both ends, around the wave and workgroup boundaries of the sort, and 30 random places"""
    n = 3000; rng = np.random.default_rng(c); holes = sorted({0, n - 1, 255, 256, 511, 512} | set(int(x) for x in rng.integers(0, n, size=30)))
    P = consecutive(n).copy(); P[holes] = 0; m = e.ResidentMsm(1, P, c, filter_ones=2); s = check_path(m, n, c); assert m.path().any_inf == 1
    inf = [int(i in holes) for i in range(n)]
    for seed in (5, 6):
        ks = spread_scalars(seed + c, n, c, inf); exp = o.msm_g1(P, o.to_arr(ks)); assert exp == linear_sum(ks, skip=set(holes)); assert model_repeats(ks, n, c, s, inf) == 0
        run_and_check(m, ks, exp)
    m.close()
    m = e.ResidentMsm(1, np.zeros((n, 8), dtype=np.uint64), c, filter_ones=2); assert m.path().one_pass; run_and_check(m, rand_scalars(9, n), None); m.close()   # nothing but infinity: no entries at all

# ---- run_product ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [13, 16])
def test_run_product_and_its_materialising_fallback(c):
    """scalars a_i b_i z formed inside the sort kernel (runtime digit walk at window 13, the compiled-in one at 16), z one element and a table, with b and z random and
    a chosen so that the products are the spread scalars t_i; a product that is the same for every i overflows, and the repeat on the two-pass path must materialise
    it first (k_fr_mul3)"""
    n = 3000; P = consecutive(n); m = e.ResidentMsm(1, P, c, filter_ones=2); s = check_path(m, n, c)
    t = spread_scalars(31 + c, n, c); b = rand_scalars(32, n); z = rand_scalars(33, n); t[7] = 0
    def run(t, b, z, repeats):
        zs = z if len(z) == n else z * n; a = [x * pow(y * w, -1, R) % R for x, y, w in zip(t, b, zs)]; assert model_repeats(t, n, c, s) == repeats
        before = e.general_path_repeats(); got = o.g1_from(m.run_product(o.to_arr(a), o.to_arr(b), o.to_arr(z)))[0]
        assert got == linear_sum(t) == o.msm_g1(P, o.to_arr(t)); assert e.general_path_repeats() == before + repeats
    run(t, b, z[:1], 0); run(t, b, z, 0)
    same = [0x1234567 << 40 | 3] * n; run(same, b, [1], 1); run(same, b, z, 1); run(t[::-1], z, b[1:2], 0)
    ks = spread_scalars(34, n, c); run_and_check(m, ks, linear_sum(ks)); m.close()               # a plain run afterwards: no product left behind

# ---- the sort and the bucket sums against the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n", [(13, 300), (16, 513), (19, 300)])
def test_sort_stage_and_bucket_sums_against_the_model(c, n):
    """random scalars with a few zeros, the three boundary digits and two key points at infinity: per bucket the count, the offset (group x region + the counts
    before it inside the group), the entries as a set (their order inside a bucket is not fixed); per group its number of entries; and every bucket sum — a
    Point29Rec on 29-bit limbs — decodes to s_b G with s_b from the model's entries, empty buckets to the point at infinity"""
    half = 1 << (c - 1); P = consecutive(n).copy(); holes = (5, n - 2); P[list(holes)] = 0; inf = [int(i in holes) for i in range(n)]
    seed = c * n
    while True:
        ks = rand_scalars(seed, n); ks[0] = 0; ks[17] = 0; ks[n - 1] = 0; ks[4] = R - 1; ks[5] = 77
        for i, pattern in ((1, half), (2, half + 1), (3, (1 << c) - 1), (6, sum(half << (c * w) for w in range(hm.num_windows(c) - 1)))):
            ks[i] = with_low_digits(i, c, pattern)                                                # (the last: every digit 2^(c-1): bucket NB - 1 in every window, never negative)
        if not tail_coincidence(ks, n, c, inf): break
        seed += 1000003
    m = e.ResidentMsm(1, P, c, filter_ones=2); s = check_path(m, n, c); ent = entries_of(ks, n, c, inf); assert not hm.overflow_expected(ent, s)
    run_and_check(m, ks, linear_sum(ks, skip=set(holes)))
    counts, offsets, group_n = hm.layout(ent, s); NB = s["NB"]
    got_counts = m.h_state("counts"); got_offsets = m.h_state("offsets"); got_entries = m.h_state("entries"); hb = m.h_state("hb29").reshape(NB, 48)
    assert got_counts.tolist() == counts and got_offsets.tolist() == offsets and m.h_state("group_n").tolist() == group_n
    assert {(0, 1), (0, 6)} | {(0, 6 + w * n) for w in range(hm.num_windows(c) - 1)} <= ent[NB - 1] and (1, 2) in ent[NB - 2] and (1, 3) in ent[0]   # the boundary digits
    for b, es in ent.items():
        dec = [hm.decode_entry(x, s["idx_bits"]) for x in got_entries[offsets[b]:offsets[b] + counts[b]]]
        assert all(lo == b & ((1 << s["low_bits"]) - 1) for lo, _, _ in dec), b; assert len(dec) == len(es) and {(sg, ix) for _, sg, ix in dec} == es, b
    empty = np.array([cnt == 0 for cnt in counts]); assert not hb[empty][:, 24:33].any()       # all-zero ZZ limbs: infinity
    for b, es in ent.items(): assert hm.point29_affine(hb[b]) == mul_g(hm.bucket_scalar(es, n, c, B0)), b
    m.close()

# ---- degenerate operands on the real path -----------------------------------------------------------------------------------------------------------------
def avoiding(ks, c, weights):
    """the scalars with every one replaced (by the next in a fixed sequence) whose digits, as the sort takes them, hit a bucket of one of these weights"""
    g = o.SplitMix64(4711); out = []
    for i, k in enumerate(ks):
        while any(abs(d) in weights for d in hm.signed_digits(hm.sorted_scalar(k, i, c), c)): k = g.field()
        out.append(k)
    return out

def degenerate_cases(c):
    """name -> (points, scalars, repeats: 1 = the flag must be raised, None = either way, the index that sits out afterwards or None)"""
    n = 600; base = consecutive(3000); K = rand_scalars(4105 + c, 3000); L = 1 << hm.htail_shape(1 << (c - 1))["lo_bits"]; cases = {}
    P = base[:n].copy(); S = K[:n]; classes = {}
    for i in range(n): classes.setdefault(hm.multiple(i, c), []).append(i)                        # (pairs among the indices whose scalars the sort takes alike: all of them at window 16)
    for idx in classes.values():
        for i, j in zip(idx[0::2], idx[1::2]): P[j] = P[i]; S[j] = S[i]
    cases["a: pairs of equal points, equal scalars"] = (P, S, 1, None)
    P = base[:400].copy(); S = K[:400]
    for i in range(0, 400, 2): P[i + 1] = neg(P[i]); S[i + 1] = S[i]
    cases["b: P, -P with equal scalars: the sum is infinity"] = (P, S, None, None)
    cases["c: every point equal, random scalars"] = (np.repeat(base[:1], n, axis=0), K[:n], 1, None)
    P = base.copy(); S = list(K); P[100:200] = P[99]; S[100:150] = [S[99]] * 50
    for i in range(1000, 1100, 2): P[i + 1] = neg(P[i]); S[i + 1] = S[i]
    cases["d: a mixture inside an ordinary query"] = (P, S, None, None)
    # one entry a bucket in window 0, every bucket sum the same point: the accumulation and the combine add nothing, the TAIL meets P + P (k_hmarg29: the column's
    # quads meet in the tree) and k_hbits29 must find ZZ = 0 in a result slot.  (The scalars 1..n sit at the indices the sort leaves as they are; the rest are zero)
    plain = plain_indices(c, n, 0); N = plain[-1] + 1; S = [0] * N
    for j, i in enumerate(plain): S[i] = j + 1
    cases["e: every point equal, scalars 1..n"] = (np.repeat(base[:1], N, axis=0), S, 1, None)
    # P in the bucket of weight 4, -P in the one of weight 16 L + 4 — the same column, and the two buckets quad 0 of that column's workgroup adds first (rows 0 and
    # 16) — with nothing else in either: the tail meets P + (-P), which its incomplete addition leaves as ZZ = 0
    i1, i2 = plain_indices(c, 2, 10)
    P = base[:n].copy(); P[i2] = neg(P[i1]); S = K[:n]; S[i1] = 0; S[i2] = 0; S = avoiding(S, c, {4, 16 * L + 4}); S[i1] = 4; S[i2] = 16 * L + 4
    cases["f: P and -P alone in two buckets the tail adds to each other"] = (P, S, 1, i2)
    # (the same with weights 4 and 8: different columns and no common weight bit, so nothing adds the two to each other)
    P = base[:n].copy(); P[i2] = neg(P[i1]); S = K[:n]; S[i1] = 4; S[i2] = 8
    cases["f0: P with scalar 4, -P with scalar 8 amid ordinary points"] = (P, S, None, i2)
    return cases

@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f", "f0"])
@pytest.mark.parametrize("c", [13, 16])
def test_degenerate_operands_raise_the_flag_once_and_stay_exact(c, case):
    """inputs a key may legally hold and the incomplete additions of this path cannot add: ZZ = 0 (mod q) must reach k_hacc_combine29's or k_hbits29's check, the MSM
    is repeated once with complete formulas, the sum is the oracle's — and ordinary scalars on the same object afterwards stay on the fast path, exact"""
    name, (P, S, repeats, out) = next((k, v) for k, v in degenerate_cases(c).items() if k.split(":")[0] == case); n = len(P)
    m = e.ResidentMsm(1, P, c, filter_ones=2); s = check_path(m, n, c)
    if repeats is not None: assert model_overflow(S, n, c, s) == 0, name                          # nothing here overflows: a repeat is the degenerate-sum flag's doing
    exp = o.msm_g1(P, o.to_arr(S)); assert (exp is None) == (case == "b"), name
    before = e.general_path_repeats(); m.set_scalars(o.to_arr(S)); got = o.g1_from(m.run())[0]; moved = e.general_path_repeats() - before
    flag = m.path().flag; print("degenerate case %r at window %d: %d repeat(s), flag word 0x%x" % (name, c, moved, flag))
    assert got == exp, name; assert moved == repeats if repeats is not None else moved in (0, 1), (name, moved)
    assert (flag != 0) == (moved == 1), (name, hex(flag))
    # who noticed: equal points inside a bucket are k_hacc_combine29's to find (bit 0; nothing overflows here, see above) — without its check only the tail's would
    # be left; in e and f every bucket holds distinct points, and it is k_hbits29 alone that finds ZZ = 0, in the result slots it says (bit 1, slots from bit 8 on)
    if case in ("a", "c"): assert flag & 1, (name, hex(flag))
    if case in ("e", "f"): assert flag & 3 == 2 and flag >> 8, (name, hex(flag))
    if case == "f": assert flag == 2 | 1 << (8 + 2), (name, hex(flag))                            # column 4 enters the sum of weight bit 2 and no other
    S2 = spread_scalars(4106, n, c, [int(i == out) for i in range(n)])
    if case in ("c", "e"): run_and_check(m, S2, o.msm_g1(P, o.to_arr(S2)), 1)                     # (a key of equal points is degenerate under any scalars: flagged again, exact again)
    elif case in ("f", "f0"): S2[out] = 0; run_and_check(m, S2, o.msm_g1(P, o.to_arr(S2)))         # (-P sits out: an ordinary run, and it must not fall back)
    else: m.set_scalars(o.to_arr(S2)); assert o.g1_from(m.run())[0] == o.msm_g1(P, o.to_arr(S2)), name   # (equal or opposite points may or may not share a bucket)
    m.close()
    m = e.ResidentMsm(1, consecutive(n), c, filter_ones=2); run_and_check(m, S2, linear_sum(S2)); m.close()   # the same scalars on an ordinary key: no repeat

# ---- natural overflow -----------------------------------------------------------------------------------------------------------------------------------------
def test_natural_overflow_of_pieces_and_of_a_region():
    """no hook: every scalar equal (sorted as 16 different values at this window, 187 entries each in one bucket a window: more than h_maxp pieces) and scalars whose
    digits all fall into the 16 buckets of one group (those the sort leaves as they are bring 3,500 entries for a region of 1,536): the oracle's sum through exactly
    one repeat, and random scalars afterwards stay on the fast path"""
    c, n = 13, 3000; P = consecutive(n); m = e.ResidentMsm(1, P, c, filter_ones=2); s = check_path(m, n, c); g = o.SplitMix64(99)
    same = [0x1234567 << 40 | 3] * n
    one_group = [sum((((5 << s["low_bits"]) | int(g.next() % (1 << s["low_bits"]))) + 1) << (c * w) for w in range(s["W"] - 1)) for _ in range(n)]
    ent = hm.expected_entries([0] * n, one_group, n, c); assert sum(len(v) for b, v in ent.items() if b >> s["low_bits"] == 5) > s["region"]   # (the scalars the sort leaves as they are: one in 16)
    for i, ks in enumerate((same, one_group)):
        assert model_repeats(ks, n, c, s) == 1; exp = linear_sum(ks); assert exp == o.msm_g1(P, o.to_arr(ks)); run_and_check(m, ks, exp, 1); assert m.path().flag & 1
        ks = spread_scalars(200 + i, n, c); assert model_repeats(ks, n, c, s) == 0; run_and_check(m, ks, linear_sum(ks))
    m.close()

# ---- ZK_MSM_H_WINDOW through the prover ---------------------------------------------------------------------------------------------------------------------
PROVE_CODE = """
import json, sys
sys.path.insert(0, %r)
from blockmaze_amd import engine as e
import numpy as np
def rd(p):
    b = open(p, 'rb').read(); n = int(np.frombuffer(b, dtype=np.uint64, count=1)[0]); return np.frombuffer(b, dtype=np.uint64, count=4 * n, offset=8).reshape(n, 4).copy()
out = []
for pk, wit, r, s in json.loads(sys.argv[1]):
    p = e.Prover(pk); z = rd(wit); out.append(p.prove(z, int(r, 16), int(s, 16))); out.append(p.prove(z, int(r, 16), int(s, 16))); p.close()
print('PROOFS ' + json.dumps(out))
"""

@pytest.mark.parametrize("window", [13, 15, 17, 19])
def test_h_window_switch_gives_the_reference_proof_bytes(window, golden_dir):
    """the shipped switch ZK_MSM_H_WINDOW, in a fresh process each (the prover reads it once): both golden circuits, proved twice, give the reference prover's bytes"""
    jobs = []; exp = []
    for name in ("groth16_small", "groth16_step"):
        d = os.path.join(golden_dir, name); meta = json.load(open(os.path.join(d, "meta.json"))); jobs.append([os.path.join(d, "pk.txt"), os.path.join(d, "wit.bin"), meta["r"], meta["s"]]); exp += [meta["proof"]] * 2
    r = subprocess.run([sys.executable, "-c", PROVE_CODE % ROOT, json.dumps(jobs)], capture_output=True, text=True, env=dict(os.environ, ZK_MSM_H_WINDOW=str(window)), timeout=120)
    line = [l for l in r.stdout.splitlines() if l.startswith("PROOFS ")]; assert line, r.stderr[-2000:]
    assert json.loads(line[0][7:]) == exp
