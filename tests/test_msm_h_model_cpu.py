"""The integer model of the H query's one-pass MSM path (tests/msm_h_model.py) checked on its own, without a GPU: the digits recompose to the scalar and keep to their
range at every window size the path accepts, the shape rules give the table worked out from MsmImpl's constructor, and the record decoder reads back what it is given."""
import os, random, re
import pytest
import field29_model as fm
import msm_h_model as hm

R = hm.R_MOD
WINDOWS = list(range(13, 20))

def all_digits(c, d):
    """a scalar below 2^253 whose digits are all d (a window value, 0 < d < 2^c) as far as they fit"""
    return sum(d << (c * w) for w in range(hm.num_windows(c))) & ((1 << 253) - 1)

def boundary_scalars(c):
    half = 1 << (c - 1)
    return [0, 1, half, half + 1, (1 << c) - 1, R - 1, all_digits(c, half), all_digits(c, half + 1), all_digits(c, (1 << c) - 1), all_digits(c, half - 1)]

@pytest.mark.parametrize("c", WINDOWS + [10, 12, 20])
def test_digits_recompose_and_keep_to_their_range(c):
    rnd = random.Random(1300 + c); half = 1 << (c - 1); W = hm.num_windows(c)
    ks = boundary_scalars(c) + [rnd.randrange(R) for _ in range(1000)]
    for k in ks:
        d = hm.signed_digits(k, c); assert len(d) == W
        assert sum(x << (c * w) for w, x in enumerate(d)) == k, (c, k)                            # in particular: nothing carried out of the top window
        assert all(-(half - 1) <= x <= half for x in d), (c, k)
    # the digit 2^(c-1) itself stays positive (bucket NB - 1, sign clear); one more turns negative and carries
    assert hm.signed_digits(half, c)[:2] == [half, 0] and hm.signed_digits(half + 1, c)[:2] == [-(half - 1), 1]
    assert hm.signed_digits((1 << c) - 1, c)[:2] == [-1, 1]
    d = hm.signed_digits(all_digits(c, half), c); assert d[0] == half and all(x == half for x in d[:W - 1])
    d = hm.signed_digits(all_digits(c, half + 1), c); assert d[0] == -(half - 1) and all(x == -(half - 2) for x in d[1:W - 1])

def test_digit_rule_is_the_kernels():
    """the comparison the model restates is the one msm.cuh makes, in all three digit walks"""
    src = open(os.path.join(fm.CSRC, "msm.cuh")).read()
    assert src.count("if (d > half)") == 3 and "d >= half" not in src
    assert "return 254 / c + 1;" in src

def test_model_constants_are_the_sources():
    msm = open(os.path.join(fm.CSRC, "msm.cuh")).read(); tail = open(os.path.join(fm.CSRC, "htail29.cuh")).read()
    def const(src, name): return int(re.search(r"\b%s = (\d+)" % name, src).group(1))
    assert const(msm, "HSORT_GROUPS") == hm.HSORT_GROUPS and const(msm, "HSORT_GROUP_THREADS") == hm.HSORT_GROUP_THREADS
    assert const(msm, "HSORT_MAX_PER_THREAD") == hm.HSORT_MAX_PER_THREAD and const(msm, "HSORT_STAGE_W") == hm.HSORT_STAGE_W
    assert const(msm, "HSORT_BIN_THREADS") * const(msm, "HSORT_PER_THREAD") == hm.HSORT_TILE and const(tail, "HTAIL_CHUNK") == hm.HTAIL_CHUNK

def test_hsort_shape_table():
    sizes = [1, 2, 300, 513, 3000, 40000, 70000, 322639, 400000]
    for n in sizes:
        assert hm.hsort_shape(n, 12) is None                                                      # 22 windows: more than a scalar's staged entries
        assert hm.hsort_shape(n, 20) is None, n                                                   # 11 low bits with 256 groups; 34 entry bits with 512
    assert hm.hsort_shape(400000, 19) is None                                                     # 9 + 1 + 23 = 33 entry bits
    for c in WINDOWS:
        for n in (1, 513, 3000, 40000, 70000):
            s = hm.hsort_shape(n, c); assert s is not None, (c, n)
            assert s["groups"] << s["low_bits"] == s["NB"] == 1 << (c - 1) and s["W"] == 254 // c + 1 and s["htail29"]
            assert (1 << s["idx_bits"]) >= n * s["W"] and s["low_bits"] + 1 + s["idx_bits"] <= 32
            assert s["region"] % 256 == 0 and s["region"] >= n * s["W"] // s["groups"] + 1024 and s["h_run"] == 14
    s = hm.hsort_shape(3000, 13); assert (s["groups"], s["low_bits"], s["W"], s["idx_bits"], s["region"], s["h_maxp"]) == (256, 4, 20, 16, 1536, 6)
    s = hm.hsort_shape(3000, 19); assert (s["groups"], s["low_bits"]) == (256, 10)
    s = hm.hsort_shape(400000, 16); assert (s["groups"], s["low_bits"], s["idx_bits"], s["h_run"]) == (512, 6, 23, 11)
    assert hm.hsort_shape(40000, 13, h_run=4)["h_maxp"] == (195 + 97 + 32 + 3) // 4 + 2
    assert hm.default_run(12 << 20) == 11 and hm.default_run((12 << 20) + 1) == 15 and hm.default_run(6 << 20) == 14 and hm.default_run((6 << 20) + 1) == 11
    # pieces = n W / NB / run: 20 and 48 at run 4, window 13
    assert hm.combine_lanes(16384, 13, 4) == 2 and hm.combine_lanes(40000, 13, 4) == 3 and hm.combine_lanes(3000, 13, 14) == 1

def test_htail_shape_table():
    exp = {13: (12, 6, 6, 1, 64), 14: (13, 7, 6, 1, 64), 15: (14, 7, 7, 1, 64), 16: (15, 8, 7, 2, 64), 17: (16, 8, 8, 2, 256), 18: (17, 9, 8, 4, 256), 19: (18, 9, 9, 4, 256)}
    for c, (top, lo, hi, rc, blk) in exp.items():
        s = hm.htail_shape(1 << (c - 1)); assert (s["top"], s["lo_bits"], s["hi_bits"], s["row_chunks"], s["marg_block"]) == (top, lo, hi, rc, blk), c
        assert s["marg_count"] == (1 << lo) + (1 << hi) * rc + 1 and s["marg_blocks"] == (1 << lo) - 1 + ((1 << hi) - 1) * rc + 1
        assert (1 << lo) // rc <= hm.HTAIL_CHUNK                                                  # no row piece longer than a chunk

def test_expected_entries_and_bucket_scalars_add_up():
    """every entry stands for +-2^(c w) P_i: summed over all buckets with weight b + 1 the model's entries give back sum k_i (b0 + i)"""
    rnd = random.Random(7); n = 40; b0 = 991
    for c in (13, 16, 19):
        ks = [rnd.randrange(R) for _ in range(n)]; ks[3] = 0; low = 1 << (c * (hm.num_windows(c) - 1)); inf = [0] * n; inf[7] = 1
        ks[4] = ((1 << (c - 1)) - hm.multiple(4, c) * R) % low; ks[5] = ((1 << (c - 1)) + 1 - hm.multiple(5, c) * R) % low   # (the digits of k + m_i r, as the sort takes them)
        ent = hm.expected_entries(inf, ks, n, c)
        assert all(0 <= b < 1 << (c - 1) for b in ent) and all(idx % n not in (3, 7) for es in ent.values() for _, idx in es)
        assert (0, 4) in ent[(1 << (c - 1)) - 1] and (1, 5) in ent[(1 << (c - 1)) - 2] and (0, 5 + n) in ent[0]
        total = sum((b + 1) * hm.bucket_scalar(es, n, c, b0) for b, es in ent.items()) % R
        assert total == sum(k * (b0 + i) for i, k in enumerate(ks) if not inf[i]) % R
        assert sum(len(es) for es in ent.values()) == sum(1 for i, k in enumerate(ks) if not inf[i] and k for d in hm.signed_digits(hm.sorted_scalar(k, i, c), c) if d)

def test_entry_and_record_decoders():
    assert hm.decode_entry((5 << 17) | (1 << 16) | 1234, 16) == (5, 1, 1234) and hm.decode_entry(77, 20) == (0, 0, 77)
    rnd = random.Random(3)
    for _ in range(8):
        w, pt = fm.g1_acc(rnd)                                                                    # 36 words within the accumulation's invariant, and its affine point
        rec = sum((w[9 * k:9 * k + 9] + [0, 0, 0] for k in range(4)), []); assert hm.point29_affine(rec) == pt
    assert hm.point29_affine([0] * 48) is None
    keep = rec[:24] + [0] * 12 + rec[36:]; assert hm.point29_affine(keep) is None              # all-zero ZZ limbs: infinity, whatever the other slots hold
    bad = rec[:24] + fm.limbs29(fm.Q_MOD) + [0, 0, 0] + rec[36:]
    with pytest.raises(AssertionError): hm.point29_affine(bad)                                    # ZZ = q: zero mod q, not the point at infinity

def test_top_window_and_overflow_prediction():
    assert [hm.top_window_bits(c) for c in WINDOWS] == [7, 2, 14, 14, 16, 2, 7]
    s = hm.hsort_shape(3000, 13); assert (s["h_run"], s["h_maxp"], s["region"], s["low_bits"]) == (14, 6, 1536, 4)
    def ent(counts): return {b: {(0, 100000 * b + j) for j in range(k)} for b, k in counts.items()}
    counts, offsets, group_n = hm.layout(ent({0: 3, 1: 2, 15: 4, 16: 5, 4095: 1}), s)
    assert (counts[0], counts[1], counts[15], counts[16], counts[4095]) == (3, 2, 4, 5, 1) and (offsets[0], offsets[1], offsets[2], offsets[15], offsets[16], offsets[17]) == (0, 3, 5, 5, 1536, 1541)
    assert offsets[4095] == 255 * 1536 and group_n[0] == 9 and group_n[1] == 5 and group_n[255] == 1 and sum(group_n) == 15
    assert not hm.overflow_expected(ent({7: 84}), s)                                              # six pieces of 14 from the start of the group: they fit
    assert hm.overflow_expected(ent({7: 85}), s) and hm.overflow_expected(ent({6: 1, 7: 84}), s)  # a seventh piece: one entry more, or the same 84 starting one entry late
    assert not hm.overflow_expected(ent({6: 1, 7: 84}), s, run=40)                                # longer runs, fewer pieces
    assert not hm.overflow_expected(ent({b: 84 for b in range(32, 48)}), s)                       # 1,344 entries in one group of 1,536 slots ...
    assert hm.overflow_expected(ent({b: 84 for b in range(32, 48)} | {b: 60 for b in range(32, 36)}), s)   # ... and 1,584

def test_tail_walk_finds_operands_that_are_the_same_point():
    """NB = 4096: weights w = hi * 64 + lo, 16 quads a workgroup of the marginal kernel, so quad 0 of column 4 adds the buckets of weight 4 and 16 * 64 + 4 first"""
    NB = 4096; a, b = 123456789, 987654321
    assert hm.tail_degenerate({3: a, 16 * 64 + 3: a}, NB) == [("column", 4)] and hm.tail_degenerate({3: a, 16 * 64 + 3: R - a}, NB) == [("column", 4)]
    assert hm.tail_degenerate({3: a, 16 * 64 + 3: b}, NB) == [] and hm.tail_degenerate({3: a, 7: R - a}, NB) == []     # weights 4 and 8: no common column, row or weight bit
    assert hm.tail_degenerate({5 * 64 + 1 - 1: a, 5 * 64 + 17 - 1: a}, NB)[0] == ("row", 5, 0)                          # a row's quad 1 takes lo = 1 and 17
    assert hm.tail_degenerate({0: a, 2: a}, NB) == [("bit", 0)]                                                         # columns 1 and 3 meet in the sum of weight bit 0
    assert hm.tail_degenerate({0: a, 2: b, 64: (a + b) % R}, NB) == []                                                  # (bucket 64: weight 65, column 1, row 1)
    assert ("bucket", 9) in hm.tail_degenerate({9: 0}, NB)

def test_scalars_are_spread_over_multiples_of_r_where_the_top_window_is_narrow():
    """k + m_i r: the same multiple of a point of the prime-order group, W digits with none carried out, the top digit below a quarter of the window — and the
    rule is the kernel's"""
    assert [hm.spread(c) for c in WINDOWS] == [16, 1024, 1, 1, 1, 16384, 1024]
    rnd = random.Random(5)
    for c in WINDOWS:
        W = hm.num_windows(c); s = hm.spread(c); ms = {hm.multiple(i, c) for i in range(70000)}; assert max(ms) < s and (s == 1 or len(ms) > min(s, 70000) * 0.6) and hm.multiple(0, c) == 0
        for k, i in [(R - 1, j) for j in range(3000)] + [(rnd.randrange(R), rnd.randrange(1 << 22)) for _ in range(500)]:
            t = hm.sorted_scalar(k, i, c); d = hm.signed_digits(t, c); assert t % R == k and sum(x << (c * w) for w, x in enumerate(d)) == t
            if s > 1: assert t < 1 << (c * W - 2) and 0 <= d[-1] <= 1 << (c - 2)
    src = open(os.path.join(fm.CSRC, "msm.cuh")).read()
    assert "return tb < c - 2 && c * W > 256 ? 1u << (c * W - 256) : 1u;" in src and "return spread > 1 ? ((i * 2654435761u) >> 16) % spread : 0u;" in src
