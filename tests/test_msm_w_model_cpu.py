"""The integer model of the witness MSMs' three-launch path (tests/msm_w_model.py) checked on its own, without a GPU: the constants and rules it restates are the
sources', and on points standing for the integers B0 + i what it says the sort leaves adds up to the plain sum sum k_i (B0 + i) (mod r) — bucket by bucket with the
weights b + 1, the ones by their subset sums — at every window the path accepts, and to the oracle's MSM."""
import functools, os, re
import pytest
import field29_model as fm
import msm_h_model as hm
import msm_w_model as wm
from oracle import pyoracle as o

R = wm.R_MOD
B0 = (1 << 45) + 0x5eed
WINDOWS = [5, 6, 7, 8]
SIZES = [1, 2, 3, 5, 255, 256, 257, 3000]

def pts_of(n, inf=()): return [None if i in inf else B0 + i for i in range(n)]
def plain_sum(ks, pts): return sum(k * p for k, p in zip(ks, pts) if p is not None) % R
def crafted(n, c):
    """digits at their edges: 2^(c-1) (stays positive, bucket NB - 1), one more (turns negative and carries), r - 1 - i (every digit negative, a carry into the top
    window), one value a few times over, and 0 / 1 between them"""
    half = 1 << (c - 1); W = hm.num_windows(c)
    base = [wm.repeat_digit(c, half, W - 2), half + 1, (1 << c) - 1, R - 1, 1, 0, wm.repeat_digit(c, 1, W - 1), 7, 7, 1, 1, 1, R - 2, 2, wm.from_digits([-(half - 1), half, -1, 1], c)]
    return [(base[i % len(base)] if i % 3 else (R - 1 - i) % R) for i in range(n)]
SCALARS = {"witness": lambda n, c: wm.witness_like(17 * n + c, n), "full": lambda n, c: wm.full_width(19 * n + c, n), "crafted": crafted}

@functools.lru_cache(maxsize=None)
def consecutive(n): return o.g1_consecutive(B0, n)
def mul_g(s): s %= R; return None if s == 0 else o.g1_op("mul", o.g1_gen(), k=s)

def test_model_constants_and_rules_are_the_sources():
    msm = open(os.path.join(fm.CSRC, "msm.cuh")).read(); impl = open(os.path.join(fm.CSRC, "msm_impl.hpp")).read()
    def const(name): return int(re.search(r"\b%s = (\d+)" % name, msm).group(1))
    assert const("WFUSED_MAX_BUCKETS") == wm.WFUSED_MAX_BUCKETS and const("WFUSED_BUCKET_LANES") == wm.WFUSED_BUCKET_LANES and const("WFUSED_ONES_LANES") == wm.WFUSED_ONES_LANES
    assert const("WFUSED_MIN_SLICE") == wm.WFUSED_MIN_SLICE and const("WTAIL_SLOTS") == wm.WTAIL_SLOTS and "MSM_ENTRY_SIGN = 0x80000000u" in msm
    assert msm.count("> cap) atomicOr(&cnt->pad[0], 1u);") == 2 and ">= cap) atomicOr" not in msm                            # a bucket filled to exactly cap fits
    assert msm.count("(i >> 2) * 15u + v - 1u") == 2                                                                          # the ones entry, both sorts
    assert msm.count("max(WFUSED_MIN_SLICE, (tot + (WFUSED_BUCKET_LANES - NB) - 1) / (WFUSED_BUCKET_LANES - NB))") == 2      # the slice length, both groups
    assert "NB >= 16 && NB <= WFUSED_MAX_BUCKETS && n * (size_t)W < (1ull << 31)" in impl
    assert "(uint32_t)std::min<size_t>(std::max<size_t>(8192, n / 8), 1u << 17)" in impl
    assert open(os.path.join(fm.CSRC, "oct29.cuh")).read().count("OCT_BLOCK = 512") == 1 and wm.OCT_GROUPS == 512 // 8

def test_wpath_shape_table():
    for c, W, NB, top in ((5, 51, 16, 4), (6, 43, 32, 5), (7, 37, 64, 6), (8, 32, 128, 7)):
        for n in SIZES + [32784, 70000]:
            s = wm.wpath_shape(n, c); assert s["fused"] and (s["W"], s["NB"], s["top"], s["RS"], s["WB"]) == (W, NB, top, 8, 1)
            assert s["cap"] == (8750 if n == 70000 else 8192)
    assert wm.wpath_shape(1 << 21, 8)["cap"] == 1 << 17 and wm.wpath_shape(1 << 20, 8)["cap"] == 1 << 17 and wm.wpath_shape((1 << 20) - 8, 8)["cap"] == (1 << 17) - 1
    for c in (4, 9, 13): s = wm.wpath_shape(3000, c); assert not s["fused"] and s["cap"] == 0 and s["RS"] == 1
    assert not wm.wpath_shape(0, 8)["fused"] and not wm.wpath_shape(3000, 8, filter_ones=False)["fused"] and not wm.wpath_shape(3000, 8, tables=False)["fused"]
    assert wm.wpath_shape(3000, 8, direct_cap=True)["cap"] == 2

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", sorted(SCALARS))
def test_the_sort_reassembles_to_the_plain_sum(kind, n):
    """sum_b (b + 1) sum_entries +-2^(c w) (B0 + i) + the ones' subset sums = sum k_i (B0 + i) (mod r), windows 5..8, with and without points at infinity, own and
    shared sort; and that scalar times G is the oracle's MSM of the points"""
    for c in WINDOWS:
        ks = SCALARS[kind](n, c); half = 1 << (c - 1); NB = half
        for inf_set, shared in (((), False), ({0, 3, n // 2, n - 1}, False), ({0, 3, n // 2, n - 1}, True)):
            pts = pts_of(n, inf_set); inf = [int(p is None) for p in pts]
            fills, ent, ones = wm.expected_sort(inf, ks, n, c, shared=shared)
            assert len(fills) == NB and all(0 <= b < NB for b in ent) and all(fills[b] == len(ent.get(b, ())) for b in range(NB))
            assert wm.reassemble(ent, ones, pts, n, c) == plain_sum(ks, pts), (kind, n, c, shared)
            # every entry names a table row below n W, once; a ones entry a group below ceil(n / 4) with a non-empty subset
            flat = [e & (wm.ENTRY_SIGN - 1) for es in ent.values() for e in es]; assert len(set(flat)) == len(flat) and all(x < n * hm.num_windows(c) for x in flat)
            assert all(e // 15 < (n + 3) // 4 for e in ones) and len({e // 15 for e in ones}) == len(ones)
            # the ones list names exactly the points with scalar one (those at infinity too, when the sort is shared)
            named = {4 * (e // 15) + j for e in ones for j in range(4) if (e % 15 + 1) >> j & 1}
            assert named == {i for i in range(n) if ks[i] == 1 and (shared or not inf[i])}
        if c == 8 or kind == "crafted":
            pts = pts_of(n); exp = mul_g(plain_sum(ks, pts)); assert exp == o.msm_g1(consecutive(n), o.to_arr(ks)), (kind, n, c)

def test_indexed_sort_takes_the_scalar_the_index_names():
    n, nv, c = 257, 700, 6; z = wm.witness_like(5, nv); g = wm.Draw(6); idx = []
    while len(idx) < n:
        v = g.below(nv)
        if v not in idx: idx.append(v)
    fills, ent, ones = wm.expected_sort(None, z, n, c, index=idx); pts = pts_of(n)
    assert wm.reassemble(ent, ones, pts, n, c) == plain_sum([z[v] for v in idx], pts)
    assert (fills, ent, ones) == wm.expected_sort(None, [z[v] for v in idx], n, c)

def test_a_bucket_filled_to_cap_fits_and_one_more_entry_overflows():
    cap = wm.wpath_shape(256, 8)["cap"]; k = wm.repeat_digit(8, 1, 32); assert k == int.from_bytes(b"\x01" * 32, "little")
    fills, _, _ = wm.expected_sort(None, [k] * 256, 256, 8); assert fills[0] == cap == 8192 and not any(fills[1:]) and not wm.overflow_expected(fills, cap)
    fills, _, _ = wm.expected_sort(None, [k] * 256 + [2 << 8], 257, 8); assert fills[0] == cap and fills[1] == 1 and not wm.overflow_expected(fills, cap)
    fills, _, _ = wm.expected_sort(None, [k] * 256 + [1 << 8], 257, 8); assert fills[0] == cap + 1 and wm.overflow_expected(fills, cap)
    k5 = wm.repeat_digit(5, 1, 51); ks = [k5] * 160 + [wm.repeat_digit(5, 1, 32)]; fills, _, _ = wm.expected_sort(None, ks, 161, 5)
    assert fills[0] == 8192 and not wm.overflow_expected(fills, 8192)
    fills, _, _ = wm.expected_sort(None, ks + [1 << 5], 162, 5); assert fills[0] == 8193 and wm.overflow_expected(fills, 8192)
    assert wm.overflow_expected([3, 0], 2) and not wm.overflow_expected([2, 2], 2)

def test_lane_offsets():
    for NB in (16, 32, 64, 128):
        lanes = wm.WFUSED_BUCKET_LANES - NB
        T, off = wm.lane_offsets([0] * NB, NB, 8192); assert T == 8 and off == [0] * (NB + 1)
        T, off = wm.lane_offsets([8 * lanes] + [0] * (NB - 1), NB, 1 << 17); assert T == 8 and off[1:] == [lanes] * NB
        T, off = wm.lane_offsets([8 * lanes + 1] + [0] * (NB - 1), NB, 1 << 17); assert T == 9 and off[NB] == (8 * lanes + 1 + 8) // 9
        T, off = wm.lane_offsets([1] * NB, NB, 8192); assert T == 8 and off == list(range(NB + 1))
        T, off = wm.lane_offsets([9000] * NB, NB, 8192); assert T == (8192 * NB + lanes - 1) // lanes and off[1] == (8192 + T - 1) // T     # fills are clipped to cap
        for seed in range(20):
            g = wm.Draw(seed); fills = [g.below(1 + g.below(9000)) for _ in range(NB)]; T, off = wm.lane_offsets(fills, NB, 8192)
            assert off[NB] <= wm.WFUSED_BUCKET_LANES and all(off[b + 1] - off[b] == -(-min(fills[b], 8192) // T) for b in range(NB))             # every bucket gets its lanes: none beyond the array

def test_g2_walk_adds_every_item_once_and_finds_the_degenerate_additions():
    """g2_results on a clean input stands for the plain sum (every lane, fold and tail item is counted once, at every window); on the degenerate inputs of
    tests/test_gpu_msm_w_path.py it finds the addition that meets +-its partner"""
    for c in WINDOWS:
        for n in (1, 3, 257, 600):
            ks = wm.witness_like(23 * n + c, n, small=False); pts = pts_of(n, {3} if n > 3 else ()); inf = [int(p is None) for p in pts]
            _, ent, ones = wm.expected_sort(inf, ks, n, c); res = wm.g2_results(ent, sorted(ones), pts, n, c, 8192)
            assert len(res) == c + 1 and wm.g2_sum(res, c) == plain_sum(ks, pts), (c, n)
        P = B0
        def walk(pts, ks):
            n = len(pts); _, ent, ones = wm.expected_sort([0] * n, ks, n, c); res = wm.g2_results(ent, sorted(ones), pts, n, c, 8192)
            return wm.g2_degenerate(ent, sorted(ones), pts, n, c, 8192), wm.g2_sum(res, c)
        assert walk([P, P], [2, 2]) == (True, 4 * P % R)                                          # one lane adds P to P
        assert walk([P, R - P], [2, 2])[0]                                                        # P and -P
        assert walk([P] * 16, [2] * 16)[0] and walk([P] * 5, [1, 0, 0, 0, 1])[0] and walk([P, P], [1 + (2 << c), 3])[0]           # lanes; two ones lanes; buckets 0 and 2 in S_0
        assert not walk([P, P], [1, 3])[0]                                                        # (a scalar ONE goes to the list of ones, not to bucket 0)
        assert walk([P, P + 1], [2, 2]) == (False, (4 * P + 2) % R) and walk([P, P + 1, P + 2, P + 3, P + 4], [1, 0, 0, 0, 1])[0] is False
        # two lanes of eight entries each whose sums coincide: found in the fold, not in a lane
        pts = [P + i for i in range(16)]; ent = {1: [0, 1, 2, 3, 12, 13, 14, 15, 4, 5, 6, 7, 8, 9, 10, 11]}
        assert wm.g2_degenerate(ent, [], pts, 16, c, 8192) and not wm.g2_degenerate({1: list(range(16))}, [], pts, 16, c, 8192)
