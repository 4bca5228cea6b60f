"""The witness MSMs' three-launch path on its own — k_wsort / k_wsort_tagged, k_wacc_lanes29 / k_wacc_lanes_g2_29 (msm.cuh), k_wfold29 / k_wtail29 (htail29.cuh),
k_wfold_g2_29 / k_wtail_g2_29 (oct29.cuh) and the flag-and-repeat logic of MsmImpl::finish_sync — against the plain-integer model of tests/msm_w_model.py and the CPU
oracle, for both groups and every window the path accepts (5 to 8).

Every object is ResidentMsm(group, P, c, filter_ones=True).  wpath() says whether it is on the path and what its last fused run reported; general_path_repeats() whether
a run was repeated on the general path.  The points are (B0 + i) G, so an expected sum is one scalar multiplication, (sum k_i (B0 + i) mod r) G; up to 3,000 points (G1)
and 600 (G2) the oracle's MSM is compared as well.  Integer work: every comparison is exact.

EVERY run asserts three things (run_check): the sum, by how much the repeat counter moved, and the flag word — the last two against a prediction:
  G1  the lanes double or cancel an operand equal to +-the accumulator, the fold and the tail add an equal operand by way of the generator and notice an opposite one
      (htail29.cuh: quad29_add<OPP>): nothing but a bucket with more entries than slots sends a G1 run to the general path.  One repeat and flag 1 iff the model's sort
      overflows, else none and flag 0.
  G2  lanes, fold and tail are incomplete: an operand equal to +-its partner leaves ZZ = 0, the tail raises bit 1 and the run is repeated.  The test points are in
      arithmetic progression, so two partial sums are now and then the same point by accident (P_a + P_b = P_c + P_d whenever a + b = c + d): whether that happens
      depends on the order the sort's atomics left the entries in.  The test reads that order back (w_state) and walks the very additions of the three kernels over it
      (msm_w_model.g2_degenerate): one repeat and flag 2 iff the walk meets such an addition, else none and flag 0 — a needless fallback fails, and so does a missing
      one.  (With an overflow: one repeat and bit 0.)"""
import functools
import numpy as np
import pytest
from oracle import pyoracle as o
from blockmaze_amd import engine as e
import msm_h_model as hm
import msm_w_model as wm

pytestmark = pytest.mark.gpu
R = o.R_MOD
B0 = (1 << 45) + 0x5eed                                                                           # far above n^2
WINDOWS = [5, 6, 7, 8]

@functools.lru_cache(maxsize=None)
def consecutive(group, n):
    P = (o.g1_consecutive if group == 1 else o.g2_consecutive)(B0, n); P.setflags(write=False); return P
@functools.lru_cache(maxsize=None)
def gen(group): return o.g1_gen() if group == 1 else o.g2_gen()
def mul_g(group, s): s %= R; return None if s == 0 else (o.g1_op if group == 1 else o.g2_op)("mul", gen(group), k=s)
def dec(group, a): return (o.g1_from if group == 1 else o.g2_from)(a)[0]
def oracle_msm(group, P, ks): return (o.msm_g1 if group == 1 else o.msm_g2)(P, o.to_arr(ks), mixed=True)
def neg_row(group, row):
    """(x, -y) on the stored words"""
    r = row.copy(); h = 4 if group == 1 else 8
    for k in range(h, 2 * h, 4):
        y = o.from_arr(row[k:k + 4])[0]; r[k:k + 4] = o.limbs((o.Q_MOD - y) % o.Q_MOD)
    return r
def table(group, pts):
    """pts: for every point the multiple of G it is — B0 + j, R - (B0 + j) for a negative, None for the point at infinity — -> the array of points"""
    jmax = max([0] + [(p if p < R // 2 else R - p) - B0 for p in pts if p is not None]); C = consecutive(group, jmax + 1); P = np.zeros((len(pts), C.shape[1]), dtype=np.uint64)
    for i, p in enumerate(pts):
        if p is not None: P[i] = C[p - B0] if p < R // 2 else neg_row(group, C[R - p - B0])
    return P
def plain(n, inf=()): return [None if i in inf else B0 + i for i in range(n)]
def linear(ks, pts): return sum(k * p for k, p in zip(ks, pts) if p is not None) % R

def device_order(m):
    """what the last fused run left: (fill, bucket -> entries in the region's order, the list of ones in its order)"""
    p = m.wpath(); fill = [int(x) for x in m.w_state("fill")]; flat = m.w_state("entries"); ent = {}; at = 0
    for b in range(p.NB): k = min(fill[b], p.cap); ent[b] = [int(x) for x in flat[at:at + k]]; at += k
    assert at == len(flat); return fill, ent, [int(x) for x in m.w_state("ones")]

def predict(m, pts, over):
    """(repeats, flag) of the object's last run, see the module's docstring; flag None: bit 0 set, the rest open"""
    p = m.wpath()
    if not p.fused: return 0, 0
    if over: return 1, (1 if m.group == 1 else None)
    if m.group == 1: return 0, 0
    _, ent, ones = device_order(m); deg = wm.g2_degenerate(ent, ones, pts, m.n, p.c, p.cap)
    if deg: print("G2: a partial sum met +-its partner (n = %d, c = %d): the run must have been repeated" % (m.n, p.c))
    return int(deg), 2 * int(deg)

def check_flag(m, repeats, flag, moved):
    got = m.wpath().flag; assert moved == repeats, "repeats of the general path: %d, expected %d (flag word 0x%x)" % (moved, repeats, got)
    assert (got & 1 and repeats == 1) if flag is None else got == flag, "flag word 0x%x, expected %s" % (got, "bit 0" if flag is None else hex(flag))

def run_check(m, ks, pts, P=None, expect_repeats=None):
    """one run on the scalars ks over the points pts (multiples of G): sum, repeats and flag; expect_repeats: what the case itself says the prediction must be"""
    p = m.wpath(); before = e.general_path_repeats(); m.set_scalars(o.to_arr(ks)); got = dec(m.group, m.run()); moved = e.general_path_repeats() - before
    assert got == mul_g(m.group, linear(ks, pts))
    if P is not None and len(ks) <= (3000 if m.group == 1 else 600): assert got == oracle_msm(m.group, P, ks)
    over = p.fused and wm.overflow_expected(wm.expected_sort([int(x is None) for x in pts], ks, m.n, p.c, shared=p.shared)[0], p.cap)
    repeats, flag = predict(m, pts, over)
    if expect_repeats is not None: assert repeats == expect_repeats, "the model predicts %d repeats, the case %d" % (repeats, expect_repeats)
    check_flag(m, repeats, flag, moved); return moved

def check_wpath(m, n, c, **kw):
    p = m.wpath(); s = wm.wpath_shape(n, c, **kw); print("wpath c=%d n=%d: %s" % (c, n, vars(p)))
    for k in ("fused", "c", "W", "NB", "cap", "RS", "WB"): assert getattr(p, k) == s[k], (k, vars(p), s)
    assert (p.bucket_lanes, p.ones_lanes, p.min_slice, p.tail_slots) == (wm.WFUSED_BUCKET_LANES, wm.WFUSED_ONES_LANES, wm.WFUSED_MIN_SLICE, wm.WTAIL_SLOTS)
    assert p.top == s["top"] and p.leader and not p.shared and p.flag == 0 and p.stream == 0; return s

# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,c,n", [(1, c, n) for c in WINDOWS for n in (1, 2, 3, 255, 256, 257, 3000)] + [(2, c, n) for c in WINDOWS for n in (1, 3, 257, 600)])
def test_every_window_and_size_takes_the_fused_path_and_sums_right(group, c, n):
    """windows 5..8 (16 to 128 buckets; 51, 43, 37, 32 digits a scalar by the generic digit walk below window 8; tails of 6, 7, 8 and 9 workgroups, with result slots
    above `top` cleared below window 8) x sizes around one sort workgroup: the object reports the model's shape, witness-like and full-width scalars stay on the path
    and sum exactly; three runs on one object, so that both parities of the fills and counters are used and cleared.  One exception, by arithmetic: 3,000 full-width
    scalars at window 5 are 3,000 x 51 x 31 / 32 = 148,000 entries for 16 buckets of 8,192 slots, about 9,260 a bucket — that run must overflow and be repeated"""
    pts = plain(n); P = consecutive(group, n); m = e.ResidentMsm(group, P, c, filter_ones=True); check_wpath(m, n, c)
    for ks in (wm.witness_like(100 * c + n, n, small=group == 1), wm.full_width(100 * c + n + 1, n), wm.witness_like(100 * c + n + 2, n)):
        crowded = (c, n) == (5, 3000) and ks[0] > 1 << 200 and ks[1] > 1 << 200                   # (the full-width run of that shape)
        moved = run_check(m, ks, pts, P, expect_repeats=int(crowded) if group == 1 else None); assert group == 2 or moved == int(crowded)
        p = m.wpath(); fills, _, ones = wm.expected_sort([0] * n, ks, n, c); T, off = wm.lane_offsets(fills, p.NB, p.cap)
        assert (p.n_ones, p.lanes, p.T) == (len(ones), off[p.NB], T), (vars(p), len(ones), off[p.NB], T)
    m.close()

def test_a_large_query_gets_an_eighth_of_its_size_as_slots():
    n = 70000; pts = plain(n); m = e.ResidentMsm(1, consecutive(1, n), 8, filter_ones=True); assert check_wpath(m, n, 8)["cap"] == 8750 == m.wpath().cap
    run_check(m, wm.witness_like(70, n), pts, expect_repeats=0); m.close()

@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("c", [4, 9])
def test_windows_4_and_9_are_not_on_the_path_and_sum_right(group, c):
    """8 and 256 buckets: the general path; the repeat counter and the flag word stay where they are"""
    n = 257; pts = plain(n); P = consecutive(group, n); m = e.ResidentMsm(group, P, c, filter_ones=True); s = check_wpath(m, n, c); assert not s["fused"]
    for ks in (wm.witness_like(40 + c, n), wm.full_width(41 + c, n)): assert run_check(m, ks, pts, P, expect_repeats=0) == 0
    with pytest.raises(e.ZkGpuError): m.w_state("fill")
    m.close()

# ---- what the sort leaves ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n", [(5, 257), (5, 3000), (8, 257), (8, 3000)])
def test_sort_state_is_the_models(c, n):
    """after a clean run: the fills, the list of ones as a set, every bucket's entries as a sorted list, and the lanes dealt to the buckets (the order inside a bucket and
    inside the list of ones is the atomics')"""
    pts = plain(n, {3, n - 1}); m = e.ResidentMsm(1, table(1, pts), c, filter_ones=True); inf = [int(x is None) for x in pts]; assert m.wpath().any_inf == 1
    for ks in (wm.witness_like(7 * c + n, n), wm.full_width(7 * c + n + 1, n)):
        if (c, n) == (5, 3000): ks = [0 if i % 3 == 0 else k for i, k in enumerate(ks)]           # (3,000 full-width scalars overflow 16 buckets of 8,192 slots)
        ks[3] = 1; ks[n - 1] = 77; ks[2] = 1                                                      # (a one and a value on points at infinity: skipped by an own sort)
        assert run_check(m, ks, pts, expect_repeats=0) == 0
        fills, ent, ones = wm.expected_sort(inf, ks, n, c); fill, dent, dones = device_order(m); p = m.wpath()
        assert fill == fills and len(dones) == len(ones) and set(dones) == ones
        for b in range(p.NB): assert sorted(dent[b]) == ent.get(b, []), b
        T, off = wm.lane_offsets(fills, p.NB, p.cap); assert [int(x) for x in m.w_state("lane_off")] == off and (p.T, p.lanes) == (T, off[p.NB])
    m.close()

# ---- the ones ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_ones_groups_at_the_end_of_the_query_and_every_nibble(group):
    """n = 5, 6, 7 (the last group holds one, two, three points: k_ones_groups counts the missing ones as infinity), all ones; then 64 points whose 16 groups carry the
    nibbles 0..15: the list holds the 15 entries 15 g + g - 1"""
    for n in (5, 6, 7):
        pts = plain(n); P = consecutive(group, n); m = e.ResidentMsm(group, P, 6, filter_ones=True); run_check(m, [1] * n, pts, P, expect_repeats=0)
        assert sorted(int(x) for x in m.w_state("ones")) == [14, 15 + (1 << (n - 4)) - 2]; m.close()
    n = 64; pts = plain(n); P = consecutive(group, n); ks = [(i >> 2) >> (i & 3) & 1 for i in range(n)]
    for c in (5, 8):
        m = e.ResidentMsm(group, P, c, filter_ones=True); run_check(m, ks, pts, P)
        assert sorted(int(x) for x in m.w_state("ones")) == [15 * g + g - 1 for g in range(1, 16)] and m.wpath().n_ones == 15; m.close()

@pytest.mark.parametrize("group", [1, 2])
def test_points_at_infinity_inside_a_ones_group(group):
    """own sort: the sort skips the points at infinity, so a group's nibble has no bit for them; (the shared sort, which keeps them and leaves the skipping to the
    groups table, is test_shared_sort's)"""
    n = 128; inf = {3, 4, 5, 6, 7, 100}; pts = plain(n, inf); P = table(group, pts); m = e.ResidentMsm(group, P, 7, filter_ones=True)
    ks = [1] * n; run_check(m, ks, pts, P); ones = sorted(int(x) for x in m.w_state("ones"))
    assert ones == sorted(wm.expected_sort([int(x is None) for x in pts], ks, n, 7)[2]) and 15 * 0 + 7 - 1 in ones and not any(x // 15 == 1 for x in ones) and 15 * 25 + 14 - 1 in ones
    ks = wm.witness_like(5, n, small=group == 1); run_check(m, ks, pts, P); m.close()

@pytest.mark.parametrize("group", [1, 2])
def test_a_list_of_ones_longer_than_the_ones_lanes(group):
    """all ones at n = 4 * 8192 + 16: 8,196 groups, four more than WFUSED_ONES_LANES — the smallest query whose lanes go round their stride loop a second time"""
    n = 4 * wm.WFUSED_ONES_LANES + 16; pts = plain(n); m = e.ResidentMsm(group, consecutive(group, n), 8, filter_ones=True); check_wpath(m, n, 8)
    run_check(m, [1] * n, pts, expect_repeats=0); assert m.wpath().n_ones == wm.WFUSED_ONES_LANES + 4
    ks = [1] * n; ks[5] = 0; ks[n - 1] = 3; run_check(m, ks, pts); m.close()

# ---- the region's edge ------------------------------------------------------------------------------------------------------------------------------------------
def edge_scalars(c):
    """scalars whose digits are all 1, filling bucket 0 to exactly its 8,192 slots: at window 8, 256 scalars of 32 digits; at window 5, 160 of 51 and one of 32"""
    return [wm.repeat_digit(8, 1, 32)] * 256 if c == 8 else [wm.repeat_digit(5, 1, 51)] * 160 + [wm.repeat_digit(5, 1, 32)]

@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("c", [5, 8])
def test_a_bucket_filled_to_cap_stays_and_one_more_entry_falls_back(group, c):
    """the sort's test is b + m > cap: 8,192 entries in a bucket of 8,192 slots raise nothing; one entry more raises bit 0, the sum comes from the general path, and the
    object works afterwards"""
    ks = edge_scalars(c); n = len(ks); pts = plain(n); P = consecutive(group, n); m = e.ResidentMsm(group, P, c, filter_ones=True)
    assert wm.expected_sort([0] * n, ks, n, c)[0][0] == m.wpath().cap == 8192
    assert run_check(m, ks, pts, P) == (0 if group == 1 else m.wpath().flag >> 1); assert int(m.w_state("fill")[0]) == 8192 and not m.wpath().flag & 1
    m.close()
    ks = ks + [1 << c]; n += 1; pts = plain(n); P = consecutive(group, n); m = e.ResidentMsm(group, P, c, filter_ones=True)
    assert run_check(m, ks, pts, P, expect_repeats=1) == 1 and m.wpath().flag & 1
    run_check(m, wm.full_width(9, n), pts, P, expect_repeats=0 if group == 1 else None); assert run_check(m, ks, pts, P, expect_repeats=1) == 1; m.close()

@pytest.mark.parametrize("group", [1, 2])
def test_two_slots_a_bucket_under_the_test_hook(group, monkeypatch):
    monkeypatch.setenv("ZK_MSM_DIRECT_CAP", "1"); n = 40; pts = plain(n); P = consecutive(group, n); m = e.ResidentMsm(group, P, 8, filter_ones=True)
    monkeypatch.delenv("ZK_MSM_DIRECT_CAP"); assert check_wpath(m, n, 8, direct_cap=True)["cap"] == 2
    assert run_check(m, [0] * 38 + [5, 5], pts, P) == (0 if group == 1 else m.wpath().flag >> 1)  # two entries: they fit
    assert run_check(m, [0] * 37 + [5, 5, 5], pts, P, expect_repeats=1) == 1                        # three do not
    assert run_check(m, wm.full_width(3, n), pts, P, expect_repeats=1) == 1; m.close()             # ten entries a bucket

# ---- digits -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("c", [5, 8])
def test_digits_at_their_edges(group, c):
    """scalars made from their digits (msm_w_model.from_digits): only the digit 2^(c-1) — bucket NB - 1, which workgroup `top` of the tail takes alone —; only the
    weight 2^s for each s below top, both signs; r - 1 - i (negative digits and the carry chain up to the top window); one non-zero scalar"""
    n = 40; pts = plain(n); P = consecutive(group, n); m = e.ResidentMsm(group, P, c, filter_ones=True); half = 1 << (c - 1); W = hm.num_windows(c); NB = half
    def only(bucket): fill = [int(x) for x in m.w_state("fill")]; assert fill[bucket] and not any(f for b, f in enumerate(fill) if b != bucket), (bucket, fill)
    run_check(m, [wm.repeat_digit(c, half, 1 + (7 * i) % (W - 2)) for i in range(n)], pts, P); only(NB - 1)
    for s in range(c - 1):
        d = 1 << s; ks = [wm.from_digits([d if (i >> w) & 1 else -d for w in range(1 + i % 5)] + [d], c) for i in range(n)]
        if s == 0: ks[0] = d << c                                                                 # (digits 1, 0 .. would be the scalar ONE)
        run_check(m, ks, pts, P); only(d - 1)
    ks = [(R - 1 - i) % R for i in range(n)]; run_check(m, ks, pts, P)
    ks = [0] * n; ks[n // 2] = wm.full_width(c, 1)[0]; run_check(m, ks, pts, P, expect_repeats=0); ks[n // 2] = R - 1; run_check(m, ks, pts, P, expect_repeats=0); m.close()

# ---- lanes ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [5, 8])
def test_lanes_are_dealt_by_fill(c):
    """(a) one bucket with nearly everything, just below its slots: the slice stays at its floor (a single bucket of at most 8,192 entries cannot lift it: that takes
    more than 8 (8,192 - NB) entries in all) and the bucket gets nearly every lane in use; (b) full-width scalars, 3,000 of them (2,000 at window 5, whose 16 buckets would overflow with more): more than 8 entries a lane, T above
    the floor; (c) a handful of entries: T = 8, a lane a bucket.  T, the lanes in use and lane_off against the model"""
    n = 3000; pts = plain(n); P = consecutive(1, n); m = e.ResidentMsm(1, P, c, filter_ones=True); NB = 1 << (c - 1); W = hm.num_windows(c)
    def lanes(ks):
        assert run_check(m, ks, pts, P, expect_repeats=0) == 0; p = m.wpath(); fills = wm.expected_sort([0] * n, ks, n, c)[0]; T, off = wm.lane_offsets(fills, NB, p.cap)
        assert [int(x) for x in m.w_state("lane_off")] == off and (p.T, p.lanes) == (T, off[NB]) and off[NB] <= wm.WFUSED_BUCKET_LANES; return T, off, fills
    per = 32 if c == 8 else 51; k = 8000 // per; T, off, fills = lanes([wm.repeat_digit(c, 1, per)] * k + [3, 5, 9, 12] + [0] * (n - k - 4))
    assert T == 8 and fills[0] == k * per and off[1] == (k * per + 7) // 8 and off[NB] == off[1] + 4
    T, off, fills = lanes(wm.full_width(11 + c, 2000 if c == 5 else n) + [0] * (1000 if c == 5 else 0)); assert T == (sum(fills) + 8192 - NB - 1) // (8192 - NB) > 8
    T, off, fills = lanes([0] * (n - 3) + [2, 3, 2 + (3 << c)]); assert T == 8 and off[NB] == 2 and sum(fills) == 4
    m.close()

# ---- degenerate sums --------------------------------------------------------------------------------------------------------------------------------------------
def degenerate_cases(c):
    """name -> (points as multiples of G, scalars, the sum as a multiple of G)"""
    P0 = B0
    return {"two copies in one lane": ([P0, P0], [2, 2]), "a point and its negative": ([P0, R - P0], [2, 2]), "two lanes of 8P meet in the fold": ([P0] * 16, [2] * 16),
            "buckets 0 and 2 meet in S_0": ([P0, P0], [1 + (2 << c), 3]), "two ones lanes meet": ([P0, B0 + 1, B0 + 2, B0 + 3, P0], [1, 0, 0, 0, 1])}

@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("c", [5, 8])
@pytest.mark.parametrize("case", sorted(degenerate_cases(8)))
def test_degenerate_sums(group, c, case):
    """Tiny deterministic inputs in which an addition meets an operand equal to +-its partner, in a lane, in the fold, in the tail, and between two ones lanes.
    G1 is complete at every one of these places (k_wacc_lanes29 doubles or cancels; quad29_add<OPP> in k_wfold29 / k_wtail29 adds an equal operand by way of the
    generator and returns the point at infinity for an opposite one): no repeat, flag 0, the exact sum.  G2 is incomplete at every one of them (XYZZ2_29::madd,
    oct29_add): one repeat, flag 2 — oct29_emit names no result slot —, the exact sum from the general path.  Afterwards the object runs ordinary scalars cleanly."""
    pts, ks = degenerate_cases(c)[case]; P = table(group, pts); m = e.ResidentMsm(group, P, c, filter_ones=True); assert m.wpath().fused
    moved = run_check(m, ks, pts, P, expect_repeats=0 if group == 1 else 1); assert moved == (0 if group == 1 else 1) and m.wpath().flag == (0 if group == 1 else 2)
    if case == "a point and its negative": assert linear(ks, pts) == 0
    n = len(pts); ks = [wm.full_width(31 + c, 1)[0] if i == 0 else 0 for i in range(n)]; run_check(m, ks, pts, P, expect_repeats=0); m.close()

# ---- shared sorts -----------------------------------------------------------------------------------------------------------------------------------------------
def pair_check(lead, fol, ks, lpts, fpts, expect=None):
    """run_pair: both sums, both flags, and the repeats of the two together.  expect: (leader's repeats, follower's) the case insists on; a leader's None: 0 or 1 — the
    flag word is shared, and the leader's copy of it races the follower's tail"""
    n = lead.n; c = lead.wpath().c; before = e.general_path_repeats(); lead.set_scalars(o.to_arr(ks)); a, b = e.run_pair(lead, fol); moved = e.general_path_repeats() - before
    assert dec(lead.group, a) == mul_g(lead.group, linear(ks, lpts)) and dec(fol.group, b) == mul_g(fol.group, linear(ks, fpts))
    pl, pf = lead.wpath(), fol.wpath(); assert pl.shared and pf.shared and pl.leader and not pf.leader
    over = wm.overflow_expected(wm.expected_sort([0] * n, ks, n, c, shared=True)[0], pl.cap)
    rf, ff = predict(fol, fpts, over); rl, fl = predict(lead, lpts, over)
    if expect is not None: assert rf == expect[1] and (expect[0] is None or rl == expect[0]), (rl, rf, expect)
    assert (pf.flag & 1 and rf == 1) if ff is None else pf.flag == ff, "follower's flag word 0x%x" % pf.flag
    if rf and not rl and not over:                                                                # only the follower's table is degenerate: the leader may have seen its flag
        assert pl.flag in (0, ff) and moved == 1 + (pl.flag != 0), (hex(pl.flag), moved)
    elif over: assert pl.flag & 1 and pf.flag & 1 and moved == 2, (hex(pl.flag), hex(pf.flag), moved)   # (the word is shared: a G2 follower's bit 1 may sit in either copy)
    else: assert pl.flag == fl and moved == rl + rf, (hex(pl.flag), moved, rl, rf)

@pytest.mark.parametrize("streams", [(0, 0), (0, 1)], ids=["one stream", "two streams"])
@pytest.mark.parametrize("c", [5, 8])
@pytest.mark.parametrize("fgroup", [1, 2])
def test_shared_sort(fgroup, c, streams):
    """A G1 leader with a G1 follower (A and L) and with a G2 follower (B1 and the G2 half of B), the follower queued behind the leader on its stream or waiting for its
    event on another: the follower takes the leader's sort, which keeps the points at infinity (the tables differ in them: points 3, 4..7 and 100 in one table only,
    first the follower's, then the leader's), and the two tail launches count their tickets in the two halves of one word.  Then an overflow — both objects repeat —
    and, for the incomplete G2 follower, an input only its table makes degenerate"""
    n = 600; inf = {3, 4, 5, 6, 7, 100}
    for linf, finf in (((), inf), (inf, ())):
        lpts, fpts = plain(n, linf), plain(n, finf); lead = e.ResidentMsm(1, table(1, lpts), c, filter_ones=True); fol = e.ResidentMsm(fgroup, table(fgroup, fpts), c, filter_ones=True)
        other = e.ResidentMsm(1, consecutive(1, 64), c, filter_ones=True); assert not fol.share_sort(other) and not fol.wpath().shared; other.close()   # another size
        assert fol.share_sort(lead); lead.set_stream(streams[0]); fol.set_stream(streams[1]); assert (lead.wpath().stream, fol.wpath().stream) == (streams[0] + 1, streams[1] + 1)
        for seed in (1, 2, 3):                                                                    # (three runs: both parities of the shared fills and counters)
            ks = wm.witness_like(50 * c + seed, n, small=fgroup == 1); ks[3] = 1; ks[5] = 1; ks[100] = 9
            pair_check(lead, fol, ks, lpts, fpts, expect=(0, 0) if fgroup == 1 else None)
            assert set(int(x) for x in fol.w_state("ones")) == wm.expected_sort([0] * n, ks, n, c, shared=True)[2]
        per = 32 if c == 8 else 51; ks = [wm.repeat_digit(c, 1, per)] * (8192 // per + 1) + [0] * (n - 8192 // per - 1)
        pair_check(lead, fol, ks, lpts, fpts, expect=(1, 1)); pair_check(lead, fol, wm.full_width(c, n), lpts, fpts, expect=(0, 0) if fgroup == 1 else None)
        lead.close(); fol.close()
    if fgroup == 2:
        lpts = plain(n); fpts = plain(n); fpts[1] = fpts[0]; lead = e.ResidentMsm(1, table(1, lpts), c, filter_ones=True); fol = e.ResidentMsm(2, table(2, fpts), c, filter_ones=True)
        assert fol.share_sort(lead); lead.set_stream(streams[0]); fol.set_stream(streams[1])
        pair_check(lead, fol, [2, 2] + [0] * (n - 2), lpts, fpts, expect=(0, 1)); pair_check(lead, fol, wm.full_width(c + 1, n), lpts, fpts); lead.close(); fol.close()

# ---- indexed and tagged runs ------------------------------------------------------------------------------------------------------------------------------------
def injective(seed, count, below):
    g = wm.Draw(seed); seen = set(); out = []
    while len(out) < count:
        v = g.below(below)
        if v not in seen: seen.add(v); out.append(v)
    return out

def finish(m, got, ks, pts, before):
    """sum, repeats and flag of an indexed or tagged run whose points took the scalars ks"""
    moved = e.general_path_repeats() - before; assert dec(m.group, got) == mul_g(m.group, linear(ks, pts)); repeats, flag = predict(m, pts, False); check_flag(m, repeats, flag, moved)

@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("c", [5, 8])
def test_indexed_scalars(group, c):
    """the B query's gather map: point i takes z[index[i]], a random injective map into a longer assignment"""
    n, nv = 300, 1000; pts = plain(n); P = consecutive(group, n); m = e.ResidentMsm(group, P, c, filter_ones=True)
    for seed in (1, 2):
        z = wm.witness_like(60 * c + seed, nv, small=group == 1); idx = injective(seed, n, nv); ks = [z[v] for v in idx]; before = e.general_path_repeats()
        finish(m, m.run_indexed(o.to_arr(z), idx), ks, pts, before); assert dec(group, m.run_indexed(o.to_arr(z), idx)) == oracle_msm(group, P, ks)
        fills, _, ones = wm.expected_sort([0] * n, z, n, c, index=idx); assert [int(x) for x in m.w_state("fill")] == fills and set(int(x) for x in m.w_state("ones")) == ones
    with pytest.raises(e.ZkGpuError): m.run_indexed(o.to_arr(z), [nv] * n)
    m.close()

def tags_of(z, conservative=()):
    """(tags, the list of the variables tagged 2): 0 / 1 for those values, 2 for anything else — and for the variables of `conservative`, whatever their value"""
    tags = np.array([2 if (v in conservative or k > 1) else k for v, k in enumerate(z)], dtype=np.uint8); return tags, [v for v in range(len(z)) if tags[v] == 2]

@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("c", [5, 8])
def test_tagged_sort_equals_the_plain_one(group, c):
    """k_wsort_tagged — the sort from a byte a variable and the list of the variables that are neither 0 nor 1 — gives what the plain run gives on the same assignment:
    a plain query at base 0 and as a slice from variable 37 on (listed variables outside the slice are ignored), an indexed query as a slice of its index list with
    var_pos (0xffffffff for the variables the list does not name), a launch sized by a bound 1,000 above the list's length (the length read from device memory),
    conservative tags (values 0 and 1 tagged 2: digits of 1 go to bucket 0, zeros nowhere), and an empty list"""
    n, nv = 300, 1000; pts = plain(n); P = consecutive(group, n); m = e.ResidentMsm(group, P, c, filter_ones=True)
    z = [1] + wm.witness_like(70 * c + group, nv - 1, small=group == 1); Z = o.to_arr(z); tags, other = tags_of(z)
    def plain_run(ks):
        before = e.general_path_repeats(); m.set_scalars(o.to_arr(ks)); got = m.run(); finish(m, got, ks, pts, before); return got
    def tagged(ks, **kw):
        ref = plain_run(ks); before = e.general_path_repeats(); got = m.run_tagged(Z, kw.pop("tags", tags), kw.pop("other", other), **kw); finish(m, got, ks, pts, before)
        assert np.array_equal(got, ref); return m.wpath()
    for base in (0, 37):
        ks = z[base:base + n]; p = tagged(ks, base=base); fills, _, ones = wm.expected_sort([0] * n, ks, n, c)
        assert [int(x) for x in m.w_state("fill")] == fills and set(int(x) for x in m.w_state("ones")) == ones and p.n_ones == len(ones)
        tagged(ks, base=base, n_other_bound=len(other) + 1000)
    L = injective(c, 500, nv); var_pos = np.full(nv, 0xffffffff, dtype=np.uint32)
    for pos, v in enumerate(L): var_pos[v] = pos
    base = 137; idx = L[base:base + n]; ks = [z[v] for v in idx]
    tagged(ks, var_pos=var_pos, index=idx, base=base); tagged(ks, var_pos=var_pos, index=idx, base=base, n_other_bound=len(other) + 1000)
    fills, _, ones = wm.expected_sort([0] * n, ks, n, c); assert [int(x) for x in m.w_state("fill")] == fills and set(int(x) for x in m.w_state("ones")) == ones
    cons = [v for v in range(40, 90) if z[v] <= 1]; assert any(z[v] == 0 for v in cons) and any(z[v] == 1 for v in cons)
    ctags, cother = tags_of(z, set(cons)); ks = z[37:37 + n]; tagged(ks, tags=ctags, other=cother, base=37)
    fill = [int(x) for x in m.w_state("fill")]; fills = wm.expected_sort([0] * n, ks, n, c)[0]
    assert fill[0] == fills[0] + sum(1 for v in cons if z[v] == 1) and fill[1:] == fills[1:]   # (variable v is point v - 37: all of 40..89 lie in the slice)
    z01 = [1] + [k if k <= 1 else 0 for k in z[1:]]; Z = o.to_arr(z01); t01, o01 = tags_of(z01); assert o01 == []
    tagged(z01[:n], tags=t01, other=o01); tagged(z01[37:37 + n], tags=t01, other=o01, base=37, n_other_bound=1000); assert m.wpath().lanes == 0
    with pytest.raises(e.ZkGpuError): m.run_tagged(Z, t01, [nv])                                   # a listed variable beyond the assignment: refused before any launch
    with pytest.raises(e.ZkGpuError): m.run_tagged(Z, t01, [], base=nv - n + 1)
    m.close()
