"""Plain-integer model of the witness MSMs' three-launch path (blockmaze_amd/csrc: k_wsort / k_wsort_tagged / k_ones_groups / k_wacc_lanes29 / k_wacc_lanes_g2_29 in
msm.cuh, k_wfold29 / k_wtail29 in htail29.cuh, k_wfold_g2_29 / k_wtail_g2_29 in oct29.cuh, the shape rules of MsmImpl's constructor in msm_impl.hpp).  No GPU, no
library: tests/test_msm_w_model_cpu.py checks it here, tests/test_gpu_msm_w_path.py compares the device with it.

  wpath_shape        whether the constructor puts n points at window c on the path, and with how many entry slots a bucket
  expected_sort      what the sort must leave: the fill of every bucket, its entries as a sorted list, the set of ones entries
  lane_offsets       the slice length T and the first lane of every bucket, as the lane kernels deal them
  overflow_expected  whether the sort raises flag bit 0 (a bucket holds more entries than slots)
  reassemble         the scalar the buckets and the ones stand for when point i is pts[i] G: what the fold, the tail and the host's Horner rule add up
  g2_degenerate      walks the additions of the G2 lanes, fold and tail over entries in the order the device left them and says whether one of them meets an operand
                     equal to +-its partner: G2's additions are incomplete, so exactly then the tail must raise flag bit 1.  (G1's lanes double or cancel, and its
                     fold and tail add an equal operand by way of the generator and notice an opposite one: nothing there raises the flag but an overflow.)"""
import msm_h_model as hm
from msm_h_model import signed_digits, num_windows

R_MOD = hm.R_MOD
# msm.cuh
WFUSED_MAX_BUCKETS = 128; WFUSED_BUCKET_LANES = 8192; WFUSED_ONES_LANES = 8192; WFUSED_MIN_SLICE = 8; WTAIL_SLOTS = 8
ENTRY_SIGN = 1 << 31
OCT_GROUPS = 64                                                                                   # oct29.cuh: a workgroup of 512 threads is 64 groups of eight

def wpath_shape(n, c, tables=True, filter_ones=True, direct_cap=False):
    """the constructor's decision for n points at window c: fused iff tables, filter_ones, n > 0, 16 <= NB <= 128 and n W < 2^31 (the table's indices fit an entry);
    then cap slots a bucket (2 under ZK_MSM_DIRECT_CAP), eight result slots and top = log2(NB)"""
    W = num_windows(c); NB = 1 << (c - 1)
    fused = bool(tables and filter_ones and n > 0 and 16 <= NB <= WFUSED_MAX_BUCKETS and n * W < 1 << 31)
    d = dict(fused=fused, c=c, W=W, NB=NB, top=NB.bit_length() - 1, WB=1 if tables and n > 0 else W)
    d["cap"] = (2 if direct_cap else min(max(8192, n // 8), 1 << 17)) if fused else 0
    d["RS"] = WTAIL_SLOTS if fused else d["WB"]
    return d

def expected_sort(inf, scalars, n, c, index=None, shared=False):
    """(fills, entries, ones): point i takes scalars[index[i]] (scalars[i] without an index).  A point at infinity is skipped unless the sort is shared (its followers'
    tables differ in which points are at infinity; the additions skip those).  Scalar 0: nothing.  Scalar 1: bit i & 3 of the nibble v of group i >> 2, and a group
    with v != 0 is ONE entry 15 g + v - 1.  Anything else: every non-zero digit d of window w is the entry (i + w n) | sign in bucket |d| - 1.
    fills: a list over the NB buckets; entries: bucket -> sorted list; ones: a set"""
    NB = 1 << (c - 1); ent = {}; nib = {}
    for i in range(n):
        if inf is not None and inf[i] and not shared: continue
        k = scalars[index[i]] if index is not None else scalars[i]
        if k == 0: continue
        if k == 1: nib[i >> 2] = nib.get(i >> 2, 0) | 1 << (i & 3); continue
        for w, d in enumerate(signed_digits(k, c)):
            if d: ent.setdefault(abs(d) - 1, []).append((i + w * n) | (ENTRY_SIGN if d < 0 else 0))
    entries = {b: sorted(v) for b, v in ent.items()}
    return [len(entries.get(b, ())) for b in range(NB)], entries, {15 * g + v - 1 for g, v in nib.items()}

def lane_offsets(fills, NB, cap):
    """(T, off): m_b = min(fill_b, cap), T = max(WFUSED_MIN_SLICE, ceil(sum m_b / (WFUSED_BUCKET_LANES - NB))), bucket b takes ceil(m_b / T) lanes from off[b] on;
    off has NB + 1 entries"""
    m = [min(f, cap) for f in fills[:NB]]; lanes = WFUSED_BUCKET_LANES - NB
    T = max(WFUSED_MIN_SLICE, (sum(m) + lanes - 1) // lanes); off = [0]
    for v in m: off.append(off[-1] + (v + T - 1) // T)
    return T, off

def overflow_expected(fills, cap):
    """a workgroup of the sort raises bit 0 when its reservation ends beyond cap: the last one of a bucket ends at the bucket's fill, so fill > cap (cap itself fits)"""
    return any(f > cap for f in fills)

def from_digits(ds, c):
    """the scalar with the signed digits ds (window 0 first); the caller keeps every digit in -(2^(c-1) - 1) .. 2^(c-1) and the last non-zero one positive, so that
    signed_digits gives ds back"""
    k = sum(d << (c * w) for w, d in enumerate(ds)); assert 0 <= k < R_MOD and signed_digits(k, c)[:len(ds)] == list(ds), (c, ds); return k

def repeat_digit(c, d, count): return from_digits([d] * count, c)

class Draw:
    """SplitMix64, the tests' generator (oracle/pyoracle.py has the same one; the model stands alone)"""
    M = (1 << 64) - 1
    def __init__(self, seed): self.s = seed & self.M
    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & self.M; z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & self.M; z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & self.M; return z ^ (z >> 31)
    def below(self, m): return self.next() % m
    def field(self): return (self.next() | self.next() << 64 | self.next() << 128 | (self.next() & ((1 << 61) - 1)) << 192)

def witness_like(seed, n, small=True):
    """an assignment as a circuit leaves it: 40 % zeros, 45 % ones, the rest full-width values and (small) values below 2^16, which repeat"""
    g = Draw(seed); out = []
    for _ in range(n):
        t = g.below(100)
        out.append(0 if t < 40 else 1 if t < 85 else g.field() if t < 93 or not small else 2 + g.below(1 << (4 + g.below(13))))
    return out

def full_width(seed, n): g = Draw(seed); return [g.field() for _ in range(n)]

def entry_value(e, pts, n, c):
    """the multiple of G an entry stands for when point i is pts[i] G (None: the point at infinity): +-2^(c w) pts[i]"""
    w, i = divmod(e & (ENTRY_SIGN - 1), n); s = pts[i]
    if s is None: return None
    v = (s << (c * w)) % R_MOD; return (R_MOD - v) % R_MOD if e & ENTRY_SIGN else v

def ones_value(e, pts, n):
    """a ones entry 15 g + v - 1: the sum of the points 4g + j, j in v, that exist and are not at infinity (k_ones_groups); None where that is the point at infinity"""
    g, v = divmod(e, 15); v += 1; live = [pts[4 * g + j] for j in range(4) if v >> j & 1 and 4 * g + j < n and pts[4 * g + j] is not None]
    s = sum(live) % R_MOD; return s if live and s else None

def reassemble(entries, ones, pts, n, c):
    """sum_b (b + 1) (sum of bucket b's entries) + the sum of the ones' subset sums (mod r)"""
    s = 0
    for b, es in entries.items():
        for e in es:
            v = entry_value(e, pts, n, c)
            if v is not None: s += (b + 1) * v
    for e in ones: s += ones_value(e, pts, n) or 0
    return s % R_MOD

# ---- G2: where an incomplete addition meets +-its partner ---------------------------------------------------------------------------------------------------
# a partial sum is None (the point at infinity) or (s, bad): s G, and bad once an addition on the way met an operand equal to +-its partner — ZZ = 0 (mod p) from
# then on, whatever is added (a product with ZZ stays 0)
def _add(a, b):
    if a is None: return b
    if b is None: return a
    return ((a[0] + b[0]) % R_MOD, a[1] or b[1] or (a[0] - b[0]) % R_MOD == 0 or (a[0] + b[0]) % R_MOD == 0)

def _lane(values):
    acc = None
    for v in values:
        if v is not None: acc = _add(acc, (v, False))
    return acc

def _strided(items, groups=OCT_GROUPS):
    """group q of a workgroup takes items q, q + 64, ... one after the other"""
    acc = [None] * groups
    for j, v in enumerate(items): acc[j % groups] = _add(acc[j % groups], v)
    return acc

def _oct_tree(acc, live):
    """block_oct29_tree: the eight groups of every wave by shuffles (each level reads the neighbours' values of before the level), the eight waves through LDS; levels
    whose partners are all empty are skipped.  The sum is group 0's"""
    acc = list(acc) + [None] * (OCT_GROUPS - len(acc))
    for wave in range(8):
        for dq in (4, 2, 1):
            if wave * 8 + dq >= live: continue
            old = acc[wave * 8:wave * 8 + 8]
            for wq in range(8 - dq): acc[wave * 8 + wq] = _add(old[wq], old[wq + dq])
    top = [acc[8 * w] for w in range(8)]
    for dq in (4, 2, 1):
        if dq * 8 >= live: continue
        old = list(top)
        for q in range(8 - dq): top[q] = _add(old[q], old[q + dq])
    return top[0]

def g2_results(entries_in_order, ones_in_order, pts, n, c, cap):
    """the top + 2 results of k_wtail_g2_29 as partial sums: S_0 .. S_(top-1), bucket NB - 1, the sum of the ones.  entries_in_order: bucket -> its entries in the
    order they lie in the region; ones_in_order: the list of ones as it lies on the device"""
    NB = 1 << (c - 1); top = NB.bit_length() - 1
    fills = [len(entries_in_order.get(b, ())) for b in range(NB)]; T, off = lane_offsets(fills, NB, cap)
    buckets = []
    for b in range(NB):
        es = list(entries_in_order.get(b, ()))[:cap]; lanes = [_lane(entry_value(e, pts, n, c) for e in es[k:k + T]) for k in range(0, len(es), T)]
        assert len(lanes) == off[b + 1] - off[b]; buckets.append(_oct_tree(_strided(lanes), min(len(lanes), OCT_GROUPS)))
    ones = list(ones_in_order); ones_lanes = [_lane(ones_value(e, pts, n) for e in ones[u::WFUSED_ONES_LANES]) for u in range(min(len(ones), WFUSED_ONES_LANES))]
    ones_lanes += [None] * (WFUSED_ONES_LANES - len(ones_lanes))
    ones_partial = [_oct_tree(_strided(ones_lanes[256 * g:256 * g + 256]), OCT_GROUPS) for g in range(WFUSED_ONES_LANES // 256)]
    res = []
    for s in range(top):
        items = [buckets[(((i >> s) << (s + 1)) | (1 << s) | (i & ((1 << s) - 1))) - 1] for i in range(NB >> 1)]
        res.append(_oct_tree(_strided(items), min(NB >> 1, OCT_GROUPS)))
    res.append(buckets[NB - 1]); res.append(_oct_tree(_strided(ones_partial), min(len(ones_partial), OCT_GROUPS)))
    return res

def g2_degenerate(entries_in_order, ones_in_order, pts, n, c, cap):
    """True iff one of the results carries ZZ = 0: the G2 tail then raises flag bit 1 (and no slot bits: oct29_emit names none)"""
    return any(r is not None and r[1] for r in g2_results(entries_in_order, ones_in_order, pts, n, c, cap))

def g2_sum(results, c):
    """the scalar the results stand for: sum_s 2^s S_s + the ones (the host's Horner rule with one-bit windows)"""
    top = (1 << (c - 1)).bit_length() - 1
    return (sum((r[0] << s) for s, r in enumerate(results[:top + 1]) if r is not None) + (results[top + 1][0] if results[top + 1] is not None else 0)) % R_MOD
