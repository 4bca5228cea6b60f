"""Plain-integer model of the H query's one-pass MSM path (blockmaze_amd/csrc: k_hsort_bin / k_hsort_group / k_hacc_runs29 / k_hacc_combine29 in msm.cuh, k_hmarg29 /
k_hbits29 in htail29.cuh, the shape rules of MsmImpl's constructor in msm_impl.hpp).  No GPU, no library: tests/test_msm_h_model_cpu.py checks it here,
tests/test_gpu_msm_h_path.py compares the device with it.

  signed_digits      the signed window digits of a scalar (msm.cuh: signed_digits / for_each_digit)
  hsort_shape        whether the constructor enables the one-pass sort for n points at window c, and with which HsortShape, run length and pieces per bucket
  htail_shape        how the weighted bucket sum cuts the weights, and the launch of its marginal kernel
  expected_entries   bucket -> the set of (sign, table index) the sort must leave there
  layout             the counts, offsets and group totals k_hsort_group must leave for them
  overflow_expected  whether those entries overflow a group's region or a bucket's pieces, i.e. whether the run must be repeated on the general path
  tail_degenerate    where the weighted bucket sum adds a point to itself or its negative, for points that are multiples of one generator
  decode_entry       a sorted entry's (low bucket bits, sign, table index)
  point29_affine     a Point29Rec (48 words) -> the affine point, None for the point at infinity"""
import field29_model as fm

R_MOD = fm.R_MOD
SCALAR_BITS = 254
# msm.cuh
HSORT_GROUPS = 1024; HSORT_TILE = 512; HSORT_GROUP_THREADS = 1024; HSORT_MAX_PER_THREAD = 24; HSORT_STAGE_W = 20
HTAIL_CHUNK = 128                                                                                 # htail29.cuh

def num_windows(c): return SCALAR_BITS // c + 1

def signed_digits(k, c):
    """the W = 254 // c + 1 digits d_w of a canonical scalar, sum d_w 2^(c w) = k: a window value (with the carry from below) above 2^(c-1) becomes itself - 2^c and
    carries one into the next window; 2^(c-1) itself stays positive"""
    half = 1 << (c - 1); full = 1 << c; carry = 0; out = []
    for w in range(num_windows(c)):
        d = ((k >> (c * w)) & (full - 1)) + carry
        if d > half: out.append(d - full); carry = 1
        else: out.append(d); carry = 0
    return out

def top_window_bits(c):
    """how many of the scalar's 254 bits the last window holds: 7, 2, 14, 14, 16, 2, 7 for c = 13..19.  Every scalar's top digit lies in 0 .. r >> c (W - 1), so a
    narrow top window would pile the n entries of that window into a handful of the lowest buckets — 97 of them at c = 13 and 19, three at c = 14 and 18 — on
    top of the n W / NB entries a bucket expects; the sort therefore spreads such scalars over multiples of r: see spread"""
    return SCALAR_BITS - c * (num_windows(c) - 1)

def spread(c):
    """how many multiples of r the H sort may add to a scalar (msm.cuh: hsort_spread): 2^(c W - 256) where the top window is narrow — 16, 1,024, 16,384, 1,024 for
    c = 13, 14, 18, 19 — and 1 (none) otherwise.  k + m r < 2^(c W - 2) still has W digits with none carried out, stands for the same multiple of a point of the
    prime-order group, and its top digit spreads over about 0.19 NB buckets"""
    W = num_windows(c); return 1 << (c * W - 256) if top_window_bits(c) < c - 2 and c * W > 256 else 1

def multiple(i, c):
    """m_i, picked by a hash of the scalar's index (msm.cuh: hsort_multiple)"""
    s = spread(c); return ((i * 2654435761 & 0xffffffff) >> 16) % s if s > 1 else 0

def sorted_scalar(k, i, c):
    """what the one-pass sort decomposes for scalar i: k + m_i r"""
    return k + multiple(i, c) * R_MOD

def default_run(total): return 15 if total > (12 << 20) else 11 if total > (6 << 20) else 14    # the three regimes of h_run by n W

def hsort_shape(n, c, h_run=None):
    """None if MsmImpl's constructor leaves the one-pass sort off for n points at window c (uniform hint, fixed-base tables, G1); otherwise a dict of what it decides"""
    W = num_windows(c); NB = 1 << (c - 1); total = n * W
    if n == 0 or W <= 1 or total >= 1 << 31 or total * 64 > 8192 << 20: return None             # (no fixed-base table: use_precompute, default cap of 8 GB)
    G = 256
    while G < HSORT_GROUPS and total // G > 16384: G <<= 1
    low = 0
    while (G << low) < NB: low += 1
    ib = 1
    while (1 << ib) < total: ib += 1
    region = ((total // G) * 5 // 4 + 1024 + 255) & ~255
    if not (W <= HSORT_STAGE_W and (G << low) == NB and 1 <= low <= 10 and low + 1 + ib <= 32 and region <= HSORT_GROUP_THREADS * HSORT_MAX_PER_THREAD): return None
    run = default_run(total) if h_run is None else h_run
    lam = total // NB
    return dict(c=c, W=W, NB=NB, groups=G, low_bits=low, idx_bits=ib, region=region, h_run=run, h_maxp=(lam + lam // 2 + 32 + run - 1) // run + 2, htail29=NB >= 512)

def combine_lanes(n, c, run):
    """the lane exponent of k_hacc_combine29 as run_impl chooses it"""
    pieces = n * num_windows(c) // (1 << (c - 1)) // run
    return 3 if pieces > 40 else 2 if pieces > 18 else 1

def htail_shape(NB):
    top = 0
    while (1 << top) < NB: top += 1
    lo = (top + 1) // 2; hi = top - lo; rc = (1 << lo) // HTAIL_CHUNK if (1 << lo) > HTAIL_CHUNK else 1
    return dict(top=top, lo_bits=lo, hi_bits=hi, row_chunks=rc, marg_block=64 if max(1 << hi, (1 << lo) // rc) <= 128 else 256,
                marg_blocks=((1 << lo) - 1) + ((1 << hi) - 1) * rc + 1, marg_count=(1 << lo) + (1 << hi) * rc + 1)

def expected_entries(points_inf, scalars, n, c):
    """bucket -> set of (sign, table index): for every point not at infinity, every non-zero scalar and every non-zero digit d of window w — the digits of
    k_i + m_i r, see spread — bucket |d| - 1 holds (d < 0, i + w n)"""
    out = {}
    for i in range(n):
        if points_inf[i] or scalars[i] == 0: continue
        for w, d in enumerate(signed_digits(sorted_scalar(scalars[i], i, c), c)):
            if d: out.setdefault(abs(d) - 1, set()).add((1 if d < 0 else 0, i + w * n))
    return out

def layout(ent, shape):
    """what k_hsort_group must leave for the model's entries: (counts, offsets, group_n) as lists over buckets / groups; offsets[b] = group x region + the counts of
    the group's buckets before b"""
    NB, G, low, region = shape["NB"], shape["groups"], shape["low_bits"], shape["region"]
    counts = [len(ent.get(b, ())) for b in range(NB)]; offsets = [0] * NB; group_n = [0] * G
    for g in range(G):
        pre = 0
        for b in range(g << low, (g + 1) << low): offsets[b] = g * region + pre; pre += counts[b]
        group_n[g] = pre
    return counts, offsets, group_n

def overflow_expected(ent, shape, run=None):
    """does the one-pass path raise its overflow flag on these entries: a group with more entries than its region (k_hsort_bin), or a bucket whose entries span more
    than h_maxp runs of its group (hacc_flush29: piece = runs since the bucket's first entry)"""
    run = shape["h_run"] if run is None else run; counts, offsets, group_n = layout(ent, shape)
    if any(t > shape["region"] for t in group_n): return True
    for b, cnt in enumerate(counts):
        off = offsets[b] - (b >> shape["low_bits"]) * shape["region"]
        if cnt and (off + cnt - 1) // run - off // run + 1 > shape["h_maxp"]: return True
    return False

def _tree(acc, add):
    """the sum a workgroup's quads leave in quad 0 (block_quad29_tree): the 16 quads of every wave by halving, then the waves the same way; only the additions
    that reach quad 0 count"""
    waves = [acc[i:i + 16] + [None] * (16 - len(acc[i:i + 16])) for i in range(0, len(acc), 16)]
    for w in waves:
        for dq in (8, 4, 2, 1):
            for q in range(dq): w[q] = add(w[q], w[q + dq])
    top = [w[0] for w in waves] + [None] * (4 - len(waves))
    for dq in (2, 1):
        for q in range(dq): top[q] = add(top[q], top[q + dq])
    return top[0]

def tail_degenerate(S, NB):
    """S: bucket -> s with bucket sum = s G (mod r; a missing bucket is the point at infinity) — every point a multiple of ONE generator, as with consecutive test
    points.  Walks the additions of k_hmarg29 and k_hbits29 in their order (quad q takes items q, q + quads, ...; then the tree) and returns the places where an
    operand is +-the other one: there the tail's incomplete addition leaves ZZ = 0, which k_hbits29 must flag.  With points in arithmetic progression that happens
    by accident now and then (P_a + P_b = P_c + P_d whenever a + b = c + d in one window): an ordinary key has no such relations"""
    t = htail_shape(NB); L = 1 << t["lo_bits"]; H = 1 << t["hi_bits"]; RC = t["row_chunks"]; nq = t["marg_block"] // 4; found = []
    def adder(where):
        def add(a, b):
            if a is None: return b
            if b is None: return a
            if (a - b) % R_MOD == 0 or (a + b) % R_MOD == 0: found.append(where)
            return (a + b) % R_MOD
        return add
    def quads(items, n_quads, add):
        acc = [None] * n_quads
        for j, v in enumerate(items):
            if v is not None: acc[j % n_quads] = add(acc[j % n_quads], v)
        return acc
    by_col, by_row = {}, {}
    for b, s in S.items():
        w = b + 1; hi, lo = divmod(w, L)
        if s % R_MOD == 0: found.append(("bucket", b))                                            # (a bucket whose entries cancel: the combine's business)
        if lo: by_col.setdefault(lo, {})[hi] = s
        if 1 <= hi < H: by_row.setdefault((hi, lo // (L // RC)), {})[lo % (L // RC)] = s
    marg = {}
    for lo, d in by_col.items():
        add = adder(("column", lo)); marg[lo] = _tree(quads([d.get(hi) for hi in range(H)], nq, add), add)
    for (hi, piece), d in by_row.items():
        add = adder(("row", hi, piece)); marg[L + hi * RC + piece] = _tree(quads([d.get(j) for j in range(L // RC)], nq, add), add)
    for s_ in range(t["top"]):
        cols = s_ < t["lo_bits"]; bit = s_ if cols else s_ - t["lo_bits"]; rc = 1 if cols else RC; count = ((L if cols else H) >> 1) * rc
        with_bit = lambda i: ((i >> bit) << (bit + 1)) | (1 << bit) | (i & ((1 << bit) - 1))
        items = [marg.get(with_bit(j) if cols else L + with_bit(j // rc) * rc + j % rc) for j in range(count)]
        if sum(v is not None for v in items) > 1: add = adder(("bit", s_)); _tree(quads(items, 64, add), add)
    return found

def decode_entry(e, idx_bits):
    """entry = low bucket bits << (idx_bits + 1) | sign << idx_bits | table index"""
    e = int(e); return e >> (idx_bits + 1), (e >> idx_bits) & 1, e & ((1 << idx_bits) - 1)

def point29_affine(rec):
    """a Point29Rec — four coordinate slots (X, Y, ZZ, ZZZ) of 12 words, the first nine of each 29-bit limbs of (coordinate x 2^261 mod q, any representative) —
    as the affine point (X / ZZ, Y / ZZZ); all-zero ZZ limbs are the point at infinity (None).  ZZ = 0 (mod q) in a record that is not all zero is no point:
    AssertionError"""
    rec = [int(x) for x in rec]; assert len(rec) == 48
    for k in range(4): assert rec[12 * k + 9:12 * k + 12] == [0, 0, 0], ("padding", k)
    if not any(rec[24:33]): return None
    pt = fm.g1_affine(sum((rec[12 * k:12 * k + 9] for k in range(4)), []))
    assert pt is not None, "ZZ = 0 (mod q) in a record that is not the point at infinity"
    return pt

def bucket_scalar(entries_of_bucket, n, c, b0):
    """s_b with bucket sum = s_b G when point i is (b0 + i) G: sum of +-2^(c w) (b0 + i) over the bucket's entries (sign, i + w n)"""
    s = 0
    for sign, idx in entries_of_bucket:
        w, i = divmod(idx, n); t = (b0 + i) << (c * w); s += -t if sign else t
    return s % R_MOD
