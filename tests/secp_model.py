"""secp256k1 sender recovery on Python integers: the model of include/zk_senders.h.  recover() decides what the reference's recoverPlain decides
(core/types/transaction_signing.go:246-271): crypto.ValidateSignatureValues (crypto/crypto.go:199-210), then libsecp256k1's secp256k1_ecdsa_recover with recid = V
(src/modules/recovery/main_impl.h:87-121), then Keccak256(pub[1:])[12:].  forge() builds signatures whose recovery computes a chosen u1 G + u2 P."""
P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
G = (GX, GY)

def on_curve(pt): return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - 7) % P == 0
def neg(pt): return None if pt is None else (pt[0], (-pt[1]) % P)
def add(a, b):
    """affine addition; None is the point at infinity"""
    if a is None: return b
    if b is None: return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0: return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else: lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)
def mul(k, pt):
    """k pt for any integer k; a multiple by N - j is formed as -(j pt), so the small families of the tests cost a few additions"""
    k %= N
    if k > N // 2: return neg(mul(N - k, pt))
    r = None
    while k:
        if k & 1: r = add(r, pt)
        pt = add(pt, pt); k >>= 1
    return r
def lincomb(u1, u2, pt): return add(mul(u1, G), mul(u2, pt))

_RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001, 0x8000000080008081, 0x8000000000008009,
       0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A, 0x000000008000808B, 0x800000000000008B, 0x8000000000008089, 0x8000000000008003,
       0x8000000000008002, 0x8000000000000080, 0x000000000000800A, 0x800000008000000A, 0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
_M = 2**64 - 1
def _rot(v, n): return ((v << n) | (v >> (64 - n))) & _M if n else v
def _f1600(s):
    for rc in _RC:
        c = [s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20] for x in range(5)]
        for x in range(5):
            d = c[(x + 4) % 5] ^ _rot(c[(x + 1) % 5], 1)
            for y in range(5): s[x + 5 * y] ^= d
        b = [0] * 25; x, y = 1, 0; b[0] = s[0]
        for t in range(24):                                     # rho and pi along the orbit (x, y) -> (y, 2x + 3y): offsets (t + 1)(t + 2) / 2
            b[y + 5 * ((2 * x + 3 * y) % 5)] = _rot(s[x + 5 * y], (t + 1) * (t + 2) // 2 % 64); x, y = y, (2 * x + 3 * y) % 5
        for y in range(5):
            for x in range(5): s[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & _M & b[(x + 2) % 5 + 5 * y])
        s[0] ^= rc
def keccak256(data):
    """the pre-standard Keccak-256 (padding 0x01 ... 0x80, rate 136) that the reference's sha3.NewKeccak256 is"""
    data = bytearray(data); data.append(0x01)
    while len(data) % 136: data.append(0)
    data[-1] |= 0x80; s = [0] * 25
    for off in range(0, len(data), 136):
        for k in range(17): s[k] ^= int.from_bytes(data[off + 8 * k: off + 8 * k + 8], "little")
        _f1600(s)
    return b"".join(v.to_bytes(8, "little") for v in s[:4])
def address(pt): return keccak256(pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big"))[12:]

def recover(h, sig, homestead):
    """h: 32 bytes; sig: R || S || V, 65 bytes, V as recoverPlain holds it after the subtraction of 27.  -> (ok, X, Y, addr); (False, 0, 0, 20 zero bytes) where
    recoverPlain returns an error"""
    bad = (False, 0, 0, bytes(20)); r = int.from_bytes(sig[:32], "big"); s = int.from_bytes(sig[32:64], "big"); v = sig[64]
    if r < 1 or s < 1: return bad                                # crypto.go:200
    if homestead and s > N // 2: return bad                      # crypto.go:205
    if not (r < N and s < N and v in (0, 1)): return bad         # crypto.go:209
    x = r                                                        # main_impl.h:104-109: recid & 2 is never set
    y2 = (x ** 3 + 7) % P; y = pow(y2, (P + 1) // 4, P)
    if y * y % P != y2: return bad                               # main_impl.h:110: ge_set_xo_var fails
    if (y & 1) != v: y = P - y
    rn = pow(r, -1, N); m = int.from_bytes(h, "big") % N
    q = lincomb(-m * rn % N, s * rn % N, (x, y))                 # main_impl.h:114-118
    if q is None: return bad                                     # main_impl.h:120
    return (True, q[0], q[1], address(q))

def forge(k, u1, u2):
    """the (hash, sig) whose recovery, homestead off, computes u1 G + u2 (k G): R = k G, r = x(R) mod N, V = the parity of y(R), hash = -u1 r, s = u2 r mod N.
    Needs x(R) < N (true for all but 2^-128 of the points) and s != 0."""
    R = mul(k, G); r = R[0]; assert 0 < r < N and u2 % N
    return ((-u1 * r) % N).to_bytes(32, "big"), r.to_bytes(32, "big") + (u2 * r % N).to_bytes(32, "big") + bytes([R[1] & 1])

def sign(h, key, nonce):
    """an ECDSA signature of the 32-byte hash h under the private key `key` with the given nonce, low-S, as the reference's crypto.Sign returns it"""
    R = mul(nonce, G); r = R[0] % N; s = pow(nonce, -1, N) * (int.from_bytes(h, "big") + r * key) % N; v = R[1] & 1; assert r and s and R[0] < N
    if s > N // 2: s = N - s; v ^= 1
    return r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([v])

# ---- the reduction of csrc/secp256k1.cuh on Python integers, and operands that take each of its paths ------------------------------------------------------------------
def fold_trace(a, b, modulus):
    """reduce512 of secp256k1.cuh restated: the 512-bit product of two 256-bit values, three folds lo + hi C (C = 2^256 - modulus) with the widths the header states,
    the masked + C where fold 3 carried, one conditional subtraction.  -> (residue, (fold-2 carry, fold-3 carry, final subtraction taken, high half non-zero))"""
    W = 1 << 256; C = W - modulus; cw = -(-C.bit_length() // 32); assert 0 <= a < W and 0 <= b < W and modulus in (P, N)
    t = a * b; lo, hi = t % W, t // W
    s1 = lo + hi * C; a1, over1 = s1 % W, s1 // W; assert over1.bit_length() <= C.bit_length() + 1 and over1 < 1 << (32 * (cw + 1))       # fold 1: CW + 1 words on
    s2 = a1 + over1 * C; b2, over2 = s2 % W, s2 // W; assert over2.bit_length() <= (1 if modulus == P else 4)                              # fold 2: p 1 bit, N 4 bits
    h3 = over2 % (1 << 64)                                                                                                                 # (two words on: p hands on one and a zero)
    s3 = b2 + h3 * C; c3, over3 = s3 % W, s3 // W; assert over3 in (0, 1)                                                                  # fold 3: a carry of 0 or 1
    r = c3 + (C if over3 else 0); assert r < W                                                                                             # the + C cannot carry
    sub = r >= modulus
    if sub: r -= modulus
    assert r == a * b % modulus, (hex(a), hex(b), hex(modulus))
    return r, (over2, over3, sub, hi != 0)

def _reduce_candidates(recipe, modulus, rng):
    """an endless stream of operand pairs by one recipe of the issue "Reach the reduction carries": a b = 2C - delta (the fold-3 carry), the same with a = 2^256 - 1,
    a b = epsilon < C (the folds end at epsilon + modulus), a b = C + d with d < 2^60 (p: fold 2 carries), and the two squares a^2 = C + d, a^2 = epsilon"""
    W = 1 << 256; C = W - modulus
    while True:
        a = rng.randrange(1, modulus)
        if recipe == "random": yield a, rng.randrange(modulus)
        elif recipe == "fold3": yield a, (2 * C - rng.randrange(1, C + 1)) * pow(a, -1, modulus) % modulus
        elif recipe == "fold3 max": yield W - 1, (W + C - rng.randrange(1, C + 1)) * pow(C - 1, -1, modulus) % modulus
        elif recipe == "epsilon": yield a, rng.randrange(C) * pow(a, -1, modulus) % modulus
        elif recipe == "C + d": yield a, (C + rng.randrange(1 << 60)) * pow(a, -1, modulus) % modulus
        else:
            x = C + rng.randrange(1 << 60) if recipe == "sqr C + d" else rng.randrange(C); assert modulus == P and recipe in ("sqr C + d", "sqr epsilon")
            a = pow(x, (P + 1) // 4, P)
            if a * a % P == x: yield a, a

# class -> (modulus, recipe, the record wanted, as (fold-2 carry or None, fold-3 carry or None, subtraction with a non-zero high half wanted))
REDUCE_CLASSES = {
    "N (0,0)": (N, "random", (0, 0, False)), "N (1,0)": (N, "random", (1, 0, False)), "N (2,0)": (N, "random", (2, 0, False)),
    "N (1,1)": (N, "fold3", (1, 1, False)), "N (1,1) a = 2^256 - 1": (N, "fold3 max", (1, 1, False)),
    "N sub": (N, "epsilon", (None, None, True)), "N sub, fold-2 carry 1": (N, "epsilon", (1, None, True)),
    "p (0,0)": (P, "random", (0, 0, False)), "p (1,0)": (P, "C + d", (1, 0, False)), "p sub": (P, "epsilon", (None, None, True)),
    "p sqr (1,0)": (P, "sqr C + d", (1, 0, False)), "p sqr sub": (P, "sqr epsilon", (None, None, True)),
}
def record_wanted(rec, want): return (want[0] is None or rec[0] == want[0]) and (want[1] is None or rec[1] == want[1]) and (not want[2] or (rec[2] and rec[3]))

_reduce_memo = {}
def reduce_cases(name, count=64, tries=None):
    """-> (the first `count` operand pairs of class `name` whose record, by fold_trace alone, is the wanted one; {record[:2]: how often} over all pairs looked at).
    Seeded by the class's name.  tries = None stops at `count` cases; a number looks at that many candidates whatever it finds."""
    key = (name, count, tries)
    if key not in _reduce_memo:
        import random
        modulus, recipe, want = REDUCE_CLASSES[name]; rng = random.Random("reduce " + name); kept = []; seen = {}
        for k, (a, b) in enumerate(_reduce_candidates(recipe, modulus, rng)):
            if (k >= tries) if tries is not None else (len(kept) >= count or k >= 1000000): break
            rec = fold_trace(a, b, modulus)[1]; seen[rec[:2]] = seen.get(rec[:2], 0) + 1
            if len(kept) < count and record_wanted(rec, want): kept.append((a, b))
        _reduce_memo[key] = (kept, seen)
    return _reduce_memo[key]

# kind -> homestead: the flag the line is sent with.  The fold-3 carry needs a product above 0.61 x 2^512 (fold 2 must carry with its low words within C of
# 2^256, so what fold 1 hands on times C exceeds 2^256 - C, and that is hi C / 2^256 up to rounding: hi > 0.61 x 2^256), so s <= N / 2 cannot reach it in u2 = s / r:
# those lines carry a high s and go in with homestead off, where any s below N is accepted.  u1 = -m / r takes any hash, so its lines keep a low s.
CRAFTED_KINDS = {"fold3 u1": True, "fold3 u2": False, "fold3 both": False, "sub u2": True, "sub u1": True}
_crafted_memo = {}
def crafted_signatures(count=64):
    """-> [(kind, homestead, hash, sig)], `count` of each kind: signatures whose recovery multiplies, in u2 = s / r or in u1 = -m / r or in both, operands of the
    class "N (1,1)" (the fold-3 carry) or "N sub" (the final subtraction after a product with a non-zero high half).  r is an x of the curve below N; s =
    (2C - delta) r or epsilon r is kept where fold_trace shows the path and s is in 1 .. N / 2 (homestead lines) or 1 .. N - 1; the hash is the 32 bytes of
    m = (2C - delta) r or epsilon r, below N."""
    if count not in _crafted_memo:
        import random
        C = 2**256 - N; out = []
        def want_of(kind): return REDUCE_CLASSES["N (1,1)" if kind.startswith("fold3") else "N sub"][2]
        def pick(kind, r, rinv, rng, top):
            for _ in range(48):
                v = ((2 * C - rng.randrange(1, C + 1)) if kind.startswith("fold3") else rng.randrange(1, C)) * r % N
                if 1 <= v <= top and record_wanted(fold_trace(v, rinv, N)[1], want_of(kind)): return v
            return None
        for kind, homestead in CRAFTED_KINDS.items():
            rng = random.Random("crafted " + kind); n = 0; top = N // 2 if homestead else N - 1
            while n < count:
                r = rng.randrange(1, N); y2 = (r ** 3 + 7) % P
                if pow(y2, (P - 1) // 2, P) != 1: continue
                rinv = pow(r, -1, N); s = pick(kind, r, rinv, rng, top) if kind.endswith(("u2", "both")) else rng.randrange(1, top + 1)
                mm = pick(kind, r, rinv, rng, N - 1) if kind.endswith(("u1", "both")) else rng.getrandbits(256)
                if s is None or mm is None: continue
                out.append((kind, homestead, mm.to_bytes(32, "big"), r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([rng.randrange(2)]))); n += 1
        _crafted_memo[count] = out
    return _crafted_memo[count]
_crafted_expected = {}
def crafted_expected(count=64):
    """recover() of every crafted line with the line's own flag: computed once a process"""
    if count not in _crafted_expected: _crafted_expected[count] = [recover(h, sig, hs) for _, hs, h, sig in crafted_signatures(count)]
    return _crafted_expected[count]
