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
