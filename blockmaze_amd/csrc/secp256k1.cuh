// secp256k1 on CDNA4 VALU, one lane per element: the field Fq (p = 2^256 - 2^32 - 977), the scalars mod N (N = 2^256 - c, c of 129 bits), the curve y^2 = x^3 + 7 in
// Jacobian coordinates, and Keccak-f[1600].  What zkRecoverSenders runs (gpu_senders.hip; DESIGN.md "Senders from signatures").
// An element is eight 32-bit limbs, little-endian, a PLAIN integer (no Montgomery form): both moduli are 2^256 minus a small constant, so a 512-bit product
// H 2^256 + L is reduced by folding, H c + L, not by Montgomery's rows.  Products are 32 x 32 -> 64 with a 64-bit addend, which hipcc lowers to v_mad_u64_u32.
//
// THE CONTRACT (tests/test_gpu_senders.py probes every line of it through zkgpu_test_secp_ops):
//   mul, sqr                any two 256-bit values in (not only canonical ones)   -> canonical, in [0, modulus)
//   reduce                  any 256-bit value                                      -> canonical
//   add, sub, neg, is_zero  canonical values in                                    -> canonical; they are wrong above the modulus and nothing calls them there
//   inv, sqrt               a canonical value in                                   -> canonical; inv(0) = 0; sqrt returns a^((p+1)/4), a root only where one exists
// There is no lazy domain: every routine hands on canonical values, so "equal" and "zero" are limb comparisons and the point addition can branch on them.
// Everything is plain C++ with loops of constant bounds that unroll fully: no limb array is indexed by a run-time value, so none goes to scratch.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace zk {
namespace secp {

struct FqP {   // the field: 2^256 = C (mod p), C = 2^32 + 977
  static constexpr int CW = 2;
  static constexpr uint32_t MOD[8] = {0xFFFFFC2Fu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  static constexpr uint32_t C[5] = {0x000003D1u, 0x00000001u, 0, 0, 0};
};
struct FnP {   // the scalars: 2^256 = C (mod N), C = 2^256 - N
  static constexpr int CW = 5;
  static constexpr uint32_t MOD[8] = {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  static constexpr uint32_t C[5] = {0x2FC9BEBFu, 0x402DA173u, 0x50B75FC4u, 0x45512319u, 0x00000001u};
};
constexpr uint32_t N_HALF[8] = {0x681B20A0u, 0xDFE92F46u, 0x57A4501Du, 0x5D576E73u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu};   // floor(N / 2)
constexpr uint32_t N_MINUS_2_LOW[4] = {0xD036413Fu, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u};                                                  // the low 128 bits of N - 2
constexpr uint32_t GX[8] = {0x16F81798u, 0x59F2815Bu, 0x2DCE28D9u, 0x029BFCDBu, 0xCE870B07u, 0x55A06295u, 0xF9DCBBACu, 0x79BE667Eu};
constexpr uint32_t GY[8] = {0xFB10D4B8u, 0x9C47D08Fu, 0xA6855419u, 0xFD17B448u, 0x0E1108A8u, 0x5DA4FBFCu, 0x26A3C465u, 0x483ADA77u};

// a 256-bit value; what it is an element of is said by the routine that takes it
struct U256 { uint32_t l[8]; };
__device__ __forceinline__ U256 u256_zero() { U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = 0;
  return r; }
__device__ __forceinline__ U256 u256_small(uint32_t v) { U256 r = u256_zero(); r.l[0] = v; return r; }
template <class A> __device__ __forceinline__ U256 u256_of(const A &a) { U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = a[i];
  return r; }
__device__ __forceinline__ bool u256_is_zero(const U256 &a) { uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.l[i];
  return o == 0; }
__device__ __forceinline__ bool u256_eq(const U256 &a, const U256 &b) { uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= a.l[i] ^ b.l[i];
  return o == 0; }
// a >= m, m a constant
template <class M> __device__ __forceinline__ bool u256_geq(const U256 &a, const M &m) { uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a.l[i] - m[i] - br; br = (t >> 32) & 1; }
  return br == 0; }
// a - m where a >= m, else a: the one conditional subtraction that ends every reduction (a < 2^256 < 2 m for both moduli)
template <class P> __device__ __forceinline__ U256 cond_sub(const U256 &a) { U256 d; uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a.l[i] - P::MOD[i] - br; d.l[i] = (uint32_t)t; br = (t >> 32) & 1; }
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = br ? a.l[i] : d.l[i];
  return r; }

// One fold: lo + hi x C, hi of HW words: the low eight words go to `out`, the words above them to `over`.  The sum has max(8, HW + CW) + 1 words, the last one its
// carry, so `over` has fold_over(HW, CW) of them.  Rows of 32 x 32 + 32 + 32 -> 64, which never overflows: (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1.
constexpr int fold_over(int hw, int cw) { return (hw + cw > 8 ? hw + cw : 8) + 1 - 8; }
template <class P, int HW> __device__ __forceinline__ void fold(const uint32_t (&lo)[8], const uint32_t (&hi)[HW], uint32_t (&out)[8], uint32_t (&over)[fold_over(HW, P::CW)]) {
  constexpr int CW = P::CW, RW = 8 + fold_over(HW, CW); uint32_t prod[RW];
#pragma unroll
  for (int i = 0; i < RW; i++) prod[i] = 0;
#pragma unroll
  for (int i = 0; i < HW; i++) { uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < CW; j++) { const uint64_t acc = (uint64_t)hi[i] * P::C[j] + prod[i + j] + carry; prod[i + j] = (uint32_t)acc; carry = acc >> 32; }
    prod[i + CW] = (uint32_t)carry; }
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < RW; i++) { c += (uint64_t)prod[i] + (i < 8 ? lo[i] : 0u); if (i < 8) out[i] = (uint32_t)c; else over[i - 8] = (uint32_t)c; c >>= 32; }
}
// 512 bits -> canonical.  Fold 1 takes the eight high words; what it leaves above 2^256 has at most CW + 1 words (bits(C) + 1 bits: 34 for p, 130 for N); fold 2
// leaves at most 2 words (p: 1 bit, N: 4 bits); fold 3 leaves a carry of 0 or 1, and where it is 1 the low words are below 2^(bits(C) + 32), so adding C once more
// cannot carry.  Then one conditional subtraction.
// (That last carry cannot be 1 for p: fold 3 adds less than 2^34 to a value that, where fold 2 carried, is below 2^67.  For N it needs the low 256 bits after fold 2
// within 2^133 of 2^256, about one product in 2^120 at random; tests/test_gpu_senders.py reaches it with constructed operands, in the raw products and inside the
// recovery: test_raw_products_on_every_path_of_the_reduction, test_crafted_signatures_take_the_reduction_carries_inside_the_recovery.)
template <class P> __device__ __forceinline__ U256 reduce512(const uint32_t (&t)[16]) {
  constexpr int CW = P::CW, O2 = fold_over(CW + 1, CW); uint32_t lo[8], hi[8], a[8], over1[CW + 1], b[8], over2[O2], c[8], over3[1];
#pragma unroll
  for (int i = 0; i < 8; i++) { lo[i] = t[i]; hi[i] = t[8 + i]; }
  static_assert(fold_over(8, CW) == CW + 1 && fold_over(2, CW) == 1, "the widths the three folds hand on");
  fold<P, 8>(lo, hi, a, over1);
  fold<P, CW + 1>(a, over1, b, over2);                                  // (N: words 10 and 11 of the sum are zero, the value being below 2^260)
  const uint32_t h3[2] = {over2[0], O2 > 1 ? over2[O2 - 1 < 1 ? O2 - 1 : 1] : 0u};   // (p hands on one word, N two)
  fold<P, 2>(b, h3, c, over3);
  uint64_t cc = 0; U256 r; const uint32_t m = 0u - over3[0];           // over3[0] is 0 or 1
#pragma unroll
  for (int i = 0; i < 8; i++) { cc += (uint64_t)c[i] + (i < CW ? (P::C[i] & m) : 0u); r.l[i] = (uint32_t)cc; cc >>= 32; }
  return cond_sub<P>(r);
}
template <class P> __device__ __forceinline__ U256 mod_mul(const U256 &a, const U256 &b) {
  uint32_t t[16];
#pragma unroll
  for (int i = 0; i < 16; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { const uint64_t acc = (uint64_t)a.l[i] * b.l[j] + t[i + j] + carry; t[i + j] = (uint32_t)acc; carry = acc >> 32; }
    t[i + 8] = (uint32_t)carry; }
  return reduce512<P>(t);
}
template <class P> __device__ __forceinline__ U256 mod_sqr(const U256 &a) { return mod_mul<P>(a, a); }
template <class P> __device__ __forceinline__ U256 mod_reduce(const U256 &a) { return cond_sub<P>(a); }       // any 256-bit value: below 2 x modulus
template <class P> __device__ __forceinline__ U256 mod_add(const U256 &a, const U256 &b) {                    // canonical in: the sum is below 2 x modulus < 2^257
  uint64_t c = 0; U256 s;
#pragma unroll
  for (int i = 0; i < 8; i++) { c += (uint64_t)a.l[i] + b.l[i]; s.l[i] = (uint32_t)c; c >>= 32; }
  // with the carry: s + 2^256 - modulus = s + C, which cannot carry again (s + 2^256 < 2 x modulus)
  const uint32_t m = 0u - (uint32_t)c; uint64_t cc = 0; U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) { cc += (uint64_t)s.l[i] + (i < P::CW ? (P::C[i] & m) : 0u); r.l[i] = (uint32_t)cc; cc >>= 32; }
  return cond_sub<P>(r);
}
template <class P> __device__ __forceinline__ U256 mod_sub(const U256 &a, const U256 &b) {                    // canonical in
  uint64_t br = 0; U256 d;
#pragma unroll
  for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)a.l[i] - b.l[i] - br; d.l[i] = (uint32_t)t; br = (t >> 32) & 1; }
  const uint32_t m = 0u - (uint32_t)br; uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { c += (uint64_t)d.l[i] + (P::MOD[i] & m); d.l[i] = (uint32_t)c; c >>= 32; }
  return d;
}
template <class P> __device__ __forceinline__ U256 mod_neg(const U256 &a) { return mod_sub<P>(u256_zero(), a); }   // 0 - 0 borrows nothing: zero stays zero
// x^(2^n): one copy of the squaring whatever n is
template <class P> __device__ __forceinline__ U256 mod_sqn(U256 x, int n) {
#pragma unroll 1
  for (int i = 0; i < n; i++) x = mod_sqr<P>(x);
  return x; }

// ---- the field ------------------------------------------------------------------------------------------------------------------------------------------------------
using Fe = U256;
__device__ __forceinline__ Fe fe_mul(const Fe &a, const Fe &b) { return mod_mul<FqP>(a, b); }
__device__ __forceinline__ Fe fe_sqr(const Fe &a) { return mod_sqr<FqP>(a); }
__device__ __forceinline__ Fe fe_add(const Fe &a, const Fe &b) { return mod_add<FqP>(a, b); }
__device__ __forceinline__ Fe fe_sub(const Fe &a, const Fe &b) { return mod_sub<FqP>(a, b); }
__device__ __forceinline__ Fe fe_neg(const Fe &a) { return mod_neg<FqP>(a); }
__device__ __forceinline__ Fe fe_dbl(const Fe &a) { return mod_add<FqP>(a, a); }
// a^(2^223 - 1) and, on the way, a^(2^2 - 1), a^(2^22 - 1): the part that p - 2 and (p + 1) / 4 share.  p = 2^256 - 2^32 - 977 in binary is 223 ones, a zero,
// 22 ones, then 0000101111 (p - 2: 0000101101; (p + 1) / 4: 223 ones, a zero, 22 ones, 000011 00 -> shifted right by two: ... 00001100).
__device__ __forceinline__ Fe fe_x223(const Fe &a, Fe &x2, Fe &x22) {
  x2 = fe_mul(fe_sqr(a), a); const Fe x3 = fe_mul(fe_sqr(x2), a);
  const Fe x6 = fe_mul(mod_sqn<FqP>(x3, 3), x3), x9 = fe_mul(mod_sqn<FqP>(x6, 3), x3), x11 = fe_mul(mod_sqn<FqP>(x9, 2), x2);
  x22 = fe_mul(mod_sqn<FqP>(x11, 11), x11);
  const Fe x44 = fe_mul(mod_sqn<FqP>(x22, 22), x22), x88 = fe_mul(mod_sqn<FqP>(x44, 44), x44), x176 = fe_mul(mod_sqn<FqP>(x88, 88), x88);
  const Fe x220 = fe_mul(mod_sqn<FqP>(x176, 44), x44);
  return fe_mul(mod_sqn<FqP>(x220, 3), x3);
}
// a^(p - 2): 255 squarings and 15 products; inv(0) = 0
__device__ __forceinline__ Fe fe_inv(const Fe &a) {
  Fe x2, x22; Fe t = fe_x223(a, x2, x22);
  t = fe_mul(mod_sqn<FqP>(t, 23), x22); t = fe_mul(mod_sqn<FqP>(t, 5), a); t = fe_mul(mod_sqn<FqP>(t, 3), x2); return fe_mul(mod_sqn<FqP>(t, 2), a);
}
// a^((p + 1) / 4): the square root of a where a has one (p = 3 mod 4); the caller squares it and compares
__device__ __forceinline__ Fe fe_sqrt(const Fe &a) {
  Fe x2, x22; Fe t = fe_x223(a, x2, x22);
  t = fe_mul(mod_sqn<FqP>(t, 23), x22); t = fe_mul(mod_sqn<FqP>(t, 6), x2); return mod_sqn<FqP>(t, 2);
}

// ---- the scalars ----------------------------------------------------------------------------------------------------------------------------------------------------
using Sc = U256;
__device__ __forceinline__ Sc sc_mul(const Sc &a, const Sc &b) { return mod_mul<FnP>(a, b); }
// a^(N - 2) by a fixed chain: N - 2 is 127 ones, a zero, then the 128 bits of N_MINUS_2_LOW.  The ones come from a^(2^k - 1) for k = 1, 2, 4, ... 64 (127 = 64 + 32 +
// 16 + 8 + 4 + 2 + 1), the low half bit by bit; the exponent is a constant, so every lane takes every branch the same way.  255 squarings (63 + 63 + 1 + 128) and 81 products.
__device__ __forceinline__ Sc sc_inv(const Sc &a) {
  const Sc o2 = sc_mul(mod_sqn<FnP>(a, 1), a), o4 = sc_mul(mod_sqn<FnP>(o2, 2), o2), o8 = sc_mul(mod_sqn<FnP>(o4, 4), o4), o16 = sc_mul(mod_sqn<FnP>(o8, 8), o8);
  const Sc o32 = sc_mul(mod_sqn<FnP>(o16, 16), o16), o64 = sc_mul(mod_sqn<FnP>(o32, 32), o32);
  Sc t = sc_mul(mod_sqn<FnP>(o64, 32), o32); t = sc_mul(mod_sqn<FnP>(t, 16), o16); t = sc_mul(mod_sqn<FnP>(t, 8), o8); t = sc_mul(mod_sqn<FnP>(t, 4), o4);
  t = sc_mul(mod_sqn<FnP>(t, 2), o2); t = sc_mul(mod_sqn<FnP>(t, 1), a);                          // 127 ones
  t = mod_sqn<FnP>(t, 1);                                                                          // the zero
#pragma unroll
  for (int w = 3; w >= 0; w--) {
    const uint32_t bits = N_MINUS_2_LOW[w];                                                         // (a constant index: four copies of the inner loop)
#pragma unroll 1
    for (int k = 31; k >= 0; k--) { t = mod_sqr<FnP>(t); if ((bits >> k) & 1u) t = sc_mul(t, a); }
  }
  return t;
}

// ---- the curve ------------------------------------------------------------------------------------------------------------------------------------------------------
struct Ge { Fe x, y; };                       // affine, never the point at infinity
struct Gej { Fe x, y, z; bool inf; };         // Jacobian (x / z^2, y / z^3); inf says infinity and then the coordinates mean nothing
struct AddCounters { uint32_t equal = 0, opposite = 0, at_infinity = 0, to_infinity = 0; };   // the exceptional branches of gej_add_ge a lane took

// 2 a (a = 0 curve: dbl-2009-l, 2 products and 5 squarings).  The group has odd prime order, so no point has y = 0 and a finite point stays finite.
__device__ __forceinline__ Gej gej_double(const Gej &a) {
  const Fe A = fe_sqr(a.x), B = fe_sqr(a.y), C = fe_sqr(B);
  const Fe t = fe_sub(fe_sub(fe_sqr(fe_add(a.x, B)), A), C), D = fe_dbl(t), E = fe_add(fe_dbl(A), A), F = fe_sqr(E);
  Gej r; r.x = fe_sub(F, fe_dbl(D)); const Fe C8 = fe_dbl(fe_dbl(fe_dbl(C)));
  r.y = fe_sub(fe_mul(E, fe_sub(D, r.x)), C8); r.z = fe_dbl(fe_mul(a.y, a.z)); r.inf = a.inf; return r;
}
// a + b, b affine (madd: 8 products and 3 squarings), each exceptional case in a branch of its own, as libsecp256k1's gej_add_ge_var has them: a at infinity (the
// result is b), equal operands (the doubling), opposite operands (infinity).  b is never infinity: the tables hold multiples 1 .. 15 of points of prime order.
__device__ __forceinline__ Gej gej_add_ge(const Gej &a, const Ge &b, AddCounters &cnt) {
  Gej r;
  if (a.inf) { cnt.at_infinity++; r.x = b.x; r.y = b.y; r.z = u256_small(1); r.inf = false; return r; }
  const Fe zz = fe_sqr(a.z), u2 = fe_mul(b.x, zz), s2 = fe_mul(fe_mul(b.y, zz), a.z), h = fe_sub(u2, a.x), rr = fe_sub(s2, a.y);
  if (u256_is_zero(h)) {
    if (u256_is_zero(rr)) { cnt.equal++; return gej_double(a); }
    cnt.opposite++; cnt.to_infinity++; r.x = u256_zero(); r.y = u256_zero(); r.z = u256_zero(); r.inf = true; return r;
  }
  const Fe hh = fe_sqr(h), hhh = fe_mul(h, hh), v = fe_mul(a.x, hh);
  r.x = fe_sub(fe_sub(fe_sqr(rr), hhh), fe_dbl(v)); r.y = fe_sub(fe_mul(rr, fe_sub(v, r.x)), fe_mul(a.y, hhh)); r.z = fe_mul(a.z, h); r.inf = false; return r;
}

// ---- Keccak-f[1600] and the address of a key ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rotl64(uint64_t v, int n) { return n ? (v << n) | (v >> (64 - n)) : v; }
__device__ __forceinline__ void keccak_f1600(uint64_t (&s)[25]) {
  constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull,
                               0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
                               0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
                               0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  constexpr int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};   // by x + 5 y
#pragma unroll 1
  for (int round = 0; round < 24; round++) {
    uint64_t c[5], b[25];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) { const uint64_t d = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
#pragma unroll
      for (int y = 0; y < 5; y++) s[x + 5 * y] ^= d; }
#pragma unroll
    for (int x = 0; x < 5; x++)
#pragma unroll
      for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64(s[x + 5 * y], ROT[x + 5 * y]);   // rho and pi: B[y, 2x + 3y] = rot(A[x, y])
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
      for (int x = 0; x < 5; x++) s[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    s[0] ^= RC[round];
  }
}
__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
// Keccak-256 (the pre-standard padding 0x01 ... 0x80, rate 136: one block) of X || Y, 64 big-endian bytes; out[k], k = 0 .. 4: bytes 12 + 4k .. 15 + 4k of the digest
// as a little-endian word, i.e. the address as it lies in memory
__device__ __forceinline__ void address_of(const Fe &x, const Fe &y, uint32_t (&out)[5]) {
  uint64_t s[25];
#pragma unroll
  for (int i = 0; i < 25; i++) s[i] = 0;
  // byte 8 k .. 8 k + 7 of the message is lane k, little-endian: the message's bytes are the limbs from the top, each byte-swapped
#pragma unroll
  for (int k = 0; k < 4; k++) {
    s[k] = (uint64_t)bswap32(x.l[7 - 2 * k]) | ((uint64_t)bswap32(x.l[6 - 2 * k]) << 32);
    s[4 + k] = (uint64_t)bswap32(y.l[7 - 2 * k]) | ((uint64_t)bswap32(y.l[6 - 2 * k]) << 32);
  }
  s[8] = 0x01ull; s[16] = 0x8000000000000000ull;                                                  // byte 64 and byte 135
  keccak_f1600(s);
  out[0] = (uint32_t)(s[1] >> 32); out[1] = (uint32_t)s[2]; out[2] = (uint32_t)(s[2] >> 32); out[3] = (uint32_t)s[3]; out[4] = (uint32_t)(s[3] >> 32);
}
// 32 big-endian bytes at a 4-byte-aligned address <-> limbs
__device__ __forceinline__ U256 load_be(const uint32_t *p) { U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = bswap32(p[7 - i]);
  return r; }
__device__ __forceinline__ void store_be(uint32_t *p, const U256 &v) {
#pragma unroll
  for (int i = 0; i < 8; i++) p[7 - i] = bswap32(v.l[i]); }

}  // namespace secp
}  // namespace zk
