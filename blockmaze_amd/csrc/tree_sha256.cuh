// SHA-256 compression nodes of the commitment trees (gpu_tree.hip: the resident tree; gpu_list_roots.hip: the roots of many lists): a node as eight big-endian
// words, its load and store in blob byte order, and one compression of left || right from the standard IV, one lane per node.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace zk {

struct Node { uint32_t w[8]; };   // eight big-endian words of SHA-256, as the compression wants them
__device__ __forceinline__ Node tree_load(const uint8_t *p) {
  const uint4 a = ((const uint4 *)p)[0], b = ((const uint4 *)p)[1];
  return {{__builtin_bswap32(a.x), __builtin_bswap32(a.y), __builtin_bswap32(a.z), __builtin_bswap32(a.w), __builtin_bswap32(b.x), __builtin_bswap32(b.y),
      __builtin_bswap32(b.z), __builtin_bswap32(b.w)}};
}
__device__ __forceinline__ void tree_store(uint8_t *p, const Node &v) {
  ((uint4 *)p)[0] = make_uint4(__builtin_bswap32(v.w[0]), __builtin_bswap32(v.w[1]), __builtin_bswap32(v.w[2]), __builtin_bswap32(v.w[3]));
  ((uint4 *)p)[1] = make_uint4(__builtin_bswap32(v.w[4]), __builtin_bswap32(v.w[5]), __builtin_bswap32(v.w[6]), __builtin_bswap32(v.w[7]));
}

// (constexpr: under full unrolling every round constant is a literal of its instruction, no load and no register)
constexpr uint32_t TREE_K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74,
    0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d,
    0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e,
    0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5,
    0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
__device__ __forceinline__ uint32_t tree_rotr(uint32_t x, int n) { return __builtin_rotateright32(x, n); }
// One compression of l || r from the standard IV (FIPS 180-4 6.2.2), one lane per node.  The message schedule is a rolling window of sixteen words in registers:
// the loop is fully unrolled, so every index is a constant and the round constants are literals.
__device__ __forceinline__ Node tree_compress(const Node &l, const Node &r) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 8; i++) { w[i] = l.w[i]; w[8 + i] = r.w[i]; }
  const uint32_t H0 = 0x6a09e667, H1 = 0xbb67ae85, H2 = 0x3c6ef372, H3 = 0xa54ff53a, H4 = 0x510e527f, H5 = 0x9b05688c, H6 = 0x1f83d9ab, H7 = 0x5be0cd19;
  uint32_t a = H0, b = H1, c = H2, d = H3, e = H4, f = H5, g = H6, h = H7;
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {
      const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      w[i & 15] += (tree_rotr(w15, 7) ^ tree_rotr(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] + (tree_rotr(w2, 17) ^ tree_rotr(w2, 19) ^ (w2 >> 10));
    }
    const uint32_t t1 = h + (tree_rotr(e, 6) ^ tree_rotr(e, 11) ^ tree_rotr(e, 25)) + (g ^ (e & (f ^ g))) + TREE_K256[i] + w[i & 15];
    const uint32_t t2 = (tree_rotr(a, 2) ^ tree_rotr(a, 13) ^ tree_rotr(a, 22)) + ((a & b) | (c & (a | b)));
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  return {{a + H0, b + H1, c + H2, d + H3, e + H4, f + H5, g + H6, h + H7}};
}
// The chained form (gpu_proof_cache.hip: a message of many blocks): one compression of the sixteen words w from the state s, which becomes the next state.  w is the
// rolling window and is used up.
__device__ __forceinline__ void tree_compress_chain(uint32_t s[8], uint32_t w[16]) {
  uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {
      const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      w[i & 15] += (tree_rotr(w15, 7) ^ tree_rotr(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] + (tree_rotr(w2, 17) ^ tree_rotr(w2, 19) ^ (w2 >> 10));
    }
    const uint32_t t1 = h + (tree_rotr(e, 6) ^ tree_rotr(e, 11) ^ tree_rotr(e, 25)) + (g ^ (e & (f ^ g))) + TREE_K256[i] + w[i & 15];
    const uint32_t t2 = (tree_rotr(a, 2) ^ tree_rotr(a, 13) ^ tree_rotr(a, 22)) + ((a & b) | (c & (a | b)));
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
}

}  // namespace zk
