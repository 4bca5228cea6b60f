// Sender inputs from raw transactions (include/zk_txs.h): what the reference does per transaction between a block body's bytes and recoverPlain —
// rlp.DecodeBytes into txdata (rlp/decode.go; core/types/transaction.go:64-100), signer.Hash (core/types/transaction_signing.go:179-189, :231-240), the chain-id
// arithmetic on V (:151-161, :274-284), tx.Hash(), and Sender's rule for a deposit (:72-76) — for n transactions in one call, one lane a transaction.
//   k_tx_walk     the 26 headers of txdata and every rule of the strict decoder; status, code, the byte range of fields 1 .. 6, a 0xC0 recipient's position, the class
//                 of V and ZKAdrress into a descriptor; R || S and V's byte straight into the layout the recovery reads
//   k_tx_hash     2n jobs, lanes 0 .. n-1 the signing hash, n .. 2n-1 the transaction hash: Keccak-256 over a segmented byte source (a prefix in registers, one range
//                 of the input with at most one byte substituted, a suffix in registers)
//   (the recovery's six launches, gpu_senders.hip, on what the two left on the device: zkTxSenders only)
//   k_tx_finish   the walk's status merged with the recovery's ok; a deposit's sender is its ZKAdrress; refused lanes zero
// and, for zkTxRecords (include/zk_bodies.h), the same walk instantiated with a second descriptor (the positions of the ZK fields, X and Y padded, a
// deposit on HomesteadSigner's road), the same hashes and the same recovery, then
//   k_body_finish   k_tx_finish with the deposit's key rule (core/state_processor.go:141-146) and the count of records of each workgroup
//   k_body_scan     the exclusive scan of those counts, one workgroup
//   k_body_scatter  rec_of, the n + 1 prefix values, the transaction of each record, rec_froms
//   k_body_gather   a wave a record: the 180 words of a zk_block_record from the transaction's bytes
// and, for zkTxRoots, verifyChainBodiesRoots and zkgpu_list_trie_roots (include/zk_tx_roots.h), on the same sponge
//   k_trie_leaf     a lane a value: the hash of its leaf in the block's Merkle-Patricia trie (DeriveSha), at its position in the sorted order of the keys
//   k_trie_level    once a key nibble depth, deepest first: the branch, and the extension around it, at the head of every run of keys that is one
//   k_trie_finish   a lane a block: its root
// and, for zkHeaders (include/zk_headers.h), on the same head reader and the same sponge over a second source type
//   k_hdr_walk, k_hdr_hash, k_hdr_finish   (described where they stand)
// Rules every kernel keeps: no lane waits for another lane; every loop is bounded by a constant or by the transaction's own length; every
// offset taken from the input is checked against the end of its list — and so against the transaction's end — before the byte there is read; the Keccak state is
// indexed by compile-time constants only; no kernel uses scratch.
#include <algorithm>
#include <cstring>
#include <string>
#include "gpu_internal.hpp"
#include "secp256k1.cuh"
#include "txs_host.hpp"

namespace zk {
constexpr int TX_THREADS = 128;
enum { TX_OK = 0, TX_MALFORMED = 1, TX_CHAIN_ID = 2, TX_SIG = 3, TX_DEPOSIT_KEY = 4 };
enum { SIGNER_FRONTIER = 0, SIGNER_HOMESTEAD = 1, SIGNER_EIP155 = 2 };
constexpr uint32_t TX_DEPOSIT = 3;                    // transaction.go:43
// the descriptor of a lane, in words; word k of lane i lies at D[k * n + i]
constexpr int TD_META = 0 /* status | code << 8 | nine-field hash << 16 */, TD_A = 1, TD_B = 2, TD_C0 = 3 /* 0xFFFFFFFF: none */, TD_ZK = 4, TD_WORDS = 9;
// txdata's 26 fields (transaction.go:64-96), three bits a field
enum { FK_U8, FK_U64, FK_BIG, FK_ADDR_NIL, FK_BYTES, FK_HASH, FK_ADDR, FK_U64S };
constexpr int TX_FIELDS = 26, F_RECIPIENT = 4, F_PAYLOAD = 6, F_ZKVALUE = 7, F_ZKSN = 8, F_ZKSNS = 9, F_ZKADDR = 11, F_ZKCMT = 12, F_ZKCMTS = 13, F_ZKPROOF = 14, F_RTCMT = 15, F_X = 18, F_Y = 19,
              F_V = 23, F_R = 24, F_S = 25;
// the second descriptor of a lane (zkTxRecords only), word k of lane i at E[k * n + i]: ZKValue, the content positions of the five hashes, ZKProof's position and size,
// "X and Y have at most 32 bytes"
constexpr int TE_VAL_LO = 0, TE_VAL_HI = 1, TE_SN = 2, TE_SNS = 3, TE_CMT = 4, TE_CMTS = 5, TE_RT = 6, TE_PROOF = 7, TE_PROOF_SIZE = 8, TE_XY_OK = 9, TE_WORDS = 10;
constexpr uint64_t fk_pack(const int *k, int from, int to) { uint64_t v = 0; for (int i = from; i < to; i++) v |= (uint64_t)k[i] << (3 * (i - from)); return v; }
constexpr int FKINDS[TX_FIELDS] = {FK_U8, FK_U64, FK_BIG, FK_U64, FK_ADDR_NIL, FK_BIG, FK_BYTES, FK_U64, FK_HASH, FK_HASH, FK_U64, FK_ADDR, FK_HASH, FK_HASH, FK_BYTES, FK_HASH,
                                    FK_U64S, FK_BYTES, FK_BIG, FK_BIG, FK_BIG, FK_BIG, FK_BIG, FK_BIG, FK_BIG, FK_BIG};
constexpr uint64_t FK_LO = fk_pack(FKINDS, 0, 16), FK_HI = fk_pack(FKINDS, 16, TX_FIELDS);

// ---- the walk -----------------------------------------------------------------------------------------------------------------------------------------------------
enum { K_BYTE, K_STR, K_LIST };
struct Head { uint32_t kind, beg, size; bool bad; };  // beg, size: the content, relative to the transaction's first byte
// Stream.readKind (decode.go:902-960) with Kind's bound (:883-894): the header at pos of a list that ends at lim (pos < lim <= the transaction's length < 2^32).  Every
// byte of the header lies below lim (willRead, :1016-1034); the content ends at or below lim.
__device__ __forceinline__ Head tx_head(const uint8_t *__restrict__ t, uint32_t pos, uint32_t lim) {
  Head h; h.kind = K_BYTE; h.beg = pos; h.size = 1; h.bad = true;
  if (pos >= lim) return h;
  const uint32_t b = t[pos];
  if (b < 0x80u) { h.bad = false; return h; }                                                      // :919-923: the byte is its own encoding
  const bool list = b >= 0xC0u; const uint32_t form = b - (list ? 0xC0u : 0x80u); uint64_t size = form; uint32_t beg = pos + 1;
  if (form >= 56u) {                                                                                // :930-941, :949-960: the length of the length
    const uint32_t ll = form - 55u;                                                                 // 1 .. 8
    if (ll > lim - pos - 1) return h;
    size = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) if (k < ll) { const uint32_t c = t[pos + 1 + k]; if (k == 0 && ll > 1 && c == 0) return h;   // readUint :980-985: a leading zero
        size = (size << 8) | c; }
    if (size < 56) return h;                                                                        // :938, :957
    beg = pos + 1 + ll;
  }
  if (size > (uint64_t)(lim - beg)) return h;                                                       // :886, :891; 2^32 and 2^63 end here
  h.kind = list ? K_LIST : K_STR; h.beg = beg; h.size = (uint32_t)size;
  if (!list && size == 1 && t[beg] < 0x80u) return h;                                               // :662, :423, :726: the byte should have stood alone
  h.bad = false; return h;
}
// Stream.uint (:703-734): a string of at most maxbytes bytes with no leading zero, the byte 0x00 refused
__device__ __forceinline__ bool tx_uint_ok(const uint8_t *__restrict__ t, const Head &h, uint32_t maxbytes) {
  if (h.kind == K_LIST) return false;                                                               // :732
  if (h.kind == K_STR && h.size > maxbytes) return false;                                           // :716
  if (h.size && t[h.beg] == 0) return false;                                                        // :710; readUint :980 with :721-723
  return true;
}
// 32 bytes at dst: the string left-padded with zeros, or zeros where it does not fit or is not wanted
__device__ __forceinline__ void tx_put32(uint8_t *__restrict__ dst, const uint8_t *__restrict__ t, uint32_t beg, uint32_t size, bool want) {
  const uint32_t pad = 32u - (size <= 32u ? size : 32u);
#pragma unroll 4
  for (uint32_t k = 0; k < 32; k++) dst[k] = (want && size <= 32u && k >= pad) ? t[beg + (k - pad)] : (uint8_t)0;
}
// BODIES (zkTxRecords): E, xy and first_bad are written as well, and a deposit takes HomesteadSigner's road; without it they are never touched and the kernel is the
// one zkTxSigningInputs and zkTxSenders have always run.
template <bool BODIES>
__global__ void __launch_bounds__(TX_THREADS) k_tx_walk(const uint8_t *__restrict__ txs, const uint64_t *__restrict__ off, uint32_t n, int signer, uint64_t chain_id, uint32_t *__restrict__ D,
                                                         uint8_t *__restrict__ rs, uint8_t *__restrict__ vout, uint8_t *__restrict__ sigs65, uint32_t *__restrict__ E, uint8_t *__restrict__ xy,
                                                         uint32_t *__restrict__ first_bad) {
  const uint32_t i = blockIdx.x * TX_THREADS + threadIdx.x; if (i >= n) return;
  uint32_t valbeg = 0, valsize = 0, sn = 0, sns = 0, cmt = 0, cmts = 0, rt = 0, pbeg = 0, psize = 0, xbeg = 0, xsize = 0, ybeg = 0, ysize = 0;   // (dead without BODIES)
  if constexpr (BODIES) { if (i == 0) first_bad[0] = n; }                                          // k_body_finish's atomicMin starts from "none"
  const uint64_t base = off[0], o0 = off[i] - base, len64 = off[i + 1] - off[i]; const uint8_t *t = txs + o0;   // (the host has checked that off does not decrease)
  bool bad = len64 == 0 || len64 > 0xFFFFFFFFull; const uint32_t len = (uint32_t)len64;
  uint32_t code = 0, a = 0, b = 0, c0 = 0xFFFFFFFFu, zk = 0, vbeg = 0, vsize = 0, rbeg = 0, rsize = 0, sbeg = 0, ssize = 0, pos = 0, lim = 0;
  if (!bad) { const Head o = tx_head(t, 0, len);                                                    // the outer item: a list (:438, :762) that ends where the input ends (:142-144)
    bad = o.bad || o.kind != K_LIST || o.beg + o.size != len; pos = o.beg; lim = len; }
#pragma unroll 1
  for (int f = 0; f < TX_FIELDS && !bad; f++) {
    if (pos == lim) { bad = true; break; }                                                          // :443-444: too few elements
    const Head h = tx_head(t, pos, lim); if (h.bad) { bad = true; break; }
    const uint32_t kind = (uint32_t)((f < 16 ? FK_LO >> (3 * f) : FK_HI >> (3 * (f - 16))) & 7u), start = pos; pos = h.beg + h.size;
    switch (kind) {
      case FK_U8: bad = !tx_uint_ok(t, h, 1); if (!bad) code = h.size ? t[h.beg] : 0u; break;
      case FK_U64: bad = !tx_uint_ok(t, h, 8); break;
      case FK_BIG: bad = h.kind == K_LIST || (h.size && t[h.beg] == 0); break;                      // :271-287; the byte 0x00 is a one-byte string here, refused by :282
      case FK_BYTES: bad = h.kind == K_LIST; break;                                                 // :386-393, :667
      case FK_HASH: bad = h.kind != K_STR || h.size != 32; break;                                   // :395-430
      case FK_ADDR: bad = h.kind != K_STR || h.size != 20; break;
      case FK_ADDR_NIL: if (h.kind != K_BYTE && h.size == 0) { if (h.kind == K_LIST) c0 = start; }  // :486-496: an empty string or an empty list is nil; the list re-encodes as 0x80
        else bad = h.kind != K_STR || h.size != 20; break;
      default:                                                                                      // []uint64: :323-336
        bad = h.kind != K_LIST;
        if (!bad) { uint32_t p = h.beg; const uint32_t e = h.beg + h.size;
#pragma unroll 1
          while (p < e) { const Head u = tx_head(t, p, e); if (u.bad || !tx_uint_ok(t, u, 8)) { bad = true; break; } p = u.beg + u.size; } }   // (p grows by at least one byte a turn)
        break;
    }
    if (f == 1) a = start;
    if (f == F_PAYLOAD) b = pos;
    if (f == F_ZKADDR) zk = h.beg;
    if (f == F_V) { vbeg = h.beg; vsize = h.size; }
    if (f == F_R) { rbeg = h.beg; rsize = h.size; }
    if (f == F_S) { sbeg = h.beg; ssize = h.size; }
    if constexpr (BODIES) {
      if (f == F_ZKVALUE) { valbeg = h.beg; valsize = h.size; }
      if (f == F_ZKSN) sn = h.beg;
      if (f == F_ZKSNS) sns = h.beg;
      if (f == F_ZKCMT) cmt = h.beg;
      if (f == F_ZKCMTS) cmts = h.beg;
      if (f == F_ZKPROOF) { pbeg = h.beg; psize = h.size; }
      if (f == F_RTCMT) rt = h.beg;
      if (f == F_X) { xbeg = h.beg; xsize = h.size; }
      if (f == F_Y) { ybeg = h.beg; ysize = h.size; }
    }
  }
  if (!bad && pos != lim) bad = true;                                                               // :449, :778: too many elements
  uint32_t status = TX_MALFORMED, nine = 0, vbyte = 0; bool put_v = false, put_r = false, put_s = false;
  if (!bad) {
    uint64_t v = 0;                                                                                 // V where it has at most 64 bits
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) if (k < vsize && vsize <= 8) v = (v << 8) | t[vbeg + k];
    const bool is_protected = !(vsize <= 1 && (v == 27 || v == 28));                                // transaction.go:165-172 (canonical: BitLen <= 8 is "at most one byte")
    bool mismatch = false, vfits = vsize <= 1; uint64_t vs = v;
    if (signer == SIGNER_EIP155 && is_protected) {                                                  // transaction_signing.go:151-161
      nine = 1;
      mismatch = vsize > 8 || (v - 35) / 2 != chain_id;                                             // :274-284 in uint64, the wrap below 35 included; wider than 64 bits never matches an id below 2^62
      vs = v - 2 * chain_id - 8; vfits = !mismatch;                                                 // :158-159: 27 or 28 where the id matched
    }
    vbyte = (uint32_t)((vs - 27) & 0xFFu);                                                          // :250
    if (code == TX_DEPOSIT) { status = TX_OK; put_r = rsize <= 32; put_s = ssize <= 32; put_v = vfits; }   // :72-76: V, R, S never looked at; written where they fit
    else { status = mismatch ? TX_CHAIN_ID : (!vfits || rsize > 32 || ssize > 32) ? TX_SIG : TX_OK; put_r = put_s = put_v = status == TX_OK; }   // :155-157, :247, :255-258
    if constexpr (BODIES) {
      if (code == TX_DEPOSIT) {                                                                     // state_processor.go:141: ExtractPKBAddress(HomesteadSigner{}, tx), whatever the block's signer
        nine = 0;                                                                                   // transaction_signing.go:206-208 with :231-240: HomesteadSigner hashes six fields, always
        const bool v_ok = vsize <= 1 && (v == 27 || v == 28);                                       // :96-113 -> recoverPlain :247 BitLen() > 8, :250 V - 27, crypto.go:209 v == 0 || v == 1; no chain id
        vbyte = (uint32_t)((v - 27) & 0xFFu);
        status = (v_ok && rsize <= 32 && ssize <= 32) ? TX_OK : TX_DEPOSIT_KEY;                     // :255-258: R and S go into 32-byte fields
        put_r = put_s = put_v = status == TX_OK;
      }
    }
  }
  const size_t nn = n;
  D[TD_META * nn + i] = status | (bad ? 0u : code << 8) | (nine << 16); D[TD_A * nn + i] = a; D[TD_B * nn + i] = b; D[TD_C0 * nn + i] = c0;
#pragma unroll
  for (uint32_t k = 0; k < 5; k++) { uint32_t w = 0;
    if (!bad) { w = (uint32_t)t[zk + 4 * k] | ((uint32_t)t[zk + 4 * k + 1] << 8) | ((uint32_t)t[zk + 4 * k + 2] << 16) | ((uint32_t)t[zk + 4 * k + 3] << 24); }
    D[(TD_ZK + k) * nn + i] = w; }
  tx_put32(rs + 64 * (size_t)i, t, rbeg, rsize, put_r); tx_put32(rs + 64 * (size_t)i + 32, t, sbeg, ssize, put_s); vout[i] = put_v ? (uint8_t)vbyte : (uint8_t)0;
  if (sigs65) { uint8_t *q = sigs65 + 65 * (size_t)i; tx_put32(q, t, rbeg, rsize, put_r); tx_put32(q + 32, t, sbeg, ssize, put_s); q[64] = put_v ? (uint8_t)vbyte : (uint8_t)0; }
  if constexpr (BODIES) {
    uint64_t val = 0;                                                                               // ZKValue: at most 8 bytes (the walk has refused more)
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) if (!bad && k < valsize && valsize <= 8) val = (val << 8) | t[valbeg + k];
    const bool dep = !bad && code == TX_DEPOSIT && status == TX_OK, xy_ok = xsize <= 32 && ysize <= 32;   // crypto.go:136-141: elliptic.Marshal cannot hold more than 32 bytes a coordinate
    const uint32_t e[TE_WORDS] = {(uint32_t)val, (uint32_t)(val >> 32), sn, sns, cmt, cmts, rt, pbeg, psize, xy_ok ? 1u : 0u};
#pragma unroll
    for (int k = 0; k < TE_WORDS; k++) E[k * nn + i] = bad ? 0u : e[k];
    tx_put32(xy + 64 * (size_t)i, t, xbeg, xsize, dep && xy_ok); tx_put32(xy + 64 * (size_t)i + 32, t, ybeg, ysize, dep && xy_ok);   // pad32(X) || pad32(Y)
  }
}

// ---- the sponge ---------------------------------------------------------------------------------------------------------------------------------------------------
// The message: pre_len bytes of (pre_lo, pre_hi), then src[0 .. src_len) with the byte at sub (an index into src; none where it is not below src_len) read as 0x80,
// then suf_len bytes of (suf_lo, suf_hi).  Byte k of a pair is bits 8k .. 8k+7 of lo for k < 8, of hi above.
struct ByteSource { uint64_t pre_lo, pre_hi, suf_lo, suf_hi; uint32_t pre_len, suf_len; const uint8_t *src; uint64_t src_len, sub; };
__device__ __forceinline__ uint64_t bs_total(const ByteSource &m) { return (uint64_t)m.pre_len + m.src_len + m.suf_len; }
// the byte at j of the padded message: the message, then pad, then zeros (the final 0x80 is the caller's)
__device__ __forceinline__ uint64_t bs_byte(const ByteSource &m, uint64_t j, uint32_t pad) {
  if (j < m.pre_len) return ((j < 8 ? m.pre_lo >> (8 * j) : m.pre_hi >> (8 * (j - 8))) & 0xFFull);
  uint64_t q = j - m.pre_len;
  if (q < m.src_len) return q == m.sub ? 0x80ull : (uint64_t)m.src[q];
  q -= m.src_len;
  if (q < m.suf_len) return ((q < 8 ? m.suf_lo >> (8 * q) : m.suf_hi >> (8 * (q - 8))) & 0xFFull);
  return q == m.suf_len ? (uint64_t)pad : 0ull;
}
// bytes j .. j+7 as a little-endian word: one 8-byte read where all eight lie in src and none is substituted
__device__ __forceinline__ uint64_t bs_word(const ByteSource &m, uint64_t j, uint32_t pad) {
  const uint64_t q = j - m.pre_len;
  if (j >= m.pre_len && q + 8 <= m.src_len && m.sub - q >= 8) { uint64_t w; __builtin_memcpy(&w, m.src + q, 8); return w; }   // (sub - q wraps to a large value for sub < q)
  uint64_t w = 0;
#pragma unroll 1
  for (uint32_t k = 0; k < 8; k++) w |= bs_byte(m, j + k, pad) << (8 * k);
  return w;
}
// rate 136, capacity 512, 32 bytes out: total / 136 + 1 blocks, the last one padded pad ... 0x80; out[k]: bytes 4k .. 4k+3 of the digest as they lie in memory
// (Src: ByteSource, or the headers' HdrSource below, through their own bs_total and bs_word)
template <class Src> __device__ __forceinline__ void sponge256(const Src &m, uint32_t pad, uint32_t (&out)[8]) {
  uint64_t s[25];
#pragma unroll
  for (int k = 0; k < 25; k++) s[k] = 0;
  const uint64_t blocks = bs_total(m) / 136 + 1;
#pragma unroll 1
  for (uint64_t blk = 0; blk < blocks; blk++) {
#pragma unroll
    for (int k = 0; k < 17; k++) s[k] ^= bs_word(m, 136 * blk + 8 * k, pad);
    if (blk + 1 == blocks) s[16] ^= 0x8000000000000000ull;
    secp::keccak_f1600(s);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) { out[2 * k] = (uint32_t)s[k]; out[2 * k + 1] = (uint32_t)(s[k] >> 32); }
}
// the encoding of a list's or an integer's length: the bytes of v from its top non-zero byte down, first byte lowest in the result; *count = how many
__device__ __forceinline__ uint64_t be_bytes(uint64_t v, uint32_t *count) {
  uint32_t c = 0; uint64_t r = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) { const uint64_t byte = (v >> (8 * k)) & 0xFFull; if (v >> (8 * k)) { r = (r << 8) | byte; c++; } }
  *count = c; return r;
}
__global__ void __launch_bounds__(TX_THREADS) k_tx_hash(const uint8_t *__restrict__ txs, const uint64_t *__restrict__ off, uint32_t n, uint64_t chain_id, const uint32_t *__restrict__ D,
                                                         uint32_t *__restrict__ sighash, uint32_t *__restrict__ txhash) {
  const uint32_t j = blockIdx.x * TX_THREADS + threadIdx.x; if (j >= 2 * n) return;
  const bool whole = j >= n; const uint32_t i = whole ? j - n : j; const size_t nn = n; uint32_t *out = (whole ? txhash : sighash) + 8 * (size_t)i;
  if (whole && !txhash) return;
  const uint32_t meta = D[TD_META * nn + i];
  if ((meta & 0xFFu) == TX_MALFORMED) {
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = 0u;
    return; }
  const uint64_t base = off[0], o0 = off[i] - base, len = off[i + 1] - off[i]; const uint32_t a = D[TD_A * nn + i], b = D[TD_B * nn + i], c0 = D[TD_C0 * nn + i];
  ByteSource m; m.pre_lo = m.pre_hi = m.suf_lo = m.suf_hi = 0; m.pre_len = m.suf_len = 0;
  if (whole) { m.src = txs + o0; m.src_len = len; m.sub = c0 == 0xFFFFFFFFu ? ~0ull : (uint64_t)c0; }   // tx.Hash(): the input, a 0xC0 recipient as the reference re-encodes it
  else {                                                                                           // signer.Hash: a fresh list header, fields 1 .. 6 as they stand, the signer's three
    m.src = txs + o0 + a; m.src_len = b - a; m.sub = c0 == 0xFFFFFFFFu ? ~0ull : (uint64_t)(c0 - a);
    if ((meta >> 16) & 1u) { uint32_t c; const uint64_t id = be_bytes(chain_id, &c);               // chain_id, 0, 0 (transaction_signing.go:187)
      if (c == 0) { m.suf_lo = 0x808080ull; m.suf_len = 3; }
      else if (c == 1 && chain_id < 0x80) { m.suf_lo = chain_id | 0x808000ull; m.suf_len = 3; }
      else { m.suf_lo = (0x80ull + c) | (id << 8); m.suf_hi = c == 8 ? id >> 56 : 0;               // 0x80 + c, the c bytes, 0x80 0x80
        const uint32_t at = 1 + c; if (at < 8) m.suf_lo |= 0x80ull << (8 * at); else m.suf_hi |= 0x80ull << (8 * (at - 8));
        if (at + 1 < 8) m.suf_lo |= 0x80ull << (8 * (at + 1)); else m.suf_hi |= 0x80ull << (8 * (at + 1 - 8));
        m.suf_len = c + 3; } }
    const uint64_t payload = m.src_len + m.suf_len;
    if (payload < 56) { m.pre_lo = 0xC0ull + payload; m.pre_len = 1; }
    else { uint32_t c; const uint64_t l = be_bytes(payload, &c); m.pre_lo = (0xF7ull + c) | (l << 8); m.pre_hi = c == 8 ? l >> 56 : 0; m.pre_len = 1 + c; }
  }
  uint32_t h[8]; sponge256(m, 0x01u, h);
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = h[k];
}
// n arbitrary byte strings through the same sponge (zkgpu_test_keccak256)
__global__ void __launch_bounds__(TX_THREADS) k_tx_keccak(const uint8_t *__restrict__ msgs, const uint64_t *__restrict__ off, uint32_t n, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * TX_THREADS + threadIdx.x; if (i >= n) return;
  ByteSource m; m.pre_lo = m.pre_hi = m.suf_lo = m.suf_hi = 0; m.pre_len = m.suf_len = 0; m.src = msgs + (off[i] - off[0]); m.src_len = off[i + 1] - off[i]; m.sub = ~0ull;
  uint32_t h[8]; sponge256(m, 0x01u, h);
#pragma unroll
  for (int k = 0; k < 8; k++) out[8 * (size_t)i + k] = h[k];
}
// ok == null: zkTxSigningInputs — froms is deposit_from.  Otherwise the recovery's verdict and sender are merged in.
__global__ void __launch_bounds__(TX_THREADS) k_tx_finish(uint32_t n, const uint32_t *__restrict__ D, const uint8_t *__restrict__ ok, const uint32_t *__restrict__ recovered,
                                                           uint32_t *__restrict__ froms, uint8_t *__restrict__ status_out, uint8_t *__restrict__ code_out, const uint32_t *__restrict__ head,
                                                           uint32_t *__restrict__ head_out) {
  const uint32_t i = blockIdx.x * TX_THREADS + threadIdx.x; if (i >= n) return;
  if (i == 0) {                                                                                     // the recovery's four counters ride in the one download (written by launches that have ended)
#pragma unroll
    for (int k = 0; k < 4; k++) head_out[k] = head ? head[k] : 0u; }
  const size_t nn = n; const uint32_t meta = D[TD_META * nn + i], code = (meta >> 8) & 0xFFu; uint32_t status = meta & 0xFFu; uint32_t f[5] = {0, 0, 0, 0, 0};
  if (status == TX_OK) {
    if (code == TX_DEPOSIT) {
#pragma unroll
      for (int k = 0; k < 5; k++) f[k] = D[(TD_ZK + k) * nn + i]; }
    else if (ok) {
      if (ok[i]) {
#pragma unroll
        for (int k = 0; k < 5; k++) f[k] = recovered[5 * (size_t)i + k]; }
      else status = TX_SIG;                                                                         // whatever recoverPlain refuses
    }
  }
#pragma unroll
  for (int k = 0; k < 5; k++) froms[5 * (size_t)i + k] = f[k];
  status_out[i] = (uint8_t)status; code_out[i] = (uint8_t)code;
}

// ---- records from the bodies' bytes (include/zk_bodies.h) ------------------------------------------------------------------------------------------
constexpr int BODY_SCAN_THREADS = 256, BODY_GATHER_THREADS = 256, REC_WORDS = 180;                 // (a scan tile covers 256 x 128 = 32,768 transactions)
constexpr uint32_t KIND_MINT = 0, KIND_SEND = 1, KIND_DEPOSIT = 2, KIND_REDEEM = 3;                // zk_batch.h
enum { BH_FIRST_BAD = 0, BH_M = 1, BH_WORDS = 4 };
// txdata.Code (transaction.go:40-46) -> ZK_KIND_* + 1, 0 where ApplyTransaction has no ZK branch (state_processor.go:108-164: codes 0 and 4, and every code above 5)
__device__ __forceinline__ uint32_t body_kind1(uint32_t code) { return code == 1 ? KIND_MINT + 1 : code == 2 ? KIND_SEND + 1 : code == 3 ? KIND_DEPOSIT + 1 : code == 5 ? KIND_REDEEM + 1 : 0u; }
// a > floor(N / 2)
__device__ __forceinline__ bool above_half_n(const secp::U256 &a) { uint64_t br = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) { const uint64_t t = (uint64_t)secp::N_HALF[k] - a.l[k] - br; br = (t >> 32) & 1; }
  return br != 0; }
// k_tx_finish for zkTxSenders, and beside it: a deposit's key rule; has_rec[i] (0 / 1: k_body_scatter replaces it by rec_of); the records of this workgroup in counts;
// the first lane with status != OK in head[BH_FIRST_BAD] (the walk has set it to n).  Every lane reaches the one barrier.
__global__ void __launch_bounds__(TX_THREADS) k_body_finish(uint32_t n, int homestead, const uint32_t *__restrict__ D, const uint32_t *__restrict__ E, const uint8_t *__restrict__ ok,
                                                             const uint32_t *__restrict__ recovered, const uint32_t *__restrict__ rs, const uint32_t *__restrict__ xy, uint32_t *__restrict__ froms,
                                                             uint8_t *__restrict__ status_out, uint8_t *__restrict__ code_out, int32_t *__restrict__ has_rec, uint32_t *__restrict__ counts,
                                                             uint32_t *__restrict__ head, const uint32_t *__restrict__ sp_head) {
  const uint32_t i = blockIdx.x * TX_THREADS + threadIdx.x; int has = 0;
  if (i < n) {
    if (i == 0) {                                                                                   // the recovery's four counters ride in the one download
#pragma unroll
      for (int k = 0; k < 4; k++) head[BH_WORDS + k] = sp_head[k]; }
    const size_t nn = n; const uint32_t meta = D[TD_META * nn + i], code = (meta >> 8) & 0xFFu; uint32_t status = meta & 0xFFu; uint32_t f[5] = {0, 0, 0, 0, 0};
    if (status == TX_OK) {
      if (code == TX_DEPOSIT) {
        // state_processor.go:141-146: addr1 = ExtractPKBAddress(HomesteadSigner{}, tx) must exist and equal addr2 = PubkeyToAddress({X, Y})
        bool good = ok[i] != 0;                                                                     // recoverPlain (transaction_signing.go:246-271) over the six-field hash
        if (good && !homestead) good = !above_half_n(secp::load_be(rs + 16 * (size_t)i + 8));      // :251 with homestead = true (crypto.go:205: s <= N / 2) where the call's recovery ran without it
        good = good && E[TE_XY_OK * nn + i] != 0;                                                   // crypto.go:136-141: X or Y of more than 32 bytes kills a reference node; refused here
        if (good) { uint32_t a[5]; secp::address_of(secp::load_be(xy + 16 * (size_t)i), secp::load_be(xy + 16 * (size_t)i + 8), a);   // crypto.go:212-215: Keccak256(pad32(X) || pad32(Y))[12:]
#pragma unroll
          for (int k = 0; k < 5; k++) good = good && a[k] == recovered[5 * (size_t)i + k]; }        // :144 addr1 != addr2; no curve check on (X, Y): the reference makes none
        if (good) {
#pragma unroll
          for (int k = 0; k < 5; k++) f[k] = D[(TD_ZK + k) * nn + i]; }                             // Sender is ZKAdrress all the same (transaction_signing.go:72-76)
        else status = TX_DEPOSIT_KEY;
      }
      else if (ok[i]) {
#pragma unroll
        for (int k = 0; k < 5; k++) f[k] = recovered[5 * (size_t)i + k]; }
      else status = TX_SIG;                                                                         // whatever recoverPlain refuses
    }
#pragma unroll
    for (int k = 0; k < 5; k++) froms[5 * (size_t)i + k] = f[k];
    status_out[i] = (uint8_t)status; code_out[i] = (uint8_t)code;
    has = status == TX_OK && body_kind1(code) != 0; has_rec[i] = has;
    if (status != TX_OK) atomicMin(head + BH_FIRST_BAD, i);
  }
  const int count = __syncthreads_count(has);
  if (threadIdx.x == 0) counts[blockIdx.x] = (uint32_t)count;
}
// an inclusive scan of one value a lane over a workgroup of T lanes through sh (T values); every lane calls it.  V: uint32_t, or uint64_t for the split's scans
template <int T, class V> __device__ __forceinline__ V block_scan_inclusive(V v, V *sh) {
  sh[threadIdx.x] = v; __syncthreads();
#pragma unroll
  for (int d = 1; d < T; d <<= 1) { const V add = threadIdx.x >= (uint32_t)d ? sh[threadIdx.x - d] : (V)0; __syncthreads(); v += add; sh[threadIdx.x] = v; __syncthreads(); }
  return v;
}
// bases[b] = the records before workgroup b; head[BH_M] = m.  One workgroup; cdiv(nb, 256) tiles, a carry between them; the loop's bound is the same for every lane.
__global__ void __launch_bounds__(BODY_SCAN_THREADS) k_body_scan(const uint32_t *__restrict__ counts, uint32_t nb, uint32_t *__restrict__ bases, uint32_t *__restrict__ head) {
  __shared__ uint32_t sh[BODY_SCAN_THREADS]; uint32_t carry = 0;
#pragma unroll 1
  for (uint32_t base = 0; base < nb; base += BODY_SCAN_THREADS) {
    const uint32_t b = base + threadIdx.x, v = b < nb ? counts[b] : 0u, incl = block_scan_inclusive<BODY_SCAN_THREADS>(v, sh);
    if (b < nb) bases[b] = carry + incl - v;
    carry += sh[BODY_SCAN_THREADS - 1]; __syncthreads();                                            // (sh is written again in the next turn)
  }
  if (threadIdx.x == 0) head[BH_M] = carry;
}
// prefix[i] = the records before transaction i, prefix[n] = m; rec_of[i] (it held has_rec[i]); src_of[j] = the transaction of record j; rec_froms[j] = froms of it
__global__ void __launch_bounds__(TX_THREADS) k_body_scatter(uint32_t n, const uint32_t *__restrict__ bases, const uint32_t *__restrict__ froms, int32_t *__restrict__ rec_of,
                                                              uint32_t *__restrict__ prefix, uint32_t *__restrict__ src_of, uint32_t *__restrict__ rec_froms) {
  __shared__ uint32_t sh[TX_THREADS];
  const uint32_t i = blockIdx.x * TX_THREADS + threadIdx.x, has = i < n ? (uint32_t)rec_of[i] : 0u, incl = block_scan_inclusive<TX_THREADS>(has, sh);
  if (i >= n) return;                                                                              // (after the last barrier)
  const uint32_t pre = bases[blockIdx.x] + incl - has;                                             // pre < m <= n where has is set
  prefix[i] = pre; rec_of[i] = has ? (int32_t)pre : -1;
  if (i == n - 1) prefix[n] = pre + has;
  if (has) { src_of[pre] = i;
#pragma unroll
    for (int k = 0; k < 5; k++) rec_froms[5 * (size_t)pre + k] = froms[5 * (size_t)i + k]; }
}
// Four source bytes at byte offset a of the upload as a little-endian word.  ALIGNED: from one or two aligned words and a shift (the upload starts at an aligned
// address and is padded to 8 bytes: the bytes of the second word that are shifted out lie inside it); otherwise four byte reads.  The caller has compared a + 3 with the
// end of the field, which the walk has compared with the end of the transaction.
template <bool ALIGNED> __device__ __forceinline__ uint32_t body_word(const uint8_t *__restrict__ up, uint64_t a) {
  if constexpr (ALIGNED) {
    const uint32_t *w = (const uint32_t *)up; const uint64_t k = a >> 2; const uint32_t sh = 8u * (uint32_t)(a & 3u); uint32_t v = w[k];
    if (sh) v = (v >> sh) | (w[k + 1] << (32u - sh));
    return v;
  }
  else return (uint32_t)up[a] | ((uint32_t)up[a + 1] << 8) | ((uint32_t)up[a + 2] << 16) | ((uint32_t)up[a + 3] << 24);
}
// A wave a record: word w of record j, w = lane, lane + 64, lane + 128 < 180, is written by one lane, whatever it holds — the kind, ZKValue, the proof's characters or
// the zeros behind a short proof, an argument, a zero slot — so no byte of recs[0 .. m) is left as the allocation had it.  The fields in zk_verify_item's order
// (zktx.go:122-133 mint, :148-160 send, :180-194 deposit, :198-210 redeem; state_processor.go:113, :124, :147, :158 for what the node passes).
template <bool ALIGNED>
__global__ void __launch_bounds__(BODY_GATHER_THREADS) k_body_gather(const uint8_t *__restrict__ up, const uint64_t *__restrict__ off, uint32_t n, const uint32_t *__restrict__ D,
                                                                      const uint32_t *__restrict__ E, const uint32_t *__restrict__ recovered, const uint32_t *__restrict__ src_of,
                                                                      const uint32_t *__restrict__ prefix, uint32_t *__restrict__ recs) {
  const uint32_t j = (blockIdx.x * BODY_GATHER_THREADS + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
  if (j >= n || j >= prefix[n]) return;                                                            // (the whole wave: the grid is sized for n records, m is known on the device only)
  const uint32_t i = src_of[j]; if (i >= n) return;
  const size_t nn = n; const uint64_t o0 = off[i] - off[0]; const uint32_t code = (D[TD_META * nn + i] >> 8) & 0xFFu, kind1 = body_kind1(code);
  const uint32_t pbeg = E[TE_PROOF * nn + i], psize = E[TE_PROOF_SIZE * nn + i], take = psize < 512u ? psize : 512u;   // the first 512 characters: verify* reads no more
  const bool valued = code == 1 || code == 5, dep = code == TX_DEPOSIT, send = code == 2;
#pragma unroll
  for (uint32_t r = 0; r < 3; r++) {
    const uint32_t w = lane + 64u * r; if (w >= (uint32_t)REC_WORDS) break;
    uint32_t val = 0;
    if (w == 0) val = kind1 - 1u;                                                                   // kind; reserved[0 .. 2] = 0 (word 1: reserved[3 .. 6] = 0)
    else if (w == 2) val = valued ? E[TE_VAL_LO * nn + i] : 0u;                                     // value_s: ZKValue for mint and redeem, 0 otherwise
    else if (w == 3) val = valued ? E[TE_VAL_HI * nn + i] : 0u;
    else if (w >= 4 && w < 132) {
      const uint32_t p = 4u * (w - 4u);
      if (p + 4u <= take) val = body_word<ALIGNED>(up, o0 + pbeg + p);
      else if (p < take) {                                                                          // the last characters of a proof shorter than 512: zero bytes behind them
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) if (p + k < take) val |= (uint32_t)up[o0 + pbeg + p + k] << (8u * k); }
    }
    else if (w >= 132) {
      const uint32_t a = (w - 132u) >> 3, q = (w - 132u) & 7u; uint32_t te = 0xFFFFFFFFu;           // which hash of the transaction is args[a]; none: zero
      if (dep) { te = a == 0 ? TE_RT : a == 3 ? TE_SN : a == 4 ? TE_CMT : a == 5 ? TE_SNS : 0xFFFFFFFFu;   // RTcmt, pk, old, ZKSN, ZKCMT, ZKSNS
        if (a == 1 && q < 5) val = recovered[5 * (size_t)i + q]; }                                  // the pk address: the recovered one, equal to PubkeyToAddress({X, Y}); twelve zero bytes behind it
      else if (send) te = a == 1 ? TE_SN : a == 2 ? TE_CMTS : a == 3 ? TE_CMT : 0xFFFFFFFFu;        // old, ZKSN, ZKCMTS, ZKCMT
      else te = a == 1 ? TE_SN : a == 2 ? TE_CMT : 0xFFFFFFFFu;                                     // old, ZKSN, ZKCMT
      if (te != 0xFFFFFFFFu) val = body_word<ALIGNED>(up, o0 + E[te * nn + i] + 4u * q);            // (a hash has exactly 32 bytes: the walk refused every other length)
    }
    recs[(size_t)REC_WORDS * j + w] = val;
  }
}

// ---- trie roots (include/zk_tx_roots.h) ------------------------------------------------------------------------------------------------------------
// DeriveSha (core/types/derive_sha.go:32-41) of many lists at once.  The values of list b stand at the global positions first[b] .. first[b+1] - 1 in the order of their
// keys; node holds 32 bytes a position.  k_trie_leaf writes every leaf's hash at its position, k_trie_level, once a key nibble depth and deepest first, replaces the hash
// at the head of every run that is a branch at that depth by the hash of the branch (or of the extension around it), k_trie_finish takes position 0 of every list.
// Every value has at least 32 bytes (the entries see to it), so every node is referenced by its hash (trie/hasher.go:176-178) and nothing is embedded.
constexpr uint64_t NIB40 = 0xFFFFFFFFFFull;
// rlp.Encode(uint(i)) (derive_sha.go:37) as nibbles (trie/encoding.go:65-75), left-aligned in 40 bits; *len: how many (2, 4, 6, 8 or 10)
__device__ __forceinline__ uint64_t trie_key(uint32_t i, uint32_t *len) {
  if (i < 0x80u) { *len = 2; return (uint64_t)(i ? i : 0x80u) << 32; }                              // 0 -> 80; 1 .. 7f -> the byte itself
  const uint32_t c = i < 0x100u ? 1u : i < 0x10000u ? 2u : i < 0x1000000u ? 3u : 4u;                // 80 + c, then the c bytes
  *len = 2 + 2 * c; return ((uint64_t)(0x80u + c) << 32) | ((uint64_t)i << (32 - 8 * c));
}
// the keys of a list of n values sorted as byte strings: the indices 1 .. min(n - 1, 127), then 0, then 128 .. n - 1
__device__ __forceinline__ uint32_t trie_index_at(uint32_t s, uint32_t n) { const uint32_t m = n - 1 < 127u ? n - 1 : 127u; return s < m ? s + 1 : s == m ? 0u : s; }
__device__ __forceinline__ uint32_t trie_pos_of(uint32_t i, uint32_t n) { const uint32_t m = n - 1 < 127u ? n - 1 : 127u; return i == 0 ? m : i < 128u ? i - 1 : i; }
__device__ __forceinline__ uint64_t trie_key_at(uint32_t s, uint32_t n) { uint32_t l; return trie_key(trie_index_at(s, n), &l); }
// two different keys: the nibbles they share (no key is a prefix of another, so they differ inside the shorter one); "they share d nibbles", d <= 10
__device__ __forceinline__ int trie_cpl(uint64_t a, uint64_t b) { return (__clzll((long long)(a ^ b)) - 24) >> 2; }
__device__ __forceinline__ bool trie_share(uint64_t a, uint64_t b, uint32_t d) { return ((a ^ b) >> (40u - 4u * d)) == 0; }
// the first position in (p, hi] whose key does not share d nibbles with kp, the key at p; positions p .. hi - 1 of a list of n.  The keys that share a prefix are
// consecutive, so a bisection finds it: at most 32 turns.
__device__ __forceinline__ uint32_t trie_run_end(uint32_t p, uint64_t kp, uint32_t d, uint32_t hi, uint32_t n) {
  uint32_t lo = p + 1;
#pragma unroll 1
  for (int it = 0; it < 32 && lo < hi; it++) { const uint32_t mid = lo + ((hi - lo) >> 1); if (trie_share(trie_key_at(mid, n), kp, d)) lo = mid + 1; else hi = mid; }
  return lo;
}
// `count` (<= 8) bytes of v behind the len bytes of (lo, hi); bytes beyond 16 are dropped (the entries refuse the lengths that would need them)
__device__ __forceinline__ void pre_append(uint64_t &lo, uint64_t &hi, uint32_t &len, uint64_t v, uint32_t count) {
  if (len < 8) { lo |= v << (8 * len); if (len + count > 8) hi |= v >> (8 * (8 - len)); }           // (len + count > 8 with count <= 8 means len > 0: the shift is below 64)
  else if (len < 16) hi |= v << (8 * (len - 8));
  len += count;
}
// hexToCompact (trie/encoding.go:37-51) of the top `count` nibbles of nibs (left-aligned in 40 bits), as an RLP string in the low bytes of the result: a single byte
// below 0x80 stands alone, otherwise 0x80 + length and the bytes; *len: its length, at most 7
__device__ __forceinline__ uint64_t trie_compact_str(uint64_t nibs, uint32_t count, uint32_t term, uint32_t *len) {
  const uint32_t odd = count & 1u, pairs = count >> 1; const uint64_t fb = ((uint64_t)((term << 1) | odd) << 4) | (odd ? nibs >> 36 : 0ull), rest = odd ? (nibs << 4) & NIB40 : nibs;
  if (pairs == 0) { *len = 1; return fb; }                                                          // 0x00 .. 0x3f: its own encoding
  uint64_t v = (0x81ull + pairs) | (fb << 8);
#pragma unroll
  for (uint32_t j = 0; j < 5; j++) if (j < pairs) v |= ((rest >> (32 - 8 * j)) & 0xFFull) << (8 * (2 + j));
  *len = 2 + pairs; return v;
}
// A lane a value: the leaf [hexToCompact(the key from max(lam_s, lam_s+1) + 1 on, terminator set), value] through one sponge — list header || key string || string
// header of the value in the prefix registers, then the value's bytes as they stand.  TXS: value i is transaction i of the walk that ran before; a malformed one marks
// its block and is not hashed, a 0xC0 recipient is read as 0x80 (k_tx_hash's substitution).  first: n_lists + 1 entries from 0 to n, not decreasing (the host has checked).
template <bool TXS>
__global__ void __launch_bounds__(TX_THREADS) k_trie_leaf(const uint8_t *__restrict__ vals, const uint64_t *__restrict__ off, uint32_t n, const uint32_t *__restrict__ first, uint32_t n_lists,
                                                           const uint32_t *__restrict__ D, uint32_t *__restrict__ blk_of, uint32_t *__restrict__ bad, uint64_t *__restrict__ node) {
  const uint32_t i = blockIdx.x * TX_THREADS + threadIdx.x; if (i >= n) return;
  uint32_t b = 0, hi = n_lists;                                                                     // the largest b with first[b] <= i: the one list with first[b] <= i < first[b+1]
#pragma unroll 1
  for (int it = 0; it < 32 && hi - b > 1; it++) { const uint32_t mid = b + ((hi - b) >> 1); if (first[mid] <= i) b = mid; else hi = mid; }
  const uint32_t f = first[b], nb = first[b + 1] - f, s = trie_pos_of(i - f, nb); const size_t g = (size_t)f + s;
  blk_of[g] = b;                                                                                    // (i -> g is a bijection inside a list)
  const uint64_t len = off[i + 1] - off[i]; uint64_t sub = ~0ull; bool skip = len > 0xFFFFFFFFull - 16;   // (this library's bound: the three headers of such a leaf would not fit the prefix)
  if constexpr (TXS) { const size_t nn = n; const uint32_t c0 = D[TD_C0 * nn + i];
    if (skip || (D[TD_META * nn + i] & 0xFFu) == TX_MALFORMED) { atomicOr(bad + b, 1u); skip = true; }   // the body does not decode: the block has no root
    else if (c0 != 0xFFFFFFFFu) sub = c0; }
  if (skip) {
#pragma unroll
    for (int k = 0; k < 4; k++) node[4 * g + k] = 0ull;
    return; }
  uint32_t L; const uint64_t key = trie_key(i - f, &L);
  const int lam_l = s ? trie_cpl(trie_key_at(s - 1, nb), key) : -1, lam_r = s + 1 < nb ? trie_cpl(key, trie_key_at(s + 1, nb)) : -1, lam = lam_l > lam_r ? lam_l : lam_r;
  const uint32_t from = (uint32_t)(lam + 1);                                                        // from <= L: two keys share fewer nibbles than the shorter one has
  uint32_t klen, c; const uint64_t kstr = trie_compact_str((key << (4 * from)) & NIB40, L - from, 1u, &klen);
  uint64_t vh = 0x80ull + len; uint32_t vhl = 1;                                                    // (a one-byte value below 0x80 would stand alone: no value here has under 32 bytes)
  if (len >= 56) { const uint64_t l = be_bytes(len, &c); vh = (0xB7ull + c) | (l << 8); vhl = 1 + c; }
  const uint64_t payload = klen + vhl + len; uint64_t lh = 0xC0ull + payload; uint32_t lhl = 1;
  if (payload >= 56) { const uint64_t l = be_bytes(payload, &c); lh = (0xF7ull + c) | (l << 8); lhl = 1 + c; }   // (c <= 5: the header fits eight bytes)
  ByteSource m; m.pre_lo = m.pre_hi = m.suf_lo = m.suf_hi = 0; m.pre_len = m.suf_len = 0; m.src = vals + (off[i] - off[0]); m.src_len = len; m.sub = sub;
  pre_append(m.pre_lo, m.pre_hi, m.pre_len, lh, lhl); pre_append(m.pre_lo, m.pre_hi, m.pre_len, kstr, klen); pre_append(m.pre_lo, m.pre_hi, m.pre_len, vh, vhl);
  uint32_t h[8]; sponge256(m, 0x01u, h);
#pragma unroll
  for (int k = 0; k < 4; k++) node[4 * g + k] = (uint64_t)h[2 * k] | ((uint64_t)h[2 * k + 1] << 32);
}
// A lane a position, acting only at the head of a run of keys that share d nibbles and is a branch at depth d: two members or more, first and last sharing exactly d.
// Its children are the heads of its at most sixteen (d + 1)-runs, found by bisection over positions; their hashes were written by the leaf launch or by a deeper
// level.  The 17-item list (trie/node.go EncodeRLP: 0xA0 and 32 bytes for a child, 0x80 for none and for the value slot) goes through the sponge a piece at a time —
// the state is indexed by constants only: the word in flight is XORed in through a chain of selects.  Where the larger adjacent prefix P at the run's two borders
// leaves a gap, d > P + 1, the branch is wrapped in the extension [hexToCompact(nibbles P + 1 .. d - 1), hash].  The result replaces the hash at the head: nothing
// outside the run reads or writes a position of the run in this launch.
__global__ void __launch_bounds__(TX_THREADS) k_trie_level(uint32_t n, uint32_t d, const uint32_t *__restrict__ first, const uint32_t *__restrict__ blk_of, uint64_t *node) {
  const uint32_t g = blockIdx.x * TX_THREADS + threadIdx.x; if (g >= n) return;
  const uint32_t b = blk_of[g], f = first[b], nb = first[b + 1] - f, s = g - f;
  uint32_t L; const uint64_t key = trie_key(trie_index_at(s, nb), &L); if (L <= d) return;
  int lam_l = -1;
  if (s) { const uint64_t kprev = trie_key_at(s - 1, nb); if (trie_share(kprev, key, d)) return; lam_l = trie_cpl(kprev, key); }   // not the head
  const uint32_t e = trie_run_end(s, key, d, nb, nb); if (e - s < 2) return;
  const uint64_t klast = trie_key_at(e - 1, nb); if (trie_share(klast, key, d + 1)) return;        // the branch lies deeper
  const int lam_r = e < nb ? trie_cpl(klast, trie_key_at(e, nb)) : -1, P = lam_l > lam_r ? lam_l : lam_r;
  uint32_t mask = 0, p = s;                                                                         // which of the sixteen children exist: nibble d of the head of each (d + 1)-run, ascending
#pragma unroll 1
  for (uint32_t c = 0; c < 16; c++) if (p < e) { const uint64_t kp = trie_key_at(p, nb); if (((kp >> (36u - 4u * d)) & 15u) == c) { mask |= 1u << c; p = trie_run_end(p, kp, d + 1, e, nb); } }
  const uint32_t cnt = (uint32_t)__popc(mask), payload = 33u * cnt + (17u - cnt), H = payload < 256u ? 2u : 3u;   // cnt >= 2: the payload has 81 .. 529 bytes
  const uint64_t hdr = payload < 256u ? (0xF8ull | ((uint64_t)payload << 8)) : (0xF9ull | ((uint64_t)(payload >> 8) << 8) | ((uint64_t)(payload & 0xFFu) << 16));
  uint64_t st[25];
#pragma unroll
  for (int k = 0; k < 25; k++) st[k] = 0;
  const uint32_t steps = H + 17u + 4u * cnt + 1u;                                                   // header bytes, seventeen item bytes, four words a child, the pad
  uint32_t wi = 0, fill = 0, hdr_i = 0, c = 0, sub = 0; uint64_t acc = 0, h0 = 0, h1 = 0, h2 = 0, h3 = 0; p = s;
#pragma unroll 1
  for (uint32_t step = 0; step < steps; step++) {
    const bool last = step + 1 == steps; uint64_t v; bool word = false;
    if (last) v = 0x01ull;
    else if (hdr_i < H) { v = (hdr >> (8 * hdr_i)) & 0xFFull; hdr_i++; }
    else if (sub == 0) {
      const bool present = c < 16 && ((mask >> c) & 1u); v = present ? 0xA0ull : 0x80ull;
      if (present && p < e) { const uint64_t *q = node + 4 * ((size_t)f + p); h0 = q[0]; h1 = q[1]; h2 = q[2]; h3 = q[3];   // (p < e always: the first pass met the same heads)
        p = trie_run_end(p, trie_key_at(p, nb), d + 1, e, nb); }
      if (present) sub = 1; else c++;
    }
    else { v = sub == 1 ? h0 : sub == 2 ? h1 : sub == 3 ? h2 : h3; word = true; if (++sub == 5) { sub = 0; c++; } }
    const uint64_t out = acc | (v << (8 * fill)); uint64_t carry = 0; bool full = true;               // fill < 8 at every turn
    if (word) carry = fill ? v >> (64 - 8 * fill) : 0ull;
    else { full = fill == 7 || last; fill = full ? 0 : fill + 1; }
    if (full) {
#pragma unroll
      for (int k = 0; k < 17; k++) st[k] ^= (uint32_t)k == wi ? out : 0ull;
      if (last) st[16] ^= 0x8000000000000000ull;
      if (++wi == 17 || last) { secp::keccak_f1600(st); wi = 0; }
      acc = carry;
    }
    else acc = out;
  }
  if ((int)d > P + 1) {                                                                             // trie.go:252-253: a short node leading up to the branch
    const uint32_t from = (uint32_t)(P + 1), cn = d - from; uint32_t klen;
    const uint64_t kstr = trie_compact_str((key << (4 * from)) & NIB40 & ~(NIB40 >> (4 * cn)), cn, 0u, &klen);   // cn <= 9, klen <= 6
    const uint32_t pl = klen + 2, sh = 8 * pl; const uint64_t pre = (0xC0ull + klen + 33u) | (kstr << 8) | (0xA0ull << (8 * (1 + klen))), b0 = st[0], b1 = st[1], b2 = st[2], b3 = st[3];
#pragma unroll
    for (int k = 0; k < 25; k++) st[k] = 0;
    if (pl == 8) { st[0] = pre; st[1] = b0; st[2] = b1; st[3] = b2; st[4] = b3; st[5] = 0x01ull; }
    else { st[0] = pre | (b0 << sh); st[1] = (b0 >> (64 - sh)) | (b1 << sh); st[2] = (b1 >> (64 - sh)) | (b2 << sh); st[3] = (b2 >> (64 - sh)) | (b3 << sh); st[4] = (b3 >> (64 - sh)) | (0x01ull << sh); }
    st[16] = 0x8000000000000000ull; secp::keccak_f1600(st);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) node[4 * (size_t)g + k] = st[k];
}
// A lane a list: emptyRoot (trie/trie.go:32) for no value, otherwise what stands at its position 0.  bad (the transaction forms): a list with a malformed
// transaction has no root — 32 zero bytes, defined = 0.
__global__ void __launch_bounds__(TX_THREADS) k_trie_finish(uint32_t n_lists, const uint32_t *__restrict__ first, const uint64_t *__restrict__ node, const uint32_t *__restrict__ bad,
                                                             uint64_t *__restrict__ roots, uint8_t *__restrict__ defined) {
  const uint32_t b = blockIdx.x * TX_THREADS + threadIdx.x; if (b >= n_lists) return;
  const uint32_t f = first[b], nb = first[b + 1] - f; const bool good = !bad || bad[b] == 0;
  uint64_t r[4] = {0xa655cc1b171fe856ull, 0x6ef8c092e64583ffull, 0xc0ad6c991be0485bull, 0x21b463e3b52f6201ull};
  if (nb) {
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = node[4 * (size_t)f + k]; }
#pragma unroll
  for (int k = 0; k < 4; k++) roots[4 * (size_t)b + k] = good ? r[k] : 0ull;
  if (defined) defined[b] = good ? 1 : 0;
}

// ---- headers from their bytes (include/zk_headers.h) -----------------------------------------------------------------------------------------------
// rlp.DecodeBytes into types.Header (core/types/block.go:72-90), Header.Hash() (:105-107), Clique's verifyHeader (consensus/clique/clique.go:269-326),
// verifyCascadingFields (:332-350), sigHash (:147-169) and ecrecover (:172-194) for n headers, one lane a header:
//   k_hdr_walk     the 17 headers of types.Header and every rule of the strict decoder, then verifyHeader's own rules; the status so far, the byte ranges of fields
//                  0 .. 11 and 13 .. 14 and Extra's content into a descriptor; R || S and the recovery byte from Extra's tail into the layout the recovery reads;
//                  the fixed-size outputs
//   k_hdr_hash     2n jobs, lanes 0 .. n-1 the seal hash (a fresh list header, fields 0 .. 11, a fresh string header, Extra less 65 bytes, fields 13 .. 14), lanes
//                  n .. 2n-1 the hash of the header's bytes as they stand
//   (the recovery's six launches on the seal hashes, homestead = false)
//   k_hdr_finish   the link and the timestamp rule against lane i - 1's hash, number and time (the caller's parent for lane 0); the recovery's verdict and the
//                  recovery-id rule; the first header whose status is not OK
enum { HDR_OK = 0, HDR_MALFORMED, HDR_FUTURE, HDR_CHECKPOINT_BENEFICIARY, HDR_VOTE, HDR_CHECKPOINT_VOTE, HDR_VANITY, HDR_SIGNATURE, HDR_EXTRA_SIGNERS, HDR_CHECKPOINT_SIGNERS,
       HDR_MIX_DIGEST, HDR_UNCLE_HASH, HDR_DIFFICULTY, HDR_ANCESTOR, HDR_TIMESTAMP, HDR_SEAL, HDR_SEAL_UNDECIDED };
static_assert(HDR_MALFORMED == ZK_HDR_MALFORMED && HDR_DIFFICULTY == ZK_HDR_DIFFICULTY && HDR_SEAL_UNDECIDED == ZK_HDR_SEAL_UNDECIDED, "zk_headers.h names these");
// the descriptor of a lane, in words; word k of lane i lies at H[k * n + i]: the status so far | where field 0 starts | where field 11 ends (Extra's own header starts) |
// where field 13 starts | where field 14 ends | Extra's content
constexpr int HD_META = 0, HD_A = 1, HD_B = 2, HD_C = 3, HD_E = 4, HD_XB = 5, HD_XS = 6, HD_WORDS = 7;
enum { HK_HASH, HK_ADDR, HK_BLOOM, HK_NONCE, HK_BIG, HK_U64, HK_BYTES, HK_HASHES };
constexpr int HDR_FIELDS = 17, HF_UNCLE = 1, HF_COINBASE = 2, HF_TXHASH = 4, HF_DIFFICULTY = 7, HF_NUMBER = 8, HF_TIME = 11, HF_EXTRA = 12, HF_MIX = 13, HF_NONCE = 14, HF_RTCMT = 15, HF_CMT = 16;
constexpr int HKINDS[HDR_FIELDS] = {HK_HASH, HK_HASH, HK_ADDR, HK_HASH, HK_HASH, HK_HASH, HK_BLOOM, HK_BIG, HK_BIG, HK_U64, HK_U64, HK_BIG, HK_BYTES, HK_HASH, HK_NONCE, HK_HASH, HK_HASHES};
constexpr uint64_t HK_ALL = fk_pack(HKINDS, 0, HDR_FIELDS);                                        // block.go:72-90, three bits a field
constexpr uint32_t HDR_VANITY_BYTES = 32, HDR_SEAL_BYTES = 65;                                     // clique.go:59-60
constexpr uint32_t P_MINUS_N[8] = {0x2FC9BAEEu, 0x402DA172u, 0x50B75FC4u, 0x45512319u, 0x00000001u, 0, 0, 0};   // recovery/main_impl.h:105: secp256k1_ecdsa_const_p_minus_order
// the per-header outputs of zk_headers.h on the device (HeadersLayout's download)
struct HdrOut { uint32_t *hash, *sealhash, *signer, *coinbase, *tx_root, *rtcmt; uint64_t *number, *time; uint32_t *extra_beg, *extra_size, *cmt_beg, *cmt_count; uint8_t *difficulty, *vote, *status; };
struct HdrParent { uint32_t have, hash[8]; uint64_t number, time; };                              // hash: bytes 4k .. 4k+3 as they lie in memory
// the OR and the AND of count bytes at beg; count is a constant at every call
__device__ __forceinline__ uint32_t hdr_or(const uint8_t *__restrict__ t, uint32_t beg, uint32_t count) { uint32_t v = 0;
#pragma unroll 4
  for (uint32_t k = 0; k < count; k++) v |= t[beg + k];
  return v; }
__device__ __forceinline__ uint32_t hdr_and(const uint8_t *__restrict__ t, uint32_t beg, uint32_t count) { uint32_t v = 0xFFu;
#pragma unroll 4
  for (uint32_t k = 0; k < count; k++) v &= t[beg + k];
  return v; }
// four bytes as they lie in memory; `want` false: zero, and nothing is read
__device__ __forceinline__ uint32_t hdr_le32(const uint8_t *__restrict__ t, uint32_t beg, bool want) {
  return want ? (uint32_t)t[beg] | ((uint32_t)t[beg + 1] << 8) | ((uint32_t)t[beg + 2] << 16) | ((uint32_t)t[beg + 3] << 24) : 0u; }
__global__ void __launch_bounds__(TX_THREADS) k_hdr_walk(const uint8_t *__restrict__ hdrs, const uint64_t *__restrict__ off, uint32_t n, uint64_t epoch, uint64_t now, uint32_t *__restrict__ H,
                                                          uint8_t *__restrict__ rs, uint8_t *__restrict__ vout, HdrOut o, uint32_t *__restrict__ first_bad) {
  const uint32_t i = blockIdx.x * TX_THREADS + threadIdx.x; if (i >= n) return;
  if (i == 0) first_bad[0] = n;                                                                    // k_hdr_finish's atomicMin starts from "none"
  const uint64_t base = off[0], o0 = off[i] - base, len64 = off[i + 1] - off[i]; const uint8_t *t = hdrs + o0;   // (the host has checked that off does not decrease)
  bool bad = len64 == 0 || len64 > 0xFFFFFFFFull; const uint32_t len = (uint32_t)len64;            // (this library's bound)
  uint32_t pos = 0, lim = 0, a = 0, b = 0, c = 0, e = 0, xb = 0, xs = 0, uncle = 0, coin = 0, txr = 0, dbeg = 0, dsize = 0, nbeg = 0, nsize = 0, tbeg = 0, tsize = 0, mix = 0, nonce = 0, rt = 0,
           cb = 0, cs = 0;
  if (!bad) { const Head h = tx_head(t, 0, len);                                                    // the outer item: a list (decode.go:438, :762) that ends where the input ends (:142-144)
    bad = h.bad || h.kind != K_LIST || h.beg + h.size != len; pos = h.beg; lim = len; a = pos; }
#pragma unroll 1
  for (int f = 0; f < HDR_FIELDS && !bad; f++) {
    if (pos == lim) { bad = true; break; }                                                          // :443-444: too few elements
    const Head h = tx_head(t, pos, lim); if (h.bad) { bad = true; break; }
    const uint32_t kind = (uint32_t)((HK_ALL >> (3 * f)) & 7u); pos = h.beg + h.size;
    switch (kind) {
      case HK_HASH: bad = h.kind != K_STR || h.size != 32; break;                                   // decodeByteArray :395-430: a lone byte and a list are refused
      case HK_ADDR: bad = h.kind != K_STR || h.size != 20; break;
      case HK_BLOOM: bad = h.kind != K_STR || h.size != 256; break;
      case HK_NONCE: bad = h.kind != K_STR || h.size != 8; break;
      case HK_BIG: bad = h.kind == K_LIST || (h.size && t[h.beg] == 0); break;                      // :271-287
      case HK_U64: bad = !tx_uint_ok(t, h, 8); break;                                               // :703-734
      case HK_BYTES: bad = h.kind == K_LIST; break;                                                 // :386-393
      default:                                                                                      // []*common.Hash: :323-336, makePtrDecoder :456-478, then :395-430
        bad = h.kind != K_LIST;
        if (!bad) { uint32_t p = h.beg; const uint32_t end = h.beg + h.size;
#pragma unroll 1
          while (p < end) { const Head u = tx_head(t, p, end); if (u.bad || u.kind != K_STR || u.size != 32) { bad = true; break; } p = u.beg + u.size; } }   // (p grows by 33 a turn)
        break;
    }
    if (f == HF_UNCLE) uncle = h.beg;
    if (f == HF_COINBASE) coin = h.beg;
    if (f == HF_TXHASH) txr = h.beg;
    if (f == HF_DIFFICULTY) { dbeg = h.beg; dsize = h.size; }
    if (f == HF_NUMBER) { nbeg = h.beg; nsize = h.size; if (nsize > 8) bad = true; }                // (this library's bound: the reference reads Number.Uint64())
    if (f == HF_TIME) { tbeg = h.beg; tsize = h.size; b = pos; }
    if (f == HF_EXTRA) { xb = h.beg; xs = h.size; c = pos; }
    if (f == HF_MIX) mix = h.beg;
    if (f == HF_NONCE) { nonce = h.beg; e = pos; }
    if (f == HF_RTCMT) rt = h.beg;
    if (f == HF_CMT) { cb = h.beg; cs = h.size; }
  }
  if (!bad && pos != lim) bad = true;                                                               // :449, :778: too many elements
  const bool good = !bad; uint64_t number = 0, time = 0; uint32_t status = HDR_MALFORMED, diff = 0, vote = 0;
  if (good) {
    const uint32_t tk = tsize < 8u ? tsize : 8u, tfrom = tbeg + tsize - tk;                         // Time.Uint64(): the low 64 bits
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) { if (k < nsize) number = (number << 8) | t[nbeg + k]; if (k < tk) time = (time << 8) | t[tfrom + k]; }
    diff = dsize == 0 ? 0u : dsize == 1 ? (uint32_t)t[dbeg] : 255u;                                 // (1 and 2 are themselves; whatever is wider is neither)
    const bool checkpoint = number % epoch == 0;                                                    // clique.go:280
    const uint32_t nonce_or = hdr_or(t, nonce, 8), nonce_and = hdr_and(t, nonce, 8); vote = nonce_and == 0xFFu ? 1u : 0u;
    bool uncle_ok = true;                                                                           // :65: Keccak256(c0)
    constexpr uint32_t UNCLE[8] = {0xe84dcc1du, 0x7a5dc7deu, 0x67b585abu, 0x1ad4ccb6u, 0x1b4512d3u, 0x13748a94u, 0xfd42a1f0u, 0x4793d440u};
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) uncle_ok = uncle_ok && hdr_le32(t, uncle + 4 * k, true) == UNCLE[k];
    status = (tsize > 8 || time > now) ? HDR_FUTURE                                                 // :276
           : (checkpoint && hdr_or(t, coin, 20)) ? HDR_CHECKPOINT_BENEFICIARY                       // :281
           : (nonce_and != 0xFFu && nonce_or != 0) ? HDR_VOTE                                       // :285
           : (checkpoint && nonce_or != 0) ? HDR_CHECKPOINT_VOTE                                    // :288
           : xs < HDR_VANITY_BYTES ? HDR_VANITY                                                     // :292
           : xs < HDR_VANITY_BYTES + HDR_SEAL_BYTES ? HDR_SIGNATURE                                 // :295
           : (!checkpoint && xs != HDR_VANITY_BYTES + HDR_SEAL_BYTES) ? HDR_EXTRA_SIGNERS           // :300
           : (checkpoint && (xs - HDR_VANITY_BYTES - HDR_SEAL_BYTES) % 20u) ? HDR_CHECKPOINT_SIGNERS   // :303
           : hdr_or(t, mix, 32) ? HDR_MIX_DIGEST                                                    // :307
           : !uncle_ok ? HDR_UNCLE_HASH                                                             // :311
           : (number > 0 && diff != 1 && diff != 2) ? HDR_DIFFICULTY : HDR_OK;                      // :315-318
  }
  const size_t nn = n;
  H[HD_META * nn + i] = status; H[HD_A * nn + i] = a; H[HD_B * nn + i] = b; H[HD_C * nn + i] = c; H[HD_E * nn + i] = e; H[HD_XB * nn + i] = xb; H[HD_XS * nn + i] = xs;
  const bool sealed = good && xs >= HDR_SEAL_BYTES; const uint32_t tail = sealed ? xb + xs - HDR_SEAL_BYTES : 0u;   // R || S || the recovery byte: Extra's last 65 (clique.go:182)
#pragma unroll 4
  for (uint32_t k = 0; k < 64; k++) rs[64 * (size_t)i + k] = sealed ? t[tail + k] : (uint8_t)0;
  vout[i] = sealed ? t[tail + 64] : (uint8_t)0;
#pragma unroll
  for (uint32_t k = 0; k < 8; k++) { o.tx_root[8 * (size_t)i + k] = hdr_le32(t, txr + 4 * k, good); o.rtcmt[8 * (size_t)i + k] = hdr_le32(t, rt + 4 * k, good); }
#pragma unroll
  for (uint32_t k = 0; k < 5; k++) o.coinbase[5 * (size_t)i + k] = hdr_le32(t, coin + 4 * k, good);
  o.number[i] = number; o.time[i] = time; o.difficulty[i] = (uint8_t)diff; o.vote[i] = (uint8_t)vote;
  o.extra_beg[i] = good ? xb : 0u; o.extra_size[i] = good ? xs : 0u; o.cmt_beg[i] = good ? cb : 0u; o.cmt_count[i] = good ? cs / 33u : 0u;
}
// The seal hash's message: pre_len bytes of pre, a[0 .. a_len), mid_len bytes of mid, x[0 .. x_len), c[0 .. c_len).  Byte k of pre and mid is bits 8k .. 8k+7.  The
// whole header's hash is the same source with a alone.  (ByteSource has one range; this one is its own type, so that the kernels on ByteSource stay what they are.)
struct HdrSource { uint64_t pre, mid; uint32_t pre_len, mid_len; const uint8_t *a, *x, *c; uint64_t a_len, x_len, c_len; };
__device__ __forceinline__ uint64_t bs_total(const HdrSource &m) { return (uint64_t)m.pre_len + m.a_len + m.mid_len + m.x_len + m.c_len; }
__device__ __forceinline__ uint64_t bs_byte(const HdrSource &m, uint64_t j, uint32_t pad) {
  if (j < m.pre_len) return (m.pre >> (8 * j)) & 0xFFull;
  uint64_t q = j - m.pre_len;
  if (q < m.a_len) return (uint64_t)m.a[q];
  q -= m.a_len;
  if (q < m.mid_len) return (m.mid >> (8 * q)) & 0xFFull;
  q -= m.mid_len;
  if (q < m.x_len) return (uint64_t)m.x[q];
  q -= m.x_len;
  if (q < m.c_len) return (uint64_t)m.c[q];
  return q == m.c_len ? (uint64_t)pad : 0ull;
}
// bytes j .. j+7 as a little-endian word: one 8-byte read where all eight lie in one of the three ranges
__device__ __forceinline__ uint64_t bs_word(const HdrSource &m, uint64_t j, uint32_t pad) {
  if (j >= m.pre_len) {
    const uint64_t q = j - m.pre_len, xa = m.a_len + m.mid_len, ca = xa + m.x_len; uint64_t w;
    if (q + 8 <= m.a_len) { __builtin_memcpy(&w, m.a + q, 8); return w; }
    if (q >= xa && q + 8 <= ca) { __builtin_memcpy(&w, m.x + (q - xa), 8); return w; }
    if (q >= ca && q + 8 <= ca + m.c_len) { __builtin_memcpy(&w, m.c + (q - ca), 8); return w; }
  }
  uint64_t w = 0;
#pragma unroll 1
  for (uint32_t k = 0; k < 8; k++) w |= bs_byte(m, j + k, pad) << (8 * k);
  return w;
}
__global__ void __launch_bounds__(TX_THREADS) k_hdr_hash(const uint8_t *__restrict__ hdrs, const uint64_t *__restrict__ off, uint32_t n, const uint32_t *__restrict__ H, uint32_t *__restrict__ sealhash,
                                                          uint32_t *__restrict__ hash) {
  const uint32_t j = blockIdx.x * TX_THREADS + threadIdx.x; if (j >= 2 * n) return;
  const bool whole = j >= n; const uint32_t i = whole ? j - n : j; const size_t nn = n; uint32_t *out = (whole ? hash : sealhash) + 8 * (size_t)i;
  const uint32_t status = H[HD_META * nn + i], xs = H[HD_XS * nn + i];
  if (status == HDR_MALFORMED || (!whole && xs < HDR_SEAL_BYTES)) {                                 // sigHash panics below 65 bytes (clique.go:163); ecrecover asks first (:179)
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = 0u;
    return; }
  const uint64_t o0 = off[i] - off[0]; const uint8_t *t = hdrs + o0;
  HdrSource m; m.pre = m.mid = 0; m.pre_len = m.mid_len = 0; m.a = m.x = m.c = t; m.a_len = m.x_len = m.c_len = 0;
  if (whole) m.a_len = off[i + 1] - off[i];                                                         // Header.Hash(): the strict decoder makes the re-encoding the input
  else {                                                                                           // sigHash (clique.go:150-166): the upstream 15 fields, Extra less its last 65 bytes
    const uint32_t a = H[HD_A * nn + i], b = H[HD_B * nn + i], c = H[HD_C * nn + i], e = H[HD_E * nn + i], xb = H[HD_XB * nn + i], rest = xs - HDR_SEAL_BYTES; uint32_t cnt;
    m.a = t + a; m.a_len = b - a; m.x = t + xb; m.x_len = rest; m.c = t + c; m.c_len = e - c;
    if (rest == 0) { m.mid = 0x80ull; m.mid_len = 1; }
    else if (rest == 1 && t[xb] < 0x80u) { }                                                        // the byte is its own encoding
    else if (rest < 56) { m.mid = 0x80ull + rest; m.mid_len = 1; }
    else { const uint64_t l = be_bytes(rest, &cnt); m.mid = (0xB7ull + cnt) | (l << 8); m.mid_len = 1 + cnt; }   // cnt <= 4
    const uint64_t payload = m.a_len + m.mid_len + m.x_len + m.c_len;                               // above 55 (the bloom alone), below the header's length
    const uint64_t l = be_bytes(payload, &cnt); m.pre = (0xF7ull + cnt) | (l << 8); m.pre_len = 1 + cnt;   // cnt <= 4
  }
  uint32_t h[8]; sponge256(m, 0x01u, h);
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = h[k];
}
__global__ void __launch_bounds__(TX_THREADS) k_hdr_finish(const uint8_t *__restrict__ hdrs, const uint64_t *__restrict__ off, uint32_t n, uint64_t period, HdrParent parent, const uint32_t *__restrict__ H,
                                                            const uint32_t *__restrict__ rs, const uint8_t *__restrict__ v, const uint8_t *__restrict__ ok, const uint32_t *__restrict__ recovered,
                                                            HdrOut o, const uint32_t *__restrict__ sp_head, uint32_t *__restrict__ head) {
  const uint32_t i = blockIdx.x * TX_THREADS + threadIdx.x; if (i >= n) return;
  if (i == 0) {                                                                                     // the recovery's four counters ride in the one download
#pragma unroll
    for (int k = 0; k < 4; k++) head[BH_WORDS + k] = sp_head[k]; }
  const size_t nn = n; uint32_t status = H[HD_META * nn + i], f[5] = {0, 0, 0, 0, 0}; const uint64_t number = o.number[i];
  if (status == HDR_OK && number > 0) {                                                             // clique.go:334-336: the genesis is the always valid dead end
    const uint8_t *t = hdrs + (off[i] - off[0]); const uint32_t ph = H[HD_A * nn + i] + 1;          // ParentHash's 32 bytes: field 0, behind its one header byte
    bool have = i ? H[HD_META * nn + (i - 1)] != HDR_MALFORMED : parent.have != 0;                  // :340-343: headers[:i]'s last, or what the caller found; a malformed one is no header
    const uint64_t pnumber = i ? o.number[i - 1] : parent.number, ptime = i ? o.time[i - 1] : parent.time;
    bool link = have && pnumber == number - 1;                                                      // :345
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) link = link && hdr_le32(t, ph + 4 * k, true) == (i ? o.hash[8 * (size_t)(i - 1) + k] : parent.hash[k]);
    if (!link) status = HDR_ANCESTOR;
    else if (ptime + period > o.time[i]) status = HDR_TIMESTAMP;                                    // :348: uint64, the wrap included (FUTURE has refused a wider Time)
    else {                                                                                          // crypto.Ecrecover(sigHash, Extra[len - 65:]) (:185)
      const secp::U256 r = secp::load_be(rs + 16 * (size_t)i), s = secp::load_be(rs + 16 * (size_t)i + 8); const uint32_t vb = v[i];
      if (vb >= 4 || secp::u256_is_zero(r) || secp::u256_is_zero(s) || secp::u256_geq(r, secp::FnP::MOD) || secp::u256_geq(s, secp::FnP::MOD)) status = HDR_SEAL;   // secp256.go:175; main_impl.h:48-51, :96-98
      else if (vb & 2u) status = secp::u256_geq(r, P_MINUS_N) ? HDR_SEAL : HDR_SEAL_UNDECIDED;      // main_impl.h:104-107; x = r + N is not taken here: the caller decides
      else if (ok[i]) {
#pragma unroll
        for (int k = 0; k < 5; k++) f[k] = recovered[5 * (size_t)i + k]; }
      else status = HDR_SEAL;                                                                       // main_impl.h:110, :120
    }
  }
#pragma unroll
  for (int k = 0; k < 5; k++) o.signer[5 * (size_t)i + k] = f[k];
  o.status[i] = (uint8_t)status;
  if (status != HDR_OK) atomicMin(head + BH_FIRST_BAD, i);
}

// ---- block bodies from their bytes (include/zk_raw_bodies.h) ---------------------------------------------------------------------------------------
// rlp.DecodeBytes(body, &types.Body{}) (core/types/block.go:143-146: Transactions, Uncles) as far as the body's structure goes, for n_blocks bodies, and their
// transactions packed end to end where every kernel above expects them:
//   k_split_count    a lane a body: the outer list, the two lists in it, every element head of the first; the status, the element count, where item 0's payload lies
//   k_split_scan     one workgroup: the exclusive scans of the counts and of the payload sizes over the blocks; n, the packed total, the largest block, the first
//                    body that is not OK
//   k_split_offsets  a lane a body: the walk again; off in packed coordinates, tx_beg and tx_size in the caller's, first
//   k_split_pack     a lane an aligned 8-byte word of the packed bytes: the payloads of the OK bodies end to end
enum { BODY_OK = 0, BODY_MALFORMED = 1, BODY_UNCLES = 2 };
static_assert(BODY_OK == ZK_BODY_OK && BODY_MALFORMED == ZK_BODY_MALFORMED && BODY_UNCLES == ZK_BODY_UNCLES, "zk_raw_bodies.h names these");
enum { SH_N = 0, SH_TOTAL = 2, SH_LARGEST = 4, SH_K = 5, SH_WORDS = 8 };                           // the split's head; n and the total are 64-bit values
constexpr int SPLIT_SCAN_THREADS = 256;
// The struct decoder (decode.go:432-454) on types.Body: the outer item a list (:438, :762) that ends where the input ends (:142-144); "too few elements" (:443-444)
// where a field finds the list at its end, "input list has too many elements" (:449, :778) where the list goes on behind the last; both fields are slices, which want
// a list (decodeListSlice :323-326).  Every element head of item 0 is read by Stream.Kind (:902-960) before anything of the element is decoded, so a head that is not
// canonical or overruns the list refuses the body whatever the element is.  pay_beg, pay_size: item 0's payload, relative to the body's first byte; count: its elements.
// All three are zero unless the status is OK.  Every turn of the walk moves p on by at least one byte.
__global__ void __launch_bounds__(TX_THREADS) k_split_count(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ body_off, uint32_t nb, uint8_t *__restrict__ status,
                                                             uint32_t *__restrict__ count, uint32_t *__restrict__ pay_beg, uint32_t *__restrict__ pay_size) {
  const uint32_t b = blockIdx.x * TX_THREADS + threadIdx.x; if (b >= nb) return;
  const uint64_t o0 = body_off[b] - body_off[0], len64 = body_off[b + 1] - body_off[b]; const uint8_t *t = raw + o0;   // (the host has checked that body_off does not decrease)
  bool bad = len64 == 0 || len64 > 0xFFFFFFFFull; const uint32_t len = (uint32_t)len64;            // an empty input: io.ErrUnexpectedEOF (:142, :910); the length: this library's bound
  uint32_t beg = 0, size = 0, usize = 0, cnt = 0, pos = 0;
  if (!bad) { const Head o = tx_head(t, 0, len); bad = o.bad || o.kind != K_LIST || o.beg + o.size != len; pos = o.beg; }
  if (!bad) { const Head a = tx_head(t, pos, len);                                                  // (pos == len: tx_head refuses, "too few elements")
    bad = a.bad || a.kind != K_LIST; beg = a.beg; size = a.size; pos = a.beg + a.size; }
  if (!bad) { const Head u = tx_head(t, pos, len); bad = u.bad || u.kind != K_LIST || u.beg + u.size != len; usize = u.size; }   // too few; not a list; too many
  uint32_t p = beg; const uint32_t e = beg + size;
#pragma unroll 1
  while (!bad && p < e) { const Head h = tx_head(t, p, e); if (h.bad) bad = true; else { p = h.beg + h.size; cnt++; } }
  const uint32_t st = bad ? BODY_MALFORMED : usize ? BODY_UNCLES : BODY_OK; const bool ok = st == BODY_OK;   // clique.go:450-455 with block_validator.go:67: no uncle
  status[b] = (uint8_t)st; count[b] = ok ? cnt : 0u; pay_beg[b] = ok ? beg : 0u; pay_size[b] = ok ? size : 0u;
}
// first[b] = the transactions before body b, base[b] = the packed bytes before it, both with an entry at nb; the head.  One workgroup; cdiv(nb, 256) tiles, a carry
// between them; the loop's bound is the same for every lane, and every lane reaches every barrier.  nb > 0.
__global__ void __launch_bounds__(SPLIT_SCAN_THREADS) k_split_scan(const uint8_t *__restrict__ status, const uint32_t *__restrict__ count, const uint32_t *__restrict__ pay_size, uint32_t nb,
                                                                    uint32_t *__restrict__ first, uint64_t *__restrict__ base, uint32_t *__restrict__ head) {
  __shared__ uint64_t sh[SPLIT_SCAN_THREADS]; __shared__ uint32_t sh_max, sh_k;
  if (threadIdx.x == 0) { sh_max = 0; sh_k = nb; }                                                  // (seen by all behind the first scan's barriers)
  uint64_t carry_n = 0, carry_z = 0; uint32_t largest = 0, k = nb;
#pragma unroll 1
  for (uint32_t tile = 0; tile < nb; tile += SPLIT_SCAN_THREADS) {
    const uint32_t b = tile + threadIdx.x; const bool in = b < nb; const uint64_t v = in ? count[b] : 0u, z = in ? pay_size[b] : 0u;
    const uint64_t incl_n = block_scan_inclusive<SPLIT_SCAN_THREADS>(v, sh), tile_n = sh[SPLIT_SCAN_THREADS - 1]; __syncthreads();   // (sh is written again)
    const uint64_t incl_z = block_scan_inclusive<SPLIT_SCAN_THREADS>(z, sh), tile_z = sh[SPLIT_SCAN_THREADS - 1]; __syncthreads();
    if (in) { const uint64_t f = carry_n + incl_n - v; first[b] = f > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)f; base[b] = carry_z + incl_z - z;   // (beyond 2^30 - 1 the host stops)
      if ((uint32_t)v > largest) largest = (uint32_t)v;
      if (status[b] != BODY_OK && b < k) k = b; }
    carry_n += tile_n; carry_z += tile_z;
  }
  atomicMax(&sh_max, largest); atomicMin(&sh_k, k); __syncthreads();
  if (threadIdx.x == 0) { first[nb] = carry_n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)carry_n; base[nb] = carry_z;
    head[SH_N] = (uint32_t)carry_n; head[SH_N + 1] = (uint32_t)(carry_n >> 32); head[SH_TOTAL] = (uint32_t)carry_z; head[SH_TOTAL + 1] = (uint32_t)(carry_z >> 32);
    head[SH_LARGEST] = sh_max; head[SH_K] = sh_k; head[6] = 0; head[7] = 0; }
}
// The walk of k_split_count again over an OK body (its heads have all been accepted): element j of body b is transaction i = first[b] + j; off[i]: where it starts in
// the packed bytes; tx_beg[i], tx_size[i]: where it lies in the caller's buffer.  off[n] and dfirst[nb] are lane 0's, whatever body 0 is; dfirst may be null.
// i < n is compared before anything is written: n is what the host read from the scan's head.
__global__ void __launch_bounds__(TX_THREADS) k_split_offsets(const uint8_t *__restrict__ raw, const uint64_t *__restrict__ body_off, uint32_t nb, const uint8_t *__restrict__ status,
                                                               const uint32_t *__restrict__ pay_beg, const uint32_t *__restrict__ pay_size, const uint32_t *__restrict__ first,
                                                               const uint64_t *__restrict__ base, uint32_t n, uint64_t *__restrict__ off, uint32_t *__restrict__ dfirst,
                                                               uint64_t *__restrict__ tx_beg, uint32_t *__restrict__ tx_size) {
  const uint32_t b = blockIdx.x * TX_THREADS + threadIdx.x; if (b >= nb) return;
  if (b == 0) { off[n] = base[nb]; if (dfirst) dfirst[nb] = n; }
  if (dfirst) dfirst[b] = first[b];
  if (status[b] != BODY_OK) return;
  const uint64_t at = body_off[b], pk = base[b]; const uint8_t *t = raw + (at - body_off[0]); const uint32_t beg = pay_beg[b], e = beg + pay_size[b]; uint32_t p = beg, i = first[b];
#pragma unroll 1
  while (p < e && i < n) { const Head h = tx_head(t, p, e); if (h.bad) break;                        // (never: k_split_count accepted this head)
    const uint32_t next = h.beg + h.size; off[i] = pk + (p - beg); tx_beg[i] = at + p; tx_size[i] = next - p; p = next; i++; }
}
// Packed word w holds the packed bytes 8w .. 8w + 7: byte d of the packed stream is byte d - base[b] of body b's item-0 payload, b the one body with base[b] <= d <
// base[b+1], found by bisection (at most 32 turns; bodies without a payload share their base with the next and are never found).  A word takes at most eight pieces,
// each from one or two aligned source words and a shift (raw starts at an aligned address and is padded to 8 bytes; the second word is read only where a wanted byte
// lies in it, so the bytes shifted out lie inside the padded upload).  Bytes at and beyond the total are zero.  words = cdiv(total, 8).
__global__ void __launch_bounds__(TX_THREADS) k_split_pack(const uint64_t *__restrict__ raw, const uint64_t *__restrict__ body_off, uint32_t nb, const uint32_t *__restrict__ pay_beg,
                                                            const uint64_t *__restrict__ base, uint64_t total, uint64_t words, uint64_t *__restrict__ dst) {
  const uint64_t w = (uint64_t)blockIdx.x * TX_THREADS + threadIdx.x; if (w >= words) return;
  uint64_t d = 8 * w, val = 0; uint32_t filled = 0;
#pragma unroll 1
  for (int piece = 0; piece < 8 && filled < 8 && d < total; piece++) {
    uint32_t b = 0, hi = nb;                                                                        // the largest b < nb with base[b] <= d; base[b+1] > d follows, base[nb] = total
#pragma unroll 1
    for (int it = 0; it < 32 && hi - b > 1; it++) { const uint32_t mid = b + ((hi - b) >> 1); if (base[mid] <= d) b = mid; else hi = mid; }
    const uint64_t left = base[b + 1] - d, s = (body_off[b] - body_off[0]) + pay_beg[b] + (d - base[b]); const uint32_t take = left < 8u - filled ? (uint32_t)left : 8u - filled;   // 1 .. 8
    const uint64_t k = s >> 3; const uint32_t r = (uint32_t)(s & 7u), shift = 8u * r; uint64_t v = raw[k] >> shift;
    if (r + take > 8u) v |= raw[k + 1] << (64u - shift);                                           // (r > 0 here: the shift is below 64)
    if (take < 8u) v &= (1ull << (8u * take)) - 1ull;
    val |= v << (8u * filled); filled += take; d += take;
  }
  dst[w] = val;
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------------
namespace {
struct Txs : PinnedStage {                           // one a process, every member under the device mutex
  DevBuf<uint32_t> io;
  DevBuf<uint32_t> raw; PinnedStage raw_pin;          // the raw bodies' own buffer and pinned buffer (SplitLayout): live while the workspace is laid out and filled from them
  static void grow(DevBuf<uint32_t> &b, size_t words) { if (b.size() >= words) return; const size_t want = std::max(words, 2 * b.size()); b = DevBuf<uint32_t>(); b = DevBuf<uint32_t>(want); }   // (a failed growth leaves no workspace)
  void grow(size_t words) { grow(io, words); }
};
Txs &txs_state() { static Txs *t = new Txs; return *t; }   // (never destroyed: the runtime may be gone when statics are)
static_assert(TXL_D_WORDS == TD_WORDS && TXL_E_WORDS == TE_WORDS && TXL_HEAD_WORDS == BH_WORDS && TXL_REC_WORDS == REC_WORDS && TXL_THREADS == TX_THREADS, "txs_layout.hpp carves for these kernels");
static_assert(TXL_H_WORDS == HD_WORDS, "txs_layout.hpp carves for k_hdr_walk");
// pinned, on a layout of txs_layout.hpp: the upload's three pieces — the bytes off[0] .. off[n) of the caller's buffer, padded to 8, off itself, the n_first entries of
// first (checked by the caller: 0 .. n, so int and uint32_t agree), padded to 8; returns where the download will land
uint8_t *stage(Txs &d, const TxsUpload &L, const uint8_t *bytes, const uint64_t *off, size_t n, const int *first) {
  d.pinned(L.pin_bytes); uint8_t *const back = d.pin + L.up, *const f = d.pin + 4 * L.first;
  if (L.total) memcpy(d.pin, bytes + off[0], L.total);
  memset(d.pin + L.total, 0, L.total8 - L.total); memcpy(d.pin + L.total8, off, 8 * (n + 1));
  if (L.n_first) { memcpy(f, first, 4 * L.n_first); memset(f + 4 * L.n_first, 0, back - (f + 4 * L.n_first)); }
  return back;
}
// The prologue of every call here: the upload staged, the workspace grown to the layout and its slack, the upload queued on s.  dev(x): region x on the device;
// host(x): where region x lies once L.down .. L.down_end has come down to `back`.
struct Staged {
  const TxsUpload &L; uint32_t *p; uint8_t *back; const uint8_t *dtx; const uint64_t *doff; const uint32_t *dfirst;
  SyncAtExit sync;                                                                                  // (also where staging or growing fails: the stream is idle then)
  Staged(const TxsUpload &L, const uint8_t *bytes, const uint64_t *off, size_t n, const int *first, hipStream_t s) : L(L) {
    Txs &d = txs_state(); back = stage(d, L, bytes, off, n, first);
    d.grow(L.end + TXL_SLACK); p = d.io.get(); if (!p) throw GpuError("txs: no workspace");
    dtx = (const uint8_t *)p; doff = (const uint64_t *)(p + L.off); dfirst = p + L.first;
    HIP_CHECK(hipMemcpyAsync(p, d.pin, L.up, hipMemcpyHostToDevice, s));
  }
  // the same without an upload: the split's launches fill the upload's place from the raw bodies (nothing of the workspace is live when it grows)
  explicit Staged(const TxsUpload &L) : L(L) {
    Txs &d = txs_state(); d.pinned(L.pin_bytes); back = d.pin + L.up;
    d.grow(L.end + TXL_SLACK); p = d.io.get(); if (!p) throw GpuError("txs: no workspace");
    dtx = (const uint8_t *)p; doff = (const uint64_t *)(p + L.off); dfirst = p + L.first;
  }
  uint32_t *dev(size_t x) const { return p + x; }
  uint8_t *host(size_t x) const { return back + 4 * (x - L.down); }
};
// The launches behind the upload: a leaf a value, a level for every nibble depth of the longest key — it depends on the largest list alone —, a root a list.  D: the
// walk's descriptor (the transaction forms: bad and defined are written) or null.
void trie_queue(const Staged &g, size_t n, size_t n_lists, size_t largest, const uint32_t *D, const TrieWords &w, hipStream_t s) {
  const dim3 block(TX_THREADS); uint32_t *blk_of = g.dev(w.blk_of), *bad = g.dev(w.bad); uint64_t *node = (uint64_t *)g.dev(w.node);
  if (D) HIP_CHECK(hipMemsetAsync(bad, 0, 4 * n_lists, s));
  if (n) {
    if (D) hipLaunchKernelGGL(k_trie_leaf<true>, dim3(cdiv(n, TX_THREADS)), block, 0, s, g.dtx, g.doff, (uint32_t)n, g.dfirst, (uint32_t)n_lists, D, blk_of, bad, node);
    else hipLaunchKernelGGL(k_trie_leaf<false>, dim3(cdiv(n, TX_THREADS)), block, 0, s, g.dtx, g.doff, (uint32_t)n, g.dfirst, (uint32_t)n_lists, (const uint32_t *)nullptr, blk_of, (uint32_t *)nullptr, node);
    const int nibbles = largest <= 1 ? 0 : largest <= 0x80 ? 2 : largest <= 0x100 ? 4 : largest <= 0x10000 ? 6 : largest <= 0x1000000 ? 8 : 10;   // of rlp(largest - 1); one value: no branch
    for (int depth = nibbles - 1; depth >= 0; depth--) hipLaunchKernelGGL(k_trie_level, dim3(cdiv(n, TX_THREADS)), block, 0, s, (uint32_t)n, (uint32_t)depth, g.dfirst, (const uint32_t *)blk_of, node);
  }
  hipLaunchKernelGGL(k_trie_finish, dim3(cdiv(n_lists, TX_THREADS)), block, 0, s, (uint32_t)n_lists, g.dfirst, (const uint64_t *)node, D ? (const uint32_t *)bad : (const uint32_t *)nullptr,
                     (uint64_t *)g.dev(w.roots), D ? (uint8_t *)g.dev(w.defined) : (uint8_t *)nullptr);
  HIP_CHECK(hipGetLastError());
}
size_t largest_list(const int *first, size_t n_lists) { size_t m = 0; for (size_t b = 0; b < n_lists; b++) m = std::max(m, (size_t)(first[b + 1] - first[b])); return m; }
}  // namespace

// zkgpu_list_trie_roots (want_tx false: the values verbatim) and zkgpu_tx_roots (want_tx: the walk first; defined is written).  The caller has checked the arguments
// and holds the device mutex; n_lists > 0.  One upload (the bytes, off, first), one download (roots, then defined).  Returns the number of roots that are defined.
size_t trie_roots(const uint8_t *vals, const uint64_t *off, size_t n, const RootsRequest &rq, bool want_tx) {
  const size_t n_lists = rq.n_lists;
  if (n > 0x3FFFFFFFu || n_lists > 0x3FFFFFFFu) throw GpuError("trie roots: more than 2^30 - 1 values or lists");
  LaneScope lane(0); hipStream_t s = gpu().stream; const TrieRootsLayout L = trie_roots_layout(n, (size_t)(off[n] - off[0]), n_lists, want_tx);
  const Staged g(L, vals, off, n, rq.first, s); uint32_t *D = g.dev(L.D);
  if (want_tx && n) hipLaunchKernelGGL(k_tx_walk<false>, dim3(cdiv(n, TX_THREADS)), dim3(TX_THREADS), 0, s, g.dtx, g.doff, (uint32_t)n, (int)SIGNER_FRONTIER, (uint64_t)0, D, (uint8_t *)g.dev(L.rs),
                                       (uint8_t *)g.dev(L.v), (uint8_t *)nullptr, (uint32_t *)nullptr, (uint8_t *)nullptr, (uint32_t *)nullptr);   // (MALFORMED and the 0xC0 position depend on no signer)
  trie_queue(g, n, n_lists, largest_list(rq.first, n_lists), want_tx ? (const uint32_t *)D : (const uint32_t *)nullptr, L.trie, s);
  HIP_CHECK(hipMemcpyAsync(g.back, g.dev(L.down), 4 * (L.down_end - L.down), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  memcpy(rq.roots, g.host(L.trie.roots), 32 * n_lists); size_t good = n_lists;
  if (want_tx) { memcpy(rq.defined, g.host(L.trie.defined), n_lists); good = 0; for (size_t b = 0; b < n_lists; b++) good += rq.defined[b] != 0; }
  return good;
}

// The caller has checked the arguments and holds the device mutex.  want_senders: zkTxSenders (sighash, sigs, deposit_from null), else zkTxSigningInputs.
// One upload (txs, then off), three launches — nine with the recovery — and one download.  Returns the number of records with status OK.
size_t tx_sender_inputs(const TxsIn &in, bool want_senders, const SenderInputsOut &o) {
  const size_t n = in.n;
  if (!n) return 0;
  if (n > 0x3FFFFFFFu) throw GpuError("txs: more than 2^30 - 1 transactions");
  LaneScope lane(0); hipStream_t s = gpu().stream; const SenderInputsLayout L = sender_inputs_layout(n, (size_t)(in.off[n] - in.off[0]));
  const Staged g(L, in.txs, in.off, n, nullptr, s);
  uint32_t *D = g.dev(L.D), *hash = g.dev(L.hash), *rs = g.dev(L.rs), *v = g.dev(L.v), *rec = g.dev(L.rec);
  const dim3 block(TX_THREADS), grid(cdiv(n, TX_THREADS)), grid2(cdiv(2 * n, TX_THREADS));
  hipLaunchKernelGGL(k_tx_walk<false>, grid, block, 0, s, g.dtx, g.doff, (uint32_t)n, in.signer, in.chain_id, D, (uint8_t *)rs, (uint8_t *)v, want_senders ? (uint8_t *)nullptr : (uint8_t *)g.dev(L.sigs),
                     (uint32_t *)nullptr, (uint8_t *)nullptr, (uint32_t *)nullptr);
  hipLaunchKernelGGL(k_tx_hash, grid2, block, 0, s, g.dtx, g.doff, (uint32_t)n, in.chain_id, (const uint32_t *)D, want_senders ? hash : g.dev(L.sighash), g.dev(L.txhash));
  HIP_CHECK(hipGetLastError());
  if (want_senders) recover_senders_queue(hash, rs, (const uint8_t *)v, n, in.signer != SIGNER_FRONTIER, rec, s);
  hipLaunchKernelGGL(k_tx_finish, grid, block, 0, s, (uint32_t)n, (const uint32_t *)D, want_senders ? (const uint8_t *)g.dev(L.ok) : (const uint8_t *)nullptr, (const uint32_t *)g.dev(L.recovered),
                     g.dev(L.froms), (uint8_t *)g.dev(L.status), (uint8_t *)g.dev(L.code), want_senders ? (const uint32_t *)rec : (const uint32_t *)nullptr, g.dev(L.head));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(g.back, g.dev(L.down), 4 * (L.down_end - L.down), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  if (want_senders) senders_keep_head((const uint32_t *)g.host(L.head));
  if (o.txhash) memcpy(o.txhash, g.host(L.txhash), 32 * n);
  if (o.sighash) memcpy(o.sighash, g.host(L.sighash), 32 * n);
  if (o.froms) memcpy(o.froms, g.host(L.froms), 20 * n);
  if (o.sigs) memcpy(o.sigs, g.host(L.sigs), 65 * n);
  memcpy(o.status, g.host(L.status), n); memcpy(o.code, g.host(L.code), n);
  size_t good = 0; for (size_t i = 0; i < n; i++) good += o.status[i] == TX_OK;
  return good;
}
// zkHeaders (include/zk_headers.h).  The caller has checked the arguments and holds the device mutex; n > 0.  One upload (the headers, then off), three launches around
// the recovery's six, one download.  Returns the number of leading headers with status OK.
size_t headers_decide(const HeadersIn &in, const HeadersOut &o) {
  const size_t n = in.n;
  if (n > 0x3FFFFFFFu) throw GpuError("headers: more than 2^30 - 1 headers");
  LaneScope lane(0); hipStream_t s = gpu().stream; const HeadersLayout L = headers_layout(n, (size_t)(in.off[n] - in.off[0]));
  const Staged g(L, in.hdrs, in.off, n, nullptr, s);
  uint32_t *H = g.dev(L.H), *rs = g.dev(L.rs), *v = g.dev(L.v), *rec = g.dev(L.rec), *d_head = g.dev(L.head);
  const HdrOut d{g.dev(L.hash), g.dev(L.sealhash), g.dev(L.signer), g.dev(L.coinbase), g.dev(L.tx_root), g.dev(L.rtcmt), (uint64_t *)g.dev(L.number), (uint64_t *)g.dev(L.time), g.dev(L.extra_beg),
                 g.dev(L.extra_size), g.dev(L.cmt_beg), g.dev(L.cmt_count), (uint8_t *)g.dev(L.difficulty), (uint8_t *)g.dev(L.vote), (uint8_t *)g.dev(L.status)};
  HdrParent parent; parent.have = in.have_parent ? 1u : 0u; parent.number = in.parent_number; parent.time = in.parent_time; memset(parent.hash, 0, sizeof parent.hash);
  if (in.have_parent) memcpy(parent.hash, in.parent_hash, 32);
  const dim3 block(TX_THREADS), grid(cdiv(n, TX_THREADS)), grid2(cdiv(2 * n, TX_THREADS));
  hipLaunchKernelGGL(k_hdr_walk, grid, block, 0, s, g.dtx, g.doff, (uint32_t)n, in.epoch ? in.epoch : (uint64_t)30000, in.now, H, (uint8_t *)rs, (uint8_t *)v, d, d_head + BH_FIRST_BAD);   // clique.go:56, :217-219
  hipLaunchKernelGGL(k_hdr_hash, grid2, block, 0, s, g.dtx, g.doff, (uint32_t)n, (const uint32_t *)H, d.sealhash, d.hash);
  HIP_CHECK(hipGetLastError());
  recover_senders_queue(d.sealhash, rs, (const uint8_t *)v, n, false, rec, s);                      // crypto.Ecrecover: no low-s rule
  hipLaunchKernelGGL(k_hdr_finish, grid, block, 0, s, g.dtx, g.doff, (uint32_t)n, in.period, parent, (const uint32_t *)H, (const uint32_t *)rs, (const uint8_t *)v, (const uint8_t *)g.dev(L.ok),
                     (const uint32_t *)g.dev(L.recovered), d, (const uint32_t *)rec, d_head);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(g.back, g.dev(L.down), 4 * (L.down_end - L.down), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  uint32_t head[BH_WORDS]; memcpy(head, g.host(L.head), sizeof head); const size_t k = head[BH_FIRST_BAD];
  if (k > n) throw GpuError("headers: the count left by the device is out of range");
  senders_keep_head((const uint32_t *)g.host(L.sp_head));
  memcpy(o.hash, g.host(L.hash), 32 * n); memcpy(o.sealhash, g.host(L.sealhash), 32 * n); memcpy(o.signer, g.host(L.signer), 20 * n); memcpy(o.coinbase, g.host(L.coinbase), 20 * n);
  memcpy(o.tx_root, g.host(L.tx_root), 32 * n); memcpy(o.rtcmt, g.host(L.rtcmt), 32 * n); memcpy(o.number, g.host(L.number), 8 * n); memcpy(o.time, g.host(L.time), 8 * n);
  memcpy(o.difficulty, g.host(L.difficulty), n); memcpy(o.vote, g.host(L.vote), n); memcpy(o.extra_beg, g.host(L.extra_beg), 4 * n); memcpy(o.extra_size, g.host(L.extra_size), 4 * n);
  memcpy(o.cmt_beg, g.host(L.cmt_beg), 4 * n); memcpy(o.cmt_count, g.host(L.cmt_count), 4 * n); memcpy(o.status, g.host(L.status), n);
  return k;
}
// zkTxRecords (include/zk_bodies.h).  The caller has checked the arguments and holds the device mutex.  One upload (txs, then off); the walk with both descriptors, the
// hashes, the recovery's six launches once for all lanes, k_body_finish, k_body_scan, k_body_scatter, k_body_gather; four words that say m; one download: the small
// outputs and recs[0 .. m).  rec_froms[m .. n) is zeroed, recs[m .. n) is not written.  first_bad: the first transaction with status != OK, n where there is none.
// borders (may be null): n_borders transaction indices in 0 .. n; rec_borders[k] = the records before transaction borders[k].  Returns m.
// rq (may be null; verifyChainBodiesRoots): the transaction trie roots of the blocks that rq->first names, and defined, as zkTxRoots writes them —
// first rides in the same upload, the trie's launches follow the hashes on the walk's descriptor, the roots come down with the records.  Without it nothing of this
// is queued and the launches are the ones zkTxRecords and verifyChainBodies have always made.
static bool g_gather_bytewise = false;                                                              // (zkgpu_test_bodies_gather: the measurement of DESIGN.md §23; under the device mutex)
void tx_records_gather_bytewise(bool on) { g_gather_bytewise = on; }
namespace {
// the launches and the downloads of tx_records on a workspace whose upload's place is filled, or will be by what is queued on s: n > 0 transactions under L
size_t records_on(const Staged &g, const RecordsLayout &L, const TxsIn &in, const BodyOut &o, size_t *first_bad, const int *borders, size_t n_borders, int *rec_borders, const RootsRequest *rq,
                  hipStream_t s) {
  const size_t n = in.n, n_blocks = rq ? rq->n_lists : 0;
  uint32_t *D = g.dev(L.D), *E = g.dev(L.E), *hash = g.dev(L.hash), *rs = g.dev(L.rs), *xy = g.dev(L.xy), *v = g.dev(L.v), *rec = g.dev(L.rec), *src_of = g.dev(L.src_of), *counts = g.dev(L.counts), *bases = g.dev(L.bases);
  uint32_t *d_head = g.dev(L.head), *d_froms = g.dev(L.froms), *d_rec_froms = g.dev(L.rec_froms), *d_rec_of = g.dev(L.rec_of), *d_prefix = g.dev(L.prefix), *d_recs = g.dev(L.recs);
  const uint32_t *recovered = g.dev(L.recovered);
  const dim3 block(TX_THREADS), grid(cdiv(n, TX_THREADS)), grid2(cdiv(2 * n, TX_THREADS));
  hipLaunchKernelGGL(k_tx_walk<true>, grid, block, 0, s, g.dtx, g.doff, (uint32_t)n, in.signer, in.chain_id, D, (uint8_t *)rs, (uint8_t *)v, (uint8_t *)nullptr, E, (uint8_t *)xy, d_head + BH_FIRST_BAD);
  hipLaunchKernelGGL(k_tx_hash, grid2, block, 0, s, g.dtx, g.doff, (uint32_t)n, in.chain_id, (const uint32_t *)D, hash, g.dev(L.txhash));
  HIP_CHECK(hipGetLastError());
  if (n_blocks) trie_queue(g, n, n_blocks, largest_list(rq->first, n_blocks), (const uint32_t *)D, L.trie, s);
  recover_senders_queue(hash, rs, (const uint8_t *)v, n, in.signer != SIGNER_FRONTIER, rec, s);    // once, for every lane; a deposit's Homestead rule where the flag is 0: k_body_finish
  hipLaunchKernelGGL(k_body_finish, grid, block, 0, s, (uint32_t)n, (int)(in.signer != SIGNER_FRONTIER), (const uint32_t *)D, (const uint32_t *)E, (const uint8_t *)g.dev(L.ok), recovered,
                     (const uint32_t *)rs, (const uint32_t *)xy, d_froms, (uint8_t *)g.dev(L.status), (uint8_t *)g.dev(L.code), (int32_t *)d_rec_of, counts, d_head, (const uint32_t *)rec);
  hipLaunchKernelGGL(k_body_scan, dim3(1), dim3(BODY_SCAN_THREADS), 0, s, (const uint32_t *)counts, (uint32_t)grid.x, bases, d_head);
  hipLaunchKernelGGL(k_body_scatter, grid, block, 0, s, (uint32_t)n, (const uint32_t *)bases, (const uint32_t *)d_froms, (int32_t *)d_rec_of, d_prefix, src_of, d_rec_froms);
  const dim3 gblock(BODY_GATHER_THREADS), ggrid(cdiv(64 * n, BODY_GATHER_THREADS));
  if (g_gather_bytewise) hipLaunchKernelGGL(k_body_gather<false>, ggrid, gblock, 0, s, g.dtx, g.doff, (uint32_t)n, (const uint32_t *)D, (const uint32_t *)E, recovered, (const uint32_t *)src_of, (const uint32_t *)d_prefix, d_recs);
  else hipLaunchKernelGGL(k_body_gather<true>, ggrid, gblock, 0, s, g.dtx, g.doff, (uint32_t)n, (const uint32_t *)D, (const uint32_t *)E, recovered, (const uint32_t *)src_of, (const uint32_t *)d_prefix, d_recs);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(g.back, d_head, 4 * BH_WORDS, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));   // m: the length of the download
  uint32_t head[BH_WORDS]; memcpy(head, g.back, sizeof head); const size_t m = head[BH_M];
  if (m > n || head[BH_FIRST_BAD] > n) throw GpuError("txs: the record count left by the device is out of range");
  HIP_CHECK(hipMemcpyAsync(g.back, g.dev(L.down), 4 * (L.recs - L.down + (size_t)REC_WORDS * m), hipMemcpyDeviceToHost, s));
  uint8_t *const roots_back = g.host(L.down_end);                                                   // (the second range lands behind the whole of the first)
  if (n_blocks) HIP_CHECK(hipMemcpyAsync(roots_back, g.dev(L.trie.roots), 4 * (L.trie.end - L.trie.roots), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (n_blocks) { memcpy(rq->roots, roots_back, 32 * n_blocks); memcpy(rq->defined, roots_back + 4 * (L.trie.defined - L.trie.roots), n_blocks); }
  senders_keep_head((const uint32_t *)g.host(L.sp_head));
  if (o.txhash) memcpy(o.txhash, g.host(L.txhash), 32 * n);
  memcpy(o.froms, g.host(L.froms), 20 * n); memcpy(o.rec_froms, g.host(L.rec_froms), 20 * m); memset(o.rec_froms + 20 * m, 0, 20 * (n - m)); memcpy(o.rec_of, g.host(L.rec_of), 4 * n);
  const uint32_t *prefix = (const uint32_t *)g.host(L.prefix);
  memcpy(o.status, g.host(L.status), n); memcpy(o.code, g.host(L.code), n); if (m) memcpy(o.recs, g.host(L.recs), 4 * (size_t)REC_WORDS * m);
  if (prefix[n] != m) throw GpuError("txs: the prefix values left by the device do not end at the record count");
  for (size_t k = 0; k < n_borders; k++) rec_borders[k] = (int)prefix[borders[k]];
  if (first_bad) *first_bad = head[BH_FIRST_BAD];
  return m;
}
}  // namespace
size_t tx_records(const TxsIn &in, const BodyOut &o, size_t *first_bad, const int *borders, size_t n_borders, int *rec_borders, const RootsRequest *rq) {
  const size_t n = in.n, n_blocks = rq ? rq->n_lists : 0;
  if (!n) { if (first_bad) *first_bad = 0; for (size_t k = 0; k < n_borders; k++) rec_borders[k] = 0; return 0; }
  if (n > 0x3FFFFFFFu) throw GpuError("txs: more than 2^30 - 1 transactions");
  LaneScope lane(0); hipStream_t s = gpu().stream; const RecordsLayout L = records_layout(n, (size_t)(in.off[n] - in.off[0]), n_blocks);
  const Staged g(L, in.txs, in.off, n, rq ? rq->first : nullptr, s);
  return records_on(g, L, in, o, first_bad, borders, n_borders, rec_borders, rq, s);
}
// ---- zkBodySplit and verifyChainRawBodies (include/zk_raw_bodies.h) --------------------------------------------------------------------------------
// The raw bodies cross the bus once, into Txs::raw.  split_count: the upload, k_split_count, k_split_scan, and the one mid-call synchronise that brings the head,
// block_first and body_status down — the layout of everything behind depends on n and on the packed total, which the device alone knows.  split_fill: the two launches
// that fill the upload's place of that layout from Txs::raw, queued in front of the launches that read it.
namespace {
static_assert(TXL_SPLIT_HEAD == SH_WORDS, "txs_layout.hpp carves for k_split_scan");
struct SplitRun { SplitLayout L; uint32_t *r; uint8_t *back; size_t n, total, largest, k; };
SplitRun split_count(const RawBodiesIn &in, const RawBodiesOut &o, bool write_unfit, hipStream_t s) {
  const size_t nb = in.n_blocks;
  if (nb > 0x3FFFFFFFu) throw GpuError("raw bodies: more than 2^30 - 1 bodies");
  Txs &d = txs_state(); SplitRun R; R.L = split_layout(nb, (size_t)(in.body_off[nb] - in.body_off[0]), in.cap); const SplitLayout &L = R.L;
  d.raw_pin.pinned(L.pin_bytes); uint8_t *pin = d.raw_pin.pin; R.back = pin + L.up;
  if (L.total) memcpy(pin, in.bodies + in.body_off[0], L.total);
  memset(pin + L.total, 0, L.total8 - L.total); memcpy(pin + L.total8, in.body_off, 8 * (nb + 1));
  Txs::grow(d.raw, L.end + TXL_SLACK); uint32_t *r = R.r = d.raw.get(); if (!r) throw GpuError("raw bodies: no workspace");
  HIP_CHECK(hipMemcpyAsync(r, pin, L.up, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_split_count, dim3(cdiv(nb, TX_THREADS)), dim3(TX_THREADS), 0, s, (const uint8_t *)r, (const uint64_t *)(r + L.body_off), (uint32_t)nb, (uint8_t *)(r + L.status), r + L.count,
                     r + L.pay_beg, r + L.pay_size);
  hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(SPLIT_SCAN_THREADS), 0, s, (const uint8_t *)(r + L.status), (const uint32_t *)(r + L.count), (const uint32_t *)(r + L.pay_size), (uint32_t)nb,
                     r + L.first, (uint64_t *)(r + L.base), r + L.head);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(R.back, r + L.down, 4 * (L.tx_beg - L.down), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  uint32_t head[SH_WORDS]; memcpy(head, R.back, sizeof head);
  const uint64_t n = (uint64_t)head[SH_N] | ((uint64_t)head[SH_N + 1] << 32), total = (uint64_t)head[SH_TOTAL] | ((uint64_t)head[SH_TOTAL + 1] << 32);
  if (n > 0x3FFFFFFFu) throw GpuError("raw bodies: more than 2^30 - 1 transactions");
  if (total > L.total || n > total || head[SH_LARGEST] > n || head[SH_K] > nb) throw GpuError("raw bodies: the counts left by the device are out of range");
  R.n = (size_t)n; R.total = (size_t)total; R.largest = head[SH_LARGEST]; R.k = head[SH_K];
  uint32_t last; memcpy(&last, R.back + 4 * (L.first + nb - L.down), 4);
  if (last != R.n) throw GpuError("raw bodies: block_first does not end at the count left by the device");
  if (R.n <= in.cap || write_unfit) { memcpy(o.block_first, R.back + 4 * (L.first - L.down), 4 * (nb + 1)); memcpy(o.body_status, R.back + 4 * (L.status - L.down), nb); }
  return R;
}
// n <= tx_cap.  The downloads of tx_beg and tx_size are queued behind the launch that writes them; split_take copies them out once the stream has been synchronised.
void split_fill(const SplitRun &R, const Staged &g, size_t nb, bool with_first, bool pack, hipStream_t s) {
  const SplitLayout &L = R.L; uint32_t *r = R.r;
  hipLaunchKernelGGL(k_split_offsets, dim3(cdiv(nb, TX_THREADS)), dim3(TX_THREADS), 0, s, (const uint8_t *)r, (const uint64_t *)(r + L.body_off), (uint32_t)nb, (const uint8_t *)(r + L.status),
                     (const uint32_t *)(r + L.pay_beg), (const uint32_t *)(r + L.pay_size), (const uint32_t *)(r + L.first), (const uint64_t *)(r + L.base), (uint32_t)R.n, (uint64_t *)g.doff,
                     with_first ? (uint32_t *)g.dfirst : (uint32_t *)nullptr, (uint64_t *)(r + L.tx_beg), r + L.tx_size);
  const size_t words = (R.total + 7) / 8;
  if (pack && words) hipLaunchKernelGGL(k_split_pack, dim3(cdiv(words, TX_THREADS)), dim3(TX_THREADS), 0, s, (const uint64_t *)r, (const uint64_t *)(r + L.body_off), (uint32_t)nb,
                                        (const uint32_t *)(r + L.pay_beg), (const uint64_t *)(r + L.base), (uint64_t)R.total, (uint64_t)words, (uint64_t *)g.p);
  HIP_CHECK(hipGetLastError());
  if (R.n) { HIP_CHECK(hipMemcpyAsync(R.back + 4 * (L.tx_beg - L.down), r + L.tx_beg, 8 * R.n, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(R.back + 4 * (L.tx_size - L.down), r + L.tx_size, 4 * R.n, hipMemcpyDeviceToHost, s)); }
}
void split_take(const SplitRun &R, const RawBodiesOut &o) {
  if (!R.n) return;
  const SplitLayout &L = R.L; memcpy(o.tx_beg, R.back + 4 * (L.tx_beg - L.down), 8 * R.n); memcpy(o.tx_size, R.back + 4 * (L.tx_size - L.down), 4 * R.n);
}
}  // namespace
// The callers have checked the arguments and hold the device mutex; n_blocks > 0.
RawSplit body_split(const RawBodiesIn &in, const RawBodiesOut &o, uint8_t *packed, uint64_t *packed_off) {
  LaneScope lane(0); hipStream_t s = gpu().stream; SyncAtExit sync;
  const SplitRun R = split_count(in, o, true, s); const RawSplit out = {R.n, R.k, R.total, R.n <= in.cap};
  if (!out.fits) return out;
  const PackedLayout P = packed_layout(R.n, R.total, in.n_blocks); const Staged g(P);
  split_fill(R, g, in.n_blocks, true, packed != nullptr, s);
  if (packed) HIP_CHECK(hipMemcpyAsync(g.back, g.p, P.up, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s)); split_take(R, o);
  if (packed) { if (R.total) memcpy(packed, g.back, R.total); memcpy(packed_off, g.back + 4 * P.off, 8 * (R.n + 1)); }
  return out;
}
RawSplit raw_records(const RawBodiesIn &in, const RawBodiesOut &o, int signer, uint64_t chain_id, const BodyOut &bo, size_t *first_bad, int *rec_borders, uint8_t *roots, uint8_t *defined, size_t *m) {
  LaneScope lane(0); hipStream_t s = gpu().stream; SyncAtExit sync; const size_t nb = in.n_blocks;
  const SplitRun R = split_count(in, o, false, s); const RawSplit out = {R.n, R.k, R.total, R.n <= in.cap};
  if (!out.fits) return out;
  const RootsRequest rq = {o.block_first, nb, roots, defined};
  if (!R.n) {                                                                                        // every body empty or refused: the roots of no transactions, as verifyChainBodiesRoots has them
    const uint64_t off0[1] = {0}; trie_roots(nullptr, off0, 0, rq, true);
    *first_bad = 0; *m = 0; for (size_t b = 0; b <= nb; b++) rec_borders[b] = 0;
    return out; }
  const RecordsLayout L = records_layout(R.n, R.total, nb); const Staged g(L);
  split_fill(R, g, nb, true, true, s);
  const TxsIn tin = {nullptr, nullptr, R.n, signer, chain_id};                                      // (the bytes and off are the device's)
  *m = records_on(g, L, tin, bo, first_bad, o.block_first, nb + 1, rec_borders, &rq, s);             // (synchronises: tx_beg and tx_size have landed)
  split_take(R, o);
  return out;
}

// Keccak-256 of n byte strings, msgs[off[i] .. off[i+1]), through k_tx_hash's sponge
void probe_keccak256(const uint8_t *msgs, const uint64_t *off, size_t n, uint8_t *out) {
  if (!n) return;
  if (!off || !out) throw GpuError("probe_keccak256: a null pointer");
  for (size_t i = 0; i < n; i++) if (off[i + 1] < off[i]) throw GpuError("probe_keccak256: offsets decrease");
  if (off[n] > off[0] && !msgs) throw GpuError("probe_keccak256: a null pointer");
  if (n > 0x3FFFFFFFu) throw GpuError("probe_keccak256: more than 2^30 - 1 strings");
  LaneScope lane(0); hipStream_t s = gpu().stream; const KeccakLayout L = keccak_layout(n, (size_t)(off[n] - off[0]));
  const Staged g(L, msgs, off, n, nullptr, s);
  hipLaunchKernelGGL(k_tx_keccak, dim3(cdiv(n, TX_THREADS)), dim3(TX_THREADS), 0, s, g.dtx, g.doff, (uint32_t)n, g.dev(L.out));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(g.back, g.dev(L.down), 4 * (L.down_end - L.down), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  memcpy(out, g.host(L.out), 32 * n);
}

}  // namespace zk
