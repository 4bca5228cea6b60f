// Sender inputs from raw transactions (include/zk_txs.h): what the reference does per transaction between a block body's bytes and recoverPlain —
// rlp.DecodeBytes into txdata (rlp/decode.go; core/types/transaction.go:64-100), signer.Hash (core/types/transaction_signing.go:179-189, :231-240), the chain-id
// arithmetic on V (:151-161, :274-284), tx.Hash(), and Sender's rule for a deposit (:72-76) — for n transactions in one call, one lane a transaction.
//   k_tx_walk     the 26 headers of txdata and every rule of the strict decoder; status, code, the byte range of fields 1 .. 6, a 0xC0 recipient's position, the class
//                 of V and ZKAdrress into a descriptor; R || S and V's byte straight into the layout the recovery reads
//   k_tx_hash     2n jobs, lanes 0 .. n-1 the signing hash, n .. 2n-1 the transaction hash: Keccak-256 over a segmented byte source (a prefix in registers, one range
//                 of the input with at most one byte substituted, a suffix in registers)
//   (the recovery's six launches, gpu_senders.hip, on what the two left on the device: zkTxSenders only)
//   k_tx_finish   the walk's status merged with the recovery's ok; a deposit's sender is its ZKAdrress; refused lanes zero
// Rules every kernel keeps: no lane waits for another lane; every loop is bounded by a constant or by the transaction's own length; every
// offset taken from the input is checked against the end of its list — and so against the transaction's end — before the byte there is read; the Keccak state is
// indexed by compile-time constants only; no kernel uses scratch.
#include <algorithm>
#include <cstring>
#include <string>
#include "gpu_internal.hpp"
#include "secp256k1.cuh"

namespace zk {
size_t recover_senders_out_words(size_t n);
void recover_senders_queue(const uint32_t *hash, const uint32_t *rs, const uint8_t *v, size_t n, bool homestead, uint32_t *out, hipStream_t s);
void senders_keep_head(const uint32_t *head);

constexpr int TX_THREADS = 128;
enum { TX_OK = 0, TX_MALFORMED = 1, TX_CHAIN_ID = 2, TX_SIG = 3 };
enum { SIGNER_FRONTIER = 0, SIGNER_HOMESTEAD = 1, SIGNER_EIP155 = 2 };
constexpr uint32_t TX_DEPOSIT = 3;                    // transaction.go:43
// the descriptor of a lane, in words; word k of lane i lies at D[k * n + i]
constexpr int TD_META = 0 /* status | code << 8 | nine-field hash << 16 */, TD_A = 1, TD_B = 2, TD_C0 = 3 /* 0xFFFFFFFF: none */, TD_ZK = 4, TD_WORDS = 9;
// txdata's 26 fields (transaction.go:64-96), three bits a field
enum { FK_U8, FK_U64, FK_BIG, FK_ADDR_NIL, FK_BYTES, FK_HASH, FK_ADDR, FK_U64S };
constexpr int TX_FIELDS = 26, F_RECIPIENT = 4, F_PAYLOAD = 6, F_ZKADDR = 11, F_V = 23, F_R = 24, F_S = 25;
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
__global__ void __launch_bounds__(TX_THREADS) k_tx_walk(const uint8_t *__restrict__ txs, const uint64_t *__restrict__ off, uint32_t n, int signer, uint64_t chain_id, uint32_t *__restrict__ D,
                                                         uint8_t *__restrict__ rs, uint8_t *__restrict__ vout, uint8_t *__restrict__ sigs65) {
  const uint32_t i = blockIdx.x * TX_THREADS + threadIdx.x; if (i >= n) return;
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
  }
  const size_t nn = n;
  D[TD_META * nn + i] = status | (bad ? 0u : code << 8) | (nine << 16); D[TD_A * nn + i] = a; D[TD_B * nn + i] = b; D[TD_C0 * nn + i] = c0;
#pragma unroll
  for (uint32_t k = 0; k < 5; k++) { uint32_t w = 0;
    if (!bad) { w = (uint32_t)t[zk + 4 * k] | ((uint32_t)t[zk + 4 * k + 1] << 8) | ((uint32_t)t[zk + 4 * k + 2] << 16) | ((uint32_t)t[zk + 4 * k + 3] << 24); }
    D[(TD_ZK + k) * nn + i] = w; }
  tx_put32(rs + 64 * (size_t)i, t, rbeg, rsize, put_r); tx_put32(rs + 64 * (size_t)i + 32, t, sbeg, ssize, put_s); vout[i] = put_v ? (uint8_t)vbyte : (uint8_t)0;
  if (sigs65) { uint8_t *q = sigs65 + 65 * (size_t)i; tx_put32(q, t, rbeg, rsize, put_r); tx_put32(q + 32, t, sbeg, ssize, put_s); q[64] = put_v ? (uint8_t)vbyte : (uint8_t)0; }
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
__device__ __forceinline__ void sponge256(const ByteSource &m, uint32_t pad, uint32_t (&out)[8]) {
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

// ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------------
namespace {
struct Txs : PinnedStage {                           // one a process, every member under the device mutex
  DevBuf<uint32_t> io;
  void grow(size_t words) { if (io.size() >= words) return; const size_t want = std::max(words, 2 * io.size()); io = DevBuf<uint32_t>(); io = DevBuf<uint32_t>(want); }   // (a failed growth leaves no workspace)
};
Txs &txs_state() { static Txs *t = new Txs; return *t; }   // (never destroyed: the runtime may be gone when statics are)
size_t up8(size_t v) { return (v + 7) / 8 * 8; }
// pinned: the bytes off[0] .. off[n) of the caller's buffer, padded to 8, then off itself; returns the bytes staged
size_t stage(Txs &d, const uint8_t *bytes, const uint64_t *off, size_t n, size_t down_bytes, uint8_t **back) {
  const size_t total = (size_t)(off[n] - off[0]), up = up8(total) + 8 * (n + 1);
  d.pinned(up + down_bytes); if (total) memcpy(d.pin, bytes + off[0], total); memset(d.pin + total, 0, up8(total) - total); memcpy(d.pin + up8(total), off, 8 * (n + 1));
  *back = d.pin + up; return up;
}
}  // namespace

// The caller has checked the arguments and holds the device mutex.  want_senders: zkTxSenders (sighash, sigs, deposit_from null), else zkTxSigningInputs.
// One upload (txs, then off), three launches — nine with the recovery — and one download.  Returns the number of records with status OK.
size_t tx_sender_inputs(const uint8_t *txs, const uint64_t *off, size_t n, int signer, uint64_t chain_id, bool want_senders, uint8_t *txhash, uint8_t *sighash, uint8_t *sigs,
                        uint8_t *froms /* deposit_from or froms; may be null for deposit_from */, uint8_t *code, uint8_t *status) {
  if (!n) return 0;
  if (n > 0x3FFFFFFFu) throw GpuError("txs: more than 2^30 - 1 transactions");
  LaneScope lane(0); hipStream_t s = gpu().stream; Txs &d = txs_state();
  // down, in words: txhash 8n | sighash 8n | froms 5n | then bytes: sigs 65n | status n | code n | the recovery's head, 4 words
  const size_t okw = (n + 3) / 4, down_words = 21 * n + (65 * n + 3) / 4 + 2 * okw + 4, down = 4 * down_words; uint8_t *back = nullptr;
  const size_t up = stage(d, txs, off, n, down, &back), total8 = up - 8 * (n + 1);
  // device, in words: up | D | hash 8n | rs 16n | v | the recovery's out | down
  const size_t w_up = up / 4, w_D = TD_WORDS * n, w_rec = recover_senders_out_words(n), words = w_up + w_D + 24 * n + okw + w_rec + down_words + 2;
  d.grow(words); uint32_t *p = d.io.get(); if (!p) throw GpuError("txs: no workspace");
  const uint8_t *dtx = (const uint8_t *)p; const uint64_t *doff = (const uint64_t *)((const uint8_t *)p + total8);
  uint32_t *D = p + w_up, *hash = D + w_D, *rs = hash + 8 * n, *v = rs + 16 * n, *rec = v + okw, *dn = rec + w_rec;
  uint32_t *d_txhash = dn, *d_sighash = dn + 8 * n, *d_froms = dn + 16 * n; uint8_t *d_sigs = (uint8_t *)(dn + 21 * n), *d_status = d_sigs + 4 * ((65 * n + 3) / 4), *d_code = d_status + 4 * okw; uint32_t *d_head = dn + down_words - 4;
  SyncAtExit sync;
  HIP_CHECK(hipMemcpyAsync(p, d.pin, up, hipMemcpyHostToDevice, s));
  const dim3 block(TX_THREADS), grid(cdiv(n, TX_THREADS)), grid2(cdiv(2 * n, TX_THREADS));
  hipLaunchKernelGGL(k_tx_walk, grid, block, 0, s, dtx, doff, (uint32_t)n, signer, chain_id, D, (uint8_t *)rs, (uint8_t *)v, want_senders ? (uint8_t *)nullptr : d_sigs);
  hipLaunchKernelGGL(k_tx_hash, grid2, block, 0, s, dtx, doff, (uint32_t)n, chain_id, (const uint32_t *)D, want_senders ? hash : d_sighash, d_txhash);
  HIP_CHECK(hipGetLastError());
  if (want_senders) recover_senders_queue(hash, rs, (const uint8_t *)v, n, signer != SIGNER_FRONTIER, rec, s);
  hipLaunchKernelGGL(k_tx_finish, grid, block, 0, s, (uint32_t)n, (const uint32_t *)D, want_senders ? (const uint8_t *)(rec + 4) : (const uint8_t *)nullptr,
                     (const uint32_t *)(rec + 4 + okw), d_froms, d_status, d_code, want_senders ? (const uint32_t *)rec : (const uint32_t *)nullptr, d_head);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(back, dn, down, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  if (want_senders) senders_keep_head((const uint32_t *)(back + down - 16));
  if (txhash) memcpy(txhash, back, 32 * n);
  if (sighash) memcpy(sighash, back + 32 * n, 32 * n);
  if (froms) memcpy(froms, back + 64 * n, 20 * n);
  if (sigs) memcpy(sigs, back + 84 * n, 65 * n);
  const uint8_t *bst = back + 84 * n + 4 * ((65 * n + 3) / 4); memcpy(status, bst, n); memcpy(code, bst + 4 * okw, n);
  size_t good = 0; for (size_t i = 0; i < n; i++) good += status[i] == TX_OK;
  return good;
}
// Keccak-256 of n byte strings, msgs[off[i] .. off[i+1]), through k_tx_hash's sponge
void probe_keccak256(const uint8_t *msgs, const uint64_t *off, size_t n, uint8_t *out) {
  if (!n) return;
  if (!off || !out) throw GpuError("probe_keccak256: a null pointer");
  for (size_t i = 0; i < n; i++) if (off[i + 1] < off[i]) throw GpuError("probe_keccak256: offsets decrease");
  if (off[n] > off[0] && !msgs) throw GpuError("probe_keccak256: a null pointer");
  if (n > 0x3FFFFFFFu) throw GpuError("probe_keccak256: more than 2^30 - 1 strings");
  LaneScope lane(0); hipStream_t s = gpu().stream; Txs &d = txs_state(); uint8_t *back = nullptr;
  const size_t up = stage(d, msgs, off, n, 32 * n, &back), total8 = up - 8 * (n + 1), words = up / 4 + 8 * n + 2;
  d.grow(words); uint32_t *p = d.io.get(); if (!p) throw GpuError("txs: no workspace");
  SyncAtExit sync;
  HIP_CHECK(hipMemcpyAsync(p, d.pin, up, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_tx_keccak, dim3(cdiv(n, TX_THREADS)), dim3(TX_THREADS), 0, s, (const uint8_t *)p, (const uint64_t *)((const uint8_t *)p + total8), (uint32_t)n, p + up / 4);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(back, p + up / 4, 32 * n, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s));
  memcpy(out, back, 32 * n);
}

}  // namespace zk
