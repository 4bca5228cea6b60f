// The workspace layouts of the transaction calls (gpu_txs.hip, gpu_senders.hip), each stated once.  A call has one device workspace and one pinned
// buffer; a layout names every region of the workspace by its offset in 32-bit words, the upload at its start, and the range that comes down again.  Region x lies at
// p + L.x on the device and, once the download has landed at `back`, at back + 4 * (L.x - L.down) on the host: nothing else positions a region.
// Host only, plain C++17, no HIP: tests/txs_layout_driver.cpp compiles it alone and holds every number here to the formulas the calls were first written with.
#pragma once
#include <cstddef>

namespace zk {
// what the kernels fix (gpu_txs.hip and gpu_senders.hip assert that these are their own constants): the words of a lane's two descriptors, of the records' head, of a
// record, of the recovery's head; the lanes of a workgroup; the words every workspace keeps free behind its last region
constexpr size_t TXL_D_WORDS = 9, TXL_E_WORDS = 10, TXL_HEAD_WORDS = 4, TXL_REC_WORDS = 180, TXL_SP_HEAD = 4, TXL_THREADS = 128, TXL_SLACK = 2;

// a cursor in words: take() rounds it up to a multiple of align_words, returns that offset and moves `count` words on
struct Carve {
  size_t at = 0;
  size_t take(size_t count, size_t align_words = 1) { at = (at + align_words - 1) / align_words * align_words; const size_t o = at; at += count; return o; }
  static size_t bytes(size_t n) { return (n + 3) / 4; }   // the words that hold n bytes
};

// the recovery's output (gpu_senders.hip): the head, four counters | ok, n bytes | froms 5n | pubs 16n where they are wanted
struct SendersOut { size_t head, ok, froms, pubs, end; };
inline SendersOut senders_out(Carve &c, size_t n, bool want_pubs) {
  SendersOut o; o.head = c.take(TXL_SP_HEAD); o.ok = c.take(Carve::bytes(n)); o.froms = c.take(5 * n); o.pubs = c.take(want_pubs ? 16 * n : 0); o.end = c.at; return o;
}
inline SendersOut senders_out(size_t n, bool want_pubs) { Carve c; return senders_out(c, n, want_pubs); }   // from the output's own start
// the trie's own arrays: blk_of n | bad n_lists | node 8n | roots 8 n_lists | defined, n_lists bytes.  roots .. end is what comes down: 32 bytes a root, then defined
// padded to 8 bytes.
struct TrieWords { size_t blk_of, bad, node, roots, defined, end; };
inline TrieWords trie_words(Carve &c, size_t n, size_t n_lists) {
  TrieWords w; w.blk_of = c.take(n, 2);                  // (even, as it has always stood: node's place depends on it)
  w.bad = c.take(n_lists);
  w.node = c.take(8 * n, 2);                             // k_trie_leaf, k_trie_level, k_trie_finish: uint64_t
  w.roots = c.take(8 * n_lists, 2);                      // k_trie_finish: uint64_t
  w.defined = c.take(Carve::bytes(n_lists)); w.end = c.take(0, 2); return w;
}

// What every call has.  The upload, at the start of the workspace and of the pinned buffer: the caller's bytes off[0] .. off[n), padded to 8 | off, n + 1 64-bit values |
// first, n_first 32-bit values, padded to 8 (the calls with a trie).  The download lands in the pinned buffer behind the upload.
struct TxsUpload {
  size_t total, total8, up;                              // bytes: the caller's, those padded to 8, the whole upload
  size_t off, first, n_first;                            // words
  size_t down, down_end;                                 // the download: regions down .. down_end
  size_t end, pin_bytes;                                 // the workspace without its slack; the pinned buffer
};
// fills the upload's part of a layout; the cursor it returns stands behind the upload, and the layout's function carves on from there
inline Carve carve_upload(TxsUpload &u, size_t n, size_t total_bytes, size_t n_first) {
  Carve c; u.total = total_bytes; u.n_first = n_first;
  c.take(Carve::bytes(u.total));                         // (k_body_gather<true> reads these as aligned words, the padding included)
  u.off = c.take(2 * (n + 1), 2);                        // every kernel that has off: uint64_t
  u.first = c.take(n_first, 2); u.up = 4 * c.take(0, 2); u.total8 = 4 * u.off; return c;
}

// zkTxSigningInputs and zkTxSenders.  Device, in words: up | D | hash 8n | rs 16n | v | the recovery's out | down.
// Down, in words: txhash 8n | sighash 8n | froms 5n | then bytes: sigs 65n | status n | code n | the recovery's head, 4 words.
struct SenderInputsLayout : TxsUpload {
  size_t D, hash, rs, v, rec, ok, recovered, txhash, sighash, froms, sigs, status, code, head;
};
inline SenderInputsLayout sender_inputs_layout(size_t n, size_t total_bytes) {
  SenderInputsLayout L; Carve c = carve_upload(L, n, total_bytes, 0);
  L.D = c.take(TXL_D_WORDS * n); L.hash = c.take(8 * n); L.rs = c.take(16 * n); L.v = c.take(Carve::bytes(n));
  const SendersOut so = senders_out(c, n, false); L.rec = so.head; L.ok = so.ok; L.recovered = so.froms;
  L.down = L.txhash = c.take(8 * n); L.sighash = c.take(8 * n); L.froms = c.take(5 * n); L.sigs = c.take(Carve::bytes(65 * n)); L.status = c.take(Carve::bytes(n)); L.code = c.take(Carve::bytes(n));
  L.head = c.take(TXL_SP_HEAD); L.down_end = L.end = c.at; L.pin_bytes = L.up + 4 * (L.down_end - L.down);
  return L;
}

// zkTxRecords.  Device, in words: up | D | E | hash 8n | rs 16n | xy 16n | v | the recovery's out | src_of n | counts nb | bases nb | down | the trie's arrays.
// Down, in words: head 4 (first_bad, m, -, -) | sp_head, the recovery's four | txhash 8n | froms 5n | rec_froms 5n | rec_of n | prefix n + 1 | status | code | recs 180 n,
// of which the first m records come down.  n_blocks: the blocks whose roots are asked for (verifyChainBodiesRoots) — block_first rides in the upload, the trie's arrays
// stand behind the download and roots .. end comes down behind it in the pinned buffer; 0: none of this.
struct RecordsLayout : TxsUpload {
  size_t D, E, hash, rs, xy, v, rec, ok, recovered, src_of, counts, bases, head, sp_head, txhash, froms, rec_froms, rec_of, prefix, status, code, recs; TrieWords trie;
};
inline RecordsLayout records_layout(size_t n, size_t total_bytes, size_t n_blocks) {
  RecordsLayout L; Carve c = carve_upload(L, n, total_bytes, n_blocks ? n_blocks + 1 : 0);
  const size_t nb = (n + TXL_THREADS - 1) / TXL_THREADS;
  L.D = c.take(TXL_D_WORDS * n); L.E = c.take(TXL_E_WORDS * n); L.hash = c.take(8 * n); L.rs = c.take(16 * n); L.xy = c.take(16 * n); L.v = c.take(Carve::bytes(n));
  const SendersOut so = senders_out(c, n, false); L.rec = so.head; L.ok = so.ok; L.recovered = so.froms;
  L.src_of = c.take(n); L.counts = c.take(nb); L.bases = c.take(nb);
  L.down = L.head = c.take(TXL_HEAD_WORDS, 2);           // (recs is placed from here: the download starts at an 8-byte boundary)
  L.sp_head = c.take(TXL_SP_HEAD);                       // k_body_finish: head[4 .. 8)
  L.txhash = c.take(8 * n); L.froms = c.take(5 * n); L.rec_froms = c.take(5 * n); L.rec_of = c.take(n); L.prefix = c.take(n + 1); L.status = c.take(Carve::bytes(n)); L.code = c.take(Carve::bytes(n));
  L.recs = c.take(TXL_REC_WORDS * n, 2);                 // 8-byte aligned on both sides of the bus
  L.down_end = c.at; L.trie = trie_words(c, n_blocks ? n : 0, n_blocks); L.end = c.at; L.pin_bytes = L.up + 4 * (L.down_end - L.down) + 4 * (L.trie.end - L.trie.roots);
  return L;
}

// zkgpu_list_trie_roots (want_tx false) and zkTxRoots.  Device, in words: up | (the walk: D | rs 16n | v) | the trie's arrays.  Down: roots, and with want_tx defined.
struct TrieRootsLayout : TxsUpload {
  size_t D, rs, v; TrieWords trie;
};
inline TrieRootsLayout trie_roots_layout(size_t n, size_t total_bytes, size_t n_lists, bool want_tx) {
  TrieRootsLayout L; Carve c = carve_upload(L, n, total_bytes, n_lists + 1);
  L.D = c.take(want_tx ? TXL_D_WORDS * n : 0); L.rs = c.take(want_tx ? 16 * n : 0); L.v = c.take(want_tx ? Carve::bytes(n) : 0);
  L.trie = trie_words(c, n, n_lists); L.down = L.trie.roots; L.down_end = want_tx ? L.trie.end : L.trie.defined; L.end = c.at; L.pin_bytes = L.up + 4 * (L.trie.end - L.trie.roots);
  return L;
}

// zkHeaders (include/zk_headers.h).  Device, in words: up | H, the walk's descriptor | rs 16n | v | the recovery's out | down.
// Down, in words: head 4 (first_bad, -, -, -) | sp_head, the recovery's four | number 2n | time 2n | hash 8n | sealhash 8n (the recovery reads it where it lies) |
// signer 5n | coinbase 5n | tx_root 8n | rtcmt 8n | extra_beg n | extra_size n | cmt_beg n | cmt_count n | then bytes: difficulty n | vote n | status n.
constexpr size_t TXL_H_WORDS = 7;
struct HeadersLayout : TxsUpload {
  size_t H, rs, v, rec, ok, recovered, head, sp_head, number, time, hash, sealhash, signer, coinbase, tx_root, rtcmt, extra_beg, extra_size, cmt_beg, cmt_count, difficulty, vote, status;
};
inline HeadersLayout headers_layout(size_t n, size_t total_bytes) {
  HeadersLayout L; Carve c = carve_upload(L, n, total_bytes, 0);
  L.H = c.take(TXL_H_WORDS * n); L.rs = c.take(16 * n); L.v = c.take(Carve::bytes(n));
  const SendersOut so = senders_out(c, n, false); L.rec = so.head; L.ok = so.ok; L.recovered = so.froms;
  L.down = L.head = c.take(TXL_HEAD_WORDS, 2);           // (number and time are placed from here: 64-bit values on both sides of the bus)
  L.sp_head = c.take(TXL_SP_HEAD);                       // k_hdr_finish: head[4 .. 8)
  L.number = c.take(2 * n, 2); L.time = c.take(2 * n, 2); L.hash = c.take(8 * n); L.sealhash = c.take(8 * n); L.signer = c.take(5 * n); L.coinbase = c.take(5 * n); L.tx_root = c.take(8 * n);
  L.rtcmt = c.take(8 * n); L.extra_beg = c.take(n); L.extra_size = c.take(n); L.cmt_beg = c.take(n); L.cmt_count = c.take(n);
  L.difficulty = c.take(Carve::bytes(n)); L.vote = c.take(Carve::bytes(n)); L.status = c.take(Carve::bytes(n));
  L.down_end = L.end = c.at; L.pin_bytes = L.up + 4 * (L.down_end - L.down);
  return L;
}

// zkgpu_test_keccak256.  Device, in words: up | out 8n, which comes down.
struct KeccakLayout : TxsUpload { size_t out; };
inline KeccakLayout keccak_layout(size_t n, size_t total_bytes) {
  KeccakLayout L; Carve c = carve_upload(L, n, total_bytes, 0);
  L.down = L.out = c.take(8 * n); L.down_end = L.end = c.at; L.pin_bytes = L.up + 4 * (L.down_end - L.down); return L;
}

// zkBodySplit and verifyChainRawBodies (include/zk_raw_bodies.h).  The raw bodies have a buffer and a pinned buffer of their own, kept beside the
// workspace: the bodies' bytes go up here, and what the split packs from them fills the upload's place of a layout above, as if the caller had supplied it.
// Device, in words: up (the bytes body_off[0] .. body_off[n_blocks), padded to 8 | body_off, n_blocks + 1 64-bit values) | pay_beg n_blocks | pay_size n_blocks |
// count n_blocks | base, n_blocks + 1 64-bit values | down.
// Down, in words: head 8 (n, 64 bits | the packed total, 64 bits | the largest block | the first body that is not OK | -, -) | first n_blocks + 1 | status, n_blocks
// bytes | tx_beg, tx_cap 64-bit values | tx_size tx_cap.  head .. tx_beg comes down at the mid-call synchronise, the first n entries of tx_beg and of tx_size behind the
// launches that wrote them.  tx_cap: the caller's cap, or the number of bytes where that is less — an element has at least one byte.
constexpr size_t TXL_SPLIT_HEAD = 8;
struct SplitLayout {
  size_t total, total8, up;                              // bytes: the caller's, those padded to 8, the whole upload
  size_t body_off, pay_beg, pay_size, count, base, head, first, status, tx_beg, tx_size, tx_cap;   // words (tx_cap: entries)
  size_t down, end, pin_bytes;
};
inline SplitLayout split_layout(size_t n_blocks, size_t total_bytes, size_t cap) {
  SplitLayout L; Carve c; L.total = total_bytes; L.tx_cap = cap < total_bytes ? cap : total_bytes;
  c.take(Carve::bytes(L.total));                         // (k_split_pack reads these as aligned 64-bit words, the padding included)
  L.body_off = c.take(2 * (n_blocks + 1), 2); L.up = 4 * c.at; L.total8 = 4 * L.body_off;
  L.pay_beg = c.take(n_blocks); L.pay_size = c.take(n_blocks); L.count = c.take(n_blocks); L.base = c.take(2 * (n_blocks + 1), 2);
  L.down = L.head = c.take(TXL_SPLIT_HEAD, 2); L.first = c.take(n_blocks + 1); L.status = c.take(Carve::bytes(n_blocks));
  L.tx_beg = c.take(2 * L.tx_cap, 2); L.tx_size = c.take(L.tx_cap); L.end = c.take(0, 2); L.pin_bytes = L.up + 4 * (L.end - L.down);
  return L;
}
// what zkBodySplit alone packs into: the upload's place and nothing behind it; the test entry brings it down again whole
struct PackedLayout : TxsUpload {};
inline PackedLayout packed_layout(size_t n, size_t total_bytes, size_t n_blocks) {
  PackedLayout L; Carve c = carve_upload(L, n, total_bytes, n_blocks + 1);
  L.down = 0; L.down_end = L.end = c.at; L.pin_bytes = 2 * L.up; return L;
}

}  // namespace zk
